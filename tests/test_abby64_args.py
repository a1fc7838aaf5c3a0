"""The fused d = 64 AbbyNormal entry points (csrc/abby.hip: asrx_abby64_fwd, asrx_abby64_bwd) reject bad calls
before any launch: return code 2 and a fixed asrx_last_error() text, checked for every argument check and for which
check answers when several fail; rows == 0 returns 0 whatever else is passed.

Validation is host code, so this runs without a GPU -- and only without one: the pointers are made-up integers
with the alignment a case needs, nothing reads them here, but a case that wrongly passed validation on a machine
with a device would launch a kernel on them.
"""
import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up pointers: host validation only, no device")


def _addr(i):
    return 0x7F0000000000 + i * 0x10000000  # distinct, 16-byte aligned


ORDER = {
    "asrx_abby64_fwd": "x W1 ldw b1 W2 b2 out out_bf16 ys idx hpre rows L H sid_base key use_noise stream",
    "asrx_abby64_bwd": "dout x hpre W1t ldw W2 ys idx dx dh dW2 db2 rows acc stream",
}
POINTERS = ["x", "W1", "b1", "W2", "b2", "out", "ys", "idx", "hpre", "dout", "W1t", "dx", "dh", "dW2", "db2"]
GOOD = dict({n: _addr(i + 1) for i, n in enumerate(POINTERS)}, ldw=64, out_bf16=0, rows=100, L=10, H=2, sid_base=0,
            key=7, use_noise=1, acc=0, stream=None)

F, B = "asrx_abby64_fwd", "asrx_abby64_bwd"
F_REQ = "x, W1, W2, b2, out, ys and idx required"
F_ALIGN = "x/W1/hpre 16-byte, out 16-byte (8 bf16) aligned"
B_REQ = "every operand is required"
B_ALIGN = "dout/x/hpre/W1t/W2/dx/dh must be 16-byte aligned"
LDW = "ldw >= 64, ldw%8 required"

CASES = [(F, "rows < 0", dict(rows=-1), "rows < 0")]
CASES += [(F, f"no {n}", {n: None}, F_REQ) for n in ("x", "W1", "W2", "b2", "out", "ys", "idx")]
CASES += [(F, f"{n} misaligned", {n: GOOD[n] + 8}, F_ALIGN) for n in ("x", "W1", "hpre", "out")]
CASES += [
    (F, "bf16 out 4-byte aligned", dict(out=GOOD["out"] + 4, out_bf16=1), F_ALIGN),
    (F, "ldw < 64", dict(ldw=56), LDW),
    (F, "ldw % 8", dict(ldw=68), LDW),
    (F, "rows before operands", dict(rows=-1, x=None), "rows < 0"),
    (F, "operands before alignment", dict(ys=None, x=GOOD["x"] + 8), F_REQ),
    (F, "alignment before ldw", dict(W1=GOOD["W1"] + 8, ldw=68), F_ALIGN),
    (B, "rows < 0", dict(rows=-1), "rows < 0"),
]
CASES += [(B, f"no {n}", {n: None}, B_REQ) for n in ORDER[B].split() if n in POINTERS]
CASES += [(B, f"{n} misaligned", {n: GOOD[n] + 8}, B_ALIGN) for n in ("dout", "x", "hpre", "W1t", "W2", "dx", "dh")]
CASES += [
    (B, "ldw < 64", dict(ldw=32), LDW),
    (B, "ldw % 8", dict(ldw=68), LDW),
    (B, "rows before operands", dict(rows=-1, dh=None), "rows < 0"),
    (B, "operands before alignment", dict(db2=None, dx=GOOD["dx"] + 8), B_REQ),
    (B, "alignment before ldw", dict(dh=GOOD["dh"] + 8, ldw=68), B_ALIGN),
]

ACCEPTED = [
    (F, "rows = 0", dict(rows=0)),
    (F, "rows = 0 with nothing else valid", dict(rows=0, x=None, out=GOOD["out"] + 4, ldw=3)),
    (B, "rows = 0", dict(rows=0)),
    (B, "rows = 0 with nothing else valid", dict(rows=0, dx=None, dh=GOOD["dh"] + 4, ldw=3)),
]


def _args(name, change):
    unknown = set(change) - set(GOOD)
    assert not unknown, unknown
    v = dict(GOOD, **change)
    return [v[k] for k in ORDER[name].split()]


def test_table_matches_the_header():
    """The argument order above is the header's, and every check of both entry points has a case."""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "asrx.h")).read()
    for name, order in ORDER.items():
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        params = [re.sub(r"\s+", " ", p).strip().split(" ")[-1].lstrip("*") for p in m.group(1).split(",")]
        assert params == order.split(), (name, params)
    assert {c[3] for c in CASES if c[0] == F} == {"rows < 0", F_REQ, F_ALIGN, LDW}
    assert {c[3] for c in CASES if c[0] == B} == {"rows < 0", B_REQ, B_ALIGN, LDW}
    assert len({(c[0], c[1]) for c in CASES}) == len(CASES)


@pytest.mark.parametrize("name,what,change,text", CASES, ids=[f"{c[0][5:]}-{c[1]}".replace(" ", "_") for c in CASES])
def test_rejected(name, what, change, text):
    from asrx import lib

    with pytest.raises(RuntimeError) as e:
        lib.call(name, *_args(name, change))
    assert str(e.value) == f"{name} failed (code 2): {name}: {text}"


@pytest.mark.parametrize("name,what,change", ACCEPTED, ids=[f"{c[0][5:]}-{c[1]}".replace(" ", "_") for c in ACCEPTED])
def test_empty_is_accepted(name, what, change):
    from asrx import lib

    lib.call(name, *_args(name, change))
