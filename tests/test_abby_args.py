"""The AbbyNormal row entry points (csrc/abby.hip: asrx_abby_fwd, _fwd2, _fwd_logits, _fwd_logits2, _fwd3, _fwd_res,
_bwd, _bwd2) reject bad calls before any launch: return code 2 and a fixed asrx_last_error() text, checked for every
argument check and the default of the dispatch switch (a multiple of 64 without an instantiation), and for which
check answers when several fail; rows == 0 returns 0 once d is accepted.

Validation is host code, so this runs without a GPU -- and only without one: the pointers are made-up integers
with the alignment a case needs, nothing reads them here, but a case that wrongly passed validation on a machine
with a device would launch a kernel on them.
"""
import os
import re

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up pointers: host validation only, no device")


def _addr(i):
    return 0x7F0000000000 + i * 0x10000000  # distinct, 16-byte aligned


TAIL = "rows d L H sid_base key use_noise"
ORDER = {
    "asrx_abby_fwd": f"x hpre W2 b2 out ys idx {TAIL} stream",
    "asrx_abby_fwd2": f"x hpre W2 b2 out out_bf16 ys idx {TAIL} tw tb tc stream",
    "asrx_abby_fwd_logits": f"x logits b2 out ys idx {TAIL} stream",
    "asrx_abby_fwd_logits2": f"x logits b2 out out_bf16 ys idx {TAIL} tw tb tc stream",
    "asrx_abby_fwd3": f"x hpre W2 logits b2 out out_bf16 ys idx {TAIL} tw tb tc nrm stream",
    "asrx_abby_fwd_res": f"x hpre W2 logits b2 res out ys idx {TAIL} stream",
    "asrx_abby_bwd": "dout x hpre W2 ys idx dx dhpre dW2 db2 rows d stream",
    "asrx_abby_bwd2": "dout x hpre W2 ys idx dx dhpre dW2 db2 rows d acc stream",
}
POINTERS = ["x", "hpre", "W2", "b2", "out", "ys", "idx", "logits", "res", "dout", "dx", "dhpre", "dW2", "db2", "tw",
            "tb", "tc", "nrm"]
GOOD = dict({n: _addr(i + 1) for i, n in enumerate(POINTERS)}, out_bf16=0, rows=100, d=128, L=100, H=1, sid_base=0,
            key=7, use_noise=0, acc=0, stream=None)
# the optional operands are absent from a plain call
GOOD.update(tw=None, tb=None, tc=None, nrm=None)
TW = dict(tw=_addr(40), tb=_addr(41), tc=_addr(42))
NRM = dict(nrm=_addr(43))


def RANGE(d):
    return f"AbbyNormal: d={d} must be a multiple of 64 in [64,1024]"


def UNSUPPORTED(d):
    return f"AbbyNormal: unsupported d={d}"


def F3_RANGE(d):
    return f"asrx_abby_fwd3: d={d} must be a multiple of 64 in [128,1024] with a norm output"


def RES_RANGE(d):
    return f"asrx_abby_fwd_res: d={d} must be a multiple of 64 in [128,1024]"


TGATE = "AbbyNormal: the fused tgate cs needs d >= 128"
F3_ROUTER = "asrx_abby_fwd3: logits or hpre/W2"
RES_OPERANDS = "asrx_abby_fwd_res: res (!= out) and logits or hpre/W2"

BAD_D = (0, 32, 100, 1088)  # outside the range check
NO_KERNEL = (192, 320, 640, 896)  # multiples of 64 in range that the dispatch switch has no case for

CASES = []
for n in ORDER:
    rng = RES_RANGE if n == "asrx_abby_fwd_res" else RANGE
    CASES += [(n, f"d = {d}", dict(d=d), rng(d)) for d in BAD_D]
    CASES += [(n, f"d = {d}", dict(d=d), UNSUPPORTED(d)) for d in NO_KERNEL]
    CASES += [(n, "bad d before rows = 0", dict(d=32, rows=0), rng(32))]

for n in ("asrx_abby_fwd2", "asrx_abby_fwd_logits2", "asrx_abby_fwd3"):
    CASES += [
        (n, "tw with d = 64", dict(TW, d=64), TGATE),
        (n, "tw before the range of d", dict(TW, d=32), TGATE),
        (n, "tw before rows = 0", dict(TW, d=64, rows=0), TGATE),
    ]

n = "asrx_abby_fwd3"
CASES += [(n, f"nrm, d = {d}", dict(NRM, d=d), F3_RANGE(d)) for d in (64,) + BAD_D]
CASES += [(n, f"nrm, d = {d}", dict(NRM, d=d), UNSUPPORTED(d)) for d in NO_KERNEL]
CASES += [
    (n, "nrm, tw with d = 64", dict(NRM, **TW, d=64), TGATE),
    (n, "nrm, no router input", dict(NRM, logits=None, hpre=None, W2=None), F3_ROUTER),
    (n, "nrm, hpre without W2", dict(NRM, logits=None, W2=None), F3_ROUTER),
    (n, "nrm, W2 without hpre", dict(NRM, logits=None, hpre=None), F3_ROUTER),
    (n, "nrm, d before router input", dict(NRM, d=64, logits=None, hpre=None), F3_RANGE(64)),
    (n, "nrm, router input before rows = 0", dict(NRM, rows=0, logits=None, hpre=None), F3_ROUTER),
    (n, "nrm, router input before the switch", dict(NRM, d=192, logits=None, hpre=None), F3_ROUTER),
    (n, "no nrm, d = 32 is the logits entry's", dict(d=32), RANGE(32)),
]

n = "asrx_abby_fwd_res"
CASES += [
    (n, "d = 64", dict(d=64), RES_RANGE(64)),
    (n, "no res", dict(res=None), RES_OPERANDS),
    (n, "res is out", dict(res=GOOD["out"]), RES_OPERANDS),
    (n, "no router input", dict(logits=None, hpre=None, W2=None), RES_OPERANDS),
    (n, "hpre without W2", dict(logits=None, W2=None), RES_OPERANDS),
    (n, "d before res", dict(d=64, res=None), RES_RANGE(64)),
    (n, "res before rows = 0", dict(rows=0, res=None), RES_OPERANDS),
    (n, "res before the switch", dict(d=192, res=None), RES_OPERANDS),
]

ACCEPTED = [(n, "rows = 0", dict(rows=0)) for n in ORDER]
ACCEPTED += [(n, "rows = 0, d = 64", dict(rows=0, d=64)) for n in ORDER if n != "asrx_abby_fwd_res"]
ACCEPTED += [
    ("asrx_abby_fwd3", "rows = 0 with nrm", dict(NRM, rows=0)),
    ("asrx_abby_fwd3", "rows = 0 with nrm and tw", dict(NRM, **TW, rows=0)),
    ("asrx_abby_fwd2", "rows = 0 with tw", dict(TW, rows=0)),
    ("asrx_abby_fwd_logits2", "rows = 0 with tw", dict(TW, rows=0)),
    ("asrx_abby_fwd_res", "rows = 0 from hpre / W2", dict(rows=0, logits=None)),
    # rows = 0 returns before the dispatch switch: a d without an instantiation is refused only with rows
    ("asrx_abby_bwd2", "rows = 0, d = 192", dict(rows=0, d=192)),
]


def _args(name, change):
    unknown = set(change) - set(GOOD)
    assert not unknown, unknown
    v = dict(GOOD, **change)
    return [v[k] for k in ORDER[name].split()]


def _ids(cases):
    return [f"{c[0][5:]}-{c[1]}".replace(" ", "_") for c in cases]


def test_table_covers_every_entry_point():
    """The entry points and their argument order are the header's; every one has the range cases, the dispatch
    default and an accepted empty call; every fixed text of abby.hip's row entry points has a case."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "asrx.h")).read()
    names = set(re.findall(r"\b(asrx_abby_(?:fwd|bwd)[a-z0-9_]*)\s*\(", hdr))
    assert names == set(ORDER)
    for name, order in ORDER.items():
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        params = [re.sub(r"\s+", " ", p).strip().split(" ")[-1].lstrip("*") for p in m.group(1).split(",")]
        assert params == order.split(), (name, params)
        texts = {c[3] for c in CASES if c[0] == name}
        assert {UNSUPPORTED(d) for d in NO_KERNEL} <= texts and len(texts) >= len(BAD_D) + len(NO_KERNEL), name
        assert any(c[0] == name for c in ACCEPTED), name
    src = open(os.path.join(root, "asr-model_amd", "csrc", "abby.hip")).read()
    fixed = set(re.findall(r'"((?:AbbyNormal|asrx_abby_fwd3|asrx_abby_fwd_res): [^"]*)"', src))
    assert len(fixed) == 7, fixed  # range, tgate, unsupported; fwd3's two; fwd_res's two
    stems = {re.sub(r"d=-?\d+", "d=%ld", c[3]) for c in CASES}
    assert fixed == stems, fixed ^ stems
    assert len({(c[0], c[1]) for c in CASES}) == len(CASES)


@pytest.mark.parametrize("name,what,change,text", CASES, ids=_ids(CASES))
def test_rejected(name, what, change, text):
    from asrx import lib

    with pytest.raises(RuntimeError) as e:
        lib.call(name, *_args(name, change))
    assert str(e.value) == f"{name} failed (code 2): {text}"


@pytest.mark.parametrize("name,what,change", ACCEPTED, ids=_ids(ACCEPTED))
def test_empty_is_accepted(name, what, change):
    from asrx import lib

    lib.call(name, *_args(name, change))
