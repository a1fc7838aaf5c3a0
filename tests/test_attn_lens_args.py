"""The per-sample-length attention entry points (csrc/attn_lens.hip: asrx_lattn_fwd, asrx_lattn_bwd) reject bad
calls before any launch, like the uniform ones (test_attn_args.py, whose table this file reuses):

- every refusal of asrx_attn_fwd2 / asrx_attn_bwd2 is given by the new entry point too, with code 2 and the same
  text, and the B*H*Lq == 0 early return stands at the same place.  One difference, which is the second new check:
  a fp8 call that the uniform forward refuses for its alignment is refused for being fp8 first;
- the three new checks: the fp8 forward ("per-sample lengths are not built for the fp8 forward", right after the
  precision check it extends, so after the early return and the empty-key check and before the alignment check),
  a null `lens` and a `lens` that is not 4-byte aligned (after the tensor alignment check, in that order).  The
  backward refuses fp8 with the uniform backward's own words (its precision check comes first);
- a child process with the HIP runtime's call log shows that a refused backward has launched nothing, the Delta
  pass included.

Host code with made-up pointers: runs only without a GPU, like test_attn_args.py.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import test_attn_args as T

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up pointers: host validation only, no device")

FWD, BWD = "asrx_lattn_fwd", "asrx_lattn_bwd"
ORDER = {
    FWD: "prec io q sq k sk v sv o so lse lens B H Lq Lk hd causal scale stream",
    BWD: "prec io q sq k sk v sv o so dO sd lse delta dq sdq dk sdk dv sdv lens B H Lq Lk hd causal scale stream",
}
UNIFORM = {FWD: "asrx_attn_fwd2", BWD: "asrx_attn_bwd2"}
GOOD = dict(T.GOOD, lens=T._addr(11))

NOFP8 = "attention: per-sample lengths are not built for the fp8 forward"
LNULL = "attention: per-sample lengths: null table"
LALIGN = "attention: per-sample lengths: table must be 4-byte aligned"
OK = T.OK


def _shared(n):
    """The uniform entry point's cases, in the words it uses."""
    out = []
    for name, what, change, text in T.CASES:
        if name != UNIFORM[n]:
            continue
        if n == FWD and change.get("prec") == T.FP8 and text == T.AL_F:
            text = NOFP8  # the fp8 refusal stands ahead of the alignment check
        out.append((n, what, change, text))
    return out


CASES = _shared(FWD) + _shared(BWD)
for n, AL, ptr in ((FWD, T.AL_F, "o"), (BWD, T.AL_B, "dv")):
    CASES += [
        (n, "lens null", dict(lens=None), LNULL),
        (n, "fp32, lens null", dict(prec=T.F32, lens=None), LNULL),
        (n, "lens + 2", dict(lens=GOOD["lens"] + 2), LALIGN),
        (n, "lens + 1", dict(lens=GOOD["lens"] + 1), LALIGN),
        (n, "fp32, lens + 2", dict(prec=T.F32, lens=GOOD["lens"] + 2), LALIGN),
        (n, "lens + 4 is aligned, Lq = 0", dict(lens=GOOD["lens"] + 4, Lq=0), OK),
        # which check answers
        (n, "alignment before lens null", {ptr: GOOD[ptr] + 8, "lens": None}, AL),
        (n, "alignment before lens alignment", dict(q=GOOD["q"] + 8, lens=GOOD["lens"] + 2), AL),
        (n, "fp32: no alignment check, lens null", dict(prec=T.F32, q=GOOD["q"] + 8, lens=None), LNULL),
        (n, "early return before lens null", dict(B=0, lens=None), OK),
        (n, "early return before lens alignment", dict(Lq=0, lens=GOOD["lens"] + 2), OK),
        (n, "no keys before lens null", dict(Lk=0, lens=None), T.NOKEYS),
        (n, "grid before lens null", dict(H=65536, lens=None), T.GRID),
        (n, "strides before lens null", dict(sq=T._st(1, 194), lens=None), T.STR4),
        (n, "head dim before lens alignment", dict(hd=96, lens=GOOD["lens"] + 2), T.HD % 96),
    ]
CASES += [
    (FWD, "fp8", dict(prec=T.FP8), NOFP8),
    (FWD, "fp8 before lens null", dict(prec=T.FP8, lens=None), NOFP8),
    (FWD, "fp8 before alignment", dict(prec=T.FP8, k=GOOD["k"] + 8), NOFP8),
    (FWD, "bad precision, not fp8", dict(prec=3, lens=None), T.PREC_F % 3),
    (FWD, "no keys before fp8", dict(prec=T.FP8, Lk=0), T.NOKEYS),
    (FWD, "early return before fp8", dict(prec=T.FP8, Lq=0), OK),
    (FWD, "io before fp8", dict(prec=T.FP8, io=1), T.IO_F % 1),
    (FWD, "head dim before fp8", dict(prec=T.FP8, hd=32), T.HD % 32),
    (BWD, "fp8: the uniform backward's words", dict(prec=T.FP8, lens=None), T.PREC_B % 2),
]
IDS = [f"{c[0][5:]}-{c[1]}".replace(" ", "_") for c in CASES]


def _call(name, change):
    from asrx import lib

    unknown = set(change) - set(GOOD)
    assert not unknown, unknown
    v = dict(GOOD, **change)
    keep, args = [], []
    for k in ORDER[name].split():
        if k in T.STRIDES:
            keep.append((ctypes.c_int64 * 3)(*v[k]))
            args.append(ctypes.cast(keep[-1], ctypes.c_void_p).value)
        else:
            args.append(v[k])
    lib.call(name, *args)


def test_table_covers_both_entry_points():
    """The header declares exactly these two asrx_lattn_* entry points; every error text of csrc/attn_lens.hip is
    pinned here for each entry point that can give it, and the texts it shares with csrc/attn.hip are the same
    strings."""
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "asrx.h")).read()
    assert set(re.findall(r"\b(asrx_lattn_[a-z0-9_]*)\s*\(", hdr)) == set(ORDER)
    rx = r'ASRX_REQUIRE\((?:[^"]|\n)*?"([^"]+)"'
    mine = set(re.findall(rx, open(os.path.join(root, "asr-model_amd", "csrc", "attn_lens.hip")).read()))
    theirs = set(re.findall(rx, open(os.path.join(root, "asr-model_amd", "csrc", "attn.hip")).read()))
    assert mine - theirs == {NOFP8, LNULL, LALIGN}
    assert theirs <= mine  # every shared refusal, word for word
    assert len({(c[0], c[1]) for c in CASES}) == len(CASES)
    for t in mine:
        pat = re.escape(t).replace("%ld", "%d").replace("%d", r"-?\d+")
        assert any(c[3] is not None and re.fullmatch(pat, c[3]) for c in CASES), t
    for n in ORDER:
        got = {c[3] for c in CASES if c[0] == n}
        assert {T.STR4, T.STR8, T.GRID, T.NOKEYS, OK, LNULL, LALIGN} <= got, n
        assert len([c for c in CASES if c[0] == n]) >= len([c for c in T.CASES if c[0] == UNIFORM[n]]) + 15


@pytest.mark.parametrize("name,what,change,text", CASES, ids=IDS)
def test_rejected(name, what, change, text):
    if text is OK:
        _call(name, change)  # code 0, nothing launched: a launch without a device would have raised
        return
    with pytest.raises(RuntimeError) as e:
        _call(name, change)
    assert str(e.value) == f"{name} failed (code 2): {text}"


_CHILD = r"""
import sys
sys.path[:0] = {paths!r}
import test_attn_lens_args as A
T = A.T
try:
    A._call(A.BWD, dict(prec=T.F32))  # a valid call: validation passes and the Delta launch is tried
    print("CONTROL: no error")
except RuntimeError as e:
    print("CONTROL:", e)
sys.stdout.flush(); sys.stderr.flush()
print("=== rejected calls ===", file=sys.stderr); sys.stderr.flush()
n = 0
bad = [dict(lens=None), dict(lens=A.GOOD["lens"] + 2), dict(prec=T.F32, lens=None), dict(prec=T.F32, lens=A.GOOD["lens"] + 1),
       dict(prec=T.FP8)] + [{{p: A.GOOD[p] + 8}} for p in ("q", "k", "v", "dO", "dq", "dk", "dv")]
for change in bad:
    try:
        A._call(A.BWD, change)
    except RuntimeError as e:
        n += "(code 2)" in str(e)
print("REJECTED:", n)
"""


def test_rejected_backward_launches_nothing():
    """As test_attn_args.py's test of the same name: one valid call, whose launch attempt must show in the HIP
    runtime's call log (without a device it fails, which is all it can do here), then twelve refused ones (the
    two new checks in both precisions, fp8, the seven misaligned tensors), which must leave no launch in it.
    Skipped where the runtime logs nothing."""
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here, os.path.join(os.path.dirname(here), "asr-model_amd")]
    env = dict(os.environ, AMD_LOG_LEVEL="3")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"CONTROL: {BWD} failed" in r.stdout and "launch failed" in r.stdout, r.stdout
    assert "REJECTED: 12" in r.stdout, r.stdout
    before, _, after = r.stderr.partition("=== rejected calls ===")
    if "hipPushCallConfiguration" not in before and "hipLaunchKernel" not in before:
        pytest.skip("the HIP runtime logs no launches here")
    assert "hipPushCallConfiguration" not in after and "hipLaunchKernel" not in after, after[-2000:]
