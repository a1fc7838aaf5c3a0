"""The attention entry points (csrc/attn.hip: asrx_attn_fwd2, asrx_attn_bwd2 and the two legacy wrappers) reject
bad calls before any launch: return code 2 and a fixed asrx_last_error() text, checked here for every argument
check, for each stride array on its own, and for which check answers when two fail.  The B*H*Lq == 0 early return
(code 0, nothing launched) has its place in that order too.

The backward checks `so`, has the H / B limit of the forward (the fp32 kernels launch dim3(., H, B)), wants the
strides of a bf16-stored q / k / v / dO to be multiples of 8 like the forward (they are read 16 bytes at a time),
and makes every check before its first launch, the Delta kernel: test_rejected_backward_launches_nothing reads
the HIP runtime's own call log for that.

Validation is host code, so this runs without a GPU -- and only without one (tests/test_gemm_wn_args.py): the
pointers are made-up integers, and a case that wrongly passed validation on a machine with a device would launch
a kernel on them.  The stride arrays are real.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up pointers: host validation only, no device")

F32, BF16, FP8 = 0, 1, 2  # prec


def _addr(i):
    return 0x7F0000000000 + i * 0x10000000  # distinct, 16-byte aligned


ORDER = {
    "asrx_attn_fwd2": "prec io q sq k sk v sv o so lse B H Lq Lk hd causal scale stream",
    "asrx_attn_fwd": "prec q sq k sk v sv o so lse B H Lq Lk hd causal scale stream",
    "asrx_attn_bwd2": "prec io q sq k sk v sv o so dO sd lse delta dq sdq dk sdk dv sdv B H Lq Lk hd causal scale "
    "stream",
    "asrx_attn_bwd": "prec q sq k sk v sv o so dO sd lse delta dq sdq dk sdk dv sdv B H Lq Lk hd causal scale stream",
}
POINTERS = ["q", "k", "v", "o", "lse", "dO", "delta", "dq", "dk", "dv"]
STRIDES = ["sq", "sk", "sv", "so", "sd", "sdq", "sdk", "sdv"]
ST = (300 * 3 * 64, 3 * 64, 64)  # contiguous (B, 300, 3, 64)
GOOD = dict({n: _addr(i + 1) for i, n in enumerate(POINTERS)}, **{s: ST for s in STRIDES}, prec=BF16, io=0, B=2, H=3,
            Lq=300, Lk=300, hd=64, causal=0, scale=0.125, stream=None)

IO_F = "attention: bf16 storage (io %d) is a bf16-mode layout"
IO_B = "attention backward: bf16 storage (io %d) is a bf16-mode layout"
PREC_F = "attention: bad precision %d"
PREC_B = "attention backward: precision %d (fp8 is forward only)"
HD = "attention: head dim %d unsupported (64 or 128)"
STR4 = "attention: strides must be multiples of 4"
STR8 = "attention: strides of bf16-stored operands must be multiples of 8"
GRID = "attention: grid too large"
NOKEYS = "attention: empty key sequence"
AL_F = "attention: bf16/fp8 modes need 16-byte aligned q/k/v/o"
AL_B = "attention backward: bf16 mode needs 16-byte aligned tensors"
OK = None  # the early return: code 0


def _st(i, v):
    s = list(ST)
    s[i] = v
    return tuple(s)


def _common(n, fwd):
    """The checks both directions share, in the words of entry point n."""
    c = [(n, f"hd {h}", dict(hd=h), HD % h) for h in (0, 32, 96, 256)]
    arrays = STRIDES[:4] if fwd else STRIDES
    for s in arrays:
        c.append((n, f"{s} seq % 4", {s: _st(1, 194)}, STR4))
    for i, what in enumerate(("batch", "seq", "head")):
        c.append((n, f"sq {what} % 4 only", dict(sq=_st(i, ST[i] + 2)), STR4))
        c.append((n, f"{arrays[-1]} {what} % 4 only", {arrays[-1]: _st(i, ST[i] + 2)}, STR4))
    c += [
        (n, "H = 65536", dict(H=65536), GRID),
        (n, "B = 65536", dict(B=65536), GRID),
        (n, "fp32, H = 65536", dict(prec=F32, H=65536), GRID),
        (n, "no keys", dict(Lk=0), NOKEYS),
        (n, "fp32, no keys", dict(prec=F32, Lk=0), NOKEYS),
        (n, "Lq = 0", dict(Lq=0), OK),
        (n, "B = 0", dict(B=0), OK),
        (n, "H = 0", dict(H=0), OK),
        # which check answers
        (n, "head dim before strides", dict(hd=32, sq=_st(1, 194)), HD % 32),
        (n, "strides before grid", dict(sk=_st(2, 66), H=65536), STR4),
        (n, "grid before the early return", dict(B=65536, Lq=0), GRID),
        (n, "strides before the early return", dict(sv=_st(0, 6), Lq=0), STR4),
        (n, "early return before no keys", dict(Lq=0, Lk=0), OK),
        (n, "early return before alignment", dict(B=0, q=GOOD["q"] + 4), OK),
        (n, "no keys before alignment", dict(Lk=0, k=GOOD["k"] + 8), NOKEYS),
    ]
    return c


CASES = []
for n in ("asrx_attn_fwd2", "asrx_attn_fwd"):
    CASES += _common(n, True)
    for p in ("q", "k", "v", "o"):
        CASES.append((n, f"{p} misaligned", {p: GOOD[p] + 8}, AL_F))
        CASES.append((n, f"fp8, {p} misaligned", {"prec": FP8, p: GOOD[p] + 4}, AL_F))
    CASES += [
        (n, "precision 3", dict(prec=3), PREC_F % 3),
        (n, "precision -1", dict(prec=-1), PREC_F % -1),
        (n, "no keys before precision", dict(prec=3, Lk=0), NOKEYS),
        (n, "precision before alignment", dict(prec=7, v=GOOD["v"] + 8), PREC_F % 7),
        (n, "early return before precision", dict(prec=3, Lq=0), OK),
    ]
n = "asrx_attn_fwd2"
CASES += [
    (n, "io 1, fp32", dict(prec=F32, io=1), IO_F % 1),
    (n, "io 2, fp8", dict(prec=FP8, io=2), IO_F % 2),
    (n, "io 3, bad precision", dict(prec=3, io=3), IO_F % 3),
    (n, "io before head dim", dict(prec=F32, io=1, hd=32), IO_F % 1),
    (n, "bf16 q, sq % 8", dict(io=1, sq=_st(1, 196)), STR8),
    (n, "bf16 k, sk % 8", dict(io=1, sk=_st(2, 68)), STR8),
    (n, "bf16 v, sv % 8", dict(io=3, sv=_st(0, ST[0] + 4)), STR8),
    (n, "% 4 before % 8", dict(io=1, sq=_st(1, 196), so=_st(1, 194)), STR4),
    (n, "% 8 before grid", dict(io=1, sq=_st(1, 196), H=65536), STR8),
    (n, "% 8 before the early return", dict(io=1, sk=_st(1, 196), Lq=0), STR8),
]

for n in ("asrx_attn_bwd2", "asrx_attn_bwd"):
    CASES += _common(n, False)
    for p in ("q", "k", "v", "dO", "dq", "dk", "dv"):
        CASES.append((n, f"{p} misaligned", {p: GOOD[p] + 8}, AL_B))
    CASES += [
        (n, "precision 2", dict(prec=FP8), PREC_B % 2),
        (n, "precision 3", dict(prec=3), PREC_B % 3),
        (n, "precision before head dim", dict(prec=FP8, hd=32), PREC_B % 2),
        (n, "precision before the early return", dict(prec=FP8, Lq=0), PREC_B % 2),
        (n, "so before grid", dict(so=_st(2, 66), B=65536), STR4),
    ]
n = "asrx_attn_bwd2"
CASES += [
    (n, "io 1, fp32", dict(prec=F32, io=1), IO_B % 1),
    (n, "io 4, fp32", dict(prec=F32, io=4), IO_B % 4),
    (n, "io before precision", dict(prec=FP8, io=2), IO_B % 2),
    (n, "bf16 q, sq % 8", dict(io=1, sq=_st(1, 196)), STR8),
    (n, "bf16 k, sk % 8", dict(io=3, sk=_st(2, 68)), STR8),
    (n, "bf16 v, sv % 8", dict(io=5, sv=_st(0, ST[0] + 4)), STR8),
    (n, "bf16 dO, sd % 8", dict(io=4, sd=_st(1, 196)), STR8),
    (n, "bf16 dO, sd % 8, o bf16 too", dict(io=6, sd=_st(2, 68)), STR8),
    (n, "% 4 before % 8", dict(io=4, sd=_st(1, 196), sdv=_st(1, 194)), STR4),
    (n, "% 8 before grid", dict(io=4, sd=_st(1, 196), H=65536), STR8),
    (n, "% 8 before no keys", dict(io=1, sq=_st(1, 196), Lk=0), STR8),
]
IDS = [f"{c[0][10:]}-{c[1]}".replace(" ", "_") for c in CASES]


def _call(name, change):
    from asrx import lib

    unknown = set(change) - set(GOOD)
    assert not unknown, unknown
    v = dict(GOOD, **change)
    keep, args = [], []
    for k in ORDER[name].split():
        if k in STRIDES:
            keep.append((ctypes.c_int64 * 3)(*v[k]))
            args.append(ctypes.cast(keep[-1], ctypes.c_void_p).value)
        else:
            args.append(v[k])
    lib.call(name, *args)


def test_table_covers_every_entry_point():
    """Every asrx_attn_* entry point of the header that takes tensors has its cases, and every error text of
    csrc/attn.hip's entry points is pinned for each entry point that can give it."""
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "asrx.h")).read()
    names = set(re.findall(r"\b(asrx_attn_[a-z0-9_]*)\s*\(", hdr))
    assert names == set(ORDER)
    src = open(os.path.join(root, "asr-model_amd", "csrc", "attn.hip")).read()
    texts = set(re.findall(r'ASRX_REQUIRE\((?:[^"]|\n)*?"([^"]+)"', src))
    assert len(texts) == 11, texts
    for t in texts:
        pat = re.escape(t).replace("%ld", "%d").replace("%d", r"-?\d+")
        assert any(c[3] is not None and re.fullmatch(pat, c[3]) for c in CASES), t
    assert len({(c[0], c[1]) for c in CASES}) == len(CASES)
    for name in names:
        mine = {c[3] for c in CASES if c[0] == name}
        assert {STR4, GRID, NOKEYS, OK} <= mine, name


@pytest.mark.parametrize("name,what,change,text", CASES, ids=IDS)
def test_rejected(name, what, change, text):
    if text is OK:
        _call(name, change)  # code 0, nothing launched: a launch without a device would have raised
        return
    with pytest.raises(RuntimeError) as e:
        _call(name, change)
    assert str(e.value) == f"{name} failed (code 2): {text}"


_CHILD = r"""
import ctypes, sys
sys.path[:0] = {paths!r}
import test_attn_args as T
try:
    T._call("asrx_attn_bwd2", dict(prec=T.F32))  # a valid call: validation passes and the Delta launch is tried
    print("CONTROL: no error")
except RuntimeError as e:
    print("CONTROL:", e)
sys.stdout.flush(); sys.stderr.flush()
print("=== rejected calls ===", file=sys.stderr); sys.stderr.flush()
n = 0
for name in ("asrx_attn_bwd2", "asrx_attn_bwd"):
    for p in ("q", "k", "v", "dO", "dq", "dk", "dv"):
        try:
            T._call(name, {{p: T.GOOD[p] + 8}})
        except RuntimeError as e:
            n += str(e).endswith(T.AL_B)
print("REJECTED:", n)
"""


def test_rejected_backward_launches_nothing():
    """The backward's alignment check used to stand after the Delta launch: a misaligned call was refused with
    the workspace already written.  A child process with the HIP runtime's call log on (AMD_LOG_LEVEL) makes one
    valid call, whose launch attempt must show in the log (without a device it fails, which is all it can do here),
    then the fourteen misaligned ones, which must leave no launch in it.  Skipped where the runtime logs nothing."""
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here, os.path.join(os.path.dirname(here), "asr-model_amd")]
    env = dict(os.environ, AMD_LOG_LEVEL="3")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "CONTROL: asrx_attn_bwd2 failed" in r.stdout and "launch failed" in r.stdout, r.stdout
    assert "REJECTED: 14" in r.stdout, r.stdout
    before, _, after = r.stderr.partition("=== rejected calls ===")
    if "hipPushCallConfiguration" not in before and "hipLaunchKernel" not in before:
        pytest.skip("the HIP runtime logs no launches here")
    assert "hipPushCallConfiguration" not in after and "hipLaunchKernel" not in after, after[-2000:]
