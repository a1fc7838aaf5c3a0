"""The attention kernels (csrc/attn_mf.hip perf mode, csrc/attn.hip parity mode) against the float64 reference
of tests/attn_ref.py, ELEMENTWISE: |got - ref| <= bound for every element of O, dQ, dK, dV, Delta within bDelta,
lse within its tolerance.  The bounds are derived in attn_ref.py and proven on the CPU by test_attn_ref.py, which
runs the same attn_ref.CASES; how they were chosen (tile, block, grid, mask and Delta-loop edges, the two
forward variants, four input families, all eight storage combinations) is written there.

asrx_attn_fwd2 / asrx_attn_bwd2 are called directly, so strides, lse and the Delta workspace are in the test's
hands.  Every operand lives in a buffer a few rows longer than L whose extra rows (and, in the padded layouts, the
gap after each row) hold NaN for inputs and a sentinel for outputs: a kernel that USES a clamped or zero-filled
row shows up as NaN, and one that writes between the logical rows breaks the sentinel, which is compared bit for
bit.  Everything stays inside the test's own allocations.

Layouts: contiguous; "kvpad": k and v the two halves of one (B, L, 2, H, hd) buffer (as dk and dv), q / dO / o / dq
with rows padded by 4 elements (fp32) or 8 (bf16); "headmajor": (B, H, L, hd) passed as a transposed view.
bf16-stored q / k / v / dO are read 16 bytes at a time, and nothing in the documents at hand says a 16-byte global
load may sit on an 8-byte boundary, so their strides must be multiples of 8 (pinned in test_attn_args.py) and no
bf16 row is padded by 4 here.

Two cases go through ops.attention for the merge_heads and gradient-sink plumbing.
"""
import faulthandler
import math

import pytest
import torch

import attn_ref as R

pytestmark = pytest.mark.gpu

PAD = 3  # extra rows of every buffer
SENTINEL = 12352.0  # exact in bf16 and fp32
WORST = {}  # (mode, output) -> (ratio, case id), printed at the end of the module


@pytest.fixture(autouse=True)
def _time_limit():
    """Each case has its own limit: a hung kernel ends the run instead of holding the GPU."""
    faulthandler.dump_traceback_later(60, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"worst err / bound, {k[0]} {k[1]}: {WORST[k][0]:.3f} ({WORST[k][1]})")


def _view(buf, layout, L, H, hd, half=None):
    """The logical (B, L, H, hd) view of a buffer made by _alloc."""
    if layout == "headmajor":
        return buf[:, :, :L].transpose(1, 2)
    if layout == "kvpad" and half is not None:
        return buf[:, :L, half]
    if layout == "kvpad":
        return buf[:, :L, :H * hd].unflatten(-1, (H, hd))
    return buf[:, :L]


def _alloc(layout, B, L, H, hd, dtype, fill, dev, pair=False):
    if layout == "headmajor":
        shape = (B, H, L + PAD, hd)
    elif layout == "kvpad" and pair:
        shape = (B, L + PAD, 2, H, hd)
    elif layout == "kvpad":
        shape = (B, L + PAD, H * hd + (8 if dtype == torch.bfloat16 else 4))
    else:
        shape = (B, L + PAD, H, hd)
    return torch.full(shape, fill, dtype=dtype, device=dev)


def _st(t):
    import ctypes

    arr = (ctypes.c_int64 * 3)(t.stride(0), t.stride(1), t.stride(2))
    return arr, ctypes.cast(arr, ctypes.c_void_p).value


def _gaps_untouched(buf, views):
    """Everything of buf outside the logical views still holds the sentinel, bit for bit."""
    c = buf.clone()
    for mk in views:
        mk(c).fill_(SENTINEL)
    it = torch.int16 if buf.dtype == torch.bfloat16 else torch.int32
    want = torch.tensor(SENTINEL, dtype=buf.dtype).view(it).item()
    return bool((c.view(it) == want).all())


def _run_kernels(case, raw, dev):
    """Forward and backward through the C-ABI in the case's layout and storage -> (got, problems)."""
    from asrx import lib

    c = case
    B, H, Lq, Lk, hd, lay = c.B, c.H, c.Lq, c.Lk, c.hd, c.layout
    nan = float("nan")
    ins = {}
    kvbuf = None
    for name, L in (("q", Lq), ("k", Lk), ("v", Lk), ("dO", Lq)):
        t = raw[name]
        if lay == "kvpad" and name in ("k", "v"):
            if kvbuf is None:
                kvbuf = _alloc(lay, B, L, H, hd, t.dtype, nan, dev, pair=True)
            view = _view(kvbuf, lay, L, H, hd, half=("k", "v").index(name))
        else:
            view = _view(_alloc(lay, B, L, H, hd, t.dtype, nan, dev), lay, L, H, hd)
        view.copy_(t.to(dev))
        ins[name] = view
    odt = torch.bfloat16 if c.io & 2 else torch.float32
    obuf = _alloc(lay, B, Lq, H, hd, odt, SENTINEL, dev)
    dqbuf = _alloc(lay, B, Lq, H, hd, torch.float32, SENTINEL, dev)
    if lay == "kvpad":
        dkvbuf = _alloc(lay, B, Lk, H, hd, torch.float32, SENTINEL, dev, pair=True)
        mk_dk, mk_dv = (lambda b: _view(b, lay, Lk, H, hd, half=0)), (lambda b: _view(b, lay, Lk, H, hd, half=1))
        dkbuf = dvbuf = dkvbuf
    else:
        dkbuf = _alloc(lay, B, Lk, H, hd, torch.float32, SENTINEL, dev)
        dvbuf = _alloc(lay, B, Lk, H, hd, torch.float32, SENTINEL, dev)
        mk_dk = mk_dv = lambda b: _view(b, lay, Lk, H, hd)
    mk_q = lambda b: _view(b, lay, Lq, H, hd)  # noqa: E731
    o, dq, dk, dv = mk_q(obuf), mk_q(dqbuf), mk_dk(dkbuf), mk_dv(dvbuf)
    rows = B * H * Lq
    lse = torch.full((rows + 8,), SENTINEL, device=dev)
    delta = torch.full((rows + 8,), SENTINEL, device=dev)

    prec = 1 if c.mode == "perf" else 0
    st = {n: _st(t) for n, t in dict(ins, o=o, dq=dq, dk=dk, dv=dv).items()}
    P = lib.ptr
    old = lib.load().asrx_set_attn_variant(c.variant)
    try:
        lib.call("asrx_attn_fwd2", prec, c.io & 3, P(ins["q"]), st["q"][1], P(ins["k"]), st["k"][1], P(ins["v"]),
                 st["v"][1], P(o), st["o"][1], P(lse), B, H, Lq, Lk, hd, int(c.causal), c.scale, lib.stream())
        lib.call("asrx_attn_bwd2", prec, c.io, P(ins["q"]), st["q"][1], P(ins["k"]), st["k"][1], P(ins["v"]),
                 st["v"][1], P(o), st["o"][1], P(ins["dO"]), st["dO"][1], P(lse), P(delta), P(dq), st["dq"][1],
                 P(dk), st["dk"][1], P(dv), st["dv"][1], B, H, Lq, Lk, hd, int(c.causal), c.scale, lib.stream())
        torch.cuda.synchronize()
    finally:
        lib.load().asrx_set_attn_variant(old)
    problems = []
    for name, buf, views in (("o", obuf, [mk_q]), ("dq", dqbuf, [mk_q]), ("dk/dv", dkbuf, [mk_dk, mk_dv]),
                             ("dv", dvbuf, [mk_dk, mk_dv])):
        if not _gaps_untouched(buf, views):
            problems.append(f"{name}: written outside the logical rows")
    for name, t in (("lse", lse), ("delta_ws", delta)):
        if not bool((t[rows:] == SENTINEL).all()):
            problems.append(f"{name}: written past B*H*Lq")
    got = {"O": o, "dQ": dq, "dK": dk, "dV": dv}
    got = {n: t.detach().double().cpu() for n, t in got.items()}
    got["lse"] = lse[:rows].view(B, H, Lq).double().cpu()
    got["Delta"] = delta[:rows].view(B, H, Lq).double().cpu()
    return got, problems


def _judge(case, got, vis, ref, problems):
    for name, (r, idx) in R.ratios(got, ref).items():
        print(f"{case.id} {name} {r:.3f}")
        key = (case.mode, name)
        if r > WORST.get(key, (0.0, ""))[0]:
            WORST[key] = (r, case.id)
        if not r <= 1.0:
            problems.append(f"err / bound {r:.3g} at {R.where(case, name, idx)}")
    r, idx = R.ratio(got["Delta"], ref["Delta"], ref["bDelta"])
    print(f"{case.id} Delta {r:.3f}")
    key = (case.mode, "Delta")
    if r > WORST.get(key, (0.0, ""))[0]:
        WORST[key] = (r, case.id)
    if not r <= 1.0:
        row = (idx[0] * case.H + idx[1]) * case.Lq + idx[2]
        problems.append(f"Delta err / bDelta {r:.3g} at (b, h, row) = {idx}, pass {row // 32768} of the Delta loop")
    tol = R.lse_tolerance(case, vis, ref["lse"])
    e = (got["lse"] - ref["lse"]).abs()
    worst = float(e.max()) if bool(torch.isfinite(e).all()) else math.inf
    print(f"{case.id} lse {worst:.3g} (tolerance {tol:.3g})")
    if not worst < tol:
        problems.append(f"lse off by {worst:.3g} (tolerance {tol:.3g})")
    assert not problems, case.id + ": " + "; ".join(problems)


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_kernels_within_bounds(cuda, case):
    """Measured worst err / bound per output and mode: DESIGN.md, attention section.  lse at the peaked2 inputs
    (max |S| 650 .. 1100): the tolerance, 8 x the fp32 CPU evaluation's error, is computed per case and came to
    2.2e-3 .. 6.4e-3; the kernels were off by 1.2e-4 .. 2.5e-4 (perf) and 2.7e-4 .. 8.1e-4 (parity)."""
    raw, vis = R.make_inputs(case)
    ref = R.reference_for(case, vis)
    got, problems = _run_kernels(case, raw, cuda)
    _judge(case, got, vis, ref, problems)


@pytest.mark.parametrize("stored", [False, True])
def test_ops_attention_plumbing(cuda, stored):
    """ops.attention in the perf mode with merge_heads: k and v as the halves of one kv-projection buffer; with
    `stored` the output is stored bf16 and its gradient arrives through the output's sink, and q's gradient leaves
    through a fork's sink."""
    from asrx import ops, prec

    case = R.Case("perf", 2, 3, 257, 192, 64, False, "flat", 2) if stored else R.Case("perf", 2, 3, 257, 192, 64, False,
                                                                                       "unit", 0, "kvpad")
    assert case in R.CASES  # so test_attn_ref.py proves the bounds for these inputs too
    c = case
    raw, vis = R.make_inputs(case)
    ref = R.reference_for(case, vis)
    q = raw["q"].to(cuda).requires_grad_(True)
    kv = torch.stack([raw["k"], raw["v"]], 2).to(cuda).requires_grad_(True)  # (B, Lk, 2, H, hd)
    dO = raw["dO"].to(cuda).reshape(c.B, c.Lq, c.H * c.hd)
    with prec.precision("bf16"):
        qf = ops.fork(q) if stored else q
        y = ops.attention(qf, kv[:, :, 0], kv[:, :, 1], False, out_bf16=stored, merge_heads=True)
        assert y.shape == (c.B, c.Lq, c.H * c.hd)
        assert y.dtype == (torch.bfloat16 if stored else torch.float32)
        if stored:
            buf, acc = ops.sink_of(y).target(y)  # what a sink-capable consumer does with its fp32 gradient
            assert acc == 0
            buf.copy_(dO)
            y.backward(torch.zeros_like(y))
        else:
            assert ops.sink_of(y) is None
            y.backward(dO)
        torch.cuda.synchronize()
    got = {"O": y.detach().view(c.B, c.Lq, c.H, c.hd), "dQ": q.grad, "dK": kv.grad[:, :, 0], "dV": kv.grad[:, :, 1]}
    got = {n: t.double().cpu() for n, t in got.items()}
    problems = []
    for name, (r, idx) in R.ratios(got, ref).items():
        print(f"ops.attention stored={stored} {name} {r:.3f}")
        if not r <= 1.0:
            problems.append(f"err / bound {r:.3g} at {R.where(case, name, idx)}")
    assert not problems, "; ".join(problems)
