"""The fused per-head AbbyNormal kernels at d = 64 (csrc/abby.hip: asrx_abby64_fwd, asrx_abby64_bwd) against the
split path they replace, kernel by kernel: asrx_gemm_wn_router + asrx_abby_fwd_logits2 forward, asrx_abby_bwd2 +
the beta = 1 input-gradient GEMM backward.  Every output is filled with ref_check.SENTINEL first.

Forward: torch.equal on out (fp32 and bf16), ys, idx and h_pre (kept or not), with and without noise, b1 zero and
non-zero.  Backward: torch.equal on dx (written, and added to a random old dx) and on dh; dW2 / db2 (and dW1 / db1
from the unchanged weight-gradient kernel on the fused dh) as tier B of ref_check.py.  The tier-B reference is the
float64 sum of the split path's own per-row terms: dz read back from asrx_abby_bwd2 itself (W2 = unit rows and
h_pre = 0 make its dh the row's 0.5 dz, exactly), SiLU(h_pre) from asrx_act_fwd (the same silu_f), the stored dh
and x rounded to bf16 as the weight-gradient kernel loads them; e32 is the same sum in fp32 on the CPU and the bound
max(ops_floor(1), 20 e32) -- one product rounding per term, then only the order of the sum differs.

Shapes (B, L, H), rows = B L H: one row, a partial 16-row group, exactly one group, one group and a row, a
partial wave / workgroup with head and position wrap, one row per position, several workgroups, and two whose last
16-row group is partial beyond the first sweep of the forward's largest grid (2048 workgroups x 4 waves, one group
per wave and sweep; the loop is unrolled by two): 196 584 rows end with 8 rows in the second sweep, the loop's
second arm, and 288 036 rows -- more than two sweeps -- end with 4 rows in the third, the first arm again.  The
backward's grid (1024 workgroups) sweeps them three and five times.

Tier B figures measured on an MI355X when these tests were added (the worse of acc = 0, 1; e and e32 relative to
the largest entry of the float64 reference, bound = max(ops_floor(1), 20 e32)):

    kernel             shape     out  e         e32       bound
    abby64_bwd         1x1x1     dW2  4.74e-08  4.74e-08  9.47e-07   (db2, dW1, db1: e = e32 = 0)
    abby64_bwd         1x17x1    dW2  1.06e-07  1.06e-07  2.12e-06
    abby64_bwd         1x17x1    db2  1.86e-08  7.29e-08  1.46e-06
    abby64_bwd         1x17x1    dW1  5.64e-08  9.86e-08  1.97e-06
    abby64_bwd         1x17x1    db1  7.44e-08  7.44e-08  1.49e-06
    abby64_bwd         2x37x6    dW2  1.28e-07  6.98e-07  1.40e-05
    abby64_bwd         2x37x6    db2  5.32e-08  7.31e-08  1.46e-06
    abby64_bwd         2x37x6    dW1  2.40e-07  3.89e-07  7.78e-06
    abby64_bwd         2x37x6    db1  1.72e-07  1.16e-07  2.33e-06
    abby64_bwd         3x2731x6  dW2  5.29e-07  8.16e-06  1.63e-04
    abby64_bwd         3x2731x6  db2  5.64e-07  1.63e-07  3.25e-06
    abby64_bwd         3x2731x6  dW1  4.08e-07  5.92e-07  1.18e-05
    abby64_bwd         3x2731x6  db1  3.62e-07  2.47e-07  4.93e-06
    abby64_bwd         4x8191x6  dW2  8.99e-07  7.44e-06  1.49e-04
    abby64_bwd         4x8191x6  db2  3.09e-07  8.67e-08  1.73e-06
    abby64_bwd         4x8191x6  dW1  6.91e-07  8.21e-07  1.64e-05
    abby64_bwd         4x8191x6  db1  4.29e-07  2.11e-07  4.22e-06
    abby64_bwd         6x8001x6  dW2  1.30e-06  9.69e-06  1.94e-04
    abby64_bwd         6x8001x6  db2  7.04e-07  3.57e-07  7.13e-06
    abby64_bwd         6x8001x6  dW1  1.00e-06  9.87e-07  1.97e-05
    abby64_bwd         6x8001x6  db1  4.22e-07  2.65e-07  5.30e-06
    abby_bwd2 (split)  4x8191x6  dW2  8.93e-07  7.44e-06  1.49e-04
    abby_bwd2 (split)  4x8191x6  db2  7.69e-07  8.67e-08  1.73e-06
    abby_bwd2 (split)  6x8001x6  dW2  9.50e-07  9.69e-06  1.94e-04
    abby_bwd2 (split)  6x8001x6  db2  5.18e-07  3.57e-07  7.13e-06

The largest e / bound of the fused kernel is 0.18 (db2 at 196584 rows; the split kernel's own is 0.44 there).  The
sums arrive through atomics, so the figures move a little from run to run.  Model level: fused against split
6.6e-08 of the largest gradient, the split path's four runs 6.6e-08 - 1.3e-07 apart (bound: the 1e-06 floor).
"""
import pytest
import torch

from ref_check import SENTINEL, gen, ops_floor, sentinel, tier_b
from ref_check import call as _call

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 5, 3), (1, 16, 1), (1, 17, 1), (2, 37, 6), (1, 777, 1), (3, 2731, 6), (4, 8191, 6),
          (6, 8001, 6)]
FWD_SWEEP_GROUPS = 2048 * 4  # the forward's largest grid: one 16-row group per wave and sweep
KEY, SID = 0x5EED1234, 3
BF16 = torch.bfloat16


def test_large_shapes_end_ragged_in_both_arms():
    """The two large shapes end in a partial 16-row group: one in the forward's second sweep (the second arm of its
    loop, unrolled by two), one in the third (the first arm again, past two sweeps)."""
    sweeps = []
    for B, L, H in SHAPES[-2:]:
        rows = B * L * H
        assert rows % 16 != 0 and L <= 8192
        sweeps.append((rows // 16) // FWD_SWEEP_GROUPS)  # the sweep that holds the last, partial group
    assert sweeps == [1, 2]


def _ids(shapes):
    return ["x".join(str(v) for v in s) for s in shapes]


_INPUTS, _SPLIT_FWD = {}, {}


def _inputs(shape):
    """x (rows, 64) with rows of mixed scale (every mode is chosen, mode 2 takes the max on some features), the
    router's weights, an upstream gradient and an old dx -- made once per shape."""
    if shape not in _INPUTS:
        B, L, H = shape
        rows = B * L * H
        g = gen(1000 + rows)
        x = torch.randn(rows, 64, generator=g) * (0.25 + 4.0 * torch.rand(rows, 1, generator=g))
        x[torch.rand(rows, 64, generator=g) < 0.05] *= 6.0  # outliers: max > 2 avg windows
        W1 = torch.randn(64, 64, generator=g) / 8
        b1 = torch.randn(64, generator=g) * 0.2
        W2 = torch.randn(3, 64, generator=g) * 0.4
        b2 = torch.randn(3, generator=g) * 0.2
        gy = torch.randn(rows, 64, generator=g)
        old = torch.randn(rows, 64, generator=g)
        _INPUTS[shape] = {k: v.cuda() for k, v in dict(x=x, W1=W1, b1=b1, W2=W2, b2=b2, gy=gy, old=old).items()}
        _INPUTS[shape]["b1z"] = torch.zeros(64, device="cuda")
    return _INPUTS[shape]


def _wb(W, trans=False):
    from asrx import gemm as G

    return G.weight_bf16(W, trans=trans, cache=False)


def _split_fwd(shape, noise, b1nz):
    """The split path's forward (kept h_pre, fp32 and bf16 out), computed once per case and left unchanged."""
    k = (shape, noise, b1nz)
    if k not in _SPLIT_FWD:
        B, L, H = shape
        rows = B * L * H
        t = _inputs(shape)
        b1 = t["b1"] if b1nz else t["b1z"]
        Wb = _wb(t["W1"])
        hpre, logits = sentinel(rows, 64), sentinel(rows, 3)
        _call("asrx_gemm_wn_router", t["x"], 64, Wb, 64, b1, t["W2"], hpre, 64, logits, rows, 64, 64)
        lg2 = sentinel(rows, 3)  # h_pre not kept: the logits must not depend on it
        _call("asrx_gemm_wn_router", t["x"], 64, Wb, 64, b1, t["W2"], None, 64, lg2, rows, 64, 64)
        assert torch.equal(lg2, logits)
        res = dict(hpre=hpre)
        for ob in (0, 1):
            out = torch.full((rows, 64), SENTINEL, device="cuda", dtype=BF16 if ob else torch.float32)
            ys, idx = sentinel(rows, 3), torch.full((rows,), 7, dtype=torch.int32, device="cuda")
            _call("asrx_abby_fwd_logits2", t["x"], logits, t["b2"], out, ob, ys, idx, rows, 64, L, H, SID, KEY,
                  int(noise), None, None, None)
            res[ob] = (out, ys, idx)
        assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
        _SPLIT_FWD[k] = res
    return _SPLIT_FWD[k]


def _fused_fwd(shape, noise, b1nz, ob, keep):
    B, L, H = shape
    rows = B * L * H
    t = _inputs(shape)
    b1 = t["b1"] if b1nz else t["b1z"]
    out = torch.full((rows, 64), SENTINEL, device="cuda", dtype=BF16 if ob else torch.float32)
    ys, idx = sentinel(rows, 3), torch.full((rows,), 7, dtype=torch.int32, device="cuda")
    hpre = sentinel(rows, 64) if keep else None
    _call("asrx_abby64_fwd", t["x"], _wb(t["W1"]), 64, b1, t["W2"], t["b2"], out, ob, ys, idx, hpre, rows, L, H, SID,
          KEY, int(noise))
    return out, ys, idx, hpre


@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_forward_equals_split(shape):
    modes = set()
    for noise in (True, False):
        for b1nz in (True, False):
            ref = _split_fwd(shape, noise, b1nz)
            for ob in (0, 1):
                for keep in (True, False):
                    out, ys, idx, hpre = _fused_fwd(shape, noise, b1nz, ob, keep)
                    what = (shape, noise, b1nz, ob, keep)
                    assert torch.equal(idx, ref[ob][2]), what
                    assert torch.equal(ys, ref[ob][1]), what
                    assert torch.equal(out, ref[ob][0]), what
                    if keep:
                        assert torch.equal(hpre, ref["hpre"]), what
            modes |= set(ref[0][2].unique().tolist())
            assert int(ref[0][2].min()) >= 0 and int(ref[0][2].max()) <= 2
    if shape[0] * shape[1] * shape[2] >= 777:
        assert modes == {0, 1, 2}, modes  # the inputs exercise every mode


def test_noise_epoch():
    """A non-zero noise epoch changes the fused forward's draws, and they are the split path's at that epoch."""
    from asrx import lib

    shape = (2, 37, 6)
    base = _fused_fwd(shape, True, True, 0, False)
    try:
        lib.call("asrx_set_noise_epoch", 12345, lib.stream())
        _SPLIT_FWD.pop((shape, True, True), None)
        ref = _split_fwd(shape, True, True)
        got = _fused_fwd(shape, True, True, 0, True)
    finally:
        lib.call("asrx_set_noise_epoch", 0, lib.stream())
        _SPLIT_FWD.pop((shape, True, True), None)
    assert torch.equal(got[0], ref[0][0]) and torch.equal(got[1], ref[0][1]) and torch.equal(got[2], ref[0][2])
    assert torch.equal(got[3], ref["hpre"])
    assert not torch.equal(got[1], base[1])
    again = _fused_fwd(shape, True, True, 0, False)
    assert torch.equal(again[1], base[1]) and torch.equal(again[0], base[0])


def _row_terms(shape, fw):
    """The split kernel's own per-row dz (rows, 3) and SiLU(h_pre) (rows, 64), as float64 on the CPU."""
    rows = shape[0] * shape[1] * shape[2]
    t = _inputs(shape)
    _, ys, idx = fw[0]
    unit = torch.zeros(3, 64, device="cuda")
    unit[0, 0] = unit[1, 1] = unit[2, 2] = 1.0
    dxs, dhs = sentinel(rows, 64), sentinel(rows, 64)
    dW2, db2 = torch.zeros(3, 64, device="cuda"), torch.zeros(3, device="cuda")
    _call("asrx_abby_bwd2", t["gy"], t["x"], torch.zeros(rows, 64, device="cuda"), unit, ys, idx, dxs, dhs, dW2, db2,
          rows, 64, 0)
    dz = 2.0 * dhs[:, :3]
    # self-check on row 0: one row's db2 is its dz (0 + dz, the other slots 0)
    d1, h1 = sentinel(1, 64), sentinel(1, 64)
    w1, b1 = torch.zeros(3, 64, device="cuda"), torch.zeros(3, device="cuda")
    _call("asrx_abby_bwd2", t["gy"], t["x"], fw["hpre"], t["W2"], ys, idx, d1, h1, w1, b1, 1, 64, 0)
    assert torch.equal(b1, dz[0]), (b1, dz[0])
    hs = sentinel(rows, 64)
    _call("asrx_act_fwd", fw["hpre"], hs, rows * 64, 2)
    return dz.double().cpu(), hs.double().cpu()


def _sums(dz, hs, dhb, xb, dh):
    return dz.t() @ hs, dz.sum(0), dhb.t() @ xb, dh.sum(0)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids(SHAPES))
def test_backward_equals_split(shape):
    """Measured rows are in the module docstring."""
    from asrx import gemm as G
    from asrx import prec

    B, L, H = shape
    rows = B * L * H
    t = _inputs(shape)
    fw = _split_fwd(shape, True, True)
    _, ys, idx = fw[0]
    hpre = fw["hpre"]
    Wt = _wb(t["W1"], trans=True)
    dz, hs = _row_terms(shape, fw)
    for acc in (0, 1):
        # split: row kernel, then dx += dh W1 on the wide GEMM
        dx_s = t["old"].clone() if acc else sentinel(rows, 64)
        dh_s = sentinel(rows, 64)
        dW2_s, db2_s = torch.zeros(3, 64, device="cuda"), torch.zeros(3, device="cuda")
        _call("asrx_abby_bwd2", t["gy"], t["x"], hpre, t["W2"], ys, idx, dx_s, dh_s, dW2_s, db2_s, rows, 64, acc)
        G.gemm_wn(dh_s, Wt, dx_s, M=rows, N=64, K=64, lda=64, ldc=64, beta=1.0)
        dx_f = t["old"].clone() if acc else sentinel(rows, 64)
        dh_f = sentinel(rows, 64)
        dW2_f, db2_f = torch.zeros(3, 64, device="cuda"), torch.zeros(3, device="cuda")
        _call("asrx_abby64_bwd", t["gy"], t["x"], hpre, Wt, 64, t["W2"], ys, idx, dx_f, dh_f, dW2_f, db2_f, rows, acc)
        assert torch.equal(dh_f, dh_s), (shape, acc)
        assert torch.equal(dx_f, dx_s), (shape, acc)
        # the weight gradient of the router's first Linear, from the fused dh (the kernel is unchanged)
        dW1, db1 = torch.zeros(64, 64, device="cuda"), torch.zeros(64, device="cuda")
        with prec.precision("bf16"):
            G.linear_wgrad(dh_f, t["x"], out=dW1, accumulate=True, db=db1)
        dhc = dh_s.cpu()
        args = (dz, hs, dhc.to(BF16).double(), t["x"].cpu().to(BF16).double(), dhc.double())
        tier_b(f"abby64_bwd {shape} acc={acc}", (dW2_f, db2_f, dW1, db1), _sums, args, ops_floor(1),
               names=("dW2", "db2", "dW1", "db1"))
        tier_b(f"abby_bwd2 (split) {shape} acc={acc}", (dW2_s, db2_s), lambda a, b: (a.t() @ b, a.sum(0)), (dz, hs),
               ops_floor(1), names=("dW2", "db2"))


def _model_run(model, batch, fused):
    from asrx import ops, prec

    ops.ABBY64_FUSED = fused
    model.zero_grad(set_to_none=True)
    model.set_noise(1, 0)
    with prec.precision("bf16"):
        out = model(**batch)
        out["loss"].backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return out["loss"].detach().clone(), out["logits"].detach().clone(), grads


def _grad_dist(a, b, scale):
    assert a.keys() == b.keys()
    return max(float((a[n] - b[n]).abs().max()) for n in a) / scale


def test_model_switch_on_equals_off(monkeypatch):
    """dims 128, 2 heads (d = 64 per head), 2 layers, B = 2, 41 frames, training: loss and logits equal with the
    switch on and off; gradients within 4 x the split path's own run-to-run spread (floor 1e-6), relative to the
    largest gradient entry.  The row threshold is lowered so this size takes the router kernels either way."""
    from asrx import lib, ops
    from asrx.config import Dimensions
    from asrx.model import Model

    monkeypatch.setattr(ops, "ROUTER_FUSED_MIN_ROWS", 1)
    monkeypatch.setattr(ops, "ABBY64_FUSED", False)
    calls = {}
    real = lib.call

    def counting(name, *a):
        calls[name] = calls.get(name, 0) + 1
        return real(name, *a)

    monkeypatch.setattr(lib, "call", counting)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = Dimensions(tokens=500, mels=128, dims=128, head=2, layer=2, act="gelu", n_type="AbbyNormal")
    model = Model(cfg).to(dev).train()
    g = gen(0)
    B, T, S = 2, 6, 41
    ids = torch.randint(3, 500, (B, T), generator=g)
    ids[:, 0] = 1
    labels = torch.cat([ids[:, 1:], torch.full((B, 1), 2)], 1)
    batch = dict(labels=labels.to(dev), text_ids=ids.to(dev), spectrogram=torch.randn(B, 128, S, generator=g).to(dev),
                 pitch=(torch.rand(B, 1, S, generator=g) * 200).to(dev),
                 waveform=(torch.randn(B, 1, S - 1, generator=g) * 0.1).to(dev))
    split = [_model_run(model, batch, False) for _ in range(4)]
    assert calls.get("asrx_abby64_fwd", 0) == 0 and calls.get("asrx_abby_bwd2", 0) > 0
    scale = max(float(v.abs().max()) for v in split[0][2].values())
    spread = max(_grad_dist(split[i][2], split[j][2], scale) for i in range(4) for j in range(i))
    bound = max(4.0 * spread, 1e-6)
    n_bwd2 = calls["asrx_abby_bwd2"]
    fused = [_model_run(model, batch, True) for _ in range(2)]
    assert calls.get("asrx_abby64_fwd", 0) > 0 and calls.get("asrx_abby64_bwd", 0) > 0
    assert calls["asrx_abby_bwd2"] > n_bwd2  # the d = 128 norms stay on the split kernels
    for loss, logits, grads in fused:
        assert torch.equal(loss, split[0][0]) and torch.equal(logits, split[0][1])
        d = _grad_dist(grads, split[0][2], scale)
        print(f"model grads: fused - split {d:.3e}, split spread {spread:.3e}, bound {bound:.3e}")
        assert d <= bound, (d, spread, bound)
