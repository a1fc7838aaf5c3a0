"""MSheath with per-sample lengths, in float64 on the CPU (tests/msheath_lens_ref.py): the masked computation over the
padded batch equals the oracle on every x[b:b+1, :T_b] -- output, input gradient and the parameter gradients summed
over the samples -- to 1e-12; the pad rows of dx are exactly zero; a finite sentinel in the pad rows of x and NaN in
those of the cotangent change nothing; and each of the five mask points is needed: switched off alone it breaks the
equality.  The equality includes the column sum over ALL L rows of the last jump output, as the kernels' column sums
and weight-gradient GEMMs form such sums (no row mask of their own): that term is what needs xzero, the zero pad rows
of x_new and of the jump output, which a per-row autograd comparison with masked means and a masked output cannot show.

The inputs are those of tests/test_gpu_msheath_lens.py (MSheath(128, 2, 4), B = 8, L = 200, the lengths
[200, 199, 1, 63, 64, 65, 128, 129], sample 1 damped), and the last test asserts that lengths matter for them.
It also pins the reciprocal identity the LENS kernels rely on when they form 1 / T_b on the device.
"""
import numpy as np
import pytest
import torch

from oracle import model as om

from msheath_lens_ref import POINTS, msheath_lens

LENS = [200, 199, 1, 63, 64, 65, 128, 129]
B, L, D, LAYER = 8, 200, 128, 4
SEED, STEP, SITE, SID = 9, 1, "t.jump", 5


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.fixture(scope="module")
def setup():
    from asrx.model import MSheath

    torch.manual_seed(3)
    mod = MSheath(D, 2, LAYER)
    with torch.no_grad():
        for i in range(LAYER):
            mod.layers[i]["v_gate"].concat.bias.fill_(0.3 + 0.1 * (i - 1))
    trainable = {n for n, p in mod.named_parameters() if p.requires_grad}
    sd = {k: v.detach().double() for k, v in mod.state_dict().items()}
    x = torch.randn(B, L, D, generator=torch.Generator().manual_seed(11))
    x[1] *= 0.1
    gout = torch.randn(B, L, D, generator=torch.Generator().manual_seed(0))
    gpol = om.Noise(SEED, STEP, torch.float64).policy(SITE, [SID + b for b in range(B)], LAYER)

    def params():
        return {f"j.{k}": v.clone().requires_grad_(k in trainable) for k, v in sd.items()}

    # the oracle on every sample alone
    P = params()
    ys, dxs = [], []
    for b, t in enumerate(LENS):
        xa = x[b:b + 1, :t].double().requires_grad_(True)
        y = om.msheath(P, "j", xa, LAYER, gpol[b:b + 1])
        y.backward(gout[b:b + 1, :t].double())
        ys.append(y.detach())
        dxs.append(xa.grad)
    # the column sums of the last jump output of every sample alone (every row live)
    with torch.no_grad():
        cs = [msheath_lens(params(), "j", x[b:b + 1, :t].double(), LAYER, gpol[b:b + 1], [t])[1].sum(dim=1)
              for b, t in enumerate(LENS)]
    alone = (ys, dxs, {k: v.grad for k, v in P.items() if v.grad is not None}, cs)
    return x.double(), gout.double(), gpol, params, alone


def _padded(setup, points, pad_x=1.0e4, pad_g=float("nan")):
    x, gout, gpol, params, _ = setup
    x, gout = x.clone(), gout.clone()
    for b, t in enumerate(LENS):
        x[b, t:] = pad_x
        gout[b, t:] = pad_g
    P = params()
    xp = x.requires_grad_(True)
    y, xs = msheath_lens(P, "j", xp, LAYER, gpol, LENS, points)
    y.backward(gout)
    return y.detach(), xp.grad, {k: v.grad for k, v in P.items() if v.grad is not None}, xs.detach()


def _distance(setup, res):
    """largest relative distance of the padded result's live rows, parameter gradients and all-row column sums of the
    last jump output to the alone runs'"""
    ys, dxs, pg, cs = setup[4]
    y, dx, g, xs = res
    ds = []
    for b, t in enumerate(LENS):
        ds += [_rel(y[b, :t], ys[b][0]), _rel(dx[b, :t], dxs[b][0]), _rel(xs[b].sum(dim=0), cs[b][0])]
    assert g.keys() == pg.keys() and len(pg) > 40
    ds += [_rel(g[k], pg[k]) for k in pg]
    return float(torch.tensor(ds, dtype=torch.float64).max())  # (NaN propagates)


def test_all_mask_points_give_the_alone_runs(setup):
    res = _padded(setup, POINTS)
    assert _distance(setup, res) < 1e-12
    y, dx, _, xs = res
    for b, t in enumerate(LENS):
        assert not y[b, t:].any() and not dx[b, t:].any() and not xs[b, t:].any()
    assert bool(torch.isfinite(dx).all())


def test_pad_values_change_nothing(setup):
    a = _padded(setup, POINTS)
    b = _padded(setup, POINTS, pad_x=-3.0e3, pad_g=7.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(a[2][k], b[2][k]) for k in a[2])


@pytest.mark.parametrize("off", POINTS)
def test_each_mask_point_is_needed(setup, off):
    res = _padded(setup, tuple(p for p in POINTS if p != off))
    d = _distance(setup, res)
    assert not d < 1e-6, (off, d)  # (NaN from the cotangent's pad rows with yzero off)


def test_lengths_matter_for_the_gpu_test_inputs(setup):
    """At least one short sample's live rows differ from the unmasked computation on the same padded tensor: the damped
    sample 1 (potential below 0.1: forced to jump, gam carries the mem mean, which the sentinel row moves)."""
    masked = _padded(setup, POINTS, pad_g=0.0)[0]
    plain = _padded(setup, (), pad_g=0.0)[0]
    assert _rel(plain[1, :LENS[1]], masked[1, :LENS[1]]) > 1e-3
    assert torch.equal(plain[0], masked[0])


def test_reciprocal_identity():
    """float32(1.0 / L), what the uniform callers pass, equals float32(1) / float32(L), what the LENS kernels form on
    the device (a correctly rounded fp32 division), for every 1 <= L <= 65536."""
    n = np.arange(1, 65537)
    assert np.array_equal((1.0 / n.astype(np.float64)).astype(np.float32), np.float32(1) / n.astype(np.float32))
