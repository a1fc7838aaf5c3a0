"""The per-sample-length semantics of the encoder (tests/enc_lens_ref.py, the rule the LENS kernels follow), proved
in float64 on the CPU against oracle.model.encode_stream run on every sample alone:

1. live rows of the padded pass equal the alone run x[b:b+1, :, :T_b] with sid s*B + b, to 1e-12;
2. every parameter gradient equals the sum of the alone gradients, to 1e-12 of its largest entry;
3. the pad rows of every masked tensor and of the gradient of the layers' input are exactly zero, with NaN in the
   pad rows of the cotangent;
4. leaving out any one of the five mask points breaks (1).

Batch: lengths [T, 1, 5, 23] at T = 40 (full, a single row, shorter than the k15 halo, an interior end), D = 8,
2 layers, 4 mel channels, zero pad frames; the stream index is 1, so the sids are B + b.
"""
import pytest
import torch

import enc_lens_ref as R
from oracle import model as om

T, D, LAYERS, MELS, B, S = 40, 8, 2, 4, 4, 1
LENS = [T, 1, 5, 23]
SEED, STEP = 7, 3
TOL = 1e-12


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(1)
    P = R.params(MELS, D, LAYERS)
    x = torch.randn(B, MELS, T, generator=g, dtype=torch.float64)
    for b, n in enumerate(LENS):
        x[b, :, n:] = 0.0  # the collator's zero pad frames
    cot = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    noise = om.Noise(SEED, STEP, torch.float64)
    sids = [S * B + b for b in range(B)]
    names = sorted(P)
    # every sample alone
    alone, gsum = [], {n: torch.zeros_like(P[n]) for n in names}
    for b, n in enumerate(LENS):
        y = om.encode_stream(P, x[b:b + 1, :, :n], LAYERS, noise, [sids[b]], True)
        gs = torch.autograd.grad(y, [P[k] for k in names], cot[b:b + 1, :n])
        for k, gk in zip(names, gs):
            gsum[k] += gk
        alone.append(y.detach())
    return dict(P=P, x=x, cot=cot, noise=noise, sids=sids, names=names, alone=alone, gsum=gsum)


def _padded(c, skip=()):
    h = R.stem(c["P"], c["x"])
    y, masked = R.layers_padded(c["P"], h, LENS, LAYERS, c["noise"], c["sids"], skip)
    return h, y, masked


def _live_err(c, y):
    return max(float((y[b, :n] - c["alone"][b][0]).abs().max()) for b, n in enumerate(LENS))


def test_live_rows_equal_the_sample_alone(case):
    _, y, _ = _padded(case)
    assert _live_err(case, y.detach()) <= TOL
    for b, n in enumerate(LENS):  # pad rows: the positional table only
        assert torch.equal(y[b, n:].detach(), om.sinusoids(T, D, torch.float64)[n:])


def test_parameter_gradients_are_the_sum_of_the_alone_gradients(case):
    c = case
    h, y, _ = _padded(c)
    cot = c["cot"].clone()
    for b, n in enumerate(LENS):
        cot[b, n:] = float("nan")  # what the pad rows of the cotangent hold reaches nothing
    gs = torch.autograd.grad(y, [c["P"][k] for k in c["names"]] + [h], cot)
    for k, gk in zip(c["names"], gs):
        ref = c["gsum"][k]
        assert torch.isfinite(gk).all(), k
        assert float((gk - ref).abs().max()) <= TOL * max(1.0, float(ref.abs().max())), k
    gh = gs[-1]
    assert torch.isfinite(gh).all()
    for b, n in enumerate(LENS):  # the gradient of the layers' input on pad rows
        assert not gh[b, :, n:].any()
        assert gh[b, :, :n].any()


def test_pad_rows_of_every_masked_tensor_are_zero(case):
    _, _, masked = _padded(case)
    assert set(masked) == {"gelu0"} | {f"L{l}.{p}" for l in range(LAYERS) for p in ("k15", "k3", "tail")}
    for name, t in masked.items():
        for b, n in enumerate(LENS):
            assert not t[b, :, n:].any(), (name, b)
            assert t[b, :, :n].any(), (name, b)


@pytest.mark.parametrize("point", R.POINTS)
def test_every_mask_point_is_needed(case, point):
    """Without the mask point some short sample's live rows move by far more than rounding (the full-length sample
    never does)."""
    _, y, _ = _padded(case, skip=(point,))
    y = y.detach()
    err = _live_err(case, y)
    print(f"without {point}: live rows off by {err:.3e}")
    assert err > 1e-6
    assert float((y[0] - case["alone"][0][0]).abs().max()) <= TOL
