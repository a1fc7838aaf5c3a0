"""Pins tests/rowops_ref.py before a GPU is involved: every written-out backward against torch autograd of
its own forward in float64 (1e-12 relative), and the forwards against the torch.nn.functional ops they
restate."""
import pytest
import torch
import torch.nn.functional as F

import rowops_ref as R

TOL = 1e-12


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _close(a, b):
    scale = float(b.abs().max().clamp_min(1e-300))
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= TOL * scale, float((a - b).abs().max()) / scale


def _autograd(out, cot, inputs):
    return torch.autograd.grad(out, inputs, cot, allow_unused=True)


@pytest.mark.parametrize("name", R.ACTS)
@pytest.mark.parametrize("shape", [(7,), (3, 5)])
def test_act_bwd(name, shape):
    g = _g(len(shape))
    x = _rn(g, *shape).requires_grad_()
    cot = _rn(g, *shape)
    (dx,) = _autograd(R.act_fwd(x, name), cot, [x])
    _close(R.act_bwd(cot, x.detach(), name), dx)


@pytest.mark.parametrize("act,act2", [("gelu", "none"), ("relu", "none"), ("gelu", "relu"), ("relu", "gelu")])
@pytest.mark.parametrize("shape", [(1, 3, 4), (2, 5, 8)])
def test_act_dropout_bwd(act, act2, shape):
    g = _g(sum(shape))
    z = _rn(g, *shape).requires_grad_()
    keep = (torch.rand(*shape, generator=g) >= 0.3).double()
    cot = _rn(g, *shape)
    (dz,) = _autograd(R.act_dropout_fwd(z, keep, 0.1, act, act2), cot, [z])
    _close(R.act_dropout_bwd(cot, z.detach(), keep, 0.1, act, act2), dz)


@pytest.mark.parametrize("rows,C", [(1, 3), (5, 8)])
def test_glu_bwd(rows, C):
    g = _g(rows + C)
    x = _rn(g, rows, 2 * C).requires_grad_()
    cot = _rn(g, rows, C)
    (dx,) = _autograd(R.glu_fwd(x), cot, [x])
    _close(R.glu_bwd(cot, x.detach()), dx)
    _close(R.glu_fwd(x.detach()), F.glu(x.detach(), -1))


@pytest.mark.parametrize("rows,d", [(1, 4), (5, 6)])
def test_axpy_row_bwd(rows, d):
    g = _g(rows * d)
    x, y = _rn(g, rows, d).requires_grad_(), _rn(g, rows, d).requires_grad_()
    s, s2 = _rn(g, rows).requires_grad_(), _rn(g, rows).requires_grad_()
    cot = _rn(g, rows, d)
    dx, ds, dy = _autograd(R.axpy_row(x, s, y), cot, [x, s, y])
    rdy, rds, rdx = R.axpy_row_bwd(cot, s.detach(), y.detach())
    _close(rdy, dy), _close(rds, ds), _close(rdx, dx)
    ds1, ds2, dy = _autograd(R.axpy_row2(x, s, s2, y), cot, [s, s2, y])
    rdy, rds1, rds2 = R.axpy_row2_bwd(cot, s.detach(), s2.detach(), y.detach())
    _close(rdy, dy), _close(rds1, ds1), _close(rds2, ds2)
    ds1, dy = _autograd(R.axpy_row2(x, s, None, y), cot, [s, y])
    rdy, rds1, rds2 = R.axpy_row2_bwd(cot, s.detach(), None, y.detach())
    _close(rdy, dy), _close(rds1, ds1)
    assert rds2 is None


@pytest.mark.parametrize("B,L,d", [(1, 1, 4), (3, 5, 6)])
def test_seg_mean_bwd(B, L, d):
    g = _g(B * L * d)
    x = _rn(g, B, L, d).requires_grad_()
    cot = _rn(g, B, d)
    (dx,) = _autograd(R.seg_sum(x, 1.0 / L), cot, [x])
    _close(R.seg_mean_bwd(cot, L), dx)
    _close(R.seg_sum(x.detach(), 1.0 / L), x.detach().mean(1))


@pytest.mark.parametrize("V,d,n", [(3, 4, 5), (7, 6, 12)])
def test_embed_bwd(V, d, n):
    g = _g(V * d)
    E = _rn(g, V, d).requires_grad_()
    ids = torch.randint(0, V, (n,), generator=g)
    ids[:2] = ids[-1]  # repeats
    cot = _rn(g, n, d)
    (dE,) = _autograd(R.embed_fwd(ids, E), cot, [E])
    dE0 = _rn(g, V, d)
    _close(R.embed_bwd(ids, cot, dE0) - dE0, dE)
    _close(R.embed_fwd(ids, E.detach()), F.embedding(ids, E.detach()))


@pytest.mark.parametrize("B,T,D", [(1, 1, 3), (2, 1, 3), (3, 7, 5), (2, 2, 4)])
def test_stem1_bwd(B, T, D):
    g = _g(B * T * D)
    x = _rn(g, B, T)
    W, b = _rn(g, D, 3).requires_grad_(), _rn(g, D).requires_grad_()
    cot = _rn(g, B, T, D)
    y = R.stem1_fwd(x, W, b)
    dW, db = _autograd(y, cot, [W, b])
    dW0, db0 = _rn(g, D, 3), _rn(g, D)
    rdW, rdb = R.stem1_bwd(cot, x, dW0, db0)
    _close(rdW - dW0, dW), _close(rdb - db0, db)
    conv = F.conv1d(x[:, None, :], W.detach()[:, None, :], b.detach(), padding=1)  # (B, D, T)
    _close(y.detach(), conv.transpose(1, 2).contiguous())


@pytest.mark.parametrize("rows,d", [(1, 6), (5, 16)])
def test_layernorm_bwd(rows, d):
    g = _g(rows * d)
    x = (_rn(g, rows, d) * 2 + 1).requires_grad_()
    w, b = _rn(g, d).requires_grad_(), _rn(g, d).requires_grad_()
    cot = _rn(g, rows, d)
    y, mean, rstd = R.layernorm_fwd(x, w, b, 1e-5)
    dx, dw, db = _autograd(y, cot, [x, w, b])
    dx0, dw0, db0 = _rn(g, rows, d), _rn(g, d), _rn(g, d)
    rdx, rdw, rdb = R.layernorm_bwd(cot, x.detach(), w.detach(), mean.detach(), rstd.detach(), dx0, dw0, db0)
    _close(rdx - dx0, dx), _close(rdw - dw0, dw), _close(rdb - db0, db)
    rdx, _, _ = R.layernorm_bwd(cot, x.detach(), w.detach(), mean.detach(), rstd.detach(), None, dw0, db0)
    _close(rdx, dx)
    _close(y.detach(), F.layer_norm(x.detach(), (d,), w.detach(), b.detach(), 1e-5))
    gw, gb = _rn(g, d), _rn(g, 1)
    for on_x in (0, 1):
        nrm, gate = R.layernorm_row_outputs(x.detach(), y.detach(), gw, gb, on_x)
        _close(nrm, x.detach().norm(dim=-1))
        _close(gate, torch.sigmoid(F.linear(x.detach() if on_x else y.detach(), gw[None], gb))[:, 0])


@pytest.mark.parametrize("B,L,d", [(1, 1, 4), (3, 5, 6)])
def test_jump_select_bwd(B, L, d):
    g = _g(B + L + d)
    xn, orig, xold = (_rn(g, B, L, d).requires_grad_() for _ in range(3))
    alpha, beta = _rn(g, B).requires_grad_(), _rn(g, B).requires_grad_()
    gam = _rn(g, B, d).requires_grad_()
    act = torch.tensor([1.0, 0.0, 1.0][:B], dtype=torch.float64)
    cot = _rn(g, B, L, d)
    out = R.jump_select(xn, orig, xold, act, alpha, beta, gam)
    want = _autograd(out, cot, [xn, orig, xold, alpha, beta, gam])
    got = R.jump_select_bwd(cot, xn.detach(), orig.detach(), act, alpha.detach(), beta.detach())
    for a, c in zip(got, want):
        _close(a, c)
    # a sample that is not at the layer contributes nothing but the pass-through
    if B > 1:
        assert all(float(t[1].abs().max()) == 0.0 for t in got[:2] + got[3:])
        assert torch.equal(got[2][1], cot[1])
    s1, s2 = _rn(g, B, L), _rn(g, B, L)
    y = _rn(g, B, L, d)
    xo = R.jump_axpy(xold.detach(), s1, s2, y, orig.detach(), act, alpha.detach(), beta.detach(), gam.detach())
    for b in range(B):
        if act[b] == 0:
            assert torch.equal(xo[b], xold[b].detach())
        else:
            u = xold[b].detach() + (s1[b] * s2[b])[:, None] * y[b]
            _close(xo[b], alpha[b].detach() * u + beta[b].detach() * orig[b].detach() + gam[b].detach())


def test_forwards_match_torch_functional():
    g = _g(0)
    x = _rn(g, 4, 9) * 3
    _close(R.act_fwd(x, "gelu"), F.gelu(x))
    _close(R.act_fwd(x, "silu"), F.silu(x))
    _close(R.act_fwd(x, "sigmoid"), torch.sigmoid(x))
    _close(R.act_fwd(x, "relu"), F.relu(x))
    assert torch.equal(R.act_fwd(x, "none"), x)
    y, z = _rn(g, 4, 9), _rn(g, 4, 9)
    _close(R.lincomb(x, y, z, 2.0, -1.0, 0.5), 2.0 * x - y + 0.5 * z)
    _close(R.lincomb(x, None, None, 2.0, 9.0, 9.0), 2.0 * x)
    t, u = _rn(g, 7, 9), _rn(g, 2, 9)
    x3 = _rn(g, 2, 5, 9)
    _close(R.add_rows(x3, t, u, 2, 5, 9), x3 + t[None, :5] + u[:, None])
    _close(R.add_rows(None, None, u, 2, 5, 9), u[:, None].expand(2, 5, 9))
    _close(R.colsum(x, y[0]), y[0] + x.sum(0))
