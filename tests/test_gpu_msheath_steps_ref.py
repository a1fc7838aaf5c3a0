"""MSheath step kernels of csrc/msheath.hip (asrx_axpy_row2*, asrx_jump_select*, asrx_jump_axpy_inplace) and the
scalar asrx_jump_select / _bwd of csrc/rowops.hip against the float64 references of tests/rowops_ref.py, in the
three tiers of tests/ref_check.py.  The per-sample `act` is mixed 0 / 1, one active sample has beta = 0, and alpha,
beta, gam are integer-valued in the exact tier.  These are the base kernels that tests/test_gpu_msheath_bwd_fused.py
trusts when it checks the _acc / _part variants.

Tier B figures measured on an MI355X when these tests were added (worst e / bound over the cases of each row;
e and e32 are relative to the largest entry of the float64 reference, bound = max(floor, 20 e32)):

    kernel [output]                  cases   e         e32       bound
    axpy_row2                            2   5.4e-08   5.4e-08   1.1e-06
    axpy_row2_bwd [dy]                   2   3.9e-08   3.9e-08   7.7e-07
    axpy_row2_bwd [ds1]                  2   2.6e-07   2.6e-07   5.1e-06
    axpy_row2_bwd [ds2]                  2   2.2e-07   2.2e-07   4.4e-06
    axpy_row2_colsum [x_new]             2   3.8e-08   4.4e-08   8.8e-07
    axpy_row2_colsum [sum of parts]      2   4.1e-07   1.5e-07   4.1e-06
    jump_select4                         2   2.9e-08   4.6e-08   9.1e-07
    jump_select4_bwd [dxn]               2   5.1e-08   5.1e-08   1.0e-06
    jump_select4_bwd [dorig]             2   3.5e-08   3.5e-08   7.1e-07
    jump_select4_bwd [dxold]             2   0         0         6.0e-08
    jump_select4_bwd [dalpha]            2   6.8e-07   1.2e-05   2.4e-04
    jump_select4_bwd [dbeta]             2   2.1e-07   1.0e-07   8.7e-06
    jump_select4_bwd [dgam]              2   1.5e-07   9.7e-08   1.9e-06
    JumpSelect fwd (d = 6, 100, 102)     3   4.1e-08   4.1e-08   8.2e-07
    JumpSelect bwd [dxn / dorig]         3   4.2e-08 / 2.9e-08   (e32 the same)   8.4e-07 / 5.8e-07
    JumpSelect bwd [dalpha]              3   9.7e-08   8.1e-08   1.9e-06
    JumpSelect bwd [dbeta]               3   8.9e-08   1.3e-07   2.6e-06
    JumpSelect bwd [dgam]                3   8.9e-08   8.5e-08   1.7e-06
    jump_axpy_inplace                    6   3.7e-08   3.8e-08   7.7e-07

The second backward of JumpSelect gave the same figures.  The bit-identity claim of jump_axpy_inplace_kernel held: it
equals axpy_row2_colsum followed by jump_select4 on every element.
"""
import math

import pytest
import torch

import rowops_ref as R
from ref_check import SENTINEL, dev, exact, f32, gen, ints, ops_floor, randn, sentinel, tier_b
from ref_check import call as _call

pytestmark = pytest.mark.gpu

BL = ((1, 1), (3, 30), (2, 65), (2, 130))


def _chunks(L):
    from asrx import lib

    return int(lib.load().asrx_mem_chunks(L))


def _act(B):
    return torch.tensor([1.0, 0.0, 1.0][:B], dtype=torch.float64)


def _coef(g, B, d, integer):
    """alpha, beta, gam; the first (active) sample keeps, i.e. beta = 0."""
    if integer:
        alpha, beta, gam = ints(g, B, lo=-2, hi=2), ints(g, B, lo=1, hi=2), ints(g, B, d)
    else:
        alpha, beta, gam = randn(g, B), randn(g, B), randn(g, B, d)
    beta[0] = 0.0
    return alpha, beta, gam


# =========================================================================================== axpy_row2
@pytest.mark.parametrize("d", [4, 132, 384, 1024])
def test_axpy_row2_exact(cuda, d):
    for B, L in BL:
        rows = B * L
        g = gen(d + rows)
        x, y, cot = ints(g, rows, d), ints(g, rows, d), ints(g, rows, d)
        s1, s2 = ints(g, rows, lo=-2, hi=2), ints(g, rows, lo=-2, hi=2)
        one = torch.ones(rows, dtype=torch.float64)
        assert 2 * 9 * d < 2 ** 24 and 15 * L < 2 ** 24  # |ds| <= 2 * 3 * 3 * d, |sum_l x_new| <= (3 + 4 * 3) L
        for s2v in (None, s2):
            out = sentinel(rows, d)
            _call("asrx_axpy_row2", dev(x), dev(s1), dev(s2v), dev(y), out, rows, d)
            exact(f"axpy_row2 d={d} {B}x{L} s2={s2v is not None}", out, R.axpy_row2(x, s1, s2v, y))
            rdy, rds1, rds2 = R.axpy_row2_bwd(cot, s1, one if s2v is None else s2v, y)
            for want_ds2 in (False, True):
                dy, ds1 = sentinel(rows, d), sentinel(rows)
                ds2 = sentinel(rows) if want_ds2 else None
                _call("asrx_axpy_row2_bwd", dev(cot), dev(s1), dev(s2v), dev(y), dy, ds1, ds2,
                      rows, d)
                exact("axpy_row2_bwd dy", dy, rdy)
                exact("axpy_row2_bwd ds1", ds1, rds1)
                if want_ds2:
                    exact("axpy_row2_bwd ds2", ds2, rds2)
        # x_new and its per-sample column sums in one pass; next_i marks the samples at the layer
        xn = R.axpy_row2(x, s1, s2, y).view(B, L, d)
        nch = _chunks(L)
        for next_i in (None, torch.tensor([2.0, 1.0, 2.0][:B])):
            out, part = sentinel(B, L, d), sentinel(B, nch, d)
            _call("asrx_axpy_row2_colsum", dev(x), dev(s1), dev(s2), dev(y), out, part, B, L, d,
                  dev(next_i), 2)
            at = torch.ones(B, dtype=torch.bool) if next_i is None else next_i == 2.0
            want = torch.where(at[:, None, None], xn, torch.full_like(xn, SENTINEL))  # others: x_new not written
            exact(f"axpy_row2_colsum out d={d} {B}x{L}", out, want)
            chunks = torch.stack([xn[:, c * 64:(c + 1) * 64].sum(1) for c in range(nch)], 1) * at[:, None, None]
            exact(f"axpy_row2_colsum part d={d} {B}x{L}", part, chunks)
            exact("axpy_row2_colsum sum of parts", part.sum(1), xn.mean(1) * L * at[:, None])


def test_axpy_row2_bwd_wrapped_rows(cuda):
    """rows = 32773 at d = 4: past the backward's 8192 x 4 row grid cap."""
    rows, d = 32773, 4
    g = gen(1)
    y, cot = ints(g, rows, d), ints(g, rows, d)
    s1, s2 = ints(g, rows, lo=-2, hi=2), ints(g, rows, lo=-2, hi=2)
    dy, ds1, ds2 = sentinel(rows, d), sentinel(rows), sentinel(rows)
    _call("asrx_axpy_row2_bwd", dev(cot), dev(s1), dev(s2), dev(y), dy, ds1, ds2, rows, d)
    for name, got, want in zip(("dy", "ds1", "ds2"), (dy, ds1, ds2), R.axpy_row2_bwd(cot, s1, s2, y)):
        exact(f"axpy_row2_bwd rows=32773 {name}", got, want)


@pytest.mark.parametrize("B,L,d", [(3, 30, 132), (2, 130, 1024)])
def test_axpy_row2_real(cuda, B, L, d):
    rows = B * L
    g = gen(B + L + d)
    x, y, cot = randn(g, rows, d), randn(g, rows, d), randn(g, rows, d)
    y[0] *= 40
    y = f32(y)
    s1, s2 = f32(randn(g, rows) + 0.5), f32((torch.rand(rows, generator=g) > 0.3).double())
    out = sentinel(rows, d)
    _call("asrx_axpy_row2", dev(x), dev(s1), dev(s2), dev(y), out, rows, d)
    tier_b(f"axpy_row2 {B}x{L}x{d}", out, R.axpy_row2, (x, s1, s2, y), ops_floor(3))  # s1 s2, product, sum
    dy, ds1, ds2 = sentinel(rows, d), sentinel(rows), sentinel(rows)
    _call("asrx_axpy_row2_bwd", dev(cot), dev(s1), dev(s2), dev(y), dy, ds1, ds2, rows, d)
    # t: per lane ceil(d4 / 64) trips of four products and four sums, a six-level wave sum, then one product
    kt = 5 * math.ceil(d / 4 / 64) + 6 + 2
    tier_b(f"axpy_row2_bwd {B}x{L}x{d}", (dy, ds1, ds2), R.axpy_row2_bwd, (cot, s1, s2, y),
           (ops_floor(2), ops_floor(kt), ops_floor(kt)), names=("dy", "ds1", "ds2"))
    nch = _chunks(L)
    out2, part = sentinel(B, L, d), sentinel(B, nch, d)
    _call("asrx_axpy_row2_colsum", dev(x), dev(s1), dev(s2), dev(y), out2, part, B, L, d, None, 0)
    tier_b(f"axpy_row2_colsum {B}x{L}x{d}", out2.view(rows, d), R.axpy_row2, (x, s1, s2, y), ops_floor(2))
    # a row lane adds 64 / nrl rows, nrl lanes are joined in order; the chunks are added here in float64
    nrl = 256 // (d // 4)
    kp = 2 + math.ceil(64 / nrl) + nrl
    tier_b(f"axpy_row2_colsum part {B}x{L}x{d}", part.double().sum(1),
           lambda *a: R.axpy_row2(*a).view(B, L, d).mean(1) * L, (x, s1, s2, y), ops_floor(kp))


# =========================================================================================== jump_select4
def _jump_fwd(entry, xn, orig, xold, act, alpha, beta, gam):
    B, L, d = xn.shape
    out = sentinel(B, L, d)
    _call(entry, dev(xn), dev(orig), dev(xold), dev(act), dev(alpha), dev(beta), dev(gam),
          out, B, L, d)
    return out


def _jump_bwd(entry, cot, xn, orig, act, alpha, beta):
    B, L, d = xn.shape
    dxn, dorig, dxold = sentinel(B, L, d), sentinel(B, L, d), sentinel(B, L, d)
    dalpha, dbeta, dgam = sentinel(B), sentinel(B), sentinel(B, d)  # the launcher zeroes its accumulators
    _call(entry, dev(cot), dev(xn), dev(orig), dev(act), dev(alpha), dev(beta), dxn, dorig,
          dxold, dalpha, dbeta, dgam, B, L, d)
    return dxn, dorig, dxold, dalpha, dbeta, dgam


JUMP_NAMES = ("dxn", "dorig", "dxold", "dalpha", "dbeta", "dgam")


@pytest.mark.parametrize("d", [4, 132, 1024])  # d = 132: d4 = 33, the second column chunk holds one column
@pytest.mark.parametrize("B", [1, 3])
def test_jump_select4_exact(cuda, d, B):
    for L in (1, 127, 128, 129):
        g = gen(d + L + B)
        xn, orig, xold, cot = (ints(g, B, L, d) for _ in range(4))
        act = _act(B)
        alpha, beta, gam = _coef(g, B, d, True)
        assert 9 * L * d < 2 ** 24  # |dalpha|, |dbeta| <= 3 * 3 * L * d
        out = _jump_fwd("asrx_jump_select4", xn, orig, xold, act, alpha, beta, gam)
        exact(f"jump_select4 {B}x{L}x{d}", out, R.jump_select(xn, orig, xold, act, alpha, beta, gam))
        got = _jump_bwd("asrx_jump_select4_bwd", cot, xn, orig, act, alpha, beta)
        for name, a, w in zip(JUMP_NAMES, got, R.jump_select_bwd(cot, xn, orig, act, alpha, beta)):
            exact(f"jump_select4_bwd {name} {B}x{L}x{d}", a, w)
        for b in range(B):
            if act[b] == 0:  # a sample that is not at the layer: the pass-through and exact zeros
                assert all(float(t[b].abs().max()) == 0.0 for t in got[:2] + got[3:])
                assert torch.equal(got[2][b].cpu(), cot[b].float())


def test_jump_select4_grid_stride(cuda):
    """L d / 4 > 512 x 256: the forward's grid-stride loop takes a second trip."""
    B, L, d = 2, 600, 1024
    g = gen(2)
    xn, orig, xold = (ints(g, B, L, d) for _ in range(3))
    act = _act(B)
    alpha, beta, gam = _coef(g, B, d, True)
    beta[0] = 2.0
    out = _jump_fwd("asrx_jump_select4", xn, orig, xold, act, alpha, beta, gam)
    exact("jump_select4 grid-stride", out, R.jump_select(xn, orig, xold, act, alpha, beta, gam))


@pytest.mark.parametrize("B,L,d", [(3, 129, 132), (3, 127, 1024)])
def test_jump_select4_real(cuda, B, L, d):
    g = gen(B * L + d)
    xn, orig, xold, cot = (randn(g, B, L, d) for _ in range(4))
    xn[0, 0] *= 40
    xn = f32(xn)
    act = _act(B)
    alpha, beta, gam = _coef(g, B, d, False)
    out = _jump_fwd("asrx_jump_select4", xn, orig, xold, act, alpha, beta, gam)
    tier_b(f"jump_select4 {B}x{L}x{d}", out, R.jump_select, (xn, orig, xold, act, alpha, beta, gam),
           ops_floor(2))  # two fused multiply-adds
    got = _jump_bwd("asrx_jump_select4_bwd", cot, xn, orig, act, alpha, beta)
    # dalpha / dbeta: per thread min(L, 128) / 8 trips of four products and four sums, a six-level wave sum,
    # three sums across the waves, one atomic per workgroup; dgam: the trips, eight row groups, one atomic per L chunk
    trips, nblk = math.ceil(min(L, 128) / 8), math.ceil(d / 4 / 32) * math.ceil(L / 128)
    ka, kg = 8 * trips + 6 + 3 + nblk, trips + 8 + math.ceil(L / 128)
    tier_b(f"jump_select4_bwd {B}x{L}x{d}", got, R.jump_select_bwd, (cot, xn, orig, act, alpha, beta),
           (ops_floor(1), ops_floor(1), ops_floor(0), ops_floor(ka), ops_floor(ka), ops_floor(kg)), names=JUMP_NAMES)


# =========================================================================================== ops.JumpSelect, d % 4 != 0
@pytest.mark.parametrize("d", [6, 100, 102])
def test_jump_select_autograd(cuda, d):
    """ops.JumpSelect: d = 6 and 102 (two 64-column workgroups) take the scalar entries, whose accumulators the
    backward zeroes before the kernel adds into them, so a second backward returns the same gradients; d = 100
    is a multiple of four and takes the float4 entries through the same autograd function."""
    from asrx import ops

    B, L = 3, 37
    g = gen(d)
    act = _act(B)
    for integer in (True, False):
        mk = ints if integer else randn
        xn, orig, xold, cot = (mk(g, B, L, d) for _ in range(4))
        alpha, beta, gam = _coef(g, B, d, integer)
        leaves = [dev(t).requires_grad_() for t in (xn, orig, xold, alpha, beta, gam)]
        out = ops.JumpSelect.apply(leaves[0], leaves[1], leaves[2], dev(act), *leaves[3:])
        g1 = torch.autograd.grad(out, leaves, dev(cot), retain_graph=True)
        g2 = torch.autograd.grad(out, leaves, dev(cot))
        got = (g1[0], g1[1], g1[2], g1[3], g1[4], g1[5])
        ref_out = R.jump_select(xn, orig, xold, act, alpha, beta, gam)
        if integer:
            exact(f"jump_select d={d}", out, ref_out)
            for name, a, w in zip(JUMP_NAMES, got, R.jump_select_bwd(cot, xn, orig, act, alpha, beta)):
                exact(f"jump_select_bwd {name} d={d}", a, w)
            assert all(torch.equal(a, b) for a, b in zip(g1, g2))
        else:
            tier_b(f"jump_select d={d}", out, R.jump_select, (xn, orig, xold, act, alpha, beta, gam), ops_floor(4))
            # a thread adds L / 4 rows of its column, four sums join the waves, then one atomic per column
            ka, kg = 2 * math.ceil(L / 4) + 4 + d, math.ceil(L / 4) + 4
            fl = (ops_floor(1), ops_floor(1), ops_floor(0), ops_floor(ka), ops_floor(ka), ops_floor(kg))
            tier_b(f"jump_select_bwd d={d}", got, R.jump_select_bwd, (cot, xn, orig, act, alpha, beta), fl,
                   names=JUMP_NAMES)
            tier_b(f"jump_select_bwd again d={d}", g2, R.jump_select_bwd, (cot, xn, orig, act, alpha, beta), fl,
                   names=JUMP_NAMES)


# =========================================================================================== jump_axpy_inplace
def _jump_axpy(xio, xout, s1, s2, y, orig, act, alpha, beta, gam):
    B, L, d = y.shape
    _call("asrx_jump_axpy_inplace", xio, xout, dev(s1), dev(s2), dev(y), dev(orig), dev(act),
          dev(alpha), dev(beta), dev(gam), B, L, d)


@pytest.mark.parametrize("d", [4, 132, 1024])
@pytest.mark.parametrize("integer", [True, False])
def test_jump_axpy_inplace(cuda, d, integer):
    for B, L in ((3, 30), (2, 130)):
        g = gen(d + L + integer)
        mk = ints if integer else randn
        xin, y, orig = (mk(g, B, L, d) for _ in range(3))
        s1 = ints(g, B, L, lo=-2, hi=2) if integer else f32(randn(g, B, L) + 0.5)
        s2 = ints(g, B, L, lo=-2, hi=2) if integer else f32((torch.rand(B, L, generator=g) > 0.3).double())
        act = _act(B)
        alpha, beta, gam = _coef(g, B, d, integer)
        ref = R.jump_axpy(xin, s1, s2, y, orig, act, alpha, beta, gam)
        xio = dev(xin)  # in place: samples not at the layer are not touched
        _jump_axpy(xio, xio, s1, s2, y, orig, act, alpha, beta, gam)
        xsrc, xout = dev(xin), sentinel(B, L, d)  # out of place: they are copied
        _jump_axpy(xsrc, xout, s1, s2, y, orig, act, alpha, beta, gam)
        assert torch.equal(xsrc.cpu(), xin.float())
        assert torch.equal(xio, xout)
        for b in range(B):
            if act[b] == 0:
                assert torch.equal(xout[b].cpu(), xin[b].float())
        if integer:
            exact(f"jump_axpy_inplace {B}x{L}x{d}", xout, ref)
            continue
        tier_b(f"jump_axpy_inplace {B}x{L}x{d}", xout, R.jump_axpy, (xin, s1, s2, y, orig, act, alpha, beta, gam),
               ops_floor(4))  # s1 s2 and three fused multiply-adds
        # tier C: the same bits as axpy_row2_colsum followed by jump_select4
        xn, part = sentinel(B, L, d), sentinel(B, _chunks(L), d)
        _call("asrx_axpy_row2_colsum", dev(xin), dev(s1), dev(s2), dev(y), xn, part, B, L, d,
              None, 0)
        two = sentinel(B, L, d)
        _call("asrx_jump_select4", xn, dev(orig), dev(xin), dev(act), dev(alpha), dev(beta),
              dev(gam), two, B, L, d)
        assert torch.equal(xout, two)
