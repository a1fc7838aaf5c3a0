"""Row and elementwise kernels of csrc/rowops.hip against the float64 references of tests/rowops_ref.py, kernel by
kernel, in the three tiers of tests/ref_check.py: exact on small-integer data (every element, sentinel-filled
outputs), real inputs within max(floor, 20 x e32), and torch.equal between the float4 and the scalar form (forced
by a view that starts one float into its buffer) where the source claims bit-identity.

Tier B figures measured on an MI355X when these tests were added (worst e / bound over the cases of each row;
e and e32 are relative to the largest entry of the float64 reference, bound = max(floor, 20 e32)):

    kernel [output]                  cases   e         e32       bound
    lincomb                              1   9.7e-08   9.7e-08   1.9e-06
    act gelu    fwd / bwd               14   5.0e-08 / 3.3e-07   (e32 the same)   1e-05 / 1e-04
    act silu    fwd / bwd               14   9.0e-08 / 1.5e-07   1.8e-08 / 1.5e-07   1e-05 / 1e-04
    act sigmoid fwd / bwd               14   9.7e-08 / 6.6e-07   8.2e-08 / 6.6e-07   1e-05 / 1e-04
    act gelu fwd / bwd, 25.2 M           1   4.2e-08 / 1.2e-07   4.2e-08 / 1.1e-07   1e-05 / 1e-04
    add_rows                             1   9.1e-08   9.1e-08   1.8e-06
    axpy_row                             2   5.1e-08   5.1e-08   1.0e-06
    axpy_row_bwd [dy]                    2   4.2e-08   4.2e-08   8.5e-07
    axpy_row_bwd [ds]                    2   5.8e-08   5.8e-08   1.2e-06
    seg_mean fwd                         5   1.1e-07   8.6e-08   1.7e-06
    seg_mean bwd                         5   5.5e-08   5.5e-08   1.1e-06
    colsum_ld                            6   1.1e-07   1.1e-07   2.2e-06
    Embedding bwd                        2   5.6e-09   6.0e-09   6.0e-07
    stem1_fwd                           16   6.4e-08   6.4e-08   1.3e-06
    stem1_bwd [dW]                      16   5.0e-08   5.0e-08   1.0e-06
    stem1_bwd [db]                      16   1.1e-07   3.9e-08   7.8e-07
    glu fwd / bwd                        6   5.6e-08 / 4.9e-07   (e32 the same)   1e-05 / 1e-04
    layernorm_fwd [y]                   41   8.4e-07   1.4e-07   3.2e-06
    layernorm_fwd [mean]                41   5.7e-08   4.3e-09   6.0e-07
    layernorm_fwd [rstd]                41   7.3e-08   7.3e-08   1.5e-06
    layernorm_fwd3 [y]                  24   1.1e-06   7.1e-08   2.7e-06
    layernorm_fwd3 [nrm]                24   3.8e-08   3.8e-08   7.7e-07
    layernorm_fwd3 [gate on y / on x]   24   8.4e-07 / 5.3e-07   6.7e-07 / 5.0e-07   1.3e-05 / 1.0e-05
    layernorm_bwd(_acc) [dx]           122   1.8e-07   1.8e-07   3.7e-06
    layernorm_bwd(_acc) [dw]           122   2.7e-07   7.9e-08   1.6e-06
    layernorm_bwd(_acc) [db]           122   1.6e-07   5.5e-08   1.1e-06
    layernorm, x one float offset        1   y 7.0e-07, dx 1.1e-07, dw 7.2e-08, db 1.0e-07 (bounds 1.5e-05 .. 1.1e-06)
    linear relu, fp32 [y/dx/dW/db]       1   0 / 1.9e-07 / 1.4e-07 / 1.1e-07   (fixed bounds 1e-05 / 1e-04)
    act_dropout with relu fwd / bwd      4   1.1e-07 / 1.5e-07   1.1e-07 / 1.3e-07   1e-05 / 1e-04

The largest e / bound is 0.40 (layernorm_fwd3 y at d = 768, one row).  Every bit-identity claim of the source held:
the float4 forms of lincomb, act_fwd, act_bwd, add_rows and axpy_row equal their scalar forms, and
ln_fwd_t_kernel's bf16 output equals the round-to-nearest-even of its fp32 output.
"""
import math

import pytest
import torch

import rowops_ref as R
from ref_check import BWD_TRANS, FWD_TRANS, SENTINEL, dev, dev_offset, exact, f32, gen, ints, ops_floor, randn, rel
from ref_check import call as _call
from ref_check import sentinel, tier_b

pytestmark = pytest.mark.gpu

N_VEC = (4, 8, 12, 2052)  # n4 = 1, 2, 3 and one size over two workgroups
N_SCALAR = (1, 7, 2051)  # n % 4 != 0: the scalar form
N4_BIG = 3 * 8192 * 256 + 4 * 256 + 3  # first float4 count with a second loop trip and a tail behind the 8192 cap
ROW_SHAPES = [(r, d) for r in (1, 5, 33) for d in (4, 6, 100, 384)]


@pytest.fixture(autouse=True)
def _fp32():
    from asrx import prec

    with prec.precision("fp32"):
        yield


def _mk(off):
    return dev_offset if off else dev


def _outlier(t, dim0=0):
    """One row (or, for a vector, one element past the first) scaled by 40; fp32-exact."""
    t = t.clone()
    if t.dim() == 1:
        if t.numel() >= 8:
            t[t.numel() // 2] *= 40
    else:
        t[dim0] *= 40
    return f32(t)


# =========================================================================================== lincomb
def _lincomb(x, y, z, a, b, c, out):
    _call("asrx_lincomb", x, y, z, float(a), float(b), float(c), out, x.numel())


@pytest.mark.parametrize("n", N_VEC + N_SCALAR)
def test_lincomb_exact(cuda, n):
    g = gen(n)
    for has_y, has_z in ((0, 0), (1, 0), (0, 1), (1, 1)):
        x, y, z = ints(g, n), (ints(g, n) if has_y else None), (ints(g, n) if has_z else None)
        a, b, c = (float(v) for v in ints(g, 3, lo=-2, hi=2))
        ref = R.lincomb(x, y, z, a, b, c)
        for off in (False, True):
            out = sentinel(n, offset=off)
            _lincomb(_mk(off)(x), _mk(off)(y), _mk(off)(z), a, b, c, out)
            exact(f"lincomb n={n} y={has_y} z={has_z} off={off}", out, ref)
        out = sentinel(n)  # one misaligned operand among aligned ones
        _lincomb(dev_offset(x), dev(y), dev(z), a, b, c, out)
        exact(f"lincomb n={n} x offset", out, ref)


def test_lincomb_real_and_paths(cuda):
    n = 2052
    g = gen(1)
    x, y, z = _outlier(randn(g, n)), randn(g, n), f32(randn(g, n) + 3)
    a, b, c = 1.7, -0.3, 0.9
    a, b, c = (float(torch.tensor(v, dtype=torch.float32)) for v in (a, b, c))
    out, out_s = sentinel(n), sentinel(n, offset=True)
    _lincomb(dev(x), dev(y), dev(z), a, b, c, out)
    _lincomb(dev_offset(x), dev_offset(y), dev_offset(z), a, b, c, out_s)
    assert torch.equal(out, out_s)  # tier C: lincomb4_kernel == lincomb_kernel
    # three products and two sums round into each element
    tier_b("lincomb", out, R.lincomb, (x, y, z, a, b, c), ops_floor(5))


def test_lincomb_large(cuda):
    n = 4 * N4_BIG
    g = torch.Generator(device="cuda").manual_seed(2)
    x, y, z = (torch.randint(-3, 4, (n,), generator=g, device="cuda", dtype=torch.float32) for _ in range(3))
    out = torch.full((n,), SENTINEL, device="cuda")
    _lincomb(x, y, z, 2.0, -1.0, -2.0, out)
    ref = 2.0 * x.double() - y.double() - 2.0 * z.double()
    assert float(ref.abs().max()) < 2 ** 24
    assert torch.equal(out, ref.float())


# =========================================================================================== activations
def _act_fwd(x, y, name):
    from asrx.gemm import ACT

    _call("asrx_act_fwd", x, y, x.numel(), ACT[name])


def _act_bwd(g, x, dx, name):
    from asrx.gemm import ACT

    _call("asrx_act_bwd", g, x, dx, x.numel(), ACT[name])


def _act_input(g, n):
    x = randn(g, n) * 2
    x[x == 0] = 1.0
    return _outlier(x)


@pytest.mark.parametrize("name", R.ACTS)
def test_act_fwd_bwd(cuda, name):
    """All five activations, forward and derivative; `none` and `relu` are exact (a copy, a select, a product
    with 0 or 1), the others use __expf / erff / v_rcp (the project's 1e-5 / 1e-4 floors)."""
    g = gen(len(name))
    for n in N_VEC + N_SCALAR:
        x, cot = _act_input(g, n), randn(g, n)
        for off in (False, True):
            y, dx = sentinel(n, offset=off), sentinel(n, offset=off)
            _act_fwd(_mk(off)(x), y, name)
            _act_bwd(_mk(off)(cot), _mk(off)(x), dx, name)
            tag = f"act.{name} n={n} off={int(off)}"
            if name in ("none", "relu"):
                exact(tag + " fwd", y, R.act_fwd(x, name))
                exact(tag + " bwd", dx, R.act_bwd(cot, x, name))
            else:
                tier_b(tag + " fwd", y, R.act_fwd, (x, name), FWD_TRANS)
                tier_b(tag + " bwd", dx, R.act_bwd, (cot, x, name), BWD_TRANS)


@pytest.mark.parametrize("name", R.ACTS)
def test_act_vec_equals_scalar(cuda, name):
    """Tier C: act_fwd4 / act_bwd4 against act_fwd / act_bwd."""
    n = 2052
    g = gen(7)
    x, cot = _act_input(g, n), randn(g, n)
    y, dx, ys, dxs = sentinel(n), sentinel(n), sentinel(n, offset=True), sentinel(n, offset=True)
    _act_fwd(dev(x), y, name)
    _act_fwd(dev_offset(x), ys, name)
    _act_bwd(dev(cot), dev(x), dx, name)
    _act_bwd(dev_offset(cot), dev_offset(x), dxs, name)
    assert torch.equal(y, ys)
    assert torch.equal(dx, dxs)


def _device_tier_b(name, got, fn, args, floor):
    """tier_b with the float64 and the float32 evaluation of the reference on the device (the 25 M-element
    cases only)."""
    ref = fn(*[a.double() if torch.is_tensor(a) else a for a in args])
    r32 = fn(*args)
    scale = ref.abs().max()
    e = float((got.double() - ref).abs().max() / scale)
    e32 = float((r32.double() - ref).abs().max() / scale)
    bound = max(floor, 20 * e32)
    print(f"TIERB {name:<44s} e={e:.2e} e32={e32:.2e} bound={bound:.2e}")
    assert e <= bound, (name, e, e32, bound)


def test_act_fwd_large(cuda):
    n = 4 * N4_BIG
    x = torch.randn(n, generator=torch.Generator(device="cuda").manual_seed(3), device="cuda") * 2
    y = torch.full((n,), SENTINEL, device="cuda")
    _act_fwd(x, y, "gelu")
    _device_tier_b("act.gelu fwd large", y, R.act_fwd, (x, "gelu"), FWD_TRANS)


def test_act_bwd_large(cuda):
    n = 4 * N4_BIG
    g = torch.Generator(device="cuda").manual_seed(4)
    x = torch.randn(n, generator=g, device="cuda") * 2
    cot = torch.randn(n, generator=g, device="cuda")
    dx = torch.full((n,), SENTINEL, device="cuda")
    _act_bwd(cot, x, dx, "gelu")
    _device_tier_b("act.gelu bwd large", dx, R.act_bwd, (cot, x, "gelu"), BWD_TRANS)


# =========================================================================================== add_rows
def _add_rows(x, t, u, out, B, L, d):
    _call("asrx_add_rows", x, t, u, out, B, L, d)


ADD_SHAPES = sorted({(1, 1, n) for n in N_VEC + N_SCALAR} | {(1, 3, 4), (3, 171, 4)} |
                    {(B, L, d) for B, L in ((1, 1), (3, 5), (2, 33)) for d in (4, 6, 100, 384)})
ADD_NULLS = ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1))


@pytest.mark.parametrize("B,L,d", ADD_SHAPES)
def test_add_rows_exact(cuda, B, L, d):
    g = gen(B * 1000 + L * 10 + d)
    for hx, ht, hu in ADD_NULLS:
        x = ints(g, B, L, d) if hx else None
        t = ints(g, L + 3, d) if ht else None  # a table longer than L: rows [0, L) are added
        u = ints(g, B, d) if hu else None
        ref = R.add_rows(x, t, u, B, L, d)
        for off in (False, True):
            out = sentinel(B, L, d, offset=off)
            _add_rows(_mk(off)(x), _mk(off)(t), _mk(off)(u), out, B, L, d)
            exact(f"add_rows {B}x{L}x{d} x={hx} t={ht} u={hu} off={off}", out, ref)


def test_add_rows_real_and_paths(cuda):
    B, L, d = 2, 33, 100
    g = gen(5)
    x, t, u = _outlier(randn(g, B, L, d)), randn(g, L + 3, d), f32(randn(g, B, d) + 3)
    out, out_s = sentinel(B, L, d), sentinel(B, L, d, offset=True)
    _add_rows(dev(x), dev(t), dev(u), out, B, L, d)
    _add_rows(dev_offset(x), dev_offset(t), dev_offset(u), out_s, B, L, d)
    assert torch.equal(out, out_s)  # tier C: add_rows4_kernel == add_rows_kernel
    tier_b("add_rows", out, R.add_rows, (x, t, u, B, L, d), ops_floor(2))  # two sums


def test_add_rows_large(cuda):
    B, L, d = 1, N4_BIG, 4
    g = torch.Generator(device="cuda").manual_seed(6)
    x = torch.randint(-3, 4, (B, L, d), generator=g, device="cuda", dtype=torch.float32)
    t = torch.randint(-3, 4, (L + 1, d), generator=g, device="cuda", dtype=torch.float32)
    u = torch.randint(-3, 4, (B, d), generator=g, device="cuda", dtype=torch.float32)
    out = torch.full((B, L, d), SENTINEL, device="cuda")
    _add_rows(x, t, u, out, B, L, d)
    ref = R.add_rows(x.double(), t.double(), u.double(), B, L, d)
    assert torch.equal(out, ref.float())


def test_lincomb_add_rows_autograd(cuda):
    """ops.LinComb and ops.AddRows through autograd, exact: the coefficient-scaled cotangents, and the table
    gradient summed over the batch into rows [0, L) of a longer table (the rows past L stay zero)."""
    from asrx import ops

    B, L, d = 3, 5, 100
    g = gen(16)
    x, y, z, cot = (ints(g, B, L, d) for _ in range(4))
    t = ints(g, L + 3, d)
    leaves = [dev(v).requires_grad_() for v in (x, y, z)]
    out = ops.LinComb.apply(*leaves, 2.0, -1.0, -2.0)
    exact("LinComb fwd", out, R.lincomb(x, y, z, 2.0, -1.0, -2.0))
    for name, got, k in zip("xyz", torch.autograd.grad(out, leaves, dev(cot)), (2.0, -1.0, -2.0)):
        exact(f"LinComb d{name}", got, k * cot)
    exact("add fwd", ops.add(dev(x), dev(y)), x + y)
    xg, tg = dev(x).requires_grad_(), dev(t).requires_grad_()
    out = ops.add_rows(xg, tg)
    exact("AddRows fwd", out, R.add_rows(x, t, None, B, L, d))
    out.backward(dev(cot))
    exact("AddRows dx", xg.grad, cot)
    exact("AddRows dt", tg.grad, torch.cat([cot.sum(0), torch.zeros(3, d, dtype=torch.float64)]))


# =========================================================================================== axpy_row
def _axpy_row(x, s, y, out):
    _call("asrx_axpy_row", x, s, y, out, x.shape[0], x.shape[1])


AXPY_SHAPES = sorted({(1, n) for n in N_VEC + N_SCALAR} | {(3, 4), (513, 4)} | set(ROW_SHAPES))


@pytest.mark.parametrize("rows,d", AXPY_SHAPES)
def test_axpy_row_exact(cuda, rows, d):
    g = gen(rows * 7 + d)
    x, y, cot = ints(g, rows, d), ints(g, rows, d), ints(g, rows, d)
    s = ints(g, rows, lo=-2, hi=2)
    for sv in (None, s):
        ref = R.axpy_row(x, sv, y)
        for off in (False, True):
            out = sentinel(rows, d, offset=off)
            _axpy_row(_mk(off)(x), dev(sv), _mk(off)(y), out)
            exact(f"axpy_row {rows}x{d} s={sv is not None} off={off}", out, ref)
    assert 9 * d < 2 ** 24  # |ds| <= 3 * 3 * d
    rdy, rds, rdx = R.axpy_row_bwd(cot, s, y)
    dy, ds = sentinel(rows, d), sentinel(rows)
    _call("asrx_axpy_row_bwd", dev(cot), dev(s), dev(y), dy, ds, rows, d)
    exact("axpy_row_bwd dy", dy, rdy)
    exact("axpy_row_bwd ds", ds, rds)
    dy, ds, dxc = sentinel(rows, d), sentinel(rows), sentinel(rows, d)
    _call("asrx_axpy_row_bwd2", dev(cot), dev(s), dev(y), dy, ds, dxc, rows, d)
    exact("axpy_row_bwd2 dy", dy, rdy)
    exact("axpy_row_bwd2 ds", ds, rds)
    exact("axpy_row_bwd2 dxc", dxc, rdx)


@pytest.mark.parametrize("rows,d", [(33, 100), (5, 384)])
def test_axpy_row_real_and_paths(cuda, rows, d):
    from asrx import ops

    g = gen(rows + d)
    x, y, cot = randn(g, rows, d), _outlier(randn(g, rows, d)), randn(g, rows, d)
    s = f32(randn(g, rows) + 0.5)
    out, out_s = sentinel(rows, d), sentinel(rows, d, offset=True)
    _axpy_row(dev(x), dev(s), dev(y), out)
    _axpy_row(dev_offset(x), dev(s), dev_offset(y), out_s)
    assert torch.equal(out, out_s)  # tier C: axpy_row4_kernel == axpy_row_kernel
    tier_b(f"axpy_row {rows}x{d}", out, R.axpy_row, (x, s, y), ops_floor(2))  # a product and a sum
    # through autograd (ops.AxpyRow): ds is a lane chain of d / 64 products, then a six-level wave sum
    xg, sg, yg = (dev(v).requires_grad_() for v in (x, s, y))
    ops.axpy_row(xg, sg, yg).backward(dev(cot))
    tier_b(f"axpy_row_bwd {rows}x{d}", (yg.grad, sg.grad, xg.grad), R.axpy_row_bwd, (cot, s, y),
           (ops_floor(1), ops_floor(math.ceil(d / 64) + 7), ops_floor(0)), names=("dy", "ds", "dx"))


def test_axpy_row_large(cuda):
    rows, d = N4_BIG, 4
    g = torch.Generator(device="cuda").manual_seed(8)
    x, y = (torch.randint(-3, 4, (rows, d), generator=g, device="cuda", dtype=torch.float32) for _ in range(2))
    s = torch.randint(-2, 3, (rows,), generator=g, device="cuda", dtype=torch.float32)
    out = torch.full((rows, d), SENTINEL, device="cuda")
    _axpy_row(x, s, y, out)
    assert torch.equal(out, R.axpy_row(x.double(), s.double(), y.double()).float())


# =========================================================================================== per-sample column sums
SEG_SHAPES = [(1, 1, 6), (3, 63, 64), (2, 64, 100), (2, 65, 384), (2, 1030, 100)]  # the last: 17 chunks


def _chunks(L):
    from asrx import lib

    return int(lib.load().asrx_mem_chunks(L))


@pytest.mark.parametrize("B,L,d", SEG_SHAPES)
def test_seg_colsum_det_exact(cuda, B, L, d):
    x = ints(gen(L + d), B, L, d)
    assert 3 * L < 2 ** 24
    nch = _chunks(L)
    assert nch == (L + 63) // 64
    part, out = sentinel(B * nch * d), sentinel(B, d)
    _call("asrx_seg_colsum_det", dev(x), part, out, B, L, d, 1.0)
    exact("seg_colsum_det out", out, R.seg_sum(x, 1.0))
    chunks = torch.stack([x[:, c * 64:(c + 1) * 64].sum(1) for c in range(nch)], 1)  # (B, nch, d)
    exact("seg_colsum_det part", part.view(B, nch, d), chunks)


@pytest.mark.parametrize("B,L,d", SEG_SHAPES)
def test_seg_mean_real(cuda, B, L, d):
    from asrx import ops

    g = gen(L * 3 + d)
    x, cot = _outlier(f32(randn(g, B, L, d) + 0.5)), randn(g, B, d)
    xg = dev(x).requires_grad_()
    out = ops.seg_mean(xg)
    out.backward(dev(cot))
    # a wave adds min(L, 64) / 4 rows, three sums join the waves, then one sum per chunk, then the scale
    k = math.ceil(min(L, 64) / 4) + 3 + _chunks(L) + 1
    tier_b(f"seg_mean {B}x{L}x{d}", out, R.seg_sum, (x, float(torch.tensor(1.0 / L, dtype=torch.float32))),
           ops_floor(k))
    # 1 / L rounded to fp32, then one product
    tier_b(f"seg_mean_bwd {B}x{L}x{d}", xg.grad, R.seg_mean_bwd, (cot, L), ops_floor(2))


@pytest.mark.parametrize("rows", [1, 5, 1030])
@pytest.mark.parametrize("d", [6, 64, 100])
def test_colsum_exact(cuda, rows, d):
    from asrx import ops

    g = gen(rows + d)
    assert 3 * rows + SENTINEL < 2 ** 24
    for ld in (d, d + 28):
        buf = ints(g, rows, ld)
        bd = dev(buf)
        col0 = 0 if ld == d else 4  # a column block inside a wider row
        ref = R.colsum(buf[:, col0:col0 + d], torch.full((d,), SENTINEL, dtype=torch.float64))
        out = sentinel(d)  # accumulated into: the sentinel is the non-zero start
        _call("asrx_colsum_ld", bd.data_ptr() + 4 * col0, ld, out, rows, d)
        exact(f"colsum_ld rows={rows} d={d} ld={ld}", out, ref)
        if ld == d:
            out = sentinel(d)
            _call("asrx_colsum", bd, out, rows, d)
            exact(f"colsum rows={rows} d={d}", out, ref)
            exact("ops.colsum", ops.colsum(bd), buf.sum(0))


@pytest.mark.parametrize("rows,d", [(5, 100), (1030, 6), (1030, 100)])
def test_colsum_real(cuda, rows, d):
    g = gen(rows * d)
    x = _outlier(randn(g, rows, d))
    out0 = randn(g, d)
    chunks = min(max(rows // 512, 1), 1024)
    chunk = -(-rows // chunks)
    # per wave two chains of chunk / 8 rows and their sum, three sums join the waves, one atomic per chunk
    k = math.ceil(chunk / 8) + 1 + 3 + (-(-rows // chunk))
    for ld in (d, d + 28):
        buf = f32(randn(g, rows, ld))
        buf[:, :d] = x
        out = dev(out0)
        _call("asrx_colsum_ld", dev(buf), ld, out, rows, d)
        tier_b(f"colsum_ld {rows}x{d} ld={ld}", out, R.colsum, (x, out0), ops_floor(k))


# =========================================================================================== embedding
def _ids(g, V):
    ids = torch.randint(1, 30, (40,), generator=g)
    ids[ids == 17] = 18
    ids[3], ids[21] = 0, V - 1
    ids[torch.tensor([1, 5, 8, 13, 20, 27, 33, 38, 39])] = 17  # one id nine times
    assert int((ids == 17).sum()) == 9 and 0 in ids and V - 1 in ids
    return ids


@pytest.mark.parametrize("d", [6, 384])
def test_embedding_exact(cuda, d):
    V = 50
    g = gen(d)
    ids, E, cot = _ids(g, V), ints(g, V, d), ints(g, 40, d)
    y = sentinel(40, d)
    _call("asrx_embed_fwd", dev(ids), dev(E), y, 40, d)
    exact("embed_fwd", y, R.embed_fwd(ids, E))
    dE = sentinel(V, d)
    _call("asrx_embed_bwd", dev(ids), dev(cot), dE, 40, d)
    exact("embed_bwd", dE, R.embed_bwd(ids, cot, torch.full((V, d), SENTINEL, dtype=torch.float64)))
    unused = torch.tensor([v for v in range(V) if v not in set(ids.tolist())])
    assert len(unused) >= 19 and bool((dE.cpu()[unused] == SENTINEL).all())  # rows of unused ids: not written


@pytest.mark.parametrize("d", [6, 384])
def test_embedding_real(cuda, d):
    from asrx import ops

    V = 50
    g = gen(d + 1)
    ids, E, cot = _ids(g, V), randn(g, V, d), _outlier(randn(g, 40, d))
    Eg = dev(E).requires_grad_()
    y = ops.Embedding.apply(dev(ids), Eg)
    y.backward(dev(cot))
    exact("Embedding fwd", y, R.embed_fwd(ids, E))  # a copy
    tier_b(f"Embedding bwd d={d}", Eg.grad, R.embed_bwd, (ids, cot, torch.zeros(V, d, dtype=torch.float64)),
           ops_floor(9))  # up to nine atomic adds into a row


# =========================================================================================== stem1
STEM_T = (1, 2, 130, 261)  # 261: two 256-step chunks of asrx_stem1_bwd's launcher
STEM_D = (6, 64, 100, 384)


@pytest.mark.parametrize("T", STEM_T)
def test_stem1_exact(cuda, T):
    B = 3
    assert 9 * B * T + SENTINEL < 2 ** 24
    for D in STEM_D:
        g = gen(T * D)
        x, W, b = ints(g, B, T), ints(g, D, 3, lo=-2, hi=2), ints(g, D)
        cot = ints(g, B, T, D)
        y = sentinel(B, T, D)
        _call("asrx_stem1_fwd", dev(x), dev(W), dev(b), y, B, T, D)
        exact(f"stem1_fwd T={T} D={D}", y, R.stem1_fwd(x, W, b))
        dW, db = sentinel(D, 3), sentinel(D)  # accumulated into
        _call("asrx_stem1_bwd", dev(cot), dev(x), dW, db, B, T, D)
        rdW, rdb = R.stem1_bwd(cot, x, torch.full((D, 3), SENTINEL, dtype=torch.float64),
                               torch.full((D,), SENTINEL, dtype=torch.float64))
        exact(f"stem1_bwd dW T={T} D={D}", dW, rdW)
        exact(f"stem1_bwd db T={T} D={D}", db, rdb)


@pytest.mark.parametrize("T", STEM_T)
def test_stem1_real(cuda, T):
    from asrx import ops

    B = 3
    for D in STEM_D:
        g = gen(T + D)
        x, W, b = _outlier(randn(g, B, T)), randn(g, D, 3), f32(randn(g, D) + 2)
        cot = randn(g, B, T, D)
        Wg, bg = dev(W).requires_grad_(), dev(b).requires_grad_()
        y = ops.Stem1.apply(dev(x), Wg, bg)
        y.backward(dev(cot))
        tier_b(f"stem1_fwd T={T} D={D}", y, R.stem1_fwd, (x, W, b), ops_floor(6))  # three products, three sums
        # per wave min(T, 256) / 4 product-sums, three sums join the waves, one atomic per (sample, chunk)
        k = 2 * math.ceil(min(T, 256) / 4) + 3 + B * math.ceil(T / 256)
        z3, z1 = torch.zeros(D, 3, dtype=torch.float64), torch.zeros(D, dtype=torch.float64)
        tier_b(f"stem1_bwd T={T} D={D}", (Wg.grad, bg.grad), R.stem1_bwd, (cot, x, z3, z1), ops_floor(k),
               names=("dW", "db"))


# =========================================================================================== GLU
@pytest.mark.parametrize("rows", [1, 33])
@pytest.mark.parametrize("C", [3, 64, 100])
def test_glu(cuda, rows, C):
    from asrx import ops

    g = gen(rows + C)
    x, cot = _outlier(randn(g, rows, 2 * C)), randn(g, rows, C)
    xg = dev(x).requires_grad_()
    y = ops.glu(xg)
    y.backward(dev(cot))
    tier_b(f"glu_fwd {rows}x{C}", y, R.glu_fwd, (x,), FWD_TRANS)
    tier_b(f"glu_bwd {rows}x{C}", xg.grad, R.glu_bwd, (cot, x), BWD_TRANS)
    dx = sentinel(rows, 2 * C)  # every element of both halves is written
    _call("asrx_glu_bwd", dev(cot), dev(x), dx, rows, C)
    assert torch.equal(dx, xg.grad)


# =========================================================================================== LayerNorm
LN_T = (128, 256, 384, 512, 768, 1024)  # ln_fwd_t_kernel<E> / ln_bwd_t_kernel<E>
LN_G = (6, 100, 192, 2048)  # generic kernels; 2048 is the backward's documented limit
LN_ROWS = (1, 3, 5, 37)
EPS_LN = 1e-5


def _ln_data(g, rows, d):
    x = randn(g, rows, d) * 2 + 50
    x[0] *= 40
    return f32(x), f32(randn(g, d) + 1), randn(g, d)


def _ln_k(d):
    """Dependent fp32 operations behind an element of y: two row sums (a lane chain of d / 64, a six-level
    wave sum), and centre, square, scale, + eps, rsqrt, product, product, + b."""
    return 2 * (math.ceil(d / 64) + 6) + 8


def _ln_fwd(x, w, b, off=False):
    rows, d = x.shape
    y, mean, rstd = sentinel(rows, d), sentinel(rows), sentinel(rows)
    _call("asrx_layernorm_fwd", _mk(off)(x), dev(w), dev(b), y, mean, rstd, rows, d, EPS_LN)
    return y, mean, rstd


def _ln_check_fwd(tag, x, w, b, off=False):
    d = x.shape[1]
    tier_b(tag, _ln_fwd(x, w, b, off), R.layernorm_fwd, (x, w, b, EPS_LN),
           (ops_floor(_ln_k(d)), ops_floor(math.ceil(d / 64) + 7), ops_floor(_ln_k(d))), names=("y", "mean", "rstd"))


@pytest.mark.parametrize("d", LN_T + LN_G)
def test_layernorm_fwd(cuda, d):
    for rows in LN_ROWS:
        _ln_check_fwd(f"ln_fwd d={d} rows={rows}", *_ln_data(gen(d + rows), rows, d))


def test_layernorm_fwd_wrapped_rows(cuda):
    """rows = 32773 at d = 128: past the 8192 x 4 row grid cap, the first prefetch of a wrapped row."""
    _ln_check_fwd("ln_fwd d=128 rows=32773", *_ln_data(gen(9), 32773, 128))


def test_layernorm_offset_x_takes_generic_path(cuda):
    """x one float into its buffer at d = 128 is not 8-byte aligned: the generic kernels must serve it."""
    x, w, b = _ln_data(gen(10), 37, 128)
    _ln_check_fwd("ln_fwd d=128 x offset", x, w, b, off=True)
    _ln_check_bwd("ln_bwd d=128 x offset", gen(11), x, w, acc=0, off=True)


def _ln_fwd3(x, w, b, nrm, gw, gb, on_x, bf16):
    rows, d = x.shape
    y = torch.full((rows, d), SENTINEL, device="cuda", dtype=torch.bfloat16 if bf16 else torch.float32)
    mean, rstd = sentinel(rows), sentinel(rows)
    nr = sentinel(rows) if nrm else None
    gate = sentinel(rows) if gw is not None else None
    _call("asrx_layernorm_fwd3", dev(x), dev(w), dev(b), y, int(bf16), mean, rstd, nr,
          dev(gw), dev(gb), gate, int(on_x), rows, d, EPS_LN)
    return y, mean, rstd, nr, gate


@pytest.mark.parametrize("d", LN_T)
def test_layernorm_fwd3(cuda, d):
    fl = (ops_floor(_ln_k(d)), ops_floor(math.ceil(d / 64) + 7), ops_floor(_ln_k(d)))
    for rows in LN_ROWS:
        g = gen(3 * d + rows)
        x, w, b = _ln_data(g, rows, d)
        gb = randn(g, 1)
        tag = f"ln_fwd3 d={d} rows={rows}"
        y, mean, rstd, nrm, _ = _ln_fwd3(x, w, b, True, None, None, 0, False)
        tier_b(tag + " nrm", (y, mean, rstd), R.layernorm_fwd, (x, w, b, EPS_LN), fl, names=("y", "mean", "rstd"))
        # |x|: squares, a lane chain and a wave sum, a square root
        tier_b(tag, nrm, lambda a: torch.sqrt((a * a).sum(-1)), (x,), ops_floor(math.ceil(d / 64) + 8),
               names=("nrm",))
        for on_x in (0, 1):  # gate weights scaled so that the sigmoid is not saturated
            gw = f32(randn(g, d) / (25 * math.sqrt(d)) if on_x else randn(g, d) / math.sqrt(d))
            y2, m2, r2, _, gate = _ln_fwd3(x, w, b, False, gw, gb, on_x, False)
            assert torch.equal(y2, y) and torch.equal(m2, mean) and torch.equal(r2, rstd)

            def gate_ref(a, ww, bb, gww, gbb, ox=on_x):
                yy = R.layernorm_fwd(a, ww, bb, EPS_LN)[0]
                return R.layernorm_row_outputs(a, yy, gww, gbb, ox)[1]

            tier_b(tag + f" gate_on_x={on_x}", gate, gate_ref, (x, w, b, gw, gb), FWD_TRANS, names=("gate",))
        # tier C: the bf16 output is the round-to-nearest-even of the fp32 output
        y16, m16, r16, n16, _ = _ln_fwd3(x, w, b, True, None, None, 0, True)
        assert torch.equal(y16, y.to(torch.bfloat16))
        assert torch.equal(m16, mean) and torch.equal(r16, rstd) and torch.equal(n16, nrm)


def _ln_check_bwd(tag, g, x, w, acc, off=False, entry=None):
    rows, d = x.shape
    _, mean, rstd = R.layernorm_fwd(x, w, torch.zeros(d, dtype=torch.float64), EPS_LN)
    mean, rstd = f32(mean), f32(rstd)  # the kernel's inputs
    dy = _outlier(randn(g, rows, d), dim0=rows - 1)
    dx0, dw0, db0 = randn(g, rows, d), randn(g, d), randn(g, d)  # dw / db accumulate into non-zero buffers
    dx = dev(dx0) if acc else sentinel(rows, d)
    dw, db = dev(dw0), dev(db0)
    ptrs = (dev(dy), _mk(off)(x), dev(w), dev(mean), dev(rstd), dx, dw, db, rows, d)
    if entry == "asrx_layernorm_bwd":
        assert not acc
        _call(entry, *ptrs)
    else:
        _call("asrx_layernorm_bwd_acc", *ptrs, int(acc))
    grid = min(math.ceil(rows / 4), 1024)
    # dx: the forward's chain plus two more row sums; dw / db: a wave's rows, three sums, one atomic per workgroup
    kx = _ln_k(d) + 2 * (math.ceil(d / 64) + 6) + 6
    kw = 2 * math.ceil(rows / (4 * grid)) + 3 + grid + 2
    tier_b(tag, (dx, dw, db), R.layernorm_bwd, (dy, x, w, mean, rstd, dx0 if acc else None, dw0, db0),
           (ops_floor(kx), ops_floor(kw), ops_floor(kw)), names=("dx", "dw", "db"))


@pytest.mark.parametrize("d", LN_T + LN_G)
def test_layernorm_bwd(cuda, d):
    for rows in LN_ROWS:
        g = gen(5 * d + rows)
        x, w, _ = _ln_data(g, rows, d)
        for acc in (0, 1):
            _ln_check_bwd(f"ln_bwd d={d} rows={rows} acc={acc}", g, x, w, acc)
        _ln_check_bwd(f"ln_bwd d={d} rows={rows} plain", g, x, w, 0, entry="asrx_layernorm_bwd")


def test_layernorm_bwd_wrapped_rows(cuda):
    """rows = 4101 at d = 128: past the backward's 1024 x 4 row grid cap."""
    g = gen(12)
    x, w, _ = _ln_data(g, 4101, 128)
    for acc in (0, 1):
        _ln_check_bwd(f"ln_bwd d=128 rows=4101 acc={acc}", g, x, w, acc)


def test_layer_norm_autograd(cuda):
    """ops.LayerNormFn at a register-resident width, parameter gradients straight into .grad."""
    from asrx import ops

    rows, d = 37, 384
    g = gen(13)
    x, w, b = _ln_data(g, rows, d)
    cot = randn(g, rows, d)
    xg, wg, bg = (dev(v).requires_grad_() for v in (x, w, b))
    y = ops.layer_norm(xg, wg, bg, EPS_LN)
    y.backward(dev(cot))

    def ref(cc, a, ww, bb):
        yy, mean, rstd = R.layernorm_fwd(a, ww, bb, EPS_LN)
        z = torch.zeros(d, dtype=a.dtype)
        return (yy,) + R.layernorm_bwd(cc, a, ww, mean, rstd, None, z, z)

    kx = _ln_k(d) + 2 * (math.ceil(d / 64) + 6) + 6
    kw = 2 + 3 + 10 + 2
    tier_b("layer_norm autograd", (y, xg.grad, wg.grad, bg.grad), ref, (cot, x, w, b),
           (ops_floor(_ln_k(d)), ops_floor(kx), ops_floor(kw), ops_floor(kw)), names=("y", "dx", "dw", "db"))


# =========================================================================================== ReLU
def test_relu_act_autograd(cuda):
    from asrx import ops

    for n, off in ((2052, False), (2051, False), (100, True)):
        g = gen(n)
        x, cot = _act_input(g, n), randn(g, n)
        xg = _mk(off)(x).requires_grad_()
        y = ops.act(xg, "relu")
        y.backward(dev(cot))
        exact(f"relu fwd n={n}", y, R.act_fwd(x, "relu"))
        exact(f"relu bwd n={n}", xg.grad, R.act_bwd(cot, x, "relu"))
        assert bool((xg.grad.cpu()[x.float() < 0] == 0).all())


def test_relu_linear(cuda):
    """ops.linear(..., act="relu") in fp32 mode: output, input gradient and parameter gradients against float64.
    Integer x and W with half-integer biases keep every pre-activation at least 0.5 from zero, so rounding
    cannot move an element across the kink."""
    from asrx import ops

    rows, K, N = 37, 64, 96
    g = gen(14)
    x, W = ints(g, rows, K), ints(g, N, K, lo=-2, hi=2)
    b = ints(g, N) + 0.5
    cot = randn(g, rows, N)
    z = x @ W.t() + b
    assert float(z.abs().min()) >= 0.5 and bool((z < 0).any()) and bool((z > 0).any())
    xg, Wg, bg = (dev(v).requires_grad_() for v in (x, W, b))
    y = ops.linear(xg, Wg, bg, act="relu")
    y.backward(dev(cot))
    gz = cot * (z > 0).double()
    for name, got, want, tol in (("y", y, z.clamp_min(0), 1e-5), ("dx", xg.grad, gz @ W, 1e-4),
                                 ("dW", Wg.grad, gz.t() @ x, 1e-4), ("db", bg.grad, gz.sum(0), 1e-4)):
        e = rel(got, want)
        print(f"TIERB relu_linear.{name:<32s} e={e:.2e} bound={tol:.2e}")
        assert e <= tol, (name, e)
    assert bool((y.cpu()[z < 0] == 0).all())  # exactly zero where the unit is off


@pytest.mark.parametrize("name", ["relu", "gelu", "silu"])
def test_small_linear_rejects_undifferentiated_acts(cuda, name):
    """small_linear's backward differentiates the sigmoid only: any other activation is an error return from
    both launchers (nothing is launched), not a forward whose gradient would silently be the identity."""
    from asrx import ops
    from asrx.gemm import ACT

    g = gen(17)
    x, W, b = dev(randn(g, 5, 64)), dev(randn(g, 2, 64)), dev(randn(g, 2))
    with pytest.raises(RuntimeError, match="small_linear"):
        ops.small_linear(x, W, b, act=name)
    y, dx, dW, db = sentinel(5, 2), sentinel(5, 64), sentinel(2, 64), sentinel(2)
    with pytest.raises(RuntimeError, match="small_linear_bwd"):
        _call("asrx_small_linear_bwd", dev(randn(g, 5, 2)), y, x, W, dx, dW, db, 5, 64, 2, ACT[name], 0.0)
    assert all(bool((t == SENTINEL).all()) for t in (dx, dW, db))


@pytest.mark.parametrize("act,act2", [("relu", "none"), ("gelu", "relu"), ("relu", "gelu"), ("relu", "relu")])
def test_relu_act_dropout(cuda, act, act2):
    """asrx_act_dropout_fwd / _bwd with relu as either activation; the mask is the same entry's output for
    act none on an all-ones input (mask parity with the oracle is test_act_dropout_fused's)."""
    from asrx.gemm import ACT

    B, T, C, sid, key, p = 2, 50, 384, 3, 0x1234ABCD, 0.1
    g = gen(15)
    z, cot = randn(g, B, T, C), randn(g, B, T, C)
    z[z == 0] = 1.0
    ones = torch.ones(B, T, C, device="cuda")
    m = sentinel(B, T, C)
    _call("asrx_act_dropout_fwd", ones, None, m, B, T, C, sid, key, p, ACT["none"], ACT["none"])
    keep = (m.cpu() != 0).double()
    assert 0.8 < float(keep.mean()) < 0.97
    y, dz = sentinel(B, T, C), sentinel(B, T, C)
    _call("asrx_act_dropout_fwd", dev(z), None, y, B, T, C, sid, key, p, ACT[act], ACT[act2])
    _call("asrx_act_dropout_bwd", dev(cot), dev(z), dz, B, T, C, sid, key, p, ACT[act], ACT[act2])
    p32 = float(torch.tensor(p, dtype=torch.float32))
    tier_b(f"act_dropout {act}+{act2} fwd", y, R.act_dropout_fwd, (z, keep, p32, act, act2), FWD_TRANS)
    tier_b(f"act_dropout {act}+{act2} bwd", dz, R.act_dropout_bwd, (cot, z, keep, p32, act, act2), BWD_TRANS)
    off = (z < 0) if act == "relu" else (keep == 0)
    assert bool((dz.cpu()[off] == 0).all())  # no gradient through a unit that is off
