"""MSheath with per-sample lengths (MSheath.run(lens=), asrx/msheath.py, the asrx_*_lens_* entry points of
csrc/rowops.hip, csrc/msheath.hip and csrc/gemm_wn.hip): in a padded batch, sample b comes out bit for bit as
mod.run(x[b:b+1, :T_b], noise, site, sid_base + b) gives it alone.

The module is MSheath(D, 2, 4) as test_msheath sets it up (concat biases spread, sample 1 damped so that its potential
is below 0.1: it is forced to jump and gam carries its mem mean), in train mode.  B = 8, L = 200 and the lengths
[200, 199, 1, 63, 64, 65, 128, 129]: a single row, both sides of the 64-row mem chunk and of the 128-row jump chunk,
the last row, the full length.  The pad rows of x hold a large finite sentinel and those of the cotangent NaN.
"""
import pytest
import torch

from oracle import model as om

pytestmark = pytest.mark.gpu

LENS = [200, 199, 1, 63, 64, 65, 128, 129]
B, L, LAYER = 8, 200, 4
SEED, STEP, SITE, SID = 9, 1, "t.jump", 5
SENTINEL = 1.0e4


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _module(D):
    from asrx.model import MSheath

    torch.manual_seed(3)
    mod = MSheath(D, 2, LAYER).cuda()
    mod.fused = True
    mod.train()
    with torch.no_grad():
        for i in range(LAYER):
            mod.layers[i]["v_gate"].concat.bias.fill_(0.3 + 0.1 * (i - 1))
    return mod


def _inputs(D, lens=LENS, Lmax=L, pad=SENTINEL):
    nb = len(lens)
    x = torch.randn(nb, Lmax, D, generator=torch.Generator().manual_seed(11))
    x[1] *= 0.1
    gout = torch.randn(nb, Lmax, D, generator=torch.Generator().manual_seed(0))
    for b, t in enumerate(lens):
        x[b, t:] = pad
        gout[b, t:] = float("nan")
    return x, gout


def _run(mod, x, gout, precision, lens, sid=SID, grad=True):
    """-> y, dx, {name: parameter gradient} of one forward + backward."""
    from asrx import prec
    from asrx.noise import NoiseCtx

    for p in mod.parameters():
        p.grad = None
    xi = x.cuda().requires_grad_(grad)
    with prec.precision(precision):
        y = mod.run(xi, NoiseCtx(SEED, STEP, True), SITE, sid, lens=lens)
        if grad:
            y.backward(gout.cuda())
    torch.cuda.synchronize()
    if not grad:
        return y.detach(), None, {}
    return y.detach(), xi.grad, {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None}


_CACHE = {}


def _runs(D, precision):
    """The padded batch with lengths and every sample alone, computed once per (D, precision)."""
    from asrx import ops

    key = (D, precision)
    if key not in _CACHE:
        mod = _module(D)
        x, gout = _inputs(D)
        batch = _run(mod, x, gout, precision, ops.seq_lens(LENS))
        alone = [_run(mod, x[b:b + 1, :t].contiguous(), gout[b:b + 1, :t].contiguous(), precision, None, SID + b)
                 for b, t in enumerate(LENS)]
        _CACHE[key] = (mod, x, gout, batch, alone)
    return _CACHE[key]


def _oracle_grads(mod, x, gout):
    """float64: the oracle on every x[b:b+1, :T_b], parameter gradients summed over the samples."""
    trainable = {n for n, p in mod.named_parameters() if p.requires_grad}
    P = {f"j.{k}": v.detach().cpu().double().requires_grad_(k in trainable) for k, v in mod.state_dict().items()}
    onoise = om.Noise(SEED, STEP, torch.float64)
    gpol = onoise.policy(SITE, [SID + b for b in range(B)], LAYER)
    for b, t in enumerate(LENS):
        y = om.msheath(P, "j", x[b:b + 1, :t].double(), LAYER, gpol[b:b + 1])
        y.backward(gout[b:b + 1, :t].double())
    return {k[2:]: v.grad for k, v in P.items() if v.grad is not None}


def _check_bitwise(batch, alone, what):
    y, dx, _ = batch
    for b, t in enumerate(LENS):
        ya, dxa, _ = alone[b]
        assert torch.equal(y[b, :t], ya[0]), (what, "y", b, t)
        assert torch.equal(dx[b, :t], dxa[0]), (what, "dx", b, t)
        assert not y[b, t:].any() and not dx[b, t:].any(), (what, "pad rows", b, t)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())


@pytest.mark.parametrize("D", [128, 384])
def test_module_fp32(cuda, D):
    """fp32 parity mode: live rows of y and dx equal the alone runs', pad rows are exactly zero, everything is finite;
    parameter gradients within 2e-3 (test_msheath's gate) of the float64 oracle's per-sample sum and of the float64
    sum of the alone runs' gradients."""
    mod, x, gout, batch, alone = _runs(D, "fp32")
    _check_bitwise(batch, alone, f"fp32 D={D}")
    pg = batch[2]
    assert len(pg) > 40 and all(bool(torch.isfinite(g).all()) for g in pg.values())
    ref = _oracle_grads(mod, x, gout)
    checked = 0
    for n, g in pg.items():
        s = sum(a[2][n].double() for a in alone if n in a[2])
        e_alone = _rel(g, s)
        line = f"fp32 D={D} {n}: to the alone sum {e_alone:.2e}"
        if n in ref and not n.startswith("shared_head"):
            e, ea = _rel(g, ref[n]), _rel(s, ref[n])
            print(line + f", to the oracle {e:.2e} (the alone sum's own {ea:.2e})")
            assert e < 2e-3, (n, e)
            checked += 1
        else:
            print(line)
        assert e_alone < 2e-3, (n, e_alone)
    assert checked > 40


@pytest.mark.parametrize("D", [128, 384])
def test_module_bf16(cuda, D):
    """bf16 perf mode: the same equalities (y and dx bit for bit); parameter gradients within 2^-8 of the float64 sum
    of the alone runs' (the bound of test_module_switch_on_off_bf16: one bf16 step of an operand)."""
    mod, x, gout, batch, alone = _runs(D, "bf16")
    _check_bitwise(batch, alone, f"bf16 D={D}")
    pg = batch[2]
    assert len(pg) > 40 and all(bool(torch.isfinite(g).all()) for g in pg.values())
    for n, g in pg.items():
        s = sum(a[2][n].double() for a in alone if n in a[2])
        e = _rel(g, s)
        print(f"bf16 D={D} {n}: to the alone sum {e:.2e}")
        assert e <= 2.0 ** -8, (n, e)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_nan_pad_rows_of_x_leave_y_unchanged(cuda, precision):
    """Forward only: GEMM rows are independent, so NaN in x's pad rows reaches no live row (and no pad row of y)."""
    from asrx import ops

    mod, x, gout, batch, _ = _runs(128, precision)
    xn, _ = _inputs(128, pad=float("nan"))
    with torch.no_grad():
        y, _, _ = _run(mod, xn, gout, precision, ops.seq_lens(LENS), grad=False)
    assert torch.equal(y, batch[0])


@pytest.mark.parametrize("switch", ["BWD_FUSED", "ROW_COLSUM"])
def test_switches_off(cuda, monkeypatch, switch):
    """The six-step backward and the two-launch x_new form use the same LENS kernels: the same equalities."""
    from asrx import msheath as ms
    from asrx import ops

    mod, x, gout, batch, alone = _runs(128, "fp32")
    monkeypatch.setattr(ms, switch, False)
    off = _run(mod, x, gout, "fp32", ops.seq_lens(LENS))
    off_alone = [_run(mod, x[b:b + 1, :t].contiguous(), gout[b:b + 1, :t].contiguous(), "fp32", None, SID + b)
                 for b, t in enumerate(LENS)]
    _check_bitwise(off, off_alone, switch + " off")
    if switch == "BWD_FUSED":  # the forward is untouched (the two x_new forms sum their chunks in different orders)
        assert torch.equal(off[0], batch[0])
    for n, g in off[2].items():
        s = sum(a[2][n].double() for a in off_alone if n in a[2])
        assert _rel(g, s) < 2e-3, (n, _rel(g, s))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_no_grad(cuda, monkeypatch, precision):
    """Without autograd: the Python loop with the LENS kernels (never the composite call), y as in training."""
    from asrx import lib, ops

    mod, x, gout, batch, _ = _runs(128, precision)
    calls = []
    real = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    with torch.no_grad():
        y, _, _ = _run(mod, x, gout, precision, ops.seq_lens(LENS), grad=False)
    assert "asrx_msheath_fwd" not in calls and "asrx_jump_lens_axpy_inplace" in calls
    assert torch.equal(y, batch[0])


def test_full_length_table(cuda, monkeypatch):
    """An all-full table takes the calls, the grad_fn class and the kernels of lens=None: equal results."""
    from asrx import lib, ops

    mod = _module(128)
    x, gout = _inputs(128, lens=[L] * B)
    names = []
    real = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])

    def one(lens):
        from asrx import prec
        from asrx.noise import NoiseCtx

        del names[:]
        for p in mod.parameters():
            p.grad = None
        xi = x.cuda().requires_grad_(True)
        with prec.precision("fp32"):
            y = mod.run(xi, NoiseCtx(SEED, STEP, True), SITE, SID, lens=lens)
            fn = type(y.grad_fn)
            y.backward(gout.cuda())
        return y.detach(), xi.grad, fn, list(names)

    one(None)  # (the first call of a module also builds its derived v_gate weights)
    y0, g0, f0, n0 = one(None)
    y1, g1, f1, n1 = one(ops.seq_lens([L] * B))
    y2, g2, f2, n2 = one(ops.SeqLens.full(B, L, torch.device("cuda", torch.cuda.current_device())))
    assert n0 == n1 == n2 and not any("_lens_" in n for n in n0)
    assert f0 is f1 is f2
    assert torch.equal(y0, y1) and torch.equal(y0, y2) and torch.equal(g0, g1) and torch.equal(g0, g2)


def test_lengths_matter(cuda):
    """The damped sample (forced to jump, gam carries the mem mean; T = 199 with a large sentinel in its one pad row)
    differs on its live rows from the run that ignores the lengths on the same padded tensor."""
    mod, x, gout, batch, _ = _runs(128, "fp32")
    with torch.no_grad():
        y, _, _ = _run(mod, x, gout, "fp32", None, grad=False)
    assert bool(torch.isfinite(y).all())
    assert not torch.equal(y[1, :LENS[1]], batch[0][1, :LENS[1]])
    assert torch.equal(y[0], batch[0][0])  # the full-length sample does not


def test_control_kernel_512_threads(cuda):
    """D = 768 (the 512-thread control kernel), B = 3, forward: live rows equal the alone runs', pad rows zero."""
    from asrx import ops

    lens = [130, 129, 64]
    mod = _module(768)
    x, gout = _inputs(768, lens=lens, Lmax=130)
    with torch.no_grad():
        y, _, _ = _run(mod, x, gout, "fp32", ops.seq_lens(lens), grad=False)
        for b, t in enumerate(lens):
            ya, _, _ = _run(mod, x[b:b + 1, :t].contiguous(), gout, "fp32", None, SID + b, grad=False)
            assert torch.equal(y[b, :t], ya[0]), b
            assert not y[b, t:].any()


# ------------------------------------------------------------------------------------------ kernel level, C-ABI
def _seg(x, lens):
    from asrx import lib

    nb, Lx, D = x.shape
    nch = int(lib.load().asrx_mem_chunks(Lx))
    part = torch.full((nb, nch, D), float("nan"), device="cuda")
    out = torch.empty(nb, D, device="cuda")
    if lens is None:
        lib.call("asrx_seg_colsum_det", x.data_ptr(), part.data_ptr(), out.data_ptr(), nb, Lx, D, 1.0 / Lx,
                 lib.stream())
    else:
        lib.call("asrx_seg_colsum_lens_det", x.data_ptr(), part.data_ptr(), out.data_ptr(), lens.data_ptr(), nb, Lx, D,
                 lib.stream())
    return out


@pytest.mark.parametrize("D", [128, 100])
def test_seg_colsum_lens_det(cuda, D):
    """The pooled mean against the uniform twin on each sample alone, bit for bit (the first ceil(T_b / 64) chunk sums
    in order, times 1 / T_b formed on the device as float(1.0 / T_b))."""
    x, _ = _inputs(D, pad=float("nan"))
    x = x.cuda()
    out = _seg(x, torch.tensor(LENS, dtype=torch.int32, device="cuda"))
    for b, t in enumerate(LENS):
        assert torch.equal(out[b:b + 1], _seg(x[b:b + 1, :t].contiguous(), None)), (b, t)


def test_table_with_zero_and_too_long(cuda):
    """Straight through the C-ABI a table may hold 0 and L + 7: the empty sample's mean is 0 and finite, the
    overlong one is clamped to the full length."""
    x = torch.randn(3, 70, 128, device="cuda")
    out = _seg(x, torch.tensor([0, 77, 70], dtype=torch.int32, device="cuda"))
    full = _seg(x, None)
    assert not out[0].any() and bool(torch.isfinite(out).all())
    assert torch.equal(out[1], full[1]) and torch.equal(out[2], full[2])


def test_row_tile_list(cuda):
    """asrx_row_lens_tiles against a host-computed set: a 128-row tile is listed only if it holds a live row of a sample
    at the layer."""
    from asrx import gemm as G

    Lx, lens, next_i, layer = 200, [200, 1, 129, 56, 200, 64], [1.0, 1.0, 1.0, 2.0, 2.0, 1.0], 1
    M = Lx * len(lens)
    tl, cnt = G.row_tiles(torch.tensor(next_i, device="cuda"), layer, Lx, M,
                          lens=torch.tensor(lens, dtype=torch.int32, device="cuda"))
    got = tl[:int(cnt)].tolist()
    want = sorted({r // 128 for b, t in enumerate(lens) if next_i[b] == layer for r in range(b * Lx, b * Lx + t)})
    assert got == want
    uniform, ucnt = G.row_tiles(torch.tensor(next_i, device="cuda"), layer, Lx, M)
    assert set(got) < set(uniform[:int(ucnt)].tolist())


def test_value_errors(cuda, monkeypatch):
    """What the LENS path cannot take raises ValueError and never falls back to kernels that ignore the lengths."""
    from asrx import decisions
    from asrx import msheath as ms
    from asrx import ops
    from asrx.model import MSheath
    from asrx.noise import NoiseCtx

    mod = _module(128)
    x = torch.randn(2, 40, 128, device="cuda")
    noise = NoiseCtx(SEED, STEP, True)
    short = ops.seq_lens([40, 17])
    with torch.no_grad():
        mod.run(x, noise, SITE, SID, lens=short)  # the control: this call is fine
        with pytest.raises(ValueError):
            mod.run(x, noise, SITE, SID, lens=ops.seq_lens([40, 17, 3]))  # wrong count
        with pytest.raises(ValueError):
            mod.run(x, noise, SITE, SID, lens=ops.seq_lens([41, 17]))  # a length above L
        monkeypatch.setattr(ms, "DETERMINISTIC", False)
        with pytest.raises(ValueError):
            mod.run(x, noise, SITE, SID, lens=short)
        monkeypatch.setattr(ms, "DETERMINISTIC", True)
        monkeypatch.setattr(decisions, "active", lambda: True)
        with pytest.raises(ValueError):
            mod.run(x, noise, SITE, SID, lens=short)
        monkeypatch.undo()
        monkeypatch.setattr(mod, "fused", False)
        with pytest.raises(ValueError):
            mod.run(x, noise, SITE, SID, lens=short)
        monkeypatch.undo()
        wide = MSheath(192, 2, LAYER).cuda()  # a width outside ROW_DIMS: the composed path
        with pytest.raises(ValueError):
            wide.run(torch.randn(2, 40, 192, device="cuda"), noise, SITE, SID, lens=short)
        # all-full lengths are no lengths: the composed path takes them
        wide.run(torch.randn(2, 40, 192, device="cuda"), noise, SITE, SID, lens=ops.seq_lens([40, 40]))


# ------------------------------------------------- kernel level, C-ABI: the ops that reach across rows, against
# the uniform twin on the sample alone (torch.equal).  What a LENS kernel must not read holds NaN.
KD, KM, KDH = 128, 8, 64
NAN = float("nan")


def _p(t):
    return None if t is None else t.data_ptr()


def _tab(lens):
    return torch.tensor(lens, dtype=torch.int32, device="cuda")


def _row_weights(D=KD):
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g).cuda()  # noqa: E731
    return dict(lnw=1 + 0.1 * r(D), lnb=0.1 * r(D), gw=0.2 * r(D), gb=0.1 * r(1), mval=r(KM), w2=0.3 * r(KDH), b2=0.1 * r(1),
                cw=r(2), cb=0.1 * r(1), tx=torch.full((1,), 0.1).cuda())


def _row_fwd3(W, x, SH, lens=None, next_i=None, layer=0):
    """asrx_msheath_row_fwd3 / its lens form on x (B, L, D), SH (B, L, M + Dh) -> the outputs, NaN-prefilled."""
    from asrx import lib

    nb, Lx, D = x.shape
    rows, nch = nb * Lx, int(lib.load().asrx_mem_chunks(Lx))
    o = {k: torch.full((nb, Lx), NAN, device="cuda") for k in ("mean", "rstd", "nx", "g", "ion", "kv", "m2")}
    o["px"], o["xnew"] = torch.full((nb, Lx, D), NAN, device="cuda"), torch.full((nb, Lx, D), NAN, device="cuda")
    o["part"] = torch.full((nb, nch, D), NAN, device="cuda")
    head = [_p(x), _p(W["lnw"]), _p(W["lnb"]), _p(W["gw"]), _p(W["gb"]), _p(SH), KM + KDH, _p(W["mval"]), _p(W["w2"]),
            _p(W["b2"]), _p(W["cw"]), _p(W["cb"]), _p(W["tx"]), _p(o["px"])] + \
           [_p(o[k]) for k in ("mean", "rstd", "nx", "g", "ion", "kv", "m2")] + [_p(o["xnew"]), _p(o["part"])]
    tail = [rows, D, KM, KDH, 1e-5, 1.0 / D ** 0.5, _p(next_i), layer, Lx, lib.stream()]
    if lens is None:
        lib.call("asrx_msheath_row_fwd3", *head, *tail)
    else:
        lib.call("asrx_msheath_row_lens_fwd3", *head, _p(lens), *tail)
    torch.cuda.synchronize()
    return o


def _colsum(x, s1, s2, y, lens=None, next_i=None, layer=0):
    from asrx import lib

    nb, Lx, D = x.shape
    out = torch.full((nb, Lx, D), NAN, device="cuda")
    part = torch.full((nb, int(lib.load().asrx_mem_chunks(Lx)), D), NAN, device="cuda")
    if lens is None:
        lib.call("asrx_axpy_row2_colsum", _p(x), _p(s1), _p(s2), _p(y), _p(out), _p(part), nb, Lx, D, _p(next_i), layer,
                 lib.stream())
    else:
        lib.call("asrx_axpy_row2_lens_colsum", _p(x), _p(s1), _p(s2), _p(y), _p(out), _p(part), _p(lens), nb, Lx, D,
                 _p(next_i), layer, lib.stream())
    torch.cuda.synchronize()
    return out, part


def _ctrl_weights(D):
    g = torch.Generator().manual_seed(6)
    return dict(mg_w=(0.1 * torch.randn(D, generator=g)).cuda(), mg_b=torch.zeros(1).cuda(),
                jump_s=torch.tensor([0.3, 0.5, 0.7]).cuda())


def _ctrl_fwd(C, policy, gpol, ion, mem_w, mem_part, lens=None, layer_i=0, layers=4):
    """asrx_msheath_ctrl_fwd3 / its lens form -> every output (rec as int32 words)."""
    from asrx import lib

    nb, Lx = ion.shape
    D = mem_w.shape[-1]
    o = {k: torch.full((nb,), NAN, device="cuda") for k in ("mem_v", "alpha", "beta", "active", "next_out")}
    o.update({k: torch.full((nb, D), NAN, device="cuda") for k in ("mem", "gam", "mwo")})
    o["rec"] = torch.zeros(nb, int(lib.load().asrx_msheath_rec_bytes()) // 4, dtype=torch.int32, device="cuda")
    head = [_p(policy), _p(gpol), gpol.stride(0), _p(ion), _p(C["mg_w"]), _p(C["mg_b"]), _p(o["mem_v"]), _p(mem_w), D,
            _p(mem_part), _p(o["mem"]), _p(C["jump_s"]), None, layer_i, layers]
    tail = [nb, Lx, D] + [_p(o[k]) for k in ("alpha", "beta", "gam", "mwo", "active", "next_out", "rec")] + [lib.stream()]
    if lens is None:
        lib.call("asrx_msheath_ctrl_fwd3", *head, *tail)
    else:
        lib.call("asrx_msheath_ctrl_lens_fwd3", *head, _p(lens), *tail)
    torch.cuda.synchronize()
    return o


def _jump_ctrl_bwd(C, g, xn, orig, f, mem_w, g_mwo, lens=None, with_dxn=True, layer_i=0, layers=4):
    """The jump backward's partials, then the control backward that adds them; f: the control forward's outputs."""
    from asrx import lib

    nb, Lx, D = g.shape
    has_orig = torch.zeros(nb, dtype=torch.int32, device="cuda")
    o = {k: torch.full((nb, Lx, D), NAN, device="cuda") for k in ("dxn", "dorig", "dx")}
    part = torch.full((int(lib.load().asrx_jump_bwd_part_floats(nb, Lx, D)),), NAN, device="cuda")
    o.update(g_policy=torch.full((nb, 3), NAN, device="cuda"), g_mem_w=torch.full((nb, D), NAN, device="cuda"),
             g_mem=torch.full((nb, D), NAN, device="cuda"), g_jump_s=torch.zeros(3, device="cuda"),
             g_mg_w=torch.zeros(D, device="cuda"), g_mg_b=torch.zeros(1, device="cuda"), has_orig=has_orig)
    ja = [_p(g), _p(xn), _p(orig), _p(f["active"]), _p(f["alpha"]), _p(f["beta"]), _p(has_orig),
          _p(o["dxn"]) if with_dxn else None, _p(o["dorig"]), _p(o["dx"]), _p(part)]
    cb = [_p(g_mwo), _p(f["mem_v"]), _p(mem_w), D, _p(f["mem"]), _p(C["jump_s"]), _p(f["rec"]), layer_i, layers, nb, D,
          _p(o["g_policy"]), 0, _p(o["g_mem_w"]), _p(o["g_mem"]), _p(o["g_jump_s"]), _p(has_orig), _p(C["mg_w"]),
          _p(o["g_mg_w"]), _p(o["g_mg_b"]), lib.stream()]
    if lens is None:
        lib.call("asrx_jump_select4_bwd_part2", *ja, nb, Lx, D, lib.stream())
        lib.call("asrx_msheath_ctrl_bwd4", _p(part), Lx, *cb)
    else:
        lib.call("asrx_jump_lens_select4_bwd_part2", *ja, _p(lens), nb, Lx, D, lib.stream())
        lib.call("asrx_msheath_ctrl_lens_bwd4", _p(part), _p(lens), Lx, *cb)
    torch.cuda.synchronize()
    return o


def _row_inputs(lens, Lx, D=KD, seed=21):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(len(lens), Lx, D, generator=g).cuda()
    SH = torch.randn(len(lens), Lx, KM + KDH, generator=g).cuda()
    for b, t in enumerate(lens):
        x[b, min(t, Lx):] = NAN
        SH[b, min(t, Lx):] = NAN
    return x, SH


@pytest.mark.parametrize("with_next_i", [False, True])
def test_row_fwd3_chunk_sums(cuda, with_next_i):
    """asrx_msheath_row_lens_fwd3: the chunk sums, x_new and the row scalars of each sample at the layer equal the twin's
    on the sample alone; pad rows and the partials of chunks with no live row are zeros; pad rows are not read (NaN)."""
    W = _row_weights()
    x, SH = _row_inputs(LENS, L)
    next_i = torch.tensor([1., 1., 1., 0., 1., 1., 0., 1.], device="cuda") if with_next_i else None
    o = _row_fwd3(W, x, SH, _tab(LENS), next_i, 1 if with_next_i else 0)
    for b, t in enumerate(LENS):
        nc = (t + 63) // 64
        if with_next_i and float(next_i[b]) != 1.0:
            assert not o["part"][b].any() and not o["ion"][b].any() and not o["px"][b].any()
            continue
        a = _row_fwd3(W, x[b:b + 1, :t].contiguous(), SH[b:b + 1, :t].contiguous())
        assert torch.equal(o["part"][b, :nc], a["part"][0]), (b, t)
        assert not o["part"][b, nc:].any()
        for k in ("xnew", "px", "mean", "rstd", "nx", "g", "ion", "kv", "m2"):
            assert torch.equal(o[k][b, :t], a[k][0]), (k, b, t)
            assert not o[k][b, t:].any(), (k, b, t)


def test_axpy_row2_lens_colsum(cuda):
    """asrx_axpy_row2_lens_colsum against asrx_axpy_row2_colsum on the sample alone: x_new, its chunk sums."""
    g = torch.Generator().manual_seed(22)
    x, y = torch.randn(B, L, KD, generator=g).cuda(), torch.randn(B, L, KD, generator=g).cuda()
    s1, s2 = torch.rand(B, L, generator=g).cuda(), (torch.rand(B, L, generator=g) > 0.5).float().cuda()
    for b, t in enumerate(LENS):
        for v in (x, y, s1, s2):
            v[b, t:] = NAN
    next_i = torch.tensor([0., 0., 0., 0., 2., 0., 0., 0.], device="cuda")
    out, part = _colsum(x, s1, s2, y, _tab(LENS), next_i, 0)
    for b, t in enumerate(LENS):
        nc = (t + 63) // 64
        if b == 4:
            assert not part[b].any()
            continue
        ao, ap = _colsum(*(v[b:b + 1, :t].contiguous() for v in (x, s1, s2, y)))
        assert torch.equal(out[b, :t], ao[0]) and not out[b, t:].any(), (b, t)
        assert torch.equal(part[b, :nc], ap[0]) and not part[b, nc:].any(), (b, t)


def _ctrl_inputs(lens, Lx, D, seed=23, p_ion=0.1):
    g = torch.Generator().manual_seed(seed)
    nb, nch = len(lens), (Lx + 63) // 64
    policy = torch.softmax(torch.randn(nb, 3, generator=g), -1).cuda()
    gpol = torch.randn(nb, 3, generator=g).cuda()
    ion = (torch.rand(nb, Lx, generator=g) < p_ion).float().cuda()
    ion[0] = (torch.rand(Lx, generator=g) < 0.5).float().cuda()  # one sample well above the 0.1 threshold
    mem_w = torch.randn(nb, D, generator=g).cuda()
    mem_part = torch.randn(nb, nch, D, generator=g).cuda()
    for b, t in enumerate(lens):
        ion[b, min(t, Lx):] = NAN
        mem_part[b, (min(t, Lx) + 63) // 64:] = NAN
    return policy, gpol, ion, mem_w, mem_part


def _ctrl_alone(C, inp, b, t):
    policy, gpol, ion, mem_w, mem_part = inp
    return _ctrl_fwd(C, policy[b:b + 1].contiguous(), gpol[b:b + 1].contiguous(), ion[b:b + 1, :t].contiguous(),
                     mem_w[b:b + 1].contiguous(), mem_part[b:b + 1, :(t + 63) // 64].contiguous())


@pytest.mark.parametrize("Lx,lens,D", [(L, LENS, 128), (6200, [6200, 6145, 6144, 100], 128),
                                      (6200, [6200, 6145, 6144, 100], 768)])
def test_ctrl_fwd(cuda, Lx, lens, D):
    """asrx_msheath_ctrl_lens_fwd3 against the twin on the sample alone, every output and the record.  L = 6200 takes
    the non-prefetched ion loop (more than 6144 rows) in the batch while the samples of 6144 and 100 rows alone take
    the prefetched branch: both add a thread's values in the same order.  D = 768: the 512-thread kernel."""
    C = _ctrl_weights(D)
    inp = _ctrl_inputs(lens, Lx, D)
    o = _ctrl_fwd(C, *inp, lens=_tab(lens))
    for b, t in enumerate(lens):
        a = _ctrl_alone(C, inp, b, t)
        for k in o:
            assert torch.equal(o[k][b:b + 1], a[k]), (k, b, t)
    assert all(bool(torch.isfinite(o[k]).all()) for k in o if k != "rec")


@pytest.mark.parametrize("with_dxn", [True, False])
def test_jump_partials_and_ctrl_bwd(cuda, with_dxn):
    """asrx_jump_lens_select4_bwd_part2 then asrx_msheath_ctrl_lens_bwd4 against the twins on the sample alone:
    g_policy, g_mem, g_mem_w, and the live rows of dxn and dorig; the pad rows this pass writes first are zeros and
    pad rows of g are not read (NaN)."""
    D = KD
    C = _ctrl_weights(D)
    inp = _ctrl_inputs(LENS, L, D)
    lt = _tab(LENS)
    f = _ctrl_fwd(C, *inp, lens=lt)
    gen = torch.Generator().manual_seed(24)
    g, xn, orig = (torch.randn(B, L, D, generator=gen).cuda() for _ in range(3))
    g_mwo = torch.randn(B, D, generator=gen).cuda()
    for b, t in enumerate(LENS):
        g[b, t:] = NAN
        xn[b, t:] = NAN
        orig[b, t:] = NAN
    o = _jump_ctrl_bwd(C, g, xn, orig, f, inp[3], g_mwo, lens=lt, with_dxn=with_dxn)
    jumped = 0
    for b, t in enumerate(LENS):
        fa = _ctrl_alone(C, inp, b, t)
        a = _jump_ctrl_bwd(C, g[b:b + 1, :t].contiguous(), xn[b:b + 1, :t].contiguous(), orig[b:b + 1, :t].contiguous(),
                           fa, inp[3][b:b + 1].contiguous(), g_mwo[b:b + 1].contiguous(), with_dxn=with_dxn)
        for k in ("g_policy", "g_mem", "g_mem_w", "has_orig"):
            assert torch.equal(o[k][b:b + 1], a[k]), (k, b, t)
        if with_dxn:
            assert torch.equal(o["dxn"][b, :t], a["dxn"][0]) and not o["dxn"][b, t:].any(), (b, t)
        if float(f["beta"][b]) != 0.0:  # a jump: this pass is dorig's first writer
            jumped += 1
            assert torch.equal(o["dorig"][b, :t], a["dorig"][0]) and not o["dorig"][b, t:].any(), (b, t)
    assert jumped >= 1
    assert all(bool(torch.isfinite(o[k]).all()) for k in ("g_policy", "g_mem", "g_mem_w", "g_jump_s", "g_mg_w"))


def test_chain_with_zero_and_too_long(cuda):
    """A table holding 0 and L + 7 straight through the C-ABI, down the forward chain (row forward, control, jump
    select, the closing axpy) and the jump partials -> control backward: the empty sample's rows are all zero and
    everything about it finite (its means are 0), the overlong one gives the uniform kernels' full-length result."""
    from asrx import lib

    Lx, lens, D = 70, [0, 77, 37], KD
    lt = _tab(lens)
    W, C = _row_weights(), _ctrl_weights(D)
    x, SH = _row_inputs(lens, Lx)
    policy, gpol, _, mem_w, _ = _ctrl_inputs(lens, Lx, D)
    gen = torch.Generator().manual_seed(25)
    gate, hh = torch.rand(3, Lx, generator=gen).cuda(), torch.randn(3, Lx, D, generator=gen).cuda()
    g = torch.randn(3, Lx, D, generator=gen).cuda()
    g_mwo = torch.randn(3, D, generator=gen).cuda()

    def chain(xs, SHs, sl, table):
        r = _row_fwd3(W, xs, SHs, table)
        f = _ctrl_fwd(C, policy[sl].contiguous(), gpol[sl].contiguous(), r["ion"], mem_w[sl].contiguous(), r["part"],
                      lens=table)
        nb = xs.shape[0]
        xo, y = torch.full_like(xs, NAN), torch.full_like(xs, NAN)
        args = [_p(r["xnew"]), _p(xs), _p(xs), _p(f["active"]), _p(f["alpha"]), _p(f["beta"]), _p(f["gam"]), _p(xo)]
        if table is None:
            lib.call("asrx_jump_select4", *args, nb, Lx, D, lib.stream())
            lib.call("asrx_axpy_row", _p(xo), _p(gate[sl].contiguous()), _p(hh[sl].contiguous()), _p(y), nb * Lx, D,
                     lib.stream())
        else:
            lib.call("asrx_jump_lens_select4", *args, _p(table), nb, Lx, D, lib.stream())
            lib.call("asrx_axpy_lens_row", _p(xo), _p(gate[sl].contiguous()), _p(hh[sl].contiguous()), _p(y), _p(table),
                     nb, Lx, D, lib.stream())
        bw = _jump_ctrl_bwd(C, g[sl].contiguous(), r["xnew"], xs, f, mem_w[sl].contiguous(), g_mwo[sl].contiguous(),
                            lens=table)
        return r, f, xo, y, bw

    r, f, xo, y, bw = chain(x, SH, slice(0, 3), lt)
    # the empty sample: zero rows, zero means, everything finite
    for t in (r["px"], r["xnew"], r["ion"], r["g"], r["part"], xo, y, bw["dxn"]):
        assert not t[0].any()
    assert not f["mem"][0].any()
    for d in (f, bw):
        assert all(bool(torch.isfinite(v[0]).all()) for k, v in d.items() if v.is_floating_point() and v.shape[0] == 3
                   and k not in ("dorig", "dx"))
    # the overlong one: the uniform kernels on the sample alone at full length
    r1, f1, xo1, y1, bw1 = chain(x[1:2].contiguous(), SH[1:2].contiguous(), slice(1, 2), None)
    assert torch.equal(y[1:2], y1) and torch.equal(xo[1:2], xo1) and torch.equal(r["part"][1:2], r1["part"])
    for k in ("mem", "gam", "mwo", "alpha", "beta", "mem_v", "rec"):
        assert torch.equal(f[k][1:2], f1[k]), k
    for k in ("g_policy", "g_mem", "g_mem_w", "dxn"):
        assert torch.equal(bw[k][1:2], bw1[k]), k
    # and the short one still stops at its length
    assert not y[2, 37:].any() and bool(torch.isfinite(y).all())
