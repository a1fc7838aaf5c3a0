"""The MSheath layer backward without its carrier passes (asrx/msheath.py BWD_FUSED): the jump backward that stores
no dxn, the x_new backward from (g, alpha), the row backward's mode 2, the row forward without a px store and the
split-destination weight gradient, each against the kernel sequence it replaces, and the whole module with the
switch on and off.  (The issue's mode 1 -- the row backward forming g' on adapter layers -- measured no gain and is
not built; adapter layers run parts 1-2 ahead of the unchanged row backward, checked exactly here.)"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

LAYER = 1  # the layer index the kernel-level cases run at
SHAPES = [(D, B, L, M) for D in (128, 384, 1024) for B in (3, 4) for L in (30, 70) for M in (16, 64)]


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


@functools.lru_cache(maxsize=None)
def _case(D, B, L, M):
    """Random layer state through the C-ABI: the row forward's outputs (asrx_msheath_row_fwd3, with and without a px
    store) on random x / SH / weights, and random backward inputs.  Sample 1 is not at the layer; sample 0 is with
    beta = 0 (no jump), the others jump.  Built once per shape and left unchanged."""
    from asrx import lib

    dev = "cuda"
    g = torch.Generator().manual_seed(1000 * D + 100 * B + L + M)
    Dh, rows = D // 2, B * L
    N = M + Dh

    def rn(*s, scale=1.0):
        return (torch.randn(*s, generator=g) * scale).to(dev)

    c = dict(D=D, B=B, L=L, M=M, Dh=Dh, N=N, rows=rows)
    c["x"] = rn(B, L, D)
    c["lnw"], c["lnb"], c["gw"], c["gb"] = 1 + rn(D, scale=0.2), rn(D, scale=0.2), rn(D, scale=D ** -0.5), rn(1)
    c["SH"] = rn(rows, N)
    c["mval"], c["w2"], c["b2"] = rn(M), rn(Dh, scale=Dh ** -0.5), rn(1, scale=0.1)
    # the STE gate's potential cw0 kv + cw1 m2 + cb is spread around the threshold tx row by row (kv and m2 are
    # zero-mean in the random weights), so ion takes both values inside every sample
    c["cw"], c["cb"], c["tx"] = torch.tensor([0.8, 1.2], device=dev), rn(1, scale=0.02), torch.zeros(1, device=dev)
    c["next_i"] = torch.tensor([LAYER, LAYER + 1, LAYER, LAYER][:B], dtype=torch.float32, device=dev)
    c["active"] = (c["next_i"] == LAYER).float()
    nchunk = int(lib.load().asrx_mem_chunks(L))
    st = lib.stream()
    P = lib.ptr

    def fwd(with_px):
        o = {k: torch.full((rows,), 7.0, device=dev) for k in ("mean", "rstd", "nx", "g", "ion", "kv", "m2")}
        o["px"] = torch.full((B, L, D), 7.0, device=dev) if with_px else None
        o["x_new"] = torch.full((B, L, D), 7.0, device=dev)
        o["part"] = torch.full((B, nchunk, D), 7.0, device=dev)
        lib.call("asrx_msheath_row_fwd3", P(c["x"]), P(c["lnw"]), P(c["lnb"]), P(c["gw"]), P(c["gb"]), P(c["SH"]), N,
                 P(c["mval"]), P(c["w2"]), P(c["b2"]), P(c["cw"]), P(c["cb"]), P(c["tx"]), P(o["px"]), P(o["mean"]),
                 P(o["rstd"]), P(o["nx"]), P(o["g"]), P(o["ion"]), P(o["kv"]), P(o["m2"]), P(o["x_new"]), P(o["part"]),
                 rows, D, M, Dh, 1e-5, 1.0 / math.sqrt(D), P(c["next_i"]), LAYER, L, st)
        return o

    c["fwd"], c["fwd_nopx"] = fwd(True), fwd(False)
    c["gj"], c["x0"], c["dorig0"] = rn(B, L, D), rn(B, L, D), rn(B, L, D)
    c["alpha"] = rn(B)
    c["beta"] = torch.tensor([0.0, 0.4, 0.7, -0.3][:B], device=dev)
    c["g_mem"] = rn(B, D)
    c["dpx"], c["out"] = rn(B, L, D), rn(B, L, D)  # an adapter layer's dpx and update (any values)
    torch.cuda.synchronize()
    return c


def _jump(c, fused, has_orig, dxn):
    from asrx import lib

    P, B, L, D = lib.ptr, c["B"], c["L"], c["D"]
    dorig = c["dorig0"].clone()
    dx = torch.full((B, L, D), 7.0, device="cuda")
    part = torch.full((int(lib.load().asrx_jump_bwd_part_floats(B, L, D)),), 7.0, device="cuda")
    lib.call("asrx_jump_select4_bwd_part2" if fused else "asrx_jump_select4_bwd_part", P(c["gj"]),
             P(c["fwd"]["x_new"]), P(c["x0"]), P(c["active"]), P(c["alpha"]), P(c["beta"]), P(has_orig), P(dxn),
             P(dorig), P(dx), P(part), B, L, D, lib.stream())
    return dorig, dx, part


def _row_bwd(c, mode, dpx, dgv, dion, dx):
    """asrx_msheath_row_bwd (mode 0) / asrx_msheath_row_bwd2 -> dSH and the parameter gradients (dx in place)."""
    from asrx import lib

    P, D, M, Dh, N, rows, f = lib.ptr, c["D"], c["M"], c["Dh"], c["N"], c["rows"], c["fwd"]
    dSH = torch.full((rows, N), 7.0, device="cuda")
    pg = {k: torch.zeros(n, device="cuda") for k, n in (("dlnw", D), ("dlnb", D), ("dgw", D), ("dgb", 1), ("dmval", M),
                                                         ("dw2", Dh), ("db2", 1), ("dcw", 2), ("dcb", 1), ("db1", Dh))}
    args = (P(dpx), P(c["x"]), P(c["lnw"]), P(c["lnb"]), P(f["mean"]), P(f["rstd"]), P(dgv), P(f["g"]), P(c["gw"]),
            P(dion), P(c["SH"]), N, P(f["nx"]), P(c["mval"]), P(c["w2"]), P(c["cw"]), P(f["kv"]), P(f["m2"]), P(dx),
            P(pg["dlnw"]), P(pg["dlnb"]), P(pg["dgw"]), P(pg["dgb"]), P(dSH), P(pg["dmval"]), P(pg["dw2"]),
            P(pg["db2"]), P(pg["dcw"]), P(pg["dcb"]), P(pg["db1"]), rows, D, M, Dh, 1.0 / math.sqrt(D),
            P(c["next_i"]), LAYER, c["L"], lib.stream())
    if mode == 0:
        lib.call("asrx_msheath_row_bwd", *args)
    else:
        lib.call("asrx_msheath_row_bwd2", mode, P(c["gj"]), P(c["alpha"]), P(c["g_mem"]), 1.0 / c["L"], P(f["ion"]),
                 *args)
    return dSH, pg


def _old(c, has_orig, out, dpx):
    """The three-kernel sequence: jump backward (dxn stored) -> x_new backward -> row backward.  dpx None: the layer
    has no adapter and dpx is the x_new backward's dout."""
    from asrx import lib

    P, B, L, D, rows, f = lib.ptr, c["B"], c["L"], c["D"], c["rows"], c["fwd"]
    dxn = torch.full((B, L, D), 7.0, device="cuda")
    dorig, dx, part = _jump(c, False, has_orig, dxn)
    dout = torch.full((B, L, D), 7.0, device="cuda")
    dgv, dion = torch.full((rows,), 7.0, device="cuda"), torch.full((rows,), 7.0, device="cuda")
    lib.call("asrx_axpy_row2_bwd_acc", P(dxn), P(c["g_mem"]), 1.0 / L, P(c["active"]), P(f["g"]), P(f["ion"]), P(out),
             P(dout), P(dgv), P(dion), P(dx), B, L, D, lib.stream())
    dSH, pg = _row_bwd(c, 0, dout if dpx is None else dpx, dgv, dion, dx)
    return dict(dorig=dorig, dx=dx, part=part, dout=dout, dgv=dgv, dion=dion, dSH=dSH, pg=pg)


def _has_orig(c, v):
    return torch.full((c["B"],), v, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("D,B,L,M", SHAPES)
def test_adapter_sequence_is_bit_equal(cuda, D, B, L, M):
    """Adapter-layer form: asrx_jump_select4_bwd_part2 (no dxn) -> asrx_axpy_row2_bwd_acc2 (from g and alpha) ->
    asrx_msheath_row_bwd gives the old sequence's dout, dgv, dion, dSH, dx, dorig and partial sums bit for bit."""
    from asrx import lib

    c = _case(D, B, L, M)
    P, f = lib.ptr, c["fwd"]
    for ho in (0, 1):
        has_orig = _has_orig(c, ho)
        old = _old(c, has_orig, c["out"], c["dpx"])
        dorig, dx, part = _jump(c, True, has_orig, None)
        dout = torch.full((B, L, D), 7.0, device="cuda")
        dgv, dion = torch.full((B * L,), 7.0, device="cuda"), torch.full((B * L,), 7.0, device="cuda")
        lib.call("asrx_axpy_row2_bwd_acc2", P(c["gj"]), P(c["alpha"]), P(c["g_mem"]), 1.0 / L, P(c["active"]),
                 P(f["g"]), P(f["ion"]), P(c["out"]), P(dout), P(dgv), P(dion), P(dx), B, L, D, lib.stream())
        dSH, _ = _row_bwd(c, 0, c["dpx"], dgv, dion, dx)
        new = dict(dorig=dorig, dx=dx, part=part, dout=dout, dgv=dgv, dion=dion, dSH=dSH)
        torch.cuda.synchronize()
        for k, v in new.items():
            assert torch.equal(v, old[k]), (k, ho)
        assert bool(torch.isfinite(dx).all()) and torch.equal(dx[1], c["gj"][1])  # off the layer: the pass-through


@pytest.mark.parametrize("D,B,L,M", SHAPES)
def test_mode2_matches_sequence(cuda, D, B, L, M):
    """No-adapter form: the jump backward without dxn, then asrx_msheath_row_bwd2 mode 2 alone (px recomputed, the
    x_new backward inside), against the old sequence with out = px from asrx_msheath_row_fwd3 and dpx = dout.  The
    only difference is the order of the per-row sum t = g' . px (lane layout of the row kernel instead of float4
    strides), so dSH and dx agree to fp32 rounding: gate 1e-4 of the tensor's max (test_msheath's input-gradient
    gate).  Measured on MI355X over these cases: at most 1.24e-7 (dx) and 2.1e-7 (dSH).  Two runs are bit-equal (no
    atomics on the data path)."""
    c = _case(D, B, L, M)
    for ho in (0, 1):
        has_orig = _has_orig(c, ho)
        old = _old(c, has_orig, c["fwd"]["px"], None)
        runs = []
        for _ in range(2):
            dorig, dx, part = _jump(c, True, has_orig, None)
            dSH, pg = _row_bwd(c, 2, None, None, None, dx)
            runs.append((dx, dSH, pg))
        torch.cuda.synchronize()
        (dx, dSH, pg), (dx2, dSH2, _) = runs
        assert torch.equal(dx, dx2) and torch.equal(dSH, dSH2)
        assert torch.equal(dorig, old["dorig"]) and torch.equal(part, old["part"])
        e_dx, e_sh = _rel(dx, old["dx"]), _rel(dSH, old["dSH"])
        print(f"mode 2 vs sequence D={D} B={B} L={L} M={M} has_orig={ho}: dx {e_dx:.2e} dSH {e_sh:.2e}")
        assert e_dx <= 1e-4 and e_sh <= 1e-4, (e_dx, e_sh)
        assert torch.equal(dx[1], c["gj"][1]) and not bool(dSH[L:2 * L].any())  # sample 1 is not at the layer
        for k, v in pg.items():  # parameter gradients (float atomics in both): same gate as the module test
            assert _rel(v, old["pg"][k]) < 2e-3, k


@pytest.mark.parametrize("D,B,L,M", SHAPES)
def test_row_fwd3_without_px(cuda, D, B, L, M):
    c = _case(D, B, L, M)
    a, b = c["fwd"], c["fwd_nopx"]
    for k in ("x_new", "part", "mean", "rstd", "nx", "g", "ion", "kv", "m2"):
        assert torch.equal(a[k], b[k]), k
    assert 0 < float(a["ion"][:L].sum()) < L  # both branches of the STE gate occur in a sample at the layer


def _bf(t):
    return t.to(torch.bfloat16).double()


@pytest.mark.parametrize("splitk", [1, 4, None])
@pytest.mark.parametrize("msplit,M,N", [(64, 256, 384), (16, 80, 128)])
@pytest.mark.parametrize("R", [37, 4100])
def test_wgrad_split(cuda, R, msplit, M, N, splitk):
    """asrx_wgrad_split (two destinations, one pass) against two wgrad_cols calls and against float64 on the
    bf16-rounded operands, accumulating into pre-filled destinations; tolerance and normalisation of
    test_wgrad_bf16_register_staged.  splitk None: through gemm.wgrad_cols2 (its own split-K choice)."""
    from asrx import gemm as G, lib, prec

    g = torch.Generator().manual_seed(R + M)
    dy, x = torch.randn(R, M, generator=g), torch.randn(R, N, generator=g)
    w0, w1 = torch.randn(msplit, N, generator=g), torch.randn(M - msplit, N, generator=g)
    dyc, xc = dy.to(cuda), x.to(cuda)
    o0, o1, r0, r1 = w0.to(cuda), w1.to(cuda), w0.to(cuda), w1.to(cuda)
    with prec.precision("bf16"):
        if splitk is None:
            G.wgrad_cols2(dyc, msplit, o0, o1, xc)
        else:
            lib.call("asrx_wgrad_split", lib.ptr(dyc), M, lib.ptr(xc), 0, N, lib.ptr(o0), N, lib.ptr(o1), N, msplit, M,
                     N, R, splitk, lib.stream())
        G.wgrad_cols(dyc, 0, msplit, xc, r0)
        G.wgrad_cols(dyc, msplit, M - msplit, xc, r1)
    torch.cuda.synchronize()
    ref = torch.cat([w0, w1]).double() + _bf(dy).t() @ _bf(x)
    scale = (_bf(dy).t().abs() @ _bf(x).abs()).max()
    got, two = torch.cat([o0, o1]).cpu().double(), torch.cat([r0, r1]).cpu().double()
    assert float((got - ref).abs().max() / scale) < 1e-5
    assert float((got - two).abs().max() / scale) < 1e-5


def _module_runs(monkeypatch, D, B, L, precision):
    """MSheath(D, 2, 4) as test_msheath sets it up (concat bias spread, one damped sample): output, input gradient
    and parameter gradients with BWD_FUSED on and off."""
    from asrx import msheath as ms
    from asrx import prec
    from asrx.model import MSheath
    from asrx.noise import NoiseCtx

    torch.manual_seed(3)
    layer = 4
    mod = MSheath(D, 2, layer).cuda()
    mod.fused = True
    with torch.no_grad():
        for i in range(layer):
            mod.layers[i]["v_gate"].concat.bias.fill_(0.3 + 0.1 * (i - 1))
    x = torch.randn(B, L, D)
    x[1] *= 0.1
    gout = torch.randn(B, L, D, generator=torch.Generator().manual_seed(0)).cuda()

    def run(on):
        monkeypatch.setattr(ms, "BWD_FUSED", on)
        for p in mod.parameters():
            p.grad = None
        xi = x.cuda().requires_grad_(True)
        with prec.precision(precision):
            y = mod.run(xi, NoiseCtx(9, 1, True), "t.jump", 5)
            y.backward(gout)
        torch.cuda.synchronize()
        return y.detach(), xi.grad, {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None}

    return run(True), run(False)


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("D", [128, 384])
@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("L", [30, 70])
def test_module_switch_on_off(cuda, monkeypatch, D, B, L, det):
    """fp32 parity mode, BWD_FUSED on and off: equal output, input gradient within 1e-4 of its max, parameter
    gradients within 2e-3 (test_msheath's gates).  det False: the jump backward's atomic form
    (asrx_jump_select4_bwd_acc2 with no dxn)."""
    from asrx import msheath as ms

    monkeypatch.setattr(ms, "DETERMINISTIC", det)
    (y1, g1, p1), (y0, g0, p0) = _module_runs(monkeypatch, D, B, L, "fp32")
    assert torch.equal(y1, y0)
    assert _rel(g1, g0) < 1e-4, _rel(g1, g0)
    assert p1.keys() == p0.keys() and len(p0) > 40
    for n in p0:
        assert _rel(p1[n], p0[n]) < 2e-3, (n, _rel(p1[n], p0[n]))


@pytest.mark.parametrize("B,L", [(3, 70), (4, 30)])
def test_module_switch_on_off_bf16(cuda, monkeypatch, B, L):
    """bf16 perf mode at D = 384, where the backward goes through gemm.wgrad_cols2 -> asrx_wgrad_split.  On and off
    feed the bf16 GEMMs a dSH that differs by fp32 rounding (mode 2, <= 2.1e-7), so an operand can land on the
    neighbouring bf16 value: one such step is 2^-8 of the operand, and no result may move by more than that share of
    its tensor's largest element (the other differences, fp32 atomics' order, are four orders below).  The forward
    is untouched: equal output."""
    from asrx import lib

    calls = []
    real = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    (y1, g1, p1), (y0, g0, p0) = _module_runs(monkeypatch, 384, B, L, "bf16")
    assert calls.count("asrx_wgrad_split") == 4 and "asrx_msheath_row_bwd" in calls  # one per layer; off: the old path
    assert torch.equal(y1, y0)
    assert _rel(g1, g0) <= 2.0 ** -8, _rel(g1, g0)
    assert p1.keys() == p0.keys() and len(p0) > 40
    for n in p0:
        print(f"bf16 on/off B={B} L={L} {n}: {_rel(p1[n], p0[n]):.2e}")
        assert _rel(p1[n], p0[n]) <= 2.0 ** -8, (n, _rel(p1[n], p0[n]))
