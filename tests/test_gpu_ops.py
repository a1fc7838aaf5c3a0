"""Per-op parity of the HIP kernels (fp32 parity mode) against the oracle restatement (float64 CPU).
Forward values and gradients (the oracle's autograd) are compared on the same inputs and the same
keyed noise."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import keys as K
from oracle import model as om

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fp32():
    from asrx import prec

    with prec.precision("fp32"):
        yield


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _grads(fn_gpu, fn_ref, inputs, gout_seed=0):
    """Run fn on GPU tensors and CPU float64 leaves; backprop the same random cotangent."""
    g_in = [t.detach().to("cuda").requires_grad_(t.is_floating_point()) for t in inputs]
    r_in = [t.detach().double().requires_grad_(t.is_floating_point()) for t in inputs]
    yg = fn_gpu(*g_in)
    yr = fn_ref(*r_in)
    gout = torch.randn(yr.shape, generator=torch.Generator().manual_seed(gout_seed), dtype=torch.float64)
    yg.backward(gout.float().cuda())
    yr.backward(gout)
    return yg, yr, [t.grad for t in g_in], [t.grad for t in r_in]


@pytest.mark.parametrize("d,H", [(128, 1), (384, 1), (64, 3), (128, 4), (512, 1)])
def test_abby_normal(cuda, d, H):
    from asrx import ops
    from asrx.model import AbbyNormal

    torch.manual_seed(0)
    mod = AbbyNormal(d).cuda()
    B, L = 2, 37
    x = torch.randn(B, L, H, d) * 3.0 if H > 1 else torch.randn(B, L, d) * 3.0
    x[0, 0] *= 40.0  # make max-pool mode and large |x| rows show up
    P = {f"n.{k}": v.detach().cpu() for k, v in mod.state_dict().items()}
    seed, step, site, sid_base = 5, 2, "t.abby", 3
    key = K.site_key(seed, step, site)
    noise = om.Noise(seed, step, torch.float64)
    sids = [sid_base + b for b in range(B)]

    def ref(xr, w0, b0, w2, b2, nz=noise, PS=None):
        PP = dict(P if PS is None else PS)
        PP.update({"n.mode_router.0.weight": w0, "n.mode_router.0.bias": b0, "n.mode_router.2.weight": w2,
                   "n.mode_router.2.bias": b2})
        g = nz.abby(site, sids, H, L)  # (B, H, L, 3)
        g = g.permute(0, 2, 1, 3) if H > 1 else g[:, 0]
        return om.abby_normal(PP, "n", xr, g)

    def gpu(xg, w0, b0, w2, b2):
        return ops.AbbyNormalFn.apply(xg, w0, b0, w2, b2, L, H, sid_base, key, True, True)

    r = mod.mode_router
    ins = [x, r[0].weight.detach().cpu(), r[0].bias.detach().cpu(), r[2].weight.detach().cpu(),
           r[2].bias.detach().cpu()]
    yg, yr, gg, gr = _grads(gpu, ref, ins)
    assert _rel(yg, yr) < 1e-5
    assert _rel(gg[0], gr[0]) < 1e-4
    # weight gradients are sums over rows that include a 40x outlier row: fp32 accumulation error is
    # ~1e-7 * sum|terms|, i.e. relative to max|grad| it scales with the cancellation in the sum.  The
    # yardstick is the same restatement run in float32 on the CPU (its own rounding error against
    # float64): the HIP gradients must be within 2e-3, or within 20x that fp32 CPU error
    n32 = om.Noise(seed, step, torch.float32)
    r32 = [t.detach().float().requires_grad_(True) for t in ins]
    y32 = ref(*r32, nz=n32, PS={k: v.float() for k, v in P.items()})
    y32.backward(torch.randn(yr.shape, generator=torch.Generator().manual_seed(0), dtype=torch.float64).float())
    for a, b, c in zip(gg[1:], gr[1:], r32[1:]):
        e, e32 = _rel(a, b), _rel(c.grad, b)
        assert e < max(2e-3, 20 * e32), (e, e32)


def test_layer_norm(cuda):
    from asrx import ops

    x = torch.randn(5, 33, 192) * 2 + 1
    w, b = torch.randn(192), torch.randn(192)
    yg, yr, gg, gr = _grads(lambda a, c, d: ops.layer_norm(a, c, d), lambda a, c, d: F.layer_norm(a, (192,), c, d),
                            [x, w, b])
    assert _rel(yg, yr) < 1e-5
    for a, c in zip(gg, gr):
        assert _rel(a, c) < 1e-4


@pytest.mark.parametrize("Lq,Lk,causal,hd", [(101, 101, False, 64), (8, 101, False, 64), (70, 70, True, 64),
                                             (130, 3, False, 64), (64, 64, True, 64), (101, 101, False, 128),
                                             (70, 70, True, 128), (8, 130, False, 128)])
def test_attention(cuda, Lq, Lk, causal, hd):
    """Exact-fp32 parity-mode attention (hd 64 and the reference config's hd 128, model.py:746)
    against float64 softmax attention: output and q/k/v gradients."""
    from asrx import ops

    B, H = 2, 3
    g = torch.Generator().manual_seed(Lq + Lk)
    q = torch.randn(B, Lq, H, hd, generator=g)
    k = torch.randn(B, Lk, H, hd, generator=g)
    v = torch.randn(B, Lk, H, hd, generator=g)

    def ref(q, k, v):
        s = (q.transpose(1, 2) @ k.transpose(1, 2).transpose(-1, -2)) / math.sqrt(hd)
        if causal:
            s = s.masked_fill(torch.ones(Lq, Lk, dtype=torch.bool).triu(1), float("-inf"))
        return (torch.softmax(s, -1) @ v.transpose(1, 2)).transpose(1, 2)

    yg, yr, gg, gr = _grads(lambda a, b, c: ops.attention(a, b, c, causal), ref, [q, k, v])
    assert _rel(yg, yr) < 1e-5
    for a, b in zip(gg, gr):
        assert _rel(a, b) < 1e-4


@pytest.mark.parametrize("B,H,Lq,Lk,causal,hd", [(1, 2, 300, 300, False, 64), (2, 3, 600, 517, False, 64),
                                                   (1, 2, 256, 256, True, 64), (2, 1, 70, 70, True, 64),
                                                   (1, 2, 33, 3001, False, 64), (1, 1, 513, 64, False, 64),
                                                   (2, 2, 300, 517, False, 128), (1, 2, 256, 256, True, 128),
                                                   (1, 1, 33, 3001, False, 128)])
def test_attention_bf16(cuda, B, H, Lq, Lk, causal, hd):
    """Perf-mode flash attention (32x32x16 bf16 MFMA, transposed-read V) against float64 softmax
    attention on the same bf16-rounded q, k, v: output and log-sum-exp (hd 64 and 128)."""
    from asrx import lib, prec

    g = torch.Generator().manual_seed(Lq * 3 + Lk + causal)
    q, k, v = (torch.randn(B, L, H, hd, generator=g) for L in (Lq, Lk, Lk))
    o = torch.empty(B, Lq, H, hd, device=cuda)
    lse = torch.empty(B, H, Lq, device=cuda)
    qg, kg, vg = q.to(cuda), k.to(cuda), v.to(cuda)
    st = lambda t: (ctypes_arr(t.stride(0), t.stride(1), t.stride(2)))  # noqa: E731
    import ctypes

    def ctypes_arr(*s):
        return (ctypes.c_int64 * 3)(*s)

    lib.call("asrx_attn_fwd", 1, lib.ptr(qg), st(qg), lib.ptr(kg), st(kg), lib.ptr(vg), st(vg), lib.ptr(o), st(o),
             lib.ptr(lse), B, H, Lq, Lk, hd, int(causal), 1.0 / math.sqrt(hd), lib.stream())
    bq, bk, bv = (t.to(torch.bfloat16).double().transpose(1, 2) for t in (q, k, v))
    s = bq @ bk.transpose(-1, -2) / math.sqrt(hd)
    if causal:
        s = s.masked_fill(torch.ones(Lq, Lk, dtype=torch.bool).triu(1), float("-inf"))
    ref_lse = torch.logsumexp(s, -1)
    ref = (torch.softmax(s, -1) @ bv).transpose(1, 2)
    assert _rel(o, ref) < 1e-2
    assert float((lse.cpu().double() - ref_lse).abs().max()) < 1e-3


@pytest.mark.parametrize("B,H,Lq,Lk,causal,hd", [(1, 2, 300, 300, False, 64), (2, 3, 600, 517, False, 64),
                                                   (1, 2, 256, 256, True, 64), (2, 1, 70, 70, True, 64),
                                                   (1, 2, 33, 3001, False, 64), (1, 1, 513, 64, False, 64),
                                                   (1, 2, 700, 700, True, 64), (2, 2, 300, 517, False, 128),
                                                   (1, 2, 700, 700, True, 128), (1, 1, 33, 3001, False, 128)])
def test_attention_bf16_backward(cuda, B, H, Lq, Lk, causal, hd):
    """Perf-mode flash-attention backward (dkdv kernel with the key on the lane, dq kernel with the
    query on the lane, 32x32x16 bf16 MFMA) against float64 autograd of softmax attention on the
    same bf16-rounded q, k, v, dO.  P and dS are rounded to bf16 before their products, so the
    tolerance is the bf16 one (3e-2 of max |grad|)."""
    from asrx import ops, prec

    g = torch.Generator().manual_seed(Lq * 5 + Lk + causal)
    q, k, v = (torch.randn(B, L, H, hd, generator=g) for L in (Lq, Lk, Lk))
    dO = torch.randn(B, Lq, H, hd, generator=g)
    rnd = lambda t: t.to(torch.bfloat16).float()  # noqa: E731
    q, k, v, dO = rnd(q), rnd(k), rnd(v), rnd(dO)
    qg, kg, vg = (t.to(cuda).requires_grad_(True) for t in (q, k, v))
    with prec.precision("bf16"):
        o = ops.attention(qg, kg, vg, causal)
        o.backward(dO.to(cuda))
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    s = (qr.transpose(1, 2) @ kr.transpose(1, 2).transpose(-1, -2)) / math.sqrt(hd)
    if causal:
        s = s.masked_fill(torch.ones(Lq, Lk, dtype=torch.bool).triu(1), float("-inf"))
    ref = (torch.softmax(s, -1) @ vr.transpose(1, 2)).transpose(1, 2)
    ref.backward(dO.double())
    assert _rel(o.detach(), ref.detach()) < 1e-2
    for a, b in ((qg.grad, qr.grad), (kg.grad, kr.grad), (vg.grad, vr.grad)):
        assert _rel(a, b) < 3e-2, _rel(a, b)


@pytest.mark.parametrize("masked", [False, True])
def test_rotary(cuda, masked):
    from asrx import ops
    from asrx.model import rotary_freqs

    B, L, H, hd = 2, 50, 3, 64
    D = H * hd
    x = torch.randn(B, L, D)
    src = torch.randn(B, L, D)
    scale = hd ** -0.25
    f = rotary_freqs(D, H, masked, "cuda")

    def ref(x, src):
        xq = (x * scale).view(B, L, H, hd).permute(0, 2, 1, 3)
        return om.rotary(xq, src, D, H, masked).permute(0, 2, 1, 3).reshape(B, L, D)

    yg, yr, gg, gr = _grads(lambda a, s: ops.rotary(a, s, f, hd, scale), ref, [x, src])
    assert _rel(yg, yr) < 1e-5
    for a, b in zip(gg, gr):
        assert _rel(a, b) < 1e-4


def test_v_gate(cuda):
    from asrx import ops
    from asrx.model import v_gate

    torch.manual_seed(1)
    D = 128
    mod = v_gate(D, mem=64, thresh=0.3).cuda()
    x = torch.randn(2, 40, D)
    P = {f"v.{k}": v.detach().cpu().double() for k, v in mod.state_dict().items()}

    def ref(xr):
        ion, xval = om.v_gate(P, "v", xr)
        return ion[..., 0] + 0.0 * xval[..., 0]

    def gpu(xg):
        return ops.v_gate(mod, xg)

    yg, yr, gg, gr = _grads(gpu, ref, [x])
    assert torch.equal(yg.detach().cpu().double(), yr.detach())
    assert _rel(gg[0], gr[0]) < 1e-4
    # parameter gradients
    mod.zero_grad()
    yg2 = ops.v_gate(mod, x.cuda())
    go = torch.randn(yg2.shape)
    yg2.backward(go.cuda())
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items() if k != "v.tx"}
    Pr["v.tx"] = P["v.tx"]
    ion, _ = om.v_gate(Pr, "v", x.double())
    ion[..., 0].backward(go.double())
    for name in ["mkey", "mval", "mlp.0.weight", "mlp.2.weight", "concat.weight", "concat.bias"]:
        pg = dict(mod.named_parameters())[name].grad
        assert _rel(pg, Pr["v." + name].grad) < 1e-4, name


def test_tgate(cuda):
    from asrx import ops
    from asrx.model import tgate

    torch.manual_seed(2)
    D = 128
    mod = tgate(D, num_types=3).cuda()
    x = torch.randn(3, 21, D)
    P = {f"t.{k}": v.detach().cpu().double().requires_grad_(True) for k, v in mod.state_dict().items()}
    yg, yr, gg, gr = _grads(lambda a: ops.tgate(mod, a), lambda a: om.tgate(P, "t", a), [x])
    assert _rel(yg, yr) < 1e-5
    assert _rel(gg[0], gr[0]) < 1e-4
    # the three gates' weight / bias gradients land in their own p.grad (no cat backward)
    for n, p in mod.named_parameters():
        assert p.grad is not None, n
        assert _rel(p.grad, P[f"t.{n}"].grad) < 1e-4, n


def test_conv3_weight_norm(cuda):
    """weight_norm(Conv1d(C, C, 3)) (model.py:140) through ops.conv3: g / v read directly (no torch
    parametrization), forward and gradients of x, g, v, b against float64 torch."""
    from asrx import ops
    from torch.nn.utils.parametrizations import weight_norm

    torch.manual_seed(4)
    C, O, B, T = 64, 96, 2, 33
    conv = weight_norm(torch.nn.Conv1d(C, O, kernel_size=3, padding=1))
    with torch.no_grad():
        conv.parametrizations.weight.original0.mul_(torch.rand(O, 1, 1) + 0.5)
    ref = weight_norm(torch.nn.Conv1d(C, O, kernel_size=3, padding=1)).double()
    ref.load_state_dict({k: v.double() for k, v in conv.state_dict().items()})
    conv = conv.cuda()
    x = torch.randn(B, T, C)
    go = torch.randn(B, T, O)
    xg = x.cuda().requires_grad_(True)
    y = ops.conv3(xg, conv)
    y.backward(go.cuda())
    xr = x.double().requires_grad_(True)
    yr = ref(xr.transpose(1, 2)).transpose(1, 2)
    yr.backward(go.double())
    assert _rel(y, yr) < 1e-5
    assert _rel(xg.grad, xr.grad) < 1e-5
    pg = dict(conv.named_parameters())
    for n, p in ref.named_parameters():
        assert _rel(pg[n].grad, p.grad) < 1e-4, n


def test_cross_entropy_device_mean(cuda):
    """F.cross_entropy(ignore_index=0) (model.py:670): one-pass log-sum-exp, on-device mean and count,
    backward scaled by the device gradient; rows with label 0 ignored."""
    from asrx import ops

    torch.manual_seed(6)
    R, V = 37, 1003
    z = torch.randn(R, V) * 4
    lab = torch.randint(1, V, (R,))
    lab[::5] = 0
    zg = z.cuda().requires_grad_(True)
    loss = ops.CrossEntropy.apply(zg, lab.cuda())
    (loss * 2.5).backward()
    zr = z.double().requires_grad_(True)
    lr = F.cross_entropy(zr, lab, ignore_index=0)
    (lr * 2.5).backward()
    assert abs(float(loss) - float(lr)) < 1e-5 * max(1.0, abs(float(lr)))
    assert _rel(zg.grad, zr.grad) < 1e-5


def test_blend(cuda):
    from asrx import ops

    torch.manual_seed(7)
    d, g = torch.randn(2, 9, 64), torch.randn(2, 9, 64)
    bl = torch.nn.Parameter(torch.tensor(0.3).cuda())
    dg_, gg_ = d.cuda().requires_grad_(True), g.cuda().requires_grad_(True)
    out = ops.blend(dg_, gg_, bl)
    go = torch.randn(out.shape)
    out.backward(go.cuda())
    dr, gr_ = d.double().requires_grad_(True), g.double().requires_grad_(True)
    br = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
    s = torch.sigmoid(br)
    outr = s * dr + (1 - s) * gr_
    outr.backward(go.double())
    assert _rel(out, outr) < 1e-6
    assert _rel(dg_.grad, dr.grad) < 1e-6 and _rel(gg_.grad, gr_.grad) < 1e-6
    assert abs(float(bl.grad) - float(br.grad)) < 1e-4 * max(1.0, abs(float(br.grad)))


def test_fork_sink_and_stream_groups(cuda):
    """ops.fork: consumers that accumulate into the sink (AbbyNormal, Linear, rotary |src|) plus one
    that returns its gradient normally give x the summed gradient; split_rows / group: the views of a
    stream group map back to the group tensor, and their gradients are joined in one kernel."""
    from asrx import ops
    from asrx.model import AbbyNormal

    torch.manual_seed(8)
    D, B, L = 128, 2, 19
    ab = AbbyNormal(D).cuda()
    W = torch.randn(D, D, device="cuda") / D ** 0.5
    f = torch.rand(D // 4, device="cuda")
    x0 = torch.randn(B, L, D, device="cuda")

    def run(use_fork):
        x = x0.clone().requires_grad_(True)
        h = ops.fork(x) if use_fork else x
        y = ops.abby_normal(ab, h, L, 1, 0, 0, False).sum() + ops.linear(h, W).pow(2).sum()
        y = y + ops.rotary(ops.linear(h, W), h, f, 64, 0.5).sum() + (h * h).sum()
        y.backward()
        return x.grad

    assert _rel(run(True), run(False)) < 1e-5
    z = torch.randn(3 * B, L, D, device="cuda", requires_grad=True)
    parts = ops.split_rows(z * 1.0, 3)
    assert ops.group(parts) is parts[0]._asrx_group[0] and ops.group(parts[1:]).shape == (2 * B, L, D)
    w = torch.randn(3, device="cuda")
    (parts[0].sum() * w[0] + parts[1].pow(2).sum() * w[1] + parts[2].sum() * w[2]).backward()
    ref = torch.cat([torch.full((B, L, D), float(w[0]), device="cuda"), 2 * float(w[1]) * z[B:2 * B].detach(),
                     torch.full((B, L, D), float(w[2]), device="cuda")])
    assert _rel(z.grad, ref) < 1e-6


@pytest.mark.parametrize("fused,D,B", [(True, 128, 4), (True, 384, 4), (True, 384, 3), (False, 128, 4),
                                       (False, 192, 4)])
def test_msheath(cuda, fused, D, B):
    """MSheath (model.py:387-507), the fused single-node path (asrx/msheath.py, hand-written backward)
    and the per-op composition, against the oracle's per-sample while-loop: output, input gradient and
    every parameter's gradient, with potentials spread around the 0.1 threshold so samples take
    different layer/jump trajectories."""
    from asrx import ops  # noqa: F401
    from asrx.model import MSheath
    from asrx.noise import NoiseCtx

    from asrx import msheath as ms

    torch.manual_seed(3)
    layer = 4
    mod = MSheath(D, 2, layer).cuda()
    mod.fused = fused
    assert ms.supported(mod, D) == (D in ms.ROW_DIMS)  # D=192: the composed path (no fused row kernel)
    with torch.no_grad():
        for i in range(layer):  # spread x_val around the 0.3 threshold so potentials vary per sample
            mod.layers[i]["v_gate"].concat.bias.fill_(0.3 + 0.1 * (i - 1))
    L = 30  # B = 3: an odd sample count (the row pass's LDS layout after the per-sample next_i copy)
    x = torch.randn(B, L, D)
    x[1] *= 0.1
    trainable = {n for n, p in mod.named_parameters() if p.requires_grad}  # v_gate.tx is frozen
    P = {f"j.{k}": v.detach().cpu().double().requires_grad_(k in trainable) for k, v in mod.state_dict().items()}
    seed, step, site, sid_base = 9, 1, "t.jump", 5
    noise = NoiseCtx(seed, step, True)
    onoise = om.Noise(seed, step, torch.float64)
    gpol = onoise.policy(site, [sid_base + b for b in range(B)], layer)
    yg, yr, gg, gr = _grads(lambda a: mod.run(a, noise, site, sid_base),
                            lambda a: om.msheath(P, "j", a, layer, gpol), [x])
    assert _rel(yg, yr) < 1e-5
    assert _rel(gg[0], gr[0]) < 1e-4
    pn = dict(mod.named_parameters())
    checked = 0
    for n, p in pn.items():
        ref = P[f"j.{n}"].grad
        if not p.requires_grad or ref is None or n.startswith("shared_head"):
            continue
        assert p.grad is not None, n
        assert _rel(p.grad, ref) < 2e-3, (n, _rel(p.grad, ref))
        checked += 1
    assert checked > 40


def test_encoder_stream(cuda):
    from asrx.model import AudioEncoder
    from asrx.noise import NoiseCtx

    torch.manual_seed(4)
    D, layers = 128, 2
    enc = AudioEncoder(128, D, 2, layers, "gelu", "AbbyNormal").cuda().train()
    B, T = 2, 101
    spec = torch.randn(B, 128, T)
    pitch = torch.rand(B, 1, T) * 100
    wav = torch.randn(B, 1, T - 1)
    seed, step = 11, 0
    noise = NoiseCtx(seed, step, True)
    P = {f"enc.{k}": v.detach().cpu().double() for k, v in enc.state_dict().items()}
    # weight_norm's computed weight is not in the state dict; the oracle recomputes it from g, v
    outs = enc.encode([pitch.cuda(), spec.cuda(), wav.cuda()], noise, B)
    onoise = om.Noise(seed, step, torch.float64)
    for s, src in enumerate([pitch, spec, wav]):
        ref = om.encode_stream(P, src.double(), layers, onoise, [s * B + b for b in range(B)], True)
        assert _rel(outs[s], ref) < 1e-5, s


@pytest.mark.parametrize("K,C,T", [(3, 384, 101), (15, 128, 517), (15, 384, 16), (7, 6, 33), (5, 64, 1)])
def test_dwconv(cuda, K, C, T):
    """Depthwise conv (ConvLite.depth model.py:101, encoder k3 model.py:147) on channels-last input:
    forward, input and weight/bias gradients vs torch float64 conv1d(groups=C) -- the tiled float4
    kernels for C % 4 == 0 and the generic kernels otherwise (C = 6)."""
    from asrx import ops

    torch.manual_seed(K * 1000 + C + T)
    B = 3
    x = torch.randn(B, T, C)
    w = torch.randn(C, 1, K) * 0.3
    b = torch.randn(C)

    def ref(x, w, b):
        return F.conv1d(x.transpose(1, 2), w, b, padding=K // 2, groups=C).transpose(1, 2)

    yg, yr, gg, gr = _grads(ops.DWConv.apply, ref, [x, w, b])
    assert _rel(yg, yr) < 1e-5
    for a, r in zip(gg, gr):
        assert _rel(a, r) < 1e-5


@pytest.mark.parametrize("C,T", [(384, 301), (128, 3001), (6, 40)])
def test_batchnorm_per_sample(cuda, C, T):
    """ConvLite.bn (model.py:103, 114) in train mode at the reference's batch 1, applied per clip:
    forward and gradients vs torch float64 batch_norm on each clip separately."""
    from asrx import ops

    torch.manual_seed(C + T)
    B = 3
    x = torch.randn(B, T, C) * 2 + 5  # offset mean: exercises the one-pass (Welford) statistics
    w = torch.rand(C) + 0.5
    b = torch.randn(C)

    def ref(x, w, b):
        outs = [F.batch_norm(x[i:i + 1].transpose(1, 2), None, None, w, b, training=True, eps=1e-5).transpose(1, 2)
                for i in range(B)]
        return torch.cat(outs)

    yg, yr, gg, gr = _grads(lambda x, w, b: ops.BatchNormPS.apply(x, w, b, 1e-5, None), ref, [x, w, b])
    assert _rel(yg, yr) < 1e-5
    for a, r in zip(gg, gr):
        assert _rel(a, r) < 2e-5


def _e4m3_rows(t):
    """Per-row e4m3 quantisation of the fp8 attention mode (attn_f8.hip): x / s rounded to OCP
    e4m3 (RNE), s = max|x_row| / 448; returns the dequantised values s * e4m3(x / s)."""
    s = t.abs().amax(-1, keepdim=True) / 448.0
    s = torch.where(s > 0, s, torch.ones_like(s))
    return (t / s).to(torch.float8_e4m3fn).to(torch.float32) * s


@pytest.mark.parametrize("B,H,Lq,Lk,causal,hd", [(1, 2, 300, 300, False, 64), (2, 3, 600, 517, False, 64),
                                                   (1, 2, 256, 256, True, 64), (2, 1, 70, 70, True, 64),
                                                   (1, 2, 33, 3001, False, 64), (1, 1, 513, 64, False, 64),
                                                   (2, 2, 1, 77, False, 64), (2, 2, 300, 517, False, 128),
                                                   (1, 2, 256, 256, True, 128), (2, 1, 1, 77, False, 128)])
def test_attention_fp8(cuda, B, H, Lq, Lk, causal, hd):
    """fp8 attention mode (prec 2: e4m3 QK^T with per-row scales, bf16 P and V) against float64
    softmax attention on the same per-row e4m3-quantised q, k and bf16 v (tight: the kernel computes
    exactly that), and, on unit-variance inputs (scores of std ~1, as after the model's hd^-0.25 and
    AbbyNormal), against the unquantised inputs: the accuracy cost of the mode, stated tolerance
    5e-2 relative Frobenius error of o."""
    import ctypes

    from asrx import lib

    sc = 1.0 / math.sqrt(hd)
    g = torch.Generator().manual_seed(Lq * 7 + Lk + causal)

    def st(t):
        return (ctypes.c_int64 * 3)(t.stride(0), t.stride(1), t.stride(2))

    def run(q, k, v):
        o = torch.empty(B, Lq, H, hd, device=cuda)
        lse = torch.empty(B, H, Lq, device=cuda)
        qg, kg, vg = q.to(cuda), k.to(cuda), v.to(cuda)
        lib.call("asrx_attn_fwd", 2, lib.ptr(qg), st(qg), lib.ptr(kg), st(kg), lib.ptr(vg), st(vg), lib.ptr(o),
                 st(o), lib.ptr(lse), B, H, Lq, Lk, hd, int(causal), sc, lib.stream())
        torch.cuda.synchronize()
        return o, lse

    def ref(qq, kk, vv):
        s = qq.double().transpose(1, 2) @ kk.double().transpose(1, 2).transpose(-1, -2) * sc
        if causal:
            s = s.masked_fill(torch.ones(Lq, Lk, dtype=torch.bool).triu(1), float("-inf"))
        return (torch.softmax(s, -1) @ vv.double().transpose(1, 2)).transpose(1, 2), torch.logsumexp(s, -1)

    q, k, v = (torch.randn(B, L, H, hd, generator=g) * 3.0 for L in (Lq, Lk, Lk))
    o, lse = run(q, k, v)
    r8, l8 = ref(_e4m3_rows(q), _e4m3_rows(k), v.to(torch.bfloat16).float())
    assert _rel(o, r8) < 1e-2
    assert float((lse.cpu().double() - l8).abs().max()) < 2e-3
    q, k, v = (torch.randn(B, L, H, hd, generator=g) for L in (Lq, Lk, Lk))
    o, _ = run(q, k, v)
    r32, _ = ref(q, k, v)
    o = o.cpu().double()
    assert float((o - r32).norm() / r32.norm()) < 5e-2


def test_attention_fp8_mode_forward_only(cuda):
    """prec.attention('fp8') routes ops.attention's forward to the fp8 kernel; its backward runs the
    bf16 kernels (asrx_attn_bwd rejects prec 2)."""
    from asrx import ops, prec

    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(1, 130, 2, 64, generator=g).to(cuda).requires_grad_() for _ in range(3))
    with prec.precision("bf16"):
        ob = ops.attention(q, k, v, False)
        with prec.attention("fp8"):
            assert prec.attention_prec() == prec.PREC_FP8ATT
            of = ops.attention(q, k, v, False)
        of.sum().backward()
    assert 0 < _rel(of, ob) < 5e-2
    assert all(torch.isfinite(t.grad).all() for t in (q, k, v))


@pytest.mark.parametrize("B,T,C,sid_base,act,act2", [(2, 101, 384, 0, "gelu", "none"), (3, 77, 64, 64, "gelu", "none"),
                                                     (1, 33, 8, 5, "none", "none"), (2, 50, 384, 3, "gelu", "gelu"),
                                                     (2, 50, 384, 3, "relu", "gelu"), (2, 50, 384, 3, "gelu", "relu")])
def test_act_dropout_fused(cuda, B, T, C, sid_base, act, act2):
    """Fused act + dropout (encoder layer tail) and the float4 dropout: masks equal the oracle's keyed
    mask (keep iff uniform(key, (sid*C + c)*8192 + t) >= p, oracle/keys.py), forward/backward
    bit-identical to Act then Dropout."""
    import numpy as np

    from asrx import ops
    from oracle import noise as onoise

    key, p = 0x1234ABCD, 0.1
    g = torch.Generator().manual_seed(B * T + C)
    z = torch.randn(B, T, C, generator=g).to(cuda).requires_grad_()
    gout = torch.randn(B, T, C, generator=g).to(cuda)
    y = ops.ActDropout.apply(z, act, sid_base, key, p, act2)
    (dz,) = torch.autograd.grad(y, z, gout)
    z2 = z.detach().clone().requires_grad_()
    y2 = ops.Dropout.apply(ops.act(z2, act) if act != "none" else z2 * 1.0, sid_base, key, p)
    if act2 != "none":
        y2 = ops.act(y2, act2)
    (dz2,) = torch.autograd.grad(y2, z2, gout)
    assert torch.equal(y, y2) and torch.equal(dz, dz2)
    if act2 != "none":
        return
    b, t, c = np.meshgrid(np.arange(B), np.arange(T), np.arange(C), indexing="ij")
    idx = (((sid_base + b) * C + c) * 8192 + t).astype(np.uint64) & 0xFFFFFFFF
    keep = torch.from_numpy(np.asarray(onoise.uniform(key, idx.ravel())).reshape(B, T, C) >= p)
    assert torch.equal((y.detach().cpu() != 0), keep & (z.detach().cpu() != 0))


def test_dropout_add_fused(cuda):
    """ConvLite tail res + Dropout(y) in one pass: forward and both gradients bit-identical to
    add(res, Dropout(y))."""
    from asrx import ops

    g = torch.Generator().manual_seed(11)
    res, y = (torch.randn(2, 97, 384, generator=g).to(cuda).requires_grad_() for _ in range(2))
    gout = torch.randn(2, 97, 384, generator=g).to(cuda)
    out = ops.DropoutAdd.apply(res, y, 7, 0xBEEF, 0.1)
    d1 = torch.autograd.grad(out, (res, y), gout)
    out2 = ops.add(res, ops.Dropout.apply(y, 7, 0xBEEF, 0.1))
    d2 = torch.autograd.grad(out2, (res, y), gout)
    assert torch.equal(out, out2)
    assert all(torch.equal(a, b) for a, b in zip(d1, d2))


def test_noise_epoch(cuda):
    """asrx_set_noise_epoch: a nonzero epoch changes every keyed draw (dropout masks and AbbyNormal's
    gumbel decisions), epoch 0 restores the oracle's keys exactly; stream-ordered, so it also steers
    launches replayed from a captured graph."""
    from asrx import lib, ops

    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 301, 384, generator=g).to(cuda)
    key = 0xC0FFEE
    y0 = ops.Dropout.apply(x, 0, key, 0.1)
    lib.call("asrx_set_noise_epoch", 7, lib.stream())
    try:
        y7 = ops.Dropout.apply(x, 0, key, 0.1)
        y7b = ops.ActDropout.apply(x, "none", 0, key, 0.1, "none")
        pol7 = ops.policy_noise(4, 3, 0, key, cuda)
    finally:
        lib.call("asrx_set_noise_epoch", 0, lib.stream())
    y0b = ops.Dropout.apply(x, 0, key, 0.1)
    pol0 = ops.policy_noise(4, 3, 0, key, cuda)
    assert torch.equal(y0, y0b)
    assert not torch.equal((y0 == 0), (y7 == 0))
    assert torch.equal(y7, y7b)  # both kernels of the TU see the same epoch
    assert not torch.equal(pol0, pol7)
    keep7 = float((y7 != 0).double().mean())
    assert 0.88 < keep7 < 0.92
    # graph capture: the epoch set before a replay decides its draws
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = ops.Dropout.apply(x, 0, key, 0.1)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.Dropout.apply(x, 0, key, 0.1)
    res = []
    for ep in (0, 7, 0):
        lib.call("asrx_set_noise_epoch", ep, lib.stream())
        graph.replay()
        res.append(out.clone())
    lib.call("asrx_set_noise_epoch", 0, lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(res[0], y0) and torch.equal(res[1], y7) and torch.equal(res[2], y0)
