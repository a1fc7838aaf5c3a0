"""The encoder with per-sample lengths on the GPU: in a zero-padded batch every sample comes out as it would alone.

Kernel level (fp32 mode, like test_gpu_encoder_fused.py): ops.glu_dwconv, ops.act_dwconv, ops.batch_norm_silu,
ops.act("gelu") and ops.act_dropout (act2 "none" and "gelu") with lens=.
Shapes: C in {8, 136, 384} (one float4 chunk, across a 32-column chunk, the model's width), B = 8, T = 101, lengths
[101, 100, 1, 5, 16, 17, 23, 33]: 1 and 5 are shorter than the k15 halo and than the 32 row groups of the statistics
kernels, 16 and 17 the edge of the 16-row tile, 23 puts the k15 halo across a half-dead tile, 33 is the row-group
wrap, 100 and 101 the last row and the full length.  One more: T = 530, C = 8, lengths [530, 511, 513, 17], across
the weight-gradient kernel's 512-row chunk.
For each, with a fixed random cotangent:
 1. live rows of the output and of the input gradient are torch.equal to the uniform op on x[b:b+1, :T_b] (the
    dropout with sid_base + b; the BatchNorm statistics of sample b too);
 2. output and input-gradient rows at or past T_b are exactly zero; NaN in the pad rows of the input (convs and
    BatchNorm) and of the cotangent changes no output or input gradient and leaves every result finite;
 3. parameter gradients against the float64 sum of the alone terms, within the bounds the project holds these ops
    to: 1e-5 of the largest entry for the convs (test_dwconv), 2e-5 for BatchNorm (test_batchnorm_per_sample);
 4. a full-length table gives torch.equal results and the grad_fn class of lens=None;
 5. lengths matter: for the ops that reach across rows (convs, BatchNorm) the live rows of sample 2 differ from
    the lens=None result.  A row-local op (act, act_dropout) cannot differ on a live row, by construction; there
    the live rows are equal and the pad rows of that sample differ.

Module level: AudioEncoder.encode with lens on the three streams of test_encoder_stream, see test_encode_lens.
"""
import copy

import pytest
import torch

from oracle import model as om

pytestmark = pytest.mark.gpu

LENS8 = [101, 100, 1, 5, 16, 17, 23, 33]
SHAPES = [(8, 101, LENS8), (136, 101, LENS8), (384, 101, LENS8), (8, 530, [530, 511, 513, 17])]
SHAPE_IDS = ["C8", "C136", "C384", "T530"]
SID = 3
KEY = 0x5EED


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _run(fn, inputs, cot):
    """fn on fresh CUDA leaves, backprop the cotangent: (output with its grad_fn, gradients of the leaves)."""
    leaves = [t.detach().clone().cuda().requires_grad_() for t in inputs]
    y = fn(*leaves)
    y.backward(cot.cuda())
    torch.cuda.synchronize()
    return y, [t.grad for t in leaves]


def _glu_dwconv(C, T, B):
    return [torch.randn(B, T, 2 * C) * 2, torch.randn(C, 1, 15) * 0.3, torch.randn(C)]


def _act_dwconv(C, T, B):
    return [torch.randn(B, T, C) * 2, torch.randn(C, 1, 3) * 0.3, torch.randn(C)]


def _bn(C, T, B):
    return [torch.randn(B, T, C) * 2 + 5, torch.rand(C) + 0.5, torch.randn(C)]


def _x(C, T, B):
    return [torch.randn(B, T, C) * 2]


def _ops():
    from asrx import ops

    # name -> (inputs, fn(lens, sid, stats) -> callable on the leaves, NaN into the input's pad rows, param bound,
    #          reaches across rows)
    return {
        "glu_dwconv": (_glu_dwconv, lambda L, sid, st: lambda x, w, b: ops.glu_dwconv(x, w, b, lens=L), True, 1e-5,
                       True),
        "act_dwconv": (_act_dwconv, lambda L, sid, st: lambda x, w, b: ops.act_dwconv(x, "gelu", w, b, lens=L), True,
                       1e-5, True),
        "batch_norm_silu": (_bn, lambda L, sid, st: lambda x, w, b: ops.batch_norm_silu(x, w, b, 1e-5, st, lens=L),
                            True, 2e-5, True),
        "act_gelu": (_x, lambda L, sid, st: lambda x: ops.act(x, "gelu", lens=L), False, None, False),
        "act_dropout": (_x, lambda L, sid, st: lambda x: ops.act_dropout(x, "gelu", sid, KEY, 0.1, "none", lens=L),
                        False, None, False),
        "act_dropout_gelu": (_x, lambda L, sid, st: lambda x: ops.act_dropout(x, "gelu", sid, KEY, 0.1, "gelu",
                                                                               lens=L), False, None, False),
    }


OPS = ["glu_dwconv", "act_dwconv", "batch_norm_silu", "act_gelu", "act_dropout", "act_dropout_gelu"]


@pytest.fixture(autouse=True)
def _fp32():
    from asrx import prec

    with prec.precision("fp32"):
        yield


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("op", OPS)
def test_op_lens(cuda, op, shape):
    from asrx import ops

    C, T, lens = shape
    B = len(lens)
    make, fn, nan_in, ptol, crosses = _ops()[op]
    torch.manual_seed(1000 * OPS.index(op) + C + T)
    inputs = make(C, T, B)
    cot = torch.randn(B, T, C)
    L = ops.seq_lens(lens)
    st = []
    y, gs = _run(fn(L, SID, st), inputs, cot)
    assert "Lens" in type(y.grad_fn).__name__
    y = y.detach()
    # 1, 2: every sample alone
    psum = [torch.zeros_like(p, dtype=torch.float64) for p in inputs[1:]]
    for b, n in enumerate(lens):
        sb = []
        yb, gb = _run(fn(None, SID + b, sb), [inputs[0][b:b + 1, :n]] + inputs[1:], cot[b:b + 1, :n])
        assert "Lens" not in type(yb.grad_fn).__name__
        assert torch.equal(y[b, :n], yb.detach()[0]), (b, n)
        assert torch.equal(gs[0][b, :n], gb[0][0]), (b, n)
        assert not y[b, n:].any() and not gs[0][b, n:].any(), (b, n)
        if st:
            assert torch.equal(st[0][0][b], sb[0][0][0]) and torch.equal(st[0][1][b], sb[0][1][0]), (b, n)
        for s, g in zip(psum, gb[1:]):
            s += g.double().cpu()
    # 3: parameter gradients
    for g, s in zip(gs[1:], psum):
        print(f"{op} C={C} T={T}: param grad rel diff {_rel(g, s):.3e} (bound {ptol:g})")
        assert _rel(g, s) < ptol
    # 2: NaN in the pad rows
    xin, cn = inputs[0].clone(), cot.clone()
    for b, n in enumerate(lens):
        cn[b, n:] = float("nan")
        if nan_in:
            xin[b, n:] = float("nan")
    y2, g2 = _run(fn(L, SID, []), [xin] + inputs[1:], cn)
    assert torch.equal(y2.detach(), y) and torch.equal(g2[0], gs[0])
    for g, s in zip(g2[1:], psum):
        assert torch.isfinite(g).all() and _rel(g, s) < ptol
    # 4: a full-length table is the uniform path
    yn, gn = _run(fn(None, SID, []), inputs, cot)
    yf, gf = _run(fn(ops.seq_lens([T] * B), SID, []), inputs, cot)
    assert type(yf.grad_fn) is type(yn.grad_fn)
    assert torch.equal(yf.detach(), yn.detach()) and torch.equal(gf[0], gn[0])
    # 5: lengths matter (sample 2 is the shortest but one)
    n = lens[2]
    if crosses:
        assert not torch.equal(yn.detach()[2, :n], y[2, :n])
    else:
        assert torch.equal(yn.detach()[2, :n], y[2, :n]) and not torch.equal(yn.detach()[2, n:], y[2, n:])


def test_c_abi_clamps_the_table(cuda):
    """A table holding 0 and T + 7, straight through the C-ABI: an all-zero sample with mean = rstd = 0, and the
    full-length result."""
    from asrx import lib, ops

    torch.manual_seed(5)
    B, T, C = 2, 37, 136
    x = (torch.randn(B, T, C) * 2 + 5).cuda()
    w, b = (torch.rand(C) + 0.5).cuda(), torch.randn(C).cuda()
    tab = torch.tensor([0, T + 7], dtype=torch.int32).cuda()
    P, S = lib.ptr, lib.stream
    y, mean, rstd = torch.full_like(x, 7.0), torch.full((B, C), 7.0).cuda(), torch.full((B, C), 7.0).cuda()
    lib.call("asrx_bn_silu_lens_fwd", P(x), P(w), P(b), P(y), P(mean), P(rstd), P(tab), B, T, C, 1e-5, 1, S())
    yr, mr, rr = torch.empty_like(x[1:]), torch.empty(1, C).cuda(), torch.empty(1, C).cuda()
    lib.call("asrx_bn_silu_fwd", P(x[1:]), P(w), P(b), P(yr), P(mr), P(rr), 1, T, C, 1e-5, 1, S())
    assert not y[0].any() and not mean[0].any() and not rstd[0].any()
    assert torch.equal(y[1:], yr) and torch.equal(mean[1:], mr) and torch.equal(rstd[1:], rr)
    # the k15 conv
    wc, bc = (torch.randn(C, 1, 15) * 0.3).cuda(), torch.randn(C).cuda()
    y = torch.full_like(x, 7.0)
    lib.call("asrx_dwconv_lens_fwd", P(x), P(wc), P(bc), P(y), P(tab), B, T, C, 15, S())
    yr = torch.empty_like(x[1:])
    lib.call("asrx_dwconv_fwd", P(x[1:]), P(wc), P(bc), P(yr), 1, T, C, 15, S())
    assert not y[0].any() and torch.equal(y[1:], yr)
    # the running statistics: the empty sample adds mean 0 and variance 0, the other its own with T / (T - 1)
    rm, rv = torch.zeros(C).cuda(), torch.ones(C).cuda()
    lib.call("asrx_bn_running_lens", P(mean), P(rstd), P(rm), P(rv), None, P(tab), B, C, T, 1e-5, 0.1, S())
    var = (1.0 / rstd[1].double() ** 2 - 1e-5) * T / (T - 1)
    assert _rel(rm, 0.1 * mean[1].double() / 2) < 1e-5
    assert _rel(rv, 0.9 + 0.1 * var / 2) < 1e-5


def test_seq_lens_refusals(cuda):
    from asrx import ops

    with pytest.raises(ValueError):
        ops.seq_lens([3, 0])
    with pytest.raises(ValueError):
        ops.seq_lens([])
    with pytest.raises(TypeError):
        ops.seq_lens(torch.tensor([3, 4]).cuda())
    with pytest.raises(TypeError):
        ops.seq_lens([3.5, 4])
    x = torch.randn(3, 9, 8).cuda()
    with pytest.raises(ValueError):  # the wrong count
        ops.act(x, "gelu", lens=ops.seq_lens([3, 4]))
    with pytest.raises(ValueError):  # a length above T
        ops.act(x, "gelu", lens=ops.seq_lens([3, 4, 10]))
    L = ops.seq_lens([3, 4, 9])
    with pytest.raises(ValueError):  # a shape the float4 kernels refuse: no fall-back to kernels that ignore lens
        ops.act(torch.randn(3, 9, 6).cuda(), "gelu", lens=L)
    with pytest.raises(ValueError):
        ops.batch_norm_silu(torch.randn(3, 9, 6).cuda(), torch.ones(6).cuda(), torch.zeros(6).cuda(), 1e-5, None,
                            lens=L)
    ops.FUSED_ENCODER = False
    try:
        with pytest.raises(ValueError):
            ops.act_dropout(x, "gelu", 0, KEY, 0.1, lens=L)
        with pytest.raises(ValueError):
            ops.glu_dwconv(torch.randn(3, 9, 16).cuda(), torch.randn(8, 1, 15).cuda(), torch.zeros(8).cuda(), lens=L)
    finally:
        ops.FUSED_ENCODER = True
    j = ops.SeqLens.join([L, ops.SeqLens.full(2, 9, x.device)])
    assert j.lens == (3, 4, 9, 9, 9) and j.table.tolist() == [3, 4, 9, 9, 9] and j.table.dtype == torch.int32


# ------------------------------------------------------------------------------------------------ module level
MB, MT, MD, MLAYERS = 3, 101, 128, 2
MLENS = [[101, 37, 5], [101, 37, 5], [100, 36, 4]]  # pitch, spectrogram, waveform (T - 1 frames)
SEED, STEP = 11, 0


def _streams():
    g = torch.Generator().manual_seed(4)
    pitch = torch.rand(MB, 1, MT, generator=g) * 100
    spec = torch.randn(MB, 128, MT, generator=g)
    wav = torch.randn(MB, 1, MT - 1, generator=g)
    out = [pitch, spec, wav]
    for s, x in enumerate(out):
        for b, n in enumerate(MLENS[s]):
            x[b, :, n:] = 0.0  # the collator's zero pad frames
    cots = [torch.randn(MB, x.shape[-1], MD, generator=g) for x in out]
    return out, cots


def _grads(enc):
    return {n: p.grad.detach().double().cpu() for n, p in enc.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_encode_lens(cuda, train, precision):
    """AudioEncoder(128, 128, 2, 2, "gelu", "AbbyNormal") on the three streams of test_encoder_stream with B = 3,
    lengths [101, 37, 5] (pitch, spectrogram) and [100, 36, 4] (waveform), zero pad frames, NaN in the pad rows of
    the cotangents.  Live rows of every encoding are torch.equal to enc.layers(enc.stem(x_b), noise, s B + b) on
    the sample alone; pad rows equal the sinusoid table.  fp32 train also: forward within 1e-5 of the float64 oracle
    per sample (test_encoder_stream's bound); every parameter gradient against the oracle's summed per-sample
    gradients at no more than twice the distance of the uniform path run on each sample alone (its gradients
    summed in float64), or 2e-5 where that is larger -- the batch adds the samples' terms in another order and the
    float-atomic sums move by a few ulp from run to run (measured: every distance 5e-6 at most, worst ratio 1.97 at
    encoder.1.2.beta, 6.6e-7 against 3.4e-7; depth.bias, a bias ahead of BatchNorm whose true gradient is zero, holds
    the same rounding noise on both paths, ratio 1.00); the running statistics against the float64 formula from
    the oracle's per-sample statistics with T_b / (T_b - 1), to 1e-5, and unlike what lens=None leaves."""
    from asrx import prec
    from asrx.model import AudioEncoder, sinusoids
    from asrx.noise import NoiseCtx

    torch.manual_seed(4)
    enc = AudioEncoder(128, MD, 2, MLAYERS, "gelu", "AbbyNormal").cuda()
    enc.train(train)
    enc0 = copy.deepcopy(enc)
    streams, cots = _streams()
    noise = NoiseCtx(SEED, STEP, train)
    cn = [c.clone() for c in cots]
    for s in range(3):
        for b, n in enumerate(MLENS[s]):
            cn[s][b, n:] = float("nan")
    with prec.precision(precision):
        outs = enc.encode([x.cuda() for x in streams], noise, MB, lens=MLENS)
        torch.autograd.backward(outs, [c.cuda() for c in cn])
        torch.cuda.synchronize()
        glens = _grads(enc)
        running = [(l[3].bn.running_mean.clone(), l[3].bn.running_var.clone()) for l in enc.encoder]
        assert all(torch.isfinite(g).all() for g in glens.values())
        # every sample alone through the uniform path
        alone = copy.deepcopy(enc0)
        gsum = {}
        for s, x in enumerate(streams):
            T = x.shape[-1]
            pe = sinusoids(T, MD, outs[s].device)
            for b, n in enumerate(MLENS[s]):
                alone.zero_grad(set_to_none=True)
                yb = alone.layers(alone.stem(x[b:b + 1, :, :n].contiguous().cuda()), noise, s * MB + b)
                yb.backward(cots[s][b:b + 1, :n].cuda())
                torch.cuda.synchronize()
                assert torch.equal(outs[s][b, :n], yb[0]), (s, b)
                assert torch.equal(outs[s][b, n:], pe[n:]), (s, b)
                for k, g in _grads(alone).items():
                    gsum[k] = gsum.get(k, 0) + g
        with pytest.raises(ValueError):  # a length above T
            enc.encode([x.cuda() for x in streams], noise, MB, lens=[None, None, [MT, 1, 1]])
    if not (train and precision == "fp32"):
        return
    # the float64 oracle, every sample alone
    P = {f"enc.{k}": v.detach().cpu().double().requires_grad_(v.is_floating_point())
         for k, v in enc0.state_dict().items()}
    onoise = om.Noise(SEED, STEP, torch.float64)
    stats = []  # (layer order within a call) per-sample statistics of the BatchNorm input
    orig = om._batch_norm_per_sample

    def spy(y, P_, pre, training, eps=1e-5):
        stats[-1].append((y.detach().mean(dim=(0, 2)), y.detach().var(dim=(0, 2), unbiased=False)))
        return orig(y, P_, pre, training, eps)

    names = [n for n, p in enc0.named_parameters()]
    gref = {n: torch.zeros_like(P["enc." + n]) for n in names}
    om._batch_norm_per_sample = spy
    try:
        for s, x in enumerate(streams):
            for b, n in enumerate(MLENS[s]):
                stats.append([])
                ref = om.encode_stream(P, x[b:b + 1, :, :n].double(), MLAYERS, onoise, [s * MB + b], True)
                assert _rel(outs[s][b:b + 1, :n], ref) < 1e-5, (s, b)
                gs = torch.autograd.grad(ref, [P["enc." + k] for k in names], cots[s][b:b + 1, :n].double(),
                                         allow_unused=True)
                for k, g in zip(names, gs):
                    if g is not None:
                        gref[k] += g
    finally:
        om._batch_norm_per_sample = orig
    worst = 0.0
    for k in names:
        if k not in glens:
            continue
        scale = float(gref[k].abs().max().clamp_min(1e-30))
        d_alone = float((gsum[k] - gref[k]).abs().max()) / scale
        d_lens = float((glens[k] - gref[k]).abs().max()) / scale
        bound = max(2 * d_alone, 2e-5)
        worst = max(worst, d_lens / max(d_alone, 1e-30))
        print(f"{k}: to the oracle, alone {d_alone:.3e}  lens {d_lens:.3e}  ratio {d_lens / max(d_alone, 1e-30):.2f}")
        assert d_lens <= bound, (k, d_lens, d_alone)
    print(f"worst ratio lens / alone: {worst:.2f}")
    # running statistics: one update per stream group, (pitch, spectrogram) then the waveform
    flat = [(s, b) for s in range(3) for b in range(MB)]
    for l, layer in enumerate(enc.encoder):
        bn0 = enc0.encoder[l][3].bn
        rm, rv, m = bn0.running_mean.double().cpu(), bn0.running_var.double().cpu(), bn0.momentum
        for grp in ([0, 1], [2]):
            idx = [i for i, (s, b) in enumerate(flat) if s in grp]
            mean = torch.stack([stats[i][l][0] for i in idx]).mean(0)
            var = torch.stack([stats[i][l][1] * MLENS[flat[i][0]][flat[i][1]]
                               / max(MLENS[flat[i][0]][flat[i][1]] - 1, 1) for i in idx]).mean(0)
            rm, rv = (1 - m) * rm + m * mean, (1 - m) * rv + m * var
        assert _rel(running[l][0], rm) < 1e-5, l
        assert _rel(running[l][1], rv) < 1e-5, l
    with prec.precision(precision):
        padded = copy.deepcopy(enc0)
        padded.encode([x.cuda() for x in streams], noise, MB)
        torch.cuda.synchronize()
    for l, layer in enumerate(padded.encoder):
        assert not torch.equal(layer[3].bn.running_var, running[l][1])
        assert not torch.equal(layer[3].bn.running_mean, running[l][0])
