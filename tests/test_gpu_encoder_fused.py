"""The encoder's fused chains against the composition of the stand-alone ops they replace, on the same
inputs: GLU -> depthwise k15 (PreDWConv "glu"), BatchNorm -> SiLU (BatchNormSiLU), GELU -> depthwise k3
(PreDWConv "gelu").  Forward outputs and input gradients are bit-identical (torch.equal); parameter
gradients are float-atomic sums on both sides and are held to the tolerances test_dwconv /
test_batchnorm_per_sample use against float64 (1e-5 and 2e-5 of the largest entry).

Shapes: B = 3 (odd); T = 1 and 5 are shorter than the k15 halo (and than the 32 row groups of the
statistics kernels), 37 is no multiple of the 16-row tile, 101 spans several tiles; C = 136 crosses a
32-column chunk (C / 4 = 34), 384 is the model's width; C = 6 must take the stand-alone ops."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3
TS = [1, 5, 37, 101]
CS = [8, 136, 384]
N_OLD = 12  # runs of the stand-alone encoder that give its run-to-run spread


@pytest.fixture(autouse=True)
def _fp32():
    from asrx import prec

    with prec.precision("fp32"):
        yield


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _run(fn, inputs, seed=0):
    """fn on fresh CUDA leaves, backprop a fixed random cotangent: (output, gradients of the leaves)."""
    leaves = [t.detach().clone().cuda().requires_grad_() for t in inputs]
    y = fn(*leaves)
    gout = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed)).cuda()
    y.backward(gout)
    torch.cuda.synchronize()
    return y.detach(), [t.grad for t in leaves]


def _check(fused, old, inputs, ptol):
    yf, gf = _run(fused, inputs)
    yo, go = _run(old, inputs)
    assert torch.equal(yf, yo)
    assert torch.equal(gf[0], go[0])  # input gradient
    for a, r in zip(gf[1:], go[1:]):  # parameter gradients
        print(f"param grad rel diff {_rel(a, r):.3e}")
        assert _rel(a, r) < ptol


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("T", TS)
def test_glu_dwconv(cuda, T, C):
    from asrx import ops

    torch.manual_seed(15000 + C + T)
    x = torch.randn(B, T, 2 * C) * 2
    w = torch.randn(C, 1, 15) * 0.3
    b = torch.randn(C)
    _check(lambda x, w, b: ops.PreDWConv.apply(x, w, b, "glu"),
           lambda x, w, b: ops.DWConv.apply(ops.glu(x), w, b), [x, w, b], 1e-5)


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("T", TS)
def test_gelu_dwconv(cuda, T, C):
    from asrx import ops

    torch.manual_seed(3000 + C + T)
    x = torch.randn(B, T, C) * 2
    w = torch.randn(C, 1, 3) * 0.3
    b = torch.randn(C)
    _check(lambda x, w, b: ops.PreDWConv.apply(x, w, b, "gelu"),
           lambda x, w, b: ops.DWConv.apply(ops.act(x, "gelu"), w, b), [x, w, b], 1e-5)


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("T", TS)
def test_batchnorm_silu(cuda, T, C):
    from asrx import ops

    torch.manual_seed(C + T)
    x = torch.randn(B, T, C) * 2 + 5
    w = torch.rand(C) + 0.5
    b = torch.randn(C)
    sf, so = [], []
    _check(lambda x, w, b: ops.BatchNormSiLU.apply(x, w, b, 1e-5, sf),
           lambda x, w, b: ops.act(ops.BatchNormPS.apply(x, w, b, 1e-5, so), "silu"), [x, w, b], 2e-5)
    for a, r in zip(sf[0], so[0]):  # the per-sample statistics handed to the running-average update
        assert torch.equal(a, r)


@pytest.mark.parametrize("C", CS + [6])
@pytest.mark.parametrize("T", [5, 101])
def test_batchnorm_silu_eval(cuda, T, C):
    """Running statistics: the fused apply equals batch_norm_eval followed by act, bit for bit (C = 6 through the
    stand-alone kernels)."""
    from asrx import ops

    torch.manual_seed(7 + C + T)
    x = (torch.randn(B, T, C) * 2 + 5).cuda()
    w, b = (torch.rand(C) + 0.5).cuda(), torch.randn(C).cuda()
    rm, rv = (torch.randn(C) + 5).cuda(), (torch.rand(C) * 4 + 0.1).cuda()
    with torch.no_grad():
        yf = ops.batch_norm_silu_eval(x, w, b, rm, rv, 1e-5)
        yo = ops.act(ops.batch_norm_eval(x, w, b, rm, rv, 1e-5), "silu")
    assert torch.equal(yf, yo)


def test_wrappers_route(cuda):
    """The wrappers the model calls take the fused kernels by default and the stand-alone ops for C = 6 (no float4
    columns) or with the switch off -- and match either way."""
    from asrx import ops

    def fns():
        return [(lambda x, w, b: ops.glu_dwconv(x, w, b), lambda x, w, b: ops.DWConv.apply(ops.glu(x), w, b), 2, 15),
                (lambda x, w, b: ops.act_dwconv(x, "gelu", w, b),
                 lambda x, w, b: ops.DWConv.apply(ops.act(x, "gelu"), w, b), 1, 3),
                (lambda x, w, b: ops.batch_norm_silu(x, w, b, 1e-5, None),
                 lambda x, w, b: ops.act(ops.BatchNormPS.apply(x, w, b, 1e-5, None), "silu"), 1, 0)]

    T = 37
    for C, want_fused in [(8, True), (6, False)]:
        for i, (fused, old, mul, K) in enumerate(fns()):
            torch.manual_seed(100 * C + i)
            x = torch.randn(B, T, mul * C) * 2
            w = torch.randn(C, 1, K) * 0.3 if K else torch.rand(C) + 0.5
            b = torch.randn(C)
            y = fused(*[t.cuda().requires_grad_() for t in (x, w, b)])
            name = type(y.grad_fn).__name__
            assert (name in ("PreDWConvBackward", "BatchNormSiLUBackward")) == want_fused, (C, i, name)
            _check(fused, old, [x, w, b], 2e-5 if K == 0 else 1e-5)
    assert ops.FUSED_ENCODER
    ops.FUSED_ENCODER = False
    try:
        y = ops.glu_dwconv(torch.randn(B, T, 16).cuda().requires_grad_(), torch.randn(8, 1, 15).cuda(),
                           torch.randn(8).cuda())
        assert type(y.grad_fn).__name__ == "DWConvBackward"
    finally:
        ops.FUSED_ENCODER = True


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_encoder_fused_vs_separate(cuda, mode):
    """One train-mode forward + backward of a 2-layer AudioEncoder over three streams (two stream groups), with
    the fused ops and with the stand-alone ops (ops.FUSED_ENCODER): encodings and the input gradient are
    bit-identical; every parameter gradient lies within the spread of the stand-alone path's own runs
    (float-atomic sums; N_OLD runs give the spread, see below)."""
    from asrx import ops, prec
    from asrx.model import AudioEncoder
    from asrx.noise import NoiseCtx

    torch.manual_seed(4)
    enc = AudioEncoder(128, 128, 2, 2, "gelu", "AbbyNormal").cuda().train()
    Bn, T = 2, 101
    spec = torch.randn(Bn, 128, T).cuda()
    pitch = (torch.rand(Bn, 1, T) * 100).cuda()
    wav = torch.randn(Bn, 1, T - 1).cuda()
    gouts = [torch.randn(Bn, t, 128, generator=torch.Generator().manual_seed(s)).cuda()
             for s, t in enumerate([T, T, T - 1])]

    def run(fused):
        ops.FUSED_ENCODER = fused
        try:
            for p in enc.parameters():
                p.grad = None
            sp = spec.clone().requires_grad_()
            with prec.precision(mode):
                outs = enc.encode([pitch, sp, wav], NoiseCtx(11, 0, True), Bn)
                torch.autograd.backward(outs, gouts)
            torch.cuda.synchronize()
            grads = {n: p.grad.detach().double().cpu() for n, p in enc.named_parameters() if p.grad is not None}
            return [o.detach().float() for o in outs], sp.grad.detach().clone(), grads
        finally:
            ops.FUSED_ENCODER = True

    old = [run(False) for _ in range(N_OLD)]
    of, df, gf = run(True)
    o1, d1, g1 = old[0]
    for a, r in zip(of, o1):
        assert torch.equal(a, r)
    assert torch.equal(df, d1)
    assert sorted(gf) == sorted(g1) and len(g1) > 20
    # The spread of the stand-alone path: the largest difference between any two of its runs, over all
    # parameters, each relative to the parameter's largest gradient.  One pair of runs is no estimate of it:
    # per parameter a pair differs by 0 to 7 ulp at random (also in the stem and LayerNorm sums, which no fused
    # kernel feeds differently), so N_OLD runs give the spread, and a parameter passes when the fused gradient
    # is no further than that from the nearest of them.
    pairs = [(i, j) for i in range(N_OLD) for j in range(i)]
    own = {n: max(_rel(old[i][2][n], old[j][2][n]) for i, j in pairs) for n in g1}
    spread, worst = max(own.values()), []
    for n in g1:
        diff = min(_rel(gf[n], o[2][n]) for o in old)
        print(f"{mode} {n}: old-vs-old {own[n]:.3e} fused-vs-old {diff:.3e}")
        if diff > spread:
            worst.append((n, diff))
    print(f"{mode} spread of the stand-alone path {spread:.3e}")
    assert not worst, (spread, worst)
