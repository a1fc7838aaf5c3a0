"""asrx.optim.GradStats (asrx_grad_stats, csrc/gradstats.hip) against float64 torch on the CPU: every
chunk / alignment path of the kernel, non-finite detection at each of them, determinism, and the
gradient set of a real model with the measure + step pair free of host syncs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# Tolerance of a per-parameter sum of squares (relative; the terms are non-negative, so the relative
# error of an fp32 summation tree of depth m is at most m * 2^-24, each rounding at most 2^-24):
#   a lane adds into 4 accumulators: at most 16 float4 loads per chunk (4096 / (64 lanes * 4)), plus one
#   peeled head or tail scalar                                                     -> 17 adds in a chain
#   (s0 + s1) + (s2 + s3)                                                          ->  2
#   xor-shuffle tree over the 64 lanes                                             ->  6
#   the square itself                                                              ->  1
# m = 26.  Chunk partials are summed in double and rounded to fp32 once more, which the factor 2 the
# bound is used with covers many times over.  inv_scale is a power of two in every case below, so the
# product inv_scale * g is exact.  total_norm = sqrt(sum) halves the relative error and rounds twice.
M_DEPTH = 17 + 2 + 6 + 1
TOL = 2 * M_DEPTH * 2.0 ** -24


def _params(grads, dev):
    """One parameter per entry: a CPU gradient tensor, an already-made device gradient (a view), or None."""
    out = []
    for g in grads:
        shape = () if g is None else g.shape
        p = torch.zeros(shape, device=dev, requires_grad=True)
        if g is not None:
            p.grad = g if g.is_cuda else g.to(dev)
        out.append(p)
    return out


def _shape_set(dev, gen):
    from asrx.optim import GS_CHUNK as C

    shapes = [(), (1,), (3,), (5,), (63,), (64,), (65,), (C - 1,), (C,), (C + 1,), (3 * C + 7,), (37, 53), (16, 4, 3)]
    grads = [torch.randn(s, generator=gen) * (0.5 + i) for i, s in enumerate(shapes)]
    flat = (torch.randn(2 * C + 64, generator=gen) * 3).to(dev)  # bucket views: misaligned bases
    assert flat.data_ptr() % 16 == 0
    views = [flat[1:1 + C + 5], flat[2:2 + 70], flat[3:3 + 2 * C + 1]]
    assert [v.data_ptr() % 16 for v in views] == [4, 8, 12]
    grads = grads[:6] + [None] + grads[6:] + views  # a parameter without a gradient in the middle
    return grads


def _ref(grads, inv_scale):
    live = [g for g in grads if g is not None]
    sumsq = torch.stack([(g.detach().double().cpu() * inv_scale).square().sum() for g in live])
    return sumsq, float(sumsq.sum().sqrt())


def _check(stats, grads, inv_scale, max_norm):
    sumsq, total = _ref(grads, inv_scale)
    got = stats.sumsq.double().cpu()
    ctl = stats.ctl.double().cpu()
    assert got.shape == sumsq.shape
    err = ((got - sumsq).abs() / sumsq.clamp_min(1e-300)).max()
    print("sumsq rel err", float(err), "total rel err", abs(float(ctl[2]) - total) / total)
    assert float(err) <= TOL
    assert abs(float(ctl[2]) - total) <= TOL * total
    assert float(ctl[1]) == 0.0 and float(ctl[3]) == 0.0
    if max_norm <= 0:
        assert float(ctl[0]) == inv_scale
    else:
        want = inv_scale * min(1.0, max_norm / (total + 1e-6))
        # the quotient sees the norm's error once more and two roundings of its own
        assert abs(float(ctl[0]) - want) <= (TOL + 3 * 2.0 ** -24) * want
    assert torch.equal(stats.coef, stats.ctl[0]) and torch.equal(stats.found_inf, stats.ctl[1])
    assert torch.equal(stats.total_norm, stats.ctl[2])


def test_shapes_alignment_and_coef(cuda):
    from asrx.optim import GradStats

    gen = torch.Generator().manual_seed(0)
    grads = _shape_set(cuda, gen)
    params = _params(grads, cuda)
    _, total = _ref(grads, 1.0)
    for inv_scale in (1.0, 1.0 / 1024):
        for max_norm in (0.0, 2.0 * total * inv_scale, 0.5 * total * inv_scale):
            st = GradStats(params, max_norm=max_norm).measure(inv_scale)
            _check(st, grads, inv_scale, max_norm)
            assert len(st.norms()) == len(grads) - 1 and "6" not in st.norms()  # the grad=None one is left out
    # a second call: 300 tensors of sizes 1..300 (many tensors per workgroup, several workgroups)
    many = [torch.randn(n, generator=gen) for n in range(1, 301)]
    st = GradStats(_params(many, cuda), max_norm=1.0).measure()
    _check(st, many, 1.0, 1.0)


def test_non_finite_values(cuda):
    from asrx.optim import GS_CHUNK as C, GradStats

    gen = torch.Generator().manual_seed(1)
    a = torch.randn(3 * C + 7, generator=gen).to(cuda)  # aligned: vector body, 3-element scalar tail
    b = torch.randn(64 * 4 + 2, generator=gen).to(cuda)  # one float4 per lane, then a 2-element tail
    flat = torch.randn(C + 16, generator=gen).to(cuda)
    v = flat[1:1 + C + 5]  # misaligned view: 3 peeled head elements, a second chunk
    z = torch.randn((), generator=gen).to(cuda)
    st = GradStats(_params([a, b, v, z], cuda), max_norm=1.0)
    ctl = st.measure().ctl.cpu()
    assert ctl[1] == 0 and ctl[0] > 0
    places = {"first": (a, 0), "last": (a, 3 * C + 6), "peeled head": (v, 1), "scalar tail": (b, 257),
              "chunk interior": (a, C + 1001), "second chunk of a view": (v, C + 3), "0-d": (z, None)}
    for where, (t, idx) in places.items():
        for bad in (float("nan"), float("inf"), float("-inf"), 1e30):
            keep = t.clone()
            if idx is None:
                t.fill_(bad)
            else:
                t[idx] = bad
            ctl = st.measure().ctl.cpu()
            t.copy_(keep)
            assert ctl[1] == 1.0 and ctl[0] == 0.0, (where, bad, ctl)
            assert ctl[3] == (0.0 if bad == 1e30 else 1.0), (where, bad, ctl)  # 1e30 is finite; its square is not
    ctl = st.measure().ctl.cpu()  # restored
    assert ctl[1] == 0 and ctl[3] == 0 and ctl[0] > 0
    # large, tiny and signed-zero values are finite
    odd = torch.cat([torch.full((40,), 1e-42), torch.full((40,), -0.0), torch.full((40,), 1e18),
                     torch.full((3,), -1e-45)]).to(cuda)
    s2 = GradStats(_params([odd], cuda)).measure()
    ctl = s2.ctl.cpu()
    assert ctl[1] == 0.0 and ctl[3] == 0.0 and ctl[0] == 1.0
    assert abs(float(ctl[2]) - (40 ** 0.5) * 1e18) <= TOL * (40 ** 0.5) * 1e18


def test_deterministic(cuda):
    from asrx.optim import GradStats

    gen = torch.Generator().manual_seed(2)
    grads = _shape_set(cuda, gen) + [torch.randn(n, generator=gen) for n in range(1, 301)]
    params = _params(grads, cuda)
    st = GradStats(params, max_norm=1.0)
    one = st.measure(0.5)._stats.clone()
    two = st.measure(0.5)._stats.clone()
    three = GradStats(params, max_norm=1.0).measure(0.5)._stats.clone()
    assert torch.equal(one, two) and torch.equal(one, three)


def test_model_gradients_and_sync_free_step(cuda):
    from asrx import prec
    from asrx.config import Dimensions
    from asrx.model import Model
    from asrx.optim import GradStats, MaxFactor, reference_param_groups

    torch.manual_seed(0)
    model = Model(Dimensions(tokens=300, mels=128, dims=128, head=2, layer=2, act="gelu", n_type="AbbyNormal"))
    model = model.to(cuda).train()
    g = torch.Generator().manual_seed(1)
    B, T, S = 2, 8, 101  # a 1 s clip
    spec = torch.randn(B, 128, S, generator=g)
    pitch = torch.rand(B, 1, S, generator=g) * 200
    wav = torch.randn(B, 1, S - 1, generator=g) * 0.1
    ids = torch.randint(3, 300, (B, T), generator=g)
    ids[:, 0] = 1
    labels = torch.cat([ids[:, 1:], torch.full((B, 1), 2)], 1)
    model.set_noise(1, 0)
    with prec.precision("fp32"):
        out = model(labels=labels.to(cuda), text_ids=ids.to(cuda), spectrogram=spec.to(cuda), pitch=pitch.to(cuda),
                    waveform=wav.to(cuda))
        out["loss"].backward()
    want = {n: float(p.grad.detach().double().cpu().norm()) for n, p in model.named_parameters() if p.grad is not None}
    assert len(want) > 20
    stats = GradStats(model.named_parameters(), max_norm=1.0)
    norms = stats.measure().norms()
    assert list(norms) == list(want)  # exactly the names that have a gradient, in model order
    worst = max(abs(norms[n] - want[n]) / want[n] for n in want if want[n] > 0)
    print("worst norm rel err", worst, "of", len(want))
    for n in want:
        assert abs(norms[n] - want[n]) <= TOL * want[n], n
    total = sum(v * v for v in want.values()) ** 0.5
    assert abs(float(stats.total_norm) - total) <= TOL * total
    assert float(stats.found_inf) == 0.0

    opt = MaxFactor(reference_param_groups(model), lr=2.5e-3)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    probe = torch.ones(1, device=cuda)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        stats.measure()
        opt.step(grad_ctl=stats)  # first call: builds tables and workspaces
        stats.measure()
        opt.step(grad_ctl=stats)
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert opt.sync_skips() == 0
    moved = 0
    for n, p in model.named_parameters():
        assert torch.isfinite(p).all(), n
        if n not in want:
            assert torch.equal(p, before[n]), n
        else:
            moved += not torch.equal(p, before[n])  # an all-zero parameter with a zero gradient stays put
    assert moved > len(want) // 2
    if not honoured:
        pytest.skip("this torch build does not raise on .item() under set_sync_debug_mode('error'): "
                    "the sync-free claim is not checked here")


def test_4096_tensors_in_one_call(cuda):
    """The documented per-call limit is accepted (bucket-style views: 4096 misaligned bases), one more is refused."""
    from asrx.optim import GS_MAX_TENSORS, GradStats

    assert GS_MAX_TENSORS >= 4096
    gen = torch.Generator().manual_seed(3)
    flat = torch.randn(GS_MAX_TENSORS * 7 + 16, generator=gen)
    dflat = flat.to(cuda)
    spans = [(7 * i, 1 + i % 7) for i in range(GS_MAX_TENSORS)]
    params = _params([dflat[o:o + n] for o, n in spans], cuda)
    st = GradStats(params, max_norm=1.0).measure()
    want = torch.stack([flat[o:o + n].double().square().sum() for o, n in spans])
    got = st.sumsq.double().cpu()
    assert float(((got - want).abs() / want).max()) <= TOL
    assert abs(float(st.total_norm) - float(want.sum().sqrt())) <= TOL * float(want.sum().sqrt())
    assert float(st.found_inf) == 0.0
    extra = _params([dflat[:3]], cuda)
    with pytest.raises(ValueError, match="at most"):
        GradStats(params + extra).measure()
