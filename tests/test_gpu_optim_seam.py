"""MaxFactor.step under a GradStats control word (asrx_maxfactor_step_ex): exact gradient scale, norm
clipping, the skipped step and its step counts, and the clip / cap branch (optimizerc.py:121-128).
Shapes, groups, hyper-parameters and tolerances (2e-6 parameters, 1e-5 state) are those of
tests/test_gpu_optim.py, restated in tests/maxfactor_clip_ref.py beside the float64 restatement."""
import pytest
import torch

import maxfactor_clip_ref as ref
from oracle import maxfactor as omf

pytestmark = pytest.mark.gpu

STATE = ("row_var", "col_var", "v")


def _optimizer(dev_params, **over):
    from asrx.optim import MaxFactor

    groups = [{"params": [d for d, (_, gi) in zip(dev_params, ref.SHAPES) if gi == 0], "bias": 1.0},
              {"params": [d for d, (_, gi) in zip(dev_params, ref.SHAPES) if gi == 1], "bias": 2.0}]
    return MaxFactor(groups, **dict(ref.HP, **over))


def _device_params(cuda):
    return [p.to(cuda).requires_grad_(True) for p in ref.make_params()]


def _snapshot(opt, dev):
    return [[d.detach().clone()] + [opt.state[d][k].clone() for k in STATE if k in opt.state[d]] for d in dev]


def _assert_equal(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y)
        for u, v in zip(x, y):
            assert torch.equal(u, v), ref.SHAPES[i]


def _assert_state_close(opt, dev, states):
    for i, d in enumerate(dev):
        for k in STATE:
            if k in states[i] and (k != "v" or d.dim() <= 1):
                assert ref.rel(opt.state[d][k], states[i][k]) < 1e-5, (ref.SHAPES[i], k)


def test_power_of_two_scale_is_exact(cuda):
    """Gradients 1024 g under inv_scale = 1 / 1024 give the bits of a plain run on g."""
    from asrx.optim import GradStats

    a, b = _device_params(cuda), _device_params(cuda)
    oa, ob = _optimizer(a), _optimizer(b)
    stats = GradStats(b, max_norm=0.0)
    gen = torch.Generator().manual_seed(1)
    for _ in range(3):
        for x, y, g in zip(a, b, ref.make_grads(gen)):
            x.grad, y.grad = g.to(cuda), (g * 1024).to(cuda)
        oa.step()
        ob.step(grad_ctl=stats.measure(inv_scale=1.0 / 1024))
    torch.cuda.synchronize()
    assert float(stats.coef) == 1.0 / 1024 and float(stats.found_inf) == 0.0
    _assert_equal(_snapshot(oa, a), _snapshot(ob, b))
    assert ob.sync_skips() == 0 and all(float(ob.state[d]["step"]) == 3 for d in b)


def test_norm_clip_matches_oracle(cuda):
    """max_norm below the measured norm: the step is the oracle's on g * coef."""
    from asrx.optim import GradStats

    dev = _device_params(cuda)
    cpu = [p.double() for p in ref.make_params()]
    states = [omf.init_state(p) for p in cpu]
    opt = _optimizer(dev)
    gen = torch.Generator().manual_seed(1)
    for it in range(3):
        grads = ref.make_grads(gen)
        norm = float(torch.stack([g.double().square().sum() for g in grads]).sum().sqrt())
        max_norm = 0.25 * norm
        coef64 = min(1.0, max_norm / (norm + 1e-6))
        assert coef64 < 0.26
        for d, g in zip(dev, grads):
            d.grad = g.to(cuda)
        stats = GradStats(dev, max_norm=max_norm).measure()
        opt.step(grad_ctl=stats)
        for i, g in enumerate(grads):
            omf.step_param(cpu[i], g.double() * coef64, states[i], ref.group_of(i))
        torch.cuda.synchronize()
        assert abs(float(stats.coef) - coef64) < 1e-5 * coef64
        for i, (d, r) in enumerate(zip(dev, cpu)):
            assert ref.rel(d, r) < 2e-6, (it, ref.SHAPES[i], ref.rel(d, r))
    _assert_state_close(opt, dev, states)


def test_skipped_step_leaves_no_trace(cuda):
    """[good, bad, good, good]: the bad step (one NaN) changes nothing, and does not count."""
    from asrx.optim import GradStats

    dev = _device_params(cuda)
    cpu = [p.double() for p in ref.make_params()]
    states = [omf.init_state(p) for p in cpu]
    opt = _optimizer(dev)
    stats = GradStats(dev)
    gen = torch.Generator().manual_seed(1)
    for it in range(4):
        grads = ref.make_grads(gen)
        bad = it == 1
        if bad:
            grads[5].view(-1)[1234] = float("nan")
        for d, g in zip(dev, grads):
            d.grad = g.to(cuda)
        before = _snapshot(opt, dev)
        opt.step(grad_ctl=stats.measure())
        torch.cuda.synchronize()
        assert float(stats.found_inf) == float(bad)
        if bad:
            _assert_equal(before, _snapshot(opt, dev))
            continue
        for i, g in enumerate(grads):
            omf.step_param(cpu[i], g.double(), states[i], ref.group_of(i))
        # beta_t at t = 2 and t = 3 differ by ~38 %: a count that advanced on the bad step cannot pass
        for i, (d, r) in enumerate(zip(dev, cpu)):
            assert ref.rel(d, r) < 2e-6, (it, ref.SHAPES[i], ref.rel(d, r))
    assert opt.sync_skips() == 1
    assert all(float(opt.state[d]["step"]) == 3 for d in dev)
    assert all(float(v["step"]) == 3 for v in opt.state_dict()["state"].values())
    _assert_state_close(opt, dev, states)


def test_skip_as_last_step_is_settled_by_state_dict(cuda):
    from asrx.optim import GradStats

    dev = _device_params(cuda)
    opt = _optimizer(dev)
    stats = GradStats(dev)
    gen = torch.Generator().manual_seed(1)
    for it in range(2):
        grads = ref.make_grads(gen)
        if it == 1:
            grads[0][0, 0] = float("inf")
        for d, g in zip(dev, grads):
            d.grad = g.to(cuda)
        opt.step(grad_ctl=stats.measure())
    assert all(float(v["step"]) == 1 for v in opt.state_dict()["state"].values())
    assert opt.sync_skips() == 1


BINDING_CAP = 1.0e-3  # 0.4 lr: found on the CPU with the float64 restatement (see the counts asserted below)


@pytest.mark.parametrize("cap", [1e6, 0.0, BINDING_CAP])
def test_update_rms_cap(cuda, cap):
    dev = _device_params(cuda)
    cpu = [p.double() for p in ref.make_params()]
    states = [omf.init_state(p) for p in cpu]
    opt = _optimizer(dev, clip=True, cap=cap)
    if cap == 1e6:
        plain = _device_params(cuda)
        opt_plain = _optimizer(plain)
    gen = torch.Generator().manual_seed(1)
    bound = free = 0
    for it in range(3):
        grads = ref.make_grads(gen)
        for i, (d, g) in enumerate(zip(dev, grads)):
            d.grad = g.to(cuda)
            ratio = ref.step_param(cpu[i], g.double(), states[i], ref.group_of(i, clip=True, cap=cap))
            assert abs(ratio - 1) > 1e-3, (it, ref.SHAPES[i], ratio)  # no case decided by fp32 rounding
            bound += ratio > 1
            free += ratio < 1
        opt.step()
        if cap == 1e6:
            for d, g in zip(plain, grads):
                d.grad = g.to(cuda)
            opt_plain.step()
        torch.cuda.synchronize()
        for i, (d, r) in enumerate(zip(dev, cpu)):
            assert ref.rel(d, r) < 2e-6, (it, ref.SHAPES[i], ref.rel(d, r))
    _assert_state_close(opt, dev, states)
    n = 3 * len(ref.SHAPES)
    if cap == 1e6:  # never binds: the bits of a clip=False run
        assert (bound, free) == (0, n)
        _assert_equal(_snapshot(opt, dev), _snapshot(opt_plain, plain))
    elif cap == 0.0:  # always binds with a zero allowance: only the decay multiply is left
        assert (bound, free) == (n, 0)
        keep = (1 - ref.HP["lr"] * ref.HP["decay"]) ** 3
        for i, (d, p0) in enumerate(zip(dev, ref.make_params())):
            assert ref.rel(d, p0.double() * keep) < 2e-6, ref.SHAPES[i]
    else:  # both branches of the comparison are exercised, per the float64 reference alone
        print("cap binds for", bound, "parameter steps and not for", free)
        assert bound >= 1 and free >= 1
        per_param = [states[i]["step"] for i in range(len(cpu))]
        assert per_param == [3] * len(cpu)
