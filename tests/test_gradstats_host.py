"""Host side of the step seam (asrx.optim.GradStats, MaxFactor clip / cap): record layout, argument
checks, and the float64 clip restatement (tests/maxfactor_clip_ref.py) pinned to oracle/maxfactor.py."""
import pytest
import torch

import maxfactor_clip_ref as ref
from oracle import maxfactor as omf


def test_grad_stats_record_layout():
    from asrx import lib, optim

    assert optim._GREC.itemsize == lib.load().asrx_grad_stats_param_bytes() == 24
    assert optim._REC.itemsize == lib.load().asrx_maxfactor_param_bytes()
    # a record packed without clip keeps zero in its last slot, and zero means "no cap"
    assert optim._REC.names[-1] == "cap" and optim._REC.fields["cap"][1] == optim._REC.itemsize - 4
    assert {"asrx_grad_stats", "asrx_grad_stats_param_bytes", "asrx_maxfactor_step_ex"} <= set(lib.SIGNATURES)


def test_grad_stats_refuses_cpu_tensors():
    from asrx.optim import GradStats, MaxFactor

    p = torch.zeros(5, requires_grad=True)
    p.grad = torch.ones(5)
    with pytest.raises(RuntimeError, match="device tensors"):
        GradStats([("p", p)]).measure()
    with pytest.raises(RuntimeError, match="device tensors"):
        MaxFactor([p]).step()
    q = torch.zeros(3, requires_grad=True)  # nothing to measure is an error, not an empty result
    with pytest.raises(ValueError):
        GradStats([q]).measure()
    with pytest.raises(RuntimeError, match="measure"):
        GradStats([q]).ctl


def test_grad_stats_accepts_names_or_bare_parameters():
    from asrx.optim import GradStats

    a, b = torch.zeros(2), torch.zeros(3)
    assert [n for n, _ in GradStats([("x", a), ("y", b)])._params] == ["x", "y"]
    assert [n for n, _ in GradStats([a, b])._params] == ["0", "1"]
    assert [n for n, _ in GradStats(torch.nn.Linear(2, 2).named_parameters())._params] == ["weight", "bias"]


def test_maxfactor_clip_arguments():
    from asrx.optim import MaxFactor

    p = torch.zeros(4, requires_grad=True)
    with pytest.raises(ValueError):
        MaxFactor([p], clip=True, cap=-1)
    with pytest.raises(ValueError):
        MaxFactor([p], clip=True, cap=float("nan"))
    opt = MaxFactor([p], clip=True, cap=0.5)  # no longer raises
    assert opt.param_groups[0]["clip"] and opt.param_groups[0]["cap"] == 0.5
    assert opt.sync_skips() == 0 and opt.state_dict()["state"] == {}


def test_clip_restatement_matches_oracle_without_clip():
    """clip=False: the restatement is oracle/maxfactor.py to float64 rounding, over 3 steps."""
    a = [p.double() for p in ref.make_params()]
    b = [p.clone() for p in a]
    sa, sb = [omf.init_state(p) for p in a], [omf.init_state(p) for p in b]
    gen = torch.Generator().manual_seed(1)
    for _ in range(3):
        for i, g in enumerate(ref.make_grads(gen)):
            omf.step_param(a[i], g.double(), sa[i], ref.group_of(i))
            assert ref.step_param(b[i], g.double(), sb[i], ref.group_of(i)) is None
    for i in range(len(a)):
        assert ref.rel(b[i], a[i]) < 1e-14, ref.SHAPES[i]
        for k in sa[i]:
            if k != "step":
                assert ref.rel(sb[i][k], sa[i][k]) < 1e-13, (ref.SHAPES[i], k)
        assert sa[i]["step"] == sb[i]["step"] == 3


def test_clip_restatement_cap_semantics():
    """A huge cap never binds (equal to clip=False); cap=0 leaves only the decay multiply."""
    p0 = [p.double() for p in ref.make_params()]
    gen = torch.Generator().manual_seed(1)
    grads = ref.make_grads(gen)
    for i, g in enumerate(grads):
        a, b, c = p0[i].clone(), p0[i].clone(), p0[i].clone()
        ref.step_param(a, g.double(), omf.init_state(a), ref.group_of(i))
        r = ref.step_param(b, g.double(), omf.init_state(b), ref.group_of(i, clip=True, cap=1e6))
        assert r < 1 and torch.equal(a, b)
        ref.step_param(c, g.double(), omf.init_state(c), ref.group_of(i, clip=True, cap=0.0))
        assert torch.equal(c, p0[i] * (1 - ref.HP["lr"] * ref.HP["decay"]))


def test_native_tensor_limit_is_an_error():
    """More gradients than the kernel's offset table holds fails with a message, before any launch."""
    from asrx import lib, optim

    with pytest.raises(RuntimeError, match="at most 4096 gradients"):
        lib.call("asrx_grad_stats", 0, optim.GS_MAX_TENSORS + 1, 1, 1.0, 0.0, 1e-6, 0, 0, 0)
    with pytest.raises(RuntimeError, match="no gradients"):
        lib.call("asrx_grad_stats", 0, 0, 0, 1.0, 0.0, 1e-6, 0, 0, 0)
