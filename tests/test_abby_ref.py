"""The float64 AbbyNormal reference of tests/abby_ref.py is honest before tests/test_gpu_abby_ref.py relies on it (no
GPU here): it equals oracle.model.abby_normal, its float32 evaluation is inside every bound, every listed mutation
is outside one (the failure message names the case that was tried last), the null mutation is shown to be null,
and the input recipes keep their promises -- exclusion caps, every mode and both arms of mode 2 among the checked
rows, tied maxima where first and last argmax differ -- for every case the GPU test runs.
"""
import pytest
import torch
import torch.nn.functional as F

import abby_ref as A

FWD_CASES = [(tier, d, r) for tier in ("mixed", "ties") for d in A.DS for r in A.SMALL_ROWS]
FWD_CASES += [("mixed", d, r) for d, r in A.FWD_WRAP]
BWD_CASES = [(tier, d, r) for tier in ("mixed", "ties") for d in A.DS for r in A.SMALL_ROWS]
BWD_CASES += [(tier, d, r) for tier in ("mixed", "ties") for d, r in A.BWD_WRAP]


def _id(c):
    return f"{c[0]}-d{c[1]}-r{c[2]}"


def test_max_pool_routes_a_tie_to_its_first_position():
    x = torch.tensor([[[1.0, 2, 2, 2, 1, 2, 2]]], dtype=torch.float64, requires_grad=True)
    F.max_pool1d(x, 3, 1, 1).sum().backward()
    assert x.grad.flatten().tolist() == [0, 3, 1, 1, 0, 2, 0]


def test_wrap_counts_end_ragged_in_both_arms():
    """From the grid caps read in abby.hip (asrx_abby_fwd*: min(ceil(rows / 4), 4096) workgroups of 4 waves;
    asrx_abby_bwd2: 1024; at d = 64 a wave takes 4 rows, so the backward sweeps 1024 x 16 rows), so that a change of
    the caps fails here instead of leaving the wrap cases short of a wrap: each wrap count ends in a partial
    workgroup, the `+ 3` ones in the second sweep -- the second arm of the loops unrolled by two, or the second trip
    of the AHEAD == 1 loop -- and the `+ 5` ones in the third, the first arm again."""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "asr-model_amd", "csrc", "abby.hip")).read()
    waves = int(re.search(r"constexpr int ABBY_WAVES = (\d+);", src).group(1))

    ROW = r"std::min<int64_t>\(\(rows \+ ABBY_WAVES - 1\) / ABBY_WAVES, (\d+)\)"  # one row per wave
    ROW4 = r"std::min<int64_t>\(\(rows \+ 4 \* ABBY_WAVES - 1\) / \(4 \* ABBY_WAVES\), (\d+)\)"  # d = 64: four

    def caps(entry, pat):
        """The grid caps of that form in the body of one entry point."""
        body = src[src.index(f'extern "C" int {entry}('):]
        return {int(v) for v in re.findall(pat, body[:body.index("\n}\n")])}

    for entry in ("asrx_abby_fwd2", "asrx_abby_fwd_logits2", "asrx_abby_fwd3", "asrx_abby_fwd_res"):
        assert caps(entry, ROW) == {A.FWD_SWEEP // waves}, entry
    assert caps("asrx_abby_bwd2", ROW) == {A.BWD_SWEEP // waves}
    assert caps("asrx_abby_bwd2", ROW4) == {A.BWD64_SWEEP // (4 * waves)}
    assert waves == 4 and A.FWD_SWEEP == 16384 and A.BWD_SWEEP == 4096 and A.BWD64_SWEEP == 4 * 4096

    def last(rows, sweep, per_wg):
        assert rows % per_wg != 0  # ragged: the last workgroup is partial
        return (rows - 1) // sweep  # the sweep that holds the last row

    assert [last(r, A.FWD_SWEEP, 4) for _, r in A.FWD_WRAP] == [1, 2, 1]
    bw = [(d, last(r, A.BWD64_SWEEP if d == 64 else A.BWD_SWEEP, 16 if d == 64 else 4)) for d, r in A.BWD_WRAP]
    assert bw == [(128, 1), (128, 2), (384, 1), (384, 2), (768, 1), (1024, 1), (64, 1)]
    assert {d for d, _ in A.BWD_WRAP if d >= 768} == {768, 1024}  # both AHEAD == 1 instantiations wrap


def test_equals_the_oracle():
    """One small case through oracle.model.abby_normal (float64, with gumbel noise): equal forward values, and the
    same gradients to rounding."""
    from oracle import model as om

    d, rows = 128, 9
    t = A.data("mixed", d, rows)
    g = A.gen(5)
    W1 = torch.randn(d, d, generator=g, dtype=torch.float64) / 8
    b1 = torch.randn(d, generator=g, dtype=torch.float64) * 0.2
    gum = torch.randn(rows, 3, generator=g, dtype=torch.float64)
    P = {"n.mode_router.0.weight": W1, "n.mode_router.0.bias": b1, "n.mode_router.2.weight": t.W2,
         "n.mode_router.2.bias": t.b2}
    x = t.x.clone().requires_grad_(True)
    want = om.abby_normal(P, "n", x, gum)
    hpre = F.linear(t.x, W1, b1)
    got = A.forward(t.x, hpre=hpre, W2=t.W2, b2=t.b2, gumbel=gum)
    assert torch.equal(got.out, want.detach())
    assert len(set(got.idx.tolist())) > 1
    want.backward(t.gy)
    b = A.backward(t.x, hpre, t.W2, t.b2, gum, t.gy, got.idx)
    dx = b.dx + b.dhpre @ W1  # the host's share of dx
    assert A.row_err(dx, x.grad) < 1e-12


def _fwd_case(case, form):
    t = A.data(*case)
    r64, r32 = A.fwd_pair(t, form, tw=t.tw, tb=t.tb)
    keep = A.keep_fwd(r64, form, case[0])
    return t, r64, r32, keep


@pytest.mark.parametrize("case", FWD_CASES, ids=_id)
def test_forward_case(case):
    """float32 inside the bounds; exclusion cap; modes and arms among the checked rows; tie shares."""
    tier, d, rows = case
    for form in ("logits", "hpre") if tier == "mixed" else ("logits",):  # the ties tier forces mode 2: logits only
        t, r64, r32, keep = _fwd_case(case, form)
        e32 = A.fwd_errors(r32, r64, keep, d)
        A.check(f"f32 {_id(case)} {form}", e32, e32)
        # the yardstick itself is a few fp32 roundings (tc: a d-term dot product whose row can cancel)
        assert all(v < (1e-4 if k == "tc" else 1e-5) for k, v in e32.items()), e32
        assert float((~keep).float().mean()) <= A.CAP, (case, form, int((~keep).sum()))
        assert torch.equal(r32.ys.argmax(-1)[keep], r64.idx[keep])
        if form == "logits":
            # 1 - 2 x 0.3: holds because the mode control's normal draw is clamped to [-1, 1] (abby_ref.py, modes)
            assert torch.equal(r64.idx, t.modes) and float(r64.zgap.min()) >= 0.39
            assert float(r64.ys.max()) < 0.8  # far from saturation
        m2 = keep & (r64.idx == 1)
        cond = r64.cond[m2]
        if tier == "ties":
            assert float(r64.cmargin.min()) >= 1e-5
        if rows >= 74:
            assert set(r64.idx[keep].tolist()) == {0, 1, 2} or (tier == "ties" and form == "logits")
            assert bool(cond.any()) and not bool(cond.all())
            share = float(cond.float().mean())
            both = float((cond.any(-1) & ~cond.all(-1)).float().mean())
            if tier == "mixed":
                assert 0.15 <= share <= 0.45 and both >= 0.6, (case, form, share, both)
                assert float(r64.base.max()) > 4.0 and float(r64.base.min()) == 1.0
            elif d >= 128:
                assert 0.4 <= share <= 0.6, (case, share)


@pytest.mark.parametrize("d", A.DS)
def test_ties_tier_has_tied_maxima(d):
    """Windows with `cond` true and a tied maximum: first and last argmax differ exactly there (d >= 128; at d = 64,
    W = 3, a tied maximum can never exceed 2 avg, so the tier checks only the forward)."""
    t = A.data("ties", d, 74)
    W, pad = A.window(d)
    sq = F.pad(t.x * t.x, (pad, pad), value=-1.0).unfold(-1, W, 1)  # (rows, d, W)
    mx = sq.amax(-1, keepdim=True)
    first = (sq == mx).float().argmax(-1)
    last = W - 1 - (sq == mx).flip(-1).float().argmax(-1)
    tied = (sq == mx).sum(-1) > 1
    cond = mx.squeeze(-1) > 2.0 * sq.clamp_min(0).sum(-1) / W
    assert torch.equal(first != last, tied)
    share = float((cond & tied).float().mean())
    if d == 64:
        assert share == 0.0
    else:
        assert 0.1 <= share <= 0.6, share


@pytest.mark.parametrize("case", BWD_CASES, ids=_id)
def test_backward_case(case):
    tier, d, rows = case
    t = A.data(*case)
    r64, r32, keep, gy = A.bwd_pair(t)
    if tier == "ties":
        assert bool(keep.all())
    assert float((~keep).float().mean()) <= A.CAP, (case, int((~keep).sum()))
    assert torch.equal(r64.idx, t.modes)
    e32 = A.bwd_errors(r32, r64, keep)
    A.check(f"f32 {_id(case)} bwd", e32, e32)
    # the yardstick: dx a few fp32 roundings; dz is a difference of row sums, so dhpre per row, and dW2 / db2 at
    # few rows, carry the row's cancellation (up to 2e-2 on a row of the largest cases)
    assert e32["dx"] < 1e-5 and e32["dhpre"] < 0.1 and max(e32["dW2"], e32["db2"]) < 1e-2, e32
    assert float(r64.dhpre[r64.dead].abs().max() if bool(r64.dead.any()) else 0.0) == 0.0
    if rows >= 74:
        cond = r64.cond[keep & (r64.idx == 1)]
        assert bool(cond.any()) and not bool(cond.all())
        assert float(r64.dhpre.abs().max()) > 0 and float(r64.dW2.abs().max()) > 0


# which output shows a mutation, and on which tier
MUT_WHERE = {
    "window": ("fwd", "mixed", "out"), "avg_shift": ("fwd", "mixed", "out"), "avg_count": ("fwd", "mixed", "edge"),
    "thr22": ("fwd", "mixed", "out"), "mode2_avg": ("fwd", "mixed", "out"), "last_argmax": ("bwd", "ties", "dx"),
    "nrm_nosqrt": ("fwd", "mixed", "nrm"), "tc_after_res": ("fwd", "mixed", "tc"), "dx_no_pool": ("bwd", "mixed", "dx"),
    "dW2_hpre": ("bwd", "mixed", "dW2"),
}


def _mutated(mut, kind, case):
    """(errors of the mutated float64 reference, bounds from the float32 evaluation) of one case."""
    t = A.data(*case)
    if kind == "fwd":
        kw = dict(res=t.res, tw=t.tw, tb=t.tb)
        r64, r32 = A.fwd_pair(t, "logits", **kw)
        keep = A.keep_fwd(r64, "logits")
        with torch.no_grad():
            m = A.forward(t.x, logits=t.logits, b2=t.b2, mut=mut, **kw)
        return A.fwd_errors(m, r64, keep, case[1]), A.bounds(A.fwd_errors(r32, r64, keep, case[1]))
    r64, r32, keep, gy = A.bwd_pair(t)
    m = A.backward(t.x, t.hpre, t.W2, t.b2, t.gumbel, gy, r64.idx, mut=mut)
    return A.bwd_errors(m, r64, keep), A.bounds(A.bwd_errors(r32, r64, keep))


def test_mutation_table_is_the_reference_list():
    assert set(MUT_WHERE) == set(A.MUTATIONS) and not set(A.NULL_MUTATIONS) & set(A.MUTATIONS)


@pytest.mark.parametrize("mut", A.MUTATIONS)
def test_mutation_is_caught(mut):
    """Every d at 74 rows: the mutation is outside the bound of its output at EVERY d that can show it (last_argmax
    needs d >= 128), so no instantiation hides it."""
    kind, tier, key = MUT_WHERE[mut]
    for d in A.DS:
        if mut == "last_argmax" and d == 64:
            continue
        case = (tier, d, 74)
        e, b = _mutated(mut, kind, case)
        print(f"MUTATION {mut:<12s} {_id(case)} {key}: e={e[key]:.2e} bound={b[key]:.2e}")
        assert e[key] > b[key], (f"mutation {mut} not caught on {key} of case {_id(case)}: e={e[key]:.3e} "
                                 f"bound={b[key]:.3e}")


@pytest.mark.parametrize("mut", A.NULL_MUTATIONS)
def test_null_mutation_is_not_detectable(mut):
    """biased_std: inside every bound of every output, forward and backward, at every d -- no test can see it."""
    for d in A.DS:
        for kind, tier in (("fwd", "mixed"), ("bwd", "mixed"), ("bwd", "ties")):
            e, b = _mutated(mut, kind, (tier, d, 74))
            assert all(e[k] <= b[k] for k in e), (mut, d, kind, e, b)
            assert all(e[k] < 1e-9 for k in e if k not in ("dhpre", "dW2", "db2")), (mut, d, kind, e)
