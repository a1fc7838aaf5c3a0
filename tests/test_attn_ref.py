"""The bounds of tests/attn_ref.py proven on the CPU: this decides whether test_gpu_attn_ref.py means anything.

1. A float64 model of the kernels' documented roundings stays inside the bounds, max(err / bound) < 1 over EVERY
   element of O, dQ, dK, dV (and Delta inside bDelta, lse inside its tolerance), for every case the GPU test runs:
   both tests parametrise over attn_ref.CASES.  Worst ratio of the model per group (measured, printed by
   test_model_worst_ratio_per_group):

       family   hd   O      dQ     dK     dV     Delta
       unit     64   0.752  0.133  0.164  0.463  0.084
       unit    128   0.834  0.120  0.144  0.440  0.065
       peaked6  64   0.865  0.123  0.157  0.473  0.075
       peaked6 128   0.827  0.103  0.116  0.435  0.043
       peaked2  64   0.549  0.097  0.164  0.409  0.042   (q[..., :8] *= 512: max |S| 650 .. 1100, 350 .. 2300 rows
       peaked2 128   0.498  0.092  0.128  0.406  0.030    with one P above 0.99; the score-accumulation term widens it)
       flat     64   0.678  0.190  0.029  0.425  0.190
       flat    128   0.762  0.132  0.021  0.458  0.133

2. The same formulas in torch float32 stay inside the parity bound: 0.1 .. 0.6 of it at unit-scale inputs, 0.05 ..
   0.09 at the peaked2 ones, where the bound is the worst case of hd roundings of a score of 1e3.
3. A mutated model leaves the bounds: causal mask off by one, key 64 dropped, the last partial key tile ignored,
   the scale missing from dK, Delta without the RD rounding, non-zero dK / dV of keys no query sees.  Those that do
   NOT (INSIDE below, asserted so that the record stays true):
   - "delta_nord" never does, at any case (dQ and dK stay at the unmutated model's own figures, 0.2 at most): bDelta
     carries u |dO| |O| exactly where the Delta pass rounds dO, and that term is as large as the whole effect of
     leaving the rounding out.  This harness cannot tell an unrounded Delta from a rounded one; the model-level
     parity record (test_parity_record.py) is what guards that.
   - "droptail" at causal 129 x 129 with the peaked2 inputs: the tail is key 128, which only query 128 sees, and
     that row is one-hot on another key.
   - "noscale_dk" at 3700 x 8 (the Delta-loop case): with flat values dK is rounding noise, 0.3 of its bound even
     when 8 (or 11) times too large.
   - o stored bf16 with Delta's bound NOT widened for it: O leaves the bound (1.07 .. 1.49, the stored value's own
     rounding) but dQ and dK stay inside (0.38 and 0.06 at most), which agrees with model.py's note that a bf16
     o is harmless to the parameter gradients once dO is rounded consistently.
"""
import collections
import functools

import pytest

import attn_ref as R

PERF = [c for c in R.CASES if c.mode == "perf"]
PARITY = [c for c in R.CASES if c.mode == "parity"]
# the mutations run where the layout and the forward variant (the same numbers on the CPU) are the plain ones
MUT = [(c, m) for c in PERF if c.layout == "contig" and c.variant == 1 for m in R.MUTATIONS
       if R.mutation_applies(c, m)]


def _inside(case, m):
    return (m == "delta_nord" or (m == "droptail" and (case.Lq, case.Lk, case.family) == (129, 129, "peaked2"))
            or (m == "noscale_dk" and (case.Lq, case.Lk) == (3700, 8)))


@functools.lru_cache(maxsize=8)
def _ref(case):
    raw, vis = R.make_inputs(case)
    return raw, vis, R.reference_for(case, vis)


@functools.lru_cache(maxsize=None)
def _model(case):
    """Ratios of the unmutated rounding model: {O, dQ, dK, dV, Delta, lse: (value, ...)}."""
    raw, vis, ref = _ref(case)
    mod = R.rounding_model(vis["q"], vis["k"], vis["v"], vis["dO"], case.causal, case.scale, bool(case.io & 2))
    out = {n: r for n, (r, _) in R.ratios(mod, ref).items()}
    out["Delta"], _ = R.ratio(mod["Delta"], ref["Delta"], ref["bDelta"])
    out["lse"] = float((mod["lse"] - ref["lse"]).abs().max()) / R.lse_tolerance(case, vis, ref["lse"])
    return out


def test_cases_cover_the_issue():
    """The shapes, both head dims, both forward variants, the four input families, all eight storage
    combinations, three layouts in both storage types, and the two-pass Delta loop are all in attn_ref.CASES."""
    shapes = {(c.Lq, c.Lk, c.causal) for c in R.CASES}
    assert {(a, b, False) for a, b in R.NONCAUSAL} | {(a, b, True) for a, b in R.CAUSAL} <= shapes
    for mode in ("perf", "parity"):
        cs = [c for c in R.CASES if c.mode == mode]
        assert {(c.Lq, c.Lk, c.causal) for c in cs} >= shapes - {(3700, 8, False)} and {c.hd for c in cs} == {64, 128}
        assert {(c.B, c.H) for c in cs} >= {(1, 1), (2, 3)}
        assert {c.layout for c in cs} == {"contig", "kvpad", "headmajor"}
        assert {c.family for c in cs} >= {"unit", "peaked6", "peaked2", "flat"}
    for hd in (64, 128):
        assert {c.io for c in PERF if c.hd == hd} == set(range(8))
        assert {(c.layout, c.io) for c in PERF if c.hd == hd} >= {(lay, io) for lay in ("kvpad", "headmajor")
                                                                   for io in (0, 7)}
        assert {c.io for c in PERF if c.hd == hd and c.B * c.H * c.Lq > 32768} >= {0, 6}
    assert {c.variant for c in PERF if c.hd == 64} == {0, 1}
    assert all(c.B * c.H * c.Lq <= 2 * 32768 for c in R.CASES)  # the Delta loop case is two passes, no more


@pytest.mark.parametrize("case", PERF, ids=[c.id for c in PERF])
def test_rounding_model_within_bounds(case):
    r = _model(case)
    print(case.id, {k: round(v, 3) for k, v in r.items()})
    for name, v in r.items():
        assert v < 1.0, (name, v)


def test_model_worst_ratio_per_group():
    worst = collections.defaultdict(lambda: collections.defaultdict(float))
    for c in PERF:
        for k, v in _model(c).items():
            worst[(c.family, c.hd)][k] = max(worst[(c.family, c.hd)][k], v)
    for key in sorted(worst):
        print(key, {k: round(v, 3) for k, v in worst[key].items()})
    assert max(max(w.values()) for w in worst.values()) < 1.0
    # the bounds are not slack either: the model uses 0.4 of bO and a third of bV in every group
    assert all(w["O"] > 0.4 and w["dV"] > 0.3 for w in worst.values())


def test_peaked_level():
    """PEAK2 is the largest candidate; with it the scores reach 1e2 .. 1e3 and many rows are near one-hot, and the
    rounding model stays under 1 (worst 0.549, O)."""
    assert R.PEAK2 == max(R.PEAK2_CANDIDATES)
    cs = [c for c in PERF if c.family == "peaked2"]
    assert len(cs) >= 8
    for c in cs:
        ref = _ref(c)[2]
        assert 1e2 < float(ref["smax"].max()) < 2e3
        assert int((ref["P"].amax(-1) > 0.99).sum()) >= 100
        assert max(v for k, v in _model(c).items()) < 1.0


@pytest.mark.parametrize("case", PARITY, ids=[c.id for c in PARITY])
def test_parity_bound_holds_for_torch_fp32(case):
    """softmax attention and its gradients evaluated in torch float32 (no bf16 rounding) against the float64
    reference: inside the parity bound u = (Lk + hd + 8) 2^-24."""
    raw, vis, ref = _ref(case)
    f = {k: v.float() for k, v in vis.items()}
    mod = R.rounding_model(f["q"], f["k"], f["v"], f["dO"], case.causal, case.scale, rnd=lambda x: x)
    rr = R.ratios(mod, ref)
    print(case.id, {k: round(v[0], 3) for k, v in rr.items()})
    for name, (v, idx) in rr.items():
        assert v < 1.0, R.where(case, name, idx)
    assert R.ratio(mod["Delta"], ref["Delta"], ref["bDelta"])[0] < 1.0
    assert float((mod["lse"].double() - ref["lse"]).abs().max()) < R.lse_tolerance(case, vis, ref["lse"])


@pytest.mark.parametrize("case,m", MUT, ids=[f"{c.id}-{m}" for c, m in MUT])
def test_mutation_leaves_the_bounds(case, m):
    raw, vis, ref = _ref(case)
    mod = R.rounding_model(vis["q"], vis["k"], vis["v"], vis["dO"], case.causal, case.scale, bool(case.io & 2),
                           mutate=m, dO_raw=raw["dO"].double())
    worst = max(v for v, _ in R.ratios(mod, ref).values())
    print(case.id, m, worst)
    if _inside(case, m):
        assert worst < 1.0  # the recorded exceptions (module docstring)
    else:
        assert worst > 1.0


def test_every_mutation_is_exercised():
    for m in R.MUTATIONS:
        hit = [c for c, mm in MUT if mm == m and not _inside(c, m)]
        assert len(hit) >= (0 if m == "delta_nord" else 4), m
    # the two masks are caught by orders of magnitude, not by a whisker
    c = next(c for c in PERF if (c.Lq, c.Lk, c.causal, c.family, c.io) == (257, 257, True, "unit", 0))
    raw, vis, ref = _ref(c)
    for m, floor in (("causal+1", 100.0), ("drop64", 5.0)):
        mod = R.rounding_model(vis["q"], vis["k"], vis["v"], vis["dO"], c.causal, c.scale, mutate=m)
        assert max(v for v, _ in R.ratios(mod, ref).values()) > floor


STORED_O = [c for c in PERF if c.io & 2 and c.layout == "contig"]


@pytest.mark.parametrize("case", STORED_O, ids=[c.id for c in STORED_O])
def test_bf16_o_against_the_unwidened_bound(case):
    """o stored bf16, judged by the bounds of an fp32 o (no u |dO| |O| in bDelta beyond RD's, no u |O| in bO): O
    itself leaves its bound, dQ and dK do not (module docstring)."""
    raw, vis, _ = _ref(case)
    ref = R.reference(vis["q"], vis["k"], vis["v"], vis["dO"], case.causal, case.scale, case.u, case.rd, False)
    mod = R.rounding_model(vis["q"], vis["k"], vis["v"], vis["dO"], case.causal, case.scale, True)
    rr = {k: v for k, (v, _) in R.ratios(mod, ref).items()}
    print(case.id, rr)
    assert rr["O"] > 1.0 and rr["dQ"] < 1.0 and rr["dK"] < 1.0
