"""Attention with per-sample lengths, on the CPU: what test_gpu_attn_lens.py judges the kernels by.

1. The two proofs of test_attn_ref.py over every per-sample case of attn_lens_cases.RAGGED (a B = 1 attn_ref.Case of
   each sample's own lengths): the float64 rounding model of the perf kernels stays inside the componentwise bounds,
   and torch float32 stays inside the parity bound.  Worst err / bound of the model over these cases: 0.818 (O),
   0.443 (dV), 0.146 (dK), 0.117 (dQ), 0.132 (Delta); torch fp32 against the parity bound 0.015 at most.
2. The stated semantics, independently of any kernel: a float64 attention over the zero-padded batch with the keys
   at or past k_len masked to -inf and the output rows at or past q_len set to zero equals, on the live region, the
   per-sample attn_ref.reference, and its gradients are exactly zero on the dead rows of q, k and v whatever the
   incoming gradient holds there.
"""
import pytest
import torch

import attn_lens_cases as L
import attn_ref as R

PERF = [c for c in L.SAMPLES if c.mode == "perf"]
PARITY = [c for c in L.SAMPLES if c.mode == "parity"]


def test_cases_cover_the_edges():
    assert {r.launch for r in L.RAGGED} == set(L.LAUNCHES)
    for la, (causal, (Lq, Lk), lens) in L.LAUNCHES.items():
        assert max(a for a, _ in lens) == Lq and max(b for _, b in lens) == Lk  # the launch is the padded batch
        for mode in ("perf", "parity"):
            assert {r.hd for r in L.RAGGED if r.launch == la and r.mode == mode} == {64, 128}
    for la in L.LARGE:
        rs = [r for r in L.RAGGED if r.launch == la]
        assert {(r.family, r.io) for r in rs if r.layout == "contig"} >= {("unit", 0), ("flat", 7)}
        assert {r.io for r in rs if r.layout == "kvpad"} == {0, 7}
        assert {r.variant for r in rs if r.hd == 64} == {0, 1}
    lens = {x for _, _, ls in L.LAUNCHES.values() for x in ls}
    assert {(256, 257), (33, 64), (1, 1), (65, 65), (70, 300), (300, 70), (257, 65), (31, 256)} <= lens


@pytest.mark.parametrize("case", PERF, ids=[c.id for c in PERF])
def test_rounding_model_within_bounds(case):
    raw, vis, ref = L.sample(case)
    mod = R.rounding_model(vis["q"], vis["k"], vis["v"], vis["dO"], case.causal, case.scale, bool(case.io & 2))
    out = {n: r for n, (r, _) in R.ratios(mod, ref).items()}
    out["Delta"], _ = R.ratio(mod["Delta"], ref["Delta"], ref["bDelta"])
    out["lse"] = float((mod["lse"] - ref["lse"]).abs().max()) / R.lse_tolerance(case, vis, ref["lse"])
    print(case.id, {k: round(v, 3) for k, v in out.items()})
    for name, v in out.items():
        assert v < 1.0, (name, v)


@pytest.mark.parametrize("case", PARITY, ids=[c.id for c in PARITY])
def test_parity_bound_holds_for_torch_fp32(case):
    raw, vis, ref = L.sample(case)
    f = {k: v.float() for k, v in vis.items()}
    mod = R.rounding_model(f["q"], f["k"], f["v"], f["dO"], case.causal, case.scale, rnd=lambda x: x)
    rr = R.ratios(mod, ref)
    print(case.id, {k: round(v[0], 3) for k, v in rr.items()})
    for name, (v, idx) in rr.items():
        assert v < 1.0, R.where(case, name, idx)
    assert R.ratio(mod["Delta"], ref["Delta"], ref["bDelta"])[0] < 1.0
    assert float((mod["lse"].double() - ref["lse"]).abs().max()) < R.lse_tolerance(case, vis, ref["lse"])


def _padded_reference(q, k, v, dO, lens, causal, scale):
    """Float64 attention over the padded batch (B, L, H, hd): dead keys masked to -inf, dead output rows zero.
    -> O, dQ, dK, dV by autograd."""
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    B, Lq, Lk = q.shape[0], q.shape[1], k.shape[1]
    ql = torch.tensor([a for a, _ in lens])
    kl = torch.tensor([b for _, b in lens])
    S = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    hidden = (torch.arange(Lk)[None, :] >= kl[:, None])[:, None, None, :].expand(B, 1, Lq, Lk).clone()
    if causal:
        hidden = hidden | torch.ones(Lq, Lk, dtype=torch.bool).triu(1)
    P = torch.softmax(S.masked_fill(hidden, float("-inf")), -1)
    O = torch.einsum("bhij,bjhd->bihd", P, v)
    live = (torch.arange(Lq)[None, :] < ql[:, None])[:, :, None, None]
    O = torch.where(live, O, torch.zeros_like(O))
    O.backward(dO)
    return O.detach(), q.grad, k.grad, v.grad


SEMANTICS = [r for r in L.RAGGED if r.mode == "parity" and r.hd == 64]


@pytest.mark.parametrize("rag", SEMANTICS, ids=[r.id for r in SEMANTICS])
def test_masked_padded_reference_is_the_per_sample_reference(rag):
    (Lq, Lk), lens = rag.extents, rag.lens
    g = torch.Generator().manual_seed(5)
    q, k, v, dO = (10.0 * torch.randn(len(lens), n, L.H, rag.hd, generator=g, dtype=torch.float64)
                   for n in (Lq, Lk, Lk, Lq))  # the pad rows hold noise
    refs = []
    for b, (case, (ql, kl)) in enumerate(zip(rag.samples, lens)):
        raw, vis, ref = L.sample(case)
        refs.append(ref)
        for t, name, n in ((q, "q", ql), (k, "k", kl), (v, "v", kl), (dO, "dO", ql)):
            t[b, :n] = vis[name][0]
    O, dQ, dK, dV = _padded_reference(q, k, v, dO, lens, rag.causal, 1.0 / rag.hd ** 0.5)
    for b, (ref, (ql, kl)) in enumerate(zip(refs, lens)):
        for got, name, n in ((O, "O", ql), (dQ, "dQ", ql), (dK, "dK", kl), (dV, "dV", kl)):
            torch.testing.assert_close(got[b, :n], ref[name][0], rtol=1e-9, atol=1e-11, msg=f"{name} of sample {b}")
            assert not got[b, n:].any(), f"{name} of sample {b}: a dead row is not exactly zero"
