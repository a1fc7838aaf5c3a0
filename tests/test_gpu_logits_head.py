"""The logits-free head (ops.logits_head: asrx_gemm_wn_head + asrx_head_merge; essentials.py:893-920 evaluation,
model.py:691-699 the greedy step) against the stored logits of ops.LogitsCE on the same tensors.

The head runs LogitsCE's main loop and reduces the same fp32 values, so its argmax must be exactly
torch.argmax of those logits (random fp32 rows have no ties; the tie rule has its own test with bit-identical
columns), and lse / loss agree with float64 logsumexp / F.cross_entropy of the stored logits within the 1e-5
of test_gpu_ce_fused.py."""
import functools

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
NJS = (1, 2, 3)
SHAPES = [
    (130, 1000, 384),   # two row tiles, the second ragged; a ragged last column tile at every width
    (33, 4096, 768),
    (256, 40000, 384),  # the real vocabulary, once
]


def _inputs(rows, V, D):
    g = torch.Generator().manual_seed(rows + V + D)  # as test_gpu_ce_fused.py
    h = (torch.randn(rows, D, generator=g) * 0.5).to(torch.bfloat16)
    W = torch.randn(V, D, generator=g) * 0.05
    labels = torch.randint(3, V, (rows,), generator=g)
    labels[::7] = 0  # ignore_index rows
    return h, W, labels


@functools.lru_cache(maxsize=None)
def _stored(rows, V, D):
    """LogitsCE's stored fp32 logits for one shape and their float64 statistics (shared by the tile widths)."""
    from asrx import ops, prec

    dev = torch.device("cuda:0")
    h, W, labels = _inputs(rows, V, D)
    hg, Wg, lg = h.to(dev), W.to(dev), labels.to(dev)
    with prec.precision("bf16"), torch.no_grad():
        logits, _ = ops.LogitsCE.apply(hg, Wg, lg, None, False)
    z = logits.double().cpu()
    return {"h": hg, "W": Wg, "labels": lg, "argmax": logits.argmax(-1).cpu(), "lse": torch.logsumexp(z, -1),
            "loss_rows": F.cross_entropy(z, labels, ignore_index=0, reduction="none"),
            "loss": F.cross_entropy(z, labels, ignore_index=0), "cpu_labels": labels}


@gpu
@pytest.mark.parametrize("nj", NJS)
@pytest.mark.parametrize("rows,V,D", SHAPES)
def test_head_matches_stored_logits(cuda, rows, V, D, nj):
    from asrx import ops, prec

    ref = _stored(rows, V, D)
    with prec.precision("bf16"), torch.no_grad():
        assert ops.logits_ce_ok(ref["h"], ref["W"])
        out = ops.logits_head(ref["h"], ref["W"], ref["labels"], nj=nj)
    torch.cuda.synchronize()
    labels = ref["cpu_labels"]
    pred = out["pred"].cpu()
    assert pred.dtype == torch.int64 and pred.shape == (rows,)
    assert torch.equal(pred, ref["argmax"]), int((pred != ref["argmax"]).sum())
    assert int(out["count"]) == int((labels != 0).sum())
    assert int(out["correct"]) == int(((pred == labels) & (labels != 0)).sum())
    lse = out["lse"].double().cpu()
    err = float(((lse - ref["lse"]).abs() / ref["lse"].abs()).max())
    print("lse rel err", err)
    assert err < 1e-5
    lr = out["loss_rows"].double().cpu()
    assert bool((lr[labels == 0] == 0).all())
    live = labels != 0
    err = float(((lr[live] - ref["loss_rows"][live]).abs() / ref["loss_rows"][live].abs()).max())
    print("loss_rows rel err", err)
    assert err < 1e-5
    err = abs(float(out["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    print("loss rel err", err)
    assert err < 1e-5


# ---- ties: one weight row copied to chosen columns gives bit-identical logits there ------------------------
TIE_V, TIE_D, TIE_ROWS = 1000, 384, 130


def _tie_pairs(nj):
    """(lower, higher) columns of the tied pair per placement, in the kernel's geometry at tile width 128 nj:
    a lane's quarter is Q = 8 nj columns, a column wave's slab W = 32 nj, a tile BN = 128 nj."""
    Q, Wv, BN = 8 * nj, 32 * nj, 128 * nj
    last = (TIE_V - 1) // BN * BN  # the ragged last tile's first column
    assert TIE_V - last < BN
    return {"same float4": (4, 5), "lane quarters of one wave": (1, Q + 1), "column waves of one tile": (2, Wv + 2),
            "different tiles": (3, BN + 3), "ragged last tile": (BN + 5, last + 7)}


def _tie_case(nj):
    """h, W and the expected argmax: row r aims at placement r % 5 (its h is a multiple of that weight row)."""
    g = torch.Generator().manual_seed(17 + nj)
    W = torch.randn(TIE_V, TIE_D, generator=g) * 0.05
    pairs = list(_tie_pairs(nj).values())
    assert len({c for p in pairs for c in p}) == 2 * len(pairs)
    for lo, hi in pairs:
        W[hi] = W[lo]
    want = torch.tensor([pairs[r % len(pairs)][0] for r in range(TIE_ROWS)])
    scale = 6.0 + torch.rand(TIE_ROWS, 1, generator=g)
    h = (W[want].to(torch.bfloat16).float() * scale).to(torch.bfloat16)
    return h, W, want


@pytest.mark.parametrize("nj", NJS)
def test_tie_cases_have_exact_ties_in_float64(nj):
    """The construction itself, without a GPU: in float64 on the bf16 operands the tied columns hold the row's
    maximum with exactly equal values, and torch.argmax returns the lower one."""
    h, W, want = _tie_case(nj)
    z = h.double() @ W.to(torch.bfloat16).double().t()
    pairs = list(_tie_pairs(nj).values())
    for r in range(TIE_ROWS):
        lo, hi = pairs[r % len(pairs)]
        assert z[r, lo] == z[r, hi] == z[r].max()
        assert int((z[r] == z[r].max()).sum()) == 2
    assert torch.equal(z.argmax(-1), want)


@gpu
@pytest.mark.parametrize("nj", NJS)
def test_ties_take_the_lowest_column(cuda, nj):
    from asrx import ops, prec

    h, W, want = _tie_case(nj)
    with prec.precision("bf16"), torch.no_grad():
        out = ops.logits_head(h.to(cuda), W.to(cuda), want.to(cuda), nj=nj)
    pred = out["pred"].cpu()
    names = list(_tie_pairs(nj))
    bad = [(r, names[r % len(names)], int(pred[r]), int(want[r])) for r in range(TIE_ROWS) if pred[r] != want[r]]
    assert not bad, bad[:8]
    assert int(out["correct"]) == TIE_ROWS == int(out["count"])  # the labels are the expected columns (all != 0)


@gpu
def test_strided_last_position_rows(cuda):
    """The decode form: the last position of each sample through a strided view (lda = T D), no labels."""
    from asrx import ops, prec

    B, T, D, V = 3, 5, 384, 1000
    g = torch.Generator().manual_seed(9)
    h3 = (torch.randn(B, T, D, generator=g) * 0.5).to(torch.bfloat16).to(cuda)
    W = (torch.randn(V, D, generator=g) * 0.05).to(cuda)
    with prec.precision("bf16"), torch.no_grad():
        last = h3[:, -1]
        assert not last.is_contiguous()
        got = ops.logits_head(last, W)
        full = ops.logits_head(h3.reshape(-1, D), W)["pred"].view(B, T)
        assert set(got) == {"pred"}
        assert got["pred"].shape == (B,)
        assert torch.equal(got["pred"], full[:, -1])
        assert torch.equal(full, ops.linear(h3, W).argmax(-1))


@gpu
def test_bad_and_ignored_labels(cuda):
    from asrx import ops, prec

    rows, V, D = 16, 1000, 384
    g = torch.Generator().manual_seed(2)
    h = torch.randn(rows, D, generator=g).to(torch.bfloat16).to(cuda)
    W = (torch.randn(V, D, generator=g) * 0.05).to(cuda)
    with prec.precision("bf16"), torch.no_grad():
        for bad in (V, -100):
            labels = torch.randint(1, V, (rows,), generator=g)
            labels[3] = bad
            out = ops.logits_head(h, W, labels.to(cuda))
            assert torch.isnan(out["loss"]).item()
            assert bool(((out["pred"] >= 0) & (out["pred"] < V)).all())
            assert int(out["count"]) == rows
        out = ops.logits_head(h, W, torch.zeros(rows, dtype=torch.long, device=cuda))
    assert torch.isnan(out["loss"]).item()
    assert float(out["count"]) == 0 and int(out["correct"]) == 0
    assert bool(((out["pred"] >= 0) & (out["pred"] < V)).all())
    with prec.precision("bf16"), torch.no_grad(), pytest.raises(ValueError, match="one per row"):
        ops.logits_head(h, W, torch.zeros(rows - 1, dtype=torch.long, device=cuda))  # never reaches a kernel


@gpu
def test_fp32_mode_takes_the_fallback(cuda):
    """Parity mode (and fused=False): the same keys and dtypes from ops.linear + the one-pass cross entropy."""
    from asrx import ops, prec

    rows, V, D = 33, 1000, 384
    h, W, labels = _inputs(rows, V, D)
    hb, W, labels = h.to(cuda), W.to(cuda), labels.to(cuda)
    with prec.precision("bf16"), torch.no_grad():
        fused = ops.logits_head(hb, W, labels)
        unfused = ops.logits_head(hb, W, labels, fused=False)
    with prec.precision("fp32"), torch.no_grad():
        hf = hb.float()
        assert not ops.logits_ce_ok(hf, W)
        out = ops.logits_head(hf, W, labels)
        z = ops.linear(hf, W)
    for o in (out, unfused):
        assert set(o) == set(fused)
        for k in fused:
            assert o[k].dtype == fused[k].dtype and o[k].shape == fused[k].shape, k
    assert torch.equal(out["pred"], z.argmax(-1))
    lr = F.cross_entropy(z.double().cpu(), labels.cpu(), ignore_index=0)
    assert abs(float(out["loss"]) - float(lr)) / float(lr) < 1e-5
    assert int(out["count"]) == int((labels != 0).sum())
    assert int(out["correct"]) == int(((out["pred"] == labels) & (labels != 0)).sum())
    assert torch.equal(unfused["pred"], fused["pred"])


@gpu
def test_refuses_grad_mode(cuda):
    from asrx import ops, prec

    h = torch.randn(8, 384).to(torch.bfloat16).to(cuda)
    W = (torch.randn(1000, 384) * 0.05).to(cuda).requires_grad_(True)
    with prec.precision("bf16"):
        with pytest.raises(RuntimeError, match="not differentiable"):
            ops.logits_head(h, W)
        with torch.no_grad():
            assert ops.logits_head(h, W)["pred"].shape == (8,)
