"""Model.evaluate and Model.generate(fused_head=True) (the logits-free head, ops.logits_head) against
Model.forward / the default generate: same predictions and loss, no logits tensor, no host synchronisation."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(cuda, tokens, dims=384, head=6, layer=2):
    from asrx.config import Dimensions
    from asrx.model import Model

    torch.manual_seed(0)
    cfg = Dimensions(tokens=tokens, mels=128, dims=dims, head=head, layer=layer, act="gelu", n_type="AbbyNormal")
    return Model(cfg).to(cuda)


def _batch(cuda, tokens, B=2, T=16, S=301):
    """The batch of test_model_fused_ce_matches_unfused: three streams, labels = ids shifted, EOS last."""
    g = torch.Generator().manual_seed(4)
    spec = torch.randn(B, 128, S, generator=g).to(cuda)
    pitch = (torch.rand(B, 1, S, generator=g) * 200).to(cuda)
    wav = (torch.randn(B, 1, S - 1, generator=g) * 0.1).to(cuda)
    ids = torch.randint(3, tokens, (B, T), generator=g)
    ids[:, 0] = 1
    labels = torch.cat([ids[:, 1:], torch.full((B, 1), 2)], 1).to(cuda)
    return {"labels": labels, "text_ids": ids.to(cuda), "spectrogram": spec, "pitch": pitch, "waveform": wav}


@pytest.fixture(scope="module")
def small(cuda):
    return _model(cuda, 1000), _batch(cuda, 1000)


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("training", [False, True])
def test_evaluate_matches_forward(small, training, mode):
    from asrx import prec

    model, batch = small
    model.train(training)
    try:
        with prec.precision(mode):
            model.set_noise(3, 1)
            with torch.no_grad():
                ref = model(**batch)
            model.set_noise(3, 1)
            out = model.evaluate(**batch)
            assert model.noise_step == (2 if training else 1)  # as forward in the same mode
        assert model.training == training
        assert out["logits"] is None
        assert set(out) == {"loss", "predictions", "correct", "count", "logits"}
        want = ref["logits"].argmax(-1)
        assert out["predictions"].dtype == torch.int64 and out["predictions"].shape == want.shape
        assert torch.equal(out["predictions"], want)
        l0, l1 = float(ref["loss"]), float(out["loss"])
        print("loss", l0, l1)
        assert abs(l0 - l1) / abs(l0) < 1e-5
        labels = batch["labels"]
        assert int(out["count"]) == int((labels != 0).sum())
        assert int(out["correct"]) == int(((want == labels) & (labels != 0)).sum())
    finally:
        model.eval()


def test_evaluate_honours_fused_ce_switch(small):
    from asrx import prec

    model, batch = small
    model.eval()
    res = []
    try:
        for fused in (True, False):
            model.fused_ce = fused
            model.set_noise(3, 1)
            with prec.precision("bf16"):
                res.append(model.evaluate(**batch))
    finally:
        model.fused_ce = True
    assert torch.equal(res[0]["predictions"], res[1]["predictions"])
    assert abs(float(res[0]["loss"]) - float(res[1]["loss"])) / abs(float(res[1]["loss"])) < 1e-5


def test_evaluate_peak_memory_is_below_forward_by_the_logits(cuda):
    """tokens = 40000: forward holds the (B, T, V) fp32 logits, evaluate never makes them, so its peak over the
    whole call is lower by at least half the logits' size.

    The text length is 512 here, not the 16 of the other tests: a call's peak is the larger of the processor
    phase's peak (shared line for line by both calls) and what is live when the logits are made plus the
    logits.  At T = 16 the logits are 5.1 MB against a processor-phase peak of 46.0 MB with 21.3 MB live after
    it (measured, B = 2, S = 301), so both calls peak inside the processor at the same 45 981 184 bytes and
    the logits cannot show in a whole-call peak, whatever the head does; only the head phase differs there
    (26.4 MB against 21.4 MB).  The difference shows once half the logits (160 kB per text position) exceed
    that 24.7 MB gap plus the text side's own growth, i.e. from a few hundred positions on."""
    from asrx import prec

    V, B, T = 40000, 2, 512
    model = _model(cuda, V).eval()
    batch = _batch(cuda, V, B, T)
    logits_bytes = B * T * V * 4
    peaks = {}
    with prec.precision("bf16"), torch.no_grad():
        for name in ("forward", "evaluate", "forward", "evaluate"):  # the second round is the warmed one
            model.set_noise(3, 1)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = model(**batch) if name == "forward" else model.evaluate(**batch)
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated() - base
            del out
    print("peak bytes over the call", peaks, "logits", logits_bytes)
    assert peaks["forward"] - peaks["evaluate"] >= logits_bytes // 2


def test_evaluate_does_not_sync_with_the_host(small):
    from asrx import prec

    model, batch = small
    model.eval()
    probe = torch.ones(1, device=batch["labels"].device)
    with prec.precision("bf16"):
        model.evaluate(**batch)  # warm-up: tables, workspaces, side streams
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = model.evaluate(**batch)
            try:
                probe.item()
                honoured = False
            except RuntimeError:
                honoured = True
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(out["loss"]).item()
    if not honoured:
        pytest.skip("this torch build does not raise on .item() under set_sync_debug_mode('error'): "
                    "the sync-free claim is not checked here")


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_generate_fused_head_is_token_identical(cuda, mode):
    from asrx import prec

    model = _model(cuda, 304, dims=128, head=2, layer=2).eval()
    g = torch.Generator().manual_seed(6)
    B, S = 2, 101
    feats = {"spectrogram": torch.randn(B, 128, S, generator=g).to(cuda),
             "pitch": (torch.rand(B, 1, S, generator=g) * 200).to(cuda),
             "waveform": (torch.randn(B, 1, S - 1, generator=g) * 0.1).to(cuda)}
    model.set_noise(5, 0)
    with prec.precision(mode):
        ref = model.generate(max_new_tokens=6, **feats)
        got = model.generate(max_new_tokens=6, fused_head=True, **feats)
    assert got.dtype == ref.dtype == torch.int64
    assert torch.equal(got, ref), (got.tolist(), ref.tolist())
