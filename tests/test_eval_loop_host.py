"""asrx.metrics.evaluate_loader (the reference's evaluation block, essentials.py:875-935) on a stub model whose
evaluate / generate return prepared tensors: the loss average, sample count, token accuracy and WER are what
compute_metrics / wer_batch give on the same ids.  No GPU."""
import numpy as np
import pytest
import torch

from asrx import metrics


class _Tok:
    """ids -> words "w<id>" (pad / bos / eos / -100 dropped, as the reference's batch_decode)."""

    def batch_decode(self, ids_list):
        return [" ".join(f"w{i}" for i in metrics.clean_ids(ids)) for ids in ids_list]


class _Stub:
    """Model.evaluate / Model.generate with prepared answers, one per batch in loader order."""

    def __init__(self, preds, losses, gen=None):
        self.preds, self.losses, self.gen = preds, losses, gen
        self.i = -1
        self.calls = []
        self.mode = None

    def eval(self):
        self.mode = "eval"
        return self

    def evaluate(self, labels, text_ids, spectrogram=None, pitch=None, waveform=None):
        self.i += 1
        self.calls.append(("evaluate", spectrogram is not None, pitch is not None, waveform is not None))
        pred = self.preds[self.i]
        live = labels != 0
        return {"loss": torch.tensor(self.losses[self.i]), "predictions": pred, "logits": None,
                "correct": ((pred == labels) & live).sum(), "count": live.sum().float()}

    def generate(self, spectrogram=None, pitch=None, waveform=None, max_new_tokens=150, fused_head=False):
        self.calls.append(("generate", max_new_tokens, fused_head))
        return self.gen[self.i]


def _loader():
    g = torch.Generator().manual_seed(0)
    out = []
    for B, T in ((3, 7), (2, 5), (4, 7)):
        labels = torch.randint(3, 50, (B, T), generator=g)
        labels[:, -1] = 2
        labels[0, -3:] = 0  # padding
        ids = torch.cat([torch.ones(B, 1, dtype=torch.long), labels[:, :-1]], 1)
        out.append({"text_ids": ids, "labels": labels.int(), "spectrogram": torch.zeros(B, 4, 9), "pitch": None})
    return out


def _noisy(labels, g):
    pred = labels.long().clone()
    flip = torch.rand(pred.shape, generator=g) < 0.3
    pred[flip] = torch.randint(3, 50, (int(flip.sum()),), generator=g)
    return pred


def test_evaluate_loader_teacher_forced():
    loader = _loader()
    g = torch.Generator().manual_seed(1)
    preds = [_noisy(b["labels"], g) for b in loader]
    losses = [2.5, 1.25, 4.0]
    model = _Stub(preds, losses)
    res = metrics.evaluate_loader(model, loader, _Tok())
    assert set(res) == {"loss", "wer", "samples", "token_accuracy"}
    assert model.mode == "eval"
    assert model.calls == [("evaluate", True, False, False)] * 3
    assert res["samples"] == 9
    assert res["loss"] == pytest.approx(sum(losses) / 3, rel=1e-12)
    all_p = [row for p in preds for row in p.tolist()]
    all_l = [row for b in loader for row in b["labels"].tolist()]
    want = metrics.compute_metrics({"predictions": np.array(all_p, dtype=object),
                                    "label_ids": np.array(all_l, dtype=object)}, tokenizer=_Tok())["wer"]
    assert 0 < want < 100
    assert res["wer"] == pytest.approx(want, rel=1e-12)
    tok = _Tok()
    assert res["wer"] == pytest.approx(metrics.wer_batch(tok.batch_decode(all_l), tok.batch_decode(all_p)), rel=1e-12)
    correct = sum(int(((p == b["labels"]) & (b["labels"] != 0)).sum()) for p, b in zip(preds, loader))
    count = sum(int((b["labels"] != 0).sum()) for b in loader)
    assert 0 < correct < count
    assert res["token_accuracy"] == pytest.approx(correct / count, rel=1e-12)


def test_evaluate_loader_generate_uses_the_fused_head():
    loader = _loader()
    g = torch.Generator().manual_seed(2)
    preds = [_noisy(b["labels"], g) for b in loader]
    # decoded sequences of their own lengths (BOS first), different per batch
    gen = [torch.cat([torch.ones(b["labels"].shape[0], 1, dtype=torch.long), _noisy(b["labels"], g)[:, :n]], 1)
           for b, n in zip(loader, (4, 5, 2))]
    model = _Stub(preds, [1.0, 2.0, 3.0], gen)
    res = metrics.evaluate_loader(model, loader, _Tok(), generate=True)
    assert [c for c in model.calls if c[0] == "generate"] == [("generate", 7, True), ("generate", 5, True),
                                                              ("generate", 7, True)]
    assert res["loss"] == pytest.approx(2.0, rel=1e-12)
    tok = _Tok()
    all_p = [row for p in gen for row in p.tolist()]
    all_l = [row for b in loader for row in b["labels"].tolist()]
    assert res["wer"] == pytest.approx(metrics.wer_batch(tok.batch_decode(all_l), tok.batch_decode(all_p)), rel=1e-12)
    # token accuracy stays the teacher-forced one
    correct = sum(int(((p == b["labels"]) & (b["labels"] != 0)).sum()) for p, b in zip(preds, loader))
    count = sum(int((b["labels"] != 0).sum()) for b in loader)
    assert res["token_accuracy"] == pytest.approx(correct / count, rel=1e-12)


def test_evaluate_loader_without_batches():
    assert metrics.evaluate_loader(_Stub([], []), [], _Tok()) == {"loss": 0.0, "wer": 0.0, "samples": 0,
                                                                  "token_accuracy": 0.0}


def test_logits_head_refuses_cpu_tensors():
    from asrx import ops

    h = torch.randn(4, 384).to(torch.bfloat16)
    W = torch.randn(1000, 384)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="CPU tensor"):
            ops.logits_head(h, W)
        with pytest.raises(RuntimeError, match="CPU tensor"):
            ops.logits_head(h, W, torch.ones(4, dtype=torch.long))
