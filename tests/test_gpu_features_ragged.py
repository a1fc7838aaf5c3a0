"""extract_features_batch over clips of different lengths: one load_batch, one ragged log-mel call, per-clip
views equal to per-file extract_features, and collate=True equal to DataCollator of the per-clip dicts."""
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENGTHS = [16000, 4640, 12345, 8001, 2560]  # 160 | n (16000, 2560), the 4640 whose T is 28, two general ones


class Tok:
    def encode(self, s):
        return [len(w) + 3 for w in s.split()]


def _write_wav(path, n, seed):
    rng = np.random.default_rng(seed)
    x = 0.4 * np.sin(2 * np.pi * 0.011 * np.arange(n)) * (0.5 + rng.random()) + 0.05 * rng.standard_normal(n)
    pcm = np.clip(np.round(x * 32767), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.tobytes())


@pytest.fixture(scope="module")
def items(tmp_path_factory):
    d = tmp_path_factory.mktemp("ragged_wavs")
    out = []
    for i, n in enumerate(LENGTHS):
        p = d / f"clip{i}.wav"
        _write_wav(p, n, 40 + i)
        out.append({"audio": str(p), "transcription": " ".join(["word"] * (i + 1)) + f" tail{i}"})
    return out


@pytest.fixture(scope="module")
def per_file(cuda, items):
    from asrx import features

    return [features.extract_features(it, tokenizer=Tok(), spectrogram=True, waveform=True) for it in items]


def test_batch_views_match_per_file(cuda, items, per_file):
    from asrx import data

    batched = data.extract_features_batch(items, tokenizer=Tok(), spectrogram=True, waveform=True)
    assert len(batched) == len(items)
    for n, fb, f1 in zip(LENGTHS, batched, per_file):
        assert fb.keys() == f1.keys()
        assert fb["labels"] == f1["labels"]
        assert fb["spectrogram"].shape == (128, 1 + n // 160) == f1["spectrogram"].shape
        assert torch.equal(fb["spectrogram"], f1["spectrogram"])
        assert fb["waveform"].shape == f1["waveform"].shape and fb["waveform"].shape[0] == 1
        assert torch.equal(fb["waveform"], f1["waveform"])
    assert batched[1]["waveform"].shape == (1, 28)  # 4640 samples: int(0.29 * 100) bins


def test_collate_matches_data_collator(cuda, items, per_file):
    from asrx import data
    from asrx.features import DataCollator

    ref = DataCollator(Tok())(per_file)
    got = data.extract_features_batch(items, tokenizer=Tok(), spectrogram=True, waveform=True, collate=True)
    assert got.keys() == ref.keys() == {"spectrogram", "waveform", "text_ids", "labels"}
    assert got["spectrogram"].shape == (5, 128, 101) and got["waveform"].shape == (5, 1, 100)
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].device == ref[k].device, k
        assert torch.equal(got[k], ref[k]), k


def test_collate_spectrogram_only(cuda, items, per_file):
    from asrx import data
    from asrx.features import DataCollator

    ref = DataCollator(Tok())([dict(f, waveform=None) for f in per_file])
    got = data.extract_features_batch(items, tokenizer=Tok(), spectrogram=True, collate=True)
    assert got.keys() == ref.keys()
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
