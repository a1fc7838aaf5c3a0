"""Ragged-batch log-mel and waveform pool (mel.logmel_ragged: asrx_logmel_ragged + asrx_wave_pool_ragged).

The reference in every case is the per-clip call on wav[b, :n_b] (mel.logmel / mel.wave_pool, themselves
gated against the float64 oracle): clip b's part of the ragged result is bit-identical to it
(torch.equal), and everything past it is exactly 0 -- the batch DataCollator pads and stacks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LAYOUTS = ("BFM", "BMF")
EDGE_LENGTHS = [12345, 1, 159, 160, 2559, 2560, 2561, 4640]  # F = 78, 1, 1, 2, 16, 17, 17, 30; 5 tiles per clip
POOL_LENGTHS = [160, 2560, 4640, 9120, 12345, 7680]


def _clip(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    f = rng.uniform(100, 300)
    x = 0.5 * np.sin(2 * np.pi * f * t) * (1 + 0.3 * np.sin(2 * np.pi * 3 * t)) + 0.05 * rng.standard_normal(n)
    return (x / np.abs(x).max()).astype(np.float32)


def _batch(clips, cuda, fill=0.0, row_extra=0):
    """(B, Nmax) device buffer holding the clips, `fill` past each of them; row_extra > 0 makes it a column
    slice of a wider tensor (row stride Nmax + row_extra)."""
    nmax = max(len(c) for c in clips)
    host = np.full((len(clips), nmax + row_extra), fill, dtype=np.float32)
    for b, c in enumerate(clips):
        host[b, :len(c)] = c
    return torch.from_numpy(host).to(cuda)[:, :nmax]


def _per_clip(wav, lengths, layout):
    from asrx.mel import logmel

    return [logmel(wav[b:b + 1, :n].contiguous(), layout=layout)[0] for b, n in enumerate(lengths)]


def _live(out, b, F, layout):
    return out[b, :F] if layout == "BFM" else out[b, :, :F]


def _pad(out, b, F, layout):
    return out[b, F:] if layout == "BFM" else out[b, :, F:]


def _check(res, refs, lengths, layout):
    from asrx.mel import n_frames

    out = res.mel
    assert res.F == [n_frames(n) for n in lengths]
    fmax = max(res.F)
    assert tuple(out.shape) == ((len(lengths), fmax, 128) if layout == "BFM" else (len(lengths), 128, fmax))
    assert not bool(torch.isnan(out).any())
    for b, F in enumerate(res.F):
        assert torch.equal(_live(out, b, F, layout), refs[b]), (b, lengths[b])
        assert bool((_pad(out, b, F, layout) == 0).all()), (b, lengths[b])


@pytest.fixture(scope="module")
def edge(cuda):
    """The tile-edge batch: a clip shorter than half a window, an exactly full tile (2559 -> 16 frames), a
    tile with one live frame (2560, 2561 -> 17), whole dead tiles; the per-clip references, computed once."""
    clips = [_clip(n, 100 + i) for i, n in enumerate(EDGE_LENGTHS)]
    wav = _batch(clips, cuda)
    refs = {lay: _per_clip(wav, EDGE_LENGTHS, lay) for lay in LAYOUTS}
    return clips, wav, refs


@pytest.mark.parametrize("layout", LAYOUTS)
def test_ragged_tile_edges(cuda, edge, layout):
    from asrx.mel import logmel_ragged
    from oracle import mel as omel

    clips, wav, refs = edge
    B, fmax = len(clips), 78
    out = torch.full((B, fmax, 128) if layout == "BFM" else (B, 128, fmax), float("nan"), device=cuda)
    res = logmel_ragged(wav, EDGE_LENGTHS, layout=layout, out=out)
    assert res.mel is out and res.pool is None
    _check(res, refs[layout], EDGE_LENGTHS, layout)
    host = out.cpu().numpy()
    for b, F in enumerate(res.F):
        ref = omel.log_mel(clips[b].astype(np.float64))  # (128, F)
        got = host[b, :F].T if layout == "BFM" else host[b, :, :F]
        assert got.shape == ref.shape
        err = np.abs(got - ref).max()
        assert err < 2e-4, (b, err)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_ragged_lengths_are_honoured(cuda, edge, layout):
    """What the buffer holds past n_b is never used (NaN there changes nothing), and a row stride that is no
    multiple of 4 (the element-wise staging path) gives the same bits."""
    from asrx.mel import logmel_ragged

    clips, _, refs = edge
    nan_tail = _batch(clips, cuda, fill=float("nan"))
    assert bool(torch.isnan(nan_tail[1, 1:]).all())
    _check(logmel_ragged(nan_tail, EDGE_LENGTHS, layout=layout), refs[layout], EDGE_LENGTHS, layout)
    odd = _batch(clips, cuda, fill=float("nan"), row_extra=1)
    assert odd.stride(0) % 4 != 0
    _check(logmel_ragged(odd, torch.tensor(EDGE_LENGTHS), layout=layout), refs[layout], EDGE_LENGTHS, layout)


def test_ragged_per_clip_floor(cuda):
    """The clip-max floor is per clip: a loud clip, a clip 74 dB quieter and a clip whose quiet tail is floored
    share a batch and each equals its per-clip result (no clip sees another's max)."""
    from asrx.mel import logmel_ragged

    n = 48000
    t = np.arange(n) / 16000.0
    rng = np.random.default_rng(3)
    loud_then_quiet = (np.where(t < 1.3, 0.5, 1e-6) * rng.standard_normal(n)).astype(np.float32)
    rng = np.random.default_rng(5)
    clips = [(0.5 * rng.standard_normal(48000)).astype(np.float32),
             (1e-4 * rng.standard_normal(20000)).astype(np.float32), loud_then_quiet[:40000]]
    lengths = [len(c) for c in clips]
    wav = _batch(clips, cuda)
    for layout in LAYOUTS:
        refs = _per_clip(wav, lengths, layout)
        _check(logmel_ragged(wav, lengths, layout=layout), refs, lengths, layout)
    ref2 = refs[2].cpu().numpy()  # (128, 251): the floored entries are the clip's minimum
    floored = np.unique(np.nonzero((ref2 == ref2.min()).any(axis=0))[0] // 16)
    assert 0 < len(floored) < (ref2.shape[1] + 15) // 16, floored


def test_ragged_pool(cuda):
    from asrx.mel import logmel, logmel_ragged, ragged_plan, wave_pool

    clips = [_clip(n, 200 + i) for i, n in enumerate(POOL_LENGTHS)]
    wav = _batch(clips, cuda, fill=float("nan"))
    plan = ragged_plan(POOL_LENGTHS)
    assert plan.T == [1, 16, 28, 56, 77, 48] and plan.fused == [True, True, False, False, False, True]
    pool_out = torch.full((len(clips), plan.Tmax), float("nan"), device=cuda)
    res = logmel_ragged(wav, POOL_LENGTHS, layout="BMF", pool=True, pool_out=pool_out)
    assert res.pool is pool_out and res.T == plan.T
    _check(res, _per_clip(wav, POOL_LENGTHS, "BMF"), POOL_LENGTHS, "BMF")
    for b, (n, T) in enumerate(zip(POOL_LENGTHS, plan.T)):
        x = wav[b:b + 1, :n].contiguous()
        ref = logmel(x, layout="BMF", pool=True)[1] if plan.fused[b] else wave_pool(x, T)
        assert torch.equal(pool_out[b:b + 1, :T], ref), (b, n)
        assert bool((pool_out[b, T:] == 0).all()), (b, n)
    with pytest.raises(ValueError):
        logmel_ragged(wav, POOL_LENGTHS[:-1] + [159], pool=True)


def test_ragged_uniform_odd_batch(cuda):
    """B = 5 equal lengths: the ragged call equals logmel on the same buffer, pool included."""
    from asrx.mel import logmel, logmel_ragged

    wav = _batch([_clip(16000, 300 + i) for i in range(5)], cuda)
    for layout in LAYOUTS:
        ref, ref_pool = logmel(wav, layout=layout, pool=True)
        res = logmel_ragged(wav, [16000] * 5, layout=layout, pool=True)
        assert res.F == [101] * 5 and res.T == [100] * 5
        assert torch.equal(res.mel, ref)
        assert torch.equal(res.pool, ref_pool)


def test_ragged_several_tiles_per_workgroup(cuda):
    """41 clips x 19 tiles = 779 tiles > the 768 resident workgroups: a workgroup walks two tiles, live and dead
    ones of different clips in turn."""
    from asrx.mel import logmel, logmel_ragged, wave_pool

    rng = np.random.default_rng(7)
    lengths = [48000, 160, 47999, 2560] + rng.integers(200, 48001, 37).tolist()
    noise = (0.3 * rng.standard_normal(48000)).astype(np.float32)
    clips = [noise[:n] * np.float32(10.0 ** -(i % 5)) for i, n in enumerate(lengths)]
    wav = _batch(clips, cuda, fill=float("nan"))
    res = logmel_ragged(wav, lengths, layout="BFM", pool=True)
    _check(res, _per_clip(wav, lengths, "BFM"), lengths, "BFM")
    bmf = logmel_ragged(wav, lengths, layout="BMF")
    assert torch.equal(bmf.mel, res.mel.transpose(1, 2))
    for b in (0, 1, 2, 3, 4, 40):
        n, T = lengths[b], res.T[b]
        x = wav[b:b + 1, :n].contiguous()
        ref = logmel(x, pool=True)[1] if n == 160 * T else wave_pool(x, T)
        assert torch.equal(res.pool[b:b + 1, :T], ref) and bool((res.pool[b, T:] == 0).all())


def test_ragged_argument_checks(cuda):
    from asrx.mel import logmel_ragged

    wav = torch.zeros(2, 1000, device=cuda)
    with pytest.raises(ValueError):
        logmel_ragged(wav, torch.tensor([1000, 500], device=cuda))  # device lengths would synchronise
    with pytest.raises(ValueError):
        logmel_ragged(wav, [1000, 1001])  # longer than the buffer
    with pytest.raises(ValueError):
        logmel_ragged(wav, [1000])  # one length per clip
    with pytest.raises(ValueError):
        logmel_ragged(wav, [1000, 500], out=torch.empty(2, 7, 127, device=cuda))
