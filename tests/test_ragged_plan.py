"""mel.ragged_plan: the host side of the ragged log-mel's clip table.  T is the reference's own expression
int((n / sample_rate) * (sample_rate // hop)) in double precision (essentials.py:495), not n // hop."""
import pytest
import torch

LENGTHS = [160, 2560, 4640, 9120, 12345, 7680, 1, 159]


def test_ragged_plan_known_values():
    from asrx.mel import ragged_plan

    p = ragged_plan(LENGTHS)
    assert p.n == LENGTHS
    assert p.F == [2, 17, 30, 58, 78, 49, 1, 1]
    assert p.T == [1, 16, 28, 56, 77, 48, 0, 0]
    # 4640 and 9120 are multiples of 160 whose bin count is one short: not fused
    assert [n for n, f in zip(p.n, p.fused) if f] == [160, 2560, 7680]
    assert p.Fmax == 78 and p.Tmax == 77


def test_ragged_plan_matches_reference_expression():
    from asrx.mel import ragged_plan

    g = torch.Generator().manual_seed(0)
    n = torch.randint(1, 480001, (500,), generator=g).tolist() + [160 * k for k in range(1, 3001, 7)]
    p = ragged_plan(torch.tensor(n))  # a CPU int64 tensor is accepted as well
    for ni, Fi, Ti, fi in zip(n, p.F, p.T, p.fused):
        target = int((ni / 16000) * (16000 // 160))
        assert Fi == 1 + ni // 160 and Ti == target
        assert fi == (ni > target and ni == target * 160)  # extract_features' fused-pool test
    assert p.Fmax == max(p.F) and p.Tmax == max(p.T)


def test_ragged_plan_table_layout():
    from asrx.mel import ragged_plan

    t = ragged_plan(LENGTHS).table()
    assert t.dtype == torch.int32 and t.shape == (8, 4) and t.is_contiguous()
    assert t[:, 0].tolist() == LENGTHS
    assert t[:, 1].tolist() == [2, 17, 30, 58, 78, 49, 1, 1]
    assert t[:, 2].tolist() == [1, 16, 28, 56, 77, 48, 0, 0]
    assert t[:, 3].tolist() == [1, 1, 0, 0, 0, 1, 0, 0]


def test_ragged_plan_rejects_bad_lengths():
    from asrx.mel import ragged_plan

    with pytest.raises(ValueError):
        ragged_plan([])
    with pytest.raises(ValueError):
        ragged_plan([16000, 0])
