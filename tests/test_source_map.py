"""The host-side source map of a carried state (sqair_amd/carried.py: SourceMap) against a brute-force model: an explicit list
saying, for every particle row of the next step, which row of the last step it continues (-1: it starts fresh).  NumPy only; the
GPU tests (test_stream_state.py, test_forecast.py, test_stream_train.py) cover the same behaviour end to end."""
import numpy as np
import pytest

from sqair_amd.carried import SourceMap


class Rows(object):
    """The model: every operation applied to the explicit list, row by row."""

    def __init__(self, R, K):
        self.R, self.K, self.rows = R, K, [-1] * R   # (at construction every row is fresh)

    def reset(self, lanes):
        for j in lanes:
            for k in range(self.K):
                self.rows[j * self.K + k] = -1

    def resample(self, src):
        old = list(self.rows)
        self.rows = [-1 if s < 0 else old[s] for s in src]

    def take(self):
        rows, self.rows = self.rows, list(range(self.R))
        return rows


def _same(m, ref):
    assert m.pending().tolist() == ref.rows
    assert m.pending().dtype == np.int64


@pytest.mark.parametrize("B,K", [(1, 1), (3, 4), (5, 2)])
def test_random_sequences_match_the_row_list(B, K):
    R = B * K
    rng = np.random.default_rng(100 * B + K)
    m, ref = SourceMap(R, K, "T"), Rows(R, K)
    _same(m, ref)
    for _ in range(300):
        op = rng.integers(3)
        if op == 0:
            lanes = rng.integers(0, B, size=rng.integers(0, B + 1))   # (repeats and the empty list included)
            m.reset(lanes if rng.integers(2) else lanes.tolist())
            ref.reset(lanes.tolist())
        elif op == 1:
            src = rng.integers(-1, R, size=R)
            m.resample(src.astype(rng.choice([np.int32, np.int64])))
            ref.resample(src.tolist())
        else:
            got, want = m.take(), ref.take()
            # identity may come back as None or as the identity map itself
            assert (list(range(R)) if got is None else got.tolist()) == want
            assert m.take() is None   # disarmed
        _same(m, ref)


def test_reset_then_resample_composes_and_fresh_rows_stay_fresh():
    m = SourceMap(6, 2, "T")
    assert m.take().tolist() == [-1] * 6   # the first step: all fresh
    assert m.take() is None and m.pending().tolist() == [0, 1, 2, 3, 4, 5]
    m.reset(1)   # (a scalar lane)
    assert m.pending().tolist() == [0, 1, -1, -1, 4, 5]
    m.resample([1, 1, 3, 0, -1, 2])   # rows that continue a reset row (3, 2) are fresh too; -1 stays -1
    assert m.pending().tolist() == [1, 1, -1, 0, -1, -1]
    m.resample([3, 2, 5, 0, 1, 1])    # a second resample composes with the first
    assert m.pending().tolist() == [0, -1, -1, 1, 1, 1]
    m.reset([0])
    assert m.take().tolist() == [-1, -1, -1, 1, 1, 1]
    assert m.take() is None


def test_validation_errors_name_the_caller():
    m = SourceMap(6, 2, "SqairStream")
    for bad in ([3], [-1], [0.0], 3, np.array([1.5])):
        with pytest.raises(ValueError, match=r"^SqairStream\.reset: lanes must be integers in \[0, 3\)$"):
            m.reset(bad)
    for bad in ([0] * 5, [0] * 7, [0, 1, 2, 3, 4, 6], [-2, 0, 0, 0, 0, 0], [0.0] * 6, np.zeros((6, 1), dtype=np.int64)):
        with pytest.raises(ValueError, match=r"^SqairStream\.resample: src_rows must be 6 integers in \[-1, 6\)$"):
            m.resample(bad)
    assert m.pending().tolist() == [-1] * 6   # a refused call arms nothing
    with pytest.raises(ValueError, match=r"^StreamTrainer\.reset"):
        SourceMap(6, 2, "StreamTrainer").reset([3])
