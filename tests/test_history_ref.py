"""No GPU: the NumPy tracer of the track history (tests/history_ref.py, the reference of tests/test_history.py) on genealogies worked
out by hand."""
import numpy as np
import pytest

from tests import history_ref as H


def _tag(s, T, R, N):
    """Outputs of step s in which every value says where it came from: where[t, r, n, c] = 1000 s + 100 t + 10 r + n + c / 8."""
    t, r, n, c = np.meshgrid(np.arange(T), np.arange(R), np.arange(N), np.arange(4), indexing="ij")
    where = (1000 * s + 100 * t + 10 * r + n + c / 8.0).astype(np.float32)
    return dict(where=where, presence=np.ones((T, R, N), np.float32),
                obj_id=np.broadcast_to(np.arange(N, dtype=np.float32), (T, R, N)).copy(),
                log_w=(where[..., 0, 0] + 0.5).astype(np.float32))


def _run(maps, T=1, R=4, N=2, **edit):
    rec = H.Recorder(R)
    for s, m in enumerate(maps):
        o = _tag(s, T, R, N)
        for k, fn in edit.items():
            o[k] = fn(s, o[k])
        rec.push(m, **o)
    return rec


def test_coalescence_to_one_ancestor():
    # one lane of K = 4; step 1 keeps rows (0, 0, 2, 3), step 2 keeps (1, 1, 1, 1) of those, step 3 identity
    rec = _run([[-1] * 4, [0, 0, 2, 3], [1, 1, 1, 1], [0, 1, 2, 3]])
    o = H.trace(rec.steps, L=8, lag=4, K=4)
    assert o["ancestor_row"].tolist() == [[0, 0, 0, 0], [1, 1, 1, 1], [0, 1, 2, 3], [0, 1, 2, 3]]
    assert o["unique_ancestors"][:, 0].tolist() == [1, 1, 4, 4]
    assert o["valid"].all() and o["frame_index"].tolist() == [[0] * 4, [1] * 4, [2] * 4, [3] * 4]
    # the values are those stored at the ancestor's row: frame 0 of every path is step 0's row 0, frame 1 step 1's row 1
    assert (o["where"][0, :, 0, 0] == 0.0).all() and (o["where"][1, :, 0, 0] == 1010.0).all()
    assert o["where"][2, :, 1, 2].tolist() == [2001.25, 2011.25, 2021.25, 2031.25]
    assert o["log_w"][1].tolist() == [1010.5] * 4
    # from the rows the next step would start from: everything one resampling further
    n = H.trace(rec.steps, L=8, lag=4, K=4, start_rows=[3, 3, 0, 0])
    assert n["ancestor_row"].tolist() == [[0, 0, 0, 0], [1, 1, 1, 1], [3, 3, 0, 0], [3, 3, 0, 0]]
    assert n["unique_ancestors"][:, 0].tolist() == [1, 1, 2, 2]


def test_lane_reset_in_the_middle_ends_the_paths_of_that_lane():
    # two lanes of K = 2; lane 1 (rows 2, 3) starts a new clip at step 2
    rec = _run([[-1] * 4, [0, 1, 2, 3], [0, 1, -1, -1], [1, 1, 3, 2]])
    assert rec.steps[3]["t0"].tolist() == [3, 3, 1, 1]
    o = H.trace(rec.steps, L=4, lag=4, K=2)
    assert o["ancestor_row"].tolist() == [[1, 1, -1, -1], [1, 1, -1, -1], [1, 1, 3, 2], [0, 1, 2, 3]]
    assert o["valid"].tolist() == [[1, 1, 0, 0], [1, 1, 0, 0], [1, 1, 1, 1], [1, 1, 1, 1]]
    assert o["frame_index"].tolist() == [[0, 0, -1, -1], [1, 1, -1, -1], [2, 2, 0, 0], [3, 3, 1, 1]]
    assert o["unique_ancestors"].tolist() == [[1, 0], [1, 0], [1, 2], [2, 2]]
    assert (o["where"][:2, 2:] == 0).all() and (o["presence"][:2, 2:] == 0).all() and (o["log_w"][:2, 2:] == 0).all()
    assert o["where"][2, 2, 0, 0] == 2030.0 and o["where"][2, 3, 0, 0] == 2020.0


def test_a_start_row_of_minus_one_gives_an_empty_path():
    rec = _run([[-1] * 4, [0, 1, 2, 3]])
    o = H.trace(rec.steps, L=4, lag=2, K=2, start_rows=[1, -1, 7, 2])   # (7: out of range, as the import reads it)
    assert o["ancestor_row"].tolist() == [[1, -1, -1, 2], [1, -1, -1, 2]]
    assert o["valid"][:, 1].tolist() == [0, 0] and o["valid"][:, 2].tolist() == [0, 0] and o["valid"][:, 0].tolist() == [1, 1]
    assert o["unique_ancestors"].tolist() == [[1, 1], [1, 1]]
    assert (o["obj_id"][:, 1] == 0).all() and (o["frame_index"][:, 1] == -1).all()


def test_the_ring_wraps_and_older_steps_are_absent():
    maps = [[-1] * 4] + [[1, 0, 3, 2]] * 5   # rows swap inside their lane at every step
    rec = _run(maps)
    o = H.trace(rec.steps, L=3, lag=3, K=2)   # six steps pushed, three kept
    assert o["ancestor_row"].tolist() == [[0, 1, 2, 3], [1, 0, 3, 2], [0, 1, 2, 3]]
    assert o["frame_index"].tolist() == [[3] * 4, [4] * 4, [5] * 4]
    assert o["where"][0, 0, 0, 0] == 3000.0 and o["where"][1, 0, 0, 0] == 4010.0
    # fewer steps pushed than the lag asks for: the oldest frames are invalid
    e = H.trace(rec.steps[:2], L=3, lag=3, K=2)
    assert e["valid"].tolist() == [[0] * 4, [1] * 4, [1] * 4] and e["ancestor_row"][0].tolist() == [-1] * 4
    assert e["unique_ancestors"].tolist() == [[0, 0], [2, 2], [2, 2]]
    # lag < L looks at the newest steps only
    s = H.trace(rec.steps, L=3, lag=1, K=2)
    assert s["frame_index"].tolist() == [[5] * 4] and s["where"][0, 1, 0, 0] == 5010.0
    # nothing pushed at all
    z = H.empty_trace(T=1, R=4, N=2, n_what=3, lag=2, K=2, max_tracks=2)
    assert not z["valid"].any() and (z["track_id"] == -1).all() and z["what"].shape == (2, 4, 2, 3)


def test_chunks_of_more_than_one_frame():
    rec = _run([[-1] * 4, [1, 1, 2, 2]], T=3)
    assert rec.steps[1]["t0"].tolist() == [3] * 4
    o = H.trace(rec.steps, L=2, lag=2, K=2)
    assert o["where"].shape == (6, 4, 2, 4)
    assert o["frame_index"][:, 0].tolist() == [0, 1, 2, 3, 4, 5]
    assert o["where"][:, 0, 0, 0].tolist() == [10.0, 110.0, 210.0, 1000.0, 1100.0, 1200.0]   # step 0 at row 1, then step 1 at row 0
    assert o["ancestor_row"].tolist() == [[1, 1, 2, 2], [0, 1, 2, 3]]


def test_an_id_changing_slot_under_compaction_is_one_track():
    # id 5 sits in slot 1 at step 0 and, after the object before it left, in slot 0 from step 1 on; id 9 appears at step 2
    def ids(s, v):
        v[:] = [[7, 5], [5, -1], [5, 9]][s]
        return v

    def pres(s, v):
        v[:] = [[1, 1], [1, 0], [1, 1]][s]
        return v
    rec = _run([[-1] * 2, [0, 1], [0, 1]], R=2, obj_id=ids, presence=pres)
    o = H.trace(rec.steps, L=4, lag=3, K=2, max_tracks=4)
    assert o["track_id"].tolist() == [[5, 7, 9, -1]] * 2 and o["n_tracks"].tolist() == [3, 3]
    assert o["track_present"][:, 0].tolist() == [[1, 1, 0, 0], [1, 0, 0, 0], [1, 0, 1, 0]]
    # the where of id 5 comes from slot 1, then slot 0, slot 0
    assert o["track_where"][:, 0, 0, 0].tolist() == [1.0, 1000.0, 2000.0]
    assert o["track_where"][:, 0, 1, 0].tolist() == [0.0, 0.0, 0.0] and o["track_where"][0, 0, 1, 1] == 0.125
    assert (o["track_where"][1, 0, 1] == 0).all() and (o["track_where"][:, :, 3] == 0).all()


def test_more_ids_than_max_tracks_keeps_the_smallest_and_counts_all():
    def ids(s, v):
        v[:, 0] = [[30, 10], [20, 10], [40, 50]][s]
        v[:, 1] = [[3, 1], [3, 1], [3, 1]][s]
        return v
    rec = _run([[-1] * 2, [0, 1], [0, 1]], R=2, obj_id=ids)
    o = H.trace(rec.steps, L=4, lag=3, K=2, max_tracks=3)
    assert o["n_tracks"].tolist() == [5, 2]
    assert o["track_id"].tolist() == [[10, 20, 30], [1, 3, -1]]
    assert o["track_present"][:, 0].tolist() == [[1, 0, 1], [1, 1, 0], [0, 0, 0]]


def test_same_bits_tells_signed_zeros_and_nans_apart():
    a = np.array([0.0, np.nan], np.float32)
    assert H.same_bits(a, a.copy()) and not H.same_bits(a, np.array([-0.0, np.nan], np.float32))
    with pytest.raises(AssertionError):
        H.trace([], L=2, lag=3, K=1)
