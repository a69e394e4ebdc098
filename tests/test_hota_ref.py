"""No GPU: the two references of tests/hota_ref.py -- the published algorithm in float64 and the header's integer statement in Python
ints -- held to answers known by hand, and to each other on the kernel tests' own tables (tests/hota_cases.py).

The gap between the two was MEASURED on those tables (profiles/hota_parity.json, section ``statement_vs_float``; with
SQAIR_PARITY_DIR set this test writes that section) and is stated in ``MEASURED`` below: the worst |difference| of a clip's HOTA,
DetA and AssA at any of the nineteen thresholds and the number of clips whose TP differs at any threshold.  The test allows four
times the measured gap, and nothing where the gap is zero."""
import functools

import numpy as np
import pytest

from tests import hota_cases as HC
from tests import hota_ref as R
from tests import score_ref as SR
from tests.kernel_unit import merge_parity

# measured on tests/hota_cases.py's three cases, 24 lanes each, by case (see the module's docstring).  The gap of the wide case, 16 crowded truths, comes from near-ties of the assignment that the
# truncations of the integer statement break the other way in 2 of its 23 clips; at the product sizes only the last bit of a sum moves
MEASURED = {"G4_N4_P32_L64": dict(hota=2.220446049250313e-16, deta=0.0, assa=2.220446049250313e-16, clips_tp_differs=0),
            "G1_N4_P8_L16": dict(hota=0.0, deta=0.0, assa=0.0, clips_tp_differs=0),
            "G16_N14_P64_L32_wide": dict(hota=0.0021999134305397683, deta=0.003318817384399708, assa=0.001154404532568376,
                                         clips_tp_differs=2)}
BOX = (10.0, 10.0, 4.0, 6.0)


def clip(frames, G, N, P=8, L=64):
    """Both references on one clip given by hand: ``frames`` = [(truths, objects)], truths = {g: box}, objects = {j: (box, id)} (a
    frame of None has no truth).  Returns (figures of the integer statement, figures of the float algorithm, ints, match, log)."""
    T = len(frames)
    x = dict(box=np.zeros((T, 1, N, 4), np.float32), presence=np.zeros((T, 1, N), np.float32), ids=np.zeros((T, 1, N), np.int32),
             map_count=np.zeros((T, 1), np.int32), truth_box=np.zeros((T, 1, G, 4), np.float32), truth_present=np.zeros((T, 1, G), np.int32),
             truth_valid=np.zeros((T, 1), np.int32))
    for f, fr in enumerate(frames):
        if fr is None:
            continue
        x["truth_valid"][f, 0] = 1
        for g, bx in fr[0].items():
            x["truth_box"][f, 0, g], x["truth_present"][f, 0, g] = bx, 1
        for j, (bx, i) in fr[1].items():
            x["box"][f, 0, j], x["presence"][f, 0, j], x["ids"][f, 0, j] = bx, 1.0, i
    return both(x, G, N, P, L)


def both(x, G, N, P, L, b=0):
    sims = [[] for _ in range(np.asarray(x["map_count"]).shape[1])]
    log = R.append(R.new_log(len(sims), G, N, P, L), *[x[k] for k in HC.INPUTS], sims=sims)
    recs = R.records(log, b)
    ints, floats, match, _ = R.solve_lane(recs, G, P)
    fi, ff, _ = R.hota_float(sims[b], [r[1] for r in recs], [r[2] for r in recs], G, P)
    return R.figures(ints, floats), R.figures(fi, ff), ints, match, log


def shifted(dy=0.0, dx=0.0, box=BOX):
    return (box[0] + dy, box[1] + dx, box[2], box[3])


def test_perfect_tracking_gives_one_everywhere():
    frames = [({0: BOX, 1: shifted(20)}, {0: (BOX, 5), 1: (shifted(20), 6)}) for _ in range(6)]
    for fig in clip(frames, 2, 3)[:2]:
        for n in ("hota", "deta", "assa", "detre", "detpr", "assre", "asspr", "loca", "hota0", "loca0"):
            assert fig[n] == 1.0, n
        assert (fig["hota_alpha"] == 1.0).all()


@pytest.mark.parametrize("n", [1, 3, 8])
def test_an_id_switch_half_way_halves_the_association(n):
    frames = [({0: BOX}, {0: (BOX, 5 if f < n else 9)}) for f in range(2 * n)]
    for fig in clip(frames, 1, 2)[:2]:
        assert (fig["deta_alpha"] == 1.0).all() and np.allclose(fig["assa_alpha"], 0.5, rtol=0, atol=1e-15)
        assert np.allclose(fig["hota_alpha"], np.sqrt(0.5), rtol=0, atol=1e-15)


def test_an_all_miss_clip():
    frames = [({0: BOX}, {0: (shifted(30), 5)}) for _ in range(4)]
    a, b, ints, match, _ = clip(frames, 1, 2)
    assert (ints[:, 0] == 0).all() and (ints[:, 1] == 4).all() and (ints[:, 2] == 4).all()
    for fig in (a, b):
        assert (fig["deta_alpha"] == 0.0).all() and fig["hota"] != fig["hota"]      # AssA has no denominator: NaN


def test_an_iou_of_exactly_one_half_is_a_tp_at_thresholds_1_to_10():
    assert SR.iou64(np.float32(BOX), np.float32(shifted(dx=2.0))) == 0.5      # 16 / (24 + 24 - 16)
    a, b, ints, _, log = clip([({0: BOX}, {0: (shifted(dx=2.0), 5)})], 1, 1)
    assert log["log_q"][0, 0, 0, 0] == 1 << 19 == R.A[9]
    assert ints[:, 0].tolist() == [1] * 10 + [0] * 9
    assert a["deta_alpha"].tolist() == b["deta_alpha"].tolist() == [1.0] * 10 + [0.0] * 9


def test_the_alignment_score_overrules_the_larger_iou():
    """Nine frames tie truth 0 to id 5 and truth 1 to id 6; in the tenth only truth 0 is there, id 5 overlaps it by 1/2 and id 6 by
    more: IoU alone would take id 6, the alignment score takes id 5."""
    far = shifted(25)
    frames = [({0: BOX, 1: far}, {0: (BOX, 5), 1: (far, 6)}) for _ in range(9)]
    frames.append(({0: BOX}, {0: (shifted(dx=2.0), 5), 1: (shifted(dx=1.0), 6)}))
    iou = SR.iou_table(np.float32([[[BOX]]]), np.float32([[[shifted(dx=2.0), shifted(dx=1.0)]]]))[0, 0, 0]
    assert iou[1] > iou[0] == 0.5
    a, b, ints, match, _ = clip(frames, 2, 2)
    assert match[9].tolist() == [0, -1]
    assert ints[:, 0].tolist() == [19] * 10 + [18] * 9


def test_an_unkeyed_object_is_a_false_positive_at_every_threshold():
    keyed = [({0: BOX}, {0: (BOX, 5)}) for _ in range(3)]
    a, _, ints, _, log = clip(keyed + [({0: BOX}, {0: (BOX, 5), 1: (BOX, -4)})], 1, 2)      # a negative id word on the truth's box
    assert (ints[:, 2] == 1).all() and (ints[:, 0] == 4).all() and log["log_col"][0, 3].tolist() == [0, -2] and log["totals_c"][0, 3] == 1
    _, _, ints, _, log = clip(keyed + [({0: BOX}, {0: (BOX, 5), 1: (BOX, 6)})], 1, 2, P=1)   # no column left
    assert (ints[:, 2] == 1).all() and log["log_col"][0, 3].tolist() == [0, -2]
    _, _, ints, _, log = clip(keyed + [({0: BOX}, {0: (BOX, 5), 1: (BOX, 5)})], 1, 2)        # the word held twice
    assert (ints[:, 2] == 1).all() and log["log_col"][0, 3].tolist() == [0, -2]


def test_a_dropped_frame_counts_nothing_and_an_untruthed_one_touches_nothing():
    frames = [({0: BOX}, {0: (BOX, 5)}) for _ in range(3)] + [None] + [({0: BOX}, {0: (shifted(30), 7)}) for _ in range(2)]
    _, _, ints, _, log = clip(frames, 1, 1, L=3)
    assert log["frames"][0] == 3 and log["dropped_frames"][0] == 2 and (log["col_id"][0] == [5] + [-1] * 7).all()
    assert (ints == [3, 0, 0, 3 << 20]).all()
    _, _, ints, _, log = clip(frames, 1, 1, L=64)
    assert log["frames"][0] == 5 and log["dropped_frames"][0] == 0 and (ints[:, :3] == [3, 2, 2]).all()


def test_two_clips_double_the_totals():
    c = HC.CASES[0]
    x = HC.make(c)
    log = R.append(R.new_log(HC.B, c.G, c.N, c.P, c.L), *[x[k] for k in HC.INPUTS])
    once, oi, of, oc, _, _ = R.solve(log, close=np.ones(HC.B, np.int32))
    assert (once["col_id"] == -1).all() and not once["frames"].any() and np.array_equal(once["totals_i"], oi)
    again = R.append(once, *[x[k] for k in HC.INPUTS])
    assert np.array_equal(again["log_q"], log["log_q"]) and np.array_equal(again["col_id"], log["col_id"])
    twice = R.solve(again, close=np.ones(HC.B, np.int32))[0]
    assert np.array_equal(twice["totals_i"], 2 * oi) and np.array_equal(twice["totals_f"], 2 * of)
    assert np.array_equal(twice["totals_c"][:, :3], 2 * oc[:, :3]) and np.array_equal(twice["totals_c"][:, 3], 2 * log["totals_c"][:, 3])
    one, two = R.figures(oi.sum(0), of.sum(0)), R.figures(twice["totals_i"].sum(0), twice["totals_f"].sum(0))
    assert one["hota"] == two["hota"] and one["assa"] == two["assa"]


@functools.lru_cache(maxsize=None)
def gap(i):
    """The measured figures of case i: the worst |integer statement - float algorithm| of a clip's HOTA, DetA, AssA at a threshold and the clips
    whose TP differs at a threshold."""
    c = HC.CASES[i]
    x = HC.make(c)
    worst, differs, clips = dict(hota=0.0, deta=0.0, assa=0.0), 0, 0
    sims = [[] for _ in range(HC.B)]
    log = R.append(R.new_log(HC.B, c.G, c.N, c.P, c.L), *[x[k] for k in HC.INPUTS], sims=sims)
    for b in range(HC.B):
        recs = R.records(log, b)
        if not recs:
            continue
        clips += 1
        ints, floats, _, _ = R.solve_lane(recs, c.G, c.P)
        fi, ff, _ = R.hota_float(sims[b], [r[1] for r in recs], [r[2] for r in recs], c.G, c.P)
        differs += bool((ints[:, 0] != fi[:, 0]).any())
        a, f = R.figures(ints, floats), R.figures(fi, ff)
        for n in worst:      # (per threshold; a threshold without a denominator in either is NaN in that one and not compared)
            d = np.abs(a[n + "_alpha"] - f[n + "_alpha"])
            worst[n] = max(worst[n], float(np.nanmax(d)) if np.isfinite(d).any() else 0.0)
    return worst, differs, clips


@pytest.mark.parametrize("i", range(len(HC.CASES)), ids=[HC.case_id(c) for c in HC.CASES])
def test_the_integer_statement_against_the_float_algorithm(i):
    worst, differs, clips = gap(i)
    print(HC.case_id(HC.CASES[i]), "clips", clips, "worst gap", worst, "clips whose TP differs", differs)

    def update(data):
        data["statement_vs_float"][HC.case_id(HC.CASES[i])] = dict(clips=clips, clips_tp_differs=differs, **worst)
    merge_parity("hota_parity.json", R.fresh_parity, update)
    assert clips >= HC.B - 1
    measured = MEASURED[HC.case_id(HC.CASES[i])]
    for n, v in worst.items():
        assert v <= 4.0 * measured[n], (n, v)
    assert differs <= 4 * measured["clips_tp_differs"]
