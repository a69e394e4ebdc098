"""The inputs of tests/test_idf_kernel.py (GPU) and of the checks tests/test_idf_ref.py makes on the very same arrays (CPU): 200 lanes
of T = 8 frames per case, (G, N, P) = (4, 4, 8) -- overflowing --, (4, 4, 32), (1, 4, 1), (3, 4, 5) and, on the wide library,
(16, 14, 64), iou_min 0.5 and 0.3.

Boxes, presences, ids, map_count and the truth come from the generator of tests/score_cases.py, run for this module's B and T.  On top
of its ids (a hypothesis redrawn with probability 0.1 per frame) the id words CHURN: in every third lane the hypothesis of every
object is redrawn in every frame, so that a clip sees more ids than P columns where P is small; in every 13th lane the first present
object of a frame carries a negative id; in every 17th lane the second present object repeats the word of the first.  ``ids`` are the
int32 words of the float ids.  ``truth_match`` is the score's own output for these inputs (tests/score_ref.py), which the kernel under
test only reads."""
import collections
import ctypes as C
import functools

import numpy as np
import torch

from sqair_amd import _capi
from tests import idf_ref as R
from tests import score_cases as SC
from tests import score_ref as SR
from tests.abi_host import LANE_LIBS, kept_handle

Case = collections.namedtuple("Case", "G N P iou_min wide seed")
CASES = [Case(G, N, P, iou, wide, 1000 * G + 10 * P + int(10 * iou))
         for G, N, P, wide in ((4, 4, 8, False), (4, 4, 32, False), (1, 4, 1, False), (3, 4, 5, False), (16, 14, 64, True)) for iou in (0.5, 0.3)]
B, T = 200, 8
FRAGILE_CAP = SC.FRAGILE_CAP      # of the lanes: the score's


def case_id(c):
    return "G{}_N{}_P{}_iou{:g}{}".format(c.G, c.N, c.P, c.iou_min, "_wide" if c.wide else "")


def _generate(c):
    """tests/score_cases.py's generator for B lanes of T frames (its module constants say 210 and 6: set for the call, put back)."""
    saved = SC.B, SC.T
    SC.B, SC.T = B, T
    try:
        return SC.make.__wrapped__(SC.Case(c.G, c.N, c.iou_min, c.wide, c.seed))
    finally:
        SC.B, SC.T = saved


@functools.lru_cache(maxsize=None)
def make(c):
    """{name: array} for the case; made once, never written to."""
    x = {k: np.array(v) for k, v in _generate(c).items()}
    rng = np.random.default_rng(c.seed + 1)
    obj_id, presence = x["obj_id"], x["presence"]
    for b in range(B):
        for f in range(T):
            here = np.flatnonzero(presence[f, b] != 0)
            if b % 3 == 0:
                for j in here:
                    obj_id[f, b, j] = np.float32(1 + j + 100 * int(rng.integers(0, 400)))
            if b % 13 == 5 and here.size:
                obj_id[f, b, here[0]] = np.float32(-3.0)
            if b % 17 == 4 and here.size >= 2:
                obj_id[f, b, here[1]] = obj_id[f, b, here[0]]
    x["ids"] = SR.words(obj_id).copy()
    ref = SR.score(box=x["box"], presence=presence, obj_id=obj_id, map_count=x["map_count"], truth_box=x["truth_box"],
                   truth_present=x["truth_present"], truth_valid=x["truth_valid"], iou_min=c.iou_min)
    x["truth_match"] = ref.truth_match.astype(np.int32)
    for a in x.values():
        a.setflags(write=False)
    return x


# ------------------------------------------------------------------------------------------------ the solve on caller tables (GPU)
NOTE = ("per case of tests/test_idf_solve_kernel.py (solve) and tests/test_idf_kernel.py (accumulate): the lanes compared, the "
        "lanes left out as fragile and the events counted; every compared word is an integer and is compared exactly")


def record(section, case, **figures):
    """One case's figures into idf_parity.json under SQAIR_PARITY_DIR (tests/test_idf_solve_kernel.py and tests/test_idf_kernel.py
    write the same file)."""
    from tests.kernel_unit import merge_parity

    def update(data):
        data["build_id"] = _capi.build_id()
        data["device"] = torch.cuda.get_device_name(0)
        data[section][case] = figures
    merge_parity("idf_parity.json", lambda: {"note": NOTE, "solve": {}, "accumulate": {}}, update)


def handle(lib_name):
    return kept_handle(("idf", lib_name), LANE_LIBS[lib_name], k_particles=2, n_steps_per_image=4, n_what=6)


def to_device(t):
    return {n: torch.from_numpy(np.array(v)).cuda() for n, v in t.items()}


def struct(d, P):
    return _capi.SqairLaneIdf(P=P, **{n: d[n].data_ptr() for n in _capi.IDF_TABLE + ("totals",)})


def run_solve(lib_name, d, G, P, close=None, want_open=True, want_assign=True):
    """One launch on the device table ``d`` (updated in place); returns (open, assign) as arrays or None."""
    lib, h = handle(lib_name)
    n = d["col_id"].shape[0]
    open_ = torch.full((n, len(R.TOTALS)), -7, dtype=torch.int64, device="cuda") if want_open else None
    assign = torch.full((n, G), -7, dtype=torch.int32, device="cuda") if want_assign else None
    mask = None if close is None else torch.from_numpy(np.asarray(close, np.int32)).cuda()
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = lib.sqair_lane_idf_solve(h, C.byref(struct(d, P)), G, n, ptr(mask), ptr(open_), ptr(assign),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    return (None if open_ is None else open_.cpu().numpy()), (None if assign is None else assign.cpu().numpy())
