"""No GPU: the C-ABI of lane motion (include/sqair_hip.h: sqair_set_motion, sqair_lane_identity_motion_test) -- exported and declared,
the binding mirrors the header's struct, the motion paragraph carries the semantics, every refusal is made before any HIP call (dummy
device pointers are enough) and leaves the handle as it was, the motion goes off with the identity (and so with the estimate and the
state) -- and the argument errors of SqairStream(motion=...)."""
import ctypes as C
import functools
import os

import pytest

from sqair_amd import _capi
from sqair_amd.stream import SqairStream
from tests.abi_host import (DUMMY, LIBS, ROOT, dummy, err as _err, estimate, fields as header_fields, handle, paragraph, phrases,
                            prototype, set_state as _state, stated_once)

INF = float("inf")
N = 3
_est = functools.partial(estimate, fields=("box", "presence", "obj_id", "map_count", "what"))


def _ident(M=6):
    idt = dummy(_capi.SqairLaneIdentity, 0x5000, _capi.IDENT_MEMORY, iou_min=0.3, reid_dist=4.0, reid_what=INF, M=M, max_age=10)
    for i, n in enumerate(_capi.IDENT_FIELDS):
        setattr(idt, n, 0x7000 + 0x100 * i)
    return idt


def _motion(q=0.25, r=1.0, v0_var=16.0, gate=3.0, without=(), nis=True):
    return dummy(_capi.SqairLaneMotion, 0x9000, ("trk_kf", "velocity") + (("nis",) if nis else ()), without, q=q, r=r, v0_var=v0_var,
                 gate=gate)


def test_the_symbols_are_exported_and_declared_and_the_abi_is_unchanged():
    names = ("sqair_set_motion", "sqair_lane_identity_motion_test")
    for path in (None, _capi.WIDE_LIB_PATH, _capi.TIMELINE_LIB_PATH):
        lib = _capi.lib(path)
        assert all(hasattr(lib, n) for n in names) and lib.sqair_abi_version() == 2
    assert all(n in _capi.EXPORTED_SYMBOLS for n in names) and _capi.ABI_VERSION == 2
    assert prototype("sqair_set_motion") == "int sqair_set_motion(SqairHandle* h, const SqairLaneMotion* m, int T, int B)"
    assert prototype("sqair_lane_identity_motion_test") == (
        "int sqair_lane_identity_motion_test(SqairHandle* h, const float* box, const float* presence, const float* obj_id, "
        "const float* what, const int32_t* best_row, int T, int B, const SqairLaneIdentity* id, const SqairLaneMotion* m, void* stream)")
    fields = header_fields("SqairLaneMotion")
    assert fields == [("float", "q"), ("float", "r"), ("float", "v0_var"), ("float", "gate"), ("float*", "trk_kf"), ("float*", "velocity"),
                      ("float*", "nis")]
    assert [n for _, n in fields] == [n for n, _ in _capi.SqairLaneMotion._fields_]
    assert [n for _, n in fields] == list(_capi.MOTION_SCALARS) + list(_capi.MOTION_MEMORY) + list(_capi.MOTION_FIELDS)
    assert C.sizeof(_capi.SqairLaneMotion) == 16 + 8 * 3 and _capi.SqairLaneMotion.trk_kf.offset == 16
    assert _capi.motion_shapes(2, 3, 5) == dict(velocity=(2, 3, 5, 2), nis=(2, 3, 5))
    assert _capi.motion_memory_shapes(3, 6) == dict(trk_kf=(3, 6, 2, 5)) and _capi.MOTION_STATE == ("p", "v", "Ppp", "Ppv", "Pvv")


def test_the_header_states_the_semantics_once():
    doc = paragraph("lane motion: a constant-velocity filter per track", "typedef struct SqairLaneMotion")
    phrases(doc, ("the motion paragraph", "REPLACED by a motion instantiation", "k_lane_identity_motion", "k_lane_identity_motion_opt",
                  "the same node count", "nothing changes and nothing more is launched", "unchanged bit for bit",
                  "Needs an identity (sqair_set_identity)", "box CENTRE", "(p, v, Ppp, Ppv, Pvv)", "written back at the end of the pass",
                  "h, w are not filtered", "never read", "The caller starts with zeros", "white-acceleration variance",
                  "measurement variance in px^2", "velocity variance of a newborn track", "in sigmas",
                  "best_row[t,b] == -1", "no predict step", "P. Predict", "p += v", "Ppp' = Ppp + 2 Ppv + Pvv + q/4",
                  "Ppv' = Ppv + Pvv + q/2", "Pvv' = Pvv + q", "S = Ppp' + r", "(p_y - h/2, p_x - w/2, h, w)",
                  "uses the predicted box where it used trk_box[e]", "fmaf(0.5, h, y)", "d2 = dy dy / S_y + dx dx / S_x",
                  "d2 <= gate * gate", "a NaN never passes", "this replaces dc2 <= r * r", "only the on/off switch of re-identification",
                  "the dw <= reid_what gate and the ranking by dw stay", "the ranking key is d2, ties to the smallest e", "greedy in j",
                  "Points 2, 3, 5, 6, 7 and 8 are untouched", "U. Update", "y = z - p", "k0 = Ppp'/S", "k1 = Ppv'/S", "p += k0 y",
                  "v += k1 y", "Ppp = (1 - k0) Ppp'", "Ppv = (1 - k0) Ppv'", "Pvv = Pvv' - k1 Ppv'", "(z, 0, r, 0, v0_var)",
                  "no predict in its birth frame", "keep the predicted state", "coasts at its velocity", "the gate widens by itself",
                  "velocity[t,b,j,0..2)", "0 for an absent slot, a non-finite lane and a newborn", "nis[t,b,j] (optional)",
                  "All arithmetic is fp32", "every array in LDS", "two passes of six frames leave the bits of one pass of twelve",
                  "NULL m: off", "Refused", "no identity set", "a T other than the estimate's", "a B other than the state's",
                  "not finite and positive", "a NULL trk_kf or velocity", "switches the motion off", "Out of scope", "filtering h, w",
                  "the particles' spread as r", "lane tracks and lane forecasts", "training passes", "identities across lanes"))
    stated_once("lane motion: a constant-velocity filter per track")
    # the identity's own out-of-scope sentence stays and points here; DESIGN and README point to the header
    ident = paragraph("lane identities: stable per-lane track ids", "typedef struct SqairLaneIdentity")
    phrases(ident, ("a motion model for the unseen track", "sqair_set_motion, the motion paragraph below"))
    for name in ("DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "sqair_set_motion" in text and "a motion model for the unseen track" in text, name


@pytest.mark.parametrize("path", LIBS)
def test_set_motion_refusals_before_any_hip_call_leave_the_handle_unchanged(path):
    with handle(path, k_particles=2, n_steps_per_image=N) as (lib, h):
        B, T = 4, 2
        on = lambda m=None, t=T, b=B: lib.sqair_set_motion(h, C.byref(m or _motion()), t, b)
        assert lib.sqair_set_motion(None, C.byref(_motion()), T, B) == -1
        assert on() == -1 and "needs an identity (sqair_set_identity)" in _err(lib, h)          # no state, no estimate, no identity
        _state(lib, h, B)
        assert on() == -1 and "needs an identity" in _err(lib, h)
        assert lib.sqair_set_estimate(h, C.byref(_est()), T, B) == 0
        assert on() == -1 and "needs an identity" in _err(lib, h)                               # an estimate, no identity
        assert lib.sqair_set_identity(h, C.byref(_ident()), T, B) == 0
        assert on() == 0
        # every refusal below leaves the registered motion as it was: the handle still refuses and accepts the same things, and
        # switching off and on again works as before
        for t in (1, 3, 0):
            assert on(t=t) == -1 and "T = {}".format(t) in _err(lib, h) and "T = 2" in _err(lib, h)
        assert on(b=B + 1) == -1 and "B = 5" in _err(lib, h) and "B = 4" in _err(lib, h)
        for name in ("q", "r", "v0_var", "gate"):
            for bad in (0.0, -1.0, INF, -INF, float("nan")):
                assert on(_motion(**{name: bad})) == -1 and name + " must be finite and > 0" in _err(lib, h), (name, bad)
        for missing in ("trk_kf", "velocity"):
            assert on(_motion(without=(missing,))) == -1 and "trk_kf and velocity must not be NULL" in _err(lib, h), missing
        assert on(_motion(nis=False)) == 0                                                      # nis is optional
        for kw in (dict(q=1e-6), dict(r=1e6), dict(v0_var=1e-3), dict(gate=100.0)):
            assert on(_motion(**kw)) == 0, kw
        assert lib.sqair_set_motion(h, None, 0, 0) == 0 and on() == 0                           # NULL: off; and on again
        assert lib.sqair_set_identity(h, C.byref(_ident()), T, B) == 0                          # the identity re-registered: it stays
        assert lib.sqair_set_motion(h, None, 0, 0) == 0


def test_a_refused_registration_leaves_the_pass_as_it_was():
    """What a handle does with a pass is what its registration says: a pass of another T is refused for the estimate's T with or
    without a (refused) motion, and an accepted motion changes nothing about that."""
    from tests.abi_host import fwd_args
    with handle(k_particles=2, n_steps_per_image=N) as (lib, h):
        B = 4
        _state(lib, h, B)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and lib.sqair_set_identity(h, C.byref(_ident()), 2, B) == 0
        assert lib.sqair_set_motion(h, C.byref(_motion(q=-1.0)), 2, B) == -1
        assert lib.sqair_set_motion(h, C.byref(_motion()), 2, B) == 0
        for T in (1, 3):
            assert lib.sqair_forward(*fwd_args(h, B, T=T)) == -1 and "T = 2" in _err(lib, h)
        assert lib.sqair_forward_train(*fwd_args(h, B, T=2)) == -1 and "carried state" in _err(lib, h)   # training never runs it


def test_the_identity_going_off_takes_the_motion_with_it():
    """The motion can only be set while an identity is: after anything that switches the identity off, a NULL-free sqair_set_motion
    is refused until the identity is set again -- and setting the identity again does not bring an old motion back."""
    with handle(k_particles=2, n_steps_per_image=N) as (lib, h):
        B = 4
        ident = lambda T=2, b=B: lib.sqair_set_identity(h, C.byref(_ident()), T, b)
        on = lambda T=2, b=B: lib.sqair_set_motion(h, C.byref(_motion()), T, b)
        refused = lambda T=2, b=B: on(T, b) == -1 and "needs an identity" in _err(lib, h)
        _state(lib, h, B)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and ident() == 0 and on() == 0
        assert lib.sqair_set_identity(h, None, 0, 0) == 0 and refused()                         # the identity off
        assert ident() == 0 and on() == 0
        assert lib.sqair_set_estimate(h, None, 0, 0) == 0 and refused()                         # the estimate off
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and refused() and ident() == 0 and on() == 0
        assert lib.sqair_set_estimate(h, C.byref(_est(without=("box",))), 2, B) == 0            # a field of the identity's goes
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and refused() and ident() == 0 and on() == 0
        assert lib.sqair_set_estimate(h, C.byref(_est()), 3, B) == 0 and refused(3)             # another T
        assert ident(3) == 0 and on(2) == -1 and on(3) == 0
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0 and refused(3)               # the state off
        _state(lib, h, B)
        assert refused(3)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and ident() == 0 and on() == 0
        _state(lib, h, B + 1)                                                                   # another B
        assert refused(2, B + 1)
        # beside the score and score_ids: they go their own way
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B + 1) == 0 and ident(2, B + 1) == 0 and on(2, B + 1) == 0
        assert lib.sqair_set_lane_match(h, 0, 1, 0) == 0 and lib.sqair_set_lane_match(h, 0, 0, 0) == 0
        assert lib.sqair_set_motion(h, None, 0, 0) == 0 and lib.sqair_set_score_ids(h, 1) == -1   # (no score set)


@pytest.mark.parametrize("path", LIBS)
def test_kernel_entry_point_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=N) as (lib, h):
        good = dict(box=DUMMY, presence=DUMMY, obj_id=DUMMY, what=DUMMY, best_row=DUMMY, T=1, B=3)
        order = ("box", "presence", "obj_id", "what", "best_row", "T", "B")
        call = lambda idt, m, **kw: lib.sqair_lane_identity_motion_test(h, *[dict(good, **kw)[k] for k in order],
                                                                        C.byref(idt) if idt is not None else None, C.byref(m), DUMMY)
        assert lib.sqair_lane_identity_motion_test(None, *[good[k] for k in order], C.byref(_ident()), C.byref(_motion()), DUMMY) == -1
        for kw in (dict(box=None), dict(presence=None), dict(obj_id=None), dict(best_row=None), dict(T=0), dict(T=65536), dict(B=0)):
            assert call(_ident(), _motion(), **kw) == -1 and "sqair_lane_identity_motion_test" in _err(lib, h), kw
        assert call(None, _motion()) == -1
        assert call(_ident(), _motion(), what=None) == -1 and "trk_what needs what" in _err(lib, h)
        assert call(_ident(M=17), _motion()) == -1 and "N = 3..16" in _err(lib, h)
        for name in ("q", "r", "v0_var", "gate"):
            for bad in (0.0, -1.0, INF, float("nan")):
                assert call(_ident(), _motion(**{name: bad})) == -1 and name + " must be finite and > 0" in _err(lib, h)
        for missing in ("trk_kf", "velocity"):
            assert call(_ident(), _motion(without=(missing,))) == -1 and "must not be NULL" in _err(lib, h)
        # NULL m is sqair_lane_identity_test: its refusals, under its name
        bad = lib.sqair_lane_identity_motion_test(h, None, DUMMY, DUMMY, DUMMY, DUMMY, 1, 3, C.byref(_ident()), None, DUMMY)
        assert bad == -1 and "sqair_lane_identity_test: " in _err(lib, h)


def test_stream_argument_errors():
    """The motion's arguments are checked before the stream touches its core."""
    class Core(object):
        class cfg(object):
            sample_from_prior = False
    for kw in (dict(), dict(estimate=True)):
        with pytest.raises(ValueError, match=r"^SqairStream: motion is for a stream with identity=True"):
            SqairStream(Core(), 2, motion=True, **kw)
    with pytest.raises(ValueError, match=r"^SqairStream: motion_nis is for a stream with motion=True"):
        SqairStream(Core(), 2, estimate=True, identity=True, motion_nis=True)
    for name in ("motion_q", "motion_r", "motion_v0", "motion_gate"):
        for bad in (0.0, -1.0, INF, float("nan")):
            with pytest.raises(ValueError, match=r"^SqairStream: {} must be finite and > 0".format(name)):
                SqairStream(Core(), 2, estimate=True, identity=True, motion=True, **{name: bad})
