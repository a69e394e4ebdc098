"""Host-side checks that need no GPU: the C-ABI library loads, exports every symbol include/sqair_hip.h
declares, its parameter table agrees with the Python inventory, and the binding made from the header (sqair_amd/_abi.py) is what a C
compiler reads in it."""
import ctypes as C
import re

import numpy as np
import pytest

from sqair_amd import _abi, _capi
from sqair_amd.flags import make_flags
from sqair_amd.model import make_config
from sqair_amd.params import param_offsets, param_spec
from tests.abi_host import code, constant, fields as header_fields, functions, gcc as _gcc, handle, prototype


def test_library_loads_and_exports_header_symbols():
    lib = _capi.lib()
    names = functions()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), "missing export " + n
    assert set(names) == set(_capi.EXPORTED_SYMBOLS), "ctypes prototypes and header disagree"
    # a host-only read-out of the plan: a measurement helper, bound and exported but not in the header
    assert "sqair_debug_plan_t" in _capi._PROTOS and hasattr(lib, "sqair_debug_plan_t") and "sqair_debug_plan_t" not in names
    assert lib.sqair_abi_version() == _capi.ABI_VERSION == 2
    assert lib.sqair_build_flags() == b"product"


def test_build_id_is_compiled_in_and_a_stale_binary_is_refused(tmp_path):
    """The id a library reports is the hash of the sources IT was compiled from (csrc/build.py passes it to hipcc), not a hash
    taken from disk at run time: a binary that does not belong to the sources beside it is refused by the binding, and the
    measurement tools (bench.py, tools/timeline.py) get their `build_id` from the loaded library."""
    from sqair_amd.csrc import build as B
    assert _capi.build_id() == _capi.source_id() == B.binary_id(_capi.LIB_PATH)
    assert re.fullmatch(r"[0-9a-f]{16}", _capi.build_id())
    # a deliberately stale copy: same code, another id compiled in (both occurrences: the marker and the exported string)
    blob = open(_capi.LIB_PATH, "rb").read()
    good = _capi.build_id().encode()
    assert blob.count(good) >= 2
    stale = tmp_path / "libsqair_hip.so"
    stale.write_bytes(blob.replace(good, b"0123456789abcdef"))
    assert B.binary_id(str(stale)) == "0123456789abcdef"
    with pytest.raises(_capi.StaleLibraryError, match="compiled from sources 0123456789abcdef but the sources on disk are " + good.decode()):
        _capi.lib(str(stale))
    assert _capi.lib(str(stale), allow_stale=True).sqair_build_id() == b"0123456789abcdef"
    assert _capi.build_id(str(stale)) == "0123456789abcdef"   # the LIBRARY's value, whatever the disk says
    # csrc/build.py rebuilds on an id mismatch, not on modification times
    assert B.binary_id(str(tmp_path / "absent.so")) is None


@pytest.mark.parametrize("N,hw,cell", [(3, (50, 50), "GRU"), (4, (50, 50), "GRU"), (6, (50, 50), "GRU"), (4, (128, 128), "GRU"),
                                       (3, (50, 50), "LSTM"), (3, (50, 50), "GRU/LSTM"), (4, (50, 50), "LSTM/LSTM"),
                                       (3, (50, 50), "GRU/GRU/LSTM"), (4, (50, 50), "LSTM/LSTM/LSTM"),
                                       (3, (50, 50), "GRU/GRU/GRU"), (3, (50, 50), "VanillaRNN/VanillaRNN/LSTM"),
                                       (4, (50, 50), "VanillaRNN/LSTM/VanillaRNN")])
def test_param_table_matches_python_spec(N, hw, cell):
    cs = cell.split("/") + ["GRU", "VanillaRNN"][len(cell.split("/")) - 1:]
    flags = dict(n_steps_per_image=N, time_transition=cs[0], prior_transition=cs[1], transition=cs[2])
    with handle(hw=hw, **flags) as (lib, h):
        spec = param_spec(make_flags(**flags), hw)
        off, total = param_offsets(spec)
        assert lib.sqair_param_count(h) == total
        assert lib.sqair_param_entries(h) == len(spec)
        for i, (name, shape, _, _) in enumerate(spec):
            cname, coff, cnum = C.c_char_p(), C.c_int64(), C.c_int64()
            assert lib.sqair_param_entry(h, i, C.byref(cname), C.byref(coff), C.byref(cnum)) == 0
            assert cname.value.decode() == name
            assert coff.value == off[name][0]
            assert cnum.value == (int(np.prod(shape)) if len(shape) else 1)
        if N == 3 and hw == (50, 50) and cell == "GRU":
            assert total == 2951522  # reference notebooks/play.ipynb:362
        assert lib.sqair_packed_bytes(h) > total * 4
        assert lib.sqair_workspace_bytes(h, 10, 32) > 0
        assert lib.sqair_noise_width(h) == 55


def test_create_rejects_bad_config():
    lib = _capi.lib()
    F = make_flags()
    cfg = make_config(F, (50, 50))
    cfg.n_steps_per_image = 0
    h = C.c_void_p()
    assert lib.sqair_create(C.byref(cfg), C.byref(h)) != 0
    cfg = make_config(F, (50, 50))
    cfg.n_hidden = 72          # not 32 * n_units: n_hidden // 2 must be a whole number of 16-column tiles' worth of units
    assert lib.sqair_create(C.byref(cfg), C.byref(h)) != 0
    with pytest.raises(ValueError):
        make_config(make_flags(n_units=0), (50, 50))
    cfg = make_config(F, (37, 41))   # any frame size (H * W not a multiple of 4 goes through a padded copy)
    assert lib.sqair_create(C.byref(cfg), C.byref(h)) == 0
    lib.sqair_destroy(h)


def test_flag_errors_mirror_reference():
    with pytest.raises(ValueError):
        make_config(make_flags(prop_prior_type="bogus"), (50, 50))   # propagate.py:42-43
    with pytest.raises(ValueError):
        make_config(make_flags(disc_prior_type="bogus"), (50, 50))   # sqair_modules.py:224
    with pytest.raises(ValueError):
        make_flags(not_a_flag=1)


@pytest.mark.parametrize("flags", [dict(n_what=100), dict(n_what=128, n_units=16), dict(n_steps_per_image=12), dict(n_units=10),
                                   dict(n_units=13, time_transition="LSTM", prior_transition="LSTM", transition="LSTM"),
                                   dict(n_steps_per_image=14, n_what=128)])
def test_wide_library_accepts_the_rest_of_the_flag_range(flags):
    """Beyond what the product library is laid out for (n_what <= 50, 8 slots, n_units <= 8) the SAME sources compiled with
    -DSQAIR_WIDE serve the configuration through the same C-ABI (reference flags take any value:
    sqair/common_model_flags.py:32-56, configs/mlp_mnist_model.py:42-52); the product library says no instead of misbehaving."""
    F = make_flags(**flags)
    cfg = make_config(F, (50, 50))
    path = _capi.lib_path_for(cfg.n_what, cfg.n_steps_per_image, cfg.n_hidden)
    assert path == _capi.WIDE_LIB_PATH
    h = C.c_void_p()
    assert _capi.lib().sqair_create(C.byref(cfg), C.byref(h)) != 0
    with handle(path, **flags) as (lib, h):
        assert lib.sqair_build_flags() == b"wide" and lib.sqair_abi_version() == _capi.ABI_VERSION
        spec = param_spec(F, (50, 50))
        off, total = param_offsets(spec)
        assert lib.sqair_param_count(h) == total and lib.sqair_param_entries(h) == len(spec)
        for i, (name, shape, _, _) in enumerate(spec):
            cname, coff, cnum = C.c_char_p(), C.c_int64(), C.c_int64()
            assert lib.sqair_param_entry(h, i, C.byref(cname), C.byref(coff), C.byref(cnum)) == 0
            assert (cname.value.decode(), coff.value, cnum.value) == (name, off[name][0], int(np.prod(shape)) if len(shape) else 1)
        assert lib.sqair_noise_width(h) == 4 + int(F.n_what) + 1
        assert lib.sqair_workspace_bytes(h, 3, 2) > 0 and lib.sqair_backward_bytes(h, 3, 2) > 0


def test_limits_of_both_builds():
    lib, wide = _capi.lib(), _capi.lib(_capi.WIDE_LIB_PATH)
    h = C.c_void_p()
    for flags, ok_product, ok_wide in [(dict(n_what=50, n_steps_per_image=8, n_units=8), True, True),
                                       (dict(n_what=51), False, True), (dict(n_steps_per_image=9), False, True),
                                       (dict(n_units=9), False, True), (dict(n_what=129), False, False),
                                       (dict(n_steps_per_image=17), False, False), (dict(n_units=17), False, False),
                                       (dict(k_particles=256), True, True), (dict(k_particles=257), False, False),
                                       (dict(n_steps_per_image=16, n_what=128), False, False)]:   # (the adjoint's LDS staging)
        cfg = make_config(make_flags(**flags), (50, 50))
        for l, ok in ((lib, ok_product), (wide, ok_wide)):
            rc = l.sqair_create(C.byref(cfg), C.byref(h))
            assert (rc == 0) == ok, (flags, l.sqair_build_flags(), rc)
            if rc == 0:
                l.sqair_destroy(h)


def test_accepted_slot_counts_of_both_builds():
    """n_steps_per_image 1 .. 17: the product build takes up to its 8 slots; the wide build up to 14 -- at 15 and 16 a row of
    k_logprob_bwd (sq_logprob_bwd_lds_bytes at the workspace's pstats pitch) no longer fits 150 KB of LDS.  The two sets are what
    the library accepted when sqair_create still carried its own copy of that size, with 800 where the small parameters take 738."""
    h = C.c_void_p()
    for path, accepted in ((_capi.LIB_PATH, range(1, 9)), (_capi.WIDE_LIB_PATH, range(1, 15))):
        l = _capi.lib(path)
        for N in range(1, 18):
            rc = l.sqair_create(C.byref(make_config(make_flags(n_steps_per_image=N), (50, 50))), C.byref(h))
            assert (rc == 0) == (N in accepted), (l.sqair_build_flags(), N, rc)
            if rc == 0:
                l.sqair_destroy(h)


def test_run_time_options_host_side():
    """sqair_set_option without a GPU: the in-launch slot chain lays the inference workspace out like the training tape for the
    configurations it serves (shipped cells, n_hidden 256, up to 320 particle rows) and leaves the others alone; the wide build
    refuses it; vi_target takes 0 / 1."""
    K5 = dict(k_particles=5, n_steps_per_image=4)
    with handle(**K5) as (lib, h), handle(**K5) as (_, fresh):
        base = lib.sqair_workspace_bytes(h, 10, 32)
        train = lib.sqair_train_workspace_bytes(h, 10, 32)
        assert lib.sqair_set_option(h, b"slot_chain", 1) == 0
        on = lib.sqair_workspace_bytes(h, 10, 32)
        assert on > 5 * base and on >= train          # per-slot buffers kept apart + the launches' control blocks
        assert lib.sqair_workspace_bytes(h, 10, 256) == lib.sqair_workspace_bytes(fresh, 10, 256)   # 1280 rows: the chain keeps out
        assert lib.sqair_set_option(h, b"slot_chain", 0) == 0
        assert lib.sqair_workspace_bytes(h, 10, 32) == base
        assert lib.sqair_set_option(h, b"vi_target", 1) == 0 and lib.sqair_set_option(h, b"vi_target", 0) == 0
        assert lib.sqair_set_option(h, b"vi_target", 7) == -2 and b"vi_target" in lib.sqair_last_error(h)
    with handle(time_transition="LSTM", **K5) as (lib, h):
        base = lib.sqair_workspace_bytes(h, 10, 32)
        assert lib.sqair_set_option(h, b"slot_chain", 1) == 0
        assert lib.sqair_workspace_bytes(h, 10, 32) == base      # LSTM temporal cell: one launch per op
    with handle(_capi.WIDE_LIB_PATH, **K5) as (wide, h):
        assert wide.sqair_set_option(h, b"slot_chain", 1) == -2 and b"wide build" in wide.sqair_last_error(h)


def test_compaction_test_entries_host_side():
    """sqair_compact_test_layout / sqair_compact_test / sqair_compact_bwd_test (tests/test_compact_kernel.py drives them on the
    GPU): exported by both builds under the unchanged ABI version, the layout query answers without a GPU with each build's own
    record, and NULL arguments are refused before any HIP call."""
    for path, W, pres, ident, slots in ((_capi.LIB_PATH, 168, 54, 165, 8), (_capi.WIDE_LIB_PATH, 416, 132, 409, 16)):
        lib = _capi.lib(path)
        for name in ("sqair_compact_test_layout", "sqair_compact_test", "sqair_compact_bwd_test"):
            assert name in _capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert lib.sqair_abi_version() == _capi.ABI_VERSION == 2
        for flags, snh, psnh, spec in ((dict(), 256, 256, path == _capi.LIB_PATH), (dict(time_transition="LSTM"), 512, 256, False),
                                       (dict(n_units=5, prior_transition="LSTM"), 256, 512, False), (dict(n_units=2), 128, 128, False)):
            with handle(path, k_particles=5, n_steps_per_image=4, **flags) as (_, h):
                buf = (C.c_int32 * 24)(*([-5] * 24))
                assert lib.sqair_compact_test_layout(h, buf, 24) == 20
                v = list(buf)
                assert v[20:] == [-5] * 4 and v[:3] == [W, pres, ident] and v[16:19] == [slots, 4, 50]
                assert v[11:13] == [snh, psnh] and v[19] == int(spec)
                assert v[13] == lib.sqair_debug_padded_count(h, None) and 0 <= v[14] <= v[13] - snh and 0 <= v[15] <= v[13] - psnh
                short = (C.c_int32 * 3)()
                assert lib.sqair_compact_test_layout(h, short, 3) == 20 and list(short) == [W, pres, ident]
                assert lib.sqair_compact_test_layout(h, None, 3) == -1 and lib.sqair_compact_test_layout(None, short, 3) == -1
                assert lib.sqair_compact_test(h, *([None] * 13), 0, 1, None) == -1
                assert lib.sqair_compact_bwd_test(h, *([None] * 10), 1, None) == -1


def test_backward_decoder_refusals_host_side():
    """sqair_backward_decoder (the decoder adjoint of the training step as a unit entry) says no before any HIP call to what it
    does not serve -- an n_hidden that is padded, a frame whose H * W is not a multiple of 4 -- and its scratch size answers
    without a GPU."""
    T, B = 3, 4
    buf = (C.c_float * 16)()     # stands for every device buffer: a refusal comes before anything is read
    for flags, hw, msg in ((dict(n_units=5), (50, 50), b"an n_hidden that is padded"), (dict(), (37, 41), b"needs H * W to be a multiple of 4")):
        with handle(hw=hw, k_particles=2, n_steps_per_image=3, **flags) as (lib, h):
            nb =lib.sqair_backward_scratch_bytes(h, T, B)
            assert nb > 0 and lib.sqair_backward_scratch_bytes(h, 0, B) == -1
            rc = lib.sqair_backward_decoder(h, buf, buf, buf, buf, buf, T, B, buf, lib.sqair_workspace_bytes(h, T, B), buf, nb, buf, None,
                                            None)
            assert rc == -1 and msg in lib.sqair_last_error(h), lib.sqair_last_error(h)
            assert lib.sqair_backward_decoder(h, buf, buf, buf, buf, buf, T, B, buf, lib.sqair_workspace_bytes(h, T, B), buf, nb - 4, buf,
                                              None, None) == -1 and b"too small" in lib.sqair_last_error(h)


def _all_set(cls, buf, **over):
    """A description whose every pointer is `buf` and every int a value the entry accepts, then `over`."""
    t = cls()
    for name, typ in cls._fields_:
        setattr(t, name, C.addressof(buf) if typ is C.c_void_p else 1024)
    for k, v in over.items():
        setattr(t, k, v)
    return t


def test_slot_adjoint_test_entries_refuse_host_side():
    """sqair_slot_tail_bwd_test / sqair_crop_chain_bwd_test / sqair_where_param_grads_test / sqair_gru_gates_bwd_test
    (tests/test_slot_adjoint_kernels.py drives them on the GPU): exported by both builds under the unchanged ABI version, and a NULL
    required pointer, a slot out of range, a pitch below the width and a frame that cannot be trained are refused with the entry's
    name in the error text before any HIP call (`buf` stands for every device buffer: nothing reads it).  The same for
    sqair_logprob_test / sqair_logprob_bwd_test (tests/test_logprob_kernels.py): a NULL required pointer, B < 1, T < 1, a pstats pitch
    below 9 + 2 n_what or beyond the LDS."""
    buf = (C.c_float * 16)()
    for path in (_capi.LIB_PATH, _capi.WIDE_LIB_PATH):
        K2 = dict(k_particles=2, n_steps_per_image=3)
        with handle(path, **K2) as (lib, h), handle(path, hw=(200, 200), **K2) as (_, big):
            assert lib.sqair_abi_version() == _capi.ABI_VERSION == 2

            def refused(fn, cls, handle=h, **over):
                name = fn.encode()
                assert fn in _capi.EXPORTED_SYMBOLS
                rc = getattr(lib, fn)(handle, C.byref(_all_set(cls, buf, **over)), None)
                err = lib.sqair_last_error(handle)
                assert rc == -1 and err.startswith(name + b": "), (fn, over, rc, err)
                return err
            for fn in ("sqair_slot_tail_bwd_test", "sqair_crop_chain_bwd_test", "sqair_where_param_grads_test", "sqair_gru_gates_bwd_test"):
                assert getattr(lib, fn)(None, None, None) == -1
                assert getattr(lib, fn)(h, None, None) == -1 and lib.sqair_last_error(h).startswith(fn.encode())
            S, K, W, G = _capi.SqairSlotTailBwdTest, _capi.SqairCropChainBwdTest, _capi.SqairWhereParamGradsTest, _capi.SqairGruGatesBwdTest
            tail = dict(is_disc=0, slot=1, B=2, enc_pre=0)
            for p in ("rec_new", "d_rec_new", "s1h", "enc", "noise", "flat", "d_s1pre", "d_raw_out", "d_enc"):
                assert b"NULL" in refused("sqair_slot_tail_bwd_test", S, **dict(tail, **{p: None}))
            for p in ("rec_prev", "d_rec_prev", "hraw", "d_hraw"):
                assert b"propagation needs" in refused("sqair_slot_tail_bwd_test", S, **dict(tail, **{p: None}))
            for slot in (-1, 3):
                assert b"slot" in refused("sqair_slot_tail_bwd_test", S, **dict(tail, slot=slot))
            assert b"B < 1" in refused("sqair_slot_tail_bwd_test", S, **dict(tail, B=0))
            for ld, v in (("s1h_ld", 127), ("ds_ld", 127), ("ds2_ld", 127), ("enc_ld", 99), ("de_ld", 99), ("dr_ld", 0), ("h_ld", 249),
                          ("dh_ld", 249)):
                assert b"pitch" in refused("sqair_slot_tail_bwd_test", S, **dict(tail, **{ld: v}))
            crop = dict(mode=2, slot=0, B=2, mask_dact=0, g_row_add=0, mask_row_add=0)
            for p in ("img", "g_out", "flat", "d_rec_prev", "rec_new", "d_rec_new", "tp", "d_tp", "noise", "d_mask", "w3", "t2"):
                refused("sqair_crop_chain_bwd_test", K, **dict(crop, **{p: None}))
            for p in ("rec_prev", "wb", "d_wb"):
                refused("sqair_crop_chain_bwd_test", K, **dict(crop, mode=1, **{p: None}))
            for mode in (0, 4):
                assert b"mode" in refused("sqair_crop_chain_bwd_test", K, **dict(crop, mode=mode))
            for slot in (-1, 3):
                assert b"slot" in refused("sqair_crop_chain_bwd_test", K, **dict(crop, slot=slot))
            for ld, v in (("tp_ld", 7), ("dtp_ld", 7), ("t2_ld", 255), ("dt2_ld", 255), ("g_row_mul", 0), ("mask_row_mul", 0)):
                assert b"pitch" in refused("sqair_crop_chain_bwd_test", K, **dict(crop, **{ld: v}))
            for ld, v in (("wb_ld", 3), ("g_row_mul", 2), ("mask_row_mul", 2)):   # crop #1 covers the N = 3 slots of a row
                assert b"pitch" in refused("sqair_crop_chain_bwd_test", K, **dict(crop, mode=1, **{ld: v}))
            assert b"200 x 200" in refused("sqair_crop_chain_bwd_test", K, handle=big, **crop)   # a frame the crop adjoint cannot stage
            wpg = dict(T=2, B=2, tp_ld=8)
            for p in ("d_tp", "d_rec_p", "rec_p", "noise", "flat_grad"):
                assert b"NULL" in refused("sqair_where_param_grads_test", W, **dict(wpg, **{p: None}))
            assert b"pitch" in refused("sqair_where_param_grads_test", W, **dict(wpg, tp_ld=7))
            assert b"T < 1" in refused("sqair_where_param_grads_test", W, **dict(wpg, T=0))
            gru = dict(rows=4, accumulate_dh=0, dup_h_off=-1, h_ld=0)
            for p in ("d_hn", "z", "r", "hc", "hprev", "d_rh", "dpre1", "d_h"):
                assert b"NULL" in refused("sqair_gru_gates_bwd_test", G, **dict(gru, **{p: None}))
            for ld, v in (("dhn_ld", 255), ("z_ld", 255), ("r_ld", 255), ("hc_ld", 255), ("h_ld", 255), ("drh_ld", 255), ("dp_ld", 767),
                          ("dh_ld", 255), ("dupz_ld", 255), ("dupr_ld", 255)):
                assert b"pitch" in refused("sqair_gru_gates_bwd_test", G, **dict(gru, **{ld: v}))
            assert b"pitch" in refused("sqair_gru_gates_bwd_test", G, **dict(gru, dup_h_off=512, dupz_ld=767))
            assert b"rows" in refused("sqair_gru_gates_bwd_test", G, **dict(gru, rows=0))
            # the log-probability kernels' entries (tests/test_logprob_kernels.py): the same rules
            for fn in ("sqair_logprob_test", "sqair_logprob_bwd_test"):
                assert getattr(lib, fn)(None, None, None) == -1
                assert getattr(lib, fn)(h, None, None) == -1 and lib.sqair_last_error(h).startswith(fn.encode())
            LF, LB = _capi.SqairLogprobTest, _capi.SqairLogprobBwdTest
            fwd = dict(B=2, T=3, t=2, t_global=0, ps_ld=112)
            for p in ("rec_p", "rec_d", "rec_prev", "pstats", "spre", "flat", "qz", "pz", "disc_lp"):
                assert b"NULL" in refused("sqair_logprob_test", LF, **dict(fwd, **{p: None}))
            bwd = dict(B=2, T=3, t_global0=0, ps_ld=112)
            for p in ("rec_p", "rec_d", "rec_m", "pstats", "spre", "g_lw", "g_dl", "d_rec_p", "d_rec_d", "d_rec_m", "d_pstats", "d_spre", "flat",
                      "flat_grad"):
                assert b"NULL" in refused("sqair_logprob_bwd_test", LB, **dict(bwd, **{p: None}))
            for fn, cls, ok in (("sqair_logprob_test", LF, fwd), ("sqair_logprob_bwd_test", LB, bwd)):
                assert b"B < 1" in refused(fn, cls, **dict(ok, B=0))
                assert b"T < 1" in refused(fn, cls, **dict(ok, T=0))
                assert b"pitch" in refused(fn, cls, **dict(ok, ps_ld=9 + 2 * 50 - 1))        # below [logit | 4 + n_what | 4 + n_what]
                assert b"LDS" in refused(fn, cls, **dict(ok, ps_ld=1 << 20))                  # a row that no longer fits the LDS
            assert b"t < 0" in refused("sqair_logprob_test", LF, **dict(fwd, t=-1))
            assert b"200 x 200" in refused("sqair_logprob_bwd_test", LB, handle=big, **bwd)  # a configuration that cannot be trained


def test_slot_forward_test_entries_refuse_host_side():
    """sqair_slot_crop_test / sqair_slot_tail_test / sqair_linear_what_test (tests/test_slot_forward_kernels.py drives them on the
    GPU): exported by both builds under the unchanged ABI version; a NULL required pointer, a mode or slot out of range, B < 1, a pitch
    below the width, an operand that is not 16-byte aligned, tp together with t2, tp_out without t2, the RNN block where the tail
    cannot ride in the next slot's layer (the wide library, a GRU slot cell, the last slot), what_done and the whole of
    sqair_linear_what_test on the wide library are refused with the entry's name in the error text before any HIP call (`buf` stands
    for every device buffer: nothing reads it)."""
    buf = (C.c_float * 16)()
    CR, TL, WH = _capi.SqairSlotCropTest, _capi.SqairSlotTailTest, _capi.SqairLinearWhatTest
    for path in (_capi.LIB_PATH, _capi.WIDE_LIB_PATH):
        wide = path == _capi.WIDE_LIB_PATH
        K2 = dict(k_particles=2, n_steps_per_image=3)
        with handle(path, **K2) as (lib, h), handle(path, transition="GRU", **K2) as (_, gru):
            assert lib.sqair_abi_version() == _capi.ABI_VERSION == 2

            def call(fn, cls, handle=h, **over):
                assert fn in _capi.EXPORTED_SYMBOLS
                return getattr(lib, fn)(handle, C.byref(_all_set(cls, buf, **over)), None), lib.sqair_last_error(handle)

            def refused(fn, cls, handle=h, **over):
                rc, err = call(fn, cls, handle, **over)
                assert rc == -1 and err.startswith(fn.encode() + b": "), (fn, over, rc, err)
                return err
            for fn in ("sqair_slot_crop_test", "sqair_slot_tail_test", "sqair_linear_what_test"):
                assert getattr(lib, fn)(None, None, None) == -1
                assert getattr(lib, fn)(h, None, None) == -1 and lib.sqair_last_error(h).startswith(fn.encode())
            # the crop: mode 2 with t2 (so tp NULL) is a description the entry accepts up to the launch
            crop = dict(mode=2, slot=1, B=2, specialised=0, tp=None, out_row_add=0, mask_row_add=0)
            for p in ("img", "out", "flat", "rec_new", "noise", "rec_prev", "w3"):
                refused("sqair_slot_crop_test", CR, **dict(crop, **{p: None}))
            for p in ("rec_prev", "wb"):
                assert b"mode 1" in refused("sqair_slot_crop_test", CR, **dict(crop, mode=1, **{p: None}))
            for mode in (0, 4):
                assert b"mode" in refused("sqair_slot_crop_test", CR, **dict(crop, mode=mode))
            for slot in (-1, 3):
                assert b"slot" in refused("sqair_slot_crop_test", CR, **dict(crop, slot=slot))
            assert b"B < 1" in refused("sqair_slot_crop_test", CR, **dict(crop, B=0))
            assert b"exactly one" in refused("sqair_slot_crop_test", CR, **dict(crop, tp=C.addressof(buf)))
            assert b"exactly one" in refused("sqair_slot_crop_test", CR, **dict(crop, t2=None))
            assert b"tp_out needs t2" in refused("sqair_slot_crop_test", CR, **dict(crop, tp=C.addressof(buf), t2=None))
            for ld, v in (("t2_ld", 255), ("tp_out_ld", 7), ("out_row_mul", 0), ("out_row_add", -1), ("mask_row_mul", 0), ("mask_row_add", -1)):
                assert b"pitch" in refused("sqair_slot_crop_test", CR, **dict(crop, **{ld: v}))
            assert b"pitch" in refused("sqair_slot_crop_test", CR, **dict(crop, tp=C.addressof(buf), t2=None, tp_out=None, tp_ld=7))
            for ld, v in (("wb_ld", 3), ("out_row_mul", 2), ("mask_row_mul", 2)):   # crop #1 covers the N = 3 slots of a row
                assert b"pitch" in refused("sqair_slot_crop_test", CR, **dict(crop, mode=1, **{ld: v}))
            assert b"aligned" in refused("sqair_slot_crop_test", CR, **dict(crop, t2=C.addressof(buf) + 4))
            assert b"aligned" in refused("sqair_slot_crop_test", CR, **dict(crop, w3=C.addressof(buf) + 8))
            assert b"aligned" in refused("sqair_slot_crop_test", CR, **dict(crop, t2_ld=1026))
            # the tail, without the RNN block
            tail = dict(is_disc=0, slot=1, B=2, what_done=0, out=None)
            for p in ("rec_new", "noise", "s1p", "flat", "packed", "enc"):
                assert b"NULL" in refused("sqair_slot_tail_test", TL, **dict(tail, **{p: None}))
            for p in ("rec_prev", "hraw"):
                assert b"propagation needs" in refused("sqair_slot_tail_test", TL, **dict(tail, **{p: None}))
            for slot in (-1, 3):
                assert b"slot" in refused("sqair_slot_tail_test", TL, **dict(tail, slot=slot))
            assert b"B < 1" in refused("sqair_slot_tail_test", TL, **dict(tail, B=0))
            for ld, v in (("s1p_ld", 127), ("s1h_ld", 127), ("enc_ld", 99), ("h_ld", 249)):
                assert b"pitch" in refused("sqair_slot_tail_test", TL, **dict(tail, **{ld: v}))
            rnn = dict(tail, slot=0, out=C.addressof(buf))
            if wide:
                assert b"what_done" in refused("sqair_slot_tail_test", TL, **dict(tail, what_done=1))
                assert b"RNN block" in refused("sqair_slot_tail_test", TL, **rnn)
            else:
                assert b"RNN block" in refused("sqair_slot_tail_test", TL, handle=gru, **rnn)          # a GRU slot cell: no fused tail
                assert b"slot + 1" in refused("sqair_slot_tail_test", TL, **dict(rnn, slot=2))           # the last slot has no next layer
                for p in ("hid", "add"):
                    assert b"RNN block needs" in refused("sqair_slot_tail_test", TL, **dict(rnn, **{p: None}))
                for ld in ("hid_ld", "add_ld", "out_ld"):
                    assert b"pitch" in refused("sqair_slot_tail_test", TL, **dict(rnn, **{ld: 255}))
                assert b"aligned" in refused("sqair_slot_tail_test", TL, **dict(rnn, hid=C.addressof(buf) + 4))
                assert b"aligned" in refused("sqair_slot_tail_test", TL, **dict(rnn, hid_ld=1026))
            # the head layer with the what sample in its epilogue
            what = dict(mode=1, slot=1, B=2)
            if wide:
                assert b"wide library" in refused("sqair_linear_what_test", WH, **what)
            else:
                for p in ("x", "noise", "rec_new", "packed"):
                    assert b"NULL" in refused("sqair_linear_what_test", WH, **dict(what, **{p: None}))
                for p in ("enc", "rec_prev"):
                    assert b"mode 1" in refused("sqair_linear_what_test", WH, **dict(what, **{p: None}))
                for mode in (-1, 2):
                    assert b"mode" in refused("sqair_linear_what_test", WH, **dict(what, mode=mode))
                for slot in (-1, 3):
                    assert b"slot" in refused("sqair_linear_what_test", WH, **dict(what, slot=slot))
                assert b"B < 1" in refused("sqair_linear_what_test", WH, **dict(what, B=0))
                for ld, v in (("x_ld", 255), ("enc_ld", 99)):
                    assert b"pitch" in refused("sqair_linear_what_test", WH, **dict(what, **{ld: v}))
                rc, err = call("sqair_linear_what_test", WH, **dict(what, x_ld=1026))                   # the launcher's own refusal: its code
                assert rc == -5 and err.startswith(b"sqair_linear_what_test: "), (rc, err)


# ---- the binding is read from the header (sqair_amd/_abi.py): gcc (tests/abi_host.py) judges what the parser read -------------------
def test_every_struct_has_the_header_layout(tmp_path):
    """Every struct of the header is passed by address: the ctypes classes made from the parse must have the size, the field offsets
    and the field sizes a C compiler gives the header's structs.  The struct list is the header's, not a list kept here."""
    structs = _abi.header().structs
    assert len(structs) >= 30 and {"SqairConfig", "SqairOutputs", "SqairSmc", "SqairCarry", "SqairDenseContract", "SqairDxTest",
                                   "SqairLogprobBwdTest", "SqairLinearWhatTest"} <= set(structs)
    # the parse skipped none and kept the order: every closing brace of the header is a parsed struct's or the extern "C" guard's
    closes = [code().index("}} {};".format(name)) for name in structs]
    assert code().count("}") == len(structs) + 1 and closes == sorted(closes)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "sqair_hip.h"', "int main(void) {"]
    for name, fields in structs.items():
        lines.append('  printf("{0} %zu\\n", sizeof({0}));'.format(name))
        for f in fields:
            lines.append('  printf("{0}.{1} %zu %zu\\n", offsetof({0}, {1}), sizeof((({0}*)0)->{1}));'.format(name, f.name))
    got = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in _gcc(tmp_path, "layout", lines + ["  return 0;", "}"]).splitlines()}
    for name, fields in structs.items():
        cls = getattr(_capi, name)
        assert issubclass(cls, C.Structure) and [n for n, _ in cls._fields_] == [f.name for f in fields], name
        assert got[name] == [C.sizeof(cls)], name
        for f in fields:
            assert got[name + "." + f.name] == [getattr(cls, f.name).offset, getattr(cls, f.name).size], (name, f.name)
    # the forms a field takes
    assert _capi.SqairCarry.smc.offset == 40 and dict(_capi.SqairCarry._fields_)["smc"] is C.POINTER(_capi.SqairSmc)
    assert dict(_capi.SqairLogprobTest._fields_)["out"] is C.c_void_p          # an address set as an integer
    assert dict(_capi.SqairConfig._fields_)["where_prior_mean"] is C.c_float * 4
    assert dict(_capi.SqairDxTest._fields_)["gru"] is _capi.SqairDxGru and dict(_capi.SqairDxTest._fields_)["r"] is _capi.SqairDxRange * 3
    assert len(_capi.DENSE_ROUTES) == constant("SQAIR_DENSE_ROUTES")


def test_every_prototype_reads_as_the_compiler_reads_it(tmp_path):
    """One _Static_assert per function of the header: the type of the function is the return type and the parameters printed back
    from the parse, const-ness, base type and pointer depth.  Nothing is linked or run.  The mapping to ctypes is then a table: one
    function of each kind."""
    functions = _abi.header().functions
    # the parse skipped none: every parenthesis of the header opens the parameters of a parsed function
    assert code().count("(") == len(functions) >= 103 and all(name + "(" in code() for name in functions)

    def claim(name, ret, params):
        return '_Static_assert(__builtin_types_compatible_p(__typeof__(&{0}), {1} (*)({2})), "{0}");'.format(
            name, _abi.spell(ret), ", ".join(_abi.spell(p) for p in params) or "void")
    head = ['#include "sqair_hip.h"']
    assert _gcc(tmp_path, "protos", head + [claim(n, *f) for n, f in functions.items()], run=False) == 0
    # (the claim can fail: one const dropped, one depth off)
    ret, params = functions["sqair_elbo"]
    assert _abi.spell(params[10]) == "const float* const*"
    for wrong in (params[10]._replace(pointer_const=()), params[10]._replace(pointer_depth=1, pointer_const=())):
        assert _gcc(tmp_path, "wrong", head + [claim("sqair_elbo", ret, params[:10] + [wrong] + params[11:])], run=False) != 0
    P, V, I = C.POINTER, C.c_void_p, C.c_int
    for name, want in (("sqair_create", (I, [P(_capi.SqairConfig), V])), ("sqair_last_error", (C.c_char_p, [V])),
                       ("sqair_set_option", (I, [V, C.c_char_p, I])), ("sqair_history_bytes", (C.c_int64, [V, I, I, I, C.c_uint32])),
                       ("sqair_forward_train_carry", (I, [V] * 5 + [I, I, P(_capi.SqairCarry), P(_capi.SqairOutputs), V, C.c_int64, V])),
                       ("sqair_fill_noise", (I, [V, V, I, I, I, I, C.c_uint64, C.c_uint64, V]))):
        assert _capi._PROTOS[name] == want, name
        fn = getattr(_capi.lib(), name)
        assert fn.restype is want[0] and list(fn.argtypes) == want[1], name


_EVERY_CONSTRUCT = """/* a comment
 * over lines, with a ; and a { in it */
#ifndef SQAIR_T_H
#define SQAIR_T_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define SQAIR_N 3u
#define SQAIR_M 12   /* trailing */
typedef struct SqairHandle SqairHandle;
typedef struct SqairIn {
  int32_t a, b;      /* two declarators */
  float m[4];
  const float* p; float*  q;
} SqairIn;
typedef struct {
  SqairIn in; SqairIn two[2];
  const SqairIn* ref;
  int64_t* n; double* d; uint64_t seed; uint32_t bits; char tag; void* any;
} SqairOut;
int sqair_version(void);
const char* sqair_name(const SqairHandle* h);
int64_t sqair_run(SqairHandle** out, const SqairOut* o /* NULL: off */,
                  const float* const* rows, const char* name, int n, float x, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SQAIR_T_H */
"""


def test_the_parser_reads_the_subset_and_refuses_the_rest(tmp_path):
    F, P = _abi.Field, _abi.Param

    def parse(text):
        (tmp_path / "t.h").write_text(text)
        return _abi.parse_header(str(tmp_path / "t.h"))
    got = parse(_EVERY_CONSTRUCT)
    assert got.constants == {"SQAIR_N": 3, "SQAIR_M": 12}
    assert list(got.structs.items()) == [
        ("SqairIn", [F("a", "int32_t", False, 0, None), F("b", "int32_t", False, 0, None), F("m", "float", False, 0, 4),
                     F("p", "float", True, 1, None), F("q", "float", False, 1, None)]),
        ("SqairOut", [F("in", "SqairIn", False, 0, None), F("two", "SqairIn", False, 0, 2), F("ref", "SqairIn", True, 1, None),
                      F("n", "int64_t", False, 1, None), F("d", "double", False, 1, None), F("seed", "uint64_t", False, 0, None),
                      F("bits", "uint32_t", False, 0, None), F("tag", "char", False, 0, None), F("any", "void", False, 1, None)])]
    assert list(got.functions.items()) == [
        ("sqair_version", (P("", "int", False, 0), [])),
        ("sqair_name", (P("", "char", True, 1), [P("h", "SqairHandle", True, 1)])),
        ("sqair_run", (P("", "int64_t", False, 0), [P("out", "SqairHandle", False, 2), P("o", "SqairOut", True, 1),
                                                    P("rows", "float", True, 2, (0,)), P("name", "char", True, 1), P("n", "int", False, 0),
                                                    P("x", "float", False, 0), P("stream", "void", False, 1)]))]
    classes, protos = _abi.bind(got)
    assert [t for _, t in classes["SqairOut"]._fields_] == [classes["SqairIn"], classes["SqairIn"] * 2, C.POINTER(classes["SqairIn"]),
                                                           C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_char, C.c_void_p]
    assert protos["sqair_run"] == (C.c_int64, [C.c_void_p, C.POINTER(classes["SqairOut"]), C.c_void_p, C.c_char_p, C.c_int, C.c_float,
                                               C.c_void_p])
    assert protos["sqair_name"] == (C.c_char_p, [C.c_void_p]) and protos["sqair_version"] == (C.c_int, [])
    # what the subset leaves out fails, and the message names the text
    for text, named in (("typedef struct S { int32_t a : 3; } S;", "int32_t a : 3"),
                        ("typedef union U { int32_t a; float b; } U;", "typedef union U { int32_t a"),
                        ("typedef enum { SQAIR_A, SQAIR_B } E;", "typedef enum { SQAIR_A, SQAIR_B } E"),
                        ("typedef struct S { void (*fn)(int); } S;", "void (*fn)(int)"),
                        ("typedef struct S { size_t n; } S;", "size_t n"),
                        ("int sqair_f(unsigned n);", "unsigned n"),
                        ("int sqair_f(SqairLater* p);", "SqairLater* p"),
                        ("void sqair_f(int n);", "void sqair_f(int n);"),
                        ("typedef struct S { int32_t* a, b; } S;", "int32_t* a, b"),
                        ("typedef struct S { float*** p; } S;", "float*** p"),
                        ("#define SQAIR_X (1 << 3)", "#define SQAIR_X (1 << 3)"),
                        ("#define SQAIR_X 0x10", "0x10"),
                        ("typedef struct S { int32_t a;", "typedef struct S { int32_t a"),
                        ("int sqair_f(int n); /* no end", "/* no end"),
                        ("int sqair_f(int n);\n}", "}")):
        with pytest.raises(_abi.HeaderError) as e:
            parse(text)
        assert named in str(e.value), (text, str(e.value))


def test_importing_the_binding_without_the_header_says_why(tmp_path, monkeypatch):
    monkeypatch.setattr(_abi, "HEADER_PATH", str(tmp_path / "include" / "sqair_hip.h"))
    _abi.header.cache_clear()
    try:
        with pytest.raises(ImportError, match="read from the C header, and the header ships with the library"):
            _abi.header()
    finally:
        monkeypatch.undo()
        _abi.header.cache_clear()
    assert _abi.header() is _abi.header() and "SqairConfig" in _abi.header().structs   # parsed once per process


# the *_INT_FIELDS tuples as they were written by hand before the binding was read from the header: the recorded result to reproduce
_INT_FIELDS_BEFORE = dict(FORECAST_LANE_INT_FIELDS=("best_row",), ESTIMATE_INT_FIELDS=("best_row", "map_count"),
                          LAYERS_INT_FIELDS=("match", "owner"), SCORE_INT_FIELDS=("truth_match", "tp", "fn", "fp", "idsw"),
                          TRAJ_INT_FIELDS=("link", "state", "count_map"), TRACK_LANE_INT_FIELDS=("best_row", "first_frame"))


def test_buffer_element_types_are_the_headers():
    """What the allocation code asks the binding -- the element type of a struct's pointer field -- against the field's type as the
    header spells it, and for a few against the words of the header's text."""
    txt = " ".join(code().split())      # (runs of blanks as one)
    names = {"float*": "float32", "const float*": "float32", "int32_t*": "int32", "const int32_t*": "int32", "int64_t*": "int64",
             "double*": "float64"}
    for struct, fields in (("SqairLaneScore", ("truth_box", "truth_present", "truth_valid", "counts", "iou_sum", "last_id", "match_iou", "tp")),
                           ("SqairLaneIdentity", ("trk_id", "trk_box", "trk_what", "next_id", "counts", "lane_id")),
                           ("SqairLaneIdf", ("col_id", "overlap", "frames", "totals")),
                           ("SqairTrajScore", ("counts", "sums", "lane_counts", "link", "link_iou")),
                           ("SqairTraceOutputs", ("where", "log_w", "valid", "ancestor_row", "track_id", "track_where"))):
        spelled = {n: ty for ty, n in header_fields(struct)}
        for f in fields:
            assert _capi.field_dtype(struct, f) == names[spelled[f]], (struct, f)
    assert "double* iou_sum;" in txt and _capi.field_dtype("SqairLaneScore", "iou_sum") == "float64"
    assert "int64_t* counts;" in txt and _capi.field_dtype("SqairLaneScore", "counts") == "int64"
    assert "int32_t* truth_present;" in txt and _capi.field_dtype("SqairLaneScore", "truth_present") == "int32"
    assert "float* trk_box" in txt and _capi.field_dtype("SqairLaneIdentity", "trk_box") == "float32"
    assert "int64_t* open," in prototype("sqair_lane_idf_solve") and _capi.field_dtype("sqair_lane_idf_solve", "open") == "int64"   # a parameter
    for scalar in (("SqairLaneScore", "G"), ("SqairCarry", "smc"), ("SqairCarry", "state_in")):   # no array of a device type
        with pytest.raises(KeyError):
            _capi.field_dtype(*scalar)
    for name, before in _INT_FIELDS_BEFORE.items():
        assert getattr(_capi, name) == before, name
    assert _capi.IDENT_INT_FIELDS == _capi.IDENT_FIELDS == ("lane_id", "how", "track_len")
