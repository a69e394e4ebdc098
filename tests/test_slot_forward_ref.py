"""The reference of the slot loop's forward kernels (tests/slot_forward_ref.py), pinned without a GPU.

Part A: the pieces slot_forward_ref adds to the adjoint reference -- the head layers in front of the `what` sample, the transform's
output layer, the presence Bernoulli, the z-record with the next slot's layer, what a launch reads of the records -- reproduce
SqairOracle.discovery_core / propagation_core for one slot and the slot after it, with a GRU and an LSTM temporal cell (the heads read the
hidden half of [h | c]).

Part B: the power check over the GPU module's own case list (built without a GPU): each mistake of slot_forward_ref.MISTAKES, made in the
float32 evaluation of the reference, puts at least one (case, output) of tests/test_slot_forward_kernels.py over that output's bar."""
import numpy as np
import pytest
import torch

from oracle import sqair_oracle as O
from sqair_amd.flags import make_flags
from sqair_amd.params import init_params
from tests import slot_adjoint_ref as R
from tests import slot_forward_ref as SF

F64 = torch.float64
HW, G, NW, NH, B, N = (14, 17), 6, 7, 128, 5, 3
L = dict(W=40, WHERE=1, WHAT=5, PRES=12, LOGIT=13)        # a record layout of this test's own


def _close(a, b, tol=1e-12):
    a, b = a.detach().numpy(), b.detach().numpy().reshape(a.shape)
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), np.abs(a - b).max()


@pytest.fixture(scope="module", params=["GRU", "LSTM"])
def model(request):
    F = make_flags(n_units=NH // 32, n_what=NW, glimpse_size=G, n_steps_per_image=N, k_particles=1, time_transition=request.param)
    P = init_params(F, HW, seed=5, jitter=0.3)
    P["prop.cholesky_scale"] = np.linspace(-0.6, 0.7, 10)
    orc = O.SqairOracle(P, O.make_cfg(F, HW), F64)
    rng = np.random.default_rng(11)
    t = lambda *s: torch.as_tensor(rng.standard_normal(s))
    snh = 2 * NH if request.param == "LSTM" else NH
    x = dict(img=torch.as_tensor(rng.uniform(size=(B,) + HW)), what_tm1=t(B, N, NW), where_tm1=t(B, N, 4) * 0.5,
             pres_tm1=torch.as_tensor([[1.0, 1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 1], [0, 0, 1]]), temporal=t(B, N, snh) * 0.5,
             what_km1=t(B, NW), where_km1=t(B, 4), pres_km1=torch.as_tensor([[1.0], [1.0], [0.0], [1.0], [1.0]]), hidden=t(B, NH) * 0.5,
             noise=t(B, 2, N, NW + 5), cond=t(B, NH))
    x["noise"][..., -1] = torch.as_tensor(rng.uniform(size=(B, 2, N)))
    return orc, x, request.param


def _records(x, slot, is_disc, where_now=None):
    """The records a launch of `slot` reads, NaN everywhere else."""
    rec_prev, rec_new = np.full((B, N, L["W"]), np.nan), np.full((B, N, L["W"]), np.nan)
    if is_disc:
        if slot > 0:
            rec_new[:, slot - 1, L["PRES"]] = x["pres_km1"][:, 0].numpy()
    else:
        rec_prev[:, slot, L["PRES"]] = x["pres_tm1"][:, slot].numpy()
        rec_prev[:, slot, L["WHAT"]:L["WHAT"] + NW] = x["what_tm1"][:, slot].numpy()
        rec_prev[:, slot, L["WHERE"]:L["WHERE"] + 4] = x["where_tm1"][:, slot].numpy()
    return rec_prev, rec_new


def test_propagation_slot_and_the_next_slots_layer(model):
    orc, x, cell = model
    P, k = orc.P, 1
    nz = x["noise"][:, 0, k]
    z_k = (x["what_tm1"][:, k], x["where_tm1"][:, k], x["pres_tm1"][:, k:k + 1], torch.zeros(B, 1, dtype=F64))
    state = (x["what_km1"], x["where_km1"], x["pres_km1"], x["hidden"])
    with R.recorded() as rec:
        out, state2 = orc.propagation_core(x["img"], z_k, x["temporal"][:, k], state, nz[:, :4], nz[:, 4:4 + NW], nz[:, 4 + NW:])
    rec_prev, rec_new = _records(x, k, False)
    ops = SF.slot_operands(rec_prev, rec_new, x["noise"].numpy(), L, False, k, NW, F64)
    _close(ops["prev"], x["pres_tm1"][:, k]); _close(ops["what_tm1"], x["what_tm1"][:, k]); _close(ops["where_tm1"], x["where_tm1"][:, k])
    _close(ops["eps_where"], nz[:, :4]); _close(ops["eps"], nz[:, 4:4 + NW]); _close(ops["u"], nz[:, 4 + NW])
    # the transform's output layer on the second hidden layer's activations
    _close(SF.transform_out(P, "prop", O.elu(rec["prop.transform.l1"][0])), rec["prop.transform.l2"][0])
    # the glimpse encoder's Gaussian head (crop #2) and the heads on the new temporal state's HIDDEN part
    feat = O.mlp2_hidden(P, "enc.glimpse", rec["enc.glimpse:in"][1])
    loc2, scale2 = SF.gaussian_head(P, "enc.what_head", feat)
    t_out = out["temporal_state"][:, :NH]
    if cell == "LSTM":
        assert out["temporal_state"].shape[1] == 2 * NH
    hraw = SF.prop_heads_raw(P, t_out)
    _close(hraw, torch.cat([rec["prop.what_head"][0], rec["prop.gates"][0]], -1))
    s = SF.what_sample(ops, False, loc2, scale2, hraw)
    for f in ("what", "what_loc", "what_scale"):
        _close(s[f], out[f])
    # the tail with the Bernoulli: s1p = the hidden pre-activation without the `what` rows' part
    r0, r1 = SF.rows_of(SF.STEPS_FEATURES["prop"], "what", NH, NW)
    w0 = P["prop.steps.l0.w"]
    assert r1 == w0.shape[0]
    s1p = rec["prop.steps.l0"][0] - out["what"] @ w0[r0:r1]
    t = SF.tail(P, "prop", NH, ops, s1p, enc_loc=loc2, enc_scale=scale2, hraw=hraw)
    _close(t["logit"], out["presence_logit"]); _close(t["prob"], out["presence_prob"])
    assert torch.equal(t["pres"], out["presence"][:, 0]) and 0 < float(t["pres"].sum()) < B
    assert torch.all(t["logit"][x["pres_tm1"][:, k] == 0] == -88.0)
    given = SF.tail(P, "prop", NH, ops, s1p, what=out["what"])                     # what_done
    _close(given["logit"], out["presence_logit"]); assert torch.equal(given["pres"], t["pres"])
    assert torch.all(t["logit_terms"] >= t["logit"].abs() * (1 - 1e-12))
    # the z-record and slot k + 1's layer: its hidden state as the oracle computes it from the state slot k leaves
    z = SF.z_record(out["where"], out["what"], t["pres"], t["logit"])
    z_n = (x["what_tm1"][:, k + 1], x["where_tm1"][:, k + 1], x["pres_tm1"][:, k + 1:k + 2], torch.zeros(B, 1, dtype=F64))
    nz2 = x["noise"][:, 0, k + 1]
    with R.recorded() as rec2:
        out2, state3 = orc.propagation_core(x["img"], z_n, x["temporal"][:, k + 1], state2, nz2[:, :4], nz2[:, 4:4 + NW], nz2[:, 4 + NW:])
    tau = x["temporal"][:, k + 1, NH:] if cell == "LSTM" else x["temporal"][:, k + 1]
    loc1 = SF.gaussian_head(P, "enc.what_head", O.mlp2_hidden(P, "enc.glimpse", rec2["enc.glimpse:in"][0]))[0]
    rest = torch.cat([loc1, torch.zeros(B, NW + 5, dtype=F64), z_n[0], z_n[1], z_n[2], tau], -1)
    add = rest @ P["prop.rnn.i2h.w"] + P["prop.rnn.i2h.b"] + P["prop.rnn.h2h.b"]
    _close(SF.next_slot_layer(P, "prop", NH, z, state2[3], add), state3[3])


def test_discovery_slot_and_the_next_slots_layer(model):
    orc, x, _ = model
    P, k = orc.P, 1
    nz = x["noise"][:, 1, k]
    state = (x["what_km1"], x["where_km1"], x["pres_km1"], x["hidden"])
    with R.recorded() as rec:
        out, state2 = orc.discovery_core(x["img"], x["cond"], state, nz[:, :4], nz[:, 4:4 + NW], nz[:, 4 + NW:])
    rec_prev, rec_new = _records(x, k, True)
    ops = SF.slot_operands(rec_prev, rec_new, x["noise"].numpy(), L, True, k, NW, F64)
    _close(ops["prev"], x["pres_km1"][:, 0]); _close(ops["eps"], nz[:, 4:4 + NW]); _close(ops["u"], nz[:, 4 + NW])
    assert torch.equal(SF.slot_operands(rec_prev, rec_new, x["noise"].numpy(), L, True, 0, NW, F64)["prev"], torch.ones(B, dtype=F64))
    _close(SF.transform_out(P, "disc", O.elu(rec["disc.transform.l1"][0])), rec["disc.transform.l2"][0])
    feat = O.mlp2_hidden(P, "enc.glimpse", rec["enc.glimpse:in"][0])
    loc, scale = SF.gaussian_head(P, "enc.what_head", feat)
    _close(loc, out["what_loc"]); _close(scale, out["what_scale"])
    _close(SF.what_sample(ops, True, loc, scale)["what"], out["what"])
    r0, r1 = SF.rows_of(SF.STEPS_FEATURES["disc"], "what", NH, NW)
    w0 = P["disc.steps.l0.w"]
    assert r1 == w0.shape[0]
    t = SF.tail(P, "disc", NH, ops, rec["disc.steps.l0"][0] - out["what"] @ w0[r0:r1], enc_loc=loc, enc_scale=scale)
    _close(t["what"], out["what"]); _close(t["logit"], out["presence_logit"]); _close(t["prob"], out["presence_prob"])
    assert torch.equal(t["pres"], out["presence"][:, 0])
    z = SF.z_record(out["where"], out["what"], t["pres"], t["logit"])
    nz2 = x["noise"][:, 1, k + 1]
    out2, state3 = orc.discovery_core(x["img"], x["cond"], state2, nz2[:, :4], nz2[:, 4:4 + NW], nz2[:, 4 + NW:])
    rest = torch.cat([orc.input_encoder(x["img"]), x["cond"], torch.zeros(B, NW + 5, dtype=F64)], -1)
    add = rest @ P["disc.rnn.i2h.w"] + P["disc.rnn.i2h.b"] + P["disc.rnn.h2h.b"]
    _close(SF.next_slot_layer(P, "disc", NH, z, state2[3], add), state3[3])


def test_a_mistake_is_undone_on_the_way_out():
    saved = (R.MIN_STD, R.ABSENT_LOGIT, R.gates_of, R.where_tril, R.where_scale_of, O.st_crop)
    for m in SF.MISTAKES:
        with SF.mistake(m):
            pass
        assert saved == (R.MIN_STD, R.ABSENT_LOGIT, R.gates_of, R.where_tril, R.where_scale_of, O.st_crop)


# ------------------------------------------------------------------------------------------------ the power check
# u <= prob for u < prob differs from the right comparison only on a row with u == prob exactly, which the presence condition of the
# GPU cases (|u - prob64| >= 1e-3) rules out: no case can see it, and none is asked to.
UNSEEN = ("u_le_prob",)
KERNELS_OF = dict(disc_head_swapped=("linear_what",), min_std_dropped=("linear_what", "slot_tail", "rnn_tail", "crop"),
                  gate_complement=("slot_tail", "rnn_tail", "linear_what"), what_tm1_wrong_slot=("slot_tail", "rnn_tail", "linear_what"),
                  disc_prev_from_slot_k=("slot_tail", "rnn_tail"), absent_logit_80=("slot_tail", "rnn_tail"), u_le_prob=("slot_tail", "rnn_tail"),
                  prop_scale_offset_minus_1_dropped=("crop",), cholesky_transposed=("crop",), crop_xy_exchanged=("crop",),
                  grid_G_for_G_minus_1=("crop",))


@pytest.fixture(scope="module")
def gpu_cases():
    from tests import test_slot_forward_kernels as K
    K.cases()
    yield K
    K.close_handles()


def test_gpu_case_list_meets_its_conditions(gpu_cases):
    """What the GPU cases promise, verified here: every uniform at least 1e-3 from the float64 probability, a row with u = 0 and one
    with the largest float below 1, rows with previous presence 0 (logit exactly -88, presence 0), both presence outcomes; the shapes
    the kernels' structure asks for."""
    K = gpu_cases
    seen = dict(R=set(), nw=set(), nh=set(), wd=set(), s1h=set(), phase=set(), slot0=set())
    for kern in ("slot_tail", "rnn_tail"):
        for name, c in K.cases(kern).items():
            inp, ref = c["inp"], c["ref"]
            hd = K.handle(inp["hname"])
            u = inp["noise"][:, 1 if inp["is_disc"] else 0, inp["slot"], 4 + hd.nw].astype(np.float64)
            assert np.all(np.abs(u - ref["prob"][:, 0]) >= K.U_MARGIN), name
            if inp["R"] >= 5:
                assert (u == 0).any() and (u == K.U_MAX).any(), name
            if inp["R"] > 1 and not (inp["is_disc"] and inp["slot"] == 0):
                assert (ref["logit"][:, 0] == -88.0).any(), name
            if inp["R"] >= 16:
                assert 0 < ref["pres"].sum() < inp["R"], name
            if kern == "slot_tail":
                for k, v in dict(R=inp["R"], nw=hd.nw, nh=hd.nh, wd=inp["wd"], s1h=inp["s1h"], phase=inp["is_disc"], slot0=inp["slot"] == 0).items():
                    seen[k].add((hd.wide, v))
    assert {(False, r) for r in (1, 5, 16, 17, 37)} <= seen["R"] and {(False, w) for w in (1, 7, 10, 33, 50)} <= seen["nw"]
    assert {(True, 64), (True, 65), (True, 128)} <= seen["nw"] and {(False, 128), (False, 256), (True, 512)} <= seen["nh"]
    for k in ("wd", "s1h", "phase", "slot0"):
        assert {(False, False), (False, True)} <= seen[k], k
    rows = {(K.handle(c["inp"]["hname"]).nh, c["inp"]["R"]) for c in K.cases("rnn_tail").values()}
    assert {(256, 256), (256, 259), (128, 512), (128, 515)} <= rows
    what = {(c["inp"]["mode"], K.handle(c["inp"]["hname"]).nh) for c in K.cases("linear_what").values()}
    assert what == {(0, 128), (0, 256), (1, 128), (1, 256)}
    assert {c["inp"]["R"] for c in K.cases("linear_what").values()} >= {1, 17, 160, 6001}
    assert {K.handle(c["inp"]["hname"]).nw for c in K.cases("linear_what").values()} >= {1, 3, 10, 33, 50}


@pytest.mark.parametrize("mistake", SF.MISTAKES)
def test_gpu_cases_see_the_mistake(gpu_cases, mistake):
    K = gpu_cases
    seen = None
    for kern in KERNELS_OF[mistake]:
        bars = {k: (0.0 if k == "pres" else R.bar_from_fp32(v)) for k, v in K.worst32(kern).items()}
        for case in sorted(K.CASES[kern]):
            over = {k: (e, bars[k]) for k, e in K.mutated_errors(kern, case, mistake).items() if not e <= bars[k]}
            if over:
                seen = (kern, case, {k: "%.2e > %.2e" % v for k, v in over.items()})
                break
        if seen:
            break
    if mistake in UNSEEN:
        assert seen is None, "a case violates the presence condition: " + str(seen)
        return
    assert seen is not None, "no (case, output) of tests/test_slot_forward_kernels.py exceeds its bar with " + mistake
    print(mistake, "seen by", *seen)
    # and without the mistake the float32 reference is under every bar (the bars are 8 x its own worst error)
    kern, case, _ = seen
    clean = K.mutated_errors(kern, case, None)
    assert all(e <= (0.0 if k == "pres" else R.bar_from_fp32(K.worst32(kern)[k])) for k, e in clean.items())
