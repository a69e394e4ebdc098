"""Reference for the forward kernels of the slot loop (k_crop_row, k_slot_tail, k_rnn_tail, k_linear_what).

The tail (gated `what` mixture, sample, steps predictor, presence logit) and the crop chain (where sample, spatial transformer, mask)
are tests/slot_adjoint_ref.py's tail_forward / crop_forward, which tests/test_slot_adjoint_ref.py pins against the oracle.  New here is
only what those leave out, written on the oracle's own functions (oracle/sqair_oracle.py) and run in float64 and float32 from the same
code: the presence Bernoulli, the z-record of a finished slot, the next slot's VanillaRNN layer on it, the two head layers in front of
the `what` sample, the transform's output layer in front of the `where` sample, and what a launch reads of records and noise.

Which rows of a parameter a launch reads comes from the ORACLE's input order (the torch.cat lines of discovery_core /
propagation_core, restated in RNN_INPUT and STEPS_FEATURES and pinned by tests/test_slot_forward_ref.py), never from the library's
packing plan.  Parameters are dictionaries of the oracle's names; a reference slices the rows it needs, so every other row may be NaN.

`mistake(name)` makes one deliberate mistake (MISTAKES) in whatever is evaluated inside it: the power check of
tests/test_slot_forward_ref.py applies each to the float32 evaluation and asks the GPU cases' bars to see it."""
import contextlib

import numpy as np
import torch

from oracle import sqair_oracle as O
from tests import slot_adjoint_ref as R

# slot_rnn's input, in order (discovery_core: rnn_inpt; propagation_core: rnn_inpt); widths: nh, nw, 4 or 1
RNN_INPUT = {"disc": (("input_enc", "nh"), ("cond", "nh"), ("what", "nw"), ("where", 4), ("pres", 1)),
             "prop": (("loc1", "nw"), ("what", "nw"), ("where", 4), ("pres", 1), ("what_tm1", "nw"), ("where_tm1", 4), ("pres_tm1", 1),
                      ("temporal", "nh"))}
# compute_presence's features, in order (discovery_core: [hidden, what]; propagation_core: [hidden, temporal_state, what])
STEPS_FEATURES = {"disc": (("hidden", "nh"), ("what", "nw")), "prop": (("hidden", "nh"), ("temporal", "nh"), ("what", "nw"))}

MISTAKES = ("disc_head_swapped", "min_std_dropped", "gate_complement", "what_tm1_wrong_slot", "disc_prev_from_slot_k", "absent_logit_80",
            "u_le_prob", "prop_scale_offset_minus_1_dropped", "cholesky_transposed", "crop_xy_exchanged", "grid_G_for_G_minus_1")
_mistake = None


def rows_of(order, field, nh, nw):
    """(first, last + 1) of `field` among the rows of a matrix whose inputs come in `order`."""
    at = 0
    for name, w in order:
        w = dict(nh=nh, nw=nw).get(w, w)
        if name == field:
            return at, at + w
        at += w
    raise KeyError(field)


def _st_crop_grid_G(img, where_logits, G):
    """O.st_crop with the grid -1 + 2 j / G (the mistake) for linspace(-1, 1, G) = -1 + 2 j / (G - 1)."""
    _, H, W = img.shape
    sx, sy, tx, ty = O.to_coords(where_logits)
    g = -1.0 + 2.0 * torch.arange(G, dtype=img.dtype) / G
    x = 0.5 * (W - 1) * (sx[:, None] * g[None, :] + tx[:, None] + 1.0)
    y = 0.5 * (H - 1) * (sy[:, None] * g[None, :] + ty[:, None] + 1.0)
    return O.bilinear_gather(img, x, y)


@contextlib.contextmanager
def mistake(name):
    """Everything evaluated inside makes the mistake `name` (None: nothing changes)."""
    global _mistake
    assert name is None or name in MISTAKES, name
    saved = (R.MIN_STD, R.ABSENT_LOGIT, R.gates_of, R.where_tril, R.where_scale_of, O.st_crop, _mistake)
    gates_of, where_tril, st_crop = R.gates_of, R.where_tril, O.st_crop
    try:
        _mistake = name
        if name == "min_std_dropped":
            R.MIN_STD = 0.0
        elif name == "absent_logit_80":
            R.ABSENT_LOGIT = 80.0
        elif name == "gate_complement":          # 1 - gate for gate, on the forget gate (the first third)
            def wrong(raw):
                g = gates_of(raw)
                n = g.shape[-1] // 3
                return torch.cat([1.0 - g[..., :n], g[..., n:]], -1)
            R.gates_of = wrong
        elif name == "prop_scale_offset_minus_1_dropped":
            R.where_scale_of = lambda raw, offset, is_disc: O.softplus(raw + offset) + R.MIN_STD
        elif name == "cholesky_transposed":
            R.where_tril = lambda ch, scale: where_tril(ch, scale).transpose(-1, -2)
        elif name == "crop_xy_exchanged":
            O.st_crop = lambda img, wl, G: st_crop(img, wl[..., [1, 0, 3, 2]], G)
        elif name == "grid_G_for_G_minus_1":
            O.st_crop = _st_crop_grid_G
        yield
    finally:
        R.MIN_STD, R.ABSENT_LOGIT, R.gates_of, R.where_tril, R.where_scale_of, O.st_crop, _mistake = saved


def params(P, dtype):
    return {k: R.T(v, dtype) for k, v in P.items()}


# ------------------------------------------------------------------------------------------------ what a launch reads of records and noise
def slot_operands(rec_prev, rec_new, noise, L, is_disc, slot, nw, dtype):
    """Of records [R, N, W] (columns L) and one frame's noise [R, 2, N, 4 + nw + 1]: the noise of (phase, slot), the previous presence
    (discovery: 1 at slot 0, else this frame's slot - 1; propagation: t - 1's slot), and in propagation what / where of t - 1."""
    ph = 1 if is_disc else 0
    nz = R.T(noise, dtype)[:, ph, slot]
    o = dict(eps_where=nz[:, :4], eps=nz[:, 4:4 + nw], u=nz[:, 4 + nw])
    if is_disc:
        k = slot if _mistake == "disc_prev_from_slot_k" else slot - 1
        o["prev"] = torch.ones(nz.shape[0], dtype=dtype) if slot == 0 else R.T(rec_new, dtype)[:, k, L["PRES"]]
    else:
        rp = R.T(rec_prev, dtype)
        k = (slot + 1) % rp.shape[1] if _mistake == "what_tm1_wrong_slot" else slot
        o.update(prev=rp[:, slot, L["PRES"]], what_tm1=rp[:, k, L["WHAT"]:L["WHAT"] + nw], where_tm1=rp[:, slot, L["WHERE"]:L["WHERE"] + 4])
    return o


# ------------------------------------------------------------------------------------------------ the head layers in front of the sample
def gaussian_head(P, name, feat):
    """SqairOracle.gaussian_head: loc | softplus(raw) + 1e-2 of linear(name)."""
    s = O.linear(P, name, feat)
    n = s.shape[-1] // 2
    loc, raw = s[..., :n], s[..., n:]
    if _mistake == "disc_head_swapped" and name == "enc.what_head":
        loc, raw = raw, loc
    return loc, O.softplus(raw) + R.MIN_STD


def prop_heads_raw(P, feat):
    """propagation_core: the raw what-head (loc, raw scale) and the three raw gates of the new temporal state = tail_forward's hraw."""
    return torch.cat([O.linear(P, "prop.what_head", feat), O.linear(P, "prop.gates", feat)], -1)


def transform_out(P, core, t2):
    """The transform's output layer on its second hidden layer's activations (discovery_core / propagation_core: tp)."""
    return O.linear(P, core + ".transform.l2", t2)


# ------------------------------------------------------------------------------------------------ the tail, with the Bernoulli
def what_sample(ops, is_disc, enc_loc, enc_scale, hraw=None):
    """what, what_loc, what_scale alone (tail_forward without a steps predictor)."""
    z = torch.zeros(enc_loc.shape[0], 1, dtype=enc_loc.dtype)
    lv = dict(enc_loc=enc_loc, enc_scale=enc_scale, bump=torch.zeros_like(enc_loc), s1_rest=z)
    if not is_disc:
        lv.update(hraw=hraw, what_tm1=ops["what_tm1"])
    c = dict(eps=ops["eps"], w_what=torch.zeros(enc_loc.shape[1], 1, dtype=enc_loc.dtype), w2=z[0], b2=z[0, 0], prev=ops["prev"], is_disc=is_disc)
    t = R.tail_forward(lv, c)
    return {k: t[k] for k in ("what", "what_loc", "what_scale")}


def tail(P, core, nh, ops, s1p, enc_loc=None, enc_scale=None, hraw=None, what=None):
    """The slot's tail from the operands of its launch; `what` given (what_done): the sample exists, the mixture is skipped.
    P: {core}.steps.l0.w (its `what` rows are read), .steps.l1.w, .steps.l1.b.  Adds prob and the presence (u < prob) * prev."""
    is_disc = core == "disc"
    nw = ops["eps"].shape[-1]
    r0, r1 = rows_of(STEPS_FEATURES[core], "what", nh, nw)
    c = dict(eps=ops["eps"], w_what=P[core + ".steps.l0.w"][r0:r1], w2=P[core + ".steps.l1.w"][:, 0], b2=P[core + ".steps.l1.b"][0],
             prev=ops["prev"], is_disc=is_disc)
    if what is not None:   # loc + 0 * eps: the given sample, exactly
        lv = dict(enc_loc=what, enc_scale=torch.zeros_like(what), bump=torch.zeros_like(what), s1_rest=s1p)
        t = R.tail_forward(lv, dict(c, is_disc=True, eps=torch.zeros_like(what)))   # (the `what` noise is not an operand then)
        t = {k: v for k, v in t.items() if k not in ("what_loc", "what_scale")}
    else:
        lv = dict(enc_loc=enc_loc, enc_scale=enc_scale, bump=torch.zeros_like(enc_loc), s1_rest=s1p)
        if not is_disc:
            lv.update(hraw=hraw, what_tm1=ops["what_tm1"])
        t = R.tail_forward(lv, c)
    t["prob"] = torch.sigmoid(t["logit"])                                     # compute_presence
    hit = (ops["u"] <= t["prob"]) if _mistake == "u_le_prob" else (ops["u"] < t["prob"])
    t["pres"] = hit.to(s1p.dtype) * ops["prev"]
    # the size of the logit's terms (the scale its error is judged on: a sum of products that may cancel)
    t["logit_terms"] = ops["prev"] * (t["hidden"].abs() @ c["w2"].abs() + c["b2"].abs()) + (1.0 - ops["prev"]) * R.ABSENT_LOGIT
    return t


# ------------------------------------------------------------------------------------------------ the z-record and the next slot's layer
def z_record(where, what, pres, logit):
    """[where 4 | what n_what | presence | logit] of a finished slot."""
    return torch.cat([where, what, pres[:, None], logit[:, None]], -1)


def next_slot_layer(P, core, nh, z, hidden, add):
    """slot_rnn (VanillaRNN) of the next slot: tanh(rnn_inpt W_i + hidden W_h + b), with everything of rnn_inpt W_i + b that does not
    come from the finished slot's record in `add`.  Of {core}.rnn.i2h.w the rows of what, where and presence are read (the logit has
    none), of {core}.rnn.h2h.w all."""
    nw = z.shape[-1] - 6
    Wi = P[core + ".rnn.i2h.w"]
    where, what, pres = z[:, :4], z[:, 4:4 + nw], z[:, 4 + nw:5 + nw]
    pre = add + hidden @ P[core + ".rnn.h2h.w"]
    for name, x in (("what", what), ("where", where), ("pres", pres)):
        r0, r1 = rows_of(RNN_INPUT[core], name, nh, nw)
        pre = pre + x @ Wi[r0:r1]
    return torch.tanh(pre)


# ------------------------------------------------------------------------------------------------ metric helpers shared with the GPU tests
def np64(t):
    return {k: np.asarray(v.detach().numpy(), np.float64) for k, v in t.items()}
