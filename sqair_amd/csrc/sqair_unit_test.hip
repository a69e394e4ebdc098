// The kernel unit-test entries: one kernel (or one fused pair) of the pass on caller-owned device buffers, through the launchers and
// the argument builders the pass itself calls, so that what a test launches is what a pass launches.  Host code only: this unit holds
// no kernel.  (The dense family's entries: sqair_dense_test.hip.  The Python side of the tests: tests/kernel_unit.py.)
#include <vector>

#include "sqair_internal.h"
#include "sqair_bwd.h"

// An entry that takes a description `t` opens with this: NULL handle -1, NULL description refused by name.
#define SQ_UNIT_ENTRY(name)           \
  static const char* who = name;      \
  if (!h) return -1;                  \
  if (!t) return sq_refuse(h, who, "no description")
// ... and every entry ends with this: the launcher's refusal (rc != 0) under the entry's name, else the launch and its completion checked.
static int sq_unit_done(SqairHandle* h, const char* who, int rc, const char* refused, hipStream_t s) {
  if (rc != 0) { sq_set_error(h, std::string(who) + ": " + refused); return rc; }
  SQ_CHECK_HIP(hipGetLastError());
  SQ_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// Slot compaction on raw device buffers (tests/test_compact_kernel.py; its adjoint: sqair_compact_bwd_test below): the launch of the
// frame loop with the handle's Dims, one frame.  The layout query tells a caller the widths and columns of THIS build's buffers, so that a
// test hard-codes neither the product nor the wide record.
extern "C" int sqair_compact_test_layout(const SqairHandle* h, int32_t* out, int n) {
  if (!h || !out || n < 0) return -1;
  const Dims d = make_dims(h->cfg, 1);
  const int32_t v[20] = {rec::W, rec::PRES, rec::ID, rec::WHERE, rec::WHAT, rec::LOGIT, rec::WHERE_LOC, rec::WHERE_SCALE, rec::WHAT_LOC,
                         rec::WHAT_SCALE, rec::PROB, d.snh, d.psnh, (int32_t)h->n_params, h->po.temporal_init, h->po.prior_init,
                         SQ_MAXN, d.N, d.nw, sq_spec_ok(d) ? 1 : 0};
  for (int i = 0; i < n && i < 20; ++i) out[i] = v[i];
  return 20;
}
extern "C" int sqair_compact_test(SqairHandle* h, const float* rec_p, const float* rec_d, const float* rec_prev, const float* temporal_p,
                                  const float* prior_p, const float* last_id_prev, const float* flat, float* rec_next,
                                  float* temporal_next, float* prior_next, float* last_id_next, int32_t* src_out,
                                  const SqairOutputs* out, int t, int B, void* stream) {
  if (!h || !rec_p || !rec_d || !rec_prev || !temporal_p || !prior_p || !last_id_prev || !flat || !rec_next || !temporal_next ||
      !prior_next || !last_id_next || !src_out || !out || t < 0 || B < 1) return -1;
  hipStream_t s = (hipStream_t)stream;
  Dims d = make_dims(h->cfg, B);
  d.spec = h->opt_specialised && sq_spec_ok(d) ? (h->opt_specialised_mask & SPEC_ALL) : 0;
  CompactArgs ka; memset(&ka, 0, sizeof(ka));
  ka.rec_p = rec_p; ka.rec_d = rec_d; ka.rec_prev = rec_prev; ka.temporal_p = temporal_p; ka.prior_p = prior_p;
  ka.last_id_prev = last_id_prev; ka.last_id_next = last_id_next;
  ka.rec_next = rec_next; ka.temporal_next = temporal_next; ka.prior_next = prior_next;
  ka.flat = flat; ka.t = t; ka.out = *out; ka.src_out = src_out;
  sq_launch_compact(ka, h->po, d, s);
  return sq_unit_done(h, "sqair_compact_test", 0, "", s);
}
// the compaction adjoint on raw device buffers
extern "C" int sqair_compact_bwd_test(SqairHandle* h, const int32_t* src, const float* d_rec_next, const float* d_temporal_next,
                                      const float* d_prior_next, float* d_rec_p, float* d_rec_d, float* d_temporal_p, float* d_prior_p,
                                      float* d_new_temporal, float* d_new_prior, int B, void* stream) {
  if (!h || !src || !d_rec_next || !d_temporal_next || !d_prior_next || !d_rec_p || !d_rec_d || !d_temporal_p || !d_prior_p ||
      !d_new_temporal || !d_new_prior || B < 1) return -1;
  hipStream_t s = (hipStream_t)stream;
  const Dims d = make_dims(h->cfg, B);
  // the kernel indexes LDS with `src`: refuse anything that is not N distinct slots of [0, 2N) per row (the forward's src_out is)
  std::vector<int32_t> hs((size_t)d.R * d.N);
  SQ_CHECK_HIP(hipMemcpyAsync(hs.data(), src, hs.size() * 4, hipMemcpyDeviceToHost, s));
  SQ_CHECK_HIP(hipStreamSynchronize(s));
  for (int r = 0; r < d.R; ++r) {
    unsigned seen = 0;
    for (int j = 0; j < d.N; ++j) {
      const int32_t v = hs[(size_t)r * d.N + j];
      if (v < 0 || v >= 2 * d.N || (seen >> v & 1u)) { sq_set_error(h, "sqair_compact_bwd_test: src is not a slot selection"); return -1; }
      seen |= 1u << v;
    }
  }
  CompactBwdArgs ka; memset(&ka, 0, sizeof(ka));
  ka.src = src; ka.d_rec_next = d_rec_next; ka.d_temporal_next = d_temporal_next; ka.d_prior_next = d_prior_next;
  ka.d_rec_p = d_rec_p; ka.d_rec_d = d_rec_d; ka.d_temporal_p = d_temporal_p; ka.d_prior_p = d_prior_p;
  ka.d_new_temporal = d_new_temporal; ka.d_new_prior = d_new_prior;
  sq_launch_compact_bwd(ka, h->po, d, s);
  return sq_unit_done(h, "sqair_compact_bwd_test", 0, "", s);
}

// ------------------------------------------------------------------------------------------------
// The element-wise adjoints of the slot loop on raw device buffers (unit-test entries, tests/test_slot_adjoint_kernels.py): the
// caller's pointers and pitches reach the launchers of the reverse sweep unchanged; Dims, POff and the parameter offsets are the
// handle's, through the helpers sq_backward itself calls (sq_pass_dims, sq_tail_param_offsets, sq_crop_slots).
// ------------------------------------------------------------------------------------------------
extern "C" int sqair_slot_tail_bwd_test(SqairHandle* h, const SqairSlotTailBwdTest* t, void* stream) {
  SQ_UNIT_ENTRY("sqair_slot_tail_bwd_test");
  if (t->B < 1) return sq_refuse(h, who, "B < 1");
  const Dims d = sq_pass_dims(h, t->B, 0);
  const int nsp = d.nh / 2;
  const bool disc = t->is_disc != 0;
  if (t->slot < 0 || t->slot >= d.N) return sq_refuse(h, who, "slot outside [0, N)");
  if (!t->rec_new || !t->d_rec_new || !t->s1h || !t->enc || !t->noise || !t->flat || !t->d_s1pre || !t->d_raw_out || !t->d_enc)
    return sq_refuse(h, who, "a required pointer is NULL");
  if (!disc && (!t->rec_prev || !t->d_rec_prev || !t->hraw || !t->d_hraw))
    return sq_refuse(h, who, "propagation needs rec_prev, d_rec_prev, hraw and d_hraw");
  if (t->s1h_ld < nsp || t->ds_ld < nsp || (t->d_s1pre2 && t->ds2_ld < nsp) || t->enc_ld < 2 * d.nw || t->de_ld < 2 * d.nw || t->dr_ld < 1 ||
      (!disc && (t->h_ld < 5 * d.nw || t->dh_ld < 5 * d.nw)))
    return sq_refuse(h, who, "a pitch is smaller than the width");
  hipStream_t s = (hipStream_t)stream;
  TailBwdArgs ta; memset(&ta, 0, sizeof(ta));
  ta.is_disc = disc ? 1 : 0; ta.slot = t->slot; ta.rec_prev = t->rec_prev; ta.rec_new = t->rec_new; ta.d_rec_new = t->d_rec_new;
  ta.d_rec_prev = t->d_rec_prev; ta.s1h = t->s1h; ta.s1h_ld = t->s1h_ld; ta.hraw = t->hraw; ta.h_ld = t->h_ld; ta.enc = t->enc;
  ta.enc_ld = t->enc_ld; ta.noise = t->noise; ta.d_s1pre = t->d_s1pre; ta.ds_ld = t->ds_ld; ta.d_s1pre2 = t->d_s1pre2; ta.ds2_ld = t->ds2_ld;
  ta.enc_pre = t->enc_pre; ta.d_raw_out = t->d_raw_out; ta.dr_ld = t->dr_ld; ta.d_enc = t->d_enc; ta.de_ld = t->de_ld;
  ta.d_hraw = t->d_hraw; ta.dh_ld = t->dh_ld; ta.flat = t->flat;
  sq_tail_param_offsets(h, disc, &ta);
  const int rc = sq_launch_slot_tail_bwd(ta, d, s);
  return sq_unit_done(h, who, rc, "launch refused (dynamic LDS limit)", s);
}

extern "C" int sqair_crop_chain_bwd_test(SqairHandle* h, const SqairCropChainBwdTest* t, void* stream) {
  SQ_UNIT_ENTRY("sqair_crop_chain_bwd_test");
  if (t->B < 1) return sq_refuse(h, who, "B < 1");
  if (t->mode != CROP_PROP1 && t->mode != CROP_PROP2 && t->mode != CROP_DISC) return sq_refuse(h, who, "mode is not 1, 2 or 3");
  const Dims d = sq_pass_dims(h, t->B, 0);
  const bool p1 = t->mode == CROP_PROP1;
  const int nslots = sq_crop_slots(t->mode, d);
  if (!p1 && (t->slot < 0 || t->slot >= d.N)) return sq_refuse(h, who, "slot outside [0, N)");
  if (!t->img || !t->g_out || !t->flat || !t->d_rec_prev) return sq_refuse(h, who, "a required pointer is NULL");
  if (p1 && (!t->rec_prev || !t->wb || !t->d_wb)) return sq_refuse(h, who, "mode 1 needs rec_prev, wb and d_wb");
  if (!p1 && (!t->rec_new || !t->d_rec_new || !t->tp || !t->d_tp || !t->noise))
    return sq_refuse(h, who, "modes 2 and 3 need rec_new, d_rec_new, tp, d_tp and noise");
  if (t->mask && !t->d_mask) return sq_refuse(h, who, "a mask needs d_mask");
  if (t->d_t2 && !p1 && (!t->w3 || !t->t2)) return sq_refuse(h, who, "d_t2 needs w3 and t2");
  if ((p1 && t->wb_ld < 4) || (!p1 && (t->tp_ld < 8 || t->dtp_ld < 8)) || (t->d_t2 && !p1 && (t->t2_ld < d.nh || t->dt2_ld < d.nh)) ||
      t->g_row_mul < nslots || t->g_row_add < 0 || (t->mask && (t->mask_row_mul < nslots || t->mask_row_add < 0)))
    return sq_refuse(h, who, "a pitch is smaller than the width");
  if (!sq_trainable_frame(h)) return sq_refuse(h, who, std::string(sqair_last_error(h)));
  hipStream_t s = (hipStream_t)stream;
  CropChainBwdArgs ca; memset(&ca, 0, sizeof(ca));
  ca.mode = t->mode; ca.slot = t->slot; ca.img = t->img; ca.rec_prev = t->rec_prev; ca.rec_new = t->rec_new; ca.d_rec_prev = t->d_rec_prev;
  ca.d_rec_new = t->d_rec_new; ca.wb = t->wb; ca.wb_ld = t->wb_ld; ca.d_wb = t->d_wb; ca.mask = t->mask; ca.mask_row_mul = t->mask_row_mul;
  ca.mask_row_add = t->mask_row_add; ca.d_mask = t->d_mask; ca.mask_dact = t->mask_dact; ca.g_out = t->g_out; ca.g_row_mul = t->g_row_mul;
  ca.g_row_add = t->g_row_add; ca.tp = t->tp; ca.tp_ld = t->tp_ld; ca.d_tp = t->d_tp; ca.dtp_ld = t->dtp_ld; ca.noise = t->noise;
  ca.flat = t->flat; ca.w3 = t->w3; ca.t2 = t->t2; ca.t2_ld = t->t2_ld; ca.d_t2 = t->d_t2; ca.dt2_ld = t->dt2_ld;
  const int rc = sq_launch_crop_chain_bwd(ca, h->po, d, nslots, s);
  return sq_unit_done(h, who, rc, "launch refused (frame alignment or dynamic LDS limit)", s);
}

extern "C" int sqair_where_param_grads_test(SqairHandle* h, const SqairWhereParamGradsTest* t, void* stream) {
  SQ_UNIT_ENTRY("sqair_where_param_grads_test");
  if (t->T < 1 || t->B < 1) return sq_refuse(h, who, "T < 1 or B < 1");
  if (!t->d_tp || !t->d_rec_p || !t->rec_p || !t->noise || !t->flat_grad) return sq_refuse(h, who, "a required pointer is NULL");
  if (t->tp_ld < 8) return sq_refuse(h, who, "a pitch is smaller than the width");
  const Dims d = sq_pass_dims(h, t->B, 0);
  if ((int64_t)t->T * d.R * d.N > (int64_t)1 << 24) return sq_refuse(h, who, "more than 2^24 (frame, row, slot) rows");
  hipStream_t s = (hipStream_t)stream;
  sq_launch_where_param_grads(t->d_tp, t->tp_ld, t->d_rec_p, t->rec_p, t->noise, t->T, d, t->flat_grad, h->po, s);
  return sq_unit_done(h, who, 0, "", s);
}

extern "C" int sqair_gru_gates_bwd_test(SqairHandle* h, const SqairGruGatesBwdTest* t, void* stream) {
  SQ_UNIT_ENTRY("sqair_gru_gates_bwd_test");
  const int nh = h->cfg.n_hidden;
  if (t->rows < 1 || (int64_t)t->rows * nh > (int64_t)1 << 30) return sq_refuse(h, who, "rows outside [1, 2^30 / n_hidden]");
  if (!t->d_hn || !t->z || !t->r || !t->hc || !t->hprev || !t->d_rh || !t->dpre1 || !t->d_h) return sq_refuse(h, who, "a required pointer is NULL");
  if (t->dhn_ld < nh || t->z_ld < nh || t->r_ld < nh || t->hc_ld < nh || (t->h_ld != 0 && t->h_ld < nh) || t->drh_ld < nh || t->dp_ld < 3 * nh ||
      t->dh_ld < nh || (t->dup_z && t->dupz_ld < (t->dup_h_off >= 0 ? t->dup_h_off + nh : nh)) || (t->dup_r && t->dupr_ld < nh))
    return sq_refuse(h, who, "a pitch is smaller than the width");
  hipStream_t s = (hipStream_t)stream;
  sq_launch_gru_bwd_a(t->d_hn, t->dhn_ld, t->z, t->z_ld, t->hc, t->hc_ld, t->hprev, t->h_ld, t->dpre1, t->dp_ld, t->d_h, t->dh_ld, t->rows, nh,
                      t->accumulate_dh, s, t->dup_z, t->dupz_ld, t->dup_h_off);
  sq_launch_gru_bwd_b(t->d_rh, t->drh_ld, t->r, t->r_ld, t->hprev, t->h_ld, t->dpre1, t->dp_ld, t->d_h, t->dh_ld, t->rows, nh, s, t->dup_r,
                      t->dupr_ld);
  return sq_unit_done(h, who, 0, "", s);
}

// ------------------------------------------------------------------------------------------------
// The log-probability kernels on raw device buffers (unit-test entries, tests/test_logprob_kernels.py): k_logprob as section H of
// the forward pass launches it, k_logprob_bwd as H^T of sq_backward does.  The caller's pointers, the pstats pitch and the time
// source reach sq_launch_logprob / sq_launch_logprob_bwd unchanged; Dims, POff and SqairConfig are the handle's.
// ------------------------------------------------------------------------------------------------
extern "C" int sqair_logprob_test(SqairHandle* h, const SqairLogprobTest* t, void* stream) {
  SQ_UNIT_ENTRY("sqair_logprob_test");
  if (t->B < 1) return sq_refuse(h, who, "B < 1");
  if (t->T < 1) return sq_refuse(h, who, "T < 1");
  if (t->t < 0) return sq_refuse(h, who, "t < 0");
  if (!t->rec_p || !t->rec_d || !t->rec_prev || !t->pstats || !t->flat || !t->qz || !t->pz || !t->disc_lp)
    return sq_refuse(h, who, "a required pointer is NULL");
  if (h->cfg.rec_where_prior && !t->spre) return sq_refuse(h, who, "a required pointer is NULL (spre: the recurrent where prior reads it)");
  const Dims d = make_dims(h->cfg, t->B);
  if (t->ps_ld < 9 + 2 * d.nw) return sq_refuse(h, who, "a pitch is smaller than the width");
  if (sq_logprob_lds_bytes(d, t->ps_ld) > 150 * 1024) return sq_refuse(h, who, "a pitch asks for more than 150 KB of LDS");
  hipStream_t s = (hipStream_t)stream;
  LogprobArgs la; memset(&la, 0, sizeof(la));
  la.rec_p = t->rec_p; la.rec_d = t->rec_d; la.rec_prev = t->rec_prev; la.pstats = t->pstats; la.ps_ld = t->ps_ld; la.spre = t->spre;
  la.flat = t->flat; la.t_global = t->t_global; la.t_row = t->t_row; la.t = t->t; la.n_frames = t->T; la.qz = t->qz; la.pz = t->pz;
  la.disc_lp = t->disc_lp; la.gen = nullptr; la.cfg = h->cfg;
  if (t->out) la.out = *t->out;
  const int rc = sq_launch_logprob(la, h->po, d, s);
  return sq_unit_done(h, who, rc, "launch refused (dynamic LDS limit)", s);
}

extern "C" int sqair_logprob_bwd_test(SqairHandle* h, const SqairLogprobBwdTest* t, void* stream) {
  SQ_UNIT_ENTRY("sqair_logprob_bwd_test");
  if (t->B < 1) return sq_refuse(h, who, "B < 1");
  if (t->T < 1) return sq_refuse(h, who, "T < 1");
  if (!t->rec_p || !t->rec_d || !t->rec_m || !t->pstats || !t->g_lw || !t->g_dl || !t->d_rec_p || !t->d_rec_d || !t->d_rec_m || !t->d_pstats ||
      !t->d_spre || !t->flat || !t->flat_grad)
    return sq_refuse(h, who, "a required pointer is NULL");
  if (h->cfg.rec_where_prior && !t->spre) return sq_refuse(h, who, "a required pointer is NULL (spre: the recurrent where prior reads it)");
  const Dims d = sq_pass_dims(h, t->B, 0);
  if (t->ps_ld < 9 + 2 * d.nw) return sq_refuse(h, who, "a pitch is smaller than the width");
  if (sq_logprob_bwd_lds_bytes(d, t->ps_ld) > 150 * 1024) return sq_refuse(h, who, "a pitch asks for more than 150 KB of LDS");
  if (!sq_trainable_frame(h)) return sq_refuse(h, who, std::string(sqair_last_error(h)));
  hipStream_t s = (hipStream_t)stream;
  LogprobBwdArgs la; memset(&la, 0, sizeof(la));
  la.rec_p = t->rec_p; la.rec_d = t->rec_d; la.rec_m = t->rec_m; la.pstats = t->pstats; la.ps_ld = t->ps_ld; la.spre = t->spre;
  la.g_lw = t->g_lw; la.g_dl = t->g_dl; la.d_rec_p = t->d_rec_p; la.d_rec_d = t->d_rec_d; la.d_rec_m = t->d_rec_m;
  la.d_pstats = t->d_pstats; la.d_spre = t->d_spre; la.flat = t->flat; la.flat_grad = t->flat_grad; la.t_global0 = t->t_global0;
  la.t_row = t->t_row; la.cfg = h->cfg;
  const int rc = sq_launch_logprob_bwd(la, h->po, d, t->T, s);
  return sq_unit_done(h, who, rc, "launch refused (dynamic LDS limit)", s);
}

// ------------------------------------------------------------------------------------------------
// The forward kernels of the slot loop on raw device buffers (unit-test entries, tests/test_slot_forward_kernels.py): k_crop_row,
// k_slot_tail, k_rnn_tail and k_linear_what through the argument builders and the launch helpers the pass itself calls (sq_pass_dims,
// sq_crop_args, sq_tail_args, sq_run_rnn_tail, sq_run_what: sqair_api.hip), so that what a test launches is what a pass launches.
// ------------------------------------------------------------------------------------------------
extern "C" int sqair_slot_crop_test(SqairHandle* h, const SqairSlotCropTest* t, void* stream) {
  SQ_UNIT_ENTRY("sqair_slot_crop_test");
  if (t->B < 1) return sq_refuse(h, who, "B < 1");
  if (t->mode != CROP_PROP1 && t->mode != CROP_PROP2 && t->mode != CROP_DISC) return sq_refuse(h, who, "mode is not 1, 2 or 3");
  const Dims d = sq_pass_dims(h, t->B, t->specialised ? SPEC_CROP : 0);
  const bool p1 = t->mode == CROP_PROP1;
  const int nslots = sq_crop_slots(t->mode, d);
  if (!p1 && (t->slot < 0 || t->slot >= d.N)) return sq_refuse(h, who, "slot outside [0, N)");
  if (!t->img || !t->out || !t->flat) return sq_refuse(h, who, "a required pointer is NULL");
  if (p1 && (!t->rec_prev || !t->wb)) return sq_refuse(h, who, "mode 1 needs rec_prev and wb");
  if (!p1 && (!t->rec_new || !t->noise)) return sq_refuse(h, who, "modes 2 and 3 need rec_new and noise");
  if (t->mode == CROP_PROP2 && !t->rec_prev) return sq_refuse(h, who, "mode 2 needs rec_prev");
  if (!p1 && (t->tp != nullptr) == (t->t2 != nullptr)) return sq_refuse(h, who, "modes 2 and 3 need exactly one of tp and t2");
  if (!p1 && t->t2 && !t->w3) return sq_refuse(h, who, "t2 needs w3");
  if (!p1 && t->tp_out && !t->t2) return sq_refuse(h, who, "tp_out needs t2 (the launch writes it from its own output layer)");
  if ((p1 && t->wb_ld < 4) || (!p1 && t->tp && t->tp_ld < 8) || (!p1 && t->t2 && t->t2_ld < d.nh) || (!p1 && t->tp_out && t->tp_out_ld < 8) ||
      t->out_row_mul < nslots || t->out_row_add < 0 || (t->mask && (t->mask_row_mul < nslots || t->mask_row_add < 0)))
    return sq_refuse(h, who, "a pitch is smaller than the width");
  if (!p1 && t->t2 && ((reinterpret_cast<uintptr_t>(t->t2) & 15) != 0 || (t->t2_ld & 3) != 0 || (reinterpret_cast<uintptr_t>(t->w3) & 15) != 0))
    return sq_refuse(h, who, "t2 / w3 are not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  CropOperands co; memset(&co, 0, sizeof(co));
  co.mode = t->mode; co.slot = t->slot; co.img = t->img; co.mask = t->mask; co.mask_row_mul = t->mask_row_mul; co.mask_row_add = t->mask_row_add;
  co.out = t->out; co.out_row_mul = t->out_row_mul; co.out_row_add = t->out_row_add; co.rec_prev = t->rec_prev; co.rec_new = t->rec_new;
  co.wb = t->wb; co.wb_ld = t->wb_ld; co.tp = t->tp; co.tp_ld = t->tp_ld; co.t2 = t->t2; co.t2_ld = t->t2_ld; co.w3 = t->w3; co.noise = t->noise;
  co.flat = t->flat; co.tp_out = t->tp_out; co.tp_out_ld = t->tp_out_ld;
  const int rc = sq_launch_crop(sq_crop_args(co), h->po, d, nslots, s);
  return sq_unit_done(h, who, rc, "launch refused", s);
}

extern "C" int sqair_slot_tail_test(SqairHandle* h, const SqairSlotTailTest* t, void* stream) {
  SQ_UNIT_ENTRY("sqair_slot_tail_test");
  if (t->B < 1) return sq_refuse(h, who, "B < 1");
  const Dims d = make_dims(h->cfg, t->B);
  const int nsp = d.nh / 2;
  const bool disc = t->is_disc != 0, wd = t->what_done != 0, rnn = t->out != nullptr;
  if (t->slot < 0 || t->slot >= d.N) return sq_refuse(h, who, "slot outside [0, N)");
#ifdef SQAIR_WIDE
  if (wd) return sq_refuse(h, who, "what_done: the wide library has no what fusion");
#endif
  if (!t->rec_new || !t->noise || !t->s1p || !t->flat || !t->packed) return sq_refuse(h, who, "a required pointer is NULL");
  if (!wd && !t->enc) return sq_refuse(h, who, "a required pointer is NULL (enc: read unless what_done)");
  if (!disc && (!t->rec_prev || (!wd && !t->hraw))) return sq_refuse(h, who, "propagation needs rec_prev and, unless what_done, hraw");
  if (t->s1p_ld < nsp || (t->s1h_out && t->s1h_ld < nsp) || (!wd && t->enc_ld < 2 * d.nw) || (!disc && !wd && t->h_ld < 5 * d.nw))
    return sq_refuse(h, who, "a pitch is smaller than the width");
  if (rnn) {
    const LayerId id = disc ? L_DISC_RNN : L_PROP_RNN;
    if (!sq_can_fuse_tail(h, id)) return sq_refuse(h, who, "the RNN block needs a configuration whose tail can ride in the next slot's layer");
    if (t->slot + 1 >= d.N) return sq_refuse(h, who, "the RNN block is the NEXT slot's layer: slot + 1 outside [0, N)");
    if (!t->hid || !t->add) return sq_refuse(h, who, "the RNN block needs hid and add");
    if (t->hid_ld < d.nh || t->add_ld < d.nh || t->out_ld < d.nh) return sq_refuse(h, who, "a pitch is smaller than the width");
    if ((reinterpret_cast<uintptr_t>(t->hid) & 15) != 0 || (t->hid_ld & 3) != 0) return sq_refuse(h, who, "hid is not a 16-byte aligned A operand");
  }
  hipStream_t s = (hipStream_t)stream;
  TailOperands io; memset(&io, 0, sizeof(io));
  io.is_disc = disc ? 1 : 0; io.slot = t->slot; io.what_done = wd ? 1 : 0; io.hraw = t->hraw; io.h_ld = t->h_ld; io.enc = t->enc; io.enc_ld = t->enc_ld;
  io.rec_prev = t->rec_prev; io.rec_new = t->rec_new; io.noise = t->noise; io.s1p = t->s1p; io.s1p_ld = t->s1p_ld;
  io.s1h_out = t->s1h_out; io.s1h_ld = t->s1h_ld;
  const TailArgs ta = sq_tail_args(h, io, t->flat, t->packed);
  const int rc = rnn ? sq_run_rnn_tail(h, ta, d, disc ? L_DISC_RNN : L_PROP_RNN, t->hid, t->hid_ld, t->add, t->add_ld, t->out, t->out_ld, t->packed, s)
                     : sq_launch_slot_tail(ta, d, s);
  return sq_unit_done(h, who, rc, "launch refused", s);
}

extern "C" int sqair_linear_what_test(SqairHandle* h, const SqairLinearWhatTest* t, void* stream) {
  SQ_UNIT_ENTRY("sqair_linear_what_test");
#ifdef SQAIR_WIDE
  return sq_refuse(h, who, "the wide library has no what fusion");
#else
  const SqairConfig& c = h->cfg;
  if (c.n_hidden != 128 && c.n_hidden != 256) return sq_refuse(h, who, "n_hidden is neither 128 nor 256");
  if (t->B < 1) return sq_refuse(h, who, "B < 1");
  if (t->mode != 0 && t->mode != 1) return sq_refuse(h, who, "mode is not 0 or 1");
  if (t->slot < 0 || t->slot >= c.n_steps_per_image) return sq_refuse(h, who, "slot outside [0, N)");
  if (!t->x || !t->noise || !t->rec_new || !t->packed) return sq_refuse(h, who, "a required pointer is NULL");
  if (t->mode == 1 && (!t->enc || !t->rec_prev)) return sq_refuse(h, who, "mode 1 needs enc and rec_prev");
  if (t->x_ld < c.n_hidden || (t->mode == 1 && t->enc_ld < 2 * c.n_what)) return sq_refuse(h, who, "a pitch is smaller than the width");
  if ((int64_t)t->B * c.k_particles > (int64_t)1 << 24) return sq_refuse(h, who, "more than 2^24 rows");
  hipStream_t s = (hipStream_t)stream;
  const int rc = sq_run_what(h, t->mode, t->x, t->x_ld, t->B * c.k_particles, t->slot, t->noise, t->enc, t->enc_ld, t->rec_prev, t->rec_new,
                             t->packed, s);
  return sq_unit_done(h, who, rc, "launch refused (x is not a 16-byte aligned A operand)", s);
#endif
}
