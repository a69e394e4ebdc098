// Unit-test and measurement entries of the dense family: one layer (or cell) described in the planner's vocabulary (sqair_pack.h),
// packed through the planners the product's plan goes through, and launched as the pass launches it.  Host code only.
#include <algorithm>

#include "sqair_internal.h"
#include "sqair_bwd.h"
#include "sqair_dx.h"

// A plan on the device, as sqair_pack_params lays a handle's out: weights behind their zero block, then the biases.
struct DevPack {
  float *w, *bias;   // offsets into them: PackedLayer::w_off / b_off; bias NULL when none was asked for
  float* rest;       // the entry's own `extra` floats of the scratch, 64-byte aligned
};
// scratch = [index tables int32: widx, then bidx_a | bidx_b in its place | zero block, packed weights | packed biases | extra].
// Weights from wflat, biases from bflat (NULL: zero biases); bias = false: no bias buffer at all.  -1 + "<who>: scratch too small".
static int dev_pack(SqairHandle* h, const char* who, const PackPlan& p, const float* wflat, const float* bflat, bool bias,
                    void* scratch, int64_t scratch_bytes, int64_t extra, hipStream_t s, DevPack* out) {
  const int64_t nw = p.packed_w() - 256, nb = bias ? p.packed_b() : 0;   // (2 nb <= nw: a tile has 16 biases and >= 256 weights)
  if (scratch_bytes < (2 * nw + 256 + nb + extra) * 4) return sq_no(h, std::string(who) + ": scratch too small");
  int* idx = (int*)scratch;
  out->w = (float*)scratch + nw;
  out->bias = bias ? out->w + 256 + nw : nullptr;
  out->rest = out->w + 256 + nw + nb;
  SQ_CHECK_HIP(hipMemcpyAsync(idx, p.widx.data() + 256, nw * 4, hipMemcpyHostToDevice, s));
  SQ_CHECK_HIP(hipMemsetAsync(out->w, 0, 256 * 4, s));
  SQ_CHECK_HIP(hipStreamSynchronize(s));
  sq_launch_pack(wflat, out->w + 256, idx, nw, s);
  if (nb && bflat) {
    SQ_CHECK_HIP(hipMemcpyAsync(idx, p.bidx_a.data(), nb * 4, hipMemcpyHostToDevice, s));
    SQ_CHECK_HIP(hipMemcpyAsync(idx + nb, p.bidx_b.data(), nb * 4, hipMemcpyHostToDevice, s));
    SQ_CHECK_HIP(hipStreamSynchronize(s));
    sq_launch_pack_bias(bflat, out->bias, idx, idx + nb, nb, s);
  } else if (nb) SQ_CHECK_HIP(hipMemsetAsync(out->bias, 0, nb * 4, s));
  return 0;
}
// what sq_run fills from the handle's packed buffer
static void bind(Lin& l, const DevPack& dp, const PackedLayer& L, int M, int N) {
  l.a.wp = dp.w + L.w_off; l.a.wzero = dp.w; l.a.bias = dp.bias + L.b_off; l.a.M = M; l.a.N = N;
}
// A-operand contract: rows padded to a multiple of 4 floats, finite
static int stage_rows(SqairHandle* h, float* dst, int ld, const float* x, int K, int M, int64_t tail, hipStream_t s) {
  SQ_CHECK_HIP(hipMemsetAsync(dst, 0, ((size_t)M * ld + tail) * 4, s));
  SQ_CHECK_HIP(hipMemcpy2DAsync(dst, (size_t)ld * 4, x, (size_t)K * 4, (size_t)K * 4, M, hipMemcpyDeviceToDevice, s));
  return 0;
}
// rows [0, K) of a row-major matrix at flat offset `w`, leading dimension ld
static PackSeg dense(int64_t w, int ld, int K) { return {w, ld, rm_range(0, K)}; }

// What the dense unit entry points time after their one checked launch: nothing (sqair_linear_test), the launch `reps` times back to
// back (sqair_debug_linear_time), or `nodes` launches, dependent or not, as one HIP graph replayed `reps` times (..._graph_time)
struct LinearTiming { int reps = 0, nodes = 0; bool dependent = false; };
static int sq_linear_test(SqairHandle* h, const float* x, const float* wmat, const float* b, float* y, int M, int Kdim, int Ndim, int act,
                          void* scratch, int64_t scratch_bytes, const LinearTiming& tm, float* us_out, void* stream) {
  if (!h || !x || !wmat || !y || !scratch) return -1;
  hipStream_t s = (hipStream_t)stream;
  PackPlan p;
  const PackedLayer L = sq_plan_layer(p, 0, {Kdim}, {{Ndim, 0, {dense(0, Ndim, Kdim)}, b ? 0 : -1}});
  const int kpad = (Kdim + 3) & ~3;
  DevPack dp;
  int rc = dev_pack(h, "sqair_linear_test", p, wmat, b, true, scratch, scratch_bytes, (int64_t)M * kpad, s, &dp);
  if (rc != 0) return rc;
  float* d_x = dp.rest;
  if ((rc = stage_rows(h, d_x, kpad, x, Kdim, M, 0, s)) != 0) return rc;
  Lin l;
  l.seg(d_x, kpad, Kdim).out(y, Ndim).act(act);
  bind(l, dp, L, M, Ndim);
  if (sq_launch_linear(l.a, L, s) != 0) { sq_set_error(h, "sqair_linear_test: A-operand contract violated"); return -5; }
  SQ_CHECK_HIP(hipGetLastError());
  SQ_CHECK_HIP(hipStreamSynchronize(s));
  if (tm.reps < 1) return 0;
  SqCapture cap(s);   // (the events of both timed modes; the graph of the second)
  float ms = 0.0f;
  if (tm.nodes > 0) {
    // `nodes` launches of this layer captured as ONE HIP graph -- the same launch over and over (no data dependence), or
    // (dependent) every launch reading what the previous one wrote -- and the graph replayed `reps` times between two HIP events:
    // time per graph NODE (kernel + the dependent-dispatch boundary), on whatever build of the library this is.  The figure
    // bench.py's timeline calls the SLOT of a dense launch, measured without the stamps.
    // dependent: every launch reads what the previous one wrote -- IN PLACE, input columns [0, K) and output columns [0, N) of
    // one buffer of pitch max(K, N) behind the other scratch (a race between the workgroups of a row tile: the values mean
    // nothing, tanh keeps them finite; what is timed is a launch whose operand comes out of the previous launch's stores)
    Lin l2;
    if (tm.dependent) {
      const int ldz = (std::max(kpad, Ndim) + 3) & ~3;
      float* d_z = d_x + (size_t)M * kpad;
      if (scratch_bytes < (d_z - (float*)scratch + (int64_t)M * ldz + 16) * 4) return sq_no(h, "sqair_debug_linear_graph_time: scratch too small");
      if ((rc = stage_rows(h, d_z, ldz, x, Kdim, M, 16, s)) != 0) return rc;
      l2.seg(d_z, ldz, Kdim).out(d_z, ldz).act(act);
      bind(l2, dp, L, M, Ndim);
    }
    SQ_CHECK_HIP(cap.begin());
    for (int i = 0; i < tm.nodes; ++i)   // (a failed launch: cap ends the capture on the way out)
      if (sq_launch_linear(tm.dependent ? l2.a : l.a, L, s) != 0) { sq_set_error(h, "sqair_debug_linear_graph_time: A-operand contract violated inside the capture"); return -5; }
    SQ_CHECK_HIP(cap.end());
    SQ_CHECK_HIP(cap.instantiate());
    SQ_CHECK_HIP(cap.events());
    for (int i = 0; i < 2; ++i) SQ_CHECK_HIP(hipGraphLaunch(cap.exec, s));
    (void)hipEventRecord(cap.ev[0], s);
    for (int i = 0; i < tm.reps; ++i) SQ_CHECK_HIP(hipGraphLaunch(cap.exec, s));
  } else {  // the same launch `reps` times back to back between two events
    SQ_CHECK_HIP(cap.events());
    for (int i = 0; i < 3; ++i) sq_launch_linear(l.a, L, s);
    (void)hipEventRecord(cap.ev[0], s);
    for (int i = 0; i < tm.reps; ++i) sq_launch_linear(l.a, L, s);
  }
  (void)hipEventRecord(cap.ev[1], s);
  SQ_CHECK_HIP(hipStreamSynchronize(s));
  SQ_CHECK_HIP(hipEventElapsedTime(&ms, cap.ev[0], cap.ev[1]));
  *us_out = ms * 1e3f / ((float)tm.reps * (float)std::max(tm.nodes, 1));
  return 0;
}
extern "C" int sqair_linear_test(SqairHandle* h, const float* x, const float* wmat, const float* b, float* y, int M,
                                 int Kdim, int Ndim, int act, void* scratch, int64_t scratch_bytes, void* stream) {
  return sq_linear_test(h, x, wmat, b, y, M, Kdim, Ndim, act, scratch, scratch_bytes, LinearTiming{}, nullptr, stream);
}
// measurement helper (tools/time_linear.py): average time of one dense launch of the given shape, launches back to back
extern "C" int sqair_debug_linear_time(SqairHandle* h, const float* x, const float* wmat, const float* b, float* y, int M, int Kdim,
                                       int Ndim, int act, void* scratch, int64_t scratch_bytes, int reps, float* us_out, void* stream) {
  if (!h || !us_out || reps < 1) return -1;
  return sq_linear_test(h, x, wmat, b, y, M, Kdim, Ndim, act, scratch, scratch_bytes, LinearTiming{reps, 0, false}, us_out, stream);
}

// measurement helper (tools/dense_graph_time.py): the dense launches of the passes issued between (on = 1) and the read-out.
// entry i -> {layer id (-1 - id: the VanillaRNN layer with the slot tail fused in front), rows, K padded, N}; returns the count.
extern "C" int sqair_debug_dense_log(SqairHandle* h, int on) {
  if (!h) return -1;
  if (on) h->dense_log.clear();
  h->dense_log_on = on != 0;
  return (int)(h->dense_log.size() / 4);
}
extern "C" int sqair_debug_dense_log_entry(const SqairHandle* h, int i, int* out4) {
  if (!h || !out4 || i < 0 || (size_t)i * 4 + 3 >= h->dense_log.size()) return -1;
  for (int q = 0; q < 4; ++q) out4[q] = h->dense_log[(size_t)i * 4 + q];
  return 0;
}
// measurement helper (tools/dense_graph_time.py): time per NODE of a HIP graph of `nodes` launches of one dense layer -- the same
// launch again and again, or (dependent != 0) each reading what the previous one wrote -- replayed `replays` times between HIP events
extern "C" int sqair_debug_linear_graph_time(SqairHandle* h, const float* x, const float* wmat, const float* b, float* y, int M, int Kdim,
                                             int Ndim, int act, void* scratch, int64_t scratch_bytes, int nodes, int replays,
                                             int dependent, float* us_out, void* stream) {
  if (!h || !us_out || nodes < 1 || replays < 1) return -1;
  return sq_linear_test(h, x, wmat, b, y, M, Kdim, Ndim, act, scratch, scratch_bytes, LinearTiming{replays, nodes, dependent != 0},
                        us_out, stream);
}

// snt.GRU step through the two launches the pass uses: gates [z | r | candidate's input part] over [x | h], then the candidate's
// recurrent matrix on r * h
extern "C" int sqair_gru_test(SqairHandle* h, const float* x, const float* hstate, const float* gru_flat, float* h_out,
                              int M, int Kx, void* scratch, int64_t scratch_bytes, void* stream) {
  if (!h || !x || !hstate || !gru_flat || !h_out || !scratch) return -1;
  hipStream_t s = (hipStream_t)stream;
  const int nh = h->cfg.n_hidden;
  // gru_flat: for g in (z, r, h): w_g [Kx,nh], u_g [nh,nh], b_g [nh]  (the order add_gru() lays them out)
  const int64_t u0 = (int64_t)Kx * nh, b0 = u0 + (int64_t)nh * nh, gs = b0 + nh;
  PackPlan p;
  std::vector<PackBlock> gates;
  for (int g = 0; g < 3; ++g) gates.push_back({nh, 0, {dense(g * gs, nh, Kx), g < 2 ? dense(g * gs + u0, nh, nh) : PackSeg()}, g * gs + b0});
  const PackedLayer L1 = sq_plan_layer(p, 0, {Kx, nh}, gates);
  const PackedLayer L2 = sq_plan_layer(p, 1, {nh}, {{nh, 0, {dense(2 * gs + u0, nh, nh)}}});
  const int kpad = (Kx + 3) & ~3;
  DevPack dp;
  int rc = dev_pack(h, "sqair_gru_test", p, gru_flat, gru_flat, true, scratch, scratch_bytes, (int64_t)M * (3 * nh + kpad), s, &dp);
  if (rc != 0) return rc;
  float* d_z = dp.rest;
  float* d_rh = d_z + (int64_t)M * nh;
  float* d_xh = d_rh + (int64_t)M * nh;
  float* d_x = d_xh + (int64_t)M * nh;
  if ((rc = stage_rows(h, d_x, kpad, x, Kx, M, 0, s)) != 0) return rc;
  Lin g1;
  g1.seg(d_x, kpad, Kx).seg(hstate, nh, nh).out(d_z, nh).gru1(hstate, nh, d_rh, nh, d_xh, nh, nh);
  bind(g1, dp, L1, M, 3 * nh);
  if (sq_launch_linear(g1.a, L1, s) != 0) { sq_set_error(h, "sqair_gru_test: A-operand contract violated"); return -5; }
  Lin g2;
  g2.seg(d_rh, nh, nh).add(d_xh, nh, nh).out(h_out, nh).gru2(hstate, nh, d_z, nh, nh);
  bind(g2, dp, L2, M, nh);
  sq_launch_linear(g2.a, L2, s);
  SQ_CHECK_HIP(hipGetLastError());
  SQ_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// snt.LSTM step through the launches the forward pass uses: one gate GEMM over [x | h] + the element-wise cell kernel
extern "C" int sqair_lstm_test(SqairHandle* h, const float* x, const float* hstate, const float* cstate, const float* lstm_flat,
                               float* state_out, int M, int Kx, void* scratch, int64_t scratch_bytes, void* stream) {
  if (!h || !x || !hstate || !cstate || !lstm_flat || !state_out || !scratch) return -1;
  hipStream_t s = (hipStream_t)stream;
  const int nh = h->cfg.n_hidden;
  // lstm_flat: w_gates [(Kx + nh), 4 nh] then b_gates [4 nh] (the order of the reference's LSTM variables)
  PackPlan p;
  const PackedLayer L = sq_plan_layer(p, 0, {Kx, nh}, {{4 * nh, 0, {dense(0, 4 * nh, Kx), dense((int64_t)Kx * 4 * nh, 4 * nh, nh)},
                                                       (int64_t)(Kx + nh) * 4 * nh}});
  const int kpad = (Kx + 3) & ~3;
  DevPack dp;
  int rc = dev_pack(h, "sqair_lstm_test", p, lstm_flat, lstm_flat, true, scratch, scratch_bytes, (int64_t)M * (kpad + 4 * nh), s, &dp);
  if (rc != 0) return rc;
  float* d_x = dp.rest;
  float* d_g = d_x + (int64_t)M * kpad;
  if ((rc = stage_rows(h, d_x, kpad, x, Kx, M, 0, s)) != 0) return rc;
  Lin g;
  g.seg(d_x, kpad, Kx).seg(hstate, nh, nh).out(d_g, 4 * nh);
  bind(g, dp, L, M, 4 * nh);
  if (sq_launch_linear(g.a, L, s) != 0) { sq_set_error(h, "sqair_lstm_test: A-operand contract violated"); return -5; }
  sq_launch_lstm_cell(d_g, 4 * nh, cstate, nh, state_out, 2 * nh, M, nh, s);
  SQ_CHECK_HIP(hipGetLastError());
  SQ_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// adjoint of the element-wise LSTM cell: gates [M, 4 nh] (pre-activations i, j, f, o), c_prev, d h', d c' -> d gates, d c_prev
extern "C" int sqair_lstm_cell_bwd_test(SqairHandle* h, const float* gates, const float* c_prev, const float* d_h, const float* d_c,
                                        float* d_gates, float* d_cprev, int M, void* stream) {
  if (!h || !gates || !c_prev || !d_h || !d_c || !d_gates || !d_cprev) return -1;
  hipStream_t s = (hipStream_t)stream;
  const int nh = h->cfg.n_hidden;
  sq_launch_lstm_cell_bwd(gates, 4 * nh, c_prev, nh, d_h, nh, d_c, nh, d_gates, 4 * nh, d_cprev, nh, M, nh, s);
  SQ_CHECK_HIP(hipGetLastError());
  SQ_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// the transposed pack (dX = dY W^T) of a dense forward matrix [Kdim, Ndim] at flat offset 0, as build_plan_T makes a layer's
static PackedLayer plan_dense_T(PackPlan& t, int Kdim, int Ndim) {
  PackPlan f;
  return sq_plan_layer_T(t, f, sq_plan_layer(f, 0, {Kdim}, {{Ndim, 0, {dense(0, Ndim, Kdim)}}}));
}

// ------------------------------------------------------------------------------------------------
// dense-layer backward through the kernels of the training step (unit-test entry): y = act(x W + b) was computed forward;
// given dL/dy returns dL/dx (k_linear on the transposed pack, the route of the decoder layers), dL/dW and dL/db (routed as
// sqair_backward routes a block: the grouped kernel, or k_wgrad2 on its own for operands the grouped kernel declines).
// ------------------------------------------------------------------------------------------------
extern "C" int sqair_linear_bwd_test(SqairHandle* h, const float* x, const float* wmat, const float* y, const float* dy,
                                     float* dx, float* dw, float* db, int M, int Kdim, int Ndim, int act, void* scratch,
                                     int64_t scratch_bytes, void* stream) {
  if (!h || !x || !wmat || !y || !dy || !dx || !dw || !db || !scratch) return -1;
  hipStream_t s = (hipStream_t)stream;
  PackPlan p;
  const PackedLayer L = plan_dense_T(p, Kdim, Ndim);   // K' = Ndim inputs (dpre), N' = Kdim outputs (dx)
  const int npad = (Ndim + 3) & ~3;
  DevPack dp;
  const int rc = dev_pack(h, "sqair_linear_bwd_test", p, wmat, nullptr, true, scratch, scratch_bytes, (int64_t)M * npad, s, &dp);
  if (rc != 0) return rc;
  float* d_dpre = dp.rest;          // [M][npad], 16-byte aligned rows
  SQ_CHECK_HIP(hipMemsetAsync(d_dpre, 0, (size_t)M * npad * 4, s));
  SQ_CHECK_HIP(hipMemsetAsync(dw, 0, (size_t)Kdim * Ndim * 4, s));   // (the weight-gradient kernels accumulate with atomics)
  SQ_CHECK_HIP(hipMemsetAsync(db, 0, (size_t)Ndim * 4, s));
  sq_launch_dact2(dy, Ndim, y, Ndim, d_dpre, npad, M, Ndim, act, act, 1 << 30, 0, s);
  WgradBatch wbatch;
  if (!wbatch.add(x, Kdim, d_dpre, npad, dw, Ndim, M, Kdim, Ndim, nullptr, nullptr, db, nullptr))
    sq_launch_wgrad_acc(x, Kdim, d_dpre, npad, dw, Ndim, M, Kdim, Ndim, s, nullptr, nullptr, db, nullptr);
  if (wbatch.flush(s) != 0) { sq_set_error(h, "sqair_linear_bwd_test: the grouped weight-gradient launch failed"); return -2; }
  Lin l;
  l.seg(d_dpre, npad, Ndim).out(dx, Kdim).act(ACT_NONE);
  bind(l, dp, L, M, Kdim);
  if (sq_launch_linear(l.a, L, s) != 0) { sq_set_error(h, "sqair_linear_bwd_test: A-operand contract violated"); return -5; }
  SQ_CHECK_HIP(hipGetLastError());
  SQ_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// ------------------------------------------------------------------------------------------------
// The dense family's operand contract, one launch (unit-test entry): everything a Lin can say -- segments with pitches, widths and
// row divisors, a broadcast segment, the addend, the split activation, both scales, a padded output pitch -- goes to
// sq_launch_linear as the caller gave it.  Only the weights are packed here: nseg segments of the one matrix w.
// ------------------------------------------------------------------------------------------------
extern "C" int sqair_linear_contract_test(SqairHandle* h, const SqairDenseContract* c, void* stream) {
  if (!h || !c || !c->w || !c->out || !c->scratch || c->nseg < 1 || c->nseg > 4 || c->M < 1 || c->N < 1 || c->out_ld < c->N) return -1;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> seg_width;
  PackBlock blk{c->N, 0, {}, c->b ? 0 : -1};
  int k0 = 0;   // first row of the segment in w
  for (int i = 0; i < c->nseg; ++i) {
    if (c->seg[i].width < 1) { sq_set_error(h, "sqair_linear_contract_test: a segment without inputs"); return -1; }
    seg_width.push_back(c->seg[i].width);
    blk.seg.push_back(dense((int64_t)k0 * c->N, c->N, c->seg[i].width));
    k0 += c->seg[i].width;
  }
  PackPlan p;
  const PackedLayer L = sq_plan_layer(p, 0, seg_width, {blk});
  DevPack dp;
  int rc = dev_pack(h, "sqair_linear_contract_test", p, c->w, c->b, true, c->scratch, c->scratch_bytes, 0, s, &dp);
  if (rc != 0) return rc;
  Lin l;
  for (int i = 0; i < c->nseg; ++i) l.seg(c->seg[i].p, c->seg[i].ld, c->seg[i].width, c->seg[i].rdiv);
  if (c->add) l.add(c->add, c->add_ld, c->add_n, c->add_rdiv);
  l.out(c->out, c->out_ld).act2(c->act_a, c->act_b, c->act_split);
  l.a.scale = c->scale; l.a.scale_ptr = c->scale_ptr;
  bind(l, dp, L, c->M, c->N);
  rc = sq_launch_linear(l.a, L, s);
  if (rc != 0) { sq_set_error(h, "sqair_linear_contract_test: A-operand contract violated"); return rc; }
  SQ_CHECK_HIP(hipGetLastError());
  SQ_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// The routed dX GEMM, one launch (unit-test entry): dpre, the ranges and the GRU block reach sq_launch_linear_dx as given; the
// forward matrix w [Kdim, width] is packed transposed, as sqair_linear_bwd_test packs it.
extern "C" int sqair_linear_dx_test(SqairHandle* h, const SqairDxTest* t, void* stream) {
  if (!h || !t || !t->dpre || !t->w || !t->scratch || t->M < 1 || t->width < 1 || t->Kdim < 1) return -1;
  hipStream_t s = (hipStream_t)stream;
  PackPlan p;
  const PackedLayer L = plan_dense_T(p, t->Kdim, t->width);
  DevPack dp;
  int rc = dev_pack(h, "sqair_linear_dx_test", p, t->w, nullptr, false, t->scratch, t->scratch_bytes, 0, s, &dp);
  if (rc != 0) return rc;
  DxArgs a; memset(&a, 0, sizeof(a));
  a.dpre = t->dpre; a.ld = t->ld; a.width = t->width; a.wp = dp.w + L.w_off; a.wzero = dp.w; a.scale_ptr = t->scale_ptr; a.M = t->M;
  a.nranges = t->nranges;
  for (int i = 0; i < 3 && i < t->nranges; ++i) {
    const SqairDxRange& r = t->r[i];
    a.r[i] = DxRange{r.n0, r.n1, r.dst, r.dst_ld, r.dst2, r.dst2_ld, r.add, r.add_ld, r.saved, r.saved_ld, r.act_a, r.act_b, r.act_split};
  }
  const SqairDxGru& g = t->gru;
  a.gru = DxGru{g.mode, g.g0, g.g0_ld, g.g1, g.g1_ld, g.hprev, g.h_ld, g.dpre1, g.dp_ld, g.d_h, g.dh_ld, g.acc_dh, g.dup, g.dup_ld,
                g.dup_h_off, g.nh};
  rc = sq_launch_linear_dx(a, L.kc, L.nt, s);
  if (rc == -5) { sq_set_error(h, "sqair_linear_dx_test: operand contract violated (alignment, pitch, range start or range count)"); return rc; }
  if (rc == -6) { sq_set_error(h, "sqair_linear_dx_test: the GRU epilogue takes one range [0, nh) without a saved output, at most 16 K chunks on the product build"); return rc; }
  if (rc != 0) { sq_set_error(h, "sqair_linear_dx_test: launch refused"); return rc; }
  SQ_CHECK_HIP(hipGetLastError());
  SQ_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// the routes the two dense launchers took (sqair_common.h: DenseRoute, in the order sqair_hip.h documents)
extern "C" int sqair_debug_dense_routes(int64_t* out, int n) {
  static_assert(DR_COUNT == SQAIR_DENSE_ROUTES, "sqair_hip.h documents every route");
  if (!out || n < 0) return -1;
  for (int i = 0; i < n && i < DR_COUNT; ++i) out[i] = (int64_t)sq_dense_route_hits(i);
  return DR_COUNT;
}
