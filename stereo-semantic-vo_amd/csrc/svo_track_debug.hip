// svo_track_debug.hip - the tracker's counters, sticky flags and parity / timing probes (include/svo.h: svo_track_overflowed,
// svo_track_epnp_fallbacks, svo_debug_track_*, svo_debug_stream_*), and svo_sync's look at the timeout flag.
#include <string>
#include <vector>

#include "svo_track_priv.h"

// One int32 counter of every sequence's TrackState (`offset`: offsetof(TrackState, field)) in one strided copy; waits for the stream
static int track_read_counter(svo_ctx* ctx, size_t offset, std::vector<int32_t>* v) {
  v->assign((size_t)ctx->n_seq, 0);
  SVO_HIP(ctx, hipMemcpy2DAsync(v->data(), sizeof(int32_t), static_cast<const uint8_t*>(ctx->d_track) + offset, sizeof(TrackState), sizeof(int32_t),
                                (size_t)ctx->n_seq, hipMemcpyDeviceToHost, ctx->stream));
  SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVO_OK;
}

// Parity probe: what the dense depth sources handed the tail for frame `frame` of the last call (the context's own arrays)
extern "C" int svo_debug_track_depths(svo_ctx* ctx, int frame, svo_kp* kp, float* depth, int32_t* n) {
  if (!ctx || !kp || !depth || !n || frame < 0 || frame >= ctx->max_batch) return SVO_E_INVALID;
  if (ctx->opt_depth_source == 0) { ctx->last_error = "svo_debug_track_depths: depth_source must be 1, 2 or 3"; return SVO_E_INVALID; }
  hipSetDevice(ctx->device);
  SVO_HIP(ctx, hipDeviceSynchronize());
  const size_t K = ctx->max_kp;
  SVO_HIP(ctx, hipMemcpy(n, ctx->d_nkp + frame, sizeof(int32_t), hipMemcpyDeviceToHost));
  SVO_HIP(ctx, hipMemcpy(kp, ctx->d_kp + frame * K, K * sizeof(svo_kp), hipMemcpyDeviceToHost));
  SVO_HIP(ctx, hipMemcpy(depth, ctx->d_depth + frame * K, K * sizeof(float), hipMemcpyDeviceToHost));
  return SVO_OK;
}

// svo_sync's look at the sticky flags of the tracker's sequences (the stream is idle here): bit 4 = a wait inside the pose chain
// ran into its bound (k_tp_tail_ord's frame part waiting for the samples of its own launch, or a kernel polling for a hand-over
// record with "pose_flag").  The frame concerned was treated as a PnP failure (record: n_pnp_inliers = -1) - nothing stale was
// consumed -; the context falls back to the two-launch pose chain, whose kernels never wait for each other, and says so (once
// per svo_track_reset / svo_track_multi_reset, naming the sequences concerned when there are several).
int svo_track_check_timeout(svo_ctx* ctx) {
  if (!ctx->d_track || ctx->timeout_reported) return SVO_OK;
  const int n = ctx->n_seq;
  std::vector<int32_t> v;
  { const int rc = track_read_counter(ctx, offsetof(TrackState, overflow), &v); if (rc) return rc; }
  std::string seqs;
  for (int q = 0; q < n; ++q)
    if (v[(size_t)q] & 4) seqs += (seqs.empty() ? "" : ", ") + std::to_string(q);
  if (seqs.empty()) return SVO_OK;
  ctx->timeout_reported = true;
  ctx->opt_tail_fused = 0;
  ctx->opt_pose_flag = 0;
  ctx->last_error = std::string("tracker: a wait inside the pose chain timed out (sticky flag 4") +
                    (n > 1 ? "; sequence(s) " + seqs + " of " + std::to_string(n) : std::string()) +
                    "): the frame was treated as a PnP failure (n_pnp_inliers = -1); "
                    "the context now runs the two-launch pose chain (tail_fused = 0, pose_flag = 0)";
  return SVO_E_TIMEOUT;
}

// Sticky flag of the tracker (0 = fine), a bit set (device side: atomicOr), OR-ed over the sequences.  1: a frame wanted more than
// 4096 live map points or a map point outlived the position table (2^20 ids) - results after that are not the reference's.
// 4: a bounded wait inside the pose chain timed out (above).
extern "C" int svo_track_overflowed(svo_ctx* ctx, int32_t* flag) {
  if (!ctx || !flag || !ctx->d_track) return SVO_E_INVALID;
  std::vector<int32_t> v;
  { const int rc = track_read_counter(ctx, offsetof(TrackState, overflow), &v); if (rc) return rc; }
  int32_t any = 0;
  for (int32_t f : v) any |= f;
  *flag = any;
  return SVO_OK;
}

// How the index chain's stream was chosen (svo_stream_burst, or track_index_stream with SVO_POOLED_QUEUES=1): out[0] = candidates
// tried (0: probe switched off), out[1] = "two chains together / one alone" on the pose and the index stream in per cent
// (~105 side by side, ~200: the two chains of the tail take turns instead of overlapping).
extern "C" int svo_debug_stream_probe(svo_ctx* ctx, int32_t out[2]) {
  if (!ctx || !out) return SVO_E_INVALID;
  out[0] = ctx->idx_probe_attempts; out[1] = ctx->idx_probe_spins;
  return SVO_OK;
}

// Do the front end's / the dense stage's queued grids hold the tail's two streams up?  (include/svo.h; svo_probe_block_percent)
extern "C" int svo_debug_stream_pipes(svo_ctx* ctx, int32_t out[4]) {
  if (!ctx || !out) return SVO_E_INVALID;
  hipSetDevice(ctx->device);
  { const int rcq = svo_track_quiesce(ctx, true); if (rcq) return rcq; }
  hipStream_t fill[2] = {ctx->stream_fe_batch, ctx->stream_dense}, tail[2] = {ctx->stream, ctx->stream_idx};
  for (int f = 0; f < 2; ++f)
    for (int t = 0; t < 2; ++t)
      out[2 * f + t] = fill[f] && tail[t] && fill[f] != tail[t] ? svo_probe_block_percent(fill[f], tail[t]) : -1;
  return SVO_OK;
}

// How many RANSAC samples of the order-preserving EPnP (epnp_exact = 2) were handed to its sequential fallback since
// svo_track_reset (a zero or repeated singular value, 25 Jacobi sweeps): same results, ~10x the time of the frame concerned.
extern "C" int svo_track_epnp_fallbacks(svo_ctx* ctx, int64_t* count) {
  if (!ctx || !count || !ctx->d_track) return SVO_E_INVALID;
  std::vector<int32_t> v;
  { const int rc = track_read_counter(ctx, offsetof(TrackState, epnp_fallbacks), &v); if (rc) return rc; }
  int64_t total = 0;
  for (int32_t c : v) total += c;
  *count = total;
  return SVO_OK;
}

extern "C" int svo_debug_track_matches(svo_ctx* ctx, int32_t* cur_mp) {
  if (!ctx || !cur_mp || !ctx->d_track) return SVO_E_INVALID;
  TrackState* st = reinterpret_cast<TrackState*>(ctx->d_track);
  SVO_HIP(ctx, hipMemcpyAsync(cur_mp, st->dbg_cur_mp, sizeof(int32_t) * ctx->max_kp,
                              hipMemcpyDeviceToHost, ctx->stream));
  SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVO_OK;
}

extern "C" int svo_debug_track_gate(svo_ctx* ctx, double F[9], int32_t* n_vetoed) {
  if (!ctx || !ctx->d_track) return SVO_E_INVALID;
  TrackState* st = reinterpret_cast<TrackState*>(ctx->d_track);
  if (F) SVO_HIP(ctx, hipMemcpyAsync(F, st->F, 72, hipMemcpyDeviceToHost, ctx->stream));
  if (n_vetoed) SVO_HIP(ctx, hipMemcpyAsync(n_vetoed, &st->n_vetoed, 4, hipMemcpyDeviceToHost, ctx->stream));
  SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVO_OK;
}

// Parity probe: map-point identities, RANSAC outcome and PnP pose of n frames of the last batched call (work slots first ..).
extern "C" int svo_debug_track_frames(svo_ctx* ctx, int first, int n, svo_track_debug* out) {
  if (!ctx || !out || !ctx->d_work || first < 0 || n < 1 || first + n > ctx->work_cap) return SVO_E_INVALID;
  hipSetDevice(ctx->device);
  SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<TrackWork> w((size_t)n);
  SVO_HIP(ctx, svo_memcpy_sync(ctx, w.data(), reinterpret_cast<TrackWork*>(ctx->d_work) + (size_t)ctx->work_last_half * ctx->work_cap + first,
                         sizeof(TrackWork) * (size_t)n, hipMemcpyDeviceToHost));
  for (int f = 0; f < n; ++f) {
    const TrackWork& q = w[f];
    svo_track_debug& o = out[f];
    for (int j = 0; j < TRK_MAXKP; ++j) { o.match_gid[j] = -1; o.new_gid[j] = q.new_gid[j]; }
    for (int e = 0; e < q.n_edges && e < TRK_MAXKP; ++e) o.match_gid[q.edge_kp[e]] = q.edge_gid[e];
    o.frame_id = q.frame_id;
    o.pnp_best = q.pnp_best; o.pnp_iterations = q.pnp_iterations; o.pnp_inliers = q.pnp_inliers; o.pnp_ok = q.pnp_ok;
    o.active_rows[0] = q.diag[0] & 0xffff; o.active_rows[1] = q.diag[1] & 0xffff;
    o.rounds[0] = q.diag[0] >> 16; o.rounds[1] = q.diag[1] >> 16;
    o.resolve_us = (int32_t)((q.rt[1] - q.rt[0]) / 100);   // s_memrealtime: 100 MHz
    for (int i = 0; i < 6; ++i) o.rt[i] = q.rt[i];
    memcpy(o.T_pnp, q.T_pnp, sizeof o.T_pnp);
  }
  return SVO_OK;
}

// Diagnostics: s_memtime stamps (shader clock) of k_ti_resolve's phases for work slot `slot` of the last call:
// begin, pass 1, pass 2, frame end, done.
extern "C" int svo_debug_track_stamps(svo_ctx* ctx, int slot, int64_t ts[8]) {
  if (!ctx || !ts || !ctx->d_work || slot < 0 || slot >= ctx->work_cap) return SVO_E_INVALID;
  SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  TrackWork* w = reinterpret_cast<TrackWork*>(ctx->d_work) + (size_t)ctx->work_last_half * ctx->work_cap + slot;
  SVO_HIP(ctx, svo_memcpy_sync(ctx, ts, w->ts, sizeof(long long) * 8, hipMemcpyDeviceToHost));
  return SVO_OK;
}

// Diagnostics: s_memrealtime stamps (100 MHz) of work slot `slot` of the last batched call: k_ti_resolve start / end,
// k_tp_hyp start, k_tp_frame end - where the two chains of the tail wait for each other (tools/chain_times.py).
extern "C" int svo_debug_track_realtime(svo_ctx* ctx, int slot, int64_t rt[4]) {
  if (!ctx || !rt || !ctx->d_work || slot < 0 || slot >= ctx->work_cap) return SVO_E_INVALID;
  SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  TrackWork* w = reinterpret_cast<TrackWork*>(ctx->d_work) + (size_t)ctx->work_last_half * ctx->work_cap + slot;
  SVO_HIP(ctx, svo_memcpy_sync(ctx, rt, w->rt, sizeof(long long) * 4, hipMemcpyDeviceToHost));   // (the first four stamps)
  return SVO_OK;
}

// Parity probe: cv::solvePnPRansac's outcome for the frame just tracked (winning sample, consensus, samples visited)
// and the pose it handed to PoseOptimization (before the CV_32F rounding), row-major 4x4.
extern "C" int svo_debug_track_pnp(svo_ctx* ctx, svo_pnp_stats* stats, double T_pnp[16]) {
  if (!ctx || !ctx->d_track) return SVO_E_INVALID;
  TrackState* st = reinterpret_cast<TrackState*>(ctx->d_track);
  SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (stats) SVO_HIP(ctx, svo_memcpy_sync(ctx, stats, &st->pnp, sizeof *stats, hipMemcpyDeviceToHost));
  if (T_pnp) {
    PnpHyp h;
    svo_pnp_stats s;
    SVO_HIP(ctx, svo_memcpy_sync(ctx, &s, &st->pnp, sizeof s, hipMemcpyDeviceToHost));
    if (s.best_hypothesis < 0) return SVO_E_INVALID;
    SVO_HIP(ctx, svo_memcpy_sync(ctx, &h, &st->hyp[s.best_hypothesis], sizeof h, hipMemcpyDeviceToHost));
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T_pnp[4 * r + c] = h.R[3 * r + c]; T_pnp[4 * r + 3] = h.t[r]; }
    T_pnp[12] = 0; T_pnp[13] = 0; T_pnp[14] = 0; T_pnp[15] = 1;
  }
  return SVO_OK;
}

// Diagnostics: s_memtime stamps of the pose chain for the frame just tracked: [0] k_tp_hyp start, [1] correspondences
// gathered, [2] EPnP start, [3] EPnP done, [4] consensus counted; [8] k_tp_frame start, [9] RANSAC rule applied,
// [10] PoseOptimization done, [11] record written.
extern "C" int svo_debug_track_pose_stamps(svo_ctx* ctx, int64_t ts[16]) {
  if (!ctx || !ts || !ctx->d_track) return SVO_E_INVALID;
  SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  TrackState* st = reinterpret_cast<TrackState*>(ctx->d_track);
  SVO_HIP(ctx, svo_memcpy_sync(ctx, ts, st->pose_ts, sizeof(long long) * 16, hipMemcpyDeviceToHost));
  return SVO_OK;
}
