// svo_track_entries.hip - the tracker's entry points on one context: svo_track_frame, the batched entries (svo_track_batch_dev and
// what the host-fed and colour entries hand to svo_track_batch_fed), the many-sequence step and svo_track_tail_dev - each the front
// end of its frames (sparse stereo or a dense depth source), then tail_enqueue (svo_track.hip).
#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "svo_track_priv.h"

// ---- a call's attachments ------------------------------------------------------------------------------------------------------
// Every entry that delivers svo_track_map_out's records or runs the dynamic-keypoint loop brackets its work with ONE of these: the
// one-shot attachments are armed for the call and disarmed when it ends, however it ends.
namespace {
struct TrackCall {
  svo_ctx* ctx = nullptr;
  bool direct = false;
  // gray / bgr (may be null): the call's left images, rows gray_stride / bgr_stride bytes apart - the loop takes the ones it tracks
  // on; host: the attachments' arrays are host memory; direct_: the entry synchronises before it returns
  int begin(svo_ctx* c, const char* who, const uint8_t* gray, int gray_stride, const uint8_t* bgr, int bgr_stride, bool host, bool direct_) {
    const int rc = map_begin(c, host);
    if (rc) return rc;
    ctx = c; direct = direct_;
    if (!dyn_active(c)) return SVO_OK;
    const bool colour = dyn_colour(c);
    if (colour && !bgr) return dyn_colour_needs_bgr(c, who);
    return dyn_begin(c, colour ? bgr : gray, colour ? bgr_stride : gray_stride, host, direct);
  }
  // rc: the entry's outcome so far.  A direct entry's host arrays are complete when it returns (svo_track_priv.h, HostStage)
  int end(int rc) {
    if (!ctx) return rc;
    map_end(ctx);
    if (dyn_active(ctx)) dyn_end(ctx);
    if (direct) { const int rcf = svo_track_host_out_flush(ctx); if (rc == SVO_OK) rc = rcf; }
    ctx = nullptr;
    return rc;
  }
  ~TrackCall() { end(SVO_OK); }
};
}  // namespace

// the staged host outputs of both attachments (HostStage, svo_track_priv.h): all of them ...
int svo_track_host_out_flush(svo_ctx* ctx) {
  const int rc = stage_hand_over(ctx, dyn_host_stage(ctx), 0);
  return rc ? rc : stage_hand_over(ctx, map_host_stage(ctx), 0);
}
// ... and, when a host-fed call begins, those that are two such calls old
int svo_track_host_out_call_begins(svo_ctx* ctx) {
  for (HostStage* S : {dyn_host_stage(ctx), map_host_stage(ctx)}) {
    if (!S) continue;
    ++S->calls;
    const int rc = stage_hand_over(ctx, S, 2);
    if (rc) return rc;
  }
  return SVO_OK;
}

// colour entries: the gray of pairs f0 .. f0 + b - 1 of the call is written here, on the stream that reads it first - `first`: once
// the readers of the gray staging in the previous colour call (and the dynamic-keypoint loop's copy of it) are done with it
static int bgr_to_gray(svo_ctx* ctx, hipStream_t s, const SvoBgrSrc* bgr, const uint8_t* d_grayL, const uint8_t* d_grayR, int stride, int f0,
                       int b, bool first) {
  if (!bgr || !bgr->convert) return SVO_OK;
  if (first) {
    for (int k = 0; k < bgr->n_wait; ++k) SVO_HIP(ctx, hipStreamWaitEvent(s, bgr->wait[k], 0));
    const int rc = dyn_wait_gray_read(ctx, s);
    if (rc) return rc;
  }
  const size_t gray_img = (size_t)ctx->g.H * stride, bgr_img = (size_t)ctx->g.H * bgr->stride;
  svo_launch_bgr2gray(s, bgr->L + f0 * bgr_img, bgr->stride, bgr_img, const_cast<uint8_t*>(d_grayL) + f0 * gray_img, stride, gray_img,
                      ctx->g.W, ctx->g.H, b);
  svo_launch_bgr2gray(s, bgr->R + f0 * bgr_img, bgr->stride, bgr_img, const_cast<uint8_t*>(d_grayR) + f0 * gray_img, stride, gray_img,
                      ctx->g.W, ctx->g.H, b);
  return SVO_OK;
}
static int tb_done_events(svo_ctx* ctx) {
  for (int q = 0; q < 2; ++q)
    if (!ctx->tb_done[q]) SVO_HIP(ctx, hipEventCreateWithFlags(&ctx->tb_done[q], hipEventDisableTiming));
  return SVO_OK;
}

// The batched tracker's front-end stream ("fe_cu_percent" of the CUs): side by side with both chains of the tail.
int svo_track_fe_batch_stream(svo_ctx* ctx) {
  if (ctx->stream_fe_batch) return SVO_OK;
  const int dev = ctx->device, pct = ctx->opt_fe_cu_percent;
  int attempts = 0, percent = 0;
  const int rc = svo_pick_stream(ctx, [dev, pct](hipStream_t* s) { return pct < 100 ? svo_stream_create_masked(s, dev, pct) : svo_stream_create(s, -1); },
                                 {ctx->stream, ctx->stream_idx}, &ctx->stream_fe_batch, &attempts, &percent,
                                 {ctx->stream, ctx->stream_idx, ctx->stream_dense}, {ctx->stream_dense});   // (its grids wait for their eighth of the CUs: no chain, and not the dense stage, behind them)
  if (rc == SVO_OK) { ctx->stream_diag_done = true; track_stream_diag(ctx); }
  return rc;
}

// SVO_STREAM_DIAG=1: how long a grid of many small workgroups (the index chain's shape) takes on each of the tracker's streams, alone
// and while front-end-like grids keep the front end's stream busy - printed once per context (docs/NEXT_ROUNDS.md, process states).
__global__ void k_diag_spin(long long cycles) {
  const long long t0 = clock64();
  while (clock64() - t0 < cycles) __builtin_amdgcn_s_sleep(2);
}
void track_stream_diag(svo_ctx* ctx) {
  static const bool on = []() { const char* e = getenv("SVO_STREAM_DIAG"); return e && e[0] == '1'; }();
  if (!on || !ctx->stream_idx || !ctx->stream_fe_batch) return;
  hipStream_t ss[3] = {ctx->stream, ctx->stream_idx, ctx->stream_fe_batch};
  const char* nm[3] = {"pose", "index", "front end"};
  auto grid_us = [](hipStream_t q, int wgs, int threads, long long cyc) {
    double best = 1e30;
    for (int rep = 0; rep < 3; ++rep) {
      hipStreamSynchronize(q);
      const auto t0 = std::chrono::steady_clock::now();
      hipLaunchKernelGGL(k_diag_spin, dim3(wgs), dim3(threads), 0, q, cyc);
      hipStreamSynchronize(q);
      best = std::min(best, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    return best;
  };
  for (int k = 0; k < 3; ++k) {
    const double one = grid_us(ss[k], 1, 64, 4000), many = grid_us(ss[k], 3072, 64, 4000), big = grid_us(ss[k], 2048, 256, 40000);
    double beside = 0;
    if (k < 2) {
      for (int i = 0; i < 4; ++i) hipLaunchKernelGGL(k_diag_spin, dim3(4096), dim3(256), 0, ss[2], 100000LL);
      beside = grid_us(ss[k], 3072, 64, 4000);
      hipStreamSynchronize(ss[2]);
    }
    fprintf(stderr, "[svo stream diag] ctx %p %-9s stream %p: 1 workgroup %.0f us, 3072 x 64 threads %.0f us, 2048 x 256 threads (18 us each) %.0f us, 3072 x 64 beside front-end grids %.0f us\n",
            (void*)ctx, nm[k], (void*)ss[k], one, many, big, beside);
  }
  (void)hipGetLastError();
}

// Depth source 1 (svo_set_option "depth_source"): the reference's live data flow - a dense disparity map
// (src/Tracking.cc:226 `MB`, here the ELAS map D1) -> frame::disp2Depth (src/frame.cc:140-164: depth =
// bf / disp wherever disp != 0, else -1) -> `depthimg.at<float>(y, x)` at the truncated keypoint position;
// keypoints_r = x - disp unless disp == -1 (src/frame.cc:122-138).  D == nullptr: no map, no depth.
// blockIdx.y = frame slot of a batch: map `map_stride` floats further on (0 floats: one frame), `produced` (may
// be null) says whether that frame has a map at all.
__global__ void k_tk_dense_depth(const svo_kp* kp, const int32_t* nkp, const float* D, int W, float bf,
                                 float* uR, float* depth, int K, size_t map_stride, const int32_t* produced) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= K) return;
  kp += (size_t)blockIdx.y * K; nkp += blockIdx.y; uR += (size_t)blockIdx.y * K; depth += (size_t)blockIdx.y * K;
  if (D) D += (size_t)blockIdx.y * map_stride;
  if (produced && !produced[blockIdx.y]) D = nullptr;
  float u = -1.0f, z = -1.0f;
  if (i < *nkp && D) {
    const float disp = D[(size_t)(int)kp[i].y * W + (int)kp[i].x];
    if (disp != -1.0f) u = kp[i].x - disp;
    if (disp != 0.0f) z = bf / disp;
  }
  uR[i] = u; depth[i] = z;
}

// room for B frames' dense maps (two float maps and one flag per frame)
static int dense_reserve(svo_ctx* ctx, int B) {
  if (ctx->dense_cap >= B) return SVO_OK;
  const size_t n = (size_t)ctx->g.W * ctx->g.H;
  SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->d_dense) hipFree(ctx->d_dense);
  ctx->d_dense = nullptr; ctx->dense_cap = 0;
  SVO_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->d_dense), (2 * n * sizeof(float) + sizeof(int32_t)) * (size_t)B));
  ctx->dense_cap = B;
  return SVO_OK;
}

extern "C" int svo_track_frame(svo_ctx* ctx, const uint8_t* grayL, int strideL,
                               const uint8_t* grayR, int strideR, double timestamp,
                               const int32_t* boxes, int n_boxes, svo_track_result* res) {
  (void)timestamp;
  if (!ctx || !grayL || !grayR || !res || strideL < ctx->g.W || strideR < ctx->g.W || n_boxes < 0 ||
      n_boxes > SVO_MAX_BOXES || (n_boxes > 0 && !boxes))
    return SVO_E_INVALID;
  if (!ctx->d_track || ctx->n_seq != 1) return SVO_E_INVALID;   // svo_track_reset first
  { const int rcd = svo_track_dyn_refuse_single(ctx, "svo_track_frame"); if (rcd) return rcd; }
  hipSetDevice(ctx->device);
  { const int rcq = svo_track_quiesce(ctx); if (rcq) return rcq; }
  int rc = svo_upload_image(ctx, grayL, strideL, 0);
  if (rc) return rc;
  if ((rc = svo_upload_image(ctx, grayR, strideR, 1))) return rc;
  return svo_track_frame_staged(ctx, boxes, n_boxes, res, nullptr, nullptr, 0);
}

// svo_track_frame / svo_track_frame_bgr from the point where the pair's gray images are in staging slots 0 / 1
int svo_track_frame_staged(svo_ctx* ctx, const int32_t* boxes, int n_boxes, svo_track_result* res, const uint8_t* d_bgrL,
                           const uint8_t* d_bgrR, int bgr_pitch) {
  TrackCall call;   // (the attachments' arrays: host memory, complete when the entry returns)
  int rc = call.begin(ctx, "svo_track_frame", ctx->d_stage, ctx->stage_pitch, d_bgrL, bgr_pitch, true, true);
  if (rc) return rc;
  const SvoGeom& g = ctx->g;
  TrackState* st = reinterpret_cast<TrackState*>(ctx->d_track);
  uint8_t* dL = ctx->d_stage;
  uint8_t* dR = ctx->d_stage + (size_t)g.H * ctx->stage_pitch;
  // the frame's boxes go to HBM with the images (pinned staging: the copies are asynchronous, the caller's array may be
  // pageable); from there on a gated frame is device work only
  int32_t* h_box = reinterpret_cast<int32_t*>(ctx->h_pinned + ctx->pinned_bytes - 4096);   // the buffer's last page: reserved for this (svo_msa.hip stays below it)
  h_box[0] = n_boxes;
  if (n_boxes > 0) memcpy(h_box + 4, boxes, 16 * (size_t)n_boxes);
  SVO_HIP(ctx, hipMemcpyAsync(&st->n_boxes, h_box, 4, hipMemcpyHostToDevice, ctx->stream));
  if (n_boxes > 0)
    SVO_HIP(ctx, hipMemcpyAsync(st->boxes, h_box + 4, 16 * (size_t)n_boxes, hipMemcpyHostToDevice, ctx->stream));
  const svo_boxes_dev bx{st->boxes, &st->n_boxes, SVO_MAX_BOXES};
  const SvoFeBufs fb = svo_fe_own(ctx);
  const float* dense = nullptr;   // depth_source 1, 2, 3: the frame's dense map (nullptr: none was produced)
  if (ctx->opt_depth_source == 1) {
    if ((rc = svo_launch_orb(ctx, ctx->stream, fb, dL, dR, ctx->stage_pitch, 1, 1))) return rc;   // left image only
    svo_elas_params ep;
    svo_elas_default_params(0, &ep);
    float *dD1 = nullptr, *dD2 = nullptr;
    int produced = 0;
    if ((rc = svo_elas_run_dev(ctx, dL, dR, ctx->stage_pitch, g.W, g.H, &ep, &dD1, &dD2, &produced))) return rc;
    dense = produced ? dD1 : nullptr;
  } else if (ctx->opt_depth_source == 2) {
    // the reference's live configuration: frame::MB = MSA::solve(left, right, 48, 1) (src/Tracking.cc:225-228)
    if ((rc = svo_launch_orb(ctx, ctx->stream, fb, dL, dR, ctx->stage_pitch, 1, 1))) return rc;
    if ((rc = dense_reserve(ctx, 1))) return rc;
    // (colour entry: MSA gets the true colour pair, as in the reference; gray entry: B = G = R copies of the gray)
    if ((rc = d_bgrL ? svo_msa_run_dev(ctx, d_bgrL, d_bgrR, bgr_pitch, g.W, g.H, 48, ctx->d_dense, true)
                     : svo_msa_run_dev(ctx, dL, dR, ctx->stage_pitch, g.W, g.H, 48, ctx->d_dense)))
      return rc;
    dense = ctx->d_dense;
  } else if (ctx->opt_depth_source == 3) {
    // the body of the reference's frame::ElasMatch (src/frame.cc:94-120): SGBM on the gray pair; invalid pixels are -1
    if ((rc = svo_launch_orb(ctx, ctx->stream, fb, dL, dR, ctx->stage_pitch, 1, 1))) return rc;
    if ((rc = dense_reserve(ctx, 1))) return rc;
    // (colour entry with "sgbm_colour": the cn = 3 solver on the BGR pair, as the reference calls it)
    svo_sgbm_params sp;
    if (d_bgrL && ctx->opt_sgbm_colour) {
      svo_sgbm_default_params_bgr(g.H, &sp);
      rc = svo_sgbm_run_bgr_dev(ctx, ctx->stream, d_bgrL, d_bgrR, bgr_pitch, (size_t)g.H * bgr_pitch, g.W, g.H, 1, &sp, ctx->opt_sgbm_mode, ctx->d_dense);
    } else {
      svo_sgbm_default_params(g.H, &sp);
      rc = svo_sgbm_run_dev(ctx, ctx->stream, dL, dR, ctx->stage_pitch, (size_t)g.H * ctx->stage_pitch, g.W, g.H, 1, &sp, ctx->opt_sgbm_mode, ctx->d_dense);
    }
    if (rc) return rc;
    dense = ctx->d_dense;
  } else {
    if ((rc = svo_launch_orb(ctx, ctx->stream, fb, dL, dR, ctx->stage_pitch, 1, 2))) return rc;
    if ((rc = svo_launch_stereo(ctx, ctx->stream, fb, dL, dR, ctx->stage_pitch, 1, &ctx->cam))) return rc;
  }
  if (ctx->opt_depth_source != 0) {
    SvoTimer t(ctx, "k_tk_dense_depth");
    hipLaunchKernelGGL(k_tk_dense_depth, dim3((ctx->max_kp + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_kp,
                       ctx->d_nkp, dense, g.W, ctx->cam.bf, ctx->d_uR, ctx->d_depth, ctx->max_kp, (size_t)0,
                       (const int32_t*)nullptr);
  }
  svo_track_result* d_res = reinterpret_cast<svo_track_result*>(ctx->d_scratch);
  rc = tail_enqueue(ctx, ctx->d_kp, ctx->d_desc, ctx->d_nkp, ctx->d_depth, ctx->max_kp, 1, 1, d_res, n_boxes > 0 ? &bx : nullptr);
  if (rc) return rc;
  SVO_HIP(ctx, hipMemcpyAsync(res, d_res, sizeof *res, hipMemcpyDeviceToHost, ctx->stream));
  SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->track_frame++;
  return call.end(res->n_pnp_inliers == -1 ? svo_track_check_timeout(ctx) : SVO_OK);   // (-1: the record is valid, the frame was tracked as a PnP failure)
}

// One time step of n_seq independent sequences: pair q is the next frame of sequence q.
extern "C" int svo_track_multi_step_dev(svo_ctx* ctx, const uint8_t* d_grayL, const uint8_t* d_grayR,
                                        int stride, int n_seq, const svo_boxes_dev* boxes, svo_track_result* d_results) {
  if (!ctx || !d_grayL || !d_grayR || !d_results || stride < ctx->g.W) return SVO_E_INVALID;
  if (!ctx->d_track || n_seq != ctx->n_seq) return SVO_E_INVALID;   // svo_track_multi_reset(n_seq) first
  { const int rcc = svo_track_multi_step_check(ctx, "svo_track_multi_step_dev", false); if (rcc) return rcc; }
  return svo_track_multi_step_fed(ctx, d_grayL, d_grayR, stride, n_seq, boxes, d_results, nullptr);
}

// what both many-sequence entries refuse before anything is allocated or enqueued
int svo_track_multi_step_check(svo_ctx* ctx, const char* who, bool has_bgr) {
  { const int rcd = dyn_refuse_multi(ctx, who); if (rcd) return rcd; }
  { const int rcm = svo_track_map_refuse(ctx, who); if (rcm) return rcm; }
  if (ctx->opt_depth_source != 0) {   // the many-sequence mode has the sparse matcher only
    ctx->last_error = std::string(who) + ": depth_source must be 0";
    return SVO_E_INVALID;
  }
  if (dyn_colour(ctx) && !has_bgr) return dyn_colour_needs_bgr(ctx, who);
  return SVO_OK;
}
// The step of the two many-sequence entries, which have checked their arguments and called svo_track_multi_step_check; with the
// loop in force (adopted by svo_track_multi_reset) its images are the gray the front end reads, or - colour = 1 - the colour left frames
int svo_track_multi_step_fed(svo_ctx* ctx, const uint8_t* d_grayL, const uint8_t* d_grayR, int stride, int n_seq,
                             const svo_boxes_dev* boxes, svo_track_result* d_results, const SvoBgrSrc* bgr) {
  TrackCall call;   // (svo_track_dynamic_out's arrays: device memory, sequence by sequence)
  int rc = call.begin(ctx, "svo_track_multi_step_dev", d_grayL, stride, bgr ? bgr->L : nullptr, bgr ? bgr->stride : 0, false, false);
  if (rc) return rc;
  hipSetDevice(ctx->device);
  { const int rcs = svo_shard_quiesce(ctx); if (rcs) return rcs; }   // (a sharded call of this context may still be in flight: staging sets, work records)
  // the step's front end on stream `s` into `fb`: the colour entry's gray of the 2 n_seq images first, ORB, sparse stereo
  auto front_end = [&](hipStream_t s, const SvoFeBufs& fb) -> int {
    SVO_HIP(ctx, svo_rect_gate(ctx, s));   // (images of svo_rect_batch_dev(consumer = ctx): the tail reads them behind this front end)
    int rcf = bgr_to_gray(ctx, s, bgr, d_grayL, d_grayR, stride, 0, n_seq, true);
    if (rcf == SVO_OK) rcf = svo_launch_orb(ctx, s, fb, d_grayL, d_grayR, stride, n_seq, 2 * n_seq);
    if (rcf == SVO_OK) rcf = svo_launch_stereo(ctx, s, fb, d_grayL, d_grayR, stride, n_seq, &ctx->cam);
    if (rcf == SVO_OK && bgr && bgr->convert && bgr->done) SVO_HIP(ctx, hipEventRecord(bgr->done, s));
    return rcf;
  };
  if (ctx->opt_multi_pipeline) {
    // Pipelined steps (svo_set_option("multi_pipeline", 1)): the front end is stateless, so step t + 1's may run while
    // step t's tail is still busy - on its own stream, into the other of two private output sets.  Contract: between
    // consecutive steps nothing else is enqueued on this context (svo_sync and reading results are fine).
    if (ctx->ms_cap < n_seq) {
      SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
      if (ctx->stream_fe) SVO_HIP(ctx, hipStreamSynchronize(ctx->stream_fe));
      ctx->ms_cap = 0;   // a failed allocation below leaves empty sets and no capacity behind, never freed memory
      if ((rc = fe_sets_alloc(ctx->ms_out, 2, 2 * (size_t)n_seq, n_seq, ctx->max_kp, false))) return rc;
      for (int p = 0; p < 2; ++p) {
        if (!ctx->ms_fe_done[p]) SVO_HIP(ctx, hipEventCreateWithFlags(&ctx->ms_fe_done[p], hipEventDisableTiming));
        if (!ctx->ms_tail_done[p]) SVO_HIP(ctx, hipEventCreateWithFlags(&ctx->ms_tail_done[p], hipEventDisableTiming));
        ctx->ms_tail_recorded[p] = false;
      }
      ctx->ms_cap = n_seq;
    }
    if ((rc = track_resources(ctx, 1, n_seq))) return rc;   // streams and events exist from here on
    if (!ctx->stream_fe) {   // (confining it to a share of the CUs only costs: 88 % -6 %, 75 % -8 %, 50 % -34 % with 64 sequences)
      int attempts = 0, percent = 0;
      const int rcp = svo_pick_stream(ctx, [](hipStream_t* q) { return svo_stream_create(q, -1); }, {ctx->stream, ctx->stream_idx}, &ctx->stream_fe,
                                      &attempts, &percent, {ctx->stream, ctx->stream_idx}, {});
      if (rcp) return rcp;
    }
    const int p = ctx->ms_parity;
    if (ctx->ms_tail_recorded[p]) {
      SVO_HIP(ctx, hipStreamWaitEvent(ctx->stream_fe, ctx->ms_tail_done[p], 0));   // the tail that read this set two steps ago
    } else {
      SVO_HIP(ctx, hipEventRecord(ctx->ev_frontend, ctx->stream));                  // first use: after whatever came before
      SVO_HIP(ctx, hipStreamWaitEvent(ctx->stream_fe, ctx->ev_frontend, 0));
    }
    const SvoFeBufs fb = svo_fe_own(ctx).with_outputs(ctx->ms_out[p]);   // (right x and SAD: the context's own arrays)
    if ((rc = front_end(ctx->stream_fe, fb))) return rc;
    SVO_HIP(ctx, hipEventRecord(ctx->ms_fe_done[p], ctx->stream_fe));
    SVO_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ms_fe_done[p], 0));
    if ((rc = tail_enqueue(ctx, fb.kp, fb.desc, fb.nkp, fb.depth, ctx->max_kp, 1, n_seq, d_results, boxes))) return rc;
    SVO_HIP(ctx, hipEventRecord(ctx->ms_tail_done[p], ctx->stream));
    ctx->ms_tail_recorded[p] = true;
    ctx->ms_parity ^= 1;
    ctx->track_frame++;
    return SVO_OK;
  }
  const SvoFeBufs fb = svo_fe_own(ctx);
  if ((rc = front_end(ctx->stream, fb))) return rc;
  if ((rc = tail_enqueue(ctx, ctx->d_kp, ctx->d_desc, ctx->d_nkp, ctx->d_depth, ctx->max_kp, 1, n_seq, d_results, boxes))) return rc;
  ctx->track_frame++;
  return SVO_OK;
}

int svo_track_batch_fed(svo_ctx* ctx, const uint8_t* d_grayL, const uint8_t* d_grayR, int stride, int B,
                        const svo_boxes_dev* boxes, svo_track_result* d_results, const hipEvent_t* pair_ready, const SvoBgrSrc* bgr) {
  if (!ctx) return SVO_E_INVALID;
  TrackCall call;   // (the attachments' arrays: host memory for the host-fed entries, device memory otherwise)
  int rc = call.begin(ctx, "svo_track_batch", d_grayL, stride, bgr ? bgr->L : nullptr, bgr ? bgr->stride : 0, pair_ready != nullptr, false);
  if (rc) return rc;
  if (!d_grayL || !d_grayR || !d_results || B < 1 || stride < ctx->g.W) return SVO_E_INVALID;
  if (B > ctx->max_batch) return SVO_E_CAPACITY;
  if (!ctx->d_track || ctx->n_seq != 1) return SVO_E_INVALID;
  hipSetDevice(ctx->device);
  { const int rcs = svo_shard_quiesce(ctx); if (rcs) return rcs; }   // (a sharded call of this context may still be in flight: staging sets, work records)
  const size_t gray_img = (size_t)ctx->g.H * stride, bgr_img = bgr ? (size_t)ctx->g.H * bgr->stride : 0;
  if (ctx->opt_depth_source == 1 || ctx->opt_depth_source == 3) {
    // (depth_source 3: the same pipeline with SGBM maps, which have no host phase - chunks of svo_sgbm_chunk() pairs, every pair
    // produces a map)
    // BASELINE configs[4] as a pipeline: the dense front end (ORB on the left images, ELAS maps, the reference's per-keypoint
    // lookups - src/Tracking.cc:225-228, src/frame.cc:122-164) runs on a stream of its own; svo_elas_batch_dev moves the call's
    // pairs through its GPU -> host -> GPU stages in chunks, and as soon as a chunk's last GPU phase is enqueued the hook
    // below hangs that chunk's depth lookups behind it and enqueues the ordered tail of its frames on the tail's streams - the
    // tail of chunk c runs while chunks c + 1 ... are still in the dense stage (whose host phases - support-point filter,
    // Delaunay - block this thread, not the GPU).  Every chunk uses its own half of the work records, like consecutive calls
    // of the sparse path.
    const size_t n = (size_t)ctx->g.W * ctx->g.H, K = ctx->max_kp;
    if ((rc = dense_reserve(ctx, B))) return rc;
    if ((rc = track_resources(ctx, B, 1))) return rc;
    if (!ctx->stream_dense) {   // the dense stage's stream: beside both chains of the tail
      // (confined: a hardware queue of its own - which may still sit behind the dispatch pipe of one of the chains or of the front
      // end's queue: picked by measurement either way)
      const int dev = ctx->device, pct = ctx->opt_dense_cu_percent;
      int attempts = 0, percent = 0;
      const int rcp = svo_pick_stream(ctx, [dev, pct](hipStream_t* q) { return pct < 100 ? svo_stream_create_masked(q, dev, pct) : svo_stream_create(q, 0); },
                                      {ctx->stream, ctx->stream_idx}, &ctx->stream_dense, &attempts, &percent,
                                      {ctx->stream, ctx->stream_idx, ctx->stream_fe_batch}, {ctx->stream_fe_batch});
      if (rcp) return rcp;
    }
    float* dD1 = ctx->d_dense;
    float* dD2 = dD1 + n * (size_t)ctx->dense_cap;
    int32_t* d_prod = reinterpret_cast<int32_t*>(dD2 + n * (size_t)ctx->dense_cap);
    if (ctx->h_prod_cap < B) {
      if (ctx->h_prod) { SVO_HIP(ctx, hipStreamSynchronize(ctx->stream_dense)); hipHostFree(ctx->h_prod); ctx->h_prod = nullptr; ctx->h_prod_cap = 0; }
      if (hipHostMalloc(reinterpret_cast<void**>(&ctx->h_prod), sizeof(int32_t) * (size_t)B) != hipSuccess) { (void)hipGetLastError(); return SVO_E_NOMEM; }
      ctx->h_prod_cap = B;
    }
    svo_elas_params ep;
    svo_elas_default_params(0, &ep);
    if ((rc = tb_done_events(ctx))) return rc;
    // the dense stage writes the ctx's own result arrays and maps: everything the ctx stream holds (an earlier call's tail) first
    SVO_HIP(ctx, svo_rect_gate(ctx, ctx->stream));   // (and a rectifier's images: the dense stage's streams fork from here)
    SVO_HIP(ctx, hipEventRecord(ctx->ev_frontend, ctx->stream));
    SVO_HIP(ctx, hipStreamWaitEvent(ctx->stream_dense, ctx->ev_frontend, 0));
    struct Hook {
      svo_ctx* ctx; const svo_boxes_dev* boxes; svo_track_result* d_results; float* dD1; int32_t* d_prod;
      size_t n, K; int chunk;
      static int run(void* u, int f0, int b) {
        Hook& h = *static_cast<Hook*>(u);
        svo_ctx* ctx = h.ctx;
        hipStream_t sd = ctx->stream_dense;
        if (track_events_reserve(ctx->ev_sub, h.chunk + 1) != hipSuccess) return SVO_E_HIP;
        if (hipMemcpyAsync(h.d_prod + f0, ctx->h_prod + f0, sizeof(int32_t) * (size_t)b, hipMemcpyHostToDevice, sd) != hipSuccess) return SVO_E_HIP;
        const SvoFeBufs o = svo_fe_own(ctx).outputs_at(h.K, f0, f0);
        hipLaunchKernelGGL(k_tk_dense_depth, dim3((ctx->max_kp + 255) / 256, b), dim3(256), 0, sd, o.kp, o.nkp,
                           h.dD1 + h.n * f0, ctx->g.W, ctx->cam.bf, o.uR, o.depth, ctx->max_kp, h.n, h.d_prod + f0);
        if (hipEventRecord(ctx->ev_sub[h.chunk], sd) != hipSuccess) return SVO_E_HIP;
        const int p = ctx->tb_parity;
        std::vector<hipEvent_t> wait(b, nullptr);
        wait[0] = ctx->ev_sub[h.chunk];
        svo_boxes_dev bj{nullptr, nullptr, 0};
        if (h.boxes && h.boxes->boxes && h.boxes->n) bj = svo_boxes_dev{h.boxes->boxes + (size_t)f0 * h.boxes->stride * 4, h.boxes->n + f0, h.boxes->stride};
        int rc = tail_enqueue(ctx, o.kp, o.desc, o.nkp, o.depth, ctx->max_kp, b, 1, h.d_results + f0, bj.boxes ? &bj : nullptr, wait.data(),
                              nullptr, p, ctx->tb_used[p] ? ctx->tb_done[p] : ctx->ev_frontend, true);
        if (rc == SVO_OK && hipEventRecord(ctx->tb_done[p], ctx->stream) != hipSuccess) rc = SVO_E_HIP;   // the pose chain is the last reader of this half
        if (rc) return rc;
        ctx->tb_used[p] = true;
        ctx->tb_parity ^= 1;
        ctx->track_frame += b;
        ++h.chunk;
        return SVO_OK;
      }
    } hook{ctx, boxes, d_results, dD1, d_prod, n, K, 0};
    if (pair_ready) SVO_HIP(ctx, hipStreamWaitEvent(ctx->stream_dense, pair_ready[B - 1], 0));   // host-fed: the call's uploads
    if ((rc = bgr_to_gray(ctx, ctx->stream_dense, bgr, d_grayL, d_grayR, stride, 0, B, true))) return rc;   // (ELAS runs on the gray, like ORB: the reference never calls libelas)
    rc = svo_launch_orb(ctx, ctx->stream_dense, svo_fe_own(ctx), d_grayL, d_grayR, stride, B, B);   // left images only
    if (rc == SVO_OK && ctx->opt_depth_source == 3) {
      // (colour entries with "sgbm_colour": the cn = 3 solver on the BGR pairs, in its own, smaller chunks)
      const bool colour = bgr && ctx->opt_sgbm_colour;
      svo_sgbm_params sp;
      if (colour) svo_sgbm_default_params_bgr(ctx->g.H, &sp); else svo_sgbm_default_params(ctx->g.H, &sp);
      for (int f0 = 0, step = colour ? svo_sgbm_chunk_bgr() : svo_sgbm_chunk(); f0 < B && rc == SVO_OK; f0 += step) {
        const int b = std::min(step, B - f0);
        for (int k = 0; k < b; ++k) ctx->h_prod[f0 + k] = 1;
        rc = colour ? svo_sgbm_run_bgr_dev(ctx, ctx->stream_dense, bgr->L + f0 * bgr_img, bgr->R + f0 * bgr_img, bgr->stride, bgr_img,
                                           ctx->g.W, ctx->g.H, b, &sp, ctx->opt_sgbm_mode, dD1 + n * f0)
                    : svo_sgbm_run_dev(ctx, ctx->stream_dense, d_grayL + f0 * gray_img, d_grayR + f0 * gray_img, stride, gray_img, ctx->g.W,
                              ctx->g.H, b, &sp, ctx->opt_sgbm_mode, dD1 + n * f0);
        if (rc == SVO_OK) rc = Hook::run(&hook, f0, b);
      }
      return rc;
    }
    if (rc == SVO_OK)
      rc = svo_elas_batch_dev_hooked(ctx, ctx->stream_dense, d_grayL, d_grayR, stride, ctx->g.W, ctx->g.H, B, &ep, dD1, dD2, ctx->h_prod,
                                     &Hook::run, &hook);
    return rc;
  } else if (ctx->opt_depth_source == 2) {
    // MSA maps, up to eight frames in flight (most of a solve is the host tree builds)
    const size_t n = (size_t)ctx->g.W * ctx->g.H;
    if ((rc = dense_reserve(ctx, B))) return rc;
    if (pair_ready) SVO_HIP(ctx, hipStreamWaitEvent(ctx->stream, pair_ready[B - 1], 0));   // host-fed: the call's uploads
    SVO_HIP(ctx, svo_rect_gate(ctx, ctx->stream));
    if ((rc = bgr_to_gray(ctx, ctx->stream, bgr, d_grayL, d_grayR, stride, 0, B, true))) return rc;
    if ((rc = svo_launch_orb(ctx, ctx->stream, svo_fe_own(ctx), d_grayL, d_grayR, stride, B, B))) return rc;   // left images only
    // (colour entries: MSA gets the true colour pairs, as in the reference; gray entries: B = G = R copies of the gray)
    if ((rc = bgr ? svo_msa_run_many_dev(ctx, bgr->L, bgr->R, bgr->stride, bgr_img, ctx->g.W, ctx->g.H, 48, B, ctx->d_dense, true)
                  : svo_msa_run_many_dev(ctx, d_grayL, d_grayR, stride, (size_t)ctx->g.H * stride, ctx->g.W, ctx->g.H, 48, B,
                                         ctx->d_dense)))
      return rc;
    hipLaunchKernelGGL(k_tk_dense_depth, dim3((ctx->max_kp + 255) / 256, B), dim3(256), 0, ctx->stream, ctx->d_kp, ctx->d_nkp,
                       ctx->d_dense, ctx->g.W, ctx->cam.bf, ctx->d_uR, ctx->d_depth, ctx->max_kp, n, (const int32_t*)nullptr);
  } else {
    // The front end runs in sub-batches on its own stream, so that only the first sub-batch stands in front of the
    // ordered tail: while the tail works through sub-batch j, the front end of j + 1 runs beside it.  Sub-batch j writes the
    // keypoints of its LEFT images to frame slots f0 .. f0 + b - 1 (what the tail reads); its right images use the slots
    // behind them, which the next sub-batch's left images overwrite later on the same stream.
    rc = track_resources(ctx, B, 1);
    if (rc) return rc;
    const int SUB = 32, nsub = (B + SUB - 1) / SUB;
    // The front end of a batched call runs beside the ordered tail, and its kernels are large enough to fill every CU: the
    // tail's small dependent kernels (100 single-wave RANSAC workgroups that want a CU's float64 pipe each) then queue for
    // slots and run at a fraction of their speed - 7 us per frame on average (tools/option_sweep.py: 13.2 k frames/s with the
    // front end on all CUs, 14.1 k on a quarter of them, 14.4 k on 32 CUs; stream priorities did not change that).  So the
    // batched tracker's front-end stream is confined to a share of the compute units (default an eighth: four CUs of every XCD): the
    // front end needs ~7 us per pair on the whole chip against the tail's ~70 us per frame - an eighth of the chip keeps up.
    { const int rcf = svo_track_fe_batch_stream(ctx); if (rcf) return rcf; }
    SVO_HIP(ctx, track_events_reserve(ctx->ev_sub, nsub));
    // Output sets alternate between calls: this call's front end writes set p while the tail of the previous call still reads
    // the other one - it only has to wait for the tail of the call BEFORE that (first use of a set: for whatever the ctx
    // stream holds).  The front end's working set (pyramids, corner lists) is shared: stream_fe runs the calls' sub-batches
    // one after the other anyway.
    const int p = ctx->tb_parity;
    if (p == 1 && !ctx->tb_out[1].kp && (rc = fe_sets_alloc(&ctx->tb_out[1], 1, ctx->max_images, ctx->max_batch, ctx->max_kp, true)))
      return rc;
    if ((rc = tb_done_events(ctx))) return rc;
    if (ctx->tb_used[p]) {
      SVO_HIP(ctx, hipStreamWaitEvent(ctx->stream_fe_batch, ctx->tb_done[p], 0));
    } else {
      SVO_HIP(ctx, hipEventRecord(ctx->ev_frontend, ctx->stream));
      SVO_HIP(ctx, hipStreamWaitEvent(ctx->stream_fe_batch, ctx->ev_frontend, 0));
    }
    std::vector<hipEvent_t> wait(B, nullptr);
    const SvoFeBufs set = svo_fe_own(ctx).with_outputs(ctx->tb_out[p]);   // (set 0: tb_out[0] is empty, the context's own outputs)
    const size_t K = ctx->max_kp, img = (size_t)ctx->g.H * stride;
    hipStream_t fs = ctx->stream_fe_batch;
    SVO_HIP(ctx, svo_rect_gate(ctx, fs));   // (images of svo_rect_batch_dev(consumer = ctx): both chains read them behind the sub-batch events)
    for (int j = 0; j < nsub && rc == SVO_OK; ++j) {
      const int f0 = j * SUB, b = std::min(SUB, B - f0);
      const SvoFeBufs fb = set.outputs_at(K, f0, f0);
      if (pair_ready && hipStreamWaitEvent(fs, pair_ready[f0 + b - 1], 0) != hipSuccess) rc = SVO_E_HIP;   // host-fed: this sub-batch's uploads
      if (rc) break;
      rc = bgr_to_gray(ctx, fs, bgr, d_grayL, d_grayR, stride, f0, b, j == 0);   // (colour entries: this sub-batch's gray, on the front end's share of the CUs)
      if (rc == SVO_OK) rc = svo_launch_orb(ctx, fs, fb, d_grayL + f0 * img, d_grayR + f0 * img, stride, b, 2 * b);
      if (rc == SVO_OK) rc = svo_launch_stereo(ctx, fs, fb, d_grayL + f0 * img, d_grayR + f0 * img, stride, b, &ctx->cam);
      if (rc == SVO_OK && hipEventRecord(ctx->ev_sub[j], fs) != hipSuccess) rc = SVO_E_HIP;
      wait[f0] = ctx->ev_sub[j];
    }
    if (rc) return rc;
    // (the index chain: its inputs arrive through the sub-batch events; its half of the work records was last read by the pose
    // chain of the call before the previous one - the same event the front end waited for)
    if ((rc = tail_enqueue(ctx, set.kp, set.desc, set.nkp, set.depth, ctx->max_kp, B, 1, d_results, boxes, wait.data(), nullptr, p,
                           ctx->tb_used[p] ? ctx->tb_done[p] : ctx->ev_frontend, true)))
      return rc;
    SVO_HIP(ctx, hipEventRecord(ctx->tb_done[p], ctx->stream));   // the pose chain is the last reader of this call's set
    ctx->tb_used[p] = true;
    ctx->tb_parity ^= 1;
    ctx->track_frame += B;
    return SVO_OK;
  }
  if ((rc = tail_enqueue(ctx, ctx->d_kp, ctx->d_desc, ctx->d_nkp, ctx->d_depth, ctx->max_kp, B, 1, d_results, boxes))) return rc;
  ctx->track_frame += B;
  return SVO_OK;
}

extern "C" int svo_track_batch_dev(svo_ctx* ctx, const uint8_t* d_grayL, const uint8_t* d_grayR,
                                   int stride, int B, const svo_boxes_dev* boxes, svo_track_result* d_results) {
  if (ctx) { const int rcd = svo_track_dyn_refuse_single(ctx, "svo_track_batch_dev"); if (rcd) return rcd; }
  return svo_track_batch_fed(ctx, d_grayL, d_grayR, stride, B, boxes, d_results, nullptr);
}

// The ordered tail alone, for front-end results produced elsewhere (another context, another GPU): frame f's keypoints
// at d_kp + f * kp_stride, descriptors at d_desc + f * kp_stride * 32, count d_n[f], depths d_depth + f * kp_stride.
extern "C" int svo_track_tail_dev(svo_ctx* ctx, const svo_kp* d_kp, const uint8_t* d_desc, const int32_t* d_n,
                                  const float* d_depth, int kp_stride, int B, const svo_boxes_dev* boxes,
                                  svo_track_result* d_results) {
  if (!ctx || !d_kp || !d_desc || !d_n || !d_depth || !d_results || B < 1 || kp_stride < 1) return SVO_E_INVALID;
  if (!ctx->d_track || ctx->n_seq != 1) return SVO_E_INVALID;   // svo_track_reset first
  { const int rcd = svo_track_dyn_refuse(ctx, "svo_track_tail_dev"); if (rcd) return rcd; }
  hipSetDevice(ctx->device);
  { const int rcs = svo_shard_quiesce(ctx); if (rcs) return rcs; }   // (a sharded call of this context may still be in flight: staging sets, work records)
  TrackCall call;   // (svo_track_map_out's arrays: device memory)
  int rc = call.begin(ctx, "svo_track_tail_dev", nullptr, 0, nullptr, 0, false, false);
  if (rc == SVO_OK) rc = tail_enqueue(ctx, d_kp, d_desc, d_n, d_depth, kp_stride, B, 1, d_results, boxes);
  if (rc) return rc;
  ctx->track_frame += B;
  return SVO_OK;
}
