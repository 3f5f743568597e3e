// svo_colour.hip - colour (8UC3 BGR) input of the tracker (include/svo.h: svo_bgr_to_gray, svo_track_frame_bgr,
// svo_track_batch_bgr_dev; svo_track_batch_bgr_host lives with the other host-fed entries in svo_hostfeed.hip).
//
// The reference's driver reads KITTI image_2 / image_3 unchanged (main.cpp:160-161): 8UC3 BGR.  Two stages consume them:
// cv::ORB reduces the colour to gray itself (COLOR_BGR2GRAY in fixed point, src/frame.cc:75-79), and frame::MB hands the
// colour to MSA::solve (src/frame.cc:82-91), whose cost, median filter and tree weights work on the three channels.  The
// colour entries therefore convert each pair once on the device (k_bgr2gray, bit-exact with that fixed point) for ORB, the
// sparse matcher and ELAS, and give MSA the colour itself.
#include <string.h>

#include <algorithm>

#include "svo_internal.h"
#include "svo_gate.h"

namespace {

constexpr int BGR_PX = 1024;                        // pixels per workgroup: 256 lanes x 4
constexpr int BGR_LDS_DW = (3 * BGR_PX + 3) / 4 + 5;   // the segment's dwords + a misaligned start + the last lane's over-read

// cv::cvtColor(COLOR_BGR2GRAY) for 8U: fixed-point weights 0.114 / 0.587 / 0.299 in 14 bits (1868 + 9617 + 4899 = 16384, so
// B = G = R = v gives v) - the same formula as host/png_reader.h
__device__ __forceinline__ uint32_t bgr_gray(uint32_t b, uint32_t g, uint32_t r) {
  return (b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14;
}

// One workgroup per 1024-pixel segment of a row (blockIdx.x), row blockIdx.y of image blockIdx.z.  The segment's 3072 colour
// bytes are read as coalesced dwords from the dword boundary at or below its start (a row of any stride may start at any
// byte; a dword that holds one byte of the row never crosses a page) into LDS; lane t then takes its 12 bytes from there at
// the row's byte offset (three dwords shifted across dword boundaries) and writes pixels 4t .. 4t + 3 as one dword - bytes
// at the row's tail and where the gray row is not dword-aligned.
__global__ __launch_bounds__(256) void k_bgr2gray(const uint8_t* __restrict__ bgr, int bgr_stride, size_t bgr_frame,
                                                  uint8_t* __restrict__ gray, int gray_pitch, size_t gray_frame, int W) {
  __shared__ uint32_t seg[BGR_LDS_DW];
  const int t = threadIdx.x, x0 = blockIdx.x * BGR_PX;
  const int npx = min(BGR_PX, W - x0);
  const uint8_t* src = bgr + blockIdx.z * bgr_frame + (size_t)blockIdx.y * bgr_stride + 3 * (size_t)x0;
  const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 3);
  const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src - mis);
  const int ndw = (mis + 3 * npx + 3) >> 2;
  for (int k = t; k < ndw; k += 256) seg[k] = s32[k];
  __syncthreads();
  const int p = 4 * t;
  if (p >= npx) return;
  const int o = mis + 3 * p, q = o >> 2, sh = 8 * (o & 3);
  const uint32_t w0 = seg[q], w1 = seg[q + 1], w2 = seg[q + 2], w3 = seg[q + 3];
  auto cat = [sh](uint32_t lo, uint32_t hi) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> sh); };
  const uint32_t d0 = cat(w0, w1), d1 = cat(w1, w2), d2 = cat(w2, w3);   // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3 (low byte first)
  const uint32_t g0 = bgr_gray(d0 & 255u, (d0 >> 8) & 255u, (d0 >> 16) & 255u);
  const uint32_t g1 = bgr_gray(d0 >> 24, d1 & 255u, (d1 >> 8) & 255u);
  const uint32_t g2 = bgr_gray((d1 >> 16) & 255u, d1 >> 24, d2 & 255u);
  const uint32_t g3 = bgr_gray((d2 >> 8) & 255u, (d2 >> 16) & 255u, d2 >> 24);
  const uint32_t packed = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
  uint8_t* dst = gray + blockIdx.z * gray_frame + (size_t)blockIdx.y * gray_pitch + x0 + p;
  if (p + 4 <= npx && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
    *reinterpret_cast<uint32_t*>(dst) = packed;
  } else {
    const int nv = min(4, npx - p);
    for (int k = 0; k < nv; ++k) dst[k] = (uint8_t)(packed >> (8 * k));
  }
}

// Colour staging of a context, allocated by the first colour call that needs it (a context that never sees colour has none).
struct SvoColour {
  uint8_t* d_pair = nullptr;   // svo_track_frame_bgr: the colour pair in HBM (left, then right), H rows of pair_pitch bytes each
  uint8_t* h_pair = nullptr;   //   and its pinned staging, same layout
  int pair_pitch = 0;
  uint8_t* d_gray = nullptr;   // svo_track_batch_bgr_dev: max_batch left grays, then max_batch right grays, H x stage_pitch each
  hipEvent_t gray_free[4] = {nullptr, nullptr, nullptr, nullptr};   // the readers of d_gray in the last call are done with it
  int n_free = 0;
  uint8_t* d_tmp = nullptr;    // svo_bgr_to_gray: device copies of the caller's images (grown on demand)
  size_t tmp_bytes = 0;
};

SvoColour* colour_of(svo_ctx* ctx) {
  if (!ctx->colour) ctx->colour = new SvoColour();
  return reinterpret_cast<SvoColour*>(ctx->colour);
}

}  // namespace

void svo_launch_bgr2gray(hipStream_t st, const uint8_t* bgr, int bgr_stride, size_t bgr_frame, uint8_t* gray, int gray_pitch,
                         size_t gray_frame, int W, int H, int n) {
  if (W < 1 || H < 1 || n < 1) return;
  const dim3 grid((unsigned)((W + BGR_PX - 1) / BGR_PX), (unsigned)H, (unsigned)n);
  hipLaunchKernelGGL(k_bgr2gray, grid, dim3(256), 0, st, bgr, bgr_stride, bgr_frame, gray, gray_pitch, gray_frame, W);
}

void svo_colour_release(svo_ctx* ctx) {
  SvoColour* c = reinterpret_cast<SvoColour*>(ctx->colour);
  if (!c) return;
  if (c->d_pair) hipFree(c->d_pair);
  if (c->h_pair) hipHostFree(c->h_pair);
  if (c->d_gray) hipFree(c->d_gray);
  if (c->d_tmp) hipFree(c->d_tmp);
  for (hipEvent_t e : c->gray_free) if (e) hipEventDestroy(e);
  delete c;
  ctx->colour = nullptr;
}

extern "C" int svo_bgr_to_gray(svo_ctx* ctx, const uint8_t* bgr, int width, int height, int bgr_stride, uint8_t* gray,
                               int gray_stride) {
  if (!ctx || !bgr || !gray || width < 1 || height < 1 || width > (1 << 20) || height > 65535 || bgr_stride < 3 * width ||
      gray_stride < width)
    return SVO_E_INVALID;
  hipSetDevice(ctx->device);
  { const int rcq = svo_track_quiesce(ctx); if (rcq) return rcq; }
  SvoColour* c = colour_of(ctx);
  // the caller's rows keep their stride (and alignment) on the device: the kernel sees the layout the caller has
  const size_t in_bytes = (size_t)(height - 1) * bgr_stride + 3 * (size_t)width;
  const size_t out_off = (in_bytes + 255) & ~(size_t)255;
  const size_t out_bytes = (size_t)(height - 1) * gray_stride + width;
  if (c->tmp_bytes < out_off + out_bytes) {
    SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (c->d_tmp) hipFree(c->d_tmp);
    c->d_tmp = nullptr; c->tmp_bytes = 0;
    if (hipMalloc(reinterpret_cast<void**>(&c->d_tmp), out_off + out_bytes) != hipSuccess) {
      (void)hipGetLastError();
      ctx->last_error = "svo_bgr_to_gray: hipMalloc";
      return SVO_E_NOMEM;
    }
    c->tmp_bytes = out_off + out_bytes;
  }
  SVO_HIP(ctx, hipMemcpyAsync(c->d_tmp, bgr, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  svo_launch_bgr2gray(ctx->stream, c->d_tmp, bgr_stride, 0, c->d_tmp + out_off, gray_stride, 0, width, height, 1);
  SVO_HIP(ctx, hipGetLastError());
  SVO_HIP(ctx, hipMemcpy2DAsync(gray, gray_stride, c->d_tmp + out_off, gray_stride, width, height, hipMemcpyDeviceToHost, ctx->stream));
  SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVO_OK;
}

extern "C" int svo_track_frame_bgr(svo_ctx* ctx, const uint8_t* bgrL, int strideL, const uint8_t* bgrR, int strideR,
                                   double timestamp, const int32_t* boxes, int n_boxes, svo_track_result* res) {
  (void)timestamp;
  if (!ctx || !bgrL || !bgrR || !res || strideL < 3 * ctx->g.W || strideR < 3 * ctx->g.W || n_boxes < 0 ||
      n_boxes > SVO_MAX_BOXES || (n_boxes > 0 && !boxes))
    return SVO_E_INVALID;
  if (!ctx->d_track || ctx->n_seq != 1) return SVO_E_INVALID;   // svo_track_reset first
  { const int rcd = svo_track_dyn_refuse_single(ctx, "svo_track_frame_bgr"); if (rcd) return rcd; }
  hipSetDevice(ctx->device);
  { const int rcq = svo_track_quiesce(ctx); if (rcq) return rcq; }
  const int W = ctx->g.W, H = ctx->g.H;
  SvoColour* c = colour_of(ctx);
  if (!c->d_pair) {
    const int pitch = (3 * W + 255) & ~255;
    const size_t bytes = 2 * (size_t)H * pitch;
    if (hipMalloc(reinterpret_cast<void**>(&c->d_pair), bytes) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&c->h_pair), bytes) != hipSuccess) {
      (void)hipGetLastError();
      if (c->d_pair) hipFree(c->d_pair);
      c->d_pair = nullptr; c->h_pair = nullptr;
      ctx->last_error = "svo_track_frame_bgr: out of memory for the colour staging";
      return SVO_E_NOMEM;
    }
    memset(c->h_pair, 0, bytes);
    c->pair_pitch = pitch;
  }
  // rows gathered into the pinned staging, one linear upload (svo_upload_image's reasoning: a 2-D copy from pageable memory
  // is slow); the previous call synchronised, so the staging is free
  const size_t img = (size_t)H * c->pair_pitch;
  const uint8_t* src[2] = {bgrL, bgrR};
  const int stride[2] = {strideL, strideR};
  for (int side = 0; side < 2; ++side)
    for (int y = 0; y < H; ++y) memcpy(c->h_pair + side * img + (size_t)y * c->pair_pitch, src[side] + (size_t)y * stride[side], 3 * (size_t)W);
  SVO_HIP(ctx, hipMemcpyAsync(c->d_pair, c->h_pair, 2 * img, hipMemcpyHostToDevice, ctx->stream));
  // the gray of both images into the staging slots svo_track_frame uploads to; from there on the gray path's kernels
  svo_launch_bgr2gray(ctx->stream, c->d_pair, c->pair_pitch, img, ctx->d_stage, ctx->stage_pitch, (size_t)H * ctx->stage_pitch, W, H, 2);
  return svo_track_frame_staged(ctx, boxes, n_boxes, res, c->d_pair, c->d_pair + img, c->pair_pitch);
}

namespace {
// the gray staging of the device-fed colour entries (max_batch left grays, then max_batch right grays), made by the first of them
int gray_staging(svo_ctx* ctx, SvoColour* c, const char* who) {
  if (c->d_gray) return SVO_OK;
  const size_t img = (size_t)ctx->g.H * ctx->stage_pitch;
  { const int rcq = svo_track_quiesce(ctx); if (rcq) return rcq; }
  if (hipMalloc(reinterpret_cast<void**>(&c->d_gray), 2 * (size_t)ctx->max_batch * img) != hipSuccess) {
    (void)hipGetLastError();
    c->d_gray = nullptr;
    ctx->last_error = std::string(who) + ": out of memory for the gray staging";
    return SVO_E_NOMEM;
  }
  // (rows are W bytes wide in a pitch of stage_pitch: the padding is never read as image content, but keep it defined)
  SVO_HIP(ctx, hipMemsetAsync(c->d_gray, 0, 2 * (size_t)ctx->max_batch * img, ctx->stream));
  SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 4; ++k)
    if (!c->gray_free[k]) SVO_HIP(ctx, hipEventCreateWithFlags(&c->gray_free[k], hipEventDisableTiming));
  c->n_free = 0;
  return SVO_OK;
}
}  // namespace

extern "C" int svo_track_batch_bgr_dev(svo_ctx* ctx, const uint8_t* d_bgrL, const uint8_t* d_bgrR, int stride, int B,
                                       const svo_boxes_dev* boxes, svo_track_result* d_results) {
  if (!ctx || !d_bgrL || !d_bgrR || !d_results || B < 1 || stride < 3 * ctx->g.W) return SVO_E_INVALID;
  if (B > ctx->max_batch) return SVO_E_CAPACITY;
  if (!ctx->d_track || ctx->n_seq != 1) return SVO_E_INVALID;   // svo_track_reset first
  { const int rcd = svo_track_dyn_refuse_single(ctx, "svo_track_batch_bgr_dev"); if (rcd) return rcd; }
  hipSetDevice(ctx->device);
  SvoColour* c = colour_of(ctx);
  const size_t img = (size_t)ctx->g.H * ctx->stage_pitch;
  { const int rcg = gray_staging(ctx, c, "svo_track_batch_bgr_dev"); if (rcg) return rcg; }
  uint8_t* gL = c->d_gray;
  uint8_t* gR = c->d_gray + (size_t)ctx->max_batch * img;
  SvoBgrSrc src;
  src.L = d_bgrL; src.R = d_bgrR; src.stride = stride; src.convert = true;
  src.wait = c->gray_free; src.n_wait = c->n_free;
  int rc = svo_track_batch_fed(ctx, gL, gR, ctx->stage_pitch, B, boxes, d_results, nullptr, &src);
  if (rc) return rc;
  // who read the gray staging: the front-end stream (sparse depth), the dense stage's streams and the main stream otherwise -
  // the next call's conversion waits for them
  int nf = 0;
  if (ctx->opt_depth_source == 0) {
    SVO_HIP(ctx, hipEventRecord(c->gray_free[nf++], ctx->stream_fe_batch));
  } else {
    if (ctx->stream_dense) SVO_HIP(ctx, hipEventRecord(c->gray_free[nf++], ctx->stream_dense));
    if (ctx->stream_elas_a) SVO_HIP(ctx, hipEventRecord(c->gray_free[nf++], ctx->stream_elas_a));
    SVO_HIP(ctx, hipEventRecord(c->gray_free[nf++], ctx->stream));
  }
  c->n_free = nf;
  return SVO_OK;
}

// svo_track_multi_step_dev for n_seq BGR pairs: their gray goes to the same staging, on the stream the step's front end runs on
// (svo_track_multi_step_fed); the staging's readers - that front end, and the copy the dynamic-keypoint loop takes of the left
// grays with colour = 0 - are what the next colour call's conversion waits for
extern "C" int svo_track_multi_step_bgr_dev(svo_ctx* ctx, const uint8_t* d_bgrL, const uint8_t* d_bgrR, int stride, int n_seq,
                                            const svo_boxes_dev* boxes, svo_track_result* d_results) {
  if (!ctx || !d_bgrL || !d_bgrR || !d_results || stride < 3 * ctx->g.W) return SVO_E_INVALID;
  if (!ctx->d_track || n_seq != ctx->n_seq) return SVO_E_INVALID;   // svo_track_multi_reset(n_seq) first
  { const int rcc = svo_track_multi_step_check(ctx, "svo_track_multi_step_bgr_dev", true); if (rcc) return rcc; }
  hipSetDevice(ctx->device);
  SvoColour* c = colour_of(ctx);
  { const int rcg = gray_staging(ctx, c, "svo_track_multi_step_bgr_dev"); if (rcg) return rcg; }
  const size_t img = (size_t)ctx->g.H * ctx->stage_pitch;
  SvoBgrSrc src;
  src.L = d_bgrL; src.R = d_bgrR; src.stride = stride; src.convert = true;
  src.wait = c->gray_free; src.n_wait = c->n_free;
  src.done = c->gray_free[3];   // (never among the events waited for: at most three were recorded by a batched call, one by a step)
  const int rc = svo_track_multi_step_fed(ctx, c->d_gray, c->d_gray + (size_t)ctx->max_batch * img,
                                          ctx->stage_pitch, n_seq, boxes, d_results, &src);
  if (rc) return rc;
  std::swap(c->gray_free[0], c->gray_free[3]);
  c->n_free = 1;
  return SVO_OK;
}
