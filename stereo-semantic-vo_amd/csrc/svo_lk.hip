// svo_lk.hip - sparse pyramidal Lucas-Kanade (svo_lk_*): cv::calcOpticalFlowPyrLK as the reference's Tracking::Track names it
// (src/Tracking.cc:189-223) with its default arguments, after the written contract of DESIGN.md section 8 "LK": on 8-bit
// single-channel images, and (the _bgr entries) on the 8UC3 BGR images the reference's call is made on.
//   k_lk_pyrdown   one pyramid level of every frame of a batch: [1 4 6 4 1]^2, reflect-101, tile + halo in LDS, separable;
//                  CN interleaved channels, each on its own (one channel of one frame per blockIdx.z)
//   k_lk_scharr    one level's (dx, dy) int16 pairs of every frame that is some pair's previous image, per channel
//   k_lk_track     one wavefront per point, all levels in one launch: the 441 window pixels are 7 per lane, the I patch and both
//                  derivative patches stay in registers over the iterations, the window sums are exact integers reduced on DPP,
//                  the float tail is computed by every lane alike.  One template on the channel count, two instantiations:
//                  <1> keeps an I value per register, <3> holds a lane's 21 samples with two I values to a register
//   k_lk_compact   order-preserving erase of the status-0 points, then a frame's seeds appended (svo_lk_chain_dev)
// Compiled with -ffp-contract=off like the rest of the library: every float operation of the tail rounds once.
#include <algorithm>

#include "svo_internal.h"
#include "svo_wave.h"

namespace {

constexpr int LK_WIN = 21, LK_NPIX = LK_WIN * LK_WIN, LK_MAX_COUNT = 30;
constexpr int LK_MAX_DIM = 4096, LK_MAX_PTS = 4096, LK_MAX_FRAMES = 4096;   // (frames: gridDim.z of the level launches, 2 B launches of the chain)
constexpr int LK_PD_TX = 32, LK_PD_TY = 8;                       // k_lk_pyrdown: output tile of a 256-thread workgroup
constexpr int LK_PD_SW = 2 * LK_PD_TX + 3, LK_PD_SH = 2 * LK_PD_TY + 3;

// Level `level` of a w0 x h0 image: its size, its byte offset in a frame's pyramid slot (levels >= 1; level 0 is the caller's
// image) and its entry offset in a frame's derivative slot (levels >= 0)
struct LkLevel { int w, h; size_t ioff, doff; };
__host__ __device__ inline LkLevel lk_level(int w0, int h0, int level) {
  LkLevel L{w0, h0, 0, 0};
  for (int l = 0; l < level; ++l) {
    const size_t px = (size_t)L.w * L.h;
    L.doff += px;
    if (l >= 1) L.ioff += px;
    L.w = (L.w + 1) >> 1; L.h = (L.h + 1) >> 1;
  }
  return L;
}

// BORDER_REFLECT_101 for |i| < n and i <= 2 n - 2
__device__ __forceinline__ int lk_reflect(int i, int n) {
  i = abs(i);
  return i >= n ? 2 * (n - 1) - i : i;
}

template <int CN>
__global__ __launch_bounds__(256) void k_lk_pyrdown(const uint8_t* __restrict__ src, int spitch, size_t sframe, int sw, int sh,
                                                    uint8_t* __restrict__ dst, size_t dframe, int dw, int dh) {
  __shared__ uint8_t tile[LK_PD_SH][LK_PD_SW + 1];
  __shared__ uint16_t hsum[LK_PD_SH][LK_PD_TX];
  const int fr = blockIdx.z / CN, ch = blockIdx.z - fr * CN;
  src += fr * sframe + ch; dst += fr * dframe + ch;
  const int tid = threadIdx.y * LK_PD_TX + threadIdx.x;
  const int x0 = 2 * blockIdx.x * LK_PD_TX - 2, y0 = 2 * blockIdx.y * LK_PD_TY - 2;
  // (a tile that hangs over the right or lower edge reaches past what one reflection covers: those source pixels feed no stored
  // output, the clamp only keeps their reads inside the image)
  for (int i = tid; i < LK_PD_SH * LK_PD_SW; i += 256) {
    const int ty = i / LK_PD_SW, tx = i - ty * LK_PD_SW;
    const int sx = min(max(lk_reflect(x0 + tx, sw), 0), sw - 1), sy = min(max(lk_reflect(y0 + ty, sh), 0), sh - 1);
    tile[ty][tx] = src[(size_t)sy * spitch + sx * CN];
  }
  __syncthreads();
  for (int i = tid; i < LK_PD_SH * LK_PD_TX; i += 256) {
    const int ty = i / LK_PD_TX, tx = i - ty * LK_PD_TX;
    const uint8_t* r = &tile[ty][2 * tx];
    hsum[ty][tx] = (uint16_t)(r[0] + 4 * r[1] + 6 * r[2] + 4 * r[3] + r[4]);
  }
  __syncthreads();
  const int ox = blockIdx.x * LK_PD_TX + threadIdx.x, oy = blockIdx.y * LK_PD_TY + threadIdx.y;
  if (ox >= dw || oy >= dh) return;
  const int ty = 2 * threadIdx.y, tx = threadIdx.x;
  const int v = hsum[ty][tx] + 4 * hsum[ty + 1][tx] + 6 * hsum[ty + 2][tx] + 4 * hsum[ty + 3][tx] + hsum[ty + 4][tx];
  dst[((size_t)oy * dw + ox) * CN] = (uint8_t)((v + 128) >> 8);
}

// dx = [3 10 3]^T x [-1 0 1], dy = [-1 0 1]^T x [3 10 3], neighbours reflect-101 inside the level; dx in the low half-word.
// One thread per sample of the w * CN a row holds: channel c of pixel x has entry x * CN + c, its neighbours are channel c too.
template <int CN>
__global__ __launch_bounds__(256) void k_lk_scharr(const uint8_t* __restrict__ img, int pitch, size_t iframe, int w, int h,
                                                   uint32_t* __restrict__ der, size_t dframe) {
  const int xs = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (xs >= w * CN || y >= h) return;
  const int px = xs / CN, ch = xs - px * CN;
  img += blockIdx.z * iframe; der += blockIdx.z * dframe;
  const int x = xs, xm = lk_reflect(px - 1, w) * CN + ch, xp = lk_reflect(px + 1, w) * CN + ch, ym = lk_reflect(y - 1, h), yp = lk_reflect(y + 1, h);
  const uint8_t *r0 = img + (size_t)ym * pitch, *r1 = img + (size_t)y * pitch, *r2 = img + (size_t)yp * pitch;
  const int a = r0[xm], b = r0[x], c = r0[xp], d = r1[xm], f = r1[xp], g = r2[xm], k = r2[x], l = r2[xp];
  const int dx = 3 * (c - a) + 10 * (f - d) + 3 * (l - g);
  const int dy = 3 * (g - a) + 10 * (k - b) + 3 * (l - c);
  der[(size_t)y * w * CN + x] = (uint32_t)(dx & 0xffff) | ((uint32_t)dy << 16);
}

struct LkW { int w00, w01, w10, w11; };
// cvRound of the float32 products (v_cvt_i32_f32 rounds half to even), the fourth weight is the remainder to 2^14
__device__ __forceinline__ LkW lk_weights(float a, float b) {
  LkW q;
  q.w00 = __float2int_rn(((1.f - a) * (1.f - b)) * 16384.f);
  q.w01 = __float2int_rn((a * (1.f - b)) * 16384.f);
  q.w10 = __float2int_rn(((1.f - a) * b) * 16384.f);
  q.w11 = 16384 - q.w00 - q.w01 - q.w10;
  return q;
}

// the four weighted taps of the CN channels of pixel (x, y), pixels outside the level read reflect-101 (x, y in [-21, size + 19]):
// one address per tap, the channels are its CN bytes
template <int CN>
__device__ __forceinline__ void lk_tap_img(const uint8_t* __restrict__ img, int pitch, int w, int h, int x, int y, const LkW& q,
                                           int out[CN]) {
  const int x0 = CN * lk_reflect(x, w), x1 = CN * lk_reflect(x + 1, w);
  const uint8_t *r0 = img + (size_t)lk_reflect(y, h) * pitch, *r1 = img + (size_t)lk_reflect(y + 1, h) * pitch;
#pragma unroll
  for (int c = 0; c < CN; ++c) out[c] = r0[x0 + c] * q.w00 + r0[x1 + c] * q.w01 + r1[x0 + c] * q.w10 + r1[x1 + c] * q.w11;
}

template <int CN>
__device__ __forceinline__ void lk_der_at(const uint32_t* __restrict__ der, int w, int h, int x, int y, uint32_t d[CN]) {
  const bool in = (unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h;   // BORDER_CONSTANT 0
  const uint32_t* e = der + ((size_t)y * w + x) * CN;
#pragma unroll
  for (int c = 0; c < CN; ++c) d[c] = in ? e[c] : 0u;
}

__device__ __forceinline__ bool lk_outside(int ix, int iy, int w, int h) { return ix < -LK_WIN || ix >= w || iy < -LK_WIN || iy >= h; }

// exact sum over the wave of int32 partials whose total needs more than 32 bits: the two half-words separately
__device__ __forceinline__ long long lk_wave_sum64(int v) {
  return (long long)wave_sum_i32_dpp(v >> 16) * 65536 + wave_sum_i32_dpp(v & 0xffff);
}
__device__ __forceinline__ float lk_scaled(long long sum) { return (float)(double)sum * (1.f / 1048576.f); }   // one rounding, then 2^-20

// A lane's I patch: sample s = CN k + c is channel c of its pixel k.  One channel: a value per register.  More: I is at most
// 8160, so two values share a register, sample s in half-word s & 1 of v[s >> 1] (set() is called with s ascending).
template <int CN>
struct LkPatch {
  uint32_t v[(7 * CN + 1) / 2];
  __device__ __forceinline__ void set(int s, int val) { if (s & 1) v[s >> 1] |= (uint32_t)val << 16; else v[s >> 1] = (uint32_t)val; }
  __device__ __forceinline__ int get(int s) const { return (int)((v[s >> 1] >> (16 * (s & 1))) & 0xffffu); }
};
template <>
struct LkPatch<1> {
  int v[7];
  __device__ __forceinline__ void set(int s, int val) { v[s] = val; }
  __device__ __forceinline__ int get(int s) const { return v[s]; }
};

// Pairs (fprev0 + blockIdx.y, fprev0 + blockIdx.y + 1) of the resident frames of CN interleaved channels; point list blockIdx.y
// at pts + blockIdx.y * 2 max_pts with counts[blockIdx.y] entries (counts == nullptr: aux = n_fixed); one wavefront per point, every
// lane holds the CN channels of its 7 pixels (7 CN samples).  pyr_bytes and der_entries are a frame's slot sizes (all channels),
// a level's offsets are CN times the one-channel ones.
// SEQS (svo_track_multi_step_dev's loop, many sequences that advance together): the resident frames are two halves of n_seq slots,
// pair blockIdx.y = (fprev0 + blockIdx.y, aux + blockIdx.y) - sequence blockIdx.y's previous and current left image -, counts is
// never null.  Otherwise aux is n_fixed.  The arithmetic is the same code.
template <int CN, bool SEQS = false>
__global__ __launch_bounds__(256) void k_lk_track(const uint8_t* __restrict__ img0, int stride0, size_t frame0,
                                                  const uint8_t* __restrict__ pyr, size_t pyr_bytes, const uint32_t* __restrict__ der,
                                                  size_t der_entries, int w0, int h0, int top, int fprev0,
                                                  const float* __restrict__ pts, const int32_t* __restrict__ counts, int aux,
                                                  int max_pts, float* __restrict__ next, uint8_t* __restrict__ status,
                                                  float* __restrict__ err) {
  // I <= 8160 and |gx|, |gy| <= 4080 (16 * 255).  A lane's int32 partial sums of 7 CN products, and the wave's error sum:
  static_assert(7LL * CN * 4080 * 4080 < (1LL << 31), "s11, s12, s22");                  // three channels: 21 * 4080^2
  static_assert(7LL * CN * 8160 * 4080 < (1LL << 31), "s1, s2");                         // 21 * 8160 * 4080
  static_assert((long long)LK_NPIX * CN * 8160 < (1LL << 24), "err: exact in an int32 and in a float");   // 1323 * 8160
  const int lane = threadIdx.x & 63;
  const int idx = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n = min(SEQS || counts ? counts[blockIdx.y] : aux, max_pts);
  if (idx >= n) return;                                     // (whole wavefronts leave: the DPP sums below see all 64 lanes)
  const size_t slot = (size_t)blockIdx.y * max_pts + idx;
  const int fprev = fprev0 + blockIdx.y, fnext = SEQS ? aux + (int)blockIdx.y : fprev + 1;
  const float ptx = pts[2 * slot], pty = pts[2 * slot + 1];

  int wx[7], wy[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const int p = lane + 64 * k;
    wy[k] = p < LK_NPIX ? p / LK_WIN : 0;                   // (lanes 57..63 have no seventh pixel: they redo pixel 0 with weight 0)
    wx[k] = p < LK_NPIX ? p - wy[k] * LK_WIN : 0;
  }
  const bool seventh = lane + 64 * 6 < LK_NPIX;

  LkPatch<CN> Iv;                                           // the I patch
  int gxy[7 * CN];                                          // the packed (gx, gy) patch
  float ox = 0.f, oy = 0.f, e = 0.f;
  int st = 1;
  for (int level = top; level >= 0; --level) {
    const LkLevel L = lk_level(w0, h0, level);
    const int pitch = level ? CN * L.w : stride0;
    const uint8_t* I = level ? pyr + fprev * pyr_bytes + CN * L.ioff : img0 + fprev * frame0;
    const uint8_t* J = level ? pyr + fnext * pyr_bytes + CN * L.ioff : img0 + fnext * frame0;
    const uint32_t* G = der + fprev * der_entries + CN * L.doff;
    const float sc = 1.f / (float)(1 << level);
    float px = ptx * sc, py = pty * sc;
    if (level == top) { ox = px; oy = py; } else { ox = ox * 2.f; oy = oy * 2.f; }
    px -= 10.f; py -= 10.f;
    const int ipx = (int)floorf(px), ipy = (int)floorf(py);
    if (lk_outside(ipx, ipy, L.w, L.h)) { if (level == 0) st = 0; continue; }
    const LkW q = lk_weights(px - (float)ipx, py - (float)ipy);
    int s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const int x = ipx + wx[k], y = ipy + wy[k];
      int iv[CN];
      lk_tap_img<CN>(I, pitch, L.w, L.h, x, y, q, iv);
      uint32_t d00[CN], d01[CN], d10[CN], d11[CN];
      lk_der_at<CN>(G, L.w, L.h, x, y, d00); lk_der_at<CN>(G, L.w, L.h, x + 1, y, d01);
      lk_der_at<CN>(G, L.w, L.h, x, y + 1, d10); lk_der_at<CN>(G, L.w, L.h, x + 1, y + 1, d11);
#pragma unroll
      for (int c = 0; c < CN; ++c) {
        const int s = CN * k + c;
        Iv.set(s, (iv[c] + 256) >> 9);
        int gx = (int16_t)d00[c] * q.w00 + (int16_t)d01[c] * q.w01 + (int16_t)d10[c] * q.w10 + (int16_t)d11[c] * q.w11;
        int gy = ((int)d00[c] >> 16) * q.w00 + ((int)d01[c] >> 16) * q.w01 + ((int)d10[c] >> 16) * q.w10 + ((int)d11[c] >> 16) * q.w11;
        gx = (gx + 8192) >> 14; gy = (gy + 8192) >> 14;
        if (k == 6 && !seventh) gx = gy = 0;
        gxy[s] = (int)((uint32_t)(gx & 0xffff) | ((uint32_t)gy << 16));
        s11 += gx * gx; s12 += gx * gy; s22 += gy * gy;
      }
    }
    const float A11 = lk_scaled(lk_wave_sum64(s11)), A12 = lk_scaled(lk_wave_sum64(s12)), A22 = lk_scaled(lk_wave_sum64(s22));
    float D = A11 * A22 - A12 * A12;
    const float t = A11 - A22;
    const float min_eig = ((A22 + A11) - sqrtf(t * t + (4.f * A12) * A12)) / 882.f;   // 2 * 21 * 21: without the channel count
    if ((double)min_eig < 1e-4 || D < 1.1920928955078125e-7f) { if (level == 0) st = 0; continue; }
    D = 1.f / D;
    float nx = ox - 10.f, ny = oy - 10.f, pdx = 0.f, pdy = 0.f;
    for (int j = 0; j < LK_MAX_COUNT; ++j) {
      const int inx = (int)floorf(nx), iny = (int)floorf(ny);
      if (lk_outside(inx, iny, L.w, L.h)) { if (level == 0) st = 0; break; }
      const LkW r = lk_weights(nx - (float)inx, ny - (float)iny);
      int s1 = 0, s2 = 0;
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        int jv[CN];
        lk_tap_img<CN>(J, pitch, L.w, L.h, inx + wx[k], iny + wy[k], r, jv);
#pragma unroll
        for (int c = 0; c < CN; ++c) {
          const int s = CN * k + c;
          const int diff = ((jv[c] + 256) >> 9) - Iv.get(s);
          s1 += diff * (int16_t)gxy[s]; s2 += diff * (gxy[s] >> 16);
        }
      }
      const float b1 = lk_scaled(lk_wave_sum64(s1)), b2 = lk_scaled(lk_wave_sum64(s2));
      const float dx = (A12 * b2 - A22 * b1) * D, dy = (A12 * b1 - A11 * b2) * D;
      nx += dx; ny += dy;
      ox = nx + 10.f; oy = ny + 10.f;
      if ((double)dx * dx + (double)dy * dy <= 1e-4) break;
      if (j > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + pdy) < 0.01) { ox -= dx * 0.5f; oy -= dy * 0.5f; break; }
      pdx = dx; pdy = dy;
    }
    if (level == 0 && st) {
      const float fx = ox - 10.f, fy = oy - 10.f;
      const int ifx = (int)floorf(fx), ify = (int)floorf(fy);
      if (lk_outside(ifx, ify, L.w, L.h)) st = 0;
      else {
        const LkW r = lk_weights(fx - (float)ifx, fy - (float)ify);
        int s = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
          int jv[CN];
          lk_tap_img<CN>(J, pitch, L.w, L.h, ifx + wx[k], ify + wy[k], r, jv);
#pragma unroll
          for (int c = 0; c < CN; ++c) {
            const int diff = ((jv[c] + 256) >> 9) - Iv.get(CN * k + c);
            s += (k == 6 && !seventh) ? 0 : abs(diff);
          }
        }
        e = (float)wave_sum_i32_dpp(s) / (float)(32 * LK_NPIX * CN);   // 32 * 21 * cn * 21: 14112 or 42336
      }
    }
  }
  if (lane == 0) {
    next[2 * slot] = ox; next[2 * slot + 1] = oy;
    status[slot] = (uint8_t)st;
    if (err) err[slot] = e;
  }
}

// One workgroup: the tracked points with status != 0 in order, then the frame's seeds while the list has room
__device__ __forceinline__ void lk_compact_body(int* wsum, const float* __restrict__ trk, const uint8_t* __restrict__ st,
                                                const int32_t* __restrict__ n_prev, const float* __restrict__ seeds,
                                                const int32_t* __restrict__ n_seed, int max_seeds, int max_pts,
                                                float* __restrict__ list, int32_t* __restrict__ n_out, int32_t* __restrict__ dropped) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = n_prev ? min(max(*n_prev, 0), max_pts) : 0;
  int base = 0;
  for (int c0 = 0; c0 < n; c0 += 256) {
    const int i = c0 + tid;
    const bool keep = i < n && st[i] != 0;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int q = 0; q < wv; ++q) off += wsum[q];
    if (keep) {
      const int o = off + __popcll(m & ((1ull << lane) - 1));
      list[2 * o] = trk[2 * i]; list[2 * o + 1] = trk[2 * i + 1];
    }
    base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  const int ns = min(max(*n_seed, 0), max_seeds), take = min(ns, max_pts - base);
  for (int j = tid; j < take; j += 256) { list[2 * (base + j)] = seeds[2 * j]; list[2 * (base + j) + 1] = seeds[2 * j + 1]; }
  if (tid == 0) { *n_out = base + take; *dropped = ns - take; }
}
__global__ __launch_bounds__(256) void k_lk_compact(const float* __restrict__ trk, const uint8_t* __restrict__ st,
                                                    const int32_t* __restrict__ n_prev, const float* __restrict__ seeds,
                                                    const int32_t* __restrict__ n_seed, int max_seeds, int max_pts,
                                                    float* __restrict__ list, int32_t* __restrict__ n_out, int32_t* __restrict__ dropped) {
  __shared__ int wsum[4];
  lk_compact_body(wsum, trk, st, n_prev, seeds, n_seed, max_seeds, max_pts, list, n_out, dropped);
}
// The same for many sequences, workgroup q = sequence q: its tracked points at trk + q * 2 max_pts (status at st + q * max_pts), its
// seeds at seeds + q * 2 max_seeds, its list at list + q * 2 max_pts; the counts are arrays over the sequences (n_prev == nullptr:
// no sequence has a previous list)
__global__ __launch_bounds__(256) void k_lk_compact_seqs(const float* __restrict__ trk, const uint8_t* __restrict__ st,
                                                         const int32_t* __restrict__ n_prev, const float* __restrict__ seeds,
                                                         const int32_t* __restrict__ n_seed, int max_seeds, int max_pts,
                                                         float* __restrict__ list, int32_t* __restrict__ n_out,
                                                         int32_t* __restrict__ dropped) {
  __shared__ int wsum[4];
  const size_t q = blockIdx.x;
  lk_compact_body(wsum, trk + q * 2 * max_pts, st + q * max_pts, n_prev ? n_prev + q : nullptr, seeds + q * 2 * max_seeds,
                  n_seed + q, max_seeds, max_pts, list + q * 2 * max_pts, n_out + q, dropped + q);
}

}  // namespace

int lk_top_level(int W, int H, int max_level) {
  int top = 0;
  while (top < max_level) {
    W = (W + 1) >> 1; H = (H + 1) >> 1;
    if (W <= LK_WIN || H <= LK_WIN) break;
    ++top;
  }
  return top;
}

// Parameters, sizes and counts first, on the host alone, so that they are answered the same with or without a context
int lk_check(const svo_lk_params* p, int W, int H, int n, int frames) {
  if (!p) return SVO_E_INVALID;
  svo_lk_params d;
  svo_lk_default_params(&d);
  if (p->winSize != d.winSize || p->maxCount != d.maxCount || p->epsilon != d.epsilon || p->minEigThreshold != d.minEigThreshold ||
      p->maxLevel < 0 || p->maxLevel > 3)
    return SVO_E_INVALID;
  if (W <= LK_WIN || H <= LK_WIN || n < 0 || frames < 1) return SVO_E_INVALID;   // level 0 reflects up to 21 pixels out: it needs 22
  if (W > LK_MAX_DIM || H > LK_MAX_DIM || n > LK_MAX_PTS || frames > LK_MAX_FRAMES) return SVO_E_CAPACITY;
  return SVO_OK;
}

namespace {

int lk_args(svo_ctx* ctx, const char* who, bool pointers, const svo_lk_params* p, int W, int H, int stride, int cn, int n, int frames) {
  int rc = lk_check(p, W, H, n, frames);
  if (rc == SVO_OK && (!ctx || !pointers || stride < cn * W)) rc = SVO_E_INVALID;
  if (rc && ctx)
    ctx->last_error = std::string(who) + (rc == SVO_E_CAPACITY ? ": image larger than 4096 x 4096, more than 4096 points or more than 4096 frames"
                                                               : ": invalid argument or unsupported parameters");
  return rc;
}

template <typename T>
int lk_grow(svo_ctx* ctx, LkArena* A, T** p, size_t* cap, size_t count) {
  if (*cap >= count && *p) return SVO_OK;
  if (A->last) SVO_HIP(ctx, hipStreamSynchronize(A->last));
  if (*p) { hipFree(*p); *p = nullptr; }
  *cap = 0;
  if (hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    ctx->last_error = "svo_lk: device allocation failed";
    return SVO_E_NOMEM;
  }
  *cap = count;
  return SVO_OK;
}

}  // namespace

// the arena `*holder` (made on first use): pyramids and derivatives of `frames` images of cn channels, point buffers for `pts` points
// (0: untouched), level-0 storage for `img_frames` images (0: none)
int lk_reserve_in(svo_ctx* ctx, void** holder, hipStream_t s, int W, int H, int cn, int top, int frames, size_t pts, int img_frames,
                  LkArena** out) {
  if (!*holder) *holder = new LkArena();
  LkArena* A = static_cast<LkArena*>(*holder);
  *out = A;
  if (A->last && A->last != s) SVO_HIP(ctx, hipStreamSynchronize(A->last));   // one user at a time
  A->dbg_cn = 0;
  const LkLevel end = lk_level(W, H, top + 1);
  int rc;
  if ((rc = lk_grow(ctx, A, &A->pyr, &A->cap_pyr, std::max<size_t>(end.ioff, 1) * cn * frames)) ||
      (rc = lk_grow(ctx, A, &A->der, &A->cap_der, end.doff * cn * frames)))
    return rc;
  if (img_frames > 0 && (rc = lk_grow(ctx, A, &A->img, &A->cap_img, (size_t)W * H * cn * img_frames))) return rc;
  if (pts && A->cap_pts < pts) {
    size_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    A->cap_pts = 0;
    if ((rc = lk_grow(ctx, A, &A->pts, &c0, 2 * pts)) || (rc = lk_grow(ctx, A, &A->next, &c1, 2 * pts)) ||
        (rc = lk_grow(ctx, A, &A->err, &c2, pts)) || (rc = lk_grow(ctx, A, &A->status, &c3, pts)))
      return rc;
    A->cap_pts = pts;
  }
  A->last = s;
  return SVO_OK;
}

void lk_arena_free(void** holder) {
  if (!*holder) return;
  LkArena* A = static_cast<LkArena*>(*holder);
  void* bufs[] = {A->img, A->pyr, A->der, A->pts, A->next, A->err, A->status};
  for (void* b : bufs)
    if (b) hipFree(b);
  delete A;
  *holder = nullptr;
}

void lk_slot_px(int W, int H, int top, size_t* pyr_px, size_t* der_px) {
  const LkLevel end = lk_level(W, H, top + 1);
  *pyr_px = end.ioff; *der_px = end.doff;
}

namespace {

// the context's own arena (svo_lk_*)
int lk_reserve(svo_ctx* ctx, hipStream_t s, int W, int H, int cn, int top, int frames, size_t pts, bool host_images, LkArena** out) {
  return lk_reserve_in(ctx, &ctx->lk, s, W, H, cn, top, frames, pts, host_images ? 2 : 0, out);
}

// pyramid levels 1 .. top of `frames` resident images, and the derivatives of levels 0 .. top of frames der_first ..
// der_first + der_frames - 1 (a frame that is no pair's previous image needs none: the tracker reads the previous frame's only)
template <int CN>
void lk_build_cn(hipStream_t s, LkArena* A, const uint8_t* img0, int stride0, size_t frame0, int W, int H, int top, int frames,
                 int der_first, int der_frames) {
  const LkLevel end = lk_level(W, H, top + 1);
  for (int l = 0; l <= top; ++l) {
    const LkLevel L = lk_level(W, H, l);
    const uint8_t* src = l ? A->pyr + CN * L.ioff : img0;
    const int pitch = l ? CN * L.w : stride0;
    const size_t frame = l ? CN * end.ioff : frame0;
    if (der_frames > 0)
      hipLaunchKernelGGL(k_lk_scharr<CN>, dim3((CN * L.w + 63) / 64, (L.h + 3) / 4, der_frames), dim3(64, 4), 0, s,
                         src + der_first * frame, pitch, frame, L.w, L.h, A->der + CN * (der_first * end.doff + L.doff), CN * end.doff);
    if (l < top && frames > 0) {
      const LkLevel N = lk_level(W, H, l + 1);
      hipLaunchKernelGGL(k_lk_pyrdown<CN>, dim3((N.w + LK_PD_TX - 1) / LK_PD_TX, (N.h + LK_PD_TY - 1) / LK_PD_TY, CN * frames),
                         dim3(LK_PD_TX, LK_PD_TY), 0, s, src, pitch, frame, L.w, L.h, A->pyr + CN * N.ioff, CN * end.ioff, N.w, N.h);
    }
  }
}

}  // namespace

void lk_build(hipStream_t s, LkArena* A, int cn, const uint8_t* img0, int stride0, size_t frame0, int W, int H, int top, int frames,
              int der_first, int der_frames) {
  if (cn == 3) lk_build_cn<3>(s, A, img0, stride0, frame0, W, H, top, frames, der_first, der_frames);
  else lk_build_cn<1>(s, A, img0, stride0, frame0, W, H, top, frames, der_first, der_frames);
}

void lk_launch_track(hipStream_t s, LkArena* A, int cn, const uint8_t* img0, int stride0, size_t frame0, int W, int H, int top,
                     int fprev0, int pairs, const float* pts, const int32_t* counts, int n_fixed, int max_pts, float* next,
                     uint8_t* status, float* err) {
  const LkLevel end = lk_level(W, H, top + 1);
  const int waves = counts ? max_pts : n_fixed;
  hipLaunchKernelGGL(cn == 3 ? k_lk_track<3> : k_lk_track<1>, dim3((waves + 3) / 4, pairs), dim3(256), 0, s, img0, stride0, frame0,
                     A->pyr, cn * end.ioff, A->der, cn * end.doff, W, H, top, fprev0, pts, counts, n_fixed, max_pts, next, status,
                     err);
}

void lk_launch_compact(hipStream_t s, const float* trk, const uint8_t* st, const int32_t* n_prev, const float* seeds, const int32_t* n_seed,
                       int max_seeds, int max_pts, float* list, int32_t* n_out, int32_t* dropped) {
  hipLaunchKernelGGL(k_lk_compact, dim3(1), dim3(256), 0, s, trk, st, n_prev, seeds, n_seed, max_seeds, max_pts, list, n_out, dropped);
}

// svo_track_multi_step_dev's loop: `nseq` pairs (fprev0 + q, fnext0 + q) of the arena's slots, sequence q's points at
// pts + q * 2 max_pts with counts[q] entries, results at next + q * 2 max_pts and status + q * max_pts
void lk_launch_track_seqs(hipStream_t s, LkArena* A, int cn, const uint8_t* img0, int stride0, size_t frame0, int W, int H, int top,
                          int fprev0, int fnext0, int nseq, const float* pts, const int32_t* counts, int max_pts, float* next,
                          uint8_t* status) {
  const LkLevel end = lk_level(W, H, top + 1);
  const auto kernel = cn == 3 ? k_lk_track<3, true> : k_lk_track<1, true>;
  hipLaunchKernelGGL(kernel, dim3((max_pts + 3) / 4, nseq), dim3(256), 0, s, img0, stride0,
                     frame0, A->pyr, cn * end.ioff, A->der, cn * end.doff, W, H, top, fprev0, pts, counts, fnext0, max_pts, next, status,
                     (float*)nullptr);
}

void lk_launch_compact_seqs(hipStream_t s, int nseq, const float* trk, const uint8_t* st, const int32_t* n_prev, const float* seeds,
                            const int32_t* n_seed, int max_seeds, int max_pts, float* list, int32_t* n_out, int32_t* dropped) {
  hipLaunchKernelGGL(k_lk_compact_seqs, dim3(nseq), dim3(256), 0, s, trk, st, n_prev, seeds, n_seed, max_seeds, max_pts, list, n_out,
                     dropped);
}

namespace {

int lk_track_pair(svo_ctx* ctx, const char* who, int cn, const uint8_t* prev, const uint8_t* next, int stride, int W, int H,
                  const svo_lk_params* p, const float* pts, int n, float* next_pts, uint8_t* status, float* err) {
  int rc = lk_args(ctx, who, prev && next && (n == 0 || (pts && next_pts && status)), p, W, H, stride, cn, n, 2);
  if (rc || n == 0) return rc;
  SVO_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int top = lk_top_level(W, H, p->maxLevel);
  LkArena* A = nullptr;
  if ((rc = lk_reserve(ctx, s, W, H, cn, top, 2, n, true, &A))) return rc;
  const size_t row = (size_t)cn * W, img = row * H;
  SVO_HIP(ctx, hipMemcpy2DAsync(A->img, row, prev, stride, row, H, hipMemcpyHostToDevice, s));
  SVO_HIP(ctx, hipMemcpy2DAsync(A->img + img, row, next, stride, row, H, hipMemcpyHostToDevice, s));
  SVO_HIP(ctx, hipMemcpyAsync(A->pts, pts, 2 * (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
  lk_build(s, A, cn, A->img, (int)row, img, W, H, top, 2, 0, 1);
  lk_launch_track(s, A, cn, A->img, (int)row, img, W, H, top, 0, 1, A->pts, nullptr, n, n, A->next, A->status, A->err);
  SVO_HIP(ctx, hipGetLastError());
  SVO_HIP(ctx, hipMemcpyAsync(next_pts, A->next, 2 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
  SVO_HIP(ctx, hipMemcpyAsync(status, A->status, n, hipMemcpyDeviceToHost, s));
  if (err) SVO_HIP(ctx, hipMemcpyAsync(err, A->err, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
  SVO_HIP(ctx, hipStreamSynchronize(s));
  A->W = W; A->H = H; A->top = top; A->dbg_cn = cn; A->dbg_next_der = false;
  return SVO_OK;
}

int lk_batch(svo_ctx* ctx, const char* who, int cn, const uint8_t* d_frames, int stride, int W, int H, int B, const svo_lk_params* p,
             const float* d_pts, const int32_t* d_counts, int max_pts, float* d_next, uint8_t* d_status, float* d_err) {
  int rc = lk_args(ctx, who, d_frames && B >= 2 && (max_pts == 0 || (d_pts && d_counts && d_next && d_status)), p, W, H, stride, cn,
                   max_pts, B);
  if (rc || max_pts == 0) return rc;
  SVO_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int top = lk_top_level(W, H, p->maxLevel);
  LkArena* A = nullptr;
  if ((rc = lk_reserve(ctx, s, W, H, cn, top, B, 0, false, &A))) return rc;
  const size_t frame = (size_t)H * stride;
  lk_build(s, A, cn, d_frames, stride, frame, W, H, top, B, 0, B - 1);
  lk_launch_track(s, A, cn, d_frames, stride, frame, W, H, top, 0, B - 1, d_pts, d_counts, 0, max_pts, d_next, d_status, d_err);
  SVO_HIP(ctx, hipGetLastError());
  SVO_HIP(ctx, hipStreamSynchronize(s));
  return SVO_OK;
}

int lk_chain(svo_ctx* ctx, const char* who, int cn, const uint8_t* d_frames, int stride, int W, int H, int B, const svo_lk_params* p,
             const float* d_seeds, const int32_t* d_seed_counts, int max_seeds, int max_pts, float* d_lists, int32_t* d_list_counts,
             int32_t* d_dropped) {
  int rc = lk_args(ctx, who,
                   d_frames && B >= 1 && max_seeds >= 0 && max_pts >= 1 && d_seeds && d_seed_counts && d_lists && d_list_counts && d_dropped,
                   p, W, H, stride, cn, std::max(max_pts, max_seeds), B);
  if (rc) return rc;
  SVO_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int top = lk_top_level(W, H, p->maxLevel);
  LkArena* A = nullptr;
  if ((rc = lk_reserve(ctx, s, W, H, cn, top, B, max_pts, false, &A))) return rc;
  const size_t frame = (size_t)H * stride;
  lk_build(s, A, cn, d_frames, stride, frame, W, H, top, B, 0, B - 1);
  for (int f = 0; f < B; ++f) {                             // enqueued back to back: the counts never come to the host
    float* list = d_lists + (size_t)f * 2 * max_pts;
    if (f)
      lk_launch_track(s, A, cn, d_frames, stride, frame, W, H, top, f - 1, 1, list - 2 * (size_t)max_pts, d_list_counts + f - 1, 0,
                      max_pts, A->next, A->status, nullptr);
    hipLaunchKernelGGL(k_lk_compact, dim3(1), dim3(256), 0, s, A->next, A->status, f ? d_list_counts + f - 1 : nullptr,
                       d_seeds + (size_t)f * 2 * max_seeds, d_seed_counts + f, max_seeds, max_pts, list, d_list_counts + f,
                       d_dropped + f);
  }
  SVO_HIP(ctx, hipGetLastError());
  SVO_HIP(ctx, hipStreamSynchronize(s));
  return SVO_OK;
}

// the probe of the last single-pair call of `cn` channels: a level as h x w x cn bytes, its derivatives as h x w x cn entries
int lk_debug(svo_ctx* ctx, const char* who, int cn, int which, int frame, int level, void* host, int* w, int* h, int* top) {
  if (!ctx || which < 0 || which > 1 || frame < 0 || frame > 1 || level < 0) return SVO_E_INVALID;
  LkArena* A = static_cast<LkArena*>(ctx->lk);
  if (!A || !A->dbg_cn) {
    ctx->last_error = std::string(who) + (cn == 3 ? ": no svo_lk_track_bgr call to report" : ": no svo_lk_track call to report");
    return SVO_E_INVALID;
  }
  if (A->dbg_cn != cn) {
    ctx->last_error = std::string(who) + (cn == 3 ? ": the last LK call was a gray one (svo_lk_debug_level reports it)"
                                                  : ": the last LK call was a colour one (svo_lk_debug_level_bgr reports it)");
    return SVO_E_INVALID;
  }
  if (top) *top = A->top;
  if (level > A->top) { ctx->last_error = std::string(who) + ": level above the effective top level"; return SVO_E_INVALID; }
  const LkLevel L = lk_level(A->W, A->H, level), end = lk_level(A->W, A->H, A->top + 1);
  if (w) *w = L.w;
  if (h) *h = L.h;
  if (!host) return SVO_OK;
  SVO_HIP(ctx, hipSetDevice(ctx->device));
  const size_t px = (size_t)L.w * L.h * cn, img = (size_t)A->W * A->H * cn;
  if (which == 1 && frame == 1 && !A->dbg_next_der) {       // the tracker had no use for them: built here, on demand
    lk_build(ctx->stream, A, cn, A->img, cn * A->W, img, A->W, A->H, A->top, 0, 1, 1);
    SVO_HIP(ctx, hipGetLastError());
    A->dbg_next_der = true;
  }
  if (which == 1)
    SVO_HIP(ctx, svo_memcpy_sync(ctx, host, A->der + cn * (frame * end.doff + L.doff), px * sizeof(uint32_t), hipMemcpyDeviceToHost));
  else
    SVO_HIP(ctx, svo_memcpy_sync(ctx, host, level ? A->pyr + cn * (frame * end.ioff + L.ioff) : A->img + frame * img, px,
                                 hipMemcpyDeviceToHost));
  return SVO_OK;
}

}  // namespace

extern "C" int svo_lk_default_params(svo_lk_params* p) {
  if (!p) return SVO_E_INVALID;
  p->winSize = 21;
  p->maxLevel = 3;
  p->maxCount = 30;
  p->epsilon = 0.01;
  p->minEigThreshold = 1e-4;
  return SVO_OK;
}

extern "C" int svo_lk_track(svo_ctx* ctx, const uint8_t* prev, const uint8_t* next, int stride, int W, int H, const svo_lk_params* p,
                            const float* pts, int n, float* next_pts, uint8_t* status, float* err) {
  return lk_track_pair(ctx, "svo_lk_track", 1, prev, next, stride, W, H, p, pts, n, next_pts, status, err);
}
extern "C" int svo_lk_track_bgr(svo_ctx* ctx, const uint8_t* prev, const uint8_t* next, int stride, int W, int H,
                                const svo_lk_params* p, const float* pts, int n, float* next_pts, uint8_t* status, float* err) {
  return lk_track_pair(ctx, "svo_lk_track_bgr", 3, prev, next, stride, W, H, p, pts, n, next_pts, status, err);
}

extern "C" int svo_lk_batch_dev(svo_ctx* ctx, const uint8_t* d_frames, int stride, int W, int H, int B, const svo_lk_params* p,
                                const float* d_pts, const int32_t* d_counts, int max_pts, float* d_next, uint8_t* d_status,
                                float* d_err) {
  return lk_batch(ctx, "svo_lk_batch_dev", 1, d_frames, stride, W, H, B, p, d_pts, d_counts, max_pts, d_next, d_status, d_err);
}
extern "C" int svo_lk_batch_bgr_dev(svo_ctx* ctx, const uint8_t* d_frames, int stride, int W, int H, int B, const svo_lk_params* p,
                                    const float* d_pts, const int32_t* d_counts, int max_pts, float* d_next, uint8_t* d_status,
                                    float* d_err) {
  return lk_batch(ctx, "svo_lk_batch_bgr_dev", 3, d_frames, stride, W, H, B, p, d_pts, d_counts, max_pts, d_next, d_status, d_err);
}

extern "C" int svo_lk_chain_dev(svo_ctx* ctx, const uint8_t* d_frames, int stride, int W, int H, int B, const svo_lk_params* p,
                                const float* d_seeds, const int32_t* d_seed_counts, int max_seeds, int max_pts, float* d_lists,
                                int32_t* d_list_counts, int32_t* d_dropped) {
  return lk_chain(ctx, "svo_lk_chain_dev", 1, d_frames, stride, W, H, B, p, d_seeds, d_seed_counts, max_seeds, max_pts, d_lists,
                  d_list_counts, d_dropped);
}
extern "C" int svo_lk_chain_bgr_dev(svo_ctx* ctx, const uint8_t* d_frames, int stride, int W, int H, int B, const svo_lk_params* p,
                                    const float* d_seeds, const int32_t* d_seed_counts, int max_seeds, int max_pts, float* d_lists,
                                    int32_t* d_list_counts, int32_t* d_dropped) {
  return lk_chain(ctx, "svo_lk_chain_bgr_dev", 3, d_frames, stride, W, H, B, p, d_seeds, d_seed_counts, max_seeds, max_pts, d_lists,
                  d_list_counts, d_dropped);
}

extern "C" int svo_lk_debug_level(svo_ctx* ctx, int which, int frame, int level, void* host, int* w, int* h, int* top) {
  return lk_debug(ctx, "svo_lk_debug_level", 1, which, frame, level, host, w, h, top);
}
extern "C" int svo_lk_debug_level_bgr(svo_ctx* ctx, int which, int frame, int level, void* host, int* w, int* h, int* top) {
  return lk_debug(ctx, "svo_lk_debug_level_bgr", 3, which, frame, level, host, w, h, top);
}

void svo_lk_release(svo_ctx* ctx) {
  if (ctx) lk_arena_free(&ctx->lk);
}
