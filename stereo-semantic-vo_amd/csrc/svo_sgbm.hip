// svo_sgbm.hip - semi-global block matching on the device: the reference's third dense solver (src/frame.cc:94-120, the body
// of frame::ElasMatch: cv::StereoSGBM::create(0, 16, 3) with a fixed parameter set, compute, convertTo(CV_32F, 1/16)).
// The algorithm is the written contract of include/svo.h ("semi-global block matching") and DESIGN.md section 8 - 8-bit gray,
// five directions, one pass, then the left-right check and the speckle filter - all integer, bit-exact against the numpy
// restatement tests/sgbm_ref.py.  gfx950 only.
//
// Volumes are [y][x][d] int16 (x < D never written or read).  Per pair:
//   k_sgbm_hsum     prefilter + Birchfield-Tomasi cost + the 9 columns of the block sum, one workgroup per row (planes in LDS)
//   k_sgbm_vsum     the 9 rows of the block sum                                                      -> C
//   k_sgbm_paths    directions 0 / 2, then 1 / 3: one lane group per 1-D path, d across the lanes     -> A = L0 + L1, B = L2 + L3
//   k_sgbm_winner   direction 4 along the rows, S4 = sat16(A + B), S = sat16(S4 + L4), winner,
//                   uniqueness, subpixel, right-image bids (atomicMin on (minS, W-1-x))               -> disp1, bids
//   k_sgbm_lr       left-right check
//   k_sgbm_cc_*     speckles: union-find over the pixels' right / lower edges, sizes, removal, float map
// Paths are independent: no hand-over between workgroups, no fence inside a kernel.
//
// The cost and path stages are templates on the channel count CN (DESIGN.md section 8 "f-4 SGBM: colour").  CN = 1 is the gray
// solver above, unchanged.  CN = 3 takes interleaved 8UC3 rows: k_sgbm_hsum makes one pass per channel over the same four LDS
// planes and accumulates into T; P1 and P2 are three times gray's; C is the low 16 bits of the true block sum; the carried
// Lp and m are wrapped to int16 while the unwrapped int32 step goes into A and B, which are int32 volumes there (so a chunk
// of the arena holds half as many colour pairs).
//
// MODE_HH (DESIGN.md section 8 "f-4 SGBM: MODE_HH"; the restatement is tests/sgbm_hh_ref.py): the second pass's directions 5,
// 6 and 7 (predecessors below) run through the same k_sgbm_paths - 5 / 6, then 7 - into two further volumes X = L5 + L7 and
// Y = L6 (two directions are the most an int16 holds; int32 with CN = 3), which the arena gets the first time a context asks
// for the mode; k_sgbm_winner<.., 1> still walks direction 4 along the row and forms S = sat16(S4 + L4 + X + Y).
#include "svo_internal.h"

#include <limits.h>

#include <algorithm>

namespace {

constexpr int SGBM_P1 = 648, SGBM_P2 = 2592, SGBM_CAP = 63, SGBM_R = 4;
constexpr int SGBM_CHUNK = 4;          // pairs of a batch that share the arena's volumes
constexpr int SGBM_CHUNK_BGR = 2;      // colour: A and B are int32, so the same bytes hold half as many pairs
constexpr int SGBM_MAX_W = 3072;       // k_sgbm_hsum keeps 20 bytes per column in LDS
constexpr int SGBM_MAX_H = 4096;
constexpr int16_t SGBM_INVALID = -16;

struct SgbmArena {
  int16_t *C = nullptr, *A = nullptr, *B = nullptr;       // cap_n volumes each (colour calls use A and B as int32 volumes of half as many pairs)
  int16_t *X = nullptr, *Y = nullptr;                     // MODE_HH: L5 + L7 and L6, like A and B; null until a call asks for the mode
  int16_t *dbgS4 = nullptr, *dbgS = nullptr;              // svo_sgbm_process only (one volume each)
  int16_t *disp1 = nullptr, *dbg_disp2 = nullptr, *dbg_lr = nullptr;
  uint32_t* bid = nullptr;
  int32_t *label = nullptr, *root = nullptr, *cnt = nullptr;
  uint8_t* img = nullptr;                                 // svo_sgbm_process: the uploaded pair
  float* dispf = nullptr;                                 // svo_sgbm_process: the float map
  size_t cap_vol = 0, cap_pix = 0, cap_img_bytes = 0;     // elements per image the buffers were made for
  int cap_n = 0;
  bool has_dbg = false, has_hh = false;
  int W = 0, H = 0, D = 0;                                // the last svo_sgbm_process call (svo_sgbm_debug_volume)
  bool dbg_valid = false;
  hipStream_t last = nullptr;
};

__device__ __forceinline__ int sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }
__device__ __forceinline__ int wrap16(int v) { return (int16_t)v; }   // the low 16 bits, sign-extended

template <int CN> struct SgbmAcc { typedef int16_t type; };
template <> struct SgbmAcc<3> { typedef int32_t type; };               // L0 + L1 and L2 + L3 leave int16 with three channels

// Birchfield-Tomasi on two packed (u | u0 << 8 | u1 << 16) entries
__device__ __forceinline__ int bt_cost(uint32_t a, uint32_t b) {
  const int u = a & 255, u0 = (a >> 8) & 255, u1 = a >> 16;
  const int v = b & 255, v0 = (b >> 8) & 255, v1 = b >> 16;
  const int c0 = max(0, max(u - v1, v0 - u));
  const int c1 = max(0, max(v - u1, u0 - v));
  return min(c0, c1);
}

// (I points at channel c of pixel (0, 0); pixels are CN bytes apart)
template <int CN>
__device__ __forceinline__ int prefilter_px(const uint8_t* I, int stride, int W, int H, int x, int y) {
  if (x == 0 || x == W - 1) return SGBM_CAP;
  const uint8_t* r = I + (size_t)y * stride;
  const uint8_t* rm = I + (size_t)max(y - 1, 0) * stride;
  const uint8_t* rp = I + (size_t)min(y + 1, H - 1) * stride;
  const int a = (x + 1) * CN, b = (x - 1) * CN;
  const int v = 2 * ((int)r[a] - (int)r[b]) + ((int)rm[a] - (int)rm[b]) + ((int)rp[a] - (int)rp[b]);
  return min(max(v, -SGBM_CAP), SGBM_CAP) + SGBM_CAP;
}

// T(x, y, d) = sum over dx of the pixel cost at (clamp(x + dx, D, W - 1), y, d).  Grid (H, pairs), blockDim = D * (256 / D):
// thread -> (column offset, d), so that a wave's stores are contiguous.  LDS: 4 byte planes, then 4 packed planes.
template <int CN>
__global__ void k_sgbm_hsum(const uint8_t* L, const uint8_t* R, int stride, size_t frame, int W, int H, int D, int16_t* T, size_t vol) {
  extern __shared__ uint32_t lds[];
  uint32_t* pk = lds;                                        // [4][W]: gradient L, gray L, gradient R, gray R
  uint8_t* raw = reinterpret_cast<uint8_t*>(lds + 4 * (size_t)W);   // [4][W]
  const int y = blockIdx.x;
  L += blockIdx.y * frame; R += blockIdx.y * frame; T += blockIdx.y * vol;
  const int d = threadIdx.x % D, cols = blockDim.x / D;
  // CN = 3: one pass per channel over the same planes; a thread adds to the T entries it wrote itself in the pass before
  // (the row's sum is at most 9 * 567 = 5103)
#pragma unroll
  for (int c = 0; c < CN; ++c) {
    if (c) __syncthreads();                                  // the pass before has read the planes
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
      raw[x] = (uint8_t)prefilter_px<CN>(L + c, stride, W, H, x, y);
      raw[W + x] = L[(size_t)y * stride + x * CN + c];
      raw[2 * W + x] = (uint8_t)prefilter_px<CN>(R + c, stride, W, H, x, y);
      raw[3 * W + x] = R[(size_t)y * stride + x * CN + c];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * W; i += blockDim.x) {
      const int x = i % W;
      const uint8_t* p = raw + (i - x);
      const int u = p[x];
      const int ul = x > 0 ? (u + p[x - 1]) / 2 : u;
      const int ur = x < W - 1 ? (u + p[x + 1]) / 2 : u;
      pk[i] = (uint32_t)u | ((uint32_t)min(u, min(ul, ur)) << 8) | ((uint32_t)max(u, max(ul, ur)) << 16);
    }
    __syncthreads();
    for (int x = D + threadIdx.x / D; x < W; x += cols) {
      int sum = 0;
#pragma unroll
      for (int dx = -SGBM_R; dx <= SGBM_R; ++dx) {
        const int xx = min(max(x + dx, D), W - 1), xr = xx - d;
        sum += bt_cost(pk[xx], pk[2 * W + xr]) + (bt_cost(pk[W + xx], pk[3 * W + xr]) >> 2);
      }
      int16_t* t = &T[((size_t)y * W + x) * D + d];
      *t = (int16_t)(c ? *t + sum : sum);
    }
  }
}

// C(x, y, d) = sum over dy of T(x, clamp(y + dy, 0, H - 1), d).  Grid (ceil((W - D) * D / 256), H, pairs).
// The conversion keeps the low 16 bits: the value itself in gray (at most 15 309), wrap16 of the true sum with three channels.
__global__ void k_sgbm_vsum(const int16_t* T, int16_t* C, int W, int H, int D, size_t vol) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (e >= (W - D) * D) return;
  T += blockIdx.z * vol; C += blockIdx.z * vol;
  const size_t row = (size_t)W * D, off = (size_t)D * D + e;
  int sum = 0;
#pragma unroll
  for (int dy = -SGBM_R; dy <= SGBM_R; ++dy) sum += T[(size_t)min(max(y + dy, 0), H - 1) * row + off];
  C[(size_t)y * row + off] = (int16_t)sum;
}

// Path p of direction `dir` (predecessor offsets (-1,0), (-1,-1), (0,-1), (+1,-1), (+1,0), and MODE_HH's (+1,+1), (0,+1), (-1,+1)):
// first pixel, step, length (0: no such path).  Directions 5 to 7 are 3 to 1 upside down: first pixel in the bottom row or a side
// column, sy = -1.
__device__ __forceinline__ void sgbm_path(int dir, int p, int W, int H, int D, int& x, int& y, int& sx, int& sy, int& len) {
  const int nx = W - D;
  len = 0; x = D; y = 0; sx = 0; sy = 0;
  if (p < 0) return;
  const bool up = dir > 4;                       // rows bottom to top
  if (dir == 0 || dir == 4) {
    if (p >= H) return;
    y = p; x = dir == 0 ? D : W - 1; sx = dir == 0 ? 1 : -1; len = nx;
  } else if (dir == 2 || dir == 6) {
    if (p >= nx) return;
    x = D + p; y = up ? H - 1 : 0; sy = up ? -1 : 1; len = H;
  } else {
    if (p >= nx + H - 1) return;
    const bool right = dir == 1 || dir == 7;     // columns left to right
    sy = up ? -1 : 1; sx = right ? 1 : -1;
    int k = 0;                                   // rows between the first pixel and the row the direction starts from
    if (p < nx) x = D + p; else { x = right ? D : W - 1; k = p - nx + 1; }
    y = up ? H - 1 - k : k;
    len = min(right ? W - x : x - D + 1, H - k);
  }
}

template <int G>
__device__ __forceinline__ int group_min(int v) {
#pragma unroll
  for (int o = G / 2; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, G));
  return v;
}

// One step of L(p, d) = C + min(Lp[d], Lp[d-1] + P1, Lp[d+1] + P1, m + P2) - (m + P2) on a lane group (lane = d; lanes >= D idle)
// (P1, P2 = CN times gray's.  With CN = 3 the caller carries Lp and m wrapped to int16; the result is the unwrapped int32.)
template <int G, int CN>
__device__ __forceinline__ int sgbm_step(int c, int Lp, int m, int d, int D) {
  constexpr int P1 = SGBM_P1 * CN, P2 = SGBM_P2 * CN;
  const int lo = __shfl_up(Lp, 1, G), hi = __shfl_down(Lp, 1, G);
  int a = min(Lp, m + P2);
  if (d > 0) a = min(a, lo + P1);
  if (d < D - 1) a = min(a, hi + P1);
  return c + a - (m + P2);
}

// what the next pixel of a path sees of this one's step: the value as stored in a short, and the short of the unwrapped minimum
template <int G, int CN>
__device__ __forceinline__ void sgbm_carry(int v, bool lane, int& Lp, int& m) {
  Lp = CN == 1 ? v : wrap16(v);
  m = group_min<G>(lane ? v : INT_MAX);
  if (CN != 1) m = wrap16(m);
}

// Directions dir0 (blockIdx.y = 0, into out0) and dir1 (blockIdx.y = 1, into out1): written (add = 0) or added to what is there.
// blockDim 256 = 256 / G paths; a wave runs to its longest path, lanes of shorter ones idle (no workgroup barrier in here).
template <int G, int CN>
__global__ void k_sgbm_paths(const int16_t* C, typename SgbmAcc<CN>::type* out0, typename SgbmAcc<CN>::type* out1, int dir0, int dir1,
                             int add, int W, int H, int D, size_t vol) {
  typedef typename SgbmAcc<CN>::type acc_t;
  const int dir = blockIdx.y ? dir1 : dir0;
  acc_t* out = (blockIdx.y ? out1 : out0) + blockIdx.z * vol;
  C += blockIdx.z * vol;
  const int d = threadIdx.x % G, p = blockIdx.x * (blockDim.x / G) + threadIdx.x / G;
  int x, y, sx, sy, len;
  sgbm_path(dir, p, W, H, D, x, y, sx, sy, len);
  int wl = len;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) wl = max(wl, __shfl_xor(wl, o));
  const bool lane = d < D;
  int Lp = 0, m = 0;
  constexpr int U = 4;
  for (int k0 = 0; k0 < wl; k0 += U) {
    int c[U], prev[U];
    size_t idx[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {          // the loads of U steps first: they do not depend on the recurrence
      const bool on = lane && k0 + u < len;
      idx[u] = ((size_t)(y + (k0 + u) * sy) * W + (x + (k0 + u) * sx)) * D + d;
      c[u] = on ? C[idx[u]] : 0;
      prev[u] = (on && add) ? out[idx[u]] : 0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int v = sgbm_step<G, CN>(c[u], Lp, m, d, D);
      if (lane && k0 + u < len) out[idx[u]] = (acc_t)(prev[u] + v);
      sgbm_carry<G, CN>(v, lane, Lp, m);
    }
  }
}

// Direction 4 along row p (right to left), the sums, and the winner of every pixel.  bid: H x W, 0xffffffff = no bid.
// HH = 1 (MODE_HH): X = L5 + L7 and Y = L6 are read beside A and B, and S = sat16(S4 + L4 + X + Y) - one saturation of the
// second pass's four steps added together.  HH = 0: X and Y are null and not touched.
template <int G, int CN, int HH>
__global__ void k_sgbm_winner(const int16_t* C, const typename SgbmAcc<CN>::type* A, const typename SgbmAcc<CN>::type* B,
                              const typename SgbmAcc<CN>::type* X, const typename SgbmAcc<CN>::type* Y, int16_t* dbgS4, int16_t* dbgS, int16_t* disp1,
                              uint32_t* bid, int W, int H, int D, size_t vol, size_t pix) {
  C += blockIdx.z * vol; A += blockIdx.z * vol; B += blockIdx.z * vol;
  if (HH) { X += blockIdx.z * vol; Y += blockIdx.z * vol; }
  disp1 += blockIdx.z * pix; bid += blockIdx.z * pix;
  const int d = threadIdx.x % G, y = blockIdx.x * (blockDim.x / G) + threadIdx.x / G;
  const bool row = y < H, lane = d < D && row;
  const int yy = row ? y : 0;
  if (row) for (int x = d; x < D; x += G) disp1[(size_t)yy * W + x] = SGBM_INVALID;   // columns without a disparity
  const unsigned long long gmask = (G == 64 ? ~0ull : ((1ull << (G & 63)) - 1)) << ((threadIdx.x % 64) / G * G);
  int Lp = 0, m = 0;
  constexpr int U = 4;
  const int len = W - D;
  for (int k0 = 0; k0 < len; k0 += U) {
    int c[U], s4[U], xy[U];
    size_t idx[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool on = lane && k0 + u < len;
      idx[u] = ((size_t)yy * W + (W - 1 - k0 - u)) * D + d;
      c[u] = on ? C[idx[u]] : 0;
      s4[u] = on ? sat16((int)A[idx[u]] + (int)B[idx[u]]) : 0;
      xy[u] = (HH && on) ? (int)X[idx[u]] + (int)Y[idx[u]] : 0;     // gray: at most 3 * 15 309; colour: int32 steps of bounded paths
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool on = lane && k0 + u < len;      // (uniform over the group's lanes below D)
      const int x = W - 1 - k0 - u;
      const int v = sgbm_step<G, CN>(c[u], Lp, m, d, D);
      sgbm_carry<G, CN>(v, lane, Lp, m);
      const int s = HH ? sat16(s4[u] + v + xy[u]) : sat16(s4[u] + v);
      if (on && dbgS) { dbgS4[idx[u]] = (int16_t)s4[u]; dbgS[idx[u]] = (int16_t)s; }
      // first minimum over d ascending: smallest (S, d)
      const int key = group_min<G>(d < D ? (((s + 32768) << 8) | d) : INT_MAX);
      const int minS = (key >> 8) - 32768, best = key & 255;
      const bool rej = d < D && abs(best - d) > 1 && s * 90 < minS * 100;
      const bool rejected = (__ballot(rej) & gmask) != 0;
      const int sm = __shfl(s, max(best - 1, 0), G), sp = __shfl(s, min(best + 1, G - 1), G);
      if (on && d == 0) {
        int out = SGBM_INVALID;
        if (!rejected) {
          out = best * 16;
          if (best > 0 && best < D - 1) {
            const int den = max(sm + sp - 2 * minS, 1);
            out += ((sm - sp) * 16 + den) / (2 * den);   // C division: truncates toward zero
          }
          // lowest minS wins the right-image column, ties to the largest x
          atomicMin(&bid[(size_t)yy * W + (x - best)], ((uint32_t)(minS + 32768) << 16) | (uint32_t)(W - 1 - x));
        }
        disp1[(size_t)yy * W + x] = (int16_t)out;
      }
    }
  }
}

__device__ __forceinline__ int sgbm_disp2(const uint32_t* bid_row, int W, int x2) {
  const uint32_t k = bid_row[x2];
  return k == 0xffffffffu ? -1 : (W - 1 - (int)(k & 0xffff)) - x2;
}

// Left-right check, in place; dbg_disp2 / dbg_lr (may be null): the right-image map and the checked map for svo_sgbm_debug_volume
__global__ void k_sgbm_lr(int16_t* disp1, const uint32_t* bid, int16_t* dbg_disp2, int16_t* dbg_lr, int W, int H, size_t pix) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const size_t i = blockIdx.z * pix + (size_t)y * W + x;
  const uint32_t* brow = bid + blockIdx.z * pix + (size_t)y * W;
  int d1 = disp1[i];
  if (d1 != SGBM_INVALID) {
    int bad = 0;
    const int ab[2] = {d1 >> 4, (d1 + 15) >> 4};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int xa = x - ab[k];
      if (xa >= 0 && xa < W) {
        const int d2 = sgbm_disp2(brow, W, xa);
        if (d2 >= 0 && abs(d2 - ab[k]) > 1) ++bad;
      }
    }
    if (bad == 2) { d1 = SGBM_INVALID; disp1[i] = SGBM_INVALID; }
  }
  if (dbg_disp2) { dbg_disp2[i] = (int16_t)sgbm_disp2(brow, W, x); dbg_lr[i] = (int16_t)d1; }
}

// ---- speckles: components of valid pixels over the edges with |difference| <= 512 ---------------------------------------
__device__ __forceinline__ int cc_load(const int32_t* L, int i) { return __hip_atomic_load(&L[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int cc_find(const int32_t* L, int i) {
  for (int p = cc_load(L, i); p != i; p = cc_load(L, i)) i = p;
  return i;
}
// labels only ever decrease (atomicMin on a root), so a stale read is an ancestor and the returned old value settles each round
__device__ __forceinline__ void cc_unite(int32_t* L, int a, int b) {
  for (;;) {
    a = cc_find(L, a); b = cc_find(L, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[b], a);
    if (old == b) return;
    b = old;
  }
}

__global__ void k_sgbm_cc_init(const int16_t* disp, int32_t* label, int32_t* cnt, int n, size_t pix) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t o = blockIdx.y * pix + i;
  label[o] = disp[o] != SGBM_INVALID ? i : -1;
  cnt[o] = 0;
}

__global__ void k_sgbm_cc_merge(const int16_t* disp, int32_t* label, int W, int H, size_t pix) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  disp += blockIdx.z * pix; label += blockIdx.z * pix;
  const int i = y * W + x, v = disp[i];
  if (v == SGBM_INVALID) return;
  if (x + 1 < W) { const int w = disp[i + 1]; if (w != SGBM_INVALID && abs(w - v) <= 512) cc_unite(label, i, i + 1); }
  if (y + 1 < H) { const int w = disp[i + W]; if (w != SGBM_INVALID && abs(w - v) <= 512) cc_unite(label, i, i + W); }
}

__global__ void k_sgbm_cc_count(const int32_t* label, int32_t* root, int32_t* cnt, int n, size_t pix) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  label += blockIdx.y * pix; root += blockIdx.y * pix; cnt += blockIdx.y * pix;
  int r = -1;
  if (label[i] >= 0) { r = cc_find(label, i); atomicAdd(&cnt[r], 1); }
  root[i] = r;
}

// components of at most 100 pixels go; the float map is disp16 / 16 (invalid: -16 / 16 = -1.0f exactly)
__global__ void k_sgbm_cc_apply(int16_t* disp, const int32_t* root, const int32_t* cnt, float* out, int n, size_t pix) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t o = blockIdx.y * pix + i;
  int v = disp[o];
  const int r = root[o];
  if (r >= 0 && cnt[blockIdx.y * pix + r] <= 100) { v = SGBM_INVALID; disp[o] = SGBM_INVALID; }
  if (out) out[o] = (float)v / 16.0f;
}

int sgbm_check(const svo_sgbm_params* p, int W, int H, int cn = 1, int mode = SVO_SGBM_MODE_SGBM) {
  if (!p) return SVO_E_INVALID;
  if (mode != SVO_SGBM_MODE_SGBM && mode != SVO_SGBM_MODE_HH) return SVO_E_INVALID;
  svo_sgbm_params d;
  if (cn == 3) svo_sgbm_default_params_bgr(H, &d); else svo_sgbm_default_params(H, &d);
  const int D = p->numDisparities;
  if (D != 16 && D != 32 && D != 48 && D != 64) return SVO_E_INVALID;
  if (p->minDisparity != d.minDisparity || p->blockSize != d.blockSize || p->P1 != d.P1 || p->P2 != d.P2 ||
      p->disp12MaxDiff != d.disp12MaxDiff || p->preFilterCap != d.preFilterCap || p->uniquenessRatio != d.uniquenessRatio ||
      p->speckleWindowSize != d.speckleWindowSize || p->speckleRange != d.speckleRange)
    return SVO_E_INVALID;
  if (H < 2 || W <= D + 8) return SVO_E_INVALID;
  if (W > SGBM_MAX_W || H > SGBM_MAX_H) return SVO_E_CAPACITY;
  return SVO_OK;
}

// The parameters and sizes first (host arithmetic only, so that they are answered the same with or without a context or a
// device), then the pointers; the reason goes to the context's last_error when there is one.
int sgbm_args(svo_ctx* ctx, const char* who, bool pointers, const svo_sgbm_params* p, int W, int H, int stride, int cn, int mode) {
  int rc = sgbm_check(p, W, H, cn, mode);
  if (rc == SVO_OK && (!ctx || !pointers || stride < cn * W)) rc = SVO_E_INVALID;
  if (rc && ctx)
    ctx->last_error = std::string(who) + (rc == SVO_E_CAPACITY ? ": image larger than 3072 x 4096"
                                          : mode != SVO_SGBM_MODE_SGBM && mode != SVO_SGBM_MODE_HH
                                              ? ": invalid mode (SVO_SGBM_MODE_SGBM = 0 or SVO_SGBM_MODE_HH = 1)"
                                              : ": invalid argument or unsupported parameters");
  return rc;
}

template <typename T>
int sgbm_alloc(svo_ctx* ctx, T** p, size_t count) {
  if (*p) { hipFree(*p); *p = nullptr; }
  if (hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    ctx->last_error = "svo_sgbm: device allocation failed";
    return SVO_E_NOMEM;
  }
  return SVO_OK;
}

// the context's arena: volumes for n gray pairs of W x H x D (the debug copies and the host path's staging with dbg; img_bytes:
// the uploaded pair).  A colour call of k pairs asks for n = 2 k: its A and B are int32.  hh: the call runs MODE_HH and needs
// X and Y, which are made at the first such call; a growth of the arena leaves them as they are (too small now, has_hh off) and
// the next call with hh makes them again at the new size.  An arena never asked is what it was without the mode.
int sgbm_reserve(svo_ctx* ctx, hipStream_t s, int W, int H, int D, int n, bool dbg, bool hh, SgbmArena** out, size_t img_bytes = 0) {
  if (!ctx->sgbm) ctx->sgbm = new SgbmArena();
  SgbmArena* A = static_cast<SgbmArena*>(ctx->sgbm);
  *out = A;
  if (A->last && A->last != s) SVO_HIP(ctx, hipStreamSynchronize(A->last));   // one user at a time
  const size_t pix = (size_t)W * H, vol = pix * D;
  int rc;
  if (A->cap_vol < vol || A->cap_pix < pix || A->cap_n < n) {
    if (A->last) SVO_HIP(ctx, hipStreamSynchronize(A->last));
    const size_t v = std::max(vol, A->cap_vol), q = std::max(pix, A->cap_pix);
    const size_t m = (size_t)std::max(n, A->cap_n);
    A->cap_vol = A->cap_pix = 0; A->cap_n = 0; A->has_dbg = false; A->has_hh = false; A->dbg_valid = false; A->cap_img_bytes = 0;
    if ((rc = sgbm_alloc(ctx, &A->C, v * m)) || (rc = sgbm_alloc(ctx, &A->A, v * m)) || (rc = sgbm_alloc(ctx, &A->B, v * m)) ||
        (rc = sgbm_alloc(ctx, &A->disp1, q * m)) || (rc = sgbm_alloc(ctx, &A->bid, q * m)) || (rc = sgbm_alloc(ctx, &A->label, q * m)) ||
        (rc = sgbm_alloc(ctx, &A->root, q * m)) || (rc = sgbm_alloc(ctx, &A->cnt, q * m)))
      return rc;
    A->cap_vol = v; A->cap_pix = q; A->cap_n = (int)m;
  }
  if (hh && !A->has_hh) {
    if (A->last) SVO_HIP(ctx, hipStreamSynchronize(A->last));
    if ((rc = sgbm_alloc(ctx, &A->X, A->cap_vol * A->cap_n)) || (rc = sgbm_alloc(ctx, &A->Y, A->cap_vol * A->cap_n))) return rc;
    A->has_hh = true;
  }
  if (dbg && !A->has_dbg) {
    if (A->last) SVO_HIP(ctx, hipStreamSynchronize(A->last));
    if ((rc = sgbm_alloc(ctx, &A->dbgS4, A->cap_vol)) || (rc = sgbm_alloc(ctx, &A->dbgS, A->cap_vol)) ||
        (rc = sgbm_alloc(ctx, &A->dbg_disp2, A->cap_pix)) || (rc = sgbm_alloc(ctx, &A->dbg_lr, A->cap_pix)) ||
        (rc = sgbm_alloc(ctx, &A->img, 2 * A->cap_pix)) || (rc = sgbm_alloc(ctx, &A->dispf, A->cap_pix)))
      return rc;
    A->has_dbg = true;
    A->cap_img_bytes = 2 * A->cap_pix;
  }
  if (dbg && A->cap_img_bytes < img_bytes) {   // a colour pair: three bytes per pixel
    if (A->last) SVO_HIP(ctx, hipStreamSynchronize(A->last));
    A->cap_img_bytes = 0; A->dbg_valid = false;
    if ((rc = sgbm_alloc(ctx, &A->img, img_bytes))) return rc;
    A->cap_img_bytes = img_bytes;
  }
  A->last = s;
  return SVO_OK;
}

template <int G, int CN>
void sgbm_launch_paths(hipStream_t s, SgbmArena* A, int W, int H, int D, int n, size_t vol, size_t pix, bool dbg, int mode) {
  typedef typename SgbmAcc<CN>::type acc_t;
  const int gpb = 256 / G, nx = W - D;
  const int n02 = std::max(H, nx), n13 = nx + H - 1;
  acc_t *a = reinterpret_cast<acc_t*>(A->A), *b = reinterpret_cast<acc_t*>(A->B);
  hipLaunchKernelGGL((k_sgbm_paths<G, CN>), dim3((n02 + gpb - 1) / gpb, 2, n), dim3(256), 0, s, A->C, a, b, 0, 2, 0, W, H, D, vol);
  hipLaunchKernelGGL((k_sgbm_paths<G, CN>), dim3((n13 + gpb - 1) / gpb, 2, n), dim3(256), 0, s, A->C, a, b, 1, 3, 1, W, H, D, vol);
  if (mode == SVO_SGBM_MODE_HH) {
    // directions 5 (into X) and 6 (into Y; its nx paths are the first of the grid's n13), then 7 added to X: every entry with
    // x >= D lies on one path of each direction, so the first launch overwrites what X and Y held
    acc_t *x = reinterpret_cast<acc_t*>(A->X), *y = reinterpret_cast<acc_t*>(A->Y);
    hipLaunchKernelGGL((k_sgbm_paths<G, CN>), dim3((n13 + gpb - 1) / gpb, 2, n), dim3(256), 0, s, A->C, x, y, 5, 6, 0, W, H, D, vol);
    hipLaunchKernelGGL((k_sgbm_paths<G, CN>), dim3((n13 + gpb - 1) / gpb, 1, n), dim3(256), 0, s, A->C, x, x, 7, 7, 1, W, H, D, vol);
    hipLaunchKernelGGL((k_sgbm_winner<G, CN, 1>), dim3((H + gpb - 1) / gpb, 1, n), dim3(256), 0, s, A->C, a, b, x, y, dbg ? A->dbgS4 : nullptr,
                       dbg ? A->dbgS : nullptr, A->disp1, A->bid, W, H, D, vol, pix);
    return;
  }
  hipLaunchKernelGGL((k_sgbm_winner<G, CN, 0>), dim3((H + gpb - 1) / gpb, 1, n), dim3(256), 0, s, A->C, a, b, (const acc_t*)nullptr,
                     (const acc_t*)nullptr, dbg ? A->dbgS4 : nullptr, dbg ? A->dbgS : nullptr, A->disp1, A->bid, W, H, D, vol, pix);
}

// filterSpeckles(disp, -16, 100, 16 * 32) on the n maps in A->disp1, then the float maps (d_disp may be null)
void sgbm_speckles(hipStream_t s, SgbmArena* A, int W, int H, int n, float* d_disp) {
  const size_t pix = (size_t)W * H;
  const dim3 gp(((int)pix + 255) / 256, n);
  hipLaunchKernelGGL(k_sgbm_cc_init, gp, dim3(256), 0, s, A->disp1, A->label, A->cnt, (int)pix, pix);
  hipLaunchKernelGGL(k_sgbm_cc_merge, dim3((W + 255) / 256, H, n), dim3(256), 0, s, A->disp1, A->label, W, H, pix);
  hipLaunchKernelGGL(k_sgbm_cc_count, gp, dim3(256), 0, s, A->label, A->root, A->cnt, (int)pix, pix);
  hipLaunchKernelGGL(k_sgbm_cc_apply, gp, dim3(256), 0, s, A->disp1, A->root, A->cnt, d_disp, (int)pix, pix);
}

// n <= cap_n resident pairs (pair b at dL / dR + b * frame) -> d_disp (+ b * W * H floats; may be null), int16 maps in A->disp1
// (CN = 3: n <= cap_n / 2 pairs of interleaved three-channel rows)
template <int CN>
int sgbm_enqueue(svo_ctx* ctx, hipStream_t s, SgbmArena* A, const uint8_t* dL, const uint8_t* dR, int stride, size_t frame, int W,
                 int H, int D, int n, float* d_disp, bool dbg, int mode) {
  const size_t pix = (size_t)W * H, vol = pix * D;
  if (dbg) {   // the debug volumes are zero where nothing is defined
    SVO_HIP(ctx, hipMemsetAsync(A->C, 0, vol * sizeof(int16_t), s));
    SVO_HIP(ctx, hipMemsetAsync(A->dbgS4, 0, vol * sizeof(int16_t), s));
    SVO_HIP(ctx, hipMemsetAsync(A->dbgS, 0, vol * sizeof(int16_t), s));
  }
  SVO_HIP(ctx, hipMemsetAsync(A->bid, 0xff, pix * n * sizeof(uint32_t), s));
  // (T goes through the front of A->A as int16; the paths overwrite it)
  hipLaunchKernelGGL(k_sgbm_hsum<CN>, dim3(H, n), dim3(D * (256 / D)), 20 * (size_t)W, s, dL, dR, stride, frame, W, H, D, A->A, vol);
  hipLaunchKernelGGL(k_sgbm_vsum, dim3(((W - D) * D + 255) / 256, H, n), dim3(256), 0, s, A->A, A->C, W, H, D, vol);
  if (D == 16) sgbm_launch_paths<16, CN>(s, A, W, H, D, n, vol, pix, dbg, mode);
  else if (D == 32) sgbm_launch_paths<32, CN>(s, A, W, H, D, n, vol, pix, dbg, mode);
  else sgbm_launch_paths<64, CN>(s, A, W, H, D, n, vol, pix, dbg, mode);
  hipLaunchKernelGGL(k_sgbm_lr, dim3((W + 255) / 256, H, n), dim3(256), 0, s, A->disp1, A->bid, dbg ? A->dbg_disp2 : nullptr,
                     dbg ? A->dbg_lr : nullptr, W, H, pix);
  sgbm_speckles(s, A, W, H, n, d_disp);
  SVO_HIP(ctx, hipGetLastError());
  return SVO_OK;
}

}  // namespace

extern "C" int svo_sgbm_default_params(int height, svo_sgbm_params* p) {
  if (!p || height < 0) return SVO_E_INVALID;
  p->minDisparity = 0;
  p->numDisparities = ((height / 8) + 15) & -16;
  p->blockSize = 9;
  p->P1 = 8 * 81;
  p->P2 = 32 * 81;
  p->disp12MaxDiff = 1;
  p->preFilterCap = 63;
  p->uniquenessRatio = 10;
  p->speckleWindowSize = 100;
  p->speckleRange = 32;
  return SVO_OK;
}

// ElasMatch's set for a three-channel image: P1 = 8 cn 81, P2 = 32 cn 81 (src/frame.cc:103-104)
extern "C" int svo_sgbm_default_params_bgr(int height, svo_sgbm_params* p) {
  const int rc = svo_sgbm_default_params(height, p);
  if (rc) return rc;
  p->P1 *= 3;
  p->P2 *= 3;
  return SVO_OK;
}

namespace {

// B resident pairs -> B float maps, a chunk of pairs at a time, enqueued on `s` (no synchronisation)
template <int CN>
int sgbm_run(svo_ctx* ctx, hipStream_t s, const uint8_t* dL, const uint8_t* dR, int stride, size_t frame, int W, int H, int B,
             const svo_sgbm_params* p, int mode, float* d_disp) {
  constexpr int chunk = CN == 3 ? SGBM_CHUNK_BGR : SGBM_CHUNK, unit = SGBM_CHUNK / chunk;
  int rc = sgbm_check(p, W, H, CN, mode);
  if (rc) { ctx->last_error = "svo_sgbm: unsupported parameters or image size"; return rc; }
  SgbmArena* A = nullptr;
  if ((rc = sgbm_reserve(ctx, s, W, H, p->numDisparities, std::min(B, chunk) * unit, false, mode == SVO_SGBM_MODE_HH, &A))) return rc;
  A->dbg_valid = false;
  for (int f0 = 0; f0 < B; f0 += chunk) {
    const int n = std::min(chunk, B - f0);
    if ((rc = sgbm_enqueue<CN>(ctx, s, A, dL + f0 * frame, dR + f0 * frame, stride, frame, W, H, p->numDisparities, n,
                               d_disp + (size_t)f0 * W * H, false, mode)))
      return rc;
  }
  return SVO_OK;
}

template <int CN>
int sgbm_process(svo_ctx* ctx, const char* who, const uint8_t* L, const uint8_t* R, int stride, int W, int H, const svo_sgbm_params* p,
                 int mode, int16_t* disp16, float* disp) {
  int rc = sgbm_args(ctx, who, L && R, p, W, H, stride, CN, mode);
  if (rc) return rc;
  SVO_HIP(ctx, hipSetDevice(ctx->device));
  SgbmArena* A = nullptr;
  hipStream_t s = ctx->stream;
  const size_t pix = (size_t)W * H, row = (size_t)W * CN, img = pix * CN;
  if ((rc = sgbm_reserve(ctx, s, W, H, p->numDisparities, SGBM_CHUNK / (CN == 3 ? SGBM_CHUNK_BGR : SGBM_CHUNK), true, mode == SVO_SGBM_MODE_HH, &A, 2 * img))) return rc;
  A->dbg_valid = false;
  SVO_HIP(ctx, hipMemcpy2DAsync(A->img, row, L, stride, row, H, hipMemcpyHostToDevice, s));
  SVO_HIP(ctx, hipMemcpy2DAsync(A->img + img, row, R, stride, row, H, hipMemcpyHostToDevice, s));
  if ((rc = sgbm_enqueue<CN>(ctx, s, A, A->img, A->img + img, (int)row, img, W, H, p->numDisparities, 1, A->dispf, true, mode))) return rc;
  if (disp16) SVO_HIP(ctx, hipMemcpyAsync(disp16, A->disp1, pix * sizeof(int16_t), hipMemcpyDeviceToHost, s));
  if (disp) SVO_HIP(ctx, hipMemcpyAsync(disp, A->dispf, pix * sizeof(float), hipMemcpyDeviceToHost, s));
  SVO_HIP(ctx, hipStreamSynchronize(s));
  A->W = W; A->H = H; A->D = p->numDisparities; A->dbg_valid = true;
  return SVO_OK;
}

}  // namespace

int svo_sgbm_run_dev(svo_ctx* ctx, hipStream_t s, const uint8_t* dL, const uint8_t* dR, int stride, size_t frame, int W, int H, int B,
                     const svo_sgbm_params* p, int mode, float* d_disp) {
  return sgbm_run<1>(ctx, s, dL, dR, stride, frame, W, H, B, p, mode, d_disp);
}

int svo_sgbm_run_bgr_dev(svo_ctx* ctx, hipStream_t s, const uint8_t* dL, const uint8_t* dR, int stride, size_t frame, int W, int H,
                         int B, const svo_sgbm_params* p, int mode, float* d_disp) {
  return sgbm_run<3>(ctx, s, dL, dR, stride, frame, W, H, B, p, mode, d_disp);
}

int svo_sgbm_chunk() { return SGBM_CHUNK; }
int svo_sgbm_chunk_bgr() { return SGBM_CHUNK_BGR; }

namespace {

template <int CN>
int sgbm_batch(svo_ctx* ctx, const char* who, const uint8_t* d_L, const uint8_t* d_R, int stride, int W, int H, int B,
               const svo_sgbm_params* p, int mode, float* d_disp) {
  int rc = sgbm_args(ctx, who, d_L && d_R && d_disp && B >= 1, p, W, H, stride, CN, mode);
  if (rc) return rc;
  SVO_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = sgbm_run<CN>(ctx, ctx->stream, d_L, d_R, stride, (size_t)H * stride, W, H, B, p, mode, d_disp))) return rc;
  SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVO_OK;
}

}  // namespace

// The entries without a mode are the ones with a mode at SVO_SGBM_MODE_SGBM: one body each, which reports under the name of the
// entry the caller called.
extern "C" int svo_sgbm_process_mode(svo_ctx* ctx, const uint8_t* L, const uint8_t* R, int stride, int W, int H, const svo_sgbm_params* p,
                                     int mode, int16_t* disp16, float* disp) {
  return sgbm_process<1>(ctx, "svo_sgbm_process_mode", L, R, stride, W, H, p, mode, disp16, disp);
}

extern "C" int svo_sgbm_process_bgr_mode(svo_ctx* ctx, const uint8_t* L, const uint8_t* R, int stride, int W, int H,
                                         const svo_sgbm_params* p, int mode, int16_t* disp16, float* disp) {
  return sgbm_process<3>(ctx, "svo_sgbm_process_bgr_mode", L, R, stride, W, H, p, mode, disp16, disp);
}

extern "C" int svo_sgbm_batch_mode_dev(svo_ctx* ctx, const uint8_t* d_L, const uint8_t* d_R, int stride, int W, int H, int B,
                                       const svo_sgbm_params* p, int mode, float* d_disp) {
  return sgbm_batch<1>(ctx, "svo_sgbm_batch_mode_dev", d_L, d_R, stride, W, H, B, p, mode, d_disp);
}

extern "C" int svo_sgbm_batch_bgr_mode_dev(svo_ctx* ctx, const uint8_t* d_L, const uint8_t* d_R, int stride, int W, int H, int B,
                                           const svo_sgbm_params* p, int mode, float* d_disp) {
  return sgbm_batch<3>(ctx, "svo_sgbm_batch_bgr_mode_dev", d_L, d_R, stride, W, H, B, p, mode, d_disp);
}

extern "C" int svo_sgbm_process(svo_ctx* ctx, const uint8_t* L, const uint8_t* R, int stride, int W, int H, const svo_sgbm_params* p,
                                int16_t* disp16, float* disp) {
  return sgbm_process<1>(ctx, "svo_sgbm_process", L, R, stride, W, H, p, SVO_SGBM_MODE_SGBM, disp16, disp);
}

extern "C" int svo_sgbm_process_bgr(svo_ctx* ctx, const uint8_t* L, const uint8_t* R, int stride, int W, int H, const svo_sgbm_params* p,
                                    int16_t* disp16, float* disp) {
  return sgbm_process<3>(ctx, "svo_sgbm_process_bgr", L, R, stride, W, H, p, SVO_SGBM_MODE_SGBM, disp16, disp);
}

extern "C" int svo_sgbm_batch_dev(svo_ctx* ctx, const uint8_t* d_L, const uint8_t* d_R, int stride, int W, int H, int B,
                                  const svo_sgbm_params* p, float* d_disp) {
  return sgbm_batch<1>(ctx, "svo_sgbm_batch_dev", d_L, d_R, stride, W, H, B, p, SVO_SGBM_MODE_SGBM, d_disp);
}

extern "C" int svo_sgbm_batch_bgr_dev(svo_ctx* ctx, const uint8_t* d_L, const uint8_t* d_R, int stride, int W, int H, int B,
                                      const svo_sgbm_params* p, float* d_disp) {
  return sgbm_batch<3>(ctx, "svo_sgbm_batch_bgr_dev", d_L, d_R, stride, W, H, B, p, SVO_SGBM_MODE_SGBM, d_disp);
}

extern "C" int svo_sgbm_filter_speckles(svo_ctx* ctx, int16_t* disp16, int W, int H) {
  if (!ctx) return SVO_E_INVALID;
  if (!disp16 || W < 1 || H < 1) { ctx->last_error = "svo_sgbm_filter_speckles: invalid argument"; return SVO_E_INVALID; }
  if (W > SGBM_MAX_W || H > SGBM_MAX_H) { ctx->last_error = "svo_sgbm_filter_speckles: image larger than 3072 x 4096"; return SVO_E_CAPACITY; }
  SVO_HIP(ctx, hipSetDevice(ctx->device));
  SgbmArena* A = nullptr;
  hipStream_t s = ctx->stream;
  int rc = sgbm_reserve(ctx, s, W, H, 16, 1, false, false, &A);
  if (rc) return rc;
  A->dbg_valid = false;
  const size_t bytes = (size_t)W * H * sizeof(int16_t);
  SVO_HIP(ctx, hipMemcpyAsync(A->disp1, disp16, bytes, hipMemcpyHostToDevice, s));
  sgbm_speckles(s, A, W, H, 1, nullptr);
  SVO_HIP(ctx, hipGetLastError());
  SVO_HIP(ctx, hipMemcpyAsync(disp16, A->disp1, bytes, hipMemcpyDeviceToHost, s));
  SVO_HIP(ctx, hipStreamSynchronize(s));
  return SVO_OK;
}

extern "C" int svo_sgbm_debug_volume(svo_ctx* ctx, int which, int16_t* host) {
  if (!ctx || !host || which < 0 || which > 4) return SVO_E_INVALID;
  SgbmArena* A = static_cast<SgbmArena*>(ctx->sgbm);
  if (!A || !A->dbg_valid) { ctx->last_error = "svo_sgbm_debug_volume: no svo_sgbm_process call to report"; return SVO_E_INVALID; }
  SVO_HIP(ctx, hipSetDevice(ctx->device));
  const size_t pix = (size_t)A->W * A->H, vol = pix * A->D;
  const int16_t* src[5] = {A->C, A->dbgS4, A->dbgS, A->dbg_disp2, A->dbg_lr};
  SVO_HIP(ctx, svo_memcpy_sync(ctx, host, src[which], (which < 3 ? vol : pix) * sizeof(int16_t), hipMemcpyDeviceToHost));
  return SVO_OK;
}

void svo_sgbm_release(svo_ctx* ctx) {
  if (!ctx || !ctx->sgbm) return;
  SgbmArena* A = static_cast<SgbmArena*>(ctx->sgbm);
  void* bufs[] = {A->C, A->A, A->B, A->X, A->Y, A->dbgS4, A->dbgS, A->disp1, A->dbg_disp2, A->dbg_lr, A->bid, A->label, A->root, A->cnt, A->img, A->dispf};
  for (void* b : bufs)
    if (b) hipFree(b);
  delete A;
  ctx->sgbm = nullptr;
}
