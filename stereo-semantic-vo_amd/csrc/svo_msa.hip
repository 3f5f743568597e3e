// svo_msa.hip - the reference's MSA dense stereo: its device stages one by one, and
// MSA::solve end to end for C >= 1 pairs (msa_chunk_device).  The host-side graph stages that produce the aggregation
// tree (build, Tarjan arborescence, region Kruskal, BFS orders; MSA.cpp:152-926) are in svo_msa_graph.hip.
//
//  svo_ctmf : Thirdparty/MB/ctmf.h:7 `ctmf(src, dst, width, height, src_step, dst_step, r, channels, memsize)`,
//             the constant-time median filter MSA runs on the colour images (r = 1, 3 channels,
//             MSA.cpp:58-59) and on the winner-take-all disparity map (r = 2, 1 channel, MSA.cpp:1006).
//             What ctmf.c computes (ctmf.c:222-320): per channel the true median (rank 2r^2+2r of the
//             (2r+1)^2 window) with the window clamped to the image - rows and columns are REPLICATED at the
//             borders (`MAX(0, ..)`/`MIN(m-1, ..)` and the `r`-fold first column), not zero-padded as its
//             comment says.  The stripe decomposition (`memsize`) is a cache optimisation of the CPU code
//             and does not change results; it has no counterpart here.
//             GPU: one thread per (pixel, channel); the median is found by bisection on the 8-bit value
//             range (8 counting passes over the window held in registers) - O(r^2) per pixel, which for the
//             radii MSA uses (1, 2) is 9 / 25 elements.
//  svo_msa_init : `MSA::init` (MSA.cpp:22-63) - gray conversion (:42-47), `gradient` (:65-76), `getCost` (:78-108:
//             the two cost volumes, cost = 0.11 * min(mean |dBGR|, 7) + 0.89 * min(|dgrad|, 2) in float64, stored
//             as float), `ctmf` r = 1 on both colour images and `gradient_after_ctmf` (:110-139).  All per-pixel
//             work; the right-reference volume is the left one re-indexed (costR[j][d] = costL[j + d'][d'],
//             d' = min(d, m - 1 - j): the reference's "copy the previous disparity" chain in closed form).
//  svo_msa_tree_dp : `MSA::TreeDp` (MSA.cpp:929-990) - the two-pass cost aggregation over the spanning tree, level by
//             level (a node after all its children on the way up, after its parent on the way down), one thread
//             per (node, disparity); the children are added in the order the reference's adjacency chain yields
//             them, each `+=` rounded to float as there.
//  svo_msa_wta / svo_msa_lrcheck : `MSA::WTA` (:992-1006, first minimum + 5x5 ctmf) and `MSA::LRcheck` (:1027-1105).
#include <math.h>

#include <algorithm>
#include <functional>
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <mutex>
#include <thread>
#include <vector>

#include "svo_internal.h"

namespace {

template <int R>
__global__ __launch_bounds__(256) void k_ctmf(const uint8_t* src, uint8_t* dst, int width, int height,
                                              int src_step, int dst_step, int cn) {
  const int xc = blockIdx.x * 256 + threadIdx.x;   // column * cn + channel
  const int y = blockIdx.y;
  if (xc >= width * cn) return;
  const int x = xc / cn, c = xc - x * cn;
  constexpr int N = (2 * R + 1) * (2 * R + 1);
  uint8_t v[N];
#pragma unroll
  for (int dy = -R; dy <= R; ++dy) {
    const uint8_t* row = src + (size_t)min(max(y + dy, 0), height - 1) * src_step;
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) v[(dy + R) * (2 * R + 1) + dx + R] = row[min(max(x + dx, 0), width - 1) * cn + c];
  }
  // smallest value m with #{v <= m} > t, t = 2r^2 + 2r  (ctmf.c:271-312)
  int lo = 0, hi = 255;
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int mid = (lo + hi) >> 1;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) cnt += v[k] <= mid;
    if (cnt > 2 * R * R + 2 * R) hi = mid; else lo = mid + 1;
  }
  dst[(size_t)y * dst_step + xc] = (uint8_t)lo;
}

__device__ __forceinline__ uint8_t msa_gray(const uint8_t* bgr) {   // MSA.cpp:44-45
  return (uint8_t)(int)(0.299 * bgr[2] + 0.587 * bgr[1] + 0.114 * bgr[0] + 0.5);
}
__global__ void k_msa_gray(const uint8_t* bgr, int n, uint8_t* gray) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) gray[i] = msa_gray(bgr + 3 * (size_t)i);
}
// central difference along x (`along_rows`) or y, one-sided at the borders, plus `offset` (MSA.cpp:65-76, 118-138)
__global__ void k_msa_gradient(const uint8_t* img, int n, int m, int along_rows, double offset, double* gra) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= m) return;
  const int t = i * m + j;
  const int len = along_rows ? m : n, pos = along_rows ? j : i, st = along_rows ? 1 : m;
  double g;
  if (pos == 0) g = (double)img[t + st] - (double)img[t];
  else if (pos == len - 1) g = (double)img[t] - (double)img[t - st];
  else g = ((double)img[t + st] - (double)img[t - st]) * 0.5;
  gra[t] = g + offset;
}
__global__ void k_msa_cost(const uint8_t* bgrL, const uint8_t* bgrR, const double* graL, const double* graR, int n, int m,
                           int disp, float* costL) {
  const int idx = blockIdx.x * 256 + threadIdx.x;   // (pixel, d), d fastest
  if (idx >= n * m * disp) return;
  const int t = idx / disp, d = idx - t * disp, i = t / m, j = t - i * m;
  const int o = (j - d >= 0) ? t - d : i * m;
  const double dif_gra = fmin(fabs(graL[t] - graR[o]), 2.0);
  double dif_col = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) dif_col += abs((int)bgrL[3 * (size_t)t + k] - (int)bgrR[3 * (size_t)o + k]);
  dif_col = fmin(dif_col / 3, 7.0);
  costL[idx] = (float)(0.11 * dif_col + (1 - 0.11) * dif_gra);
}
__global__ void k_msa_cost_right(const float* costL, int n, int m, int disp, float* costR) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * m * disp) return;
  const int t = idx / disp, d = idx - t * disp, j = t % m;
  const int dd = min(d, m - 1 - j);
  costR[idx] = costL[(size_t)(t + dd) * disp + dd];
}

// One tree on the device and the volumes of one aggregation over it (blockIdx.y of every TreeDp kernel picks the tree).
// (MsaBfsRec - first child's position | weight to parent + (children << 8) | parent's position | pixel - is declared in
// svo_internal.h: the host-side tree builder writes the records itself)
struct MsaTab {
  const MsaBfsRec* rec;        // the tree by level-order position (k_msa_dp_bfs)
  const int32_t* level_ptr; int32_t levels, N;
  const float* cost;           // [pixel][D] in
  float* up;                   // work: [D][position] (k_msa_dp_bfs), [pixel][D] (level launches)
  float* A;                    // [pixel][D] out
  const int32_t *nodes, *child_ptr, *child, *parent;   // the tree by pixel: the level launches only
  const uint8_t *child_c, *parent_c;
};
// TreeDp with one launch per level: level l of every tree in one launch (a tree with fewer levels sits it out).
// leaves -> root: all children of the level's nodes are final
__global__ void k_msa_dp_up_many(const MsaTab* tabs, int l, int D, const double* Exp) {
  const MsaTab t = tabs[blockIdx.y];
  if (l >= t.levels) return;
  const int beg = t.level_ptr[l], cnt = t.level_ptr[l + 1] - beg;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= cnt * D) return;
  const int u = t.nodes[beg + idx / D], d = idx % D;
  float acc = t.cost[(size_t)u * D + d];
  for (int e = t.child_ptr[u]; e < t.child_ptr[u + 1]; ++e)
    acc = (float)((double)acc + Exp[t.child_c[e]] * (double)t.up[(size_t)t.child[e] * D + d]);
  t.up[(size_t)u * D + d] = acc;
}
// root -> leaves: the parents of the level's nodes are final
__global__ void k_msa_dp_down_many(const MsaTab* tabs, int l, int D, const double* Exp) {
  const MsaTab t = tabs[blockIdx.y];
  if (l >= t.levels) return;
  const int beg = t.level_ptr[l], cnt = t.level_ptr[l + 1] - beg;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= cnt * D) return;
  const int v = t.nodes[beg + idx / D], d = idx % D, u = t.parent[v];
  if (u < 0) { t.A[(size_t)v * D + d] = t.up[(size_t)v * D + d]; return; }
  const double w = Exp[t.parent_c[v]];
  t.A[(size_t)v * D + d] = (float)(w * (double)t.A[(size_t)u * D + d] + (1 - w * w) * (double)t.up[(size_t)v * D + d]);
}

// ---- TreeDp as ONE launch per aggregation -------------------------------------------------------------------------
// The recurrences run per disparity: nothing couples A[.][d] to A[.][d'].  So one workgroup takes ONE disparity of one
// tree and walks all ~2000 levels itself - leaves to root, then root to leaves - with a workgroup barrier per level
// instead of a kernel launch per level (2 x 2000 launches per aggregation before).  Nodes are addressed by their
// position g in level order (children of a node are consecutive there, MsaBfsRec::cpos), the per-disparity values live in
// a transposed slab upT[d][g] (coalesced), and the values of the level just finished - all the next level needs -
// stay in LDS: a level costs one LDS round trip and a barrier, the HBM reads of the next level's own terms are issued a
// level ahead.  Arithmetic and its order are those of k_msa_dp_up_many / k_msa_dp_down_many (the child's weighted term
// Exp[c] * (double)up[child] is formed by the child, added by the parent in child order).

// upT[d][g] = cost[node(g)][d]  (64 positions x D disparities per workgroup, transposed through LDS)
__global__ __launch_bounds__(256) void k_msa_bfs_gather(const MsaTab* tabs, int D) {
  extern __shared__ float msa_tile[];   // 64 x (D + 1)
  const MsaTab t = tabs[blockIdx.y];
  const int g0 = blockIdx.x * 64;
  if (g0 >= t.N) return;
  const float* cost = t.cost;
  float* upT = t.up;
  for (int idx = threadIdx.x; idx < 64 * D; idx += 256) {
    const int gi = idx / D, d = idx - gi * D;
    if (g0 + gi < t.N) msa_tile[gi * (D + 1) + d] = cost[(size_t)t.rec[g0 + gi].node * D + d];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 64 * D; idx += 256) {
    const int d = idx >> 6, gi = idx & 63;
    if (g0 + gi < t.N) upT[(size_t)d * t.N + g0 + gi] = msa_tile[gi * (D + 1) + d];
  }
}

template <int T>
__global__ __launch_bounds__(T) void k_msa_dp_bfs(const MsaTab* tabs, int D, const double* Exp, int maxw, int maxl) {
  extern __shared__ double msa_lds[];   // Exp[256] | two level buffers of maxw doubles | level_ptr (maxl + 2 ints)
  const MsaTab t = tabs[blockIdx.y];
  const int d = blockIdx.x, tid = threadIdx.x, L = t.levels;
  double* E = msa_lds;
  double* cur = msa_lds + 256;
  double* prev = cur + maxw;
  int* lp = reinterpret_cast<int*>(prev + maxw);
  for (int i = tid; i < 256; i += T) E[i] = Exp[i];
  for (int i = tid; i <= L; i += T) lp[i] = t.level_ptr[i];
  __syncthreads();
  float* up = t.up + (size_t)d * t.N;
  float* A = t.A;
  const MsaBfsRec* rec = t.rec;
  MsaBfsRec r_n = {0, 0, -1, 0};
  float own_n = 0.f;
  // ---- leaves -> root ------------------------------------------------------------------------------------------
  if (L > 0 && tid < lp[L] - lp[L - 1]) { r_n = rec[lp[L - 1] + tid]; own_n = up[lp[L - 1] + tid]; }
  for (int l = L - 1; l >= 0; --l) {
    const int beg = lp[l], cbeg = lp[l + 1], cnt = cbeg - beg;
    MsaBfsRec r = r_n;
    float own = own_n;
    if (l > 0 && tid < beg - lp[l - 1]) { r_n = rec[lp[l - 1] + tid]; own_n = up[lp[l - 1] + tid]; }   // next level's terms: in flight now
    for (int i = tid; i < cnt; i += T) {
      if (i != tid) { r = rec[beg + i]; own = up[beg + i]; }
      float acc = own;
      const int c0 = r.cpos - cbeg, nch = (r.meta >> 8) & 255;
      for (int c = 0; c < nch; ++c) acc = (float)((double)acc + prev[c0 + c]);
      up[beg + i] = acc;
      cur[i] = E[r.meta & 255] * (double)acc;
    }
    __syncthreads();
    double* x = cur; cur = prev; prev = x;
  }
  // ---- root -> leaves ------------------------------------------------------------------------------------------
  float* curA = reinterpret_cast<float*>(cur);
  float* prevA = reinterpret_cast<float*>(prev);
  if (L > 0 && tid < lp[1] - lp[0]) { r_n = rec[lp[0] + tid]; own_n = up[lp[0] + tid]; }
  for (int l = 0; l < L; ++l) {
    const int beg = lp[l], cnt = lp[l + 1] - beg, pbeg = l > 0 ? lp[l - 1] : 0;
    MsaBfsRec r = r_n;
    float upv = own_n;
    if (l + 1 < L && tid < lp[l + 2] - lp[l + 1]) { r_n = rec[lp[l + 1] + tid]; own_n = up[lp[l + 1] + tid]; }
    for (int i = tid; i < cnt; i += T) {
      if (i != tid) { r = rec[beg + i]; upv = up[beg + i]; }
      float a = upv;
      if (r.ppos >= 0) {
        const double w = E[r.meta & 255];
        a = (float)(w * (double)prevA[r.ppos - pbeg] + (1 - w * w) * (double)upv);
      }
      A[(size_t)r.node * D + d] = a;
      curA[i] = a;
    }
    __syncthreads();
    float* x = curA; curA = prevA; prevA = x;
  }
}
__global__ void k_msa_argmin(const float* costA, int N, int D, uint8_t* disp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  int k = 0;
  float best = costA[(size_t)i * D];
  for (int j = 1; j < D; ++j) { const float c = costA[(size_t)i * D + j]; if (c < best) { best = c; k = j; } }
  disp[i] = (uint8_t)k;
}
__global__ void k_msa_lrcheck(const uint8_t* d1, const uint8_t* d2, int n, int m, int D, float* cost, uint8_t* mask) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * m * D) return;
  const int t = idx / D, d = idx - t * D, j = t % m, dd = d1[t];
  const bool stable = j - dd >= 0 && dd > 0 && d2[t - dd] == dd;
  if (d == 0) mask[t] = stable ? 1 : 0;
  cost[idx] = stable ? (float)abs(d - dd) : 0.0f;
}

struct DevBuf {   // device allocations of one solve; reset() hands the same buffers out again in the same order
  struct Slot { void* p; size_t bytes; };
  std::vector<Slot> slots;
  size_t cursor = 0;
  ~DevBuf() { for (Slot& q : slots) hipFree(q.p); }
  void reset() { cursor = 0; }
  template <typename T> T* get(size_t count) {
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    if (cursor == slots.size()) slots.push_back(Slot{nullptr, 0});
    Slot& q = slots[cursor++];
    if (q.bytes < bytes) {
      if (q.p) hipFree(q.p);
      q.p = nullptr; q.bytes = 0;
      if (hipMalloc(&q.p, bytes) != hipSuccess) { q.p = nullptr; return nullptr; }
      q.bytes = bytes;
    }
    return reinterpret_cast<T*>(q.p);
  }
};

// the buffers of svo_msa_solve / the tracker's MSA mode live as long as the ctx (index 0: the ctx stream; 1, 2: the
// lanes of svo_msa_run_many_dev) - a solve allocates ~0.55 GB per pair at KITTI size and hipFree synchronises the device
struct MsaHostStore;   // host-side buffers of a solve (kept for the same reason: page faults)
struct MsaArena { DevBuf dev, io; MsaHostStore* host = nullptr; };   // dev: the solver's buffers; io: svo_msa_solve's uploaded pair and output
struct MsaArenas { std::vector<MsaArena*> a; std::mutex m; };
MsaArena& msa_arena(svo_ctx* ctx, int idx) {
  if (!ctx->msa_arenas) ctx->msa_arenas = new MsaArenas();
  MsaArenas* A = static_cast<MsaArenas*>(ctx->msa_arenas);
  std::lock_guard<std::mutex> lock(A->m);
  while ((int)A->a.size() <= idx) A->a.push_back(new MsaArena());
  A->a[idx]->dev.reset(); A->a[idx]->io.reset();
  return *A->a[idx];
}

}  // namespace

// Level-order records of a tree for k_msa_dp_bfs.  nodes: pixels in level order; returns false when some node's children are
// not consecutive positions in child order (cannot happen for a breadth-first `seq`; the caller then keeps the
// level-by-level launches).
static bool msa_bfs_records(int N, const int32_t* nodes, const std::vector<int32_t>& level_ptr, const int32_t* child_ptr,
                            const int32_t* child, const int32_t* parent, const uint8_t* parent_c, std::vector<int32_t>& pos,
                            std::vector<MsaBfsRec>& rec, int* maxw) {
  pos.resize(N);
  for (int g = 0; g < N; ++g) pos[nodes[g]] = g;
  rec.resize(N);
  int cpos = 1;
  bool ok = true;
  for (int g = 0; g < N; ++g) {
    const int u = nodes[g], nch = child_ptr[u + 1] - child_ptr[u];
    for (int j = 0; j < nch && ok; ++j) ok = cpos + j < N && nodes[cpos + j] == child[child_ptr[u] + j];
    rec[g] = MsaBfsRec{cpos, (int32_t)parent_c[u] | (nch << 8), parent[u] >= 0 ? pos[parent[u]] : -1, u};
    if (nch > 255) ok = false;
    cpos += nch;
  }
  int w = 0;
  for (size_t l = 0; l + 1 < level_ptr.size(); ++l) w = std::max(w, level_ptr[l + 1] - level_ptr[l]);
  *maxw = w;
  return ok && cpos == N;
}

static bool msa_level_launches() { return getenv("SVO_MSA_LEVEL_LAUNCHES") != nullptr; }   // read per call: a test may set and clear it

// How one chunk's aggregations run: as k_msa_dp_bfs (every tree in level order, the levels fit its LDS buffers, opt-in above
// 64 KB granted) or as one launch per level (otherwise, or when SVO_MSA_LEVEL_LAUNCHES asks for it).
constexpr int kMsaDpThreads = 512;
struct MsaDpPlan {
  bool bfs = true;
  int maxw = 0;             // widest level of any tree
  std::vector<int> width;   // widest level l over the trees: the grid of that level's launch
  void add(const std::vector<int32_t>& level_ptr, bool bfs_ok) {
    bfs = bfs && bfs_ok;
    if (width.size() + 1 < level_ptr.size()) width.resize(level_ptr.size() - 1, 0);
    for (size_t l = 0; l + 1 < level_ptr.size(); ++l) {
      width[l] = std::max(width[l], level_ptr[l + 1] - level_ptr[l]);
      maxw = std::max(maxw, width[l]);
    }
  }
  size_t lds() const { return sizeof(double) * (256 + 2 * (size_t)maxw) + sizeof(int) * (width.size() + 2); }
  void decide(svo_ctx* ctx, int D) {
    choose(ctx, D);
    const int32_t rec[4] = {bfs ? 1 : 0, maxw, (int32_t)width.size(), (int32_t)lds()};   // what svo_debug_msa_plan reports
    memcpy(ctx->msa_plan, rec, sizeof rec);
  }
  void choose(svo_ctx* ctx, int D) {
    if (msa_level_launches() || lds() > 150 * 1024 || (size_t)64 * (D + 1) * sizeof(float) > 64 * 1024) { bfs = false; return; }
    if (ctx->msa_lds_state == 0)
      ctx->msa_lds_state = hipFuncSetAttribute(reinterpret_cast<const void*>(k_msa_dp_bfs<kMsaDpThreads>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024) == hipSuccess ? 1 : -1;
    bfs = bfs && (ctx->msa_lds_state > 0 || lds() <= 64 * 1024);
  }
};

extern "C" int svo_debug_msa_plan(svo_ctx* ctx, int32_t out[5]) {
  if (!ctx || !out) return SVO_E_INVALID;
  memcpy(out, ctx->msa_plan, sizeof ctx->msa_plan);
  out[4] = ctx->msa_lds_state;
  return SVO_OK;
}
// One aggregation (both sweeps) of the trees tabs[0 .. ntrees): two launches, or two per level
static void msa_aggregate(hipStream_t s, const MsaTab* d_tabs, int ntrees, int N, int D, const double* d_Exp, const MsaDpPlan& p) {
  const int L = (int)p.width.size();
  if (p.bfs) {
    hipLaunchKernelGGL(k_msa_bfs_gather, dim3((unsigned)((N + 63) / 64), ntrees), dim3(256), (size_t)64 * (D + 1) * sizeof(float), s, d_tabs, D);
    hipLaunchKernelGGL(k_msa_dp_bfs<kMsaDpThreads>, dim3(D, ntrees), dim3(kMsaDpThreads), p.lds(), s, d_tabs, D, d_Exp, p.maxw, L);
    return;
  }
  auto grid = [&](int l) { return dim3((unsigned)(((size_t)p.width[l] * D + 255) / 256), ntrees); };
  for (int l = L - 1; l >= 0; --l) hipLaunchKernelGGL(k_msa_dp_up_many, grid(l), dim3(256), 0, s, d_tabs, l, D, d_Exp);
  for (int l = 0; l < L; ++l) hipLaunchKernelGGL(k_msa_dp_down_many, grid(l), dim3(256), 0, s, d_tabs, l, D, d_Exp);
}
// The by-pixel arrays of one tree for the level launches: device copies from `buf`, pointers into `tab`
static int msa_upload_by_pixel(svo_ctx* ctx, hipStream_t s, DevBuf& buf, int N, const int32_t* nodes, const int32_t* child_ptr,
                               const int32_t* child, const uint8_t* child_c, const int32_t* parent, const uint8_t* parent_c, MsaTab& tab) {
  int32_t* d_int[4] = {buf.get<int32_t>(N), buf.get<int32_t>(N + 1), buf.get<int32_t>(N), buf.get<int32_t>(N)};
  uint8_t* d_byte[2] = {buf.get<uint8_t>(N), buf.get<uint8_t>(N)};
  if (!d_int[0] || !d_int[1] || !d_int[2] || !d_int[3] || !d_byte[0] || !d_byte[1]) { ctx->last_error = "svo_msa: hipMalloc"; return SVO_E_NOMEM; }
  SVO_HIP(ctx, hipMemcpyAsync(d_int[0], nodes, (size_t)N * 4, hipMemcpyHostToDevice, s));
  SVO_HIP(ctx, hipMemcpyAsync(d_int[1], child_ptr, ((size_t)N + 1) * 4, hipMemcpyHostToDevice, s));
  if (N > 1) {
    SVO_HIP(ctx, hipMemcpyAsync(d_int[2], child, ((size_t)N - 1) * 4, hipMemcpyHostToDevice, s));
    SVO_HIP(ctx, hipMemcpyAsync(d_byte[0], child_c, (size_t)N - 1, hipMemcpyHostToDevice, s));
  }
  SVO_HIP(ctx, hipMemcpyAsync(d_int[3], parent, (size_t)N * 4, hipMemcpyHostToDevice, s));
  SVO_HIP(ctx, hipMemcpyAsync(d_byte[1], parent_c, (size_t)N, hipMemcpyHostToDevice, s));
  tab.nodes = d_int[0]; tab.child_ptr = d_int[1]; tab.child = d_int[2]; tab.parent = d_int[3];
  tab.child_c = d_byte[0]; tab.parent_c = d_byte[1];
  return SVO_OK;
}

extern "C" int svo_msa_tree_dp(svo_ctx* ctx, const float* cost, int N, int D, const int32_t* seq, const int32_t* child_ptr,
                               const int32_t* child, const uint8_t* child_c, int root, double o, float* costA) {
  if (!ctx) return SVO_E_INVALID;
  if (!cost || !seq || !child_ptr || !child || !child_c || !costA || N < 1 || D < 1 || D > 256 || root < 0 || root >= N ||
      !(o > 0) || seq[0] != root || child_ptr[0] != 0 || child_ptr[N] != N - 1) {
    ctx->last_error = "svo_msa_tree_dp: invalid argument (need a spanning tree in BFS order from `root`)";
    return SVO_E_INVALID;
  }
  // parents, edge weights towards the parent, depths (seq is a BFS order: parents come before children)
  std::vector<int32_t> parent(N, -2), depth(N, 0), level_ptr, nodes(N);
  std::vector<uint8_t> parent_c(N, 0);
  parent[root] = -1;
  int max_depth = 0;
  for (int k = 0; k < N; ++k) {
    const int u = seq[k];
    if (u < 0 || u >= N || parent[u] == -2) { ctx->last_error = "svo_msa_tree_dp: seq is not a BFS order of the tree"; return SVO_E_INVALID; }
    for (int e = child_ptr[u]; e < child_ptr[u + 1]; ++e) {
      const int v = child[e];
      if (v < 0 || v >= N || parent[v] != -2) { ctx->last_error = "svo_msa_tree_dp: not a tree"; return SVO_E_INVALID; }
      parent[v] = u; parent_c[v] = child_c[e]; depth[v] = depth[u] + 1;
      max_depth = std::max(max_depth, depth[v]);
    }
  }
  level_ptr.assign(max_depth + 2, 0);
  for (int v = 0; v < N; ++v) ++level_ptr[depth[v] + 1];
  for (int l = 0; l <= max_depth; ++l) level_ptr[l + 1] += level_ptr[l];
  {
    std::vector<int32_t> fill(level_ptr.begin(), level_ptr.end() - 1);
    for (int k = 0; k < N; ++k) nodes[fill[depth[seq[k]]]++] = seq[k];
  }
  double Exp[256];
  for (int i = 0; i <= 255; ++i) Exp[i] = exp(-i * 1.0 / o / 255);   // MSA::setExp, MSA.cpp:1126-1130
  std::vector<MsaBfsRec> rec;
  std::vector<int32_t> pos;
  int maxw = 0;
  MsaDpPlan plan;
  plan.add(level_ptr, msa_bfs_records(N, nodes.data(), level_ptr, child_ptr, child, parent.data(), parent_c.data(), pos, rec, &maxw));
  SVO_HIP(ctx, hipSetDevice(ctx->device));
  plan.decide(ctx, D);
  DevBuf buf;
  const size_t V = (size_t)N * D;
  float* d_cost = buf.get<float>(V); float* d_up = buf.get<float>(V); float* d_A = buf.get<float>(V);
  MsaBfsRec* d_rec = buf.get<MsaBfsRec>(N);
  int32_t* d_lp = buf.get<int32_t>(level_ptr.size());
  MsaTab* d_tab = buf.get<MsaTab>(1);
  double* d_E = buf.get<double>(256);
  if (!d_cost || !d_up || !d_A || !d_rec || !d_lp || !d_tab || !d_E) { ctx->last_error = "svo_msa_tree_dp: hipMalloc"; return SVO_E_NOMEM; }
  hipStream_t s = ctx->stream;
  MsaTab tab{d_rec, d_lp, max_depth + 1, N, d_cost, d_up, d_A, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (plan.bfs) SVO_HIP(ctx, hipMemcpyAsync(d_rec, rec.data(), (size_t)N * sizeof(MsaBfsRec), hipMemcpyHostToDevice, s));
  else if (const int rc = msa_upload_by_pixel(ctx, s, buf, N, nodes.data(), child_ptr, child, child_c, parent.data(), parent_c.data(), tab)) return rc;
  SVO_HIP(ctx, hipMemcpyAsync(d_cost, cost, V * sizeof(float), hipMemcpyHostToDevice, s));
  SVO_HIP(ctx, hipMemcpyAsync(d_lp, level_ptr.data(), level_ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  SVO_HIP(ctx, hipMemcpyAsync(d_tab, &tab, sizeof tab, hipMemcpyHostToDevice, s));
  SVO_HIP(ctx, hipMemcpyAsync(d_E, Exp, sizeof Exp, hipMemcpyHostToDevice, s));
  {
    SvoTimer t(ctx, "k_msa_tree_dp");
    msa_aggregate(s, d_tab, 1, N, D, d_E, plan);
  }
  SVO_HIP(ctx, hipMemcpyAsync(costA, d_A, V * sizeof(float), hipMemcpyDeviceToHost, s));
  SVO_HIP(ctx, hipStreamSynchronize(s));
  SVO_HIP(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_msa_wta(svo_ctx* ctx, const float* costA, int width, int height, int D, uint8_t* disparity) {
  if (!ctx) return SVO_E_INVALID;
  if (!costA || !disparity || width < 5 || height < 5 || D < 1 || D > 256) { ctx->last_error = "svo_msa_wta: invalid argument"; return SVO_E_INVALID; }
  SVO_HIP(ctx, hipSetDevice(ctx->device));
  DevBuf buf;
  const size_t N = (size_t)width * height;
  float* d_A = buf.get<float>(N * D); uint8_t* d_raw = buf.get<uint8_t>(N); uint8_t* d_med = buf.get<uint8_t>(N);
  if (!d_A || !d_raw || !d_med) { ctx->last_error = "svo_msa_wta: hipMalloc"; return SVO_E_NOMEM; }
  hipStream_t s = ctx->stream;
  SVO_HIP(ctx, hipMemcpyAsync(d_A, costA, N * D * sizeof(float), hipMemcpyHostToDevice, s));
  {
    SvoTimer t(ctx, "k_msa_wta");
    hipLaunchKernelGGL(k_msa_argmin, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, d_A, (int)N, D, d_raw);
    hipLaunchKernelGGL(k_ctmf<2>, dim3((width + 255) / 256, height), dim3(256), 0, s, d_raw, d_med, width, height, width, width, 1);
  }
  SVO_HIP(ctx, hipMemcpyAsync(disparity, d_med, N, hipMemcpyDeviceToHost, s));
  SVO_HIP(ctx, hipStreamSynchronize(s));
  SVO_HIP(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_msa_lrcheck(svo_ctx* ctx, const uint8_t* d1, const uint8_t* d2, int width, int height, int D, float* cost,
                               uint8_t* mask) {
  if (!ctx) return SVO_E_INVALID;
  if (!d1 || !d2 || !cost || !mask || width < 1 || height < 1 || D < 1 || D > 256) { ctx->last_error = "svo_msa_lrcheck: invalid argument"; return SVO_E_INVALID; }
  SVO_HIP(ctx, hipSetDevice(ctx->device));
  DevBuf buf;
  const size_t N = (size_t)width * height;
  uint8_t* a = buf.get<uint8_t>(N); uint8_t* b = buf.get<uint8_t>(N); uint8_t* mk = buf.get<uint8_t>(N);
  float* c = buf.get<float>(N * D);
  if (!a || !b || !mk || !c) { ctx->last_error = "svo_msa_lrcheck: hipMalloc"; return SVO_E_NOMEM; }
  hipStream_t s = ctx->stream;
  SVO_HIP(ctx, hipMemcpyAsync(a, d1, N, hipMemcpyHostToDevice, s));
  SVO_HIP(ctx, hipMemcpyAsync(b, d2, N, hipMemcpyHostToDevice, s));
  {
    SvoTimer t(ctx, "k_msa_lrcheck");
    hipLaunchKernelGGL(k_msa_lrcheck, dim3((unsigned)((N * D + 255) / 256)), dim3(256), 0, s, a, b, height, width, D, c, mk);
  }
  SVO_HIP(ctx, hipMemcpyAsync(cost, c, N * D * sizeof(float), hipMemcpyDeviceToHost, s));
  SVO_HIP(ctx, hipMemcpyAsync(mask, mk, N, hipMemcpyDeviceToHost, s));
  SVO_HIP(ctx, hipStreamSynchronize(s));
  SVO_HIP(ctx, hipGetLastError());
  return SVO_OK;
}

// n rows x m columns (the reference's naming), BGR interleaved, `step` bytes per row.
extern "C" int svo_msa_init(svo_ctx* ctx, const uint8_t* bgrL, const uint8_t* bgrR, int width, int height, int step, int disp,
                            float* costL, float* costR, uint8_t* m_img3L, uint8_t* m_img3R, double* r_graL, double* c_graL,
                            double* r_graR, double* c_graR) {
  if (!ctx) return SVO_E_INVALID;
  const int n = height, m = width;
  if (!bgrL || !bgrR || !costL || !costR || !m_img3L || !m_img3R || !r_graL || !c_graL || !r_graR || !c_graR || n < 2 ||
      m < 2 || disp < 1 || disp > 256 || step < 3 * m || (size_t)n * m * disp > (size_t)1 << 30) {
    ctx->last_error = "svo_msa_init: invalid argument";
    return SVO_E_INVALID;
  }
  SVO_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = (size_t)n * m, V = N * disp;
  // one arena: 2 colour images, 2 median images, 2 gray, 2 gray-of-median, 6 gradient maps, 2 cost volumes
  const size_t bytes = 4 * 3 * N + 4 * N + 6 * N * sizeof(double) + 2 * V * sizeof(float) + 64;
  uint8_t* base = nullptr;
  SVO_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&base), bytes));
  double* g = reinterpret_cast<double*>(base);                 // graL graR r_graL c_graL r_graR c_graR
  float* cL = reinterpret_cast<float*>(g + 6 * N);
  float* cR = cL + V;
  uint8_t* img3[2] = {reinterpret_cast<uint8_t*>(cR + V), reinterpret_cast<uint8_t*>(cR + V) + 3 * N};
  uint8_t* med3[2] = {img3[1] + 3 * N, img3[1] + 6 * N};
  uint8_t* gray[2] = {med3[1] + 3 * N, med3[1] + 4 * N};
  uint8_t* mgray[2] = {gray[1] + N, gray[1] + 2 * N};
  hipStream_t s = ctx->stream;
  int rc = SVO_OK;
  auto chk = [&](hipError_t e) { if (e != hipSuccess && rc == SVO_OK) { rc = SVO_E_HIP; ctx->last_error = hipGetErrorString(e); } };
  chk(hipMemcpy2DAsync(img3[0], 3 * (size_t)m, bgrL, step, 3 * (size_t)m, n, hipMemcpyHostToDevice, s));
  chk(hipMemcpy2DAsync(img3[1], 3 * (size_t)m, bgrR, step, 3 * (size_t)m, n, hipMemcpyHostToDevice, s));
  if (rc == SVO_OK) {
    const dim3 px((m + 255) / 256, n);
    const unsigned nbN = (unsigned)((N + 255) / 256), nbV = (unsigned)((V + 255) / 256);
    for (int side = 0; side < 2; ++side) {
      SvoTimer t(ctx, "k_msa_gray_gradient");
      hipLaunchKernelGGL(k_msa_gray, dim3(nbN), dim3(256), 0, s, img3[side], (int)N, gray[side]);
      hipLaunchKernelGGL(k_msa_gradient, px, dim3(256), 0, s, gray[side], n, m, 1, 127.5, g + side * N);
    }
    {
      SvoTimer t(ctx, "k_msa_cost");
      hipLaunchKernelGGL(k_msa_cost, dim3(nbV), dim3(256), 0, s, img3[0], img3[1], g, g + N, n, m, disp, cL);
      hipLaunchKernelGGL(k_msa_cost_right, dim3(nbV), dim3(256), 0, s, cL, n, m, disp, cR);
    }
    for (int side = 0; side < 2; ++side) {
      {
        SvoTimer t(ctx, "k_ctmf");
        hipLaunchKernelGGL(k_ctmf<1>, dim3((3 * m + 255) / 256, n), dim3(256), 0, s, img3[side], med3[side], m, n, 3 * m, 3 * m, 3);
      }
      SvoTimer t(ctx, "k_msa_gray_gradient");
      hipLaunchKernelGGL(k_msa_gray, dim3(nbN), dim3(256), 0, s, med3[side], (int)N, mgray[side]);
      hipLaunchKernelGGL(k_msa_gradient, px, dim3(256), 0, s, mgray[side], n, m, 1, 0.0, g + (2 + 2 * side) * N);
      hipLaunchKernelGGL(k_msa_gradient, px, dim3(256), 0, s, mgray[side], n, m, 0, 0.0, g + (3 + 2 * side) * N);
    }
    chk(hipMemcpyAsync(costL, cL, V * sizeof(float), hipMemcpyDeviceToHost, s));
    chk(hipMemcpyAsync(costR, cR, V * sizeof(float), hipMemcpyDeviceToHost, s));
    chk(hipMemcpyAsync(m_img3L, med3[0], 3 * N, hipMemcpyDeviceToHost, s));
    chk(hipMemcpyAsync(m_img3R, med3[1], 3 * N, hipMemcpyDeviceToHost, s));
    double* outs[4] = {r_graL, c_graL, r_graR, c_graR};
    for (int k = 0; k < 4; ++k) chk(hipMemcpyAsync(outs[k], g + (2 + k) * N, N * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  chk(hipStreamSynchronize(s));
  chk(hipGetLastError());
  hipFree(base);
  return rc;
}

extern "C" int svo_ctmf(svo_ctx* ctx, const uint8_t* src, uint8_t* dst, int width, int height, int src_step,
                        int dst_step, int r, int channels) {
  if (!ctx) return SVO_E_INVALID;
  if (!src || !dst || width < 1 || height < 1 || channels < 1 || channels > 4 || r < 1 || r > 3 ||
      src_step < width * channels || dst_step < width * channels) {
    ctx->last_error = "svo_ctmf: invalid argument (radius 1..3, 1..4 channels)";
    return SVO_E_INVALID;
  }
  SVO_HIP(ctx, hipSetDevice(ctx->device));
  const size_t sbytes = (size_t)src_step * height, dbytes = (size_t)dst_step * height;
  uint8_t *d_src = nullptr, *d_dst = nullptr;
  SVO_HIP(ctx, hipMalloc(reinterpret_cast<void**>(&d_src), sbytes));
  if (hipMalloc(reinterpret_cast<void**>(&d_dst), dbytes) != hipSuccess) { hipFree(d_src); ctx->last_error = "svo_ctmf: hipMalloc"; return SVO_E_HIP; }
  int rc = SVO_OK;
  hipStream_t s = ctx->stream;
  const dim3 grid((width * channels + 255) / 256, height);
  if (hipMemcpyAsync(d_src, src, sbytes, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(d_dst, dst, dbytes, hipMemcpyHostToDevice, s) != hipSuccess) rc = SVO_E_HIP;   // keep dst padding
  if (rc == SVO_OK) {
    SvoTimer t(ctx, "k_ctmf");
    if (r == 1) hipLaunchKernelGGL(k_ctmf<1>, grid, dim3(256), 0, s, d_src, d_dst, width, height, src_step, dst_step, channels);
    else if (r == 2) hipLaunchKernelGGL(k_ctmf<2>, grid, dim3(256), 0, s, d_src, d_dst, width, height, src_step, dst_step, channels);
    else hipLaunchKernelGGL(k_ctmf<3>, grid, dim3(256), 0, s, d_src, d_dst, width, height, src_step, dst_step, channels);
  }
  if (rc == SVO_OK && (hipMemcpyAsync(dst, d_dst, dbytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
                       hipStreamSynchronize(s) != hipSuccess)) rc = SVO_E_HIP;
  hipFree(d_src); hipFree(d_dst);
  if (rc) ctx->last_error = "svo_ctmf: HIP error";
  return rc;
}

// ---- MSA::solve: what the chunk solver below needs besides the stages above ------------------------------------
namespace {

__global__ void k_msa_scale(const uint8_t* d, int n, int scale, uint8_t* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (uint8_t)(d[i] * scale);
}

}  // namespace
extern "C" int svo_msa_tree(const uint8_t* m_img3, const double* r_gra, const double* c_gra, int width, int height, int32_t* seq,
                            int32_t* child_ptr, int32_t* child, uint8_t* child_c, int32_t* root);
namespace {
struct HostTree {                       // what svo_msa_tree returns, plus what the level-by-level sweep needs
  std::vector<int32_t> seq, child_ptr, child, parent, nodes, level_ptr, depth_, fill_;
  std::vector<uint8_t> child_c, parent_c;
  int32_t root = -1;
  int rc = SVO_OK;
  // What k_msa_dp_bfs needs - the records by level-order position, the level boundaries, the widest level - in ONE pass over
  // the breadth-first sequence: `seq` IS the level order (a node's children sit at consecutive positions right after those of
  // the nodes before it), so a node's position, its parent's position and its depth are known when its parent is visited.
  // The by-pixel arrays of the level-launch fallback (nodes, parent, parent_c) are left to levels_full(); bfs_ok = false
  // sends the caller there (cannot happen for a breadth-first seq).  Round 4: the five passes of levels_full() were 12 % of a
  // tree's host time.
  void levels(int N) {
    rec.resize(N);
    ppos_.resize(N); pc_.resize(N); dpos_.resize(N);
    ppos_[0] = -1; pc_[0] = 0; dpos_[0] = 0;
    level_ptr.clear(); level_ptr.push_back(0);
    int cpos = 1, w = 0, level_start = 0;
    bool ok = true;
    for (int g = 0; g < N; ++g) {
      if (g >= cpos) { ok = false; break; }          // position g was never handed out: not a tree in breadth-first order
      const int u = seq[g], e0 = child_ptr[u], nch = child_ptr[u + 1] - e0;
      if (dpos_[g] != dpos_[level_start]) {          // first node of the next level
        w = std::max(w, g - level_start);
        level_ptr.push_back(g);
        level_start = g;
      }
      if (nch > 255 || cpos + nch > N) { ok = false; break; }
      for (int j = 0; j < nch; ++j) {
        if (seq[cpos + j] != child[e0 + j]) { ok = false; break; }
        ppos_[cpos + j] = g; pc_[cpos + j] = child_c[e0 + j]; dpos_[cpos + j] = dpos_[g] + 1;
      }
      if (!ok) break;
      rec[g] = MsaBfsRec{cpos, (int32_t)pc_[g] | (nch << 8), ppos_[g], u};
      cpos += nch;
    }
    if (ok && cpos == N) {
      w = std::max(w, N - level_start);
      level_ptr.push_back(N);
      maxw = w;
      bfs_ok = true;
      full_ = false;
      return;
    }
    levels_full(N);
  }
  // The tree of one image, ready for k_msa_dp_bfs: svo_msa_tree_rec writes the level-order records and the level boundaries
  // WHILE it walks the tree breadth-first (round 5: the breadth-first sequence, the child lists in CSR form and levels() were
  // three passes over the tree with random access each - 15 % of a tree's host time).  The by-pixel arrays (seq, child lists)
  // exist only on the fallback path (SVO_MSA_LEVEL_LAUNCHES, or a node with more than 255 children).
  void build(const uint8_t* med3, const double* r_gra, const double* c_gra, int m, int n) {
    const int N = n * m;
    if (!msa_level_launches()) {
      rec.resize(N);
      rc = svo_msa_tree_rec(med3, r_gra, c_gra, m, n, rec.data(), &level_ptr, &maxw, &root);
      if (rc == SVO_OK) { bfs_ok = true; full_ = false; have_csr_ = false; return; }
      if (rc != SVO_E_CAPACITY) return;
    }
    seq.resize(N); child_ptr.resize(N + 1); child.resize(N); child_c.resize(N);
    rc = svo_msa_tree(med3, r_gra, c_gra, m, n, seq.data(), child_ptr.data(), child.data(), child_c.data(), &root);
    have_csr_ = true;
    if (rc == SVO_OK) levels(N);
  }
  bool have_csr_ = false;
  // the level-launch fallback's arrays, on demand (the child lists by pixel are read back from the records if need be)
  void need_full(int N) {
    if (full_) return;
    if (!have_csr_) {
      seq.resize(N); child_ptr.assign(N + 1, 0); child.resize(N); child_c.resize(N);
      for (int g = 0; g < N; ++g) { seq[g] = rec[g].node; child_ptr[rec[g].node + 1] = (rec[g].meta >> 8) & 255; }
      for (int u = 0; u < N; ++u) child_ptr[u + 1] += child_ptr[u];
      for (int g = 0; g < N; ++g) {
        const int e0 = child_ptr[rec[g].node], nch = (rec[g].meta >> 8) & 255;
        for (int j = 0; j < nch; ++j) { child[e0 + j] = rec[rec[g].cpos + j].node; child_c[e0 + j] = (uint8_t)(rec[rec[g].cpos + j].meta & 255); }
      }
      have_csr_ = true;
    }
    levels_full(N);
  }
  void levels_full(int N) {
    full_ = true;
    parent.assign(N, -1); parent_c.assign(N, 0);
    std::vector<int32_t>& depth = depth_;
    depth.assign(N, 0);
    int max_depth = 0;
    for (int k = 0; k < N; ++k) {
      const int u = seq[k];
      for (int e = child_ptr[u]; e < child_ptr[u + 1]; ++e) {
        const int v = child[e];
        parent[v] = u; parent_c[v] = child_c[e]; depth[v] = depth[u] + 1;
        max_depth = std::max(max_depth, depth[v]);
      }
    }
    level_ptr.assign(max_depth + 2, 0);
    for (int v = 0; v < N; ++v) ++level_ptr[depth[v] + 1];
    for (int l = 0; l <= max_depth; ++l) level_ptr[l + 1] += level_ptr[l];
    fill_.assign(level_ptr.begin(), level_ptr.end() - 1);
    nodes.resize(N);
    for (int k = 0; k < N; ++k) nodes[fill_[depth[seq[k]]]++] = seq[k];
    bfs_ok = msa_bfs_records(N, nodes.data(), level_ptr, child_ptr.data(), child.data(), parent.data(), parent_c.data(), fill_, rec, &maxw);
  }
  std::vector<MsaBfsRec> rec;   // the tree by level-order position (k_msa_dp_bfs)
  int maxw = 0;                 // widest level
  bool bfs_ok = false;          // children are consecutive in level order (always, for a breadth-first seq)
  bool full_ = false;           // nodes / parent / parent_c are filled in
  std::vector<int32_t> ppos_, dpos_;
  std::vector<uint8_t> pc_;
};

struct MsaHostStore {   // what a solve downloads, builds and uploads; the next solve on the same arena uses the buffers again
  std::vector<HostTree> tree;               // 2b: left image of pair b, 2b + 1: right image
  std::vector<std::vector<uint8_t>> med;    // their median images
  std::vector<std::vector<double>> gra;     // per pair: r_graL c_graL r_graR c_graR
  std::vector<MsaTab> tabs;                 // [side * C + b]
  double Exp[512];                          // the weights of the first two aggregations | of the refinement
};

__global__ void k_msa_gray_to_bgr(const uint8_t* gray, int stride, int m, int n, uint8_t* bgr) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= m) return;
  const uint8_t v = gray[(size_t)i * stride + j];
  uint8_t* o = bgr + ((size_t)i * m + j) * 3;
  o[0] = v; o[1] = v; o[2] = v;
}
__global__ void k_msa_to_float(const uint8_t* d, int n, float* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (float)d[i];
}

}  // namespace

// MSA's input image in its tight 8UC3 layout: B = G = R copies of a gray image on the device (what a grayscale file read as
// colour gives), or a pitched copy of a colour image on the device (the colour entries, main.cpp:160-161)
static hipError_t msa_load_img3(hipStream_t st, const uint8_t* src, int pitch, bool bgr, int m, int n, uint8_t* img3) {
  if (bgr) return hipMemcpy2DAsync(img3, 3 * (size_t)m, src, pitch, 3 * (size_t)m, n, hipMemcpyDeviceToDevice, st);
  hipLaunchKernelGGL(k_msa_gray_to_bgr, dim3((m + 255) / 256, n), dim3(256), 0, st, src, pitch, m, n, img3);
  return hipSuccess;
}

// ------------------------------------------------------------------------------------------------------------
// MSA::solve (MSA.cpp:1132-1169) for C >= 1 pairs together, on stream `s` with the buffers of arena `ar`: everything per
// pixel / per node on the GPU and resident there (the cost volumes never leave HBM), the 2C aggregation trees on host
// threads in between, then every stage of the aggregation once for the whole chunk - the sweeps of all trees in one
// launch (one per level on the fallback path), the per-pixel stages over the maps stacked into one tall image.
// Pair b: rows `pitch` bytes apart at dL / dR + b * frame_stride, gray or (bgr) 8UC3.  The C disparity maps (uint8, n x m
// each) are left in the arena; `emit` enqueues whatever turns them into the caller's output before the final wait.
// With two lanes alternating over the chunks (svo_msa_run_many_dev), host_phase is held over the tree builders and
// gpu_phase from the tree upload to the end, so that the trees of one chunk grow while the GPU aggregates the previous
// one and initialises the next.
// ------------------------------------------------------------------------------------------------------------
static int msa_chunk_device(svo_ctx* ctx, hipStream_t s, MsaArena& ar, const uint8_t* dL, const uint8_t* dR, int pitch,
                            size_t frame_stride, bool bgr, int m, int n, int d, int C, std::mutex* host_phase, std::mutex* gpu_phase,
                            const std::function<void(const uint8_t*)>& emit) {
  const bool dbg = getenv("SVO_MSA_DEBUG") != nullptr;
  auto t_last = std::chrono::steady_clock::now();
  auto mark = [&](const char* name) {   // wall clock of a host-visible stage: a profile entry, a line under SVO_MSA_DEBUG
    { HostTimer t(ctx, name); t.t0 = t_last; }
    const auto now = std::chrono::steady_clock::now();
    if (dbg) fprintf(stderr, "[msa x%d] %-30s %8.2f ms\n", C, name, std::chrono::duration<double, std::milli>(now - t_last).count());
    t_last = now;
  };
  const int D = d + 1, T2 = 2 * C;
  const size_t N = (size_t)n * m, V = N * D;
  DevBuf& buf = ar.dev;
  uint8_t* img3[2] = {buf.get<uint8_t>(3 * N), buf.get<uint8_t>(3 * N)};   // one pair as tight 8UC3, when the caller's is not
  uint8_t* med3[2] = {buf.get<uint8_t>(3 * N), buf.get<uint8_t>(3 * N)};
  uint8_t* gray = buf.get<uint8_t>(N);
  double* g = buf.get<double>(6 * N);                                      // graL graR r_graL c_graL r_graR c_graR
  float* cost = buf.get<float>(V * T2);                                    // [side * C + b][pixel][disparity]: costL, costR
  float* d_up = buf.get<float>(V * T2); float* d_A = buf.get<float>(V * T2);   // the aggregations' work and result volumes, same index
  uint8_t* d_disp = buf.get<uint8_t>(N * T2); uint8_t* d_raw = buf.get<uint8_t>(N * T2);
  uint8_t* d_mask = buf.get<uint8_t>(N * C);
  double* d_Exp = buf.get<double>(512);
  MsaBfsRec* d_rec = buf.get<MsaBfsRec>(N * T2);
  int32_t* d_lp = buf.get<int32_t>((N + 1) * T2);
  MsaTab* d_tabs = buf.get<MsaTab>(T2);
  if (!img3[0] || !img3[1] || !med3[0] || !med3[1] || !gray || !g || !cost || !d_up || !d_A || !d_disp || !d_raw || !d_mask ||
      !d_Exp || !d_rec || !d_lp || !d_tabs) {
    ctx->last_error = "svo_msa_solve: hipMalloc";
    return SVO_E_NOMEM;
  }
  if (!ar.host) ar.host = new MsaHostStore();
  MsaHostStore& hs = *ar.host;
  if ((int)hs.tree.size() < T2) { hs.tree.resize(T2); hs.med.resize(T2); }
  if ((int)hs.gra.size() < C) hs.gra.resize(C);
  for (int k = 0; k < T2; ++k) hs.med[k].resize(3 * N);
  for (int b = 0; b < C; ++b) hs.gra[b].resize(4 * N);
  hs.tabs.resize(T2);
  mark("host_msa_alloc");
  const dim3 px((m + 255) / 256, n);
  const unsigned nbN = (unsigned)((N + 255) / 256), nbV = (unsigned)((V + 255) / 256);

  // 1. MSA::init per pair; the median images and their gradients go to the host for the tree builders
  const bool in_place = bgr && pitch == 3 * m;
  for (int b = 0; b < C; ++b) {
    const uint8_t* im[2] = {dL + b * frame_stride, dR + b * frame_stride};
    for (int side = 0; side < 2 && !in_place; ++side) {
      SVO_HIP(ctx, msa_load_img3(s, im[side], pitch, bgr, m, n, img3[side]));
      im[side] = img3[side];
    }
    float* cL = cost + (size_t)b * V;
    float* cR = cost + (size_t)(C + b) * V;
    {
      SvoTimer t(ctx, "k_msa_init", s);
      for (int side = 0; side < 2; ++side) {
        hipLaunchKernelGGL(k_msa_gray, dim3(nbN), dim3(256), 0, s, im[side], (int)N, gray);
        hipLaunchKernelGGL(k_msa_gradient, px, dim3(256), 0, s, gray, n, m, 1, 127.5, g + side * N);
      }
      hipLaunchKernelGGL(k_msa_cost, dim3(nbV), dim3(256), 0, s, im[0], im[1], g, g + N, n, m, D, cL);
      hipLaunchKernelGGL(k_msa_cost_right, dim3(nbV), dim3(256), 0, s, cL, n, m, D, cR);
      for (int side = 0; side < 2; ++side) {
        hipLaunchKernelGGL(k_ctmf<1>, dim3((3 * m + 255) / 256, n), dim3(256), 0, s, im[side], med3[side], m, n, 3 * m, 3 * m, 3);
        hipLaunchKernelGGL(k_msa_gray, dim3(nbN), dim3(256), 0, s, med3[side], (int)N, gray);
        hipLaunchKernelGGL(k_msa_gradient, px, dim3(256), 0, s, gray, n, m, 1, 0.0, g + (2 + 2 * side) * N);
        hipLaunchKernelGGL(k_msa_gradient, px, dim3(256), 0, s, gray, n, m, 0, 0.0, g + (3 + 2 * side) * N);
      }
    }
    for (int side = 0; side < 2; ++side) SVO_HIP(ctx, hipMemcpyAsync(hs.med[2 * b + side].data(), med3[side], 3 * N, hipMemcpyDeviceToHost, s));
    SVO_HIP(ctx, hipMemcpyAsync(hs.gra[b].data(), g + 2 * N, 4 * N * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  SVO_HIP(ctx, hipStreamSynchronize(s));
  mark("host_msa_init_and_download");

  // 2. the 2C trees, on as many host threads as are sensible (the reference builds a pair's two one after the other).  A
  // lane's init kernels and downloads - its own arena - have run while the other lane built its trees.
  std::unique_lock<std::mutex> host_lock;
  if (host_phase) host_lock = std::unique_lock<std::mutex>(*host_phase);
  std::vector<HostTree>& tree = hs.tree;
  {
    std::atomic<int> next(0);
    auto work = [&]() {
      for (int k = next.fetch_add(1); k < T2; k = next.fetch_add(1)) {
        const double* gra = hs.gra[k >> 1].data() + 2 * (k & 1) * N;
        tree[k].build(hs.med[k].data(), gra, gra + N, m, n);
      }
    };
    const int T = std::max(1, std::min(std::min(T2, 32), 2 * svo_host_cpus()));   // (measured on a 16-CPU quota: 32 builders 58 frames/s, 16: 51, 64: 36)
    std::vector<std::thread> pool;
    for (int t = 1; t < T; ++t) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
  }
  mark("host_msa_trees");
  for (int k = 0; k < T2; ++k)
    if (tree[k].rc) { ctx->last_error = "svo_msa_solve: tree construction failed"; return tree[k].rc; }
  if (host_lock.owns_lock()) host_lock.unlock();
  std::unique_lock<std::mutex> gpu_lock;
  if (gpu_phase) gpu_lock = std::unique_lock<std::mutex>(*gpu_phase);

  // 3. trees to the device, tabs[side * C + b]: in level order, or by pixel when some tree of the chunk needs the level launches
  MsaDpPlan plan;
  for (int k = 0; k < T2; ++k) plan.add(tree[k].level_ptr, tree[k].bfs_ok);
  plan.decide(ctx, D);
  for (int k = 0; k < T2; ++k) {
    HostTree& t = tree[k];
    if (!plan.bfs) t.need_full((int)N);   // (rewrites level_ptr, to the same values: before its copy is enqueued)
    const size_t i = (size_t)(k & 1) * C + (k >> 1);
    const int levels = (int)t.level_ptr.size() - 1;
    MsaTab& tab = hs.tabs[i];
    tab = MsaTab{d_rec + i * N, d_lp + i * (N + 1), levels, (int32_t)N, cost + i * V, d_up + i * V, d_A + i * V,
                 nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    SVO_HIP(ctx, hipMemcpyAsync(d_lp + i * (N + 1), t.level_ptr.data(), (size_t)(levels + 1) * 4, hipMemcpyHostToDevice, s));
    if (plan.bfs) {
      SVO_HIP(ctx, hipMemcpyAsync(d_rec + i * N, t.rec.data(), N * sizeof(MsaBfsRec), hipMemcpyHostToDevice, s));
      continue;
    }
    if (const int rc = msa_upload_by_pixel(ctx, s, buf, (int)N, t.nodes.data(), t.child_ptr.data(), t.child.data(), t.child_c.data(),
                                           t.parent.data(), t.parent_c.data(), tab)) return rc;
  }
  SVO_HIP(ctx, hipMemcpyAsync(d_tabs, hs.tabs.data(), sizeof(MsaTab) * T2, hipMemcpyHostToDevice, s));
  for (int i = 0; i <= 255; ++i) { hs.Exp[i] = exp(-i * 1.0 / 0.1 / 255); hs.Exp[256 + i] = exp(-i * 1.0 / (0.1 / 2) / 255); }
  SVO_HIP(ctx, hipMemcpyAsync(d_Exp, hs.Exp, sizeof hs.Exp, hipMemcpyHostToDevice, s));

  // 4. TreeDp + WTA for the right and the left images (one launch: they are independent until the L/R check), the L/R
  // check, TreeDp + WTA again over the left trees with the sharper weights and the checked costs
  auto wta = [&](int maps) {   // first minimum + 5x5 median of the maps [0, maps)
    SvoTimer tm(ctx, "k_msa_wta", s);
    hipLaunchKernelGGL(k_msa_argmin, dim3((unsigned)((N * maps + 255) / 256)), dim3(256), 0, s, d_A, (int)(N * maps), D, d_raw);
    for (int k = 0; k < maps; ++k)
      hipLaunchKernelGGL(k_ctmf<2>, px, dim3(256), 0, s, d_raw + (size_t)k * N, d_disp + (size_t)k * N, m, n, m, m, 1);
  };
  {
    SvoTimer tm(ctx, "k_msa_tree_dp", s);
    msa_aggregate(s, d_tabs, T2, (int)N, D, d_Exp, plan);
  }
  wta(T2);
  {
    SvoTimer tm(ctx, "k_msa_lrcheck", s);   // the C maps as one tall image: the check only looks along a row
    hipLaunchKernelGGL(k_msa_lrcheck, dim3((unsigned)((V * C + 255) / 256)), dim3(256), 0, s, d_disp, d_disp + N * C, n * C, m, D, cost, d_mask);
  }
  {
    SvoTimer tm(ctx, "k_msa_tree_dp", s);
    msa_aggregate(s, d_tabs, C, (int)N, D, d_Exp + 256, plan);
  }
  wta(C);
  emit(d_disp);
  mark("host_msa_enqueue_aggregation");
  SVO_HIP(ctx, hipStreamSynchronize(s));
  mark("host_msa_wait_aggregation");
  SVO_HIP(ctx, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_msa_solve(svo_ctx* ctx, const uint8_t* bgrL, const uint8_t* bgrR, int width, int height, int step, int d,
                             int scale, uint8_t* disparity) {
  if (!ctx) return SVO_E_INVALID;
  const int n = height, m = width, D = d + 1;
  if (!bgrL || !bgrR || !disparity || n < 5 || m < 5 || d < 0 || D > 256 || step < 3 * m || scale < 1 ||
      (size_t)n * m * D > (size_t)1 << 30 || (int64_t)n * m > (1 << 24)) {
    ctx->last_error = "svo_msa_solve: invalid argument";
    return SVO_E_INVALID;
  }
  SVO_HIP(ctx, hipSetDevice(ctx->device));
  const size_t N = (size_t)n * m;
  MsaArena& ar = msa_arena(ctx, 0);
  uint8_t* img3[2] = {ar.io.get<uint8_t>(3 * N), ar.io.get<uint8_t>(3 * N)};
  uint8_t* d_out = ar.io.get<uint8_t>(N);
  if (!img3[0] || !img3[1] || !d_out) { ctx->last_error = "svo_msa_solve: hipMalloc"; return SVO_E_NOMEM; }
  hipStream_t s = ctx->stream;
  if (ctx->h_pinned && 6 * N + 4096 <= ctx->pinned_bytes) {   // (the buffer's last page belongs to svo_track_frame's boxes)
    // rows gathered into the pinned buffer, one linear copy per image (a 2-D copy from pageable memory costs ~10 ms)
    const uint8_t* src[2] = {bgrL, bgrR};
    for (int side = 0; side < 2; ++side) {
      uint8_t* h = reinterpret_cast<uint8_t*>(ctx->h_pinned) + 3 * N * side;
      for (int y = 0; y < n; ++y) memcpy(h + (size_t)y * 3 * m, src[side] + (size_t)y * step, 3 * (size_t)m);
      SVO_HIP(ctx, hipMemcpyAsync(img3[side], h, 3 * N, hipMemcpyHostToDevice, s));
    }
  } else {
    SVO_HIP(ctx, hipMemcpy2DAsync(img3[0], 3 * (size_t)m, bgrL, step, 3 * (size_t)m, n, hipMemcpyHostToDevice, s));
    SVO_HIP(ctx, hipMemcpy2DAsync(img3[1], 3 * (size_t)m, bgrR, step, 3 * (size_t)m, n, hipMemcpyHostToDevice, s));
  }
  const int rc = msa_chunk_device(ctx, s, ar, img3[0], img3[1], 3 * m, 0, true, m, n, d, 1, nullptr, nullptr, [&](const uint8_t* maps) {
    hipLaunchKernelGGL(k_msa_scale, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, maps, (int)N, scale, d_out);
  });
  if (rc) return rc;
  SVO_HIP(ctx, svo_memcpy_sync(ctx, disparity, d_out, N, hipMemcpyDeviceToHost));
  return SVO_OK;
}

// frame::MB (src/frame.cc:82-91) for the tracker's dense-depth mode: C gray or colour pairs already on the device, the
// disparities as CV_32F like `disp_img.convertTo(disp_32f, CV_32F, 1)` at d_disp
static int msa_float_chunk(svo_ctx* ctx, hipStream_t s, int arena, const uint8_t* dL, const uint8_t* dR, int pitch, size_t frame_stride,
                           int W, int H, int d, int C, float* d_disp, std::mutex* host_phase, std::mutex* gpu_phase, bool bgr) {
  const size_t NC = (size_t)W * H * C;
  return msa_chunk_device(ctx, s, msa_arena(ctx, arena), dL, dR, pitch, frame_stride, bgr, W, H, d, C, host_phase, gpu_phase,
                          [&](const uint8_t* maps) {
    hipLaunchKernelGGL(k_msa_to_float, dim3((unsigned)((NC + 255) / 256)), dim3(256), 0, s, maps, (int)NC, d_disp);
  });
}

int svo_msa_run_dev(svo_ctx* ctx, const uint8_t* dL, const uint8_t* dR, int pitch, int W, int H, int d, float* d_disp, bool bgr) {
  if (H < 5 || W < 5 || d < 0 || d > 255) return SVO_E_INVALID;
  return msa_float_chunk(ctx, ctx->stream, 0, dL, dR, pitch, 0, W, H, d, 1, d_disp, nullptr, nullptr, bgr);
}

// B frames (frame b at dL + b * frame_stride bytes, map b at d_disp + b * W * H floats), solved in chunks that share
// their launches and build their trees side by side.
int svo_msa_run_many_dev(svo_ctx* ctx, const uint8_t* dL, const uint8_t* dR, int pitch, size_t frame_stride, int W, int H, int d,
                         int B, float* d_disp, bool bgr) {
  const size_t N = (size_t)W * H;
  if (B <= 1 || ctx->profiling || (int64_t)N * (d + 1) * 16 > ((int64_t)1 << 31) || getenv("SVO_MSA_FRAME_BY_FRAME")) {
    for (int b = 0; b < B; ++b) {
      const int rc = svo_msa_run_dev(ctx, dL + b * frame_stride, dR + b * frame_stride, pitch, W, H, d, d_disp + b * N, bgr);
      if (rc) return rc;
    }
    return SVO_OK;
  }
  // chunks of up to 16 frames: ~0.55 GB of HBM per frame at KITTI size (six cost-sized volumes: two costs, and a work and a
  // result volume for each of the two aggregations that share a launch)
  const int nchunk = (B + 15) / 16;
  if (nchunk == 1) return msa_float_chunk(ctx, ctx->stream, 1, dL, dR, pitch, frame_stride, W, H, d, B, d_disp, nullptr, nullptr, bgr);
  // two lanes (threads, streams, arenas) take the chunks alternately
  SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));   // whatever produced the frames
  std::mutex host_phase, gpu_phase;
  hipStream_t st[2] = {nullptr, nullptr};
  for (int t = 0; t < 2; ++t) SVO_HIP(ctx, hipStreamCreateWithFlags(&st[t], hipStreamNonBlocking));
  int rcs[2] = {SVO_OK, SVO_OK};
  auto lane_work = [&](int t) {
    if (hipSetDevice(ctx->device) != hipSuccess) { rcs[t] = SVO_E_HIP; return; }
    for (int c = t; c < nchunk; c += 2) {
      const int b0 = 16 * c, C = std::min(16, B - b0);
      const int rc = msa_float_chunk(ctx, st[t], 1 + t, dL + b0 * frame_stride, dR + b0 * frame_stride, pitch, frame_stride, W, H, d, C,
                                     d_disp + b0 * N, &host_phase, &gpu_phase, bgr);
      if (rc) { rcs[t] = rc; return; }
    }
  };
  {
    std::thread other(lane_work, 1);
    lane_work(0);
    other.join();
  }
  for (int t = 0; t < 2; ++t) hipStreamDestroy(st[t]);
  return rcs[0] ? rcs[0] : rcs[1];
}

extern "C" int svo_msa_batch_dev(svo_ctx* ctx, const uint8_t* d_L, const uint8_t* d_R, int stride, int width, int height, int B,
                                 int d, float* d_disp) {
  if (!ctx) return SVO_E_INVALID;
  if (!d_L || !d_R || !d_disp || B < 1 || width < 5 || height < 5 || stride < width || d < 0 || d > 255 ||
      (int64_t)width * height > (1 << 24)) {
    ctx->last_error = "svo_msa_batch_dev: invalid argument";
    return SVO_E_INVALID;
  }
  SVO_HIP(ctx, hipSetDevice(ctx->device));
  return svo_msa_run_many_dev(ctx, d_L, d_R, stride, (size_t)height * stride, width, height, d, B, d_disp);
}

void svo_msa_release(svo_ctx* ctx) {
  if (!ctx || !ctx->msa_arenas) return;
  MsaArenas* A = static_cast<MsaArenas*>(ctx->msa_arenas);
  for (MsaArena* a : A->a) { delete a->host; delete a; }
  delete A;
  ctx->msa_arenas = nullptr;
}
