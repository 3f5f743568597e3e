// svo_loop.hip - loop verification on the device (svo_loop_* in include/svo.h): ORB-SLAM2's ORBmatcher::SearchByBoW over two
// frames' FeatureVectors and Sim3Solver with the scale fixed to 1 (Horn's closed form inside RANSAC) over the matched map points.
// The contract, operation by operation: DESIGN.md section 8 "Loop verification"; the numpy twin: tests/loop_ref.py.
//
// An object of its own on a stream of its own, like the vocabulary (svo_bow.hip): nothing here runs on another object's streams;
// svo_loop_wait records an event on a producer's stream and makes the object's stream wait for it, nothing else.
//
// Three kernels, 256 threads a workgroup:
//   k_loop_pairs  a thread per candidate slot: (q0 + i, cand.frame) or (-1, -1).
//   k_loop_match  a workgroup per pair.  The heads of the node runs of a's FeatureVector look their node up in b's (binary search);
//                 a common node is a task, the four waves take tasks from a counter.  Within a task the i1 are a dependent chain on
//                 ONE wave; b's features of the node are spread over the lanes, 64 a chunk, a lane keeps "has a map point and is
//                 not matched yet" of its positions as one bit per chunk in a register (a node has at most 2048 / 64 = 32 chunks).
//                 A lane does 8 x (xor, popcount) per position and keeps its two smallest keys (dist << 11 | position); the best is
//                 the wave's minimum, the second best the minimum of what is left.  Then the whole workgroup takes the 30-bin
//                 histogram, one thread the three maxima, and the matches of the other bins go.
//   k_loop_solve  a workgroup per pair.  The correspondences are gathered once, in ascending i1 (ballot prefix), into the object's
//                 scratch (12 float64 a correspondence, field by field so that lanes read side by side).  Iterations run 256 at a
//                 time: a lane draws the sample of its iteration and takes Horn's alignment (the 4 x 4 Jacobi in registers), then a
//                 wave counts the inliers of 64 hypotheses one after the other, its lanes over the correspondences; ONE thread
//                 replays the sequential rule over the counts after every 256.  The refit sums over the inliers by ONE thread.
// No floating-point atomics, no device log / pow / atan2 (the iteration bounds are a table made on the host), every ordered sum
// taken by one thread: the same bytes on every run.
//
// Not here: SearchBySim3, OptimizeSim3, scale estimation, covisibility consistency, loop correction, feedback into the tracker.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "svo_internal.h"
#include "svo_wave.h"

namespace {

constexpr int LOOP_NT = 256;
constexpr int LOOP_WAVES = LOOP_NT / 64;
constexpr int LOOP_MAX_KP = 2048;
constexpr int LOOP_MAX_ITS = 1024;
constexpr int LOOP_NF = 12;              // float64 values of a correspondence: Xc1, Xc2, p1, p2, maxerr1, maxerr2
constexpr int LOOP_SWEEPS = 12;          // the 4 x 4 Jacobi's most sweeps
constexpr int LOOP_NONE = 0x7fffffff;

__device__ __forceinline__ int loop_clamp(int v, int hi) { return min(max(v, 0), hi); }

// ---- candidates -> pairs ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(LOOP_NT) k_loop_pairs(const svo_bow_cand* cand, const int32_t* cand_n, int q0, int Q, int top_k,
                                                        int32_t* pairs) {
  const int s = blockIdx.x * LOOP_NT + threadIdx.x;
  if (s >= Q * top_k) return;
  const int i = s / top_k, t = s - i * top_k;
  int a = -1, b = -1;
  if (t < loop_clamp(cand_n[i], top_k)) {
    const int f = cand[s].frame;
    if (f >= 0) { a = q0 + i; b = f; }
  }
  pairs[2 * s] = a;
  pairs[2 * s + 1] = b;
}

// ---- SearchByBoW -----------------------------------------------------------------------------------------------------------------
struct MatchArgs {
  const uint8_t* desc; const svo_kp* kp; const int32_t* n; int kp_stride;
  const svo_bow_feature* fv; const int32_t* fv_n;
  const svo_map_obs* obs; const int32_t* obs_n; int obs_stride;
  const int32_t* pairs;
  int th_low; float nn_ratio; int check_orientation;
  int32_t* match; int32_t* match_n;
};

// C round(): a half goes away from zero (x is finite here or the bin is refused)
__device__ __forceinline__ int loop_bin(float a1, float a2) {
  float rot = a1 - a2;
  if (rot < 0.0f) rot += 360.0f;
  const float x = rot * (1.0f / 30);
  if (!(x > -1000.0f && x < 1000.0f)) return -1;
  int b = (int)roundf(x);
  if (b == 30) b = 0;
  return (b >= 0 && b < 30) ? b : -1;
}

__global__ void __launch_bounds__(LOOP_NT) k_loop_match(MatchArgs A) {
  __shared__ uint32_t mpA[LOOP_MAX_KP / 32], mpB[LOOP_MAX_KP / 32];   // "has a map point"
  __shared__ int32_t s_match[LOOP_MAX_KP];
  __shared__ uint16_t taskA[LOOP_MAX_KP], taskB[LOOP_MAX_KP];         // a common node: where its run starts in either vector
  __shared__ int s_ntask, s_next, s_cnt, hist[30], keep[3];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int S = A.kp_stride;
  int32_t* out = A.match + (size_t)p * S;
  const int fa = A.pairs[2 * p], fb = A.pairs[2 * p + 1];
  if (fa < 0 || fb < 0) {     // skipped: as for "no match"
    for (int i = tid; i < S; i += LOOP_NT) out[i] = -1;
    if (tid == 0) A.match_n[p] = 0;
    return;
  }
  const int nA = loop_clamp(A.n[fa], S), nB = loop_clamp(A.n[fb], S);
  const int nfA = loop_clamp(A.fv_n[fa], S), nfB = loop_clamp(A.fv_n[fb], S);
  const int noA = loop_clamp(A.obs_n[fa], A.obs_stride), noB = loop_clamp(A.obs_n[fb], A.obs_stride);
  const svo_bow_feature* fvA = A.fv + (size_t)fa * S;
  const svo_bow_feature* fvB = A.fv + (size_t)fb * S;
  const svo_map_obs* obA = A.obs + (size_t)fa * A.obs_stride;
  const svo_map_obs* obB = A.obs + (size_t)fb * A.obs_stride;
  for (int i = tid; i < LOOP_MAX_KP / 32; i += LOOP_NT) { mpA[i] = 0; mpB[i] = 0; }
  for (int i = tid; i < S; i += LOOP_NT) s_match[i] = -1;
  if (tid < 30) hist[tid] = 0;
  if (tid == 0) { s_ntask = 0; s_next = 0; s_cnt = 0; }
  __syncthreads();
  for (int i = tid; i < noA; i += LOOP_NT) {
    const int k = obA[i].kp;
    if (k >= 0 && k < nA) atomicOr(&mpA[k >> 5], 1u << (k & 31));
  }
  for (int i = tid; i < noB; i += LOOP_NT) {
    const int k = obB[i].kp;
    if (k >= 0 && k < nB) atomicOr(&mpB[k >> 5], 1u << (k & 31));
  }
  // the common nodes
  for (int q = tid; q < nfA; q += LOOP_NT) {
    const uint32_t node = fvA[q].node;
    if (q > 0 && fvA[q - 1].node == node) continue;
    int lo = 0, hi = nfB;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (fvB[mid].node < node) lo = mid + 1; else hi = mid;
    }
    if (lo < nfB && fvB[lo].node == node) {
      const int t = atomicAdd(&s_ntask, 1);
      taskA[t] = (uint16_t)q; taskB[t] = (uint16_t)lo;
    }
  }
  __syncthreads();
  const int ntask = s_ntask;
  for (;;) {
    int t = 0;
    if (lane == 0) t = atomicAdd(&s_next, 1);
    t = __builtin_amdgcn_readfirstlane(t);
    if (t >= ntask) break;
    const int sA = taskA[t], sB = taskB[t];
    const uint32_t node = fvA[sA].node;
    int eA = sA + 1, eB = sB + 1;
    while (eA < nfA && fvA[eA].node == node) ++eA;
    while (eB < nfB && fvB[eB].node == node) ++eB;
    const int n1 = eA - sA, n2 = eB - sB, chunks = (n2 + 63) >> 6;      // n2 <= 2048: chunks <= 32
    uint32_t avail = 0;      // bit c: position c * 64 + lane of the run has a map point and is not matched yet
    for (int c = 0; c < chunks; ++c) {
      const int pos = c * 64 + lane;
      if (pos < n2) {
        const uint32_t f2 = fvB[sB + pos].feature;
        if (f2 < (uint32_t)nB && ((mpB[f2 >> 5] >> (f2 & 31)) & 1u)) avail |= 1u << c;
      }
    }
    for (int q = 0; q < n1; ++q) {
      const uint32_t i1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)fvA[sA + q].feature);
      if (i1 >= (uint32_t)nA || !((mpA[i1 >> 5] >> (i1 & 31)) & 1u)) continue;
      const uint32_t* da = reinterpret_cast<const uint32_t*>(A.desc + ((size_t)fa * S + i1) * 32);
      uint32_t d1[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) d1[j] = da[j];
      int m1 = LOOP_NONE, m2 = LOOP_NONE;
      for (int c = 0; c < chunks; ++c) {
        if (!((avail >> c) & 1u)) continue;
        const int pos = c * 64 + lane;
        const uint32_t f2 = fvB[sB + pos].feature;
        const uint32_t* db = reinterpret_cast<const uint32_t*>(A.desc + ((size_t)fb * S + f2) * 32);
        int d = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) d += __popc(d1[j] ^ db[j]);
        const int key = (d << 11) | pos;
        if (key < m1) { m2 = m1; m1 = key; } else if (key < m2) m2 = key;
      }
      const int best = (int)wave_min_u32_dpp((uint32_t)m1);
      if (best == LOOP_NONE) continue;
      const int second = (int)wave_min_u32_dpp((uint32_t)(m1 == best ? m2 : m1));
      const int best1 = best >> 11, pos = best & 2047;
      const int best2 = second == LOOP_NONE ? 256 : second >> 11;
      if (best1 < A.th_low && (float)best1 < A.nn_ratio * (float)best2) {
        if (lane == (pos & 63)) {
          avail &= ~(1u << (pos >> 6));
          s_match[i1] = (int32_t)fvB[sB + pos].feature;
        }
      }
    }
  }
  __syncthreads();
  if (A.check_orientation) {
    const svo_kp* kA = A.kp + (size_t)fa * S;
    const svo_kp* kB = A.kp + (size_t)fb * S;
    for (int i = tid; i < nA; i += LOOP_NT) {
      const int m = s_match[i];
      if (m >= 0) {
        const int b = loop_bin(kA[i].angle, kB[m].angle);
        if (b >= 0) atomicAdd(&hist[b], 1);
      }
    }
    __syncthreads();
    if (tid == 0) {     // ComputeThreeMaxima
      int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
      for (int i = 0; i < 30; ++i) {
        const int s = hist[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
        else if (s > max3) { max3 = s; i3 = i; }
      }
      if ((float)max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
      else if ((float)max3 < 0.1f * (float)max1) i3 = -1;
      keep[0] = i1; keep[1] = i2; keep[2] = i3;
    }
    __syncthreads();
    const int k1 = keep[0], k2 = keep[1], k3 = keep[2];
    for (int i = tid; i < nA; i += LOOP_NT) {
      const int m = s_match[i];
      if (m >= 0) {
        const int b = loop_bin(kA[i].angle, kB[m].angle);
        if (b < 0 || (b != k1 && b != k2 && b != k3)) s_match[i] = -1;
      }
    }
    __syncthreads();
  }
  int mine = 0;
  for (int i = tid; i < S; i += LOOP_NT) {
    const int m = i < nA ? s_match[i] : -1;
    out[i] = m;
    mine += m >= 0;
  }
  if (mine) atomicAdd(&s_cnt, mine);
  __syncthreads();
  if (tid == 0) A.match_n[p] = s_cnt;
}

// ---- Sim3Solver, fixed scale -----------------------------------------------------------------------------------------------------
struct SolveArgs {
  const svo_kp* kp; const svo_map_obs* obs; const int32_t* obs_n; int obs_stride;
  const uint8_t* Tcw; int pose_stride;
  const int32_t* pairs; const int32_t* match; int kp_stride;
  double fx, fy, cx, cy, chi2;
  double sigma2[8];
  int min_inliers, refine;
  uint64_t seed;
  const int32_t* bounds;      // the iteration bound for N = 0 .. max_kp
  double* scratch; int cap;   // per pair LOOP_NF x cap float64
  svo_loop_result* result; uint8_t* inliers;
};

__device__ __forceinline__ uint64_t loop_splitmix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// three draws without replacement from 0 .. N - 1 (N >= 3): avail[r] taken, then avail[r] = avail[size - 1], without the array
__device__ __forceinline__ void loop_sample(uint64_t seed, int it, int N, int idx[3]) {
  const uint64_t base = seed + 3ull * (uint64_t)it;
  const int r0 = (int)__umul64hi(loop_splitmix(base), (uint64_t)N);
  const int r1 = (int)__umul64hi(loop_splitmix(base + 1), (uint64_t)(N - 1));
  const int r2 = (int)__umul64hi(loop_splitmix(base + 2), (uint64_t)(N - 2));
  const int v0 = N - 1;                              // what slot r0 holds after the first draw
  const int v1 = (N - 2 == r0) ? v0 : N - 2;         // what slot r1 holds after the second
  idx[0] = r0;
  idx[1] = (r1 == r0) ? v0 : r1;
  idx[2] = (r2 == r1) ? v1 : ((r2 == r0) ? v0 : r2);
}

struct LoopPose { double R[9], t[3]; };   // R12, t12

// The eigenvector of the largest eigenvalue of the symmetric 4 x 4 a (the lower index among equal ones) by a two-sided cyclic
// Jacobi, as a unit quaternion's rotation matrix.  Constant indices only: everything stays in registers.
__device__ __forceinline__ void loop_quat_rot(const double M[9], double R[9]) {
  double a[4][4], v[4][4];
  a[0][0] = M[0] + M[4] + M[8];
  a[0][1] = M[5] - M[7];
  a[0][2] = M[6] - M[2];
  a[0][3] = M[1] - M[3];
  a[1][1] = M[0] - M[4] - M[8];
  a[1][2] = M[1] + M[3];
  a[1][3] = M[6] + M[2];
  a[2][2] = -M[0] + M[4] - M[8];
  a[2][3] = M[5] + M[7];
  a[3][3] = -M[0] - M[4] + M[8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < i) a[i][j] = a[j][i];
      v[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < LOOP_SWEEPS; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = a[p][q];
        if (apq != 0.0) {
          const double app = a[p][p], aqq = a[q][q];
          const double g = 100.0 * fabs(apq);
          if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
            a[p][q] = 0.0; a[q][p] = 0.0;
          } else {
            rotated = true;
            const double theta = (aqq - app) / (2.0 * apq);
            const double den = fabs(theta) + sqrt(theta * theta + 1.0);
            const double t = theta < 0.0 ? -1.0 / den : 1.0 / den;
            const double c = 1.0 / sqrt(t * t + 1.0);
            const double s = t * c;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              if (k != p && k != q) {
                const double akp = a[k][p], akq = a[k][q];
                const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
                a[k][p] = np_; a[p][k] = np_;
                a[k][q] = nq_; a[q][k] = nq_;
              }
            }
            a[p][p] = app - t * apq;
            a[q][q] = aqq + t * apq;
            a[p][q] = 0.0; a[q][p] = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const double vkp = v[k][p], vkq = v[k][q];
              v[k][p] = c * vkp - s * vkq;
              v[k][q] = s * vkp + c * vkq;
            }
          }
        }
      }
    if (!rotated) break;
  }
  double best = a[0][0], w = v[0][0], x = v[1][0], y = v[2][0], z = v[3][0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (a[j][j] > best) { best = a[j][j]; w = v[0][j]; x = v[1][j]; y = v[2][j]; z = v[3][j]; }
  const double nrm = sqrt(((w * w + x * x) + y * y) + z * z);
  w = w / nrm; x = x / nrm; y = y / nrm; z = z / nrm;
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z); R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y); R[7] = 2.0 * (y * z + w * x); R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// Horn over the three correspondences idx[] of the scratch block C (field f of correspondence j: C[f * cap + j])
__device__ __forceinline__ void loop_horn3(const double* C, int cap, const int idx[3], LoopPose& H) {
  double P1[3][3], P2[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      P1[k][c] = C[(size_t)c * cap + idx[k]];
      P2[k][c] = C[(size_t)(3 + c) * cap + idx[k]];
    }
  double O1[3], O2[3], M[9];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    O1[c] = ((P1[0][c] + P1[1][c]) + P1[2][c]) / 3.0;
    O2[c] = ((P2[0][c] + P2[1][c]) + P2[2][c]) / 3.0;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) { P1[k][c] = P1[k][c] - O1[c]; P2[k][c] = P2[k][c] - O2[c]; }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[i * 3 + j] = (P2[0][i] * P1[0][j] + P2[1][i] * P1[1][j]) + P2[2][i] * P1[2][j];
  loop_quat_rot(M, H.R);
#pragma unroll
  for (int i = 0; i < 3; ++i) H.t[i] = O1[i] - ((H.R[i * 3] * O2[0] + H.R[i * 3 + 1] * O2[1]) + H.R[i * 3 + 2] * O2[2]);
}

// both reprojection tests of correspondence j under the pose (R12, t12) / (R21, t21)
__device__ __forceinline__ bool loop_inlier(const SolveArgs& A, const double* C, int j, const double R[9], const double t[3],
                                            const double t21[3]) {
  const size_t cap = (size_t)A.cap;
  const double x1 = C[j], y1 = C[cap + j], z1 = C[2 * cap + j];
  const double x2 = C[3 * cap + j], y2 = C[4 * cap + j], z2 = C[5 * cap + j];
  const double X = ((R[0] * x2 + R[1] * y2) + R[2] * z2) + t[0];
  const double Y = ((R[3] * x2 + R[4] * y2) + R[5] * z2) + t[1];
  const double Z = ((R[6] * x2 + R[7] * y2) + R[8] * z2) + t[2];
  const double du1 = C[6 * cap + j] - (A.fx * X / Z + A.cx), dv1 = C[7 * cap + j] - (A.fy * Y / Z + A.cy);
  const double e1 = du1 * du1 + dv1 * dv1;
  const double U = ((R[0] * x1 + R[3] * y1) + R[6] * z1) + t21[0];
  const double V = ((R[1] * x1 + R[4] * y1) + R[7] * z1) + t21[1];
  const double W = ((R[2] * x1 + R[5] * y1) + R[8] * z1) + t21[2];
  const double du2 = (A.fx * U / W + A.cx) - C[8 * cap + j], dv2 = (A.fy * V / W + A.cy) - C[9 * cap + j];
  const double e2 = du2 * du2 + dv2 * dv2;
  return e1 < C[10 * cap + j] && e2 < C[11 * cap + j];
}

__device__ __forceinline__ void loop_t21(const double R[9], const double t[3], double t21[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) t21[i] = -((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]);
}

__global__ void __launch_bounds__(LOOP_NT) k_loop_solve(SolveArgs A) {
  __shared__ int16_t ixA[LOOP_MAX_KP], ixB[LOOP_MAX_KP];     // keypoint -> its record, -1: no map point
  __shared__ int16_t ci1[LOOP_MAX_KP];                       // correspondence -> i1
  __shared__ uint8_t flag[LOOP_MAX_KP];
  __shared__ double hyp[12 * LOOP_NT];                       // value k of the round's hypothesis h: hyp[k * 256 + h]
  __shared__ int cnt[LOOP_MAX_ITS];
  __shared__ double s_pose[12];
  __shared__ int s_wtot[LOOP_WAVES], s_N, s_best, s_winner, s_visited, s_status, s_at, s_ninl;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = A.kp_stride;
  svo_loop_result* res = A.result + p;
  uint8_t* inl = A.inliers ? A.inliers + (size_t)p * S : nullptr;
  const int fa = A.pairs[2 * p], fb = A.pairs[2 * p + 1];
  double* C = A.scratch + (size_t)p * LOOP_NF * A.cap;
  const size_t cap = (size_t)A.cap;
  const bool skipped = fa < 0 || fb < 0;
  int N = 0;
  if (!skipped) {
    const int noA = loop_clamp(A.obs_n[fa], A.obs_stride), noB = loop_clamp(A.obs_n[fb], A.obs_stride);
    const svo_map_obs* obA = A.obs + (size_t)fa * A.obs_stride;
    const svo_map_obs* obB = A.obs + (size_t)fb * A.obs_stride;
    for (int i = tid; i < S; i += LOOP_NT) { ixA[i] = -1; ixB[i] = -1; }
    if (tid == 0) s_N = 0;
    __syncthreads();
    for (int i = tid; i < noA; i += LOOP_NT) {
      const int k = obA[i].kp;
      if (k >= 0 && k < S) ixA[k] = (int16_t)i;
    }
    for (int i = tid; i < noB; i += LOOP_NT) {
      const int k = obB[i].kp;
      if (k >= 0 && k < S) ixB[k] = (int16_t)i;
    }
    __syncthreads();
    const float* Ta = reinterpret_cast<const float*>(A.Tcw + (size_t)fa * A.pose_stride);
    const float* Tb = reinterpret_cast<const float*>(A.Tcw + (size_t)fb * A.pose_stride);
    const int32_t* mt = A.match + (size_t)p * S;
    const svo_kp* kA = A.kp + (size_t)fa * S;
    const svo_kp* kB = A.kp + (size_t)fb * S;
    // the correspondences in ascending i1
    for (int base = 0; base < S; base += LOOP_NT) {
      const int i1 = base + tid;
      int m = -1, ra = -1, rb = -1;
      if (i1 < S) {
        m = mt[i1];
        if (m >= 0 && m < S) { ra = ixA[i1]; rb = ixB[m]; }
      }
      const bool is = ra >= 0 && rb >= 0;
      const unsigned long long bal = __ballot(is);
      if (lane == 0) s_wtot[wave] = __popcll(bal);
      __syncthreads();
      int at = s_N;
      for (int w = 0; w < wave; ++w) at += s_wtot[w];
      at += __popcll(bal & ((1ull << lane) - 1ull));
      if (is) {
        const svo_map_obs oa = obA[ra], ob = obB[rb];
        double X1[3], X2[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          X1[r] = (((double)Ta[r * 4] * (double)oa.X + (double)Ta[r * 4 + 1] * (double)oa.Y) + (double)Ta[r * 4 + 2] * (double)oa.Z) +
                  (double)Ta[r * 4 + 3];
          X2[r] = (((double)Tb[r * 4] * (double)ob.X + (double)Tb[r * 4 + 1] * (double)ob.Y) + (double)Tb[r * 4 + 2] * (double)ob.Z) +
                  (double)Tb[r * 4 + 3];
          C[r * cap + at] = X1[r];
          C[(3 + r) * cap + at] = X2[r];
        }
        C[6 * cap + at] = A.fx * X1[0] / X1[2] + A.cx;
        C[7 * cap + at] = A.fy * X1[1] / X1[2] + A.cy;
        C[8 * cap + at] = A.fx * X2[0] / X2[2] + A.cx;
        C[9 * cap + at] = A.fy * X2[1] / X2[2] + A.cy;
        C[10 * cap + at] = A.chi2 * A.sigma2[loop_clamp(kA[i1].octave, 7)];
        C[11 * cap + at] = A.chi2 * A.sigma2[loop_clamp(kB[m].octave, 7)];
        ci1[at] = (int16_t)i1;
      }
      __syncthreads();
      if (tid == 0) s_N += (s_wtot[0] + s_wtot[1]) + (s_wtot[2] + s_wtot[3]);
      __syncthreads();
    }
    N = s_N;
  }
  if (inl)
    for (int i = tid; i < S; i += LOOP_NT) inl[i] = 0;
  if (skipped || N < A.min_inliers) {
    if (tid == 0) {
      svo_loop_result r;
      r.status = skipped ? SVO_LOOP_SKIPPED : SVO_LOOP_FEW;
      r.n_matches = N; r.bound = 0; r.visited = 0; r.winner = -1; r.n_inliers = 0;
      r.sample[0] = r.sample[1] = r.sample[2] = -1; r.reserved = 0;
      for (int i = 0; i < 16; ++i) r.T12[i] = (i % 5 == 0) ? 1.0 : 0.0;
      *res = r;
    }
    return;
  }
  const int bound = min(max(A.bounds[N], 1), LOOP_MAX_ITS);
  if (tid == 0) { s_best = 0; s_winner = -1; s_visited = 0; s_status = SVO_LOOP_REJECTED; s_at = 0; }
  __syncthreads();
  for (int r0 = 0; r0 < bound; r0 += LOOP_NT) {
    const int it = r0 + tid;
    if (it < bound) {
      int idx[3];
      loop_sample(A.seed, it, N, idx);
      LoopPose H;
      loop_horn3(C, A.cap, idx, H);
#pragma unroll
      for (int k = 0; k < 9; ++k) hyp[k * LOOP_NT + tid] = H.R[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) hyp[(9 + k) * LOOP_NT + tid] = H.t[k];
    }
    __syncthreads();
    for (int h = wave * 64; h < wave * 64 + 64 && r0 + h < bound; ++h) {
      double R[9], t[3], t21[3];
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = hyp[k * LOOP_NT + h];
#pragma unroll
      for (int k = 0; k < 3; ++k) t[k] = hyp[(9 + k) * LOOP_NT + h];
      loop_t21(R, t, t21);
      int c = 0;
      for (int j = lane; j < N; j += 64) c += loop_inlier(A, C, j, R, t, t21) ? 1 : 0;
      c = wave_sum_i32_dpp(c);
      if (lane == 0) cnt[r0 + h] = c;
    }
    __syncthreads();
    if (tid == 0) {     // Sim3Solver::iterate, sequentially over the counts
      const int end = min(bound, r0 + LOOP_NT);
      int i = s_at;
      for (; i < end; ++i) {
        s_visited = i + 1;
        if (cnt[i] >= s_best) {
          s_best = cnt[i]; s_winner = i;
          if (cnt[i] > A.min_inliers) { s_status = SVO_LOOP_OK; break; }
        }
      }
      s_at = i;
    }
    __syncthreads();
    if (s_status == SVO_LOOP_OK) break;
  }
  // the result's hypothesis again (every thread the same), its flags
  const int winner = s_winner;
  int idx[3];
  loop_sample(A.seed, winner, N, idx);
  LoopPose H;
  loop_horn3(C, A.cap, idx, H);
  double t21[3];
  loop_t21(H.R, H.t, t21);
  for (int j = tid; j < N; j += LOOP_NT) flag[j] = loop_inlier(A, C, j, H.R, H.t, t21) ? 1 : 0;
  __syncthreads();
  int n_inl = s_best;
  if (A.refine && n_inl > 0) {
    if (tid == 0) {     // Horn over all inliers, ascending, by one thread
      double O1[3] = {0.0, 0.0, 0.0}, O2[3] = {0.0, 0.0, 0.0}, M[9];
      for (int j = 0; j < N; ++j)
        if (flag[j]) {
#pragma unroll
          for (int c = 0; c < 3; ++c) { O1[c] += C[c * cap + j]; O2[c] += C[(3 + c) * cap + j]; }
        }
      const double dn = (double)n_inl;
#pragma unroll
      for (int c = 0; c < 3; ++c) { O1[c] = O1[c] / dn; O2[c] = O2[c] / dn; }
#pragma unroll
      for (int k = 0; k < 9; ++k) M[k] = 0.0;
      for (int j = 0; j < N; ++j)
        if (flag[j]) {
          double a1[3], a2[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) { a1[c] = C[c * cap + j] - O1[c]; a2[c] = C[(3 + c) * cap + j] - O2[c]; }
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) M[i * 3 + k] += a2[i] * a1[k];
        }
      double R[9];
      loop_quat_rot(M, R);
#pragma unroll
      for (int k = 0; k < 9; ++k) s_pose[k] = R[k];
#pragma unroll
      for (int i = 0; i < 3; ++i) s_pose[9 + i] = O1[i] - ((R[i * 3] * O2[0] + R[i * 3 + 1] * O2[1]) + R[i * 3 + 2] * O2[2]);
      s_ninl = 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 9; ++k) H.R[k] = s_pose[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) H.t[k] = s_pose[9 + k];
    loop_t21(H.R, H.t, t21);
    int mine = 0;
    for (int j = tid; j < N; j += LOOP_NT) {
      const bool in = loop_inlier(A, C, j, H.R, H.t, t21);
      flag[j] = in ? 1 : 0;
      mine += in ? 1 : 0;
    }
    if (mine) atomicAdd(&s_ninl, mine);
    __syncthreads();
    n_inl = s_ninl;
  }
  if (inl) {
    __syncthreads();      // (the zeros above are this workgroup's own stores)
    for (int j = tid; j < N; j += LOOP_NT)
      if (flag[j]) inl[ci1[j]] = 1;
  }
  if (tid == 0) {
    svo_loop_result r;
    r.status = s_status; r.n_matches = N; r.bound = bound; r.visited = s_visited; r.winner = winner; r.n_inliers = n_inl;
    r.sample[0] = idx[0]; r.sample[1] = idx[1]; r.sample[2] = idx[2]; r.reserved = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int k = 0; k < 3; ++k) r.T12[i * 4 + k] = H.R[i * 3 + k];
      r.T12[i * 4 + 3] = H.t[i];
    }
    r.T12[12] = 0.0; r.T12[13] = 0.0; r.T12[14] = 0.0; r.T12[15] = 1.0;
    *res = r;
  }
}

thread_local std::string g_loop_err;

}  // namespace

struct svo_loop {
  int device = 0, max_kp = 0, max_pairs = 0;
  bool ready = false;
  std::string last_error;
  hipStream_t stream = nullptr;
  hipEvent_t producer_done = nullptr;
  double* d_scratch = nullptr;
  int32_t* d_bounds = nullptr;
  uint8_t* d_stage = nullptr;        // svo_loop_verify: one pair's inputs and outputs
  bool have_bounds = false;
  double b_prob = 0.0; int b_min = 0, b_max = 0;     // what d_bounds was made from
};

#define LOOP_HIP(l, expr)                                                         \
  do {                                                                            \
    hipError_t _e = (expr);                                                       \
    if (_e != hipSuccess) {                                                       \
      (l)->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);        \
      return SVO_E_HIP;                                                           \
    }                                                                             \
  } while (0)

static int loop_fail(svo_loop* loop, const char* who, const std::string& why) {
  const std::string m = std::string(who) + ": " + why;
  if (loop) loop->last_error = m; else g_loop_err = m;
  return SVO_E_INVALID;
}

static size_t loop_round(size_t v) { return (v + 255) & ~(size_t)255; }
struct LoopStage { size_t desc, kp, n, fv, fv_n, obs, obs_n, Tcw, pairs, match, match_n, result, inliers, total; };
static LoopStage loop_stage(const svo_loop* loop) {
  LoopStage s;
  const size_t K = (size_t)loop->max_kp;
  size_t o = 0;
  s.desc = o; o += loop_round(2 * K * 32);
  s.kp = o; o += loop_round(2 * K * sizeof(svo_kp));
  s.n = o; o += loop_round(2 * sizeof(int32_t));
  s.fv = o; o += loop_round(2 * K * sizeof(svo_bow_feature));
  s.fv_n = o; o += loop_round(2 * sizeof(int32_t));
  s.obs = o; o += loop_round(2 * K * sizeof(svo_map_obs));
  s.obs_n = o; o += loop_round(2 * sizeof(int32_t));
  s.Tcw = o; o += loop_round(2 * 64);
  s.pairs = o; o += loop_round(2 * sizeof(int32_t));
  s.match = o; o += loop_round(K * sizeof(int32_t));
  s.match_n = o; o += loop_round(sizeof(int32_t));
  s.result = o; o += loop_round(sizeof(svo_loop_result));
  s.inliers = o; o += loop_round(K);
  s.total = o;
  return s;
}

static int loop_ready(svo_loop* loop) {
  if (loop->ready) { hipSetDevice(loop->device); return SVO_OK; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || loop->device >= ndev) {
    (void)hipGetLastError();
    loop->last_error = "svo_loop: no HIP device " + std::to_string(loop->device);
    return SVO_E_NODEVICE;
  }
  hipSetDevice(loop->device);
  // (a call that failed half way left what it had made: every handle is made once, svo_loop_destroy frees them all)
  if (!loop->stream) LOOP_HIP(loop, hipStreamCreateWithFlags(&loop->stream, hipStreamNonBlocking));
  if (!loop->producer_done) LOOP_HIP(loop, hipEventCreateWithFlags(&loop->producer_done, hipEventDisableTiming));
  const size_t scr = (size_t)loop->max_pairs * LOOP_NF * loop->max_kp * sizeof(double);
  if ((!loop->d_scratch && hipMalloc(reinterpret_cast<void**>(&loop->d_scratch), scr) != hipSuccess) ||
      (!loop->d_bounds && hipMalloc(reinterpret_cast<void**>(&loop->d_bounds), (size_t)(loop->max_kp + 1) * sizeof(int32_t)) != hipSuccess) ||
      (!loop->d_stage && hipMalloc(reinterpret_cast<void**>(&loop->d_stage), loop_stage(loop).total) != hipSuccess)) {
    (void)hipGetLastError();
    loop->last_error = "svo_loop: out of device memory";
    return SVO_E_NOMEM;
  }
  loop->ready = true;
  return SVO_OK;
}

static bool loop_finite(double v) { return v == v && v - v == 0.0; }

static int loop_check_params(svo_loop* loop, const char* who, const svo_loop_params* P, bool match, bool solve) {
  if (match) {
    if (P->th_low < 1 || P->th_low > 256) return loop_fail(loop, who, "th_low must be 1 .. 256");
    if (!(P->nn_ratio > 0.0f && P->nn_ratio <= 1.0f)) return loop_fail(loop, who, "nn_ratio must be in (0, 1]");
  }
  if (solve) {
    if (!(P->prob > 0.0 && P->prob < 1.0)) return loop_fail(loop, who, "prob must be in (0, 1)");
    if (P->min_inliers < 3) return loop_fail(loop, who, "min_inliers must be >= 3");
    if (P->max_iterations < 1 || P->max_iterations > LOOP_MAX_ITS) return loop_fail(loop, who, "max_iterations must be 1 .. 1024");
    if (!loop_finite(P->chi2) || P->chi2 <= 0.0) return loop_fail(loop, who, "chi2 must be finite and > 0");
    if (!loop_finite(P->scale_factor) || P->scale_factor <= 0.0f) return loop_fail(loop, who, "scale_factor must be finite and > 0");
  }
  return SVO_OK;
}

static int loop_check_cam(svo_loop* loop, const char* who, const svo_camera* cam) {
  if (!loop_finite(cam->fx) || !loop_finite(cam->fy) || !loop_finite(cam->cx) || !loop_finite(cam->cy))
    return loop_fail(loop, who, "a camera value is not finite");
  if (cam->fx <= 0.0f || cam->fy <= 0.0f) return loop_fail(loop, who, "fx and fy must be > 0");
  return SVO_OK;
}

extern "C" int svo_loop_default_params(svo_loop_params* p) {
  if (!p) return SVO_E_INVALID;
  memset(p, 0, sizeof *p);
  p->th_low = 50; p->nn_ratio = 0.75f; p->check_orientation = 1;
  p->prob = 0.99; p->min_inliers = 20; p->max_iterations = 300;
  p->seed = 0x5eed5eed5eed5eedull;
  p->chi2 = 9.210; p->scale_factor = 1.2f; p->refine = 0;
  return SVO_OK;
}

// Sim3Solver::SetRansacParameters for every N, with the host's log and pow
extern "C" int svo_loop_bounds(const svo_loop_params* params, int n_max, int32_t* bounds) {
  const char* who = "svo_loop_bounds";
  if (!params || !bounds) return loop_fail(nullptr, who, "params or bounds is NULL");
  if (n_max < 0) return loop_fail(nullptr, who, "n_max is negative");
  if (int rc = loop_check_params(nullptr, who, params, false, true)) return rc;
  for (int N = 0; N <= n_max; ++N) {
    int b = 0;
    if (N == params->min_inliers) b = 1;
    else if (N > params->min_inliers) {
      const double eps = (double)params->min_inliers / (double)N;
      const double v = ceil(log(1.0 - params->prob) / log(1.0 - pow(eps, 3.0)));
      if (!(v < (double)params->max_iterations) || v < 0.0) b = params->max_iterations;     // (also a NaN or an infinity)
      else b = v < 1.0 ? 1 : (int)v;
    }
    bounds[N] = b;
  }
  return SVO_OK;
}

extern "C" const char* svo_loop_last_error(const svo_loop* loop) { return loop ? loop->last_error.c_str() : g_loop_err.c_str(); }

extern "C" int svo_loop_create(int device, int max_kp, int max_pairs, svo_loop** out) {
  const char* who = "svo_loop_create";
  if (!out) return loop_fail(nullptr, who, "out is NULL");
  *out = nullptr;
  if (device < 0) return loop_fail(nullptr, who, "device is negative");
  if (max_kp < 1 || max_kp > LOOP_MAX_KP) return loop_fail(nullptr, who, "max_kp must be 1 .. 2048");
  if (max_pairs < 1 || max_pairs > 65535) return loop_fail(nullptr, who, "max_pairs must be 1 .. 65535");
  svo_loop* loop = new svo_loop();
  loop->device = device; loop->max_kp = max_kp; loop->max_pairs = max_pairs;
  g_loop_err.clear();
  *out = loop;
  return SVO_OK;
}

extern "C" void svo_loop_destroy(svo_loop* loop) {
  if (!loop) return;
  if (loop->stream) {
    hipSetDevice(loop->device);
    hipStreamSynchronize(loop->stream);
    if (loop->d_scratch) hipFree(loop->d_scratch);
    if (loop->d_bounds) hipFree(loop->d_bounds);
    if (loop->d_stage) hipFree(loop->d_stage);
    if (loop->producer_done) hipEventDestroy(loop->producer_done);
    hipStreamDestroy(loop->stream);
  }
  delete loop;
}

extern "C" int svo_loop_sync(svo_loop* loop) {
  if (!loop) return SVO_E_INVALID;
  if (!loop->ready) return SVO_OK;
  hipSetDevice(loop->device);
  LOOP_HIP(loop, hipStreamSynchronize(loop->stream));
  return SVO_OK;
}

extern "C" void* svo_loop_stream(svo_loop* loop) {
  if (!loop || loop_ready(loop) != SVO_OK) return nullptr;
  return loop->stream;
}

extern "C" int svo_loop_wait(svo_loop* loop, void* stream) {
  const char* who = "svo_loop_wait";
  if (!loop) return loop_fail(nullptr, who, "loop is NULL");
  if (!stream) return loop_fail(loop, who, "stream is NULL");
  if (int rc = loop_ready(loop)) return rc;
  LOOP_HIP(loop, hipEventRecord(loop->producer_done, static_cast<hipStream_t>(stream)));
  LOOP_HIP(loop, hipStreamWaitEvent(loop->stream, loop->producer_done, 0));
  return SVO_OK;
}

extern "C" int svo_loop_pairs_dev(svo_loop* loop, const svo_bow_cand* d_cand, const int32_t* d_cand_n, int q0, int Q, int top_k,
                                  int32_t* d_pairs) {
  const char* who = "svo_loop_pairs_dev";
  if (!loop) return loop_fail(nullptr, who, "loop is NULL");
  if (!d_cand) return loop_fail(loop, who, "d_cand is NULL");
  if (!d_cand_n) return loop_fail(loop, who, "d_cand_n is NULL");
  if (!d_pairs) return loop_fail(loop, who, "d_pairs is NULL");
  if (reinterpret_cast<uintptr_t>(d_cand) & 7u) return loop_fail(loop, who, "d_cand is not 8-byte aligned");
  if (q0 < 0) return loop_fail(loop, who, "q0 is negative");
  if (top_k < 1 || top_k > 16) return loop_fail(loop, who, "top_k must be 1 .. 16");
  if (Q < 1 || (long long)Q * top_k > loop->max_pairs) return loop_fail(loop, who, "Q * top_k must be 1 .. max_pairs");
  if (int rc = loop_ready(loop)) return rc;
  hipLaunchKernelGGL(k_loop_pairs, dim3((Q * top_k + LOOP_NT - 1) / LOOP_NT), dim3(LOOP_NT), 0, loop->stream, d_cand, d_cand_n, q0, Q,
                     top_k, d_pairs);
  LOOP_HIP(loop, hipGetLastError());
  return SVO_OK;
}

static int loop_check_match(svo_loop* loop, const char* who, const svo_loop_params* params, const uint8_t* d_desc, const svo_kp* d_kp,
                            const int32_t* d_n, int kp_stride, const svo_bow_feature* d_fv, const int32_t* d_fv_n,
                            const svo_map_obs* d_obs, const int32_t* d_obs_n, int obs_stride, const int32_t* d_pairs, int n_pairs,
                            const int32_t* d_match, const int32_t* d_match_n) {
  if (!params) return loop_fail(loop, who, "params is NULL");
  if (!d_desc) return loop_fail(loop, who, "d_desc is NULL");
  if (!d_kp) return loop_fail(loop, who, "d_kp is NULL");
  if (!d_n) return loop_fail(loop, who, "d_n is NULL");
  if (!d_fv) return loop_fail(loop, who, "d_fv is NULL");
  if (!d_fv_n) return loop_fail(loop, who, "d_fv_n is NULL");
  if (!d_obs) return loop_fail(loop, who, "d_obs is NULL");
  if (!d_obs_n) return loop_fail(loop, who, "d_obs_n is NULL");
  if (!d_pairs) return loop_fail(loop, who, "d_pairs is NULL");
  if (!d_match) return loop_fail(loop, who, "d_match is NULL");
  if (!d_match_n) return loop_fail(loop, who, "d_match_n is NULL");
  if (reinterpret_cast<uintptr_t>(d_desc) & 3u) return loop_fail(loop, who, "d_desc is not 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_fv) & 7u) return loop_fail(loop, who, "d_fv is not 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_obs) & 15u) return loop_fail(loop, who, "d_obs is not 16-byte aligned");
  if (kp_stride < 1 || kp_stride > loop->max_kp) return loop_fail(loop, who, "kp_stride must be 1 .. max_kp");
  if (obs_stride < 1 || obs_stride > loop->max_kp) return loop_fail(loop, who, "obs_stride must be 1 .. max_kp");
  if (n_pairs < 1 || n_pairs > loop->max_pairs) return loop_fail(loop, who, "n_pairs must be 1 .. max_pairs");
  return loop_check_params(loop, who, params, true, false);
}

static int loop_check_solve(svo_loop* loop, const char* who, const svo_camera* cam, const svo_loop_params* params, const svo_kp* d_kp,
                            const svo_map_obs* d_obs, const int32_t* d_obs_n, int obs_stride, const void* d_Tcw, int pose_stride_bytes,
                            const int32_t* d_pairs, int n_pairs, const int32_t* d_match, int kp_stride, const svo_loop_result* d_result) {
  if (!cam) return loop_fail(loop, who, "cam is NULL");
  if (!params) return loop_fail(loop, who, "params is NULL");
  if (!d_kp) return loop_fail(loop, who, "d_kp is NULL");
  if (!d_obs) return loop_fail(loop, who, "d_obs is NULL");
  if (!d_obs_n) return loop_fail(loop, who, "d_obs_n is NULL");
  if (!d_Tcw) return loop_fail(loop, who, "d_Tcw is NULL");
  if (!d_pairs) return loop_fail(loop, who, "d_pairs is NULL");
  if (!d_match) return loop_fail(loop, who, "d_match is NULL");
  if (!d_result) return loop_fail(loop, who, "d_result is NULL");
  if (reinterpret_cast<uintptr_t>(d_obs) & 15u) return loop_fail(loop, who, "d_obs is not 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_Tcw) & 3u) return loop_fail(loop, who, "d_Tcw is not 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_result) & 7u) return loop_fail(loop, who, "d_result is not 8-byte aligned");
  if (kp_stride < 1 || kp_stride > loop->max_kp) return loop_fail(loop, who, "kp_stride must be 1 .. max_kp");
  if (obs_stride < 1 || obs_stride > loop->max_kp) return loop_fail(loop, who, "obs_stride must be 1 .. max_kp");
  if (n_pairs < 1 || n_pairs > loop->max_pairs) return loop_fail(loop, who, "n_pairs must be 1 .. max_pairs");
  if (pose_stride_bytes < 64 || (pose_stride_bytes & 3)) return loop_fail(loop, who, "pose_stride_bytes must be >= 64 and a multiple of 4");
  if (int rc = loop_check_cam(loop, who, cam)) return rc;
  return loop_check_params(loop, who, params, false, true);
}

static int loop_launch_match(svo_loop* loop, const svo_loop_params* params, const uint8_t* d_desc, const svo_kp* d_kp, const int32_t* d_n,
                             int kp_stride, const svo_bow_feature* d_fv, const int32_t* d_fv_n, const svo_map_obs* d_obs,
                             const int32_t* d_obs_n, int obs_stride, const int32_t* d_pairs, int n_pairs, int32_t* d_match,
                             int32_t* d_match_n) {
  MatchArgs M;
  M.desc = d_desc; M.kp = d_kp; M.n = d_n; M.kp_stride = kp_stride; M.fv = d_fv; M.fv_n = d_fv_n;
  M.obs = d_obs; M.obs_n = d_obs_n; M.obs_stride = obs_stride; M.pairs = d_pairs;
  M.th_low = params->th_low; M.nn_ratio = params->nn_ratio; M.check_orientation = params->check_orientation;
  M.match = d_match; M.match_n = d_match_n;
  hipLaunchKernelGGL(k_loop_match, dim3(n_pairs), dim3(LOOP_NT), 0, loop->stream, M);
  LOOP_HIP(loop, hipGetLastError());
  return SVO_OK;
}

static int loop_launch_solve(svo_loop* loop, const svo_camera* cam, const svo_loop_params* params, const svo_kp* d_kp,
                             const svo_map_obs* d_obs, const int32_t* d_obs_n, int obs_stride, const void* d_Tcw, int pose_stride_bytes,
                             const int32_t* d_pairs, int n_pairs, const int32_t* d_match, int kp_stride, svo_loop_result* d_result,
                             uint8_t* d_inliers) {
  if (!loop->have_bounds || loop->b_prob != params->prob || loop->b_min != params->min_inliers || loop->b_max != params->max_iterations) {
    // other parameters than the table was made for: the calls in flight keep theirs (this synchronises the object's stream once)
    std::vector<int32_t> tab((size_t)loop->max_kp + 1);
    if (int rc = svo_loop_bounds(params, loop->max_kp, tab.data())) return rc;
    LOOP_HIP(loop, hipStreamSynchronize(loop->stream));
    LOOP_HIP(loop, hipMemcpy(loop->d_bounds, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    loop->have_bounds = true; loop->b_prob = params->prob; loop->b_min = params->min_inliers; loop->b_max = params->max_iterations;
  }
  SolveArgs V;
  V.kp = d_kp; V.obs = d_obs; V.obs_n = d_obs_n; V.obs_stride = obs_stride;
  V.Tcw = static_cast<const uint8_t*>(d_Tcw); V.pose_stride = pose_stride_bytes;
  V.pairs = d_pairs; V.match = d_match; V.kp_stride = kp_stride;
  V.fx = (double)cam->fx; V.fy = (double)cam->fy; V.cx = (double)cam->cx; V.cy = (double)cam->cy; V.chi2 = params->chi2;
  float sc = 1.0f;      // ORBextractor's scale table: a float32 running product, squared in float32
  for (int l = 0; l < 8; ++l) {
    if (l > 0) sc = sc * params->scale_factor;
    const float s2 = sc * sc;
    V.sigma2[l] = (double)s2;
  }
  V.min_inliers = params->min_inliers; V.refine = params->refine; V.seed = params->seed;
  V.bounds = loop->d_bounds; V.scratch = loop->d_scratch; V.cap = loop->max_kp;
  V.result = d_result; V.inliers = d_inliers;
  hipLaunchKernelGGL(k_loop_solve, dim3(n_pairs), dim3(LOOP_NT), 0, loop->stream, V);
  LOOP_HIP(loop, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_loop_match_dev(svo_loop* loop, const svo_loop_params* params, const uint8_t* d_desc, const svo_kp* d_kp,
                                  const int32_t* d_n, int kp_stride, const svo_bow_feature* d_fv, const int32_t* d_fv_n,
                                  const svo_map_obs* d_obs, const int32_t* d_obs_n, int obs_stride, const int32_t* d_pairs, int n_pairs,
                                  int32_t* d_match, int32_t* d_match_n) {
  const char* who = "svo_loop_match_dev";
  if (!loop) return loop_fail(nullptr, who, "loop is NULL");
  if (int rc = loop_check_match(loop, who, params, d_desc, d_kp, d_n, kp_stride, d_fv, d_fv_n, d_obs, d_obs_n, obs_stride, d_pairs,
                                n_pairs, d_match, d_match_n))
    return rc;
  if (int rc = loop_ready(loop)) return rc;
  return loop_launch_match(loop, params, d_desc, d_kp, d_n, kp_stride, d_fv, d_fv_n, d_obs, d_obs_n, obs_stride, d_pairs, n_pairs,
                           d_match, d_match_n);
}

extern "C" int svo_loop_solve_dev(svo_loop* loop, const svo_camera* cam, const svo_loop_params* params, const svo_kp* d_kp,
                                  const svo_map_obs* d_obs, const int32_t* d_obs_n, int obs_stride, const void* d_Tcw,
                                  int pose_stride_bytes, const int32_t* d_pairs, int n_pairs, const int32_t* d_match, int kp_stride,
                                  svo_loop_result* d_result, uint8_t* d_inliers) {
  const char* who = "svo_loop_solve_dev";
  if (!loop) return loop_fail(nullptr, who, "loop is NULL");
  if (int rc = loop_check_solve(loop, who, cam, params, d_kp, d_obs, d_obs_n, obs_stride, d_Tcw, pose_stride_bytes, d_pairs, n_pairs,
                                d_match, kp_stride, d_result))
    return rc;
  if (int rc = loop_ready(loop)) return rc;
  return loop_launch_solve(loop, cam, params, d_kp, d_obs, d_obs_n, obs_stride, d_Tcw, pose_stride_bytes, d_pairs, n_pairs, d_match,
                           kp_stride, d_result, d_inliers);
}

extern "C" int svo_loop_verify_dev(svo_loop* loop, const svo_camera* cam, const svo_loop_params* params, const uint8_t* d_desc,
                                   const svo_kp* d_kp, const int32_t* d_n, int kp_stride, const svo_bow_feature* d_fv,
                                   const int32_t* d_fv_n, const svo_map_obs* d_obs, const int32_t* d_obs_n, int obs_stride,
                                   const void* d_Tcw, int pose_stride_bytes, const int32_t* d_pairs, int n_pairs, int32_t* d_match,
                                   int32_t* d_match_n, svo_loop_result* d_result, uint8_t* d_inliers) {
  const char* who = "svo_loop_verify_dev";
  if (!loop) return loop_fail(nullptr, who, "loop is NULL");
  if (int rc = loop_check_match(loop, who, params, d_desc, d_kp, d_n, kp_stride, d_fv, d_fv_n, d_obs, d_obs_n, obs_stride, d_pairs,
                                n_pairs, d_match, d_match_n))
    return rc;
  if (int rc = loop_check_solve(loop, who, cam, params, d_kp, d_obs, d_obs_n, obs_stride, d_Tcw, pose_stride_bytes, d_pairs, n_pairs,
                                d_match, kp_stride, d_result))
    return rc;
  if (int rc = loop_ready(loop)) return rc;
  if (int rc = loop_launch_match(loop, params, d_desc, d_kp, d_n, kp_stride, d_fv, d_fv_n, d_obs, d_obs_n, obs_stride, d_pairs, n_pairs,
                                 d_match, d_match_n))
    return rc;
  return loop_launch_solve(loop, cam, params, d_kp, d_obs, d_obs_n, obs_stride, d_Tcw, pose_stride_bytes, d_pairs, n_pairs, d_match,
                           kp_stride, d_result, d_inliers);
}

extern "C" int svo_loop_verify(svo_loop* loop, const svo_camera* cam, const svo_loop_params* params, const uint8_t* desc,
                               const svo_kp* kp, const int32_t* n, int kp_stride, const svo_bow_feature* fv, const int32_t* fv_n,
                               const svo_map_obs* obs, const int32_t* obs_n, int obs_stride, const float* Tcw, int32_t* match,
                               svo_loop_result* result, uint8_t* inliers) {
  const char* who = "svo_loop_verify";
  if (!loop) return loop_fail(nullptr, who, "loop is NULL");
  if (!cam || !params) return loop_fail(loop, who, "cam or params is NULL");
  if (!desc || !kp || !n || !fv || !fv_n || !obs || !obs_n || !Tcw)
    return loop_fail(loop, who, "desc, kp, n, fv, fv_n, obs, obs_n or Tcw is NULL");
  if (!result) return loop_fail(loop, who, "result is NULL");
  if (kp_stride < 1 || kp_stride > loop->max_kp) return loop_fail(loop, who, "kp_stride must be 1 .. max_kp");
  if (obs_stride < 1 || obs_stride > loop->max_kp) return loop_fail(loop, who, "obs_stride must be 1 .. max_kp");
  if (int rc = loop_check_cam(loop, who, cam)) return rc;
  if (int rc = loop_check_params(loop, who, params, true, true)) return rc;
  if (int rc = loop_ready(loop)) return rc;
  const LoopStage s = loop_stage(loop);
  uint8_t* d = loop->d_stage;
  const int32_t pair[2] = {0, 1};
  LOOP_HIP(loop, hipStreamSynchronize(loop->stream));
  LOOP_HIP(loop, hipMemcpy(d + s.desc, desc, (size_t)2 * kp_stride * 32, hipMemcpyHostToDevice));
  LOOP_HIP(loop, hipMemcpy(d + s.kp, kp, (size_t)2 * kp_stride * sizeof(svo_kp), hipMemcpyHostToDevice));
  LOOP_HIP(loop, hipMemcpy(d + s.n, n, 2 * sizeof(int32_t), hipMemcpyHostToDevice));
  LOOP_HIP(loop, hipMemcpy(d + s.fv, fv, (size_t)2 * kp_stride * sizeof(svo_bow_feature), hipMemcpyHostToDevice));
  LOOP_HIP(loop, hipMemcpy(d + s.fv_n, fv_n, 2 * sizeof(int32_t), hipMemcpyHostToDevice));
  LOOP_HIP(loop, hipMemcpy(d + s.obs, obs, (size_t)2 * obs_stride * sizeof(svo_map_obs), hipMemcpyHostToDevice));
  LOOP_HIP(loop, hipMemcpy(d + s.obs_n, obs_n, 2 * sizeof(int32_t), hipMemcpyHostToDevice));
  LOOP_HIP(loop, hipMemcpy(d + s.Tcw, Tcw, 2 * 64, hipMemcpyHostToDevice));
  LOOP_HIP(loop, hipMemcpy(d + s.pairs, pair, sizeof pair, hipMemcpyHostToDevice));
  if (int rc = svo_loop_verify_dev(loop, cam, params, d + s.desc, reinterpret_cast<const svo_kp*>(d + s.kp),
                                   reinterpret_cast<const int32_t*>(d + s.n), kp_stride, reinterpret_cast<const svo_bow_feature*>(d + s.fv),
                                   reinterpret_cast<const int32_t*>(d + s.fv_n), reinterpret_cast<const svo_map_obs*>(d + s.obs),
                                   reinterpret_cast<const int32_t*>(d + s.obs_n), obs_stride, d + s.Tcw, 64,
                                   reinterpret_cast<const int32_t*>(d + s.pairs), 1, reinterpret_cast<int32_t*>(d + s.match),
                                   reinterpret_cast<int32_t*>(d + s.match_n), reinterpret_cast<svo_loop_result*>(d + s.result),
                                   d + s.inliers))
    return rc;
  LOOP_HIP(loop, hipStreamSynchronize(loop->stream));
  if (match) LOOP_HIP(loop, hipMemcpy(match, d + s.match, (size_t)kp_stride * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (inliers) LOOP_HIP(loop, hipMemcpy(inliers, d + s.inliers, (size_t)kp_stride, hipMemcpyDeviceToHost));
  LOOP_HIP(loop, hipMemcpy(result, d + s.result, sizeof(svo_loop_result), hipMemcpyDeviceToHost));
  return SVO_OK;
}
