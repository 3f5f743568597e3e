// svo_ba.hip - windowed bundle adjustment on the device over the map records (svo_ba_* in include/svo.h): the last `window` poses
// and the points they share, refined together as g2o's BlockSolver + Levenberg-Marquardt would (ORB-SLAM2's local bundle
// adjustment without its outlier rounds).  The contract, operation by operation: DESIGN.md section 8 "Windowed bundle adjustment";
// the numpy twin: tests/ba_ref.py.
//
// An object of its own on a stream of its own, like the rectifier (svo_rect.hip): nothing here runs on a tracker context's streams;
// with a producer context the object's stream waits for an event recorded on the producer's stream, nothing else.
//
// Two launches per call, one workgroup of 256 threads per window:
//   k_ba_assoc  sorts the (gid, frame, kp) keys of the window's records (bitonic, in the window's scratch), cuts the sorted keys
//               into points, applies the two drop rules and writes the edge list and the points' start.
//   k_ba_lm     the whole LM of the window.  A lane per point builds residuals, Jacobians and the point's 3 x 3 block with the
//               point's <= 8 edges in registers; per-edge blocks (pose Jacobian, W, W Dinv) live in the scratch.  Every sum over
//               points is taken by ONE thread in point order (a thread per entry of Hpp, b and Hschur), every sum over a point's
//               edges by the point's lane in frame order, chi2 and the LM's scale by one wave in point order: no floating-point
//               atomics, the same bits on every run.  The <= 42 x 42 system is factored in LDS (LDL^T, a thread per row).
#include <float.h>
#include <math.h>
#include <string.h>

#include <string>

#include "svo_pose_dev.h"

namespace {

constexpr int BA_NT = 256;
constexpr int BA_MAXW = 8;              // frames of a window
constexpr int BA_MAXN = 6 * (BA_MAXW - 1);   // unknowns of the pose system
constexpr int BA_MAX_KP = 4096;         // records per frame the key's 13 index bits hold (with room for the "no record" key)
constexpr uint64_t BA_NOKEY = ~0ull;

struct BaArgs {
  const svo_map_obs* obs; const int32_t* counts; int obs_stride;
  const uint8_t* Tcw; int pose_stride; int first, step;
  int window, nfix, iterations, stereo;
  double huber_mono, huber_stereo, lambda_init;
  double fx, fy, cx, cy, bf; float bf32;
  int nk;                               // keys sorted per window: the power of two >= window * obs_stride
  uint8_t* scratch; size_t per_window; int pcap, ecap, nkcap;
  double* Tout; svo_ba_point* points; int points_stride; svo_ba_stats* stats;
};

// a window's scratch: [point arrays | edge arrays | keys | int arrays]
struct BaScr {
  double *X, *Xb, *Hll, *bl, *Di, *chi, *sc;       // per point: 3, 3, 6, 3, 6, 1, 1
  double *eobs, *ew, *Jp, *Wm, *Y;                 // per edge: 3, 4, 18, 18, 18
  uint64_t* keys;                                  // nkcap
  int32_t *flag, *kmask, *pidx, *eidx;             // per key
  int32_t *pgid, *pmask, *eoff;                    // per point (pmask: bits 0..7 edge in frame f, bits 8..15 that edge is stereo)
  int32_t* hdr;                                    // 0 points, 1 edges, 2 stereo edges, 3 frames with edges
};
constexpr int BA_PD = 23, BA_ED = 61;
__host__ __device__ inline size_t ba_per_window(int pcap, int ecap, int nkcap) {
  return ((size_t)BA_PD * pcap + (size_t)BA_ED * ecap + (size_t)nkcap) * 8 + ((size_t)4 * nkcap + (size_t)3 * pcap + 8) * 4 + 8;
}
__device__ inline BaScr ba_scr(const BaArgs& A, int w) {
  BaScr S;
  double* d = reinterpret_cast<double*>(A.scratch + (size_t)w * A.per_window);
  const size_t P = A.pcap, E = A.ecap, K = A.nkcap;
  S.X = d; d += 3 * P; S.Xb = d; d += 3 * P; S.Hll = d; d += 6 * P; S.bl = d; d += 3 * P; S.Di = d; d += 6 * P; S.chi = d; d += P; S.sc = d; d += P;
  S.eobs = d; d += 3 * E; S.ew = d; d += 4 * E; S.Jp = d; d += 18 * E; S.Wm = d; d += 18 * E; S.Y = d; d += 18 * E;
  S.keys = reinterpret_cast<uint64_t*>(d); d += K;
  int32_t* i = reinterpret_cast<int32_t*>(d);
  S.flag = i; i += K; S.kmask = i; i += K; S.pidx = i; i += K; S.eidx = i; i += K;
  S.pgid = i; i += P; S.pmask = i; i += P; S.eoff = i; i += P;
  S.hdr = i;
  return S;
}

// the float32 start pose of frame f of window w, widened (convert::toSE3Quat restated: svo_pose_dev.h)
__device__ inline void ba_load_pose(const BaArgs& A, int w, int f, double T[16], Se3& est) {
  const float* p = reinterpret_cast<const float*>(A.Tcw + (size_t)(A.first + w * A.step + f) * A.pose_stride);
  for (int j = 0; j < 16; ++j) T[j] = (double)p[j];
  se3_from_T(T, est);
}

__device__ __forceinline__ uint32_t key_gid(uint64_t k) { return (uint32_t)(k >> 32); }
__device__ __forceinline__ int key_frame(uint64_t k) { return (int)((k >> 29) & 7u); }
__device__ __forceinline__ int key_rec(uint64_t k) { return (int)(k & 0x1fffu); }

// One head of the sorted keys: the point's records (per frame the first one: the lowest kp), its start position and the edges
// that survive the z rule.  rec[f]: record index in frame f, mask: bit f.
__device__ inline int ba_segment(const BaArgs& A, const uint64_t* keys, int i, int nvalid, const svo_map_obs* wobs, const Se3* est,
                                 int rec[BA_MAXW], double X[3]) {
  const uint32_t g = key_gid(keys[i]);
  int seen = 0;
  for (int j = i; j < nvalid && key_gid(keys[j]) == g; ++j) {
    const int f = key_frame(keys[j]);
    if (!((seen >> f) & 1)) { seen |= 1 << f; rec[f] = key_rec(keys[j]); }
  }
  const int f0 = __ffs(seen) - 1;
  const svo_map_obs& r0 = wobs[(size_t)f0 * A.obs_stride + rec[f0]];
  X[0] = (double)r0.X; X[1] = (double)r0.Y; X[2] = (double)r0.Z;
  int mask = 0;
  for (int f = 0; f < A.window; ++f) {
    if (!((seen >> f) & 1)) continue;
    double pc[3];
    quat_rot(est[f].q, X, pc);
    if (pc[2] + est[f].t[2] > 0.0) mask |= 1 << f;   // z <= 0 (or not a number) at the start estimate: no edge
  }
  return mask;
}

__global__ void __launch_bounds__(BA_NT) k_ba_assoc(BaArgs A) {
  __shared__ Se3 est[BA_MAXW];
  __shared__ int s_cnt[BA_MAXW], s_np[BA_NT], s_ne[BA_NT], s_tot[4];
  const int w = blockIdx.x, tid = threadIdx.x, W = A.window, stride = A.obs_stride, nk = A.nk;
  const BaScr S = ba_scr(A, w);
  const svo_map_obs* wobs = A.obs + (size_t)(A.first + w * A.step) * stride;
  if (tid < W) {
    double T[16];
    ba_load_pose(A, w, tid, T, est[tid]);
    const int c = A.counts[A.first + w * A.step + tid];
    s_cnt[tid] = min(max(c, 0), stride);
  }
  if (tid < 4) s_tot[tid] = 0;
  __syncthreads();
  // keys: gid (order of int32) | frame | kp (order of int16) | record index
  for (int i = tid; i < nk; i += BA_NT) {
    uint64_t key = BA_NOKEY;
    if (i < W * stride) {
      const int f = i / stride, k = i - f * stride;
      if (k < s_cnt[f]) {
        const svo_map_obs& r = wobs[(size_t)f * stride + k];
        key = ((uint64_t)((uint32_t)r.gid ^ 0x80000000u) << 32) | ((uint64_t)f << 29) | ((uint64_t)((uint32_t)((int)r.kp + 32768) & 0xffffu) << 13) |
              (uint64_t)k;
      }
    }
    S.keys[i] = key;
  }
  __syncthreads();
  for (int k = 2; k <= nk; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < nk; i += BA_NT) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint64_t a = S.keys[i], b = S.keys[ixj];
          if ((a > b) == ((i & k) == 0)) { S.keys[i] = b; S.keys[ixj] = a; }
        }
      }
      __syncthreads();
    }
  int nvalid = 0;
  for (int f = 0; f < W; ++f) nvalid += s_cnt[f];
  // heads: the point's edge count (0: not a head, or dropped) and mask
  for (int i = tid; i < nvalid; i += BA_NT) {
    int cnt = 0, mask = 0;
    if (i == 0 || key_gid(S.keys[i]) != key_gid(S.keys[i - 1])) {
      int rec[BA_MAXW];
      double X[3];
      mask = ba_segment(A, S.keys, i, nvalid, wobs, est, rec, X);
      cnt = __popc(mask);
      if (cnt < 2) { cnt = 0; mask = 0; }
    }
    S.flag[i] = cnt; S.kmask[i] = mask;
  }
  __syncthreads();
  // numbering by ascending gid: exclusive scans of "kept head" and of the edge counts, a contiguous chunk of keys per thread
  const int chunk = (nvalid + BA_NT - 1) / BA_NT, c0 = min(tid * chunk, nvalid), c1 = min(c0 + chunk, nvalid);
  int np = 0, ne = 0;
  for (int i = c0; i < c1; ++i) { np += S.flag[i] > 0; ne += S.flag[i]; }
  s_np[tid] = np; s_ne[tid] = ne;
  __syncthreads();
  if (tid == 0) {
    int a = 0, b = 0;
    for (int t = 0; t < BA_NT; ++t) { const int x = s_np[t], y = s_ne[t]; s_np[t] = a; s_ne[t] = b; a += x; b += y; }
    s_tot[0] = a; s_tot[1] = b;
  }
  __syncthreads();
  np = s_np[tid]; ne = s_ne[tid];
  for (int i = c0; i < c1; ++i) { S.pidx[i] = np; S.eidx[i] = ne; np += S.flag[i] > 0; ne += S.flag[i]; }
  __syncthreads();
  int n_stereo = 0, frames = 0;
  for (int i = tid; i < nvalid; i += BA_NT) {
    if (S.flag[i] == 0) continue;
    int rec[BA_MAXW];
    double X[3];
    const int mask = ba_segment(A, S.keys, i, nvalid, wobs, est, rec, X);
    const int p = S.pidx[i];
    int e = S.eidx[i], smask = 0;
    for (int f = 0; f < W; ++f) {
      if (!((mask >> f) & 1)) continue;
      const svo_map_obs& r = wobs[(size_t)f * stride + rec[f]];
      const bool st = A.stereo && r.depth > 0.0f;
      S.eobs[3 * (size_t)e] = (double)r.u; S.eobs[3 * (size_t)e + 1] = (double)r.v;
      S.eobs[3 * (size_t)e + 2] = st ? (double)r.u - A.bf / (double)r.depth : 0.0;
      if (st) smask |= 1 << f;
      ++e;
    }
    S.pgid[p] = (int32_t)(key_gid(S.keys[i]) ^ 0x80000000u); S.pmask[p] = mask | (smask << 8); S.eoff[p] = S.eidx[i];
    S.X[3 * (size_t)p] = X[0]; S.X[3 * (size_t)p + 1] = X[1]; S.X[3 * (size_t)p + 2] = X[2];
    if (A.points) {
      svo_ba_point* o = A.points + (size_t)w * A.points_stride + p;
      o->gid = S.pgid[p]; o->n_obs = S.flag[i];
    }
    n_stereo += __popc(smask); frames |= mask;
  }
  if (n_stereo) atomicAdd(&s_tot[2], n_stereo);
  if (frames) atomicOr(&s_tot[3], frames);
  __syncthreads();
  if (tid < 4) S.hdr[tid] = s_tot[tid];
}

struct BaLds {
  Se3 est[BA_MAXW], bak[BA_MAXW];
  double R[BA_MAXW][9], Tin[BA_MAXW][16];
  double Hs[BA_MAXN * BA_MAXN], D[BA_MAXN], bs[BA_MAXN], x[BA_MAXN], bp[BA_MAXN], Hpp[BA_MAXW - 1][36];
  double red[BA_NT], sc[4];
  int flag[2];
};

struct BaCam { double fx, fy, cx, cy, bf; float bf32; };

__device__ __forceinline__ double dot3(double a0, double b0, double a1, double b1, double a2, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// camera coordinates and the error of one edge (EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ::computeError; a mono edge's third
// component is 0)
__device__ __forceinline__ void ba_edge_error(const Se3& est, const double X[3], const double* ob, bool stereo, const BaCam& c, double pc[3],
                                              double e[3]) {
  quat_rot(est.q, X, pc);
  pc[0] += est.t[0]; pc[1] += est.t[1]; pc[2] += est.t[2];
  if (stereo) {
    const float invz32 = (float)(1.0 / pc[2]);          // const float invz = 1.0f / trans_xyz[2]
    const double invz = (double)invz32;
    const double p0 = pc[0] * invz * c.fx + c.cx, p1 = pc[1] * invz * c.fy + c.cy;
    const double p2 = p0 - (double)(c.bf32 * invz32);   // bf * invz: a float product
    e[0] = ob[0] - p0; e[1] = ob[1] - p1; e[2] = ob[2] - p2;
  } else {
    e[0] = ob[0] - (pc[0] / pc[2] * c.fx + c.cx);
    e[1] = ob[1] - (pc[1] / pc[2] * c.fy + c.cy);
    e[2] = ob[2] - 0.0;
  }
}
// RobustKernelHuber::robustify (delta <= 0: no kernel)
__device__ __forceinline__ void ba_huber(double chi, double delta, double& rho0, double& rho1) {
  if (delta > 0.0 && !(chi <= delta * delta)) {
    const double sq = sqrt(chi);
    rho0 = 2 * sq * delta - delta * delta; rho1 = delta / sq;
  } else { rho0 = chi; rho1 = 1.0; }
}
// linearizeOplus of both edge types: Jl 3 x 3 (d e / d point), Jp 3 x 6 (d e / d pose); row 2 of a mono edge is 0
__device__ __forceinline__ void ba_jacobians(const double* R, const double pc[3], bool stereo, const BaCam& c, double Jl[9], double Jp[18]) {
  const double x = pc[0], y = pc[1], z = pc[2], z_2 = z * z, fx = c.fx, fy = c.fy, bf = c.bf;
  if (stereo) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Jl[j] = -fx * R[j] / z + fx * x * R[6 + j] / z_2;
      Jl[3 + j] = -fy * R[3 + j] / z + fy * y * R[6 + j] / z_2;
      Jl[6 + j] = Jl[j] - bf * R[6 + j] / z_2;
    }
  } else {
    const double s = -1.0 / z, a0 = s * fx, a2 = s * (-x / z * fx), b1 = s * fy, b2 = s * (-y / z * fy);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Jl[j] = a0 * R[j] + a2 * R[6 + j];
      Jl[3 + j] = b1 * R[3 + j] + b2 * R[6 + j];
      Jl[6 + j] = 0.0;
    }
  }
  Jp[0] = x * y / z_2 * fx;
  Jp[1] = -(1 + (x * x / z_2)) * fx;
  Jp[2] = y / z * fx;
  Jp[3] = -1. / z * fx;
  Jp[4] = 0.0;
  Jp[5] = x / z_2 * fx;
  Jp[6] = (1 + y * y / z_2) * fy;
  Jp[7] = -x * y / z_2 * fy;
  Jp[8] = -x / z * fy;
  Jp[9] = 0.0;
  Jp[10] = -1. / z * fy;
  Jp[11] = y / z_2 * fy;
  if (stereo) {
    Jp[12] = Jp[0] - bf * y / z_2;
    Jp[13] = Jp[1] + bf * x / z_2;
    Jp[14] = Jp[2];
    Jp[15] = Jp[3];
    Jp[16] = 0.0;
    Jp[17] = Jp[5] - bf / z_2;
  } else {
#pragma unroll
    for (int j = 12; j < 18; ++j) Jp[j] = 0.0;
  }
}

// the sum p[0] + p[1] + ... in this order, by one whole wave (64 values per load, added lane by lane); the result in every lane
__device__ inline double ba_ordered_sum(const double* p, int n, int lane) {
  double acc = 0.0;
  for (int base = 0; base < n; base += 64) {
    const double v = base + lane < n ? p[base + lane] : 0.0;
#pragma unroll
    for (int l = 0; l < 64; ++l) acc += svo_readlane_f64(v, l);
  }
  return acc;
}

// robust chi2 of point p's edges at the current estimate, in frame order
__device__ inline double ba_point_chi2(const BaArgs& A, const BaScr& S, const BaLds& L, const BaCam& cam, int p) {
  const double X[3] = {S.X[3 * (size_t)p], S.X[3 * (size_t)p + 1], S.X[3 * (size_t)p + 2]};
  const int m = S.pmask[p];
  size_t e = S.eoff[p];
  double c = 0.0;
  for (int f = 0; f < A.window; ++f) {
    if (!((m >> f) & 1)) continue;
    const bool st = (m >> (8 + f)) & 1;
    double pc[3], er[3], r0, r1;
    ba_edge_error(L.est[f], X, S.eobs + 3 * e, st, cam, pc, er);
    ba_huber(dot3(er[0], er[0], er[1], er[1], er[2], er[2]), st ? A.huber_stereo : A.huber_mono, r0, r1);
    c = c + r0;
    ++e;
  }
  return c;
}

__global__ void __launch_bounds__(BA_NT) k_ba_lm(BaArgs A) {
  __shared__ BaLds L;
  const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, W = A.window, nfix = A.nfix, nfree = W - nfix, n = 6 * nfree;
  const BaScr S = ba_scr(A, w);
  const int P = S.hdr[0], E = S.hdr[1], fmask = S.hdr[3];
  BaCam cam;
  cam.fx = A.fx; cam.fy = A.fy; cam.cx = A.cx; cam.cy = A.cy; cam.bf = A.bf; cam.bf32 = A.bf32;
  if (tid < W) ba_load_pose(A, w, tid, L.Tin[tid], L.est[tid]);
  __syncthreads();
  double* Tout = A.Tout + (size_t)w * W * 16;
  svo_ba_stats* st_out = A.stats + w;
  if (P == 0) {     // no point: the input poses, status "empty"
    for (int i = tid; i < W * 16; i += BA_NT) Tout[i] = L.Tin[i / 16][i % 16];
    if (tid == 0) {
      svo_ba_stats s;
      s.status = SVO_BA_EMPTY; s.n_points = 0; s.n_edges = 0; s.n_edges_stereo = 0; s.iterations = 0; s.trials_total = 0;
      s.chi2_initial = 0.0; s.chi2_final = 0.0; s.lambda_final = 0.0;
      *st_out = s;
    }
    return;
  }
  const int ntri = n * (n + 1) / 2;
  double lam = -1.0, ni = 2.0, cur = 0.0, chi_init = 0.0;
  int nbad = 0, iters = 0, trials_total = 0;
  for (int it = 0; it < A.iterations; ++it) {
    if (tid < W) quat_to_R(L.est[tid].q, L.R[tid]);
    __syncthreads();
    // ---- buildSystem, the part that does not depend on lambda: a lane per point, its edges in frame order
    double mydiag = 0.0;
    for (int p = tid; p < P; p += BA_NT) {
      const double X[3] = {S.X[3 * (size_t)p], S.X[3 * (size_t)p + 1], S.X[3 * (size_t)p + 2]};
      const int m = S.pmask[p];
      size_t e = S.eoff[p];
      double H00 = 0, H01 = 0, H02 = 0, H11 = 0, H12 = 0, H22 = 0, b0 = 0, b1 = 0, b2 = 0, c = 0;
      for (int f = 0; f < W; ++f) {
        if (!((m >> f) & 1)) continue;
        const bool st = (m >> (8 + f)) & 1;
        double pc[3], er[3], r0, wt, Jl[9], Jp[18];
        ba_edge_error(L.est[f], X, S.eobs + 3 * e, st, cam, pc, er);
        ba_huber(dot3(er[0], er[0], er[1], er[1], er[2], er[2]), st ? A.huber_stereo : A.huber_mono, r0, wt);
        ba_jacobians(L.R[f], pc, st, cam, Jl, Jp);
        c = c + r0;
        H00 = H00 + wt * dot3(Jl[0], Jl[0], Jl[3], Jl[3], Jl[6], Jl[6]);
        H01 = H01 + wt * dot3(Jl[0], Jl[1], Jl[3], Jl[4], Jl[6], Jl[7]);
        H02 = H02 + wt * dot3(Jl[0], Jl[2], Jl[3], Jl[5], Jl[6], Jl[8]);
        H11 = H11 + wt * dot3(Jl[1], Jl[1], Jl[4], Jl[4], Jl[7], Jl[7]);
        H12 = H12 + wt * dot3(Jl[1], Jl[2], Jl[4], Jl[5], Jl[7], Jl[8]);
        H22 = H22 + wt * dot3(Jl[2], Jl[2], Jl[5], Jl[5], Jl[8], Jl[8]);
        b0 = b0 - wt * dot3(Jl[0], er[0], Jl[3], er[1], Jl[6], er[2]);
        b1 = b1 - wt * dot3(Jl[1], er[0], Jl[4], er[1], Jl[7], er[2]);
        b2 = b2 - wt * dot3(Jl[2], er[0], Jl[5], er[1], Jl[8], er[2]);
        double* ew = S.ew + 4 * e;
        ew[0] = er[0]; ew[1] = er[1]; ew[2] = er[2]; ew[3] = wt;
        if (f >= nfix) {
          double* jp = S.Jp + 18 * e;
          double* wm = S.Wm + 18 * e;
#pragma unroll
          for (int k = 0; k < 18; ++k) jp[k] = Jp[k];
#pragma unroll
          for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int a = 0; a < 3; ++a) wm[3 * r + a] = wt * dot3(Jp[r], Jl[a], Jp[6 + r], Jl[3 + a], Jp[12 + r], Jl[6 + a]);
        }
        ++e;
      }
      double* h = S.Hll + 6 * (size_t)p;
      h[0] = H00; h[1] = H01; h[2] = H02; h[3] = H11; h[4] = H12; h[5] = H22;
      double* b = S.bl + 3 * (size_t)p;
      b[0] = b0; b[1] = b1; b[2] = b2;
      S.chi[p] = c;
      mydiag = fmax(mydiag, fmax(fabs(H00), fmax(fabs(H11), fabs(H22))));
    }
    L.red[tid] = mydiag;
    __syncthreads();
    // ---- Hpp and bp: a thread per entry walks the points in order; meanwhile the last wave sums chi2
    if (tid < nfree * 27) {
      const int j = tid / 27, q = tid - 27 * j, f = nfix + j;
      int r = 0, c = 0;
      if (q < 21) { int k = q; while (k >= 6 - r) { k -= 6 - r; ++r; } c = r + k; } else { r = q - 21; }
      double acc = 0.0;
      for (int p = 0; p < P; ++p) {
        const int m = S.pmask[p];
        if (!((m >> f) & 1)) continue;
        const size_t e = (size_t)S.eoff[p] + __popc(m & ((1 << f) - 1));
        const double* jp = S.Jp + 18 * e;
        const double* ew = S.ew + 4 * e;
        if (q < 21) acc = acc + ew[3] * dot3(jp[r], jp[c], jp[6 + r], jp[6 + c], jp[12 + r], jp[12 + c]);
        else acc = acc - ew[3] * dot3(jp[r], ew[0], jp[6 + r], ew[1], jp[12 + r], ew[2]);
      }
      if (q < 21) { L.Hpp[j][6 * r + c] = acc; L.Hpp[j][6 * c + r] = acc; } else { L.bp[6 * j + r] = acc; }
    }
    if (tid >= BA_NT - 64) {
      const double c = ba_ordered_sum(S.chi, P, lane);
      if (lane == 0) L.sc[0] = c;
    }
    __syncthreads();
    cur = L.sc[0];
    const double ini = cur;
    if (it == 0) {
      chi_init = cur;
      if (A.lambda_init > 0.0) {
        lam = A.lambda_init;
      } else {      // computeLambdaInit: 1e-5 x the largest diagonal entry over all free vertices
        double md = 0.0;
        for (int j = 0; j < nfree; ++j)
          for (int r = 0; r < 6; ++r) md = fmax(fabs(L.Hpp[j][7 * r]), md);
        for (int t = 0; t < BA_NT; ++t) md = fmax(md, L.red[t]);
        lam = 1e-5 * md;
      }
    }
    double rho = 0.0;
    int qmax = 0;
    do {
      if (tid < 2) L.flag[tid] = 0;
      __syncthreads();
      // ---- Dinv = (Hll + lambda I)^-1 and Y = W Dinv, a lane per point
      for (int p = tid; p < P; p += BA_NT) {
        const double* h = S.Hll + 6 * (size_t)p;
        const double d00 = h[0] + lam, d11 = h[3] + lam, d22 = h[5] + lam, d01 = h[1], d02 = h[2], d12 = h[4];
        const double c00 = d11 * d22 - d12 * d12, c01 = d02 * d12 - d01 * d22, c02 = d01 * d12 - d02 * d11;
        const double det = (d00 * c00 + d01 * c01) + d02 * c02;
        if (!(isfinite(det) && det > 0.0)) atomicOr(&L.flag[0], 1);
        const double inv = 1.0 / det;
        double Di[6];
        Di[0] = c00 * inv; Di[1] = c01 * inv; Di[2] = c02 * inv;
        Di[3] = (d00 * d22 - d02 * d02) * inv; Di[4] = (d01 * d02 - d00 * d12) * inv; Di[5] = (d00 * d11 - d01 * d01) * inv;
        double* o = S.Di + 6 * (size_t)p;
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = Di[k];
        const int m = S.pmask[p] & 0xff;
        size_t e = (size_t)S.eoff[p] + __popc(m & ((1 << nfix) - 1));
        const int cnt = __popc(m >> nfix);
        for (int k = 0; k < cnt; ++k, ++e) {
          const double* wm = S.Wm + 18 * e;
          double* y = S.Y + 18 * e;
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            const double w0 = wm[3 * r], w1 = wm[3 * r + 1], w2 = wm[3 * r + 2];
            y[3 * r] = (w0 * Di[0] + w1 * Di[1]) + w2 * Di[2];
            y[3 * r + 1] = (w0 * Di[1] + w1 * Di[3]) + w2 * Di[4];
            y[3 * r + 2] = (w0 * Di[2] + w1 * Di[4]) + w2 * Di[5];
          }
        }
      }
      __syncthreads();
      // ---- Hschur = (Hpp + lambda I) - sum W Dinv W^T, bschur = bp - sum W Dinv bl: a thread per entry, the points in order
      for (int id = tid; id < ntri + n; id += BA_NT) {
        if (id < ntri) {
          int a = 0, k = id;
          while (k >= n - a) { k -= n - a; ++a; }
          const int b = a + k, fi = a / 6, r = a - 6 * fi, fj = b / 6, c = b - 6 * fj, si = nfix + fi, sj = nfix + fj;
          double s = 0.0;
          for (int p = 0; p < P; ++p) {
            const int m = S.pmask[p];
            if (!(((m >> si) & 1) && ((m >> sj) & 1))) continue;
            const size_t e0 = S.eoff[p];
            const double* y = S.Y + 18 * (e0 + __popc(m & ((1 << si) - 1))) + 3 * r;
            const double* wm = S.Wm + 18 * (e0 + __popc(m & ((1 << sj) - 1))) + 3 * c;
            s = s + dot3(y[0], wm[0], y[1], wm[1], y[2], wm[2]);
          }
          double h = fi == fj ? L.Hpp[fi][6 * r + c] : 0.0;
          if (a == b) h = h + lam;
          L.Hs[a * n + b] = h - s; L.Hs[b * n + a] = h - s;
        } else {
          const int a = id - ntri, fi = a / 6, r = a - 6 * fi, si = nfix + fi;
          double s = 0.0;
          for (int p = 0; p < P; ++p) {
            const int m = S.pmask[p];
            if (!((m >> si) & 1)) continue;
            const double* y = S.Y + 18 * ((size_t)S.eoff[p] + __popc(m & ((1 << si) - 1))) + 3 * r;
            const double* b = S.bl + 3 * (size_t)p;
            s = s + dot3(y[0], b[0], y[1], b[1], y[2], b[2]);
          }
          L.bs[a] = L.bp[a] - s;
        }
      }
      __syncthreads();
      // ---- LDL^T without pivoting in place (L below the diagonal of Hs), a thread per row; a pivot that is not positive fails
      for (int j = 0; j < n; ++j) {
        if (tid == 0) {
          double d = L.Hs[j * n + j];
          for (int k = 0; k < j; ++k) d -= L.Hs[j * n + k] * L.Hs[j * n + k] * L.D[k];
          if (!(d > 0.0)) L.flag[1] = 1;
          L.D[j] = d;
        }
        __syncthreads();
        if (tid > j && tid < n) {
          double s = L.Hs[tid * n + j];
          for (int k = 0; k < j; ++k) s -= L.Hs[tid * n + k] * L.Hs[j * n + k] * L.D[k];
          L.Hs[tid * n + j] = s / L.D[j];
        }
        __syncthreads();
      }
      if (tid == 0) {
        double* y = L.red;     // (the diagonal maxima are used up)
        for (int i = 0; i < n; ++i) {
          double s = L.bs[i];
          for (int k = 0; k < i; ++k) s -= L.Hs[i * n + k] * y[k];
          y[i] = s;
        }
        for (int i = 0; i < n; ++i) y[i] /= L.D[i];
        for (int i = n - 1; i >= 0; --i) {
          double s = y[i];
          for (int k = i + 1; k < n; ++k) s -= L.Hs[k * n + i] * L.x[k];
          L.x[i] = s;
        }
      }
      __syncthreads();
      const bool fail = (L.flag[0] | L.flag[1]) != 0;
      double tmp = DBL_MAX, scale = 1e-3;
      if (!fail) {
        // ---- the points by back-substitution, then the update of every free vertex
        for (int p = tid; p < P; p += BA_NT) {
          const double* b = S.bl + 3 * (size_t)p;
          double t0 = b[0], t1 = b[1], t2 = b[2];
          const int m = S.pmask[p] & 0xff;
          size_t e = (size_t)S.eoff[p] + __popc(m & ((1 << nfix) - 1));
          for (int f = nfix; f < W; ++f) {
            if (!((m >> f) & 1)) continue;
            const double* wm = S.Wm + 18 * e;
            const double* x = L.x + 6 * (f - nfix);
            t0 = t0 - (((((wm[0] * x[0] + wm[3] * x[1]) + wm[6] * x[2]) + wm[9] * x[3]) + wm[12] * x[4]) + wm[15] * x[5]);
            t1 = t1 - (((((wm[1] * x[0] + wm[4] * x[1]) + wm[7] * x[2]) + wm[10] * x[3]) + wm[13] * x[4]) + wm[16] * x[5]);
            t2 = t2 - (((((wm[2] * x[0] + wm[5] * x[1]) + wm[8] * x[2]) + wm[11] * x[3]) + wm[14] * x[4]) + wm[17] * x[5]);
            ++e;
          }
          const double* Di = S.Di + 6 * (size_t)p;
          const double dx0 = (Di[0] * t0 + Di[1] * t1) + Di[2] * t2, dx1 = (Di[1] * t0 + Di[3] * t1) + Di[4] * t2,
                       dx2 = (Di[2] * t0 + Di[4] * t1) + Di[5] * t2;
          double* X = S.X + 3 * (size_t)p;
          double* Xb = S.Xb + 3 * (size_t)p;
          Xb[0] = X[0]; Xb[1] = X[1]; Xb[2] = X[2];
          X[0] = X[0] + dx0; X[1] = X[1] + dx1; X[2] = X[2] + dx2;
          S.sc[p] = (dx0 * (lam * dx0 + b[0]) + dx1 * (lam * dx1 + b[1])) + dx2 * (lam * dx2 + b[2]);
        }
        if (tid >= nfix && tid < W && ((fmask >> tid) & 1)) {     // (a free frame without edges keeps its pose)
          L.bak[tid] = L.est[tid];
          se3_oplus(L.x + 6 * (tid - nfix), L.est[tid]);
        }
        __syncthreads();
        for (int p = tid; p < P; p += BA_NT) S.chi[p] = ba_point_chi2(A, S, L, cam, p);
        __syncthreads();
        if (tid < 64) {
          const double c = ba_ordered_sum(S.chi, P, lane), s = ba_ordered_sum(S.sc, P, lane);
          if (lane == 0) { L.sc[1] = c; L.sc[2] = s; }
        }
        __syncthreads();
        tmp = L.sc[1];
        double sp = 0.0;
        for (int a = 0; a < n; ++a) sp = sp + L.x[a] * (lam * L.x[a] + L.bp[a]);
        scale = (sp + L.sc[2]) + 1e-3;
      }
      rho = (cur - tmp) / scale;
      if (rho > 0 && isfinite(tmp)) {
        const double v = 2 * rho - 1;
        double alpha = 1. - v * v * v;
        alpha = fmin(alpha, 2. / 3.);
        lam *= fmax(1. / 3., alpha);
        ni = 2;
        cur = tmp;
      } else {
        lam *= ni;
        ni *= 2;
        if (!fail) {
          for (int p = tid; p < P; p += BA_NT) {
            double* X = S.X + 3 * (size_t)p;
            const double* Xb = S.Xb + 3 * (size_t)p;
            X[0] = Xb[0]; X[1] = Xb[1]; X[2] = Xb[2];
          }
          if (tid >= nfix && tid < W && ((fmask >> tid) & 1)) L.est[tid] = L.bak[tid];
        }
      }
      __syncthreads();
      ++qmax;
      ++trials_total;
    } while (rho < 0 && qmax < 10);
    ++iters;
    if (qmax == 10 || rho == 0) break;
    if ((ini - cur) * 1e3 < ini) ++nbad; else nbad = 0;
    if (nbad >= 3) break;
  }
  if (tid < W) {
    double T[16];
    const bool moved = tid >= nfix && ((fmask >> tid) & 1);
    if (moved) se3_to_T(L.est[tid], T);
    for (int j = 0; j < 16; ++j) Tout[16 * tid + j] = moved ? T[j] : L.Tin[tid][j];
  }
  if (A.points)
    for (int p = tid; p < P; p += BA_NT) {
      svo_ba_point* o = A.points + (size_t)w * A.points_stride + p;
      o->X = S.X[3 * (size_t)p]; o->Y = S.X[3 * (size_t)p + 1]; o->Z = S.X[3 * (size_t)p + 2];
    }
  if (tid == 0) {
    svo_ba_stats s;
    s.status = SVO_BA_OK; s.n_points = P; s.n_edges = E; s.n_edges_stereo = S.hdr[2]; s.iterations = iters; s.trials_total = trials_total;
    s.chi2_initial = chi_init; s.chi2_final = cur; s.lambda_final = lam;
    *st_out = s;
  }
}

thread_local std::string g_ba_err;

}  // namespace

struct svo_ba {
  int device = 0, max_kp = 0, max_windows = 0;
  int pcap = 0, ecap = 0, nkcap = 0;
  size_t per_window = 0;
  bool ready = false;            // the device side exists (made by the first call that needs it)
  std::string last_error;
  hipStream_t stream = nullptr;
  hipEvent_t producer_done = nullptr;
  uint8_t* d_scratch = nullptr;
  uint8_t* d_stage = nullptr;    // svo_ba_window: records, counts, poses in; poses, points, statistics out
};

#define BA_HIP(b, expr)                                                           \
  do {                                                                            \
    hipError_t _e = (expr);                                                       \
    if (_e != hipSuccess) {                                                       \
      (b)->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);        \
      return SVO_E_HIP;                                                           \
    }                                                                             \
  } while (0)

static int ba_fail(svo_ba* ba, const char* who, const std::string& why) {
  const std::string m = std::string(who) + ": " + why;
  if (ba) ba->last_error = m; else g_ba_err = m;
  return SVO_E_INVALID;
}

static size_t ba_round(size_t v) { return (v + 255) & ~(size_t)255; }
// svo_ba_window's staging: offsets of its six parts
struct BaStage { size_t obs, counts, Tin, Tout, points, stats, total; };
static BaStage ba_stage(const svo_ba* ba) {
  BaStage s;
  size_t o = 0;
  s.obs = o; o += ba_round((size_t)BA_MAXW * ba->max_kp * sizeof(svo_map_obs));
  s.counts = o; o += ba_round(BA_MAXW * sizeof(int32_t));
  s.Tin = o; o += ba_round(BA_MAXW * 16 * sizeof(float));
  s.Tout = o; o += ba_round(BA_MAXW * 16 * sizeof(double));
  s.points = o; o += ba_round((size_t)ba->pcap * sizeof(svo_ba_point));
  s.stats = o; o += ba_round(sizeof(svo_ba_stats));
  s.total = o;
  return s;
}

// the device side of the object, at the first call that needs it (svo_ba_create touches no device: its argument checks and
// those of the calls answer on a machine without one)
static int ba_ready(svo_ba* ba) {
  if (ba->ready) { hipSetDevice(ba->device); return SVO_OK; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ba->device >= ndev) {
    (void)hipGetLastError();
    ba->last_error = "svo_ba: no HIP device " + std::to_string(ba->device);
    return SVO_E_NODEVICE;
  }
  hipSetDevice(ba->device);
  BA_HIP(ba, hipStreamCreateWithFlags(&ba->stream, hipStreamNonBlocking));
  BA_HIP(ba, hipEventCreateWithFlags(&ba->producer_done, hipEventDisableTiming));
  if (hipMalloc(reinterpret_cast<void**>(&ba->d_scratch), ba->per_window * ba->max_windows) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&ba->d_stage), ba_stage(ba).total) != hipSuccess) {
    (void)hipGetLastError();
    ba->last_error = "svo_ba: out of device memory";
    return SVO_E_NOMEM;
  }
  ba->ready = true;
  return SVO_OK;
}

extern "C" int svo_ba_default_params(svo_ba_params* p) {
  if (!p) return SVO_E_INVALID;
  p->window = 8; p->n_fixed = 1; p->iterations = 10; p->stereo = 1;
  p->huber_mono = (double)(float)sqrt(5.991);     // const float deltaMono / deltaStereo of src/Optimizer.cc
  p->huber_stereo = (double)(float)sqrt(7.815);
  p->lambda_init = 0.0;
  return SVO_OK;
}

extern "C" const char* svo_ba_last_error(const svo_ba* ba) { return ba ? ba->last_error.c_str() : g_ba_err.c_str(); }

extern "C" int svo_ba_create(int device, int max_kp, int max_windows, svo_ba** out) {
  if (!out) return ba_fail(nullptr, "svo_ba_create", "out is NULL");
  *out = nullptr;
  if (device < 0) return ba_fail(nullptr, "svo_ba_create", "device is negative");
  if (max_kp < 1 || max_kp > BA_MAX_KP) return ba_fail(nullptr, "svo_ba_create", "max_kp must be 1 .. 4096");
  if (max_windows < 1 || max_windows > 65535) return ba_fail(nullptr, "svo_ba_create", "max_windows must be 1 .. 65535");
  svo_ba* ba = new svo_ba();
  ba->device = device; ba->max_kp = max_kp; ba->max_windows = max_windows;
  ba->pcap = BA_MAXW * max_kp / 2; ba->ecap = BA_MAXW * max_kp;
  ba->nkcap = 2;
  while (ba->nkcap < ba->ecap) ba->nkcap <<= 1;
  ba->per_window = ba_round(ba_per_window(ba->pcap, ba->ecap, ba->nkcap));
  g_ba_err.clear();
  *out = ba;
  return SVO_OK;
}

extern "C" void svo_ba_destroy(svo_ba* ba) {
  if (!ba) return;
  if (ba->ready) {
    hipSetDevice(ba->device);
    hipStreamSynchronize(ba->stream);
    if (ba->d_scratch) hipFree(ba->d_scratch);
    if (ba->d_stage) hipFree(ba->d_stage);
    hipEventDestroy(ba->producer_done);
    hipStreamDestroy(ba->stream);
  }
  delete ba;
}

extern "C" int svo_ba_sync(svo_ba* ba) {
  if (!ba) return SVO_E_INVALID;
  if (!ba->ready) return SVO_OK;
  hipSetDevice(ba->device);
  BA_HIP(ba, hipStreamSynchronize(ba->stream));
  return SVO_OK;
}

extern "C" void* svo_ba_stream(svo_ba* ba) {
  if (!ba || ba_ready(ba) != SVO_OK) return nullptr;
  return ba->stream;
}

// the host-side checks both entries share; NULL `ba` is answered by the callers
static int ba_check(svo_ba* ba, const char* who, const svo_camera* cam, const svo_ba_params* p, int obs_stride) {
  if (!cam) return ba_fail(ba, who, "cam is NULL");
  if (!p) return ba_fail(ba, who, "params is NULL");
  if (p->window < 2 || p->window > BA_MAXW) return ba_fail(ba, who, "window must be 2 .. 8");
  if (p->n_fixed < 1 || p->n_fixed > p->window - 1) return ba_fail(ba, who, "n_fixed must be 1 .. window - 1");
  if (p->iterations < 1 || p->iterations > 20) return ba_fail(ba, who, "iterations must be 1 .. 20");
  if (!std::isfinite(p->huber_mono) || !std::isfinite(p->huber_stereo) || !std::isfinite(p->lambda_init))
    return ba_fail(ba, who, "huber_mono, huber_stereo or lambda_init is not finite");
  if (!std::isfinite(cam->fx) || !std::isfinite(cam->fy) || !std::isfinite(cam->cx) || !std::isfinite(cam->cy) || !std::isfinite(cam->bf))
    return ba_fail(ba, who, "a camera value is not finite");
  if (!(cam->fx > 0.0f) || !(cam->fy > 0.0f)) return ba_fail(ba, who, "camera fx and fy must be positive");
  if (obs_stride < 1 || obs_stride > ba->max_kp) return ba_fail(ba, who, "obs_stride must be 1 .. max_kp");
  return SVO_OK;
}

extern "C" int svo_ba_windows_dev(svo_ba* ba, const svo_camera* cam, const svo_ba_params* p, const svo_map_obs* d_obs,
                                  const int32_t* d_counts, int obs_stride, const void* d_Tcw, int pose_stride_bytes, int first,
                                  int n_windows, int step, double* d_Tcw_out, svo_ba_point* d_points, svo_ba_stats* d_stats,
                                  svo_ctx* producer) {
  const char* who = "svo_ba_windows_dev";
  if (!ba) return ba_fail(nullptr, who, "ba is NULL");
  if (int rc = ba_check(ba, who, cam, p, obs_stride)) return rc;
  if (!d_obs) return ba_fail(ba, who, "d_obs is NULL");
  if (!d_counts) return ba_fail(ba, who, "d_counts is NULL");
  if (!d_Tcw) return ba_fail(ba, who, "d_Tcw is NULL");
  if (!d_Tcw_out) return ba_fail(ba, who, "d_Tcw_out is NULL");
  if (!d_stats) return ba_fail(ba, who, "d_stats is NULL");
  if (reinterpret_cast<uintptr_t>(d_obs) & 15u) return ba_fail(ba, who, "d_obs is not 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_Tcw) & 3u) || pose_stride_bytes < 64 || (pose_stride_bytes & 3))
    return ba_fail(ba, who, "d_Tcw must be 4-byte aligned, pose_stride_bytes a multiple of 4 and >= 64");
  if (n_windows < 1 || n_windows > ba->max_windows) return ba_fail(ba, who, "n_windows must be 1 .. max_windows");
  if (first < 0) return ba_fail(ba, who, "first is negative");
  if (step < 1) return ba_fail(ba, who, "step must be >= 1");
  if (producer && producer->device != ba->device) return ba_fail(ba, who, "producer context on another device");
  if (int rc = ba_ready(ba)) return rc;
  if (producer) {     // behind the tracker call that writes the records and poses; the producer waits for nothing
    BA_HIP(ba, hipEventRecord(ba->producer_done, producer->stream));
    BA_HIP(ba, hipStreamWaitEvent(ba->stream, ba->producer_done, 0));
  }
  BaArgs A;
  A.obs = d_obs; A.counts = d_counts; A.obs_stride = obs_stride;
  A.Tcw = static_cast<const uint8_t*>(d_Tcw); A.pose_stride = pose_stride_bytes; A.first = first; A.step = step;
  A.window = p->window; A.nfix = p->n_fixed; A.iterations = p->iterations; A.stereo = p->stereo != 0;
  A.huber_mono = p->huber_mono; A.huber_stereo = p->huber_stereo; A.lambda_init = p->lambda_init;
  A.fx = (double)cam->fx; A.fy = (double)cam->fy; A.cx = (double)cam->cx; A.cy = (double)cam->cy; A.bf = (double)cam->bf; A.bf32 = cam->bf;
  A.nk = 2;
  while (A.nk < p->window * obs_stride) A.nk <<= 1;
  A.scratch = ba->d_scratch; A.per_window = ba->per_window; A.pcap = ba->pcap; A.ecap = ba->ecap; A.nkcap = ba->nkcap;
  A.Tout = d_Tcw_out; A.points = d_points; A.points_stride = p->window * ba->max_kp / 2; A.stats = d_stats;
  hipLaunchKernelGGL(k_ba_assoc, dim3(n_windows), dim3(BA_NT), 0, ba->stream, A);
  hipLaunchKernelGGL(k_ba_lm, dim3(n_windows), dim3(BA_NT), 0, ba->stream, A);
  BA_HIP(ba, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_ba_window(svo_ba* ba, const svo_camera* cam, const svo_ba_params* p, const svo_map_obs* obs, const int32_t* counts,
                             int obs_stride, const float* Tcw, double* Tcw_out, svo_ba_point* points, int32_t* n_points,
                             svo_ba_stats* stats) {
  const char* who = "svo_ba_window";
  if (!ba) return ba_fail(nullptr, who, "ba is NULL");
  if (int rc = ba_check(ba, who, cam, p, obs_stride)) return rc;
  if (!obs || !counts || !Tcw || !Tcw_out || !stats) return ba_fail(ba, who, "obs, counts, Tcw, Tcw_out or stats is NULL");
  if ((points == nullptr) != (n_points == nullptr)) return ba_fail(ba, who, "points and n_points go together");
  if (int rc = ba_ready(ba)) return rc;
  const BaStage s = ba_stage(ba);
  const int W = p->window;
  uint8_t* d = ba->d_stage;
  BA_HIP(ba, hipStreamSynchronize(ba->stream));
  BA_HIP(ba, hipMemcpyAsync(d + s.obs, obs, (size_t)W * obs_stride * sizeof(svo_map_obs), hipMemcpyHostToDevice, ba->stream));
  BA_HIP(ba, hipMemcpyAsync(d + s.counts, counts, W * sizeof(int32_t), hipMemcpyHostToDevice, ba->stream));
  BA_HIP(ba, hipMemcpyAsync(d + s.Tin, Tcw, (size_t)W * 16 * sizeof(float), hipMemcpyHostToDevice, ba->stream));
  if (int rc = svo_ba_windows_dev(ba, cam, p, reinterpret_cast<const svo_map_obs*>(d + s.obs), reinterpret_cast<const int32_t*>(d + s.counts),
                                  obs_stride, d + s.Tin, 64, 0, 1, 1, reinterpret_cast<double*>(d + s.Tout),
                                  points ? reinterpret_cast<svo_ba_point*>(d + s.points) : nullptr,
                                  reinterpret_cast<svo_ba_stats*>(d + s.stats), nullptr))
    return rc;
  BA_HIP(ba, hipMemcpyAsync(Tcw_out, d + s.Tout, (size_t)W * 16 * sizeof(double), hipMemcpyDeviceToHost, ba->stream));
  BA_HIP(ba, hipMemcpyAsync(stats, d + s.stats, sizeof(svo_ba_stats), hipMemcpyDeviceToHost, ba->stream));
  BA_HIP(ba, hipStreamSynchronize(ba->stream));
  if (points) {
    *n_points = stats->n_points;
    if (stats->n_points > 0) {
      BA_HIP(ba, hipMemcpyAsync(points, d + s.points, (size_t)stats->n_points * sizeof(svo_ba_point), hipMemcpyDeviceToHost, ba->stream));
      BA_HIP(ba, hipStreamSynchronize(ba->stream));
    }
  }
  return SVO_OK;
}
