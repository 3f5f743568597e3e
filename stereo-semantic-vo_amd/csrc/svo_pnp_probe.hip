// svo_pnp_probe.hip - parity probes of RANSAC's stopping rule and consensus count (svo_debug_pnp_rule, svo_debug_pnp_consensus)
// and of the 12 x 12 step loop of the order-preserving EPnP (svo_debug_jacobi12):
// kernels that call the device functions of svo_pose_dev.h exactly as svo_pose.hip's and the tracker's kernels do, their launchers
// and C entries.  A translation unit of its own: nothing the library runs outside the tests is compiled differently for it.
#define EO_JACOBI12_STEPS 1      // jacobi_rows<12> of THIS translation unit leaves its step count in S.sweeps
#include "svo_pose_dev.h"

// Table mode: what the tracker tabulates per frame - pnp_update_terms(g, n) for every consensus g = 5 .. n -, the plain
// pnp_update_iters(ep, 100) beside it, and log(0.01) as the rule spells it (pnp_log_1mp).  out_d[g] = ld (g = 0 .. n; 0 below 5),
// out_d[n + 1] = log(0.01); out_i[g] = r, out_i[n + 1 + g] = pnp_update_iters.
__global__ __launch_bounds__(64) void k_pnp_rule_table(int n, double* out_d, int* out_i) {
  for (int g = threadIdx.x; g <= n; g += 64) {
    double ld = 0.0; int r = 0, it = 0;
    if (g >= 5) {
      pnp_update_terms(g, n, &ld, &r);
      it = pnp_update_iters((double)(n - g) / n, PNP_HYP);
    }
    out_d[g] = ld; out_i[g] = r; out_i[n + 1 + g] = it;
  }
  if (threadIdx.x == 0) out_d[n + 1] = pnp_log_1mp();
}
// Rule mode: one thread per case (cnt[100], ok[100], n): every instantiation of the one walker (pnp_walk) on the same samples.  Per
// case SVO_PNP_RULE_W ints: pnp_select's {best, good, iters}; pnp_select_pre's, with the terms made per sample as the tracker's tail
// makes them; then for m = 0 .. 100 the walk over the prepared terms cut at m, as the fused tail runs it with m = TP_EARLY -
// {visited, visited again (the column a separate copy of the loop once filled), best, good (-2: cut, nothing decided)} - and
// pnp_bound_after(m).
__global__ __launch_bounds__(64) void k_pnp_rule_cases(const int* __restrict__ cnt_all, const int* __restrict__ ok_all,
                                                       const int* __restrict__ n_all, int ncases, int* out_all) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= ncases) return;
  const int n = n_all[c];
  int cnt[PNP_HYP], ok[PNP_HYP], r[PNP_HYP];
  double ld[PNP_HYP];
  for (int h = 0; h < PNP_HYP; ++h) {
    cnt[h] = cnt_all[(size_t)c * PNP_HYP + h]; ok[h] = ok_all[(size_t)c * PNP_HYP + h];
    ld[h] = 1.0; r[h] = 0;
    if (ok[h] && cnt[h] > 4 && n > 5) pnp_update_terms(cnt[h], n, &ld[h], &r[h]);
  }
  int* out = out_all + (size_t)c * SVO_PNP_RULE_W;
  int good = 0, iters = 0;
  out[0] = pnp_select(cnt, ok, n, &good, &iters); out[1] = good; out[2] = iters;
  good = 0; iters = 0;
  out[3] = pnp_select_pre(cnt, ok, ld, r, n, &good, &iters); out[4] = good; out[5] = iters;
  for (int m = 0; m <= PNP_HYP; ++m) {
    int* o = out + 6 + 5 * m;
    const PnpWalk w = pnp_walk<true>(cnt, ok, ld, r, n, m);
    const bool ended = w.visited <= m;
    o[0] = w.visited; o[1] = w.visited;
    o[2] = ended ? w.best : -2; o[3] = ended ? w.good : -2;
    o[4] = pnp_bound_after(cnt, ok, n, m);
  }
}
// The consensus of one model over n points by ONE wave: pnp_consensus_wave, the function the three pnp_hyp_* kernels count with,
// here with its per-point flags.  Rt: R row-major, then t.
__global__ __launch_bounds__(64) void k_pnp_consensus_probe(const double* __restrict__ Xw, const double* __restrict__ uv, int n,
                                                            const double* __restrict__ Kp, const double* __restrict__ Rt,
                                                            int* count, uint8_t* flags) {
  const int lane = threadIdx.x;
  const double K[4] = {Kp[0], Kp[1], Kp[2], Kp[3]};
  double R[9], t[3];
  for (int i = 0; i < 9; ++i) R[i] = Rt[i];
  for (int i = 0; i < 3; ++i) t[i] = Rt[9 + i];
  const int cnt = pnp_consensus_wave(R, t, Xw, uv, n, K, flags);
  if (lane == 0) *count = cnt;
}
// The 12 x 12 step loop alone, ONE wave: the matrix goes into S.jr as solve5_wave's load_mtm leaves M^T M there (row b of At = row
// b of S.jr, everything else zero), jacobi_rows<12> runs on it as in a RANSAC sample.  rows: the 12 rows of S.jr afterwards (16
// doubles each: rotated, scaled by 1 / W, W in column 15); out_i: {steps, the step loop ran out of sweeps}.
__global__ __launch_bounds__(64) void k_jacobi12_probe(const double* __restrict__ At, double* __restrict__ rows, int* __restrict__ out_i) {
  __shared__ epnp_ord::Lds S;
  const int lane = threadIdx.x, r16 = lane & 15;
  for (int e = lane; e < 16 * 16; e += 64) S.jr[e] = 0.0;
  if (lane == 0) { S.flag = 0; S.why = 0; S.sweeps = 0; }
  epnp_ord::load_tables(S, lane);
  EO_SYNC();
  for (int e = lane; e < 144; e += 64) S.jr[(e / 12) * 16 + e % 12] = At[e];
  EO_SYNC();
  const unsigned long long ex = epnp_ord::jacobi_rows<12>(S, r16 < 12 ? 12 : 0, r16 < 12 ? 0 : r16, lane);
  for (int e = lane; e < 12 * 16; e += 64) rows[e] = S.jr[e];
  if (lane == 0) { out_i[0] = S.sweeps; out_i[1] = ex != 0 ? 1 : 0; }
}
static int svo_launch_jacobi12_probe(svo_ctx* ctx, const double* At, double* rows, int* out_i) {
  hipLaunchKernelGGL(k_jacobi12_probe, dim3(1), dim3(64), 0, ctx->stream, At, rows, out_i);
  SVO_HIP(ctx, hipGetLastError());
  return SVO_OK;
}
static int svo_launch_pnp_rule_table(svo_ctx* ctx, int n, double* out_d, int* out_i) {
  hipLaunchKernelGGL(k_pnp_rule_table, dim3(1), dim3(64), 0, ctx->stream, n, out_d, out_i);
  SVO_HIP(ctx, hipGetLastError());
  return SVO_OK;
}
static int svo_launch_pnp_rule_cases(svo_ctx* ctx, const int* cnt, const int* ok, const int* n, int ncases, int* out) {
  hipLaunchKernelGGL(k_pnp_rule_cases, dim3((ncases + 63) / 64), dim3(64), 0, ctx->stream, cnt, ok, n, ncases, out);
  SVO_HIP(ctx, hipGetLastError());
  return SVO_OK;
}
static int svo_launch_pnp_consensus_probe(svo_ctx* ctx, const double* Xw, const double* uv, int n, const double* K, const double* Rt,
                                   int* count, uint8_t* flags) {
  hipLaunchKernelGGL(k_pnp_consensus_probe, dim3(1), dim3(64), 0, ctx->stream, Xw, uv, n, K, Rt, count, flags);
  SVO_HIP(ctx, hipGetLastError());
  return SVO_OK;
}

// device scratch by bump allocation / copies on the context's stream (as svo_api.hip's entries do)
namespace {
struct Bump {
  svo_ctx* ctx; size_t off = 0;
  template <typename T> T* take(size_t count) {
    off = (off + 255) & ~size_t(255);
    T* p = reinterpret_cast<T*>(ctx->d_scratch + off);
    off += count * sizeof(T);
    return p;
  }
  bool ok() const { return off <= ctx->scratch_bytes / 2; }
};
}
#define H2D(dst, src, bytes) SVO_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream))
#define D2H(dst, src, bytes) SVO_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream))

extern "C" int svo_debug_pnp_rule(svo_ctx* ctx, int mode, int count, const int32_t* cnt, const int32_t* ok, const int32_t* n,
                                  double* out_f64, int32_t* out_i32) {
  if (!ctx || !out_i32) return SVO_E_INVALID;
  hipSetDevice(ctx->device);
  Bump bm{ctx};
  if (mode == SVO_PNP_RULE_TABLE) {          // count: the number of points n
    if (count < 5 || count > 512 || !out_f64) return SVO_E_INVALID;
    double* dD = bm.take<double>((size_t)count + 2);
    int* dI = bm.take<int>(2 * ((size_t)count + 1));
    if (!bm.ok()) return SVO_E_CAPACITY;
    int rc = svo_launch_pnp_rule_table(ctx, count, dD, dI);
    if (rc) return rc;
    D2H(out_f64, dD, 8 * ((size_t)count + 2));
    D2H(out_i32, dI, 8 * ((size_t)count + 1));
    SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SVO_OK;
  }
  if (mode != SVO_PNP_RULE_CASES || count < 1 || count > 4096 || !cnt || !ok || !n) return SVO_E_INVALID;
  for (int c = 0; c < count; ++c)
    if (n[c] < 5 || n[c] > 512) return SVO_E_INVALID;
  int* dC = bm.take<int>((size_t)count * 100);
  int* dO = bm.take<int>((size_t)count * 100);
  int* dN = bm.take<int>(count);
  int* dR = bm.take<int>((size_t)count * SVO_PNP_RULE_W);
  if (!bm.ok()) return SVO_E_CAPACITY;
  H2D(dC, cnt, 400 * (size_t)count); H2D(dO, ok, 400 * (size_t)count); H2D(dN, n, 4 * (size_t)count);
  int rc = svo_launch_pnp_rule_cases(ctx, dC, dO, dN, count, dR);
  if (rc) return rc;
  D2H(out_i32, dR, 4 * (size_t)count * SVO_PNP_RULE_W);
  SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVO_OK;
}

extern "C" int svo_debug_pnp_consensus(svo_ctx* ctx, const double* Xw, const double* obs, int n, const double K[4], const double R[9],
                                       const double t[3], int32_t* count, uint8_t* flags) {
  if (!ctx || !Xw || !obs || !K || !R || !t || !count || !flags) return SVO_E_INVALID;
  if (n < 1) return SVO_E_INVALID;
  if (n > 512) return SVO_E_CAPACITY;
  hipSetDevice(ctx->device);
  Bump bm{ctx};
  double* dX = bm.take<double>(3 * (size_t)n); double* dU = bm.take<double>(2 * (size_t)n); double* dK = bm.take<double>(4);
  double* dRt = bm.take<double>(12); int* dCnt = bm.take<int>(1); uint8_t* dF = bm.take<uint8_t>(n);
  if (!bm.ok()) return SVO_E_CAPACITY;
  H2D(dX, Xw, 24 * (size_t)n); H2D(dU, obs, 16 * (size_t)n); H2D(dK, K, 32);
  H2D(dRt, R, 72); H2D(dRt + 9, t, 24);
  int rc = svo_launch_pnp_consensus_probe(ctx, dX, dU, n, dK, dRt, dCnt, dF);
  if (rc) return rc;
  D2H(count, dCnt, 4); D2H(flags, dF, n);
  SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SVO_OK;
}

extern "C" int svo_debug_jacobi12(svo_ctx* ctx, const double At[144], double rows_out[12 * 16], int32_t* steps, int32_t* flag) {
  if (!ctx || !At || !rows_out || !steps || !flag) return SVO_E_INVALID;
  hipSetDevice(ctx->device);
  Bump bm{ctx};
  double* dA = bm.take<double>(144); double* dR = bm.take<double>(12 * 16); int* dI = bm.take<int>(2);
  if (!bm.ok()) return SVO_E_CAPACITY;
  H2D(dA, At, 8 * 144);
  int rc = svo_launch_jacobi12_probe(ctx, dA, dR, dI);
  if (rc) return rc;
  int32_t hi[2] = {0, 0};
  D2H(rows_out, dR, 8 * 12 * 16); D2H(hi, dI, 8);
  SVO_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *steps = hi[0]; *flag = hi[1];
  return SVO_OK;
}
