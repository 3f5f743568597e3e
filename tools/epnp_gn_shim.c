/* Fixture maker's and CPU test's view into the CPU restatement's gauss_newton (tools/make_epnp_gn_cases.py,
 * tests/test_epnp_gn_cpu.py).  The restatement is included as it stands.  Exported:
 *   shim_gn         the restatement's gauss_newton itself
 *   shim_gn_count   a second walk of the same loops that counts, per iteration and Householder step k, the branches taken
 *   shim_gn_cols    the column-ordered restatement: what the wave solver of csrc/svo_epnp_ord_dev.h does, lane by lane, in C -
 *                   three "lanes" own a column of A each, the fourth owns b, every lane redoes the pivot column's work */
#include "../oracle/orc_pnp_cv.c"

void shim_gn(const double L[60], const double rho[6], double betas[4]) { gauss_newton(L, rho, betas); }

/* cnt[it][k][0..3]: 1 if step k of iteration it met a negative pivot (after scaling) / took eta from a row below the diagonal /
 * met eta == 0 (qr_solve returns: the later steps of that iteration are not reached) / has |A[5][k]| >= 1e6 eta, the row the scan
 * never looks at.  betas: in / out, as gauss_newton.  Returns 0 if the walk ended on the bits of gauss_newton, else 1. */
int shim_gn_count(const double L[60], const double rho[6], double betas[4], unsigned char cnt[5][4][4]) {
  double ref[4] = {betas[0], betas[1], betas[2], betas[3]};
  gauss_newton(L, rho, ref);
  memset(cnt, 0, 5 * 4 * 4);
  for (int it = 0; it < 5; it++) {
    double A[6][4], b[6], x[4] = {0, 0, 0, 0}, A1[4], A2[4];
    compute_A_and_b_gauss_newton(L, rho, betas, &A[0][0], b);
    int k;
    for (k = 0; k < 4; k++) {
      const double diag = fabs(A[k][k]);
      double eta = diag;
      for (int i = k + 1; i < 6; i++) {
        const double elt = fabs(A[i - 1][k]);
        if (eta < elt) eta = elt;
      }
      if (eta == 0) { cnt[it][k][2] = 1; break; }
      if (eta != diag) cnt[it][k][1] = 1;
      if (fabs(A[5][k]) >= 1e6 * eta) cnt[it][k][3] = 1;
      double sum2 = 0.0;
      const double inv_eta = 1. / eta;
      for (int i = k; i < 6; i++) { A[i][k] *= inv_eta; sum2 += A[i][k] * A[i][k]; }
      double sigma = sqrt(sum2);
      if (A[k][k] < 0) { sigma = -sigma; cnt[it][k][0] = 1; }
      A[k][k] += sigma;
      A1[k] = sigma * A[k][k];
      A2[k] = -eta * sigma;
      for (int j = k + 1; j < 4; j++) {
        double sum = 0;
        for (int i = k; i < 6; i++) sum += A[i][k] * A[i][j];
        const double tau = sum / A1[k];
        for (int i = k; i < 6; i++) A[i][j] -= tau * A[i][k];
      }
    }
    if (k == 4) {
      for (int j = 0; j < 4; j++) {
        double tau = 0;
        for (int i = j; i < 6; i++) tau += A[i][j] * b[i];
        tau /= A1[j];
        for (int i = j; i < 6; i++) b[i] -= tau * A[i][j];
      }
      x[3] = b[3] / A2[3];
      for (int i = 2; i >= 0; i--) {
        double sum = 0;
        for (int j = i + 1; j < 4; j++) sum += A[i][j] * x[j];
        x[i] = (b[i] - sum) / A2[i];
      }
    }
    for (int i = 0; i < 4; i++) betas[i] += x[i];
  }
  return memcmp(ref, betas, sizeof ref) != 0;
}

/* One Householder step k as a lane sees it: p the pivot column (rows k..5 valid), o[q] the column lane q owns (q = 0, 1, 2:
 * columns 1, 2, 3 of A; q = 3: b).  R[k][j], j > k: the finished row k of column j; R[k][0]: the finished b[k]. */
static void cols_step(int k, double p[6], double o[4][6], double R[4][4], double A2[4], int* alive) {
  double eta = fabs(p[k]);
  for (int i = k + 1; i < 6; i++) {
    const double elt = fabs(p[i - 1]);
    if (eta < elt) eta = elt;
  }
  if (eta == 0) *alive = 0;
  const double inv_eta = 1. / eta;
  double sum2 = 0.0;
  for (int i = k; i < 6; i++) { p[i] *= inv_eta; sum2 += p[i] * p[i]; }
  double sigma = sqrt(sum2);
  if (p[k] < 0) sigma = -sigma;
  p[k] += sigma;
  const double A1 = sigma * p[k];
  A2[k] = -eta * sigma;
  for (int q = 3; q >= 0; q--) {          /* the lanes, in any order: a lane whose column is final leaves it alone */
    if (q < k) continue;
    double sum = 0;
    for (int i = k; i < 6; i++) sum += p[i] * o[q][i];
    const double tau = sum / A1;
    for (int i = k; i < 6; i++) o[q][i] -= tau * p[i];
  }
  for (int j = k + 1; j < 4; j++) R[k][j] = o[j - 1][k];
  R[k][0] = o[3][k];
  if (k < 3)
    for (int i = k + 1; i < 6; i++) p[i] = o[k][i];
}

void shim_gn_cols(const double L[60], const double rho[6], double betas[4]) {
  for (int it = 0; it < 5; it++) {
    double a[24], b[6], p[6], o[4][6], R[4][4], A2[4], x[4];
    int alive = 1;
    compute_A_and_b_gauss_newton(L, rho, betas, a, b);
    for (int i = 0; i < 6; i++) {
      p[i] = a[4 * i];
      for (int q = 0; q < 3; q++) o[q][i] = a[4 * i + q + 1];
      o[3][i] = b[i];
    }
    for (int k = 0; k < 4; k++) cols_step(k, p, o, R, A2, &alive);
    x[3] = R[3][0] / A2[3];
    for (int i = 2; i >= 0; i--) {
      double sum = 0;
      for (int j = i + 1; j < 4; j++) sum += R[i][j] * x[j];
      x[i] = (R[i][0] - sum) / A2[i];
    }
    for (int i = 0; i < 4; i++) betas[i] += alive ? x[i] : 0.0;
  }
}

/* n systems at once (the seeded runs of the CPU test): betas n x 4 in / out; which: 0 gauss_newton, 1 the column-ordered walk */
void shim_gn_many(int which, int n, const double* L, const double* rho, double* betas) {
  for (int s = 0; s < n; s++) {
    if (which) shim_gn_cols(L + 60 * s, rho + 6 * s, betas + 4 * s);
    else gauss_newton(L + 60 * s, rho + 6 * s, betas + 4 * s);
  }
}
