/* Fixture maker's view into the CPU restatement (tools/make_epnp_small_cases.py): how the five 3 x 3 decompositions of a five-point
 * sample end - choose_control_points' PW0^T PW0, cvInvert(CC) and the three candidates' ABt.  The restatement is included as it
 * stands and run as orc_epnp5 runs it; each 3 x 3 matrix it hands to svd_compute is built here once more by the same expressions
 * and goes through jacobi_svd's sweep loop (without V, which takes no part in the decisions), counted. */
#include "../oracle/orc_pnp_cv.c"

/* sweeps JacobiSVDImpl_ runs on the 3 x 3 matrix A (the last one rotates nothing; 30: it ran out of them); w[3]: the singular
 * values before the sort */
static int sweeps3(const double* A, double* w) {
  double At[9], W[3];
  const double eps = DBL_EPSILON * 10;
  int iter;
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) At[3 * i + k] = A[3 * k + i];      /* temp_a = A^T */
  for (int i = 0; i < 3; i++) { double sd = 0; for (int k = 0; k < 3; k++) sd += At[3 * i + k] * At[3 * i + k]; W[i] = sd; }
  for (iter = 0; iter < 30; iter++) {
    int changed = 0;
    for (int i = 0; i < 2; i++)
      for (int j = i + 1; j < 3; j++) {
        double *Ai = At + 3 * i, *Aj = At + 3 * j, a = W[i], p = 0, b = W[j], c, s;
        for (int k = 0; k < 3; k++) p += Ai[k] * Aj[k];
        if (fabs(p) <= eps * sqrt(a * b)) continue;
        p *= 2;
        double beta = a - b, gamma = cv_hypot(p, beta);
        if (beta < 0) { double delta = (gamma - beta) * 0.5; s = sqrt(delta / gamma); c = p / (gamma * s * 2); }
        else { c = sqrt((gamma + beta) / (gamma * 2)); s = p / (gamma * c * 2); }
        a = b = 0;
        for (int k = 0; k < 3; k++) {
          double t0 = c * Ai[k] + s * Aj[k], t1 = -s * Ai[k] + c * Aj[k];
          Ai[k] = t0; Aj[k] = t1;
          a += t0 * t0; b += t1 * t1;
        }
        W[i] = a; W[j] = b;
        changed = 1;
      }
    if (!changed) break;
  }
  for (int i = 0; i < 3; i++) { double sd = 0; for (int k = 0; k < 3; k++) sd += At[3 * i + k] * At[3 * i + k]; w[i] = sqrt(sd); }
  return iter < 30 ? iter + 1 : 30;
}

static int abt_sweeps(const epnp_t* e, double* w) {       /* estimate_R_and_t's ABt of the candidate whose pcs are in e */
  const int n = e->n;
  double pc0[3] = {0, 0, 0}, pw0[3] = {0, 0, 0}, abt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < n; i++)
    for (int j = 0; j < 3; j++) { pc0[j] += e->pcs[3 * i + j]; pw0[j] += e->pws[3 * i + j]; }
  for (int j = 0; j < 3; j++) { pc0[j] /= n; pw0[j] /= n; }
  for (int i = 0; i < n; i++) {
    const double* pc = e->pcs + 3 * i;
    const double* pw = e->pws + 3 * i;
    for (int j = 0; j < 3; j++) {
      abt[3 * j] += (pc[j] - pc0[j]) * (pw[0] - pw0[0]);
      abt[3 * j + 1] += (pc[j] - pc0[j]) * (pw[1] - pw0[1]);
      abt[3 * j + 2] += (pc[j] - pc0[j]) * (pw[2] - pw0[2]);
    }
  }
  return sweeps3(abt, w);
}

/* sweeps[5], w[15]: control points, CC, ABt of candidates 1, 2, 3.  Returns 1 if the restatement's own svd_compute reports two
 * EQUAL singular values for the control points' problem (dc[] after its sort), else 0. */
int shim_epnp5_small(const double Xw5[15], const double uv5[10], const double K[4], int sweeps[5], double w[15]) {
  epnp_t e;
  e.fu = K[0]; e.fv = K[1]; e.uc = K[2]; e.vc = K[3];
  e.n = 5;
  memcpy(e.pws, Xw5, sizeof e.pws);
  memcpy(e.us, uv5, sizeof e.us);
  int equal;
  {   /* choose_control_points' PW0^T PW0 */
    double c0[3] = {0, 0, 0}, pw0[15], ptp[9], dc[3], ut[9], vt[9];
    for (int i = 0; i < 5; i++) for (int j = 0; j < 3; j++) c0[j] += e.pws[3 * i + j];
    for (int j = 0; j < 3; j++) c0[j] /= 5;
    for (int i = 0; i < 5; i++) for (int j = 0; j < 3; j++) pw0[3 * i + j] = e.pws[3 * i + j] - c0[j];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) { double s = 0; for (int r = 0; r < 5; ++r) s += pw0[3 * r + a] * pw0[3 * r + b]; ptp[3 * a + b] = s; }
    sweeps[0] = sweeps3(ptp, w);
    svd_compute(ptp, 3, 3, dc, ut, vt);
    equal = dc[0] == dc[1] || dc[1] == dc[2];
  }
  choose_control_points(&e);
  {   /* compute_barycentric_coordinates' CC */
    double cc[9];
    for (int i = 0; i < 3; i++)
      for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = e.cws[j][i] - e.cws[0][i];
    sweeps[1] = sweeps3(cc, w + 3);
  }
  compute_barycentric_coordinates(&e);
  double M[10 * 12], mtm[144], d[12], ut[144], vt[144];
  for (int i = 0; i < 5; i++) fill_M(&e, M, 2 * i, e.alphas + 4 * i, e.us[2 * i], e.us[2 * i + 1]);
  for (int a = 0; a < 12; ++a)
    for (int b = 0; b < 12; ++b) {
      double s = 0;
      for (int r = 0; r < 10; ++r) s += M[12 * r + a] * M[12 * r + b];
      mtm[12 * a + b] = s;
    }
  svd_compute(mtm, 12, 12, d, ut, vt);
  double l_6x10[60], rho[6], betas[4], R[3][3], t[3];
  compute_L_6x10(ut, l_6x10);
  compute_rho(&e, rho);
  find_betas_approx_1(l_6x10, rho, betas);
  gauss_newton(l_6x10, rho, betas);
  compute_R_and_t(&e, ut, betas, R, t);
  sweeps[2] = abt_sweeps(&e, w + 6);
  find_betas_approx_2(l_6x10, rho, betas);
  gauss_newton(l_6x10, rho, betas);
  compute_R_and_t(&e, ut, betas, R, t);
  sweeps[3] = abt_sweeps(&e, w + 9);
  find_betas_approx_3(l_6x10, rho, betas);
  gauss_newton(l_6x10, rho, betas);
  compute_R_and_t(&e, ut, betas, R, t);
  sweeps[4] = abt_sweeps(&e, w + 12);
  return equal;
}
