/* Fixture maker's view into the CPU restatement (tools/make_epnp_unrolled_cases.py): how the 12 x 12 decomposition of a
 * five-point sample ends.  The restatement is included as it stands; the sweep loop below is jacobi_svd's (without V), counted. */
#include "../oracle/orc_pnp_cv.c"

/* Returns the number of sweeps JacobiSVDImpl_ runs on M^T M of the sample (the last one rotates nothing; 30: it ran out of them).
 * w[12]: the singular values before the sort.  cc[3]: singular values of the control points' 3 x 3 problem. */
int shim_epnp5_sweeps12(const double Xw5[15], const double uv5[10], const double K[4], double w[12], double cc[3]) {
  epnp_t e;
  e.fu = K[0]; e.fv = K[1]; e.uc = K[2]; e.vc = K[3];
  e.n = 5;
  memcpy(e.pws, Xw5, sizeof e.pws);
  memcpy(e.us, uv5, sizeof e.us);
  {   /* choose_control_points' PW0^T PW0 and its singular values */
    double c0[3] = {0, 0, 0}, pw0[15], ptp[9], ut[9], vt[9];
    for (int i = 0; i < 5; i++) for (int j = 0; j < 3; j++) c0[j] += e.pws[3 * i + j];
    for (int j = 0; j < 3; j++) c0[j] /= 5;
    for (int i = 0; i < 5; i++) for (int j = 0; j < 3; j++) pw0[3 * i + j] = e.pws[3 * i + j] - c0[j];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) { double s = 0; for (int r = 0; r < 5; ++r) s += pw0[3 * r + a] * pw0[3 * r + b]; ptp[3 * a + b] = s; }
    svd_compute(ptp, 3, 3, cc, ut, vt);
  }
  choose_control_points(&e);
  compute_barycentric_coordinates(&e);
  double M[10 * 12], At[144], W[12];
  for (int i = 0; i < 5; i++) fill_M(&e, M, 2 * i, e.alphas + 4 * i, e.us[2 * i], e.us[2 * i + 1]);
  for (int a = 0; a < 12; ++a)
    for (int b = 0; b < 12; ++b) {
      double s = 0;
      for (int r = 0; r < 10; ++r) s += M[12 * r + a] * M[12 * r + b];
      At[12 * b + a] = s;                         /* temp_a = (M^T M)^T */
    }
  const double eps = DBL_EPSILON * 10;
  int iter;
  for (int i = 0; i < 12; i++) { double sd = 0; for (int k = 0; k < 12; k++) sd += At[12 * i + k] * At[12 * i + k]; W[i] = sd; }
  for (iter = 0; iter < 30; iter++) {
    int changed = 0;
    for (int i = 0; i < 11; i++)
      for (int j = i + 1; j < 12; j++) {
        double *Ai = At + 12 * i, *Aj = At + 12 * j, a = W[i], p = 0, b = W[j], c, s;
        for (int k = 0; k < 12; k++) p += Ai[k] * Aj[k];
        if (fabs(p) <= eps * sqrt(a * b)) continue;
        p *= 2;
        double beta = a - b, gamma = cv_hypot(p, beta);
        if (beta < 0) { double delta = (gamma - beta) * 0.5; s = sqrt(delta / gamma); c = p / (gamma * s * 2); }
        else { c = sqrt((gamma + beta) / (gamma * 2)); s = p / (gamma * c * 2); }
        a = b = 0;
        for (int k = 0; k < 12; k++) {
          double t0 = c * Ai[k] + s * Aj[k], t1 = -s * Ai[k] + c * Aj[k];
          Ai[k] = t0; Aj[k] = t1;
          a += t0 * t0; b += t1 * t1;
        }
        W[i] = a; W[j] = b;
        changed = 1;
      }
    if (!changed) break;
  }
  for (int i = 0; i < 12; i++) { double sd = 0; for (int k = 0; k < 12; k++) sd += At[12 * i + k] * At[12 * i + k]; w[i] = sqrt(sd); }
  return iter < 30 ? iter + 1 : 30;
}
