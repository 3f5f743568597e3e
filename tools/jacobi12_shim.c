/* Fixture maker's view into the CPU restatement (tools/make_jacobi12_cases.py): the sweeps of JacobiSVDImpl_ on a given 12 x 12
 * matrix, as the wave engine's M = 12 step loop (csrc/svo_epnp_ord_dev.h, jacobi_rows<12>) has to reproduce them bit for bit.
 * The restatement is included as it stands (cv_hypot, fill_M, ...); the sweep loop below is jacobi_svd's (without V), counted,
 * with the step loop's own view of every pair test beside it: was the pair inside the 2^-40 margin of the rotation threshold, where
 * the loop leaves the comparison of the squares for the exact expression? */
#include "../oracle/orc_pnp_cv.c"

/* temp_a = (M^T M)^T of a five-point sample, as compute_pose's cvMulTransposed / the engine's load_mtm leave it: At[12 b + a]. */
void shim_jacobi12_mtm(const double Xw5[15], const double uv5[10], const double K[4], double At[144]) {
  epnp_t e;
  e.fu = K[0]; e.fv = K[1]; e.uc = K[2]; e.vc = K[3];
  e.n = 5;
  memcpy(e.pws, Xw5, sizeof e.pws);
  memcpy(e.us, uv5, sizeof e.us);
  choose_control_points(&e);
  compute_barycentric_coordinates(&e);
  double M[10 * 12];
  for (int i = 0; i < 5; i++) fill_M(&e, M, 2 * i, e.alphas + 4 * i, e.us[2 * i], e.us[2 * i + 1]);
  for (int a = 0; a < 12; ++a)
    for (int b = 0; b < 12; ++b) {
      double s = 0;
      for (int r = 0; r < 10; ++r) s += M[12 * r + a] * M[12 * r + b];
      At[12 * b + a] = s;
    }
}

/* The sweeps on At (in place).  Returns their number (the last one rotates nothing; 30: it ran out of them).  rows[144]: the rows
 * scaled by 1 / w[i], w[12]: sqrt(sum_k At[i][k]^2) (before the sort).  und[0] / und[1]: pair tests inside the margin that resolved
 * to "rotate" / "leave"; und[2..4]: sweep, i, j of the first such test (-1: none); und[5]: rotations in all. */
int shim_jacobi12_sweeps(double At[144], double rows[144], double w[12], int und[6]) {
  const double eps = DBL_EPSILON * 10, eps2 = eps * eps;
  const double eps2hi = eps2 * (1.0 + 9.094947017729282e-13), eps2lo = eps2 * (1.0 - 9.094947017729282e-13);   /* 2^-40 */
  double W[12];
  int iter;
  und[0] = und[1] = und[5] = 0; und[2] = und[3] = und[4] = -1;
  for (int i = 0; i < 12; i++) { double sd = 0; for (int k = 0; k < 12; k++) sd += At[12 * i + k] * At[12 * i + k]; W[i] = sd; }
  for (iter = 0; iter < 30; iter++) {
    int changed = 0;
    for (int i = 0; i < 11; i++)
      for (int j = i + 1; j < 12; j++) {
        double *Ai = At + 12 * i, *Aj = At + 12 * j, a = W[i], p = 0, b = W[j], c, s;
        for (int k = 0; k < 12; k++) p += Ai[k] * Aj[k];
        const int leave = fabs(p) <= eps * sqrt(a * b);
        {
          const double g = p * p, ab = a * b;
          if (!(g > ab * eps2hi) && !(g < ab * eps2lo)) {
            und[leave ? 1 : 0]++;
            if (und[2] < 0) { und[2] = iter; und[3] = i; und[4] = j; }
          }
        }
        if (leave) continue;
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
        und[5]++;
      }
    if (!changed) break;
  }
  for (int i = 0; i < 12; i++) {
    double sd = 0;
    for (int k = 0; k < 12; k++) sd += At[12 * i + k] * At[12 * i + k];
    w[i] = sqrt(sd);
    const double sc = 1 / w[i];
    for (int k = 0; k < 12; k++) rows[12 * i + k] = At[12 * i + k] * sc;
  }
  return iter < 30 ? iter + 1 : 30;
}
