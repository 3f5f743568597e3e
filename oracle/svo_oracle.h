/* svo_oracle.h - CPU restatement (plain C) of the stereo-VO tracking hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under stereo-semantic-vo_amd/ may include,
 * link or call this; only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg use it, and only as the checker / the timed CPU baseline.
 *
 * PARITY UNPINNED for the OpenCV-delegated stages (ORB, BFMatcher, 8-point F,
 * solvePnPRansac): the reference holds no tests or golden vectors, OpenCV 3.2 is
 * neither vendored nor installed, and the reference cannot be built here
 * (SURVEY.md section 8c).  The own-code stages (DescriptorDistance, the two
 * matching passes, disp2Depth / UnprojectStereo, the g2o pose-only LM) follow the
 * reference sources line by line; each function cites the lines it restates.
 */
#ifndef SVO_ORACLE_H
#define SVO_ORACLE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ORC_NLEVELS 8
#define ORC_EDGE 31          /* cv::ORB edgeThreshold default */
#define ORC_FAST_THR 20      /* cv::ORB fastThreshold default */
#define ORC_HALF_PATCH 15
#define ORC_CAP1 1024        /* cap on Harris candidates per level */

typedef struct orc_kp {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} orc_kp;

typedef struct orc_lm_stats {
  int32_t n_edges, iterations, trials_total, terminated;
  double chi2_initial, chi2_final, lambda_final;
} orc_lm_stats;

typedef struct orc_pnp_stats {
  int32_t n_points, n_inliers, best_hypothesis, ok, iterations;
} orc_pnp_stats;

/* geometry */
int orc_geometry(int W, int H, int nfeatures, int32_t w[8], int32_t h[8], float scale[8],
                 int32_t quota[8]);
void orc_umax(int32_t umax[16]);
int64_t orc_pyramid_size(int W, int H);
int64_t orc_level_offset(int W, int H, int level);

/* ORB stages */
void orc_resize_linear_u8(const uint8_t* src, int sw, int sh, int sstride, uint8_t* dst,
                          int dw, int dh, int dstride);
void orc_build_pyramid(const uint8_t* gray, int W, int H, int stride, uint8_t* pyr);
int orc_fast_score_at(const uint8_t* img, int w, int h, int stride, int x, int y);
int orc_fast_corners(const uint8_t* img, int w, int h, int stride, int thr, int border,
                     int32_t* xys, int cap);
int64_t orc_harris_at(const uint8_t* img, int stride, int x, int y);
float orc_harris_to_float(int64_t R);
float orc_fast_atan2(float y, float x);
float orc_ic_angle(const uint8_t* img, int stride, int x, int y);
void orc_sincos(float angle_rad, float* s, float* c);
void orc_gaussian_blur7(const uint8_t* src, int w, int h, int sstride, uint8_t* dst, int dstride);
void orc_describe(const uint8_t* blurred, int stride, int x, int y, float angle_deg,
                  uint8_t desc[32]);
int orc_orb_from_pyramid(const uint8_t* pyr, int W, int H, int nfeatures, orc_kp* kp,
                         uint8_t* desc);
int orc_orb_extract(const uint8_t* gray, int W, int H, int stride, int nfeatures, orc_kp* kp,
                    uint8_t* desc, uint8_t* pyr_out);

/* sparse stereo */
int orc_stereo_match(const uint8_t* pyrL, const uint8_t* pyrR, int W, int H, const orc_kp* kpL,
                     const uint8_t* dL, int nL, const orc_kp* kpR, const uint8_t* dR, int nR,
                     float bf, float fx, float* uR, float* depth);
int orc_stereo_frame(const uint8_t* grayL, int strideL, const uint8_t* grayR, int strideR, int W,
                     int H, int nfeatures, float bf, float fx, orc_kp* kpL, uint8_t* dL,
                     int32_t* nL, float* uR, float* depth, orc_kp* kpR, uint8_t* dR,
                     int32_t* nR);
void orc_disp2depth(const float* disp, int count, float bf, float* depth);
void orc_unproject(const float* uvz, int n, float fx, float fy, float cx, float cy,
                   const float Rwc[9], const float twc[3], float* xyz);

/* matching */
int orc_descriptor_distance(const uint8_t* a, const uint8_t* b);
void orc_hamming_argmin(const uint8_t* q, int M, const uint8_t* t, int N, const uint8_t* t_mask,
                        int32_t* best_idx, int32_t* best, int32_t* second);
void orc_match_greedy(const uint8_t* q, const uint8_t* q_skip, int M, const uint8_t* t, int N,
                      uint8_t* assigned, int max_dist, float ratio, int32_t* best_idx,
                      int32_t* best, int32_t* second, uint8_t* accepted);
void orc_bf_match(const uint8_t* q, int M, const uint8_t* t, int N, int32_t* train_idx,
                  int32_t* dist, uint8_t* keep);

/* pose */
void orc_huber(double e, double delta, double rho[3]);
void orc_se3_exp(const double upd[6], double q_xyzw[4], double t[3]);
/* the three coefficients of SE3Quat::exp: {sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3}; use_libm = 1: se3quat.h:240-250's
 * formulas on libm, 0: the fixed series the restatement (and the HIP path) evaluates for |t| < 0.5 (orc_pose.c) */
void orc_exp_coeffs(double t, double abc[3], int use_libm);
void orc_se3_exp_matrix(const double upd[6], double T[16]);
void orc_se3_update(const double upd[6], double T[16]);
int orc_pose_opt(const double* Xw, const double* obs, int n, const double K[4], double T[16],
                 orc_lm_stats* stats, double* trace, int trace_cap);
/* branch counters of the last orc_pose_opt call: se3_exp per regime (theta < 1e-5, series, libm), quat_from_R per branch (trace > 0,
 * largest diagonal 0 / 1 / 2), quaternions flipped for q.w < 0 (orc_pose.c) */
extern int32_t orc_pose_last_counts[8];
/* cv::solvePnPRansac(..., false, 100, 8.0, 0.99, inliers) restated (orc_pnp_cv.c).  T_fallback: the pose reported when
 * OpenCV returns false; rng_state 0 = (uint64)-1, what RANSACPointSetRegistrator::run seeds its cv::RNG with. */
int orc_pnp_ransac(const double* Xw, const double* obs, int n, const double K[4],
                   const double T_fallback[16], uint64_t rng_state, double T[16], uint8_t* inlier_mask,
                   orc_pnp_stats* stats);
int orc_solvepnp_ransac(const double* Xw, const double* obs, int n, const double K[4], const double T_fallback[16],
                        uint64_t rng_state, int refine, double T[16], uint8_t* inlier_mask, orc_pnp_stats* stats);
/* RANSACUpdateNumIters(p, ep, modelPoints, maxIters): the iteration bound of RANSACPointSetRegistrator::run */
int orc_ransac_update_num_iters(double p, double ep, int modelPoints, int maxIters);
/* the same for p = 0.99, modelPoints = 5 on arrays (the tests' exhaustive tables) */
void orc_ransac_update_num_iters_batch(const double* ep, const int32_t* maxIters, int count, int32_t* out);
void orc_ransac_log_denom_batch(const double* ep, int count, double* out);   /* log(1 - (1 - ep)^5) as that function computes it */
/* epnp::compute_pose on five correspondences: R (row-major 3x3), t */
void orc_epnp5(const double Xw5[15], const double uv5[10], const double K[4], double R_out[9], double t_out[3]);

/* fundamental matrix + semantic gating (orc_fmat.c) */
int orc_fundamental_8point(const double* pts1, const double* pts2, int n, double F[9]);
int orc_point_in_boxes(float x, float y, const int32_t* boxes, int n_boxes, int pad);
double orc_epipolar_distance(const double F[9], float last_x, float last_y, float cur_x, float cur_y);

/* tracking loop (orc_track.c) */
typedef struct orc_track_result {
  float Tcw[16];
  int32_t frame_id, n_kp, n_stereo, n_match_pass1, n_match_pass2, n_pnp_inliers, n_lm_edges,
      n_new_mappoints, n_local_map, lm_iterations, reserved[2];
} orc_track_result;
typedef struct orc_tracker orc_tracker;
orc_tracker* orc_track_create(int W, int H, int nfeatures, float fx, float fy, float cx, float cy,
                              float bf);
void orc_track_destroy(orc_tracker* t);
int orc_track_last_vetoes(const orc_tracker* t);
/* teacher forcing for the next orc_track_frame / _boxes / _dense call (see orc_track_tail's Tcw_force) */
void orc_track_force_pose(orc_tracker* t, const float Tcw[16]);
/* cur_mp_out (nullable): nfeatures int32, pool index matched to each keypoint or -1 */
int orc_track_frame(orc_tracker* t, const uint8_t* grayL, int strideL, const uint8_t* grayR,
                    int strideR, orc_track_result* res, int32_t* cur_mp_out);
/* same, with the frame's offline detection boxes: n_boxes x {left,right,top,bottom} (main.cpp:82-95) */
int orc_track_frame_dense(orc_tracker* t, const uint8_t* grayL, int strideL, const uint8_t* grayR,
                          int strideR, const float* dense_disp, const int32_t* boxes, int n_boxes,
                          orc_track_result* res, int32_t* cur_mp_out, double F_out[9]);
int orc_track_frame_boxes(orc_tracker* t, const uint8_t* grayL, int strideL, const uint8_t* grayR,
                          int strideR, const int32_t* boxes, int n_boxes, orc_track_result* res,
                          int32_t* cur_mp_out, double F_out[9]);
/* the ordered tail alone, for given front-end results (see orc_track.c); Tcw_force: teacher forcing (nullable) */
typedef struct orc_tail_debug {
  int32_t match_gid[512];   /* per keypoint: creation sequence number of the map point matched to it (frame 0: created by init), -1 none */
  int32_t new_gid[512];     /* per keypoint: creation sequence number of the map point created from it at the frame's end, -1 none */
  orc_pnp_stats pnp;        /* cv::solvePnPRansac's outcome (zeros on frame 0) */
  double T_pnp[16];         /* the pose it returned (row-major 4x4), before the CV_32F rounding and the LM */
} orc_tail_debug;
int orc_track_tail(orc_tracker* t, const orc_kp* kp, const uint8_t* desc, int nkp, const float* depth,
                   const int32_t* boxes, int n_boxes, const float* Tcw_force, orc_track_result* res,
                   int32_t* cur_mp_out, double F_out[9], orc_tail_debug* dbg);

#ifdef __cplusplus
}
#endif
/* first stage of MSA dense stereo (orc_msa.c): MSA::init, Thirdparty/MB/MSA.cpp:22-139 */
int orc_msa_init(const uint8_t* bgrL, const uint8_t* bgrR, int n, int m, int disp, float* costL, float* costR,
                 uint8_t* m3L, uint8_t* m3R, double* r_graL, double* c_graL, double* r_graR, double* c_graR);

/* tree stages of MSA::solve (orc_msa.c): setExp :1126-1130, TreeDp :929-990, WTA :992-1006, LRcheck :1027-1105 */
void orc_msa_exp_table(double o, double Exp[256]);
int orc_msa_tree_dp(const float* cost, int N, int D, const int32_t* seq, const int32_t* child_ptr,
                    const int32_t* child, const uint8_t* child_c, int root, const double Exp[256], float* costUp,
                    float* costA);
int orc_msa_wta(const float* costA, int n, int m, int D, uint8_t* disparity);
int orc_msa_lrcheck(const uint8_t* d1, const uint8_t* d2, int n, int m, int D, float* cost, uint8_t* mask);

/* graph stages + MSA::solve (orc_msa_graph.cpp, C++): MSA.cpp:152-373, 661-808, 854-926, 1132-1169 */
int orc_msa_tree(const uint8_t* m_img3, const double* r_gra, const double* c_gra, int n, int m, int32_t* seq,
                 int32_t* child_ptr, int32_t* child, uint8_t* child_c);
int orc_msa_solve(const uint8_t* bgrL, const uint8_t* bgrR, int n, int m, int d, int scale, uint8_t* out);

#endif
