/* svo.h - C-ABI of the MI355X-native stereo-VO tracking front end.
 *
 * This is the drop-in boundary.  The reference
 * (zssjh/stereo-semantic-vo) exposes no plugin/FFI seam around its hot path: the
 * seams are C++ member functions that write into public members of `frame`.
 * Every entry point below names the reference method it replaces (file:line under
 * the reference tree).  The one true C-ABI the reference owns - the YOLO dlopen
 * interface, include/YOLOv3SE.h:61-64,221-230 - is the model for the conventions:
 * opaque handle, caller-owned buffers, plain pointers and sizes, int return.
 *
 * Conventions
 *   - `svo_ctx` is one tracker context bound to ONE GPU (one HIP stream inside).
 *     Not thread-safe per context; use one context per host thread / per GPU.
 *   - All buffers are caller-owned.  Entry points ending in `_dev` take DEVICE
 *     pointers (HBM-resident, e.g. torch tensors' data_ptr()) and enqueue on the
 *     context stream without synchronising; all others take HOST pointers and
 *     return after the result is in the caller's memory.
 *   - Return 0 (SVO_OK) or a negative svo_status.  Nothing here falls back to a
 *     CPU path: if no HIP device is usable, svo_create fails with SVO_E_NODEVICE.
 *   - Images are 8-bit gray, row-major, `stride` bytes per row - except in the entries named _bgr, which take the 8UC3
 *     BGR images the reference reads (interleaved B, G, R bytes, `stride` >= 3 * W bytes per row; "colour input" below).
 *   - Keypoints use the 28-byte layout of cv::KeyPoint (pt.x, pt.y, size, angle,
 *     response, octave, class_id) so `frame::keypoints_l` can alias the buffer.
 *   - Descriptors are n x 32 bytes row-major, like `frame::f_descriptor`
 *     (CV_8U 500x32, reference src/frame.cc:78).
 */
#ifndef SVO_H
#define SVO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVO_ABI_VERSION 8   /* 8, backward-compatible addition: svo_debug_msa_plan (which kernels the last MSA tree aggregation ran as; a host-side
                              probe, see there); no existing entry changed.
                              8, backward-compatible addition: svo_loop_* (SearchByBoW matching and the fixed-scale Sim3Solver on the device; see
                              "loop verification" below); no existing entry changed.
                              8, backward-compatible addition: svo_bow_* (DBoW2 bag-of-words place recognition on the device; see "bag-of-words
                              place recognition" below); no existing entry changed.
                              8, backward-compatible addition: svo_ba_* (windowed bundle adjustment on the device over the map records; see
                              "windowed bundle adjustment" below); no existing entry changed.
                              8, backward-compatible addition: svo_track_map_out, svo_map_obs (each tracked frame's map points and observations
                              in HBM; see "the map behind a tracked frame" below); no existing entry changed.
                              8, backward-compatible addition: svo_debug_stereo_match (the sparse stereo matcher on the caller's keypoints, a
                              parity probe; see there); no existing entry changed.
                              8, backward-compatible addition: svo_track_multi_step_bgr_dev, and the dynamic-keypoint loop in the
                              many-sequence mode (svo_track_dynamic then svo_track_multi_reset; see "LK inside the tracker" below); no
                              existing entry changed.
                              7, backward-compatible additions: svo_dyn_default_params, svo_track_dynamic, svo_track_dynamic_out (the
                              dynamic-keypoint Lucas-Kanade loop inside the device-resident tracker, see "LK inside the tracker" below);
                              no existing entry changed.
                              7, backward-compatible additions: svo_sgbm_process_mode, svo_sgbm_process_bgr_mode, svo_sgbm_batch_mode_dev,
                              svo_sgbm_batch_bgr_mode_dev and the option "sgbm_mode" (the eight-direction MODE_HH, see "semi-global block
                              matching: MODE_HH" below); no existing entry changed.
                              7, backward-compatible additions: svo_lk_track_bgr, svo_lk_batch_bgr_dev, svo_lk_chain_bgr_dev,
                              svo_lk_debug_level_bgr (Lucas-Kanade on 8UC3 BGR frames, see "sparse pyramidal Lucas-Kanade" below); no
                              existing entry changed.
                              7, backward-compatible additions: svo_bgr_to_gray, svo_track_frame_bgr, svo_track_batch_bgr_dev,
                              svo_track_batch_bgr_host (8UC3 BGR input, see "colour input" below); no existing entry changed.
                              7 (round 6): + svo_track_batch_host, svo_track_sharded_host, svo_frontend_batch_host (pipelined host-fed entries:
                              images start in host memory, uploads run on a copy stream ahead of the front end, records come back to
                              host memory; svo_boxes_host), svo_create_ex (per-context stream mode), svo_stream_mode; svo_sync also
                              completes the host-fed calls' outputs.  Later: version 4's two-launch RANSAC switch is no longer accepted (SVO_E_INVALID).
                              6 (round 5, late): + svo_debug_stream_pipes.  BEHAVIOUR: a context's four main streams are hardware queues of their own,
                              created back to back at svo_create (four dispatch pipes; see svo_debug_stream_pipes) - they are BLOCKING
                              streams (they order against the NULL stream, as every hipExtStreamCreateWithCUMask stream does) without a
                              priority, kept off each other by CU masks; SVO_POOLED_QUEUES=1 restores the pooled streams of ABI 5.
                              5 (round 5): option "tail_fused" (default 1: RANSAC samples + frame part of the default solver in one launch);
                              svo_debug_stream_probe's second value is now a ratio in per cent (see there); "epnp_exact" accepts every
                              non-zero value again (ABI 3's meaning); svo_destroy waits for batched / sharded work in flight.
                              4 (round 4): + svo_track_epnp_fallbacks, svo_debug_stream_probe; "epnp_exact" defaults to 2 (the
                              order-preserving solver); options gate_group, hyp_first, dense_cu_percent, a two-launch RANSAC switch,
                              epnp_force_seq, shard_force_staged; svo_track_sharded_dev overlaps consecutive calls.
                              No signature of version 3 changed.  BEHAVIOUR changes a version-3 caller sees: (i) the tracker's
                              default RANSAC solver is the bit-comparable one - 8.8 k instead of 14.4 k frames/s on the headline
                              run, and a sample with a zero / repeated singular value is re-solved sequentially (counted by
                              svo_track_epnp_fallbacks; "epnp_exact" = 0 restores round 3's solver and rate); (ii) "epnp_exact"
                              keeps version 3's meaning for every value but 2: any other non-zero value selects the one-lane
                              checker (mode 1). */

typedef enum svo_status {
  SVO_OK = 0,
  SVO_E_INVALID = -1,   /* bad argument (null pointer, size out of range) */
  SVO_E_NODEVICE = -2,  /* no usable HIP device / kernels not loadable  */
  SVO_E_NOMEM = -3,     /* device or host allocation failed              */
  SVO_E_HIP = -4,       /* a HIP runtime call failed; see svo_last_error */
  SVO_E_CAPACITY = -5,  /* batch / keypoint capacity of the ctx exceeded */
  SVO_E_TIMEOUT = -6    /* svo_sync: a bounded wait inside the tracker's pose chain ran out (sticky flag 4, svo_track_overflowed): the frame
                           concerned was tracked as a PnP failure (its record has n_pnp_inliers = -1), nothing stale was used; returned
                           once per svo_track_reset / svo_track_multi_reset, whatever the number of sequences (svo_last_error then
                           names the sequences concerned); the context continues with the two-launch pose chain ("tail_fused" = 0) */
} svo_status;

typedef struct svo_ctx svo_ctx;

/* cv::KeyPoint-compatible record (reference: vector<cv::KeyPoint> keypoints_l,
 * include/frame.h:48). */
typedef struct svo_kp {
  float x, y;      /* pt, level-0 pixel coordinates                      */
  float size;      /* 31 * 1.2^octave                                     */
  float angle;     /* degrees [0,360), intensity-centroid orientation     */
  float response;  /* Harris response                                     */
  int32_t octave;  /* pyramid level 0..7                                  */
  int32_t class_id;/* -1                                                  */
} svo_kp;

/* Camera intrinsics the reference reads from the yaml (src/Tracking.cc:24-38). */
typedef struct svo_camera {
  float fx, fy, cx, cy, bf;
} svo_camera;

/* Statistics of one pose-only LM run (mirrors what g2o's verbose mode prints,
 * Thirdparty/g2o/g2o/core/sparse_optimizer.cpp:395-409). */
typedef struct svo_lm_stats {
  int32_t n_edges;        /* edges used (return value of PoseOptimization)  */
  int32_t iterations;     /* outer iterations executed (<= 10)              */
  int32_t trials_total;   /* inner lambda trials over all iterations        */
  int32_t terminated;     /* 1 if an LM stop rule fired before 10 iters     */
  double chi2_initial;    /* robust chi2 before the first iteration         */
  double chi2_final;      /* robust chi2 at the accepted estimate           */
  double lambda_final;
} svo_lm_stats;

/* Result of cv::solvePnPRansac (src/pnpmatch.cc:227). */
typedef struct svo_pnp_stats {
  int32_t n_points;
  int32_t n_inliers;       /* consensus of the winning sample (rows of `inliers`, src/pnpmatch.cc:229) */
  int32_t best_hypothesis; /* index 0..99 of the winning minimal sample, -1 if none */
  int32_t ok;              /* 0 => OpenCV would return false (fewer than 5 points / no consensus of 5): pose = fallback */
  int32_t iterations;      /* samples the adaptive RANSAC loop visited (<= 100) */
} svo_pnp_stats;

/* Per-frame record produced by the tracker (what Tracking::Track leaves behind:
 * pose + counters, src/Tracking.cc:180-252). */
typedef struct svo_track_result {
  float Tcw[16];           /* row-major 4x4, CV_32F like frame::Tcw        */
  int32_t frame_id;
  int32_t n_kp;            /* keypoints extracted on the left image         */
  int32_t n_stereo;        /* keypoints with depth > 0                      */
  int32_t n_match_pass1;   /* last-frame map points matched (best < 15)     */
  int32_t n_match_pass2;   /* local-map points matched (best<30, ratio>2)   */
  int32_t n_pnp_inliers;
  int32_t n_lm_edges;
  int32_t n_new_mappoints;
  int32_t n_local_map;     /* local-map size after culling                  */
  int32_t lm_iterations;
  int32_t reserved[2];
} svo_track_result;

/* Offline detection boxes (main.cpp:59-97: one box per line, 4 ints `left right top bottom`) of a device-resident
 * call, as HBM arrays: frame (or sequence) f of the call has n[f] boxes (0 <= n[f] <= 64) of four int32 each at
 * boxes + 4 * stride * f.  All pointers are DEVICE pointers; a NULL svo_boxes_dev*, NULL members or n[f] = 0 mean "no boxes". */
typedef struct svo_boxes_dev {
  const int32_t* boxes;
  const int32_t* n;
  int32_t stride;          /* boxes reserved per frame (>= the largest n[f]) */
} svo_boxes_dev;

/* The same for the host-fed entries (svo_track_batch_host, svo_track_sharded_host): HOST pointers, frame f of the call has
 * n[f] boxes at boxes + 4 * stride * f - main.cpp:82-95 reads them from one text file per frame. */
typedef struct svo_boxes_host {
  const int32_t* boxes;
  const int32_t* n;
  int32_t stride;
} svo_boxes_host;

/* Parity probe record of one tracked frame (svo_debug_track_frames). */
typedef struct svo_track_debug {
  int32_t match_gid[512];  /* per keypoint: identity (creation sequence number) of the map point matched to it by
                            * Tracking::init / pass 1 / pass 2 (CurrentFrame->MapPoints[j]), -1 none */
  int32_t new_gid[512];    /* per keypoint: identity of the map point frame::createmappoint made from it, -1 none */
  int32_t frame_id;
  int32_t pnp_best, pnp_iterations, pnp_inliers, pnp_ok;   /* cv::solvePnPRansac: winning sample, samples visited, consensus */
  int32_t active_rows[2], rounds[2];   /* matching passes 1 / 2: rows that could match at all, resolution rounds */
  int32_t resolve_us;      /* duration of the frame's k_ti_resolve launch (in-kernel wall clock) */
  int64_t rt[6];           /* in-kernel wall clock (s_memrealtime, 10 ns ticks): k_ti_resolve start / end, first RANSAC-sample
                            * workgroup start, k_tp_frame end, k_tp_frame start; rt[5] is a DURATION in the same ticks: the hand-over
                            * of the fused pose launch, from the latest announcement of an awaited RANSAC sample to the LM's first
                            * build (0 for frames without RANSAC or not decided within the awaited samples) */
  double T_pnp[16];        /* the pose solvePnPRansac returned (row-major 4x4), before the CV_32F rounding and the LM */
} svo_track_debug;

/* ---- lifecycle ----------------------------------------------------------- */

int svo_abi_version(void);
const char* svo_strerror(int status);
/* Text of the last HIP/runtime failure on this ctx ("" if none). */
const char* svo_last_error(const svo_ctx* ctx);

/* One context per GPU.  W,H: image size; max_kp: keypoint budget per image (the
 * reference hard-codes N = 500, src/frame.cc:54); max_batch: the largest number of
 * stereo pairs one batched call may carry (>= 1). */
int svo_create(svo_ctx** out, int device, int W, int H, int max_kp, int max_batch);
/* svo_create with a per-context stream mode (flags; 0 = svo_create's default):
 *   default: the context's four main streams (pose chain = the stream every host-buffer entry runs on, index chain, batched front
 *     end, dense stage) are four hardware queues of their own made back to back - four dispatch pipes whatever the process created
 *     before (svo_debug_stream_pipes).  They are BLOCKING streams (HIP has no non-blocking CU-masked stream): work another component
 *     of the process puts on the NULL stream orders against them both ways.  The pose / index queues keep off the CUs the batched
 *     front end is confined to (the first mask word: four CUs of every XCD) - 7/8 of the chip for everything that runs on them.
 *   SVO_CREATE_TAIL_ALL_CUS: those two queues may use every CU - for a context that does not run the batched tracker
 *     (front-end-only, ELAS / MSA, host-buffer entries: they run on the first queue and get the whole chip).
 *   SVO_CREATE_POOLED_STREAMS: the runtime's pooled, prioritised NON-BLOCKING streams instead (ABI 5): no ordering against the
 *     NULL stream; every further stream is picked by measuring against the streams it must run beside; the rate depends on what
 *     the process created before.  svo_create sets it when the environment has SVO_POOLED_QUEUES=1 (read at
 *     every call).  Also what a device without CU-masked streams falls back to.
 * svo_stream_mode: what is in effect - bit 0: dedicated queues, bit 1: the tail's queues are confined off the front end's CUs. */
#define SVO_CREATE_POOLED_STREAMS 1u
#define SVO_CREATE_TAIL_ALL_CUS 2u
int svo_create_ex(svo_ctx** out, int device, int W, int H, int max_kp, int max_batch, uint32_t flags);
int svo_stream_mode(const svo_ctx* ctx);
void svo_destroy(svo_ctx* ctx);
/* Tuning switches.  "pose_mfma" (0..2, default 1): how svo_pose_opt and the tracker's pose optimisation add up the edges' terms of
 * H = J^T W J, b = -J^T W e and chi2 - always in the edges' insertion order, each addition rounded (g2o's loops,
 * base_unary_edge.hpp:43-72): 1 four edges per v_mfma_f64_4x4x4_4b_f64 (A = 1.0: an in-order sum of the four lane groups' values),
 * 2 one lane per quantity with plain additions, 0 one lane for everything (the CPU loop as it stands).  Identical bits in all
 * three, and identical to the CPU restatement.
 * "fast_cand_cap" (default 2048, the maximum): length of the per-tile list of scored pixels in the FAST kernel; tiles
 * with more fall back to scanning the score tile - same results, the switch exists so that tests can force that path.
 * "track_lcap" (default 8, the maximum): claimable keypoints (Hamming distance < 30) a map point keeps as packed
 * entries in the tracker's matching passes; rows with more are evaluated on their full distance row instead - same results, the switch exists so that tests
 * can force that path.
 * "track_nblk" (default 3, the maximum): runner-up blockers stored with each packed entry; with fewer the matching passes
 * consult the full distance row more often - same results, a test switch like "track_lcap".
 * "frontend_overlap" (default 2, 0..8): slices of a batch svo_frontend_batch_dev runs side by side on their own streams
 * (scheduling only; 0 / 1: one chain; also one chain while svo_profile_enable is on, so that per-kernel times are those of
 * kernels running alone).
 * "pyr_fused" (default 1): the pyramid as three fused launches (levels kept in LDS); 0: one launch per level - same levels.
 * "track_group" (default 4, 1..64): most frames the batched tracker's pose chain takes over from its index chain per
 * stream event (group sizes ramp up 1, 1, 2, 4, ...) - scheduling only, same records.
 * "multi_pipeline" (default 0): svo_track_multi_step_dev runs the front end of a step beside the tail of the previous
 * step (its own stream, two alternating private output sets) - same records.  Contract while it is on: between consecutive
 * steps nothing else is enqueued on the context (svo_sync and reading results are fine); svo_track_multi_reset restarts it.
 * "depth_source" (default 0): where svo_track_frame / svo_track_batch_dev take keypoint depth from - 0 the sparse
 * epipolar matcher (north star), 1 a dense ELAS map (svo_elas_*), 3 a dense SGBM map (svo_sgbm_* with svo_sgbm_default_params of the
 * image height: the body of the reference's frame::ElasMatch; on the gray, also in the _bgr entries; invalid pixels are -1, so
 * their keypoints get depth -bf and fail every z > 0 test, as in the reference), 2 a dense MSA map (svo_msa_solve with d = 48: the
 * reference's live configuration, src/Tracking.cc:225-228 + src/frame.cc:82-91 - on the reference's colour input through the _bgr
 * entries; the gray entries hand MSA B = G = R copies of the gray), both read per keypoint as frame::computekeypoint_r /
 * disp2Depth do.
 * "sgbm_mode" (default 0 = SVO_SGBM_MODE_SGBM; 1 = SVO_SGBM_MODE_HH): the mode of the SGBM maps of depth_source 3 - of the gray
 * solver in the gray tracker entries and in the _bgr ones, and of the cn = 3 solver there with "sgbm_colour" = 1 (default 0: the
 * _bgr entries run SGBM on the gray they make).  Other depth sources ignore it.
 * "fe_cu_percent" (default 12 = 32 of the 256 CUs, 10..100): share of the compute units (whole 32-bit words of the CU mask; measured
 * with tools/microbench/cu_mask_probe: the first word is FOUR CUs ON EACH of the eight XCDs, not one XCD) the front-end stream of
 * svo_track_batch_dev may use.  Its kernels would otherwise fill every CU while the ordered tail runs beside them, and the
 * tail's small dependent kernels then queue for slots (7 us per frame on average); the front end needs a tenth of the tail's
 * time on the whole chip, so an eighth of it keeps up (measured: 100 % 13.2 k, 25 % 14.1 k, 12 % 14.4 k frames/s).  Scheduling only -
 * same records.
 * "dense_cu_percent" (default 88 = seven eighths of the CUs, 10..100): the same for the dense front end's stream of svo_track_batch_dev with
 * depth_source = 1 (ORB + ELAS maps + depth lookups, in chunks, beside the tail of the earlier chunks): ELAS needs most of the chip,
 * the tail's 100 single-wave RANSAC workgroups need free CUs (measured with boxes, 256 frames per call: 100 % 5.4 k, 75 % 6.4 k,
 * 50 % 5.3 k frames/s; with the later 16-pair chunks: 75 % 6.7-6.8 k, 88 % 6.9 k, 100 % 6.0 k).  Scheduling only - same records.
 * "hyp_first" (default 8; 4, 8, 12 or 16): many sequences per step (svo_track_multi_step_dev): RANSAC samples per sequence in the
 * step's first launch; the second launch holds as many again, the third the rest, and their workgroups leave at once when
 * cv::solvePnPRansac's adaptive iteration bound says the loop never reaches their sample (it visits a median of 4 samples on
 * synth-kitti, 8 or fewer on 96 % of the frames).  Same records (64 sequences: 16 -> 95 k, 8 -> 102 k, 4 -> 98 k frames/s).
 * "gate_group" (default 1): frames that carry detection boxes need the brute-force matches against the previous frame and the
 * 8-point F (src/pnpmatch.cc:253-337) before pass 1's epipolar veto.  1 = in the batched entries both are computed for a group of
 * consecutive frames in one launch each, ahead of the index chain - they depend on front-end results only, not on tracker state;
 * 0 = two launches per frame inside the chain (what the frame-by-frame entry always does).  Same records.
 * "pose_flag" (default 0): 1 = one sequence's pose kernels learn that their frame has been matched from a per-frame tag the
 * index chain publishes in HBM (agent-scope stores / polls, bounded) instead of waiting on one stream event per group of
 * frames - the pose chain then never stands still because a LATER frame of its group is slow to match (+0.6 % on the
 * headline run).  Same records.  Off by default because the poll relies on the index kernel running concurrently with the
 * polling kernel: under a tool that serialises dispatches (rocprofv3 --kernel-trace) every poll runs into its time-out.
 * "epnp_exact" (default 2): which EPnP solves the RANSAC samples of cv::solvePnPRansac (src/pnpmatch.cc:227).
 *   2 = order-preserving wave solver (csrc/svo_epnp_ord_dev.h): every IEEE operation of OpenCV 3.2's loops (epnp.cpp,
 *       JacobiSVDImpl_ / SVBkSbImpl_ of lapack.cpp: cyclic one-sided Jacobi SVDs, SVD / QR least squares, IEEE division and
 *       square root, no FMA contraction, every sum in its own k order) is kept; independent operations are spread over one
 *       wavefront per sample (Jacobi pairs on disjoint rows side by side, k-ordered sums on v_mfma_f64_4x4x4).  Bit-identical,
 *       sample by sample, to the CPU restatement the tests compare with; the rare branches it does not reproduce (a zero or
 *       repeated singular value, 25 sweeps without convergence) are handed to the sequential solver of mode 1.
 *   1 (and, as in ABI 3, every non-zero value other than 2) = the same operations, one lane per sample, loop by loop
 *       (csrc/svo_epnp_exact_dev.h): the checker of mode 2, 7.5x slower.
 *   0 = statistical wave solver (csrc/svo_epnp_dev.h; the default up to round 3): parallel-order two-sided Jacobi, normal
 *       equations, FMA - the same estimator with another rounding; 1.65x faster than mode 2, RANSAC's winner differs from a
 *       CPU run on ~3 % of the frames.
 * "tail_fused" (default 1): one sequence, default solver, no dense stage beside the tail: the frame's RANSAC samples and its frame
 *   part (RANSAC's rule, PoseOptimization, the new map points' positions, the record) run as ONE launch (k_tp_tail_ord: 100
 *   sample workgroups + the frame's workgroup, which waits for their agent-scope results) instead of two - the launch boundary
 *   and the frame part's start-up leave the pose chain's critical path (8.74 k -> 8.9-9.0 k frames/s; 9.1-9.2 k with the frame part waiting for the first 8 samples only and the
 *   context's streams on four dispatch pipes).  Same records.
 * "tail_semi" (default 1): beside a dense stage (depth_source 1 / 2, one sequence) the frame's first 8 RANSAC samples are one launch,
 *   the other 92 and the frame part a second one (k_tp_hyp_ord_first + k_tp_tail_ord): a sample workgroup of the second launch
 *   replays cv::solvePnPRansac's iteration bound over the first 8 (beyond sample 16: waits for samples 8..15, replays over 16) and
 *   leaves when the loop can never reach it - 8 CUs' float64 pipelines per ordinary frame instead of 100 taken from the dense
 *   kernels, still two launches per frame (configs[4]: 6.1-6.5 k -> 6.4-6.6 k frames/s at 256 frames per call).  2 = also with
 *   eight or more sequences per step (measured slower: 99.5 k instead of 100.9 k pairs/s; a switch).  0 = off.  Same records.
 * "epnp_force_seq" (default 0, tests): 1 = mode 2 takes its sequential fallback for every sample. */
int svo_set_option(svo_ctx* ctx, const char* key, int value);
/* Block until everything enqueued on the ctx stream has finished. */
int svo_sync(svo_ctx* ctx);
/* The ctx's hipStream_t as an opaque pointer (for event timing by the caller). */
void* svo_stream(svo_ctx* ctx);

/* ---- geometry the ctx derived from (W,H) ---------------------------------- */

/* Pyramid level sizes / scale factors / per-level keypoint quotas, 8 levels.
 * (cv::ORB defaults, src/frame.cc:77: nfeatures 500, scaleFactor 1.2, nlevels 8.) */
int svo_orb_geometry(const svo_ctx* ctx, int32_t w[8], int32_t h[8], float scale[8],
                     int32_t quota[8]);

/* ---- a-2: frame::featuredetect (src/frame.cc:75-79) ------------------------ */

/* ORB keypoints + descriptors of ONE image.  kp: capacity max_kp; desc: max_kp*32
 * bytes; *n receives the count.  Order: octave ascending, then Harris response
 * descending (ties: raster order). */
int svo_orb_extract(svo_ctx* ctx, const uint8_t* gray, int stride, svo_kp* kp,
                    uint8_t* desc, int32_t* n);

/* Stage probes used by the parity tests (same kernels as svo_orb_extract):
 * copy out pyramid level `level` of the last extracted image (tight rows). */
int svo_debug_pyramid_level(svo_ctx* ctx, int image_slot, int level, uint8_t* out);
/* FAST corners (after 3x3 NMS and the 31-px border filter) of `level` of the last
 * extracted image: xy_score receives n x 3 int32 {x, y, score}, UNORDERED. */
int svo_debug_fast_corners(svo_ctx* ctx, int image_slot, int level, int32_t* xy_score,
                           int capacity, int32_t* n);

/* ---- a-3/a-4: stereo association + depth ----------------------------------- */
/* Replaces frame::MB + frame::computekeypoint_r + frame::disp2Depth
 * (src/Tracking.cc:226-228, src/frame.cc:82-91,122-164) with the sparse epipolar
 * matcher the north star asks for.  Extracts ORB on both images, then for each
 * LEFT keypoint: row-band candidates on the right, Hamming argmin, 11x11 SAD
 * refinement +-5 px at the keypoint's pyramid level, parabola sub-pixel,
 * median-based outlier cut.  uR[i] / depth[i] = -1 where no match
 * (depth = bf / disparity, like disp2Depth). */
int svo_stereo_frame(svo_ctx* ctx, const uint8_t* grayL, int strideL, const uint8_t* grayR,
                     int strideR, const svo_camera* cam, svo_kp* kpL, uint8_t* descL,
                     int32_t* nL, float* uR, float* depth);
/* Also return the right image's keypoints (parity tests). kpR/descR may be NULL. */
int svo_stereo_frame_ex(svo_ctx* ctx, const uint8_t* grayL, int strideL, const uint8_t* grayR,
                        int strideR, const svo_camera* cam, svo_kp* kpL, uint8_t* descL,
                        int32_t* nL, float* uR, float* depth, svo_kp* kpR, uint8_t* descR,
                        int32_t* nR);

/* Parity probe of the matcher alone (same kernels as svo_stereo_frame): uploads the pair and builds the context's own
 * pyramids as svo_stereo_frame_ex does, then replaces the keypoints, descriptors and counts of both images with the
 * caller's (kpL / descL: nL entries, kpR / descR: nR entries, 32 bytes per descriptor; only x, y and octave are read)
 * and runs the matcher on them.  uR, depth, sad: max_kp entries each.  sad[i] is the best SAD of left keypoint i BEFORE
 * the median cut, -1 where the matcher did not accept it (the cut turns uR / depth to -1 and leaves sad); entries
 * >= nL are -1 in all three.  SVO_E_INVALID: nL or nR outside 0 .. max_kp, an octave outside 0 .. 7, a non-finite x or
 * y, y outside [0, H), x outside [-W, 2W] (x < 0 is legal: such a left keypoint has no candidate).  The keypoints may
 * sit anywhere else - at a level's border, where the matcher must reject them, included. */
int svo_debug_stereo_match(svo_ctx* ctx, const uint8_t* grayL, int strideL, const uint8_t* grayR, int strideR,
                           const svo_camera* cam, const svo_kp* kpL, const uint8_t* descL, int nL, const svo_kp* kpR,
                           const uint8_t* descR, int nR, float* uR, float* depth, int32_t* sad);

/* frame::disp2Depth (src/frame.cc:140-164): depth = bf/disp where disp != 0, else
 * -1, over a dense H x W float map. */
int svo_disp2depth(svo_ctx* ctx, const float* disp, int count, float bf, float* depth);
/* frame::UnprojectStereo (src/frame.cc:166-180) for n (u,v,z) triples with pose
 * Rwc (row-major 3x3) / twc: out n x 3 floats; rows with z <= 0 are left NaN. */
int svo_unproject(svo_ctx* ctx, const float* uvz, int n, const svo_camera* cam,
                  const float Rwc[9], const float twc[3], float* xyz);

/* ---- a-7/a-8/a-9: Hamming matching (src/pnpmatch.cc:14-30,61-199) ----------- */

/* pnpmatch::DescriptorDistance for `count` pairs: a,b are count x 32 bytes. */
int svo_descriptor_distance(svo_ctx* ctx, const uint8_t* a, const uint8_t* b, int count,
                            int32_t* dist);

/* Independent-row argmin: for each query row i (M x 32) scan train rows j (N x 32)
 * in index order skipping t_mask[j] != 0, with the reference's update rule
 * `if (d < best) { second = best; best = d; idx = j; }` (src/pnpmatch.cc:89-94):
 * best/second start at 256, idx at -1, ties go to the lowest j, and `second` is
 * the running best just before the last improvement - NOT the true runner-up. */
int svo_hamming_argmin(svo_ctx* ctx, const uint8_t* q, int M, const uint8_t* t, int N,
                       const uint8_t* t_mask, int32_t* best_idx, int32_t* best,
                       int32_t* second);

/* The reference's greedy, order-dependent assignment (src/pnpmatch.cc:61-156 pass 1
 * with max_dist = 15, ratio = 0; :159-199 pass 2 with max_dist = 30, ratio = 2):
 * rows are visited in index order; row i is skipped if q_skip[i] != 0; an accepted
 * row claims train column best_idx (assigned[] is updated in place), so later rows
 * cannot take it.  Accept rule: best < max_dist && (ratio <= 0 ||
 * (float)second/(float)best > ratio).  Outputs per row: best_idx (or -1), best,
 * second, accepted (0/1).  `assigned` is N bytes in/out. */
int svo_match_greedy(svo_ctx* ctx, const uint8_t* q, const uint8_t* q_skip, int M,
                     const uint8_t* t, int N, uint8_t* assigned, int max_dist, float ratio,
                     int32_t* best_idx, int32_t* best, int32_t* second, uint8_t* accepted);

/* svo_match_greedy with the reference's semantic veto of pass 1 (src/pnpmatch.cc:101-144): a row
 * that would be accepted, whose matched train point t_xy[best_idx] lies inside a detection box
 * padded by 10 px and more than 0.1 px off the line F*[q_xy[i],1], is NOT accepted, claims no
 * column, and is reported in vetoed[i] (the caller marks its map point bad).  q_xy: M x 2 floats
 * (last-frame point of each row), t_xy: N x 2 floats, boxes: n_boxes x {left,right,top,bottom}. */
int svo_match_greedy_gated(svo_ctx* ctx, const uint8_t* q, const uint8_t* q_skip, int M,
                           const uint8_t* t, int N, uint8_t* assigned, int max_dist, float ratio,
                           const float* q_xy, const float* t_xy, const int32_t* boxes, int n_boxes,
                           const double F[9], int32_t* best_idx, int32_t* best, int32_t* second,
                           uint8_t* accepted, uint8_t* vetoed);

/* a-6: cv BruteForce-Hamming match() as used by find_feature_matches
 * (src/pnpmatch.cc:253-300): nearest train row per query row (ties: lowest j),
 * then keep[i] = dist[i] <= max(2*min_dist, 30). */
int svo_bf_match(svo_ctx* ctx, const uint8_t* q, int M, const uint8_t* t, int N,
                 int32_t* train_idx, int32_t* dist, uint8_t* keep);

/* a-6: cv::findFundamentalMat(cur_pts, last_pts, CV_FM_8POINT) (src/pnpmatch.cc:336): normalised
 * 8-point algorithm in float64 on the device (one wavefront: normal matrix by wave reductions, wave-parallel Jacobi
 * eigen-solver, rank-2 projection).  pts1 / pts2: n x 2 (HOST arrays, n <= 512); F row-major with p2^T F p1 = 0,
 * scaled to F[8] = 1.  n < 8 -> F = 0 (OpenCV returns an empty matrix). */
int svo_fundamental_8point(svo_ctx* ctx, const double* pts1, const double* pts2, int n, double F[9]);

/* ---- a-10: PnP-RANSAC initial pose (src/pnpmatch.cc:212-247) ---------------- */
/* cv::solvePnPRansac(pts3d, pts2d, K, Mat(), rvec, tvec, false, 100, 8.0, 0.99, inliers) as OpenCV 3.2 runs it (the
 * version the reference links): NO extrinsic guess - every RANSAC sample is five correspondences
 * drawn by cv::RNG((uint64)-1) and solved by EPnP alone; squared reprojection error <= 8^2 (evaluated in float) counts
 * an inlier; a sample replaces the best one iff its consensus is larger, and the iteration bound then drops to
 * log(1 - 0.99) / log(1 - w^5) for inlier ratio w; the pose returned is the winning sample's (3.2 discards the refit it
 * computes on the inliers).  Xw n x 3, obs n x 2 (doubles holding the reference's float values), n <= 512;
 * K = {fx,fy,cx,cy}; T_cw row-major 4x4.  T_fallback_cw is what T_cw receives when OpenCV would return false (the
 * reference would carry on with unset rvec / tvec there).  rng_state: 0 = OpenCV's (uint64)-1.  inlier_mask: n bytes
 * (may be NULL).  All 100 samples are solved at once, one wavefront each (csrc/svo_epnp_dev.h). */
int svo_pnp_ransac(svo_ctx* ctx, const double* Xw, const double* obs, int n, const double K[4],
                   const double T_fallback_cw[16], uint64_t rng_state, double T_cw[16],
                   uint8_t* inlier_mask, svo_pnp_stats* stats);

/* Parity probe: the EPnP solve of ONE five-point sample (what every RANSAC sample of svo_pnp_ransac runs): R row-major,
 * t, and (optionally) the mean reprojection errors of the three beta candidates N = 1, 2, 3 (epnp.cpp compute_pose). */
int svo_debug_epnp5(svo_ctx* ctx, const double Xw5[15], const double uv5[10], const double K[4], double R[9],
                    double t[3], double rep_err[3]);

/* Parity probe: epnp::gauss_newton (five steps, each one epnp::qr_solve on the 6 x 4 system) of that solve alone, as one
 * wave runs it - the three beta candidates side by side.  L 6 x 10 row-major, rho[6], betas_in / betas_out 3 x 4. */
int svo_debug_epnp_gn(svo_ctx* ctx, const double L[60], const double rho[6], const double betas_in[12],
                      double betas_out[12]);

/* Parity probe: the 12 x 12 one-sided Jacobi sweeps of that solve alone (JacobiSVDImpl_ on temp_a = (M^T M)^T, without the sort), as
 * ONE wave runs them.  At 12 x 12 row-major.  rows_out: 12 rows of 16 doubles - the rotated row scaled by 1 / W in columns 0 .. 11,
 * W = sqrt(sum_k At[i][k]^2) in column 15.  steps: steps of the wave's schedule the loop ran (prologue + one period per sweep).
 * flag: 1 = it ran out of sweeps (25); the solver then redoes the sweeps in full IEEE arithmetic, as it does when a W leaves
 * [2^-100, 2^100] - inside that range the rows are JacobiSVDImpl_'s bit for bit. */
int svo_debug_jacobi12(svo_ctx* ctx, const double At[144], double rows_out[12 * 16], int32_t* steps, int32_t* flag);

/* Parity probe of RANSACPointSetRegistrator::run's sequential rule - which sample wins, how many are visited - in every form
 * the library runs its one walker in: the plain rule of svo_pnp_ransac and the tracker's variants that work from precomputed pow /
 * log terms, on the first m samples only, or report the iteration bound after m samples.  Two modes:
 *   SVO_PNP_RULE_TABLE  count = the number of points n (5 .. 512); cnt, ok, n unused (NULL).  For every consensus g = 5 .. n:
 *                       out_f64[g] = log(1 - (g / n)^5) as tabulated per frame (1.0: "denominator below DBL_MIN", the bound is 0),
 *                       out_i32[g] = rint(log(0.01) / that), out_i32[n + 1 + g] = RANSACUpdateNumIters(0.99, (n - g) / n, 5, 100);
 *                       entries below g = 5 are 0; out_f64[n + 1] = log(0.01).  out_f64: n + 2 doubles, out_i32: 2 (n + 1) ints.
 *   SVO_PNP_RULE_CASES  count cases (1 .. 4096), one thread each: cnt / ok = count x 100 (each sample's consensus and whether
 *                       it gave a model), n = count point numbers (5 .. 512); out_f64 unused.  out_i32: SVO_PNP_RULE_W ints per case:
 *                       {best, good, iters} of the plain rule; the same from precomputed terms; then for m = 0 .. 100
 *                       {samples visited within the first m or m + 1, the same from the walk that also yields the winner, its
 *                       winner, its consensus (-2 where the walk did not end within m), the iteration bound after m samples}. */
#define SVO_PNP_RULE_TABLE 0
#define SVO_PNP_RULE_CASES 1
#define SVO_PNP_RULE_W (6 + 5 * 101)
int svo_debug_pnp_rule(svo_ctx* ctx, int mode, int count, const int32_t* cnt, const int32_t* ok, const int32_t* n,
                       double* out_f64, int32_t* out_i32);

/* Parity probe of a RANSAC sample's consensus count: one wavefront counts the inliers of the model (R row-major, t) over the
 * n (1 .. 512) correspondences exactly as every sample of svo_pnp_ransac does (projection in double, rounded once to float,
 * squared distance in float <= 64).  flags: n bytes, 1 = inlier. */
int svo_debug_pnp_consensus(svo_ctx* ctx, const double* Xw, const double* obs, int n, const double K[4], const double R[9],
                            const double t[3], int32_t* count, uint8_t* flags);

/* ---- a-5: Optimizer::PoseOptimization (src/Optimizer.cc:15-86) -------------- */
/* Pose-only Levenberg-Marquardt exactly as g2o runs it for this graph: one SE3
 * vertex, n unary EdgeSE3ProjectXYZOnlyPose edges, information I2, Huber
 * delta = (double)(float)sqrt(5.991), optimize(10).  float64 throughout.
 * T_cw is in/out (row-major 4x4). */
int svo_pose_opt(svo_ctx* ctx, const double* Xw, const double* obs, int n, const double K[4],
                 double T_cw[16], svo_lm_stats* stats);

/* ---- Tracking::Track (src/Tracking.cc:180-252), device-resident ------------- */
/* Reset the tracker state held in HBM (lastframe, LocalMapPoints, frame_num). */
int svo_track_reset(svo_ctx* ctx, const svo_camera* cam);
/* Track one stereo pair given as HOST gray images; fills *res. Boxes: n_boxes (<= 64) x 4
 * int32 {left,right,top,bottom} (offline detections, main.cpp:82-95), may be NULL.  With boxes
 * the frame is gated as in the reference: no map points are created inside a box padded by 5 px,
 * and a pass-1 match that lands in a box padded by 10 px and lies > 0.1 px off the epipolar line
 * marks its map point bad (src/pnpmatch.cc:101-144). */
int svo_track_frame(svo_ctx* ctx, const uint8_t* grayL, int strideL, const uint8_t* grayR,
                    int strideR, double timestamp, const int32_t* boxes, int n_boxes,
                    svo_track_result* res);

/* Parity probe: map-point pool row matched to each keypoint of the frame just tracked
 * (CurrentFrame->MapPoints after both passes, -1 = none). cur_mp: max_kp int32. */
int svo_debug_track_matches(svo_ctx* ctx, int32_t* cur_mp);
/* Parity probe: the F matrix and the number of epipolar vetoes of the frame just tracked. */
int svo_debug_track_gate(svo_ctx* ctx, double F[9], int32_t* n_vetoed);
/* Parity probe: map-point identities, RANSAC outcome and PnP pose of `n` frames of the LAST device-resident call
 * (svo_track_batch_dev / _tail_dev / _sharded_dev: frames first .. first + n - 1 of that call; svo_track_multi_step_dev:
 * sequences first ..; svo_track_frame: first = 0, n = 1).  Synchronises. */
int svo_debug_track_frames(svo_ctx* ctx, int first, int n, svo_track_debug* out);

/* Parity probe (ABI-7 addition): the keypoints of frame `frame` of the LAST call of a tracker entry with depth_source 1, 2 or
 * 3 (svo_track_frame[_bgr]: frame 0; svo_track_batch_[bgr_]dev / _host: frames 0 .. B - 1) and the depth the dense map gave
 * each of them: bf / disp at the truncated keypoint position, -1 where disp is 0 (src/frame.cc:122-164; an invalid SGBM pixel
 * is disp = -1, so -bf).  kp, depth: max_kp entries each, *n the frame's keypoint count.  Synchronises the device. */
int svo_debug_track_depths(svo_ctx* ctx, int frame, svo_kp* kp, float* depth, int32_t* n);

/* Parity probe: cv::solvePnPRansac's outcome for the frame just tracked, and the pose (row-major 4x4, before the CV_32F
 * rounding of SetPose) it handed to PoseOptimization.  Either pointer may be NULL. */
int svo_debug_track_pnp(svo_ctx* ctx, svo_pnp_stats* stats, double T_pnp[16]);

/* ---- throughput mode: batched, device-resident ------------------------------ */
/* B stereo pairs already in HBM: d_grayL/d_grayR are B images of H rows x `stride`
 * bytes.  Runs extraction on all 2B images and the sparse stereo association for
 * the B pairs in a handful of launches on the ctx stream; does NOT synchronise.
 * Outputs (device pointers, capacity B*max_kp each): d_kpL, d_descL (x32), d_nL (B),
 * d_uR, d_depth.  Any output pointer may be NULL to keep results inside the ctx. */
int svo_frontend_batch_dev(svo_ctx* ctx, const uint8_t* d_grayL, const uint8_t* d_grayR,
                           int stride, int B, const svo_camera* cam, svo_kp* d_kpL,
                           uint8_t* d_descL, int32_t* d_nL, float* d_uR, float* d_depth);
/* Batched front end followed by the ordered tracking tail for the same B pairs
 * (frames are consecutive frames of ONE sequence, in order).  boxes (may be NULL): the frames' offline detection
 * boxes in HBM, gating the chain exactly as svo_track_frame's host boxes do (creation gates, F from brute-force
 * matches by the 8-point algorithm, epipolar veto - all on the device).  d_results: B
 * svo_track_result records in HBM.  Does not synchronise.  Consecutive calls overlap: the front end's outputs and the
 * index chain's hand-over records exist twice and alternate, so the first sub-batches and the matching of call c + 1 run
 * while the pose chain of call c is still busy.  Contract: the calls that continue one sequence are issued back to back
 * on this context; svo_sync it before any OTHER entry point uses the context in between (svo_track_reset synchronises itself). */
int svo_track_batch_dev(svo_ctx* ctx, const uint8_t* d_grayL, const uint8_t* d_grayR,
                        int stride, int B, const svo_boxes_dev* boxes, svo_track_result* d_results);

/* The ordered tracking tail ALONE, for front-end results that already lie in HBM - e.g. produced by
 * svo_frontend_batch_dev of OTHER contexts / GPUs and copied here (pair k -> GPU k mod G, then the
 * strict chain of src/Tracking.cc:231-250 in frame order on one GPU).  Frame f of the call: keypoints at
 * d_kp + f * kp_stride, descriptors at d_desc + f * kp_stride * 32, keypoint count d_n[f], per-keypoint depths
 * (<= 0: none) at d_depth + f * kp_stride.  boxes (may be NULL): frame f's detection boxes.  Records are identical to
 * svo_track_batch_dev on the same frames.  Does not synchronise. */
int svo_track_tail_dev(svo_ctx* ctx, const svo_kp* d_kp, const uint8_t* d_desc, const int32_t* d_n,
                       const float* d_depth, int kp_stride, int B, const svo_boxes_dev* boxes,
                       svo_track_result* d_results);
/* ONE sequence tracked with G contexts in one process, typically one per GPU (BASELINE configs[3]
 * "pair k -> GPU k mod 8 ... ordered tail"): the stateless front end of stereo pair k runs on ctxs[k mod G], the strict
 * temporal chain of src/Tracking.cc:231-250 runs in frame order on ctxs[0], which pulls each frame's keypoints /
 * descriptors / depths (~34 KB) on its own stream - direct peer reads (hipMemcpyPeerAsync over xGMI) where
 * hipDeviceCanAccessPeer says so, a bounce through pinned host memory otherwise; no collective.
 * d_grayL[g] / d_grayR[g]: the pairs of context g, resident on ITS device, k ascending (pair k at local index k / G),
 * `stride` bytes per row.  All contexts: same W, H, max_kp; ctxs[g] needs max_batch >= ceil(B / G).  svo_track_reset on
 * ctxs[0] first; B frames per call; d_results: B records on ctxs[0]'s device.  Records are identical to
 * svo_track_batch_dev on a single context.  boxes (may be NULL): frame k's detection boxes, on ctxs[0]'s device.
 * Does not synchronise (svo_sync(ctxs[0]) does), and consecutive calls overlap: a call's front ends run in sub-batches on
 * streams other than the pose chain's, a gather stream on ctxs[0]'s device collects them into one of two staging sets, and
 * the front ends of the next call run while this call's tail is in flight (two contexts on one GPU: the tail's own period,
 * 115 us per frame).  The images, boxes and result records of a call must stay valid until svo_sync(ctxs[0]); any other
 * entry point of one of the contexts first waits for what these calls left in flight. */
int svo_track_sharded_dev(svo_ctx* const* ctxs, int G, const uint8_t* const* d_grayL, const uint8_t* const* d_grayR,
                          int stride, int B, const svo_boxes_dev* boxes, svo_track_result* d_results);
/* ---- throughput mode, HOST-fed and pipelined (main.cpp:159-195: the reference reads one stereo pair from disk per
 * Tracking::Track; SURVEY.md section 8e: "H2D 2 P bytes, D2H ~30 KB" per pair, pair k uploaded to GPU k mod G) ------------
 * svo_track_batch_host = svo_track_batch_dev for B consecutive frames of ONE sequence that start in HOST memory: grayL / grayR
 * are B images of H rows x `stride` bytes each, back to back (frame f at grayL + f * H * stride); `results`: B records in host
 * memory.  The call does not synchronise: the images are uploaded on a copy stream of the context's own, eight pairs per
 * event, and every front-end sub-batch waits only for its own pairs; the records are copied back behind the pose chain.
 * Pinned source images (hipHostMalloc / hipHostRegister, e.g. torch's pin_memory) are copied where they lie and must stay
 * valid until svo_sync or until the second following host-fed call on this context returns; pageable images are first
 * gathered into a pinned ring by up to four worker threads inside the call (the call returns when they are staged - they
 * may be reused at once).  `results` is complete after svo_sync(ctx) (pageable: copied out of a pinned buffer there), or after the
 * second following host-fed call returned.  Both "second following call" rules hold for pinned and pageable memory alike and
 * across kinds (svo_track_batch_host, svo_track_batch_bgr_host, svo_frontend_batch_host on one context share two image sets):
 * a host-fed call first waits for what the call two back left on the set it reuses - its uploads and its outputs, normally
 * long done.  Consecutive calls overlap exactly like svo_track_batch_dev's (two image sets
 * alternate): the uploads of call c + 1 run while the tail of call c is busy.  Records are byte-identical to
 * svo_track_batch_dev's on the same frames.  boxes (may be NULL): the frames' offline detection boxes, host arrays.
 * Works with every "depth_source" (the dense stages wait for the call's last upload instead of sub-batch by sub-batch).
 * Contract as for svo_track_batch_dev: the calls that continue one sequence are issued back to back; svo_sync before any
 * other entry point uses the context. */
int svo_track_batch_host(svo_ctx* ctx, const uint8_t* grayL, const uint8_t* grayR, int stride, int B,
                         const svo_boxes_host* boxes, svo_track_result* results);
/* svo_track_sharded_dev for a sequence that starts in HOST memory - BASELINE configs[3] as SURVEY.md section 8e words it:
 * stereo pair k is uploaded to the GPU of ctxs[k mod G] on THAT context's copy stream (each GPU pulls only its own pairs
 * over its own PCIe link), its front end runs there, the ordered tail on ctxs[0].  grayL / grayR: the B frames of the call in
 * frame order (frame k at grayL + k * H * stride); results: B records in host memory, complete after svo_sync(ctxs[0]).
 * Everything else as svo_track_sharded_dev / svo_track_batch_host; records identical to both. */
int svo_track_sharded_host(svo_ctx* const* ctxs, int G, const uint8_t* grayL, const uint8_t* grayR, int stride, int B,
                           const svo_boxes_host* boxes, svo_track_result* results);
/* The stateless front end alone (svo_frontend_batch_dev), host to host and pipelined the same way.  Output arrays (host
 * pointers, capacity B * max_kp each, d_nL: B; any may be NULL) are complete after svo_sync(ctx) or after the second
 * following call returned.  Its rate is what the PCIe link delivers (0.93 MB per 1241x376 pair). */
int svo_frontend_batch_host(svo_ctx* ctx, const uint8_t* grayL, const uint8_t* grayR, int stride, int B,
                            const svo_camera* cam, svo_kp* kpL, uint8_t* descL, int32_t* nL, float* uR, float* depth);

/* ---- colour input (main.cpp:160-161: KITTI image_2 / image_3 read with CV_LOAD_IMAGE_UNCHANGED, 8UC3 BGR) ----------------
 * The reference's tracker consumes colour in two places: cv::ORB reduces it to gray (COLOR_BGR2GRAY, src/frame.cc:75-79), and
 * frame::MB hands it to MSA::solve (src/frame.cc:82-91), whose cost, 3x3 median and tree weights use the three channels.  The
 * entries below take colour pairs and convert them ON THE DEVICE with cv::cvtColor(COLOR_BGR2GRAY)'s fixed point for 8U,
 * gray = (1868 B + 9617 G + 4899 R + 8192) >> 14 (B = G = R = v gives v); from that gray on, ORB, the sparse matcher and ELAS
 * (depth_source 0 / 1) run exactly as in their gray counterparts - ELAS on gray is the only definition there is, the reference
 * never calls libelas.  With depth_source 2 MSA gets the true colour pair (the gray entries give it B = G = R copies of the
 * gray), and computes its own 0.299 / 0.587 / 0.114 gray from it, as the reference does.  Argument checks, contracts and overlap
 * rules are those of the gray counterparts, with stride >= 3 * W; gray and colour calls may follow each other within one
 * sequence, each frame's record being what its own pixels imply.  A context allocates its colour staging on the first colour
 * call.  The many-sequence mode has svo_track_multi_step_bgr_dev (below, with svo_track_multi_step_dev); svo_track_sharded_* and
 * svo_frontend_batch_* stay gray-only. */

/* BGR -> gray with cv::cvtColor(COLOR_BGR2GRAY)'s fixed-point weights; host buffers in and out (any width x height, rows
 * bgr_stride >= 3 * width and gray_stride >= width bytes apart).  Synchronises. */
int svo_bgr_to_gray(svo_ctx* ctx, const uint8_t* bgr, int width, int height, int bgr_stride, uint8_t* gray, int gray_stride);
/* svo_track_frame for 8UC3 BGR host images (main.cpp:160-161). */
int svo_track_frame_bgr(svo_ctx* ctx, const uint8_t* bgrL, int strideL, const uint8_t* bgrR, int strideR, double timestamp,
                        const int32_t* boxes, int n_boxes, svo_track_result* res);
/* svo_track_batch_dev for B BGR pairs in HBM (pair b at d_bgrL + b * H * stride), stride >= 3 * W.  The gray of each front-end
 * sub-batch is written just before it, on the front end's stream, into staging of the context's own (max_batch pairs). */
int svo_track_batch_bgr_dev(svo_ctx* ctx, const uint8_t* d_bgrL, const uint8_t* d_bgrR, int stride, int B,
                            const svo_boxes_dev* boxes, svo_track_result* d_results);
/* svo_track_batch_host for B BGR pairs in host memory (pinned or pageable), same contract.  Each upload chunk of eight pairs is
 * converted on the copy stream before its event, so a front-end sub-batch still waits for its own pairs only. */
int svo_track_batch_bgr_host(svo_ctx* ctx, const uint8_t* bgrL, const uint8_t* bgrR, int stride, int B,
                             const svo_boxes_host* boxes, svo_track_result* results);

/* Sticky flag of the device tracker (synchronises), a bit set OR-ed over the sequences and cleared by svo_track_reset /
 * svo_track_multi_reset: both bits may be set.  4: see SVO_E_TIMEOUT.  1: capacity - *flag != 0 once a frame needed more than the 4096 live
 * map points the pool holds, or a map point stayed alive for more than 2^20 creations (its slot in the position table
 * was about to be reused).  Neither can happen with the reference's 500 keypoints per frame on sequences of KITTI
 * length; results after the flag is set are not the reference's. */
int svo_track_overflowed(svo_ctx* ctx, int32_t* flag);
/* Diagnostics of the default RANSAC solver (svo_set_option "epnp_exact" = 2; cv::solvePnPRansac of src/pnpmatch.cc:227):
 * how many samples since svo_track_reset took its sequential fallback (a zero or repeated singular value in one of EPnP's
 * decompositions, or 25 Jacobi sweeps without convergence).  Results are the same either way; a frame with such a sample
 * takes about ten times as long in the pose chain.  Synchronises. */
int svo_track_epnp_fallbacks(svo_ctx* ctx, int64_t* count);

/* Diagnostics: how the stream of the tail's index chain was chosen.  The ordered tail (src/Tracking.cc:231-250 per frame) runs
 * as two chains on two streams that must overlap.  The HIP runtime maps a process's streams onto a few hardware queues per
 * priority (4 by default, least-used first), and two streams on ONE queue run one after the other: with three older
 * high-priority streams alive in the process the first two new ones share a queue, and the tracker ran at 5.9 k instead of
 * 8.8 k frames/s (tools/queue_history.py, profiles/r05_queue_pairs.jsonl).  Every stream of a context that has to run beside
 * another one is therefore PICKED BY MEASURING (svo_pick_stream): a chain of eight short dependent kernels on the existing
 * stream alone, then the same chain on both streams together; up to six candidates, the first whose ratio is below 150 % is
 * kept.  out[0] = candidates tried for the index chain's stream (0: probe off, SVO_NO_STREAM_PROBE=1; -1: no tracker call
 * yet), out[1] = "two chains together / one alone" of the chosen one, per cent (~105: side by side; ~200: serialised - then
 * svo_last_error says so). */
int svo_debug_stream_probe(svo_ctx* ctx, int32_t out[2]);

/* Diagnostics: do the large grids of the batched front end hold the ordered tail up?  gfx950 places a process's hardware queues on
 * the command processor's four dispatch pipes in creation order (position among the live queues modulo 4), and a queue whose
 * launches wait behind each other holds up the other queues of its pipe: with the front end's queue on the pose chain's pipe
 * the tracker ran at half its rate (tools/microbench/queue_block_probe, queue_prio_probe; profiles/r05_queue_block.jsonl).  A
 * context therefore makes its four main streams (pose chain, index chain, batched front end, dense stage) as four queues of
 * its own back to back - four different pipes, whatever the process did before or does elsewhere later.  This call MEASURES it
 * (about 10 ms, everything of the context synchronised first): a 3,072 x 64-thread grid on the pose stream (out[0]) and on the
 * index stream (out[1]) alone, then beside four queued launches of slot-filling grids on the front end's stream; reported as
 * 100 + 100 x (delay in rounds of the filling grids' workgroups): ~100 clear, ~180 sharing CUs only, >= 330 held up behind the pipe.
 * out[2], out[3]: the same with the dense stage's stream filling.  -1: that stream does not exist (yet). */
int svo_debug_stream_pipes(svo_ctx* ctx, int32_t out[4]);

/* Many independent sequences on one GPU ("G independent sequences" for pure
 * throughput; no counterpart in the reference, whose tracker is one static chain per process,
 * src/Tracking.cc:180-252).  svo_track_multi_reset allocates n_seq (<= max_batch) tracker states;
 * every svo_track_multi_step_dev advances ALL of them by one frame: stereo pair q (device-resident,
 * `stride` bytes per row, pairs back to back) is the next frame of sequence q, d_results[q] its record.
 * The front end runs batched over the n_seq pairs and every kernel of the temporal tail runs one
 * workgroup per sequence, so the strictly serial chain of one sequence overlaps with the others'.
 * Results are identical to n_seq separate single-sequence trackers.  boxes (may be NULL): entry q = the detection boxes
 * of sequence q's frame of this step.  Both entries want "depth_source" 0.
 * Image lifetime: a step's images are read by work the step enqueues and must stay unchanged until that work is done - until
 * svo_sync(ctx), or until work the caller orders behind svo_stream(ctx) after the step returned runs.  That rule is the same with
 * and without the dynamic-keypoint loop (whose copy of the left images is the step's last reader: the context's stream waits for
 * it) and with "multi_pipeline" 0 and 1. */
int svo_track_multi_reset(svo_ctx* ctx, int n_seq, const svo_camera* cam);
int svo_track_multi_step_dev(svo_ctx* ctx, const uint8_t* d_grayL, const uint8_t* d_grayR, int stride,
                             int n_seq, const svo_boxes_dev* boxes, svo_track_result* d_results);
/* svo_track_multi_step_dev for n_seq 8UC3 BGR pairs back to back (pair q at d_bgrL + q * H * stride), stride >= 3 * W (a backward-
 * compatible ABI-8 addition).  The gray of the 2 n_seq images is written on the device (svo_bgr_to_gray's fixed point) into the
 * context's colour staging, on the stream the step's front end runs on; from that gray on it is svo_track_multi_step_dev, records
 * byte-identical to it on that gray and to n_seq svo_track_batch_bgr_dev chains.  Gray and colour steps may alternate within a run.
 * SVO_E_INVALID for a bad stride or n_seq. */
int svo_track_multi_step_bgr_dev(svo_ctx* ctx, const uint8_t* d_bgrL, const uint8_t* d_bgrR, int stride,
                                 int n_seq, const svo_boxes_dev* boxes, svo_track_result* d_results);

/* Names + accumulated HIP-event time (ms) and launch count of the kernels the ctx
 * has timed since svo_profile_reset (only when svo_profile_enable(ctx,1)). */
int svo_profile_enable(svo_ctx* ctx, int on);
int svo_profile_reset(svo_ctx* ctx);
int svo_profile_get(svo_ctx* ctx, int index, char* name, int name_cap, double* total_ms,
                    int64_t* launches);

/* ------------------------------------------------------------------------------------------------
 * Dense ELAS stereo.  Replaces the vendored libelas,
 * Thirdparty/libelas/src/elas.h:40-165 + elas.cpp:32-150 (`Elas::process`).  Results are bit-identical
 * to the compiled reference stage by stage; see DESIGN.md section 8 for the two documented caveats
 * (duplicate right-image support points, memory libelas reads uninitialised is defined as 0).
 * ---------------------------------------------------------------------------------------------- */

/* Elas::parameters (elas.h:60-83): same fields, same order, bools as int32. */
typedef struct svo_elas_params {
  int32_t disp_min, disp_max;
  float support_threshold;
  int32_t support_texture, candidate_stepsize, incon_window_size, incon_threshold, incon_min_support;
  int32_t add_corners, grid_size;
  float beta, gamma, sigma, sradius;
  int32_t match_texture, lr_threshold;
  float speckle_sim_threshold;
  int32_t speckle_size, ipol_gap_width, filter_median, filter_adaptive_mean, postprocess_only_left;
  int32_t subsampling;              /* 1: every second pixel only; D1/D2 are then (width/2) x (height/2) */
} svo_elas_params;

/* Optional taps of every intermediate (any pointer may be NULL) and optional override of the two
 * triangle lists; used by the parity tests, which run the reference's stages on the same lists. */
typedef struct svo_elas_taps {
  uint8_t *desc1, *desc2;              /* W*H*16 each */
  int32_t* support;                    /* (u,v,d) triples */
  int32_t n_support, cap_support;
  int32_t *tri1, *tri2;                /* (c1,c2,c3) triples */
  float *planes1, *planes2;            /* (t1a,t1b,t1c,t2a,t2b,t2c) per triangle */
  int32_t n_tri1, n_tri2, cap_tri;
  int32_t *grid1, *grid2;              /* (disp_max+2)*grid_w*grid_h */
  float *D1_raw, *D2_raw, *D1_lr, *D2_lr, *D1_seg, *D2_seg, *D1_gap, *D2_gap, *D1_mean, *D2_mean;
  const int32_t *tri1_in, *tri2_in;
  int32_t n_tri1_in, n_tri2_in;
} svo_elas_taps;

/* `Elas::parameters(setting)` (elas.h:87-142): setting 0 = ROBOTICS, 1 = MIDDLEBURY. */
int svo_elas_default_params(int32_t setting, svo_elas_params* params);

/* `Elas::process(I1, I2, D1, D2, dims)` (elas.h:162, elas.cpp:32-150): dims = {width, height, bytes per
 * line}; D1/D2 are width*height floats (left / right reference), negative = invalid.  Host buffers in,
 * host buffers out (with subsampling = 1 the maps are (width/2) x (height/2), elas.h:157-160).  With fewer
 * than 3 support points it returns SVO_OK and leaves D1/D2 untouched, as the reference does (elas.cpp:70-75). */
int svo_elas_process(svo_ctx* ctx, const uint8_t* I1, const uint8_t* I2, float* D1, float* D2,
                     const int32_t* dims, const svo_elas_params* params);
int svo_elas_process_ex(svo_ctx* ctx, const uint8_t* I1, const uint8_t* I2, float* D1, float* D2,
                        const int32_t* dims, const svo_elas_params* params, svo_elas_taps* taps);

/* Throughput mode (no counterpart in the reference): B stereo pairs already in HBM (pair b at
 * d_L/d_R + b * stride * height, `stride` bytes per row), dense maps for all of them into d_D1/d_D2 (HBM,
 * pair b at + b * map size).  The small kernels of different pairs overlap on several HIP streams and the
 * two sequential host stages (support point clean-up, triangulation) run on a pool of host threads.  Results
 * are identical to B calls of svo_elas_process.  produced (host, B entries, may be NULL): 0 where a pair had
 * fewer than 3 support points and its maps were left untouched.  Synchronises before it returns. */
int svo_elas_batch_dev(svo_ctx* ctx, const uint8_t* d_L, const uint8_t* d_R, int stride, int width, int height,
                       int B, const svo_elas_params* params, float* d_D1, float* d_D2, int32_t* produced);

/* `Elas::computeDelaunayTriangulation` (elas.cpp:445-503 -> Triangle "zQB"): host-side, needs no GPU.
 * xy = n (x,y) int32 pairs; writes up to cap (c1,c2,c3) triples, counter-clockwise, in canonical order
 * (smallest index first, sorted); *n_tri = number of triangles. */
int svo_elas_delaunay(const int32_t* xy, int32_t n, int32_t* tri, int32_t cap, int32_t* n_tri);

/* ------------------------------------------------------------------------------------------------
 * MSA dense stereo: stages built so far.
 * ---------------------------------------------------------------------------------------------- */

/* `ctmf(src, dst, width, height, src_step_row, dst_step_row, r, channels, memsize)` (Thirdparty/MB/ctmf.h:7,
 * ctmf.c:222-433; called at Thirdparty/MB/MSA.cpp:58-59 with r = 1 on 3 channels and MSA.cpp:1006 with r = 2 on
 * 1 channel): per-channel (2r+1)^2 median of an 8-bit interleaved image, window clamped to the image.
 * Host buffers in and out; r in 1..3, channels in 1..4; `memsize` (a CPU cache hint) is dropped. */
int svo_ctmf(svo_ctx* ctx, const uint8_t* src, uint8_t* dst, int width, int height, int src_step_row,
             int dst_step_row, int r, int channels);

/* `MSA::init(l, r)` (Thirdparty/MB/MSA.cpp:22-63 with gradient :65-76, getCost :78-108, ctmf, gradient_after_ctmf
 * :110-139): from two 8UC3 BGR images (width x height, `step` bytes per row) the two matching-cost volumes
 * (height*width*disp floats each, disparity fastest; disp = MSA's `Disp` = d + 1, 49 in src/frame.cc:86), the
 * median-filtered colour images and the row / column gray gradients of those (float64, height*width each).
 * Host buffers in and out.  The later stages of MSA::solve are not built. */
int svo_msa_init(svo_ctx* ctx, const uint8_t* bgrL, const uint8_t* bgrR, int width, int height, int step, int disp,
                 float* costL, float* costR, uint8_t* m_img3L, uint8_t* m_img3R, double* r_graL, double* c_graL,
                 double* r_graR, double* c_graR);

/* The spanning tree MSA aggregates over, for one image: `build` -> `Tarjan` -> `getSeq0` -> `Kruskal1` -> `getSeq`
 * (MSA.cpp:152-373, 661-808, 898-926).  Host-side, needs no GPU.  m_img3 / r_gra / c_gra: outputs of svo_msa_init for that
 * image.  Outputs in the form svo_msa_tree_dp takes: seq[width*height], child_ptr[+1], child / child_c[-1], *root. */
int svo_msa_tree(const uint8_t* m_img3, const double* r_gra, const double* c_gra, int width, int height, int32_t* seq,
                 int32_t* child_ptr, int32_t* child, uint8_t* child_c, int32_t* root);

/* `MSA::TreeDp(cost)` (MSA.cpp:929-990) with `setExp(o)` (:1126-1130): two-pass aggregation of a cost volume (N nodes x
 * D disparities, float) over a spanning tree.  The tree is given as the reference holds it at that point: `seq` = its
 * BFS order from `root` (:898-926) and, per node, the children in the order its adjacency chain yields them (CSR:
 * child_ptr[N+1], child[N-1], child_c[N-1] = the edge's colour weight 0..255) - the order fixes the float rounding.
 * costA: N*D floats.  Host buffers in and out. */
int svo_msa_tree_dp(svo_ctx* ctx, const float* cost, int N, int D, const int32_t* seq, const int32_t* child_ptr,
                    const int32_t* child, const uint8_t* child_c, int root, double o, float* costA);
/* `MSA::WTA(disparity)` (MSA.cpp:992-1006): first minimum over the D disparities per pixel, then the 5x5 ctmf. */
int svo_msa_wta(svo_ctx* ctx, const float* costA, int width, int height, int D, uint8_t* disparity);
/* `MSA::LRcheck(d1, d2, cost)` (MSA.cpp:1027-1105): mask = pixels with d1 > 0 whose right-map disparity at x - d1 is
 * the same; their cost row becomes |d - d1|, every other row 0. */
int svo_msa_lrcheck(svo_ctx* ctx, const uint8_t* d1, const uint8_t* d2, int width, int height, int D, float* cost,
                    uint8_t* mask);

/* `MSA::solve(l, r, d, scale, Save)` (Thirdparty/MB/MSA.cpp:1132-1169), what `frame::MB` calls with d = 48, scale = 1
 * (src/frame.cc:82-91): dense left-reference disparity of two 8UC3 BGR images, one byte per pixel = disparity * scale.
 * The per-pixel and per-node stages run on the GPU with the cost volumes resident in HBM, the two aggregation trees are
 * built on two host threads.  No imshow / imwrite("test.png") (the reference does both on every call). */
int svo_msa_solve(svo_ctx* ctx, const uint8_t* bgrL, const uint8_t* bgrR, int width, int height, int step, int d, int scale,
                  uint8_t* disparity);

/* Throughput mode of the same solver (no counterpart in the reference): B gray stereo pairs already in HBM (pair b at
 * d_L / d_R + b * stride * height, `stride` bytes per row; a gray frame stands for the B = G = R colour image the
 * reference gets from a grayscale file), disparity maps as floats - `disp_img.convertTo(disp_32f, CV_32F, 1)` of
 * frame::MB - into d_disp (HBM, map b at + b * width * height).  Frames are solved 16 at a time: their aggregation
 * trees are built side by side on host threads and their level sweeps share launches.  Results are identical to B
 * calls of svo_msa_solve with scale 1.  Synchronises before it returns. */
int svo_msa_batch_dev(svo_ctx* ctx, const uint8_t* d_L, const uint8_t* d_R, int stride, int width, int height, int B, int d,
                      float* d_disp);

/* Diagnostics (a backward-compatible ABI-8 addition; host side only, touches no device state): how the LAST tree aggregation
 * planned on this context ran - svo_msa_tree_dp, svo_msa_solve or a chunk of svo_msa_batch_dev.  out[0] = 1: one launch per
 * aggregation (a workgroup per disparity walks the levels, level values in LDS), 0: one launch per level (the widest level or
 * the level table does not fit 150 KB of LDS, a node has more than 255 children, the sequence does not list siblings in
 * child-list order, the transposing gather's tile 64 * (D + 1) * 4 bytes exceeds 64 KB, or SVO_MSA_LEVEL_LAUNCHES is set),
 * -1: nothing planned yet.  out[1] = the widest level over the trees, out[2] = the deepest tree's number of levels, out[3] =
 * the LDS bytes the one-launch kernel needs for those two (8 * (256 + 2 * out[1]) + 4 * (out[2] + 2)), out[4] = the state of
 * its opt-in above 64 KB on this context (0 not tried, 1 granted, -1 refused). */
int svo_debug_msa_plan(svo_ctx* ctx, int32_t out[5]);

/* ---- semi-global block matching (ABI-7 additions; no existing entry changed) -----------------------------------------------
 * The reference's third dense solver: the body of frame::ElasMatch (src/frame.cc:94-120) is cv::StereoSGBM::create(0, 16, 3)
 * with a fixed parameter set, compute, convertTo(CV_32F, 1/16).  The algorithm here is OpenCV 3.2's MODE_SGBM (one pass, five
 * directions) on one 8-bit gray pair, then the disp12MaxDiff check and filterSpeckles, restated as a written contract
 * (DESIGN.md section 8 "SGBM": parity is unpinned in the sense of SURVEY section 8(c), like ORB) - all integer; the device
 * equals the numpy restatement tests/sgbm_ref.py bit for bit.  Colour callers hand these entries the gray they already make;
 * the _bgr entries below run the three-channel function the reference itself calls. */
typedef struct svo_sgbm_params {
  int32_t minDisparity;       /* 0 */
  int32_t numDisparities;     /* D: 16, 32, 48 or 64 */
  int32_t blockSize;          /* 9 */
  int32_t P1, P2;             /* 8 * 81, 32 * 81 */
  int32_t disp12MaxDiff;      /* 1 */
  int32_t preFilterCap;       /* 63 */
  int32_t uniquenessRatio;    /* 10 */
  int32_t speckleWindowSize;  /* 100 */
  int32_t speckleRange;       /* 32 */
} svo_sgbm_params;

/* ElasMatch's values for an image of `height` rows: numDisparities = ((height / 8) + 15) & -16.  Host only. */
int svo_sgbm_default_params(int height, svo_sgbm_params* params);

/* One pair, host buffers (rows `stride` bytes apart) -> the int16 map `sgbm->compute` returns (disparity * 16, -16 = invalid;
 * columns x < D are always invalid) and / or the float map disp16 / 16 (invalid = -1.0f exactly); either may be NULL.
 * Accepts numDisparities in {16, 32, 48, 64}, width > D + 8, height >= 2, every other field at its default - anything else is
 * SVO_E_INVALID; width > 3072 or height > 4096 is SVO_E_CAPACITY.  Parameters and sizes are checked first, on the host, before
 * the context or a device is touched (so a NULL ctx with an oversized image still answers SVO_E_CAPACITY).  Synchronises. */
int svo_sgbm_process(svo_ctx* ctx, const uint8_t* L, const uint8_t* R, int stride, int width, int height,
                     const svo_sgbm_params* params, int16_t* disp16, float* disp);

/* B pairs resident in HBM (pair b at d_L / d_R + b * height * stride) -> B float maps in HBM (map b at d_disp + b * width *
 * height), four pairs at a time through the context's volumes.  Identical to B calls of svo_sgbm_process.  Synchronises. */
int svo_sgbm_batch_dev(svo_ctx* ctx, const uint8_t* d_L, const uint8_t* d_R, int stride, int width, int height, int B,
                       const svo_sgbm_params* params, float* d_disp);

/* The last stage on its own, on a host map in place: cv::filterSpeckles(disp16, -16, 100, 16 * 32) - valid pixels are
 * 4-connected where they differ by at most 512, every component of at most 100 pixels becomes -16.  Synchronises. */
int svo_sgbm_filter_speckles(svo_ctx* ctx, int16_t* disp16, int width, int height);

/* Parity probe of the last svo_sgbm_process call: which = 0 the block cost C, 1 S4 (the first four directions, saturated),
 * 2 S (all five) - height x width x D int16, zero where undefined (x < D); 3 the right-image map disp2 (height x width, -1 = no
 * bid), 4 disp1 after the left-right check, before the speckle filter (height x width).  Synchronises.
 * (Also after svo_sgbm_process_bgr, whose C is the low 16 bits of the true block sum; after a batch entry: SVO_E_INVALID.) */
int svo_sgbm_debug_volume(svo_ctx* ctx, int which, int16_t* host);

/* ---- semi-global block matching on 8UC3 pairs (ABI-7 additions; no existing entry changed) ----------------------------------
 * frame::ElasMatch takes cn = leftImage.channels() and is called on the 8UC3 images main.cpp reads: P1 = 8 cn 81 = 1944,
 * P2 = 32 cn 81 = 7776, and the pixel cost is the sum over the three channels of BT(prefiltered channel) + (BT(channel) >> 2)
 * (0 .. 567).  The 9 x 9 block sum reaches 45 927 and is kept in a short as OpenCV keeps it: C is the low 16 bits of the true
 * sum, sign-extended.  Along a path the predecessor's values are read as the shorts they were stored as and its minimum as
 * the short of the unwrapped minimum; the step itself is int32 and goes unwrapped into the saturated sums S4 and S.  The
 * written contract is DESIGN.md section 8 "f-4 SGBM: colour", its executable form the numpy restatement tests/sgbm_bgr_ref.py,
 * which the device equals bit for bit; everything else (directions, winner, uniqueness, left-right check, speckles, the maps,
 * D in {16, 32, 48, 64}) is the gray contract.  Images are interleaved, rows `stride` >= 3 * width bytes apart; the channel
 * order does not matter to the result.  Width cap: 3072, as for gray (the cost stage makes one pass per channel over the
 * same 20 bytes of LDS per column); height cap 4096.  One context's arena serves gray and colour calls in turn. */

/* svo_sgbm_default_params with P1 = 1944 and P2 = 7776.  Host only. */
int svo_sgbm_default_params_bgr(int height, svo_sgbm_params* params);

/* svo_sgbm_process on two 8UC3 host images.  Accepts exactly the set svo_sgbm_default_params_bgr gives (numDisparities in
 * {16, 32, 48, 64}): gray's P1 / P2 are SVO_E_INVALID here, as this set is in the gray entries; stride < 3 * width is
 * SVO_E_INVALID; width > 3072 or height > 4096 is SVO_E_CAPACITY, answered before the context or a device is touched. */
int svo_sgbm_process_bgr(svo_ctx* ctx, const uint8_t* L, const uint8_t* R, int stride, int width, int height,
                         const svo_sgbm_params* params, int16_t* disp16, float* disp);

/* svo_sgbm_batch_dev on B resident 8UC3 pairs (pair b at d_L / d_R + b * height * stride), two pairs at a time through the
 * context's volumes (the path sums are int32 here).  Identical to B calls of svo_sgbm_process_bgr.  Synchronises. */
int svo_sgbm_batch_bgr_dev(svo_ctx* ctx, const uint8_t* d_L, const uint8_t* d_R, int stride, int width, int height, int B,
                           const svo_sgbm_params* params, float* d_disp);

/* ---- semi-global block matching: MODE_HH (ABI-7 additions; no existing entry changed) ---------------------------------------
 * cv::StereoSGBM's full eight-path mode beside MODE_SGBM; the reference sets MODE_SGBM, which stays the default everywhere.
 * Directions 0 to 4 are as above; 5, 6 and 7 have their predecessor at (+1,+1), (0,+1) and (-1,+1): OpenCV's second pass, rows
 * bottom to top and columns right to left from zeroed buffers, so the border rule (a predecessor outside the image counts as all
 * zeros with m = 0) is the same, mirrored.  sum4 = v0 + v1 + v2 + v3 and S4 = sat16(sum4) as before; sum8 = S4 + v4 + v5 + v6 + v7
 * in int32 and S = sat16(sum8): one saturation of the second pass's four steps added together.  The winner reads S; there is no
 * in-row fifth direction beyond v4.  With three channels the v are the unwrapped int32 steps and sum8 saturates on both sides.
 * Everything else is the gray or the colour contract, unchanged.  The written contract is DESIGN.md section 8 "f-4 SGBM:
 * MODE_HH" (parity with OpenCV unpinned); its executable form is tests/sgbm_hh_ref.py, which the device
 * equals bit for bit.  The two further path volumes the mode needs are allocated the first time a context is asked for it. */
enum { SVO_SGBM_MODE_SGBM = 0, SVO_SGBM_MODE_HH = 1 };   /* OpenCV's values; there is no MODE_SGBM_3WAY */

/* svo_sgbm_process, svo_sgbm_process_bgr, svo_sgbm_batch_dev and svo_sgbm_batch_bgr_dev with a mode after the parameters (those
 * four are these with SVO_SGBM_MODE_SGBM).  A mode other than the two above is SVO_E_INVALID, answered like the other argument
 * checks on the host, before the context or a device is touched.  After a svo_sgbm_process*_mode call svo_sgbm_debug_volume's
 * which = 1 is still S4 and which = 2 is S over all eight directions. */
int svo_sgbm_process_mode(svo_ctx* ctx, const uint8_t* L, const uint8_t* R, int stride, int width, int height,
                          const svo_sgbm_params* params, int mode, int16_t* disp16, float* disp);
int svo_sgbm_process_bgr_mode(svo_ctx* ctx, const uint8_t* L, const uint8_t* R, int stride, int width, int height,
                              const svo_sgbm_params* params, int mode, int16_t* disp16, float* disp);
int svo_sgbm_batch_mode_dev(svo_ctx* ctx, const uint8_t* d_L, const uint8_t* d_R, int stride, int width, int height, int B,
                            const svo_sgbm_params* params, int mode, float* d_disp);
int svo_sgbm_batch_bgr_mode_dev(svo_ctx* ctx, const uint8_t* d_L, const uint8_t* d_R, int stride, int width, int height, int B,
                                const svo_sgbm_params* params, int mode, float* d_disp);

/* ---- sparse pyramidal Lucas-Kanade (ABI-7 additions; no existing entry changed) --------------------------------------------
 * The dynamic-keypoint loop of the reference's Tracking::Track (src/Tracking.cc:189-223, commented out there): points inside
 * detection boxes followed from the last left image into the current one with cv::calcOpticalFlowPyrLK and its default
 * arguments.  The algorithm is OpenCV 3.2's, restated as a written contract (DESIGN.md section 8 "LK": parity is unpinned in
 * the sense of SURVEY section 8(c), like ORB and SGBM): on 8-bit single-channel images (svo_lk_track, svo_lk_batch_dev,
 * svo_lk_chain_dev; the device equals the numpy restatement tests/lk_ref.py bit for bit) and on 8UC3 BGR images, which is what
 * the reference's call is made on (the _bgr entries, cn = 3; tests/lk_ref.py).  Points are (x, y) float pairs and must be
 * finite. */
typedef struct svo_lk_params {
  int32_t winSize;            /* 21 (square) */
  int32_t maxLevel;           /* 0 .. 3; the level rule may stop lower (a level of width or height <= 21 is not built) */
  int32_t maxCount;           /* 30 */
  double epsilon;             /* 0.01 */
  double minEigThreshold;     /* 1e-4 */
} svo_lk_params;

/* calcOpticalFlowPyrLK's defaults: 21, 3, 30, 0.01, 1e-4.  Host only. */
int svo_lk_default_params(svo_lk_params* params);

/* One pair, host buffers (rows `stride` bytes apart), n points -> next_pts (n x 2), status (n bytes, 1 = tracked), err (n floats,
 * 0 where status is 0; may be NULL).  Accepts the defaults with maxLevel 0 .. 3 and width, height >= 22 - anything else is
 * SVO_E_INVALID; width or height > 4096 or n > 4096 is SVO_E_CAPACITY.  Parameters, sizes and n are checked first, on the host,
 * before the context or a device is touched.  n = 0 is SVO_OK and does nothing.  Working memory is the context's own LK arena,
 * grown on demand and independent of svo_create's size.  Synchronises. */
int svo_lk_track(svo_ctx* ctx, const uint8_t* prev, const uint8_t* next, int stride, int width, int height,
                 const svo_lk_params* params, const float* pts, int n, float* next_pts, uint8_t* status, float* err);

/* B frames resident in HBM (frame b at d_frames + b * height * stride), the B - 1 consecutive pairs (b, b + 1), each with its own
 * point list: d_counts[b] <= max_pts points at d_pts + b * 2 * max_pts; results at the same places of d_next, d_status, d_err
 * (d_err may be NULL; entries past a list's count are not written).  Every frame's pyramid and derivatives are built once.
 * 2 <= B <= 4096 (more is SVO_E_CAPACITY, checked on the host like the sizes).
 * Identical to B - 1 calls of svo_lk_track.  Synchronises. */
int svo_lk_batch_dev(svo_ctx* ctx, const uint8_t* d_frames, int stride, int width, int height, int B, const svo_lk_params* params,
                     const float* d_pts, const int32_t* d_counts, int max_pts, float* d_next, uint8_t* d_status, float* d_err);

/* The reference's loop over B resident frames: frame 0's list is its seeds; for every later frame the previous frame's list is
 * tracked into it, the status-0 points are erased in order, then the frame's own seeds (d_seed_counts[f] <= max_seeds points at
 * d_seeds + f * 2 * max_seeds) are appended.  A list holds max_pts points: seeds that do not fit are dropped from the end and
 * counted in d_dropped[f].  Lists at d_lists + f * 2 * max_pts, counts in d_list_counts[f].  Everything is enqueued at once, the
 * counts never come to the host between frames; synchronises at the end.  1 <= B <= 4096 (more is SVO_E_CAPACITY). */
int svo_lk_chain_dev(svo_ctx* ctx, const uint8_t* d_frames, int stride, int width, int height, int B, const svo_lk_params* params,
                     const float* d_seeds, const int32_t* d_seed_counts, int max_seeds, int max_pts, float* d_lists,
                     int32_t* d_list_counts, int32_t* d_dropped);

/* Parity probe of the last svo_lk_track call: which = 0 the image (uint8), 1 the derivatives (int16 pairs dx, dy) of level
 * `level` of frame 0 (prev) or 1 (next); *w, *h the level's size, *top the effective top level (each may be NULL; host == NULL
 * only reports them).  A level above the top is SVO_E_INVALID.  It answers only while the context's last LK call is an
 * svo_lk_track: after any other LK call, a colour one included, it is SVO_E_INVALID and svo_last_error says why.
 * Synchronises. */
int svo_lk_debug_level(svo_ctx* ctx, int which, int frame, int level, void* host, int* w, int* h, int* top);

/* The same tracker on 8UC3 frames: interleaved B, G, R, rows `stride` >= 3 * width bytes apart, channel k is byte k as stored (no
 * swap, no conversion).  This is calcOpticalFlowPyrLK with cn = 3 (DESIGN.md section 8 "LK", "colour"): the pyramid and the
 * derivatives are built per channel, every window sum runs over 21 x 21 x 3 samples, the minimum-eigenvalue divisor stays
 * 2 * 21 * 21 and err is divided by 32 * 21 * 3 * 21.  Parameters, defaults, checks (with stride >= 3 * width), capacities, the
 * order of the checks and the results' layout are those of svo_lk_track.  A context may alternate gray and colour calls. */
int svo_lk_track_bgr(svo_ctx* ctx, const uint8_t* prev, const uint8_t* next, int stride, int width, int height,
                     const svo_lk_params* params, const float* pts, int n, float* next_pts, uint8_t* status, float* err);

/* svo_lk_batch_dev on B resident 8UC3 frames (frame b at d_frames + b * height * stride, stride >= 3 * width).  Identical to
 * B - 1 calls of svo_lk_track_bgr.  Synchronises. */
int svo_lk_batch_bgr_dev(svo_ctx* ctx, const uint8_t* d_frames, int stride, int width, int height, int B, const svo_lk_params* params,
                         const float* d_pts, const int32_t* d_counts, int max_pts, float* d_next, uint8_t* d_status, float* d_err);

/* svo_lk_chain_dev on B resident 8UC3 frames: the same track / erase / append loop, nothing comes to the host between frames. */
int svo_lk_chain_bgr_dev(svo_ctx* ctx, const uint8_t* d_frames, int stride, int width, int height, int B, const svo_lk_params* params,
                         const float* d_seeds, const int32_t* d_seed_counts, int max_seeds, int max_pts, float* d_lists,
                         int32_t* d_list_counts, int32_t* d_dropped);

/* Parity probe of the last svo_lk_track_bgr call: which = 0 the level as height x width x 3 uint8, 1 its derivatives as
 * height x width x 6 int16 (for channel c, entry 2 c is dx and entry 2 c + 1 is dy).  Otherwise as svo_lk_debug_level; it answers
 * only while the context's last LK call is an svo_lk_track_bgr, after a gray one it is SVO_E_INVALID. */
int svo_lk_debug_level_bgr(svo_ctx* ctx, int which, int frame, int level, void* host, int* w, int* h, int* top);

/* ---- LK inside the tracker (ABI-7 additions; no existing entry changed) ---------------------------------------------------
 * The same dynamic-keypoint loop, run by the tracker itself beside its chains: per frame the pose record AND the list of the
 * points followed on moving objects stay in HBM, nothing comes to the host in between.  For frame f of a sequence (id = frames
 * since svo_track_reset)
 *     list(f) = survivors(f) ++ init_seeds(f) ++ create_seeds(f)        (cut at max_pts)
 *   survivors(f)     list(f - 1) tracked from left image f - 1 into left image f as svo_lk_track / svo_lk_track_bgr track it, the
 *                    status-0 points erased in order (empty at f = 0);
 *   init_seeds(f)    at id 0 only (and only if seed_frames != 0): every keypoint strictly inside one of the frame's boxes
 *                    (u > left && u < right && v > top && v < bottom), in keypoint order (src/Tracking.cc:70-85);
 *   create_seeds(f)  while id < seed_frames: every keypoint strictly inside a box that has no map point after both matching passes,
 *                    in keypoint order (src/frame.cc:209-222) - at frame 0 an inside keypoint therefore appears twice, as in the
 *                    reference.
 * Seeds that do not fit are dropped from the end and counted per frame; erase and append are svo_lk_chain_dev's.  The boxes
 * are the ones the tracker call is given.  Nothing feeds back: records, debug records and trajectory are those of the loop
 * switched off. */
typedef struct svo_dyn_params {
  int32_t enable;       /* 0 (default) / 1 */
  int32_t colour;       /* 1: LK on the 8UC3 left frames of the _bgr entries (the reference's call, cn = 3);
                           0: on gray (the gray entries' images, or the gray the _bgr entries make) */
  int32_t seed_frames;  /* create_seeds while id < seed_frames; 2 = the reference's `id <= 1` (default);
                           -1 = every frame; 0 = none (init_seeds still only at id 0 and only if seed_frames != 0) */
  int32_t max_pts;      /* list capacity, 1 .. 4096, default 512 */
  svo_lk_params lk;     /* svo_lk_default_params */
} svo_dyn_params;

/* enable 0, colour 0, seed_frames 2, max_pts 512, lk = svo_lk_default_params.  Host only. */
int svo_dyn_default_params(svo_dyn_params* params);

/* Sets the loop's parameters.  Checked on the host first, with svo_lk_track's rules in its order (the images are the context's
 * width x height, the point count is max_pts): anything svo_lk_track does not accept, or enable / colour / seed_frames out of
 * range, is SVO_E_INVALID, max_pts > 4096 SVO_E_CAPACITY.  The parameters come into force with the next svo_track_reset or
 * svo_track_multi_reset, which also empties the lists; until then the context behaves as before.  The loop belongs to the KIND of
 * reset that adopted it (the context remembers which, also for n_seq = 1):
 *   adopted by svo_track_reset: svo_track_frame, svo_track_frame_bgr, svo_track_batch_dev, svo_track_batch_bgr_dev,
 *     svo_track_batch_host and svo_track_batch_bgr_host run it, with every "depth_source"; svo_track_multi_step_dev and
 *     svo_track_multi_step_bgr_dev refuse;
 *   adopted by svo_track_multi_reset(n_seq): svo_track_multi_step_dev and svo_track_multi_step_bgr_dev run it for the n_seq
 *     sequences at once - sequence q's list is, bit for bit, that of a single-sequence context with the same parameters fed
 *     sequence q's frames and boxes; a sequence's frame id is the number of steps since the reset; per step one launch per
 *     stage (seeds, level building, track, compact) whatever n_seq is, with "multi_pipeline" 0 and 1 alike.  The single-sequence
 *     entries above refuse.
 *   svo_track_tail_dev and svo_track_sharded_* refuse either way.
 * A refusal is SVO_E_INVALID (svo_last_error names the entry and says why), enqueues nothing and leaves the context usable.
 * colour = 1 through a gray entry is SVO_E_INVALID at that call (svo_track_multi_step_bgr_dev: colour = 1 tracks on its BGR left
 * frames, colour = 0 on the gray it makes; with colour = 0 gray and colour steps may alternate).
 * Consecutive calls of a sequence continue one chain: the first frame of a call is tracked from the last left image of the call
 * before, which the context keeps in storage of its own (many sequences: two halves of n_seq images that alternate by step). */
int svo_track_dynamic(svo_ctx* ctx, const svo_dyn_params* params);

/* One-shot: the NEXT tracker call on the context writes frame f's list to lists + f * 2 * max_pts (x, y pairs), its length to
 * counts[f] and the seeds it dropped to dropped[f] (dropped may be NULL).  Device pointers for the _dev entries; host pointers for
 * svo_track_frame[_bgr] (complete when the call returns) and for the _host entries (complete under the rule of their `results`:
 * after svo_sync, or once the second following host-fed call has returned).  A call without it still advances the chain and
 * keeps the lists inside the context.  SVO_E_INVALID unless the loop is in force.
 * Many sequences (device pointers): the next step writes sequence q's list to lists + q * 2 * max_pts, its length to counts[q]
 * and its dropped seeds to dropped[q]; complete after svo_sync, or for work ordered behind svo_stream(ctx) after the step. */
int svo_track_dynamic_out(svo_ctx* ctx, float* lists, int32_t* counts, int32_t* dropped);

/* ---- the map behind a tracked frame (backward-compatible addition; no existing entry changed) ------------------------------
 * What the reference keeps in CurrentFrame->MapPoints[j] / mappoint::worldpos and its viewer, local mapping or an evaluator would
 * read (src/view.cc:7-37): for every keypoint of a frame that has a map point when the frame ends - matched by Tracking::init,
 * pass 1 or pass 2, or the one frame::createmappoint made a point from; exactly one of the two holds per keypoint - one record,
 * in ascending keypoint order.  A match the epipolar veto took away is no record. */
enum { SVO_MAP_NEW = 1 };
typedef struct svo_map_obs {   /* 32 bytes */
  int32_t  gid;      /* identity of the map point: creation sequence number since svo_track_reset
                        (the numbers svo_track_debug's match_gid / new_gid carry) */
  int16_t  kp;       /* index j of the keypoint in the frame's keypoint list */
  uint16_t flags;    /* SVO_MAP_NEW: the point exists since this frame (Tracking::init's points at frame 0,
                        frame::createmappoint's at the end of any frame) */
  float    u, v;     /* keypoints_l[j].pt */
  float    depth;    /* the depth the frame's depth source gave keypoint j (what createmappoint reads); <= 0: none */
  float    X, Y, Z;  /* mappoint::worldpos, as the frame's PnP / LM read it or as createmappoint wrote it */
} svo_map_obs;

/* One-shot, stateless: the NEXT tracker call on the context writes frame f's records to obs + f * max_kp (max_kp: svo_create's)
 * and their number to counts[f] (<= max_kp; entries of obs beyond counts[f] are not touched).  One extra launch behind the call's
 * last pose launch on svo_stream(ctx), nothing when not armed; nothing feeds back - records, debug records, trajectory and the
 * dynamic-keypoint lists are byte for byte those of a call without it.
 * Pointers: device pointers for svo_track_batch_dev, svo_track_batch_bgr_dev and svo_track_tail_dev (complete for work ordered
 * behind svo_stream(ctx), or after svo_sync); host pointers for svo_track_frame[_bgr] (complete when the call returns) and for
 * svo_track_batch_host / svo_track_batch_bgr_host (complete under the rule of their `results`: after svo_sync, or once the
 * second following host-fed call has returned).  obs must be 16-byte aligned (the records are written as two 16-byte stores).
 * It runs with every "depth_source", with boxes, and with the dynamic-keypoint loop on or off.
 * X, Y, Z are read from the tracker's position table - a ring over 2^20 map-point ids - at the END of the call, not frame by
 * frame: a frame's record is right as long as no more than 2^20 - 1024 map points are created between that frame and the end of
 * its call.  A frame creates at most 512, so any call of up to 2046 frames is safe whatever the frames hold (KITTI frames
 * create ~120: ~8,000 frames); svo_track_overflowed's flag 1 reports a live point that was lapped.
 * svo_track_multi_step[_bgr]_dev and svo_track_sharded_* called while it is armed return SVO_E_INVALID (svo_last_error names the
 * entry), enqueue nothing, leave the context usable and the attachment armed.  A NULL argument (checked on the host before a
 * device is touched), a misaligned obs, or a call before any svo_track_reset is SVO_E_INVALID. */
int svo_track_map_out(svo_ctx* ctx, svo_map_obs* obs, int32_t* counts);

/* ---- darknet YOLO detector on the device (ABI-7 additions; no existing entry changed) -------------------------------------
 * The online half of semantic gating: Semantic::Run (src/semantic.cc) calls YOLOv3::Detect(leftimg, 0.8), which goes through
 * the dlopen C-ABI of include/YOLOv3SE.h (YoloLoad / YoloDetectFromImage) into Thirdparty/darknet/src/yolo_v3.c.  These
 * entries load any compatible darknet .cfg + .weights and run the network, decoding and NMS on the device.
 *   cfg: [net] (width, height, channels) and the sections [convolutional] (filters, size, stride, pad, padding,
 *        batch_normalize, activation leaky / linear / logistic; groups = 1, binary = 0, xnor = 0), [maxpool] (size, stride,
 *        padding; darknet's defaults: size = stride, padding = (size-1)/2, out = (w + 2*padding)/stride), [route] (layers,
 *        negative or absolute), [shortcut] (from, activation linear, same shape only), [upsample] (stride >= 1, scale 1),
 *        [yolo] (mask, anchors, classes, num) and [region] (anchors, classes, coords 4, num, softmax; no tree / map /
 *        background).  Training-only keys of [net] / [yolo] / [region] (jitter, ignore_thresh, object_scale, ...) are
 *        accepted and ignored.  Any other section or key, or an unsupported value, fails with SVO_E_INVALID and
 *        svo_det_last_error names the section and its line.  All output layers must share one class count.
 *   weights: load_weights_upto's layout - int major, minor, revision, then `seen` as size_t when major*10+minor >= 2 (and
 *        both < 1000) else as int; the transposed form (major or minor > 1000) is rejected.  Per convolutional layer, in
 *        order: biases, then scales / rolling mean / rolling variance with batch_normalize, then [filters][c][size][size]
 *        weights.  A file shorter or longer than the cfg implies fails (SVO_E_INVALID).
 * Numerics: the input tensor is darknet's letterbox_image of data/255. bit for bit; convolutions are f32 products with
 * f32 accumulation on the matrix cores (summation order differs from darknet's gemm); the epilogue is darknet's
 * (x - mean)/(sqrt(var) + .000001f) * scale + bias, then the activation; logistic and exp are evaluated in double as
 * darknet does.  Decoding, do_nms_sort(0.45) and YoloDetect's record loop run on the device in darknet's order, with one
 * exception: darknet sorts with libc qsort, whose order for equal scores is unspecified - here equal scores keep the order
 * they had before the sort (a stable sort), the one point where darknet's order is not pinned. */
typedef struct svo_det svo_det;

enum { SVO_DET_CONV = 0, SVO_DET_MAXPOOL = 1, SVO_DET_ROUTE = 2, SVO_DET_SHORTCUT = 3, SVO_DET_UPSAMPLE = 4,
       SVO_DET_YOLO = 5, SVO_DET_REGION = 6 };
enum { SVO_DET_ACT_LINEAR = 0, SVO_DET_ACT_LEAKY = 1, SVO_DET_ACT_LOGISTIC = 2 };

/* One layer of svo_det_describe. */
typedef struct svo_det_layer {
  int32_t type;                      /* SVO_DET_* */
  int32_t in_w, in_h, in_c;
  int32_t out_w, out_h, out_c;
  int32_t size, stride, pad;         /* convolutional / maxpool (pad = the padding in pixels); upsample: stride */
  int32_t batch_normalize, activation;   /* convolutional: 0 / 1, SVO_DET_ACT_*; shortcut: SVO_DET_ACT_LINEAR */
  int32_t classes, num;              /* yolo / region: classes, anchors used by the layer (yolo: the mask's length) */
  int32_t from[4];                   /* route: up to 4 absolute source layers (-1 unused); shortcut: from[0] */
  int64_t n_params;                  /* floats this layer reads from the .weights file */
} svo_det_layer;

/* Host only, no device: parse `cfg` (and, if `weights` is not NULL, check the weights file's header and exact size against
 * it).  Writes up to max_layers layers, *n_layers = the network's layer count, *n_params = the floats the weights file
 * must hold after its header.  layers may be NULL with max_layers = 0. */
int svo_det_describe(const char* cfg, const char* weights, svo_det_layer* layers, int max_layers, int* n_layers,
                     int64_t* n_params);
/* Text of the last failure of `det`; with det = NULL, of the calling thread's last svo_det_describe / svo_det_create. */
const char* svo_det_last_error(const svo_det* det);

/* A detector on HIP device `device` for batches of up to max_batch images (YoloLoad + set_batch_network).  The weights live
 * in HBM; every layer's output is kept for max_batch images (svo_det_debug_tensor). */
int svo_det_create(int device, const char* cfg, const char* weights, int max_batch, svo_det** out);
int svo_det_destroy(svo_det* det);

/* Latency mode, YoloDetectFromImage's semantics on one 8-bit interleaved image (HOST memory, `stride` bytes per row):
 * C = 3 - channel k is byte k as stored, as YOLOv3::Detect hands darknet the BGR cv::Mat unswapped; C = 1 - a gray image,
 * replicated to three channels (the project's B = G = R convention for gray input to colour stages; not reference
 * behaviour, the reference has no gray detector input).  Records [class, prob, left, top, right - left, bot - top] go to
 * `result` in darknet's final order while result_idx * 6 + 5 < result_sz; *n = records written.  Synchronises. */
int svo_det_detect(svo_det* det, const uint8_t* img, int W, int H, int C, int stride, float thresh, float* result,
                   int result_sz, int* n);

/* Throughput mode: B images in HBM (image f at d_img + f * H * stride), the same records per image - frame f's at
 * d_records + 6 * max_records * f, count d_n_records[f] (<= max_records).  d_boxes_out (may be NULL; the struct is read on
 * the host, its arrays are DEVICE pointers written here): frame f's first min(count, 64, stride) records as tracker boxes
 * {left = x, right = x + w, top = y, bottom = y + h} at boxes + 4 * stride * f and their number at n[f] - the online path
 * the reference left commented in src/frame.cc:209-214 / src/Tracking.cc:70-77.  Does not synchronise: the detector runs
 * on a stream of its own.  consumer (may be NULL, same device): that context's NEXT device-resident tracking call
 * (svo_track_batch_dev, svo_track_batch_bgr_dev, svo_track_tail_dev, ...) waits on the device for these outputs before
 * it reads any box, so the boxes can be handed over with no host synchronisation in between; and this call first waits
 * on the device for the consumer's last tracking call that read boxes, so a steady detect -> track loop may reuse the same
 * box and record arrays without a host synchronisation either.  The images must stay valid until the work is done
 * (svo_det_sync, or the consumer's svo_sync after its tracking call). */
int svo_det_batch_dev(svo_det* det, const uint8_t* d_img, int W, int H, int C, int stride, int B, float thresh,
                      float* d_records, int max_records, int32_t* d_n_records, const svo_boxes_dev* d_boxes_out,
                      svo_ctx* consumer);
/* YoloDetectFromImage itself: darknet's planar float image (HOST memory, C = 3 planes of H x W floats, used as given - no
 * scaling, no channel swap), otherwise as svo_det_detect.  Synchronises.  (The drop-in libYOLOv3SE.so calls this.) */
int svo_det_detect_planar(svo_det* det, const float* data, int W, int H, int C, float thresh, float* result, int result_sz,
                          int* n);
/* Per-layer timing: with enable != 0, each later call records HIP events around the input kernel, every layer and the
 * decode; svo_det_layer_times then gives the last call's times in ms - ms[0] the input, ms[1 + i] layer i, ms[n - 1] the
 * decode + NMS + records; *n = layers + 2.  Synchronises.  Profiling adds an event per launch. */
int svo_det_profile(svo_det* det, int enable);
int svo_det_layer_times(svo_det* det, float* ms, int max_n, int* n);
/* Wait for the detector's work in flight. */
int svo_det_sync(svo_det* det);
/* Parity probe: layer `layer`'s output for image `frame` of the last call, out_c x out_h x out_w floats (layer = -1: the
 * network input, 3 x height x width).  Synchronises. */
int svo_det_debug_tensor(svo_det* det, int layer, int frame, float* host_out);

/* ---- stereo rectification on the device (ABI-8 additions; no existing entry changed) ---------------------------------------
 * Every other entry of this header starts from a RECTIFIED pair.  These entries make one from a raw pair and the calibration
 * an ORB-SLAM2 settings file carries (LEFT.K / .D / .R / .P and RIGHT.*, or the flat Camera.fx .. Camera.p2 keys):
 * cv::initUndistortRectifyMap(K, D, R, P, size, CV_32FC1) once per object, then cv::remap(INTER_LINEAR, BORDER_CONSTANT 0)
 * per image, 8-bit, 1 channel or 3 interleaved channels.  The arithmetic, operation by operation, is DESIGN.md section 8
 * "Rectification" (restated from OpenCV 3.2; parity with OpenCV itself is not pinned - the tests compare with a numpy restatement).
 *   K = (fx, fy, cx, cy); D = (k1, k2, p1, p2, k3); R = 3 x 3 row-major; P = (fx', fy', cx', cy'), the entries (0,0), (1,1),
 *   (0,2), (1,2) of the 3 x 4 projection.  Sizes: widths 8 .. 8192, heights 1 .. 8192; source and destination may differ.
 * Out of scope: computing R and P from extrinsics (cv::stereoRectify); fisheye, rational (k4..k6), thin-prism and tilted
 * models; 16-bit images; interpolations other than bilinear; rectification inside the host-fed entries
 * (svo_track_batch_host, svo_track_sharded_*): rectify into device buffers and call the device-resident ones. */
typedef struct svo_rect_cam { double K[4], D[5], R[9], P[4]; } svo_rect_cam;
typedef struct svo_rect svo_rect;

/* Builds both cameras' maps on HIP device `device` (float64, one lane per destination row: the running sums along a row are
 * part of the contract) and keeps them in HBM.  SVO_E_INVALID before any device is touched: a NULL pointer, a width outside
 * 8 .. 8192 or a height outside 1 .. 8192, a non-finite calibration value, det(Ar R) == 0 (or not finite).
 * svo_rect_last_error(NULL) says which. */
int svo_rect_create(int device, int src_w, int src_h, int dst_w, int dst_h, const svo_rect_cam* left,
                    const svo_rect_cam* right, svo_rect** out);
int svo_rect_destroy(svo_rect* rect);
/* Text of the last failure of `rect`; with rect = NULL, of the calling thread's last svo_rect_create. */
const char* svo_rect_last_error(const svo_rect* rect);
/* The rectified pair's camera for svo_track_reset and the front end: fx', fy', cx', cy' of the LEFT P (as float), bf as given
 * (0 where the caller has none). */
int svo_rect_camera(const svo_rect* rect, double bf_or_0, svo_camera* cam);
/* One raw pair, host to host: L / R rows `src_stride` bytes apart (>= cn * src_w), cn = 1 or 3, outL / outR rows
 * `dst_stride` bytes apart (>= cn * dst_w; bytes of a row beyond cn * dst_w are not written).  Synchronises. */
int svo_rect_process(svo_rect* rect, const uint8_t* L, const uint8_t* R, int src_stride, int cn, uint8_t* outL,
                     uint8_t* outR, int dst_stride);
/* B raw pairs resident in HBM (pair b at d_L / d_R + b * src_h * src_stride) -> B rectified pairs (pair b at d_outL / d_outR
 * + b * dst_h * dst_stride: the layout svo_track_batch_dev, svo_track_batch_bgr_dev, svo_track_multi_step[_bgr]_dev and
 * svo_frontend_batch_dev take), one launch for both sides (in chunks where B exceeds the grid's limit; B >= 1, no cap).
 * Does not synchronise: the rectifier runs on a stream of its own (svo_rect_stream).
 * consumer (may be NULL, same device): that context's NEXT call of one of the five entries above waits ON THE DEVICE for
 * these outputs before it reads a pixel - no host synchronisation in between.  A context never named here enqueues exactly
 * what it did before.
 * The other direction has no hidden wait: the outputs (and the inputs) of a call may be rewritten once the consumer's call
 * that read them is done - after svo_sync(consumer), or behind an event the caller records on svo_stream(consumer) after
 * that call and makes svo_rect_stream wait for (the rule svo_track_multi_step_dev states for its images).  A caller that
 * alternates between two output sets and synchronises the consumer once per two calls satisfies it. */
int svo_rect_batch_dev(svo_rect* rect, const uint8_t* d_L, const uint8_t* d_R, int src_stride, int cn, int B,
                       uint8_t* d_outL, uint8_t* d_outR, int dst_stride, svo_ctx* consumer);
/* Wait for the rectifier's work in flight; its stream (a hipStream_t). */
int svo_rect_sync(svo_rect* rect);
void* svo_rect_stream(svo_rect* rect);
/* Parity probe, side 0 = left, 1 = right; any output may be NULL: the inverse matrix iR (host float64), the float32 maps
 * (dst_h x dst_w each) and the fixed-point coordinates the remap kernel works from, sxsy[2 (i dst_w + j)] = sx, [.. + 1] =
 * sy (ix = sx >> 5, a = sx & 31); a pixel that is "outside" by its map value has sx = sy = INT32_MIN.  Synchronises. */
int svo_rect_debug_maps(svo_rect* rect, int side, double iR[9], float* mapx, float* mapy, int32_t* sxsy);

/* ---- windowed bundle adjustment over the map records (backward-compatible addition; no existing entry changed) --------------
 * What ORB-SLAM2 calls local bundle adjustment, over the records svo_track_map_out leaves in HBM: the last `window` poses and
 * the points they share, refined together - g2o's EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ edges, BlockSolver's Schur
 * complement, its Levenberg-Marquardt.  The contract, operation by operation: DESIGN.md section 8 "Windowed bundle adjustment";
 * the numpy twin: tests/ba_ref.py.  Nothing feeds back into the tracker.
 * Out of scope: chained windows (a window's fixed frames taking the previous window's result: one call per window does that),
 * outlier-removal rounds, per-octave information, marginalisation priors, the many-sequence and sharded tracker entries. */
enum { SVO_BA_OK = 0, SVO_BA_EMPTY = 1 };   /* svo_ba_stats.status; empty: no point with two edges, the input poses are returned */
typedef struct svo_ba_params {
  int32_t window;        /* frames of a window, 2 .. 8 */
  int32_t n_fixed;       /* the first n_fixed frames keep their poses, 1 .. window - 1 */
  int32_t iterations;    /* LM iterations, 1 .. 20 */
  int32_t stereo;        /* 1: a record with depth > 0 is a stereo edge (u, v, u - bf / depth); 0: every edge is mono */
  double huber_mono, huber_stereo;   /* Huber delta per edge type; <= 0: no robust kernel */
  double lambda_init;    /* > 0: the LM's first lambda (g2o's userLambdaInit); otherwise 1e-5 x the largest diagonal entry */
} svo_ba_params;
/* window 8, n_fixed 1, iterations 10, stereo 1, (double)(float)sqrt(5.991) and (double)(float)sqrt(7.815), lambda_init 0 */
int svo_ba_default_params(svo_ba_params* p);

typedef struct svo_ba_stats {
  int32_t status, n_points, n_edges, n_edges_stereo, iterations, trials_total;
  double chi2_initial, chi2_final, lambda_final;
} svo_ba_stats;
typedef struct svo_ba_point {   /* 32 bytes */
  int32_t gid, n_obs;    /* the map point and the number of its edges in the window */
  double X, Y, Z;        /* refined world position */
} svo_ba_point;
typedef struct svo_ba svo_ba;

/* An adjuster for windows of up to 8 frames x max_kp records (1 .. 4096) and up to max_windows windows a call, with a stream
 * and scratch of its own (about 2.6 KB per record of a window).  Touches no device: the stream and the scratch, whose size is
 * fixed here, come with the first call that needs them (SVO_E_NODEVICE / SVO_E_NOMEM are answered there), so the argument checks
 * of every entry answer on a machine without a GPU.  svo_ba_last_error(NULL): the calling thread's last failure without an object. */
int svo_ba_create(int device, int max_kp, int max_windows, svo_ba** out);
void svo_ba_destroy(svo_ba* ba);
int svo_ba_sync(svo_ba* ba);
void* svo_ba_stream(svo_ba* ba);
const char* svo_ba_last_error(const svo_ba* ba);

/* n_windows windows over frames resident in HBM; window w covers frames first + w * step .. + window - 1.  Frame f's records
 * are d_obs + f * obs_stride (obs_stride <= max_kp records a frame; d_counts[f] of them count, a count above obs_stride is
 * clamped on the device), its float32 4 x 4 Tcw stands at the start of element f of d_Tcw, elements pose_stride_bytes apart
 * (64 for bare poses; an array of svo_track_result fits with sizeof(svo_track_result)).
 * Outputs: d_Tcw_out n_windows x window x 16 float64 (a fixed frame, a free frame without edges and every frame of an empty
 * window: the input pose widened); d_points (may be NULL) n_windows x (window * max_kp / 2) records, the first n_points of
 * a window written, by ascending gid; d_stats one record per window.
 * Does not synchronise.  producer (may be NULL, same device): the adjuster's stream waits ON THE DEVICE for an event recorded
 * on svo_stream(producer), so the windows run behind the tracker call that writes the records and poses; the producer waits
 * for nothing and nothing else is enqueued on its streams.  Windows are independent problems: a window's outputs do not depend
 * on n_windows, on its index or on the other windows, and are the same bytes on every run.
 * SVO_E_INVALID before a device is touched (svo_ba_last_error names the argument): a NULL pointer, window outside 2 .. 8,
 * n_fixed outside 1 .. window - 1, iterations outside 1 .. 20, a non-finite parameter or camera value, fx or fy <= 0,
 * obs_stride outside 1 .. max_kp, n_windows outside 1 .. max_windows, first < 0, step < 1, d_obs not 16-byte aligned, a pose
 * stride below 64 or not a multiple of 4. */
int svo_ba_windows_dev(svo_ba* ba, const svo_camera* cam, const svo_ba_params* params, const svo_map_obs* d_obs,
                       const int32_t* d_counts, int obs_stride, const void* d_Tcw, int pose_stride_bytes, int first, int n_windows,
                       int step, double* d_Tcw_out, svo_ba_point* d_points, svo_ba_stats* d_stats, svo_ctx* producer);
/* One window, host to host: obs window x obs_stride records, counts window, Tcw window x 16 float32; points (may be NULL
 * together with n_points) holds window * max_kp / 2 records.  Synchronises. */
int svo_ba_window(svo_ba* ba, const svo_camera* cam, const svo_ba_params* params, const svo_map_obs* obs, const int32_t* counts,
                  int obs_stride, const float* Tcw, double* Tcw_out, svo_ba_point* points, int32_t* n_points, svo_ba_stats* stats);

/* ---- bag-of-words place recognition (backward-compatible addition; no existing entry changed) -------------------------------
 * DBoW2 as ORB-SLAM2 carries it (Thirdparty/DBoW2): a vocabulary tree over the 32-byte descriptors of this library, a frame's
 * BowVector and FeatureVector, L1Scoring::score, and for a query frame the best-scoring earlier frames.  The contract, operation
 * by operation: DESIGN.md section 8 "Bag of words"; the numpy twin: tests/bow_ref.py.  Parity with a compiled DBoW2 is not pinned.
 * ORB-SLAM2's published vocabulary does not fit these descriptors (it was trained on the learned rBRIEF pattern, this library
 * describes with include/svo_brief_pattern.h): a vocabulary has to be trained on the library's own descriptors.
 * Out of scope: an inverted index and DetectLoopCandidates' heuristics (covisibility groups, consistency over three keyframes),
 * loop correction or any feedback into the tracker, scorings other than L1, DBoW2's binary / YAML formats, the many-sequence
 * entries, descriptors other than 32 bytes.  (SearchByBoW and the fixed-scale Sim3Solver: "loop verification" below.) */
enum { SVO_BOW_TF_IDF = 0, SVO_BOW_TF = 1, SVO_BOW_IDF = 2, SVO_BOW_BINARY = 3 };   /* DBoW2's WeightingType */
typedef struct svo_bow_entry {     /* 16 bytes: one word of a BowVector */
  uint32_t word, reserved;         /* reserved: 0 */
  double value;
} svo_bow_entry;
typedef struct svo_bow_feature {   /* 8 bytes: one pair of a FeatureVector */
  uint32_t node, feature;          /* the node's id as the file (or the arrays) numbered it; the feature's index in its frame */
} svo_bow_feature;
typedef struct svo_bow_cand {      /* 16 bytes: one candidate of a query; an unused slot is {-1, 0, 0.0} */
  int32_t frame, reserved;
  double score;
} svo_bow_cand;
typedef struct svo_bow svo_bow;

/* A vocabulary for frames of up to max_kp features (1 .. 2048) and calls of up to max_frames frames (1 .. 65535), with a stream
 * and scratch of its own (8 bytes per feature of a call).  Both constructors parse and validate on the host and touch no device:
 * the device copy of the tree, the stream and the scratch come with the first call that needs them (SVO_E_NODEVICE / SVO_E_NOMEM
 * are answered there), so the argument checks of every entry answer on a machine without a GPU.
 * svo_bow_last_error(NULL): the calling thread's last failure without an object.
 * From text: DBoW2's loadFromTextFile format, `k L scoring weighting`, then one line per node from id 1 on, `parent is_leaf
 * b0 .. b31 weight`.  Children need not be contiguous by id; every output names nodes by the file's ids.  SVO_E_INVALID with a
 * message naming the line: k outside 2 .. 20, L outside 1 .. 10, scoring other than 0 (L1_NORM), weighting outside 0 .. 3, a parent
 * id not yet defined, a parent marked a leaf, more than k children of one node, an inner node without children, a malformed line.
 * From arrays: n_nodes nodes with the root as node 0 (its parent, descriptor and weight are ignored), parents[i] < i, descriptors
 * n_nodes x 32 bytes, weights n_nodes; a node without children is a leaf.  Words number the leaves in node-id order. */
int svo_bow_create_from_text(int device, const char* path, int max_kp, int max_frames, svo_bow** out);
int svo_bow_create(int device, int k, int L, int weighting, int n_nodes, const int32_t* parents, const uint8_t* descriptors,
                   const double* weights, int max_kp, int max_frames, svo_bow** out);
/* The text format again; weights with 17 significant digits, so a file written here loads to the same bits (DBoW2 prints 6). */
int svo_bow_save_text(svo_bow* bow, const char* path);
/* k, L, nodes (the root included), words, weighting; any output may be NULL. */
int svo_bow_describe(const svo_bow* bow, int* k, int* L, int* n_nodes, int* n_words, int* weighting);
void svo_bow_destroy(svo_bow* bow);
int svo_bow_sync(svo_bow* bow);
void* svo_bow_stream(svo_bow* bow);
const char* svo_bow_last_error(const svo_bow* bow);

/* B frames resident in HBM: frame f's descriptors at d_desc + f * kp_stride * 32, d_n[f] of them (the layouts
 * svo_frontend_batch_dev writes and svo_track_tail_dev reads; a count above kp_stride is clamped on the device, a negative one is 0).
 * Outputs, frame f at f * kp_stride elements, any of them may be NULL: d_words the word of every feature, -1 for a feature whose
 * word's weight is not > 0 (a stop word) and for the indices from the count to kp_stride; d_vec the BowVector in ascending word
 * order (L1-normalised) and d_vec_n its length; d_fv the FeatureVector, the pairs of the features that are not stopped by ascending
 * (node, feature), the node being the one at level L - levelsup of the feature's walk (the root, 0, when L - levelsup <= 0; the leaf
 * when the walk ends above that level) and d_fv_n their number.  Elements behind a frame's length are not written.
 * Does not synchronise.  producer (may be NULL, same device): the object's stream waits ON THE DEVICE for an event recorded on
 * svo_stream(producer), so the call runs behind the front end call that writes the descriptors; the producer waits for nothing
 * and nothing else is enqueued on its streams.  The same call gives the same bytes.
 * SVO_E_INVALID before a device is touched: a NULL bow, d_desc or d_n, d_desc not 4-byte aligned, kp_stride outside 1 .. max_kp,
 * B outside 1 .. max_frames, levelsup < 0, a producer on another device. */
int svo_bow_transform_dev(svo_bow* bow, const uint8_t* d_desc, const int32_t* d_n, int kp_stride, int B, int levelsup,
                          int32_t* d_words, svo_bow_entry* d_vec, int32_t* d_vec_n, svo_bow_feature* d_fv, int32_t* d_fv_n,
                          svo_ctx* producer);
/* One frame, host to host: n (0 .. max_kp) descriptors; words n, vec and fv up to n records (vec goes with vec_n, fv with fv_n;
 * each pair and words may be NULL).  Synchronises. */
int svo_bow_transform(svo_bow* bow, const uint8_t* desc, int n, int levelsup, int32_t* words, svo_bow_entry* vec, int32_t* vec_n,
                      svo_bow_feature* fv, int32_t* fv_n);
/* L1Scoring::score(A[a], B[b]) for every pair: d_scores QA x NB doubles.  Vector i of a set at i * stride records (1 <= stride <=
 * max_kp), its length in d_nA / d_nB (clamped to 0 .. stride); words ascending, as svo_bow_transform_dev writes them.  Vectors
 * without a common word score -0.0.  QA 1 .. 65535, NB >= 1.  Does not synchronise (the object's stream). */
int svo_bow_score_dev(svo_bow* bow, const svo_bow_entry* d_vecA, const int32_t* d_nA, int QA, const svo_bow_entry* d_vecB,
                      const int32_t* d_nB, int NB, int stride, double* d_scores);
/* For each query frame q = q0 .. q0 + Q - 1 of the N resident vectors: the top_k (1 .. 16) frames j of 0 .. q - gap - 1 with
 * score(vec[q], vec[j]) > min_score, by descending score, equal scores by ascending j; d_cand Q x top_k records, d_cand_n Q counts.
 * The Q x N scores are not written anywhere.  gap >= 0; min_score not a NaN.  Does not synchronise. */
int svo_bow_query_dev(svo_bow* bow, const svo_bow_entry* d_vec, const int32_t* d_vec_n, int stride, int N, int q0, int Q, int gap,
                      double min_score, int top_k, svo_bow_cand* d_cand, int32_t* d_cand_n);
/* One level of the walk alone, for tests and for training: n (>= 1) descriptors against k (1 .. 20) centres of 32 bytes; d_idx
 * the nearest centre (the earliest among equals), d_dist its Hamming distance; either may be NULL.  Runs on the object's stream,
 * does not synchronise. */
int svo_bow_assign_dev(svo_bow* bow, const uint8_t* d_desc, int n, const uint8_t* d_centres, int k, int32_t* d_idx, int32_t* d_dist);

/* ---- loop verification (backward-compatible addition; no existing entry changed) --------------------------------------------
 * What ORB-SLAM2's LoopClosing::ComputeSim3 does with a candidate, for stereo (scale fixed to 1): ORBmatcher::SearchByBoW over
 * the two frames' FeatureVectors, then Sim3Solver - RANSAC over Horn's closed-form alignment of the matched map points.  The
 * contract, operation by operation: DESIGN.md section 8 "Loop verification"; the numpy twin: tests/loop_ref.py.  Parity with a
 * compiled ORB-SLAM2 is not pinned.  Two stated departures from it: samples come from splitmix64(seed + 3 * iteration + draw)
 * instead of rand(), and the rotation is taken from the quaternion directly instead of through atan2 and cv::Rodrigues.
 * Inputs are what the other entries leave in HBM: descriptors and keypoints (svo_frontend_batch_dev), FeatureVectors
 * (svo_bow_transform_dev), candidates (svo_bow_query_dev), map records (svo_track_map_out) and the tracked poses.
 * Out of scope: SearchBySim3, OptimizeSim3, scale estimation, covisibility consistency, loop correction and any feedback into
 * the tracker; the many-sequence entries. */
enum { SVO_LOOP_OK = 0, SVO_LOOP_FEW = 1, SVO_LOOP_REJECTED = 2, SVO_LOOP_SKIPPED = 3 };   /* svo_loop_result.status */
typedef struct svo_loop_params {
  int32_t th_low;             /* SearchByBoW: best distance < th_low, 1 .. 256 */
  float nn_ratio;             /* and (float)best < nn_ratio * (float)second, (0, 1] */
  int32_t check_orientation;  /* 1: keep the three fullest bins of the rotation histogram */
  double prob;                /* RANSAC probability, (0, 1) */
  int32_t min_inliers;        /* >= 3 */
  int32_t max_iterations;     /* 1 .. 1024 */
  uint64_t seed;              /* of the samples */
  double chi2;                /* maxerr = chi2 * sigma2[octave] */
  float scale_factor;         /* ORBextractor's, for sigma2 */
  int32_t refine;             /* 1: one more alignment over all inliers of the result (not ORB-SLAM2) */
} svo_loop_params;
/* 50, 0.75f, 1, 0.99, 20, 300, seed 0x5eed5eed5eed5eed, 9.210, 1.2f, 0: what LoopClosing passes */
int svo_loop_default_params(svo_loop_params* p);
typedef struct svo_loop_result {   /* 168 bytes */
  int32_t status;       /* OK: a hypothesis with more than min_inliers inliers ended the search; REJECTED: the bound was reached, the
                           best so far is reported; FEW: fewer than min_inliers correspondences, the solver did not run; SKIPPED: a
                           negative frame index.  FEW and SKIPPED: bound 0, visited 0, winner -1, n_inliers 0, sample -1, T12 = I */
  int32_t n_matches;    /* N: the correspondences, matches whose two keypoints both have a map record */
  int32_t bound;        /* iterations admitted for N */
  int32_t visited;      /* iterations the sequential rule looked at */
  int32_t winner;       /* the result's iteration */
  int32_t n_inliers;
  int32_t sample[3];    /* the winner's three correspondences (indices into the ascending-i1 list) */
  int32_t reserved;     /* 0 */
  double T12[16];       /* row-major 4 x 4: takes b's camera coordinates to a's */
} svo_loop_result;
typedef struct svo_loop svo_loop;

/* A verifier for frames of up to max_kp keypoints (1 .. 2048) and calls of up to max_pairs pairs (1 .. 65535), with a stream and
 * scratch of its own (96 bytes per keypoint of a pair).  Touches no device: the stream and the scratch come with the first call
 * that needs them (SVO_E_NODEVICE / SVO_E_NOMEM are answered there), so the argument checks of every entry answer on a machine
 * without a GPU.  svo_loop_last_error(NULL): the calling thread's last failure without an object. */
int svo_loop_create(int device, int max_kp, int max_pairs, svo_loop** out);
void svo_loop_destroy(svo_loop* loop);
int svo_loop_sync(svo_loop* loop);
void* svo_loop_stream(svo_loop* loop);
const char* svo_loop_last_error(const svo_loop* loop);
/* Records an event on `stream` (a hipStream_t of the object's device: svo_stream(ctx), svo_bow_stream(bow), ...) and makes the
 * object's stream wait for it ON THE DEVICE: the calls that follow run behind the work enqueued on `stream` so far.  Nothing else
 * is enqueued on `stream` and nothing of its owner waits. */
int svo_loop_wait(svo_loop* loop, void* stream);
/* The iteration bound of Sim3Solver::SetRansacParameters for N = 0 .. n_max correspondences (bounds holds n_max + 1 values; 0
 * where N < min_inliers), with the host's log and pow.  Needs no object and no device: it is the table the device looks up. */
int svo_loop_bounds(const svo_loop_params* params, int n_max, int32_t* bounds);

/* The candidates of svo_bow_query_dev (Q x top_k records, Q counts; queries q0 .. q0 + Q - 1) as pairs: d_pairs holds
 * Q * top_k x 2 int32, slot i * top_k + t is (q0 + i, cand.frame) for t < the count (clamped to 0 .. top_k) and a frame >= 0,
 * else (-1, -1).  Q * top_k <= max_pairs, top_k 1 .. 16.  Does not synchronise. */
int svo_loop_pairs_dev(svo_loop* loop, const svo_bow_cand* d_cand, const int32_t* d_cand_n, int q0, int Q, int top_k,
                       int32_t* d_pairs);
/* SearchByBoW(KF1 = a, KF2 = b) for n_pairs pairs (a, b) = d_pairs[2 p], d_pairs[2 p + 1] of frames resident in HBM: frame f's
 * descriptors, keypoints and FeatureVector at f * kp_stride elements (d_n[f] keypoints, d_fv_n[f] pairs), its map records at
 * f * obs_stride (d_obs_n[f] of them, ascending kp).  A count above its stride is clamped on the device, a negative one is 0.
 * Outputs: d_match n_pairs x kp_stride int32 - for keypoint i1 of a the matched keypoint of b or -1, -1 from a's count to the
 * stride; d_match_n n_pairs counts.  A pair with a negative frame index: all -1 and 0.  Does not synchronise. */
int svo_loop_match_dev(svo_loop* loop, const svo_loop_params* params, const uint8_t* d_desc, const svo_kp* d_kp, const int32_t* d_n,
                       int kp_stride, const svo_bow_feature* d_fv, const int32_t* d_fv_n, const svo_map_obs* d_obs,
                       const int32_t* d_obs_n, int obs_stride, const int32_t* d_pairs, int n_pairs, int32_t* d_match,
                       int32_t* d_match_n);
/* The relative pose of every pair from its row of d_match (any -1 / index array of that layout; an entry outside 0 .. kp_stride - 1
 * or naming a keypoint without a map record is no correspondence; this entry is not given the keypoint counts, so a record counts
 * when its kp lies in 0 .. kp_stride - 1, where svo_loop_match_dev asks for kp below the frame's count d_n[f]).  Frame f's float32 4 x 4 Tcw stands at the start of element f
 * of d_Tcw, elements pose_stride_bytes apart (as in svo_ba_windows_dev).  d_result n_pairs records; d_inliers (may be NULL)
 * n_pairs x kp_stride bytes, 1 for the keypoints of a whose correspondence is an inlier of the result, all kp_stride written.
 * A change of prob, min_inliers or max_iterations between calls rebuilds the bound table and synchronises the object's stream once;
 * otherwise the call does not synchronise.  The same call gives the same bytes. */
int svo_loop_solve_dev(svo_loop* loop, const svo_camera* cam, const svo_loop_params* params, const svo_kp* d_kp,
                       const svo_map_obs* d_obs, const int32_t* d_obs_n, int obs_stride, const void* d_Tcw, int pose_stride_bytes,
                       const int32_t* d_pairs, int n_pairs, const int32_t* d_match, int kp_stride, svo_loop_result* d_result,
                       uint8_t* d_inliers);
/* Both stages, one behind the other on the object's stream.
 * SVO_E_INVALID before a device is touched, for the three entries above (svo_loop_last_error names the argument): a NULL
 * pointer (d_inliers excepted), d_desc not 4-byte, d_fv not 8-byte, d_obs not 16-byte aligned, kp_stride or obs_stride outside
 * 1 .. max_kp, n_pairs outside 1 .. max_pairs, th_low outside 1 .. 256, nn_ratio not in (0, 1], min_inliers < 3, max_iterations
 * outside 1 .. 1024, prob not in (0, 1), a non-finite or non-positive chi2 or scale_factor, a non-finite camera value, fx or
 * fy <= 0, a pose stride below 64 or not a multiple of 4. */
int svo_loop_verify_dev(svo_loop* loop, const svo_camera* cam, const svo_loop_params* params, const uint8_t* d_desc,
                        const svo_kp* d_kp, const int32_t* d_n, int kp_stride, const svo_bow_feature* d_fv, const int32_t* d_fv_n,
                        const svo_map_obs* d_obs, const int32_t* d_obs_n, int obs_stride, const void* d_Tcw, int pose_stride_bytes,
                        const int32_t* d_pairs, int n_pairs, int32_t* d_match, int32_t* d_match_n, svo_loop_result* d_result,
                        uint8_t* d_inliers);
/* One pair host to host: every array holds frame a, then frame b (desc 2 x kp_stride x 32 bytes, kp and fv 2 x kp_stride records,
 * obs 2 x obs_stride records, the counts 2 values, Tcw 2 x 16 float32); match (kp_stride, may be NULL), result, inliers
 * (kp_stride, may be NULL).  Synchronises. */
int svo_loop_verify(svo_loop* loop, const svo_camera* cam, const svo_loop_params* params, const uint8_t* desc, const svo_kp* kp,
                    const int32_t* n, int kp_stride, const svo_bow_feature* fv, const int32_t* fv_n, const svo_map_obs* obs,
                    const int32_t* obs_n, int obs_stride, const float* Tcw, int32_t* match, svo_loop_result* result,
                    uint8_t* inliers);

#ifdef __cplusplus
}
#endif
#endif /* SVO_H */
