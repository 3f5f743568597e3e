// svo_track_state.h - the tracker's records in HBM (TrackState, TrackWork, GatePre) and the small device helpers more than one of
// its units needs.  No kernels: a kernel is launched, and its attributes are set, only by the unit that defines it.
#pragma once
#include "svo_internal.h"
#include "svo_gate.h"

#define TRK_MAXKP 512
#define TRK_CAP 4096
#define TRK_ROWS_MAX 3072        // live rows k_ti_lists can meet: 4 frames of local points + the last frame's, + slack
#define TRK_LCAP 8               // packed entries (claimable columns) a pool row keeps; more -> the row is "dense"
#define TRK_GPOS (1 << 20)       // map-point position table: ring over map-point ids
#define TRK_DNC 24                // dense rows whose distance row is cached in LDS during a pass
#define TRK_DENSE 0xFF           // ncand marker: more than `lcap` candidates, the row's distances are in D

struct TrackPool {
  alignas(16) uint32_t desc[TRK_CAP * 8];
  int32_t create_id[TRK_CAP];
  int32_t gid[TRK_CAP];          // map-point id = creation sequence number; positions live in gpos[gid % TRK_GPOS]
  uint8_t bad[TRK_CAP];
  uint8_t in_local[TRK_CAP];
};

// Samples of the fused pose launch whose completion the frame's workgroup waits for one by one: cv::solvePnPRansac's adaptive bound
// ends within the first 8 samples on 96 % of the frames (a median of 4), and then the other 92 need not be waited for.
#define TP_EARLY 8
#define TP_FLAGS 16   // samples that announce themselves one by one (work->hyp_early)
// What the index chain hands to the pose chain for one frame.
// Written by k_ti_resolve with agent-scope (sc1) stores and published through `ready`, read by the pose kernels with agent-scope
// loads after they have seen the tag: the pose chain does not wait on stream events for the index chain (see tp_wait_work).
struct TrackWork {
  int32_t ready;                 // = frame index + 1 once the record of that frame is complete (cleared by svo_track_reset)
  int32_t frame_id, nkp, n_stereo, n_pass1, n_pass2, n_new, n_local, skip_match;
  long long ts[8];               // diagnostics: s_memtime at begin / pass 1 / pass 2 / frame end / done, dense rows, late rows
  long long rt[6];               // diagnostics: s_memrealtime (100 MHz, one clock for the chip) at k_ti_resolve start / end,
                                 // k_tp_hyp start (its workgroup 0), k_tp_frame end, k_tp_frame start, and [5] a DURATION: fused
                                 // launch, frame decided within the TP_EARLY awaited samples - from the latest of their announcement
                                 // clocks (hyp_rt) to the LM's first build; 0 otherwise
  int32_t diag[2];               // [0] rows of pass 1 | rounds << 16, [1] rows of pass 2 | rounds << 16
  int32_t n_edges;               // 3D-2D correspondences of the frame (src/pnpmatch.cc:216-224), in keypoint order:
  int32_t edge_gid[TRK_MAXKP];   //   id of the map point (CurrentFrame->MapPoints[j]->...) ...
  int32_t edge_kp[TRK_MAXKP];    //   ... and the keypoint j it is matched to
  int32_t new_gid[TRK_MAXKP];    // per keypoint: id of the map point created from it at the frame's end, or -1
  // written by the pose chain (k_tp_frame), for svo_debug_track_frames: cv::solvePnPRansac's outcome and pose
  int32_t pnp_best, pnp_iterations, pnp_inliers, pnp_ok;
  double T_pnp[16];
  int32_t hyp_done, pad_hyp;     // fused pose launch (k_tp_tail_ord): RANSAC samples of this frame that have stored their result
  long long hyp_early[TP_FLAGS]; // ... and, for the first TP_FLAGS samples, ONE word once that sample's result is stored: frame id + 1 in
                                 // the high half (ids only grow between two resets and a reset clears the records: a stale value never
                                 // equals the current one), the sample's ok << 31 | consensus in the low half - whoever sees the
                                 // announcement has the rule's inputs with it (tp_early_word)
  long long hyp_rt[TP_EARLY];    // diagnostics: s_memrealtime of an awaited sample just before it announced itself (-> rt[5])
};

struct TrackState {
  // ---- index chain -------------------------------------------------------------------------
  int32_t frame_num, npool, lastN, cur;      // cur: active half of the pool ping-pong
  int32_t next_gid, overflow, n_vetoed, n_boxes;
  int32_t epnp_fallbacks, pad_counters[3];   // RANSAC samples of the default solver that took its sequential fallback (sticky count)
  int32_t last_mp[TRK_MAXKP];
  int32_t dbg_cur_mp[TRK_MAXKP];
  svo_camera cam;
  int32_t boxes[SVO_MAX_BOXES * 4];    // {left, right, top, bottom} of the current frame
  double F[9];                         // fundamental matrix cur <- last (row-major)
  float last_xy[TRK_MAXKP * 2];        // LastFrame.keypoints_l[i].pt
  alignas(16) uint32_t last_desc[TRK_MAXKP * 8];   // LastFrame.f_descriptor
  int32_t bf_idx[TRK_MAXKP], bf_dist[TRK_MAXKP], bf_min;
  uint8_t bf_keep[TRK_MAXKP];
  // ---- pose chain --------------------------------------------------------------------------
  float lastTcw[16];
  double Xw[TRK_MAXKP * 3], obs[TRK_MAXKP * 2], K[4], Tprior[16], T[16];
  svo_lm_stats lm;
  svo_pnp_stats pnp;
  PnpHyp hyp[PNP_HYP];                 // the frame's RANSAC samples (k_tp_hyp)
  long long pose_ts[16];               // diagnostics: s_memtime stamps of k_tp_hyp (0..7) and k_tp_frame (8..15)
  // ---- large arrays (not cleared by a reset) -----------------------------------------------
  TrackPool pool[2];
  uint16_t rowmin[TRK_CAP];                // min over ALL current keypoints of the row's distances
  uint8_t ncand[TRK_CAP];                  // packed entries of the row, or TRK_DENSE
  uint32_t cand[(size_t)TRK_CAP * 2 * TRK_LCAP];   // packed entries, two words each (k_ti_lists), columns ascending
  uint16_t D[(size_t)TRK_CAP * 512];       // full distance rows (written for every row that has an entry)
  float gpos[(size_t)TRK_GPOS * 3];        // pose chain: world position of map point gid
};

// ---- block-wide exclusive scan (blockDim.x = 256 or 1024) -------------------------------------
// wave64 inclusive scan on DPP (gfx9 row shifts + row broadcasts): six dependent VALU steps, no LDS crossbar
__device__ __forceinline__ int tk_wave_incl_scan(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8  -> scan inside each row of 16
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15 into rows 1 and 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31 into rows 2 and 3
  return v;
}
__device__ __forceinline__ int block_excl_scan(int v, int* sm /*[16], 16-byte aligned*/, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int incl = tk_wave_incl_scan(v);
  const int nw = blockDim.x >> 6;
  __syncthreads();
  if (lane == 63) sm[wv] = incl;
  __syncthreads();
  const int4 a = reinterpret_cast<const int4*>(sm)[0], b = reinterpret_cast<const int4*>(sm)[1],
             c = reinterpret_cast<const int4*>(sm)[2], d = reinterpret_cast<const int4*>(sm)[3];
  const int t[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    off += w < wv ? t[w] : 0;
    tot += w < nw ? t[w] : 0;
  }
  *total = tot;
  return off + incl - v;
}

__device__ __forceinline__ void tk_unproject(const svo_camera& cam, float u, float v, float z,
                                             const float* Rwc, const float* twc, float* xyz) {
  const float x = (u - cam.cx) * z * (1 / cam.fx);
  const float y = (v - cam.cy) * z * (1 / cam.fy);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double acc = (double)Rwc[3 * r] * (double)x + (double)Rwc[3 * r + 1] * (double)y +
                       (double)Rwc[3 * r + 2] * (double)z;
    xyz[r] = (float)(acc + (double)twc[r]);
  }
}

// ---- hand-over index chain -> pose chain without stream events -----------------------------------------------------------
// The pose chain used to wait on one stream event per GROUP of frames (a wait costs ~3 us on the pose stream): whenever the
// index chain's lead shrank below a group - runs of frames whose passes need 30-47 rounds - the pose chain of frames
// g .. g + 3 stood still until frame g + 3 was matched (200-490 us per group, tools/gap_probe.py).  Now k_ti_resolve
// publishes every frame's record itself: all of its fields go out with agent-scope (sc1) stores, every thread waits for its
// own stores (s_waitcnt), and thread 0 then stores the frame's tag; the pose kernels are enqueued without any dependency on
// the index stream, poll the tag with an agent-scope load and read the record with agent-scope loads.  No release / acquire
// fence on either side: on gfx950 a release fence is buffer_wbl2 - a write-back of everything dirty in that XCD's L2, which
// holds the pyramid data of the front end running beside the tail - and sc1 accesses reach the device-coherent level by
// themselves.  The poll is bounded (~1 s): a lost hand-over sets the tracker's error flag instead of hanging the GPU.
__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ long long ld_agent(const long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(long long* p, long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#define TP_STORES_DONE() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
// work->hyp_early[k]: the frame's tag and the sample's outcome (ok << 31 | consensus) in one 8-byte word
__device__ __forceinline__ long long tp_early_word(int frame_tag, unsigned ok_cnt) { return (long long)(((unsigned long long)(unsigned)frame_tag << 32) | ok_cnt); }
__device__ __forceinline__ int tp_early_tag(long long w) { return (int)((unsigned long long)w >> 32); }
__device__ __forceinline__ int tp_early_cnt(long long w) { return (int)((unsigned)w & 0x7fffffffu); }
__device__ __forceinline__ int tp_early_ok(long long w) { return (int)(((unsigned)w >> 31) & 1u); }

// A gated frame's brute-force matches and F, solved ahead of the index chain (k_tg_bf_group / k_tg_fmat_group)
struct GatePre {
  int32_t bf_idx[TRK_MAXKP], bf_dist[TRK_MAXKP];
  double F[9];
};
