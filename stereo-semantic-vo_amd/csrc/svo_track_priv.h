// svo_track_priv.h - host-side declarations shared by the tracker's units only (svo_track.hip: the kernels of the two chains and
// tail_enqueue; svo_track_dyn.hip, svo_track_map.hip: the two attachments; svo_track_entries.hip, svo_track_shard.hip,
// svo_track_debug.hip: the entry points).  What other modules call is in svo_internal.h.
#pragma once
#include <string.h>

#include "svo_track_state.h"

#pragma GCC visibility push(hidden)   // (nothing here is called from outside the library)

// ---- svo_track.hip ---------------------------------------------------------------------------------------------------------
// The alternating front-end output sets (ms_out, tb_out): n sets of keypoints, descriptors and counts for `images` image slots and
// depths - with `stereo_aux` also right x and SAD - for `pairs` pairs, K keypoints each.  A failed allocation leaves all n sets empty.
void fe_sets_free(SvoFeBufs* sets, int n);
int fe_sets_alloc(SvoFeBufs* sets, int n, size_t images, size_t pairs, size_t K, bool stereo_aux);
// streams, events, work records and the kernels' LDS opt-ins for `frames` frames per call of `nseq` sequences
int track_resources(svo_ctx* ctx, int frames, int nseq);
// the ordered tail for front-end results that are already in HBM (see its definition)
int tail_enqueue(svo_ctx* ctx, const svo_kp* kp, const uint8_t* desc8, const int32_t* nkp, const float* depth, int kstride, int frames,
                 int nseq, svo_track_result* d_res, const svo_boxes_dev* bx, const hipEvent_t* fe_events = nullptr,
                 const int* row_of_frame = nullptr, int work_half = 0, hipEvent_t idx_wait = nullptr, bool fe_elsewhere = false);

// ---- svo_track_entries.hip, svo_track_shard.hip ------------------------------------------------------------------------------
void track_stream_diag(svo_ctx* ctx);    // SVO_STREAM_DIAG=1: its table, once per context
void shard_gather_free(svo_ctx* ctx);    // svo_track_release's part of the sharded tracker
// at least n events in `ev` (created on the current device)
inline hipError_t track_events_reserve(std::vector<hipEvent_t>& ev, int n) {
  while ((int)ev.size() < n) {
    hipEvent_t e;
    const hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (rc != hipSuccess) return rc;
    ev.push_back(e);
  }
  return hipSuccess;
}

// ---- host outputs that wait in pinned memory -------------------------------------------------------------------------------
// svo_track_dynamic_out's lists and svo_track_map_out's records for HOST arrays cannot be written where the caller wants them
// while the call is in flight: they go to one of two pinned sets, which alternate between the calls that stage something, and
// a set is handed over to the caller's arrays (wait for its event, copy out) at exactly three moments:
//   1. svo_hostfeed_flush - svo_sync and the resets                                      (svo_track_host_out_flush);
//   2. before a direct entry, svo_track_frame[_bgr], returns                             (svo_track_host_out_flush);
//   3. when a host-fed call begins on the context, armed or not: every set that was staged two or more host-fed calls ago -
//      include/svo.h's "once the second following host-fed call has returned"            (svo_track_host_out_call_begins).
// A call that finds its set still occupied hands it over first.  The owner says only how a set is copied out.
struct HostStage {
  typedef void (*CopyOut)(svo_ctx* ctx, const uint8_t* set, void* const dst[3], int frames);
  CopyOut copy_out = nullptr;
  uint8_t* set[2] = {nullptr, nullptr};     // pinned
  hipEvent_t ev[2] = {nullptr, nullptr};    // behind the copies into set q
  void* dst[2][3] = {};                     // the caller's arrays set q is for
  int frames[2] = {0, 0};                   // frames in set q that wait for their hand-over (0: none)
  int staged_at[2] = {0, 0};                // `calls` when set q was staged
  int calls = 0;                            // host-fed calls begun on the context
  int next = 0, cur = 0;                    // the set the next staging call uses; the one the call being enqueued stages in
};
inline int stage_hand_over_set(svo_ctx* ctx, HostStage* S, int q) {
  if (!S->frames[q]) return SVO_OK;
  SVO_HIP(ctx, hipEventSynchronize(S->ev[q]));
  S->copy_out(ctx, S->set[q], S->dst[q], S->frames[q]);
  S->frames[q] = 0;
  return SVO_OK;
}
// every set staged `min_age` or more host-fed calls ago
inline int stage_hand_over(svo_ctx* ctx, HostStage* S, int min_age) {
  for (int q = 0; S && q < 2; ++q)
    if (S->calls - S->staged_at[q] >= min_age) { const int rc = stage_hand_over_set(ctx, S, q); if (rc) return rc; }
  return SVO_OK;
}
// a call that stages begins: S->set[S->cur] (`bytes` bytes) is its set
inline int stage_acquire(svo_ctx* ctx, HostStage* S, size_t bytes) {
  const int q = S->cur = S->next;
  S->next ^= 1;
  const int rc = stage_hand_over_set(ctx, S, q);
  if (rc) return rc;
  if (!S->set[q] && hipHostMalloc(reinterpret_cast<void**>(&S->set[q]), bytes) != hipSuccess) { (void)hipGetLastError(); return SVO_E_NOMEM; }
  if (!S->ev[q]) SVO_HIP(ctx, hipEventCreateWithFlags(&S->ev[q], hipEventDisableTiming));
  return SVO_OK;
}
// the copies into the call's set are enqueued on `s`: its first `frames` frames belong to the caller's arrays `dst`
inline int stage_commit(svo_ctx* ctx, HostStage* S, hipStream_t s, void* const dst[3], int frames) {
  const int q = S->cur;
  SVO_HIP(ctx, hipEventRecord(S->ev[q], s));
  memcpy(S->dst[q], dst, sizeof S->dst[q]);
  S->frames[q] = frames; S->staged_at[q] = S->calls;
  return SVO_OK;
}
// (what still waits is dropped)
inline void stage_free(HostStage* S) {
  for (int q = 0; q < 2; ++q) {
    if (S->set[q]) hipHostFree(S->set[q]);
    if (S->ev[q]) hipEventDestroy(S->ev[q]);
    S->set[q] = nullptr; S->ev[q] = nullptr; S->frames[q] = 0;
  }
}

// ---- svo_track_dyn.hip: the dynamic-keypoint loop as the entries and tail_enqueue see it ---------------------------------------
bool dyn_active(const svo_ctx* ctx);   // the loop is in force (adopted by the last reset)
bool dyn_colour(const svo_ctx* ctx);   // ... and tracks on the colour frames
HostStage* dyn_host_stage(svo_ctx* ctx);   // (nullptr: no such state)
void dyn_release(svo_ctx* ctx);
// the resets, every stream idle: svo_track_dynamic's parameters come into force, for svo_track_reset (multi_nseq = 0) or
// svo_track_multi_reset (its n_seq); the lists are empty
int dyn_adopt(svo_ctx* ctx, int multi_nseq);
int dyn_refuse_multi(svo_ctx* ctx, const char* who);   // the many-sequence entries while svo_track_reset adopted the loop
int dyn_colour_needs_bgr(svo_ctx* ctx, const char* who);
// A call of an entry that runs the loop: its left images (the loop's channels; consecutive images H * stride bytes apart) and
// where svo_track_dynamic_out's arrays live - `host`: host memory, `direct`: the entry synchronises before it returns
int dyn_begin(svo_ctx* ctx, const uint8_t* src, int stride, bool host, bool direct);
void dyn_end(svo_ctx* ctx);
bool dyn_in_call(const svo_ctx* ctx);
// the stream `s` is about to write the gray images anew that the loop of the previous call (or step) read
int dyn_wait_gray_read(svo_ctx* ctx, hipStream_t s);
// tail_enqueue, while dyn_in_call - on the index stream `s`; the loop's mode says whether the call is `frames` frames of one
// sequence or one step of n_seq sequences:
// behind frame f's k_ti_resolve (its work record, keypoints and boxes as the index kernels get them): the frame's / the step's seeds
void dyn_enqueue_seeds(svo_ctx* ctx, hipStream_t s, int f, const TrackWork* work, const svo_kp* kp, int kstride, const int32_t* boxes,
                       const int32_t* nboxes, int bstride);
// behind the ev_frame record of the group f0 .. f1 - 1: the LK steps of these frames / of this step
int dyn_enqueue_group(svo_ctx* ctx, hipStream_t s, int f0, int f1, bool boxes, const hipEvent_t* fe_events, int frames);
// behind the call's last pose launch: the lists go out, the pose stream joins the loop
int dyn_finish(svo_ctx* ctx, hipStream_t s, hipStream_t pose, int frames);

// ---- svo_track_map.hip: svo_track_map_out as the entries and tail_enqueue see it ------------------------------------------------
HostStage* map_host_stage(svo_ctx* ctx);   // (nullptr: no such state)
void map_release(svo_ctx* ctx);
void map_disarm(svo_ctx* ctx);             // the resets
int map_begin(svo_ctx* ctx, bool host);   // a call of an entry that delivers the records; `host`: svo_track_map_out's arrays are host memory
void map_end(svo_ctx* ctx);
bool map_in_call(const svo_ctx* ctx);
// tail_enqueue, while map_in_call (its arguments): k_tm_obs behind the call's last pose launch on `pose`
int map_enqueue(svo_ctx* ctx, hipStream_t pose, const TrackWork* work, const svo_kp* kp, const float* depth, int kstride, int frames,
                const int* row_of_frame);

#pragma GCC visibility pop
