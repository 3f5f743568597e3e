// svo_track_dyn.hip - the dynamic-keypoint loop inside the tracker (include/svo.h: svo_track_dynamic, svo_track_dynamic_out): its
// seed kernels, its state, and the hooks through which the entries (svo_track_entries.hip) and tail_enqueue (svo_track.hip) run it.
#include <algorithm>
#include <string>

#include "svo_track_priv.h"

// ================================================================================================
// A frame's seeds
// ================================================================================================
// One workgroup behind the frame's k_ti_resolve on the index stream, one thread per keypoint.  The seeds the reference pushes to
// DY_keypoints: Tracking::init (src/Tracking.cc:70-85, frame id 0) every keypoint strictly inside a box, then frame::createmappoint
// (src/frame.cc:209-222) every keypoint strictly inside a box that has no map point after both matching passes - not in the
// frame's correspondence list work->edge_kp[0 .. n_edges).  Both parts in keypoint order, the init part first, compacted by a
// block-wide prefix sum; at frame 0 an inside keypoint appears in both.
#define DYN_MAX_SEEDS (2 * TRK_MAXKP)
__device__ __forceinline__ void td_seeds_body(const TrackWork* __restrict__ work, const svo_kp* __restrict__ kp,
                                              const int32_t* __restrict__ boxes, const int32_t* __restrict__ nboxes,
                                              float* __restrict__ seeds, int32_t* __restrict__ n_seed) {
  __shared__ alignas(16) int sm[16];
  __shared__ int sbox[SVO_MAX_BOXES * 4];
  __shared__ uint8_t has_mp[TRK_MAXKP];
  const int tid = threadIdx.x;
  const int nkp = min(max(work->nkp, 0), TRK_MAXKP), n_edges = min(max(work->n_edges, 0), TRK_MAXKP);
  const int n_boxes = (boxes && nboxes) ? min(max(*nboxes, 0), SVO_MAX_BOXES) : 0;
  if (tid < 4 * n_boxes) sbox[tid] = boxes[tid];
  has_mp[tid] = 0;
  __syncthreads();
  if (tid < n_edges) {
    const int j = work->edge_kp[tid];
    if (j >= 0 && j < TRK_MAXKP) has_mp[j] = 1;
  }
  __syncthreads();
  bool inside = false;
  float x = 0.f, y = 0.f;
  if (tid < nkp) {
    x = kp[tid].x; y = kp[tid].y;
    for (int b = 0; b < n_boxes; ++b)
      inside = inside || (x > (float)sbox[4 * b] && x < (float)sbox[4 * b + 1] && y > (float)sbox[4 * b + 2] && y < (float)sbox[4 * b + 3]);
  }
  const bool s_init = inside && work->frame_id == 0, s_create = inside && !has_mp[tid];
  int n_init, n_create;
  const int o_init = block_excl_scan(s_init ? 1 : 0, sm, &n_init);
  const int o_create = n_init + block_excl_scan(s_create ? 1 : 0, sm, &n_create);
  if (s_init) { seeds[2 * o_init] = x; seeds[2 * o_init + 1] = y; }
  if (s_create) { seeds[2 * o_create] = x; seeds[2 * o_create + 1] = y; }   // (o_create < n_init + n_create <= 2 TRK_MAXKP)
  if (tid == 0) *n_seed = n_init + n_create;
}
__global__ __launch_bounds__(TRK_MAXKP) void k_td_seeds(const TrackWork* __restrict__ work, const svo_kp* __restrict__ kp,
                                                        const int32_t* __restrict__ boxes, const int32_t* __restrict__ nboxes,
                                                        float* __restrict__ seeds, int32_t* __restrict__ n_seed) {
  td_seeds_body(work, kp, boxes, nboxes, seeds, n_seed);
}
// Many sequences (svo_track_multi_step_dev): workgroup q = sequence q, behind the step's k_ti_resolve - its work record, keypoints
// and boxes where the many-sequence kernels find them (q records, q * kstride keypoints, q * bstride boxes further on), seed list
// q and seed count q.  A sequence without boxes (nboxes[q] == 0) writes count 0.
__global__ __launch_bounds__(TRK_MAXKP) void k_td_seeds_seqs(const TrackWork* __restrict__ work, const svo_kp* __restrict__ kp, int kstride,
                                                             const int32_t* __restrict__ boxes, const int32_t* __restrict__ nboxes,
                                                             int bstride, float* __restrict__ seeds, int32_t* __restrict__ n_seed) {
  const size_t q = blockIdx.x;
  td_seeds_body(work + q, kp + q * kstride, boxes + q * bstride * 4, nboxes + q, seeds + q * 2 * DYN_MAX_SEEDS, n_seed + q);
}

// ---- the dynamic-keypoint loop inside the tracker (svo_track_dynamic) ------------------------------------------------------
// list(f) = list(f - 1) tracked from left image f - 1 into left image f (k_lk_track) with the status-0 points erased, then the
// frame's seeds (k_td_seeds) while the list has room (k_lk_compact) - svo_lk_chain_dev's loop, driven here frame by frame on the
// INDEX stream: a group's seed kernels sit behind their k_ti_resolve; its track + compact steps - and, once per sub-batch of the
// front end, the level-0 copies, pyramids and derivatives of that sub-batch's left images - behind the group's ev_frame record,
// so the pose chain's wait is never behind LK work.  Everything of the loop is
// ordered by that one stream; the pose stream joins it once, at the end of a call (what svo_sync and the calls' result copies
// wait for then covers the lists).  The left images live in an arena of this state: a ring of slots in which slot `pos` is the
// previous frame - a later call never reads an earlier call's image buffers.
enum DynMode { DYN_NONE = 0, DYN_SINGLE, DYN_MULTI };   // which reset adopted the loop in force: svo_track_reset / svo_track_multi_reset
struct DynOut { float* lists = nullptr; int32_t *counts = nullptr, *dropped = nullptr; };
struct DynState {
  svo_dyn_params next{};        // svo_track_dynamic's: adopted by the next reset
  svo_dyn_params p{};           // in force
  bool active = false;
  DynMode mode = DYN_NONE;
  int cn = 1, top = 0, cap = 0, slots = 0, pos = 0;   // cap: frames per call; slots of the arena, `pos` holds the previous left image
  // many sequences (DYN_MULTI, see dyn_multi_step): cap = n_seq, the arena's 2 n_seq slots and the 2 n_seq lists are two halves that
  // alternate by step - `half` holds the previous step's left images and lists; d_ints: counts of half 0, counts of half 1, dropped,
  // seed counts, n_seq zeros (the seed counts of a step that cannot seed)
  int half = 0;
  hipEvent_t ev_img = nullptr;  // behind a step's copy of its left images into the arena (index stream)
  bool ev_img_valid = false;
  int built_until = 0;          // frames of the tail call being enqueued whose images, pyramids and derivatives are in the arena (slots pos + 1 ..)
  void* arena = nullptr;        // LkArena of its own (the context's serves svo_lk_*)
  float *d_lists = nullptr, *d_seeds = nullptr;   // (cap + 1) lists, list 0 = the last one of the call before; cap seed lists
  int32_t* d_ints = nullptr;    // cap + 1 counts, cap + 1 dropped, cap + 1 seed counts (the last one stays 0: a frame that cannot seed)
  hipEvent_t ev_lk = nullptr;   // behind a call's last LK step (index stream)
  bool ev_lk_valid = false;
  DynOut out; bool attached = false;              // svo_track_dynamic_out, for the next call
  // the call being enqueued
  bool in_call = false, cur_on = false, cur_host = false, cur_direct = false;
  DynOut cur; int cur_off = 0;
  const uint8_t* src = nullptr; int src_stride = 0;   // its left images, cn channels: image i at src + i * H * src_stride
  // lists for host arrays of the batched entries wait in pinned memory: a set is `cap` lists, then `cap` counts and `cap` dropped counts
  HostStage stage;
  float* h_lists() const { return reinterpret_cast<float*>(stage.set[stage.cur]); }
  int32_t* h_ints() const { return reinterpret_cast<int32_t*>(h_lists() + (size_t)cap * 2 * p.max_pts); }
  int32_t* counts() const { return d_ints; }
  int32_t* dropped() const { return d_ints + cap + 1; }
  int32_t* nseed() const { return d_ints + 2 * (cap + 1); }
  // DYN_MULTI's layout of d_ints (5 cap entries): counts of list half h, dropped, seed counts, zeros
  int32_t* m_counts(int h) const { return d_ints + (size_t)h * cap; }
  int32_t* m_dropped() const { return d_ints + 2 * (size_t)cap; }
  int32_t* m_nseed() const { return d_ints + 3 * (size_t)cap; }
  int32_t* m_zeros() const { return d_ints + 4 * (size_t)cap; }
};
static DynState* dyn_of(const svo_ctx* ctx) { return reinterpret_cast<DynState*>(ctx->dyn); }
bool dyn_active(const svo_ctx* ctx) { return ctx->dyn && dyn_of(ctx)->active; }
bool dyn_colour(const svo_ctx* ctx) { return dyn_active(ctx) && dyn_of(ctx)->p.colour != 0; }
bool dyn_in_call(const svo_ctx* ctx) { return dyn_active(ctx) && dyn_of(ctx)->in_call; }
HostStage* dyn_host_stage(svo_ctx* ctx) { return ctx->dyn ? &dyn_of(ctx)->stage : nullptr; }
static void dyn_free_buffers(DynState* D) {
  lk_arena_free(&D->arena);
  if (D->d_lists) hipFree(D->d_lists);
  if (D->d_seeds) hipFree(D->d_seeds);
  if (D->d_ints) hipFree(D->d_ints);
  D->d_lists = D->d_seeds = nullptr; D->d_ints = nullptr;
  stage_free(&D->stage);
  D->cap = 0; D->slots = 0;
}
void dyn_release(svo_ctx* ctx) {
  DynState* D = dyn_of(ctx);
  if (!D) return;
  dyn_free_buffers(D);
  if (D->ev_lk) hipEventDestroy(D->ev_lk);
  if (D->ev_img) hipEventDestroy(D->ev_img);
  delete D;
  ctx->dyn = nullptr;
}
// HostStage::CopyOut: whole lists, counts and dropped counts of the set's first n frames -> dst = {lists, counts, dropped or null}
static void dyn_copy_out(svo_ctx* ctx, const uint8_t* set, void* const dst[3], int n) {
  const DynState* D = dyn_of(ctx);
  const size_t mp = (size_t)D->p.max_pts;
  const int32_t* ints = reinterpret_cast<const int32_t*>(set + (size_t)D->cap * 2 * mp * sizeof(float));
  memcpy(dst[0], set, (size_t)n * 2 * mp * sizeof(float));
  memcpy(dst[1], ints, (size_t)n * sizeof(int32_t));
  if (dst[2]) memcpy(dst[2], ints + D->cap, (size_t)n * sizeof(int32_t));
}
// svo_track_reset (multi_nseq = 0) / svo_track_multi_reset (its n_seq), every stream idle: svo_track_dynamic's parameters come into
// force for that kind of reset, the lists are empty.  Everything is sized here, once: one sequence - max_batch frames per call and
// a ring of slots; many - the two halves of n_seq slots and lists
int dyn_adopt(svo_ctx* ctx, int multi_nseq) {
  DynState* D = dyn_of(ctx);
  if (!D) return SVO_OK;
  D->attached = false; D->in_call = false; D->ev_lk_valid = false; D->pos = 0; D->stage.next = 0;   // (the resets flushed the staging)
  D->ev_img_valid = false; D->half = 0;
  if (!D->next.enable) {
    if (D->active) dyn_free_buffers(D);
    D->active = false; D->mode = DYN_NONE; D->p = D->next;
    return SVO_OK;
  }
  const int W = ctx->g.W, H = ctx->g.H, cn = D->next.colour ? 3 : 1, top = lk_top_level(W, H, D->next.lk.maxLevel);
  const DynMode mode = multi_nseq > 0 ? DYN_MULTI : DYN_SINGLE;
  const bool many = mode == DYN_MULTI;
  const int cap = many ? multi_nseq : std::max(ctx->max_batch, 1), slots = many ? 2 * cap : std::min(cap, 64) + 1;
  const size_t n_ints = many ? 5 * (size_t)cap : 3 * (size_t)(cap + 1);
  if (!D->active || mode != D->mode || cn != D->cn || top != D->top || D->next.max_pts != D->p.max_pts || cap != D->cap) {
    dyn_free_buffers(D);
    D->active = false; D->mode = DYN_NONE;
    LkArena* A = nullptr;
    const size_t mp = (size_t)D->next.max_pts;
    int rc = lk_reserve_in(ctx, &D->arena, ctx->stream, W, H, cn, top, slots, many ? mp * cap : mp, slots, &A);
    if (rc) { dyn_free_buffers(D); return rc; }
    A->last = nullptr;   // (sized once: nothing ever grows it while work is in flight)
    const size_t n_lists = many ? 2 * (size_t)cap : (size_t)(cap + 1);
    if (hipMalloc(reinterpret_cast<void**>(&D->d_lists), n_lists * 2 * mp * sizeof(float)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&D->d_seeds), (size_t)cap * 2 * DYN_MAX_SEEDS * sizeof(float)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&D->d_ints), n_ints * sizeof(int32_t)) != hipSuccess) {
      (void)hipGetLastError();
      dyn_free_buffers(D);
      ctx->last_error = "svo_track_dynamic: device allocation failed";
      return SVO_E_NOMEM;
    }
    D->cn = cn; D->top = top; D->cap = cap; D->slots = slots;
    if (!D->ev_lk) SVO_HIP(ctx, hipEventCreateWithFlags(&D->ev_lk, hipEventDisableTiming));
    if (!D->ev_img) SVO_HIP(ctx, hipEventCreateWithFlags(&D->ev_img, hipEventDisableTiming));
  }
  D->p = D->next;
  SVO_HIP(ctx, hipMemsetAsync(D->d_ints, 0, n_ints * sizeof(int32_t), ctx->stream));   // (the caller waits for the stream)
  D->active = true; D->mode = mode;
  return SVO_OK;
}
// A tracker entry that runs the loop starts a call - frames of the one sequence in one or more tail calls, or a step of the
// sequences: its left images (cn channels, consecutive images H * stride bytes apart), and where svo_track_dynamic_out's arrays
// live (one-shot; `host`: host memory, `direct`: the entry synchronises before it returns)
int dyn_begin(svo_ctx* ctx, const uint8_t* src, int stride, bool host, bool direct) {
  DynState* D = dyn_of(ctx);
  D->in_call = true; D->src = src; D->src_stride = stride; D->cur_off = 0; D->built_until = 0;
  D->cur = D->out; D->cur_on = D->attached; D->cur_host = host; D->cur_direct = direct;
  D->attached = false; D->out = DynOut{};
  if (D->cur_on && host && !direct) {
    D->stage.copy_out = dyn_copy_out;
    const int rc = stage_acquire(ctx, &D->stage, (size_t)D->cap * (2 * D->p.max_pts * sizeof(float) + 2 * sizeof(int32_t)));
    if (rc == SVO_E_NOMEM) ctx->last_error = "svo_track_dynamic_out: out of pinned memory";
    if (rc) return rc;
  }
  return SVO_OK;
}
void dyn_end(svo_ctx* ctx) {
  DynState* D = dyn_of(ctx);
  D->in_call = false; D->cur_on = false; D->cur = DynOut{}; D->src = nullptr;
}
static bool dyn_can_seed(const DynState* D, int id) { return D->p.seed_frames < 0 || id < D->p.seed_frames; }
// frames f0 .. f1 - 1 of the tail call being enqueued (`frames` in all), whose index kernels (and seed kernels) are on `s`: track +
// compact frame by frame.  Images go into the arena, with their pyramids and derivatives, AHEAD of the steps: as far as the
// stream has already waited for the call's images - to the end of the front end's sub-batch (the next non-null fe_events entry),
// so that a sub-batch costs the index stream one set of launches, not one per group.  id0: frame 0 of the tail call counted
// from the reset
static int dyn_single_group(svo_ctx* ctx, DynState* D, hipStream_t s, int f0, int f1, int id0, bool boxes, const hipEvent_t* fe_events,
                            int frames) {
  LkArena* A = static_cast<LkArena*>(D->arena);
  const int W = ctx->g.W, H = ctx->g.H, cn = D->cn, mp = D->p.max_pts;
  const size_t row = (size_t)cn * W, img = row * H;
  size_t pyr_px, der_px;
  lk_slot_px(W, H, D->top, &pyr_px, &der_px);
  int f = f0;
  while (f < f1) {
    if (f >= D->built_until) {   // (every built frame has had its step: slot `pos` is frame f - 1)
      int e = f1;
      while (e < frames && !(fe_events && fe_events[e])) ++e;
      const int n = std::min(e - f, D->slots - 1);
      if (D->pos + n > D->slots - 1) {   // the ring is used up: the previous frame moves to slot 0
        const size_t q = (size_t)D->pos;
        SVO_HIP(ctx, hipMemcpyAsync(A->img, A->img + q * img, img, hipMemcpyDeviceToDevice, s));
        if (pyr_px) SVO_HIP(ctx, hipMemcpyAsync(A->pyr, A->pyr + q * cn * pyr_px, cn * pyr_px, hipMemcpyDeviceToDevice, s));
        SVO_HIP(ctx, hipMemcpyAsync(A->der, A->der + q * cn * der_px, cn * der_px * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        D->pos = 0;
      }
      const size_t first = (size_t)D->pos + 1;
      SVO_HIP(ctx, hipMemcpy2DAsync(A->img + first * img, row, D->src + (size_t)(D->cur_off + f) * H * D->src_stride, D->src_stride, row,
                                    (size_t)H * n, hipMemcpyDeviceToDevice, s));
      LkArena V = *A;   // the slots from `first` on
      V.pyr += first * cn * pyr_px; V.der += first * cn * der_px;
      lk_build(s, &V, cn, A->img + first * img, (int)row, img, W, H, D->top, n, 0, n);
      D->built_until = f + n;
    }
    for (const int stop = std::min(f1, D->built_until); f < stop; ++f) {
      const int id = id0 + f;
      const bool seeds = boxes && dyn_can_seed(D, id);
      if (id > 0)
        lk_launch_track(s, A, cn, A->img, (int)row, img, W, H, D->top, D->pos, 1, D->d_lists + (size_t)f * 2 * mp, D->counts() + f, 0, mp,
                        A->next, A->status, nullptr);
      lk_launch_compact(s, A->next, A->status, id > 0 ? D->counts() + f : nullptr, D->d_seeds + (size_t)f * 2 * DYN_MAX_SEEDS,
                        D->nseed() + (seeds ? f : D->cap), DYN_MAX_SEEDS, mp, D->d_lists + (size_t)(f + 1) * 2 * mp, D->counts() + f + 1,
                        D->dropped() + f + 1);
      ++D->pos;
    }
  }
  return SVO_OK;
}
// the end of a tail call of `frames` frames: its lists to the attached arrays, its last list to list 0, the pose stream joins
static int dyn_single_finish(svo_ctx* ctx, DynState* D, hipStream_t s, hipStream_t pose, int frames) {
  const size_t mp = (size_t)D->p.max_pts, off = (size_t)D->cur_off, n = (size_t)frames;
  if (D->cur_on) {
    const bool staged = D->cur_host && !D->cur_direct;
    float* lists = staged ? D->h_lists() : D->cur.lists;
    int32_t* counts = staged ? D->h_ints() : D->cur.counts;
    int32_t* dropped = staged ? D->h_ints() + D->cap : D->cur.dropped;
    const hipMemcpyKind kind = D->cur_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    SVO_HIP(ctx, hipMemcpyAsync(lists + off * 2 * mp, D->d_lists + 2 * mp, n * 2 * mp * sizeof(float), kind, s));
    SVO_HIP(ctx, hipMemcpyAsync(counts + off, D->counts() + 1, n * sizeof(int32_t), kind, s));
    if (dropped) SVO_HIP(ctx, hipMemcpyAsync(dropped + off, D->dropped() + 1, n * sizeof(int32_t), kind, s));
    if (staged) {
      void* const dst[3] = {D->cur.lists, D->cur.counts, D->cur.dropped};
      const int rc = stage_commit(ctx, &D->stage, s, dst, (int)(off + n));
      if (rc) return rc;
    }
  }
  SVO_HIP(ctx, hipMemcpyAsync(D->d_lists, D->d_lists + n * 2 * mp, 2 * mp * sizeof(float), hipMemcpyDeviceToDevice, s));
  SVO_HIP(ctx, hipMemcpyAsync(D->counts(), D->counts() + n, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  D->cur_off += frames; D->built_until = 0;
  SVO_HIP(ctx, hipEventRecord(D->ev_lk, s));
  SVO_HIP(ctx, hipStreamWaitEvent(pose, D->ev_lk, 0));
  D->ev_lk_valid = true;
  return SVO_OK;
}
// the entries that have no such loop refuse while it is enabled
int svo_track_dyn_refuse(svo_ctx* ctx, const char* who) {
  if (!dyn_active(ctx)) return SVO_OK;
  ctx->last_error = std::string(who) + ": the dynamic-keypoint loop is enabled on this context (svo_track_dynamic); this entry does not run it";
  return SVO_E_INVALID;
}
// The loop's state belongs to the kind of reset that adopted it (svo_track_reset and svo_track_multi_reset(1) are otherwise the
// same call): the entries of the other kind refuse in the same way
int svo_track_dyn_refuse_single(svo_ctx* ctx, const char* who) {
  if (!dyn_active(ctx) || dyn_of(ctx)->mode != DYN_MULTI) return SVO_OK;
  ctx->last_error = std::string(who) + ": the dynamic-keypoint loop on this context was adopted by svo_track_multi_reset; only the many-sequence entries run it";
  return SVO_E_INVALID;
}
int dyn_refuse_multi(svo_ctx* ctx, const char* who) {
  if (!dyn_active(ctx) || dyn_of(ctx)->mode == DYN_MULTI) return SVO_OK;
  return svo_track_dyn_refuse(ctx, who);   // (adopted by svo_track_reset: today's refusal, today's words)
}
// One step of the many-sequence loop, on the index stream `s` behind the step's ev_frame record (the pose chain's wait is never
// behind LK work): ONE 2-D copy of the n_seq left images into the arena half that is not the previous step's, one lk_build over
// them (their derivatives serve the NEXT step, when they are the previous images), one track launch over the n_seq pairs
// (previous half's slot q, this half's slot q) - none at id 0 -, one compact launch of n_seq workgroups.  Everything of the loop
// is ordered by this one stream, so step t + 1's copy into the half step t's track launch read as "previous" cannot overtake it,
// with or without "multi_pipeline".  `seeded`: the step's k_td_seeds_seqs ran (behind its k_ti_resolve).
static int dyn_multi_step(svo_ctx* ctx, DynState* D, hipStream_t s, int id, bool seeded) {
  LkArena* A = static_cast<LkArena*>(D->arena);
  const int W = ctx->g.W, H = ctx->g.H, cn = D->cn, mp = D->p.max_pts, nseq = D->cap;
  const size_t row = (size_t)cn * W, img = row * H;
  size_t pyr_px, der_px;
  lk_slot_px(W, H, D->top, &pyr_px, &der_px);
  const int prev = D->half, cur = prev ^ 1;
  const size_t first = (size_t)cur * nseq;
  SVO_HIP(ctx, hipMemcpy2DAsync(A->img + first * img, row, D->src, D->src_stride, row, (size_t)H * nseq, hipMemcpyDeviceToDevice, s));
  SVO_HIP(ctx, hipEventRecord(D->ev_img, s));   // (a colour step's gray staging may be written anew from here on)
  D->ev_img_valid = true;
  LkArena V = *A;   // this half's slots
  V.pyr += first * cn * pyr_px; V.der += first * cn * der_px;
  lk_build(s, &V, cn, A->img + first * img, (int)row, img, W, H, D->top, nseq, 0, nseq);
  int32_t *n_prev = D->m_counts(prev), *n_cur = D->m_counts(cur), *dropped = D->m_dropped(), *n_seed = D->m_nseed(), *zeros = D->m_zeros();
  float *l_prev = D->d_lists + (size_t)prev * nseq * 2 * mp, *l_cur = D->d_lists + (size_t)cur * nseq * 2 * mp;
  if (id > 0)
    lk_launch_track_seqs(s, A, cn, A->img, (int)row, img, W, H, D->top, prev * nseq, cur * nseq, nseq, l_prev, n_prev, mp, A->next, A->status);
  lk_launch_compact_seqs(s, nseq, A->next, A->status, id > 0 ? n_prev : nullptr, D->d_seeds, seeded ? n_seed : zeros, DYN_MAX_SEEDS, mp, l_cur,
                         n_cur, dropped);
  if (D->cur_on) {   // svo_track_dynamic_out: sequence q's list at lists + q * 2 max_pts, counts[q], dropped[q]
    SVO_HIP(ctx, hipMemcpyAsync(D->cur.lists, l_cur, (size_t)nseq * 2 * mp * sizeof(float), hipMemcpyDeviceToDevice, s));
    SVO_HIP(ctx, hipMemcpyAsync(D->cur.counts, n_cur, (size_t)nseq * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (D->cur.dropped) SVO_HIP(ctx, hipMemcpyAsync(D->cur.dropped, dropped, (size_t)nseq * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  }
  D->half = cur;
  SVO_HIP(ctx, hipEventRecord(D->ev_lk, s));   // (the pose stream joins behind the step's pose kernels: dyn_finish)
  D->ev_lk_valid = true;
  return SVO_OK;
}

// ---- tail_enqueue's hooks (svo_track_priv.h); the loop's mode says which kind of call this is -----------------------------------
void dyn_enqueue_seeds(svo_ctx* ctx, hipStream_t s, int f, const TrackWork* work, const svo_kp* kp, int kstride, const int32_t* boxes,
                       const int32_t* nboxes, int bstride) {
  DynState* D = dyn_of(ctx);
  if (!dyn_can_seed(D, ctx->track_frame + f)) return;
  if (D->mode == DYN_MULTI) {
    SvoTimer t(ctx, "k_td_seeds_seqs", s);
    hipLaunchKernelGGL(k_td_seeds_seqs, dim3(D->cap), dim3(TRK_MAXKP), 0, s, work, kp, kstride, boxes, nboxes, bstride, D->d_seeds, D->m_nseed());
  } else {
    SvoTimer t(ctx, "k_td_seeds", s);
    hipLaunchKernelGGL(k_td_seeds, dim3(1), dim3(TRK_MAXKP), 0, s, work, kp, boxes, nboxes, D->d_seeds + (size_t)f * 2 * DYN_MAX_SEEDS, D->nseed() + f);
  }
}
int dyn_enqueue_group(svo_ctx* ctx, hipStream_t s, int f0, int f1, bool boxes, const hipEvent_t* fe_events, int frames) {
  DynState* D = dyn_of(ctx);
  if (D->mode == DYN_MULTI) return dyn_multi_step(ctx, D, s, ctx->track_frame, boxes && dyn_can_seed(D, ctx->track_frame));
  return dyn_single_group(ctx, D, s, f0, f1, ctx->track_frame, boxes, fe_events, frames);
}
int dyn_finish(svo_ctx* ctx, hipStream_t s, hipStream_t pose, int frames) {
  DynState* D = dyn_of(ctx);
  if (D->mode != DYN_MULTI) return dyn_single_finish(ctx, D, s, pose, frames);
  SVO_HIP(ctx, hipStreamWaitEvent(pose, D->ev_lk, 0));
  return SVO_OK;
}
int dyn_wait_gray_read(svo_ctx* ctx, hipStream_t s) {
  if (!dyn_active(ctx) || dyn_of(ctx)->p.colour) return SVO_OK;
  DynState* D = dyn_of(ctx);
  if (D->mode == DYN_MULTI ? D->ev_img_valid : D->ev_lk_valid) SVO_HIP(ctx, hipStreamWaitEvent(s, D->mode == DYN_MULTI ? D->ev_img : D->ev_lk, 0));
  return SVO_OK;
}

int dyn_colour_needs_bgr(svo_ctx* ctx, const char* who) {
  ctx->last_error = std::string(who) + ": svo_track_dynamic asked for LK on the colour frames (colour = 1), which a gray entry does not have";
  return SVO_E_INVALID;
}

extern "C" int svo_dyn_default_params(svo_dyn_params* p) {
  if (!p) return SVO_E_INVALID;
  p->enable = 0;
  p->colour = 0;
  p->seed_frames = 2;
  p->max_pts = 512;
  return svo_lk_default_params(&p->lk);
}

// Checked on the host alone, in lk_check's order; in force from the next svo_track_reset on
extern "C" int svo_track_dynamic(svo_ctx* ctx, const svo_dyn_params* p) {
  if (!ctx || !p) return SVO_E_INVALID;
  int rc = SVO_OK;
  if (p->enable < 0 || p->enable > 1 || p->colour < 0 || p->colour > 1 || p->seed_frames < -1 || p->max_pts < 1) rc = SVO_E_INVALID;
  if (rc == SVO_OK) rc = lk_check(&p->lk, ctx->g.W, ctx->g.H, p->max_pts, 1);
  if (rc) {
    ctx->last_error = rc == SVO_E_CAPACITY ? "svo_track_dynamic: image larger than 4096 x 4096 or more than 4096 points"
                                           : "svo_track_dynamic: invalid argument or unsupported parameters";
    return rc;
  }
  if (!ctx->dyn) {
    if (!p->enable) return SVO_OK;   // (nothing to switch off)
    ctx->dyn = new DynState();
  }
  dyn_of(ctx)->next = *p;
  return SVO_OK;
}

extern "C" int svo_track_dynamic_out(svo_ctx* ctx, float* lists, int32_t* counts, int32_t* dropped) {
  if (!ctx || !lists || !counts) return SVO_E_INVALID;
  if (!dyn_active(ctx)) {
    ctx->last_error = "svo_track_dynamic_out: the dynamic-keypoint loop is not enabled (svo_track_dynamic, then svo_track_reset or svo_track_multi_reset)";
    return SVO_E_INVALID;
  }
  DynState* D = dyn_of(ctx);
  D->out.lists = lists; D->out.counts = counts; D->out.dropped = dropped;
  D->attached = true;
  return SVO_OK;
}

