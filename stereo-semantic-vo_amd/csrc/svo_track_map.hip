// svo_track_map.hip - each tracked frame's map points and observations (include/svo.h: svo_track_map_out): the kernel that writes a
// call's records, frame by frame, and the attachment as the entries (svo_track_entries.hip) and tail_enqueue (svo_track.hip) see it.
#include <algorithm>
#include <string>

#include "svo_track_priv.h"

// Workgroup f = frame f of the call, thread j = keypoint j.  Behind the call's last pose launch on the pose stream: every frame's
// pose launch has finished, so its record was published (the pose kernels waited for the tag) and the position table holds every
// point the call created.  The record is read the way the pose kernels read it - the index chain wrote it on another stream with
// agent-scope stores, and the XCDs' L2s are not coherent for plain loads: the tag first, then agent-scope loads; a record whose tag
// is not the frame's (a lost hand-over: the pose chain treated the frame as a PnP failure) gives count 0, never stale records.
// "matched" comes from the frame's correspondence list (edge_kp is ascending), "created" from new_gid - exactly one per keypoint -;
// a block-wide prefix sum puts the records in keypoint order, two 16-byte stores each.
__global__ __launch_bounds__(TRK_MAXKP) void k_tm_obs(const TrackState* __restrict__ st, const TrackWork* __restrict__ work,
                                                      const svo_kp* __restrict__ kp, const float* __restrict__ depth, int kstride,
                                                      int tag0, int max_kp, svo_map_obs* __restrict__ obs, int32_t* __restrict__ counts) {
  static_assert(sizeof(svo_map_obs) == 32, "svo_map_obs: two 16-byte stores");
  __shared__ alignas(16) int sm[16];
  __shared__ int mgid[TRK_MAXKP];
  const int f = blockIdx.x, tid = threadIdx.x;
  work += f; kp += (size_t)f * kstride; depth += (size_t)f * kstride; obs += (size_t)f * max_kp;
  const bool have = ld_agent(&work->ready) == tag0 + f;
  // (keypoints and depths were written with plain stores by front-end kernels on other streams: as in tp_wait_work)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const int nkp = have ? min(max(ld_agent(&work->nkp), 0), min(TRK_MAXKP, kstride)) : 0;
  const int n_edges = have ? min(max(ld_agent(&work->n_edges), 0), TRK_MAXKP) : 0;
  const int id = ld_agent(&work->frame_id);
  mgid[tid] = -1;
  __syncthreads();
  if (tid < n_edges) {
    const int j = ld_agent(&work->edge_kp[tid]);
    if (j >= 0 && j < TRK_MAXKP) mgid[j] = ld_agent(&work->edge_gid[tid]);
  }
  __syncthreads();
  int gid = -1;
  uint32_t flags = 0;
  if (tid < nkp) {
    gid = mgid[tid];
    if (gid >= 0) {
      flags = id == 0 ? (uint32_t)SVO_MAP_NEW : 0u;   // Tracking::init's points
    } else {
      gid = ld_agent(&work->new_gid[tid]);            // frame::createmappoint's
      flags = (uint32_t)SVO_MAP_NEW;
    }
  }
  int total;
  const int pos = block_excl_scan(gid >= 0 ? 1 : 0, sm, &total);
  if (gid >= 0 && pos < max_kp) {
    const svo_kp k = kp[tid];
    const float* gp = st->gpos + 3 * (size_t)(gid & (TRK_GPOS - 1));
    uint4 a, b;
    a.x = (uint32_t)gid; a.y = (uint32_t)tid | (flags << 16); a.z = __float_as_uint(k.x); a.w = __float_as_uint(k.y);
    b.x = __float_as_uint(depth[tid]); b.y = __float_as_uint(gp[0]); b.z = __float_as_uint(gp[1]); b.w = __float_as_uint(gp[2]);
    uint4* dst = reinterpret_cast<uint4*>(obs + pos);
    dst[0] = a; dst[1] = b;
  }
  if (tid == 0) counts[f] = min(total, max_kp);
}

// ---- each tracked frame's map points and observations (svo_track_map_out) ---------------------------------------------------
// A one-shot attachment like svo_track_dynamic_out, without state of its own: ONE launch (k_tm_obs) of one
// workgroup per frame behind the call's last pose launch on the pose stream, which reads what the call left in HBM anyway - the
// frames' work records (edge list, new_gid), the call's keypoint and depth arrays, the position table - and writes the records in
// keypoint order.  On the pose stream, inside tail_enqueue: every event that lets a later call's index chain rewrite this half of
// the work records or this front-end output set (ev_frontend at the next call's start, tb_done[p] / the callers' own events behind
// tail_enqueue) is recorded on that stream after it.  Host destinations (svo_track_frame, the _host entries): the kernel writes
// staging in HBM, a copy on the pose stream takes it to one of two pinned sets, and the hand-over (HostStage, svo_track_priv.h)
// gives each frame's counts[f] records to the caller's array.
struct MapOut { svo_map_obs* obs = nullptr; int32_t* counts = nullptr; };
struct MapState {
  MapOut out; bool attached = false;        // svo_track_map_out, for the next call
  // the call being enqueued
  bool in_call = false, cur_host = false;
  MapOut cur; int cur_off = 0;
  // host destinations: staging in HBM for `cap` frames; a pinned set is `cap` frames of max_kp records, then `cap` counts
  int cap = 0;
  svo_map_obs* d_obs = nullptr; int32_t* d_counts = nullptr;
  HostStage stage;
};
static MapState* map_of(const svo_ctx* ctx) { return reinterpret_cast<MapState*>(ctx->map); }
bool map_in_call(const svo_ctx* ctx) { return ctx->map && map_of(ctx)->in_call; }
HostStage* map_host_stage(svo_ctx* ctx) { return ctx->map ? &map_of(ctx)->stage : nullptr; }
void map_release(svo_ctx* ctx) {
  MapState* M = map_of(ctx);
  if (!M) return;
  if (M->d_obs) hipFree(M->d_obs);
  if (M->d_counts) hipFree(M->d_counts);
  stage_free(&M->stage);
  delete M;
  ctx->map = nullptr;
}
void map_disarm(svo_ctx* ctx) {
  if (MapState* M = map_of(ctx)) { M->attached = false; M->out = MapOut{}; M->in_call = false; }
}
// HostStage::CopyOut: counts[f] records of each of the set's first `frames` frames -> dst = {obs, counts}; what lies behind a
// frame's records in the caller's array stays as it is
static void map_copy_out(svo_ctx* ctx, const uint8_t* set, void* const dst[3], int frames) {
  const size_t K = (size_t)ctx->max_kp;
  const svo_map_obs* h_obs = reinterpret_cast<const svo_map_obs*>(set);
  const int32_t* h_counts = reinterpret_cast<const int32_t*>(h_obs + (size_t)map_of(ctx)->cap * K);
  for (int f = 0; f < frames; ++f) {
    const int n = std::min(std::max(h_counts[f], 0), ctx->max_kp);
    static_cast<int32_t*>(dst[1])[f] = n;
    memcpy(static_cast<svo_map_obs*>(dst[0]) + (size_t)f * K, h_obs + (size_t)f * K, (size_t)n * sizeof(svo_map_obs));
  }
}
// the entries that do not deliver it refuse while it is armed - and leave it armed
int svo_track_map_refuse(svo_ctx* ctx, const char* who) {
  if (!ctx->map || !map_of(ctx)->attached) return SVO_OK;
  ctx->last_error = std::string(who) + ": svo_track_map_out is armed on this context; this entry does not deliver map observations";
  return SVO_E_INVALID;
}
// A tracker entry that delivers the records starts a call; `host`: svo_track_map_out's arrays are host memory
int map_begin(svo_ctx* ctx, bool host) {
  MapState* M = map_of(ctx);
  if (!M || !M->attached) return SVO_OK;
  M->cur = M->out; M->cur_host = host; M->cur_off = 0;
  M->attached = false; M->out = MapOut{};
  if (host) {
    const size_t cap = (size_t)std::max(ctx->max_batch, 1), K = (size_t)ctx->max_kp;
    M->stage.copy_out = map_copy_out;
    int rc = stage_acquire(ctx, &M->stage, cap * (K * sizeof(svo_map_obs) + sizeof(int32_t)));
    if (rc == SVO_OK && !M->d_obs) {
      if (hipMalloc(reinterpret_cast<void**>(&M->d_obs), cap * K * sizeof(svo_map_obs)) != hipSuccess ||
          hipMalloc(reinterpret_cast<void**>(&M->d_counts), cap * sizeof(int32_t)) != hipSuccess) { (void)hipGetLastError(); rc = SVO_E_NOMEM; }
      M->cap = (int)cap;
    }
    if (rc == SVO_E_NOMEM) ctx->last_error = "svo_track_map_out: out of memory for the staging of host arrays";
    if (rc) return rc;
  }
  M->in_call = true;
  return SVO_OK;
}
void map_end(svo_ctx* ctx) {
  if (MapState* M = map_of(ctx)) { M->in_call = false; M->cur = MapOut{}; }
}
// the end of a tail call of `frames` frames (tail_enqueue's arguments): the launch behind the call's last pose launch on `pose`
int map_enqueue(svo_ctx* ctx, hipStream_t pose, const TrackWork* work, const svo_kp* kp, const float* depth, int kstride, int frames,
                const int* row_of_frame) {
  MapState* M = map_of(ctx);
  const size_t K = (size_t)ctx->max_kp, off = (size_t)M->cur_off;
  if (M->cur_host && off + (size_t)frames > (size_t)M->cap) {
    ctx->last_error = "svo_track_map_out: more frames than max_batch";
    return SVO_E_CAPACITY;
  }
  svo_map_obs* obs = (M->cur_host ? M->d_obs : M->cur.obs) + off * K;
  int32_t* counts = (M->cur_host ? M->d_counts : M->cur.counts) + off;
  const TrackState* st = reinterpret_cast<const TrackState*>(ctx->d_track);
  const int tag0 = ctx->track_frame + 1;   // k_ti_resolve's tag of the call's frame 0
  {
    SvoTimer t(ctx, "k_tm_obs", pose);
    if (!row_of_frame) {
      hipLaunchKernelGGL(k_tm_obs, dim3(frames), dim3(TRK_MAXKP), 0, pose, st, work, kp, depth, kstride, tag0, (int)K, obs, counts);
    } else {   // (front-end rows that are not the frames' order: a launch per frame)
      for (int f = 0; f < frames; ++f)
        hipLaunchKernelGGL(k_tm_obs, dim3(1), dim3(TRK_MAXKP), 0, pose, st, work + f, kp + (size_t)row_of_frame[f] * kstride,
                           depth + (size_t)row_of_frame[f] * kstride, kstride, tag0 + f, (int)K, obs + (size_t)f * K, counts + f);
    }
  }
  if (M->cur_host) {
    svo_map_obs* h_obs = reinterpret_cast<svo_map_obs*>(M->stage.set[M->stage.cur]);
    int32_t* h_counts = reinterpret_cast<int32_t*>(h_obs + (size_t)M->cap * K);
    SVO_HIP(ctx, hipMemcpyAsync(h_obs + off * K, M->d_obs + off * K, (size_t)frames * K * sizeof(svo_map_obs), hipMemcpyDeviceToHost, pose));
    SVO_HIP(ctx, hipMemcpyAsync(h_counts + off, M->d_counts + off, (size_t)frames * sizeof(int32_t), hipMemcpyDeviceToHost, pose));
    void* const dst[3] = {M->cur.obs, M->cur.counts, nullptr};
    const int rc = stage_commit(ctx, &M->stage, pose, dst, (int)off + frames);
    if (rc) return rc;
  }
  M->cur_off += frames;
  return SVO_OK;
}

extern "C" int svo_track_map_out(svo_ctx* ctx, svo_map_obs* obs, int32_t* counts) {
  if (!ctx || !obs || !counts) return SVO_E_INVALID;   // (host only: no device is touched before this)
  if (!ctx->d_track) {
    ctx->last_error = "svo_track_map_out: svo_track_reset first";
    return SVO_E_INVALID;
  }
  if ((reinterpret_cast<uintptr_t>(obs) & 15) || (reinterpret_cast<uintptr_t>(counts) & 3)) {
    ctx->last_error = "svo_track_map_out: obs must be 16-byte aligned, counts 4-byte aligned";
    return SVO_E_INVALID;
  }
  if (!ctx->map) ctx->map = new MapState();
  MapState* M = map_of(ctx);
  M->out.obs = obs; M->out.counts = counts;
  M->attached = true;
  return SVO_OK;
}
