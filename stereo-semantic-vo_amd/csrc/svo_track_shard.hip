// svo_track_shard.hip - the sharded tracker (include/svo.h: svo_track_sharded_dev; svo_track_sharded_fed for the host-fed entry).
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "svo_track_priv.h"

// --------------------------------------------------------------------------------------------
// ONE sequence over G GPUs in one process (BASELINE configs[3]): stereo pair k goes to context
// k mod G - the stateless front end (ORB on both images + sparse stereo) shards by pair with nothing to exchange - and
// the strict temporal chain (src/Tracking.cc:231-250) runs in frame order on context 0, which pulls every frame's
// ~34 KB of keypoints / descriptors / depths from where they were produced (device-to-device copies on its own
// stream, no collective, no host round trip).  d_grayL[g] / d_grayR[g]: the pairs of context g, on ITS device, in
// order of increasing k (local index k / G).  B frames per call, records into d_results (on context 0's device).
// Records are identical to svo_track_batch_dev on one context.  Does not synchronise.
struct ShardGather {
  // staging on the tail context's device: region g (frames g, g + G, ... of a call, `per` rows) holds what context g produced
  svo_kp* kp = nullptr; uint8_t* desc = nullptr; int32_t* n = nullptr; float* depth = nullptr;
  // TWO sets of staging rows (set p at row p * per * G): call c + 1 gathers into one while the tail of call c reads the other
  int per = 0, G = 0;
  std::vector<hipEvent_t> ev;         // front end (and staging copies) of context g finished; created ON context g's device
  std::vector<int> ev_dev;            //   (an event is recorded on a stream of its own device only) - that device
  hipEvent_t ev_prev = nullptr;       // what the tail context's stream held when the (first) call began
  hipStream_t gs = nullptr;           // the gather's own stream on the tail context's device (not the pose chain's)
  std::vector<hipEvent_t> ev_sub;     // sub-batch j of the latest call gathered (the index chain waits for it before the sub-batch's first frame)
  hipEvent_t ev_gathered = nullptr;   // the latest call's gather finished: the contexts' result buffers / the bounce buffer are free again
  hipEvent_t done[2] = {nullptr, nullptr};   // the pose chain finished with staging set / work half p
  bool used[2] = {false, false};
  int parity = 0;
  std::vector<svo_ctx*> producers;    // contexts whose shard_wait points at ev_gathered
  uint8_t* h_stage = nullptr;         // pinned bounce buffer for contexts whose device the tail's device cannot read directly
  size_t h_bytes = 0;
  std::vector<int> row_of_frame;
};
static std::vector<std::pair<svo_ctx*, ShardGather*>> g_gathers;   // per tail context, freed by svo_track_release
static std::mutex g_gathers_mu;                                      // contexts may live on different host threads

static ShardGather* shard_gather(svo_ctx* ctx) {
  std::lock_guard<std::mutex> lock(g_gathers_mu);
  for (auto& p : g_gathers)
    if (p.first == ctx) return p.second;
  g_gathers.emplace_back(ctx, new ShardGather());
  return g_gathers.back().second;
}
static void shard_gather_buffers_free(ShardGather* g) {
  if (g->kp) hipFree(g->kp);
  if (g->desc) hipFree(g->desc);
  if (g->n) hipFree(g->n);
  if (g->depth) hipFree(g->depth);
  g->kp = nullptr; g->desc = nullptr; g->n = nullptr; g->depth = nullptr;
  g->per = 0; g->G = 0;
}
void shard_gather_free(svo_ctx* ctx) {
  std::lock_guard<std::mutex> lock(g_gathers_mu);
  for (auto& pr : g_gathers) {   // a context that goes away is nobody's producer any more
    auto& v = pr.second->producers;
    v.erase(std::remove(v.begin(), v.end(), ctx), v.end());
  }
  ctx->shard_wait = nullptr;
  for (size_t i = 0; i < g_gathers.size(); ++i)
    if (g_gathers[i].first == ctx) {
      ShardGather* g = g_gathers[i].second;
      for (svo_ctx* pc : g->producers) if (pc->shard_wait == g->ev_gathered) pc->shard_wait = nullptr;
      shard_gather_buffers_free(g);
      for (hipEvent_t e : g->ev) hipEventDestroy(e);
      if (g->ev_prev) hipEventDestroy(g->ev_prev);
      if (g->ev_gathered) hipEventDestroy(g->ev_gathered);
      for (hipEvent_t e : g->ev_sub) hipEventDestroy(e);
      for (int q = 0; q < 2; ++q) if (g->done[q]) hipEventDestroy(g->done[q]);
      if (g->gs) { hipStreamSynchronize(g->gs); hipStreamDestroy(g->gs); }
      if (g->h_stage) hipHostFree(g->h_stage);
      delete g;
      g_gathers.erase(g_gathers.begin() + i);
      return;
    }
}

// What a sharded call left in flight and may still read of this context: as a producer, the gather of its result arrays (and of
// the bounce buffer); as the tail context, the pose chains of the last two calls (staging sets, work records) - other entry
// points of the context wait for them (svo_track_quiesce).
int svo_shard_quiesce(svo_ctx* ctx) {
  if (ctx->shard_wait) {
    hipEvent_t e = ctx->shard_wait;
    ctx->shard_wait = nullptr;
    SVO_HIP(ctx, hipEventSynchronize(e));
  }
  ShardGather* sg = nullptr;
  {
    std::lock_guard<std::mutex> lock(g_gathers_mu);
    for (auto& pr : g_gathers)
      if (pr.first == ctx) sg = pr.second;
  }
  if (sg)
    for (int q = 0; q < 2; ++q)
      if (sg->used[q] && sg->done[q]) SVO_HIP(ctx, hipEventSynchronize(sg->done[q]));
  return SVO_OK;
}

int svo_track_sharded_fed(svo_ctx* const* ctxs, int G, const uint8_t* const* d_grayL, const uint8_t* const* d_grayR, int stride, int B,
                          const svo_boxes_dev* boxes, svo_track_result* d_results, const hipEvent_t* const* pair_ready) {
  if (!ctxs || G < 1 || !d_grayL || !d_grayR || B < 1 || !d_results) return SVO_E_INVALID;
  svo_ctx* c0 = ctxs[0];
  if (!c0 || !c0->d_track || c0->n_seq != 1) return SVO_E_INVALID;   // svo_track_reset(ctxs[0]) first
  const int K = c0->max_kp;
  for (int g = 0; g < G; ++g) {
    if (!ctxs[g] || !d_grayL[g] || !d_grayR[g] || ctxs[g]->max_kp != K || ctxs[g]->g.W != c0->g.W || ctxs[g]->g.H != c0->g.H)
      return SVO_E_INVALID;
    if ((B - g + G - 1) / G > ctxs[g]->max_batch) return SVO_E_CAPACITY;
  }
  { const int rcd = svo_track_dyn_refuse(c0, "svo_track_sharded_dev"); if (rcd) return rcd; }
  { const int rcm = svo_track_map_refuse(c0, "svo_track_sharded_dev"); if (rcm) return rcm; }
  ShardGather* sg = shard_gather(c0);
  SVO_HIP(c0, hipSetDevice(c0->device));
  { const int rcf = svo_track_fe_batch_stream(c0); if (rcf) return rcf; }
  if (!sg->gs) {   // the gather's copies feed the tail sub-batch by sub-batch: beside its chains, and never behind the front end's grids
    int attempts = 0, percent = 0;
    const int rcp = svo_pick_stream(c0, [](hipStream_t* q) { return svo_stream_create(q, 0); }, {c0->stream, c0->stream_idx, c0->stream_fe_batch},
                                    &sg->gs, &attempts, &percent, {}, {c0->stream_fe_batch});
    if (rcp) return rcp;
  }
  if (!sg->ev_gathered) SVO_HIP(c0, hipEventCreateWithFlags(&sg->ev_gathered, hipEventDisableTiming));
  for (int q = 0; q < 2; ++q)
    if (!sg->done[q]) SVO_HIP(c0, hipEventCreateWithFlags(&sg->done[q], hipEventDisableTiming));
  const int per = (B + G - 1) / G;
  const size_t wk = sizeof(svo_kp) * (size_t)K, wd = 32 * (size_t)K, wf = 4 * (size_t)K;
  if (sg->per < per || sg->G < G) {
    SVO_HIP(c0, hipStreamSynchronize(sg->gs));
    if (c0->stream_idx) SVO_HIP(c0, hipStreamSynchronize(c0->stream_idx));
    SVO_HIP(c0, hipStreamSynchronize(c0->stream));
    shard_gather_buffers_free(sg);
    const size_t rows = (size_t)per * G * 2;
    if (hipMalloc(reinterpret_cast<void**>(&sg->kp), wk * rows) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&sg->desc), wd * rows) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&sg->n), 4 * rows) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&sg->depth), wf * rows) != hipSuccess) {
      (void)hipGetLastError();
      shard_gather_buffers_free(sg);
      return SVO_E_NOMEM;
    }
    sg->per = per; sg->G = G;
    sg->used[0] = sg->used[1] = false;
  }
  const int rper = sg->per;   // rows per region (may be larger than this call needs)
  const int G0 = sg->G;       // regions per set
  for (int g = 0; g < G; ++g) {
    if (g < (int)sg->ev.size() && sg->ev_dev[g] == ctxs[g]->device) continue;
    hipSetDevice(ctxs[g]->device);
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { hipSetDevice(c0->device); return SVO_E_HIP; }
    if (g < (int)sg->ev.size()) { hipEventDestroy(sg->ev[g]); sg->ev[g] = e; sg->ev_dev[g] = ctxs[g]->device; }
    else { sg->ev.push_back(e); sg->ev_dev.push_back(ctxs[g]->device); }
  }
  hipSetDevice(c0->device);
  if (!sg->ev_prev) SVO_HIP(c0, hipEventCreateWithFlags(&sg->ev_prev, hipEventDisableTiming));
  // How the tail's device reaches each producer's results: the same device, a direct peer read over xGMI (checked on every
  // call - the contexts of a call may change), or a bounce through pinned host memory when the platform offers no peer access.
  std::vector<int> direct(G, 1);
  bool need_stage = false;
  for (int g = 1; g < G; ++g) {
    if (ctxs[g]->device == c0->device) continue;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, c0->device, ctxs[g]->device) != hipSuccess) { can = 0; (void)hipGetLastError(); }
    if (can) {
      const hipError_t e = hipDeviceEnablePeerAccess(ctxs[g]->device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) can = 0;
      (void)hipGetLastError();
    }
    direct[g] = can;
    need_stage = need_stage || !can;
  }
  if (c0->opt_shard_force_staged) {   // test switch (SVO_SHARD_FORCE_STAGED at svo_create, or the option): the bounce path even where a direct read exists
    for (int g = 1; g < G; ++g) direct[g] = 0;
    need_stage = G > 1;
  }
  const size_t region_bytes = (wk + wd + wf + 4) * (size_t)rper;
  if (need_stage && sg->h_bytes < region_bytes * G) {
    SVO_HIP(c0, hipStreamSynchronize(sg->gs));
    SVO_HIP(c0, hipStreamSynchronize(c0->stream));
    if (sg->h_stage) hipHostFree(sg->h_stage);
    sg->h_stage = nullptr; sg->h_bytes = 0;
    if (hipHostMalloc(reinterpret_cast<void**>(&sg->h_stage), region_bytes * G, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return SVO_E_NOMEM; }   // (portable: every producer's device copies into it)
    sg->h_bytes = region_bytes * G;
  }
  // The pipeline over consecutive calls: the front ends of call c + 1 run while the tail of call c is in flight.  Nothing of a
  // front end sits on the pose chain's stream: context g > 0 uses its own stream (its own GPU), context 0 its front-end
  // stream (a share of the CUs, "fe_cu_percent", like svo_track_batch_dev); the gather runs on a stream of its own into the
  // staging set the tail of call c does not read.  A front end waits only for the previous call's GATHER (the last reader of
  // the context's result buffers and of the bounce buffer), the gather for the pose chain of call c - 1 (the last reader of
  // its staging set), the index chain for the gather.
  const int p = sg->parity;
  const bool first_call = !(sg->used[0] || sg->used[1]);
  if (first_call) SVO_HIP(c0, hipEventRecord(sg->ev_prev, c0->stream));   // after whatever the tail context's stream holds
  // A front end on the TAIL's device (context 0's; in tests and one-GPU runs every context's) runs on the context's CU-confined
  // front-end stream ("fe_cu_percent"), like svo_track_batch_dev's: on all CUs at the main stream's high priority it took the
  // tail's CUs (measured with two contexts on one GPU: 5.4 k frames/s against 8.1 k).  Every context works through its pairs in
  // sub-batches (its left images' results end up contiguous, row i = its pair i; a sub-batch's right images use the slots
  // behind it, which the next sub-batch overwrites - as in svo_track_batch_dev), so that the tail can start on the first
  // sub-batch while the rest of the call's front end still runs.
  // sub-batch j of every context: its pairs sub_off[j] .. sub_off[j + 1]; 8, 8, 16, then 32 at a time - the tail of a call that
  // finds the chip idle starts after 8 pairs per context instead of 32 (the confined stream takes ~50 us per pair)
  std::vector<int> sub_off(1, 0);
  while (sub_off.back() < per) {
    const int j = (int)sub_off.size() - 1;
    sub_off.push_back(std::min(per, sub_off.back() + (j < 2 ? 8 : j == 2 ? 16 : 32)));
  }
  const int nsub = (int)sub_off.size() - 1;
  std::vector<char> confined(G, 0);
  for (int g = 0; g < G; ++g) {
    svo_ctx* c = ctxs[g];
    hipSetDevice(c->device);
    if (track_events_reserve(c->ev_sub, nsub) != hipSuccess) { hipSetDevice(c0->device); return SVO_E_HIP; }
    if (c->device == c0->device) confined[g] = 1;   // ... on context 0's front-end stream, one context after the other: two
    // confined streams kept that share of the CUs busy without a gap, and the RANSAC workgroups the dispatcher places there
    // waited for room (pose chain 111 -> 147 us per frame with two contexts on one GPU)
  }
  hipSetDevice(c0->device);
  SVO_HIP(c0, track_events_reserve(sg->ev_sub, nsub));
  const size_t img = (size_t)c0->g.H * stride;
  int rc = SVO_OK;
  // sub-batch by sub-batch, every context's share of it (contexts on the tail's device share ONE stream: all of context 0's
  // sub-batches in front of context 1's first would hold the tail up for the whole of context 0's front end)
  std::vector<hipStream_t> fsv(G, nullptr);
  for (int g = 0; g < G && rc == SVO_OK; ++g) {
    svo_ctx* c = ctxs[g];
    if ((B - g + G - 1) / G <= 0) continue;
    hipSetDevice(c->device);
    { const int rcq = svo_track_quiesce(c, false); if (rcq) { hipSetDevice(c0->device); return rcq; } }   // (a batched call of this context may still read its result arrays; its own earlier calls are ordered by the stream waits below)
    fsv[g] = confined[g] ? c0->stream_fe_batch : c->stream;
    bool waited = false;   // (contexts that share a stream: one wait is enough)
    for (int q = 0; q < g; ++q) waited = waited || fsv[q] == fsv[g];
    if (!waited && hipStreamWaitEvent(fsv[g], first_call ? sg->ev_prev : sg->ev_gathered, 0) != hipSuccess) rc = SVO_E_HIP;
  }
  for (int j = 0; j < nsub && rc == SVO_OK; ++j) {
    for (int g = 0; g < G && rc == SVO_OK; ++g) {
      const int nb = (B - g + G - 1) / G;
      const int f0 = sub_off[j], b = std::min(sub_off[j + 1], nb) - f0;
      if (b <= 0) continue;
      svo_ctx* c = ctxs[g];
      hipStream_t fs = fsv[g];
      hipSetDevice(c->device);
      const SvoFeBufs fb = svo_fe_own(c).outputs_at(K, f0, f0);
      if (pair_ready && hipStreamWaitEvent(fs, pair_ready[g][f0 + b - 1], 0) != hipSuccess) rc = SVO_E_HIP;   // host-fed: this sub-batch's uploads (context g's copy stream, its device)
      if (rc == SVO_OK) rc = svo_launch_orb(c, fs, fb, d_grayL[g] + f0 * img, d_grayR[g] + f0 * img, stride, b, 2 * b);
      if (rc == SVO_OK) rc = svo_launch_stereo(c, fs, fb, d_grayL[g] + f0 * img, d_grayR[g] + f0 * img, stride, b, &c0->cam);
      if (rc == SVO_OK && !direct[g]) {
        // bounce, first half: this sub-batch's results into the context's region of the pinned buffer, on its own stream
        uint8_t* h = sg->h_stage + region_bytes * g;
        if (hipMemcpyAsync(h + wk * f0, fb.kp, wk * b, hipMemcpyDeviceToHost, fs) != hipSuccess ||
            hipMemcpyAsync(h + wk * rper + wd * f0, fb.desc, wd * b, hipMemcpyDeviceToHost, fs) != hipSuccess ||
            hipMemcpyAsync(h + (wk + wd) * rper + wf * f0, fb.depth, wf * b, hipMemcpyDeviceToHost, fs) != hipSuccess ||
            hipMemcpyAsync(h + (wk + wd + wf) * rper + 4 * (size_t)f0, fb.nkp, 4 * (size_t)b, hipMemcpyDeviceToHost, fs) != hipSuccess)
          rc = SVO_E_HIP;
      }
      if (rc == SVO_OK && hipEventRecord(c->ev_sub[j], fs) != hipSuccess) rc = SVO_E_HIP;
    }
  }
  hipSetDevice(c0->device);
  if (rc) { if (rc == SVO_E_HIP) c0->last_error = std::string("svo_track_sharded_dev: ") + hipGetErrorString(hipGetLastError()); return rc; }
  // gather on its own stream, sub-batch by sub-batch: rows of region g of staging set p <- context g's results
  const size_t set0 = (size_t)p * rper * G0;
  if (sg->used[p]) SVO_HIP(c0, hipStreamWaitEvent(sg->gs, sg->done[p], 0));
  std::vector<hipEvent_t> wait(B, nullptr);
  for (int j = 0; j < nsub; ++j) {
    bool any = false;
    for (int g = 0; g < G; ++g) {
      const int nb = (B - g + G - 1) / G;
      const int f0 = sub_off[j], b = std::min(sub_off[j + 1], nb) - f0;
      if (b <= 0) continue;
      any = true;
      svo_ctx* c = ctxs[g];
      SVO_HIP(c0, hipStreamWaitEvent(sg->gs, c->ev_sub[j], 0));
      const size_t r0 = set0 + (size_t)g * rper + f0;
      if (!direct[g]) {
        const uint8_t* h = sg->h_stage + region_bytes * g;
        SVO_HIP(c0, hipMemcpyAsync(sg->kp + r0 * K, h + wk * f0, wk * b, hipMemcpyHostToDevice, sg->gs));
        SVO_HIP(c0, hipMemcpyAsync(sg->desc + r0 * wd, h + wk * rper + wd * f0, wd * b, hipMemcpyHostToDevice, sg->gs));
        SVO_HIP(c0, hipMemcpyAsync(sg->depth + r0 * K, h + (wk + wd) * rper + wf * f0, wf * b, hipMemcpyHostToDevice, sg->gs));
        SVO_HIP(c0, hipMemcpyAsync(sg->n + r0, h + (wk + wd + wf) * rper + 4 * (size_t)f0, 4 * (size_t)b, hipMemcpyHostToDevice, sg->gs));
        continue;
      }
      const bool same = c->device == c0->device;
      auto pull = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
        return same ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, sg->gs)
                    : hipMemcpyPeerAsync(dst, c0->device, src, c->device, bytes, sg->gs);
      };
      SVO_HIP(c0, pull(sg->kp + r0 * K, c->d_kp + (size_t)f0 * K, wk * b));
      SVO_HIP(c0, pull(sg->desc + r0 * wd, c->d_desc + (size_t)f0 * wd, wd * b));
      SVO_HIP(c0, pull(sg->depth + r0 * K, c->d_depth + (size_t)f0 * K, wf * b));
      SVO_HIP(c0, pull(sg->n + r0, c->d_nkp + f0, 4 * (size_t)b));
    }
    if (!any) break;
    SVO_HIP(c0, hipEventRecord(sg->ev_sub[j], sg->gs));
    if (sub_off[j] * G < B) wait[(size_t)sub_off[j] * G] = sg->ev_sub[j];   // frames sub_off[j] G .. of the call need sub-batch j of every context
  }
  SVO_HIP(c0, hipEventRecord(sg->ev_gathered, sg->gs));
  // the ordered tail reads frame k = g + G i from row g * rper + i of set p; its index chain starts when the gather is done
  // (which came after the pose chain that last read this set and this half of the work records)
  sg->row_of_frame.resize(B);
  for (int k = 0; k < B; ++k) sg->row_of_frame[k] = (int)set0 + (k % G) * rper + k / G;
  rc = tail_enqueue(c0, sg->kp, sg->desc, sg->n, sg->depth, K, B, 1, d_results, boxes, wait.data(), sg->row_of_frame.data(), p,
                    nullptr, true);
  if (rc) return rc;
  SVO_HIP(c0, hipEventRecord(sg->done[p], c0->stream));   // the pose chain is the last reader of this set
  for (int g = 0; g < G; ++g) {
    ctxs[g]->shard_wait = sg->ev_gathered;
    if (std::find(sg->producers.begin(), sg->producers.end(), ctxs[g]) == sg->producers.end()) sg->producers.push_back(ctxs[g]);
  }
  sg->used[p] = true;
  sg->parity ^= 1;
  c0->track_frame += B;
  return SVO_OK;
}

extern "C" int svo_track_sharded_dev(svo_ctx* const* ctxs, int G, const uint8_t* const* d_grayL, const uint8_t* const* d_grayR,
                                     int stride, int B, const svo_boxes_dev* boxes, svo_track_result* d_results) {
  return svo_track_sharded_fed(ctxs, G, d_grayL, d_grayR, stride, B, boxes, d_results, nullptr);
}
