#include "Tracking.h"

#include <algorithm>
#include <iomanip>
#include <sstream>
#include <stdexcept>

#include <hip/hip_runtime_api.h>

#include "Optimizer.h"
#include "convert.h"
#include "pnpmatch.h"
#include "rect_settings.h"

using namespace svo_host;

// cv::FileStorage stand-in: "Camera.fx: 718.856" style keys of Stereo/KITTI*.yaml
bool read_camera_yaml(const std::string& path, svo_camera& cam, int* width, int* height) {
  std::ifstream in(path);
  if (!in) return false;
  std::string line;
  int found = 0;
  while (std::getline(in, line)) {
    const size_t c = line.find(':');
    if (c == std::string::npos || line[0] == '#' || line[0] == '%') continue;
    const std::string key = line.substr(0, c);
    const double v = atof(line.c_str() + c + 1);
    if (key == "Camera.fx") { cam.fx = (float)v; ++found; }
    else if (key == "Camera.fy") { cam.fy = (float)v; ++found; }
    else if (key == "Camera.cx") { cam.cx = (float)v; ++found; }
    else if (key == "Camera.cy") { cam.cy = (float)v; ++found; }
    else if (key == "Camera.bf") { cam.bf = (float)v; ++found; }
    else if (key == "Camera.width" && width) *width = (int)v;
    else if (key == "Camera.height" && height) *height = (int)v;
  }
  return found == 5;
}

Tracking::Tracking(const std::string& strSettingPath, int dev) : device(dev) {
  int w = 1241, h = 376;
  if (!read_camera_yaml(strSettingPath, K, &w, &h)) throw std::runtime_error("bad settings file " + strSettingPath);
  bf = K.bf;
  if (svo_create(&ctx, device, w, h, 500, 1) != SVO_OK) throw std::runtime_error("svo_create failed (no GPU?)");
  width = w; height = h;
  Velocity = eye4();
}
Tracking::Tracking(const svo_camera& cam, int w, int h, int dev) : device(dev), K(cam), bf(cam.bf) {
  if (svo_create(&ctx, device, w, h, 500, 1) != SVO_OK) throw std::runtime_error("svo_create failed (no GPU?)");
  width = w; height = h;
  Velocity = eye4();
}
// TrackBatch behind the rectifier: the call's raw pairs, two sets of rectified pairs and boxes that alternate between calls (set p
// is rewritten behind read_done[p], recorded on the tracker's stream after the call that read it), one result array per call
struct Tracking::RectBatch {
  uint8_t* raw = nullptr; size_t raw_cap = 0;
  uint8_t* out[2] = {nullptr, nullptr}; size_t out_cap[2] = {0, 0};
  int32_t* boxes[2] = {nullptr, nullptr}; size_t box_cap[2] = {0, 0};
  hipEvent_t read_done[2] = {nullptr, nullptr};
  bool used[2] = {false, false};
  int parity = 0;
  struct Call { svo_track_result* d; size_t first; int n; };
  std::vector<Call> calls;
};

void Tracking::LoadRectification(const std::string& strSettingPath) {
  RectSettings s;
  std::string err;
  if (!read_rect_yaml(strSettingPath, s, err)) throw std::runtime_error("LoadRectification: " + strSettingPath + ": " + err);
  if (s.width != width || s.height != height) throw std::runtime_error("LoadRectification: the calibration's image size is not the tracker's");
  if (rect) svo_rect_destroy(rect);
  rect = nullptr;
  if (svo_rect_create(device, width, height, width, height, &s.left, &s.right, &rect) != SVO_OK)
    throw std::runtime_error(std::string("svo_rect_create: ") + svo_rect_last_error(nullptr));
  svo_rect_camera(rect, K.bf, &K);   // (bf: the value the constructor read)
  bf = K.bf;
}

static void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("TrackBatch (rectified): ") + what + ": " + hipGetErrorString(e));
}
template <typename T>
static void grow(T*& p, size_t& cap, size_t need) {   // (the caller has made sure nothing in flight uses p)
  if (need <= cap) return;
  if (p) (void)hipFree(p);
  p = nullptr; cap = 0;
  hip_check(hipMalloc(reinterpret_cast<void**>(&p), need * sizeof(T)), "hipMalloc");
  cap = need;
}

void Tracking::TrackBatchRectified(const uint8_t* L, const uint8_t* R, int stride, int n, const int32_t* flat, const int32_t* cnt, int most,
                                   bool bgr, size_t first) {
  if (!rect_batch) {
    rect_batch = new RectBatch();
    for (hipEvent_t& e : rect_batch->read_done) hip_check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
  }
  RectBatch& B = *rect_batch;
  hipStream_t rs = static_cast<hipStream_t>(svo_rect_stream(rect));
  const size_t row = (size_t)(bgr ? 3 : 1) * width, side = (size_t)n * height * row;
  const int p = B.parity;
  // the rectifier's stream: behind the tracker call that read set p two calls ago, then this call's uploads
  if (B.used[p]) hip_check(hipStreamWaitEvent(rs, B.read_done[p], 0), "hipStreamWaitEvent");
  if (2 * side > B.raw_cap || 2 * side > B.out_cap[p] || (size_t)n * (most * 4 + 1) > B.box_cap[p]) {
    hip_check(hipStreamSynchronize(rs), "hipStreamSynchronize");
    grow(B.raw, B.raw_cap, 2 * side);
    grow(B.out[p], B.out_cap[p], 2 * side);
    grow(B.boxes[p], B.box_cap[p], (size_t)n * (most * 4 + 1));
  }
  hip_check(hipMemcpy2DAsync(B.raw, row, L, stride, row, (size_t)n * height, hipMemcpyHostToDevice, rs), "upload");
  hip_check(hipMemcpy2DAsync(B.raw + side, row, R, stride, row, (size_t)n * height, hipMemcpyHostToDevice, rs), "upload");
  if (most > 0) {
    hip_check(hipMemcpyAsync(B.boxes[p], flat, (size_t)n * most * 4 * sizeof(int32_t), hipMemcpyHostToDevice, rs), "upload");
    hip_check(hipMemcpyAsync(B.boxes[p] + (size_t)n * most * 4, cnt, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, rs), "upload");
  }
  hip_check(hipStreamSynchronize(rs), "hipStreamSynchronize");   // (the caller refills its buffers when this returns)
  svo_track_result* d_res = nullptr;
  hip_check(hipMalloc(reinterpret_cast<void**>(&d_res), (size_t)n * sizeof(svo_track_result)), "hipMalloc");
  B.calls.push_back({d_res, first, n});
  if (svo_rect_batch_dev(rect, B.raw, B.raw + side, (int)row, bgr ? 3 : 1, n, B.out[p], B.out[p] + side, (int)row, ctx_batch) != SVO_OK)
    throw std::runtime_error(std::string("svo_rect_batch_dev: ") + svo_rect_last_error(rect));
  const svo_boxes_dev bd{B.boxes[p], B.boxes[p] + (size_t)n * most * 4, most};
  const int rc = (bgr ? svo_track_batch_bgr_dev : svo_track_batch_dev)(ctx_batch, B.out[p], B.out[p] + side, (int)row, n, most > 0 ? &bd : nullptr, d_res);
  if (rc != SVO_OK) throw std::runtime_error(std::string(bgr ? "svo_track_batch_bgr_dev: " : "svo_track_batch_dev: ") + svo_last_error(ctx_batch));
  hip_check(hipEventRecord(B.read_done[p], static_cast<hipStream_t>(svo_stream(ctx_batch))), "hipEventRecord");
  B.used[p] = true;
  B.parity ^= 1;
}

Tracking::~Tracking() {
  if (rect_batch) {
    if (ctx_batch) svo_sync(ctx_batch);
    for (auto& c : rect_batch->calls) (void)hipFree(c.d);
    for (int p = 0; p < 2; ++p) {
      if (rect_batch->out[p]) (void)hipFree(rect_batch->out[p]);
      if (rect_batch->boxes[p]) (void)hipFree(rect_batch->boxes[p]);
      if (rect_batch->read_done[p]) (void)hipEventDestroy(rect_batch->read_done[p]);
    }
    if (rect_batch->raw) (void)hipFree(rect_batch->raw);
    delete rect_batch;
  }
  if (rect) svo_rect_destroy(rect);
  if (ba) svo_ba_destroy(ba);
  if (bow) svo_bow_destroy(bow);
  if (loop) svo_loop_destroy(loop);
  if (ctx_batch) svo_destroy(ctx_batch);
  if (ctx_map) svo_destroy(ctx_map);
  svo_destroy(ctx);
}

void Tracking::TrackBatch(const uint8_t* L, const uint8_t* R, int stride, int n, const double* timestamps,
                          const std::vector<std::vector<std::vector<int>>>& detection_box, bool bgr) {
  if (n < 1) return;
  if (bow) throw std::runtime_error("TrackBatch: the pipelined mode keeps no descriptors on the host, so it has no bag of words (LoadVocabulary goes with Track())");
  if (n > batch_capacity) throw std::runtime_error("TrackBatch: more frames than batch_capacity");
  if (!ctx_batch) {
    if (svo_create(&ctx_batch, device, width, height, 500, batch_capacity) != SVO_OK) throw std::runtime_error("svo_create failed");
    if (svo_set_option(ctx_batch, "depth_source", depth_source) != SVO_OK || svo_set_option(ctx_batch, "sgbm_colour", sgbm_colour ? 1 : 0) != SVO_OK ||
        svo_set_option(ctx_batch, "sgbm_mode", sgbm_mode) != SVO_OK)
      throw std::runtime_error(std::string("TrackBatch: ") + svo_last_error(ctx_batch));
    if (dynamic_dev || dynamic_dev_bgr) {   // (before the reset: that is when the parameters come into force)
      svo_dyn_params dp;
      svo_dyn_default_params(&dp);
      dp.enable = 1; dp.colour = dynamic_dev_bgr ? 1 : 0; dp.max_pts = dynamic_max_pts;
      if (svo_track_dynamic(ctx_batch, &dp) != SVO_OK) throw std::runtime_error(std::string("TrackBatch: ") + svo_last_error(ctx_batch));
    }
    if (svo_track_reset(ctx_batch, &K) != SVO_OK) throw std::runtime_error(std::string("TrackBatch: ") + svo_last_error(ctx_batch));
    batch_results.reserve(1 << 16);   // (the library writes into this array until FinishBatches: it must not move)
  }
  const size_t first = batch_results.size();
  if (first + (size_t)n > batch_results.capacity()) {   // a longer sequence: complete what is in flight before the array moves
    if (svo_sync(ctx_batch) != SVO_OK) throw std::runtime_error(std::string("TrackBatch: ") + svo_last_error(ctx_batch));
    batch_results.reserve(2 * batch_results.capacity() + (size_t)n);
  }
  batch_results.resize(first + (size_t)n);
  for (int k = 0; k < n; ++k) batch_timestamps.push_back(timestamps ? timestamps[k] : 0.0);
  // the frames' boxes as the flat arrays svo_boxes_host wants (main.cpp:82-95: 4 ints per line, left right top bottom)
  int most = 0;
  for (int k = 0; k < n && k < (int)detection_box.size(); ++k) most = std::max(most, (int)detection_box[k].size());
  std::vector<int32_t> flat((size_t)n * std::max(most, 1) * 4, 0), cnt((size_t)n, 0);
  for (int k = 0; k < n && k < (int)detection_box.size(); ++k) {
    cnt[k] = (int32_t)detection_box[k].size();
    for (size_t b = 0; b < detection_box[k].size(); ++b)
      for (int j = 0; j < 4; ++j) flat[((size_t)k * most + b) * 4 + j] = detection_box[k][b][j];
  }
  const svo_boxes_host bx{flat.data(), cnt.data(), std::max(most, 1)};
  if (rect) {   // raw pairs: rectified on the device, then the device-resident entry
    if (dynamic_dev || dynamic_dev_bgr || map_out) throw std::runtime_error("TrackBatch: dynamic_dev / map_out are not available behind LoadRectification");
    TrackBatchRectified(L, R, stride, n, flat.data(), cnt.data(), most, bgr, first);
    frame_num += n;
    return;
  }
  if (dynamic_dev || dynamic_dev_bgr) {
    if (dynamic_dev_bgr && !bgr) throw std::runtime_error("Tracking::dynamic_dev_bgr needs TrackBatch(bgr = true)");
    batch_dyn_calls.emplace_back(new DynCall());
    DynCall& c = *batch_dyn_calls.back();
    c.lists.assign((size_t)n * 2 * dynamic_max_pts, 0.f); c.counts.assign((size_t)n, 0); c.dropped.assign((size_t)n, 0);
    if (svo_track_dynamic_out(ctx_batch, c.lists.data(), c.counts.data(), c.dropped.data()) != SVO_OK)
      throw std::runtime_error(std::string("svo_track_dynamic_out: ") + svo_last_error(ctx_batch));
  }
  if (map_out) {
    batch_map_calls.emplace_back(new MapCall());
    MapCall& c = *batch_map_calls.back();
    c.obs.assign((size_t)n * 500, svo_map_obs{}); c.counts.assign((size_t)n, 0);
    if (svo_track_map_out(ctx_batch, c.obs.data(), c.counts.data()) != SVO_OK)
      throw std::runtime_error(std::string("svo_track_map_out: ") + svo_last_error(ctx_batch));
  }
  const int rc = (bgr ? svo_track_batch_bgr_host : svo_track_batch_host)(ctx_batch, L, R, stride, n, most > 0 ? &bx : nullptr,
                                                                       batch_results.data() + first);
  if (rc != SVO_OK)
    throw std::runtime_error(std::string(bgr ? "svo_track_batch_bgr_host: " : "svo_track_batch_host: ") + svo_last_error(ctx_batch));
  frame_num += n;
}

void Tracking::FinishBatches(std::ofstream& f, std::ofstream& f2) {
  if (!ctx_batch) return;
  if (svo_sync(ctx_batch) != SVO_OK) throw std::runtime_error(std::string("FinishBatches: ") + svo_last_error(ctx_batch));
  if (rect_batch) {   // the rectified calls' records are in device memory
    hipStream_t rs = static_cast<hipStream_t>(svo_rect_stream(rect));
    for (auto& c : rect_batch->calls) {
      hip_check(hipMemcpyAsync(batch_results.data() + c.first, c.d, (size_t)c.n * sizeof(svo_track_result), hipMemcpyDeviceToHost, rs), "download");
      hip_check(hipStreamSynchronize(rs), "hipStreamSynchronize");
      (void)hipFree(c.d);
    }
    rect_batch->calls.clear();
  }
  for (const auto& c : batch_dyn_calls)   // (complete now: the lists of every batched frame, in order)
    for (size_t k = 0; k < c->counts.size(); ++k) {
      const Point2f* p = reinterpret_cast<const Point2f*>(c->lists.data() + k * 2 * (size_t)dynamic_max_pts);
      batch_dynamic.emplace_back(p, p + c->counts[k]);
      batch_dynamic_dropped.push_back(c->dropped[k]);
    }
  batch_dyn_calls.clear();
  for (const auto& c : batch_map_calls)   // (the same for the observations of every batched frame)
    for (size_t k = 0; k < c->counts.size(); ++k) observations.emplace_back(c->obs.begin() + k * 500, c->obs.begin() + k * 500 + c->counts[k]);
  batch_map_calls.clear();
  frame fr;   // SetPose's Rwc / twc arithmetic (src/frame.cc:66-73), SaveTrajectoryAndDraw's formats
  for (size_t k = 0; k < batch_results.size(); ++k) {
    Mat44f T;
    for (int i = 0; i < 16; ++i) T.m[i] = batch_results[k].Tcw[i];
    fr.SetPose(T);
    fr.timestamp = batch_timestamps[k];
    currentframe = &fr;
    SaveTrajectoryAndDraw(f, f2);
  }
  currentframe = nullptr;
}

const std::vector<svo_map_obs>& Tracking::Observations(size_t frame_id) const {
  if (frame_id >= observations.size()) throw std::runtime_error("Tracking::Observations: no such frame (map_out set? FinishBatches() called?)");
  return observations[frame_id];
}
Tracking::LocalBAResult Tracking::LocalBA(size_t first_frame, const svo_ba_params& params) {
  const int W = params.window;
  if (W < 2 || W > 8) throw std::runtime_error("Tracking::LocalBA: window must be 2 .. 8");
  if (first_frame + (size_t)W > observations.size() || first_frame + (size_t)W > batch_results.size())
    throw std::runtime_error("Tracking::LocalBA: no such frames (map_out set? TrackBatch() and FinishBatches() called?)");
  if (!ba && svo_ba_create(device, 500, 1, &ba) != SVO_OK) throw std::runtime_error(std::string("Tracking::LocalBA: ") + svo_ba_last_error(nullptr));
  std::vector<svo_map_obs> obs((size_t)W * 500, svo_map_obs{});
  std::vector<int32_t> counts((size_t)W, 0);
  std::vector<float> T((size_t)W * 16);
  for (int f = 0; f < W; ++f) {
    const std::vector<svo_map_obs>& o = observations[first_frame + f];
    std::copy(o.begin(), o.end(), obs.begin() + (size_t)f * 500);
    counts[f] = (int32_t)o.size();
    std::copy(batch_results[first_frame + f].Tcw, batch_results[first_frame + f].Tcw + 16, T.begin() + (size_t)f * 16);
  }
  LocalBAResult r;
  r.Tcw.assign((size_t)W * 16, 0.0);
  r.points.assign((size_t)W * 250, svo_ba_point{});
  int32_t n = 0;
  if (svo_ba_window(ba, &K, &params, obs.data(), counts.data(), 500, T.data(), r.Tcw.data(), r.points.data(), &n, &r.stats) != SVO_OK)
    throw std::runtime_error(std::string("Tracking::LocalBA: ") + svo_ba_last_error(ba));
  r.points.resize((size_t)n);
  return r;
}
void Tracking::LoadVocabulary(const std::string& path) {
  if (bow) { svo_bow_destroy(bow); bow = nullptr; }
  if (svo_bow_create_from_text(device, path.c_str(), 500, 1, &bow) != SVO_OK)
    throw std::runtime_error(std::string("Tracking::LoadVocabulary: ") + svo_bow_last_error(nullptr));
}
std::vector<svo_bow_cand> Tracking::LoopCandidates(size_t frame_id, int gap, int top_k, double min_score) {
  if (!bow) throw std::runtime_error("Tracking::LoopCandidates: no vocabulary (LoadVocabulary)");
  if (frame_id >= bow_vectors.size()) throw std::runtime_error("Tracking::LoopCandidates: no such frame (Track() called?)");
  if (top_k < 1 || top_k > 16) throw std::runtime_error("Tracking::LoopCandidates: top_k must be 1 .. 16");
  const size_t N = frame_id + 1, stride = 500;     // the frames up to the query, in the layout svo_bow_query_dev takes
  std::vector<svo_bow_entry> vec(N * stride, svo_bow_entry{});
  std::vector<int32_t> cnt(N);
  for (size_t f = 0; f < N; ++f) {
    std::copy(bow_vectors[f].begin(), bow_vectors[f].end(), vec.begin() + f * stride);
    cnt[f] = (int32_t)bow_vectors[f].size();
  }
  std::vector<svo_bow_cand> out((size_t)top_k);
  int32_t n = 0;
  uint8_t* d = nullptr;
  const size_t bv = vec.size() * sizeof(svo_bow_entry), bn = N * sizeof(int32_t), bc = out.size() * sizeof(svo_bow_cand);
  if (!svo_bow_stream(bow)) throw std::runtime_error(std::string("Tracking::LoopCandidates: ") + svo_bow_last_error(bow));
  if (hipMalloc(reinterpret_cast<void**>(&d), bv + bn + bc + 16) != hipSuccess) throw std::runtime_error("Tracking::LoopCandidates: out of device memory");
  uint8_t *d_n = d + bv, *d_c = d_n + ((bn + 15) & ~(size_t)15), *d_cn = d_c + bc;
  bool ok = hipMemcpy(d, vec.data(), bv, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d_n, cnt.data(), bn, hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && svo_bow_query_dev(bow, reinterpret_cast<svo_bow_entry*>(d), reinterpret_cast<int32_t*>(d_n), (int)stride, (int)N, (int)frame_id, 1,
                               gap, min_score, top_k, reinterpret_cast<svo_bow_cand*>(d_c), reinterpret_cast<int32_t*>(d_cn)) == SVO_OK;
  ok = ok && svo_bow_sync(bow) == SVO_OK && hipMemcpy(out.data(), d_c, bc, hipMemcpyDeviceToHost) == hipSuccess &&
       hipMemcpy(&n, d_cn, sizeof n, hipMemcpyDeviceToHost) == hipSuccess;
  (void)hipFree(d);
  if (!ok) throw std::runtime_error(std::string("Tracking::LoopCandidates: ") + svo_bow_last_error(bow));
  out.resize((size_t)n);
  return out;
}
svo_loop_result Tracking::VerifyLoop(size_t frame_id, size_t cand_frame, const svo_loop_params& params, std::vector<int32_t>* match) {
  if (!bow) throw std::runtime_error("Tracking::VerifyLoop: no vocabulary (LoadVocabulary)");
  if (!map_out) throw std::runtime_error("Tracking::VerifyLoop: needs map_out (set before the first Track())");
  const size_t have = std::min(std::min(loop_keypoints.size(), bow_features.size()), std::min(observations.size(), map_poses.size()));
  if (frame_id >= have || cand_frame >= have) throw std::runtime_error("Tracking::VerifyLoop: no such frame (Track() called?)");
  const size_t S = 500, fr[2] = {frame_id, cand_frame};
  std::vector<uint8_t> desc(2 * S * 32, 0);
  std::vector<svo_kp> kp(2 * S, svo_kp{});
  std::vector<svo_bow_feature> fv(2 * S, svo_bow_feature{});
  std::vector<svo_map_obs> obs(2 * S, svo_map_obs{});
  std::vector<float> Tcw(32);
  int32_t n[2], fv_n[2], obs_n[2];
  for (int s = 0; s < 2; ++s) {
    const size_t f = fr[s];
    const std::vector<svo_kp>& k = loop_keypoints[f];
    const std::vector<svo_map_obs>& o = observations[f];
    if (k.size() > S || bow_features[f].size() > S || o.size() > S) throw std::runtime_error("Tracking::VerifyLoop: more than 500 keypoints in a frame");
    for (const svo_map_obs& r : o)      // the device tracker's keypoint list is the classes': a record's kp names the same keypoint
      if (r.kp < 0 || (size_t)r.kp >= k.size() || k[(size_t)r.kp].x != r.u || k[(size_t)r.kp].y != r.v)
        throw std::runtime_error("Tracking::VerifyLoop: an observation does not name the kept keypoint");
    std::copy(k.begin(), k.end(), kp.begin() + s * S);
    std::copy(loop_descriptors[f].begin(), loop_descriptors[f].end(), desc.begin() + s * S * 32);
    std::copy(bow_features[f].begin(), bow_features[f].end(), fv.begin() + s * S);
    std::copy(o.begin(), o.end(), obs.begin() + s * S);
    std::copy(map_poses[f].begin(), map_poses[f].end(), Tcw.begin() + s * 16);
    n[s] = (int32_t)k.size(); fv_n[s] = (int32_t)bow_features[f].size(); obs_n[s] = (int32_t)o.size();
  }
  if (!loop && svo_loop_create(device, (int)S, 1, &loop) != SVO_OK)
    throw std::runtime_error(std::string("Tracking::VerifyLoop: ") + svo_loop_last_error(nullptr));
  std::vector<int32_t> m(S, -1);
  svo_loop_result r;
  if (svo_loop_verify(loop, &K, &params, desc.data(), kp.data(), n, (int)S, fv.data(), fv_n, obs.data(), obs_n, (int)S, Tcw.data(),
                      m.data(), &r, nullptr) != SVO_OK)
    throw std::runtime_error(std::string("Tracking::VerifyLoop: ") + svo_loop_last_error(loop));
  if (match) match->assign(m.begin(), m.begin() + n[0]);
  return r;
}
const svo_map_obs* Tracking::ObservationOf(size_t frame_id, int kp) const {
  const std::vector<svo_map_obs>& o = Observations(frame_id);   // (ascending kp)
  const auto it = std::lower_bound(o.begin(), o.end(), kp, [](const svo_map_obs& r, int j) { return r.kp < j; });
  return it != o.end() && it->kp == kp ? &*it : nullptr;
}

// Track() with map_out: the pair through svo_track_frame[_bgr] on ctx_map, armed - the colour pair where Track() was given one,
// as TrackBatch(bgr) would
void Tracking::MapFrame(const GrayImage& imLeft, const GrayImage& imRight, const BgrImage* colLeft, const BgrImage* colRight, double timestamp,
                        const std::vector<std::vector<int>>& detection_box) {
  if (!ctx_map) {
    if (svo_create(&ctx_map, device, width, height, 500, 1) != SVO_OK) throw std::runtime_error("svo_create failed");
    if (svo_set_option(ctx_map, "depth_source", depth_source) != SVO_OK || svo_set_option(ctx_map, "sgbm_colour", sgbm_colour ? 1 : 0) != SVO_OK ||
        svo_set_option(ctx_map, "sgbm_mode", sgbm_mode) != SVO_OK || svo_track_reset(ctx_map, &K) != SVO_OK)
      throw std::runtime_error(std::string("Tracking::map_out: ") + svo_last_error(ctx_map));
  }
  std::vector<int32_t> flat;
  for (const auto& b : detection_box)
    for (int j = 0; j < 4; ++j) flat.push_back(b[j]);
  std::vector<svo_map_obs> obs(500);
  int32_t count = 0;
  svo_track_result res;
  if (svo_track_map_out(ctx_map, obs.data(), &count) != SVO_OK) throw std::runtime_error(std::string("svo_track_map_out: ") + svo_last_error(ctx_map));
  const int nb = (int)detection_box.size();
  const int rc = colLeft ? svo_track_frame_bgr(ctx_map, colLeft->ptr(), colLeft->step(), colRight->ptr(), colRight->step(), timestamp,
                                               nb ? flat.data() : nullptr, nb, &res)
                         : svo_track_frame(ctx_map, imLeft.ptr(), imLeft.cols, imRight.ptr(), imRight.cols, timestamp, nb ? flat.data() : nullptr, nb, &res);
  if (rc != SVO_OK) throw std::runtime_error(std::string("Tracking::map_out: ") + svo_last_error(ctx_map));
  obs.resize((size_t)count);
  observations.push_back(std::move(obs));
  map_poses.emplace_back(res.Tcw, res.Tcw + 16);
}

void Tracking::init() {
  bool dynamic = false;   // declared outside the loop and never reset, exactly as src/Tracking.cc:44
  currentframe->SetPose(eye4());
  Velocity = eye4();
  const int n = (int)currentframe->keypoints_l.size();
  for (int i = 0; i < n && i < currentframe->N; ++i) {
    const float u = currentframe->keypoints_l[i].x, v = currentframe->keypoints_l[i].y;
    const float z = currentframe->kp_depth[i];
    for (const auto& b : currentframe->offline_box)
      if (u > b[0] - 5 && u < b[1] + 5 && v > b[2] - 5 && v < b[3] + 5) { dynamic = true; break; }
    if (currentframe->dynamic_lk)           // src/Tracking.cc:70-85 with offline_box for `boxes`: strictly inside seeds
      for (const auto& b : currentframe->offline_box)
        if (u > b[0] && u < b[1] && v > b[2] && v < b[3]) { currentframe->DY_keypoints.push_back(Point2f{u, v}); dynamic = true; break; }
    Vec3f x3D;
    if (z > 0 && !dynamic && currentframe->UnprojectStereo(u, v, z, x3D)) {
      mappoint* newmp = new mappoint(x3D, currentframe, i);
      newmp->AddObservation(currentframe, i);
      newmp->create_id = (int)currentframe->id;
      LocalMapPoints.insert(newmp);
      currentframe->MapPoints[i] = newmp;
    }
  }
}

void Tracking::GetVelocity() {
  // Velocity = Tcw * LastTwc (computed, never consumed - src/Tracking.cc:99-106)
  const Mat44f LastTwc = convert::R_t_to_Twc(lastframe.Rcw, lastframe.tcw);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double acc = 0;
      for (int k = 0; k < 4; ++k) acc += (double)currentframe->Tcw.at(r, k) * (double)LastTwc.at(k, c);
      Velocity.at(r, c) = (float)acc;
    }
}

void Tracking::Tracklastframe() {
  if (frame_num == 0) init();
  else pnpmatch::poseEstimationPnP(currentframe, lastframe, LocalMapPoints, Velocity, K);
  Optimizer::PoseOptimization(currentframe);
}

void Tracking::SaveTrajectoryAndDraw(std::ofstream& f, std::ofstream& f2) {
  const Mat33f& R = currentframe->Rwc;
  const std::vector<float> q = convert::toQuaternion(R);
  const Vec3f& t = currentframe->twc;
  if (f2.is_open())
    f2 << std::setprecision(6) << currentframe->timestamp << std::setprecision(7) << " " << t.at(0) << " "
       << t.at(1) << " " << t.at(2) << " " << q[0] << " " << q[1] << " " << q[2] << " " << q[3] << std::endl;
  if (f.is_open())
    f << std::setprecision(9) << R.at(0, 0) << " " << R.at(0, 1) << " " << R.at(0, 2) << " " << t.at(0) << " "
      << R.at(1, 0) << " " << R.at(1, 1) << " " << R.at(1, 2) << " " << t.at(1) << " " << R.at(2, 0) << " "
      << R.at(2, 1) << " " << R.at(2, 2) << " " << t.at(2) << std::endl;
}

void Tracking::Track(const GrayImage& imLeft, const GrayImage& imRight, double timestamp, std::ofstream& f,
                     std::ofstream& f2, const std::vector<std::vector<int>>& detection_box) {
  if (rect) {   // a raw pair: rectified first (svo_rect_process)
    if (imLeft.cols != width || imLeft.rows != height || imRight.cols != width || imRight.rows != height) throw std::runtime_error("Track: image size is not the calibration's");
    GrayImage rL, rR;
    rL.cols = rR.cols = width; rL.rows = rR.rows = height;
    rL.data.resize((size_t)width * height); rR.data.resize(rL.data.size());
    if (svo_rect_process(rect, imLeft.ptr(), imRight.ptr(), width, 1, rL.data.data(), rR.data.data(), width) != SVO_OK)
      throw std::runtime_error(std::string("svo_rect_process: ") + svo_rect_last_error(rect));
    TrackImages(rL, rR, nullptr, nullptr, timestamp, f, f2, detection_box);
    return;
  }
  TrackImages(imLeft, imRight, nullptr, nullptr, timestamp, f, f2, detection_box);
}

void Tracking::Track(const BgrImage& imLeft, const BgrImage& imRight, double timestamp, std::ofstream& f,
                     std::ofstream& f2, const std::vector<std::vector<int>>& detection_box) {
  BgrImage rL, rR;
  if (rect) {   // a raw colour pair: rectified first, all three channels (svo_rect_process, cn = 3)
    if (imLeft.cols != width || imLeft.rows != height || imRight.cols != width || imRight.rows != height) throw std::runtime_error("Track: image size is not the calibration's");
    rL.cols = rR.cols = width; rL.rows = rR.rows = height;
    rL.data.resize((size_t)3 * width * height); rR.data.resize(rL.data.size());
    if (svo_rect_process(rect, imLeft.ptr(), imRight.ptr(), 3 * width, 3, rL.data.data(), rR.data.data(), 3 * width) != SVO_OK)
      throw std::runtime_error(std::string("svo_rect_process: ") + svo_rect_last_error(rect));
  }
  // cv::ORB's own reduction (COLOR_BGR2GRAY, src/frame.cc:75-79), on the device
  GrayImage gL, gR;
  const BgrImage* in[2] = {rect ? &rL : &imLeft, rect ? &rR : &imRight};
  GrayImage* out[2] = {&gL, &gR};
  for (int s = 0; s < 2; ++s) {
    out[s]->cols = in[s]->cols; out[s]->rows = in[s]->rows;
    out[s]->data.resize((size_t)in[s]->cols * in[s]->rows);
    if (svo_bgr_to_gray(ctx, in[s]->ptr(), in[s]->cols, in[s]->rows, in[s]->step(), out[s]->data.data(), in[s]->cols) != SVO_OK)
      throw std::runtime_error(std::string("svo_bgr_to_gray: ") + svo_last_error(ctx));
  }
  TrackImages(gL, gR, in[0], in[1], timestamp, f, f2, detection_box);
}

void Tracking::TrackImages(const GrayImage& imLeft, const GrayImage& imRight, const BgrImage* colLeft, const BgrImage* colRight,
                           double timestamp, std::ofstream& f, std::ofstream& f2, const std::vector<std::vector<int>>& detection_box) {
  if (map_out) MapFrame(imLeft, imRight, colLeft, colRight, timestamp, detection_box);
  currentframe = new frame(ctx, imLeft, imRight, timestamp, K, detection_box);
  if (dynamic_lk) {                       // src/Tracking.cc:189-223: LK on the last list, erase by status, survivors -> DY_keypoints
    currentframe->dynamic_lk = true;      // (status and error live in the current frame here, in lastframe there)
    if (dynamic_lk_bgr) {
      if (!colLeft) throw std::runtime_error("Tracking::dynamic_lk_bgr needs the colour Track()");
      currentframe->leftimg_bgr = *colLeft;
      if (currentframe->LKTrackBgr(lastframe) < 0) throw std::runtime_error(std::string("svo_lk_track_bgr: ") + svo_last_error(ctx));
    } else if (currentframe->LKTrack(lastframe) < 0) throw std::runtime_error(std::string("svo_lk_track: ") + svo_last_error(ctx));
  }
  if (depth_source == 1) {                // src/Tracking.cc:225-228 literally: features, dense map, lookups
    currentframe->featuredetect(imLeft);
    currentframe->ElasMatch(imLeft, imRight);
    currentframe->computekeypoint_r();
    currentframe->disp2Depth(bf);
  } else if (depth_source == 2) {         // the same four calls with the reference's own MB body (MSA)
    currentframe->featuredetect(imLeft);
    if (colLeft) currentframe->MBdense(*colLeft, *colRight);
    else currentframe->MBdense(imLeft, imRight);
    currentframe->computekeypoint_r();
    currentframe->disp2Depth(bf);
  } else if (depth_source == 3) {         // the same four calls with the body of the reference's ElasMatch (SGBM)
    currentframe->featuredetect(imLeft);
    if (sgbm_colour && colLeft) currentframe->ElasMatchBgr(*colLeft, *colRight, sgbm_mode);
    else currentframe->SGBMMatch(imLeft, imRight, sgbm_mode);
    currentframe->computekeypoint_r();
    currentframe->disp2Depth(bf);
  } else {
    currentframe->MB(imLeft, imRight);    // featuredetect + stereo association in one device pass
    currentframe->computekeypoint_r();
    currentframe->disp2Depth(bf);
  }
  currentframe->id = frame_num;
  if (bow) {                              // this frame's words and vectors (ORB-SLAM2's Frame::ComputeBoW: levelsup 4)
    const int n = (int)std::min<size_t>(currentframe->keypoints_l.size(), 500);     // (f_descriptor keeps its capacity of N rows)
    std::vector<int32_t> w((size_t)n);
    std::vector<svo_bow_entry> v((size_t)n);
    std::vector<svo_bow_feature> fv((size_t)n);
    int32_t nv = 0, nf = 0;
    if (svo_bow_transform(bow, currentframe->f_descriptor.data(), n, 4, w.data(), v.data(), &nv, fv.data(), &nf) != SVO_OK)
      throw std::runtime_error(std::string("svo_bow_transform: ") + svo_bow_last_error(bow));
    v.resize((size_t)nv);
    fv.resize((size_t)nf);
    bow_words.push_back(std::move(w)); bow_vectors.push_back(std::move(v)); bow_features.push_back(std::move(fv));
    if (map_out) {                        // what VerifyLoop reads next to the FeatureVector
      loop_keypoints.emplace_back(currentframe->keypoints_l.begin(), currentframe->keypoints_l.begin() + n);
      loop_descriptors.emplace_back(currentframe->f_descriptor.begin(), currentframe->f_descriptor.begin() + (size_t)n * 32);
    }
  }
  Tracklastframe();
  SaveTrajectoryAndDraw(f, f2);
  if (frame_num > 0) GetVelocity();
  frame* prev = currentframe;
  lastframe = frame(currentframe);
  lastframe.createmappoint(LocalMapPoints);
  if (frame_num >= 4) {
    for (auto it = LocalMapPoints.begin(); it != LocalMapPoints.end();) {
      if ((*it)->create_id <= frame_num - 4) it = LocalMapPoints.erase(it);
      else ++it;
    }
  }
  // The reference leaks every frame (`new frame`, never deleted).  Map points key their
  // observations by the frame's ADDRESS, so the object must stay allocated for addresses to
  // remain unique; its payload (images, keypoints, descriptors) is released instead.
  prev->leftimg = GrayImage(); prev->rightimg = GrayImage(); prev->leftimg_bgr = BgrImage();
  std::vector<svo_kp>().swap(prev->keypoints_l);
  std::vector<uint8_t>().swap(prev->f_descriptor);
  std::vector<float>().swap(prev->keypoints_r);
  std::vector<float>().swap(prev->kp_disp);
  std::vector<float>().swap(prev->kp_depth);
  std::vector<mappoint*>().swap(prev->MapPoints);
  std::vector<float>().swap(prev->match_score);
  std::vector<bool>().swap(prev->inlier);
  std::vector<Point2f>().swap(prev->DY_keypoints);
  std::vector<Point2f>().swap(prev->LK_keypoints);
  currentframe = nullptr;
  frame_num++;
}
