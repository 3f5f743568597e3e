// Tracking.h - per-frame orchestrator, mirrors the reference's include/Tracking.h.
#pragma once
#include <fstream>
#include <memory>
#include <set>
#include <string>

#include "frame.h"

class Tracking {
 public:
  // Reads Camera.fx/fy/cx/cy/bf from an ORB-SLAM2-format yaml (the only five keys the reference
  // consumes, src/Tracking.cc:22-40) and creates the GPU context.
  Tracking(const std::string& strSettingPath, int device = 0);
  // 0: sparse epipolar stereo (default); 1: the reference's live flow, a dense disparity map (libelas here,
  // MSA there) -> disp2Depth -> per-keypoint lookups (src/Tracking.cc:226-228)
  int depth_source = 0;   // 0 sparse matcher, 1 ELAS map, 2 MSA map, 3 SGBM map (svo_set_option "depth_source")
  // With depth_source 3 and the colour Track() / TrackBatch(bgr): SGBM on the colour pair (frame::ElasMatchBgr, svo_set_option
  // "sgbm_colour"), as the reference calls it; otherwise on the gray
  bool sgbm_colour = false;
  // With depth_source 3: SVO_SGBM_MODE_SGBM (0, the reference's) or SVO_SGBM_MODE_HH (1, eight directions; svo_set_option "sgbm_mode")
  int sgbm_mode = 0;
  // The dynamic-keypoint loop of src/Tracking.cc:189-223 (commented out there): before featuredetect, the last frame's
  // DY_keypoints are followed into the current left image (frame::LKTrack), the status-0 points erased, the survivors become
  // the current frame's DY_keypoints.  Seeds - keypoints strictly inside a box, offline_box in place of the reference's online
  // `boxes` - are collected where the commented lines have them: init() (src/Tracking.cc:70-85) and frame::createmappoint
  // while id <= 1 (src/frame.cc:209-222).  After Track() the frame's list is lastframe.DY_keypoints.  Track() only.
  bool dynamic_lk = false;
  // With dynamic_lk: run that loop on the colour left images (frame::LKTrackBgr), as the reference's call would - its leftimg
  // is the 8UC3 image.  Needs the colour Track(); the seeds and everything else are unchanged.
  bool dynamic_lk_bgr = false;
  // The same loop inside the device-resident tracker (svo_track_dynamic), for TrackBatch(): set before the first TrackBatch().
  // ctx_batch is configured before its reset, every call attaches storage of its own, and after FinishBatches() batched frame
  // k's list is batch_dynamic[k] (batch_dynamic_dropped[k]: seeds that did not fit into dynamic_max_pts; the host loop's lists
  // have no capacity).  dynamic_dev_bgr: on the colour left images (svo_dyn_params.colour = 1), needs TrackBatch(bgr = true).
  bool dynamic_dev = false, dynamic_dev_bgr = false;
  int dynamic_max_pts = 4096;
  std::vector<std::vector<svo_host::Point2f>> batch_dynamic;
  std::vector<int> batch_dynamic_dropped;
  // The map behind every tracked frame (svo_track_map_out): set before the first Track() / TrackBatch().  Observations(k) are
  // frame k's records - one per keypoint that has a map point when the frame ends (the reference's CurrentFrame->MapPoints[j] and
  // mappoint::worldpos, what View::DrawMappoints / DrawGraph read) -, in keypoint order, and ObservationOf(k, j) is keypoint j's
  // (null: no map point).  Both modes hand out the DEVICE-RESIDENT tracker's records, so a frame's map does not depend on the
  // mode: TrackBatch() arms the attachment for every call (complete after FinishBatches()); Track() feeds the same pair and boxes
  // to svo_track_frame[_bgr] on a context of its own, armed (complete when Track() returns) - the stage-by-stage classes' own
  // poses differ from the device tracker's in their last bits, and so would positions derived from them.
  bool map_out = false;
  const std::vector<svo_map_obs>& Observations(size_t frame_id) const;
  const svo_map_obs* ObservationOf(size_t frame_id, int kp) const;
  // Windowed bundle adjustment (svo_ba_window) over what map_out keeps for TrackBatch(): frames first_frame .. first_frame +
  // params.window - 1, their records (Observations) and their tracked poses (batch_results), after FinishBatches().  Returns
  // the window's refined poses (Tcw, window x 16 float64) and points; nothing feeds back into the tracker.
  struct LocalBAResult { std::vector<double> Tcw; std::vector<svo_ba_point> points; svo_ba_stats stats; };
  LocalBAResult LocalBA(size_t first_frame, const svo_ba_params& params);
  // Bag-of-words place recognition (svo_bow_*): loads a vocabulary in DBoW2's text format (trained on this library's descriptors:
  // tools/bow_train.py).  From then on the frame-by-frame Track() computes every frame's words, BowVector and FeatureVector from
  // frame::f_descriptor (svo_bow_transform, levelsup 4 as ORB-SLAM2's Frame::ComputeBoW) and keeps them: bow_vectors[k],
  // bow_features[k], bow_words[k].  LoopCandidates(k, gap, top_k) are the top_k (1 .. 16) best-scoring frames of 0 .. k - gap - 1
  // with a score above min_score (svo_bow_query_dev over the kept vectors).  Nothing feeds back into the tracker.  TrackBatch()
  // keeps no descriptors on the host: with a vocabulary loaded it throws.
  void LoadVocabulary(const std::string& path);
  // Loop verification (svo_loop_verify; ORB-SLAM2's ComputeSim3 for stereo): is cand_frame the place of frame_id, and where did
  // the camera stand?  SearchByBoW over the two frames' kept FeatureVectors (bow_features), then RANSAC over Horn's alignment of
  // the matched map points: KF1 = frame_id, KF2 = cand_frame, the result's T12 takes cand_frame's camera coordinates to
  // frame_id's.  Host to host from what Track() keeps per frame once a vocabulary is loaded and map_out is set: keypoints and
  // descriptors (loop_keypoints, loop_descriptors: the device tracker beside the classes extracts the same list, so an
  // Observations record's kp indexes them - checked on u, v), Observations and the device tracker's poses (map_poses, the world
  // Observations' positions live in).  match (may be null): per keypoint of frame_id the matched keypoint of cand_frame or -1.
  // Needs map_out and a vocabulary, throws otherwise.  Nothing feeds back into the tracker.
  svo_loop_result VerifyLoop(size_t frame_id, size_t cand_frame, const svo_loop_params& params, std::vector<int32_t>* match = nullptr);
  std::vector<std::vector<svo_kp>> loop_keypoints;
  std::vector<std::vector<uint8_t>> loop_descriptors;
  std::vector<std::vector<float>> map_poses;   // per tracked frame: svo_track_result.Tcw of Track()'s device tracker (map_out)
  std::vector<svo_bow_cand> LoopCandidates(size_t frame_id, int gap, int top_k, double min_score = 0.0);
  std::vector<std::vector<svo_bow_entry>> bow_vectors;
  std::vector<std::vector<svo_bow_feature>> bow_features;
  std::vector<std::vector<int32_t>> bow_words;
  // Raw (unrectified) input: reads LEFT.K / .D / .R / .P and RIGHT.* - or the flat Camera.k1 / k2 / p1 / p2 [/ k3] keys - of the
  // settings file (rect_settings.h), builds the maps on the device (svo_rect_create; the images' size is the context's) and
  // makes the left P's fx', fy', cx', cy' the tracker's camera (bf as the file has it).  From then on Track() rectifies every
  // pair first (svo_rect_process, gray or colour) and TrackBatch() does it on the device: the call's raw pairs go to device
  // buffers of its own, svo_rect_batch_dev(.., consumer = ctx_batch) writes one of two output sets and svo_track_batch_dev /
  // svo_track_batch_bgr_dev follows with no host synchronisation in between (not with dynamic_dev or map_out, whose arrays
  // belong to the host-fed entries).  Call it before the first frame.
  void LoadRectification(const std::string& strSettingPath);
  Tracking(const svo_camera& cam, int width, int height, int device = 0);
  ~Tracking();
  void init();                                                          // src/Tracking.cc:42-97
  // src/Tracking.cc:180-252 (imdepth / img_detect / Pangolin matrix arguments dropped: GUI only)
  void Track(const svo_host::GrayImage& imLeft, const svo_host::GrayImage& imRight, double timestamp,
             std::ofstream& f, std::ofstream& f2, const std::vector<std::vector<int>>& detection_box);
  // The same for the reference's own 8UC3 BGR input (main.cpp:160-161): the seams that take gray get the gray svo_bgr_to_gray
  // makes of it on the device (cv::ORB's COLOR_BGR2GRAY), frame::MBdense (depth_source 2) gets the colour.
  void Track(const svo_host::BgrImage& imLeft, const svo_host::BgrImage& imRight, double timestamp,
             std::ofstream& f, std::ofstream& f2, const std::vector<std::vector<int>>& detection_box);
  // The same loop PIPELINED (svo_track_batch_host): the next n stereo pairs of the sequence at once, images in host memory
  // (n x rows x stride bytes each side, frame k at L + k * rows * stride); returns at once - uploads, front end and the ordered
  // tail run behind the caller's back while it decodes the next pairs.  detection_box[k]: frame k's offline boxes (may be
  // empty).  FinishBatches() waits for everything and writes the trajectory rows of all batched frames in order
  // (SaveTrajectoryAndDraw's two formats).  Not to be mixed with Track() on one sequence.
  // bgr: the images are 8UC3 BGR, `stride` >= 3 * width (svo_track_batch_bgr_host).
  void TrackBatch(const uint8_t* L, const uint8_t* R, int stride, int n, const double* timestamps,
                  const std::vector<std::vector<std::vector<int>>>& detection_box, bool bgr = false);
  void FinishBatches(std::ofstream& f, std::ofstream& f2);
  void GetVelocity();                                                   // :99-106
  void Tracklastframe();                                                // :107-121
  void SaveTrajectoryAndDraw(std::ofstream& f, std::ofstream& f2);      // :124-144

 private:
  void MapFrame(const svo_host::GrayImage& imLeft, const svo_host::GrayImage& imRight, const svo_host::BgrImage* colLeft,
                const svo_host::BgrImage* colRight, double timestamp, const std::vector<std::vector<int>>& detection_box);
  void TrackBatchRectified(const uint8_t* L, const uint8_t* R, int stride, int n, const int32_t* flat, const int32_t* cnt, int most,
                           bool bgr, size_t first);
  void TrackImages(const svo_host::GrayImage& imLeft, const svo_host::GrayImage& imRight, const svo_host::BgrImage* colLeft,
                   const svo_host::BgrImage* colRight, double timestamp, std::ofstream& f, std::ofstream& f2,
                   const std::vector<std::vector<int>>& detection_box);

 public:
  svo_ctx* ctx = nullptr;
  svo_ctx* ctx_batch = nullptr;           // TrackBatch's context (max_batch = batch_capacity), made on first use
  int batch_capacity = 64;
  std::vector<svo_track_result> batch_results;   // one record per batched frame (stable storage: reserved for the sequence)
  std::vector<double> batch_timestamps;
  struct DynCall { std::vector<float> lists; std::vector<int32_t> counts, dropped; };   // one TrackBatch()'s svo_track_dynamic_out arrays
  std::vector<std::unique_ptr<DynCall>> batch_dyn_calls;                               // (complete after svo_sync: FinishBatches collects them)
  svo_rect* rect = nullptr;               // LoadRectification
  svo_bow* bow = nullptr;                 // LoadVocabulary (500 features a frame)
  svo_loop* loop = nullptr;               // VerifyLoop's verifier (500 keypoints a frame, one pair), made on first use
  svo_ba* ba = nullptr;                   // LocalBA's adjuster (500 records a frame, one window), made on first use
  struct RectBatch;                       // TrackBatch's device buffers behind the rectifier (Tracking.cc)
  RectBatch* rect_batch = nullptr;
  svo_ctx* ctx_map = nullptr;             // Track() with map_out: the device-resident tracker beside the classes (max_batch = 1)
  std::vector<std::vector<svo_map_obs>> observations;   // per tracked frame
  struct MapCall { std::vector<svo_map_obs> obs; std::vector<int32_t> counts; };       // one TrackBatch()'s svo_track_map_out arrays
  std::vector<std::unique_ptr<MapCall>> batch_map_calls;                               // (complete after svo_sync: FinishBatches collects them)
  int width = 0, height = 0;
  int device;
  frame lastframe;
  frame* currentframe = nullptr;
  int frame_num = 0;                      // static in the reference (one tracker per process)
  svo_camera K{};
  float bf = 0;
  std::set<mappoint*, mappoint_by_creation> LocalMapPoints;
  svo_host::Mat44f Velocity;
};

bool read_camera_yaml(const std::string& path, svo_camera& cam, int* width, int* height);
