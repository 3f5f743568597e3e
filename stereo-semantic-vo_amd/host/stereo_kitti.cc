// stereo_kitti.cc - the reference's driver (main.cpp:100-210) over the MI355X front end.
// usage: stereo_kitti <vocabulary (ignored, as in the reference)> <settings.yaml> <sequence_dir>
// Sequence layout as main.cpp:20-57: times.txt, image_2/NNNNNN.png, image_3/NNNNNN.png (gray
// image_0/image_1 and .pgm are accepted too).  Writes cameratrajectory_kitti.txt / _tum.txt and
// prints the median / mean tracking time exactly like main.cpp:200-208.  No GUI, no pacing sleep,
// offline detection boxes: <sequence_dir>/boxes/<ni+1>.txt (optional; 4 ints per line,
// left right top bottom - main.cpp:82-95).
// stereo_kitti --pipelined <vocabulary> <settings.yaml> <sequence_dir> [frames per call, default 32]: the same sequence through
// Tracking::TrackBatch (svo_track_batch_host): this thread decodes the next frames while uploads, front end and ordered tail of
// the earlier ones run; same trajectory files; reports frames per second over the whole loop (decoding included).
// --colour (before the other arguments, with or without --pipelined): keep the images as 8UC3 BGR, as main.cpp:160-161 reads
// them, and track them through the colour entries (svo_track_frame_bgr's seams / svo_track_batch_bgr_host): the gray ORB sees is
// the same, MSA (depth_source 2) gets the colour.  Without it the files are reduced to gray on decode, as before.
// --dynamic-lk [--write-dynamic <dir>] (frame by frame only): Tracking::dynamic_lk, the reference's LK loop over the keypoints
// inside boxes (src/Tracking.cc:189-223); each frame's dynamic keypoints go to <dir>/NNNNNN.txt, one "x y" per line.
// --sgbm-colour (needs --colour and --depth-source 3): SGBM runs on the colour pair (cn = 3), as the reference's ElasMatch does.
// --sgbm-mode sgbm|hh (hh needs --depth-source 3): SGBM's five-direction single pass (the reference's MODE_SGBM, default) or all
// eight directions in two passes (MODE_HH).
// --dynamic-dev / --dynamic-dev-bgr (with --pipelined only): the same loop inside the device-resident tracker (svo_track_dynamic,
// Tracking::dynamic_dev), on gray or - needs --colour - on the colour left images; --write-dynamic writes the same files.
// --dynamic-lk-bgr (implies --dynamic-lk; needs --colour): the same loop on the colour left images, svo_lk_track_bgr.
// --bow <voc.txt> [--write-bow <dir>] [--loop-candidates <file> [--loop-gap G] [--loop-top K] [--loop-verify <file>]] (frame by
// frame; --loop-verify, with --write-map: every candidate through Tracking::VerifyLoop - matches, inliers, T12): bag-of-words place
// recognition (svo_bow_*) with a vocabulary trained on this library's descriptors (tools/bow_train.py); each frame's vectors and
// its best-scoring earlier frames.  The positional vocabulary argument stays ignored.
// --write-map <dir> / --write-cloud <file.ply> (any mode): each frame's map points and observations (svo_track_map_out,
// Tracking::map_out) to <dir>/NNNNNN.txt, "gid kp new u v depth X Y Z" per line; every new point of the run as an ASCII PLY.
// --rectify <settings.yaml> (any mode, gray and --colour): the sequence's images are RAW; the file's LEFT.* / RIGHT.* blocks (or its
// flat Camera.k1 .. p2 keys) are the calibration, Tracking::LoadRectification.  Frame by frame every pair goes through
// svo_rect_process first; --pipelined rectifies on the device in front of the device-resident tracker (not with --dynamic-dev /
// --write-map / --write-cloud).  It may be the settings file itself.
// stereo_kitti --decode-bgr in.(png|ppm|pgm) out.ppm: codec self-test of the colour decode (the PPM holds RGB, as the format says).
#include <algorithm>
#include <chrono>
#include <iomanip>
#include <iostream>
#include <sstream>

#include "Tracking.h"
#include "convert.h"
#include "png_reader.h"
#include "yolov3.h"

using namespace svo_host;

static bool exists(const std::string& p) { FILE* f = fopen(p.c_str(), "rb"); if (f) fclose(f); return f != nullptr; }

int main(int argc, char** argv) {
  if (argc == 4 && std::string(argv[1]) == "--decode") {   // image codec self-test: png/pgm -> pgm
    GrayImage img;
    if (!read_image(argv[2], img)) return 1;
    FILE* o = fopen(argv[3], "wb");
    if (!o) return 1;
    fprintf(o, "P5\n%d %d\n255\n", img.cols, img.rows);
    fwrite(img.data.data(), 1, img.data.size(), o);
    fclose(o);
    return 0;
  }
  if (argc == 4 && std::string(argv[1]) == "--decode-bgr") {   // colour codec self-test: png/ppm/pgm -> ppm
    BgrImage img;
    if (!read_image_bgr(argv[2], img)) return 1;
    FILE* o = fopen(argv[3], "wb");
    if (!o) return 1;
    fprintf(o, "P6\n%d %d\n255\n", img.cols, img.rows);
    std::vector<uint8_t> rgb(img.data);
    for (size_t i = 0; i < rgb.size(); i += 3) std::swap(rgb[i], rgb[i + 2]);
    fwrite(rgb.data(), 1, rgb.size(), o);
    fclose(o);
    return 0;
  }
  if (argc == 11 && std::string(argv[1]) == "--quat") {   // convert::toQuaternion self-test
    Mat33f R;
    for (int i = 0; i < 9; ++i) R.m[i] = (float)atof(argv[2 + i]);
    const std::vector<float> q = convert::toQuaternion(R);
    std::cout << std::fixed << std::setprecision(7) << q[0] << " " << q[1] << " " << q[2] << " " << q[3] << std::endl;
    return 0;
  }
  // --detect <cfg> <weights> [threshold] / --write-boxes <dir> (before the other arguments): take each frame's boxes from the
  // detector on the left image (the online mode of src/semantic.cc, YOLOv3::Detect(leftimg, 0.8)) instead of boxes/<n>.txt,
  // and / or write the boxes each frame used in the offline format (main.cpp:59-97: `left right top bottom` per line)
  std::string det_cfg, det_weights, write_dir;
  float det_thresh = 0.8f;
  for (int i = 1; i < argc;) {
    const std::string a = argv[i];
    int take = 0;
    if (a == "--detect" && i + 2 < argc) {
      det_cfg = argv[i + 1];
      det_weights = argv[i + 2];
      take = 3;
      char* end = nullptr;
      if (i + 3 < argc) {
        const float t = strtof(argv[i + 3], &end);
        if (end && *end == 0 && end != argv[i + 3]) { det_thresh = t; take = 4; }
      }
    } else if (a == "--write-boxes" && i + 1 < argc) {
      write_dir = argv[i + 1];
      take = 2;
    }
    if (!take) { ++i; continue; }
    for (int j = i; j + take < argc; ++j) argv[j] = argv[j + take];
    argc -= take;
  }
  YOLOv3 detector;
  if (!det_cfg.empty()) {
    try {
      detector.Create(det_weights, det_cfg, "");
    } catch (const std::exception& e) {
      std::cerr << e.what() << std::endl;
      return 1;
    }
  }
  bool colour = false;
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--colour") {
      colour = true;
      for (int j = i; j + 1 < argc; ++j) argv[j] = argv[j + 1];
      --argc;
      break;
    }
  int depth_source = 0;   // --depth-source N: 0 sparse matcher (default), 1 ELAS map, 2 MSA map, 3 SGBM map
  for (int i = 1; i + 1 < argc; ++i)
    if (std::string(argv[i]) == "--depth-source") {
      depth_source = atoi(argv[i + 1]);
      if (depth_source < 0 || depth_source > 3) { std::cerr << "--depth-source: 0 .. 3" << std::endl; return 1; }
      for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
      argc -= 2;
      break;
    }
  bool sgbm_colour = false;   // --sgbm-colour (needs --colour and --depth-source 3): SGBM on the 8UC3 pair, cn = 3
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--sgbm-colour") {
      sgbm_colour = true;
      for (int j = i; j + 1 < argc; ++j) argv[j] = argv[j + 1];
      --argc;
      break;
    }
  if (sgbm_colour && (!colour || depth_source != 3)) { std::cerr << "--sgbm-colour needs --colour and --depth-source 3" << std::endl; return 1; }
  int sgbm_mode = SVO_SGBM_MODE_SGBM;   // --sgbm-mode sgbm|hh (hh needs --depth-source 3)
  for (int i = 1; i + 1 < argc; ++i)
    if (std::string(argv[i]) == "--sgbm-mode") {
      const std::string m = argv[i + 1];
      if (m != "sgbm" && m != "hh") { std::cerr << "--sgbm-mode: sgbm or hh" << std::endl; return 1; }
      sgbm_mode = m == "hh" ? SVO_SGBM_MODE_HH : SVO_SGBM_MODE_SGBM;
      for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
      argc -= 2;
      break;
    }
  if (sgbm_mode == SVO_SGBM_MODE_HH && depth_source != 3) { std::cerr << "--sgbm-mode hh needs --depth-source 3" << std::endl; return 1; }
  // --dynamic-lk: Tracking::dynamic_lk (the reference's LK loop over the points inside boxes); --write-dynamic <dir>: each
  // frame's dynamic keypoints to <dir>/NNNNNN.txt, one "x y" per line (%.9g: the floats read back exactly)
  // --dynamic-dev / --dynamic-dev-bgr (with --pipelined): the same loop inside the device-resident tracker (Tracking::dynamic_dev)
  bool dynamic_lk = false, dynamic_lk_bgr = false, dynamic_dev = false, dynamic_dev_bgr = false;
  std::string dynamic_dir;
  for (int i = 1; i < argc;) {
    const std::string a = argv[i];
    int take = 0;
    if (a == "--dynamic-lk") { dynamic_lk = true; take = 1; }
    else if (a == "--dynamic-lk-bgr") { dynamic_lk = dynamic_lk_bgr = true; take = 1; }
    else if (a == "--dynamic-dev") { dynamic_dev = true; take = 1; }
    else if (a == "--dynamic-dev-bgr") { dynamic_dev = dynamic_dev_bgr = true; take = 1; }
    else if (a == "--write-dynamic" && i + 1 < argc) { dynamic_dir = argv[i + 1]; take = 2; }
    if (!take) { ++i; continue; }
    for (int j = i; j + take < argc; ++j) argv[j] = argv[j + take];
    argc -= take;
  }
  // --write-map <dir>: each frame's map points and observations (Tracking::map_out) to <dir>/NNNNNN.txt, one record per line
  // "gid kp new u v depth X Y Z" (%.9g: the floats read back exactly); --write-cloud <file.ply>: every record that is new in its
  // frame - each map point once, where it was created - as an ASCII PLY vertex list.  Frame by frame and --pipelined, gray and --colour.
  // --local-ba W [--ba-step S] [--ba-fixed F] (with --pipelined and --write-map): windowed bundle adjustment over the tracked
  // sequence (Tracking::LocalBA, svo_ba_window), one <dir>/ba_%06d.txt per window.
  std::string map_dir, cloud_file;
  int ba_window = 0, ba_step = 0, ba_fixed = 1;
  for (int i = 1; i < argc;) {
    const std::string a = argv[i];
    int take = 0;
    if (a == "--write-map" && i + 1 < argc) { map_dir = argv[i + 1]; take = 2; }
    else if (a == "--local-ba" && i + 1 < argc) { ba_window = atoi(argv[i + 1]); take = 2; }
    else if (a == "--ba-step" && i + 1 < argc) { ba_step = atoi(argv[i + 1]); take = 2; }
    else if (a == "--ba-fixed" && i + 1 < argc) { ba_fixed = atoi(argv[i + 1]); take = 2; }
    else if (a == "--write-cloud" && i + 1 < argc) { cloud_file = argv[i + 1]; take = 2; }
    if (!take) { ++i; continue; }
    for (int j = i; j + take < argc; ++j) argv[j] = argv[j + take];
    argc -= take;
  }
  const bool map_out = !map_dir.empty() || !cloud_file.empty();
  // --bow <voc.txt> (frame by frame): a vocabulary in DBoW2's text format (Tracking::LoadVocabulary; the positional vocabulary
  // argument stays ignored); --write-bow <dir>: each frame's words, BowVector and FeatureVector to <dir>/NNNNNN.txt - "n_features
  // n_words n_pairs", the words in one line, then "word value" (%.17g) per entry and "node feature" per pair;
  // --loop-candidates <file> [--loop-gap G, default 100] [--loop-top K, default 4]: per frame "frame count", then "frame score".
  // --loop-verify <file> (with --loop-candidates and --write-map): every candidate through Tracking::VerifyLoop with the default
  // parameters, one line each: "frame candidate status n_matches n_inliers" and T12's 16 values (%.17g)
  std::string bow_voc, bow_dir, loop_file, verify_file;
  int loop_gap = 100, loop_top = 4;
  for (int i = 1; i < argc;) {
    const std::string a = argv[i];
    int take = 0;
    if (a == "--bow" && i + 1 < argc) { bow_voc = argv[i + 1]; take = 2; }
    else if (a == "--write-bow" && i + 1 < argc) { bow_dir = argv[i + 1]; take = 2; }
    else if (a == "--loop-candidates" && i + 1 < argc) { loop_file = argv[i + 1]; take = 2; }
    else if (a == "--loop-verify" && i + 1 < argc) { verify_file = argv[i + 1]; take = 2; }
    else if (a == "--loop-gap" && i + 1 < argc) { loop_gap = atoi(argv[i + 1]); take = 2; }
    else if (a == "--loop-top" && i + 1 < argc) { loop_top = atoi(argv[i + 1]); take = 2; }
    if (!take) { ++i; continue; }
    for (int j = i; j + take < argc; ++j) argv[j] = argv[j + take];
    argc -= take;
  }
  std::string rectify;   // --rectify <settings.yaml>
  for (int i = 1; i + 1 < argc; ++i)
    if (std::string(argv[i]) == "--rectify") {
      rectify = argv[i + 1];
      for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
      argc -= 2;
      break;
    }
  bool pipelined = false;
  int per_call = 32;
  if (argc >= 5 && std::string(argv[1]) == "--pipelined") {
    pipelined = true;
    if (argc == 6) per_call = std::max(1, std::min(256, atoi(argv[5])));
    for (int i = 1; i < 4; ++i) argv[i] = argv[i + 1];
    argc = 4;
  }
  if (pipelined && dynamic_lk) {
    std::cerr << "--dynamic-lk / --dynamic-lk-bgr: frame by frame only (not with --pipelined, which has --dynamic-dev / --dynamic-dev-bgr)" << std::endl;
    return 1;
  }
  if (dynamic_dev && !pipelined) { std::cerr << "--dynamic-dev / --dynamic-dev-bgr need --pipelined (frame by frame: --dynamic-lk / --dynamic-lk-bgr)" << std::endl; return 1; }
  if (dynamic_lk_bgr && !colour) { std::cerr << "--dynamic-lk-bgr needs --colour" << std::endl; return 1; }
  if (dynamic_dev_bgr && !colour) { std::cerr << "--dynamic-dev-bgr needs --colour" << std::endl; return 1; }
  if (!dynamic_dir.empty() && !dynamic_lk && !dynamic_dev) {
    std::cerr << "--write-dynamic needs --dynamic-lk or, with --pipelined, --dynamic-dev" << std::endl;
    return 1;
  }
  if (!rectify.empty() && pipelined && (dynamic_dev || map_out)) {
    std::cerr << "--rectify with --pipelined: not with --dynamic-dev / --dynamic-dev-bgr / --write-map / --write-cloud" << std::endl;
    return 1;
  }
  if (!bow_voc.empty() && pipelined) {
    std::cerr << "--bow: frame by frame only (the pipelined mode keeps no descriptors on the host)" << std::endl;
    return 1;
  }
  if ((!bow_dir.empty() || !loop_file.empty()) && bow_voc.empty()) { std::cerr << "--write-bow / --loop-candidates need --bow" << std::endl; return 1; }
  if (!verify_file.empty() && (loop_file.empty() || map_dir.empty())) { std::cerr << "--loop-verify needs --loop-candidates and --write-map" << std::endl; return 1; }
  if (!bow_voc.empty() && (loop_gap < 0 || loop_top < 1 || loop_top > 16)) { std::cerr << "--loop-gap G: >= 0; --loop-top K: 1 .. 16" << std::endl; return 1; }
  if (ba_window && (!pipelined || map_dir.empty())) { std::cerr << "--local-ba needs --pipelined and --write-map" << std::endl; return 1; }
  if (ba_window && !ba_step) ba_step = ba_window;
  if (ba_window && (ba_window < 2 || ba_window > 8 || ba_fixed < 1 || ba_fixed >= ba_window || ba_step < 1)) {
    std::cerr << "--local-ba W: 2 .. 8; --ba-fixed F: 1 .. W - 1; --ba-step S: >= 1" << std::endl;
    return 1;
  }
  if (argc != 4) {
    std::cerr << "Usage: ./stereo_kitti [--rectify settings.yaml] [--detect cfg weights [threshold]] [--write-boxes dir] [--colour] [--depth-source 0..3] [--sgbm-colour] [--sgbm-mode sgbm|hh] [--dynamic-lk | --dynamic-lk-bgr | --dynamic-dev | --dynamic-dev-bgr] [--write-dynamic dir] [--write-map dir] [--write-cloud file.ply] [--pipelined] [--local-ba W [--ba-step S] [--ba-fixed F]] [--bow voc.txt [--write-bow dir] [--loop-candidates file [--loop-gap G] [--loop-top K] [--loop-verify file]]] path_to_vocabulary"
                 " path_to_settings path_to_sequence [frames_per_call]" << std::endl;
    return 1;
  }
  const std::string seq = argv[3];
  std::vector<double> vTimestamps;
  {
    std::ifstream fTimes(seq + "/times.txt");
    std::string s;
    while (std::getline(fTimes, s))
      if (!s.empty()) vTimestamps.push_back(atof(s.c_str()));
  }
  const int nImages = (int)vTimestamps.size();
  if (nImages == 0) { std::cerr << "no times.txt in " << seq << std::endl; return 1; }
  auto name = [&](const char* dir, int i, const char* ext) {
    std::stringstream ss;
    ss << seq << "/" << dir << "/" << std::setfill('0') << std::setw(6) << i << ext;
    return ss.str();
  };
  const char* dl = "image_2"; const char* dr = "image_3"; const char* ext = ".png";
  if (!exists(name(dl, 0, ext))) { dl = "image_0"; dr = "image_1"; }
  if (!exists(name(dl, 0, ext))) { ext = ".pgm"; }
  if (!exists(name(dl, 0, ext))) { dl = "image_2"; dr = "image_3"; }
  Tracking* mpTracker = new Tracking(argv[2]);
  mpTracker->depth_source = depth_source;
  mpTracker->sgbm_colour = sgbm_colour;
  mpTracker->sgbm_mode = sgbm_mode;
  mpTracker->dynamic_lk = dynamic_lk;
  mpTracker->dynamic_lk_bgr = dynamic_lk_bgr;
  mpTracker->dynamic_dev = dynamic_dev;
  mpTracker->dynamic_dev_bgr = dynamic_dev_bgr;
  mpTracker->map_out = map_out;
  if (!rectify.empty()) {
    try {
      mpTracker->LoadRectification(rectify);
    } catch (const std::exception& e) {
      std::cerr << e.what() << std::endl;
      return 1;
    }
  }
  if (!bow_voc.empty()) {
    try {
      mpTracker->LoadVocabulary(bow_voc);
    } catch (const std::exception& e) {
      std::cerr << e.what() << std::endl;
      return 1;
    }
  }
  std::ofstream loops;
  if (!loop_file.empty()) {
    loops.open(loop_file);
    if (!loops) { std::cerr << "cannot write " << loop_file << std::endl; return 1; }
  }
  std::ofstream verified;
  if (!verify_file.empty()) {
    verified.open(verify_file);
    if (!verified) { std::cerr << "cannot write " << verify_file << std::endl; return 1; }
  }
  auto write_bow = [&](int ni) {
    if (!bow_dir.empty()) {
      std::stringstream ss;
      ss << bow_dir << "/" << std::setfill('0') << std::setw(6) << ni << ".txt";
      FILE* o = fopen(ss.str().c_str(), "w");
      if (!o) { std::cerr << "cannot write " << ss.str() << std::endl; return false; }
      const auto& w = mpTracker->bow_words[(size_t)ni];
      const auto& v = mpTracker->bow_vectors[(size_t)ni];
      const auto& fv = mpTracker->bow_features[(size_t)ni];
      fprintf(o, "%zu %zu %zu\n", w.size(), v.size(), fv.size());
      for (size_t i = 0; i < w.size(); ++i) fprintf(o, "%d%s", w[i], i + 1 == w.size() ? "" : " ");
      fprintf(o, "\n");
      for (const svo_bow_entry& e : v) fprintf(o, "%u %.17g\n", e.word, e.value);
      for (const svo_bow_feature& e : fv) fprintf(o, "%u %u\n", e.node, e.feature);
      fclose(o);
    }
    if (loops.is_open()) {
      try {
        const std::vector<svo_bow_cand> c = mpTracker->LoopCandidates((size_t)ni, loop_gap, loop_top);
        loops << ni << " " << c.size() << "\n";
        char buf[64];
        for (const svo_bow_cand& e : c) { snprintf(buf, sizeof buf, "%d %.17g\n", e.frame, e.score); loops << buf; }
        if (verified.is_open()) {
          svo_loop_params lp;
          svo_loop_default_params(&lp);
          for (const svo_bow_cand& e : c) {
            const svo_loop_result r = mpTracker->VerifyLoop((size_t)ni, (size_t)e.frame, lp);
            verified << ni << " " << e.frame << " " << r.status << " " << r.n_matches << " " << r.n_inliers;
            for (int j = 0; j < 16; ++j) { snprintf(buf, sizeof buf, " %.17g", r.T12[j]); verified << buf; }
            verified << "\n";
          }
        }
      } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return false;
      }
    }
    return true;
  };
  std::vector<svo_map_obs> cloud;
  auto write_map = [&](int ni) {
    const std::vector<svo_map_obs>& obs = mpTracker->Observations((size_t)ni);
    for (const svo_map_obs& r : obs)
      if (r.flags & SVO_MAP_NEW) cloud.push_back(r);
    if (map_dir.empty()) return true;
    FILE* o = fopen((map_dir + "/" + name("", ni, ".txt").substr(seq.size() + 2)).c_str(), "w");
    if (!o) { std::cerr << "cannot write into " << map_dir << std::endl; return false; }
    for (const svo_map_obs& r : obs)
      fprintf(o, "%d %d %d %.9g %.9g %.9g %.9g %.9g %.9g\n", r.gid, (int)r.kp, (r.flags & SVO_MAP_NEW) ? 1 : 0, r.u, r.v, r.depth, r.X, r.Y, r.Z);
    fclose(o);
    return true;
  };
  // --local-ba W: windows of W frames every --ba-step frames (default W), the first --ba-fixed (default 1) fixed, over the
  // tracked sequence (Tracking::LocalBA); window k -> <map dir>/ba_%06d.txt: the refined poses of its frames as KITTI rows
  // (Twc, 12 numbers), then "# first_frame status n_points n_edges n_edges_stereo iterations trials chi2_initial chi2_final lambda_final"
  auto write_local_ba = [&]() {
    svo_ba_params bp;
    svo_ba_default_params(&bp);
    bp.window = ba_window; bp.n_fixed = ba_fixed;
    int k = 0;
    for (int f0 = 0; f0 + ba_window <= nImages; f0 += ba_step, ++k) {
      Tracking::LocalBAResult r;
      try {
        r = mpTracker->LocalBA((size_t)f0, bp);
      } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return false;
      }
      char nm[32];
      snprintf(nm, sizeof nm, "/ba_%06d.txt", k);
      FILE* o = fopen((map_dir + nm).c_str(), "w");
      if (!o) { std::cerr << "cannot write into " << map_dir << std::endl; return false; }
      for (int f = 0; f < ba_window; ++f) {
        const double* T = r.Tcw.data() + 16 * f;
        for (int i = 0; i < 3; ++i) {     // Twc = [R^T | -R^T t]
          const double t = -(T[i] * T[3] + T[4 + i] * T[7] + T[8 + i] * T[11]);
          fprintf(o, "%.17g %.17g %.17g %.17g%s", T[i], T[4 + i], T[8 + i], t, i == 2 ? "\n" : " ");
        }
      }
      fprintf(o, "# %d %d %d %d %d %d %d %.17g %.17g %.17g\n", f0, r.stats.status, r.stats.n_points, r.stats.n_edges, r.stats.n_edges_stereo,
              r.stats.iterations, r.stats.trials_total, r.stats.chi2_initial, r.stats.chi2_final, r.stats.lambda_final);
      fclose(o);
    }
    return true;
  };
  auto write_cloud = [&]() {
    if (cloud_file.empty()) return true;
    FILE* o = fopen(cloud_file.c_str(), "w");
    if (!o) { std::cerr << "cannot write " << cloud_file << std::endl; return false; }
    fprintf(o, "ply\nformat ascii 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\nend_header\n", cloud.size());
    for (const svo_map_obs& r : cloud) fprintf(o, "%.9g %.9g %.9g\n", r.X, r.Y, r.Z);
    fclose(o);
    return true;
  };
  auto write_dynamic = [&](int ni, const std::vector<Point2f>& pts) {
    FILE* o = fopen((dynamic_dir + "/" + name("", ni, ".txt").substr(seq.size() + 2)).c_str(), "w");
    if (!o) { std::cerr << "cannot write into " << dynamic_dir << std::endl; return false; }
    for (const Point2f& p : pts) fprintf(o, "%.9g %.9g\n", p.x, p.y);
    fclose(o);
    return true;
  };
  std::ofstream f("cameratrajectory_kitti.txt"); f << std::fixed;
  std::ofstream f2("cameratrajectory_tum.txt"); f2 << std::fixed;
  std::vector<float> vTimesTrack(nImages);
  std::cout << std::endl << "-------" << std::endl << "Start processing sequence ..." << std::endl
            << "Images in the sequence: " << nImages << std::endl << std::endl;
  // frame ni's boxes: from the detector on its left image, or from <sequence>/boxes/<ni+1>.txt; with --write-boxes also to
  // <dir>/<ni+1>.txt
  auto frame_boxes = [&](int ni, const GrayImage& gL, const BgrImage& cL) {
    std::vector<std::vector<int>> boxes;
    if (!det_cfg.empty()) {
      boxes = YOLOv3::TrackerBoxes(colour ? detector.Detect(cL, det_thresh) : detector.Detect(gL, det_thresh));
    } else {
      std::stringstream bp; bp << seq << "/boxes/" << (ni + 1) << ".txt";
      std::ifstream bf(bp.str());
      int l, r, t, b;
      while (bf >> l >> r >> t >> b) boxes.push_back({l, r, t, b});
    }
    if (!write_dir.empty()) {
      std::ofstream o(write_dir + "/" + std::to_string(ni + 1) + ".txt");
      for (const auto& b : boxes) o << b[0] << " " << b[1] << " " << b[2] << " " << b[3] << "\n";
    }
    return boxes;
  };
  if (pipelined) {
    mpTracker->batch_capacity = per_call;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> bufL, bufR;
    for (int n0 = 0; n0 < nImages; n0 += per_call) {
      const int n = std::min(per_call, nImages - n0);
      std::vector<std::vector<std::vector<int>>> boxes((size_t)n);
      size_t fb = 0;
      int cols = 0;
      for (int k = 0; k < n; ++k) {
        GrayImage imLeft, imRight;
        BgrImage cLeft, cRight;
        const bool ok = colour ? read_image_bgr(name(dl, n0 + k, ext), cLeft) && read_image_bgr(name(dr, n0 + k, ext), cRight)
                               : read_image(name(dl, n0 + k, ext), imLeft) && read_image(name(dr, n0 + k, ext), imRight);
        if (!ok) {
          std::cerr << std::endl << "Failed to load image at: " << name(dl, n0 + k, ext) << std::endl;
          return 1;
        }
        const std::vector<uint8_t>& l = colour ? cLeft.data : imLeft.data;
        const std::vector<uint8_t>& r = colour ? cRight.data : imRight.data;
        if (k == 0) { fb = l.size(); cols = colour ? cLeft.step() : imLeft.cols; bufL.resize(fb * n); bufR.resize(fb * n); }
        if (l.size() != fb || r.size() != fb) { std::cerr << "image size changes within the sequence" << std::endl; return 1; }
        memcpy(bufL.data() + fb * k, l.data(), fb);
        memcpy(bufR.data() + fb * k, r.data(), fb);
        boxes[k] = frame_boxes(n0 + k, imLeft, cLeft);
      }
      // (pageable buffers: the call returns when they are staged, so they are refilled at once while the GPU works)
      mpTracker->TrackBatch(bufL.data(), bufR.data(), cols, n, &vTimestamps[n0], boxes, colour);
    }
    mpTracker->FinishBatches(f, f2);
    if (dynamic_dev) {
      int lost = 0;
      for (int d : mpTracker->batch_dynamic_dropped) lost += d;
      if (lost) std::cerr << "--dynamic-dev: " << lost << " seeds did not fit into the list of " << mpTracker->dynamic_max_pts << " points" << std::endl;
      for (int ni = 0; ni < nImages && !dynamic_dir.empty(); ++ni)
        if (!write_dynamic(ni, mpTracker->batch_dynamic[(size_t)ni])) return 1;
    }
    for (int ni = 0; ni < nImages && map_out; ++ni)
      if (!write_map(ni)) return 1;
    if (!write_cloud()) return 1;
    if (ba_window && !write_local_ba()) return 1;
    const double total = std::chrono::duration_cast<std::chrono::duration<double>>(std::chrono::steady_clock::now() - t0).count();
    f.close(); f2.close();
    std::cout << std::endl << "trajectory saved!" << std::endl << "-------" << std::endl << std::endl;
    std::cout << "pipelined: " << nImages << " frames, " << per_call << " per call" << std::endl;
    std::cout << "mean tracking time: " << total / nImages << std::endl;
    std::cout << "frames per second: " << nImages / total << std::endl;
    delete mpTracker;
    return 0;
  }
  for (int ni = 0; ni < nImages; ++ni) {
    GrayImage imLeft, imRight;
    BgrImage cLeft, cRight;
    const bool ok = colour ? read_image_bgr(name(dl, ni, ext), cLeft) && read_image_bgr(name(dr, ni, ext), cRight)
                           : read_image(name(dl, ni, ext), imLeft) && read_image(name(dr, ni, ext), imRight);
    if (!ok) {
      std::cerr << std::endl << "Failed to load image at: " << name(dl, ni, ext) << std::endl;
      return 1;
    }
    const std::vector<std::vector<int>> boxes = frame_boxes(ni, imLeft, cLeft);
    const auto t1 = std::chrono::steady_clock::now();
    if (colour) mpTracker->Track(cLeft, cRight, vTimestamps[ni], f, f2, boxes);
    else mpTracker->Track(imLeft, imRight, vTimestamps[ni], f, f2, boxes);
    const auto t2 = std::chrono::steady_clock::now();
    vTimesTrack[ni] = (float)std::chrono::duration_cast<std::chrono::duration<double>>(t2 - t1).count();
    if (!dynamic_dir.empty() && !write_dynamic(ni, mpTracker->lastframe.DY_keypoints)) return 1;
    if (map_out && !write_map(ni)) return 1;
    if (!bow_voc.empty() && !write_bow(ni)) return 1;
  }
  if (!write_cloud()) return 1;
  f.close(); f2.close();
  std::cout << std::endl << "trajectory saved!" << std::endl;
  std::sort(vTimesTrack.begin(), vTimesTrack.end());
  float totaltime = 0;
  for (int ni = 0; ni < nImages; ++ni) totaltime += vTimesTrack[ni];
  std::cout << "-------" << std::endl << std::endl;
  std::cout << "median tracking time: " << vTimesTrack[nImages / 2] << std::endl;
  std::cout << "mean tracking time: " << totaltime / nImages << std::endl;
  delete mpTracker;
  return 0;
}
