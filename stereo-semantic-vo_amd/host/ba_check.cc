// ba_check.cc - one window through the bundle adjuster (svo_ba_create + svo_ba_window), from the command line.
// usage: ba_check records.bin poses.txt [n_fixed [iterations [stereo]]]
// records.bin: int32 window, int32 obs_stride, `window` int32 counts, then window x obs_stride svo_map_obs records (32 bytes each,
// what svo_track_map_out writes).  poses.txt: one row per frame, the 16 (or the first 12) numbers of its row-major Tcw.
// The camera is KITTI 00-02's unless the environment names another (SVO_CAMERA="fx fy cx cy bf").
// stdout: the refined poses, 16 numbers a row (%.17g); "# status n_points n_edges n_edges_stereo iterations trials chi2_initial
// chi2_final lambda_final"; then "gid n_obs X Y Z" per point.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <vector>

#include "../../include/svo.h"

int main(int argc, char** argv) {
  if (argc < 3 || argc > 6) {
    std::cerr << "Usage: ./ba_check records.bin poses.txt [n_fixed [iterations [stereo]]]" << std::endl;
    return 1;
  }
  FILE* in = fopen(argv[1], "rb");
  int32_t head[2] = {0, 0};
  if (!in || fread(head, 4, 2, in) != 2 || head[0] < 2 || head[0] > 8 || head[1] < 1 || head[1] > 4096) {
    std::cerr << argv[1] << ": cannot read a header with window 2 .. 8 and obs_stride 1 .. 4096" << std::endl;
    return 1;
  }
  const int W = head[0], stride = head[1];
  std::vector<int32_t> counts((size_t)W);
  std::vector<svo_map_obs> obs((size_t)W * stride);
  if (fread(counts.data(), 4, (size_t)W, in) != (size_t)W || fread(obs.data(), sizeof(svo_map_obs), obs.size(), in) != obs.size()) {
    std::cerr << argv[1] << ": shorter than its header says" << std::endl;
    return 1;
  }
  fclose(in);
  std::vector<float> T;
  std::ifstream pf(argv[2]);
  std::string line;
  while (std::getline(pf, line)) {
    std::istringstream ls(line);
    std::vector<double> v;
    double x;
    while (ls >> x) v.push_back(x);
    if (v.empty()) continue;
    if (v.size() != 12 && v.size() != 16) { std::cerr << argv[2] << ": a row has " << v.size() << " numbers, not 12 or 16" << std::endl; return 1; }
    if (v.size() == 12) { v.push_back(0); v.push_back(0); v.push_back(0); v.push_back(1); }
    for (double e : v) T.push_back((float)e);
  }
  if (T.size() != (size_t)W * 16) { std::cerr << argv[2] << ": " << T.size() / 16 << " poses for a window of " << W << std::endl; return 1; }
  svo_camera cam{718.856f, 718.856f, 607.1928f, 185.2157f, 386.1448f};
  if (const char* e = getenv("SVO_CAMERA")) {
    if (sscanf(e, "%f %f %f %f %f", &cam.fx, &cam.fy, &cam.cx, &cam.cy, &cam.bf) != 5) { std::cerr << "SVO_CAMERA: five numbers" << std::endl; return 1; }
  }
  svo_ba_params p;
  svo_ba_default_params(&p);
  p.window = W;
  p.n_fixed = argc > 3 ? atoi(argv[3]) : 1;
  if (argc > 4) p.iterations = atoi(argv[4]);
  if (argc > 5) p.stereo = atoi(argv[5]);
  svo_ba* ba = nullptr;
  if (svo_ba_create(0, stride, 1, &ba) != SVO_OK) { std::cerr << "svo_ba_create: " << svo_ba_last_error(nullptr) << std::endl; return 1; }
  std::vector<double> out((size_t)W * 16);
  std::vector<svo_ba_point> pts((size_t)W * stride / 2 + 1);
  int32_t n = 0;
  svo_ba_stats st;
  if (svo_ba_window(ba, &cam, &p, obs.data(), counts.data(), stride, T.data(), out.data(), pts.data(), &n, &st) != SVO_OK) {
    std::cerr << "svo_ba_window: " << svo_ba_last_error(ba) << std::endl;
    svo_ba_destroy(ba);
    return 1;
  }
  svo_ba_destroy(ba);
  for (int f = 0; f < W; ++f)
    for (int j = 0; j < 16; ++j) printf("%.17g%s", out[16 * f + j], j == 15 ? "\n" : " ");
  printf("# %d %d %d %d %d %d %.17g %.17g %.17g\n", st.status, st.n_points, st.n_edges, st.n_edges_stereo, st.iterations, st.trials_total,
         st.chi2_initial, st.chi2_final, st.lambda_final);
  for (int i = 0; i < n; ++i) printf("%d %d %.17g %.17g %.17g\n", pts[i].gid, pts[i].n_obs, pts[i].X, pts[i].Y, pts[i].Z);
  return 0;
}
