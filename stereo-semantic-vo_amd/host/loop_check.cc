// loop_check.cc - one pair of frames through loop verification (svo_loop_verify), from the command line.
// usage: loop_check pair.bin [refine, default 0]
// pair.bin (little endian): int32 kp_stride, obs_stride; float32 fx, fy, cx, cy; then the arrays svo_loop_verify takes, each
// holding frame a and then frame b: desc 2 x kp_stride x 32 bytes, kp 2 x kp_stride svo_kp, n 2 x int32, fv 2 x kp_stride
// svo_bow_feature, fv_n 2 x int32, obs 2 x obs_stride svo_map_obs, obs_n 2 x int32, Tcw 2 x 16 float32.
// stdout: "status n_matches bound visited winner n_inliers s0 s1 s2"; T12's 16 values (%.17g) in one line; the matches of a's
// keypoints in one line; the inlier flags in one line.  Default parameters (svo_loop_default_params) but for refine.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "../../include/svo.h"

template <class T>
static bool take(FILE* in, std::vector<T>& v, size_t n) {
  v.resize(n > 0 ? n : 1);
  return fread(v.data(), sizeof(T), n, in) == n;
}

int main(int argc, char** argv) {
  if (argc < 2 || argc > 3) {
    std::cerr << "Usage: ./loop_check pair.bin [refine]" << std::endl;
    return 1;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) { std::cerr << argv[1] << ": cannot open" << std::endl; return 1; }
  int32_t head[2];
  float camv[4];
  if (fread(head, sizeof(int32_t), 2, in) != 2 || fread(camv, sizeof(float), 4, in) != 4 || head[0] < 1 || head[0] > 2048 ||
      head[1] < 1 || head[1] > 2048) {
    std::cerr << argv[1] << ": bad header" << std::endl;
    fclose(in);
    return 1;
  }
  const size_t S = (size_t)head[0], So = (size_t)head[1];
  std::vector<uint8_t> desc;
  std::vector<svo_kp> kp;
  std::vector<svo_bow_feature> fv;
  std::vector<svo_map_obs> obs;
  std::vector<int32_t> n, fv_n, obs_n;
  std::vector<float> Tcw;
  const bool ok = take(in, desc, 2 * S * 32) && take(in, kp, 2 * S) && take(in, n, 2) && take(in, fv, 2 * S) && take(in, fv_n, 2) &&
                  take(in, obs, 2 * So) && take(in, obs_n, 2) && take(in, Tcw, 32);
  fclose(in);
  if (!ok) { std::cerr << argv[1] << ": shorter than its header says" << std::endl; return 1; }
  svo_camera cam{camv[0], camv[1], camv[2], camv[3], 0.0f};
  svo_loop_params P;
  svo_loop_default_params(&P);
  P.refine = argc > 2 ? atoi(argv[2]) : 0;
  svo_loop* loop = nullptr;
  const int cap = (int)(S > So ? S : So);
  if (svo_loop_create(0, cap, 1, &loop) != SVO_OK) {
    std::cerr << "svo_loop_create: " << svo_loop_last_error(nullptr) << std::endl;
    return 1;
  }
  std::vector<int32_t> match(S);
  std::vector<uint8_t> inl(S);
  svo_loop_result r;
  if (svo_loop_verify(loop, &cam, &P, desc.data(), kp.data(), n.data(), (int)S, fv.data(), fv_n.data(), obs.data(), obs_n.data(),
                      (int)So, Tcw.data(), match.data(), &r, inl.data()) != SVO_OK) {
    std::cerr << "svo_loop_verify: " << svo_loop_last_error(loop) << std::endl;
    svo_loop_destroy(loop);
    return 1;
  }
  svo_loop_destroy(loop);
  printf("%d %d %d %d %d %d %d %d %d\n", r.status, r.n_matches, r.bound, r.visited, r.winner, r.n_inliers, r.sample[0], r.sample[1],
         r.sample[2]);
  for (int i = 0; i < 16; ++i) printf("%.17g%s", r.T12[i], i == 15 ? "\n" : " ");
  for (size_t i = 0; i < S; ++i) printf("%d%s", match[i], i + 1 == S ? "\n" : " ");
  for (size_t i = 0; i < S; ++i) printf("%d%s", (int)inl[i], i + 1 == S ? "\n" : " ");
  return 0;
}
