// sgbm_check.cc - frame::SGBMMatch (the host class seam over svo_sgbm_process_mode) on one PGM pair, or with --bgr
// frame::ElasMatchBgr (svo_sgbm_process_bgr_mode) on one binary PPM pair; --hh, anywhere, asks for MODE_HH.
// usage: sgbm_check [--hh] <left.pgm> <right.pgm> | sgbm_check [--hh] --bgr <left.ppm> <right.ppm>; prints "sgbm_valid <valid
// pixels> of <pixels>" and the sum of the valid disparities in sixteenths.
#include <iostream>
#include <string>

#include "frame.h"
#include "image.h"

using namespace svo_host;

int main(int argc, char** argv) {
  bool hh = false;
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--hh") {
      hh = true;
      for (int j = i; j + 1 < argc; ++j) argv[j] = argv[j + 1];
      --argc;
      break;
    }
  const bool bgr = argc == 4 && std::string(argv[1]) == "--bgr";
  if (argc != 3 && !bgr) { std::cerr << "usage: sgbm_check [--hh] <left.pgm> <right.pgm> | sgbm_check [--hh] --bgr <left.ppm> <right.ppm>" << std::endl; return 2; }
  GrayImage L, R;
  BgrImage cL, cR;
  const bool ok = bgr ? read_ppm_bgr(argv[2], cL) && read_ppm_bgr(argv[3], cR) && cL.cols == cR.cols && cL.rows == cR.rows
                      : read_pgm(argv[1], L) && read_pgm(argv[2], R) && L.cols == R.cols && L.rows == R.rows;
  if (!ok) {
    std::cerr << "cannot read the pair" << std::endl;
    return 2;
  }
  svo_ctx* dev = nullptr;
  if (svo_create(&dev, 0, 1241, 376, 500, 1) != SVO_OK) return 3;   // (SGBM takes any pair size: its volumes are its own)
  frame probe;
  probe.ctx = dev;
  const int mode = hh ? SVO_SGBM_MODE_HH : SVO_SGBM_MODE_SGBM;
  const int valid = bgr ? probe.ElasMatchBgr(cL, cR, mode) : probe.SGBMMatch(L, R, mode);
  long long sum16 = 0;
  for (float d : probe.dispimg)
    if (d != -1.f) sum16 += (long long)(d * 16.f);
  std::cout << "sgbm_valid " << valid << " of " << probe.dispimg.size() << " sum16 " << sum16 << std::endl;
  svo_destroy(dev);
  return 0;
}
