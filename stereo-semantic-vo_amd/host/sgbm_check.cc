// sgbm_check.cc - frame::SGBMMatch (the host class seam over svo_sgbm_process) on one PGM pair.
// usage: sgbm_check <left.pgm> <right.pgm>; prints "sgbm_valid <valid pixels> of <pixels>" and the sum of the valid
// disparities in sixteenths.
#include <iostream>

#include "frame.h"
#include "image.h"

using namespace svo_host;

int main(int argc, char** argv) {
  if (argc != 3) { std::cerr << "usage: sgbm_check <left.pgm> <right.pgm>" << std::endl; return 2; }
  GrayImage L, R;
  if (!read_pgm(argv[1], L) || !read_pgm(argv[2], R) || L.cols != R.cols || L.rows != R.rows) {
    std::cerr << "cannot read the pair" << std::endl;
    return 2;
  }
  svo_ctx* dev = nullptr;
  if (svo_create(&dev, 0, 1241, 376, 500, 1) != SVO_OK) return 3;   // (SGBM takes any pair size: its volumes are its own)
  frame probe;
  probe.ctx = dev;
  const int valid = probe.SGBMMatch(L, R);
  long long sum16 = 0;
  for (float d : probe.dispimg)
    if (d != -1.f) sum16 += (long long)(d * 16.f);
  std::cout << "sgbm_valid " << valid << " of " << (size_t)L.cols * L.rows << " sum16 " << sum16 << std::endl;
  svo_destroy(dev);
  return 0;
}
