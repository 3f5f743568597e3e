// lk_check.cc - frame::LKTrack (the host class seam over svo_lk_track) on one PGM pair, or with --bgr frame::LKTrackBgr
// (svo_lk_track_bgr) on one PPM pair.
// usage: lk_check [--bgr] <prev> <next> <points.txt>; the text file holds one "x y" per line.  Prints one line per point,
// "lk <index> <x bits> <y bits> <status> <err bits>" (the floats as hexadecimal bit patterns), then "kept <survivors> of <points>".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

#include "frame.h"
#include "image.h"

using namespace svo_host;

static unsigned bits(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }

int main(int argc, char** argv) {
  const bool bgr = argc == 5 && std::string(argv[1]) == "--bgr";
  if (argc != 4 && !bgr) { std::cerr << "usage: lk_check [--bgr] <prev.pgm|ppm> <next.pgm|ppm> <points.txt>" << std::endl; return 2; }
  if (bgr) ++argv;
  frame last, cur;
  const bool read = bgr ? read_ppm_bgr(argv[1], last.leftimg_bgr) && read_ppm_bgr(argv[2], cur.leftimg_bgr) &&
                              last.leftimg_bgr.cols == cur.leftimg_bgr.cols && last.leftimg_bgr.rows == cur.leftimg_bgr.rows
                        : read_pgm(argv[1], last.leftimg) && read_pgm(argv[2], cur.leftimg) &&
                              last.leftimg.cols == cur.leftimg.cols && last.leftimg.rows == cur.leftimg.rows;
  if (!read) {
    std::cerr << "cannot read the pair" << std::endl;
    return 2;
  }
  std::ifstream in(argv[3]);
  for (float x, y; in >> x >> y;) last.DY_keypoints.push_back(Point2f{x, y});
  svo_ctx* dev = nullptr;
  if (svo_create(&dev, 0, 1241, 376, 500, 1) != SVO_OK) return 3;   // (LK takes any pair size: its arena is its own)
  last.ctx = cur.ctx = dev;
  const int kept = bgr ? cur.LKTrackBgr(last) : cur.LKTrack(last);
  if (kept < 0) { std::cerr << (bgr ? "svo_lk_track_bgr: " : "svo_lk_track: ") << svo_last_error(dev) << std::endl; svo_destroy(dev); return 4; }
  for (size_t i = 0; i < cur.LK_keypoints.size(); ++i)
    std::printf("lk %zu %08x %08x %d %08x\n", i, bits(cur.LK_keypoints[i].x), bits(cur.LK_keypoints[i].y), (int)cur.status[i],
                bits(cur.error[i]));
  std::printf("kept %d of %zu\n", kept, cur.LK_keypoints.size());
  svo_destroy(dev);
  return 0;
}
