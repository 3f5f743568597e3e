// rect_check.cc - one raw stereo pair through the rectifier (svo_rect_create + svo_rect_process), from the command line.
// usage: rect_check settings.yaml left.(pgm|ppm) right.(pgm|ppm) out_left out_right
// The settings file is an ORB-SLAM2 one (rect_settings.h); a P5 pair is rectified as gray, a P6 pair as 8UC3 BGR.  The outputs
// are written in the inputs' format (a PPM holds RGB, as the format says).
#include <cstdio>
#include <iostream>

#include "image.h"
#include "rect_settings.h"

using namespace svo_host;

static bool write_pnm(const char* path, const char* magic, int w, int h, const std::vector<uint8_t>& px) {
  FILE* o = fopen(path, "wb");
  if (!o) return false;
  fprintf(o, "%s\n%d %d\n255\n", magic, w, h);
  const bool ok = fwrite(px.data(), 1, px.size(), o) == px.size();
  fclose(o);
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 6) {
    std::cerr << "Usage: ./rect_check settings.yaml left.(pgm|ppm) right.(pgm|ppm) out_left out_right" << std::endl;
    return 1;
  }
  RectSettings s;
  std::string err;
  if (!read_rect_yaml(argv[1], s, err)) { std::cerr << argv[1] << ": " << err << std::endl; return 1; }
  GrayImage gL, gR;
  BgrImage cL, cR;
  int cn = 0, w = 0, h = 0;
  if (read_pgm(argv[2], gL) && read_pgm(argv[3], gR)) { cn = 1; w = gL.cols; h = gL.rows; }
  else if (read_ppm_bgr(argv[2], cL) && read_ppm_bgr(argv[3], cR)) { cn = 3; w = cL.cols; h = cL.rows; }
  else { std::cerr << "cannot read the pair as two P5 or two P6 files" << std::endl; return 1; }
  const int w2 = cn == 1 ? gR.cols : cR.cols, h2 = cn == 1 ? gR.rows : cR.rows;
  if (w != s.width || h != s.height || w2 != w || h2 != h) {
    std::cerr << "the images are " << w << " x " << h << " / " << w2 << " x " << h2 << ", the settings say " << s.width << " x " << s.height << std::endl;
    return 1;
  }
  svo_rect* rect = nullptr;
  if (svo_rect_create(0, w, h, w, h, &s.left, &s.right, &rect) != SVO_OK) {
    std::cerr << "svo_rect_create: " << svo_rect_last_error(nullptr) << std::endl;
    return 1;
  }
  std::vector<uint8_t> oL((size_t)cn * w * h), oR(oL.size());
  const uint8_t* L = cn == 1 ? gL.ptr() : cL.ptr();
  const uint8_t* R = cn == 1 ? gR.ptr() : cR.ptr();
  if (svo_rect_process(rect, L, R, cn * w, cn, oL.data(), oR.data(), cn * w) != SVO_OK) {
    std::cerr << "svo_rect_process: " << svo_rect_last_error(rect) << std::endl;
    return 1;
  }
  svo_camera cam;
  svo_rect_camera(rect, s.bf, &cam);
  svo_rect_destroy(rect);
  if (cn == 3)
    for (size_t i = 0; i < oL.size(); i += 3) { std::swap(oL[i], oL[i + 2]); std::swap(oR[i], oR[i + 2]); }
  if (!write_pnm(argv[4], cn == 1 ? "P5" : "P6", w, h, oL) || !write_pnm(argv[5], cn == 1 ? "P5" : "P6", w, h, oR)) {
    std::cerr << "cannot write the outputs" << std::endl;
    return 1;
  }
  printf("rectified %d x %d, cn = %d; camera %.9g %.9g %.9g %.9g bf %.9g\n", w, h, cn, cam.fx, cam.fy, cam.cx, cam.cy, cam.bf);
  return 0;
}
