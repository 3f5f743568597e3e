// yolov3se.cc - libYOLOv3SE.so: the dlopen C-ABI of the reference's include/YOLOv3SE.h (YoloLoad, YoloDetectFromImage,
// YoloDetectFromFile - Thirdparty/darknet/src/yolo_v3.c) over the device detector of libsvo_hip.so (svo_det_*), so that
// the reference's YOLOv3 class works against it unchanged.  YoloTrain is not provided.
#include <stdio.h>

#include <vector>

#include "../../include/svo.h"
#include "../host/png_reader.h"

extern "C" {

// parse_network_cfg + load_weights + set_batch_network(net, 1), on HIP device 0.  NULL on failure (darknet exits instead;
// svo_det_last_error(NULL) says why).
int* YoloLoad(char* cfgfile, char* weightsfile) {
  svo_det* det = nullptr;
  if (svo_det_create(0, cfgfile, weightsfile, 1, &det) != SVO_OK) {
    fprintf(stderr, "YoloLoad: %s\n", svo_det_last_error(nullptr));
    return nullptr;
  }
  return reinterpret_cast<int*>(det);
}

// darknet's planar float image as given (c = 3)
int YoloDetectFromImage(float* data, int w, int h, int c, int* _net, float threshold, float* result, int result_sz) {
  int n = 0;
  if (!_net || svo_det_detect_planar(reinterpret_cast<svo_det*>(_net), data, w, h, c, threshold, result, result_sz, &n) != SVO_OK)
    return 0;
  return n;
}

// load_image_color: the file decoded to RGB (PNG, binary PPM, PGM replicated), (float)byte / 255. in planes
int YoloDetectFromFile(char* img_path, int* _net, float threshold, float* result, int result_sz) {
  svo_host::BgrImage img;
  if (!_net || !img_path || !svo_host::read_image_bgr(img_path, img)) return 0;
  const int w = img.cols, h = img.rows;
  std::vector<float> planar((size_t)3 * w * h);
  for (int k = 0; k < 3; ++k)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x)
        planar[((size_t)k * h + y) * w + x] = (float)img.data[((size_t)y * w + x) * 3 + (2 - k)] / 255.;
  return YoloDetectFromImage(planar.data(), w, h, 3, _net, threshold, result, result_sz);
}

}  // extern "C"
