// svo_detect.h - the darknet network description shared by the host parser (svo_detect_cfg.cc) and the device forward
// (svo_detect.hip).  Restated from the reference's Thirdparty/darknet/src (parser.c, *_layer.c, yolo_v3.c).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/svo.h"

struct DetLayer {
  svo_det_layer d{};           // the public description (types, shapes, parameter count)
  int line = 0;                // cfg line of the section header
  std::vector<int> route;      // route: absolute source layers
  std::vector<int> mask;       // yolo: anchor indices
  std::vector<float> biases;   // yolo: total * 2, region: num * 2 anchors
  int total = 0;               // yolo: anchors listed (num)
  int softmax = 0;             // region
  size_t woff = 0;             // convolutional: offset of its biases in DetNet::params
};

struct DetNet {
  int w = 0, h = 0, c = 0;     // [net] width, height, channels
  int classes = 0;             // the output layers' class count
  std::vector<DetLayer> layers;
  std::vector<float> params;   // the weights file after its header, in file order
  int64_t n_params = 0;
};

// Parse `cfg`; with `weights`, read (load = true) or only size-check the weights file.  0 or SVO_E_INVALID with `err` set.
int svo_det_parse(const char* cfg, const char* weights, bool load, DetNet& net, std::string& err);
