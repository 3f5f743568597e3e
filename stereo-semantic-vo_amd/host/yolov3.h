// yolov3.h - the reference's YOLOv3 / BoxSE classes (include/YOLOv3SE.h) without OpenCV or dlopen, over the device
// detector of libsvo_hip.so (svo_det_*).  Detect returns darknet's records sorted by score, as the reference's wrapper
// does (its std::sort leaves equal scores in no particular order; std::stable_sort keeps darknet's order among them).
#pragma once
#include <algorithm>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/svo.h"
#include "image.h"

namespace svo_host {

struct BoxSE {             // cv::Rect's x, y, width, height + the class, score and name
  int x = 0, y = 0, width = 0, height = 0;
  int m_class = -1;
  float m_score = 0.0F;
  std::string m_class_name = "Unknown";
};

class YOLOv3 {
 public:
  YOLOv3() = default;
  YOLOv3(const YOLOv3&) = delete;
  YOLOv3& operator=(const YOLOv3&) = delete;
  ~YOLOv3() { Release(); }

  // YoloLoad(cfg, weights) on HIP device `device`; class names one per line (may be empty).  Throws on failure.
  void Create(const std::string& weights, const std::string& cfg, const std::string& names, int device = 0) {
    Release();
    if (svo_det_create(device, cfg.c_str(), weights.c_str(), 1, &m_det) != SVO_OK)
      throw std::runtime_error(std::string("YOLOv3::Create: ") + svo_det_last_error(nullptr));
    m_names.clear();
    if (!names.empty()) {
      std::ifstream fin(names);
      std::string s;
      while (std::getline(fin, s))
        if (!s.empty()) m_names.push_back(s);
    }
  }
  void Release() {
    if (m_det) svo_det_destroy(m_det);
    m_det = nullptr;
  }
  std::string Names(size_t idx) const { return idx < m_names.size() ? m_names[idx] : "Unknown"; }

  // YOLOv3::Detect(cv::Mat, threshold) on an 8-bit interleaved image (C = 3: channel k = byte k, BGR as stored; C = 1: gray)
  std::vector<BoxSE> Detect(const uint8_t* img, int W, int H, int C, int stride, float threshold) {
    std::vector<float> result(6000, 0.f);
    int n = 0;
    if (!m_det || svo_det_detect(m_det, img, W, H, C, stride, threshold, result.data(), (int)result.size(), &n) != SVO_OK)
      throw std::runtime_error(std::string("YOLOv3::Detect: ") + (m_det ? svo_det_last_error(m_det) : "no network"));
    std::vector<BoxSE> boxes;
    for (int i = 0; i < n; ++i) {
      BoxSE b;
      b.m_class = static_cast<int>(result[i * 6 + 0]);
      b.m_score = result[i * 6 + 1];
      b.x = static_cast<int>(result[i * 6 + 2]);
      b.y = static_cast<int>(result[i * 6 + 3]);
      b.width = static_cast<int>(result[i * 6 + 4]);
      b.height = static_cast<int>(result[i * 6 + 5]);
      if (!m_names.empty()) b.m_class_name = Names((size_t)b.m_class);
      boxes.push_back(b);
    }
    std::stable_sort(boxes.begin(), boxes.end(), [](const BoxSE& a, const BoxSE& b) { return a.m_score > b.m_score; });
    return boxes;
  }
  std::vector<BoxSE> Detect(const BgrImage& img, float threshold) { return Detect(img.ptr(), img.cols, img.rows, 3, img.step(), threshold); }
  std::vector<BoxSE> Detect(const GrayImage& img, float threshold) { return Detect(img.ptr(), img.cols, img.rows, 1, img.cols, threshold); }

  // the tracker's boxes {left, right, top, bottom} (main.cpp:82-95's order), at most 64 (the tracker's limit)
  static std::vector<std::vector<int>> TrackerBoxes(const std::vector<BoxSE>& boxes) {
    std::vector<std::vector<int>> out;
    for (const BoxSE& b : boxes) {
      if (out.size() == 64) break;
      out.push_back({b.x, b.x + b.width, b.y, b.y + b.height});
    }
    return out;
  }

 private:
  svo_det* m_det = nullptr;
  std::vector<std::string> m_names;
};

}  // namespace svo_host
