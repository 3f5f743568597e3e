// rect_settings.h - the rectification an ORB-SLAM2 settings file describes (cv::FileStorage stand-in, like read_camera_yaml):
// the !!opencv-matrix blocks LEFT.K / LEFT.D / LEFT.R / LEFT.P and RIGHT.* of the EuRoC-style files (`data: [...]` may span
// lines), or else the flat keys Camera.fx .. Camera.p2 with an optional Camera.k3 - one camera model for both sides, R = I, P = K.
#pragma once
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/svo.h"

namespace svo_host {

struct RectSettings {
  svo_rect_cam left{}, right{};
  int width = 0, height = 0;   // LEFT.width / LEFT.height, else Camera.width / Camera.height
  double bf = 0;               // Camera.bf (0: absent)
};

// false: `err` names the missing or malformed key
inline bool read_rect_yaml(const std::string& path, RectSettings& out, std::string& err) {
  std::ifstream in(path);
  if (!in) { err = "cannot open " + path; return false; }
  std::map<std::string, double> scalars;
  std::map<std::string, std::vector<double>> mats;
  std::string line, open_key, data;
  bool in_data = false;
  auto strip = [](std::string s) {
    const size_t h = s.find('#');
    if (h != std::string::npos) s.erase(h);
    const size_t a = s.find_first_not_of(" \t\r\n");
    if (a == std::string::npos) return std::string();
    return s.substr(a, s.find_last_not_of(" \t\r\n") - a + 1);
  };
  auto close_data = [&]() {
    std::vector<double> v;
    std::stringstream ss(data);
    std::string tok;
    while (std::getline(ss, tok, ','))
      if (!strip(tok).empty()) v.push_back(atof(tok.c_str()));
    mats[open_key] = v;
    in_data = false; data.clear();
  };
  while (std::getline(in, line)) {
    if (!line.empty() && line[0] == '%') continue;
    const bool indented = !line.empty() && (line[0] == ' ' || line[0] == '\t');
    std::string s = strip(line);
    if (s.empty()) continue;
    if (in_data) {   // the continuation of data: [ ...
      const size_t e = s.find(']');
      data += " " + s.substr(0, e);
      if (e != std::string::npos) close_data();
      continue;
    }
    const size_t c = s.find(':');
    if (c == std::string::npos) continue;
    const std::string key = strip(s.substr(0, c)), val = strip(s.substr(c + 1));
    if (!indented) {
      open_key.clear();
      if (val.find("!!opencv-matrix") != std::string::npos) open_key = key;
      else if (!val.empty()) scalars[key] = atof(val.c_str());
    } else if (!open_key.empty() && key == "data") {
      const size_t b = val.find('[');
      if (b == std::string::npos) { err = open_key + ": data without [ ... ]"; return false; }
      const size_t e = val.find(']', b);
      data = val.substr(b + 1, e == std::string::npos ? std::string::npos : e - b - 1);
      in_data = true;
      if (e != std::string::npos) close_data();
    }
  }
  if (in_data) { err = open_key + ": data: [ is never closed"; return false; }
  auto scalar = [&](const std::string& k, double* v) {
    const auto it = scalars.find(k);
    if (it == scalars.end()) { err = "key " + k + " is missing"; return false; }
    *v = it->second;
    return true;
  };
  double w = -1, h = -1;
  bool blocks = false;
  for (const auto& m : mats) blocks = blocks || m.first.rfind("LEFT.", 0) == 0 || m.first.rfind("RIGHT.", 0) == 0;
  if (blocks) {
    svo_rect_cam* cams[2] = {&out.left, &out.right};
    const char* sides[2] = {"LEFT", "RIGHT"};
    for (int s = 0; s < 2; ++s) {
      const std::vector<double>* part[4];
      const char* names[4] = {"K", "D", "R", "P"};
      const size_t want[4] = {9, 0, 9, 12};
      for (int k = 0; k < 4; ++k) {
        const std::string key = std::string(sides[s]) + "." + names[k];
        const auto it = mats.find(key);
        if (it == mats.end()) { err = "key " + key + " is missing"; return false; }
        if (want[k] ? it->second.size() != want[k] : (it->second.size() < 4 || it->second.size() > 5)) { err = key + " holds the wrong number of values"; return false; }
        part[k] = &it->second;
      }
      const std::vector<double>&K = *part[0], &D = *part[1], &R = *part[2], &P = *part[3];
      svo_rect_cam& c = *cams[s];
      c.K[0] = K[0]; c.K[1] = K[4]; c.K[2] = K[2]; c.K[3] = K[5];
      for (int k = 0; k < 5; ++k) c.D[k] = k < (int)D.size() ? D[k] : 0.0;
      for (int k = 0; k < 9; ++k) c.R[k] = R[k];
      c.P[0] = P[0]; c.P[1] = P[5]; c.P[2] = P[2]; c.P[3] = P[6];
    }
    if (scalars.count("LEFT.width")) w = scalars["LEFT.width"];
    if (scalars.count("LEFT.height")) h = scalars["LEFT.height"];
  } else {
    svo_rect_cam c{};
    const char* kk[4] = {"Camera.fx", "Camera.fy", "Camera.cx", "Camera.cy"};
    const char* dk[4] = {"Camera.k1", "Camera.k2", "Camera.p1", "Camera.p2"};
    for (int k = 0; k < 4; ++k)
      if (!scalar(kk[k], &c.K[k]) || !scalar(dk[k], &c.D[k])) return false;
    c.D[4] = scalars.count("Camera.k3") ? scalars["Camera.k3"] : 0.0;
    for (int k = 0; k < 9; ++k) c.R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    for (int k = 0; k < 4; ++k) c.P[k] = c.K[k];
    out.left = out.right = c;
  }
  if (w < 0 && scalars.count("Camera.width")) w = scalars["Camera.width"];
  if (h < 0 && scalars.count("Camera.height")) h = scalars["Camera.height"];
  if (w < 0 || h < 0) { err = "no image size (LEFT.width / LEFT.height or Camera.width / Camera.height)"; return false; }
  out.width = (int)w; out.height = (int)h;
  out.bf = scalars.count("Camera.bf") ? scalars["Camera.bf"] : 0.0;
  return true;
}

}  // namespace svo_host
