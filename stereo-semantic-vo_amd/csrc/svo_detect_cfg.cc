// svo_detect_cfg.cc - darknet .cfg parser and .weights reader (host only), restated from the reference's
// Thirdparty/darknet/src/parser.c (read_cfg, parse_*, load_weights_upto) and the make_*_layer shape rules.
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <set>

#include "svo_detect.h"

namespace {

struct Section {
  std::string type;   // without brackets
  int line = 0;
  std::vector<std::pair<std::string, std::string>> kv;
  std::vector<int> kv_line;
};

// read_cfg: strip ' ', '\t', '\n' (and a trailing '\r') everywhere; '#' / ';' / empty lines are comments
bool read_sections(const char* path, std::vector<Section>& out, std::string& err) {
  FILE* f = fopen(path, "r");
  if (!f) { err = std::string("cannot open cfg ") + path; return false; }
  char buf[8192];
  int nu = 0;
  bool ok = true;
  while (fgets(buf, sizeof buf, f)) {
    ++nu;
    std::string s;
    for (const char* p = buf; *p; ++p)
      if (*p != ' ' && *p != '\t' && *p != '\n' && *p != '\r') s += *p;
    if (s.empty() || s[0] == '#' || s[0] == ';') continue;
    if (s[0] == '[') {
      if (s.back() != ']') { err = "line " + std::to_string(nu) + ": malformed section header " + s; ok = false; break; }
      Section sec;
      sec.type = s.substr(1, s.size() - 2);
      sec.line = nu;
      out.push_back(sec);
      continue;
    }
    const size_t eq = s.find('=');
    if (out.empty() || eq == std::string::npos || eq == 0 || eq + 1 == s.size()) {
      err = "line " + std::to_string(nu) + ": cannot parse '" + s + "'";
      ok = false;
      break;
    }
    out.back().kv.emplace_back(s.substr(0, eq), s.substr(eq + 1));
    out.back().kv_line.push_back(nu);
  }
  fclose(f);
  return ok;
}

struct Opts {
  const Section& s;
  std::string& err;
  const std::string* find(const char* k) const {   // option_find: the first occurrence
    for (auto& p : s.kv)
      if (p.first == k) return &p.second;
    return nullptr;
  }
  bool fail(const std::string& what) const {
    err = "[" + s.type + "] at line " + std::to_string(s.line) + ": " + what;
    return false;
  }
  bool get_int(const char* k, int def, int& v) const {
    const std::string* p = find(k);
    if (!p) { v = def; return true; }
    char* end = nullptr;
    errno = 0;
    const long x = strtol(p->c_str(), &end, 10);
    if (errno || *end || x < -1000000000L || x > 1000000000L) return fail(std::string("bad integer ") + k + "=" + *p);
    v = (int)x;
    return true;
  }
  bool get_list(const char* k, std::vector<double>& v) const {
    v.clear();
    const std::string* p = find(k);
    if (!p) return true;
    const char* a = p->c_str();
    while (true) {
      char* end = nullptr;
      const double x = strtod(a, &end);
      if (end == a) return fail(std::string("bad list ") + k + "=" + *p);
      v.push_back(x);
      if (*end == 0) break;
      if (*end != ',') return fail(std::string("bad list ") + k + "=" + *p);
      a = end + 1;
    }
    return true;
  }
  // every key must be one of `allowed` (the layer's own keys and training-only keys that do not change inference)
  bool only(std::initializer_list<const char*> allowed) const {
    std::set<std::string> a;
    for (const char* k : allowed) a.insert(k);
    for (size_t i = 0; i < s.kv.size(); ++i)
      if (!a.count(s.kv[i].first)) {
        err = "[" + s.type + "] at line " + std::to_string(s.line) + ": unsupported key '" + s.kv[i].first + "' (line " +
              std::to_string(s.kv_line[i]) + ")";
        return false;
      }
    return true;
  }
};

int64_t conv_params(const svo_det_layer& d) {
  return (int64_t)d.out_c * (d.batch_normalize ? 4 : 1) + (int64_t)d.out_c * d.in_c * d.size * d.size;
}

}  // namespace

int svo_det_parse(const char* cfg, const char* weights, bool load, DetNet& net, std::string& err) {
  net = DetNet();
  if (!cfg) { err = "no cfg file"; return SVO_E_INVALID; }
  std::vector<Section> secs;
  if (!read_sections(cfg, secs, err)) return SVO_E_INVALID;
  if (secs.empty() || (secs[0].type != "net" && secs[0].type != "network")) {
    err = "the first section must be [net]";
    return SVO_E_INVALID;
  }
  {
    Opts o{secs[0], err};
    if (!o.get_int("width", 0, net.w) || !o.get_int("height", 0, net.h) || !o.get_int("channels", 0, net.c)) return SVO_E_INVALID;
    if (net.w < 1 || net.h < 1 || net.c != 3 || net.w > 8192 || net.h > 8192) {
      o.fail("width and height must be in 1..8192 and channels = 3");
      return SVO_E_INVALID;
    }
  }
  int w = net.w, h = net.h, c = net.c;
  for (size_t si = 1; si < secs.size(); ++si) {
    const Section& s = secs[si];
    Opts o{s, err};
    DetLayer L;
    L.line = s.line;
    svo_det_layer& d = L.d;
    for (int& x : d.from) x = -1;
    d.in_w = w; d.in_h = h; d.in_c = c;
    const int index = (int)net.layers.size();
    const std::string& t = s.type;
    if (t == "convolutional" || t == "conv") {
      if (!o.only({"filters", "size", "stride", "pad", "padding", "batch_normalize", "activation", "groups", "binary", "xnor"}))
        return SVO_E_INVALID;
      int filters, size, stride, pad, padding, groups, binary, xnor, bn;
      if (!o.get_int("filters", 1, filters) || !o.get_int("size", 1, size) || !o.get_int("stride", 1, stride) ||
          !o.get_int("pad", 0, pad) || !o.get_int("padding", 0, padding) || !o.get_int("groups", 1, groups) ||
          !o.get_int("binary", 0, binary) || !o.get_int("xnor", 0, xnor) || !o.get_int("batch_normalize", 0, bn))
        return SVO_E_INVALID;
      if (groups != 1 || binary != 0 || xnor != 0) { o.fail("groups must be 1, binary and xnor 0"); return SVO_E_INVALID; }
      if (filters < 1 || size < 1 || stride < 1 || padding < 0 || (bn != 0 && bn != 1)) { o.fail("bad filters / size / stride / padding / batch_normalize"); return SVO_E_INVALID; }
      if (pad) padding = size / 2;
      const std::string* act = o.find("activation");
      const std::string a = act ? *act : "logistic";
      if (a == "linear") d.activation = SVO_DET_ACT_LINEAR;
      else if (a == "leaky") d.activation = SVO_DET_ACT_LEAKY;
      else if (a == "logistic") d.activation = SVO_DET_ACT_LOGISTIC;
      else { o.fail("unsupported activation " + a); return SVO_E_INVALID; }
      d.type = SVO_DET_CONV;
      d.size = size; d.stride = stride; d.pad = padding; d.batch_normalize = bn;
      d.out_w = (w + 2 * padding - size) / stride + 1;
      d.out_h = (h + 2 * padding - size) / stride + 1;
      d.out_c = filters;
      d.n_params = conv_params(d);
      L.woff = (size_t)net.n_params;
      net.n_params += d.n_params;
    } else if (t == "maxpool" || t == "max") {
      if (!o.only({"size", "stride", "padding"})) return SVO_E_INVALID;
      int stride, size, padding;
      if (!o.get_int("stride", 1, stride) || !o.get_int("size", stride, size) || !o.get_int("padding", (size - 1) / 2, padding))
        return SVO_E_INVALID;
      if (stride < 1 || size < 1 || padding < 0) { o.fail("bad size / stride / padding"); return SVO_E_INVALID; }
      d.type = SVO_DET_MAXPOOL;
      d.size = size; d.stride = stride; d.pad = padding;
      d.out_w = (w + 2 * padding) / stride;
      d.out_h = (h + 2 * padding) / stride;
      d.out_c = c;
    } else if (t == "route") {
      if (!o.only({"layers"})) return SVO_E_INVALID;
      std::vector<double> v;
      if (!o.get_list("layers", v)) return SVO_E_INVALID;
      if (v.empty() || v.size() > 4) { o.fail("route needs 1 to 4 layers"); return SVO_E_INVALID; }
      d.type = SVO_DET_ROUTE;
      for (size_t i = 0; i < v.size(); ++i) {
        int li = (int)v[i];
        if ((double)li != v[i]) { o.fail("route layers must be integers"); return SVO_E_INVALID; }
        if (li < 0) li += index;
        if (li < 0 || li >= index) { o.fail("route layer out of range"); return SVO_E_INVALID; }
        const svo_det_layer& src = net.layers[li].d;
        if (i == 0) { d.out_w = src.out_w; d.out_h = src.out_h; d.out_c = src.out_c; }
        else if (src.out_w != d.out_w || src.out_h != d.out_h) { o.fail("route layers of different sizes"); return SVO_E_INVALID; }
        else d.out_c += src.out_c;
        L.route.push_back(li);
        d.from[i] = li;
      }
    } else if (t == "shortcut") {
      if (!o.only({"from", "activation"})) return SVO_E_INVALID;
      int from;
      if (!o.find("from")) { o.fail("shortcut needs from"); return SVO_E_INVALID; }
      if (!o.get_int("from", 0, from)) return SVO_E_INVALID;
      if (from < 0) from += index;
      if (from < 0 || from >= index) { o.fail("shortcut from out of range"); return SVO_E_INVALID; }
      const std::string* act = o.find("activation");
      if (act && *act != "linear") { o.fail("shortcut activation must be linear"); return SVO_E_INVALID; }
      const svo_det_layer& src = net.layers[from].d;
      if (src.out_w != w || src.out_h != h || src.out_c != c) { o.fail("shortcut between different shapes"); return SVO_E_INVALID; }
      d.type = SVO_DET_SHORTCUT;
      d.from[0] = from;
      d.activation = SVO_DET_ACT_LINEAR;
      d.out_w = w; d.out_h = h; d.out_c = c;
    } else if (t == "upsample") {
      if (!o.only({"stride", "scale"})) return SVO_E_INVALID;
      int stride;
      if (!o.get_int("stride", 2, stride)) return SVO_E_INVALID;
      std::vector<double> sc;
      if (!o.get_list("scale", sc)) return SVO_E_INVALID;
      if (stride < 1 || (!sc.empty() && (sc.size() != 1 || sc[0] != 1.0))) { o.fail("upsample needs stride >= 1 and scale 1"); return SVO_E_INVALID; }
      d.type = SVO_DET_UPSAMPLE;
      d.stride = stride;
      d.out_w = w * stride; d.out_h = h * stride; d.out_c = c;
    } else if (t == "yolo") {
      if (!o.only({"mask", "anchors", "classes", "num", "jitter", "ignore_thresh", "truth_thresh", "random", "max"})) return SVO_E_INVALID;
      int classes, total;
      if (!o.get_int("classes", 20, classes) || !o.get_int("num", 1, total)) return SVO_E_INVALID;
      if (classes < 1 || total < 1) { o.fail("bad classes / num"); return SVO_E_INVALID; }
      std::vector<double> mk, an;
      if (!o.get_list("mask", mk) || !o.get_list("anchors", an)) return SVO_E_INVALID;
      if (o.find("mask")) for (double x : mk) L.mask.push_back((int)x);
      else for (int i = 0; i < total; ++i) L.mask.push_back(i);
      for (int m : L.mask)
        if (m < 0 || m >= total) { o.fail("mask index out of range"); return SVO_E_INVALID; }
      if ((int)an.size() > 2 * total) { o.fail("more anchors than 2 * num"); return SVO_E_INVALID; }
      L.biases.assign(2 * total, .5f);
      for (size_t i = 0; i < an.size(); ++i) L.biases[i] = (float)an[i];   // atof -> float
      L.total = total;
      const int n = (int)L.mask.size();
      if (c != n * (classes + 5)) { o.fail("input channels must be mask size * (classes + 5)"); return SVO_E_INVALID; }
      d.type = SVO_DET_YOLO;
      d.classes = classes; d.num = n;
      d.out_w = w; d.out_h = h; d.out_c = c;
    } else if (t == "region") {
      if (!o.only({"anchors", "classes", "coords", "num", "softmax", "bias_match", "jitter", "rescore", "object_scale",
                   "noobject_scale", "class_scale", "coord_scale", "absolute", "thresh", "random", "max", "log", "sqrt",
                   "classfix", "mask_scale"}))
        return SVO_E_INVALID;
      int classes, coords, num, softmax;
      if (!o.get_int("classes", 20, classes) || !o.get_int("coords", 4, coords) || !o.get_int("num", 1, num) ||
          !o.get_int("softmax", 0, softmax))
        return SVO_E_INVALID;
      if (coords != 4 || classes < 1 || num < 1) { o.fail("region needs coords = 4, classes >= 1, num >= 1"); return SVO_E_INVALID; }
      std::vector<double> an;
      if (!o.get_list("anchors", an)) return SVO_E_INVALID;
      if ((int)an.size() > 2 * num) { o.fail("more anchors than 2 * num"); return SVO_E_INVALID; }
      L.biases.assign(2 * num, .5f);
      for (size_t i = 0; i < an.size(); ++i) L.biases[i] = (float)an[i];
      L.softmax = softmax != 0;
      if (c != num * (coords + classes + 1)) { o.fail("input channels must be num * (classes + 5)"); return SVO_E_INVALID; }
      d.type = SVO_DET_REGION;
      d.classes = classes; d.num = num;
      d.out_w = w; d.out_h = h; d.out_c = c;
    } else {
      err = "unsupported section [" + t + "] at line " + std::to_string(s.line);
      return SVO_E_INVALID;
    }
    if (d.out_w < 1 || d.out_h < 1 || d.out_c < 1) { o.fail("empty output"); return SVO_E_INVALID; }
    if (d.type == SVO_DET_YOLO || d.type == SVO_DET_REGION) {
      if (net.classes && net.classes != d.classes) { o.fail("output layers with different class counts"); return SVO_E_INVALID; }
      net.classes = d.classes;
    }
    w = d.out_w; h = d.out_h; c = d.out_c;
    net.layers.push_back(L);
  }
  if (net.layers.empty() || !net.classes) { err = "the network has no [yolo] or [region] layer"; return SVO_E_INVALID; }
  if (!weights) return SVO_OK;
  // load_weights_upto
  FILE* f = fopen(weights, "rb");
  if (!f) { err = std::string("cannot open weights ") + weights; return SVO_E_INVALID; }
  int32_t hdr[3];
  size_t head = 12;
  bool ok = fread(hdr, 4, 3, f) == 3;
  const int major = hdr[0], minor = hdr[1];
  if (ok) {
    if (major > 1000 || minor > 1000) { fclose(f); err = "transposed weights files are not supported"; return SVO_E_INVALID; }
    head += (major * 10 + minor >= 2 && major < 1000 && minor < 1000) ? 8 : 4;
  }
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  const long want = (long)head + 4 * (long)net.n_params;
  if (!ok || size != want) {
    fclose(f);
    err = std::string("weights file ") + weights + " holds " + std::to_string(size) + " bytes, the cfg implies " +
          std::to_string(want) + " (header " + std::to_string(head) + " + 4 x " + std::to_string(net.n_params) + " floats)";
    return SVO_E_INVALID;
  }
  if (load) {
    net.params.resize((size_t)net.n_params);
    fseek(f, (long)head, SEEK_SET);
    if (fread(net.params.data(), 4, net.params.size(), f) != net.params.size()) {
      fclose(f);
      err = "short read of the weights file";
      return SVO_E_INVALID;
    }
  }
  fclose(f);
  return SVO_OK;
}

static thread_local std::string g_det_err;

const std::string& svo_det_thread_error() { return g_det_err; }
void svo_det_set_thread_error(const std::string& e) { g_det_err = e; }

extern "C" int svo_det_describe(const char* cfg, const char* weights, svo_det_layer* layers, int max_layers, int* n_layers,
                                int64_t* n_params) {
  if (!cfg || max_layers < 0 || (max_layers > 0 && !layers)) { g_det_err = "svo_det_describe: bad argument"; return SVO_E_INVALID; }
  DetNet net;
  std::string err;
  const int rc = svo_det_parse(cfg, weights, false, net, err);
  if (rc) { g_det_err = err; return rc; }
  for (int i = 0; i < max_layers && i < (int)net.layers.size(); ++i) layers[i] = net.layers[i].d;
  if (n_layers) *n_layers = (int)net.layers.size();
  if (n_params) *n_params = net.n_params;
  g_det_err.clear();
  return SVO_OK;
}
