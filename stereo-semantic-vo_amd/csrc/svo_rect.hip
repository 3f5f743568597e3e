// svo_rect.hip - stereo rectification on the device (svo_rect_* in include/svo.h): cv::initUndistortRectifyMap's maps once per
// object, cv::remap (8-bit, INTER_LINEAR, BORDER_CONSTANT 0) per image.  The contract, operation by operation: DESIGN.md section 8 "Rectification".
//
// An object of its own on a stream of its own, like the detector (svo_detect.hip): nothing here runs on a tracker context's
// streams.  svo_rect_batch_dev(consumer) leaves an event in the consumer (svo_ctx::rect_ready / rect_pending); the consumer's
// entries that read caller images make the stream that reads them first wait for it (svo_rect_gate, svo_internal.h).
//
// The fixed-point map is kept the way cv::remap keeps it: per destination pixel (ix, iy) as two int16 and (a | b << 5) as one
// uint16 - 6 bytes a pixel against 8 for the float maps or for two int32.  int16 holds every coordinate that can have a tap inside
// a source of at most 8192 pixels a side (ix, iy in -1 .. 8191); everything else, "outside" by the map value included, only has to
// stay outside, which saturation keeps.  Four bytes would need 2 x (14 + 5) bits.  A thread of the remap kernel serves four
// neighbouring pixels of up to RECT_BI images of its side: the map bytes are read once per RECT_BI images.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "svo_internal.h"

namespace {

constexpr int RECT_MIN = 8, RECT_MAX = 8192;   // widths RECT_MIN .. RECT_MAX, heights 1 .. RECT_MAX
constexpr int RECT_BI = 4;              // images one thread serves from one read of its map entries
constexpr int RECT_TX = 64, RECT_TY = 4;   // a workgroup: 64 groups of 4 pixels along a row (256 pixels) x 4 rows
constexpr int RECT_ZMAX = 65534;        // grid.z = 2 sides x slices of RECT_BI images: B beyond RECT_ZMAX / 2 * RECT_BI goes in further launches
constexpr int16_t RECT_OUT = -32768;    // ix = iy of a pixel that is outside by its map value

struct RectCamDev {
  double iR[9];
  double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

// One lane per destination row: the running sums _x, _y, _w along the row are a serial chain of rounded additions (part of the
// contract), so the row is walked by one lane in float64, one rounding per operation (-ffp-contract=off).  Columns W .. pitch - 1
// of the fixed-point map (pitch = W rounded up to 4) are filled with "outside".  mapx / mapy: the float maps, dst_h x dst_w;
// dbg (may be null): sx, sy as int32, INT32_MIN where outside.
__global__ void __launch_bounds__(64) k_rect_maps(RectCamDev c, int W, int H, int pitch, float* mapx, float* mapy, short2* xy,
                                                  uint16_t* ab, int32_t* dbg) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= H) return;
  double _x = (double)i * c.iR[1] + c.iR[2], _y = (double)i * c.iR[4] + c.iR[5], _w = (double)i * c.iR[7] + c.iR[8];
  const size_t row = (size_t)i * W, prow = (size_t)i * pitch;
  for (int j = 0; j < W; ++j) {
    const double w = 1.0 / _w, x = _x * w, y = _y * w;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = 2.0 * x * y;
    const double kr = 1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2;
    const double u = c.fx * (x * kr + c.p1 * _2xy + c.p2 * (r2 + 2.0 * x2)) + c.cx;
    const double v = c.fy * (y * kr + c.p1 * (r2 + 2.0 * y2) + c.p2 * _2xy) + c.cy;
    const float mx = (float)u, my = (float)v;
    mapx[row + j] = mx; mapy[row + j] = my;
    const float fx32 = mx * 32.0f, fy32 = my * 32.0f;
    const bool ok = isfinite(fx32) && isfinite(fy32) && fabsf(fx32) < 1048576.0f && fabsf(fy32) < 1048576.0f;
    int sx = 0, sy = 0;
    if (ok) { sx = (int)rintf(fx32); sy = (int)rintf(fy32); }
    // (|s| <= 2^20: s >> 5 is in -32768 .. 32768, and 32768 is as far outside as 32767)
    const int ix = ok ? min(sx >> 5, 32767) : (int)RECT_OUT, iy = ok ? min(sy >> 5, 32767) : (int)RECT_OUT;
    xy[prow + j] = make_short2((short)ix, (short)iy);
    ab[prow + j] = ok ? (uint16_t)((sx & 31) | ((sy & 31) << 5)) : (uint16_t)0;
    if (dbg) { dbg[2 * (row + j)] = ok ? sx : INT32_MIN; dbg[2 * (row + j) + 1] = ok ? sy : INT32_MIN; }
    _x += c.iR[0]; _y += c.iR[3]; _w += c.iR[6];
  }
  for (int j = W; j < pitch; ++j) { xy[prow + j] = make_short2(RECT_OUT, RECT_OUT); ab[prow + j] = 0; }
}

struct RectRemapArgs {
  const uint8_t* src[2]; uint8_t* dst[2];       // [side]: image 0 of the launch
  const short2* xy[2]; const uint16_t* ab[2];   // [side]
  int src_w, src_h, src_stride, dst_w, dst_h, dst_stride, pitch;
  int B, slices;                                // images of the launch; slices of RECT_BI images per side (grid.z = 2 slices)
  int aligned;                                  // both destinations and dst_stride are multiples of 4: whole groups go out as dwords
};

struct __attribute__((aligned(4))) RectU3 { uint32_t x, y, z; };

// cv::remap, 8UC<CN>, INTER_LINEAR (INTER_BITS 5, weights (32 - a)(32 - b) 32 .. summing to 32768, + 16384 >> 15), BORDER_CONSTANT
// 0, every tap tested on its own.  Thread (x, y) of workgroup (bx, by, z): pixels 4 g .. 4 g + 3 (g = 64 bx + x) of row 4 by + y of
// images RECT_BI slice .. of side z / slices.  Consecutive lanes write consecutive 4 CN bytes of a destination row.
template <int CN>
__global__ void __launch_bounds__(RECT_TX * RECT_TY) k_rect_remap(RectRemapArgs A) {
  const int g = blockIdx.x * RECT_TX + threadIdx.x, i = blockIdx.y * RECT_TY + threadIdx.y;
  const int j0 = 4 * g;
  if (j0 >= A.dst_w || i >= A.dst_h) return;
  const int side = (int)blockIdx.z / A.slices, b0 = ((int)blockIdx.z - side * A.slices) * RECT_BI;
  const int b1 = min(b0 + RECT_BI, A.B);
  const size_t m = (size_t)i * A.pitch + j0;   // (pitch and j0 are multiples of 4: 16- and 8-byte aligned)
  const uint4 q = *reinterpret_cast<const uint4*>(A.xy[side] + m);
  const uint2 r = *reinterpret_cast<const uint2*>(A.ab[side] + m);
  const uint32_t qv[4] = {q.x, q.y, q.z, q.w};
  int64_t off[4];            // byte offset of tap (iy, ix) in a source image
  int w00[4], w01[4], w10[4], w11[4];   // the weights, 0 where the tap is outside the source
  const int n = min(4, A.dst_w - j0);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ix = (int)(int16_t)(qv[k] & 0xffffu), iy = (int)(int16_t)(qv[k] >> 16);
    const uint32_t e = ((k < 2 ? r.x : r.y) >> (16 * (k & 1))) & 0xffffu;
    const int a = (int)(e & 31u), b = (int)(e >> 5);
    const bool x0 = (unsigned)ix < (unsigned)A.src_w, x1 = (unsigned)(ix + 1) < (unsigned)A.src_w;
    const bool y0 = (unsigned)iy < (unsigned)A.src_h, y1 = (unsigned)(iy + 1) < (unsigned)A.src_h;
    off[k] = (int64_t)iy * A.src_stride + (int64_t)ix * CN;
    w00[k] = (x0 && y0) ? (32 - a) * (32 - b) * 32 : 0;
    w01[k] = (x1 && y0) ? a * (32 - b) * 32 : 0;
    w10[k] = (x0 && y1) ? (32 - a) * b * 32 : 0;
    w11[k] = (x1 && y1) ? a * b * 32 : 0;
  }
  const size_t src_img = (size_t)A.src_h * A.src_stride, dst_img = (size_t)A.dst_h * A.dst_stride;
  for (int b = b0; b < b1; ++b) {
    const uint8_t* s = A.src[side] + (size_t)b * src_img;
    uint8_t* d = A.dst[side] + (size_t)b * dst_img + (size_t)i * A.dst_stride + (size_t)j0 * CN;
    uint32_t o[4 * CN];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint8_t* p = s + off[k];
#pragma unroll
      for (int ch = 0; ch < CN; ++ch) {
        // (a tap with weight 0 is outside the source, or contributes nothing: it is not read)
        int acc = 16384;
        if (w00[k]) acc += w00[k] * p[ch];
        if (w01[k]) acc += w01[k] * p[CN + ch];
        if (w10[k]) acc += w10[k] * p[A.src_stride + ch];
        if (w11[k]) acc += w11[k] * p[A.src_stride + CN + ch];
        o[k * CN + ch] = (uint32_t)(acc >> 15);
      }
    }
    if (n == 4 && A.aligned) {
      if constexpr (CN == 1) {
        *reinterpret_cast<uint32_t*>(d) = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
      } else {
        RectU3 v;
        v.x = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
        v.y = o[4] | (o[5] << 8) | (o[6] << 16) | (o[7] << 24);
        v.z = o[8] | (o[9] << 8) | (o[10] << 16) | (o[11] << 24);
        *reinterpret_cast<RectU3*>(d) = v;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n) {
#pragma unroll
          for (int ch = 0; ch < CN; ++ch) d[k * CN + ch] = (uint8_t)o[k * CN + ch];
        }
    }
  }
}

thread_local std::string g_rect_err;

int round4(int v) { return (v + 3) & ~3; }

}  // namespace

struct svo_rect {
  int device = 0;
  int src_w = 0, src_h = 0, dst_w = 0, dst_h = 0, pitch = 0;
  svo_rect_cam cam[2];
  double iR[2][9];
  std::string last_error;
  hipStream_t stream = nullptr;
  float* d_mapx[2] = {nullptr, nullptr};   // the float maps, dst_h x dst_w (kept for svo_rect_debug_maps)
  float* d_mapy[2] = {nullptr, nullptr};
  short2* d_xy[2] = {nullptr, nullptr};    // (ix, iy), dst_h x pitch
  uint16_t* d_ab[2] = {nullptr, nullptr};  // a | b << 5
  uint8_t* d_stage = nullptr;              // svo_rect_process: the raw pair, then the rectified pair
  size_t stage_cap = 0;
};

#define RECT_HIP(r, expr)                                                         \
  do {                                                                            \
    hipError_t _e = (expr);                                                       \
    if (_e != hipSuccess) {                                                       \
      (r)->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);        \
      return SVO_E_HIP;                                                           \
    }                                                                             \
  } while (0)

// iR = (Ar R)^-1 as cv::invert's 3 x 3 case forms it (DESIGN.md section 8 "Rectification").  false: a non-finite value, or det == 0.
static bool rect_inverse(const svo_rect_cam& c, double iR[9], std::string& why) {
  const double* all[4] = {c.K, c.D, c.R, c.P};
  const int cnt[4] = {4, 5, 9, 4};
  for (int a = 0; a < 4; ++a)
    for (int k = 0; k < cnt[a]; ++k)
      if (!std::isfinite(all[a][k])) { why = "a calibration value is not finite"; return false; }
  const double Ar[9] = {c.P[0], 0.0, c.P[2], 0.0, c.P[1], c.P[3], 0.0, 0.0, 1.0};
  double M[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s = s + Ar[3 * i + k] * c.R[3 * k + j];
      M[3 * i + j] = s;
    }
  const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[3] * M[8] - M[5] * M[6], c02 = M[3] * M[7] - M[4] * M[6];
  const double det = M[0] * c00 - M[1] * c01 + M[2] * c02;
  if (det == 0.0 || !std::isfinite(det)) { why = "det(Ar R) is zero or not finite"; return false; }
  const double d = 1.0 / det;
  iR[0] = c00 * d;
  iR[1] = (M[2] * M[7] - M[1] * M[8]) * d;
  iR[2] = (M[1] * M[5] - M[2] * M[4]) * d;
  iR[3] = (M[5] * M[6] - M[3] * M[8]) * d;
  iR[4] = (M[0] * M[8] - M[2] * M[6]) * d;
  iR[5] = (M[2] * M[3] - M[0] * M[5]) * d;
  iR[6] = c02 * d;
  iR[7] = (M[1] * M[6] - M[0] * M[7]) * d;
  iR[8] = (M[0] * M[4] - M[1] * M[3]) * d;
  return true;
}

static void rect_free(svo_rect* r) {
  if (r->stream) hipStreamSynchronize(r->stream);
  for (int s = 0; s < 2; ++s) {
    void* ptrs[] = {r->d_mapx[s], r->d_mapy[s], r->d_xy[s], r->d_ab[s]};
    for (void* p : ptrs)
      if (p) hipFree(p);
  }
  if (r->d_stage) hipFree(r->d_stage);
  if (r->stream) hipStreamDestroy(r->stream);
  delete r;
}

static void rect_launch_maps(svo_rect* r, int side, int32_t* dbg) {
  RectCamDev c;
  memcpy(c.iR, r->iR[side], sizeof(c.iR));
  const svo_rect_cam& k = r->cam[side];
  c.fx = k.K[0]; c.fy = k.K[1]; c.cx = k.K[2]; c.cy = k.K[3];
  c.k1 = k.D[0]; c.k2 = k.D[1]; c.p1 = k.D[2]; c.p2 = k.D[3]; c.k3 = k.D[4];
  hipLaunchKernelGGL(k_rect_maps, dim3((r->dst_h + 63) / 64), dim3(64), 0, r->stream, c, r->dst_w, r->dst_h, r->pitch,
                     r->d_mapx[side], r->d_mapy[side], r->d_xy[side], r->d_ab[side], dbg);
}

static int rect_alloc(svo_rect* r) {
  RECT_HIP(r, hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
  const size_t n = (size_t)r->dst_w * r->dst_h, np = (size_t)r->pitch * r->dst_h;
  for (int s = 0; s < 2; ++s) {
    RECT_HIP(r, hipMalloc(reinterpret_cast<void**>(&r->d_mapx[s]), n * sizeof(float)));
    RECT_HIP(r, hipMalloc(reinterpret_cast<void**>(&r->d_mapy[s]), n * sizeof(float)));
    RECT_HIP(r, hipMalloc(reinterpret_cast<void**>(&r->d_xy[s]), np * sizeof(short2)));
    RECT_HIP(r, hipMalloc(reinterpret_cast<void**>(&r->d_ab[s]), np * sizeof(uint16_t)));
    rect_launch_maps(r, s, nullptr);
  }
  RECT_HIP(r, hipGetLastError());
  RECT_HIP(r, hipStreamSynchronize(r->stream));
  return SVO_OK;
}

extern "C" const char* svo_rect_last_error(const svo_rect* rect) { return rect ? rect->last_error.c_str() : g_rect_err.c_str(); }

extern "C" int svo_rect_create(int device, int src_w, int src_h, int dst_w, int dst_h, const svo_rect_cam* left,
                               const svo_rect_cam* right, svo_rect** out) {
  if (!out || !left || !right) { g_rect_err = "svo_rect_create: NULL argument"; return SVO_E_INVALID; }
  *out = nullptr;
  // (the lower limit is on the widths: heights go down to 1 - a 257 x 5 destination is one of the suite's own cases)
  if (src_w < RECT_MIN || src_w > RECT_MAX || dst_w < RECT_MIN || dst_w > RECT_MAX || src_h < 1 || src_h > RECT_MAX || dst_h < 1 ||
      dst_h > RECT_MAX) {
    g_rect_err = "svo_rect_create: widths must be 8 .. 8192, heights 1 .. 8192";
    return SVO_E_INVALID;
  }
  svo_rect* r = new svo_rect();
  r->cam[0] = *left; r->cam[1] = *right;
  for (int s = 0; s < 2; ++s) {
    std::string why;
    if (!rect_inverse(r->cam[s], r->iR[s], why)) {
      g_rect_err = std::string("svo_rect_create: ") + (s ? "right: " : "left: ") + why;
      delete r;
      return SVO_E_INVALID;
    }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    (void)hipGetLastError();
    g_rect_err = "svo_rect_create: no HIP device " + std::to_string(device);
    delete r;
    return SVO_E_NODEVICE;
  }
  r->device = device;
  r->src_w = src_w; r->src_h = src_h; r->dst_w = dst_w; r->dst_h = dst_h; r->pitch = round4(dst_w);
  hipSetDevice(device);
  const int rc = rect_alloc(r);
  if (rc) {
    g_rect_err = r->last_error;
    (void)hipGetLastError();
    rect_free(r);
    return rc == SVO_E_HIP ? SVO_E_NOMEM : rc;
  }
  g_rect_err.clear();
  *out = r;
  return SVO_OK;
}

extern "C" int svo_rect_destroy(svo_rect* rect) {
  if (!rect) return SVO_E_INVALID;
  hipSetDevice(rect->device);
  rect_free(rect);
  return SVO_OK;
}

extern "C" int svo_rect_camera(const svo_rect* rect, double bf_or_0, svo_camera* cam) {
  if (!rect || !cam) return SVO_E_INVALID;
  const double* P = rect->cam[0].P;
  cam->fx = (float)P[0]; cam->fy = (float)P[1]; cam->cx = (float)P[2]; cam->cy = (float)P[3]; cam->bf = (float)bf_or_0;
  return SVO_OK;
}

extern "C" int svo_rect_sync(svo_rect* rect) {
  if (!rect) return SVO_E_INVALID;
  hipSetDevice(rect->device);
  RECT_HIP(rect, hipStreamSynchronize(rect->stream));
  return SVO_OK;
}

extern "C" void* svo_rect_stream(svo_rect* rect) { return rect ? rect->stream : nullptr; }

// the host-side checks of both image entries
static int rect_check(svo_rect* r, const char* who, const void* a, const void* b, const void* c, const void* d, int src_stride, int cn,
                      int dst_stride) {
  const char* why = nullptr;
  if (!a || !b || !c || !d) why = "NULL image pointer";
  else if (cn != 1 && cn != 3) why = "cn must be 1 or 3";
  else if (src_stride < cn * r->src_w) why = "src_stride below cn * src_w";
  else if (dst_stride < cn * r->dst_w) why = "dst_stride below cn * dst_w";
  if (!why) return SVO_OK;
  r->last_error = std::string(who) + ": " + why;
  return SVO_E_INVALID;
}

// B pairs already in HBM, on the rectifier's stream
static int rect_run(svo_rect* r, const uint8_t* dL, const uint8_t* dR, int src_stride, int cn, int B, uint8_t* oL, uint8_t* oR,
                    int dst_stride) {
  RectRemapArgs A;
  A.src_w = r->src_w; A.src_h = r->src_h; A.src_stride = src_stride;
  A.dst_w = r->dst_w; A.dst_h = r->dst_h; A.dst_stride = dst_stride; A.pitch = r->pitch;
  for (int s = 0; s < 2; ++s) { A.xy[s] = r->d_xy[s]; A.ab[s] = r->d_ab[s]; }
  A.aligned = ((reinterpret_cast<uintptr_t>(oL) | reinterpret_cast<uintptr_t>(oR) | (uintptr_t)dst_stride) & 3u) == 0;
  const size_t src_img = (size_t)r->src_h * src_stride, dst_img = (size_t)r->dst_h * dst_stride;
  const int groups = (r->dst_w + 3) / 4;
  const int per_launch = RECT_ZMAX / 2 * RECT_BI;
  for (int f0 = 0; f0 < B; f0 += per_launch) {
    A.B = std::min(per_launch, B - f0);
    A.slices = (A.B + RECT_BI - 1) / RECT_BI;
    A.src[0] = dL + (size_t)f0 * src_img; A.src[1] = dR + (size_t)f0 * src_img;
    A.dst[0] = oL + (size_t)f0 * dst_img; A.dst[1] = oR + (size_t)f0 * dst_img;
    const dim3 grid((groups + RECT_TX - 1) / RECT_TX, (r->dst_h + RECT_TY - 1) / RECT_TY, 2 * A.slices), block(RECT_TX, RECT_TY);
    if (cn == 1) hipLaunchKernelGGL(k_rect_remap<1>, grid, block, 0, r->stream, A);
    else hipLaunchKernelGGL(k_rect_remap<3>, grid, block, 0, r->stream, A);
  }
  RECT_HIP(r, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_rect_batch_dev(svo_rect* rect, const uint8_t* d_L, const uint8_t* d_R, int src_stride, int cn, int B,
                                  uint8_t* d_outL, uint8_t* d_outR, int dst_stride, svo_ctx* consumer) {
  if (!rect) return SVO_E_INVALID;
  if (int rc = rect_check(rect, "svo_rect_batch_dev", d_L, d_R, d_outL, d_outR, src_stride, cn, dst_stride)) return rc;
  if (B < 1) { rect->last_error = "svo_rect_batch_dev: B < 1"; return SVO_E_INVALID; }
  if (consumer && consumer->device != rect->device) { rect->last_error = "svo_rect_batch_dev: consumer context on another device"; return SVO_E_INVALID; }
  hipSetDevice(rect->device);
  if (int rc = rect_run(rect, d_L, d_R, src_stride, cn, B, d_outL, d_outR, dst_stride)) return rc;
  if (consumer) {
    if (!consumer->rect_ready) RECT_HIP(rect, hipEventCreateWithFlags(&consumer->rect_ready, hipEventDisableTiming));
    RECT_HIP(rect, hipEventRecord(consumer->rect_ready, rect->stream));
    consumer->rect_pending = true;
  }
  return SVO_OK;
}

extern "C" int svo_rect_process(svo_rect* rect, const uint8_t* L, const uint8_t* R, int src_stride, int cn, uint8_t* outL,
                                uint8_t* outR, int dst_stride) {
  if (!rect) return SVO_E_INVALID;
  if (int rc = rect_check(rect, "svo_rect_process", L, R, outL, outR, src_stride, cn, dst_stride)) return rc;
  hipSetDevice(rect->device);
  const int sp = round4(cn * rect->src_w), dp = round4(cn * rect->dst_w);
  const size_t src_img = (size_t)rect->src_h * sp, dst_img = (size_t)rect->dst_h * dp, need = 2 * (src_img + dst_img);
  RECT_HIP(rect, hipStreamSynchronize(rect->stream));
  if (need > rect->stage_cap) {
    if (rect->d_stage) hipFree(rect->d_stage);
    rect->d_stage = nullptr; rect->stage_cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(&rect->d_stage), need) != hipSuccess) {
      (void)hipGetLastError();
      rect->last_error = "svo_rect_process: out of device memory";
      return SVO_E_NOMEM;
    }
    rect->stage_cap = need;
  }
  uint8_t *sL = rect->d_stage, *sR = sL + src_img, *oL = sR + src_img, *oR = oL + dst_img;   // (every part a multiple of 4 bytes)
  const size_t sw = (size_t)cn * rect->src_w, dw = (size_t)cn * rect->dst_w;
  RECT_HIP(rect, hipMemcpy2DAsync(sL, sp, L, src_stride, sw, rect->src_h, hipMemcpyHostToDevice, rect->stream));
  RECT_HIP(rect, hipMemcpy2DAsync(sR, sp, R, src_stride, sw, rect->src_h, hipMemcpyHostToDevice, rect->stream));
  if (int rc = rect_run(rect, sL, sR, sp, cn, 1, oL, oR, dp)) return rc;
  RECT_HIP(rect, hipMemcpy2DAsync(outL, dst_stride, oL, dp, dw, rect->dst_h, hipMemcpyDeviceToHost, rect->stream));
  RECT_HIP(rect, hipMemcpy2DAsync(outR, dst_stride, oR, dp, dw, rect->dst_h, hipMemcpyDeviceToHost, rect->stream));
  RECT_HIP(rect, hipStreamSynchronize(rect->stream));
  return SVO_OK;
}

extern "C" int svo_rect_debug_maps(svo_rect* rect, int side, double iR[9], float* mapx, float* mapy, int32_t* sxsy) {
  if (!rect) return SVO_E_INVALID;
  if (side < 0 || side > 1) { rect->last_error = "svo_rect_debug_maps: side must be 0 or 1"; return SVO_E_INVALID; }
  if (iR) memcpy(iR, rect->iR[side], 9 * sizeof(double));
  hipSetDevice(rect->device);
  const size_t n = (size_t)rect->dst_w * rect->dst_h;
  if (mapx) RECT_HIP(rect, hipMemcpyAsync(mapx, rect->d_mapx[side], n * sizeof(float), hipMemcpyDeviceToHost, rect->stream));
  if (mapy) RECT_HIP(rect, hipMemcpyAsync(mapy, rect->d_mapy[side], n * sizeof(float), hipMemcpyDeviceToHost, rect->stream));
  int32_t* d_dbg = nullptr;
  if (sxsy) {   // the map kernel once more, with its int32 output on (the maps it rewrites are the ones it wrote)
    if (hipMalloc(reinterpret_cast<void**>(&d_dbg), 2 * n * sizeof(int32_t)) != hipSuccess) {
      (void)hipGetLastError();
      rect->last_error = "svo_rect_debug_maps: out of device memory";
      return SVO_E_NOMEM;
    }
    rect_launch_maps(rect, side, d_dbg);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(sxsy, d_dbg, 2 * n * sizeof(int32_t), hipMemcpyDeviceToHost, rect->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(rect->stream);
    hipFree(d_dbg);
    if (e != hipSuccess) { rect->last_error = std::string("svo_rect_debug_maps: ") + hipGetErrorString(e); return SVO_E_HIP; }
  }
  RECT_HIP(rect, hipStreamSynchronize(rect->stream));
  return SVO_OK;
}
