// svo_detect.hip - darknet YOLO detection on the device (svo_det_* in include/svo.h).
// Restated from the reference's Thirdparty/darknet/src: image.c (letterbox_image, resize_image, embed_image),
// convolutional_layer.c + blas.c (gemm, normalize_cpu, scale_bias, add_bias), activations.h, maxpool_layer.c,
// route_layer.c, shortcut_layer.c, upsample_layer.c, yolo_layer.c, region_layer.c, box.c (do_nms_sort, box_iou),
// network.c (get_network_boxes) and yolo_v3.c (YoloDetect's record loop).  -ffp-contract=off keeps every float / double
// operation rounded once, as darknet's C is.
#include <float.h>
#include <math.h>
#include <string.h>

#include <algorithm>

#include "svo_detect.h"
#include "svo_gate.h"
#include "svo_internal.h"

const std::string& svo_det_thread_error();
void svo_det_set_thread_error(const std::string& e);

namespace {

constexpr int DET_MAX_ANCHORS = 16;
constexpr int DET_MAX_OUT = 8;
constexpr int DEC_THREADS = 1024;

struct DecLayer {          // one [yolo] / [region] layer for the decode kernel
  const float* out;        // its output, image 0
  int outputs;             // floats per image
  int type, w, h, n, classes, softmax;
  float anchors[2 * DET_MAX_ANCHORS];   // (w, h) of the anchors the layer uses: yolo biases[2 * mask[k]], region biases[2 * k]
};

struct DecArgs {
  int n_out;
  DecLayer L[DET_MAX_OUT];
  int classes, tmax;       // class count; detections one image can hold (sum of the layers' w * h * n)
  int netw, neth, imw, imh;
  float thresh;
};

__device__ __forceinline__ float logistic_f(float x) { return (float)(1. / (1. + exp((double)-x))); }   // activations.h
__device__ __forceinline__ float activate(float x, int act) {
  if (act == SVO_DET_ACT_LEAKY) return (x > 0) ? x : (float)(.1 * (double)x);
  if (act == SVO_DET_ACT_LOGISTIC) return logistic_f(x);
  return x;
}

// ---- input: ipl_to_image (data / 255.) + letterbox_image (resize_image's two passes, 0.5 fill, embed_image) ----
struct LetterboxGeom { int new_w, new_h, dx, dy; float w_scale, h_scale; };

// the source image: 8-bit interleaved (channel k = byte k, data / 255. in double as ipl_to_image) or darknet's planar float
// image as YoloDetectFromImage receives it (c = 3, used as given)
struct SrcU8 {
  const uint8_t* img; int stride, C;
  __device__ float operator()(int k, int x, int y) const {
    return (float)(img[(size_t)y * stride + (size_t)x * C + (C == 1 ? 0 : k)] / 255.);
  }
};
struct SrcF32 {
  const float* img; int W, H;
  __device__ float operator()(int k, int x, int y) const { return img[((size_t)k * H + y) * W + x]; }
};

// resize_image's first pass: column c of the new width, source row r
template <class S>
__device__ __forceinline__ float det_part(const S& px, int W, int k, int c, int r, const LetterboxGeom& g) {
  if (c == g.new_w - 1 || W == 1) return px(k, W - 1, r);
  const float sx = c * g.w_scale;
  const int ix = min((int)sx, W - 1);
  const float dx = sx - (int)sx;
  const int ix1 = min(ix + 1, W - 1);   // (only a rounding of sx onto W - 1 would need it; darknet would read past the row)
  return (1 - dx) * px(k, ix, r) + dx * px(k, ix1, r);
}

template <class S>
__device__ __forceinline__ void det_input_px(const S& px, int W, int H, float* __restrict__ out, int nw, int nh, LetterboxGeom g, int x,
                                             int y, int b) {
  const int rx = x - g.dx, ry = y - g.dy;
  const bool in = rx >= 0 && rx < g.new_w && ry >= 0 && ry < g.new_h;
  for (int k = 0; k < 3; ++k) {
    float v = .5f;
    if (in) {
      const float sy = ry * g.h_scale;
      const int iy = min((int)sy, H - 1);   // (in range for any new_h >= 2; the clamp only keeps reads inside the image)
      const float dy = sy - (int)sy;
      v = (1 - dy) * det_part(px, W, k, rx, iy, g);
      if (!(ry == g.new_h - 1 || H == 1)) v += dy * det_part(px, W, k, rx, min(iy + 1, H - 1), g);
    }
    out[(((size_t)b * 3 + k) * nh + y) * nw + x] = v;
  }
}

__global__ __launch_bounds__(256) void k_det_input(const uint8_t* __restrict__ imgs, size_t img_bytes, int W, int H, int C, int stride,
                                                   float* __restrict__ out, int nw, int nh, LetterboxGeom g) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
  if (x >= nw) return;
  det_input_px(SrcU8{imgs + (size_t)b * img_bytes, stride, C}, W, H, out, nw, nh, g, x, y, b);
}

__global__ __launch_bounds__(256) void k_det_input_f32(const float* __restrict__ img, int W, int H, float* __restrict__ out, int nw, int nh,
                                                       LetterboxGeom g) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= nw) return;
  det_input_px(SrcF32{img, W, H}, W, H, out, nw, nh, g, x, y, 0);
}

// ---- convolution: implicit GEMM on v_mfma_f32_16x16x4_f32 ----
// out[b][m][p] = sum_k wt[m][k] * im2col(in)[k][b * OH * OW + p], M = filters, K = C * size * size, N = B * OH * OW.
// A 256-thread block computes a 64 x 64 tile of (M, N); wave w a 32 x 32 quarter as 2 x 2 MFMA tiles.  K advances 16 at a
// time through LDS, the next slice's global loads in flight while the current one is multiplied.
constexpr int CT = 64, CK = 16, CLD = 80;   // tile, K slice, LDS row pitch (floats)

struct ConvArgs {
  const float* in; const float* wt; const float* bias; const float* scale; const float* mean; const float* var; float* out;
  int C, H, W, M, OH, OW, size, stride, pad, K, N, bn, act;
};

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_det_conv(ConvArgs a) {
  __shared__ float As[CK][CLD], Bs[CK][CLD];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int m0 = blockIdx.y * CT, n0 = blockIdx.x * CT;
  const int ss = a.size * a.size, OHW = a.OH * a.OW;
  // this thread's A loads: row am, k offsets ak .. ak + 3; B loads: column bn_, k offsets bk .. bk + 3
  const int am = t >> 2, ak = (t & 3) * 4, bn_ = t & 63, bk = (t >> 6) * 4;
  const int gn = n0 + bn_;
  const bool nvalid = gn < a.N;
  const int bimg = nvalid ? gn / OHW : 0, p = nvalid ? gn - bimg * OHW : 0;
  const int oy = p / a.OW, ox = p - oy * a.OW;
  const int iy0 = oy * a.stride - a.pad, ix0 = ox * a.stride - a.pad;
  const float* inb = a.in + (size_t)bimg * a.C * a.H * a.W;
  const bool mvalid = m0 + am < a.M;
  const float* wrow = a.wt + (size_t)(m0 + am) * a.K;
  float ra[4], rb[4];
  auto load = [&](int k0) {
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + ak + j;
      ra[j] = (mvalid && k < a.K) ? wrow[k] : 0.f;
    }
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + bk + j;
      float v = 0.f;
      if (nvalid && k < a.K) {
        const int ci = k / ss, r = k - ci * ss, ky = r / a.size, kx = r - ky * a.size;
        const int iy = iy0 + ky, ix = ix0 + kx;
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = inb[((size_t)ci * a.H + iy) * a.W + ix];
      }
      rb[j] = v;
    }
  };
  f32x4 acc[2][2];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int wm = (wv & 1) * 32, wn = (wv >> 1) * 32, lr = lane >> 4, lc = lane & 15;
  load(0);
  for (int k0 = 0; k0 < a.K; k0 += CK) {
    __syncthreads();
    for (int j = 0; j < 4; ++j) { As[ak + j][am] = ra[j]; Bs[bk + j][bn_] = rb[j]; }
    __syncthreads();
    if (k0 + CK < a.K) load(k0 + CK);
#pragma unroll
    for (int kk = 0; kk < CK / 4; ++kk) {
      const int kr = kk * 4 + lr;
      const float a0 = As[kr][wm + lc], a1 = As[kr][wm + 16 + lc];
      const float b0 = Bs[kr][wn + lc], b1 = Bs[kr][wn + 16 + lc];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  // epilogue in darknet's order: normalize_cpu, scale_bias, add_bias (or add_bias alone), then the activation
  for (int mi = 0; mi < 2; ++mi)
    for (int ni = 0; ni < 2; ++ni)
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + mi * 16 + lr * 4 + r, n = n0 + wn + ni * 16 + lc;
        if (m >= a.M || n >= a.N) continue;
        float x = acc[mi][ni][r];
        if (a.bn) {
          x = (float)((double)(x - a.mean[m]) / (sqrt((double)a.var[m]) + (double).000001f));
          x = x * a.scale[m];
        }
        x = x + a.bias[m];
        x = activate(x, a.act);
        const int b = n / OHW, q = n - b * OHW;
        a.out[((size_t)b * a.M + m) * OHW + q] = x;
      }
}

// ---- small layers ----
__global__ void k_det_maxpool(const float* __restrict__ in, float* __restrict__ out, int B, int C, int H, int W, int OH, int OW,
                              int size, int stride, int pad) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, total = (size_t)B * C * OH * OW;
  if (i >= total) return;
  const int j = (int)(i % OW), y = (int)((i / OW) % OH);
  const size_t bc = i / ((size_t)OW * OH);
  const float* src = in + bc * H * W;
  float mx = -FLT_MAX;
  for (int n = 0; n < size; ++n)
    for (int m = 0; m < size; ++m) {
      const int ch = -pad + y * stride + n, cw = -pad + j * stride + m;
      const float v = (ch >= 0 && ch < H && cw >= 0 && cw < W) ? src[(size_t)ch * W + cw] : -FLT_MAX;
      mx = (v > mx) ? v : mx;
    }
  out[i] = mx;
}

// route: source layer's [B][c][hw] into channels [off, off + c) of [B][out_c][hw]
__global__ void k_det_route(const float* __restrict__ src, float* __restrict__ out, int B, int c, int hw, int out_c, int off) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, per = (size_t)c * hw;
  if (i >= (size_t)B * per) return;
  const size_t b = i / per, r = i - b * per;
  out[(b * out_c + off) * hw + r] = src[i];
}

// shortcut (same shape, alpha = beta = 1, linear): out = 1 * x + 1 * add
__global__ void k_det_shortcut(const float* __restrict__ x, const float* __restrict__ add, float* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = x[i] + add[i];
}

__global__ void k_det_upsample(const float* __restrict__ in, float* __restrict__ out, int BC, int H, int W, int s) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, OW = (size_t)W * s, OH = (size_t)H * s;
  if (i >= (size_t)BC * OH * OW) return;
  const size_t x = i % OW, y = (i / OW) % OH, bc = i / (OW * OH);
  out[i] = in[(bc * H + y / s) * W + x / s];
}

// [yolo]: logistic on x, y (entries 0, 1), objectness and classes (4 .. 4 + classes); w, h copied
__global__ void k_det_yolo(const float* __restrict__ in, float* __restrict__ out, size_t n, int hw, int entries) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int e = (int)((i / hw) % entries);
  out[i] = (e == 2 || e == 3) ? in[i] : logistic_f(in[i]);
}

// [region] (coords 4, no background): logistic on x, y and objectness; classes by softmax (blas.c softmax, temperature 1) or
// logistic.  One thread per (image, anchor, cell).
__global__ void k_det_region(const float* __restrict__ in, float* __restrict__ out, int B, int n, int hw, int classes, int softmax) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * n * hw) return;
  const int cell = i % hw, bn = i / hw;
  const size_t base = (size_t)bn * (5 + classes) * hw + cell;
  for (int e = 0; e < 5; ++e) {
    const float v = in[base + (size_t)e * hw];
    out[base + (size_t)e * hw] = (e == 2 || e == 3) ? v : logistic_f(v);
  }
  const float* ci = in + base + (size_t)5 * hw;
  float* co = out + base + (size_t)5 * hw;
  if (!softmax) {
    for (int j = 0; j < classes; ++j) co[(size_t)j * hw] = logistic_f(ci[(size_t)j * hw]);
    return;
  }
  float largest = -FLT_MAX, sum = 0;
  for (int j = 0; j < classes; ++j)
    if (ci[(size_t)j * hw] > largest) largest = ci[(size_t)j * hw];
  for (int j = 0; j < classes; ++j) {
    const float e = (float)exp((double)(ci[(size_t)j * hw] / 1.f - largest / 1.f));
    sum += e;
    co[(size_t)j * hw] = e;
  }
  for (int j = 0; j < classes; ++j) co[(size_t)j * hw] /= sum;
}

// ---- decode + do_nms_sort + YoloDetect's record loop: one 1024-thread workgroup per image ----
struct DecScratch {
  float4* box; float* obj; float* prob; int* perm; int* perm2; int* nzi; float* nzp;
};

// exclusive prefix count of `flag` over the workgroup; *total = the workgroup's count
__device__ int det_scan(bool flag, int* lds, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const unsigned long long m = __ballot(flag);
  const int pre = __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();
  if (lane == 0) lds[wv] = __popcll(m);
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < nw; ++w) {
    const int c = lds[w];
    if (w < wv) base += c;
    tot += c;
  }
  *total = tot;
  return base + pre;
}

__device__ __forceinline__ float det_overlap(float x1, float w1, float x2, float w2) {
  const float l1 = x1 - w1 / 2, l2 = x2 - w2 / 2;
  const float left = l1 > l2 ? l1 : l2;
  const float r1 = x1 + w1 / 2, r2 = x2 + w2 / 2;
  const float right = r1 < r2 ? r1 : r2;
  return right - left;
}
__device__ __forceinline__ float det_iou(float4 a, float4 b) {
  const float w = det_overlap(a.x, a.z, b.x, b.z), h = det_overlap(a.y, a.w, b.y, b.w);
  const float i = (w < 0 || h < 0) ? 0.f : w * h;
  const float u = a.z * a.w + b.z * b.w - i;
  return i / u;
}

__global__ __launch_bounds__(DEC_THREADS) void k_det_decode(const DecArgs A, DecScratch s, float* records,
                                                            int max_records, int32_t* n_records, int32_t* boxes, int32_t* n_boxes,
                                                            int box_stride) {
  __shared__ int lds[32];
  __shared__ int sh_total;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int C = A.classes;
  const size_t T0 = (size_t)b * A.tmax;
  float4* box = s.box + T0;
  float* obj = s.obj + T0;
  float* prob = s.prob + T0 * C;
  int* perm = s.perm + T0;
  int* perm2 = s.perm2 + T0;
  int* nzi = s.nzi + T0;
  float* nzp = s.nzp + T0;
  // correct_yolo_boxes / correct_region_boxes (relative = 1)
  int new_w, new_h;
  if (((float)A.netw / A.imw) < ((float)A.neth / A.imh)) { new_w = A.netw; new_h = (A.imh * A.netw) / A.imw; }
  else { new_h = A.neth; new_w = (A.imw * A.neth) / A.imh; }
  // 1. get_network_boxes: the layers in order; yolo keeps cells (row-major) x anchors with objectness > thresh, region
  //    every anchor-major entry
  int T = 0;
  for (int li = 0; li < A.n_out; ++li) {
    const DecLayer& L = A.L[li];
    const int hw = L.w * L.h, cells = hw * L.n, E = L.classes + 5;
    const float* out = L.out + (size_t)b * L.outputs;
    for (int c0 = 0; c0 < cells; c0 += nt) {
      const int j = c0 + tid;
      int i = 0, n = 0;
      bool keep = false;
      if (j < cells) {
        if (L.type == SVO_DET_YOLO) { i = j / L.n; n = j - i * L.n; }
        else { n = j / hw; i = j - n * hw; }
        const float o = out[((size_t)n * E + 4) * hw + i];
        keep = L.type == SVO_DET_REGION || o > A.thresh;
      }
      int cnt;
      const int pos = det_scan(keep, lds, &cnt);
      if (keep) {
        const int d = T + pos;
        const int row = i / L.w, col = i % L.w;
        const float* x = out + (size_t)n * E * hw + i;
        const float objectness = x[(size_t)4 * hw];
        float4 bb;
        if (L.type == SVO_DET_YOLO) {   // get_yolo_box with lw, lh = the grid, w, h = the network
          bb.x = (col + x[0]) / L.w;
          bb.y = (row + x[(size_t)hw]) / L.h;
          bb.z = (float)(exp((double)x[(size_t)2 * hw]) * (double)L.anchors[2 * n] / (double)A.netw);
          bb.w = (float)(exp((double)x[(size_t)3 * hw]) * (double)L.anchors[2 * n + 1] / (double)A.neth);
          obj[d] = objectness;
          for (int k = 0; k < C; ++k) {
            const float pr = objectness * x[(size_t)(5 + k) * hw];
            prob[(size_t)d * C + k] = (pr > A.thresh) ? pr : 0;
          }
        } else {                        // get_region_box: w, h = the grid
          bb.x = (col + x[0]) / L.w;
          bb.y = (row + x[(size_t)hw]) / L.h;
          bb.z = (float)(exp((double)x[(size_t)2 * hw]) * (double)L.anchors[2 * n] / (double)L.w);
          bb.w = (float)(exp((double)x[(size_t)3 * hw]) * (double)L.anchors[2 * n + 1] / (double)L.h);
          const float scale = objectness;
          const float ob = scale > A.thresh ? scale : 0;
          obj[d] = ob;
          for (int k = 0; k < C; ++k) {
            float v = 0;
            if (ob != 0) {
              const float pr = scale * x[(size_t)(5 + k) * hw];
              v = (pr > A.thresh) ? pr : 0;
            }
            prob[(size_t)d * C + k] = v;
          }
        }
        bb.x = (float)(((double)bb.x - (A.netw - new_w) / 2. / A.netw) / (double)((float)new_w / A.netw));
        bb.y = (float)(((double)bb.y - (A.neth - new_h) / 2. / A.neth) / (double)((float)new_h / A.neth));
        bb.z *= (float)A.netw / new_w;
        bb.w *= (float)A.neth / new_h;
        box[d] = bb;
      }
      T += cnt;
    }
  }
  for (int i = tid; i < T; i += nt) perm[i] = i;
  __syncthreads();
  // 2. do_nms_sort: detections with objectness 0 are swapped to the end (darknet's loop, verbatim)
  if (tid == 0) {
    int k = T - 1;
    for (int i = 0; i <= k; ++i)
      if (obj[perm[i]] == 0) {
        const int sw = perm[i];
        perm[i] = perm[k];
        perm[k] = sw;
        --k;
        --i;
      }
    sh_total = k + 1;
  }
  __syncthreads();
  const int total = sh_total;
  for (int k = 0; k < C; ++k) {
    // qsort by prob[k] descending, equal scores in their order before the sort: the non-zero scores ranked, the zeros behind
    // them in their order
    int m = 0;
    for (int c0 = 0; c0 < total; c0 += nt) {
      const int i = c0 + tid;
      const float pv = i < total ? prob[(size_t)perm[i] * C + k] : 0.f;
      const bool nz = i < total && pv != 0;
      int cnt;
      const int pos = det_scan(nz, lds, &cnt);
      if (nz) { nzi[m + pos] = perm[i]; nzp[m + pos] = pv; }
      m += cnt;
    }
    __syncthreads();
    if (m == 0) continue;   // nothing to reorder (zeros keep their order) and nothing to suppress
    int z = 0;
    for (int c0 = 0; c0 < total; c0 += nt) {
      const int i = c0 + tid;
      const bool zero = i < total && prob[(size_t)perm[i] * C + k] == 0;
      int cnt;
      const int pos = det_scan(zero, lds, &cnt);
      if (zero) perm2[m + z + pos] = perm[i];
      z += cnt;
    }
    for (int q = tid; q < m; q += nt) {
      const float pq = nzp[q];
      int rank = 0;
      for (int r = 0; r < m; ++r) {
        const float pr = nzp[r];
        rank += (pr > pq || (pr == pq && r < q)) ? 1 : 0;
      }
      perm2[rank] = nzi[q];
    }
    __syncthreads();
    for (int i = tid; i < total; i += nt) perm[i] = perm2[i];
    __syncthreads();
    // suppression: only the m non-zero entries (the front of the order) can suppress or be suppressed
    for (int i = 0; i < m; ++i) {
      const int di = perm[i];
      if (prob[(size_t)di * C + k] != 0) {
        const float4 a = box[di];
        for (int j = i + 1 + tid; j < m; j += nt) {
          const int dj = perm[j];
          if (det_iou(a, box[dj]) > .45f) prob[(size_t)dj * C + k] = 0;
        }
      }
      __syncthreads();
    }
  }
  // 3. YoloDetect: every detection in the final order (the swapped tail included); max_index class, prob > threshold,
  //    result_idx * 6 + 5 < result_sz
  int nrec = 0;
  for (int c0 = 0; c0 < T; c0 += nt) {
    const int i = c0 + tid;
    bool pass = false;
    int id = 0;
    float pmax = 0;
    if (i < T) {
      const int d = perm[i];
      const float* pd = prob + (size_t)d * C;
      pmax = pd[0];
      for (int k = 1; k < C; ++k)
        if (pd[k] > pmax) { pmax = pd[k]; id = k; }
      pass = pmax > A.thresh;
    }
    int cnt;
    const int pos = det_scan(pass, lds, &cnt);
    const int ri = nrec + pos;
    if (pass && ri < max_records) {
      const float4 bb = box[perm[i]];
      int left = (int)((bb.x - bb.z / 2.) * A.imw);
      int right = (int)((bb.x + bb.z / 2.) * A.imw);
      int top = (int)((bb.y - bb.w / 2.) * A.imh);
      int bot = (int)((bb.y + bb.w / 2.) * A.imh);
      if (left < 0) left = 0;
      if (right > A.imw - 1) right = A.imw - 1;
      if (top < 0) top = 0;
      if (bot > A.imh - 1) bot = A.imh - 1;
      float* r = records + ((size_t)b * max_records + ri) * 6;
      r[0] = (float)id;
      r[1] = pmax;
      r[2] = (float)left;
      r[3] = (float)top;
      r[4] = (float)(right - left);
      r[5] = (float)(bot - top);
      if (boxes && ri < min(SVO_MAX_BOXES, box_stride)) {   // svo_boxes_dev: {left, right, top, bottom}
        int32_t* o = boxes + ((size_t)b * box_stride + ri) * 4;
        o[0] = left;
        o[1] = left + (right - left);
        o[2] = top;
        o[3] = top + (bot - top);
      }
    }
    nrec += cnt;
  }
  if (tid == 0) {
    const int n = min(nrec, max_records);
    if (n_records) n_records[b] = n;
    if (n_boxes) n_boxes[b] = min(n, min(SVO_MAX_BOXES, box_stride));
  }
}

inline unsigned blocks_for(size_t n, int t) { return (unsigned)((n + t - 1) / t); }

}  // namespace

struct svo_det {
  int device = 0, max_batch = 1;
  DetNet net;
  std::string last_error;
  hipStream_t stream = nullptr;
  float* d_params = nullptr;           // the weights file's floats, as read
  float* d_input = nullptr;            // max_batch x 3 x h x w
  std::vector<float*> d_out;           // per layer: max_batch x outputs
  std::vector<size_t> outputs;         // per layer: floats per image
  DecArgs h_args{};
  DecScratch scr{};
  void* d_scr = nullptr;
  uint8_t* d_img = nullptr; size_t img_cap = 0;    // latency mode: the uploaded image
  float* d_rec = nullptr; size_t rec_cap = 0;      // latency mode: records
  int32_t* d_nrec = nullptr;
  uint8_t* h_img = nullptr; size_t h_img_cap = 0;  // latency mode: pinned staging
  int last_B = 0;
  bool profiling = false, timed = false;
  std::vector<hipEvent_t> ev;          // svo_det_profile: input start, input end, each layer's end, decode end
};

#define DET_HIP(det, expr)                                                        \
  do {                                                                            \
    hipError_t _e = (expr);                                                       \
    if (_e != hipSuccess) {                                                       \
      (det)->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);      \
      return SVO_E_HIP;                                                           \
    }                                                                             \
  } while (0)

extern "C" const char* svo_det_last_error(const svo_det* det) { return det ? det->last_error.c_str() : svo_det_thread_error().c_str(); }

static void det_free(svo_det* d) {
  if (d->stream) hipStreamSynchronize(d->stream);
  for (hipEvent_t e : d->ev)
    if (e) hipEventDestroy(e);
  for (float* p : d->d_out)
    if (p) hipFree(p);
  void* ptrs[] = {d->d_params, d->d_input, d->d_scr, d->d_img, d->d_rec, d->d_nrec};
  for (void* p : ptrs)
    if (p) hipFree(p);
  if (d->h_img) hipHostFree(d->h_img);
  if (d->stream) hipStreamDestroy(d->stream);
  delete d;
}

static int det_alloc(svo_det* d) {
  DetNet& net = d->net;
  const size_t B = (size_t)d->max_batch;
  DET_HIP(d, hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
  DET_HIP(d, hipMalloc(&d->d_params, std::max<size_t>(1, net.params.size()) * 4));
  DET_HIP(d, hipMemcpyAsync(d->d_params, net.params.data(), net.params.size() * 4, hipMemcpyHostToDevice, d->stream));
  DET_HIP(d, hipStreamSynchronize(d->stream));
  DET_HIP(d, hipMalloc(&d->d_input, B * 3 * net.w * net.h * 4));
  d->h_args.n_out = 0;
  int tmax = 0;
  for (const DetLayer& L : net.layers) {
    const size_t o = (size_t)L.d.out_w * L.d.out_h * L.d.out_c;
    float* p = nullptr;
    DET_HIP(d, hipMalloc(&p, B * o * 4));
    d->d_out.push_back(p);
    d->outputs.push_back(o);
    if (L.d.type == SVO_DET_YOLO || L.d.type == SVO_DET_REGION) {
      if (d->h_args.n_out == DET_MAX_OUT || L.d.num > DET_MAX_ANCHORS) {
        d->last_error = "at most " + std::to_string(DET_MAX_OUT) + " output layers of at most " + std::to_string(DET_MAX_ANCHORS) + " anchors each";
        return SVO_E_INVALID;
      }
      DecLayer& D = d->h_args.L[d->h_args.n_out++];
      D.out = p;
      D.outputs = (int)o;
      D.type = L.d.type; D.w = L.d.out_w; D.h = L.d.out_h; D.n = L.d.num; D.classes = L.d.classes; D.softmax = L.softmax;
      for (int k = 0; k < L.d.num; ++k) {
        const int a = L.d.type == SVO_DET_YOLO ? L.mask[k] : k;
        D.anchors[2 * k] = L.biases[2 * a];
        D.anchors[2 * k + 1] = L.biases[2 * a + 1];
      }
      tmax += D.w * D.h * D.n;
    }
  }
  d->h_args.classes = net.classes;
  d->h_args.tmax = tmax;
  d->h_args.netw = net.w; d->h_args.neth = net.h;
  const size_t T = B * tmax;
  const size_t bytes = T * 16 + T * 4 + T * net.classes * 4 + 4 * T * 4;
  DET_HIP(d, hipMalloc(&d->d_scr, bytes));
  char* q = reinterpret_cast<char*>(d->d_scr);
  d->scr.box = reinterpret_cast<float4*>(q); q += T * 16;
  d->scr.obj = reinterpret_cast<float*>(q); q += T * 4;
  d->scr.prob = reinterpret_cast<float*>(q); q += T * net.classes * 4;
  d->scr.perm = reinterpret_cast<int*>(q); q += T * 4;
  d->scr.perm2 = reinterpret_cast<int*>(q); q += T * 4;
  d->scr.nzi = reinterpret_cast<int*>(q); q += T * 4;
  d->scr.nzp = reinterpret_cast<float*>(q);
  DET_HIP(d, hipMalloc(&d->d_nrec, 4));
  return SVO_OK;
}

extern "C" int svo_det_create(int device, const char* cfg, const char* weights, int max_batch, svo_det** out) {
  if (!out || !cfg || !weights || max_batch < 1) { svo_det_set_thread_error("svo_det_create: bad argument"); return SVO_E_INVALID; }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    (void)hipGetLastError();
    svo_det_set_thread_error("svo_det_create: no HIP device " + std::to_string(device));
    return SVO_E_NODEVICE;
  }
  svo_det* d = new svo_det();
  d->device = device;
  d->max_batch = max_batch;
  std::string err;
  int rc = svo_det_parse(cfg, weights, true, d->net, err);
  if (rc) {
    svo_det_set_thread_error(err);
    delete d;
    return rc;
  }
  hipSetDevice(device);
  rc = det_alloc(d);
  if (rc) {
    svo_det_set_thread_error(d->last_error);
    (void)hipGetLastError();
    det_free(d);
    return rc == SVO_E_HIP ? SVO_E_NOMEM : rc;
  }
  svo_det_set_thread_error("");
  *out = d;
  return SVO_OK;
}

extern "C" int svo_det_destroy(svo_det* det) {
  if (!det) return SVO_E_INVALID;
  hipSetDevice(det->device);
  det_free(det);
  return SVO_OK;
}

extern "C" int svo_det_sync(svo_det* det) {
  if (!det) return SVO_E_INVALID;
  hipSetDevice(det->device);
  DET_HIP(det, hipStreamSynchronize(det->stream));
  return SVO_OK;
}

// the forward pass and the decode for B images already in HBM
static int det_run(svo_det* d, const uint8_t* d_img, int W, int H, int C, int stride, int B, float thresh, float* d_records,
                   int max_records, int32_t* d_n, int32_t* d_boxes, int32_t* d_nb, int box_stride, bool planar_f32 = false) {
  DetNet& net = d->net;
  hipStream_t s = d->stream;
  // letterbox_image's geometry (host floats, as darknet computes them)
  LetterboxGeom g;
  if (((float)net.w / W) < ((float)net.h / H)) { g.new_w = net.w; g.new_h = (H * net.w) / W; }
  else { g.new_h = net.h; g.new_w = (W * net.h) / H; }
  if (g.new_w < 2 || g.new_h < 2) { d->last_error = "image too elongated for the network input"; return SVO_E_INVALID; }
  g.w_scale = (float)(W - 1) / (g.new_w - 1);
  g.h_scale = (float)(H - 1) / (g.new_h - 1);
  g.dx = (net.w - g.new_w) / 2;
  g.dy = (net.h - g.new_h) / 2;
  const bool prof = d->profiling;
  if (prof) DET_HIP(d, hipEventRecord(d->ev[0], s));
  if (planar_f32)
    hipLaunchKernelGGL(k_det_input_f32, dim3(blocks_for(net.w, 256), net.h, 1), dim3(256), 0, s, reinterpret_cast<const float*>(d_img), W, H,
                       d->d_input, net.w, net.h, g);
  else
    hipLaunchKernelGGL(k_det_input, dim3(blocks_for(net.w, 256), net.h, B), dim3(256), 0, s, d_img, (size_t)H * stride, W, H, C, stride,
                       d->d_input, net.w, net.h, g);
  if (prof) DET_HIP(d, hipEventRecord(d->ev[1], s));
  for (size_t li = 0; li < net.layers.size(); ++li) {
    const DetLayer& L = net.layers[li];
    const svo_det_layer& l = L.d;
    const float* in = li == 0 ? d->d_input : d->d_out[li - 1];
    float* out = d->d_out[li];
    const size_t n_out = (size_t)B * d->outputs[li];
    switch (l.type) {
      case SVO_DET_CONV: {
        ConvArgs a;
        const float* p = d->d_params + L.woff;
        a.in = in; a.out = out;
        a.bias = p; p += l.out_c;
        if (l.batch_normalize) { a.scale = p; a.mean = p + l.out_c; a.var = p + 2 * l.out_c; p += 3 * l.out_c; }
        else a.scale = a.mean = a.var = nullptr;
        a.wt = p;
        a.C = l.in_c; a.H = l.in_h; a.W = l.in_w; a.M = l.out_c; a.OH = l.out_h; a.OW = l.out_w;
        a.size = l.size; a.stride = l.stride; a.pad = l.pad; a.K = l.in_c * l.size * l.size; a.N = B * l.out_h * l.out_w;
        a.bn = l.batch_normalize; a.act = l.activation;
        hipLaunchKernelGGL(k_det_conv, dim3(blocks_for(a.N, CT), blocks_for(a.M, CT)), dim3(256), 0, s, a);
        break;
      }
      case SVO_DET_MAXPOOL:
        hipLaunchKernelGGL(k_det_maxpool, dim3(blocks_for(n_out, 256)), dim3(256), 0, s, in, out, B, l.in_c, l.in_h, l.in_w, l.out_h,
                           l.out_w, l.size, l.stride, l.pad);
        break;
      case SVO_DET_ROUTE: {
        int off = 0;
        for (int src : L.route) {
          const svo_det_layer& sl = net.layers[src].d;
          const size_t hw = (size_t)sl.out_w * sl.out_h;
          hipLaunchKernelGGL(k_det_route, dim3(blocks_for((size_t)B * sl.out_c * hw, 256)), dim3(256), 0, s, d->d_out[src], out, B, sl.out_c,
                             (int)hw, l.out_c, off);
          off += sl.out_c;
        }
        break;
      }
      case SVO_DET_SHORTCUT:
        hipLaunchKernelGGL(k_det_shortcut, dim3(blocks_for(n_out, 256)), dim3(256), 0, s, in, d->d_out[l.from[0]], out, n_out);
        break;
      case SVO_DET_UPSAMPLE:
        hipLaunchKernelGGL(k_det_upsample, dim3(blocks_for(n_out, 256)), dim3(256), 0, s, in, out, B * l.in_c, l.in_h, l.in_w, l.stride);
        break;
      case SVO_DET_YOLO:
        hipLaunchKernelGGL(k_det_yolo, dim3(blocks_for(n_out, 256)), dim3(256), 0, s, in, out, n_out, l.out_w * l.out_h, l.classes + 5);
        break;
      case SVO_DET_REGION:
        hipLaunchKernelGGL(k_det_region, dim3(blocks_for((size_t)B * l.num * l.out_w * l.out_h, 256)), dim3(256), 0, s, in, out, B, l.num,
                           l.out_w * l.out_h, l.classes, L.softmax);
        break;
    }
    if (prof) DET_HIP(d, hipEventRecord(d->ev[li + 2], s));
  }
  d->h_args.imw = W; d->h_args.imh = H; d->h_args.thresh = thresh;
  hipLaunchKernelGGL(k_det_decode, dim3(B), dim3(DEC_THREADS), 0, s, d->h_args, d->scr, d_records, max_records, d_n, d_boxes, d_nb,
                     box_stride);
  if (prof) DET_HIP(d, hipEventRecord(d->ev[net.layers.size() + 2], s));
  DET_HIP(d, hipGetLastError());
  d->timed = prof;
  d->last_B = B;
  return SVO_OK;
}

static int det_check(svo_det* det, int W, int H, int C, int stride) {
  if (W < 1 || H < 1 || (C != 1 && C != 3) || stride < W * C) {
    det->last_error = "image: W, H >= 1, C = 1 or 3, stride >= W * C";
    return SVO_E_INVALID;
  }
  return SVO_OK;
}

extern "C" int svo_det_batch_dev(svo_det* det, const uint8_t* d_img, int W, int H, int C, int stride, int B, float thresh,
                                 float* d_records, int max_records, int32_t* d_n_records, const svo_boxes_dev* d_boxes_out,
                                 svo_ctx* consumer) {
  if (!det) return SVO_E_INVALID;
  if (!d_img || !d_n_records || max_records < 0 || (max_records > 0 && !d_records) || B < 1) {
    det->last_error = "svo_det_batch_dev: bad argument";
    return SVO_E_INVALID;
  }
  if (int rc = det_check(det, W, H, C, stride)) return rc;
  if (B > det->max_batch) { det->last_error = "B exceeds max_batch"; return SVO_E_CAPACITY; }
  int32_t* bx = nullptr; int32_t* nb = nullptr; int bs = 0;
  if (d_boxes_out && d_boxes_out->boxes && d_boxes_out->n) {
    if (d_boxes_out->stride < 1) { det->last_error = "svo_det_batch_dev: box stride < 1"; return SVO_E_INVALID; }
    bx = const_cast<int32_t*>(d_boxes_out->boxes);
    nb = const_cast<int32_t*>(d_boxes_out->n);
    bs = d_boxes_out->stride;
  }
  if (consumer && consumer->device != det->device) { det->last_error = "consumer context on another device"; return SVO_E_INVALID; }
  hipSetDevice(det->device);
  if (consumer && consumer->det_read_valid)   // the consumer's last tracking call still reads the boxes an earlier call wrote
    for (hipEvent_t e : consumer->det_read) DET_HIP(det, hipStreamWaitEvent(det->stream, e, 0));
  if (int rc = det_run(det, d_img, W, H, C, stride, B, thresh, d_records, max_records, d_n_records, bx, nb, bs)) return rc;
  if (consumer) {
    if (!consumer->det_ready) DET_HIP(det, hipEventCreateWithFlags(&consumer->det_ready, hipEventDisableTiming));
    DET_HIP(det, hipEventRecord(consumer->det_ready, det->stream));
    consumer->det_pending = true;
  }
  return SVO_OK;
}

// latency mode: staging for one image of `bytes` and `cap` records (grown on demand); waits for the detector's stream first,
// since the pinned staging may still be read by the previous call's upload
static int det_stage(svo_det* det, size_t bytes, int cap) {
  DET_HIP(det, hipStreamSynchronize(det->stream));
  if (bytes > det->img_cap) {
    if (det->d_img) hipFree(det->d_img);
    if (det->h_img) hipHostFree(det->h_img);
    det->d_img = nullptr; det->h_img = nullptr; det->img_cap = 0;
    DET_HIP(det, hipMalloc(&det->d_img, bytes));
    DET_HIP(det, hipHostMalloc(&det->h_img, bytes, 0));
    det->img_cap = bytes;
  }
  if ((size_t)std::max(cap, 1) > det->rec_cap) {
    if (det->d_rec) hipFree(det->d_rec);
    det->d_rec = nullptr;
    DET_HIP(det, hipMalloc(&det->d_rec, (size_t)std::max(cap, 1) * 24));
    det->rec_cap = std::max(cap, 1);
  }
  return SVO_OK;
}

static int det_fetch(svo_det* det, float* result, int* n) {
  int32_t cnt = 0;
  DET_HIP(det, hipMemcpyAsync(&cnt, det->d_nrec, 4, hipMemcpyDeviceToHost, det->stream));
  DET_HIP(det, hipStreamSynchronize(det->stream));
  // (copies stay on the detector's stream: hipMemcpy runs on the NULL stream, a barrier against every blocking stream of
  // the process - a tracker context's host-fed work in flight included)
  if (cnt > 0) {
    DET_HIP(det, hipMemcpyAsync(result, det->d_rec, (size_t)cnt * 24, hipMemcpyDeviceToHost, det->stream));
    DET_HIP(det, hipStreamSynchronize(det->stream));
  }
  *n = cnt;
  return SVO_OK;
}

extern "C" int svo_det_detect(svo_det* det, const uint8_t* img, int W, int H, int C, int stride, float thresh, float* result,
                              int result_sz, int* n) {
  if (!det) return SVO_E_INVALID;
  if (!img || !n || result_sz < 0 || (result_sz > 0 && !result)) { det->last_error = "svo_det_detect: bad argument"; return SVO_E_INVALID; }
  if (int rc = det_check(det, W, H, C, stride)) return rc;
  hipSetDevice(det->device);
  const int cap = result_sz / 6;   // result_idx * 6 + 5 < result_sz
  const size_t bytes = (size_t)H * stride;
  if (int rc = det_stage(det, bytes, cap)) return rc;
  memcpy(det->h_img, img, bytes);
  DET_HIP(det, hipMemcpyAsync(det->d_img, det->h_img, bytes, hipMemcpyHostToDevice, det->stream));
  if (int rc = det_run(det, det->d_img, W, H, C, stride, 1, thresh, det->d_rec, cap, det->d_nrec, nullptr, nullptr, 0)) return rc;
  return det_fetch(det, result, n);
}

extern "C" int svo_det_debug_tensor(svo_det* det, int layer, int frame, float* host_out) {
  if (!det) return SVO_E_INVALID;
  if (!host_out || layer < -1 || layer >= (int)det->net.layers.size() || frame < 0 || frame >= std::max(det->last_B, 1)) {
    det->last_error = "svo_det_debug_tensor: bad layer / frame";
    return SVO_E_INVALID;
  }
  hipSetDevice(det->device);
  DET_HIP(det, hipStreamSynchronize(det->stream));
  const size_t o = layer < 0 ? (size_t)3 * det->net.w * det->net.h : det->outputs[layer];
  const float* src = (layer < 0 ? det->d_input : det->d_out[layer]) + (size_t)frame * o;
  DET_HIP(det, hipMemcpyAsync(host_out, src, o * 4, hipMemcpyDeviceToHost, det->stream));
  DET_HIP(det, hipStreamSynchronize(det->stream));
  return SVO_OK;
}

extern "C" int svo_det_detect_planar(svo_det* det, const float* data, int W, int H, int C, float thresh, float* result, int result_sz,
                                     int* n) {
  if (!det) return SVO_E_INVALID;
  if (!data || !n || C != 3 || W < 1 || H < 1 || result_sz < 0 || (result_sz > 0 && !result)) {
    det->last_error = "svo_det_detect_planar: bad argument (C must be 3)";
    return SVO_E_INVALID;
  }
  hipSetDevice(det->device);
  const int cap = result_sz / 6;
  const size_t bytes = (size_t)3 * W * H * sizeof(float);
  if (int rc = det_stage(det, bytes, cap)) return rc;
  memcpy(det->h_img, data, bytes);
  DET_HIP(det, hipMemcpyAsync(det->d_img, det->h_img, bytes, hipMemcpyHostToDevice, det->stream));
  if (int rc = det_run(det, det->d_img, W, H, 3, 0, 1, thresh, det->d_rec, cap, det->d_nrec, nullptr, nullptr, 0, true)) return rc;
  return det_fetch(det, result, n);
}

extern "C" int svo_det_profile(svo_det* det, int enable) {
  if (!det) return SVO_E_INVALID;
  hipSetDevice(det->device);
  if (enable && det->ev.empty()) {
    det->ev.assign(det->net.layers.size() + 3, nullptr);
    for (hipEvent_t& e : det->ev) DET_HIP(det, hipEventCreate(&e));
  }
  det->profiling = enable != 0;
  return SVO_OK;
}

extern "C" int svo_det_layer_times(svo_det* det, float* ms, int max_n, int* n) {
  if (!det || (max_n > 0 && !ms) || !n) return SVO_E_INVALID;
  if (!det->timed) { det->last_error = "svo_det_layer_times: the last call was not profiled (svo_det_profile)"; return SVO_E_INVALID; }
  hipSetDevice(det->device);
  DET_HIP(det, hipStreamSynchronize(det->stream));
  const int total = (int)det->ev.size() - 1;   // input, every layer, decode
  for (int i = 0; i < total && i < max_n; ++i) DET_HIP(det, hipEventElapsedTime(&ms[i], det->ev[i], det->ev[i + 1]));
  *n = total;
  return SVO_OK;
}
