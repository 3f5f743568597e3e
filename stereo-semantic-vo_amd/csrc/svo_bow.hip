// svo_bow.hip - DBoW2 bag-of-words place recognition on the device (svo_bow_* in include/svo.h): a vocabulary tree over the 32-byte
// ORB descriptors, a frame's BowVector and FeatureVector, the L1 score of two vectors and the best earlier frames of a query.
// The contract, operation by operation: DESIGN.md section 8 "Bag of words"; the numpy twin: tests/bow_ref.py.
//
// An object of its own on a stream of its own, like the rectifier (svo_rect.hip) and the adjuster (svo_ba.hip): nothing here runs
// on a tracker context's streams; with a producer context the object's stream waits for an event recorded on the producer's
// stream, nothing else.
//
// Three kernels:
//   k_bow_words   a 32-lane group per descriptor, a lane per child: 8 x (xor, popcount) against the child's centre, a min over
//                 (distance, child order) across the group, L dependent levels.  The device copy of the tree holds a node's children
//                 side by side (the host renumbers breadth first and keeps the map back to the file's ids).
//                 k_bow_assign is one level of it alone (svo_bow_assign_dev).
//   k_bow_vector  a workgroup per frame: the (word, feature) keys sorted in LDS (bitonic), a thread per run of equal words adding
//                 the weight once per occurrence, ONE thread taking the norm over the words in ascending order, the division; then
//                 the (node, feature) keys the same way for the FeatureVector.
//   k_bow_score   a wavefront per (query, database frame) pair: the query vector in LDS, the lanes look the frame's words up in it,
//                 the matches of 64 entries are taken in lane (= word) order.  k_bow_query is the same with the selection of the
//                 top_k best frames fused, so the Q x N scores are never written.
// Every sum the contract orders is taken in that order by one thread or one wave: no floating-point atomics, the same bytes on
// every run.
//
// Not here: an inverted index and ORB-SLAM2's DetectLoopCandidates heuristics (covisibility groups, consistency over three
// keyframes), loop correction or any feedback into the tracker (SearchByBoW and the fixed-scale Sim3Solver: svo_loop.hip), scorings
// other than L1, DBoW2's binary / YAML formats, the many-sequence entries, descriptors other than 32 bytes.
#include <errno.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "svo_internal.h"

namespace {

constexpr int BOW_NT = 256;
constexpr int BOW_GROUP = 32;            // lanes of a descriptor's group: one per child, k <= 20
constexpr int BOW_MAX_K = 20, BOW_MAX_L = 10;
constexpr int BOW_MAX_KP = 2048;         // features of a frame: the LDS of k_bow_vector holds their keys and values
constexpr int BOW_MAX_TOP = 16;
constexpr int BOW_WAVES = BOW_NT / 64;

// the device copy of the tree: node 0 is the root, a node's children are child0 .. child0 + nchild - 1
struct BowTree {
  const uint32_t* desc;      // n x 8
  const int32_t* child0;     // n
  const int32_t* nchild;     // n (0: a leaf)
  const int32_t* word;       // n (-1: not a leaf)
  const int32_t* fileid;     // n: the node's id in the file / the arrays it came from
  const double* wweight;     // per word
  int L, weighting;
};

__device__ __forceinline__ int bow_dist(const uint32_t f[8], const uint32_t* c) {
  int d = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) d += __popc(f[j] ^ c[j]);
  return d;
}

// the child with the smallest distance, the earliest among equals: every lane of the 32-lane group gets (distance << 5 | child)
__device__ __forceinline__ int bow_group_min(int key) {
#pragma unroll
  for (int o = BOW_GROUP / 2; o > 0; o >>= 1) key = min(key, __shfl_xor(key, o, BOW_GROUP));
  return key;
}

struct WordsArgs {
  BowTree T;
  const uint8_t* desc; const int32_t* n; int kp_stride, levelsup;
  int32_t *s_word, *s_node; int s_stride;     // scratch: per feature the word (-1: stopped) and the node of the FeatureVector
  int32_t* words;                             // caller's copy of s_word, kp_stride a frame (may be NULL)
};

__global__ void __launch_bounds__(BOW_NT) k_bow_words(WordsArgs A) {
  const int f = blockIdx.y, lane = threadIdx.x & (BOW_GROUP - 1);
  const int i = blockIdx.x * (BOW_NT / BOW_GROUP) + (threadIdx.x / BOW_GROUP);
  if (i >= A.kp_stride) return;               // (whole groups leave together)
  const int n = min(max(A.n[f], 0), A.kp_stride);
  int word = -1, nid = 0;
  if (i < n) {
    const uint32_t* fp = reinterpret_cast<const uint32_t*>(A.desc + ((size_t)f * A.kp_stride + i) * 32);
    uint32_t fd[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) fd[j] = fp[j];
    const int nid_level = A.T.L - A.levelsup;
    int node = 0, level = 0;
    bool have = nid_level <= 0;               // the root
    int nc = A.T.nchild[0];
    do {
      ++level;
      const int c0 = A.T.child0[node];
      int key = INT_MAX;
      if (lane < nc) key = (bow_dist(fd, A.T.desc + (size_t)(c0 + lane) * 8) << 5) | lane;
      key = bow_group_min(key);
      node = c0 + (key & 31);
      if (!have && level == nid_level) { nid = A.T.fileid[node]; have = true; }
      nc = A.T.nchild[node];
    } while (nc > 0);
    if (!have) nid = A.T.fileid[node];        // a leaf above level L - levelsup: the leaf itself
    word = A.T.word[node];
    if (!(A.T.wweight[word] > 0.0)) word = -1;   // a stop word
  }
  if (lane == 0) {
    if (i < n) {
      A.s_word[(size_t)f * A.s_stride + i] = word;
      A.s_node[(size_t)f * A.s_stride + i] = nid;
    }
    if (A.words) A.words[(size_t)f * A.kp_stride + i] = word;
  }
}

// n descriptors against k centres: one level of the walk
__global__ void __launch_bounds__(BOW_NT) k_bow_assign(const uint8_t* desc, int n, const uint8_t* centres, int k, int32_t* idx,
                                                       int32_t* dist) {
  const int lane = threadIdx.x & (BOW_GROUP - 1);
  const long long i = (long long)blockIdx.x * (BOW_NT / BOW_GROUP) + (threadIdx.x / BOW_GROUP);
  if (i >= n) return;
  const uint32_t* fp = reinterpret_cast<const uint32_t*>(desc + (size_t)i * 32);
  uint32_t fd[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) fd[j] = fp[j];
  int key = INT_MAX;
  if (lane < k) key = (bow_dist(fd, reinterpret_cast<const uint32_t*>(centres) + (size_t)lane * 8) << 5) | lane;
  key = bow_group_min(key);
  if (lane == 0) {
    if (idx) idx[i] = key & 31;
    if (dist) dist[i] = key >> 5;
  }
}

// ascending bitonic sort of nk (a power of two) keys in LDS by the whole workgroup
__device__ inline void bow_sort(uint64_t* keys, int nk) {
  for (int size = 2; size <= nk; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < (nk >> 1); t += BOW_NT) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const uint64_t a = keys[lo], b = keys[hi];
        if ((a > b) == up) { keys[lo] = b; keys[hi] = a; }
      }
    }
  __syncthreads();
}

struct VectorArgs {
  BowTree T;
  const int32_t* n; int kp_stride;
  const int32_t *s_word, *s_node; int s_stride;
  svo_bow_entry* vec; int32_t* vec_n;
  svo_bow_feature* fv; int32_t* fv_n;
};

__global__ void __launch_bounds__(BOW_NT) k_bow_vector(VectorArgs A) {
  __shared__ uint64_t keys[BOW_MAX_KP];
  __shared__ double vals[BOW_MAX_KP];
  __shared__ int32_t pos[BOW_MAX_KP];      // of a run's head: its place in the vector; -1 elsewhere
  __shared__ double s_norm;
  __shared__ int s_m, s_nv;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(A.n[f], 0), A.kp_stride);
  const int32_t* sw = A.s_word + (size_t)f * A.s_stride;
  const int32_t* sn = A.s_node + (size_t)f * A.s_stride;
  int nk = 2;
  while (nk < n) nk <<= 1;
  if (tid == 0) s_m = 0;
  __syncthreads();
  // (word, feature): the stopped ones behind everything else
  int mine = 0;
  for (int i = tid; i < nk; i += BOW_NT) {
    uint64_t k = ~0ull;
    if (i < n && sw[i] >= 0) { k = ((uint64_t)(uint32_t)sw[i] << 32) | (uint32_t)i; ++mine; }
    keys[i] = k;
  }
  if (mine) atomicAdd(&s_m, mine);
  bow_sort(keys, nk);
  const int m = s_m;
  const bool once = A.T.weighting == 2 || A.T.weighting == 3;      // IDF, BINARY: addIfNotExist
  for (int p = tid; p < m; p += BOW_NT) {
    const uint32_t w = (uint32_t)(keys[p] >> 32);
    int at = -1;
    if (p == 0 || (uint32_t)(keys[p - 1] >> 32) != w) {
      const double wt = A.T.wweight[w];
      double v = wt;                       // addWeight: inserted as w, then += w per further occurrence, in feature order
      if (!once)
        for (int q = p + 1; q < m && (uint32_t)(keys[q] >> 32) == w; ++q) v += wt;
      vals[p] = v;
      at = 0;
    }
    pos[p] = at;
  }
  __syncthreads();
  if (tid == 0) {     // the norm: |value| summed over the words in ascending order, one chain of at most n additions
    double norm = 0.0;
    int nv = 0;
    for (int p = 0; p < m; ++p)
      if (pos[p] == 0) { pos[p] = nv++; norm += fabs(vals[p]); }
    s_norm = norm; s_nv = nv;
  }
  __syncthreads();
  if (A.vec) {
    const double norm = s_norm;
    svo_bow_entry* out = A.vec + (size_t)f * A.kp_stride;
    for (int p = tid; p < m; p += BOW_NT)
      if (pos[p] >= 0) {
        svo_bow_entry e;
        e.word = (uint32_t)(keys[p] >> 32); e.reserved = 0;
        e.value = norm > 0.0 ? vals[p] / norm : vals[p];
        out[pos[p]] = e;
      }
  }
  if (tid == 0) {
    if (A.vec_n) A.vec_n[f] = s_nv;
    if (A.fv_n) A.fv_n[f] = m;
  }
  if (!A.fv) return;
  __syncthreads();
  for (int i = tid; i < nk; i += BOW_NT) {
    uint64_t k = ~0ull;
    if (i < n && sw[i] >= 0) k = ((uint64_t)(uint32_t)sn[i] << 32) | (uint32_t)i;
    keys[i] = k;
  }
  bow_sort(keys, nk);
  svo_bow_feature* fo = A.fv + (size_t)f * A.kp_stride;
  for (int p = tid; p < m; p += BOW_NT) {
    svo_bow_feature e;
    e.node = (uint32_t)(keys[p] >> 32); e.feature = (uint32_t)keys[p];
    fo[p] = e;
  }
}

// L1Scoring::score of the vector in LDS (qw ascending, qv; nq entries) and vector b (nb entries), by one wave; every lane returns it
__device__ inline double bow_wave_score(const uint32_t* qw, const double* qv, int nq, const svo_bow_entry* b, int nb) {
  const int lane = threadIdx.x & 63;
  double s = 0.0;
  for (int base = 0; base < nb; base += 64) {
    const int e = base + lane;
    double term = 0.0;
    bool hit = false;
    if (e < nb && nq > 0) {
      const uint32_t w = b[e].word;
      int lo = 0, hi = nq;                 // the first entry of q with a word >= w
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (qw[mid] < w) lo = mid + 1; else hi = mid;
      }
      if (lo < nq && qw[lo] == w) {
        const double vi = qv[lo], wi = b[e].value;
        term = fabs(vi - wi) - fabs(vi) - fabs(wi);
        hit = true;
      }
    }
    unsigned long long mask = __ballot(hit);
    while (mask) {                         // the common words in ascending order
      const int src = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      s += __shfl(term, src, 64);
    }
  }
  return -s / 2.0;
}

__device__ inline void bow_load_query(uint32_t* qw, double* qv, const svo_bow_entry* a, int na) {
  for (int i = threadIdx.x; i < na; i += BOW_NT) { qw[i] = a[i].word; qv[i] = a[i].value; }
  __syncthreads();
}

__global__ void __launch_bounds__(BOW_NT) k_bow_score(const svo_bow_entry* vecA, const int32_t* nA, const svo_bow_entry* vecB,
                                                      const int32_t* nB, int NB, int stride, double* scores) {
  __shared__ uint32_t qw[BOW_MAX_KP];
  __shared__ double qv[BOW_MAX_KP];
  const int a = blockIdx.y;
  const int na = min(max(nA[a], 0), stride);
  bow_load_query(qw, qv, vecA + (size_t)a * stride, na);
  const int b = blockIdx.x * BOW_WAVES + (threadIdx.x >> 6);
  if (b >= NB) return;
  const int nb = min(max(nB[b], 0), stride);
  const double s = bow_wave_score(qw, qv, na, vecB + (size_t)b * stride, nb);
  if ((threadIdx.x & 63) == 0) scores[(size_t)a * NB + b] = s;
}

struct QueryArgs {
  const svo_bow_entry* vec; const int32_t* n; int stride, q0, gap, top_k;
  double min_score;
  svo_bow_cand* cand; int32_t* cand_n;
};

__global__ void __launch_bounds__(BOW_NT) k_bow_query(QueryArgs A) {
  __shared__ uint32_t qw[BOW_MAX_KP];
  __shared__ double qv[BOW_MAX_KP];
  __shared__ double ts[BOW_WAVES][BOW_MAX_TOP];
  __shared__ int tj[BOW_WAVES][BOW_MAX_TOP];
  __shared__ int tn[BOW_WAVES];
  const int q = A.q0 + blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, K = A.top_k;
  const int nq = min(max(A.n[q], 0), A.stride);
  bow_load_query(qw, qv, A.vec + (size_t)q * A.stride, nq);
  const int last = q - A.gap;                 // frames 0 .. last - 1 are admissible
  int cnt = 0;                                // (lane 0's copy counts)
  for (int j = wave; j < last; j += BOW_WAVES) {
    const int nb = min(max(A.n[j], 0), A.stride);
    const double s = bow_wave_score(qw, qv, nq, A.vec + (size_t)j * A.stride, nb);
    if (lane == 0 && s > A.min_score) {       // this wave's list: descending score, equal scores by ascending j (j only grows here)
      int p = cnt;
      while (p > 0 && ts[wave][p - 1] < s) --p;
      if (p < K) {
        const int top = min(cnt, K - 1);
        for (int t = top; t > p; --t) { ts[wave][t] = ts[wave][t - 1]; tj[wave][t] = tj[wave][t - 1]; }
        ts[wave][p] = s; tj[wave][p] = j;
        if (cnt < K) ++cnt;
      }
    }
  }
  if (lane == 0) tn[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {                     // merge the waves' lists
    int at[BOW_WAVES];
    for (int w = 0; w < BOW_WAVES; ++w) at[w] = 0;
    svo_bow_cand* out = A.cand + (size_t)blockIdx.x * K;
    int got = 0;
    for (; got < K; ++got) {
      int best = -1;
      for (int w = 0; w < BOW_WAVES; ++w) {
        if (at[w] >= tn[w]) continue;
        if (best < 0) { best = w; continue; }
        const double sb = ts[best][at[best]], sw = ts[w][at[w]];
        if (sw > sb || (sw == sb && tj[w][at[w]] < tj[best][at[best]])) best = w;
      }
      if (best < 0) break;
      svo_bow_cand c;
      c.frame = tj[best][at[best]]; c.reserved = 0; c.score = ts[best][at[best]];
      out[got] = c;
      ++at[best];
    }
    A.cand_n[blockIdx.x] = got;
    for (int t = got; t < K; ++t) {
      svo_bow_cand c;
      c.frame = -1; c.reserved = 0; c.score = 0.0;
      out[t] = c;
    }
  }
}

thread_local std::string g_bow_err;

}  // namespace

struct svo_bow {
  int device = 0, max_kp = 0, max_frames = 0;
  int k = 0, L = 0, weighting = 0, n_words = 0;
  // the tree as given (file ids): node 0 is the root
  std::vector<int32_t> parent;
  std::vector<uint8_t> desc;
  std::vector<double> weight;
  std::vector<std::vector<int32_t>> children;
  bool ready = false;            // the device side exists (made by the first call that needs it)
  std::string last_error;
  hipStream_t stream = nullptr;
  hipEvent_t producer_done = nullptr;
  uint8_t* d_tree = nullptr;     // the device copy of the tree, one allocation
  BowTree T{};
  int32_t *d_sword = nullptr, *d_snode = nullptr;
  uint8_t* d_stage = nullptr;    // svo_bow_transform: descriptors and the count in; words, vectors and their counts out
};

#define BOW_HIP(b, expr)                                                          \
  do {                                                                            \
    hipError_t _e = (expr);                                                       \
    if (_e != hipSuccess) {                                                       \
      (b)->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);        \
      return SVO_E_HIP;                                                           \
    }                                                                             \
  } while (0)

static int bow_fail(svo_bow* bow, const char* who, const std::string& why) {
  const std::string m = std::string(who) + ": " + why;
  if (bow) bow->last_error = m; else g_bow_err = m;
  return SVO_E_INVALID;
}

static size_t bow_round(size_t v) { return (v + 255) & ~(size_t)255; }
struct BowStage { size_t desc, n, words, vec, vec_n, fv, fv_n, total; };
static BowStage bow_stage(const svo_bow* bow) {
  BowStage s;
  size_t o = 0;
  s.desc = o; o += bow_round((size_t)bow->max_kp * 32);
  s.n = o; o += bow_round(sizeof(int32_t));
  s.words = o; o += bow_round((size_t)bow->max_kp * sizeof(int32_t));
  s.vec = o; o += bow_round((size_t)bow->max_kp * sizeof(svo_bow_entry));
  s.vec_n = o; o += bow_round(sizeof(int32_t));
  s.fv = o; o += bow_round((size_t)bow->max_kp * sizeof(svo_bow_feature));
  s.fv_n = o; o += bow_round(sizeof(int32_t));
  s.total = o;
  return s;
}

// The checks both constructors share, and the object.  leaf_flag: the file's is_leaf column, or NULL (arrays: a node without
// children is a leaf).  line0: the file line of node 1 (0: no file, name nodes).
static int bow_build(const char* who, int device, int k, int L, int weighting, int n_nodes, const int32_t* parents,
                     const uint8_t* descriptors, const double* weights, const uint8_t* leaf_flag, int line0, int max_kp,
                     int max_frames, svo_bow** out) {
  auto where = [&](int id) { return line0 ? "line " + std::to_string(line0 + id - 1) : "node " + std::to_string(id); };
  if (device < 0) return bow_fail(nullptr, who, "device is negative");
  if (k < 2 || k > BOW_MAX_K) return bow_fail(nullptr, who, "k must be 2 .. 20");
  if (L < 1 || L > BOW_MAX_L) return bow_fail(nullptr, who, "L must be 1 .. 10");
  if (weighting < 0 || weighting > 3) return bow_fail(nullptr, who, "weighting must be 0 .. 3 (TF_IDF, TF, IDF, BINARY)");
  if (max_kp < 1 || max_kp > BOW_MAX_KP) return bow_fail(nullptr, who, "max_kp must be 1 .. 2048");
  if (max_frames < 1 || max_frames > 65535) return bow_fail(nullptr, who, "max_frames must be 1 .. 65535");
  if (n_nodes < 2) return bow_fail(nullptr, who, "a vocabulary needs the root and at least one node");
  std::vector<std::vector<int32_t>> children(n_nodes);
  for (int id = 1; id < n_nodes; ++id) {
    const int p = parents[id];
    if (p < 0 || p >= id) return bow_fail(nullptr, who, where(id) + ": parent " + std::to_string(p) + " is not defined yet");
    if (leaf_flag && leaf_flag[p]) return bow_fail(nullptr, who, where(id) + ": parent " + std::to_string(p) + " is marked a leaf");
    if ((int)children[p].size() >= k) return bow_fail(nullptr, who, where(id) + ": parent " + std::to_string(p) + " has more than k children");
    children[p].push_back(id);
  }
  if (leaf_flag)
    for (int id = 1; id < n_nodes; ++id)
      if (!leaf_flag[id] && children[id].empty()) return bow_fail(nullptr, who, where(id) + ": an inner node without children");
  svo_bow* bow = new svo_bow();
  bow->device = device; bow->max_kp = max_kp; bow->max_frames = max_frames;
  bow->k = k; bow->L = L; bow->weighting = weighting;
  bow->parent.assign(parents, parents + n_nodes);
  bow->parent[0] = -1;
  bow->desc.assign(descriptors, descriptors + (size_t)n_nodes * 32);
  bow->weight.assign(weights, weights + n_nodes);
  memset(bow->desc.data(), 0, 32);
  bow->weight[0] = 0.0;
  for (int id = 1; id < n_nodes; ++id) bow->n_words += children[id].empty();
  bow->children.swap(children);
  g_bow_err.clear();
  *out = bow;
  return SVO_OK;
}

// the device side of the object, at the first call that needs it (the constructors touch no device: their checks and those of
// the calls answer on a machine without one)
static int bow_ready(svo_bow* bow) {
  if (bow->ready) { hipSetDevice(bow->device); return SVO_OK; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || bow->device >= ndev) {
    (void)hipGetLastError();
    bow->last_error = "svo_bow: no HIP device " + std::to_string(bow->device);
    return SVO_E_NODEVICE;
  }
  hipSetDevice(bow->device);
  BOW_HIP(bow, hipStreamCreateWithFlags(&bow->stream, hipStreamNonBlocking));
  BOW_HIP(bow, hipEventCreateWithFlags(&bow->producer_done, hipEventDisableTiming));
  // breadth first: a node's children side by side, in their order
  const int n = (int)bow->parent.size();
  std::vector<int32_t> order;      // device index -> file id
  order.reserve(n);
  order.push_back(0);
  std::vector<int32_t> child0(n, 0), nchild(n, 0), word(n, -1), wid(n, -1);
  for (size_t at = 0; at < order.size(); ++at) {
    const std::vector<int32_t>& ch = bow->children[order[at]];
    child0[at] = (int32_t)order.size();
    nchild[at] = (int32_t)ch.size();
    for (int32_t c : ch) order.push_back(c);
  }
  std::vector<double> wweight(bow->n_words > 0 ? bow->n_words : 1, 0.0);
  int nw = 0;
  for (int id = 1; id < n; ++id)     // createWords: the leaves in node-id order
    if (bow->children[id].empty()) { wid[id] = nw; wweight[nw] = bow->weight[id]; ++nw; }
  std::vector<uint32_t> desc((size_t)n * 8);
  for (int at = 0; at < n; ++at) {
    memcpy(&desc[(size_t)at * 8], &bow->desc[(size_t)order[at] * 32], 32);
    word[at] = wid[order[at]];
  }
  size_t o = 0;
  const size_t o_desc = o; o += bow_round((size_t)n * 32);
  const size_t o_c0 = o; o += bow_round((size_t)n * 4);
  const size_t o_nc = o; o += bow_round((size_t)n * 4);
  const size_t o_word = o; o += bow_round((size_t)n * 4);
  const size_t o_file = o; o += bow_round((size_t)n * 4);
  const size_t o_ww = o; o += bow_round(wweight.size() * 8);
  const size_t scr = (size_t)bow->max_frames * bow->max_kp * sizeof(int32_t);
  if (hipMalloc(reinterpret_cast<void**>(&bow->d_tree), o) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&bow->d_sword), scr) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&bow->d_snode), scr) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&bow->d_stage), bow_stage(bow).total) != hipSuccess) {
    (void)hipGetLastError();
    bow->last_error = "svo_bow: out of device memory";
    return SVO_E_NOMEM;
  }
  uint8_t* d = bow->d_tree;
  BOW_HIP(bow, hipMemcpy(d + o_desc, desc.data(), (size_t)n * 32, hipMemcpyHostToDevice));
  BOW_HIP(bow, hipMemcpy(d + o_c0, child0.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  BOW_HIP(bow, hipMemcpy(d + o_nc, nchild.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  BOW_HIP(bow, hipMemcpy(d + o_word, word.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  BOW_HIP(bow, hipMemcpy(d + o_file, order.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  BOW_HIP(bow, hipMemcpy(d + o_ww, wweight.data(), wweight.size() * 8, hipMemcpyHostToDevice));
  bow->T.desc = reinterpret_cast<const uint32_t*>(d + o_desc);
  bow->T.child0 = reinterpret_cast<const int32_t*>(d + o_c0);
  bow->T.nchild = reinterpret_cast<const int32_t*>(d + o_nc);
  bow->T.word = reinterpret_cast<const int32_t*>(d + o_word);
  bow->T.fileid = reinterpret_cast<const int32_t*>(d + o_file);
  bow->T.wweight = reinterpret_cast<const double*>(d + o_ww);
  bow->T.L = bow->L; bow->T.weighting = bow->weighting;
  bow->ready = true;
  return SVO_OK;
}

extern "C" const char* svo_bow_last_error(const svo_bow* bow) { return bow ? bow->last_error.c_str() : g_bow_err.c_str(); }

extern "C" int svo_bow_create(int device, int k, int L, int weighting, int n_nodes, const int32_t* parents, const uint8_t* descriptors,
                              const double* weights, int max_kp, int max_frames, svo_bow** out) {
  const char* who = "svo_bow_create";
  if (!out) return bow_fail(nullptr, who, "out is NULL");
  *out = nullptr;
  if (!parents || !descriptors || !weights) return bow_fail(nullptr, who, "parents, descriptors or weights is NULL");
  return bow_build(who, device, k, L, weighting, n_nodes, parents, descriptors, weights, nullptr, 0, max_kp, max_frames, out);
}

extern "C" int svo_bow_create_from_text(int device, const char* path, int max_kp, int max_frames, svo_bow** out) {
  const char* who = "svo_bow_create_from_text";
  if (!out) return bow_fail(nullptr, who, "out is NULL");
  *out = nullptr;
  if (!path) return bow_fail(nullptr, who, "path is NULL");
  FILE* fp = fopen(path, "r");
  if (!fp) return bow_fail(nullptr, who, std::string("cannot open ") + path);
  std::string text;
  char buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, fp)) > 0) text.append(buf, got);
  fclose(fp);
  // lines; a line of blanks is skipped (a file may end in one)
  std::vector<int32_t> parents(1, -1);
  std::vector<uint8_t> desc(32, 0), leaf(1, 0);
  std::vector<double> weights(1, 0.0);
  int k = 0, L = 0, scoring = 0, weighting = 0, line = 0, line0 = 0;
  bool header = false;
  size_t at = 0;
  while (at < text.size()) {
    size_t end = text.find('\n', at);
    if (end == std::string::npos) end = text.size();
    std::string s = text.substr(at, end - at);
    at = end + 1;
    ++line;
    if (s.find_first_not_of(" \t\r") == std::string::npos) continue;
    const std::string ln = "line " + std::to_string(line);
    const char* p = s.c_str();
    char* e = nullptr;
    auto next_int = [&](long& v) {
      errno = 0;
      v = strtol(p, &e, 10);
      if (e == p || errno) return false;
      p = e;
      return true;
    };
    if (!header) {
      long v[4];
      for (int j = 0; j < 4; ++j)
        if (!next_int(v[j])) return bow_fail(nullptr, who, ln + ": the header is `k L scoring weighting`");
      k = (int)v[0]; L = (int)v[1]; scoring = (int)v[2]; weighting = (int)v[3];
      if (k < 2 || k > BOW_MAX_K) return bow_fail(nullptr, who, ln + ": k must be 2 .. 20");
      if (L < 1 || L > BOW_MAX_L) return bow_fail(nullptr, who, ln + ": L must be 1 .. 10");
      if (scoring != 0) return bow_fail(nullptr, who, ln + ": scoring must be 0 (L1_NORM)");
      if (weighting < 0 || weighting > 3) return bow_fail(nullptr, who, ln + ": weighting must be 0 .. 3 (TF_IDF, TF, IDF, BINARY)");
      header = true;
      continue;
    }
    if (parents.size() == 1) line0 = line;
    else if (line != line0 + (int)parents.size() - 1) return bow_fail(nullptr, who, ln + ": an empty line between nodes");
    long pid, isleaf;
    if (!next_int(pid) || !next_int(isleaf)) return bow_fail(nullptr, who, ln + ": a node is `parent is_leaf b0 .. b31 weight`");
    if (pid < 0 || pid >= (long)parents.size())
      return bow_fail(nullptr, who, ln + ": parent " + std::to_string(pid) + " is not defined yet");
    parents.push_back((int32_t)pid);
    leaf.push_back(isleaf > 0);
    for (int j = 0; j < 32; ++j) {
      long b;
      if (!next_int(b) || b < 0 || b > 255) return bow_fail(nullptr, who, ln + ": descriptor byte " + std::to_string(j) + " must be 0 .. 255");
      desc.push_back((uint8_t)b);
    }
    const double w = strtod(p, &e);
    if (e == p) return bow_fail(nullptr, who, ln + ": the weight is missing");
    p = e;
    if (*(p + strspn(p, " \t\r")) != 0) return bow_fail(nullptr, who, ln + ": more than 35 values");
    weights.push_back(w);
  }
  if (!header) return bow_fail(nullptr, who, "line 1: the header is `k L scoring weighting`");
  return bow_build(who, device, k, L, weighting, (int)parents.size(), parents.data(), desc.data(), weights.data(), leaf.data(), line0,
                   max_kp, max_frames, out);
}

extern "C" int svo_bow_save_text(svo_bow* bow, const char* path) {
  const char* who = "svo_bow_save_text";
  if (!bow) return bow_fail(nullptr, who, "bow is NULL");
  if (!path) return bow_fail(bow, who, "path is NULL");
  FILE* fp = fopen(path, "w");
  if (!fp) return bow_fail(bow, who, std::string("cannot write ") + path);
  fprintf(fp, "%d %d  0 %d\n", bow->k, bow->L, bow->weighting);     // (saveToTextFile's two blanks)
  for (size_t id = 1; id < bow->parent.size(); ++id) {
    fprintf(fp, "%d %d", bow->parent[id], bow->children[id].empty() ? 1 : 0);
    for (int j = 0; j < 32; ++j) fprintf(fp, " %d", (int)bow->desc[id * 32 + j]);
    fprintf(fp, " %.17g\n", bow->weight[id]);
  }
  if (fclose(fp) != 0) return bow_fail(bow, who, std::string("cannot write ") + path);
  return SVO_OK;
}

extern "C" int svo_bow_describe(const svo_bow* bow, int* k, int* L, int* n_nodes, int* n_words, int* weighting) {
  if (!bow) return bow_fail(nullptr, "svo_bow_describe", "bow is NULL");
  if (k) *k = bow->k;
  if (L) *L = bow->L;
  if (n_nodes) *n_nodes = (int)bow->parent.size();
  if (n_words) *n_words = bow->n_words;
  if (weighting) *weighting = bow->weighting;
  return SVO_OK;
}

extern "C" void svo_bow_destroy(svo_bow* bow) {
  if (!bow) return;
  if (bow->stream) {
    hipSetDevice(bow->device);
    hipStreamSynchronize(bow->stream);
    if (bow->d_tree) hipFree(bow->d_tree);
    if (bow->d_sword) hipFree(bow->d_sword);
    if (bow->d_snode) hipFree(bow->d_snode);
    if (bow->d_stage) hipFree(bow->d_stage);
    if (bow->producer_done) hipEventDestroy(bow->producer_done);
    hipStreamDestroy(bow->stream);
  }
  delete bow;
}

extern "C" int svo_bow_sync(svo_bow* bow) {
  if (!bow) return SVO_E_INVALID;
  if (!bow->ready) return SVO_OK;
  hipSetDevice(bow->device);
  BOW_HIP(bow, hipStreamSynchronize(bow->stream));
  return SVO_OK;
}

extern "C" void* svo_bow_stream(svo_bow* bow) {
  if (!bow || bow_ready(bow) != SVO_OK) return nullptr;
  return bow->stream;
}

extern "C" int svo_bow_transform_dev(svo_bow* bow, const uint8_t* d_desc, const int32_t* d_n, int kp_stride, int B, int levelsup,
                                     int32_t* d_words, svo_bow_entry* d_vec, int32_t* d_vec_n, svo_bow_feature* d_fv,
                                     int32_t* d_fv_n, svo_ctx* producer) {
  const char* who = "svo_bow_transform_dev";
  if (!bow) return bow_fail(nullptr, who, "bow is NULL");
  if (!d_desc) return bow_fail(bow, who, "d_desc is NULL");
  if (!d_n) return bow_fail(bow, who, "d_n is NULL");
  if (reinterpret_cast<uintptr_t>(d_desc) & 3u) return bow_fail(bow, who, "d_desc is not 4-byte aligned");
  if (kp_stride < 1 || kp_stride > bow->max_kp) return bow_fail(bow, who, "kp_stride must be 1 .. max_kp");
  if (B < 1 || B > bow->max_frames) return bow_fail(bow, who, "B must be 1 .. max_frames");
  if (levelsup < 0) return bow_fail(bow, who, "levelsup is negative");
  if (producer && producer->device != bow->device) return bow_fail(bow, who, "producer context on another device");
  if (int rc = bow_ready(bow)) return rc;
  if (producer) {     // behind the front end call that writes the descriptors; the producer waits for nothing
    BOW_HIP(bow, hipEventRecord(bow->producer_done, producer->stream));
    BOW_HIP(bow, hipStreamWaitEvent(bow->stream, bow->producer_done, 0));
  }
  WordsArgs W;
  W.T = bow->T; W.desc = d_desc; W.n = d_n; W.kp_stride = kp_stride; W.levelsup = levelsup;
  W.s_word = bow->d_sword; W.s_node = bow->d_snode; W.s_stride = bow->max_kp; W.words = d_words;
  const int per_block = BOW_NT / BOW_GROUP;
  hipLaunchKernelGGL(k_bow_words, dim3((kp_stride + per_block - 1) / per_block, B), dim3(BOW_NT), 0, bow->stream, W);
  if (d_vec || d_vec_n || d_fv || d_fv_n) {
    VectorArgs V;
    V.T = bow->T; V.n = d_n; V.kp_stride = kp_stride;
    V.s_word = bow->d_sword; V.s_node = bow->d_snode; V.s_stride = bow->max_kp;
    V.vec = d_vec; V.vec_n = d_vec_n; V.fv = d_fv; V.fv_n = d_fv_n;
    hipLaunchKernelGGL(k_bow_vector, dim3(B), dim3(BOW_NT), 0, bow->stream, V);
  }
  BOW_HIP(bow, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_bow_transform(svo_bow* bow, const uint8_t* desc, int n, int levelsup, int32_t* words, svo_bow_entry* vec,
                                 int32_t* vec_n, svo_bow_feature* fv, int32_t* fv_n) {
  const char* who = "svo_bow_transform";
  if (!bow) return bow_fail(nullptr, who, "bow is NULL");
  if (n < 0 || n > bow->max_kp) return bow_fail(bow, who, "n must be 0 .. max_kp");
  if (n > 0 && !desc) return bow_fail(bow, who, "desc is NULL");
  if (levelsup < 0) return bow_fail(bow, who, "levelsup is negative");
  if ((vec == nullptr) != (vec_n == nullptr)) return bow_fail(bow, who, "vec and vec_n go together");
  if ((fv == nullptr) != (fv_n == nullptr)) return bow_fail(bow, who, "fv and fv_n go together");
  if (int rc = bow_ready(bow)) return rc;
  const BowStage s = bow_stage(bow);
  uint8_t* d = bow->d_stage;
  const int32_t n32 = n;
  BOW_HIP(bow, hipStreamSynchronize(bow->stream));
  if (n > 0) BOW_HIP(bow, hipMemcpyAsync(d + s.desc, desc, (size_t)n * 32, hipMemcpyHostToDevice, bow->stream));
  BOW_HIP(bow, hipMemcpyAsync(d + s.n, &n32, sizeof n32, hipMemcpyHostToDevice, bow->stream));
  BOW_HIP(bow, hipStreamSynchronize(bow->stream));      // (n32 is a local)
  if (int rc = svo_bow_transform_dev(bow, d + s.desc, reinterpret_cast<const int32_t*>(d + s.n), bow->max_kp, 1, levelsup,
                                     reinterpret_cast<int32_t*>(d + s.words), reinterpret_cast<svo_bow_entry*>(d + s.vec),
                                     reinterpret_cast<int32_t*>(d + s.vec_n), reinterpret_cast<svo_bow_feature*>(d + s.fv),
                                     reinterpret_cast<int32_t*>(d + s.fv_n), nullptr))
    return rc;
  int32_t cnt[2] = {0, 0};
  BOW_HIP(bow, hipMemcpyAsync(&cnt[0], d + s.vec_n, sizeof(int32_t), hipMemcpyDeviceToHost, bow->stream));
  BOW_HIP(bow, hipMemcpyAsync(&cnt[1], d + s.fv_n, sizeof(int32_t), hipMemcpyDeviceToHost, bow->stream));
  if (words && n > 0) BOW_HIP(bow, hipMemcpyAsync(words, d + s.words, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, bow->stream));
  BOW_HIP(bow, hipStreamSynchronize(bow->stream));
  if (vec) {
    *vec_n = cnt[0];
    if (cnt[0] > 0) BOW_HIP(bow, hipMemcpyAsync(vec, d + s.vec, (size_t)cnt[0] * sizeof(svo_bow_entry), hipMemcpyDeviceToHost, bow->stream));
  }
  if (fv) {
    *fv_n = cnt[1];
    if (cnt[1] > 0) BOW_HIP(bow, hipMemcpyAsync(fv, d + s.fv, (size_t)cnt[1] * sizeof(svo_bow_feature), hipMemcpyDeviceToHost, bow->stream));
  }
  BOW_HIP(bow, hipStreamSynchronize(bow->stream));
  return SVO_OK;
}

extern "C" int svo_bow_score_dev(svo_bow* bow, const svo_bow_entry* d_vecA, const int32_t* d_nA, int QA, const svo_bow_entry* d_vecB,
                                 const int32_t* d_nB, int NB, int stride, double* d_scores) {
  const char* who = "svo_bow_score_dev";
  if (!bow) return bow_fail(nullptr, who, "bow is NULL");
  if (!d_vecA || !d_nA || !d_vecB || !d_nB || !d_scores) return bow_fail(bow, who, "d_vecA, d_nA, d_vecB, d_nB or d_scores is NULL");
  if ((reinterpret_cast<uintptr_t>(d_vecA) | reinterpret_cast<uintptr_t>(d_vecB) | reinterpret_cast<uintptr_t>(d_scores)) & 7u)
    return bow_fail(bow, who, "d_vecA, d_vecB or d_scores is not 8-byte aligned");
  if (QA < 1 || QA > 65535) return bow_fail(bow, who, "QA must be 1 .. 65535");
  if (NB < 1) return bow_fail(bow, who, "NB must be >= 1");
  if (stride < 1 || stride > bow->max_kp) return bow_fail(bow, who, "stride must be 1 .. max_kp");
  if (int rc = bow_ready(bow)) return rc;
  hipLaunchKernelGGL(k_bow_score, dim3((NB + BOW_WAVES - 1) / BOW_WAVES, QA), dim3(BOW_NT), 0, bow->stream, d_vecA, d_nA, d_vecB, d_nB,
                     NB, stride, d_scores);
  BOW_HIP(bow, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_bow_query_dev(svo_bow* bow, const svo_bow_entry* d_vec, const int32_t* d_vec_n, int stride, int N, int q0, int Q,
                                 int gap, double min_score, int top_k, svo_bow_cand* d_cand, int32_t* d_cand_n) {
  const char* who = "svo_bow_query_dev";
  if (!bow) return bow_fail(nullptr, who, "bow is NULL");
  if (!d_vec || !d_vec_n || !d_cand || !d_cand_n) return bow_fail(bow, who, "d_vec, d_vec_n, d_cand or d_cand_n is NULL");
  if ((reinterpret_cast<uintptr_t>(d_vec) | reinterpret_cast<uintptr_t>(d_cand)) & 7u)
    return bow_fail(bow, who, "d_vec or d_cand is not 8-byte aligned");
  if (stride < 1 || stride > bow->max_kp) return bow_fail(bow, who, "stride must be 1 .. max_kp");
  if (N < 1) return bow_fail(bow, who, "N must be >= 1");
  if (q0 < 0 || Q < 1 || Q > N - q0) return bow_fail(bow, who, "the queries q0 .. q0 + Q - 1 must lie in 0 .. N - 1");
  if (gap < 0) return bow_fail(bow, who, "gap is negative");
  if (min_score != min_score) return bow_fail(bow, who, "min_score is not a number");
  if (top_k < 1 || top_k > BOW_MAX_TOP) return bow_fail(bow, who, "top_k must be 1 .. 16");
  if (int rc = bow_ready(bow)) return rc;
  QueryArgs A;
  A.vec = d_vec; A.n = d_vec_n; A.stride = stride; A.q0 = q0; A.gap = gap; A.top_k = top_k; A.min_score = min_score;
  A.cand = d_cand; A.cand_n = d_cand_n;
  hipLaunchKernelGGL(k_bow_query, dim3(Q), dim3(BOW_NT), 0, bow->stream, A);
  BOW_HIP(bow, hipGetLastError());
  return SVO_OK;
}

extern "C" int svo_bow_assign_dev(svo_bow* bow, const uint8_t* d_desc, int n, const uint8_t* d_centres, int k, int32_t* d_idx,
                                  int32_t* d_dist) {
  const char* who = "svo_bow_assign_dev";
  if (!bow) return bow_fail(nullptr, who, "bow is NULL");
  if (!d_desc || !d_centres) return bow_fail(bow, who, "d_desc or d_centres is NULL");
  if ((reinterpret_cast<uintptr_t>(d_desc) | reinterpret_cast<uintptr_t>(d_centres)) & 3u)
    return bow_fail(bow, who, "d_desc or d_centres is not 4-byte aligned");
  if (n < 1) return bow_fail(bow, who, "n must be >= 1");
  if (k < 1 || k > BOW_MAX_K) return bow_fail(bow, who, "k must be 1 .. 20");
  if (int rc = bow_ready(bow)) return rc;
  const int per_block = BOW_NT / BOW_GROUP;
  hipLaunchKernelGGL(k_bow_assign, dim3((n + per_block - 1) / per_block), dim3(BOW_NT), 0, bow->stream, d_desc, n, d_centres, k, d_idx,
                     d_dist);
  BOW_HIP(bow, hipGetLastError());
  return SVO_OK;
}
