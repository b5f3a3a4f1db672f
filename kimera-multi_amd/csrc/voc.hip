// voc.hip — DBoW2's vocabulary transform on MI355X (gfx950): 32-byte ORB
// descriptors to L1-normalised BowVectors, the step in front of bow.hip.
//
// Restates TemplatedVocabulary<FORB>::transform(features, BowVector&) [U: DBoW2
// is not vendored; the semantics are the published algorithm, restated in
// tests/bow_transform_ref.py] behind kmx_voc_* (include/kmx_abi.h).
//
//   * The tree is held breadth first (voc_host.h): a node's children are one
//     contiguous block of 32-byte descriptors in DBoW2's load order, and the
//     top of the tree is a prefix of the node array.
//   * k_voc_descend: one lane per descriptor (8 VGPRs). Per level the lane
//     reads its node's child block, takes the child of least Hamming distance
//     (a later child only on a strictly smaller distance, so the first of equal
//     children wins) and stops at a node without children. The first
//     VOC_LDS_NODES nodes (levels 0-3 of a k = 10 tree) are staged in LDS by
//     every workgroup; deeper blocks are read with 16-byte global loads,
//     VOC_CHUNK children per step with the loads issued together. The child
//     records (first, count) of a block are read beside its descriptors, so a
//     level is one dependent memory round trip, not two.
//   * k_voc_reduce: one workgroup per frame. The word ids of the features with
//     a positive leaf weight are sorted in LDS (bitonic, as bow.hip), equal ids
//     are run-length counted, a word seen c times gets its weight by c - 1
//     sequential additions (DBoW2's addWeight; IDF / BINARY store the weight
//     once), one lane sums |v| in increasing word id and every value is
//     divided by that sum. The order of every floating-point operation is
//     DBoW2's, so the vectors equal the CPU restatement bit for bit.
// Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "voc_host.h"

namespace {

#ifndef KMX_VOC_BLOCK
#define KMX_VOC_BLOCK 512
#endif
constexpr int VOC_BLOCK = KMX_VOC_BLOCK;  // k_voc_descend: lanes (descriptors) per workgroup pass
constexpr int VOC_LDS_NODES = 1280;   // nodes staged in LDS (40 KiB of descriptors + 10 KiB of child records)
#ifndef KMX_VOC_CHUNK
#define KMX_VOC_CHUNK 10
#endif
// children whose loads are issued together: 10 measured 2.65 ms per 12.5 M
// descriptors (k = 10, L = 6) against 3.52 ms for 5 and 3.62 ms for 2, although
// its 142 VGPRs leave one workgroup per CU
constexpr int VOC_CHUNK = KMX_VOC_CHUNK;
constexpr int RED_BLOCK = 256;        // k_voc_reduce
constexpr int RED_MAX = 1024;         // max_feats, as lcd.hip
constexpr int RED_PER = RED_MAX / RED_BLOCK;
constexpr unsigned NO_WORD = 0xffffffffu;

struct VocDev {
  const uint4* desc;     // [n_nodes][2]
  const int2* child;     // [n_nodes] (first, count); count 0 = leaf
  const int* word_of;    // [n_nodes]
  const double* weight;  // [n_nodes]
  const double* word_weight;  // [n_words]
  int n_nodes, n_lds;
};

__device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
         __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// leaf[t] = the leaf node (device numbering) of feature slot t = frame * N + i
// of the batch, or -1 for a slot beyond its frame's n_feats (whose descriptor
// bytes are never read). Frame f of the batch is frame fid[f] of the
// descriptor pool (fid == nullptr: f itself).
#ifdef KMX_VOC_WAVES  // A/B: cap the registers so that this many waves fit a SIMD
__attribute__((amdgpu_waves_per_eu(KMX_VOC_WAVES, KMX_VOC_WAVES)))
#endif
__global__ __launch_bounds__(VOC_BLOCK) void k_voc_descend(VocDev v, long long total, int N, const int* n_feats,
                                                           const int* fid, const uint4* desc, int* leaf) {
  __shared__ uint4 s_desc[VOC_LDS_NODES * 2];
  __shared__ int2 s_child[VOC_LDS_NODES];
  for (int i = threadIdx.x; i < v.n_lds * 2; i += VOC_BLOCK) s_desc[i] = v.desc[i];
  for (int i = threadIdx.x; i < v.n_lds; i += VOC_BLOCK) s_child[i] = v.child[i];
  __syncthreads();
  const long long stride = (long long)gridDim.x * VOC_BLOCK;
  for (long long t = (long long)blockIdx.x * VOC_BLOCK + threadIdx.x; t < total; t += stride) {
    const int f = (int)(t / N), i = (int)(t - (long long)f * N);
    const int src = fid ? fid[f] : f;
    if (i >= n_feats[src]) {
      leaf[t] = -1;
      continue;
    }
    const uint4* dp = desc + ((size_t)src * N + i) * 2;
    const uint4 d0 = dp[0], d1 = dp[1];
    int node = 0;
    int2 c = s_child[0];
    for (int depth = 0; depth < kmx::VOC_MAX_DEPTH && c.y > 0; ++depth) {
      const int first = c.x, cnt = c.y;
      int best = 0x7fffffff, bi = first;
      int2 bc = make_int2(0, 0);
      if (first + cnt <= v.n_lds) {
        for (int j = 0; j < cnt; ++j) {
          const int dist = hamming256(d0, d1, s_desc[(first + j) * 2], s_desc[(first + j) * 2 + 1]);
          if (dist < best) { best = dist; bi = first + j; bc = s_child[first + j]; }
        }
      } else {
        // VOC_CHUNK children per step, indices clamped to the block's last
        // child: a repeated last child has that child's distance, which is
        // never strictly smaller than the best so far, so it changes nothing
        for (int j0 = 0; j0 < cnt; j0 += VOC_CHUNK) {
          uint4 r0[VOC_CHUNK], r1[VOC_CHUNK];
          int2 rc[VOC_CHUNK];
#pragma unroll
          for (int u = 0; u < VOC_CHUNK; ++u) {
            const int n = first + min(j0 + u, cnt - 1);
            r0[u] = v.desc[(size_t)n * 2];
            r1[u] = v.desc[(size_t)n * 2 + 1];
            rc[u] = v.child[n];
          }
#pragma unroll
          for (int u = 0; u < VOC_CHUNK; ++u) {
            const int dist = hamming256(d0, d1, r0[u], r1[u]);
            if (dist < best) { best = dist; bi = first + min(j0 + u, cnt - 1); bc = rc[u]; }
          }
        }
      }
      node = bi;
      c = bc;
    }
    leaf[t] = node;
  }
}

// One workgroup per frame: leaves -> sorted words -> weights -> L1 norm.
// Outputs at stride N: nnz[f], words[f][0 .. nnz), weights[f][0 .. nnz).
__global__ __launch_bounds__(RED_BLOCK) void k_voc_reduce(VocDev v, int N, int additive, const int* leaf, int* nnz,
                                                          unsigned* words, double* weights) {
  __shared__ unsigned key[RED_MAX];
  __shared__ int start[RED_MAX + 1];
  __shared__ double val[RED_MAX];
  __shared__ int s_wsum[RED_BLOCK / 64];
  __shared__ int s_nh, s_nv;
  __shared__ double s_sum;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const size_t base = (size_t)blockIdx.x * N;
  int n2 = 1;
  while (n2 < N) n2 <<= 1;
  int mine = 0;
  for (int i = tid; i < RED_MAX; i += RED_BLOCK) {
    unsigned k = NO_WORD;
    if (i < N) {
      const int node = leaf[base + i];
      if (node >= 0 && v.weight[node] > 0.0) { k = (unsigned)v.word_of[node]; ++mine; }
    }
    key[i] = k;
  }
  if (tid == 0) s_nv = 0;
  __syncthreads();
  if (mine) atomicAdd(&s_nv, mine);
  // bitonic sort, ascending (the slots beyond the features hold NO_WORD, the largest key)
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += RED_BLOCK) {
        const int l = i ^ j;
        if (l > i) {
          const bool up = (i & k) == 0;
          const unsigned a = key[i], b = key[l];
          if (up ? b < a : a < b) { key[i] = b; key[l] = a; }
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();
  // run heads and their ranks: an exclusive scan of the head flags, RED_PER
  // consecutive slots per thread
  bool head[RED_PER];
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < RED_PER; ++k) {
    const int p = tid * RED_PER + k;
    head[k] = key[p] != NO_WORD && (p == 0 || key[p - 1] != key[p]);
    cnt += head[k] ? 1 : 0;
  }
  int incl = cnt;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 63) s_wsum[w] = incl;
  __syncthreads();
  int rank = incl - cnt;
  for (int k = 0; k < w; ++k) rank += s_wsum[k];
#pragma unroll
  for (int k = 0; k < RED_PER; ++k)
    if (head[k]) start[rank++] = tid * RED_PER + k;
  if (tid == RED_BLOCK - 1) {
    s_nh = rank;
    start[rank] = s_nv;  // end of the last run: the count of contributing features
  }
  __syncthreads();
  const int nh = s_nh;
  for (int r = tid; r < nh; r += RED_BLOCK) {
    const int c = start[r + 1] - start[r];
    const double wt = v.word_weight[key[start[r]]];
    double x = wt;
    if (additive)
      for (int k = 1; k < c; ++k) x += wt;  // addWeight, once per further occurrence
    val[r] = x;
  }
  __syncthreads();
  if (tid == 0) {  // the L1 norm in increasing word id, one addition at a time
    double s = 0.0;
    for (int r = 0; r < nh; ++r) s += fabs(val[r]);
    s_sum = s;
  }
  __syncthreads();
  const double s = s_sum;
  for (int r = tid; r < nh; r += RED_BLOCK) {
    words[base + r] = key[start[r]];
    weights[base + r] = s > 0.0 ? val[r] / s : val[r];
  }
  if (tid == 0) nnz[blockIdx.x] = nh;
}

// The batch buffers (grow-only, replaced as a whole): uploaded descriptors /
// counts / frame ids, leaves, outputs.
struct VocBatch {
  kmx::DevBuf<uint4> in;                 // [dcap()][2]; only the host path has it
  kmx::DevBuf<int> nfeat, fid, nnz;      // [fcap()]
  kmx::DevBuf<int> leaf;                 // [scap()]
  kmx::DevBuf<unsigned> words;           // [scap()]
  kmx::DevBuf<double> weights;           // [scap()]
  size_t fcap() const { return nnz.cap(); }      // frames
  size_t scap() const { return weights.cap(); }  // feature slots
  size_t dcap() const { return in.cap() / 2; }   // uploaded descriptor slots
};

}  // namespace

struct kmx_voc : kmx::StreamCore {
  int n_nodes = 0, n_words = 0, max_children = 0, max_depth = 0, n_lds = 0, weighting = 0;
  int grid = 0;
  kmx::DevBuf<uint4> d_desc;
  kmx::DevBuf<int2> d_child;
  kmx::DevBuf<int> d_word_of;
  kmx::DevBuf<double> d_weight;
  kmx::DevBuf<double> d_word_weight;
  VocBatch b;
  int last_frames = 0, last_N = 0;  // the batch whose outputs the device holds
  kmx::Event ev_pool;               // orders a pool transform after the detector's stream
  bool timing = false;
  kmx::Event ev[3];
};

namespace {

// Room for a batch of n frames at stride N (and, for the host path, its descriptors).
int voc_reserve(kmx_voc* h, size_t n, size_t N, bool upload) {
  const size_t slots = n * N;
  if (n <= h->b.fcap() && slots <= h->b.scap() && (!upload || slots <= h->b.dcap())) return 0;
  KMX_HIP(hipStreamSynchronize(h->stream));  // a batch in flight uses the old buffers
  const size_t fcap = std::max(n, h->b.fcap()), scap = std::max(slots, h->b.scap());
  const size_t dcap = upload ? std::max(slots, h->b.dcap()) : h->b.dcap();
  h->b = VocBatch();  // the old batch goes first; a failure below leaves the handle without one
  VocBatch b;
  int rc;
  if ((rc = b.nfeat.alloc(fcap)) || (rc = b.fid.alloc(fcap)) || (rc = b.nnz.alloc(fcap)) ||
      (rc = b.leaf.alloc(scap)) || (rc = b.words.alloc(scap)) || (rc = b.weights.alloc(scap)) ||
      (dcap && (rc = b.in.alloc(dcap * 2))))
    return rc;
  h->b = std::move(b);
  return 0;
}

// Both kernels for n frames at stride N over the descriptor pool `desc`
// (counts d_nf indexed by pool frame; d_fid: batch frame -> pool frame, or null).
int voc_launch(kmx_voc* h, int n, int N, const int* d_nf, const int* d_fid, const uint4* desc) {
  VocDev v{h->d_desc.get(), h->d_child.get(), h->d_word_of.get(), h->d_weight.get(), h->d_word_weight.get(), h->n_nodes,
           h->n_lds};
  const long long total = (long long)n * N;
  const int grid = (int)std::min<long long>((total + VOC_BLOCK - 1) / VOC_BLOCK, h->grid);
  if (h->timing) KMX_HIP(hipEventRecord(h->ev[0], h->stream));
  hipLaunchKernelGGL(k_voc_descend, dim3(grid), dim3(VOC_BLOCK), 0, h->stream, v, total, N, d_nf, d_fid, desc,
                     h->b.leaf.get());
  KMX_HIP(hipGetLastError());
  if (h->timing) KMX_HIP(hipEventRecord(h->ev[1], h->stream));
  hipLaunchKernelGGL(k_voc_reduce, dim3(n), dim3(RED_BLOCK), 0, h->stream, v, N, h->weighting <= 1 ? 1 : 0,
                     (const int*)h->b.leaf.get(), h->b.nnz.get(), h->b.words.get(), h->b.weights.get());
  KMX_HIP(hipGetLastError());
  if (h->timing) KMX_HIP(hipEventRecord(h->ev[2], h->stream));
  h->last_frames = n;
  h->last_N = N;
  return 0;
}

int voc_fetch(kmx_voc* h, int32_t* out_nnz, uint32_t* out_words, double* out_weights) {
  const size_t n = (size_t)h->last_frames, slots = n * h->last_N;
  KMX_HIP(hipMemcpyAsync(out_nnz, h->b.nnz.get(), sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipMemcpyAsync(out_words, h->b.words.get(), sizeof(unsigned) * slots, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipMemcpyAsync(out_weights, h->b.weights.get(), sizeof(double) * slots, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

}  // namespace

int kmx::voc_batch_view(kmx_voc* h, kmx::VocBatchView* out) {
  KMX_CHECK(h && out, KMX_EINVAL, "null argument");
  out->device = h->device;
  out->n_words = h->n_words;
  out->n_frames = h->last_frames;
  out->stride = h->last_N;
  out->nnz = h->b.nnz.get();
  out->words = h->b.words.get();
  out->weights = h->b.weights.get();
  out->stream = h->stream;
  return KMX_OK;
}

extern "C" int kmx_voc_create(int device, int32_t n_nodes, const int32_t* parent, const uint8_t* descriptor,
                              const double* weight, int32_t n_words, const int32_t* word_node, int weighting,
                              kmx_voc** out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(out, KMX_EINVAL, "null argument");
  // the tree is checked before any device call
  kmx::VocLayout L;
  std::string err;
  if (int rc = kmx::voc_prepare(n_nodes, parent, descriptor, weight, n_words, word_node, weighting, &L, &err))
    return kmx::fail(rc, err);
  std::unique_ptr<kmx_voc> h(new kmx_voc());  // a failure below unwinds through the members' destructors
  int rc;
  if ((rc = h->open(device))) return rc;
  h->n_nodes = L.n_nodes;
  h->n_words = L.n_words;
  h->max_children = L.max_children;
  h->max_depth = L.max_depth;
  h->weighting = weighting;
  h->n_lds = std::min(L.n_nodes, VOC_LDS_NODES);
  // the descent's grid: the workgroups resident at once (registers and the 50 KiB LDS stage decide)
  int cus = 256, per_cu = 1;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_voc_descend, VOC_BLOCK, 0) != hipSuccess || per_cu < 1)
    per_cu = 1;
  h->grid = std::max(1, cus) * per_cu;
  if ((rc = h->ev_pool.create(hipEventDisableTiming)) || (rc = kmx::create_events(h->ev))) return rc;
  std::vector<int2> child((size_t)L.n_nodes);
  for (int i = 0; i < L.n_nodes; ++i) child[i] = make_int2(L.child_first[i], L.child_count[i]);
  if ((rc = h->d_desc.alloc((size_t)L.n_nodes * 2)) || (rc = h->d_child.alloc(child.size())) ||
      (rc = h->d_word_of.alloc(L.word_of.size())) || (rc = h->d_weight.alloc(L.weight.size())) ||
      (rc = h->d_word_weight.alloc(L.word_weight.size())))
    return rc;
  hipError_t e = hipMemcpy(h->d_desc.get(), L.desc.data(), sizeof(uint32_t) * L.desc.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_child.get(), child.data(), sizeof(int2) * child.size(),
                                     hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(h->d_word_of.get(), L.word_of.data(), sizeof(int) * L.word_of.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(h->d_weight.get(), L.weight.data(), sizeof(double) * L.weight.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(h->d_word_weight.get(), L.word_weight.data(), sizeof(double) * L.word_weight.size(),
                  hipMemcpyHostToDevice);
  if (e != hipSuccess) return kmx::fail(KMX_EHIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
  *out = h.release();
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_voc_destroy(kmx_voc* h) {
  return kmx::destroy(h);
}

extern "C" int kmx_voc_set_stream(kmx_voc* h, void* s) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  return h->adopt(s, true);
}

extern "C" int kmx_voc_info(kmx_voc* h, int32_t* n_nodes, int32_t* n_words, int32_t* max_children,
                            int32_t* max_depth, int32_t* lds_nodes, int32_t* descend_grid) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  if (n_nodes) *n_nodes = h->n_nodes;
  if (n_words) *n_words = h->n_words;
  if (max_children) *max_children = h->max_children;
  if (max_depth) *max_depth = h->max_depth;
  if (lds_nodes) *lds_nodes = h->n_lds;
  if (descend_grid) *descend_grid = h->grid;
  return KMX_OK;
}

extern "C" int kmx_voc_transform_async(kmx_voc* h, int32_t n_frames, int32_t max_feats, const int32_t* n_feats,
                                       const uint8_t* desc) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(n_frames >= 0 && max_feats >= 1 && max_feats <= RED_MAX, KMX_EINVAL,
            "need n_frames >= 0 and 1 <= max_feats <= 1024");
  KMX_CHECK(n_frames == 0 || (n_feats && desc), KMX_EINVAL, "null frame array");
  for (int f = 0; f < n_frames; ++f)
    KMX_CHECK(n_feats[f] >= 0 && n_feats[f] <= max_feats, KMX_EINVAL, "bad n_feats");
  KMX_HIP(hipSetDevice(h->device));
  h->last_frames = 0;
  if (n_frames == 0) return KMX_OK;
  if (int rc = voc_reserve(h, (size_t)n_frames, (size_t)max_feats, true)) return rc;
  const size_t slots = (size_t)n_frames * max_feats;
  KMX_HIP(hipMemcpyAsync(h->b.in.get(), desc, slots * 32, hipMemcpyHostToDevice, h->stream));
  KMX_HIP(hipMemcpyAsync(h->b.nfeat.get(), n_feats, sizeof(int) * n_frames, hipMemcpyHostToDevice, h->stream));
  return voc_launch(h, n_frames, max_feats, h->b.nfeat.get(), nullptr, h->b.in.get());
  KMX_GUARD_END
}

extern "C" int kmx_voc_transform(kmx_voc* h, int32_t n_frames, int32_t max_feats, const int32_t* n_feats,
                                 const uint8_t* desc, int32_t* out_nnz, uint32_t* out_words, double* out_weights) {
  KMX_GUARD_BEGIN
  KMX_CHECK(out_nnz && out_words && out_weights, KMX_EINVAL, "null output");
  if (int rc = kmx_voc_transform_async(h, n_frames, max_feats, n_feats, desc)) return rc;
  if (n_frames == 0) return KMX_OK;
  return voc_fetch(h, out_nnz, out_words, out_weights);
  KMX_GUARD_END
}

extern "C" int kmx_voc_transform_pool_async(kmx_voc* h, kmx_lcd* pool, int32_t n, const int32_t* frame_ids) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && pool, KMX_EINVAL, "null handle");
  KMX_CHECK(n >= 0 && (n == 0 || frame_ids), KMX_EINVAL, "bad frame id array");
  kmx::LcdPoolView pv;
  if (int rc = kmx::lcd_pool_view(pool, &pv)) return rc;
  KMX_CHECK(pv.device == h->device, KMX_EINVAL, "the frame pool is on another device");
  for (int i = 0; i < n; ++i)
    KMX_CHECK(frame_ids[i] >= 0 && frame_ids[i] < pv.n_frames, KMX_EINVAL, "frame id outside the pool");
  KMX_HIP(hipSetDevice(h->device));
  h->last_frames = 0;
  if (n == 0) return KMX_OK;
  KMX_CHECK(pv.desc && pv.n_feats && pv.max_feats >= 1 && pv.max_feats <= RED_MAX, KMX_ESTATE,
            "the pool has no frames");
  if (int rc = voc_reserve(h, (size_t)n, (size_t)pv.max_feats, false)) return rc;
  // after whatever the detector has enqueued on its stream (frame uploads)
  KMX_HIP(hipEventRecord(h->ev_pool, pv.stream));
  KMX_HIP(hipStreamWaitEvent(h->stream, h->ev_pool, 0));
  KMX_HIP(hipMemcpyAsync(h->b.fid.get(), frame_ids, sizeof(int) * n, hipMemcpyHostToDevice, h->stream));
  return voc_launch(h, n, pv.max_feats, pv.n_feats, h->b.fid.get(), reinterpret_cast<const uint4*>(pv.desc));
  KMX_GUARD_END
}

extern "C" int kmx_voc_transform_pool(kmx_voc* h, kmx_lcd* pool, int32_t n, const int32_t* frame_ids,
                                      int32_t* out_nnz, uint32_t* out_words, double* out_weights) {
  KMX_GUARD_BEGIN
  KMX_CHECK(out_nnz && out_words && out_weights, KMX_EINVAL, "null output");
  if (int rc = kmx_voc_transform_pool_async(h, pool, n, frame_ids)) return rc;
  if (n == 0) return KMX_OK;
  return voc_fetch(h, out_nnz, out_words, out_weights);
  KMX_GUARD_END
}

extern "C" int kmx_voc_sync(kmx_voc* h) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
}

extern "C" int kmx_voc_enable_timing(kmx_voc* h, int enable) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  h->timing = enable != 0;
  return KMX_OK;
}

extern "C" int kmx_voc_read_timing(kmx_voc* h, double* descend_ms, double* reduce_ms) {
  KMX_CHECK(h && descend_ms && reduce_ms, KMX_EINVAL, "null argument");
  KMX_CHECK(h->timing && h->last_frames > 0, KMX_ESTATE, "no timed transform: kmx_voc_enable_timing, then transform");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  float a = 0.f, b = 0.f;
  KMX_HIP(hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
  KMX_HIP(hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
  *descend_ms = a;
  *reduce_ms = b;
  return KMX_OK;
}
