// simplify.hip — voxel simplification and the deformation graph's arrays on
// the device (kmx_simplify_*, include/kmx_abi.h): an append-only handle whose
// result after any sequence of appends is that of one batch call, and equals
// kmx.pgmo.simplify_voxel / graph_from_mesh value for value. Every output is
// an integer, a copied input or a given constant; the only floating-point
// operation that decides anything is the voxel index floor(double(x) /
// resolution), an fp64 division (simplify_host.h), and this file is compiled
// with -ffp-contract=off.
//
// No sort and no float atomic. Two open-addressing tables of 32-bit values:
// a slot of the vertex table names a vertex, a slot of the face table an input
// face; a slot's key is recomputed from what it names (the vertex's robot,
// stamp and xyz; the face's mapped corners), which no kernel writes while a
// table is probed. Insert claims an empty slot by compare-and-swap, lowers a
// slot of its own key by atomic min, and walks on otherwise; every access to a
// slot is a relaxed agent-scope atomic, and kernel boundaries order the phases
// (insert, find, scan, write). Where a key lands depends on the run, the
// minimum per key does not. A probe loop is bounded by the slot count and
// raises an error word when it runs out; nothing spins or waits on the device.
//
// Layout. Vertices by id: xyz fp32, robot, stamp, vertex_to_control. Control
// vertices by id: representative, xyz fp64, stamp, robot. Input faces by
// position: the mapped corners (the face table's keys). Kept faces: corners
// and input position. Edges and the graph are formed on request in buffers of
// their own.
#include <algorithm>
#include <climits>
#include <memory>
#include <vector>

#include "common.h"
#include "simplify_host.h"

namespace {

using kmx::SIMP_EMPTY;
using kmx::SIMP_SCAN_BLOCK;
using kmx::SIMP_SCAN_ITEMS;
using kmx::SIMP_SCAN_SPAN;
using kmx::SIMP_SCAN_TOP;
typedef unsigned long long u64;

constexpr int SIMP_BLOCK = 256;
constexpr int SIMP_HUB = 32;          // an edge bucket above this goes to the wave-per-bucket kernel
constexpr int SIMP_HUB_WAVES = 1024;  // its grid; a wave strides over the hub list
enum { ST_ERR = 0, ST_NEW_CONTROL = 1, ST_NEW_KEPT = 2, ST_EDGES = 3, ST_HUBS = 4, ST_WORDS = 8 };
enum { ERR_VTABLE = 1, ERR_FTABLE = 2 };

__device__ __forceinline__ uint32_t slot_load(uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool slot_claim(uint32_t* p, uint32_t* seen, uint32_t id) {
  return __hip_atomic_compare_exchange_strong(p, seen, id, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void slot_min(uint32_t* p, uint32_t id) {
  (void)__hip_atomic_fetch_min(p, id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ u64 mix64(u64 x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

// The key of a vertex, from the vertex's own row.
struct VKey {
  int r, ix, iy, iz;
  long long win;
  __device__ bool operator==(const VKey& o) const {
    return r == o.r && ix == o.ix && iy == o.iy && iz == o.iz && win == o.win;
  }
  __device__ u64 hash() const {
    u64 h = mix64((u64)(uint32_t)ix | ((u64)(uint32_t)iy << 32));
    h = mix64(h ^ ((u64)(uint32_t)iz | ((u64)(uint32_t)r << 32)));
    return mix64(h ^ (u64)win);
  }
};
struct VKeys {
  const float* xyz;
  const int* robot;
  const long long* stamp;
  double resolution;
  long long horizon;
  __device__ VKey operator()(uint32_t v) const {
    VKey k;
    k.r = robot[v];
    k.ix = (int)kmx::simp_voxel(xyz[3 * (size_t)v], resolution);
    k.iy = (int)kmx::simp_voxel(xyz[3 * (size_t)v + 1], resolution);
    k.iz = (int)kmx::simp_voxel(xyz[3 * (size_t)v + 2], resolution);
    k.win = kmx::simp_window(stamp[v], horizon);
    return k;
  }
};

// The key of an input face: its mapped corners, sorted.
struct FKey {
  int a, b, c;
  __device__ bool operator==(const FKey& o) const { return a == o.a && b == o.b && c == o.c; }
  __device__ u64 hash() const { return mix64(mix64((u64)(uint32_t)a | ((u64)(uint32_t)b << 32)) ^ (u64)(uint32_t)c); }
};
__device__ __forceinline__ FKey fkey_of(int x, int y, int z) {
  int t;
  if (x > y) { t = x; x = y; y = t; }
  if (y > z) { t = y; y = z; z = t; }
  if (x > y) { t = x; x = y; y = t; }
  return FKey{x, y, z};
}
struct FKeys {
  const int* fctl;  // [input position][3]
  __device__ FKey operator()(uint32_t p) const {
    return fkey_of(fctl[3 * (size_t)p], fctl[3 * (size_t)p + 1], fctl[3 * (size_t)p + 2]);
  }
};

// After the insert kernel a slot holds the lowest id of its key. false: the
// table is full (the host's size rule makes that a bug, never a wait).
template <class Keys>
__device__ bool tab_insert(uint32_t* tab, u64 slots, const Keys& keys, uint32_t id) {
  const auto me = keys(id);
  const u64 mask = slots - 1;
  u64 s = me.hash() & mask;
  for (u64 probe = 0; probe < slots; ++probe) {
    uint32_t cur = slot_load(tab + s);
    if (cur == SIMP_EMPTY) {
      if (slot_claim(tab + s, &cur, id)) return true;  // a failure leaves the occupant in cur
    }
    if (cur == id) return true;
    if (keys(cur) == me) {
      slot_min(tab + s, id);
      return true;
    }
    s = (s + 1) & mask;
  }
  return false;
}

// The value of id's key; SIMP_EMPTY when the key is absent.
template <class Keys>
__device__ uint32_t tab_find(uint32_t* tab, u64 slots, const Keys& keys, uint32_t id) {
  const auto me = keys(id);
  const u64 mask = slots - 1;
  u64 s = me.hash() & mask;
  for (u64 probe = 0; probe < slots; ++probe) {
    const uint32_t cur = slot_load(tab + s);
    if (cur == SIMP_EMPTY) return SIMP_EMPTY;
    if (cur == id || keys(cur) == me) return cur;
    s = (s + 1) & mask;
  }
  return SIMP_EMPTY;
}

// ------------------------------------------------------------------ vertices
// ids[i] (NULL: first + i) for i < n
__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_vinsert(uint32_t* tab, u64 slots, VKeys keys, const int* ids,
                                                             long long first, long long n, int* status) {
  const long long i = (long long)blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t v = ids ? (uint32_t)ids[i] : (uint32_t)(first + i);
  if (!tab_insert(tab, slots, keys, v)) atomicOr(status + ST_ERR, ERR_VTABLE);
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_vfind(uint32_t* tab, u64 slots, VKeys keys, long long first,
                                                           long long n, int* rep, int* flag, int* status) {
  const long long i = (long long)blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t v = (uint32_t)(first + i);
  uint32_t r = tab_find(tab, slots, keys, v);
  if (r == SIMP_EMPTY) {
    atomicOr(status + ST_ERR, ERR_VTABLE);
    r = v;
  }
  rep[i] = (int)r;
  flag[i] = r == v ? 1 : 0;
}

// New vertex first + i: a representative takes control id c0 + excl[i] and
// writes its control row; any other takes its representative's id, an older
// one's from vmap, a new one's from the scan.
__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_vwrite(long long first, long long n, int c0, const int* rep,
                                                            const int* flag, const int* excl, const float* xyz,
                                                            const int* robot, const long long* stamp, int* vmap,
                                                            int* crep, double* cxyz, long long* cstamp, int* crobot) {
  const long long i = (long long)blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (i >= n) return;
  const long long v = first + i;
  if (flag[i]) {
    const int c = c0 + excl[i];
    vmap[v] = c;
    crep[c] = (int)v;
    cxyz[3 * (size_t)c] = (double)xyz[3 * v];
    cxyz[3 * (size_t)c + 1] = (double)xyz[3 * v + 1];
    cxyz[3 * (size_t)c + 2] = (double)xyz[3 * v + 2];
    cstamp[c] = stamp[v];
    crobot[c] = robot[v];
  } else {
    const long long r = rep[i];
    vmap[v] = r < first ? vmap[r] : c0 + excl[r - first];
  }
}

// ---------------------------------------------------------------------- scan
// excl[i] = sum of flag[0 .. i) in three kernels: a workgroup's sum of its
// SIMP_SCAN_SPAN elements, one workgroup's exclusive scan of those sums
// (SIMP_SCAN_TOP at a time, with a carry), and the apply.
__device__ __forceinline__ int block_exclusive(int v, int* s_buf, int* total) {
  const int t = threadIdx.x;
  s_buf[t] = v;
  __syncthreads();
  for (int off = 1; off < SIMP_SCAN_BLOCK; off <<= 1) {
    const int add = t >= off ? s_buf[t - off] : 0;
    __syncthreads();
    s_buf[t] += add;
    __syncthreads();
  }
  const int incl = s_buf[t];
  *total = s_buf[SIMP_SCAN_BLOCK - 1];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(SIMP_SCAN_BLOCK) void k_simp_scan_part(const int* flag, long long n, int* part) {
  __shared__ int s_buf[SIMP_SCAN_BLOCK];
  const long long base = (long long)blockIdx.x * SIMP_SCAN_SPAN + (long long)threadIdx.x * SIMP_SCAN_ITEMS;
  int v = 0;
#pragma unroll
  for (int j = 0; j < SIMP_SCAN_ITEMS; ++j)
    if (base + j < n) v += flag[base + j];
  int total;
  (void)block_exclusive(v, s_buf, &total);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

__global__ __launch_bounds__(SIMP_SCAN_BLOCK) void k_simp_scan_top(int* part, long long nb, int* total_out) {
  __shared__ int s_buf[SIMP_SCAN_BLOCK];
  static_assert(SIMP_SCAN_TOP == SIMP_SCAN_BLOCK, "one partial per lane and pass");
  int carry = 0;
  for (long long b0 = 0; b0 < nb; b0 += SIMP_SCAN_TOP) {
    const long long b = b0 + threadIdx.x;
    const int v = b < nb ? part[b] : 0;
    int total;
    const int e = block_exclusive(v, s_buf, &total);
    if (b < nb) part[b] = carry + e;
    carry += total;
  }
  if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(SIMP_SCAN_BLOCK) void k_simp_scan_apply(const int* flag, long long n, const int* part,
                                                                     int* excl) {
  __shared__ int s_buf[SIMP_SCAN_BLOCK];
  const long long base = (long long)blockIdx.x * SIMP_SCAN_SPAN + (long long)threadIdx.x * SIMP_SCAN_ITEMS;
  int f[SIMP_SCAN_ITEMS];
  int v = 0;
#pragma unroll
  for (int j = 0; j < SIMP_SCAN_ITEMS; ++j) {
    f[j] = base + j < n ? flag[base + j] : 0;
    v += f[j];
  }
  int total;
  int e = part[blockIdx.x] + block_exclusive(v, s_buf, &total);
#pragma unroll
  for (int j = 0; j < SIMP_SCAN_ITEMS; ++j) {
    if (base + j < n) excl[base + j] = e;
    e += f[j];
  }
}

// --------------------------------------------------------------------- faces
__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_finsert_kept(uint32_t* tab, u64 slots, FKeys keys, const int* pos,
                                                                  long long n, int* status) {
  const long long i = (long long)blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (i >= n) return;
  if (!tab_insert(tab, slots, keys, (uint32_t)pos[i])) atomicOr(status + ST_ERR, ERR_FTABLE);
}

// Input face f0 + j: its corners through vmap into fctl; then into the table unless degenerate.
__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_fmap(const int* raw, const int* vmap, long long f0, long long n,
                                                          int* fctl) {
  const long long j = (long long)blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (j >= n) return;
  const long long p = f0 + j;
  const int a = vmap[raw[3 * j]], b = vmap[raw[3 * j + 1]], c = vmap[raw[3 * j + 2]];
  fctl[3 * p] = a;
  fctl[3 * p + 1] = b;
  fctl[3 * p + 2] = c;
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_finsert(uint32_t* tab, u64 slots, FKeys keys, long long f0,
                                                             long long n, int* status) {
  const long long j = (long long)blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (j >= n) return;
  const long long p = f0 + j;
  const int a = keys.fctl[3 * p], b = keys.fctl[3 * p + 1], c = keys.fctl[3 * p + 2];
  if (a == b || b == c || a == c) return;
  if (!tab_insert(tab, slots, keys, (uint32_t)p)) atomicOr(status + ST_ERR, ERR_FTABLE);
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_ffind(uint32_t* tab, u64 slots, FKeys keys, long long f0,
                                                           long long n, int* flag, int* status) {
  const long long j = (long long)blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (j >= n) return;
  const long long p = f0 + j;
  const int a = keys.fctl[3 * p], b = keys.fctl[3 * p + 1], c = keys.fctl[3 * p + 2];
  int keep = 0;
  if (!(a == b || b == c || a == c)) {
    const uint32_t r = tab_find(tab, slots, keys, (uint32_t)p);
    if (r == SIMP_EMPTY) atomicOr(status + ST_ERR, ERR_FTABLE);
    keep = r == (uint32_t)p ? 1 : 0;
  }
  flag[j] = keep;
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_fwrite(long long f0, long long n, int k0, const int* flag,
                                                            const int* excl, const int* fctl, int* fkept, int* fkpos) {
  const long long j = (long long)blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (j >= n || !flag[j]) return;
  const long long p = f0 + j;
  const size_t k = (size_t)k0 + (size_t)excl[j];
  fkept[3 * k] = fctl[3 * p];
  fkept[3 * k + 1] = fctl[3 * p + 1];
  fkept[3 * k + 2] = fctl[3 * p + 2];
  fkpos[k] = (int)p;
}

// --------------------------------------------------------------------- edges
// Side s of the 3 K sides: face s / 3, corners (s % 3, (s % 3 + 1) % 3).
__device__ __forceinline__ void side_of(const int* fkept, long long s, int* lo, int* hi) {
  const long long f = s / 3;
  const int j = (int)(s - 3 * f);
  const int a = fkept[3 * f + j], b = fkept[3 * f + (j == 2 ? 0 : j + 1)];
  *lo = a < b ? a : b;
  *hi = a < b ? b : a;
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_ecount(const int* fkept, long long sides, int* cnt) {
  const long long s = (long long)blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (s >= sides) return;
  int lo, hi;
  side_of(fkept, s, &lo, &hi);
  atomicAdd(cnt + lo, 1);
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_efill(const int* fkept, long long sides, const int* start,
                                                           int* cur, int* ehi) {
  const long long s = (long long)blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (s >= sides) return;
  int lo, hi;
  side_of(fkept, s, &lo, &hi);
  ehi[(size_t)start[lo] + (size_t)atomicAdd(cur + lo, 1)] = hi;
}

// Element e of a bucket goes to its rank: the elements below it, and its equals
// before it. The first of its value gets the flag. The fill order inside the
// bucket does not reach the result: equal values are interchangeable.
__device__ __forceinline__ void bucket_place(const int* in, int m, int e, int lo, int* sorted, int* slo, int* flag) {
  const int h = in[e];
  int rank = 0, before = 0;
  for (int j = 0; j < m; ++j) {
    const int o = in[j];
    rank += o < h ? 1 : 0;
    before += (o == h && j < e) ? 1 : 0;
  }
  sorted[rank + before] = h;
  slo[rank + before] = lo;
  flag[rank + before] = before == 0 ? 1 : 0;
}

// A lane owns a bucket of at most SIMP_HUB sides; a larger one joins the hub list.
__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_esort(long long n_control, const int* start, const int* cnt,
                                                           const int* ehi, int* sorted, int* slo, int* flag,
                                                           int* hubs, int* status) {
  const long long lo = (long long)blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (lo >= n_control) return;
  const int m = cnt[lo];
  if (m == 0) return;
  if (m > SIMP_HUB) {
    hubs[atomicAdd(status + ST_HUBS, 1)] = (int)lo;
    return;
  }
  const size_t b = (size_t)start[lo];
  for (int e = 0; e < m; ++e) bucket_place(ehi + b, m, e, (int)lo, sorted + b, slo + b, flag + b);
}

// A wave owns a hub: its lanes take the bucket's elements 64 at a time.
__global__ __launch_bounds__(64) void k_simp_esort_hub(const int* hubs, const int* start, const int* cnt,
                                                       const int* ehi, int* sorted, int* slo, int* flag,
                                                       const int* status) {
  const int nh = status[ST_HUBS];
  for (int w = blockIdx.x; w < nh; w += gridDim.x) {
    const int lo = hubs[w];
    const int m = cnt[lo];
    const size_t b = (size_t)start[lo];
    for (int e = threadIdx.x; e < m; e += 64) bucket_place(ehi + b, m, e, lo, sorted + b, slo + b, flag + b);
  }
}

__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_ewrite(long long sides, const int* flag, const int* excl,
                                                            const int* slo, const int* sorted, int* pairs) {
  const long long s = (long long)blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (s >= sides || !flag[s]) return;
  pairs[2 * (size_t)excl[s]] = slo[s];
  pairs[2 * (size_t)excl[s] + 1] = sorted[s];
}

// --------------------------------------------------------------------- graph
// bad[2 a], bad[2 a + 1]: robot a's control vertices without a keyframe, and the first of them.
__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_link(long long n_control, const int* crobot,
                                                          const long long* cstamp, const long long* kf_off,
                                                          const long long* kf_stamp, long long* link, int* bad) {
  const long long c = (long long)blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (c >= n_control) return;
  const int a = crobot[c];
  const long long s = cstamp[c];
  const long long r0 = kf_off[a], r1 = kf_off[a + 1];
  const long long pos = kmx::simp_lower((const int64_t*)kf_stamp, r0, r1, s);
  link[c] = pos;
  if (!(pos < r1 && kf_stamp[pos] == s)) {
    atomicAdd(bad + 2 * a, 1);
    atomicMin(bad + 2 * a + 1, (int)c);
  }
}

// Lane i < E writes mesh edge i's two directions, lane E + c control vertex c's two links.
__global__ __launch_bounds__(SIMP_BLOCK) void k_simp_emit(long long n_edges, long long n_control, int nk,
                                                          const int* pairs, const long long* link, double w_mesh,
                                                          double w_link, int* src, int* dst, double* w) {
  const long long i = (long long)blockIdx.x * SIMP_BLOCK + threadIdx.x;
  if (i >= n_edges + n_control) return;
  int a, b;
  double wt;
  if (i < n_edges) {
    a = pairs[2 * i] + nk;
    b = pairs[2 * i + 1] + nk;
    wt = w_mesh;
  } else {
    a = (int)(i - n_edges) + nk;
    b = (int)link[i - n_edges];
    wt = w_link;
  }
  src[2 * i] = a;
  dst[2 * i] = b;
  src[2 * i + 1] = b;
  dst[2 * i + 1] = a;
  w[2 * i] = wt;
  w[2 * i + 1] = wt;
}

unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

struct kmx_simplify : kmx::StreamCore {
  kmx_simplify_params P{};
  int64_t n_vertices = 0, n_faces_in = 0, n_control = 0, n_kept = 0, n_edges = 0;
  int64_t vcap = 0, fcap = 0, tcap = 0, rawcap = 0;
  uint64_t vslots = 0, fslots = 0;
  int vrehash = 0, frehash = 0;
  bool edges_valid = false;
  // vertices and control vertices (the control arrays have the vertices' capacity)
  kmx::DevBuf<float> d_vxyz;
  kmx::DevBuf<int> d_vrobot, d_vmap, d_crep, d_crobot;
  kmx::DevBuf<long long> d_vstamp, d_cstamp;
  kmx::DevBuf<double> d_cxyz;
  // input faces' mapped corners, kept faces and their input positions
  kmx::DevBuf<int> d_fctl, d_fkept, d_fkpos;
  kmx::DevBuf<uint32_t> d_vtab, d_ftab;
  // one append's or one request's work space: [tcap] each, partials by the scan's span
  kmx::DevBuf<int> d_rep, d_flag, d_excl, d_part, d_raw;
  // edges: per control vertex count, start and cursor, hubs; per side hi, sorted hi, lo; the pairs
  kmx::DevBuf<int> d_ecnt, d_estart, d_ecur, d_hubs, d_ehi, d_esorted, d_elo, d_pairs;
  // graph
  kmx::DevBuf<long long> d_kfoff, d_kfstamp, d_link;
  kmx::DevBuf<int> d_src, d_dst, d_bad;
  kmx::DevBuf<double> d_w;
  kmx::DevBuf<int> d_status;
  bool timing = false, timed[3] = {false, false, false};
  kmx::Event ev[6];  // add, edges, graph: begin and end

  VKeys vkeys() const {
    return VKeys{d_vxyz.get(), d_vrobot.get(), d_vstamp.get(), P.resolution, (long long)P.horizon_ns};
  }
  FKeys fkeys() const { return FKeys{d_fctl.get()}; }
  int64_t device_bytes() const {
    return (int64_t)(d_vxyz.cap() * 4 + (d_vrobot.cap() + d_vmap.cap() + d_crep.cap() + d_crobot.cap()) * 4 +
                     (d_vstamp.cap() + d_cstamp.cap()) * 8 + d_cxyz.cap() * 8 +
                     (d_fctl.cap() + d_fkept.cap() + d_fkpos.cap()) * 4 + (d_vtab.cap() + d_ftab.cap()) * 4 +
                     (d_rep.cap() + d_flag.cap() + d_excl.cap() + d_part.cap() + d_raw.cap()) * 4 +
                     (d_ecnt.cap() + d_estart.cap() + d_ecur.cap() + d_hubs.cap() + d_ehi.cap() + d_esorted.cap() +
                      d_elo.cap() + d_pairs.cap()) * 4 +
                     (d_kfoff.cap() + d_kfstamp.cap() + d_link.cap()) * 8 + (d_src.cap() + d_dst.cap() + d_bad.cap()) * 4 +
                     d_w.cap() * 8 + d_status.cap() * 4);
  }
};

namespace {

int64_t simp_next_cap(int64_t cap, int64_t need) {
  int64_t c = std::max<int64_t>(cap, 1024);
  while (c < need) c *= 2;
  return c;
}

// A buffer grown before a later one fails keeps its contents, so the handle stays as it was.
int simp_reserve_vertices(kmx_simplify* h, int64_t need) {
  if (need <= h->vcap) return 0;
  KMX_HIP(hipStreamSynchronize(h->stream));
  const size_t c = (size_t)simp_next_cap(h->vcap, need), u = (size_t)h->n_vertices, uc = (size_t)h->n_control;
  int rc;
  if ((rc = h->d_vxyz.grow_keep(u * 3, c * 3)) || (rc = h->d_vrobot.grow_keep(u, c)) ||
      (rc = h->d_vstamp.grow_keep(u, c)) || (rc = h->d_vmap.grow_keep(u, c)) || (rc = h->d_crep.grow_keep(uc, c)) ||
      (rc = h->d_cxyz.grow_keep(uc * 3, c * 3)) || (rc = h->d_cstamp.grow_keep(uc, c)) ||
      (rc = h->d_crobot.grow_keep(uc, c)))
    return rc;
  h->vcap = (int64_t)c;
  return 0;
}

int simp_reserve_faces(kmx_simplify* h, int64_t need) {
  if (need <= h->fcap) return 0;
  KMX_HIP(hipStreamSynchronize(h->stream));
  const size_t c = (size_t)simp_next_cap(h->fcap, need), u = (size_t)h->n_faces_in, uk = (size_t)h->n_kept;
  int rc;
  if ((rc = h->d_fctl.grow_keep(u * 3, c * 3)) || (rc = h->d_fkept.grow_keep(uk * 3, c * 3)) ||
      (rc = h->d_fkpos.grow_keep(uk, c)))
    return rc;
  h->fcap = (int64_t)c;
  return 0;
}

// The work space for n elements (contents are not kept).
int simp_reserve_tmp(kmx_simplify* h, int64_t need) {
  if (need <= h->tcap) return 0;
  KMX_HIP(hipStreamSynchronize(h->stream));
  const size_t c = (size_t)simp_next_cap(h->tcap, need);
  int rc;
  if ((rc = h->d_rep.alloc(c)) || (rc = h->d_flag.alloc(c)) || (rc = h->d_excl.alloc(c)) ||
      (rc = h->d_part.alloc((c + SIMP_SCAN_SPAN - 1) / SIMP_SCAN_SPAN)))
    return rc;
  h->tcap = (int64_t)c;
  return 0;
}

template <class T>
int simp_fit(kmx_simplify* h, kmx::DevBuf<T>& b, size_t need) {
  if (need <= b.cap()) return 0;
  KMX_HIP(hipStreamSynchronize(h->stream));
  return b.alloc((size_t)simp_next_cap((int64_t)b.cap(), (int64_t)need));
}

// excl[0 .. n) from flag[0 .. n), and the sum into *total (device).
int simp_scan(kmx_simplify* h, const int* flag, int64_t n, int* excl, int* total) {
  const int64_t nb = (n + SIMP_SCAN_SPAN - 1) / SIMP_SCAN_SPAN;
  if (nb)
    hipLaunchKernelGGL(k_simp_scan_part, dim3((unsigned)nb), dim3(SIMP_SCAN_BLOCK), 0, h->stream, flag, (long long)n,
                       h->d_part.get());
  hipLaunchKernelGGL(k_simp_scan_top, dim3(1), dim3(SIMP_SCAN_BLOCK), 0, h->stream, h->d_part.get(), (long long)nb,
                     total);
  if (nb)
    hipLaunchKernelGGL(k_simp_scan_apply, dim3((unsigned)nb), dim3(SIMP_SCAN_BLOCK), 0, h->stream, flag, (long long)n,
                       (const int*)h->d_part.get(), excl);
  KMX_HIP(hipGetLastError());
  return 0;
}

// A table of at least twice `items` slots: a larger one is cleared and the
// present keys (the control representatives, the kept faces) go in again.
int simp_grow_vtab(kmx_simplify* h, int64_t items) {
  const uint64_t want = kmx::simp_slots_for(h->vslots, h->P.initial_slots, items);
  if (want == h->vslots) return 0;
  KMX_HIP(hipStreamSynchronize(h->stream));
  kmx::DevBuf<uint32_t> t;
  if (int rc = t.alloc((size_t)want)) return rc;
  KMX_HIP(hipMemsetAsync(t.get(), 0xff, sizeof(uint32_t) * want, h->stream));
  if (h->n_control) {
    hipLaunchKernelGGL(k_simp_vinsert, dim3(blocks_of(h->n_control, SIMP_BLOCK)), dim3(SIMP_BLOCK), 0, h->stream,
                       t.get(), (u64)want, h->vkeys(), (const int*)h->d_crep.get(), 0LL, (long long)h->n_control,
                       h->d_status.get());
    KMX_HIP(hipGetLastError());
  }
  KMX_HIP(hipStreamSynchronize(h->stream));
  if (h->vslots) h->vrehash++;
  h->d_vtab = std::move(t);
  h->vslots = want;
  return 0;
}

int simp_grow_ftab(kmx_simplify* h, int64_t items) {
  const uint64_t want = kmx::simp_slots_for(h->fslots, h->P.initial_slots, items);
  if (want == h->fslots) return 0;
  KMX_HIP(hipStreamSynchronize(h->stream));
  kmx::DevBuf<uint32_t> t;
  if (int rc = t.alloc((size_t)want)) return rc;
  KMX_HIP(hipMemsetAsync(t.get(), 0xff, sizeof(uint32_t) * want, h->stream));
  if (h->n_kept) {
    hipLaunchKernelGGL(k_simp_finsert_kept, dim3(blocks_of(h->n_kept, SIMP_BLOCK)), dim3(SIMP_BLOCK), 0, h->stream,
                       t.get(), (u64)want, h->fkeys(), (const int*)h->d_fkpos.get(), (long long)h->n_kept,
                       h->d_status.get());
    KMX_HIP(hipGetLastError());
  }
  KMX_HIP(hipStreamSynchronize(h->stream));
  if (h->fslots) h->frehash++;
  h->d_ftab = std::move(t);
  h->fslots = want;
  return 0;
}

int simp_read_status(kmx_simplify* h, int* st) {
  KMX_HIP(hipMemcpyAsync(st, h->d_status.get(), sizeof(int) * ST_WORDS, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  if (st[ST_ERR])
    return kmx::fail(KMX_EHIP, std::string("a hash table's probe ran out of slots (") +
                                   (st[ST_ERR] & ERR_VTABLE ? "vertex" : "face") + " table): the handle is unusable");
  return 0;
}

int simp_form_edges(kmx_simplify* h) {
  if (h->edges_valid) return 0;
  const int64_t C = h->n_control, sides = 3 * h->n_kept;
  h->n_edges = 0;
  if (sides == 0) {
    h->edges_valid = true;
    return 0;
  }
  KMX_CHECK(sides < INT32_MAX, KMX_EUNSUP, "2^31 - 1 face sides or more");
  int rc;
  if ((rc = simp_reserve_tmp(h, std::max(C, sides))) || (rc = simp_fit(h, h->d_ecnt, (size_t)C)) ||
      (rc = simp_fit(h, h->d_estart, (size_t)C)) || (rc = simp_fit(h, h->d_ecur, (size_t)C)) ||
      (rc = simp_fit(h, h->d_hubs, (size_t)C)) || (rc = simp_fit(h, h->d_ehi, (size_t)sides)) ||
      (rc = simp_fit(h, h->d_esorted, (size_t)sides)) || (rc = simp_fit(h, h->d_elo, (size_t)sides)) ||
      (rc = simp_fit(h, h->d_pairs, (size_t)sides * 2)))
    return rc;
  int* st = h->d_status.get();
  if (h->timing) KMX_HIP(hipEventRecord(h->ev[2], h->stream));
  KMX_HIP(hipMemsetAsync(h->d_ecnt.get(), 0, sizeof(int) * C, h->stream));
  KMX_HIP(hipMemsetAsync(h->d_ecur.get(), 0, sizeof(int) * C, h->stream));
  KMX_HIP(hipMemsetAsync(st + ST_HUBS, 0, sizeof(int), h->stream));
  const dim3 gs(blocks_of(sides, SIMP_BLOCK)), gc(blocks_of(C, SIMP_BLOCK)), b(SIMP_BLOCK);
  hipLaunchKernelGGL(k_simp_ecount, gs, b, 0, h->stream, (const int*)h->d_fkept.get(), (long long)sides,
                     h->d_ecnt.get());
  KMX_HIP(hipGetLastError());
  if ((rc = simp_scan(h, h->d_ecnt.get(), C, h->d_estart.get(), st + ST_EDGES))) return rc;  // (the word is rewritten below)
  hipLaunchKernelGGL(k_simp_efill, gs, b, 0, h->stream, (const int*)h->d_fkept.get(), (long long)sides,
                     (const int*)h->d_estart.get(), h->d_ecur.get(), h->d_ehi.get());
  hipLaunchKernelGGL(k_simp_esort, gc, b, 0, h->stream, (long long)C, (const int*)h->d_estart.get(),
                     (const int*)h->d_ecnt.get(), (const int*)h->d_ehi.get(), h->d_esorted.get(), h->d_elo.get(),
                     h->d_flag.get(), h->d_hubs.get(), st);
  hipLaunchKernelGGL(k_simp_esort_hub, dim3(SIMP_HUB_WAVES), dim3(64), 0, h->stream, (const int*)h->d_hubs.get(),
                     (const int*)h->d_estart.get(), (const int*)h->d_ecnt.get(), (const int*)h->d_ehi.get(),
                     h->d_esorted.get(), h->d_elo.get(), h->d_flag.get(), (const int*)st);
  KMX_HIP(hipGetLastError());
  if ((rc = simp_scan(h, h->d_flag.get(), sides, h->d_excl.get(), st + ST_EDGES))) return rc;
  hipLaunchKernelGGL(k_simp_ewrite, gs, b, 0, h->stream, (long long)sides, (const int*)h->d_flag.get(),
                     (const int*)h->d_excl.get(), (const int*)h->d_elo.get(), (const int*)h->d_esorted.get(),
                     h->d_pairs.get());
  KMX_HIP(hipGetLastError());
  if (h->timing) {
    KMX_HIP(hipEventRecord(h->ev[3], h->stream));
    h->timed[1] = true;
  }
  int host[ST_WORDS];
  if ((rc = simp_read_status(h, host))) return rc;
  h->n_edges = host[ST_EDGES];
  h->edges_valid = true;
  return 0;
}

}  // namespace

extern "C" int kmx_simplify_create(const kmx_simplify_params* params, int device, kmx_simplify** out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(out, KMX_EINVAL, "null argument");
  std::string err;
  if (int rc = kmx::simp_check_params(params, &err)) return kmx::fail(rc, err);
  std::unique_ptr<kmx_simplify> h(new kmx_simplify());  // a failure below unwinds through the members' destructors
  int rc;
  if ((rc = h->open(device)) || (rc = kmx::create_events(h->ev))) return rc;
  h->P = *params;
  if ((rc = h->d_status.alloc(ST_WORDS))) return rc;
  KMX_HIP(hipMemsetAsync(h->d_status.get(), 0, sizeof(int) * ST_WORDS, h->stream));
  if ((rc = simp_reserve_vertices(h.get(), 1)) || (rc = simp_reserve_faces(h.get(), 1)) ||
      (rc = simp_reserve_tmp(h.get(), 1)) || (rc = simp_grow_vtab(h.get(), 0)) || (rc = simp_grow_ftab(h.get(), 0)))
    return rc;
  KMX_HIP(hipStreamSynchronize(h->stream));
  *out = h.release();
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_simplify_destroy(kmx_simplify* h) {
  return kmx::destroy(h);
}

extern "C" int kmx_simplify_set_stream(kmx_simplify* h, void* s) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  return h->adopt(s, true);
}

extern "C" int kmx_simplify_sync(kmx_simplify* h) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
}

extern "C" int kmx_simplify_info(kmx_simplify* h, kmx_simplify_info_t* info) {
  KMX_CHECK(h && info, KMX_EINVAL, "null argument");
  info->n_vertices = h->n_vertices;
  info->n_faces_in = h->n_faces_in;
  info->n_control = h->n_control;
  info->n_faces_kept = h->n_kept;
  info->vertex_slots = (int64_t)h->vslots;
  info->face_slots = (int64_t)h->fslots;
  info->device_bytes = h->device_bytes();
  info->vertex_rehashes = h->vrehash;
  info->face_rehashes = h->frehash;
  info->scan_span = SIMP_SCAN_SPAN;
  info->scan_span2 = (int32_t)kmx::SIMP_SCAN_SPAN2;
  return KMX_OK;
}

extern "C" int kmx_simplify_add(kmx_simplify* h, int64_t n, const int32_t* robot, const int64_t* stamp_ns,
                                const float* xyz, int64_t nf, const int32_t* faces, int64_t* first_vertex_out,
                                int64_t* counts_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  std::string err;
  if (int rc = kmx::simp_check_add(h->P, h->n_vertices, h->n_faces_in, n, robot, stamp_ns, xyz, nf, faces, &err))
    return kmx::fail(rc, err);
  if (first_vertex_out) *first_vertex_out = h->n_vertices;
  if (counts_out) counts_out[0] = counts_out[1] = 0;
  if (n == 0 && nf == 0) return KMX_OK;
  KMX_HIP(hipSetDevice(h->device));
  const int64_t v0 = h->n_vertices, f0 = h->n_faces_in, c0 = h->n_control, k0 = h->n_kept;
  int rc;
  if ((rc = simp_reserve_vertices(h, v0 + n)) || (rc = simp_reserve_faces(h, f0 + nf)) ||
      (rc = simp_reserve_tmp(h, std::max(n, nf))) || (rc = simp_fit(h, h->d_raw, (size_t)nf * 3)) ||
      (rc = simp_grow_vtab(h, c0 + n)) || (rc = simp_grow_ftab(h, k0 + nf)))
    return rc;
  int* st = h->d_status.get();
  const dim3 b(SIMP_BLOCK);
  if (n) {
    KMX_HIP(hipMemcpyAsync(h->d_vxyz.get() + 3 * v0, xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice, h->stream));
    KMX_HIP(hipMemcpyAsync(h->d_vrobot.get() + v0, robot, sizeof(int) * n, hipMemcpyHostToDevice, h->stream));
    KMX_HIP(hipMemcpyAsync(h->d_vstamp.get() + v0, stamp_ns, sizeof(long long) * n, hipMemcpyHostToDevice, h->stream));
  }
  if (nf) KMX_HIP(hipMemcpyAsync(h->d_raw.get(), faces, sizeof(int) * 3 * nf, hipMemcpyHostToDevice, h->stream));
  KMX_HIP(hipMemsetAsync(st + ST_NEW_CONTROL, 0, 2 * sizeof(int), h->stream));
  if (h->timing) KMX_HIP(hipEventRecord(h->ev[0], h->stream));
  if (n) {
    const dim3 g(blocks_of(n, SIMP_BLOCK));
    hipLaunchKernelGGL(k_simp_vinsert, g, b, 0, h->stream, h->d_vtab.get(), (u64)h->vslots, h->vkeys(),
                       (const int*)nullptr, (long long)v0, (long long)n, st);
    hipLaunchKernelGGL(k_simp_vfind, g, b, 0, h->stream, h->d_vtab.get(), (u64)h->vslots, h->vkeys(), (long long)v0,
                       (long long)n, h->d_rep.get(), h->d_flag.get(), st);
    KMX_HIP(hipGetLastError());
    if ((rc = simp_scan(h, h->d_flag.get(), n, h->d_excl.get(), st + ST_NEW_CONTROL))) return rc;
    hipLaunchKernelGGL(k_simp_vwrite, g, b, 0, h->stream, (long long)v0, (long long)n, (int)c0,
                       (const int*)h->d_rep.get(), (const int*)h->d_flag.get(), (const int*)h->d_excl.get(),
                       (const float*)h->d_vxyz.get(), (const int*)h->d_vrobot.get(),
                       (const long long*)h->d_vstamp.get(), h->d_vmap.get(), h->d_crep.get(), h->d_cxyz.get(),
                       h->d_cstamp.get(), h->d_crobot.get());
    KMX_HIP(hipGetLastError());
  }
  if (nf) {
    const dim3 g(blocks_of(nf, SIMP_BLOCK));
    hipLaunchKernelGGL(k_simp_fmap, g, b, 0, h->stream, (const int*)h->d_raw.get(), (const int*)h->d_vmap.get(),
                       (long long)f0, (long long)nf, h->d_fctl.get());
    hipLaunchKernelGGL(k_simp_finsert, g, b, 0, h->stream, h->d_ftab.get(), (u64)h->fslots, h->fkeys(), (long long)f0,
                       (long long)nf, st);
    hipLaunchKernelGGL(k_simp_ffind, g, b, 0, h->stream, h->d_ftab.get(), (u64)h->fslots, h->fkeys(), (long long)f0,
                       (long long)nf, h->d_flag.get(), st);
    KMX_HIP(hipGetLastError());
    if ((rc = simp_scan(h, h->d_flag.get(), nf, h->d_excl.get(), st + ST_NEW_KEPT))) return rc;
    hipLaunchKernelGGL(k_simp_fwrite, g, b, 0, h->stream, (long long)f0, (long long)nf, (int)k0,
                       (const int*)h->d_flag.get(), (const int*)h->d_excl.get(), (const int*)h->d_fctl.get(),
                       h->d_fkept.get(), h->d_fkpos.get());
    KMX_HIP(hipGetLastError());
  }
  if (h->timing) {
    KMX_HIP(hipEventRecord(h->ev[1], h->stream));
    h->timed[0] = true;
  }
  int host[ST_WORDS];
  if ((rc = simp_read_status(h, host))) return rc;  // waits: the caller's arrays are free again
  h->n_vertices = v0 + n;
  h->n_faces_in = f0 + nf;
  h->n_control = c0 + host[ST_NEW_CONTROL];
  h->n_kept = k0 + host[ST_NEW_KEPT];
  h->edges_valid = false;
  if (counts_out) {
    counts_out[0] = host[ST_NEW_CONTROL];
    counts_out[1] = host[ST_NEW_KEPT];
  }
  return KMX_OK;
  KMX_GUARD_END
}

namespace {
bool simp_range_ok(int64_t first, int64_t n, int64_t total) {
  return first >= 0 && n >= 0 && first <= total && n <= total - first;
}
}  // namespace

extern "C" int kmx_simplify_get_control(kmx_simplify* h, int64_t first, int64_t n, double* xyz, int64_t* stamp_ns,
                                        int32_t* robot, int32_t* representative) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(simp_range_ok(first, n, h->n_control), KMX_EINVAL, "range outside the control vertices");
  if (n == 0) return KMX_OK;
  KMX_HIP(hipSetDevice(h->device));
  const hipMemcpyKind D2H = hipMemcpyDeviceToHost;
  if (xyz) KMX_HIP(hipMemcpyAsync(xyz, h->d_cxyz.get() + 3 * first, sizeof(double) * 3 * n, D2H, h->stream));
  if (stamp_ns) KMX_HIP(hipMemcpyAsync(stamp_ns, h->d_cstamp.get() + first, sizeof(int64_t) * n, D2H, h->stream));
  if (robot) KMX_HIP(hipMemcpyAsync(robot, h->d_crobot.get() + first, sizeof(int) * n, D2H, h->stream));
  if (representative) KMX_HIP(hipMemcpyAsync(representative, h->d_crep.get() + first, sizeof(int) * n, D2H, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_simplify_get_vertex_map(kmx_simplify* h, int64_t first, int64_t n, int32_t* out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(simp_range_ok(first, n, h->n_vertices), KMX_EINVAL, "range outside the vertices");
  if (n == 0) return KMX_OK;
  KMX_CHECK(out, KMX_EINVAL, "null output");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipMemcpyAsync(out, h->d_vmap.get() + first, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_simplify_get_faces(kmx_simplify* h, int64_t first, int64_t n, int32_t* out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(simp_range_ok(first, n, h->n_kept), KMX_EINVAL, "range outside the kept faces");
  if (n == 0) return KMX_OK;
  KMX_CHECK(out, KMX_EINVAL, "null output");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipMemcpyAsync(out, h->d_fkept.get() + 3 * first, sizeof(int) * 3 * n, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_simplify_edges(kmx_simplify* h, int64_t* n_edges_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_HIP(hipSetDevice(h->device));
  if (int rc = simp_form_edges(h)) return rc;
  if (n_edges_out) *n_edges_out = h->n_edges;
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_simplify_get_edges(kmx_simplify* h, int32_t* pairs) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(h->edges_valid, KMX_ESTATE, "the edges are not formed: kmx_simplify_edges");
  if (h->n_edges == 0) return KMX_OK;
  KMX_CHECK(pairs, KMX_EINVAL, "null output");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipMemcpyAsync(pairs, h->d_pairs.get(), sizeof(int) * 2 * h->n_edges, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_simplify_graph(kmx_simplify* h, int32_t n_robots, const int64_t* kf_offset, const int64_t* kf_stamp,
                                  double w_mesh, double w_link, int32_t* src, int32_t* dst, double* w, int64_t* link,
                                  int64_t* n_directed_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  std::string err;
  if (int rc = kmx::simp_check_graph(h->P, h->n_control, n_robots, kf_offset, kf_stamp, w_mesh, w_link, &err))
    return kmx::fail(rc, err);
  KMX_HIP(hipSetDevice(h->device));
  int rc;
  if ((rc = simp_form_edges(h))) return rc;
  const int64_t C = h->n_control, E = h->n_edges, nk = kf_offset[n_robots], nd = 2 * E + 2 * C;
  KMX_CHECK(nd < INT32_MAX, KMX_EUNSUP, "2^31 - 1 directed edges or more");
  if (n_directed_out) *n_directed_out = nd;
  if (!src && !dst && !w && !link) return KMX_OK;
  if (C == 0) return KMX_OK;  // no control vertex: no face, no edge
  const size_t nr = (size_t)n_robots;
  if ((rc = simp_fit(h, h->d_kfoff, nr + 1)) || (rc = simp_fit(h, h->d_kfstamp, (size_t)nk)) ||
      (rc = simp_fit(h, h->d_link, (size_t)C)) || (rc = simp_fit(h, h->d_bad, 2 * nr)) ||
      (rc = simp_fit(h, h->d_src, (size_t)nd)) || (rc = simp_fit(h, h->d_dst, (size_t)nd)) ||
      (rc = simp_fit(h, h->d_w, (size_t)nd)))
    return rc;
  std::vector<int> bad(2 * nr);
  for (size_t a = 0; a < nr; ++a) {
    bad[2 * a] = 0;
    bad[2 * a + 1] = INT_MAX;
  }
  const hipMemcpyKind H2D = hipMemcpyHostToDevice, D2H = hipMemcpyDeviceToHost;
  KMX_HIP(hipMemcpyAsync(h->d_kfoff.get(), kf_offset, sizeof(int64_t) * (nr + 1), H2D, h->stream));
  if (nk) KMX_HIP(hipMemcpyAsync(h->d_kfstamp.get(), kf_stamp, sizeof(int64_t) * nk, H2D, h->stream));
  KMX_HIP(hipMemcpyAsync(h->d_bad.get(), bad.data(), sizeof(int) * 2 * nr, H2D, h->stream));
  if (h->timing) KMX_HIP(hipEventRecord(h->ev[4], h->stream));
  hipLaunchKernelGGL(k_simp_link, dim3(blocks_of(C, SIMP_BLOCK)), dim3(SIMP_BLOCK), 0, h->stream, (long long)C,
                     (const int*)h->d_crobot.get(), (const long long*)h->d_cstamp.get(),
                     (const long long*)h->d_kfoff.get(), (const long long*)h->d_kfstamp.get(), h->d_link.get(),
                     h->d_bad.get());
  hipLaunchKernelGGL(k_simp_emit, dim3(blocks_of(E + C, SIMP_BLOCK)), dim3(SIMP_BLOCK), 0, h->stream, (long long)E,
                     (long long)C, (int)nk, (const int*)h->d_pairs.get(), (const long long*)h->d_link.get(), w_mesh,
                     w_link, h->d_src.get(), h->d_dst.get(), h->d_w.get());
  KMX_HIP(hipGetLastError());
  if (h->timing) {
    KMX_HIP(hipEventRecord(h->ev[5], h->stream));
    h->timed[2] = true;
  }
  KMX_HIP(hipMemcpyAsync(bad.data(), h->d_bad.get(), sizeof(int) * 2 * nr, D2H, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  for (size_t a = 0; a < nr; ++a)
    if (bad[2 * a]) return kmx::fail(KMX_EINVAL, kmx::simp_missing_message((int32_t)a, bad[2 * a], bad[2 * a + 1]));
  if (src) KMX_HIP(hipMemcpyAsync(src, h->d_src.get(), sizeof(int) * nd, D2H, h->stream));
  if (dst) KMX_HIP(hipMemcpyAsync(dst, h->d_dst.get(), sizeof(int) * nd, D2H, h->stream));
  if (w) KMX_HIP(hipMemcpyAsync(w, h->d_w.get(), sizeof(double) * nd, D2H, h->stream));
  if (link) KMX_HIP(hipMemcpyAsync(link, h->d_link.get(), sizeof(int64_t) * C, D2H, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_simplify_enable_timing(kmx_simplify* h, int enable) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  h->timing = enable != 0;
  h->timed[0] = h->timed[1] = h->timed[2] = false;
  return KMX_OK;
}

extern "C" int kmx_simplify_read_timing(kmx_simplify* h, double* add_ms, double* edges_ms, double* graph_ms) {
  KMX_CHECK(h && add_ms && edges_ms && graph_ms, KMX_EINVAL, "null argument");
  KMX_CHECK(h->timing, KMX_ESTATE, "timing is off: kmx_simplify_enable_timing");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  float ms[3] = {0.f, 0.f, 0.f};
  for (int i = 0; i < 3; ++i)
    if (h->timed[i]) KMX_HIP(hipEventElapsedTime(&ms[i], h->ev[2 * i], h->ev[2 * i + 1]));
  *add_ms = ms[0];
  *edges_ms = ms[1];
  *graph_ms = ms[2];
  return KMX_OK;
}
