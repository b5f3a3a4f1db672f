// mesh.hip — mesh deformation on the device (kmx_mesh_*, include/kmx_abi.h):
// every mesh vertex is bound once to the k nearest control nodes of its robot
// inside a time window (k_mesh_bind), and moved by the distance-weighted blend
// of those nodes' rigid corrections whenever the trajectory changes
// (k_mesh_deform). All arithmetic is fp64 and this file is compiled with
// -ffp-contract=off: the squared distances, and with them the ranking, are bit
// for bit those of the host reference (tests/mesh_ref.py).
//
// Layout. Nodes by id: Rrest [9], g [3] and the 15-double row {R, g, p} that
// the deform kernel gathers (120 B). For the bind kernel the nodes are also
// kept robot by robot ("sorted": robot a owns positions [off[a], off[a+1]),
// stamps non-decreasing inside): stamps, ids and positions (24 B each). Inside
// one robot the position grows with the node id, so a tie on distance goes to
// the lower position. Vertices: xyz fp32, robot, stamp; bindings idx[k] int32,
// w[k] fp64, count.
#include <algorithm>
#include <climits>
#include <memory>
#include <vector>

#include "common.h"
#include "mesh_host.h"

namespace {

constexpr int MESH_BLOCK = 256;
constexpr int MESH_LDS_NODES = 1024;  // 24 KiB of node positions per workgroup: six workgroups per CU
constexpr int MESH_ROW = 15;          // R[9] g[3] p[3]

struct MeshBindArgs {
  long long first, n;
  long long window;
  const int* off;          // [n_robots + 1]
  const long long* s_stamp;  // sorted
  const int* s_id;
  const double* s_g;  // [.][3]
  const float* vxyz;
  const int* vrobot;
  const long long* vstamp;
  int* bidx;
  double* bw;
  int* bcnt;
  int* global_blocks;
};

// Offers positions [lo, hi) to the lane's best K + 1 (distance, position)
// pairs, kept sorted. A candidate enters only when it is strictly less than
// the last pair, so the result depends on the candidates alone, not on the
// order they are offered in. q(p) = base + 3 (p - shift).
template <int K>
__device__ __forceinline__ void mesh_scan(const double* base, int shift, int lo, int hi, double vx, double vy,
                                          double vz, double (&bd)[K + 1], int (&bp)[K + 1]) {
  for (int p = lo; p < hi; ++p) {
    const double* q = base + 3 * (size_t)(p - shift);
    const double dx = vx - q[0], dy = vy - q[1], dz = vz - q[2];
    const double d = dx * dx + dy * dy + dz * dz;
    if (d < bd[K] || (d == bd[K] && p < bp[K])) {
      bd[K] = d;
      bp[K] = p;
#pragma unroll
      for (int j = K; j >= 1; --j) {
        const bool less = bd[j] < bd[j - 1] || (bd[j] == bd[j - 1] && bp[j] < bp[j - 1]);
        const double td = less ? bd[j - 1] : bd[j];
        const int tp = less ? bp[j - 1] : bp[j];
        bd[j - 1] = less ? bd[j] : bd[j - 1];
        bp[j - 1] = less ? bp[j] : bp[j - 1];
        bd[j] = td;
        bp[j] = tp;
      }
    }
  }
}

// A lane owns a vertex. The workgroup stages the union of its lanes' windows
// (one range of sorted positions) in LDS when it fits, and reads the L2
// otherwise; the arithmetic is the same.
template <int K>
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_bind(MeshBindArgs a) {
  __shared__ double s_g[MESH_LDS_NODES * 3];
  __shared__ int s_lo, s_hi;
  const int tid = threadIdx.x;
  const long long i = a.first + (long long)blockIdx.x * MESH_BLOCK + tid;
  const bool live = i < a.first + a.n;
  if (tid == 0) {
    s_lo = INT_MAX;
    s_hi = 0;
  }
  __syncthreads();
  int lo = 0, hi = 0;
  double vx = 0.0, vy = 0.0, vz = 0.0;
  if (live) {
    const int r = a.vrobot[i];
    const long long s = a.vstamp[i];
    const int r0 = a.off[r], r1 = a.off[r + 1];
    lo = kmx::mesh_lower((const int64_t*)a.s_stamp, r0, r1, kmx::mesh_sat_sub(s, a.window));
    hi = kmx::mesh_upper((const int64_t*)a.s_stamp, r0, r1, kmx::mesh_sat_add(s, a.window));
    vx = (double)a.vxyz[3 * i];
    vy = (double)a.vxyz[3 * i + 1];
    vz = (double)a.vxyz[3 * i + 2];
    if (lo < hi) {
      atomicMin(&s_lo, lo);
      atomicMax(&s_hi, hi);
    }
  }
  __syncthreads();
  const int u0 = s_lo, u1 = s_hi;
  const int span = u1 > u0 ? u1 - u0 : 0;
  const bool staged = span <= MESH_LDS_NODES;
  if (staged)
    for (int e = tid; e < span * 3; e += MESH_BLOCK) s_g[e] = a.s_g[(size_t)u0 * 3 + e];
  __syncthreads();
  if (!staged && tid == 0) atomicAdd(a.global_blocks, 1);
  if (!live) return;
  double bd[K + 1];
  int bp[K + 1];
#pragma unroll
  for (int j = 0; j <= K; ++j) {
    bd[j] = __builtin_inf();
    bp[j] = INT_MAX;
  }
  if (staged)
    mesh_scan<K>(s_g, u0, lo, hi, vx, vy, vz, bd, bp);
  else
    mesh_scan<K>(a.s_g, 0, lo, hi, vx, vy, vz, bd, bp);
  const int m = hi - lo;
  const int kept = m < K + 1 ? m : K + 1;
  int count = m == 0 ? 0 : (m == 1 ? 1 : kept - 1);
  double w[K];
#pragma unroll
  for (int j = 0; j < K; ++j) w[j] = 0.0;
  if (m == 1) {
    w[0] = 1.0;
  } else if (m >= 2) {
    double dmax2 = 0.0;
#pragma unroll
    for (int j = 1; j <= K; ++j)
      if (j == kept - 1) dmax2 = bd[j];
    const double dmax = sqrt(dmax2);
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (j < count) {
        const double t = 1.0 - sqrt(bd[j]) / dmax;
        w[j] = t * t;
        sum += w[j];
      }
    if (sum > 0.0) {
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (j < count) w[j] = w[j] / sum;
    } else {  // d_max == 0 (a NaN sum), or every used node at d_max
      count = 1;
      w[0] = 1.0;
#pragma unroll
      for (int j = 1; j < K; ++j) w[j] = 0.0;
    }
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    a.bidx[i * K + j] = j < count ? a.s_id[bp[j]] : -1;
    a.bw[i * K + j] = j < count ? w[j] : 0.0;
  }
  a.bcnt[i] = count;
}

// rows[j] = {Rcur_j Rrest_j^T, g_j, p_j}
__global__ void k_mesh_node(long long n, const double* Rcur, const double* p, const double* Rrest, const double* g,
                            double* rows) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const double* A = Rcur + 9 * j;
  const double* B = Rrest + 9 * j;
  double* o = rows + MESH_ROW * j;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      o[3 * r + c] = A[3 * r] * B[3 * c] + A[3 * r + 1] * B[3 * c + 1] + A[3 * r + 2] * B[3 * c + 2];
  for (int c = 0; c < 3; ++c) {
    o[9 + c] = g[3 * j + c];
    o[12 + c] = p[3 * j + c];
  }
}

struct MeshPartial {
  double sum, max;
  int unbound, partial;
};

// A lane owns a vertex: 12 B of position, its binding, K node rows gathered
// from the L2, 12 B out. The displacement statistics leave the workgroup as
// one partial, reduced in a fixed tree.
template <int K>
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_deform(long long first, long long n, const float* vxyz,
                                                            const int* bidx, const double* bw, const int* bcnt,
                                                            const double* rows, float* out, MeshPartial* part) {
  __shared__ double s_sum[MESH_BLOCK], s_max[MESH_BLOCK];
  __shared__ int s_unb[MESH_BLOCK], s_par[MESH_BLOCK];
  const int tid = threadIdx.x;
  const long long rel = (long long)blockIdx.x * MESH_BLOCK + tid;
  double d2 = 0.0;
  int unb = 0, par = 0;
  if (rel < n) {
    const long long i = first + rel;
    const float fx = vxyz[3 * i], fy = vxyz[3 * i + 1], fz = vxyz[3 * i + 2];
    const int cnt = bcnt[i];
    float ox = fx, oy = fy, oz = fz;
    if (cnt == 0) {
      unb = 1;
    } else {
      const double vx = (double)fx, vy = (double)fy, vz = (double)fz;
      double ax = 0.0, ay = 0.0, az = 0.0;
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (j < cnt) {
          const double* r = rows + (size_t)bidx[i * K + j] * MESH_ROW;
          const double wj = bw[i * K + j];
          const double dx = vx - r[9], dy = vy - r[10], dz = vz - r[11];
          ax += wj * (r[0] * dx + r[1] * dy + r[2] * dz + r[12]);
          ay += wj * (r[3] * dx + r[4] * dy + r[5] * dz + r[13]);
          az += wj * (r[6] * dx + r[7] * dy + r[8] * dz + r[14]);
        }
      ox = (float)ax;
      oy = (float)ay;
      oz = (float)az;
      const double ex = (double)ox - vx, ey = (double)oy - vy, ez = (double)oz - vz;
      d2 = ex * ex + ey * ey + ez * ez;
      par = cnt < K ? 1 : 0;
    }
    out[3 * rel] = ox;
    out[3 * rel + 1] = oy;
    out[3 * rel + 2] = oz;
  }
  s_sum[tid] = d2;
  s_max[tid] = d2;
  s_unb[tid] = unb;
  s_par[tid] = par;
  __syncthreads();
  for (int s = MESH_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) {
      s_sum[tid] += s_sum[tid + s];
      s_max[tid] = s_max[tid] > s_max[tid + s] ? s_max[tid] : s_max[tid + s];
      s_unb[tid] += s_unb[tid + s];
      s_par[tid] += s_par[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) part[blockIdx.x] = MeshPartial{s_sum[0], s_max[0], s_unb[0], s_par[0]};
}

struct MeshStatsDev {
  double sum, max;
  long long unbound, partial;
};

// One wave: lane l takes partials l, l + 64, ... in order, then a fixed tree.
__global__ __launch_bounds__(64) void k_mesh_stats(const MeshPartial* part, int nb, MeshStatsDev* out) {
  const int l = threadIdx.x;
  double sum = 0.0, mx = 0.0;
  long long unb = 0, par = 0;
  for (int b = l; b < nb; b += 64) {
    sum += part[b].sum;
    mx = mx > part[b].max ? mx : part[b].max;
    unb += part[b].unbound;
    par += part[b].partial;
  }
  for (int s = 32; s > 0; s >>= 1) {
    sum += __shfl_xor(sum, s, 64);
    const double om = __shfl_xor(mx, s, 64);
    mx = mx > om ? mx : om;
    unb += __shfl_xor(unb, s, 64);
    par += __shfl_xor(par, s, 64);
  }
  if (l == 0) *out = MeshStatsDev{sum, mx, unb, par};
}

}  // namespace

struct kmx_mesh : kmx::StreamCore {
  kmx_mesh_params P{};
  kmx::MeshNodeIndex index;
  int64_t n_vertices = 0, ncap = 0, vcap = 0;  // the capacities are of eight buffers each, set once all have grown
  bool nodes_dirty = false;
  // nodes by id, the staging of current poses, and the sorted layout
  kmx::DevBuf<double> d_rrest, d_g, d_rows, d_rcur, d_p;
  kmx::DevBuf<long long> d_s_stamp;
  kmx::DevBuf<int> d_s_id, d_off;
  kmx::DevBuf<double> d_s_g;
  std::vector<int32_t> h_off, h_s_id;
  std::vector<int64_t> h_s_stamp;
  std::vector<double> h_s_g;
  // vertices and bindings
  kmx::DevBuf<float> d_vxyz, d_out;
  kmx::DevBuf<int> d_vrobot, d_bidx, d_bcnt;
  kmx::DevBuf<long long> d_vstamp;
  kmx::DevBuf<double> d_bw;
  kmx::DevBuf<MeshPartial> d_part;
  kmx::DevBuf<MeshStatsDev> d_stats;
  kmx::DevBuf<int> d_gblocks;
  int last_bind_blocks = 0;
  bool timing = false, bind_timed = false, deform_timed = false;
  kmx::Event ev[4];  // bind begin/end, deform begin/end
};

namespace {

int64_t mesh_next_cap(int64_t cap, int64_t need) {
  int64_t c = std::max<int64_t>(cap, 1024);
  while (c < need) c *= 2;
  return c;
}

// Room for `need` nodes. A buffer grown before a later one fails keeps its
// contents, so the handle stays as it was.
int mesh_reserve_nodes(kmx_mesh* h, int64_t need) {
  if (need <= h->ncap) return 0;
  KMX_HIP(hipStreamSynchronize(h->stream));
  const size_t c = (size_t)mesh_next_cap(h->ncap, need), u = (size_t)h->index.n_nodes;
  int rc;
  if ((rc = h->d_rrest.grow_keep(u * 9, c * 9)) || (rc = h->d_g.grow_keep(u * 3, c * 3)) ||
      (rc = h->d_rows.grow_keep(u * MESH_ROW, c * MESH_ROW)) || (rc = h->d_rcur.alloc(c * 9)) ||
      (rc = h->d_p.alloc(c * 3)) || (rc = h->d_s_stamp.alloc(c)) || (rc = h->d_s_id.alloc(c)) ||
      (rc = h->d_s_g.alloc(c * 3)))
    return rc;
  h->ncap = (int64_t)c;
  h->nodes_dirty = true;  // the sorted arrays are new
  return 0;
}

int mesh_reserve_vertices(kmx_mesh* h, int64_t need) {
  if (need <= h->vcap) return 0;
  KMX_HIP(hipStreamSynchronize(h->stream));
  const size_t c = (size_t)mesh_next_cap(h->vcap, need), u = (size_t)h->n_vertices, k = (size_t)h->P.k;
  int rc;
  if ((rc = h->d_vxyz.grow_keep(u * 3, c * 3)) || (rc = h->d_vrobot.grow_keep(u, c)) ||
      (rc = h->d_vstamp.grow_keep(u, c)) || (rc = h->d_bidx.grow_keep(u * k, c * k)) ||
      (rc = h->d_bw.grow_keep(u * k, c * k)) || (rc = h->d_bcnt.grow_keep(u, c)) || (rc = h->d_out.alloc(c * 3)) ||
      (rc = h->d_part.alloc((c + MESH_BLOCK - 1) / MESH_BLOCK)))
    return rc;
  h->vcap = (int64_t)c;
  return 0;
}

int mesh_form_rows(kmx_mesh* h, int64_t first, int64_t n, const double* d_Rcur, const double* d_p) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_mesh_node, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (long long)n, d_Rcur, d_p,
                     h->d_rrest.get() + 9 * first, h->d_g.get() + 3 * first, h->d_rows.get() + MESH_ROW * first);
  KMX_HIP(hipGetLastError());
  return 0;
}

template <int K>
void mesh_launch_bind(kmx_mesh* h, const MeshBindArgs& a, int blocks) {
  hipLaunchKernelGGL(k_mesh_bind<K>, dim3(blocks), dim3(MESH_BLOCK), 0, h->stream, a);
}

template <int K>
void mesh_launch_deform(kmx_mesh* h, long long first, long long n, float* out, int blocks) {
  hipLaunchKernelGGL(k_mesh_deform<K>, dim3(blocks), dim3(MESH_BLOCK), 0, h->stream, first, n, h->d_vxyz.get(),
                     h->d_bidx.get(), h->d_bw.get(), h->d_bcnt.get(), h->d_rows.get(), out, h->d_part.get());
}

#define MESH_K_SWITCH(k, call)  \
  switch (k) {                  \
    case 1: call(1); break;     \
    case 2: call(2); break;     \
    case 3: call(3); break;     \
    case 4: call(4); break;     \
    case 5: call(5); break;     \
    case 6: call(6); break;     \
    case 7: call(7); break;     \
    default: call(8); break;    \
  }

// Both deform kernels for a checked, non-empty range; `out` holds n rows.
int mesh_enqueue_deform(kmx_mesh* h, int64_t first, int64_t n, float* out) {
  const int blocks = (int)((n + MESH_BLOCK - 1) / MESH_BLOCK);
  if (h->timing) KMX_HIP(hipEventRecord(h->ev[2], h->stream));
#define MESH_CALL(K) mesh_launch_deform<K>(h, (long long)first, (long long)n, out, blocks)
  MESH_K_SWITCH(h->P.k, MESH_CALL)
#undef MESH_CALL
  KMX_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_mesh_stats, dim3(1), dim3(64), 0, h->stream, (const MeshPartial*)h->d_part.get(), blocks,
                     h->d_stats.get());
  KMX_HIP(hipGetLastError());
  if (h->timing) {
    KMX_HIP(hipEventRecord(h->ev[3], h->stream));
    h->deform_timed = true;
  }
  return 0;
}

}  // namespace

extern "C" int kmx_mesh_create(const kmx_mesh_params* params, int device, kmx_mesh** out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(out, KMX_EINVAL, "null argument");
  std::string err;
  if (int rc = kmx::mesh_check_params(params, &err)) return kmx::fail(rc, err);
  std::unique_ptr<kmx_mesh> h(new kmx_mesh());  // a failure below unwinds through the members' destructors
  int rc;
  if ((rc = h->open(device)) || (rc = kmx::create_events(h->ev))) return rc;
  h->P = *params;
  h->index.init(params->n_robots);
  if ((rc = h->d_off.alloc((size_t)params->n_robots + 1)) || (rc = h->d_stats.alloc(1)) || (rc = h->d_gblocks.alloc(1)))
    return rc;
  if (hipMemset(h->d_off.get(), 0, sizeof(int) * ((size_t)params->n_robots + 1)) != hipSuccess ||
      hipMemset(h->d_gblocks.get(), 0, sizeof(int)) != hipSuccess)
    return kmx::fail(KMX_EHIP, "hipMemset failed");
  if ((rc = mesh_reserve_nodes(h.get(), 1)) || (rc = mesh_reserve_vertices(h.get(), 1))) return rc;
  *out = h.release();
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_mesh_destroy(kmx_mesh* h) {
  return kmx::destroy(h);
}

extern "C" int kmx_mesh_set_stream(kmx_mesh* h, void* s) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  return h->adopt(s, true);
}

extern "C" int kmx_mesh_info(kmx_mesh* h, kmx_mesh_info_t* info, int64_t* per_robot_nodes,
                             int64_t* per_robot_vertices) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  if (info) {
    KMX_HIP(hipSetDevice(h->device));
    int gb = 0;
    KMX_HIP(hipMemcpyAsync(&gb, h->d_gblocks.get(), sizeof(int), hipMemcpyDeviceToHost, h->stream));
    KMX_HIP(hipStreamSynchronize(h->stream));
    info->n_nodes = h->index.n_nodes;
    info->n_vertices = h->n_vertices;
    info->node_capacity = h->ncap;
    info->vertex_capacity = h->vcap;
    // per node: Rrest, g, row, the pose staging, and the sorted stamp, id and position;
    // per vertex: xyz in and out, robot, stamp, count and k (id, weight) pairs
    info->device_bytes = h->ncap * (8 * (9 + 3 + MESH_ROW + 9 + 3) + 8 + 4 + 24) +
                         h->vcap * (12 + 12 + 4 + 8 + 4 + 12 * (int64_t)h->P.k) +
                         (h->vcap + MESH_BLOCK - 1) / MESH_BLOCK * (int64_t)sizeof(MeshPartial);
    info->k = h->P.k;
    info->lds_nodes = MESH_LDS_NODES;
    info->last_bind_blocks = h->last_bind_blocks;
    info->last_bind_global_blocks = gb;
  }
  for (int a = 0; a < h->P.n_robots; ++a) {
    if (per_robot_nodes) per_robot_nodes[a] = (int64_t)h->index.ids[(size_t)a].size();
    if (per_robot_vertices) per_robot_vertices[a] = h->index.n_vertices[(size_t)a];
  }
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_mesh_add_nodes(kmx_mesh* h, int64_t n, const int32_t* robot, const int64_t* stamp_ns,
                                  const double* Rrest, const double* g) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  std::string err;
  if (int rc = h->index.check_nodes(n, robot, stamp_ns, Rrest, g, &err)) return kmx::fail(rc, err);
  if (n == 0) return KMX_OK;
  KMX_HIP(hipSetDevice(h->device));
  const int64_t n0 = h->index.n_nodes;
  if (int rc = mesh_reserve_nodes(h, n0 + n)) return rc;
  KMX_HIP(hipMemcpyAsync(h->d_rrest.get() + 9 * n0, Rrest, sizeof(double) * 9 * n, hipMemcpyHostToDevice, h->stream));
  KMX_HIP(hipMemcpyAsync(h->d_g.get() + 3 * n0, g, sizeof(double) * 3 * n, hipMemcpyHostToDevice, h->stream));
  // current = rest until kmx_mesh_set_node_poses says otherwise
  if (int rc = mesh_form_rows(h, n0, n, h->d_rrest.get() + 9 * n0, h->d_g.get() + 3 * n0)) return rc;
  KMX_HIP(hipStreamSynchronize(h->stream));  // the caller's arrays are free again
  h->index.append_nodes(n, robot, stamp_ns, g);
  h->nodes_dirty = true;
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_mesh_set_node_poses(kmx_mesh* h, int64_t first, int64_t n, const double* Rcur, const double* p) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(kmx::mesh_range_ok(first, n, h->index.n_nodes), KMX_EINVAL, "node range outside the nodes added");
  if (n == 0) return KMX_OK;
  KMX_CHECK(Rcur && p, KMX_EINVAL, "null pose array");
  KMX_CHECK(kmx::mesh_all_finite(Rcur, (size_t)n * 9) && kmx::mesh_all_finite(p, (size_t)n * 3), KMX_EINVAL,
            "node pose is not finite");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipMemcpyAsync(h->d_rcur.get() + 9 * first, Rcur, sizeof(double) * 9 * n, hipMemcpyHostToDevice, h->stream));
  KMX_HIP(hipMemcpyAsync(h->d_p.get() + 3 * first, p, sizeof(double) * 3 * n, hipMemcpyHostToDevice, h->stream));
  if (int rc = mesh_form_rows(h, first, n, h->d_rcur.get() + 9 * first, h->d_p.get() + 3 * first)) return rc;
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_mesh_add_vertices(kmx_mesh* h, int64_t n, const int32_t* robot, const int64_t* stamp_ns,
                                     const float* xyz, int64_t* first_id_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  std::string err;
  if (int rc = h->index.check_vertices(n, h->n_vertices, robot, stamp_ns, xyz, &err)) return kmx::fail(rc, err);
  if (first_id_out) *first_id_out = h->n_vertices;
  if (n == 0) return KMX_OK;
  KMX_HIP(hipSetDevice(h->device));
  const int64_t v0 = h->n_vertices;
  if (int rc = mesh_reserve_vertices(h, v0 + n)) return rc;
  KMX_HIP(hipMemcpyAsync(h->d_vxyz.get() + 3 * v0, xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice, h->stream));
  KMX_HIP(hipMemcpyAsync(h->d_vrobot.get() + v0, robot, sizeof(int) * n, hipMemcpyHostToDevice, h->stream));
  KMX_HIP(hipMemcpyAsync(h->d_vstamp.get() + v0, stamp_ns, sizeof(long long) * n, hipMemcpyHostToDevice, h->stream));
  KMX_HIP(hipMemsetAsync(h->d_bcnt.get() + v0, 0, sizeof(int) * n, h->stream));  // unbound
  KMX_HIP(hipMemsetAsync(h->d_bidx.get() + v0 * h->P.k, 0xff, sizeof(int) * n * h->P.k, h->stream));
  KMX_HIP(hipMemsetAsync(h->d_bw.get() + v0 * h->P.k, 0, sizeof(double) * n * h->P.k, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  h->index.count_vertices(n, robot);
  h->n_vertices = v0 + n;
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_mesh_bind(kmx_mesh* h, int64_t first, int64_t n) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(kmx::mesh_range_ok(first, n, h->n_vertices), KMX_EINVAL, "vertex range outside the vertices added");
  if (n == 0) return KMX_OK;
  KMX_HIP(hipSetDevice(h->device));
  if (h->nodes_dirty) {
    KMX_HIP(hipStreamSynchronize(h->stream));
    h->index.sorted_layout(&h->h_off, &h->h_s_stamp, &h->h_s_id, &h->h_s_g);
    const size_t nn = (size_t)h->index.n_nodes;
    KMX_HIP(hipMemcpyAsync(h->d_off.get(), h->h_off.data(), sizeof(int) * h->h_off.size(), hipMemcpyHostToDevice,
                           h->stream));
    if (nn) {
      KMX_HIP(hipMemcpyAsync(h->d_s_stamp.get(), h->h_s_stamp.data(), sizeof(long long) * nn, hipMemcpyHostToDevice,
                             h->stream));
      KMX_HIP(hipMemcpyAsync(h->d_s_id.get(), h->h_s_id.data(), sizeof(int) * nn, hipMemcpyHostToDevice, h->stream));
      KMX_HIP(hipMemcpyAsync(h->d_s_g.get(), h->h_s_g.data(), sizeof(double) * 3 * nn, hipMemcpyHostToDevice,
                             h->stream));
    }
    h->nodes_dirty = false;
  }
  KMX_HIP(hipMemsetAsync(h->d_gblocks.get(), 0, sizeof(int), h->stream));
  MeshBindArgs a{(long long)first, (long long)n, (long long)h->P.window_ns, h->d_off.get(), h->d_s_stamp.get(),
                 h->d_s_id.get(), h->d_s_g.get(), h->d_vxyz.get(), h->d_vrobot.get(), h->d_vstamp.get(),
                 h->d_bidx.get(), h->d_bw.get(), h->d_bcnt.get(), h->d_gblocks.get()};
  const int blocks = (int)((n + MESH_BLOCK - 1) / MESH_BLOCK);
  if (h->timing) KMX_HIP(hipEventRecord(h->ev[0], h->stream));
#define MESH_CALL(K) mesh_launch_bind<K>(h, a, blocks)
  MESH_K_SWITCH(h->P.k, MESH_CALL)
#undef MESH_CALL
  KMX_HIP(hipGetLastError());
  if (h->timing) {
    KMX_HIP(hipEventRecord(h->ev[1], h->stream));
    h->bind_timed = true;
  }
  h->last_bind_blocks = blocks;
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_mesh_get_bindings(kmx_mesh* h, int64_t first, int64_t n, int32_t* idx, double* w, int32_t* count) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(kmx::mesh_range_ok(first, n, h->n_vertices), KMX_EINVAL, "vertex range outside the vertices added");
  if (n == 0) return KMX_OK;
  KMX_HIP(hipSetDevice(h->device));
  const size_t k = (size_t)h->P.k;
  if (idx)
    KMX_HIP(hipMemcpyAsync(idx, h->d_bidx.get() + first * k, sizeof(int) * n * k, hipMemcpyDeviceToHost, h->stream));
  if (w) KMX_HIP(hipMemcpyAsync(w, h->d_bw.get() + first * k, sizeof(double) * n * k, hipMemcpyDeviceToHost,
                                h->stream));
  if (count) KMX_HIP(hipMemcpyAsync(count, h->d_bcnt.get() + first, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_mesh_deform_device(kmx_mesh* h, int64_t first, int64_t n, void* dev_xyz_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(kmx::mesh_range_ok(first, n, h->n_vertices), KMX_EINVAL, "vertex range outside the vertices added");
  if (n == 0) return KMX_OK;
  KMX_CHECK(dev_xyz_out, KMX_EINVAL, "null output");
  KMX_HIP(hipSetDevice(h->device));
  return mesh_enqueue_deform(h, first, n, static_cast<float*>(dev_xyz_out));
  KMX_GUARD_END
}

extern "C" int kmx_mesh_deform(kmx_mesh* h, int64_t first, int64_t n, float* xyz_out, kmx_mesh_stats* stats_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(kmx::mesh_range_ok(first, n, h->n_vertices), KMX_EINVAL, "vertex range outside the vertices added");
  if (stats_out) *stats_out = kmx_mesh_stats{n, 0, 0, 0.0, 0.0};
  if (n == 0) return KMX_OK;
  KMX_CHECK(xyz_out, KMX_EINVAL, "null output");
  KMX_HIP(hipSetDevice(h->device));
  if (int rc = mesh_enqueue_deform(h, first, n, h->d_out.get())) return rc;
  MeshStatsDev s{};
  KMX_HIP(hipMemcpyAsync(xyz_out, h->d_out.get(), sizeof(float) * 3 * n, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipMemcpyAsync(&s, h->d_stats.get(), sizeof(s), hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  if (stats_out) {
    stats_out->n_unbound = s.unbound;
    stats_out->n_partial = s.partial;
    stats_out->max_displacement = std::sqrt(s.max);
    stats_out->sum_sq_displacement = s.sum;
  }
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_mesh_sync(kmx_mesh* h) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
}

extern "C" int kmx_mesh_enable_timing(kmx_mesh* h, int enable) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  h->timing = enable != 0;
  h->bind_timed = h->deform_timed = false;
  return KMX_OK;
}

extern "C" int kmx_mesh_read_timing(kmx_mesh* h, double* bind_ms, double* deform_ms) {
  KMX_CHECK(h && bind_ms && deform_ms, KMX_EINVAL, "null argument");
  KMX_CHECK(h->timing, KMX_ESTATE, "timing is off: kmx_mesh_enable_timing");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  float a = 0.f, b = 0.f;
  if (h->bind_timed) KMX_HIP(hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
  if (h->deform_timed) KMX_HIP(hipEventElapsedTime(&b, h->ev[2], h->ev[3]));
  *bind_ms = a;
  *deform_ms = b;
  return KMX_OK;
}
