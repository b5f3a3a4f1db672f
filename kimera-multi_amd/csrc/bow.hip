// bow.hip — the BoW candidate stage of Kimera-Multi-LCD on MI355X (gfx950).
//
// Replaces DBoW2 Database::queryL1 and L1Scoring::score as called by
// LoopClosureDetector::detectLoop / detectLoopWithRobot (drawio:2574-2580,
// 2612-2633) behind kmx_bow_* (include/kmx_abi.h).
//
//   * k_bow_query: one workgroup per query (grid-stride over the batch), with
//     a private dense accumulator acc[n_entries] and touched-list in HBM.
//     The query's words are visited in increasing word id; for each word the
//     workgroup streams the word's posting list in parallel — an entry occurs
//     at most once per posting list, so there are no write conflicts inside a
//     word — and a barrier separates words. Every entry therefore accumulates
//     |q - d| - |q| - |d| in exactly DBoW2's order (word, then entry), so the
//     scores are bit-identical to the CPU restatement (oracle/bow_oracle.c).
//   * Top-K (max_db_results) by (acc ascending, entry id ascending):
//     LDS histograms over the acc range narrow the candidates to <= SEL_CAP,
//     which are sorted in LDS (bitonic) — no pass over all n_entries.
//   * k_bow_pair_score: one thread per pair, the sorted-list merge of
//     L1Scoring::score (nss factor against the previous keyframe).
//   * Database::add (kmx_bow_add_entries / kmx_bow_add_from_voc): every
//     entry's vector stays in a device-resident forward store; the newest
//     entries (the tail) are scored per query by k_bow_tail and merged with
//     the inverted file's results, and are sealed into the inverted file on
//     the device (k_bow_seal_*, k_bow_cptr) every tail_cap adds. Queries and
//     nss factors by entry id (k_bow_gather, k_bow_entry_score) read the
//     forward store, so a keyframe's vector never leaves the GPU.
//   * detectLoop's decision (kmx_bow_detect_entries / kmx_bow_decide_results):
//     k_bow_decide, a wave per query, does the nss gate, the alpha cut and
//     computeIslands; k_bow_temporal, one wave, checkTemporalConstraint over
//     the queries in order, its state resident in the handle across calls. One
//     48-byte record per query comes back.
// Compiled with -ffp-contract=off (no FMA to contract here anyway).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "bow_host.h"
#include "common.h"

namespace {

constexpr int BOW_BLOCK = 256;
constexpr int NBINS = 1024;
constexpr int SEL_CAP = 2048;
constexpr int MAX_RESULTS = 256;
constexpr int LEVELS = 6;

struct BowDb {
  const int* ptr;     // [n_words + 1]
  const int* ent;     // posting entry ids (increasing per word)
  const double* wt;   // posting weights
  int n_words, n_entries;
};

__device__ __forceinline__ bool key_less(double a, int ia, double b, int ib) {
  return a < b || (a == b && ia < ib);
}

// First histogram bin b at which the running count reaches `need` (the last
// bin if none does), and the count strictly before it: a block-wide prefix
// sum over NBINS bins (NBINS / BLOCK consecutive bins per thread), replacing
// a serial walk over the bins by one thread. Results in *sb, *scb; needs a
// __syncthreads() before they are read. `wsum` holds BLOCK / 64 ints.
template <int BLOCK>
__device__ __forceinline__ void find_bin(const int* hist, int need, int* wsum, int* sb, int* scb) {
  constexpr int PER = NBINS / BLOCK;
  static_assert(PER * BLOCK == NBINS, "NBINS must be a multiple of the block size");
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int h[PER], mine = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) { h[k] = hist[tid * PER + k]; mine += h[k]; }
  int incl = mine;  // inclusive scan over the wave
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  int base = 0;
  for (int k = 0; k < w; ++k) base += wsum[k];
  int cum = base + incl - mine;  // count before this thread's first bin
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int b = tid * PER + k;
    if (cum < need && cum + h[k] >= need) { *sb = b; *scb = cum; }
    else if (b == NBINS - 1 && cum + h[k] < need) { *sb = b; *scb = cum; }
    cum += h[k];
  }
}

// The workgroup's next query (workgroup-uniform): one atomic per query on a
// counter the launch starts at 0, so a workgroup that drew short posting lists
// takes more queries instead of every workgroup taking every gridDim-th one.
__device__ __forceinline__ int next_query(int* next, int nq) {
  __shared__ int s_q;
  __syncthreads();  // the previous query's readers of s_q are done
  if (threadIdx.x == 0) s_q = atomicAdd(next, 1);
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(min(s_q, nq));  // uniform: keep it in a scalar register
}

__global__ __launch_bounds__(BOW_BLOCK) void k_bow_query(BowDb db, int nq, const long long* qptr,
                                                         const unsigned* qw, const double* qv,
                                                         const int* max_id, int K, double* acc_all,
                                                         int* touched_all, int* out_n, int* out_id,
                                                         double* out_score, int* err, int* next) {
  __shared__ int s_nt, s_ns, s_b, s_cb, s_done;
  __shared__ int s_wsum[BOW_BLOCK / 64];
  __shared__ int hist[NBINS];
  __shared__ double c_val[SEL_CAP];
  __shared__ int c_id[SEL_CAP];
  const int tid = threadIdx.x;
  double* acc = acc_all + (size_t)blockIdx.x * db.n_entries;
  int* touched = touched_all + (size_t)blockIdx.x * db.n_entries;
  for (;;) {  // a work queue: the next query from a counter (queries differ in postings by 10x)
    const int q = next_query(next, nq);
    if (q >= nq) break;
    const int mid = max_id ? max_id[q] : -1;
    if (tid == 0) s_nt = 0;
    __syncthreads();
    // ---- phase 1: inverted-file accumulation, word by word
    for (long long i = qptr[q]; i < qptr[q + 1]; ++i) {
      const unsigned w = qw[i];
      if (w < (unsigned)db.n_words) {
        const double qval = qv[i];
        const int p0 = db.ptr[w], p1 = db.ptr[w + 1];
        for (int p = p0 + tid; p < p1; p += BOW_BLOCK) {
          const int e = db.ent[p];
          if (!(e < mid || mid == -1)) continue;
          const double d = db.wt[p];
          const double v = fabs(qval - d) - fabs(qval) - fabs(d);
          const double a = acc[e];
          if (a == 0.0) touched[atomicAdd(&s_nt, 1)] = e;  // values are < 0: 0 = untouched
          acc[e] = a + v;
        }
      }
      __syncthreads();
    }
    const int nt = s_nt;
    // ---- phase 2: top-K by (acc, id). Level l splits the current range into
    // NBINS bins; an entry stays in play while its bin equals the chosen bin
    // at every earlier level (bins recomputed from the same (lo, width) chain,
    // so membership is consistent), and is certain once its bin is below it.
    const int need0 = min(K, nt);
    int need = need0;
    double lvl_lo[LEVELS], lvl_w[LEVELS];
    int lvl_b[LEVELS];
    if (tid == 0) { s_ns = 0; s_done = 0; }
    __syncthreads();
    auto bin_of = [&](double a, int l) {
      int bb = (int)floor((a - lvl_lo[l]) / lvl_w[l]);
      return bb < 0 ? 0 : (bb >= NBINS ? NBINS - 1 : bb);
    };
    auto in_play = [&](double a, int level) {
      for (int l = 0; l < level; ++l)
        if (bin_of(a, l) != lvl_b[l]) return false;
      return true;
    };
    int level = 0;
    for (; level < LEVELS && need > 0; ++level) {
      lvl_lo[level] = level == 0 ? -2.0 : lvl_lo[level - 1] + lvl_b[level - 1] * lvl_w[level - 1];
      lvl_w[level] = (level == 0 ? 2.0 : lvl_w[level - 1]) / NBINS;
      for (int b = tid; b < NBINS; b += BOW_BLOCK) hist[b] = 0;
      __syncthreads();
      for (int i = tid; i < nt; i += BOW_BLOCK) {
        const double a = acc[touched[i]];
        if (in_play(a, level)) atomicAdd(&hist[bin_of(a, level)], 1);
      }
      __syncthreads();
      find_bin<BOW_BLOCK>(hist, need, s_wsum, &s_b, &s_cb);  // first bin reaching `need`
      __syncthreads();
      if (tid == 0) s_done = (s_ns + s_cb + hist[s_b] <= SEL_CAP) ? 1 : 0;
      __syncthreads();
      const int b = s_b, done = s_done, cb = s_cb;
      lvl_b[level] = b;
      for (int i = tid; i < nt; i += BOW_BLOCK) {
        const int e = touched[i];
        const double a = acc[e];
        if (!in_play(a, level)) continue;
        const int bb = bin_of(a, level);
        if (bb < b || (done && bb == b)) {
          const int slot = atomicAdd(&s_ns, 1);
          if (slot < SEL_CAP) { c_val[slot] = a; c_id[slot] = e; }
        }
      }
      __syncthreads();
      if (done) { need = 0; break; }
      need -= cb;
    }
    if (need > 0 && tid == 0) atomicExch(err, 1);  // > SEL_CAP exactly tied scores
    const int nc = min(s_ns, SEL_CAP);
    // bitonic sort of the candidates (padded to a power of two)
    int n2 = 1;
    while (n2 < nc) n2 <<= 1;
    for (int i = nc + tid; i < n2; i += BOW_BLOCK) { c_val[i] = 1.0; c_id[i] = 0x7fffffff; }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < n2; i += BOW_BLOCK) {
          const int l = i ^ j;
          if (l > i) {
            const bool up = (i & k) == 0;
            const bool sw = up ? key_less(c_val[l], c_id[l], c_val[i], c_id[i])
                               : key_less(c_val[i], c_id[i], c_val[l], c_id[l]);
            if (sw) {
              const double tv = c_val[i]; c_val[i] = c_val[l]; c_val[l] = tv;
              const int ti = c_id[i]; c_id[i] = c_id[l]; c_id[l] = ti;
            }
          }
        }
        __syncthreads();
      }
    }
    const int nout = min(need0, nc);
    for (int i = tid; i < nout; i += BOW_BLOCK) {
      out_id[(size_t)q * K + i] = c_id[i];
      out_score[(size_t)q * K + i] = -c_val[i] / 2.0;
    }
    if (tid == 0) out_n[q] = nout;
    // ---- phase 3: clear the accumulator for the next query
    for (int i = tid; i < nt; i += BOW_BLOCK) acc[touched[i]] = 0.0;
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// k_bow_query_lds: the same queryL1 with the accumulator in LDS.
//   * The database's entries are cut into chunks of `ch` (<= LCH) entries; a
//     chunk's accumulator is an LDS array, so the per-posting read-modify-write
//     that bounds k_bow_query (a dependent HBM round trip per word, then a
//     workgroup barrier) becomes an LDS one.
//   * Within a chunk, wave v of the LW_WAVES owns the entry sub-range
//     [v*sch, (v+1)*sch): it walks the query's words in order over its own
//     part of each posting list ([cptr[w][s], cptr[w][s+1]), s = sub-chunk;
//     lists ascend in entry id). No two waves touch an entry and a wave's LDS
//     operations complete in order, so every entry accumulates in DBoW2's
//     word order with no barrier at all. The wave applies several words'
//     pieces per step (collisions detected by LDS marks) and keeps three
//     steps of postings in flight (unconditional clamped loads, so the
//     compiler waits only for the step being applied).
//   * After each chunk, the chunk's K best (acc, id) are selected as in
//     k_bow_query (LDS histograms + bitonic sort) and merged with the running
//     list by merge-path ranks, so the result equals a top-K over all entries.
constexpr int LW_WAVES = 16;
constexpr int LW_BLOCK = 64 * LW_WAVES;
constexpr int LCH = 14336;     // max entries per chunk (112 KB of LDS), a multiple of LW_WAVES
constexpr int LSEL = 1024;     // candidate cap per chunk
constexpr int QW = 128;        // query words staged per batch
#ifndef KMX_BOW_PG
#define KMX_BOW_PG 8
#endif
constexpr int PG = KMX_BOW_PG;  // lanes per piece group: a step applies 64 / PG pieces of <= PG postings
constexpr int NGRP = 64 / PG;
constexpr int PC = 176;        // pieces per wave table

__global__ __launch_bounds__(LW_BLOCK) void k_bow_query_lds(BowDb db, const int* cptr, int nch, int ch, int nq,
                                                            const long long* qptr, const unsigned* qw,
                                                            const double* qv, const int* max_id, int K,
                                                            int* out_n, int* out_id, double* out_score,
                                                            int* err, int* next) {
  extern __shared__ __attribute__((aligned(16))) char bsm[];
  double* acc = reinterpret_cast<double*>(bsm);                   // [ch]
  double* c_val = acc + LCH;                                        // [LSEL]        \  selection scratch;
  double* m_val = c_val + LSEL;                                     // [MAX_RESULTS]  | the accumulation's
  int* c_id = reinterpret_cast<int*>(m_val + MAX_RESULTS);          // [LSEL]         | conflict marks
  int* m_id = c_id + LSEL;                                          // [MAX_RESULTS] /  alias it
  double* r_val = reinterpret_cast<double*>(m_id + MAX_RESULTS);    // [MAX_RESULTS] running best
  double* wq = r_val + MAX_RESULTS;                                 // [QW] query weights
  int* r_id = reinterpret_cast<int*>(wq + QW);                      // [MAX_RESULTS]
  int* pstart = r_id + MAX_RESULTS;                                 // [LW_WAVES][PC] piece: first posting
  unsigned short* pinfo = reinterpret_cast<unsigned short*>(pstart + LW_WAVES * PC);  // len-1 | word << 4
  int* hist = reinterpret_cast<int*>(pinfo + LW_WAVES * PC);        // [NBINS]
  __shared__ int s_ns, s_b, s_cb, s_done, s_nt, s_nr;
  __shared__ int s_wsum[LW_WAVES];
  const int tid = threadIdx.x, v = tid >> 6, lane = tid & 63;
  const int nsub = nch * LW_WAVES, sch = ch / LW_WAVES;
  for (;;) {  // a work queue: the next query from a counter (queries differ in postings by 10x)
    const int q = next_query(next, nq);
    if (q >= nq) break;
    const int mid = max_id ? max_id[q] : -1;
    const int lim = (mid < 0) ? db.n_entries : min(mid, db.n_entries);  // entries < lim are eligible
    const long long q0 = qptr[q], q1 = qptr[q + 1];
    if (tid == 0) s_nr = 0;
    for (int c = 0; c < nch && c * ch < lim; ++c) {
      const int lo = c * ch, n_here = min(ch, lim - lo);
      for (int i = tid; i < n_here; i += LW_BLOCK) acc[i] = 0.0;
      // ---- accumulation, query words in order, QW words staged at a time.
      // Each wave turns its sub-range of the batch's posting lists into pieces
      // of <= PG postings (a long list becomes consecutive pieces of the same
      // word) and applies 64 / PG pieces per step, one per PG-lane group
      // (PG = 8: 8 pieces; 16 and 32 measured 5 % and 29 % slower). Pieces of
      // different words may hit the same entry: the lanes mark their entries
      // with their group and read the marks back; on a collision the step's
      // pieces are applied one after another, so every entry still
      // accumulates in word order.
      int* my_start = pstart + v * PC;
      unsigned short* my_info = pinfo + v * PC;
      // volatile: the read-back must see other lanes' writes (no store-to-load forwarding)
      volatile unsigned char* mark = reinterpret_cast<unsigned char*>(c_val) + v * sch;
      const int g = lane / PG, j = lane - g * PG;
      const int sub = c * LW_WAVES + v;
      const bool sub_live = lo + v * sch < lim;
      const bool sub_cut = lo + (v + 1) * sch > lim;  // the sub-range holding max_id: drop entries >= lim
      const int mlo = lo + v * sch;
      auto run = [&](int np) {  // apply this wave's piece table [0, np)
        const int nst = (np + NGRP - 1) / NGRP;
        auto fetch = [&](int st, int& e, double& dv, int& wi, bool& ok) {
          const int pc = min(NGRP * st + g, max(np - 1, 0));
          const unsigned info = my_info[pc];
          ok = (NGRP * st + g < np) && (j <= (int)(info & 31u));
          wi = (int)(info >> 5);
          const int idx = ok ? my_start[pc] + j : 0;
          e = db.ent[idx];
          dv = db.wt[idx];
        };
        auto apply = [&](int e, double dv, int wi, bool ok) {
          const int el = e - mlo;
          if (ok) mark[el] = (unsigned char)g;
          bool clash = ok && mark[el] != (unsigned char)g;
          const double qval = wq[wi];
          const double val = fabs(qval - dv) - fabs(qval) - fabs(dv);
          if (!__any(clash)) {
            if (ok) acc[e - lo] += val;
          } else {  // one group at a time, in piece (= word) order
            volatile double* vacc = acc;
            for (int gg = 0; gg < NGRP; ++gg) {
              if (ok && g == gg) vacc[e - lo] = vacc[e - lo] + val;
              __builtin_amdgcn_wave_barrier();
              asm volatile("" ::: "memory");
            }
          }
        };
        int e0, e1, e2, e3, w0, w1, w2, w3;
        double d0, d1, d2, d3;
        bool k0, k1, k2, k3;
        fetch(0, e0, d0, w0, k0);
        fetch(1, e1, d1, w1, k1);
        fetch(2, e2, d2, w2, k2);
        for (int st = 0; st < nst; st += 4) {
          fetch(st + 3, e3, d3, w3, k3);
          apply(e0, d0, w0, k0);
          if (st + 1 >= nst) break;
          fetch(st + 4, e0, d0, w0, k0);
          apply(e1, d1, w1, k1);
          if (st + 2 >= nst) break;
          fetch(st + 5, e1, d1, w1, k1);
          apply(e2, d2, w2, k2);
          if (st + 3 >= nst) break;
          fetch(st + 6, e2, d2, w2, k2);
          apply(e3, d3, w3, k3);
        }
      };
      for (long long b0 = q0; b0 < q1; b0 += QW) {
        const int nw = (int)min((long long)QW, q1 - b0);
        __syncthreads();  // accumulator zeroed / previous batch's weights no longer read
        for (int i = tid; i < nw; i += LW_BLOCK) wq[i] = qv[b0 + i];
        __syncthreads();
        int np = 0;
        for (int w0 = 0; w0 < nw; w0 += 64) {
          // this lane's word: posting range in the wave's sub-range, piece count
          const int i = w0 + lane;
          int a = 0, b = 0;
          if (i < nw && sub_live) {
            const unsigned w = qw[b0 + i];
            if (w < (unsigned)db.n_words) {
              a = cptr[(size_t)w * (nsub + 1) + sub];
              b = cptr[(size_t)w * (nsub + 1) + sub + 1];
              if (sub_cut)
                while (a < b && db.ent[b - 1] >= lim) --b;
            }
          }
          const int cnt = (b - a + PG - 1) / PG;
          int incl = cnt;  // inclusive scan of the piece counts over the wave
#pragma unroll
          for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
          }
          const int gtot = __shfl(incl, 63, 64);
          if (np + gtot > PC) {  // table full: apply it first
            run(np);
            np = 0;
          }
          if (gtot > PC) {  // one 64-word group with very long lists: plain order-preserving loop
            for (int k = 0; k < 64 && w0 + k < nw; ++k) {
              const int ak = __shfl(a, k, 64), bk = __shfl(b, k, 64);
              const double qval = wq[w0 + k];
              for (int sl = ak + lane; sl < bk; sl += 64) {
                const double d = db.wt[sl];
                acc[db.ent[sl] - lo] += fabs(qval - d) - fabs(qval) - fabs(d);
              }
            }
            continue;
          }
          for (int k = 0, pos = np + incl - cnt; k < cnt; ++k, ++pos) {
            my_start[pos] = a + k * PG;
            my_info[pos] = (unsigned short)((min(PG, b - a - k * PG) - 1) | (i << 5));
          }
          np += gtot;
        }
        run(np);
      }
      __syncthreads();
      // ---- this chunk's best min(K, touched) by (acc, id): LDS histogram narrowing
      if (tid == 0) { s_nt = 0; s_ns = 0; s_done = 0; }
      __syncthreads();
      {
        int cnt = 0;
        for (int i = tid; i < n_here; i += LW_BLOCK) cnt += (acc[i] != 0.0) ? 1 : 0;
        if (cnt) atomicAdd(&s_nt, cnt);
      }
      __syncthreads();
      const int nt = s_nt;
      const int need0 = min(K, nt);
      int need = need0;
      double lvl_lo[LEVELS], lvl_w[LEVELS];
      int lvl_b[LEVELS];
      auto bin_of = [&](double a, int l) {
        int bb = (int)floor((a - lvl_lo[l]) / lvl_w[l]);
        return bb < 0 ? 0 : (bb >= NBINS ? NBINS - 1 : bb);
      };
      auto in_play = [&](double a, int level) {
        for (int l = 0; l < level; ++l)
          if (bin_of(a, l) != lvl_b[l]) return false;
        return true;
      };
      for (int level = 0; level < LEVELS && need > 0; ++level) {
        lvl_lo[level] = level == 0 ? -2.0 : lvl_lo[level - 1] + lvl_b[level - 1] * lvl_w[level - 1];
        lvl_w[level] = (level == 0 ? 2.0 : lvl_w[level - 1]) / NBINS;
        for (int b = tid; b < NBINS; b += LW_BLOCK) hist[b] = 0;
        __syncthreads();
        for (int i = tid; i < n_here; i += LW_BLOCK) {
          const double a = acc[i];
          if (a != 0.0 && in_play(a, level)) atomicAdd(&hist[bin_of(a, level)], 1);
        }
        __syncthreads();
        find_bin<LW_BLOCK>(hist, need, s_wsum, &s_b, &s_cb);  // first bin reaching `need`
        __syncthreads();
        if (tid == 0) s_done = (s_ns + s_cb + hist[s_b] <= LSEL) ? 1 : 0;
        __syncthreads();
        const int b = s_b, done = s_done, cb = s_cb;
        lvl_b[level] = b;
        for (int i = tid; i < n_here; i += LW_BLOCK) {
          const double a = acc[i];
          if (a == 0.0 || !in_play(a, level)) continue;
          const int bb = bin_of(a, level);
          if (bb < b || (done && bb == b)) {
            const int slot = atomicAdd(&s_ns, 1);
            if (slot < LSEL) { c_val[slot] = a; c_id[slot] = lo + i; }
          }
        }
        __syncthreads();
        if (done) { need = 0; break; }
        need -= cb;
      }
      if (need > 0 && tid == 0) atomicExch(err, 1);  // > LSEL exactly tied scores
      const int nc = min(s_ns, LSEL);
      int n2 = 1;
      while (n2 < nc) n2 <<= 1;
      for (int i = nc + tid; i < n2; i += LW_BLOCK) { c_val[i] = 1.0; c_id[i] = 0x7fffffff; }
      __syncthreads();
      for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int i = tid; i < n2; i += LW_BLOCK) {
            const int l = i ^ j;
            if (l > i) {
              const bool up = (i & k) == 0;
              const bool sw = up ? key_less(c_val[l], c_id[l], c_val[i], c_id[i])
                                 : key_less(c_val[i], c_id[i], c_val[l], c_id[l]);
              if (sw) {
                const double tv = c_val[i]; c_val[i] = c_val[l]; c_val[l] = tv;
                const int ti = c_id[i]; c_id[i] = c_id[l]; c_id[l] = ti;
              }
            }
          }
          __syncthreads();
        }
      }
      // ---- merge the chunk's sorted best (na) into the running best (nr) by ranks
      const int na = min(need0, nc), nr = s_nr;
      const int nm = min(K, na + nr);
      for (int i = tid; i < na + nr; i += LW_BLOCK) {
        const bool fromA = i < na;
        const int k = fromA ? i : i - na;
        const double val = fromA ? c_val[k] : r_val[k];
        const int id = fromA ? c_id[k] : r_id[k];
        int l = 0, h = fromA ? nr : na;  // elements of the other list ordered before (val, id)
        while (l < h) {
          const int m = (l + h) >> 1;
          const bool before = fromA ? key_less(r_val[m], r_id[m], val, id) : key_less(c_val[m], c_id[m], val, id);
          if (before) l = m + 1;
          else h = m;
        }
        const int pos = k + l;
        if (pos < nm) { m_val[pos] = val; m_id[pos] = id; }
      }
      __syncthreads();
      for (int i = tid; i < nm; i += LW_BLOCK) { r_val[i] = m_val[i]; r_id[i] = m_id[i]; }
      if (tid == 0) s_nr = nm;
      __syncthreads();
    }
    __syncthreads();
    const int nout = s_nr;
    for (int i = tid; i < nout; i += LW_BLOCK) {
      out_id[(size_t)q * K + i] = r_id[i];
      out_score[(size_t)q * K + i] = -r_val[i] / 2.0;
    }
    if (tid == 0) out_n[q] = nout;
    __syncthreads();
  }
}
constexpr size_t LDS_BOW = sizeof(double) * (LCH + LSEL + 2 * MAX_RESULTS + QW) +
                           sizeof(int) * (LSEL + 2 * MAX_RESULTS + LW_WAVES * PC + NBINS) +
                           sizeof(unsigned short) * LW_WAVES * PC;
static_assert(LW_WAVES * (LCH / LW_WAVES) <= sizeof(double) * (LSEL + MAX_RESULTS) + sizeof(int) * (LSEL + MAX_RESULTS),
              "conflict marks must fit the selection scratch");
static_assert(QW <= 2048 && PG <= 32 && 64 % PG == 0, "piece info packs len - 1 in 5 bits and the word in 11");
static_assert(LDS_BOW + 64 <= 160 * 1024, "k_bow_query_lds exceeds the 160 KiB of LDS per CU");

// L1Scoring::score of pairs (a_i, b_i): merge of the two sorted word lists.
__global__ void k_bow_pair_score(int n, const long long* aptr, const unsigned* aw, const double* av,
                                 const long long* bptr, const unsigned* bw, const double* bv, double* out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  long long i = aptr[t], j = bptr[t];
  const long long ie = aptr[t + 1], je = bptr[t + 1];
  double s = 0.0;
  while (i < ie && j < je) {
    const unsigned x = aw[i], y = bw[j];
    if (x == y) {
      s += fabs(av[i] - bv[j]) - fabs(av[i]) - fabs(bv[j]);
      ++i;
      ++j;
    } else if (x < y) {
      ++i;
    } else {
      ++j;
    }
  }
  out[t] = -s / 2.0;
}

// ---------------------------------------------------------------------------
// The streaming database (Database::add): a forward store of every entry's
// vector, entry-major, a sealed base [0, n_sealed) that the two query kernels
// above serve unchanged, and an unsealed tail [n_sealed, n_entries) that
// exists only in the forward store.
struct BowFwd {
  const long long* fptr;  // [n_entries + 1]
  const unsigned* fw;     // words, strictly increasing per entry
  const double* fv;       // weights
};

constexpr int TAIL_MAX = 1024;      // the largest tail_cap: what k_bow_tail's LDS sort holds beside MAX_RESULTS
constexpr int TAIL_DEFAULT = 64;    // measured: DESIGN.md section 12
constexpr int TL_WAVES = 16;
constexpr int TL_BLOCK = 64 * TL_WAVES;
constexpr int TL_QW = 2048;         // query words staged in LDS (longer queries are searched in HBM)
constexpr int TL_SORT = 2048;       // >= TAIL_MAX + MAX_RESULTS, a power of two
static_assert(TAIL_MAX + MAX_RESULTS <= TL_SORT && (TL_SORT & (TL_SORT - 1)) == 0, "tail sort capacity");

// L1Scoring::score of stored entries a and b; an id of -1 scores 0 and reads nothing.
__device__ __forceinline__ double entry_score(const BowFwd& f, int a, int b) {
  double s = 0.0;
  if (a >= 0 && b >= 0) {
    long long i = f.fptr[a], j = f.fptr[b];
    const long long ie = f.fptr[a + 1], je = f.fptr[b + 1];
    while (i < ie && j < je) {
      const unsigned x = f.fw[i], y = f.fw[j];
      if (x == y) {
        s += fabs(f.fv[i] - f.fv[j]) - fabs(f.fv[i]) - fabs(f.fv[j]);
        ++i;
        ++j;
      } else if (x < y) {
        ++i;
      } else {
        ++j;
      }
    }
  }
  return -s / 2.0;
}

// The same for pairs of stored entries a_ids[t], b_ids[t].
__global__ void k_bow_entry_score(int n, BowFwd f, const int* a_ids, const int* b_ids, double* out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  out[t] = entry_score(f, a_ids[t], b_ids[t]);
}

// Inclusive scan of one value per thread over a block of TL_BLOCK threads
// (every thread calls it); *total = the block's sum. s_w holds TL_WAVES values.
__device__ __forceinline__ long long block_scan_incl(long long x, long long* s_w, long long* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  long long incl = x;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const long long t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 63) s_w[w] = incl;
  __syncthreads();
  long long base = 0, tot = 0;
  for (int k = 0; k < TL_WAVES; ++k) {
    if (k < w) base += s_w[k];
    tot += s_w[k];
  }
  __syncthreads();  // s_w may be written again
  *total = tot;
  return base + incl;
}

// One block. SRC 0: out[i + 1] = out[0] + sum of nnz[0..i] (appending a
// vocabulary batch: out = fptr + n_entries). SRC 1: out[0] = 0, out[i + 1] =
// the summed lengths of entries ids[0..i] (queries by entry id).
template <int SRC>
__global__ __launch_bounds__(TL_BLOCK) void k_bow_scan_len(int n, const int* nnz_or_ids, const long long* fptr,
                                                           long long* out) {
  __shared__ long long s_w[TL_WAVES];
  long long carry = SRC == 0 ? out[0] : 0;
  if (SRC == 1 && threadIdx.x == 0) out[0] = 0;
  for (int t0 = 0; t0 < n; t0 += TL_BLOCK) {
    const int i = t0 + (int)threadIdx.x;
    long long len = 0;
    if (i < n) {
      const int v = nnz_or_ids[i];
      len = SRC == 0 ? v : fptr[v + 1] - fptr[v];
    }
    long long tot;
    const long long incl = block_scan_incl(len, s_w, &tot);
    if (i < n) out[i + 1] = carry + incl;
    carry += tot;
  }
}

// Frame b of a vocabulary batch (nnz[b] words at stride) -> its place in the forward store.
__global__ void k_bow_voc_compact(const int* nnz, const unsigned* words, const double* weights, int stride,
                                  const long long* fptr_new, unsigned* fw, double* fv) {
  const int b = blockIdx.x;
  const int n = min(nnz[b], stride);
  const long long dst = fptr_new[b];
  for (int k = threadIdx.x; k < n; k += blockDim.x) {
    fw[dst + k] = words[(size_t)b * stride + k];
    fv[dst + k] = weights[(size_t)b * stride + k];
  }
}

// Query q := entry ids[q] of `src`, copied to the query buffers (qptr from k_bow_scan_len<1>).
__global__ void k_bow_gather(BowFwd src, const int* ids, const long long* qptr, unsigned* qw, double* qv) {
  const int q = blockIdx.x;
  const long long s0 = src.fptr[ids[q]], d0 = qptr[q];
  const int n = (int)(qptr[q + 1] - d0);
  for (int k = threadIdx.x; k < n; k += blockDim.x) {
    qw[d0 + k] = src.fw[s0 + k];
    qv[d0 + k] = src.fv[s0 + k];
  }
}

// k_bow_tail: after a base query kernel, score the unsealed entries against
// each query and merge them into its results in place. One workgroup per
// query (grid-stride). A wave per tail entry: the lanes read 64 consecutive
// words of the entry, each looks its word up in the query (staged in LDS,
// sorted: a binary search), and the matches are added lane by lane in ballot
// order, so the sum is one chain over the common words in increasing word id
// starting from 0.0 — the chain k_bow_query / k_bow_query_lds build for a
// sealed entry, bit for bit. Query words >= n_words cannot match: stored
// words are < n_words. A tail entry is a result iff its sum is non-zero and
// (id < max_id or max_id == -1). The candidates (<= TAIL_MAX) and the base's
// results (<= MAX_RESULTS) are sorted in LDS by (score descending, id
// ascending); score = -acc / 2 is exact, so this is the (acc, id) order.
__global__ __launch_bounds__(TL_BLOCK) void k_bow_tail(BowFwd f, int n_sealed, int n_entries, int nq,
                                                       const long long* qptr, const unsigned* qw, const double* qv,
                                                       const int* max_id, int K, int* out_n, int* out_id,
                                                       double* out_score) {
  __shared__ double c_val[TL_SORT];
  __shared__ double s_qv[TL_QW];
  __shared__ int c_id[TL_SORT];
  __shared__ unsigned s_qw[TL_QW];
  __shared__ int s_nc;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int q = blockIdx.x; q < nq; q += gridDim.x) {
    const long long q0 = qptr[q];
    const int nw = (int)min(qptr[q + 1] - q0, (long long)INT32_MAX);
    const bool staged = nw <= TL_QW;
    __syncthreads();  // the previous query's readers of LDS are done
    if (staged)
      for (int i = tid; i < nw; i += TL_BLOCK) {
        s_qw[i] = qw[q0 + i];
        s_qv[i] = qv[q0 + i];
      }
    if (tid == 0) s_nc = 0;
    __syncthreads();
    const unsigned* sw = staged ? s_qw : qw + q0;
    const double* sv = staged ? s_qv : qv + q0;
    const int mid = max_id ? max_id[q] : -1;
    const int hi = (mid == -1) ? n_entries : min(mid, n_entries);  // entries < hi are eligible
    for (int e = n_sealed + wv; e < hi; e += TL_WAVES) {
      const long long p0 = f.fptr[e], p1 = f.fptr[e + 1];
      double s = 0.0;
      for (long long pb = p0; pb < p1; pb += 64) {
        const long long p = pb + lane;
        const bool ok = p < p1;
        const unsigned w = ok ? f.fw[p] : 0u;
        int lo = 0, up = nw;
        while (lo < up) {
          const int m = (lo + up) >> 1;
          if (sw[m] < w) lo = m + 1;
          else up = m;
        }
        const bool hit = ok && lo < nw && sw[lo] == w;
        double v = 0.0;
        if (hit) {
          const double qval = sv[lo], d = f.fv[p];
          v = fabs(qval - d) - fabs(qval) - fabs(d);
        }
        unsigned long long mask = __ballot(hit);
        while (mask) {  // ordered: lane order is word order
          const int l = __ffsll((long long)mask) - 1;
          s += __shfl(v, l, 64);
          mask &= mask - 1;
        }
      }
      if (lane == 0 && s != 0.0) {
        const int slot = atomicAdd(&s_nc, 1);  // <= tail size <= TAIL_MAX
        if (slot < TAIL_MAX) { c_val[slot] = -s / 2.0; c_id[slot] = e; }
      }
    }
    __syncthreads();
    const int nc = min(s_nc, TAIL_MAX);
    if (nc == 0) continue;  // the base's results stand
    const int nb = min(out_n[q], K);
    for (int i = tid; i < nb; i += TL_BLOCK) {
      c_val[nc + i] = out_score[(size_t)q * K + i];
      c_id[nc + i] = out_id[(size_t)q * K + i];
    }
    const int nt = nc + nb;
    int n2 = 1;
    while (n2 < nt) n2 <<= 1;
    for (int i = nt + tid; i < n2; i += TL_BLOCK) { c_val[i] = -1.0; c_id[i] = 0x7fffffff; }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < n2; i += TL_BLOCK) {
          const int l = i ^ j;
          if (l > i) {
            const bool up = (i & k) == 0;
            // key_less on (-score, id): larger scores first, then smaller ids
            const bool sw2 = up ? key_less(-c_val[l], c_id[l], -c_val[i], c_id[i])
                                : key_less(-c_val[i], c_id[i], -c_val[l], c_id[l]);
            if (sw2) {
              const double tv = c_val[i]; c_val[i] = c_val[l]; c_val[l] = tv;
              const int ti = c_id[i]; c_id[i] = c_id[l]; c_id[l] = ti;
            }
          }
        }
        __syncthreads();
      }
    }
    const int nout = min(K, nt);
    for (int i = tid; i < nout; i += TL_BLOCK) {
      out_id[(size_t)q * K + i] = c_id[i];
      out_score[(size_t)q * K + i] = c_val[i];
    }
    if (tid == 0) out_n[q] = nout;
  }
}

// ---- sealing the tail into the base, on the device
// cnt[w + 1] += 1 for every tail posting of word w (cnt zeroed, n_words + 1 ints).
__global__ void k_bow_seal_count(const unsigned* fw, long long p0, long long p1, int n_words, int* cnt) {
  for (long long p = p0 + blockIdx.x * (long long)blockDim.x + threadIdx.x; p < p1;
       p += (long long)gridDim.x * blockDim.x) {
    const unsigned w = fw[p];
    if (w < (unsigned)n_words) atomicAdd(&cnt[w + 1], 1);
  }
}

// One block: new_ptr[i] = old_ptr[i] + (tail postings of words < i), i in [0, n_words].
__global__ __launch_bounds__(TL_BLOCK) void k_bow_seal_ptr(int n_words, const int* old_ptr, const int* cnt,
                                                           int* new_ptr) {
  __shared__ long long s_w[TL_WAVES];
  long long carry = 0;
  for (int t0 = 0; t0 <= n_words; t0 += TL_BLOCK) {
    const int i = t0 + (int)threadIdx.x;
    long long tot;
    const long long incl = block_scan_incl(i <= n_words ? cnt[i] : 0, s_w, &tot);
    if (i <= n_words) new_ptr[i] = old_ptr[i] + (int)(carry + incl);
    carry += tot;
  }
}

// Tail postings, a wave per tail entry, dropped into their word's segment of
// tmp in arrival order (cursor zeroed, n_words ints); k_bow_seal_place orders
// each segment by entry id. A word's segment starts at new_ptr[w] - old_ptr[w].
__global__ void k_bow_seal_fill(BowFwd f, int e0, int e1, int n_words, const int* old_ptr, const int* new_ptr,
                                int* cursor, int* tmp_e, double* tmp_v, int n_tmp) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwave = (gridDim.x * blockDim.x) >> 6;
  for (int e = e0 + wave; e < e1; e += nwave) {
    const long long p1 = f.fptr[e + 1];
    for (long long p = f.fptr[e] + lane; p < p1; p += 64) {
      const unsigned w = f.fw[p];
      if (w >= (unsigned)n_words) continue;
      const int slot = new_ptr[w] - old_ptr[w] + atomicAdd(&cursor[w], 1);
      if (slot >= 0 && slot < n_tmp) { tmp_e[slot] = e; tmp_v[slot] = f.fv[p]; }
    }
  }
}

// A wave per word: the old list moves to its shifted place, and the word's
// tail segment follows it ordered by entry id (rank by counting: an entry
// occurs once per word, so the ranks are a permutation). Lists stay ascending.
__global__ void k_bow_seal_place(int n_words, const int* old_ptr, const int* new_ptr, const int* old_ent,
                                 const double* old_wt, const int* tmp_e, const double* tmp_v, int* new_ent,
                                 double* new_wt) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwave = (gridDim.x * blockDim.x) >> 6;
  for (int w = wave; w < n_words; w += nwave) {
    const int o0 = old_ptr[w], o1 = old_ptr[w + 1], d0 = new_ptr[w], d1 = new_ptr[w + 1];
    const int n_old = o1 - o0;
    for (int k = lane; k < n_old; k += 64) {
      new_ent[d0 + k] = old_ent[o0 + k];
      new_wt[d0 + k] = old_wt[o0 + k];
    }
    const int t0 = d0 - o0, L = (d1 - d0) - n_old, dst = d0 + n_old;
    for (int i = lane; i < L; i += 64) {
      const int e = tmp_e[t0 + i];
      int rank = 0;
      for (int k = 0; k < L; ++k) rank += tmp_e[t0 + k] < e ? 1 : 0;
      new_ent[dst + rank] = e;
      new_wt[dst + rank] = tmp_v[t0 + i];
    }
  }
}

// cptr[w][c] = first posting of word w with entry >= c * sch (c < nsub), and
// the list's end at c == nsub: what kmx_bow_set_database builds on the host.
__global__ void k_bow_cptr(int n_words, int nsub, int sch, const int* ptr, const int* ent, int* cptr) {
  const size_t total = (size_t)n_words * (nsub + 1);
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
    const int w = (int)(t / (nsub + 1)), c = (int)(t - (size_t)w * (nsub + 1));
    int lo = ptr[w], up = ptr[w + 1];
    if (c < nsub) {
      const long long bound = (long long)c * sch;
      while (lo < up) {
        const int m = lo + ((up - lo) >> 1);
        if (ent[m] < bound) lo = m + 1;
        else up = m;
      }
    } else {
      lo = up;
    }
    cptr[t] = lo;
  }
}

// ---------------------------------------------------------------------------
// detectLoop decided on the device: k_bow_decide, one
// wave per query, takes the query results where the kernels above leave them
// through the nss gate, the alpha cut and computeIslands to the best island;
// k_bow_temporal, one wave, walks the call's queries in order through
// checkTemporalConstraint and compacts the LOOP_DETECTED pairs.
constexpr int DEC_PENDING = -1;  // k_bow_decide -> k_bow_temporal: an island awaits the constraint
constexpr int DEC_WAVE = 64;

struct BowDecide {
  int use_nss;
  double alpha, min_nss;
  int gap, min_matches;
};

// k_bow_decide. A workgroup is one wave, so its __syncthreads() orders the
// wave's LDS traffic and is no workgroup barrier. Every branch around one is
// taken by the whole wave (n, k and the status are the same in all lanes).
//   * the kept count k: the prefix with score >= alpha * nss (first failing
//     index, a min over the lanes);
//   * the k pairs in id order: each lane ranks its <= 4 elements by counting
//     the ids below them in LDS (ids are unique; the index breaks a tie so
//     that the ranks are a permutation whatever a caller passes);
//   * island heads by ballot: island j's first position lands in s_head[j];
//   * one lane per island walks its members in id order: the sum is one chain
//     from 0.0, as computeIslands adds it (a tree or shuffle sum would round
//     differently), the best member by strict > (lowest id on a tie);
//   * the best kept island: a lane's first maximum over its islands, then a
//     shuffle reduction on (island_score, island index), so the first island
//     in id order wins a tie, as std::max_element does.
// tin[q] = {status or DEC_PENDING, query id, island start, island end} and
// tmatch[q] = the match id are the temporal pass's coalesced input. Block 0 also copies the query kernels'
// error flag into the result header.
__global__ __launch_bounds__(DEC_WAVE) void k_bow_decide(int nq, int K, int mode, BowDecide p, const int* qids,
                                                         const int* n_in, const int* id_in, const double* sc_in,
                                                         const double* nss_in, const int* has_prev,
                                                         kmx_bow_detect_record* rec, int4* tin, int* tmatch,
                                                         const int* qerr, int* hdr) {
  __shared__ int u_id[MAX_RESULTS];
  __shared__ double u_sc[MAX_RESULTS];
  __shared__ int s_id[MAX_RESULTS];
  __shared__ double s_sc[MAX_RESULTS];
  __shared__ int s_head[MAX_RESULTS];
  const int lane = threadIdx.x;
  if (blockIdx.x == 0 && lane == 0) {  // the header: no candidates yet (k_bow_temporal counts them), the error flag
    hdr[0] = 0;
    hdr[1] = qerr ? qerr[0] : 0;
  }
  for (int q = blockIdx.x; q < nq; q += gridDim.x) {
    const int qid = qids ? qids[q] : q;
    const int n = max(0, min(n_in[q], K));
    const bool hp = has_prev ? has_prev[q] != 0 : true;
    const double nss = (p.use_nss && nss_in) ? nss_in[q] : 1.0;
    const double nss_rep = hp ? nss : 0.0;
    auto emit = [&](int status, int match, int kept, int i_start, int i_end, double score, double i_score) {
      if (lane == 0) {
        kmx_bow_detect_record r;
        r.query_id = qid;
        r.status = status;
        r.match_id = match;
        r.n_kept = kept;
        r.island_start = i_start;
        r.island_end = i_end;
        r.score = score;
        r.nss = nss_rep;
        r.island_score = i_score;
        rec[q] = r;
        tin[q] = make_int4(status, qid, i_start, i_end);
        tmatch[q] = match;
      }
    };
    if (n == 0) {  // before the nss test, as on the host
      emit(KMX_BOW_NO_MATCHES, -1, 0, -1, -1, 0.0, 0.0);
      continue;
    }
    const bool low_nss = mode == KMX_BOW_MODE_INTER ? !(hp && nss >= p.min_nss) : (!hp || nss < p.min_nss);
    if (p.use_nss && low_nss) {
      emit(KMX_BOW_LOW_NSS_FACTOR, -1, 0, -1, -1, 0.0, 0.0);
      continue;
    }
    const double thr = p.alpha * nss;  // one multiplication
    const size_t row = (size_t)q * K;
    if (mode == KMX_BOW_MODE_INTER) {  // the top result, no islands
      const int id0 = id_in[row];
      const double sc0 = sc_in[row];
      if (sc0 >= thr) emit(KMX_BOW_LOOP_DETECTED, id0, 1, id0, id0, sc0, sc0);
      else emit(KMX_BOW_LOW_SCORE, -1, 0, -1, -1, 0.0, 0.0);
      continue;
    }
    __syncthreads();  // the previous query's LDS reads are done
    int fail = n;     // first index whose score fails the cut: a prefix, not a count
    for (int i = lane; i < n; i += DEC_WAVE) {
      const int id = id_in[row + i];
      const double s = sc_in[row + i];
      u_id[i] = id;
      u_sc[i] = s;
      if (!(s >= thr)) fail = min(fail, i);
    }
#pragma unroll
    for (int off = DEC_WAVE / 2; off > 0; off >>= 1) fail = min(fail, __shfl_xor(fail, off, DEC_WAVE));
    const int k = fail;
    if (k == 0) {
      emit(KMX_BOW_LOW_SCORE, -1, 0, -1, -1, 0.0, 0.0);
      continue;
    }
    __syncthreads();
    if (k == 1) {  // computeIslands keeps a single result whatever min_matches_per_island says
      emit(DEC_PENDING, u_id[0], 1, u_id[0], u_id[0], u_sc[0], u_sc[0]);
      continue;
    }
    for (int i = lane; i < k; i += DEC_WAVE) {
      const int id = u_id[i];
      int r = 0;
      for (int j = 0; j < k; ++j) {
        const int o = u_id[j];
        r += (o < id || (o == id && j < i)) ? 1 : 0;
      }
      s_id[r] = id;
      s_sc[r] = u_sc[i];
    }
    __syncthreads();
    int ni = 0;
    for (int i0 = 0; i0 < k; i0 += DEC_WAVE) {
      const int i = i0 + lane;
      const bool head = i < k && (i == 0 || (long long)s_id[i] - s_id[i - 1] >= p.gap);
      const unsigned long long m = __ballot(head);
      if (head) s_head[ni + __popcll(m & ((1ull << lane) - 1ull))] = i;
      ni += __popcll(m);
    }
    __syncthreads();
    bool have = false;
    double b_sum = 0.0, l_best_sc = 0.0;
    int b_idx = 0x7fffffff, l_start = -1, l_end = -1, l_best = -1;
    for (int j = lane; j < ni; j += DEC_WAVE) {
      const int i0 = s_head[j], i1 = (j + 1 < ni) ? s_head[j + 1] : k;
      const int st = s_id[i0], en = s_id[i1 - 1];
      double sum = 0.0, bs = s_sc[i0];
      int be = st;
      for (int i = i0; i < i1; ++i) {  // ordered: left to right in id order, from 0.0
        const double sc = s_sc[i];
        sum += sc;
        if (i > i0 && sc > bs) {
          bs = sc;
          be = s_id[i];
        }
      }
      // the id span, not the member count
      if ((long long)en - st + 1 >= p.min_matches && (!have || sum > b_sum)) {
        have = true;
        b_sum = sum;
        b_idx = j;
        l_start = st;
        l_end = en;
        l_best = be;
        l_best_sc = bs;
      }
    }
#pragma unroll
    for (int off = DEC_WAVE / 2; off > 0; off >>= 1) {
      const int o_have = __shfl_xor(have ? 1 : 0, off, DEC_WAVE);
      const double o_sum = __shfl_xor(b_sum, off, DEC_WAVE);
      const int o_idx = __shfl_xor(b_idx, off, DEC_WAVE);
      if (o_have && (!have || o_sum > b_sum || (o_sum == b_sum && o_idx < b_idx))) {
        have = true;
        b_sum = o_sum;
        b_idx = o_idx;
      }
    }
    if (!have) {
      emit(KMX_BOW_NO_GROUPS, -1, k, -1, -1, 0.0, 0.0);
      continue;
    }
    const int owner = b_idx & (DEC_WAVE - 1);  // the lane whose own best island won
    emit(DEC_PENDING, __shfl(l_best, owner, DEC_WAVE), k, __shfl(l_start, owner, DEC_WAVE),
         __shfl(l_end, owner, DEC_WAVE), __shfl(l_best_sc, owner, DEC_WAVE), b_sum);
  }
}

// k_bow_temporal: checkTemporalConstraint over the call's queries in order,
// one wave. The state {entries, latest query, latest island start, end} is a
// recurrence, but its inputs are not: a step takes TMP_DEPTH * 64 queries, each
// lane loading TMP_DEPTH tin (16 bytes per lane, contiguous per load) and match
// ids, all independent, and the next step's loads are issued before the
// current ones are stepped through (one group of 64 per step in flight left
// the wave waiting a memory latency per 64 queries). The state is stepped in
// wave-uniform registers over the pending lanes only (ballot, then readlane by
// the set bit). A query settled by k_bow_decide leaves the state alone. Every
// LOOP_DETECTED appends (query id, match id) to cand in query order; hdr[0] =
// their count. All stores are per-lane vector stores.
constexpr int TMP_DEPTH = 4;

__global__ __launch_bounds__(DEC_WAVE) void k_bow_temporal(int nq, int max_between_queries, int max_between_islands,
                                                           int min_temporal, const int4* tin, const int* tmatch,
                                                           kmx_bow_detect_record* rec, int* state, int* cand,
                                                           int* hdr) {
  const int lane = threadIdx.x;
  // A query kernel raised its flag (k_bow_decide copied it to hdr[1]): the rows
  // are an incomplete selection and the call returns KMX_EUNSUP, so the state
  // stays what it was. hdr[0] is 0 from k_bow_decide. The whole wave leaves.
  if (hdr[1] != 0) return;
  int te = __builtin_amdgcn_readfirstlane(state[0]);
  int lq = __builtin_amdgcn_readfirstlane(state[1]);
  int a1 = __builtin_amdgcn_readfirstlane(state[2]);
  int a2 = __builtin_amdgcn_readfirstlane(state[3]);
  int nc = 0;
  const int4 none = make_int4(KMX_BOW_NO_MATCHES, 0, 0, 0);
  int4 nxt[TMP_DEPTH];
  int nxt_m[TMP_DEPTH];
  auto load = [&](int q0) {
#pragma unroll
    for (int d = 0; d < TMP_DEPTH; ++d) {
      const int q = q0 + d * DEC_WAVE + lane;
      nxt[d] = q < nq ? tin[q] : none;
      nxt_m[d] = q < nq ? tmatch[q] : -1;
    }
  };
  load(0);
  for (int q0 = 0; q0 < nq; q0 += TMP_DEPTH * DEC_WAVE) {
    int4 cur[TMP_DEPTH];
    int cur_m[TMP_DEPTH];
#pragma unroll
    for (int d = 0; d < TMP_DEPTH; ++d) {
      cur[d] = nxt[d];
      cur_m[d] = nxt_m[d];
    }
    load(q0 + TMP_DEPTH * DEC_WAVE);
#pragma unroll
    for (int d = 0; d < TMP_DEPTH; ++d) {
      const int4 t = cur[d];
      const int q = q0 + d * DEC_WAVE + lane;
      const bool pend = q < nq && t.x == DEC_PENDING;
      int st = t.x;
      unsigned long long m = __ballot(pend);
      while (m) {
        const int l = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int qid = __builtin_amdgcn_readlane(t.y, l);
        const int b1 = __builtin_amdgcn_readlane(t.z, l), b2 = __builtin_amdgcn_readlane(t.w, l);
        // checkTemporalConstraint, as selects on scalars (no branch per query)
        const bool fresh = (te == 0) | (qid - lq > max_between_queries);
        const bool overlap = ((b1 <= a1) & (a1 <= b2)) | ((a1 <= b1) & (b1 <= a2)) | ((b1 <= a2) & (a2 <= b2)) |
                             ((a1 <= b2) & (b2 <= a2));
        const bool near = max(a1 - b2, b1 - a2) <= max_between_islands;
        te = (!fresh & (overlap | near)) ? te + 1 : 1;
        lq = qid;
        a1 = b1;
        a2 = b2;
        if (lane == l) st = te > min_temporal ? KMX_BOW_LOOP_DETECTED : KMX_BOW_FAILED_TEMPORAL_CONSTRAINT;
      }
      if (pend) rec[q].status = st;
      const bool loop = pend && st == KMX_BOW_LOOP_DETECTED;
      const unsigned long long lm = __ballot(loop);
      if (loop) {
        const int pos = nc + __popcll(lm & ((1ull << lane) - 1ull));
        cand[2 * pos] = t.y;
        cand[2 * pos + 1] = cur_m[d];
      }
      nc += __popcll(lm);
    }
  }
  if (lane < 4) state[lane] = lane == 0 ? te : lane == 1 ? lq : lane == 2 ? a1 : a2;
  if (lane == 0) hdr[0] = nc;
}

// Before the query of kmx_bow_detect_entries, one thread per query: whether a
// previous keyframe exists (entry id - 1 of src; inter mode: and is a
// non-empty vector), the nss factor against it (k_bow_entry_score's sum; 0
// without one or without use_nss), and in intra mode max_id = max(id - window, 0).
// ids_in == nullptr: the queries are the consecutive entries first, first + 1,
// ... (a keyframe stream), written to ids_out here instead of being uploaded.
__global__ void k_bow_detect_prep(int nq, int mode, int window, int use_nss, BowFwd src, int first,
                                  const int* ids_in, int* ids_out, int* has_prev, int* max_id, double* nss) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nq) return;
  const int id = ids_in ? ids_in[t] : first + t;
  if (!ids_in) ids_out[t] = id;
  bool hp = id > 0;
  if (mode == KMX_BOW_MODE_INTER) {
    if (hp) hp = src.fptr[id] - src.fptr[id - 1] > 0;
  } else {
    max_id[t] = max(id - window, 0);
  }
  has_prev[t] = hp ? 1 : 0;
  nss[t] = use_nss ? entry_score(src, id, id - 1) : 0.0;
}

// The handle's device buffers in the six sets that live and die together. A
// set is replaced as a whole (h->qry = BowQuerySet()) and a grown one is built
// aside and moved in, so no buffer is named again to be freed.
struct BowDbSet {  // the inverted file over [0, n_sealed) and the base query's scratch
  kmx::DevBuf<int> ptr, ent;  // ent / wt hold ent.cap() postings
  kmx::DevBuf<double> wt;
  int n_wg = 0;
  kmx::DevBuf<double> acc;  // HBM-accumulator query: acc.cap() per-workgroup slots, with touched
  kmx::DevBuf<int> touched;
  kmx::DevBuf<int> cptr;  // LDS-accumulator query (k_bow_query_lds): per-word chunk split points
};
struct BowQuerySet {  // query scratch: qptr.cap() queries (+ 1), qw.cap() words, id.cap() results
  kmx::DevBuf<long long> qptr;
  kmx::DevBuf<unsigned> qw;
  kmx::DevBuf<double> qv;
  kmx::DevBuf<int> maxid, n, id;
  kmx::DevBuf<double> score;
};
struct BowPairSet {  // pair-score scratch: aptr.cap() pairs (+ 1), aw.cap() words a side
  kmx::DevBuf<long long> aptr, bptr;
  kmx::DevBuf<unsigned> aw, bw;
  kmx::DevBuf<double> av, bv, out;
};
struct BowFwdSet {  // the forward store (every entry's vector) and the seal's grow-only scratch
  kmx::DevBuf<long long> fptr;  // [fe_cap() + 1]
  kmx::DevBuf<unsigned> fw;     // [fw.cap()] postings, with fv
  kmx::DevBuf<double> fv;
  std::vector<int64_t> h_fptr{0};  // host mirror of fptr (8 bytes per entry; no words or weights)
  kmx::DevBuf<int> cnt, tmp_e;
  kmx::DevBuf<double> tmp_v;  // allocated after tmp_e: its capacity is the pair's
  size_t fe_cap() const { return fptr.cap() ? fptr.cap() - 1 : 0; }
};
struct BowIdSet {  // entry-id scratch: eid [2 cap()], eout [cap()]
  kmx::DevBuf<int> eid;
  kmx::DevBuf<double> eout;
  size_t cap() const { return eout.cap(); }
};
struct BowDetSet {  // detection scratch (grow-only) and the result block with its pinned host mirror
  kmx::DevBuf<int> hasprev;  // [cap()] has_prev, then [cap()] k_bow_decide's match ids
  kmx::DevBuf<int4> tin;
  kmx::DevBuf<char> dout;
  kmx::PinnedBuf<char> h_dout;
  int nq = -1;  // the enqueued call's query count (kmx_bow_detect_fetch)
  size_t cap() const { return tin.cap(); }
};

}  // namespace

struct kmx_bow : kmx::StreamCore {
  int n_words = 0, n_entries = 0;
  BowDbSet db;
  kmx::DevBuf<int> d_err;
  bool lds = true;
  int ch = 0, nch = 0;
  BowQuerySet qry;
  BowPairSet pair;
  // streaming database: entries [0, n_sealed) are in the inverted file,
  // [n_sealed, n_entries) only in the forward store
  int n_sealed = 0;
  int tail_cap = TAIL_DEFAULT, tail_cap_set = TAIL_DEFAULT;
  BowFwdSet fwd;
  kmx::Event ev;  // orders this handle after another handle's stream
  BowIdSet ids;
  // detection on the device: the temporal constraint's state (4 ints, then 4
  // of scratch for a pass that leaves the state alone), and the result block
  // [records nq][n_cand, error][cand 2 * nq], mirrored in pinned host memory
  // so that one copy brings a call's results back
  kmx::DevBuf<int> d_tstate;
  BowDetSet det;
  bool timing = false;
  kmx::Event tev[4];  // created by the first timed detection
};

namespace {
// Room in the forward store for ne entries and np postings: capacity
// doubling, one device-to-device copy of what is held per doubling.
int bow_fwd_reserve(kmx_bow* h, size_t ne, size_t np) {
  BowFwdSet& F = h->fwd;
  const bool grow_e = !F.fptr.get() || ne > F.fe_cap(), grow_p = !F.fw.get() || np > F.fw.cap();
  if (!grow_e && !grow_p) return 0;
  const size_t held_e = (size_t)h->n_entries + 1, held_p = (size_t)F.h_fptr.back();
  kmx::DevBuf<long long> nf;
  kmx::DevBuf<unsigned> nw;
  kmx::DevBuf<double> nv;
  int rc = 0;
  const size_t ec = std::max<size_t>({ne, 2 * F.fe_cap(), 1024}), pc = std::max<size_t>({np, 2 * F.fw.cap(), 65536});
  if (grow_e) rc = nf.alloc(ec + 1);
  if (!rc && grow_p) rc = nw.alloc(pc);
  if (!rc && grow_p) rc = nv.alloc(pc);
  if (rc) return rc;
  hipError_t e = hipSuccess;
  if (grow_e)
    e = F.fptr.get()
            ? hipMemcpyAsync(nf.get(), F.fptr.get(), sizeof(long long) * held_e, hipMemcpyDeviceToDevice, h->stream)
            : hipMemsetAsync(nf.get(), 0, sizeof(long long), h->stream);
  if (grow_p && F.fw.get() && held_p) {
    if (e == hipSuccess)
      e = hipMemcpyAsync(nw.get(), F.fw.get(), sizeof(unsigned) * held_p, hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(nv.get(), F.fv.get(), sizeof(double) * held_p, hipMemcpyDeviceToDevice, h->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // queries in flight read the old store
  if (e != hipSuccess) return kmx::fail(KMX_EHIP, std::string("forward store: ") + hipGetErrorString(e));
  if (grow_e) F.fptr = std::move(nf);
  if (grow_p) {
    F.fw = std::move(nw);
    F.fv = std::move(nv);
  }
  return 0;
}

// Seal the tail: the inverted file over [0, n_entries), built on the device
// from the old one and the tail's vectors in the forward store. Afterwards
// d_ptr / d_ent / d_wt / d_cptr are what kmx_bow_set_database builds from the
// same entries. No posting crosses to the host (its totals are in h_fptr).
int bow_seal(kmx_bow* h) {
  const int n = h->n_entries, e0 = h->n_sealed, nw = h->n_words;
  if (n == e0) return KMX_OK;
  KMX_HIP(hipSetDevice(h->device));
  const long long p0 = h->fwd.h_fptr[e0], p1 = h->fwd.h_fptr[n];
  const size_t n_tail = (size_t)(p1 - p0), n_new = (size_t)p1;
  int rc = 0;
  if (!h->fwd.cnt.get() && (rc = h->fwd.cnt.alloc((size_t)nw + 1))) return rc;
  if (n_tail > h->fwd.tmp_v.cap() || !h->fwd.tmp_v.get()) {
    h->fwd.tmp_e.reset();
    h->fwd.tmp_v.reset();
    const size_t cap = std::max<size_t>(n_tail, 65536);
    if ((rc = h->fwd.tmp_e.alloc(cap)) || (rc = h->fwd.tmp_v.alloc(cap))) return rc;
  }
  const int nch = std::max(1, (n + h->ch - 1) / h->ch), nsub = nch * LW_WAVES, sch = h->ch / LW_WAVES;
  const size_t cneed = h->lds ? (size_t)nw * (nsub + 1) : 0;
  const size_t sneed = h->lds ? 1 : (size_t)h->db.n_wg * std::max(n, 1);
  // the new file is built aside: an early return frees it and the handle keeps the old one
  BowDbSet nb;
  if ((rc = nb.ptr.alloc((size_t)nw + 1)) || (rc = nb.ent.alloc(n_new)) || (rc = nb.wt.alloc(n_new)) ||
      (cneed > h->db.cptr.cap() && (rc = nb.cptr.alloc(cneed))) ||
      (sneed > h->db.acc.cap() && ((rc = nb.acc.alloc(sneed)) || (rc = nb.touched.alloc(sneed)))))
    return rc;
  int *new_ptr = nb.ptr.get(), *new_ent = nb.ent.get(), *new_cptr = nb.cptr.get();
  double *new_wt = nb.wt.get(), *new_acc = nb.acc.get();
  BowFwd f{h->fwd.fptr.get(), h->fwd.fw.get(), h->fwd.fv.get()};
  hipError_t e = hipMemsetAsync(h->fwd.cnt.get(), 0, sizeof(int) * ((size_t)nw + 1), h->stream);
  if (e == hipSuccess && n_tail) {
    const int grid = (int)std::min<size_t>((n_tail + 255) / 256, 2048);
    hipLaunchKernelGGL(k_bow_seal_count, dim3(grid), dim3(256), 0, h->stream, (const unsigned*)h->fwd.fw.get(), p0, p1,
                       nw, h->fwd.cnt.get());
  }
  if (e == hipSuccess)
    hipLaunchKernelGGL(k_bow_seal_ptr, dim3(1), dim3(TL_BLOCK), 0, h->stream, nw, (const int*)h->db.ptr.get(),
                       (const int*)h->fwd.cnt.get(), new_ptr);
  if (e == hipSuccess) e = hipMemsetAsync(h->fwd.cnt.get(), 0, sizeof(int) * ((size_t)nw + 1), h->stream);
  if (e == hipSuccess && n_tail)
    hipLaunchKernelGGL(k_bow_seal_fill, dim3(std::min((n - e0 + 3) / 4, 2048)), dim3(256), 0, h->stream, f, e0, n, nw,
                       (const int*)h->db.ptr.get(), (const int*)new_ptr, h->fwd.cnt.get(), h->fwd.tmp_e.get(),
                       h->fwd.tmp_v.get(), (int)n_tail);
  if (e == hipSuccess)
    hipLaunchKernelGGL(k_bow_seal_place, dim3(std::min((nw + 3) / 4, 4096)), dim3(256), 0, h->stream, nw,
                       (const int*)h->db.ptr.get(), (const int*)new_ptr, (const int*)h->db.ent.get(),
                       (const double*)h->db.wt.get(), (const int*)h->fwd.tmp_e.get(), (const double*)h->fwd.tmp_v.get(),
                       new_ent, new_wt);
  if (e == hipSuccess && h->lds) {  // in place when the table keeps its shape: only earlier queries read it
    const int grid = (int)std::min<size_t>((cneed + 255) / 256, 4096);
    hipLaunchKernelGGL(k_bow_cptr, dim3(grid), dim3(256), 0, h->stream, nw, nsub, sch, (const int*)new_ptr,
                       (const int*)new_ent, new_cptr ? new_cptr : h->db.cptr.get());
  }
  if (e == hipSuccess && new_acc) e = hipMemsetAsync(new_acc, 0, sizeof(double) * sneed, h->stream);
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // the old arrays are read until here
  if (e != hipSuccess) return kmx::fail(KMX_EHIP, std::string("kmx_bow_seal: ") + hipGetErrorString(e));
  h->db.ptr = std::move(nb.ptr);
  h->db.ent = std::move(nb.ent);
  h->db.wt = std::move(nb.wt);
  if (new_cptr) h->db.cptr = std::move(nb.cptr);
  if (new_acc) {
    h->db.acc = std::move(nb.acc);
    h->db.touched = std::move(nb.touched);
  }
  h->nch = nch;
  h->n_sealed = n;
  return KMX_OK;
}
}  // namespace

extern "C" int kmx_bow_create(int device, kmx_bow** out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(out, KMX_EINVAL, "null argument");
  std::unique_ptr<kmx_bow> h(new kmx_bow());
  int rc;
  if ((rc = h->open(device)) || (rc = h->d_err.alloc(2)) || (rc = h->d_tstate.alloc(8))) return rc;
  // these two have always been reported with the allocations' code
  if (hipMemset(h->d_tstate.get(), 0, 8 * sizeof(int)) != hipSuccess || h->ev.create(hipEventDisableTiming))
    return kmx::fail(KMX_ENOMEM, "kmx_bow_create: hipMemset / hipEventCreate failed");
  *out = h.release();
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_bow_destroy(kmx_bow* h) {
  return kmx::destroy(h);
}

// Unlike the other handles', a borrowed stream is left alone: only a stream of the handle's own is synchronised.
extern "C" int kmx_bow_set_stream(kmx_bow* h, void* s) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  return h->adopt(s, false);
}

extern "C" int kmx_bow_set_database(kmx_bow* h, int32_t n_words, int32_t n_entries, const int64_t* vptr,
                                    const uint32_t* words, const double* weights) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && vptr && n_words > 0 && n_entries >= 0, KMX_EINVAL, "bad argument");
  {  // before any device call: a refused database leaves the handle as it was
    std::string err;
    if (int rc = kmx::bow_check_csr(n_words, 0, 0, n_entries, vptr, words, weights, &err)) return kmx::fail(rc, err);
  }
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  const int64_t nnz = vptr[n_entries];
  KMX_CHECK(nnz >= 0 && nnz < INT32_MAX, KMX_EINVAL, "database too large (postings must fit int32)");
  std::vector<int> ptr((size_t)n_words + 1, 0);
  for (int64_t k = vptr[0]; k < vptr[n_entries]; ++k) ptr[words[k] + 1]++;  // words checked above
  for (int w = 0; w < n_words; ++w) ptr[w + 1] += ptr[w];
  std::vector<int> fill(ptr.begin(), ptr.end() - 1), ent(std::max<int64_t>(nnz, 1));
  std::vector<double> wt(std::max<int64_t>(nnz, 1));
  for (int e = 0; e < n_entries; ++e)  // entries added in id order: posting lists ascending
    for (int64_t k = vptr[e]; k < vptr[e + 1]; ++k) {
      const int p = fill[words[k]]++;
      ent[p] = e;
      wt[p] = weights[k];
    }
  h->db = BowDbSet();
  h->n_words = n_words;
  h->n_entries = n_entries;
  // KMX_BOW_LDS=0 selects the HBM-accumulator kernel; KMX_BOW_CHUNK sets the
  // entries per LDS chunk (tests use small chunks to cover the merge)
  h->lds = true;
  if (const char* v = std::getenv("KMX_BOW_LDS")) h->lds = std::atoi(v) != 0;
  h->ch = LCH;
  if (const char* v = std::getenv("KMX_BOW_CHUNK")) h->ch = std::max(1, std::min(LCH, std::atoi(v)));
  h->ch = (h->ch + LW_WAVES - 1) / LW_WAVES * LW_WAVES;  // whole sub-ranges, one per wave
  h->nch = std::max(1, (n_entries + h->ch - 1) / h->ch);
  std::vector<int> cptr;
  if (h->lds) {  // first posting of each wave sub-range in every word's (ascending) list
    const int nsub = h->nch * LW_WAVES, sch = h->ch / LW_WAVES;
    cptr.assign((size_t)n_words * (nsub + 1), 0);
    for (int w = 0; w < n_words; ++w) {
      int p = ptr[w];
      for (int c = 0; c <= nsub; ++c) {
        const long long bound = (long long)c * sch;
        while (p < ptr[w + 1] && ent[p] < bound) ++p;
        cptr[(size_t)w * (nsub + 1) + c] = (c == nsub) ? ptr[w + 1] : p;
      }
    }
  }
  // persistent query workgroups: the HBM kernel gives each an acc / touched
  // scratch of n_entries; the LDS kernel runs one workgroup per CU
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device);
  h->db.n_wg = h->lds ? std::max(1, cus) : std::max(1, cus * 4);
  const size_t scratch = h->lds ? 1 : (size_t)h->db.n_wg * std::max(n_entries, 1);
  int rc;
  if ((rc = h->db.ptr.alloc(ptr.size())) || (rc = h->db.ent.alloc(ent.size())) || (rc = h->db.wt.alloc(wt.size())) ||
      (rc = h->db.acc.alloc(scratch)) || (rc = h->db.touched.alloc(scratch)) ||
      (h->lds && (rc = h->db.cptr.alloc(cptr.size())))) {
    h->db = BowDbSet();
    return rc;
  }
  if (h->lds) KMX_HIP(hipMemcpy(h->db.cptr.get(), cptr.data(), sizeof(int) * cptr.size(), hipMemcpyHostToDevice));
  KMX_HIP(hipMemcpy(h->db.ptr.get(), ptr.data(), sizeof(int) * ptr.size(), hipMemcpyHostToDevice));
  KMX_HIP(hipMemcpy(h->db.ent.get(), ent.data(), sizeof(int) * ent.size(), hipMemcpyHostToDevice));
  KMX_HIP(hipMemcpy(h->db.wt.get(), wt.data(), sizeof(double) * wt.size(), hipMemcpyHostToDevice));
  KMX_HIP(hipMemset(h->db.acc.get(), 0, sizeof(double) * scratch));
  // the forward store: the same vectors entry-major (one more upload of the
  // CSR), all of them sealed. KMX_BOW_TAIL overrides kmx_bow_set_tail_cap.
  h->n_entries = 0;  // until the forward store holds them
  h->n_sealed = 0;
  h->fwd = BowFwdSet();
  h->tail_cap = h->tail_cap_set;
  if (const char* v = std::getenv("KMX_BOW_TAIL")) h->tail_cap = std::max(0, std::min(TAIL_MAX, std::atoi(v)));
  const int64_t held = vptr[n_entries] - vptr[0];
  if (int rc2 = bow_fwd_reserve(h, (size_t)n_entries, (size_t)held)) {
    h->db = BowDbSet();
    return rc2;
  }
  std::vector<int64_t> fp((size_t)n_entries + 1);
  for (int e = 0; e <= n_entries; ++e) fp[e] = vptr[e] - vptr[0];
  KMX_HIP(hipMemcpy(h->fwd.fptr.get(), fp.data(), sizeof(long long) * fp.size(), hipMemcpyHostToDevice));
  if (held) {
    KMX_HIP(hipMemcpy(h->fwd.fw.get(), words + vptr[0], sizeof(unsigned) * (size_t)held, hipMemcpyHostToDevice));
    KMX_HIP(hipMemcpy(h->fwd.fv.get(), weights + vptr[0], sizeof(double) * (size_t)held, hipMemcpyHostToDevice));
  }
  h->fwd.h_fptr.swap(fp);
  h->n_entries = h->n_sealed = n_entries;
  KMX_HIP(hipMemsetAsync(h->d_tstate.get(), 0, 8 * sizeof(int), h->stream));  // a new stream of keyframes
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_bow_reset(kmx_bow* h, int32_t n_words) {
  const int64_t zero = 0;
  return kmx_bow_set_database(h, n_words, 0, &zero, nullptr, nullptr);
}

extern "C" int kmx_bow_set_tail_cap(kmx_bow* h, int32_t cap) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(cap >= 0 && cap <= TAIL_MAX, KMX_EINVAL, "tail_cap must be in [0, 1024]");
  h->tail_cap_set = cap;
  if (!std::getenv("KMX_BOW_TAIL")) h->tail_cap = cap;
  if (h->db.ptr.get() && h->n_entries - h->n_sealed > h->tail_cap) return bow_seal(h);
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_bow_seal(kmx_bow* h) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && h->db.ptr.get(), KMX_ESTATE, "kmx_bow_set_database or kmx_bow_reset first");
  return bow_seal(h);
  KMX_GUARD_END
}

extern "C" int kmx_bow_info(kmx_bow* h, int32_t* n_words, int32_t* n_entries, int32_t* n_sealed, int32_t* tail_cap,
                            int64_t* n_postings, int64_t* device_bytes) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  if (n_words) *n_words = h->n_words;
  if (n_entries) *n_entries = h->n_entries;
  if (n_sealed) *n_sealed = h->n_sealed;
  if (tail_cap) *tail_cap = h->tail_cap;
  if (n_postings) *n_postings = h->fwd.h_fptr.back();
  if (device_bytes) {
    size_t b = 0;
    if (h->db.ptr.get())
      b = sizeof(int) * ((size_t)h->n_words + 1) + (sizeof(int) + sizeof(double)) * h->db.ent.cap() +
          sizeof(int) * h->db.cptr.cap() + (sizeof(int) + sizeof(double)) * h->db.acc.cap() +
          sizeof(long long) * (h->fwd.fe_cap() + 1) + (sizeof(unsigned) + sizeof(double)) * h->fwd.fw.cap();
    *device_bytes = (int64_t)b;
  }
  return KMX_OK;
}

extern "C" int kmx_bow_add_entries(kmx_bow* h, int32_t n, const int64_t* vptr, const uint32_t* words,
                                   const double* weights, int32_t* first_id_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(h->db.ptr.get(), KMX_ESTATE, "kmx_bow_set_database or kmx_bow_reset first");
  std::string err;
  if (int rc = kmx::bow_check_csr(h->n_words, h->n_entries, h->fwd.h_fptr.back(), n, vptr, words, weights, &err))
    return kmx::fail(rc, err);
  if (first_id_out) *first_id_out = h->n_entries;
  if (n == 0) return KMX_OK;
  const int64_t total = vptr[n] - vptr[0], base = h->fwd.h_fptr.back();
  KMX_HIP(hipSetDevice(h->device));
  if (int rc = bow_fwd_reserve(h, (size_t)h->n_entries + n, (size_t)(base + total))) return rc;
  const size_t m0 = h->fwd.h_fptr.size();  // n_entries + 1
  for (int e = 1; e <= n; ++e) h->fwd.h_fptr.push_back(base + (vptr[e] - vptr[0]));
  hipError_t e1 = hipMemcpyAsync(h->fwd.fptr.get() + m0, h->fwd.h_fptr.data() + m0, sizeof(long long) * n,
                                 hipMemcpyHostToDevice, h->stream);
  if (e1 == hipSuccess && total)
    e1 = hipMemcpyAsync(h->fwd.fw.get() + base, words + vptr[0], sizeof(unsigned) * total, hipMemcpyHostToDevice,
                        h->stream);
  if (e1 == hipSuccess && total)
    e1 = hipMemcpyAsync(h->fwd.fv.get() + base, weights + vptr[0], sizeof(double) * total, hipMemcpyHostToDevice,
                        h->stream);
  if (e1 == hipSuccess) e1 = hipStreamSynchronize(h->stream);  // the caller's arrays are free again
  if (e1 != hipSuccess) {
    h->fwd.h_fptr.resize(m0);  // the entries were not added
    return kmx::fail(KMX_EHIP, std::string("kmx_bow_add_entries: ") + hipGetErrorString(e1));
  }
  h->n_entries += n;
  if (h->n_entries - h->n_sealed > h->tail_cap) return bow_seal(h);
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_bow_add_from_voc(kmx_bow* h, kmx_voc* voc, int32_t* first_id_out, int32_t* n_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && voc, KMX_EINVAL, "null handle");
  KMX_CHECK(h->db.ptr.get(), KMX_ESTATE, "kmx_bow_set_database or kmx_bow_reset first");
  kmx::VocBatchView vb;
  if (int rc = kmx::voc_batch_view(voc, &vb)) return rc;
  KMX_CHECK(vb.device == h->device, KMX_EINVAL, "the vocabulary is on another device");
  KMX_CHECK(vb.n_words == h->n_words, KMX_EINVAL, "the vocabulary's word count differs from the database's");
  KMX_CHECK(vb.n_frames > 0 && vb.stride > 0 && vb.nnz && vb.words && vb.weights, KMX_ESTATE,
            "the vocabulary holds no transformed batch");
  const int n = vb.n_frames;
  const int64_t base = h->fwd.h_fptr.back(), most = (int64_t)n * vb.stride;  // a frame has <= stride words
  KMX_CHECK(n < INT32_MAX - h->n_entries, KMX_EINVAL, "database too large (entries must fit int32)");
  KMX_CHECK(most < (int64_t)INT32_MAX - base, KMX_EINVAL, "database too large (postings must fit int32)");
  KMX_HIP(hipSetDevice(h->device));
  if (int rc = bow_fwd_reserve(h, (size_t)h->n_entries + n, (size_t)(base + most))) return rc;
  // after the transform, which runs on the vocabulary's stream
  KMX_HIP(hipEventRecord(h->ev, vb.stream));
  KMX_HIP(hipStreamWaitEvent(h->stream, h->ev, 0));
  long long* fnew = h->fwd.fptr.get() + h->n_entries;
  // no weight check here (bow_check_csr's "finite and > 0"): k_voc_reduce keeps
  // only leaves with a positive weight and divides by their positive sum
  hipLaunchKernelGGL(k_bow_scan_len<0>, dim3(1), dim3(TL_BLOCK), 0, h->stream, n, vb.nnz,
                     (const long long*)nullptr, fnew);
  KMX_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_bow_voc_compact, dim3(n), dim3(256), 0, h->stream, vb.nnz, (const unsigned*)vb.words,
                     vb.weights, vb.stride, (const long long*)fnew, h->fwd.fw.get(), h->fwd.fv.get());
  KMX_HIP(hipGetLastError());
  // the new entries' offsets come back to the host mirror: 8 bytes per entry, no words or weights
  const size_t m0 = h->fwd.h_fptr.size();
  h->fwd.h_fptr.resize(m0 + n);
  hipError_t e1 = hipMemcpyAsync(h->fwd.h_fptr.data() + m0, fnew + 1, sizeof(long long) * n, hipMemcpyDeviceToHost,
                                 h->stream);
  if (e1 == hipSuccess) e1 = hipStreamSynchronize(h->stream);
  if (e1 != hipSuccess) {
    h->fwd.h_fptr.resize(m0);
    return kmx::fail(KMX_EHIP, std::string("kmx_bow_add_from_voc: ") + hipGetErrorString(e1));
  }
  if (first_id_out) *first_id_out = h->n_entries;
  if (n_out) *n_out = n;
  h->n_entries += n;
  if (h->n_entries - h->n_sealed > h->tail_cap) return bow_seal(h);
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_bow_get_entries(kmx_bow* h, int32_t first, int32_t n, int64_t* vptr_out, uint32_t* words_out,
                                   double* weights_out, int64_t cap) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && vptr_out, KMX_EINVAL, "null argument");
  KMX_CHECK(h->db.ptr.get(), KMX_ESTATE, "kmx_bow_set_database or kmx_bow_reset first");
  KMX_CHECK(first >= 0 && n >= 0 && (int64_t)first + n <= h->n_entries, KMX_EINVAL, "entry range outside the database");
  const int64_t p0 = h->fwd.h_fptr[first], total = h->fwd.h_fptr[(size_t)first + n] - p0;
  for (int i = 0; i <= n; ++i) vptr_out[i] = h->fwd.h_fptr[(size_t)first + i] - p0;
  if (!words_out) return KMX_OK;  // sizes only
  KMX_CHECK(weights_out && cap >= total, KMX_EINVAL, "output arrays too small (vptr_out[n] words)");
  if (total == 0) return KMX_OK;
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipMemcpyAsync(words_out, h->fwd.fw.get() + p0, sizeof(unsigned) * total, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipMemcpyAsync(weights_out, h->fwd.fv.get() + p0, sizeof(double) * total, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

namespace {
// Room for nq queries of nw words in all and their K results each.
int bow_reserve_queries(kmx_bow* h, size_t nq, size_t nw, int32_t K) {
  if (nq + 1 > h->qry.qptr.cap() || nw > h->qry.qw.cap() || nq * K > h->qry.id.cap()) {
    KMX_HIP(hipStreamSynchronize(h->stream));  // a query in flight uses the old buffers
    h->qry = BowQuerySet();  // the old set goes first; a failure below leaves the handle without one
    const size_t qcap = std::max<size_t>(nq + 1, 1024), wcap = std::max<size_t>(nw, 1);
    const size_t rcap = std::max<size_t>(nq * K, 1);
    BowQuerySet b;
    int rc;
    if ((rc = b.qptr.alloc(qcap)) || (rc = b.qw.alloc(wcap)) || (rc = b.qv.alloc(wcap)) ||
        (rc = b.maxid.alloc(qcap)) || (rc = b.n.alloc(qcap)) || (rc = b.id.alloc(rcap)) ||
        (rc = b.score.alloc(rcap)))
      return rc;
    h->qry = std::move(b);
  }
  return KMX_OK;
}

int bow_upload_queries(kmx_bow* h, int32_t nq, const int64_t* qptr, const uint32_t* words, const double* weights,
                       const int32_t* max_id, int32_t K) {
  const size_t nw = (size_t)qptr[nq];
  if (int rc = bow_reserve_queries(h, (size_t)nq, nw, K)) return rc;
  KMX_HIP(hipMemcpyAsync(h->qry.qptr.get(), qptr, sizeof(long long) * (nq + 1), hipMemcpyHostToDevice, h->stream));
  if (nw) {
    KMX_HIP(hipMemcpyAsync(h->qry.qw.get(), words, sizeof(unsigned) * nw, hipMemcpyHostToDevice, h->stream));
    KMX_HIP(hipMemcpyAsync(h->qry.qv.get(), weights, sizeof(double) * nw, hipMemcpyHostToDevice, h->stream));
  }
  if (max_id) KMX_HIP(hipMemcpyAsync(h->qry.maxid.get(), max_id, sizeof(int) * nq, hipMemcpyHostToDevice, h->stream));
  return KMX_OK;
}

// The query kernels over the queries in d_qptr / d_qw / d_qv: the base's
// kernel, then, only when there are unsealed entries, k_bow_tail.
int bow_launch_query(kmx_bow* h, int32_t nq, bool has_max_id, int32_t max_results) {
  // only after an add whose seal failed: k_bow_tail holds TAIL_MAX candidates, so seal first
  if (h->n_entries - h->n_sealed > TAIL_MAX)
    if (int rc = bow_seal(h)) return rc;
  KMX_HIP(hipMemsetAsync(h->d_err.get(), 0, 2 * sizeof(int), h->stream));  // error flag, query counter
  BowDb db{h->db.ptr.get(), h->db.ent.get(), h->db.wt.get(), h->n_words, h->n_sealed};
  const int grid = std::min(nq, h->db.n_wg);
  const int* mid = has_max_id ? (const int*)h->qry.maxid.get() : nullptr;
  if (h->lds) {
    hipLaunchKernelGGL(k_bow_query_lds, dim3(grid), dim3(LW_BLOCK), LDS_BOW, h->stream, db,
                       (const int*)h->db.cptr.get(), h->nch, h->ch, nq, (const long long*)h->qry.qptr.get(),
                       (const unsigned*)h->qry.qw.get(), (const double*)h->qry.qv.get(), mid, max_results,
                       h->qry.n.get(), h->qry.id.get(), h->qry.score.get(), h->d_err.get(), h->d_err.get() + 1);
  } else {
    hipLaunchKernelGGL(k_bow_query, dim3(grid), dim3(BOW_BLOCK), 0, h->stream, db, nq,
                       (const long long*)h->qry.qptr.get(), (const unsigned*)h->qry.qw.get(),
                       (const double*)h->qry.qv.get(), mid, max_results, h->db.acc.get(), h->db.touched.get(),
                       h->qry.n.get(), h->qry.id.get(), h->qry.score.get(), h->d_err.get(), h->d_err.get() + 1);
  }
  KMX_HIP(hipGetLastError());
  if (h->n_entries > h->n_sealed) {
    BowFwd f{h->fwd.fptr.get(), h->fwd.fw.get(), h->fwd.fv.get()};
    hipLaunchKernelGGL(k_bow_tail, dim3(std::min(nq, 4096)), dim3(TL_BLOCK), 0, h->stream, f, h->n_sealed, h->n_entries,
                       nq, (const long long*)h->qry.qptr.get(), (const unsigned*)h->qry.qw.get(),
                       (const double*)h->qry.qv.get(), mid, max_results, h->qry.n.get(), h->qry.id.get(),
                       h->qry.score.get());
    KMX_HIP(hipGetLastError());
  }
  return KMX_OK;
}

int bow_fetch_results(kmx_bow* h, int32_t nq, int32_t max_results, int32_t* out_n, int32_t* out_ids,
                      double* out_scores) {
  int err = 0;
  KMX_HIP(hipMemcpyAsync(out_n, h->qry.n.get(), sizeof(int) * nq, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipMemcpyAsync(out_ids, h->qry.id.get(), sizeof(int) * (size_t)nq * max_results, hipMemcpyDeviceToHost,
                         h->stream));
  KMX_HIP(hipMemcpyAsync(out_scores, h->qry.score.get(), sizeof(double) * (size_t)nq * max_results,
                         hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipMemcpyAsync(&err, h->d_err.get(), sizeof(int), hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  KMX_CHECK(!err, KMX_EUNSUP, "too many exactly tied scores at the max_results cut");
  return KMX_OK;
}

int bow_reserve_ids(kmx_bow* h, size_t n) {
  if (n <= h->ids.cap()) return KMX_OK;
  KMX_HIP(hipStreamSynchronize(h->stream));
  h->ids = BowIdSet();
  const size_t cap = std::max<size_t>(n, 1024);
  BowIdSet b;
  int rc;
  if ((rc = b.eid.alloc(2 * cap)) || (rc = b.eout.alloc(cap))) return rc;
  h->ids = std::move(b);
  return KMX_OK;
}
}  // namespace

extern "C" int kmx_bow_query_async(kmx_bow* h, int32_t nq, const int64_t* qptr, const uint32_t* words,
                                   const double* weights, const int32_t* max_id, int32_t max_results) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && h->db.ptr.get(), KMX_ESTATE, "kmx_bow_set_database first");
  KMX_CHECK(nq >= 0 && qptr && max_results > 0 && max_results <= MAX_RESULTS, KMX_EINVAL,
            "bad argument (max_results in [1, 256])");
  KMX_HIP(hipSetDevice(h->device));
  for (int q = 0; q < nq; ++q) KMX_CHECK(qptr[q + 1] >= qptr[q], KMX_EINVAL, "qptr not monotone");
  if (int rc = bow_upload_queries(h, nq, qptr, words, weights, max_id, max_results)) return rc;
  if (nq == 0) return KMX_OK;
  return bow_launch_query(h, nq, max_id != nullptr, max_results);
  KMX_GUARD_END
}

extern "C" int kmx_bow_query(kmx_bow* h, int32_t nq, const int64_t* qptr, const uint32_t* words,
                             const double* weights, const int32_t* max_id, int32_t max_results, int32_t* out_n,
                             int32_t* out_ids, double* out_scores) {
  KMX_GUARD_BEGIN
  KMX_CHECK(out_n && out_ids && out_scores, KMX_EINVAL, "null output");
  if (int rc = kmx_bow_query_async(h, nq, qptr, words, weights, max_id, max_results)) return rc;
  if (nq == 0) return KMX_OK;
  return bow_fetch_results(h, nq, max_results, out_n, out_ids, out_scores);
  KMX_GUARD_END
}

extern "C" int kmx_bow_query_entries_async(kmx_bow* h, kmx_bow* src, int32_t nq, const int32_t* entry_ids,
                                           const int32_t* max_id, int32_t max_results) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && h->db.ptr.get() && src && src->db.ptr.get(), KMX_ESTATE,
            "kmx_bow_set_database or kmx_bow_reset first");
  KMX_CHECK(nq >= 0 && (nq == 0 || entry_ids) && max_results > 0 && max_results <= MAX_RESULTS, KMX_EINVAL,
            "bad argument (max_results in [1, 256])");
  KMX_CHECK(src->device == h->device, KMX_EINVAL, "the source database is on another device");
  size_t nw = 0;
  for (int q = 0; q < nq; ++q) {
    KMX_CHECK(entry_ids[q] >= 0 && entry_ids[q] < src->n_entries, KMX_EINVAL, "entry id outside the source database");
    nw += (size_t)(src->fwd.h_fptr[(size_t)entry_ids[q] + 1] - src->fwd.h_fptr[entry_ids[q]]);
  }
  if (nq == 0) return KMX_OK;
  KMX_HIP(hipSetDevice(h->device));
  int rc;
  if ((rc = bow_reserve_queries(h, (size_t)nq, nw, max_results)) || (rc = bow_reserve_ids(h, (size_t)nq))) return rc;
  if (src != h && src->stream != h->stream) {  // after the adds enqueued on the source's stream
    KMX_HIP(hipEventRecord(h->ev, src->stream));
    KMX_HIP(hipStreamWaitEvent(h->stream, h->ev, 0));
  }
  KMX_HIP(hipMemcpyAsync(h->ids.eid.get(), entry_ids, sizeof(int) * nq, hipMemcpyHostToDevice, h->stream));
  if (max_id) KMX_HIP(hipMemcpyAsync(h->qry.maxid.get(), max_id, sizeof(int) * nq, hipMemcpyHostToDevice, h->stream));
  BowFwd f{src->fwd.fptr.get(), src->fwd.fw.get(), src->fwd.fv.get()};
  hipLaunchKernelGGL(k_bow_scan_len<1>, dim3(1), dim3(TL_BLOCK), 0, h->stream, nq, (const int*)h->ids.eid.get(), f.fptr,
                     h->qry.qptr.get());
  KMX_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_bow_gather, dim3(nq), dim3(256), 0, h->stream, f, (const int*)h->ids.eid.get(),
                     (const long long*)h->qry.qptr.get(), h->qry.qw.get(), h->qry.qv.get());
  KMX_HIP(hipGetLastError());
  return bow_launch_query(h, nq, max_id != nullptr, max_results);
  KMX_GUARD_END
}

extern "C" int kmx_bow_query_entries(kmx_bow* h, kmx_bow* src, int32_t nq, const int32_t* entry_ids,
                                     const int32_t* max_id, int32_t max_results, int32_t* out_n, int32_t* out_ids,
                                     double* out_scores) {
  KMX_GUARD_BEGIN
  KMX_CHECK(out_n && out_ids && out_scores, KMX_EINVAL, "null output");
  if (int rc = kmx_bow_query_entries_async(h, src, nq, entry_ids, max_id, max_results)) return rc;
  if (nq == 0) return KMX_OK;
  return bow_fetch_results(h, nq, max_results, out_n, out_ids, out_scores);
  KMX_GUARD_END
}

extern "C" int kmx_bow_fetch(kmx_bow* h, int32_t nq, int32_t max_results, int32_t* out_n, int32_t* out_ids,
                             double* out_scores) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && out_n && out_ids && out_scores, KMX_EINVAL, "null argument");
  KMX_CHECK(nq >= 0 && max_results > 0 && (size_t)nq + 1 <= h->qry.qptr.cap() &&
            (size_t)nq * max_results <= h->qry.id.cap(), KMX_EINVAL, "no enqueued query of this shape");
  if (nq == 0) return KMX_OK;
  KMX_HIP(hipSetDevice(h->device));
  return bow_fetch_results(h, nq, max_results, out_n, out_ids, out_scores);
  KMX_GUARD_END
}

extern "C" int kmx_bow_score_entries(kmx_bow* src, int32_t n, const int32_t* a_ids, const int32_t* b_ids,
                                     double* out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(src && n >= 0 && (n == 0 || (a_ids && b_ids && out)), KMX_EINVAL, "bad argument");
  KMX_CHECK(src->db.ptr.get(), KMX_ESTATE, "kmx_bow_set_database or kmx_bow_reset first");
  for (int i = 0; i < n; ++i)
    KMX_CHECK(a_ids[i] >= -1 && a_ids[i] < src->n_entries && b_ids[i] >= -1 && b_ids[i] < src->n_entries,
              KMX_EINVAL, "entry id outside the database (-1: no entry)");
  if (n == 0) return KMX_OK;
  KMX_HIP(hipSetDevice(src->device));
  if (int rc = bow_reserve_ids(src, (size_t)n)) return rc;
  KMX_HIP(hipMemcpyAsync(src->ids.eid.get(), a_ids, sizeof(int) * n, hipMemcpyHostToDevice, src->stream));
  KMX_HIP(hipMemcpyAsync(src->ids.eid.get() + src->ids.cap(), b_ids, sizeof(int) * n, hipMemcpyHostToDevice,
                         src->stream));
  BowFwd f{src->fwd.fptr.get(), src->fwd.fw.get(), src->fwd.fv.get()};
  hipLaunchKernelGGL(k_bow_entry_score, dim3((n + 255) / 256), dim3(256), 0, src->stream, n, f,
                     (const int*)src->ids.eid.get(), (const int*)(src->ids.eid.get() + src->ids.cap()),
                     src->ids.eout.get());
  KMX_HIP(hipGetLastError());
  KMX_HIP(hipMemcpyAsync(out, src->ids.eout.get(), sizeof(double) * n, hipMemcpyDeviceToHost, src->stream));
  KMX_HIP(hipStreamSynchronize(src->stream));
  return KMX_OK;
  KMX_GUARD_END
}

// ---- detectLoop / detectLoopWithRobot decided on the device
namespace {
// The result block of a call of nq queries: records, then {n_cand, error}, then the candidate pairs.
size_t det_hdr_off(size_t nq) { return sizeof(kmx_bow_detect_record) * nq; }
size_t det_cand_off(size_t nq) { return det_hdr_off(nq) + 2 * sizeof(int); }
size_t det_bytes(size_t nq) { return det_cand_off(nq) + 2 * sizeof(int) * nq; }
static_assert(sizeof(kmx_bow_detect_record) == 48, "kmx_bow_detect_record is 48 bytes");

int bow_reserve_detect(kmx_bow* h, size_t nq) {
  if (nq <= h->det.cap()) return KMX_OK;
  KMX_HIP(hipStreamSynchronize(h->stream));
  h->det = BowDetSet();
  const size_t cap = std::max<size_t>(nq, 1024);
  BowDetSet b;
  int rc;
  if ((rc = b.hasprev.alloc(2 * cap)) || (rc = b.tin.alloc(cap)) || (rc = b.dout.alloc(det_bytes(cap))) ||
      (rc = b.h_dout.alloc(det_bytes(cap))))
    return rc;
  h->det = std::move(b);
  return KMX_OK;
}

int bow_time(kmx_bow* h, int k) {  // event k of the enqueued detection, when timing is on
  if (!h->timing) return KMX_OK;
  if (!h->tev[k])
    if (int rc = h->tev[k].create()) return rc;
  KMX_HIP(hipEventRecord(h->tev[k], h->stream));
  return KMX_OK;
}

// k_bow_decide over nq rows of stride K on the device and, in intra mode,
// k_bow_temporal on `state`; then the copy of the result block to its host
// mirror (no synchronise).
int bow_launch_decide(kmx_bow* h, int32_t nq, int32_t K, int32_t mode, const kmx_bow_detect_params* p,
                      const int* qids, const int* n, const int* ids, const double* scores, const double* nss,
                      const int* has_prev, const int* qerr, int* state) {
  char* out = h->det.dout.get();
  kmx_bow_detect_record* rec = reinterpret_cast<kmx_bow_detect_record*>(out);
  int* hdr = reinterpret_cast<int*>(out + det_hdr_off((size_t)nq));
  int* cand = reinterpret_cast<int*>(out + det_cand_off((size_t)nq));
  const BowDecide d{p->use_nss, p->alpha, p->min_nss_factor, p->max_intraisland_gap, p->min_matches_per_island};
  hipLaunchKernelGGL(k_bow_decide, dim3(std::min(nq, 1 << 20)), dim3(DEC_WAVE), 0, h->stream, nq, K, mode, d, qids, n,
                     ids, scores, nss, has_prev, rec, h->det.tin.get(), h->det.hasprev.get() + h->det.cap(), qerr, hdr);
  KMX_HIP(hipGetLastError());
  if (int rc = bow_time(h, 2)) return rc;
  if (mode == KMX_BOW_MODE_INTRA) {
    hipLaunchKernelGGL(k_bow_temporal, dim3(1), dim3(DEC_WAVE), 0, h->stream, nq, p->max_nrFrames_between_queries,
                       p->max_nrFrames_between_islands, p->min_temporal_matches, (const int4*)h->det.tin.get(),
                       (const int*)(h->det.hasprev.get() + h->det.cap()), rec, state,
                       cand, hdr);
    KMX_HIP(hipGetLastError());
  }
  if (int rc = bow_time(h, 3)) return rc;
  KMX_HIP(hipMemcpyAsync(h->det.h_dout.get(), out, det_bytes((size_t)nq), hipMemcpyDeviceToHost, h->stream));
  h->det.nq = nq;
  return KMX_OK;
}

int bow_fetch_decide(kmx_bow* h, int32_t nq, kmx_bow_detect_record* records_out, int32_t* cand_out,
                     int32_t* n_cand_out) {
  KMX_HIP(hipStreamSynchronize(h->stream));
  const int* hdr = reinterpret_cast<const int*>(h->det.h_dout.get() + det_hdr_off((size_t)nq));
  KMX_CHECK(!hdr[1], KMX_EUNSUP, "too many exactly tied scores at the max_results cut");
  const int nc = std::max(0, std::min(hdr[0], nq));
  std::copy_n(reinterpret_cast<const kmx_bow_detect_record*>(h->det.h_dout.get()), nq, records_out);
  if (cand_out) std::copy_n(reinterpret_cast<const int*>(h->det.h_dout.get() + det_cand_off((size_t)nq)),
                            2 * (size_t)nc, cand_out);
  if (n_cand_out) *n_cand_out = nc;
  return KMX_OK;
}
}  // namespace

extern "C" int kmx_bow_detect_entries_async(kmx_bow* h, kmx_bow* src, int32_t nq, const int32_t* entry_ids,
                                            int32_t mode, const kmx_bow_detect_params* params) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  if (!src) src = h;
  std::string err;
  if (int rc = kmx::bow_check_detect_params(params, mode, MAX_RESULTS, &err)) return kmx::fail(rc, err);
  KMX_CHECK(h->db.ptr.get() && src->db.ptr.get(), KMX_ESTATE, "kmx_bow_set_database or kmx_bow_reset first");
  KMX_CHECK(nq >= 0 && (nq == 0 || entry_ids), KMX_EINVAL, "bad argument");
  KMX_CHECK(src->device == h->device, KMX_EINVAL, "the source database is on another device");
  KMX_CHECK(mode == KMX_BOW_MODE_INTER || src == h, KMX_EINVAL, "intra mode queries the database's own entries");
  size_t nw = 0;
  bool consecutive = true;  // a keyframe stream: the ids are made on the device, not uploaded
  for (int q = 0; q < nq; ++q) {
    KMX_CHECK(entry_ids[q] >= 0 && entry_ids[q] < src->n_entries, KMX_EINVAL, "entry id outside the source database");
    nw += (size_t)(src->fwd.h_fptr[(size_t)entry_ids[q] + 1] - src->fwd.h_fptr[entry_ids[q]]);
    consecutive = consecutive && entry_ids[q] - entry_ids[0] == q;
  }
  h->det.nq = -1;
  if (nq == 0) {
    h->det.nq = 0;
    return KMX_OK;
  }
  const int32_t K = params->max_db_results;
  const bool intra = mode == KMX_BOW_MODE_INTRA;
  KMX_HIP(hipSetDevice(h->device));
  int rc;
  if ((rc = bow_reserve_queries(h, (size_t)nq, nw, K)) || (rc = bow_reserve_ids(h, (size_t)nq)) ||
      (rc = bow_reserve_detect(h, (size_t)nq)))
    return rc;
  if (src != h && src->stream != h->stream) {  // after the adds enqueued on the source's stream
    KMX_HIP(hipEventRecord(h->ev, src->stream));
    KMX_HIP(hipStreamWaitEvent(h->stream, h->ev, 0));
  }
  if ((rc = bow_time(h, 0))) return rc;
  if (!consecutive)
    KMX_HIP(hipMemcpyAsync(h->ids.eid.get(), entry_ids, sizeof(int) * nq, hipMemcpyHostToDevice, h->stream));
  BowFwd f{src->fwd.fptr.get(), src->fwd.fw.get(), src->fwd.fv.get()};
  hipLaunchKernelGGL(k_bow_detect_prep, dim3((nq + 255) / 256), dim3(256), 0, h->stream, nq, mode,
                     params->recent_frames_window, params->use_nss, f, entry_ids[0],
                     consecutive ? (const int*)nullptr : (const int*)h->ids.eid.get(), h->ids.eid.get(),
                     h->det.hasprev.get(), h->qry.maxid.get(), h->ids.eout.get());
  KMX_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_bow_scan_len<1>, dim3(1), dim3(TL_BLOCK), 0, h->stream, nq, (const int*)h->ids.eid.get(), f.fptr,
                     h->qry.qptr.get());
  KMX_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_bow_gather, dim3(nq), dim3(256), 0, h->stream, f, (const int*)h->ids.eid.get(),
                     (const long long*)h->qry.qptr.get(), h->qry.qw.get(), h->qry.qv.get());
  KMX_HIP(hipGetLastError());
  if ((rc = bow_launch_query(h, nq, intra, K))) return rc;
  if ((rc = bow_time(h, 1))) return rc;
  return bow_launch_decide(h, nq, K, mode, params, h->ids.eid.get(), h->qry.n.get(), h->qry.id.get(),
                           h->qry.score.get(), params->use_nss ? h->ids.eout.get() : nullptr, h->det.hasprev.get(),
                           h->d_err.get(), h->d_tstate.get());
  KMX_GUARD_END
}

extern "C" int kmx_bow_detect_fetch(kmx_bow* h, int32_t nq, kmx_bow_detect_record* records_out, int32_t* cand_out,
                                    int32_t* n_cand_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && nq >= 0 && (nq == 0 || records_out), KMX_EINVAL, "bad argument");
  KMX_CHECK(nq == h->det.nq, KMX_EINVAL, "no enqueued detection of this size");
  if (n_cand_out) *n_cand_out = 0;
  if (nq == 0) return KMX_OK;
  KMX_HIP(hipSetDevice(h->device));
  return bow_fetch_decide(h, nq, records_out, cand_out, n_cand_out);
  KMX_GUARD_END
}

extern "C" int kmx_bow_detect_entries(kmx_bow* h, kmx_bow* src, int32_t nq, const int32_t* entry_ids, int32_t mode,
                                      const kmx_bow_detect_params* params, kmx_bow_detect_record* records_out,
                                      int32_t* cand_out, int32_t* n_cand_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(nq <= 0 || records_out, KMX_EINVAL, "null output");
  if (int rc = kmx_bow_detect_entries_async(h, src, nq, entry_ids, mode, params)) return rc;
  return kmx_bow_detect_fetch(h, nq, records_out, cand_out, n_cand_out);
  KMX_GUARD_END
}

extern "C" int kmx_bow_decide_results(kmx_bow* h, int32_t nq, int32_t K, const int32_t* query_ids, const int32_t* n,
                                      const int32_t* ids, const double* scores, const double* nss,
                                      const int32_t* has_prev, int32_t mode, const kmx_bow_detect_params* params,
                                      int32_t use_state, kmx_bow_detect_record* records_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  std::string err;
  if (int rc = kmx::bow_check_detect_params(params, mode, MAX_RESULTS, &err)) return kmx::fail(rc, err);
  if (int rc = kmx::bow_check_result_counts(nq, K, MAX_RESULTS, n, &err)) return kmx::fail(rc, err);
  if (nq == 0) return KMX_OK;
  KMX_CHECK(ids && scores && records_out, KMX_EINVAL, "null argument");
  KMX_HIP(hipSetDevice(h->device));
  int rc;
  if ((rc = bow_reserve_queries(h, (size_t)nq, 0, K)) || (rc = bow_reserve_ids(h, (size_t)nq)) ||
      (rc = bow_reserve_detect(h, (size_t)nq)))
    return rc;
  const size_t rows = (size_t)nq * K;
  KMX_HIP(hipMemcpyAsync(h->qry.n.get(), n, sizeof(int) * nq, hipMemcpyHostToDevice, h->stream));
  KMX_HIP(hipMemcpyAsync(h->qry.id.get(), ids, sizeof(int) * rows, hipMemcpyHostToDevice, h->stream));
  KMX_HIP(hipMemcpyAsync(h->qry.score.get(), scores, sizeof(double) * rows, hipMemcpyHostToDevice, h->stream));
  if (query_ids) KMX_HIP(hipMemcpyAsync(h->ids.eid.get(), query_ids, sizeof(int) * nq, hipMemcpyHostToDevice,
                                        h->stream));
  if (nss) KMX_HIP(hipMemcpyAsync(h->ids.eout.get(), nss, sizeof(double) * nq, hipMemcpyHostToDevice, h->stream));
  if (has_prev) KMX_HIP(hipMemcpyAsync(h->det.hasprev.get(), has_prev, sizeof(int) * nq, hipMemcpyHostToDevice,
                                       h->stream));
  int* state = h->d_tstate.get();
  if (!use_state) {  // a pass of its own: from zeros, in the scratch half
    state += 4;
    KMX_HIP(hipMemsetAsync(state, 0, 4 * sizeof(int), h->stream));
  }
  if ((rc = bow_time(h, 0)) || (rc = bow_time(h, 1))) return rc;
  if ((rc = bow_launch_decide(h, nq, K, mode, params, query_ids ? h->ids.eid.get() : nullptr, h->qry.n.get(),
                              h->qry.id.get(), h->qry.score.get(), nss ? h->ids.eout.get() : nullptr,
                              has_prev ? h->det.hasprev.get() : nullptr, nullptr, state)))
    return rc;
  return bow_fetch_decide(h, nq, records_out, nullptr, nullptr);
  KMX_GUARD_END
}

extern "C" int kmx_bow_get_temporal_state(kmx_bow* h, int32_t* state4_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && state4_out, KMX_EINVAL, "null argument");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipMemcpyAsync(state4_out, h->d_tstate.get(), 4 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_bow_set_temporal_state(kmx_bow* h, const int32_t* state4) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && state4, KMX_EINVAL, "null argument");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipMemcpyAsync(h->d_tstate.get(), state4, 4 * sizeof(int), hipMemcpyHostToDevice, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));  // the caller's array is free again
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_bow_enable_timing(kmx_bow* h, int on) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  h->timing = on != 0;
  return KMX_OK;
}

extern "C" int kmx_bow_read_detect_timing(kmx_bow* h, double* ms3_out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && ms3_out, KMX_EINVAL, "null argument");
  KMX_CHECK(h->timing && h->tev[0] && h->tev[1] && h->tev[2] && h->tev[3], KMX_ESTATE,
            "no detection was enqueued with timing on");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  for (int k = 0; k < 3; ++k) {
    float ms = 0.f;
    KMX_HIP(hipEventElapsedTime(&ms, h->tev[k], h->tev[k + 1]));
    ms3_out[k] = ms;
  }
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_bow_sync(kmx_bow* h) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
}

extern "C" int kmx_bow_score_pairs(kmx_bow* h, int32_t n, const int64_t* aptr, const uint32_t* aw,
                                   const double* av, const int64_t* bptr, const uint32_t* bw, const double* bv,
                                   double* out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && n >= 0 && aptr && bptr && out, KMX_EINVAL, "bad argument");
  if (n == 0) return KMX_OK;
  KMX_HIP(hipSetDevice(h->device));
  const size_t na = (size_t)aptr[n], nb = (size_t)bptr[n];
  if ((size_t)n + 1 > h->pair.aptr.cap() || std::max(na, nb) > h->pair.aw.cap()) {
    h->pair = BowPairSet();
    const size_t pcap = std::max<size_t>(n + 1, 1024), pwcap = std::max<size_t>(std::max(na, nb), 1);
    BowPairSet b;
    int rc;
    if ((rc = b.aptr.alloc(pcap)) || (rc = b.bptr.alloc(pcap)) || (rc = b.aw.alloc(pwcap)) ||
        (rc = b.bw.alloc(pwcap)) || (rc = b.av.alloc(pwcap)) || (rc = b.bv.alloc(pwcap)) || (rc = b.out.alloc(pcap)))
      return rc;
    h->pair = std::move(b);
  }
  KMX_HIP(hipMemcpyAsync(h->pair.aptr.get(), aptr, sizeof(long long) * (n + 1), hipMemcpyHostToDevice, h->stream));
  KMX_HIP(hipMemcpyAsync(h->pair.bptr.get(), bptr, sizeof(long long) * (n + 1), hipMemcpyHostToDevice, h->stream));
  if (na) {
    KMX_HIP(hipMemcpyAsync(h->pair.aw.get(), aw, sizeof(unsigned) * na, hipMemcpyHostToDevice, h->stream));
    KMX_HIP(hipMemcpyAsync(h->pair.av.get(), av, sizeof(double) * na, hipMemcpyHostToDevice, h->stream));
  }
  if (nb) {
    KMX_HIP(hipMemcpyAsync(h->pair.bw.get(), bw, sizeof(unsigned) * nb, hipMemcpyHostToDevice, h->stream));
    KMX_HIP(hipMemcpyAsync(h->pair.bv.get(), bv, sizeof(double) * nb, hipMemcpyHostToDevice, h->stream));
  }
  hipLaunchKernelGGL(k_bow_pair_score, dim3((n + 255) / 256), dim3(256), 0, h->stream, n,
                     (const long long*)h->pair.aptr.get(), (const unsigned*)h->pair.aw.get(),
                     (const double*)h->pair.av.get(), (const long long*)h->pair.bptr.get(),
                     (const unsigned*)h->pair.bw.get(), (const double*)h->pair.bv.get(), h->pair.out.get());
  KMX_HIP(hipGetLastError());
  KMX_HIP(hipMemcpyAsync(out, h->pair.out.get(), sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}
