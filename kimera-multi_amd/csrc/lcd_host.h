// lcd_host.h — host-side logic of lcd.hip that needs no device: the opengv
// sampler tables, the parameter and argument checks of kmx_lcd_create /
// kmx_lcd_verify* / kmx_lcd_verify_matches, the staging layouts of the small
// synchronous calls and the spread form's range schedule. Plain C++, so `make
// lcd_check` can build it with the host sanitizers (lcd_check.cpp).
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "kmx_abi.h"

namespace kmx {

// Solver constants the host shares with the kernels of lcd.hip.
constexpr int PNP_S = 6;  // EPnP's minimal sample
#ifndef KMX_SG
#define KMX_SG 6
#endif
constexpr int SG = KMX_SG;            // Stewenius hypotheses per wave (groups of lanes)
constexpr int SPREAD_PER_NISTER = 2;  // Nister hypotheses per wave (one at a time)
constexpr int SPREAD_WAVES = 1024;    // waves of one k_rs_hyps launch at most

// ---------------------------------------------------------------- sampler --
// One pass of opengv's drawIndexSample: S swaps of the persistent shuffle over
// the problem's K indices, each by std::uniform_int_distribution<int>(0,
// INT_MAX) over std::mt19937 (GCC-9 rejection or GCC-11 x >> 1).
inline int sampler_draw(std::mt19937& rng, int variant) {
  uint32_t x;
  if (variant == KMX_RNG_GCC11) {
    x = (uint32_t)rng() >> 1;
  } else {
    do x = (uint32_t)rng();
    while (x >= 0x80000000u);
  }
  return (int)x;
}
inline void sample_row(std::mt19937& rng, int variant, int K, int pmax, int S, short* out) {
  std::vector<int> sh(K);
  for (int i = 0; i < K; ++i) sh[i] = i;
  for (int p = 0; p < pmax; ++p) {
    for (int i = 0; i < S; ++i) {
      const int j = i + (int)((size_t)sampler_draw(rng, variant) % (size_t)(K - i));
      std::swap(sh[i], sh[j]);
    }
    for (int i = 0; i < S; ++i) out[(size_t)p * S + i] = (short)sh[i];
  }
}

// opengv sampler table: for every K in [S, N], the S indices drawn by each of
// the first pmax passes (std::mt19937 seeded per problem). Rows are
// independent, so they are built on a few host threads.
inline void build_table(const kmx_lcd_params& P, int N, int pmax, std::vector<short>& tab, int S = 5) {
  const int rows = std::max(N - S + 1, 1);
  tab.assign((size_t)rows * pmax * S, 0);
  const int nt = std::max(1, std::min(8, rows / 32));
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t)
    th.emplace_back([&, t] {
      for (int K = S + t; K <= N; K += nt) {
        std::mt19937 rng(P.ransac_seed);
        sample_row(rng, P.rng_variant, K, pmax, S, tab.data() + (size_t)(K - S) * pmax * S);
      }
    });
  for (auto& x : th) x.join();
}

inline bool rec_sampled(const kmx_lcd_params& P) { return P.pose_recovery_type == 1 || !P.use_1point_3d3d; }
inline int rec_S(const kmx_lcd_params& P) { return P.pose_recovery_type == 1 ? PNP_S : 3; }
// every pass the serial loop can reach: (max_iter + 1) iterations + 10 * max_iter skips
inline int lcd_pmax(const kmx_lcd_params& P) { return P.ransac_max_iterations + 1 + 10 * P.ransac_max_iterations; }

// ----------------------------------------------------------------- checks --
// The parameters of kmx_lcd_create: KMX_OK, or KMX_EINVAL / KMX_EUNSUP with *err set.
inline int lcd_check_params(const kmx_lcd_params* params, std::string* err) {
  auto bad = [&](int code, const char* m) {
    if (err) *err = m;
    return code;
  };
  if (!params) return bad(KMX_EINVAL, "null argument");
  if (params->norm != KMX_NORM_L1 && params->norm != KMX_NORM_HAMMING) return bad(KMX_EINVAL, "bad norm");
  if (params->rng_variant != KMX_RNG_GCC9 && params->rng_variant != KMX_RNG_GCC11)
    return bad(KMX_EINVAL, "bad rng variant");
  if (params->ransac_randomize != 0) return bad(KMX_EUNSUP, "ransac_randomize = 1 is not reproducible; use 0");
  if (params->use_1point_3d3d != 0 && params->use_1point_3d3d != 1)
    return bad(KMX_EINVAL, "use_1point_3d3d is 0 or 1");
  if (params->algorithm_2d2d != KMX_ALGO_STEWENIUS && params->algorithm_2d2d != KMX_ALGO_NISTER)
    return bad(KMX_EUNSUP, "ransac_2d2d_algorithm: 0 (Stewenius) and 1 (Nister) are built");
  if (params->ransac_max_iterations <= 0) return bad(KMX_EINVAL, "ransac_max_iterations must be > 0");
  if (params->rng_stream != 0 && params->rng_stream != 1) return bad(KMX_EINVAL, "rng_stream is 0 or 1");
  return KMX_OK;
}

// n candidates' frame ids against a pool of F frames. Reads cq / cm [0, n).
inline int lcd_check_cands(int32_t n, int F, const int32_t* cq, const int32_t* cm, std::string* err) {
  for (int i = 0; i < n; ++i)
    if (!(cq[i] >= 0 && cq[i] < F && cm[i] >= 0 && cm[i] < F)) {
      if (err) *err = "candidate frame id out of range";
      return KMX_EINVAL;
    }
  return KMX_OK;
}

// The correspondences of kmx_lcd_verify_matches as CSR: candidate i's pairs
// are (iq[k], im[k]) for k in [mptr[i], mptr[i + 1]), indices into the
// features of frames cq[i] / cm[i] (checked ids; nfeat[f]: frame f's count),
// at most N pairs per candidate. Structure first: every mptr difference is
// checked before an index is read, so an absurd mptr reads nothing, and the
// index arrays may be null when mptr holds no pair.
inline int lcd_check_csr(int32_t n, int N, const int64_t* mptr, const int32_t* iq, const int32_t* im,
                         const int32_t* cq, const int32_t* cm, const int* nfeat, std::string* err) {
  auto bad = [&](const char* m) {
    if (err) *err = m;
    return KMX_EINVAL;
  };
  if (n <= 0) return KMX_OK;
  if (!mptr) return bad("null mptr");
  if (mptr[0] < 0) return bad("mptr[0] < 0");
  for (int i = 0; i < n; ++i) {
    // (a decreasing mptr first: the difference of two int64 values in range cannot overflow then)
    if (mptr[i + 1] < mptr[i] || mptr[i + 1] - mptr[i] > N)
      return bad("a candidate has more pairs than max_feats (or mptr decreases)");
  }
  if (mptr[n] > mptr[0] && !(iq && im)) return bad("null i_query / i_match with correspondences in mptr");
  for (int i = 0; i < n; ++i) {
    const int nq = nfeat[cq[i]], nm = nfeat[cm[i]];
    for (int64_t k = mptr[i]; k < mptr[i + 1]; ++k)
      if (!(iq[k] >= 0 && iq[k] < nq && im[k] >= 0 && im[k] < nm))
        return bad("correspondence index outside its frame's features");
  }
  return KMX_OK;
}

// ---------------------------------------------------------------- staging --
inline size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }

// kmx_lcd_match's pinned staging block: [cq][cm] in, [pairs][K] out.
struct LcdMatchLayout {
  size_t o_cq, o_cm, o_pairs, o_K, total;
};
inline LcdMatchLayout lcd_match_layout(int n, int N) {
  LcdMatchLayout L{};
  const size_t kin = al16(sizeof(int32_t) * (size_t)n);
  L.o_cq = 0;
  L.o_cm = kin;
  L.o_pairs = 2 * kin;
  L.o_K = L.o_pairs + al16(2 * sizeof(int32_t) * (size_t)n * N);
  L.total = L.o_K + kin;
  return L;
}

// kmx_lcd_verify_matches' block: every input in one host-to-device copy,
// [mptr - base][cq][cm][i_query][i_match][T_prior], and the outputs after the
// inputs (zero-copy kernels read and write at once): [results][masks].
// in_bytes: the inputs' extent (the copy's size).
struct LcdVerifyLayout {
  size_t o_mptr, o_cq, o_cm, o_iq, o_im, o_prior, in_bytes, o_res, o_mask, total;
};
inline LcdVerifyLayout lcd_verify_layout(int n, int N, size_t total_pairs, bool prior, bool masks) {
  LcdVerifyLayout L{};
  const size_t ids = al16(sizeof(int32_t) * (size_t)n), idx = al16(sizeof(int32_t) * total_pairs);
  L.o_mptr = 0;
  L.o_cq = al16(sizeof(int64_t) * ((size_t)n + 1));
  L.o_cm = L.o_cq + ids;
  L.o_iq = L.o_cm + ids;
  L.o_im = L.o_iq + idx;
  L.o_prior = L.o_im + idx;
  L.in_bytes = L.o_prior + (prior ? sizeof(double) * 12 * (size_t)n : 0);
  L.o_res = al16(L.in_bytes);
  L.o_mask = L.o_res + al16(sizeof(kmx_lcd_result) * (size_t)n);
  L.total = L.o_mask + (masks ? (size_t)n * N : 0);
  return L;
}

// ----------------------------------------------------- the spread form's ranges --
// ransac_spread launches hypothesis ranges [pa, pb) of growing size until no
// candidate needs more. The first range: a true loop closure's loop (~30
// iterations) in one pass; where the launch has the waves for it (one or two
// candidates), a whole 500-iteration loop (510) at once — one hypothesis per
// wave costs the same latency, and a look-alike then needs one range, not two.
inline int spread_first_range(int n) { return (int64_t)n * 510 <= SPREAD_WAVES ? 510 : 66; }
// then the rest of a 500-iteration loop, then its skips
inline int spread_next_range(int pa) { return pa < 510 ? 510 - pa : 1500; }
inline int spread_per_max(int algorithm_2d2d) { return algorithm_2d2d == KMX_ALGO_STEWENIUS ? SG : SPREAD_PER_NISTER; }
// One range of `range` passes from pa for n candidates: `per` hypotheses per
// wave — as few as the launch's waves allow (one wave works through its
// hypotheses one after another; the batch of SG Stewenius hypotheses per wave
// only pays where waves are short) — on G waves per candidate, ending at pb.
struct SpreadStep {
  int per, G, pb;
};
inline SpreadStep spread_step(int n, int pa, int range, int per_max, int pmax) {
  SpreadStep s{};
  s.per = std::max(1, std::min(per_max, (int)(((int64_t)n * range + SPREAD_WAVES - 1) / SPREAD_WAVES)));
  s.G = (range + s.per - 1) / s.per;
  s.G = std::max(1, std::min(s.G, SPREAD_WAVES / n));
  s.pb = std::min(pa + s.G * s.per, pmax);
  return s;
}

}  // namespace kmx
