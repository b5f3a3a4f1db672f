// bow_host.h — host-side checks of bow.hip that need no device: the CSR
// validation kmx_bow_add_entries runs before any device call, and the
// parameter and shape checks of kmx_bow_detect_entries / kmx_bow_decide_results.
// Plain C++, so `make bow_check` can build it with the host sanitizers
// (bow_check.cpp).
#pragma once
#include <climits>
#include <cstdint>
#include <string>

#include "kmx_abi.h"

namespace kmx {

// n BowVectors as CSR (vptr[n + 1], words, weights) to be appended to a
// database over n_words words that holds n_entries_now entries and
// n_postings_now postings. KMX_OK, or KMX_EINVAL with *err set: vptr must be
// monotone from a value >= 0, a vector's words strictly increasing and
// < n_words, every weight finite and > 0, and the totals must stay below
// INT32_MAX (posting lists are indexed with int). The totals are checked
// before a word or a weight is read, so an absurd vptr reads nothing.
// The weights: the query kernels take an accumulator of exactly 0.0 for "entry
// not touched yet", which holds because a contribution |q - d| - |q| - |d| of
// positive finite weights is negative; DBoW2 stores no other weight.
inline int bow_check_csr(int32_t n_words, int64_t n_entries_now, int64_t n_postings_now, int64_t n,
                         const int64_t* vptr, const uint32_t* words, const double* weights, std::string* err) {
  auto bad = [&](const char* m) {
    if (err) *err = m;
    return KMX_EINVAL;
  };
  if (n_words <= 0 || n < 0 || n_entries_now < 0 || n_postings_now < 0) return bad("bad argument");
  if (n == 0) return KMX_OK;
  if (!vptr) return bad("null vptr");
  if (n >= (int64_t)INT32_MAX - n_entries_now) return bad("database too large (entries must fit int32)");
  if (vptr[0] < 0) return bad("vptr not monotone");
  for (int64_t e = 0; e < n; ++e)
    if (vptr[e + 1] < vptr[e]) return bad("vptr not monotone");
  const int64_t total = vptr[n] - vptr[0];
  if (total >= (int64_t)INT32_MAX - n_postings_now) return bad("database too large (postings must fit int32)");
  if (total > 0 && !words) return bad("null words");
  if (total > 0 && !weights) return bad("null weights");
  for (int64_t e = 0; e < n; ++e)
    for (int64_t k = vptr[e]; k < vptr[e + 1]; ++k) {
      if (words[k] >= (uint32_t)n_words) return bad("word id >= n_words");
      if (k > vptr[e] && words[k] <= words[k - 1]) return bad("BowVector words must be strictly increasing");
      // x - x is 0 for a finite x and NaN for an infinity or a NaN; -0.0 > 0.0 is false
      const double x = weights[k];
      if (!(x > 0.0) || !(x - x == 0.0)) return bad("BowVector weights must be finite and > 0");
    }
  return KMX_OK;
}

// The detection parameters of kmx_bow_detect_entries / kmx_bow_decide_results
// (kmx_abi.h): KMX_OK, or KMX_EINVAL with *err set. max_results_cap is the
// query kernels' MAX_RESULTS.
inline int bow_check_detect_params(const kmx_bow_detect_params* p, int32_t mode, int32_t max_results_cap,
                                   std::string* err) {
  auto bad = [&](const char* m) {
    if (err) *err = m;
    return KMX_EINVAL;
  };
  if (!p) return bad("null params");
  if (mode != KMX_BOW_MODE_INTRA && mode != KMX_BOW_MODE_INTER) return bad("mode must be 0 (intra) or 1 (inter)");
  if (p->use_nss != 0 && p->use_nss != 1) return bad("use_nss must be 0 or 1");
  // x - x is 0 for a finite x and NaN for an infinity or a NaN
  if (!(p->alpha - p->alpha == 0.0)) return bad("alpha must be finite");
  if (!(p->min_nss_factor - p->min_nss_factor == 0.0)) return bad("min_nss_factor must be finite");
  if (p->max_db_results < 1 || p->max_db_results > max_results_cap) return bad("max_db_results must be in [1, 256]");
  if (p->recent_frames_window < 0) return bad("recent_frames_window must be >= 0");
  if (p->max_intraisland_gap < 0) return bad("max_intraisland_gap must be >= 0");
  if (p->min_matches_per_island < 0) return bad("min_matches_per_island must be >= 0");
  if (p->max_nrFrames_between_queries < 0) return bad("max_nrFrames_between_queries must be >= 0");
  if (p->max_nrFrames_between_islands < 0) return bad("max_nrFrames_between_islands must be >= 0");
  if (p->min_temporal_matches < 0) return bad("min_temporal_matches must be >= 0");
  return KMX_OK;
}

// The shape of caller-supplied query results (kmx_bow_decide_results): nq rows
// of stride K, n[q] results in row q. Reads n[0 .. nq) and nothing else.
inline int bow_check_result_counts(int64_t nq, int32_t K, int32_t max_results_cap, const int32_t* n,
                                   std::string* err) {
  auto bad = [&](const char* m) {
    if (err) *err = m;
    return KMX_EINVAL;
  };
  if (nq < 0 || nq >= (int64_t)INT32_MAX / 256) return bad("bad query count");
  if (K < 1 || K > max_results_cap) return bad("K must be in [1, 256]");
  if (nq == 0) return KMX_OK;
  if (!n) return bad("null result counts");
  for (int64_t q = 0; q < nq; ++q)
    if (n[q] < 0 || n[q] > K) return bad("a result count outside [0, K]");
  return KMX_OK;
}

}  // namespace kmx
