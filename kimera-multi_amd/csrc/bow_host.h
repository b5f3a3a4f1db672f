// bow_host.h — host-side checks of bow.hip that need no device: the CSR
// validation kmx_bow_add_entries runs before any device call. Plain C++, so
// `make bow_check` can build it with the host sanitizers (bow_check.cpp).
#pragma once
#include <climits>
#include <cstdint>
#include <string>

#include "kmx_abi.h"

namespace kmx {

// n BowVectors as CSR (vptr[n + 1], words) to be appended to a database over
// n_words words that holds n_entries_now entries and n_postings_now postings.
// KMX_OK, or KMX_EINVAL with *err set: vptr must be monotone from a value
// >= 0, a vector's words strictly increasing and < n_words, and the totals
// must stay below INT32_MAX (posting lists are indexed with int). The totals
// are checked before a word is read, so an absurd vptr reads nothing.
inline int bow_check_csr(int32_t n_words, int64_t n_entries_now, int64_t n_postings_now, int64_t n,
                         const int64_t* vptr, const uint32_t* words, std::string* err) {
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
  for (int64_t e = 0; e < n; ++e)
    for (int64_t k = vptr[e]; k < vptr[e + 1]; ++k) {
      if (words[k] >= (uint32_t)n_words) return bad("word id >= n_words");
      if (k > vptr[e] && words[k] <= words[k - 1]) return bad("BowVector words must be strictly increasing");
    }
  return KMX_OK;
}

}  // namespace kmx
