// bow_check.cpp — bow.hip's host code (bow_host.h: the CSR validation of
// kmx_bow_add_entries, the parameter and shape checks of kmx_bow_detect_entries
// and kmx_bow_decide_results) as a stand-alone program, built by `make
// bow_check` with the host address and undefined-behaviour sanitizers. It feeds
// kmx::bow_check_csr the inputs kmx_bow_add_entries and kmx_bow_set_database
// must reject (weights that are not finite and > 0 among them), in arrays of
// exactly the stated size so that a read past either is a report, and
// kmx::bow_check_detect_params / bow_check_result_counts malformed parameter
// sets and counts. CPU only.
#include <climits>
#include <cstdio>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "bow_host.h"

namespace {

int g_fail = 0;

// `weights` empty: every word gets the legal weight 0.5
void expect_code(int32_t n_words, int64_t n_now, int64_t post_now, const std::vector<int64_t>& vptr,
                 const std::vector<uint32_t>& words, int code, const char* what,
                 const std::vector<double>& weights = {}) {
  // exact-size copies, so a read past any array is a sanitizer report
  std::vector<int64_t> vp(vptr);
  std::vector<uint32_t> w(words);
  std::vector<double> x(weights.empty() ? std::vector<double>(words.size(), 0.5) : weights);
  std::string err;
  const int64_t n = vp.empty() ? 0 : (int64_t)vp.size() - 1;
  const int rc = kmx::bow_check_csr(n_words, n_now, post_now, n, vp.empty() ? nullptr : vp.data(),
                                    w.empty() ? nullptr : w.data(), x.empty() ? nullptr : x.data(), &err);
  if (rc != code || (code != KMX_OK && err.find(what) == std::string::npos)) {
    std::fprintf(stderr, "expected %d (%s), got %d (%s)\n", code, what, rc, err.c_str());
    ++g_fail;
  }
}

void expect_params(const kmx_bow_detect_params* p, int32_t mode, int code, const char* what) {
  std::string err;
  const int rc = kmx::bow_check_detect_params(p, mode, 256, &err);
  if (rc != code || (code != KMX_OK && err.find(what) == std::string::npos)) {
    std::fprintf(stderr, "params: expected %d (%s), got %d (%s)\n", code, what, rc, err.c_str());
    ++g_fail;
  }
}

void expect_counts(int32_t K, const std::vector<int32_t>& n, int code, const char* what) {
  std::vector<int32_t> c(n);  // exactly nq ints
  std::string err;
  const int rc = kmx::bow_check_result_counts((int64_t)c.size(), K, 256, c.empty() ? nullptr : c.data(), &err);
  if (rc != code || (code != KMX_OK && err.find(what) == std::string::npos)) {
    std::fprintf(stderr, "counts: expected %d (%s), got %d (%s)\n", code, what, rc, err.c_str());
    ++g_fail;
  }
}

}  // namespace

int main() {
  // empty input: no vectors, one empty vector, empty vectors between full ones
  expect_code(10, 0, 0, {}, {}, KMX_OK, "");
  expect_code(10, 0, 0, {0}, {}, KMX_OK, "");
  expect_code(10, 5, 7, {0, 0}, {}, KMX_OK, "");
  expect_code(10, 0, 0, {0, 2, 2, 5, 5}, {1, 9, 0, 4, 8}, KMX_OK, "");
  expect_code(10, 0, 0, {3, 5}, {7, 7, 7, 2, 3}, KMX_OK, "");  // vptr need not start at 0
  // a non-monotone vptr
  expect_code(10, 0, 0, {0, 3, 2}, {1, 2, 3}, KMX_EINVAL, "vptr not monotone");
  expect_code(10, 0, 0, {-1, 2}, {1, 2}, KMX_EINVAL, "vptr not monotone");
  // a repeated word, a decreasing word
  expect_code(10, 0, 0, {0, 3}, {1, 4, 4}, KMX_EINVAL, "strictly increasing");
  expect_code(10, 0, 0, {0, 2, 4}, {1, 4, 5, 2}, KMX_EINVAL, "strictly increasing");
  // a word equal to n_words, and beyond
  expect_code(10, 0, 0, {0, 3}, {1, 4, 10}, KMX_EINVAL, "word id >= n_words");
  expect_code(10, 0, 0, {0, 1}, {0xffffffffu}, KMX_EINVAL, "word id >= n_words");
  // int32 overflow of the total: refused before a word is read (there are none)
  expect_code(10, 0, 0, {0, (int64_t)INT32_MAX}, {}, KMX_EINVAL, "postings must fit int32");
  expect_code(10, 0, (int64_t)INT32_MAX - 3, {0, 3}, {1, 2, 3}, KMX_EINVAL, "postings must fit int32");
  expect_code(10, 0, (int64_t)INT32_MAX - 4, {0, 3}, {1, 2, 3}, KMX_OK, "");
  expect_code(10, 0, 0, {0, INT64_MAX}, {}, KMX_EINVAL, "postings must fit int32");
  expect_code(10, (int64_t)INT32_MAX - 1, 0, {0, 0}, {}, KMX_EINVAL, "entries must fit int32");
  expect_code(0, 0, 0, {0, 0}, {}, KMX_EINVAL, "bad argument");
  // random valid batches, and each with one word broken
  std::mt19937 rng(4321);
  int batches = 0;
  for (int rep = 0; rep < 300; ++rep) {
    const int32_t n_words = 1 + (int32_t)(rng() % 50);
    const int n = (int)(rng() % 6);
    std::vector<int64_t> vptr{(int64_t)(rng() % 3)};
    std::vector<uint32_t> words(vptr[0], 0xdeadbeefu);  // never read: before vptr[0]
    for (int e = 0; e < n; ++e) {
      for (int32_t w = 0; w < n_words; ++w)
        if (rng() % 3 == 0) words.push_back((uint32_t)w);
      vptr.push_back((int64_t)words.size());
    }
    expect_code(n_words, rep, rep * 7, vptr, words, KMX_OK, "");
    ++batches;
    const size_t first = (size_t)vptr[0];
    if (words.size() > first) {
      std::vector<uint32_t> broken(words);
      const size_t k = first + rng() % (words.size() - first);
      broken[k] = (uint32_t)n_words + (uint32_t)(rng() % 3);
      expect_code(n_words, rep, rep * 7, vptr, broken, KMX_EINVAL, "word id >= n_words");
    }
  }
  // ---- the weights: finite and > 0 (the query kernels read an accumulator of 0.0 as "untouched")
  {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const char* msg = "weights must be finite and > 0";
    const std::vector<int64_t> vp{0, 2, 2, 5};
    const std::vector<uint32_t> wd{1, 9, 0, 4, 8};
    expect_code(10, 0, 0, vp, wd, KMX_OK, "", {0.25, 0.75, 0.5, 0.25, 0.25});
    expect_code(10, 0, 0, vp, wd, KMX_OK, "", {0.25, 0.75, std::numeric_limits<double>::denorm_min(), 0.25, 0.25});
    expect_code(10, 0, 0, vp, wd, KMX_OK, "", {std::numeric_limits<double>::min() / 4, 0.75, 0.5, 0.25, 1e300});
    expect_code(10, 0, 0, vp, wd, KMX_EINVAL, msg, {0.0, 0.75, 0.5, 0.25, 0.25});
    expect_code(10, 0, 0, vp, wd, KMX_EINVAL, msg, {0.25, -0.0, 0.5, 0.25, 0.25});
    expect_code(10, 0, 0, vp, wd, KMX_EINVAL, msg, {0.25, 0.75, -0.5, 0.25, 0.25});
    expect_code(10, 0, 0, vp, wd, KMX_EINVAL, msg, {0.25, 0.75, nan, 0.25, 0.25});
    expect_code(10, 0, 0, vp, wd, KMX_EINVAL, msg, {0.25, 0.75, 0.5, inf, 0.25});
    expect_code(10, 0, 0, vp, wd, KMX_EINVAL, msg, {0.25, 0.75, 0.5, -inf, 0.25});
    // a bad weight in the last vector of a batch, at its last word
    expect_code(10, 0, 0, vp, wd, KMX_EINVAL, msg, {0.25, 0.75, 0.5, 0.25, 0.0});
    expect_code(10, 7, 70, vp, wd, KMX_EINVAL, msg, {0.25, 0.75, 0.5, 0.25, nan});
    // weights before vptr[0] are not the batch's: never read, whatever they hold
    expect_code(10, 0, 0, {3, 5}, {7, 7, 7, 2, 3}, KMX_OK, "", {nan, -1.0, 0.0, 0.5, 0.5});
    expect_code(10, 0, 0, {3, 5}, {7, 7, 7, 2, 3}, KMX_EINVAL, msg, {0.5, 0.5, 0.5, 0.5, 0.0});
    // null weights with postings stay an error; with none they are fine
    std::string err;
    const int64_t vp1[2] = {0, 1}, vp0[2] = {0, 0};
    const uint32_t w1[1] = {3};
    if (kmx::bow_check_csr(10, 0, 0, 1, vp1, w1, nullptr, &err) != KMX_EINVAL ||
        err.find("null weights") == std::string::npos ||
        kmx::bow_check_csr(10, 0, 0, 1, vp0, nullptr, nullptr, &err) != KMX_OK) {
      std::fprintf(stderr, "null weights: not handled as stated\n");
      ++g_fail;
    }
  }
  // ---- the detection parameters (kmx_bow_detect_entries / kmx_bow_decide_results)
  const kmx_bow_detect_params good{1, 0.4, 0.05, 50, 100, 3, 1, 2, 3, 1};
  expect_params(&good, KMX_BOW_MODE_INTRA, KMX_OK, "");
  expect_params(&good, KMX_BOW_MODE_INTER, KMX_OK, "");
  expect_params(nullptr, KMX_BOW_MODE_INTRA, KMX_EINVAL, "null params");
  expect_params(&good, 2, KMX_EINVAL, "mode");
  expect_params(&good, -1, KMX_EINVAL, "mode");
  int n_params = 0;
  auto with = [&](auto set, const char* what) {
    kmx_bow_detect_params p = good;
    set(p);
    expect_params(&p, KMX_BOW_MODE_INTRA, what[0] ? KMX_EINVAL : KMX_OK, what);
    ++n_params;
  };
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  with([](kmx_bow_detect_params& p) { p.max_db_results = 0; }, "max_db_results");
  with([](kmx_bow_detect_params& p) { p.max_db_results = 257; }, "max_db_results");
  with([](kmx_bow_detect_params& p) { p.max_db_results = -1; }, "max_db_results");
  with([](kmx_bow_detect_params& p) { p.max_db_results = INT32_MAX; }, "max_db_results");
  with([](kmx_bow_detect_params& p) { p.max_db_results = 1; }, "");
  with([](kmx_bow_detect_params& p) { p.max_db_results = 256; }, "");
  with([](kmx_bow_detect_params& p) { p.use_nss = 2; }, "use_nss");
  with([](kmx_bow_detect_params& p) { p.use_nss = -1; }, "use_nss");
  with([](kmx_bow_detect_params& p) { p.use_nss = 0; }, "");
  with([&](kmx_bow_detect_params& p) { p.alpha = inf; }, "alpha");
  with([&](kmx_bow_detect_params& p) { p.alpha = -inf; }, "alpha");
  with([&](kmx_bow_detect_params& p) { p.alpha = nan; }, "alpha");
  with([](kmx_bow_detect_params& p) { p.alpha = 0.0; }, "");
  with([&](kmx_bow_detect_params& p) { p.min_nss_factor = nan; }, "min_nss_factor");
  with([&](kmx_bow_detect_params& p) { p.min_nss_factor = inf; }, "min_nss_factor");
  with([](kmx_bow_detect_params& p) { p.recent_frames_window = -1; }, "recent_frames_window");
  with([](kmx_bow_detect_params& p) { p.recent_frames_window = 0; }, "");
  with([](kmx_bow_detect_params& p) { p.max_intraisland_gap = -3; }, "max_intraisland_gap");
  with([](kmx_bow_detect_params& p) { p.min_matches_per_island = INT32_MIN; }, "min_matches_per_island");
  with([](kmx_bow_detect_params& p) { p.max_nrFrames_between_queries = -1; }, "max_nrFrames_between_queries");
  with([](kmx_bow_detect_params& p) { p.max_nrFrames_between_queries = 0; }, "");
  with([](kmx_bow_detect_params& p) { p.max_nrFrames_between_islands = -1; }, "max_nrFrames_between_islands");
  with([](kmx_bow_detect_params& p) { p.min_temporal_matches = -1; }, "min_temporal_matches");
  with([](kmx_bow_detect_params& p) { p.min_temporal_matches = 0; }, "");
  // the result counts of kmx_bow_decide_results, in an array of exactly nq
  expect_counts(7, {}, KMX_OK, "");
  expect_counts(7, {0, 7, 3}, KMX_OK, "");
  expect_counts(7, {0, 8, 3}, KMX_EINVAL, "outside [0, K]");
  expect_counts(7, {0, 7, -1}, KMX_EINVAL, "outside [0, K]");
  expect_counts(0, {0}, KMX_EINVAL, "K must be");
  expect_counts(257, {0}, KMX_EINVAL, "K must be");
  expect_counts(256, {256}, KMX_OK, "");
  {
    std::string err;
    if (kmx::bow_check_result_counts(3, 7, 256, nullptr, &err) != KMX_EINVAL ||
        kmx::bow_check_result_counts(-1, 7, 256, nullptr, &err) != KMX_EINVAL ||
        kmx::bow_check_result_counts((int64_t)INT32_MAX, 7, 256, nullptr, &err) != KMX_EINVAL) {
      std::fprintf(stderr, "null or absurd result counts were not refused\n");
      ++g_fail;
    }
  }
  if (g_fail) {
    std::fprintf(stderr, "bow_check: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("bow_check ok: %d random batches, malformed batches rejected; %d parameter sets\n", batches, n_params);
  return 0;
}
