// lcd_check.cpp — lcd.hip's host code (lcd_host.h: the CSR check of
// kmx_lcd_verify_matches, the staging layouts of the small synchronous calls,
// the opengv sampler tables and the spread form's range schedule) as a
// stand-alone program, built by `make lcd_check` with the host address and
// undefined-behaviour sanitizers. Malformed correspondences come in arrays of
// exactly the promised size, so a read past either is a report. CPU only.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "lcd_host.h"

namespace {

int g_fail = 0;
#define EXPECT(cond, ...)                  \
  do {                                     \
    if (!(cond)) {                         \
      std::fprintf(stderr, __VA_ARGS__);   \
      std::fprintf(stderr, "\n");          \
      ++g_fail;                            \
    }                                      \
  } while (0)

// A pool of three frames with 4, 7 and 0 features; candidate i is (cq[i], cm[i]).
const int kNfeat[3] = {4, 7, 0};

// iq / im hold exactly mptr.back() - 0 entries as promised by a well-formed
// mptr (entries before mptr[0] are never the call's); `null_idx`: pass null.
void expect_csr(int N, const std::vector<int64_t>& mptr, const std::vector<int32_t>& cq, const std::vector<int32_t>& cm,
                const std::vector<int32_t>& iq, const std::vector<int32_t>& im, int code, const char* what,
                bool null_idx = false) {
  std::vector<int64_t> mp(mptr);  // exact-size copies
  std::vector<int32_t> q(iq), m(im), a(cq), b(cm);
  std::string err;
  const int n = (int)mp.size() - 1;
  const int rc = kmx::lcd_check_csr(n, N, mp.data(), null_idx ? nullptr : q.data(), null_idx ? nullptr : m.data(),
                                    a.data(), b.data(), kNfeat, &err);
  EXPECT(rc == code && (code == KMX_OK || err.find(what) != std::string::npos), "csr: expected %d (%s), got %d (%s)",
         code, what, rc, err.c_str());
}

void check_csr() {
  const char* structure = "more pairs than max_feats (or mptr decreases)";
  const char* index = "outside its frame's features";
  // accepted: empty candidates (null arrays too), base > 0, exactly N pairs, repeated indices
  expect_csr(4, {0, 0, 0}, {0, 1}, {1, 0}, {}, {}, KMX_OK, "");
  expect_csr(4, {0, 0, 0}, {0, 1}, {1, 0}, {}, {}, KMX_OK, "", true);
  expect_csr(4, {7, 7}, {0}, {1}, {}, {}, KMX_OK, "", true);
  expect_csr(4, {0, 2, 2, 3}, {0, 2, 1}, {1, 2, 0}, {0, 3, 6}, {6, 0, 3}, KMX_OK, "");
  expect_csr(4, {2, 4}, {0}, {1}, {-9, 99, 1, 2}, {-9, 99, 5, 6}, KMX_OK, "");  // entries before base are not read
  expect_csr(4, {0, 4}, {0}, {1}, {0, 1, 2, 3}, {3, 4, 5, 6}, KMX_OK, "");      // K == N
  expect_csr(4, {0, 3}, {0}, {1}, {1, 1, 1}, {2, 2, 2}, KMX_OK, "");            // repeated indices
  // rejected on structure, before an index is read
  expect_csr(4, {-1, 2}, {0}, {1}, {0, 1}, {0, 1}, KMX_EINVAL, "mptr[0] < 0");
  expect_csr(8, {0, 5, 0}, {0, 0}, {1, 1}, {}, {}, KMX_EINVAL, structure, true);  // total 0, null arrays
  expect_csr(8, {0, 5, 0}, {0, 0}, {1, 1}, {}, {}, KMX_EINVAL, structure);        // total 0, empty arrays
  expect_csr(4, {0, 3, 2, 4}, {0, 0, 0}, {1, 1, 1}, {0, 1, 2, 3}, {0, 1, 2, 3}, KMX_EINVAL, structure);  // the middle
  expect_csr(4, {0, 2, 1}, {0, 0}, {1, 1}, {0}, {0}, KMX_EINVAL, structure);                             // the end
  expect_csr(4, {0, 5}, {0}, {1}, {0, 1, 2, 3, 0}, {0, 1, 2, 3, 4}, KMX_EINVAL, structure);  // K = N + 1
  expect_csr(4, {0, 1, INT64_MAX}, {0, 0}, {1, 1}, {0}, {0}, KMX_EINVAL, structure);
  // rejected on an index: equal to its frame's n_feats (query, match), negative
  expect_csr(8, {0, 2}, {0}, {1}, {0, 4}, {0, 1}, KMX_EINVAL, index);
  expect_csr(8, {0, 2}, {0}, {1}, {0, 3}, {7, 1}, KMX_EINVAL, index);
  expect_csr(8, {0, 2}, {0}, {1}, {0, -1}, {0, 1}, KMX_EINVAL, index);
  expect_csr(8, {0, 2}, {0}, {1}, {0, 1}, {0, INT32_MIN}, KMX_EINVAL, index);
  expect_csr(8, {0, 0, 1}, {0, 2}, {1, 1}, {0}, {0}, KMX_EINVAL, index);  // a frame without features
  // null index arrays with a positive total, null mptr
  expect_csr(8, {0, 1, 3}, {0, 0}, {1, 1}, {}, {}, KMX_EINVAL, "null i_query / i_match", true);
  std::string err;
  const int32_t c0[1] = {0};
  EXPECT(kmx::lcd_check_csr(1, 8, nullptr, nullptr, nullptr, c0, c0, kNfeat, &err) == KMX_EINVAL, "null mptr accepted");
  EXPECT(kmx::lcd_check_csr(0, 8, nullptr, nullptr, nullptr, nullptr, nullptr, kNfeat, &err) == KMX_OK, "n = 0");
  // the candidates' frame ids, in arrays of exactly n
  const std::vector<int32_t> ok{0, 2, 1}, hi{0, 3, 1}, neg{0, -1, 1};
  EXPECT(kmx::lcd_check_cands(3, 3, ok.data(), ok.data(), &err) == KMX_OK, "cands ok");
  EXPECT(kmx::lcd_check_cands(3, 3, hi.data(), ok.data(), &err) == KMX_EINVAL, "cq == F accepted");
  EXPECT(kmx::lcd_check_cands(3, 3, ok.data(), neg.data(), &err) == KMX_EINVAL, "cm < 0 accepted");
  EXPECT(kmx::lcd_check_cands(0, 3, nullptr, nullptr, &err) == KMX_OK, "no cands");
}

void check_params() {
  kmx_lcd_params good{};
  good.ransac_max_iterations = 500;
  std::string err;
  EXPECT(kmx::lcd_check_params(&good, &err) == KMX_OK, "params: %s", err.c_str());
  EXPECT(kmx::lcd_check_params(nullptr, &err) == KMX_EINVAL, "null params accepted");
  auto with = [&](auto set, int code) {
    kmx_lcd_params p = good;
    set(p);
    EXPECT(kmx::lcd_check_params(&p, &err) == code, "params: expected %d (last message: %s)", code, err.c_str());
  };
  with([](kmx_lcd_params& p) { p.norm = 2; }, KMX_EINVAL);
  with([](kmx_lcd_params& p) { p.norm = KMX_NORM_HAMMING; }, KMX_OK);
  with([](kmx_lcd_params& p) { p.rng_variant = -1; }, KMX_EINVAL);
  with([](kmx_lcd_params& p) { p.ransac_randomize = 1; }, KMX_EUNSUP);
  with([](kmx_lcd_params& p) { p.use_1point_3d3d = 2; }, KMX_EINVAL);
  with([](kmx_lcd_params& p) { p.algorithm_2d2d = 2; }, KMX_EUNSUP);
  with([](kmx_lcd_params& p) { p.algorithm_2d2d = KMX_ALGO_NISTER; }, KMX_OK);
  with([](kmx_lcd_params& p) { p.ransac_max_iterations = 0; }, KMX_EINVAL);
  with([](kmx_lcd_params& p) { p.rng_stream = 2; }, KMX_EINVAL);
  good.ransac_max_iterations = 1;
  EXPECT(kmx::lcd_pmax(good) == 12, "pmax(1)");
  good.ransac_max_iterations = 500;
  EXPECT(kmx::lcd_pmax(good) == 5501, "pmax(500)");
}

// Regions (offset, bytes) in the block's order: each 16-aligned, none
// overlapping the next, the last ending at `total`.
void expect_regions(const std::vector<std::pair<size_t, size_t>>& r, size_t total, const char* what, int n) {
  for (size_t i = 0; i < r.size(); ++i) {
    EXPECT(r[i].first % 16 == 0, "%s n=%d: region %zu at %zu is not 16-aligned", what, n, i, r[i].first);
    const size_t end = r[i].first + r[i].second, next = i + 1 < r.size() ? r[i + 1].first : total;
    EXPECT(end <= next, "%s n=%d: region %zu ends at %zu, past %zu", what, n, i, end, next);
  }
  EXPECT(r.back().first + r.back().second == total, "%s n=%d: total %zu is not the last end", what, n, total);
}

void check_layouts() {
  for (int n : {1, 8, 64, 1025})
    for (int N : {5, 64, 97, 1024}) {
      const kmx::LcdMatchLayout M = kmx::lcd_match_layout(n, N);
      const size_t ids = sizeof(int32_t) * (size_t)n;
      // the block ends with K's padded extent (it is reserved whole)
      expect_regions({{M.o_cq, ids}, {M.o_cm, ids}, {M.o_pairs, 8 * (size_t)n * N}, {M.o_K, kmx::al16(ids)}}, M.total,
                     "match", n);
      for (size_t total : {(size_t)0, (size_t)1, (size_t)n * N})
        for (int prior = 0; prior < 2; ++prior)
          for (int masks = 0; masks < 2; ++masks) {
            const kmx::LcdVerifyLayout L = kmx::lcd_verify_layout(n, N, total, prior != 0, masks != 0);
            const size_t pr = prior ? sizeof(double) * 12 * n : 0;
            EXPECT(L.in_bytes == L.o_prior + pr && L.in_bytes <= L.o_res, "verify n=%d: inputs' extent", n);
            // the results' region is reserved to its padded end, where the (possibly empty) masks start
            expect_regions({{L.o_mptr, sizeof(int64_t) * ((size_t)n + 1)}, {L.o_cq, ids}, {L.o_cm, ids},
                            {L.o_iq, sizeof(int32_t) * total}, {L.o_im, sizeof(int32_t) * total}, {L.o_prior, pr},
                            {L.o_res, sizeof(kmx_lcd_result) * (size_t)n}, {L.o_mask, masks ? (size_t)n * N : 0}},
                           L.total, "verify", n);
          }
    }
}

void check_sampler() {
  for (int variant : {KMX_RNG_GCC9, KMX_RNG_GCC11})
    for (int S : {5, 3, 6}) {
      const int pmax = 78;
      for (int K : {S, S + 1, 300}) {
        std::mt19937 rng(12345);
        std::vector<short> row((size_t)pmax * S);  // exactly pmax passes
        kmx::sample_row(rng, variant, K, pmax, S, row.data());
        for (int p = 0; p < pmax; ++p) {
          std::set<short> seen;
          for (int i = 0; i < S; ++i) {
            const short v = row[(size_t)p * S + i];
            EXPECT(v >= 0 && v < K, "sample_row S=%d K=%d: index %d", S, K, (int)v);
            seen.insert(v);
          }
          EXPECT((int)seen.size() == S, "sample_row S=%d K=%d pass %d: repeated index", S, K, p);
        }
      }
      // tables: N = 40 builds on one thread, N = 300 on eight; each row is
      // sample_row from a freshly seeded engine (the serial build)
      kmx_lcd_params P{};
      P.ransac_seed = 12345;
      P.rng_variant = variant;
      std::vector<short> t40, t300, row((size_t)pmax * S);
      kmx::build_table(P, 40, pmax, t40, S);
      kmx::build_table(P, 300, pmax, t300, S);
      EXPECT(t40.size() == (size_t)(40 - S + 1) * pmax * S && t300.size() == (size_t)(300 - S + 1) * pmax * S,
             "table sizes");
      for (int K = S; K <= 300; ++K) {
        std::mt19937 rng(P.ransac_seed);
        kmx::sample_row(rng, variant, K, pmax, S, row.data());
        const size_t at = (size_t)(K - S) * pmax * S, bytes = sizeof(short) * row.size();
        EXPECT(std::memcmp(t300.data() + at, row.data(), bytes) == 0, "table(300) row K=%d S=%d", K, S);
        if (K <= 40) EXPECT(std::memcmp(t40.data() + at, row.data(), bytes) == 0, "table(40) row K=%d S=%d", K, S);
      }
      // N < S: the one zero row, nothing drawn
      std::vector<short> t0;
      kmx::build_table(P, S - 1, pmax, t0, S);
      EXPECT(t0 == std::vector<short>((size_t)pmax * S, 0), "N < S: not the one zero row (S=%d)", S);
    }
}

// The schedule as ransac_spread drives it, every range answering "more".
int check_schedule() {
  int cases = 0;
  for (int n : {1, 2, 3, 4, 5, 6, 7, 8, 64})
    for (int per_max : {kmx::SG, kmx::SPREAD_PER_NISTER})
      for (int pmax : {12, 78, 5501, 5511}) {
        int pa = 0, range = kmx::spread_first_range(n), it = 0;
        EXPECT(range == ((int64_t)n * 510 <= kmx::SPREAD_WAVES ? 510 : 66), "first range n=%d", n);
        for (; pa < pmax; ++it) {
          EXPECT(it < pmax + 1, "n=%d pmax=%d: range index %d reaches d_more's capacity", n, pmax, it);
          const kmx::SpreadStep s = kmx::spread_step(n, pa, range, per_max, pmax);
          EXPECT(s.per >= 1 && s.per <= per_max && s.G >= 1, "n=%d: per %d G %d", n, s.per, s.G);
          EXPECT((int64_t)n * s.G <= kmx::SPREAD_WAVES, "n=%d: %d waves", n, n * s.G);
          EXPECT(s.pb > pa && s.pb <= pmax, "n=%d pmax=%d: range [%d, %d)", n, pmax, pa, s.pb);
          if (s.pb <= pa) break;  // (reported; do not spin)
          pa = s.pb;
          range = kmx::spread_next_range(pa);
          EXPECT(range == (pa < 510 ? 510 - pa : 1500) && range > 0, "next range at %d", pa);
        }
        EXPECT(pa == pmax, "n=%d pmax=%d: the loop ends at %d", n, pmax, pa);
        ++cases;
      }
  return cases;
}

}  // namespace

int main() {
  check_csr();
  check_params();
  check_layouts();
  check_sampler();
  const int cases = check_schedule();
  if (g_fail) {
    std::fprintf(stderr, "lcd_check: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("lcd_check ok: malformed correspondences rejected, layouts, sampler tables, %d schedules\n", cases);
  return 0;
}
