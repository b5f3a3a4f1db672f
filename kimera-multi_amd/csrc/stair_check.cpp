// stair_check.cpp — the host half of kmx_cert_escape (cert_host.h: the
// argument checks over ladders of step lengths and directions, and the choice
// rule) as a stand-alone program, built by `make stair_check` with the host
// address and undefined-behaviour sanitizers. Every array is passed in a
// vector of exactly the stated size, so a read past one is a report. CPU only.
#include <cstdio>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "cert_host.h"

namespace {

int g_fail = 0;
const double kNaN = std::numeric_limits<double>::quiet_NaN();
const double kInf = std::numeric_limits<double>::infinity();

void expect_check(const std::vector<double>& alpha, int32_t n_alpha, const std::vector<double>& y, int code,
                  const char* what, const char* name) {
  std::vector<double> a(alpha), v(y);  // exact-size copies
  std::string err;
  const int rc = kmx::cert_escape_check(n_alpha, a.empty() ? nullptr : a.data(), v.size(),
                                        v.empty() ? nullptr : v.data(), &err);
  if (rc != code || (code != KMX_OK && err.find(what) == std::string::npos)) {
    std::fprintf(stderr, "%s: expected %d (%s), got %d (%s)\n", name, code, what, rc, err.c_str());
    ++g_fail;
  }
}

void expect_choice(const std::vector<double>& cost, double cost0, int32_t want, const char* name) {
  std::vector<double> c(cost);
  const int32_t got = kmx::cert_escape_choose((int32_t)c.size(), c.empty() ? nullptr : c.data(), cost0);
  if (got != want) {
    std::fprintf(stderr, "%s: expected candidate %d, got %d\n", name, want, got);
    ++g_fail;
  }
}

std::vector<double> ladder(int k) {  // 2^-j, j = 0 .. k-1
  std::vector<double> a((size_t)k);
  double v = 1.0;
  for (int j = 0; j < k; ++j, v *= 0.5) a[(size_t)j] = v;
  return a;
}

}  // namespace

int main() {
  int checks = 0, choices = 0;
  const std::vector<double> y(4 * 5, 0.25);
  // the ladder and the direction
  for (int k = 1; k <= kmx::CT_MAX_ALPHA; ++k, ++checks) expect_check(ladder(k), k, y, KMX_OK, "", "a ladder of 1..8");
  expect_check({0.0}, 1, y, KMX_OK, "", "alpha = 0");
  expect_check({-1.0, 1e300, 1e-300}, 3, y, KMX_OK, "", "negative, huge and tiny step lengths");
  expect_check(ladder(1), 1, {}, KMX_EINVAL, "null", "null y");
  expect_check({}, 1, y, KMX_EINVAL, "null", "null alpha");
  expect_check({}, 0, y, KMX_EINVAL, "n_alpha", "n_alpha == 0");
  expect_check(ladder(9), 9, y, KMX_EINVAL, "n_alpha", "n_alpha == 9");
  expect_check(ladder(2), -3, y, KMX_EINVAL, "n_alpha", "n_alpha < 0");
  expect_check({1.0, kNaN}, 2, y, KMX_EINVAL, "alpha not finite", "NaN in alpha");
  expect_check({kInf}, 1, y, KMX_EINVAL, "alpha not finite", "inf in alpha");
  checks += 9;
  {
    std::vector<double> v(y);
    v.back() = kNaN;
    expect_check(ladder(8), 8, v, KMX_EINVAL, "y not finite", "NaN in the last entry of y");
    v = y;
    v.front() = -kInf;
    expect_check(ladder(8), 8, v, KMX_EINVAL, "y not finite", "-inf in y");
    // only the first n_alpha step lengths are read
    std::vector<double> a = ladder(3);
    a.push_back(kNaN);
    expect_check(a, 3, y, KMX_OK, "", "a NaN behind the ladder's end");
    checks += 3;
  }
  // the choice rule
  expect_choice({5.0, 3.0, 4.0}, 10.0, 1, "the lowest descending candidate");
  expect_choice({3.0, 5.0, 3.0}, 10.0, 0, "a tie goes to the earlier index");
  expect_choice({10.0, 11.0, 12.0}, 10.0, -1, "equal to the point's cost is no descent");
  expect_choice({11.0, 9.0, 12.0}, 10.0, 1, "one candidate descends");
  expect_choice({kNaN, 9.0, kNaN}, 10.0, 1, "a NaN cost is never chosen");
  expect_choice({kNaN, kNaN}, 10.0, -1, "only NaN costs");
  expect_choice({-kInf, 9.0}, 10.0, 1, "-inf is not finite: not chosen");
  expect_choice({kInf}, 10.0, -1, "+inf does not descend");
  expect_choice({1.0}, kNaN, -1, "a point cost that is NaN: nothing is chosen");
  expect_choice({-2.0, -3.0}, -1.0, 1, "negative costs");
  expect_choice({0.0}, 0.0, -1, "zero against zero");
  expect_choice({}, 1.0, -1, "no candidates");
  choices += 12;
  // against a plain restatement on random costs with ties and NaNs
  std::mt19937 rng(99);
  for (int rep = 0; rep < 2000; ++rep, ++choices) {
    const int k = 1 + (int)(rng() % kmx::CT_MAX_ALPHA);
    std::vector<double> c((size_t)k);
    for (double& v : c) {
      const unsigned q = rng() % 10;
      v = q == 0 ? kNaN : q == 1 ? kInf : (double)(rng() % 7);  // few values: ties are common
    }
    const double c0 = (double)(rng() % 7);
    int32_t want = -1;
    for (int j = 0; j < k; ++j) {
      if (!(c[(size_t)j] < c0) || !std::isfinite(c[(size_t)j])) continue;
      if (want < 0 || c[(size_t)j] < c[(size_t)want]) want = j;
    }
    expect_choice(c, c0, want, "random costs");
  }
  if (g_fail) {
    std::fprintf(stderr, "stair_check: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("stair_check ok: %d argument checks, %d choices\n", checks, choices);
  return 0;
}
