// project_check.cpp — so3_project.h (the nearest rotation of k_traj and of the
// chordal initialisation) as a stand-alone program, built by `make
// project_check` with the host address and undefined-behaviour sanitizers. It
// runs so3_project_block on the exact cases of tests/golden/make_rounding_ref.py
// (rank 2 under signed permutations, rank 1, the zero block, the identity, the
// reflections) and on a generated ladder of singular value ratios down to
// 1e-300 with both determinant signs and scales from 1e-150 to 1e150, and
// asserts that every result is finite, orthogonal to 64 eps and of determinant
// +1, and that the well-conditioned ones are the known rotation. CPU only.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "so3_project.h"

namespace {

int g_fail = 0;

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "project_check.cpp:%d: %s\n", __LINE__, #cond);  \
      ++g_fail;                                                             \
    }                                                                       \
  } while (0)

const double EPS = 2.220446049250313e-16;

struct M3 {
  double a[3][3];
};

M3 mul(const M3& x, const M3& y) {
  M3 z{};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      for (int k = 0; k < 3; ++k) z.a[i][j] += x.a[i][k] * y.a[k][j];
  return z;
}

M3 transpose(const M3& x) {
  M3 z{};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) z.a[i][j] = x.a[j][i];
  return z;
}

double det(const M3& x) {
  return x.a[0][0] * (x.a[1][1] * x.a[2][2] - x.a[1][2] * x.a[2][1]) -
         x.a[0][1] * (x.a[1][0] * x.a[2][2] - x.a[1][2] * x.a[2][0]) +
         x.a[0][2] * (x.a[1][0] * x.a[2][1] - x.a[1][1] * x.a[2][0]);
}

M3 diag(double a, double b, double c) {
  M3 z{};
  z.a[0][0] = a;
  z.a[1][1] = b;
  z.a[2][2] = c;
  return z;
}

M3 project(const M3& m) {
  double in[9], out[3][3];
  for (int i = 0; i < 9; ++i) in[i] = m.a[i / 3][i % 3];
  kmx::so3_project_block(in, out);
  M3 z{};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) z.a[i][j] = out[i][j];
  return z;
}

// finite, R^T R = I to 64 eps, det R = +1
bool is_rotation(const M3& r) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      if (!std::isfinite(r.a[i][j])) return false;
  const M3 g = mul(transpose(r), r);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      if (std::fabs(g.a[i][j] - (i == j ? 1.0 : 0.0)) > 64 * EPS) return false;
  return std::fabs(det(r) - 1.0) <= 64 * EPS;
}

double max_diff(const M3& x, const M3& y) {
  double d = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) d = std::fmax(d, std::fabs(x.a[i][j] - y.a[i][j]));
  return d;
}

// signed permutation: row i has s[i] in column p[i]
M3 perm(int p0, int p1, int p2, double s0, double s1, double s2) {
  M3 z{};
  z.a[0][p0] = s0;
  z.a[1][p1] = s1;
  z.a[2][p2] = s2;
  return z;
}

uint64_t g_state = 0x9e3779b97f4a7c15ull;
double uniform() {  // xorshift64*, in (-1, 1)
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (double)((g_state * 0x2545f4914f6cdd1dull) >> 11) / 4503599627370496.0 - 1.0;
}

// a rotation from a random unit quaternion
M3 random_rotation() {
  double q[4], n = 0.0;
  do {
    n = 0.0;
    for (double& x : q) {
      x = uniform();
      n += x * x;
    }
  } while (n < 1e-3 || n > 1.0);
  n = std::sqrt(n);
  const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  M3 r{};
  r.a[0][0] = 1 - 2 * (y * y + z * z); r.a[0][1] = 2 * (x * y - z * w); r.a[0][2] = 2 * (x * z + y * w);
  r.a[1][0] = 2 * (x * y + z * w); r.a[1][1] = 1 - 2 * (x * x + z * z); r.a[1][2] = 2 * (y * z - x * w);
  r.a[2][0] = 2 * (x * z - y * w); r.a[2][1] = 2 * (y * z + x * w); r.a[2][2] = 1 - 2 * (x * x + y * y);
  return r;
}

void exact_cases() {
  const M3 d = diag(1.0, 0.5, 0.0);
  // rank 2 with distinct singular values: the answer is P diag(1, 1, +-1) Q, a signed permutation of det +1
  const M3 P[4] = {perm(0, 1, 2, 1, 1, 1), perm(1, 2, 0, 1, -1, 1), perm(2, 1, 0, -1, 1, 1), perm(0, 2, 1, 1, 1, -1)};
  const M3 Q[4] = {perm(0, 1, 2, 1, 1, 1), perm(2, 0, 1, 1, 1, 1), perm(0, 2, 1, 1, -1, -1), perm(1, 0, 2, -1, 1, 1)};
  for (int k = 0; k < 4; ++k) {
    const M3 r = project(mul(mul(P[k], d), Q[k]));
    CHECK(is_rotation(r));
    const double s = det(P[k]) * det(Q[k]);
    CHECK(max_diff(r, mul(mul(P[k], diag(1.0, 1.0, s)), Q[k])) <= 64 * EPS);
  }
  M3 a{{{1, 2, 3}, {2, 4, 6}, {1, 0, 1}}};
  M3 na = a;
  for (auto& row : na.a)
    for (double& x : row) x = -x;
  const M3 ra = project(a), rn = project(na);
  CHECK(is_rotation(ra));
  CHECK(is_rotation(rn));
  // rank 1: any completion, but R v1 = u1 (u1 = (1, 2, 3) / sqrt 14 = v1)
  const M3 r1 = project(M3{{{1, 2, 3}, {2, 4, 6}, {3, 6, 9}}});
  CHECK(is_rotation(r1));
  const double u[3] = {1 / std::sqrt(14.0), 2 / std::sqrt(14.0), 3 / std::sqrt(14.0)};
  for (int i = 0; i < 3; ++i) CHECK(std::fabs(r1.a[i][0] * u[0] + r1.a[i][1] * u[1] + r1.a[i][2] * u[2] - u[i]) <= 64 * EPS);
  CHECK(max_diff(project(M3{}), diag(1, 1, 1)) == 0.0);  // the zero block gives I
  CHECK(max_diff(project(diag(1, 1, 1)), diag(1, 1, 1)) == 0.0);
  CHECK(max_diff(project(diag(-1.0 / 9, -3.0 / 9, -5.0 / 9)), diag(1, -1, -1)) <= 64 * EPS);
  CHECK(max_diff(project(diag(1.0 / 9, -3.0 / 9, -5.0 / 9)), diag(1, -1, -1)) <= 64 * EPS);
  // non-finite input: the identity, not a fault
  M3 bad = diag(1, 1, 1);
  bad.a[1][2] = INFINITY;
  CHECK(max_diff(project(bad), diag(1, 1, 1)) == 0.0);
}

void ladder() {
  const double ratio[] = {1.0, 0.5, 1e-2, 1e-4, 1e-6, 1e-8, 1e-12, 1e-16, 1e-30, 1e-100, 1e-300, 0.0};
  const double scale[] = {1.0, 3e3, 1e-3, 1e150, 1e-150};
  for (double s3 : ratio)
    for (double s2 : {0.9, 0.3, 1e-5})
      for (double sc : scale)
        for (double sign : {1.0, -1.0})
          for (int draw = 0; draw < 4; ++draw) {
            if (s3 > s2) continue;
            const M3 U = random_rotation(), V = random_rotation();
            const M3 m = mul(mul(U, diag(sc, sc * s2, sign * sc * s3)), transpose(V));
            const M3 r = project(m);
            CHECK(is_rotation(r));
            // U and V are rotations, so the nearest rotation is U V^T for either sign (the SVD's
            // U diag(1, 1, sign) carries it); sigma2 - sigma3 >= 0.1 sigma1 bounds its condition
            if (s2 - s3 >= 0.1) CHECK(max_diff(r, mul(U, transpose(V))) <= 1e-13);
          }
}

}  // namespace

int main() {
  exact_cases();
  ladder();
  if (g_fail) {
    std::fprintf(stderr, "project_check: %d failure(s)\n", g_fail);
    return 1;
  }
  std::puts("project_check ok");
  return 0;
}
