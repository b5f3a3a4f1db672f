// The nearest rotation to a 3x3 block, shared by chordal.hip (k_ch_project*)
// and pgo.hip (k_traj). Host and device: project_check.cpp runs it on the CPU
// under the host sanitizers.
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define KMX_HD __host__ __device__
#define KMX_FORCEINLINE __forceinline__
#else
#define KMX_HD
#define KMX_FORCEINLINE inline __attribute__((always_inline))
#endif

namespace kmx {

KMX_HD inline void so3_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// A unit vector orthogonal to the unit vector u: the axis u is least along, made orthogonal.
KMX_HD inline void so3_any_orthogonal(const double* u, double* v) {
  int e = 0;
  if (fabs(u[1]) < fabs(u[e])) e = 1;
  if (fabs(u[2]) < fabs(u[e])) e = 2;
  double w[3] = {0.0, 0.0, 0.0};
  w[e] = 1.0;
  const double dot = u[e];
  double nn = 0.0;
  for (int k = 0; k < 3; ++k) {
    w[k] -= dot * u[k];
    nn += w[k] * w[k];
  }
  nn = sqrt(nn);
  for (int k = 0; k < 3; ++k) v[k] = w[k] / nn;
}

// v orthogonal to the unit vector u, and unit (one Gram-Schmidt step)
KMX_HD inline void so3_orthonormalize(const double* u, double* v) {
  double dot = 0.0, nn = 0.0;
  for (int k = 0; k < 3; ++k) dot += u[k] * v[k];
  for (int k = 0; k < 3; ++k) {
    v[k] -= dot * u[k];
    nn += v[k] * v[k];
  }
  nn = sqrt(nn);
  for (int k = 0; k < 3; ++k) v[k] /= nn;
}

// The nearest rotation to the row-major 3x3 block Xin, as project_so3: with
// the SVD M = U S V^T, R = U diag(1, 1, det(U V^T)) V^T. One-sided Jacobi turns
// the columns of A = M V orthogonal (V a product of plane rotations); with u1,
// u2 and v1, v2 the directions of the two largest singular values,
//   R = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T,
// since det(U V^T) u3 v3^T = (u1 x u2)(v1 x v2)^T whatever the signs of u3 and
// v3: the determinant fix lands on the smallest singular direction and the
// smallest singular value is never divided by. A block of rank < 2 has no
// unique projection; the missing directions are completed so that the result
// is a rotation (the zero block gives I, as numpy's SVD does).
KMX_HD KMX_FORCEINLINE void so3_project_block(const double* __restrict__ Xin, double Rm[3][3]) {
  double A[3][3], Vm[3][3];
  double amax = 0.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      A[r][c] = Xin[3 * r + c];
      Vm[r][c] = r == c ? 1.0 : 0.0;
      amax = fmax(amax, fabs(A[r][c]));
      Rm[r][c] = r == c ? 1.0 : 0.0;
    }
  if (amax > 0.0 && amax < INFINITY) {
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) A[r][c] /= amax;  // the projection does not depend on the scale
    for (int sweep = 0; sweep < 30; ++sweep) {
      bool rotated = false;
      for (int i = 0; i < 2; ++i)
        for (int j = i + 1; j < 3; ++j) {
          double aii = 0.0, ajj = 0.0, aij = 0.0;
          for (int r = 0; r < 3; ++r) {
            aii += A[r][i] * A[r][i];
            ajj += A[r][j] * A[r][j];
            aij += A[r][i] * A[r][j];
          }
          if (fabs(aij) <= 1e-17 * sqrt(aii * ajj) || aij == 0.0) continue;
          rotated = true;
          const double zeta = (ajj - aii) / (2.0 * aij);
          const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
          for (int r = 0; r < 3; ++r) {
            const double ai = A[r][i], aj = A[r][j];
            A[r][i] = cs * ai - sn * aj;
            A[r][j] = sn * ai + cs * aj;
            const double vi = Vm[r][i], vj = Vm[r][j];
            Vm[r][i] = cs * vi - sn * vj;
            Vm[r][j] = sn * vi + cs * vj;
          }
        }
      if (!rotated) break;
    }
    double s2[3];
    for (int c = 0; c < 3; ++c) s2[c] = A[0][c] * A[0][c] + A[1][c] * A[1][c] + A[2][c] * A[2][c];
    int c1 = 0;
    if (s2[1] > s2[c1]) c1 = 1;
    if (s2[2] > s2[c1]) c1 = 2;
    int c2 = c1 == 0 ? 1 : 0;
    for (int c = 0; c < 3; ++c)
      if (c != c1 && s2[c] > s2[c2]) c2 = c;
    double u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
    const double n1 = sqrt(s2[c1]);
    for (int r = 0; r < 3; ++r) {
      u1[r] = A[r][c1] / n1;
      v1[r] = Vm[r][c1];
    }
    if (s2[c2] > 1e-280) {
      const double n2 = sqrt(s2[c2]);
      for (int r = 0; r < 3; ++r) {
        u2[r] = A[r][c2] / n2;
        v2[r] = Vm[r][c2];
      }
      so3_orthonormalize(u1, u2);
      so3_orthonormalize(v1, v2);
    } else {
      so3_any_orthogonal(u1, u2);
      so3_any_orthogonal(v1, v2);
    }
    so3_cross(u1, u2, u3);
    so3_cross(v1, v2, v3);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) Rm[r][c] = u1[r] * v1[c] + u2[r] * v2[c] + u3[r] * v3[c];
  }
}

}  // namespace kmx
