"""High-precision reference for the 5-point relative-pose problem (mpmath).

Written from the published formulation (Nister 2004; Stewenius, Engels,
Nister 2006), independently of the restatement's text:

  1. the 5 x 9 system  f1_i^T E f2_i = 0  has a four-dimensional null space
     X, Y, Z, W (orthonormal, from a Householder QR of its transpose);
  2. E = x X + y Y + z Z + W must satisfy det E = 0 and
     2 E E^T E - tr(E E^T) E = 0: ten cubics in x, y, z, expanded here by
     generic polynomial arithmetic (dicts exponent -> coefficient);
  3. Gauss-Jordan elimination of the 10 x 20 coefficient matrix in the
     graded order (ten cubic monomials first) leaves [I | B]; the rows of B
     give the 10 x 10 matrix of "multiply by x" on the quotient ring's basis
     {x^2, xy, y^2, xz, yz, z^2, x, y, z, 1};
  4. its eigenvectors (mp.eig) are that basis evaluated at the ten solutions.

Every solution comes back with its eigenvalue. `solve_with_condition` adds a
condition estimate kappa per solution: the largest change of the (unit
Frobenius norm, sign-free) solution under four random relative perturbations
of every input component by 2^-40, divided by 2^-40.

40 digits by default. A problem whose answer is decided by the rounding of its
inputs (zero baseline: f1 = R f2 up to 1e-16, condition ~ 1e32) needs more:
there the solutions at 40 digits differ from those at 80 and 120 in the first
digit, while 80 and 120 agree to the last; the caller passes `dps`.
"""
from __future__ import annotations

from dataclasses import dataclass

import mpmath as mp
import numpy as np

DPS = 40
PERT = 2.0 ** -40

# graded order: cubics, then the quotient basis
_CUBIC = [(3, 0, 0), (2, 1, 0), (1, 2, 0), (0, 3, 0), (2, 0, 1), (1, 1, 1), (0, 2, 1), (1, 0, 2), (0, 1, 2), (0, 0, 3)]
_BASIS = [(2, 0, 0), (1, 1, 0), (0, 2, 0), (1, 0, 1), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
_MONO = _CUBIC + _BASIS


@dataclass
class Solution:
    E: np.ndarray        # 3 x 3, unit Frobenius norm (real part for a complex solution), rounded to double
    eig: complex         # eigenvalue of the action matrix (the solution's x)
    real: bool
    sep: float           # distance of eig to the nearest other eigenvalue
    kappa: float = float("nan")


def _padd(a, b, s=1):
    out = dict(a)
    for k, v in b.items():
        out[k] = out.get(k, 0) + s * v
    return out


def _pmul(a, b):
    out = {}
    for (i, j, k), u in a.items():
        for (l, m, n), v in b.items():
            key = (i + l, j + m, k + n)
            out[key] = out.get(key, 0) + u * v
    return out


def _pscale(a, s):
    return {k: s * v for k, v in a.items()}


def _system(f1, f2):
    """f1, f2: 5 x 3 nested lists of mpf. Returns the null-space basis N (4 x 9) and the ten cubics."""
    Q = mp.matrix(9, 5)
    for i in range(5):
        for a in range(3):
            for b in range(3):
                Q[3 * a + b, i] = f1[i][a] * f2[i][b]
    Qf, _ = mp.qr(Q, mode="full")
    N = [[Qf[r, 5 + c] for r in range(9)] for c in range(4)]  # X, Y, Z, W
    keys = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
    E = [[{keys[c]: N[c][3 * a + b] for c in range(4)} for b in range(3)] for a in range(3)]
    # det E
    def minor(r0, c0, r1, c1):
        return _padd(_pmul(E[r0][c0], E[r1][c1]), _pmul(E[r0][c1], E[r1][c0]), -1)
    det = _padd(_padd(_pmul(E[0][0], minor(1, 1, 2, 2)), _pmul(E[0][1], minor(1, 0, 2, 2)), -1),
                _pmul(E[0][2], minor(1, 0, 2, 1)))
    # 2 E E^T E - tr(E E^T) E
    EEt = [[{} for _ in range(3)] for _ in range(3)]
    for a in range(3):
        for b in range(a, 3):
            s = {}
            for c in range(3):
                s = _padd(s, _pmul(E[a][c], E[b][c]))
            EEt[a][b] = EEt[b][a] = s
    tr = _padd(_padd(EEt[0][0], EEt[1][1]), EEt[2][2])
    polys = [det]
    for a in range(3):
        for b in range(3):
            s = {}
            for c in range(3):
                s = _padd(s, _pmul(EEt[a][c], E[c][b]))
            polys.append(_padd(_pscale(s, 2), _pmul(tr, E[a][b]), -1))
    return N, polys


def _eigen_solutions(N, polys):
    """Returns a list of (eig, (x, y, z), E as 9 mpc, unnormalised)."""
    M = [[p.get(mono, mp.mpf(0)) for mono in _MONO] for p in polys]
    # Gauss-Jordan with partial pivoting on the cubic block
    for c in range(10):
        piv = max(range(c, 10), key=lambda r: abs(M[r][c]))
        M[c], M[piv] = M[piv], M[c]
        d = M[c][c]
        M[c] = [v / d for v in M[c]]
        for r in range(10):
            if r != c and M[r][c] != 0:
                f = M[r][c]
                M[r] = [u - f * v for u, v in zip(M[r], M[c])]
    A = mp.matrix(10, 10)
    # x * {x^2, xy, y^2, xz, yz, z^2} = cubics x^3, x^2y, xy^2, x^2z, xyz, xz^2
    for row, cub in enumerate([0, 1, 2, 4, 5, 7]):
        for j in range(10):
            A[row, j] = -M[cub][10 + j]
    A[6, 0] = 1  # x * x = x^2
    A[7, 1] = 1  # x * y = xy
    A[8, 3] = 1  # x * z = xz
    A[9, 6] = 1  # x * 1 = x
    lam, V = mp.eig(A)
    out = []
    for s in range(10):
        w = V[9, s]
        x, y, z = V[6, s] / w, V[7, s] / w, V[8, s] / w
        out.append((lam[s], (x, y, z), _combine(N, x, y, z)))
    return out


def _combine(N, x, y, z):
    return [x * N[0][i] + y * N[1][i] + z * N[2][i] + N[3][i] for i in range(9)]


def _newton(polys, xyz, tol):
    """Gauss-Newton on the ten cubics from a nearby start (real solutions):
    the perturbed problem's solution next to the unperturbed one. None if it
    does not settle."""
    v = [mp.re(c) for c in xyz]
    coef = [[p.get(m, 0) for m in _MONO] for p in polys]
    for _ in range(12):
        pw = [[mp.mpf(1), c, c * c, c * c * c] for c in v]
        val = [pw[0][i] * pw[1][j] * pw[2][k] for i, j, k in _MONO]
        dx = [i * pw[0][i - 1] * pw[1][j] * pw[2][k] if i else 0 for i, j, k in _MONO]
        dy = [j * pw[0][i] * pw[1][j - 1] * pw[2][k] if j else 0 for i, j, k in _MONO]
        dz = [k * pw[0][i] * pw[1][j] * pw[2][k - 1] if k else 0 for i, j, k in _MONO]
        JtJ = mp.matrix(3, 3)
        Jtr = mp.matrix(3, 1)
        for c in coef:
            r = mp.fdot(c, val)
            g = [mp.fdot(c, dx), mp.fdot(c, dy), mp.fdot(c, dz)]
            for a in range(3):
                Jtr[a] += g[a] * r
                for b in range(3):
                    JtJ[a, b] += g[a] * g[b]
        try:
            d = mp.lu_solve(JtJ, Jtr)
        except ZeroDivisionError:
            return None
        v = [v[a] - d[a] for a in range(3)]
        if max(abs(d[a]) for a in range(3)) <= tol * max(1, max(abs(c) for c in v)):
            return v
    return None


def _unit_real(Ev):
    e = [mp.re(v) for v in Ev]
    n = mp.sqrt(sum(v * v for v in e))
    return [v / n for v in e]


def _dist(a, b):
    return min(max(abs(x - y) for x, y in zip(a, b)), max(abs(x + y) for x, y in zip(a, b)))


def _to_mp(f):
    return [[mp.mpf(float(v)) for v in row] for row in np.asarray(f, np.float64)]


def solve(f1, f2, dps=DPS):
    """All ten solutions of the sample (f1_i^T E f2_i = 0), as Solution records."""
    with mp.workdps(dps):
        sols, _, _ = _solve_records(_to_mp(f1), _to_mp(f2))
    return sols


def _solve_records(F1, F2):
    N, polys = _system(F1, F2)
    raw = _eigen_solutions(N, polys)
    lams = [r[0] for r in raw]
    scale = max(1, max(abs(l) for l in lams))
    sols, units = [], []
    for s, (lam, _, Ev) in enumerate(raw):
        real = abs(mp.im(lam)) <= mp.mpf(10) ** (-mp.mp.dps // 2) * scale
        sep = min(abs(lam - lams[o]) for o in range(10) if o != s)
        u = _unit_real(Ev)
        units.append(u)
        sols.append(Solution(E=np.array([float(v) for v in u]).reshape(3, 3), eig=complex(lam), real=bool(real),
                             sep=float(sep)))
    return sols, units, [r[1] for r in raw]


def solve_with_condition(f1, f2, seed=0, dps=DPS):
    """solve() plus kappa for every real solution: four random relative
    perturbations (every input component times 1 +- 2^-40), the largest
    change of the solution (max-abs over the nine entries) divided by 2^-40.
    The perturbed problem's solution is followed from the unperturbed one by
    Gauss-Newton on the perturbed cubics (quadratic from a start 2^-40 away);
    where that does not settle, the perturbed problem is solved afresh and
    the nearest of its solutions taken."""
    rng = np.random.Generator(np.random.PCG64(seed))
    with mp.workdps(dps):
        F1, F2 = _to_mp(f1), _to_mp(f2)
        sols, units, xyz = _solve_records(F1, F2)
        change = [mp.mpf(0)] * 10
        tol = mp.mpf(10) ** (-(dps // 2))  # quadratic: a step of 1e-20 leaves an error of ~1e-40
        for _ in range(4):
            s1 = rng.choice([-1.0, 1.0], (5, 3))
            s2 = rng.choice([-1.0, 1.0], (5, 3))
            G1 = [[F1[i][c] * (1 + mp.mpf(PERT) * s1[i, c]) for c in range(3)] for i in range(5)]
            G2 = [[F2[i][c] * (1 + mp.mpf(PERT) * s2[i, c]) for c in range(3)] for i in range(5)]
            Np, pp = _system(G1, G2)
            fresh = None
            for s in range(10):
                if not sols[s].real:
                    continue
                v = _newton(pp, xyz[s], tol)
                if v is not None:
                    d = _dist(units[s], _unit_real(_combine(Np, *v)))
                else:
                    if fresh is None:
                        fresh = [_unit_real(r[2]) for r in _eigen_solutions(Np, pp)]
                    d = min(_dist(units[s], p) for p in fresh)
                change[s] = max(change[s], d)
        for s in range(10):
            if sols[s].real:
                sols[s].kappa = float(change[s] / mp.mpf(PERT))
    return sols
