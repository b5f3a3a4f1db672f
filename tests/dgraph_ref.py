"""The deformation graph contract (include/kmx_abi.h, "Deformation graph
optimisation") in numpy / scipy.sparse: the residual and its Jacobian, the
operators the device evaluates (cost, b = J^T r, J^T J v, the 6x6 diagonal
blocks), Levenberg-Marquardt with lambda I damping and block-Jacobi PCG, and,
for the operator tests, every operator entry together with the sum of the
absolute values of its terms and their number.

Unknowns per node: (omega, delta), R <- Exp(omega) R, t <- t + delta.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

EPS = float(np.finfo(np.float64).eps)

DEFAULTS = dict(lambda_init=1e-5, lambda_factor=10.0, lambda_min=1e-10, lambda_max=1e5, rel_tol=1e-5, abs_tol=0.0,
                cg_rtol=1e-6, max_iterations=100, cg_max_iterations=500)


def skew(a):
    a = np.asarray(a, np.float64)
    S = np.zeros(a.shape[:-1] + (3, 3))
    S[..., 0, 1], S[..., 0, 2] = -a[..., 2], a[..., 1]
    S[..., 1, 0], S[..., 1, 2] = a[..., 2], -a[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -a[..., 1], a[..., 0]
    return S


def exp_so3(w):
    """Rodrigues: I + A [w]x + B [w]x^2, the series below |w|^2 = 1e-8."""
    w = np.asarray(w, np.float64)
    th2 = (w * w).sum(-1)
    small = th2 < 1e-8
    th = np.sqrt(np.where(small, 1.0, th2))
    A = np.where(small, 1.0 - th2 / 6.0, np.sin(th) / th)
    B = np.where(small, 0.5 - th2 / 24.0, (1.0 - np.cos(th)) / np.where(small, 1.0, th2))
    K = skew(w)
    return np.eye(3) + A[..., None, None] * K + B[..., None, None] * (K @ K)


@dataclass
class Problem:
    R_rest: np.ndarray
    g: np.ndarray
    src: np.ndarray
    dst: np.ndarray
    w: np.ndarray
    mode: np.ndarray
    R_hat: np.ndarray
    t_hat: np.ndarray
    kappa: np.ndarray
    tau: np.ndarray
    d: np.ndarray = None

    @property
    def n(self):
        return self.g.shape[0]

    @property
    def m(self):
        return self.src.shape[0]


def make_problem(R_rest, g, src, dst, w=None, mode=None, R_hat=None, t_hat=None, kappa=0.0, tau=0.0) -> Problem:
    R_rest = np.asarray(R_rest, np.float64).reshape(-1, 3, 3)
    g = np.asarray(g, np.float64).reshape(-1, 3)
    n = g.shape[0]
    src, dst = np.asarray(src, np.int64).reshape(-1), np.asarray(dst, np.int64).reshape(-1)
    m = src.shape[0]
    w = np.ones(m) if w is None else np.broadcast_to(np.asarray(w, np.float64), (m,)).copy()
    mode = np.zeros(n, np.uint8) if mode is None else np.asarray(mode, np.uint8)
    R_hat = R_rest.copy() if R_hat is None else np.asarray(R_hat, np.float64).reshape(-1, 3, 3)
    t_hat = g.copy() if t_hat is None else np.asarray(t_hat, np.float64).reshape(-1, 3)
    kappa = np.where(mode == 1, np.broadcast_to(np.asarray(kappa, np.float64), (n,)), 0.0)
    tau = np.where(mode == 1, np.broadcast_to(np.asarray(tau, np.float64), (n,)), 0.0)
    P = Problem(R_rest, g, src, dst, w, mode, R_hat, t_hat, kappa, tau)
    P.d = edge_d(R_rest, g, src, dst)
    return P


def edge_d(R_rest, g, src, dst):
    """d_e = Rrest_i^T (g_j - g_i), each entry summed over the inner index in order."""
    dg = g[dst] - g[src]
    R = R_rest[src]
    d = np.empty((src.shape[0], 3))
    for c in range(3):
        v = R[:, 0, c] * dg[:, 0]
        v = v + R[:, 1, c] * dg[:, 1]
        v = v + R[:, 2, c] * dg[:, 2]
        d[:, c] = v
    return d


def well_posed(P: Problem) -> bool:
    """Union-find over the edges of weight > 0: every component holds a hard
    node or a soft node with tau > 0."""
    parent = np.arange(P.n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for e in np.nonzero(P.w > 0)[0]:
        a, b = find(P.src[e]), find(P.dst[e])
        if a != b:
            parent[max(a, b)] = min(a, b)
    held = {find(i) for i in range(P.n) if P.mode[i] == 2 or (P.mode[i] == 1 and P.tau[i] > 0)}
    return all(find(i) in held for i in range(P.n))


def pin(P: Problem, R, t):
    """Hard nodes at their priors."""
    R, t = np.array(R, np.float64), np.array(t, np.float64)
    hard = P.mode == 2
    R[hard], t[hard] = P.R_hat[hard], P.t_hat[hard]
    return R, t


def residual(P: Problem, R, t):
    """The stacked residual: sqrt(w_e) r_e per edge, then per soft node
    sqrt(kappa) (R - Rhat) row by row and sqrt(tau) (t - that)."""
    R, t = pin(P, R, t)
    a = np.einsum("eij,ej->ei", R[P.src], P.d)
    re = np.sqrt(P.w)[:, None] * (a + t[P.src] - t[P.dst])
    soft = np.nonzero(P.mode == 1)[0]
    rr = np.sqrt(P.kappa[soft])[:, None] * (R[soft] - P.R_hat[soft]).reshape(-1, 9)
    rt = np.sqrt(P.tau[soft])[:, None] * (t[soft] - P.t_hat[soft])
    return np.concatenate([re.ravel(), rr.ravel(), rt.ravel()])


def cost(P: Problem, R, t) -> float:
    r = residual(P, R, t)
    return float(r @ r)


def jacobian(P: Problem, R, t):
    """d residual / d (omega, delta) at (R, t), sparse [rows, 6 n]; the columns
    of hard nodes are zero."""
    R, t = pin(P, R, t)
    n, m = P.n, P.m
    sw = np.sqrt(P.w)
    a = np.einsum("eij,ej->ei", R[P.src], P.d)
    rows, cols, vals = [], [], []
    e = np.arange(m)
    Ka = -skew(a) * sw[:, None, None]
    for r in range(3):
        for c in range(3):
            rows.append(3 * e + r), cols.append(6 * P.src + c), vals.append(Ka[:, r, c])
        rows.append(3 * e + r), cols.append(6 * P.src + 3 + r), vals.append(sw)
        rows.append(3 * e + r), cols.append(6 * P.dst + 3 + r), vals.append(-sw)
    soft = np.nonzero(P.mode == 1)[0]
    s = np.arange(soft.shape[0])
    base = 3 * m
    sk = np.sqrt(P.kappa[soft])
    for c in range(3):  # column c of R: d (omega x R_c) / d omega = -[R_c]x
        Kc = -skew(R[soft][:, :, c]) * sk[:, None, None]
        for r in range(3):
            for k in range(3):
                rows.append(base + 9 * s + 3 * r + c), cols.append(6 * soft + k), vals.append(Kc[:, r, k])
    base += 9 * soft.shape[0]
    st = np.sqrt(P.tau[soft])
    for r in range(3):
        rows.append(base + 3 * s + r), cols.append(6 * soft + 3 + r), vals.append(st)
    nrows = base + 3 * soft.shape[0]
    J = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nrows, 6 * n)).tocsr()
    free = np.repeat((P.mode != 2).astype(np.float64), 6)
    return J @ sp.diags(free)


def blocks(P: Problem, R, t):
    """The 6x6 diagonal blocks of J^T J [n, 6, 6] from the closed form; 0 at hard nodes."""
    R, t = pin(P, R, t)
    a = np.einsum("eij,ej->ei", R[P.src], P.d)
    B = np.zeros((P.n, 6, 6))
    w = P.w
    aa = (a * a).sum(1)
    A = w[:, None, None] * (aa[:, None, None] * np.eye(3) - a[:, :, None] * a[:, None, :])
    S = w[:, None, None] * skew(a)
    np.add.at(B[:, :3, :3], P.src, A)
    np.add.at(B[:, :3, 3:], P.src, S)
    np.add.at(B[:, 3:, :3], P.src, -S)
    np.add.at(B[:, 3:, 3:], P.src, w[:, None, None] * np.eye(3))
    np.add.at(B[:, 3:, 3:], P.dst, w[:, None, None] * np.eye(3))
    B[:, :3, :3] += (2.0 * P.kappa)[:, None, None] * np.eye(3)
    B[:, 3:, 3:] += P.tau[:, None, None] * np.eye(3)
    B[P.mode == 2] = 0.0
    return B


TRIU = np.triu_indices(6)  # the upper triangle row by row: the device's 21 entries


def retract(P: Problem, R, t, x):
    x = np.asarray(x, np.float64).reshape(-1, 6)
    return exp_so3(x[:, :3]) @ R, t + x[:, 3:]


def pcg(J, lam, Minv, b, rtol, max_it):
    """(J^T J + lam I) x = -b from x = 0, preconditioned by the blocks Minv
    [n, 6, 6]; the two-reduction form. Returns (x, iterations)."""
    def prec(r):
        return np.einsum("nij,nj->ni", Minv, r.reshape(-1, 6)).ravel()
    x = np.zeros_like(b)
    r = -b
    bb = float(r @ r)
    z = prec(r)
    p = z.copy()
    rz = float(r @ z)
    it = 0
    active = bb > 0.0 and not (bb <= rtol * rtol * bb) and max_it > 0
    while active:
        q = J.T @ (J @ p) + lam * p
        pq = float(p @ q)
        if not pq > 0.0:
            break
        alpha = rz / pq
        x += alpha * p
        r -= alpha * q
        rr = float(r @ r)
        z = prec(r)
        rz_new = float(r @ z)
        it += 1
        beta = rz_new / rz
        rz = rz_new
        if rr <= rtol * rtol * bb or it >= max_it:
            break
        p = z + beta * p
    return x, it


def solve(P: Problem, R0=None, t0=None, **params) -> dict:
    """Levenberg-Marquardt as the contract states it. Returns R, t, log (cost,
    trial_cost, lam, cg_iterations, accepted per outer iteration), iterations,
    accepted, stop_reason, cg_iterations, cost_initial, cost_final."""
    q = dict(DEFAULTS)
    q.update(params)
    R, t = pin(P, P.R_rest if R0 is None else R0, P.g if t0 is None else t0)
    free = np.repeat(P.mode != 2, 6)
    lam = q["lambda_init"]
    r = residual(P, R, t)
    f = float(r @ r)
    J = jacobian(P, R, t)
    b = J.T @ r
    out = dict(cost_initial=f, log=[], iterations=0, accepted=0, cg_iterations=0, stop_reason=5)
    if float(b @ b) > 0.0 and q["max_iterations"] > 0:
        Bk = blocks(P, R, t)
        while True:
            M = Bk + lam * np.eye(6)
            Minv = np.linalg.inv(M)
            Minv[P.mode == 2] = 0.0
            x, cg_it = pcg(J, lam, Minv, b, q["cg_rtol"], q["cg_max_iterations"])
            x = np.where(free, x, 0.0)
            Rt, tt = retract(P, R, t, x)
            rt = residual(P, Rt, tt)
            fp = float(rt @ rt)
            acc = bool(fp < f)
            out["log"].append(dict(cost=f, trial_cost=fp, lam=lam, cg_iterations=cg_it, accepted=acc))
            out["iterations"] += 1
            out["cg_iterations"] += cg_it
            stop = 0
            if acc:
                out["accepted"] += 1
                lam = max(lam / q["lambda_factor"], q["lambda_min"])
                if fp <= q["abs_tol"]:
                    stop = 2
                elif f - fp <= q["rel_tol"] * f:
                    stop = 1
                R, t, r, f = Rt, tt, rt, fp
            else:
                lam = lam * q["lambda_factor"]
                if lam > q["lambda_max"]:
                    stop = 4
            if not stop and out["iterations"] >= q["max_iterations"]:
                stop = 3
            if stop:
                out["stop_reason"] = stop
                break
            if acc:
                J = jacobian(P, R, t)
                b = J.T @ r
                Bk = blocks(P, R, t)
    elif float(b @ b) > 0.0:
        out["stop_reason"] = 3
    out.update(R=R, t=t, cost_final=f, lambda_final=lam)
    return out


# ---------------------------------------------------------------------------
# The operators entry by entry, with the sum of the absolute values of the
# terms of each entry (every subtraction taken as an addition, through every
# level of the expression) and the number of those terms when the expression is
# expanded into products of inputs. Any order of evaluation in fp64 stays
# within (roundings on the longest path) eps (absolute sum) of the exact value,
# and the roundings on a path are fewer than the terms plus the few levels of
# products: the tests allow 4 (terms) eps (absolute sum) between two
# evaluations.
class T:
    """value, absolute sum, number of terms; arrays of one shape."""
    __slots__ = ("v", "a", "n")

    def __init__(self, v, a=None, n=None):
        self.v = np.asarray(v, np.float64)
        self.a = np.abs(self.v) if a is None else a
        self.n = np.ones(self.v.shape) if n is None else n

    def __add__(self, o):
        return T(self.v + o.v, self.a + o.a, self.n + o.n)

    def __sub__(self, o):
        return T(self.v - o.v, self.a + o.a, self.n + o.n)

    def __neg__(self):
        return T(-self.v, self.a, self.n)

    def __mul__(self, o):
        return T(self.v * o.v, self.a * o.a, self.n * o.n)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


class _Acc:
    def __init__(self, n, k):
        self.v, self.a, self.n = np.zeros((n, k)), np.zeros((n, k)), np.zeros((n, k))

    def add(self, idx, col, x: T, sign=1.0):
        np.add.at(self.v[:, col], idx, sign * x.v)
        np.add.at(self.a[:, col], idx, x.a)
        np.add.at(self.n[:, col], idx, x.n)

    def zero(self, rows):
        self.v[rows], self.a[rows], self.n[rows] = 0.0, 0.0, 0.0


def operators(P: Problem, R, t, v=None) -> dict:
    """cost (scalars), grad [n, 6], blocks [n, 21], jtj [n, 6] (with v [n, 6]):
    each a (value, absolute sum, terms) triple. Edges of weight 0 are skipped."""
    R, t = pin(P, R, t)
    n = P.n
    use = P.w > 0
    src, dst = P.src[use], P.dst[use]
    w = T(P.w[use])
    d = [T(P.d[use][:, c]) for c in range(3)]
    Ri = [[T(R[src][:, r, c]) for c in range(3)] for r in range(3)]
    a = [Ri[r][0] * d[0] + Ri[r][1] * d[1] + Ri[r][2] * d[2] for r in range(3)]
    ti = [T(t[src][:, c]) for c in range(3)]
    tj = [T(t[dst][:, c]) for c in range(3)]
    r = [a[c] + ti[c] - tj[c] for c in range(3)]
    soft = np.nonzero(P.mode == 1)[0]
    hard = P.mode == 2
    kap, tau = T(P.kappa[soft]), T(P.tau[soft])
    Rs = [[T(R[soft][:, r_, c]) for c in range(3)] for r_ in range(3)]
    E = [[Rs[r_][c] - T(P.R_hat[soft][:, r_, c]) for c in range(3)] for r_ in range(3)]
    et = [T(t[soft][:, c]) - T(P.t_hat[soft][:, c]) for c in range(3)]
    # cost
    ce = w * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    se = None
    for r_ in range(3):
        for c in range(3):
            se = E[r_][c] * E[r_][c] if se is None else se + E[r_][c] * E[r_][c]
    cp = kap * se + tau * (et[0] * et[0] + et[1] * et[1] + et[2] * et[2])
    out = {"cost": (float(ce.v.sum() + cp.v.sum()), float(ce.a.sum() + cp.a.sum()), float(ce.n.sum() + cp.n.sum()))}
    # gradient
    G = _Acc(n, 6)
    axr = _cross(a, r)
    for c in range(3):
        G.add(src, c, w * axr[c])
        G.add(src, 3 + c, w * r[c])
        G.add(dst, 3 + c, w * r[c], -1.0)
    for c in range(3):  # kappa sum over the columns k of R_k x E_k
        x = None
        for k in range(3):
            col = _cross([Rs[0][k], Rs[1][k], Rs[2][k]], [E[0][k], E[1][k], E[2][k]])[c]
            x = col if x is None else x + col
        G.add(soft, c, kap * x)
        G.add(soft, 3 + c, tau * et[c])
    G.zero(hard)
    out["grad"] = (G.v, G.a, G.n)
    # blocks: the 21 entries of the upper triangle, row by row
    B = _Acc(n, 21)
    two = T(np.full(soft.shape[0], 2.0))
    diag = {0: (1, 2), 6: (0, 2), 11: (0, 1)}
    for k, (p_, q_) in diag.items():
        B.add(src, k, w * (a[p_] * a[p_] + a[q_] * a[q_]))
        B.add(soft, k, two * kap)
    for k, (p_, q_) in {1: (0, 1), 2: (0, 2), 7: (1, 2)}.items():
        B.add(src, k, w * (a[p_] * a[q_]), -1.0)
    for k, (c, sgn) in {4: (2, -1.0), 5: (1, 1.0), 8: (2, 1.0), 10: (0, -1.0), 12: (1, -1.0), 13: (0, 1.0)}.items():
        B.add(src, k, w * a[c], sgn)
    for k in (15, 18, 20):
        B.add(src, k, w)
        B.add(dst, k, w)
        B.add(soft, k, tau)
    B.zero(hard)
    out["blocks"] = (B.v, B.a, B.n)
    if v is not None:
        v = np.where(hard[:, None], 0.0, np.asarray(v, np.float64).reshape(-1, 6))
        vi = [T(v[src][:, c]) for c in range(6)]
        vj = [T(v[dst][:, c]) for c in range(6)]
        wxa = _cross(vi[:3], a)
        u = [wxa[c] + vi[3 + c] - vj[3 + c] for c in range(3)]
        axu = _cross(a, u)
        H = _Acc(n, 6)
        for c in range(3):
            H.add(src, c, w * axu[c])
            H.add(src, 3 + c, w * u[c])
            H.add(dst, 3 + c, w * u[c], -1.0)
            H.add(soft, c, two * kap * T(v[soft][:, c]))
            H.add(soft, 3 + c, tau * T(v[soft][:, 3 + c]))
        H.zero(hard)
        out["jtj"] = (H.v, H.a, H.n)
    return out


# ------------------------------------------------------------------ test shapes
def grid_problem(nx=8, ny=8, n_kf=6, seed=0, spacing=1.0):
    """An nx x ny grid of control vertices (Rrest = I) with its mesh edges in
    both directions, and n_kf keyframes (random rest rotations) above it, each
    linked in both directions to its three nearest vertices. Returns (R_rest,
    g, src, dst, keyframe ids): keyframes are the last n_kf nodes."""
    from scipy.spatial.transform import Rotation
    rng = np.random.Generator(np.random.PCG64(seed))
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    gv = np.stack([ix.ravel() * spacing, iy.ravel() * spacing, 0.1 * rng.standard_normal(nx * ny)], 1)
    vid = lambda i, j: i * ny + j  # noqa: E731
    und = [(vid(i, j), vid(i + 1, j)) for i in range(nx - 1) for j in range(ny)] + \
          [(vid(i, j), vid(i, j + 1)) for i in range(nx) for j in range(ny - 1)]
    nv = nx * ny
    gk = np.stack([rng.uniform(0, (nx - 1) * spacing, n_kf), rng.uniform(0, (ny - 1) * spacing, n_kf),
                   rng.uniform(0.5, 1.5, n_kf)], 1).reshape(n_kf, 3)
    for k in range(n_kf):
        near = np.argsort(((gv - gk[k]) ** 2).sum(1), kind="stable")[:3]
        und += [(nv + k, int(p)) for p in near]
    und = np.asarray(und, np.int64)
    src = np.stack([und[:, 0], und[:, 1]], 1).ravel()
    dst = np.stack([und[:, 1], und[:, 0]], 1).ravel()
    Rk = Rotation.random(n_kf, random_state=np.random.RandomState(seed)).as_matrix() if n_kf else np.zeros((0, 3, 3))
    R_rest = np.concatenate([np.tile(np.eye(3), (nv, 1, 1)), Rk])
    return R_rest, np.concatenate([gv, gk]), src, dst, np.arange(nv, nv + n_kf)
