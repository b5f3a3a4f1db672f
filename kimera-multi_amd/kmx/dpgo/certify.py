"""Dual optimality certificate of an RBCD solution on MI355X (SURVEY.md §9.1;
kmx_cert_*, cert.hip).

RBCD optimises the rank-r relaxation; its rounded trajectory is the global
optimum only if the certificate matrix S(X) = Q - Lambda(X) is positive
semidefinite. Certifier finds the smallest eigenvalue of S by Lanczos on the
device and decides CERTIFIED (the smallest Ritz value theta_min has a
residual rho <= eta / 10 and theta_min - rho >= -eta), NEGATIVE (an eigenvalue
below -eta: X is a stationary point that is not optimal, and the Ritz vector
is a descent direction at rank r + 1) or UNDECIDED. NEGATIVE is a proof (Ritz
values lie inside the spectrum). CERTIFIED is a residual statement: S has an
eigenvalue within rho of theta_min, the smallest the Krylov space shows; no
Lanczos rule bounds lambda_min from below. Held against dense eigenvalues on
almost stationary points, the factor 1/10 left no false certificate where
rho <= eta left 20 in 1350 runs. The graph is the team graph
on one device, poses flattened.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import abi
from ..abi import check, fptr, iptr
from .chordal import _index, _real


class Certifier:
    """One kmx_cert handle: set_graph, set_point, then min_eig (and
    set_weights / set_point again) any number of times. There is no CPU
    fallback."""

    def __init__(self, device: int = 0):
        L = abi.lib()
        if abi.device_count() <= device:
            raise abi.KmxError(f"no HIP device {device} visible (kmx has no CPU fallback)")
        h = C.c_void_p()
        check(L.kmx_cert_create(device, C.byref(h)), "kmx_cert_create")
        self.L, self.h, self.n, self.m, self.r = L, h, 0, 0, 0

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.L.kmx_cert_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- argument checks (no library call; ValueError)
    @staticmethod
    def check_graph(n_poses, src, dst, R, t, kappa, tau, weight=None):
        """Shapes, dtypes and values of set_graph's arguments -> the arrays the
        library gets. The values are checked here as the library checks them
        (an index out of range, src == dst, a value that is not finite, kappa
        or tau <= 0, weight < 0), so a malformed graph is refused without a
        device."""
        n = int(n_poses)
        if n < 1:
            raise ValueError(f"n_poses: expected >= 1, got {n_poses}")
        src = _index(src, "src")
        m = src.shape[0]
        dst = _index(dst, "dst", (m,))
        R = _real(R, (m, 3, 3), "R")
        t = _real(t, (m, 3), "t")
        kappa = _real(kappa, (m,), "kappa")
        tau = _real(tau, (m,), "tau")
        weight = None if weight is None else _real(weight, (m,), "weight")
        if m:
            if src.min() < 0 or src.max() >= n or dst.min() < 0 or dst.max() >= n:
                raise ValueError("src / dst: edge endpoint out of range")
            if (src == dst).any():
                raise ValueError("src / dst: edge from a pose to itself")
            for name, a in (("R", R), ("t", t), ("kappa", kappa), ("tau", tau)):
                if not np.isfinite(a).all():
                    raise ValueError(f"{name}: not finite")
            if not (kappa > 0).all() or not (tau > 0).all():
                raise ValueError("kappa / tau: expected > 0")
        Certifier.check_weights(m, weight)
        return n, src, dst, R, t, kappa, tau, weight

    @staticmethod
    def check_weights(m, weight):
        if weight is None:
            return None
        weight = _real(weight, (m,), "weight")
        if not np.isfinite(weight).all() or (weight < 0).any():
            raise ValueError("weight: expected finite values >= 0")
        return weight

    @staticmethod
    def check_point(n_poses, X):
        X = np.asarray(X)
        if X.ndim != 3 or X.shape[0] != n_poses or X.shape[2] != 4:
            raise ValueError(f"X: expected shape ({n_poses}, r, 4), got {X.shape}")
        if not 3 <= X.shape[1] <= 8:
            raise ValueError(f"X: r must be in 3..8, got {X.shape[1]}")
        X = _real(X, X.shape, "X")
        if not np.isfinite(X).all():
            raise ValueError("X: not finite")
        return X

    @staticmethod
    def check_escape(n_poses, r, y, alphas):
        """escape's arguments -> (y [4n], alphas [k]) as the library gets
        them: a point of rank 3..7 (there is no rank 9), a finite y [4n] (or
        [n, 4]) and 1..8 finite step lengths."""
        if not 3 <= int(r) <= 7:
            raise ValueError(f"escape: the point's rank must be in 3..7 (set_point first; no rank 9), got {r}")
        y = np.asarray(y)
        if y.shape == (n_poses, 4):
            y = y.reshape(-1)
        y = _real(y, (4 * n_poses,), "y")
        if not np.isfinite(y).all():
            raise ValueError("y: not finite")
        alphas = np.asarray(alphas)
        if alphas.ndim != 1 or not 1 <= alphas.shape[0] <= 8:
            raise ValueError(f"alphas: expected 1..8 step lengths, got shape {alphas.shape}")
        alphas = _real(alphas, alphas.shape, "alphas")
        if not np.isfinite(alphas).all():
            raise ValueError("alphas: not finite")
        return y, alphas

    # ---- the library
    def set_graph(self, n_poses, src, dst, R, t, kappa, tau, weight=None):
        """Poses 0..n_poses-1 (the team, flattened); edges src -> dst with R
        [m,3,3], t [m,3], kappa, tau, weight [m] (None: 1)."""
        n, src, dst, R, t, kappa, tau, weight = self.check_graph(n_poses, src, dst, R, t, kappa, tau, weight)
        check(self.L.kmx_cert_set_graph(self.h, n, src.shape[0], iptr(src), iptr(dst), fptr(R), fptr(t), fptr(kappa),
                                        fptr(tau), None if weight is None else fptr(weight)), "kmx_cert_set_graph")
        self.n, self.m, self.r = n, src.shape[0], 0

    def set_weights(self, weight):
        """New weights for the same edges (None: 1); a point that is set is
        evaluated again for them."""
        weight = self.check_weights(self.m, weight)
        check(self.L.kmx_cert_set_weights(self.h, None if weight is None else fptr(weight)), "kmx_cert_set_weights")

    def set_point(self, X) -> dict:
        """X [n, r, 4] (kmx_pgo_get_iterate's layout, robots concatenated) ->
        {cost = tr(X Q X^T), trace_lambda, stationarity = |X S|_F}."""
        X = self.check_point(self.n, X)
        info = abi.CertPointInfo()
        check(self.L.kmx_cert_set_point(self.h, X.shape[1], fptr(X), C.byref(info)), "kmx_cert_set_point")
        self.r = X.shape[1]
        return {"cost": info.cost, "trace_lambda": info.trace_lambda, "stationarity": info.stationarity}

    def apply(self, v) -> np.ndarray:
        """S v for v [4n]: the Lanczos loop's kernel on caller data."""
        v = _real(v, (4 * self.n,), "v")
        out = np.zeros(4 * self.n)
        check(self.L.kmx_cert_apply(self.h, fptr(v), fptr(out)), "kmx_cert_apply")
        return out

    def lambda_blocks(self) -> np.ndarray:
        """Lambda_i [n, 3, 3] of the point."""
        out = np.zeros((self.n, 3, 3))
        check(self.L.kmx_cert_get_lambda(self.h, fptr(out)), "kmx_cert_get_lambda")
        return out

    def min_eig(self, eta: float, *, max_steps: int = 0, test_every: int = 0, check_every: int = 0, seed: int = 0,
                want_vector: bool = False) -> dict:
        """-> {decision ("CERTIFIED" / "NEGATIVE" / "UNDECIDED"), steps,
        theta_min, theta_max, residual} and, with want_vector, y [4n]: the
        unit Ritz vector of theta_min. 0 for max_steps / test_every /
        check_every: the library's default (5000, 10, 50). CERTIFIED:
        residual <= eta / 10 and theta_min - residual >= -eta; NEGATIVE:
        theta_min < -eta."""
        if isinstance(eta, (bool, str)) or not np.isscalar(eta) or not np.isfinite(eta) or not eta > 0:
            raise ValueError(f"eta: expected a finite number > 0, got {eta!r}")
        if max_steps < 0 or test_every < 0 or check_every < 0:
            raise ValueError("max_steps, test_every and check_every must be >= 0")
        p = abi.CertParams(float(eta), int(max_steps), int(test_every), int(check_every), 0, int(seed) % 2**64)
        res = abi.CertResult()
        y = np.zeros(4 * self.n) if want_vector else None
        check(self.L.kmx_cert_min_eig(self.h, C.byref(p), C.byref(res), None if y is None else fptr(y)),
              "kmx_cert_min_eig")
        out = {"decision": abi.CERT_DECISION[res.decision], "steps": int(res.steps), "theta_min": res.theta_min,
               "theta_max": res.theta_max, "residual": res.residual}
        if y is not None:
            out["y"] = y
        return out

    def escape(self, y, alphas) -> dict:
        """The staircase's escape step on the device (kmx_cert_escape): the
        cost tr(X+ Q X+^T) of every rank-(r+1) candidate X+ = [X; alpha y^T]
        (Stiefel blocks re-orthonormalised, as escape_point) -> {"cost": [k],
        "best": the index of the lowest cost strictly below the point's own,
        -1 when none descends}."""
        y, alphas = self.check_escape(self.n, self.r, y, alphas)
        cost = np.zeros(alphas.shape[0])
        best = C.c_int32(-1)
        check(self.L.kmx_cert_escape(self.h, fptr(y), alphas.shape[0], fptr(alphas), fptr(cost), C.byref(best)),
              "kmx_cert_escape")
        return {"cost": cost, "best": int(best.value)}

    def escape_commit(self, k: int):
        """Candidate k of the last escape becomes the handle's point at rank
        r + 1 (no upload) -> (X+ [n, r + 1, 4], set_point's info)."""
        X = np.zeros((self.n, self.r + 1, 4))
        info = abi.CertPointInfo()
        check(self.L.kmx_cert_escape_commit(self.h, int(k), fptr(X), C.byref(info)), "kmx_cert_escape_commit")
        self.r += 1
        return X, {"cost": info.cost, "trace_lambda": info.trace_lambda, "stationarity": info.stationarity}

    def escape_timing(self) -> dict:
        """Device times (ms, HIP events) of the last escape: its kernels and
        its transfers."""
        ms = np.zeros(2)
        check(self.L.kmx_cert_get_escape_timing(self.h, fptr(ms)), "kmx_cert_get_escape_timing")
        return {"escape_ms": float(ms[0]), "transfer_ms": float(ms[1])}

    def coefficients(self):
        """(alpha [k], beta [k]) of the last min_eig, the steps the host read."""
        cnt = C.c_int32(0)
        check(self.L.kmx_cert_get_coefficients(self.h, 0, None, None, C.byref(cnt)), "kmx_cert_get_coefficients")
        a, b = np.zeros(max(cnt.value, 1)), np.zeros(max(cnt.value, 1))
        check(self.L.kmx_cert_get_coefficients(self.h, cnt.value, fptr(a), fptr(b), C.byref(cnt)),
              "kmx_cert_get_coefficients")
        return a[:cnt.value], b[:cnt.value]

    def timing(self) -> dict:
        """Device times (ms, HIP events) of the last set_point and of the last
        min_eig's parts (the Lanczos steps and the vector pass: the launches
        alone, summed over the batches; the transfers), and the host's:
        host_rule_ms, the decisions between the batches, and host_wall_ms, the
        whole min_eig call."""
        ms, hm = np.zeros(4), np.zeros(2)
        check(self.L.kmx_cert_get_timing(self.h, fptr(ms)), "kmx_cert_get_timing")
        check(self.L.kmx_cert_get_host_timing(self.h, fptr(hm)), "kmx_cert_get_host_timing")
        out = dict(zip(("set_point_ms", "lanczos_ms", "vector_ms", "transfer_ms"), ms.tolist()))
        out.update(host_rule_ms=float(hm[0]), host_wall_ms=float(hm[1]))
        return out


def ritz(alpha, beta, eta: float) -> dict:
    """The decision rule on a tridiagonal (kmx_cert_ritz; host only)."""
    alpha = np.ascontiguousarray(alpha, np.float64)
    beta = np.ascontiguousarray(beta, np.float64)
    if alpha.ndim != 1 or beta.shape != alpha.shape:
        raise ValueError("alpha and beta: expected two vectors of one length")
    res = abi.CertResult()
    check(abi.lib().kmx_cert_ritz(alpha.shape[0], fptr(alpha), fptr(beta), float(eta), C.byref(res)), "kmx_cert_ritz")
    return {"decision": abi.CERT_DECISION[res.decision], "steps": int(res.steps), "theta_min": res.theta_min,
            "theta_max": res.theta_max, "residual": res.residual}


def start_vector(seed: int, count: int) -> np.ndarray:
    """The Lanczos start vector of `seed` before its normalisation (host only)."""
    out = np.zeros(max(int(count), 1))
    check(abi.lib().kmx_cert_start_vector(int(seed) % 2**64, int(count), fptr(out)), "kmx_cert_start_vector")
    return out[:count]


def flatten_team(g, X_by_robot):
    """The team graph with poses flattened by the robots' offsets ->
    (n, src, dst, X [n, r, 4])."""
    n_poses = np.asarray(g.n_poses, np.int64)
    off = np.concatenate([[0], np.cumsum(n_poses)])
    src = (off[np.asarray(g.r1)] + np.asarray(g.p1)).astype(np.int32)
    dst = (off[np.asarray(g.r2)] + np.asarray(g.p2)).astype(np.int32)
    parts = []
    for a in range(int(g.n_robots)):
        Xa = np.asarray(X_by_robot[a], np.float64)
        if Xa.ndim != 3 or Xa.shape[0] != n_poses[a] or Xa.shape[2] != 4:
            raise ValueError(f"X_by_robot[{a}]: expected shape ({n_poses[a]}, r, 4), got {Xa.shape}")
        parts.append(Xa)
    return int(off[-1]), src, dst, np.ascontiguousarray(np.concatenate(parts))


def split_team(g, X):
    """flatten_team's inverse for the point: X [n, r, 4] -> {robot: [n_a, r, 4]}."""
    n_poses = np.asarray(g.n_poses, np.int64)
    off = np.concatenate([[0], np.cumsum(n_poses)])
    X = np.asarray(X, np.float64)
    if X.ndim != 3 or X.shape[0] != off[-1] or X.shape[2] != 4:
        raise ValueError(f"X: expected shape ({int(off[-1])}, r, 4), got {X.shape}")
    return {a: np.ascontiguousarray(X[off[a]:off[a + 1]]) for a in range(int(g.n_robots))}


def rounding_lift(X) -> np.ndarray:
    """The lifting matrix Y [r, 3] to round X [n, r, 4] with
    (kmx.pipeline.rounded(X, Y)): the three dominant eigenvectors of
    sum_i Y_i Y_i^T (r x r, on the host), the third's sign chosen so that most
    Y^T Y_i have a positive determinant. A solution that left the span of the
    lifting matrix it started from (the staircase's) has no other; for an exact
    lift X_i = Y0 [R_i | t_i] it spans Y0's columns and gives the same rounded
    relative trajectory."""
    X = np.asarray(X, np.float64)
    if X.ndim != 3 or X.shape[2] != 4 or X.shape[1] < 3:
        raise ValueError(f"X: expected shape (n, r >= 3, 4), got {X.shape}")
    Yi = X[:, :, :3]
    M = np.einsum("nac,nbc->ab", Yi, Yi)
    _, V = np.linalg.eigh(M)
    Y = np.ascontiguousarray(V[:, ::-1][:, :3])
    det = np.linalg.det(np.einsum("ad,nac->ndc", Y, Yi))
    if (det > 0).sum() < (det < 0).sum():
        Y[:, 2] = -Y[:, 2]
    return Y


def certify_team(g, X_by_robot, weights=None, *, eta: float, device: int = 0, want_vector: bool = False, **kw) -> dict:
    """The certificate of the team's iterate X_by_robot ({robot: [n_a, r, 4]} or
    a list) on the graph g (PoseGraphData) with `weights` ([m]; None: g.weight,
    e.g. the final GNC weights). -> {decision, theta_min, theta_max, residual,
    steps, stationarity, cost, trace_lambda, timing} and, with want_vector, y.
    kw: max_steps, test_every, check_every, seed."""
    n, src, dst, X = flatten_team(g, X_by_robot)
    c = Certifier(device)
    try:
        c.set_graph(n, src, dst, g.R, g.t, g.kappa, g.tau, g.weight if weights is None else weights)
        info = c.set_point(X)
        out = c.min_eig(eta, want_vector=want_vector, **kw)
        out.update(info)
        out["eta"] = float(eta)
        out["timing"] = c.timing()
    finally:
        c.close()
    return out


def escape_point(X, y, alpha: float) -> np.ndarray:
    """The rank-(r+1) point [X; alpha y^T] with the Stiefel blocks
    re-orthonormalised (QR with a positive diagonal): the one use of the
    negative direction. X [n, r, 4], y [4n] -> [n, r + 1, 4]. To second order
    tr(X+ Q X+^T) = tr(X Q X^T) + alpha^2 y^T S y."""
    X = np.asarray(X, np.float64)
    n, r, _ = X.shape
    y = np.asarray(y, np.float64).reshape(n, 4)
    Xp = np.concatenate([X, alpha * y[:, None, :]], axis=1)
    q, rr = np.linalg.qr(Xp[:, :, :3])
    d = np.sign(np.diagonal(rr, axis1=1, axis2=2))
    d[d == 0] = 1.0
    Xp[:, :, :3] = q * d[:, None, :]
    return Xp
