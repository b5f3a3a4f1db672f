"""Chordal initialisation on MI355X (kmx_chordal_*,
chordal.hip): the two linear systems of
kmx.dpgo.init.chordal_initialization solved by Jacobi-preconditioned conjugate
gradients on the device, for a batch of graphs (blocks) at once.

Chordal initialisation is an L2 method: outlier loop closures at weight 1 pull
it as hard as inliers do, and it can then be worse than the odometry chain.
ChordalSolver.solve_robust is the robust form: GNC-TLS around the two solves,
with the residuals, the weights, mu and the stop test per block on the device
(dpgo's robust local initialisation [U]; the rule is stated in numpy by
kmx.dpgo.init.robust_chordal_initialization). Both are opt-in
(localInitializationMethod / local_init); the default stays the odometry chain.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import abi
from ..abi import check, fptr, iptr


def _real(a, shape, name):
    a = np.asarray(a)
    if a.dtype == object or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise ValueError(f"{name}: expected real numbers, got dtype {a.dtype}")
    if a.shape != shape:
        raise ValueError(f"{name}: expected shape {shape}, got {a.shape}")
    return np.ascontiguousarray(a, np.float64)


def _index(a, name, shape=None):
    a = np.asarray(a)
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name}: expected integers, got dtype {a.dtype}")
    if a.ndim != 1 or (shape is not None and a.shape != shape):
        raise ValueError(f"{name}: expected shape {shape or '(k,)'}, got {a.shape}")
    if a.size and (a.min() < -2**31 or a.max() >= 2**31):
        raise ValueError(f"{name}: does not fit int32")
    return np.ascontiguousarray(a, np.int32)


class ChordalSolver:
    """One kmx_chordal handle: set_graph once, then solve (and set_weights)
    any number of times. There is no CPU fallback."""

    def __init__(self, device: int = 0):
        L = abi.lib()
        if abi.device_count() <= device:
            raise abi.KmxError(f"no HIP device {device} visible (kmx has no CPU fallback)")
        h = C.c_void_p()
        check(L.kmx_chordal_create(device, C.byref(h)), "kmx_chordal_create")
        self.L, self.h, self.n, self.n_blocks, self.m = L, h, 0, 0, 0

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.L.kmx_chordal_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- argument checks (no library call; ValueError)
    @staticmethod
    def check_graph(n_poses, block_ptr, src, dst, R, t, kappa, tau, weight=None, anchors=(0,)):
        """Shapes and dtypes of set_graph's arguments -> the arrays the library
        gets. What the values must satisfy is the library's to check."""
        n = int(n_poses)
        if n < 1:
            raise ValueError(f"n_poses: expected >= 1, got {n_poses}")
        block_ptr = _index(block_ptr, "block_ptr")
        if block_ptr.shape[0] < 2:
            raise ValueError("block_ptr: expected at least one block (two entries)")
        src = _index(src, "src")
        m = src.shape[0]
        dst = _index(dst, "dst", (m,))
        R = _real(R, (m, 3, 3), "R")
        t = _real(t, (m, 3), "t")
        kappa = _real(kappa, (m,), "kappa")
        tau = _real(tau, (m,), "tau")
        weight = None if weight is None else _real(weight, (m,), "weight")
        anchors = _index(np.atleast_1d(np.asarray(anchors)), "anchors")
        return n, block_ptr, src, dst, R, t, kappa, tau, weight, anchors

    @staticmethod
    def check_start(n_poses, R_init, t_init):
        R_init = None if R_init is None else _real(R_init, (n_poses, 3, 3), "R_init")
        t_init = None if t_init is None else _real(t_init, (n_poses, 3), "t_init")
        return R_init, t_init

    # ---- the library
    def set_graph(self, n_poses, block_ptr, src, dst, R, t, kappa, tau, weight=None, anchors=(0,)):
        """Poses 0..n_poses-1 in contiguous blocks block_ptr [n_blocks + 1];
        edges src -> dst with R [m,3,3], t [m,3], kappa, tau, weight [m]
        (None: 1); anchors: the poses held at R = I, t = 0 (at least one per
        connected component)."""
        n, block_ptr, src, dst, R, t, kappa, tau, weight, anchors = self.check_graph(
            n_poses, block_ptr, src, dst, R, t, kappa, tau, weight, anchors)
        check(self.L.kmx_chordal_set_graph(
            self.h, n, block_ptr.shape[0] - 1, iptr(block_ptr), src.shape[0], iptr(src), iptr(dst), fptr(R), fptr(t),
            fptr(kappa), fptr(tau), None if weight is None else fptr(weight), anchors.shape[0], iptr(anchors)),
            "kmx_chordal_set_graph")
        self.n, self.n_blocks, self.m = n, block_ptr.shape[0] - 1, src.shape[0]

    def set_weights(self, weight):
        """New weights for the same edges (None: 1). Weights that cut a free
        pose off every anchor are refused and the previous ones stay."""
        if weight is not None:
            weight = _real(weight, (self.m,), "weight")
        check(self.L.kmx_chordal_set_weights(self.h, None if weight is None else fptr(weight)),
              "kmx_chordal_set_weights")

    def solve(self, R_init=None, t_init=None, *, rtol: float = 0.0, max_iterations: int = 0, check_every: int = 0):
        """-> (R [n,3,3], t [n,3], info): info is a list with one dict per
        block (iterations_rot, iterations_trans, converged, relres_rot,
        relres_trans). 0 for rtol / max_iterations / check_every: the
        library's default (1e-10, 20000, 50)."""
        R_init, t_init = self.check_start(self.n, R_init, t_init) if self.n else (None, None)
        if rtol < 0 or max_iterations < 0 or check_every < 0:
            raise ValueError("rtol, max_iterations and check_every must be >= 0")
        p = abi.ChordalParams(float(rtol), int(max_iterations), int(check_every))
        R = np.zeros((max(self.n, 1), 3, 3))
        t = np.zeros((max(self.n, 1), 3))
        info = (abi.ChordalBlockInfo * max(self.n_blocks, 1))()
        check(self.L.kmx_chordal_solve(self.h, C.byref(p), None if R_init is None else fptr(R_init),
                                       None if t_init is None else fptr(t_init), fptr(R), fptr(t), info),
              "kmx_chordal_solve")
        out = [{"iterations_rot": int(b.iterations_rot), "iterations_trans": int(b.iterations_trans),
                "converged": bool(b.converged), "relres_rot": list(b.relres_rot),
                "relres_trans": list(b.relres_trans)} for b in info[:self.n_blocks]]
        return R, t, out

    # ---- GNC-TLS around the solve (kmx_chordal_residuals / kmx_chordal_solve_robust)
    @staticmethod
    def check_fixed(m, fixed):
        """The fixed mask -> uint8 [m] (None stays None: no edge is fixed)."""
        if fixed is None:
            return None
        fixed = np.asarray(fixed)
        if not (fixed.dtype == np.bool_ or np.issubdtype(fixed.dtype, np.integer)):
            raise ValueError(f"fixed: expected booleans or integers, got dtype {fixed.dtype}")
        if fixed.shape != (m,):
            raise ValueError(f"fixed: expected shape ({m},), got {fixed.shape}")
        return np.ascontiguousarray(fixed != 0, np.uint8)

    @staticmethod
    def check_robust(barc, mu_init, mu_step, max_updates):
        for name, v in (("barc", barc), ("mu_init", mu_init), ("mu_step", mu_step)):
            if isinstance(v, (bool, str)) or not np.isscalar(v) or not np.isfinite(v) or v < 0:
                raise ValueError(f"{name}: expected a finite number >= 0, got {v!r}")
        if mu_step != 0 and not mu_step > 1:
            raise ValueError(f"mu_step: expected > 1 (or 0: the default), got {mu_step!r}")
        if isinstance(max_updates, bool) or not isinstance(max_updates, (int, np.integer)) or max_updates < 0:
            raise ValueError(f"max_updates: expected an integer >= 0, got {max_updates!r}")

    def residuals(self, R, t, mu=None, barc: float = 5.0, fixed=None):
        """dpgo's measurement error [U] r^2 = kappa |R_j - R_i R_ij|_F^2 +
        tau |t_j - t_i - R_i t_ij|^2 of every edge at the poses R [n,3,3],
        t [n,3] -> r2 [m]; with mu ([n_blocks], > 0) also the GNC-TLS factor g
        [m] of every edge for its block's mu and barc (fixed edges: 1) ->
        (r2, g). The kernel of solve_robust's loop."""
        R = _real(R, (self.n, 3, 3), "R")
        t = _real(t, (self.n, 3), "t")
        if mu is not None:
            mu = _real(mu, (self.n_blocks,), "mu")
        fixed = self.check_fixed(self.m, fixed)
        self.check_robust(barc, 0.0, 0.0, 0)
        r2 = np.zeros(max(self.m, 1))
        g = np.zeros(max(self.m, 1)) if mu is not None else None
        check(self.L.kmx_chordal_residuals(
            self.h, fptr(R), fptr(t), None if mu is None else fptr(mu), float(barc),
            None if fixed is None else fixed.ctypes.data_as(C.POINTER(C.c_uint8)), fptr(r2),
            None if g is None else fptr(g)), "kmx_chordal_residuals")
        return r2[:self.m] if g is None else (r2[:self.m], g[:self.m])

    def solve_robust(self, fixed, R_init=None, t_init=None, *, barc: float = 0.0, mu_init: float = 0.0,
                     mu_step: float = 0.0, max_updates: int = 0, rtol: float = 0.0, max_iterations: int = 0,
                     check_every: int = 0, start_projected: bool = False):
        """GNC-TLS around solve, decided on the device: the
        edges of the mask `fixed` ([m]; the odometry) keep their weight, every
        other edge gets w0 g with g in [0, 1] from its residual and the block's
        mu. The fixed edges must connect every free pose to an anchor by
        themselves. -> (R, t, g [m], info, rinfo): info as solve's, for each
        block's last solve; rinfo one dict per block (updates, converged,
        n_kept, n_rejected, n_fractional, mu). 0 for a parameter: the
        library's default (barc 5, mu_init from the residuals, mu_step 1.4,
        max_updates 100). The handle's weights are unchanged."""
        fixed = self.check_fixed(self.m, fixed)
        R_init, t_init = self.check_start(self.n, R_init, t_init) if self.n else (None, None)
        if rtol < 0 or max_iterations < 0 or check_every < 0:
            raise ValueError("rtol, max_iterations and check_every must be >= 0")
        self.check_robust(barc, mu_init, mu_step, max_updates)
        p = abi.ChordalParams(float(rtol), int(max_iterations), int(check_every))
        rp = abi.ChordalRobustParams(float(barc), float(mu_init), float(mu_step), int(max_updates),
                                     1 if start_projected else 0)
        R = np.zeros((max(self.n, 1), 3, 3))
        t = np.zeros((max(self.n, 1), 3))
        g = np.zeros(max(self.m, 1))
        info = (abi.ChordalBlockInfo * max(self.n_blocks, 1))()
        rinfo = (abi.ChordalRobustInfo * max(self.n_blocks, 1))()
        check(self.L.kmx_chordal_solve_robust(
            self.h, C.byref(p), C.byref(rp), None if fixed is None else fixed.ctypes.data_as(C.POINTER(C.c_uint8)),
            None if R_init is None else fptr(R_init), None if t_init is None else fptr(t_init), fptr(R), fptr(t),
            fptr(g), info, rinfo), "kmx_chordal_solve_robust")
        out = [{"iterations_rot": int(b.iterations_rot), "iterations_trans": int(b.iterations_trans),
                "converged": bool(b.converged), "relres_rot": list(b.relres_rot),
                "relres_trans": list(b.relres_trans)} for b in info[:self.n_blocks]]
        rout = [{"updates": int(b.updates), "converged": int(b.converged), "n_kept": int(b.n_kept),
                 "n_rejected": int(b.n_rejected), "n_fractional": int(b.n_fractional), "mu": float(b.mu)}
                for b in rinfo[:self.n_blocks]]
        return R, t, g[:self.m], out, rout

    def robust_stats(self) -> dict:
        """Figures of the last solve_robust: device times (ms), the number of
        GNC passes, CG iterations per stage summed over blocks and solves."""
        v = np.zeros(8)
        check(self.L.kmx_chordal_get_robust_stats(self.h, fptr(v)), "kmx_chordal_get_robust_stats")
        return {"total_ms": v[0], "first_solve_ms": v[1], "gnc_ms": v[2], "gnc_passes": int(v[3]),
                "cg_iterations_rot": int(v[4]), "cg_iterations_trans": int(v[5]), "solves": int(v[6])}

    def timing(self) -> dict:
        """Device times (ms) of the last solve's parts."""
        ms = np.zeros(4)
        check(self.L.kmx_chordal_get_timing(self.h, fptr(ms)), "kmx_chordal_get_timing")
        return dict(zip(("upload_ms", "rotation_ms", "translation_ms", "download_ms"), ms.tolist()))
