"""Chordal initialisation on MI355X (kmx_chordal_*,
chordal.hip): the two linear systems of
kmx.dpgo.init.chordal_initialization solved by Jacobi-preconditioned conjugate
gradients on the device, for a batch of graphs (blocks) at once.

Chordal initialisation is an L2 method: outlier loop closures at weight 1 pull
it as hard as inliers do, and it can then be worse than the odometry chain.
Nothing selects it by default.
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

    def timing(self) -> dict:
        """Device times (ms) of the last solve's parts."""
        ms = np.zeros(4)
        check(self.L.kmx_chordal_get_timing(self.h, fptr(ms)), "kmx_chordal_get_timing")
        return dict(zip(("upload_ms", "rotation_ms", "translation_ms", "download_ms"), ms.tolist()))
