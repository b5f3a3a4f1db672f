"""MeshSimplifier: the append-only handle of kmx_simplify_* (include/kmx_abi.h,
csrc/simplify.hip): voxel simplification of a mesh that arrives in blocks, and
the deformation graph's edge arrays, on the device.

After any sequence of ``add`` calls the arrays equal what
``graph.simplify_voxel`` and ``graph.graph_from_mesh`` return for the
concatenated input: the same values, order and dtypes. Those two numpy
functions are the reference and stay as they are.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import abi


def _check(rc: int, what: str) -> None:
    """A rejected argument is the ValueError the numpy functions raise."""
    if rc in (abi.KMX_EINVAL, abi.KMX_EUNSUP):
        raise ValueError(f"{what}: {abi.lib().kmx_last_error().decode(errors='replace')}")
    abi.check(rc, what)


def horizon_to_ns(horizon_s) -> int:
    """simplify_voxel's window length in nanoseconds; 0: off."""
    if horizon_s is None:
        return 0
    if not horizon_s > 0:
        raise ValueError("horizon_s must be > 0")
    ns = int(round(float(horizon_s) * 1e9))
    if not 1 <= ns < 2 ** 63:
        raise ValueError("horizon_s must be at least half a nanosecond and fit int64 nanoseconds")
    return ns


class MeshSimplifier:
    def __init__(self, resolution: float, horizon_s=None, n_robots: int = 1, device: int = 0,
                 initial_slots: int = 0):
        self._h = C.c_void_p()
        if not resolution > 0:
            raise ValueError("resolution must be > 0")
        self.resolution, self.n_robots, self.device = float(resolution), int(n_robots), int(device)
        self.horizon_ns = horizon_to_ns(horizon_s)
        L = abi.lib()
        p = abi.SimplifyParams(self.resolution, self.horizon_ns, self.n_robots, int(initial_slots))
        _check(L.kmx_simplify_create(C.byref(p), device, C.byref(self._h)), "kmx_simplify_create")
        self._L = L
        self.n_vertices = self.n_faces_in = self.n_control = self.n_faces = 0
        abi.check(L.kmx_simplify_enable_timing(self._h, 1), "kmx_simplify_enable_timing")

    # ------------------------------------------------------------------ life
    def close(self):
        if self._h:
            self._L.kmx_simplify_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_stream(self, hip_stream):
        abi.check(self._L.kmx_simplify_set_stream(self._h, C.c_void_p(hip_stream)), "kmx_simplify_set_stream")

    def info(self) -> dict:
        i = abi.SimplifyInfo()
        abi.check(self._L.kmx_simplify_info(self._h, C.byref(i)), "kmx_simplify_info")
        return {n: getattr(i, n) for n, _ in abi.SimplifyInfo._fields_}

    def timing(self) -> dict:
        """Device times (ms) of the last add, edge formation and graph (0 for one that has not run); waits."""
        a, e, g = C.c_double(0), C.c_double(0), C.c_double(0)
        abi.check(self._L.kmx_simplify_read_timing(self._h, C.byref(a), C.byref(e), C.byref(g)),
                  "kmx_simplify_read_timing")
        return {"add_ms": a.value, "edges_ms": e.value, "graph_ms": g.value}

    # ---------------------------------------------------------------- append
    def add(self, xyz, faces, stamp, robot):
        """xyz [n, 3] (fp32), stamp [n] int64 ns, robot [n] (or one id), faces
        [f, 3]: vertex ids over everything added so far, this call included.
        Returns (first new vertex id, new control vertices, new kept faces)."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = xyz.shape[0]
        stamp = np.ascontiguousarray(stamp, np.int64).reshape(-1)
        robot = np.ascontiguousarray(np.broadcast_to(np.asarray(robot, np.int32), (n,)) if np.ndim(robot) == 0
                                     else np.asarray(robot, np.int32).reshape(-1))
        if stamp.shape[0] != n or robot.shape[0] != n:
            raise ValueError("one stamp and one robot id per vertex")
        F = np.asarray(faces).reshape(-1, 3)
        if F.size and (F.min() < -2 ** 31 or F.max() >= 2 ** 31):  # no wrap below; the library checks the rest
            raise ValueError("face index out of range")
        F = np.ascontiguousarray(F, np.int32)
        first, counts = C.c_int64(0), np.zeros(2, np.int64)
        _check(self._L.kmx_simplify_add(self._h, n, abi.iptr(robot), abi.i64ptr(stamp), abi.f32ptr(xyz), F.shape[0],
                                        abi.iptr(F), C.byref(first), abi.i64ptr(counts)), "kmx_simplify_add")
        self.n_vertices += n
        self.n_faces_in += F.shape[0]
        self.n_control += int(counts[0])
        self.n_faces += int(counts[1])
        return first.value, int(counts[0]), int(counts[1])

    # --------------------------------------------------------------- results
    def control(self, first: int = 0, n: int | None = None, representative: bool = False):
        """(xyz float64 [c, 3], stamp int64 [c], robot int32 [c]) of control
        vertices [first, first + n); with `representative`, also the vertex id
        each was taken from."""
        n = self.n_control - first if n is None else n
        m = max(n, 0)
        xyz, st = np.empty((m, 3), np.float64), np.empty(m, np.int64)
        rb, rep = np.empty(m, np.int32), np.empty(m, np.int32)
        _check(self._L.kmx_simplify_get_control(self._h, first, n, abi.fptr(xyz), abi.i64ptr(st), abi.iptr(rb),
                                                abi.iptr(rep)), "kmx_simplify_get_control")
        return (xyz, st, rb, rep) if representative else (xyz, st, rb)

    def vertex_map(self, first: int = 0, n: int | None = None):
        n = self.n_vertices - first if n is None else n
        out = np.empty(max(n, 0), np.int32)
        _check(self._L.kmx_simplify_get_vertex_map(self._h, first, n, abi.iptr(out)), "kmx_simplify_get_vertex_map")
        return out

    def faces(self, first: int = 0, n: int | None = None):
        n = self.n_faces - first if n is None else n
        out = np.empty((max(n, 0), 3), np.int32)
        _check(self._L.kmx_simplify_get_faces(self._h, first, n, abi.iptr(out)), "kmx_simplify_get_faces")
        return out

    def edges(self):
        """The unique mesh edges (lo < hi) int32 [e, 2] in lexicographic order."""
        ne = C.c_int64(0)
        _check(self._L.kmx_simplify_edges(self._h, C.byref(ne)), "kmx_simplify_edges")
        out = np.empty((ne.value, 2), np.int32)
        _check(self._L.kmx_simplify_get_edges(self._h, abi.iptr(out)), "kmx_simplify_get_edges")
        return out

    def graph_arrays(self, kf_stamp, w_mesh: float = 1.0, w_link: float = 1.0):
        """(src int32, dst int32, w float64, link int64, kf_offset int64) from the device."""
        ks = [np.asarray(s, np.int64).reshape(-1) for s in kf_stamp]
        off = np.concatenate([[0], np.cumsum([s.shape[0] for s in ks])]).astype(np.int64)
        cat = np.ascontiguousarray(np.concatenate(ks)) if ks else np.zeros(0, np.int64)
        nd = C.c_int64(0)
        args = (self._h, len(ks), abi.i64ptr(off), abi.i64ptr(cat), float(w_mesh), float(w_link))
        _check(self._L.kmx_simplify_graph(*args, None, None, None, None, C.byref(nd)), "kmx_simplify_graph")
        src, dst = np.empty(nd.value, np.int32), np.empty(nd.value, np.int32)
        w, link = np.empty(nd.value, np.float64), np.empty(self.n_control, np.int64)
        _check(self._L.kmx_simplify_graph(*args, abi.iptr(src), abi.iptr(dst), abi.fptr(w), abi.i64ptr(link),
                                          C.byref(nd)), "kmx_simplify_graph")
        return src, dst, w, link, off

    def graph(self, kf_stamp, kf_rest, w_mesh: float = 1.0, w_link: float = 1.0) -> dict:
        """graph_from_mesh's dict for the mesh added so far: src, dst, w and
        link from the device; the node arrays are the keyframes' and the
        control vertices' rows, concatenated here."""
        src, dst, w, link, off = self.graph_arrays(kf_stamp, w_mesh, w_link)
        cx, cs, cr = self.control()
        nr, nk, c = len(kf_stamp), int(off[-1]), cx.shape[0]
        R = np.concatenate([np.asarray(kf_rest[a][0], np.float64).reshape(-1, 3, 3) for a in range(nr)] +
                           [np.tile(np.eye(3), (c, 1, 1))])
        g = np.concatenate([np.asarray(kf_rest[a][1], np.float64).reshape(-1, 3) for a in range(nr)] + [cx])
        if R.shape[0] != nk + c or g.shape[0] != nk + c:
            raise ValueError("kf_rest[a]: one pose per keyframe stamp")
        robot = np.concatenate([np.full(len(kf_stamp[a]), a, np.int32) for a in range(nr)] + [cr]).astype(np.int32)
        stamp = np.concatenate([np.asarray(kf_stamp[a], np.int64) for a in range(nr)] + [cs]).astype(np.int64)
        return {"R_rest": R, "g": g, "robot": robot, "stamp": stamp, "src": src, "dst": dst, "w": w,
                "n_keyframes": nk, "kf_offset": off, "link": link}


def simplify_voxel_gpu(xyz, faces, stamp, robot, resolution: float, horizon_s=None, device: int = 0):
    """simplify_voxel on the device: the same five arrays."""
    if not resolution > 0:
        raise ValueError("resolution must be > 0")
    horizon_to_ns(horizon_s)
    xyz = np.asarray(xyz).reshape(-1, 3)
    robot = np.asarray(robot, np.int32).reshape(-1)
    stamp = np.asarray(stamp, np.int64).reshape(-1)
    if stamp.shape[0] != xyz.shape[0] or robot.shape[0] != xyz.shape[0]:
        raise ValueError("one stamp and one robot id per vertex")
    if robot.size and robot.min() < 0:
        raise ValueError("robot id out of range")
    with MeshSimplifier(resolution, horizon_s, int(robot.max(initial=0)) + 1, device) as ms:
        ms.add(xyz, faces, stamp, robot)
        cx, cs, cr = ms.control()
        return cx, cs, cr, ms.faces(), ms.vertex_map()
