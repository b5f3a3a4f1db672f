"""MeshDeformer: the streaming handle of kmx_mesh_* (include/kmx_abi.h).

Keyframes are the control nodes: a keyframe's odometry pose is its rest pose
and its optimised pose the current one. Vertices carry the robot and the stamp
they were observed at. ``deform`` binds what was added since the last bind and
moves every vertex; ``update_trajectory`` then ``deform`` follows a new
trajectory without binding again.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import abi


def _poses(R, t, n=None):
    R = np.ascontiguousarray(R, np.float64).reshape(-1, 3, 3)
    t = np.ascontiguousarray(t, np.float64).reshape(-1, 3)
    if R.shape[0] != t.shape[0] or (n is not None and R.shape[0] != n):
        raise ValueError("R [n, 3, 3] and t [n, 3] must have one row per keyframe")
    return R, t


class MeshDeformer:
    def __init__(self, k: int = 4, window_s: float = 1.0, n_robots: int = 1, device: int = 0, *,
                 window_ns: int | None = None):
        """window_ns, when given, is the window in whole nanoseconds and window_s is not read."""
        self._h = C.c_void_p()
        self.k, self.n_robots, self.device = int(k), int(n_robots), int(device)
        self.window_ns = int(round(float(window_s) * 1e9)) if window_ns is None else int(window_ns)
        if not -2 ** 63 <= self.window_ns < 2 ** 63:
            raise ValueError("the window does not fit int64 nanoseconds")
        L = abi.lib()
        p = abi.MeshParams(self.k, self.n_robots, self.window_ns)
        abi.check(L.kmx_mesh_create(C.byref(p), device, C.byref(self._h)), "kmx_mesh_create")
        self._L = L
        self._node_ids = [[] for _ in range(self.n_robots)]  # per robot: arrays of node ids, in keyframe order
        self.n_nodes = 0
        self.n_vertices = 0
        self._bound = 0  # vertices [0, _bound) are bound
        self.enable_timing(True)  # two event records per bind and per deform

    # ------------------------------------------------------------------ life
    def close(self):
        if self._h:
            self._L.kmx_mesh_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream):
        abi.check(self._L.kmx_mesh_set_stream(self._h, C.c_void_p(hip_stream)), "kmx_mesh_set_stream")

    def sync(self):
        abi.check(self._L.kmx_mesh_sync(self._h), "kmx_mesh_sync")

    def info(self) -> dict:
        i = abi.MeshInfo()
        pn, pv = np.zeros(self.n_robots, np.int64), np.zeros(self.n_robots, np.int64)
        abi.check(self._L.kmx_mesh_info(self._h, C.byref(i), abi.i64ptr(pn), abi.i64ptr(pv)), "kmx_mesh_info")
        out = {n: getattr(i, n) for n, _ in abi.MeshInfo._fields_}
        out["nodes_per_robot"], out["vertices_per_robot"] = pn, pv
        return out

    # ----------------------------------------------------------------- nodes
    def add_nodes(self, robot, stamps_ns, R_rest, g):
        """Control nodes with their own robot ids ([n]); a bare control point
        has R_rest = I. Returns the first new node id."""
        robot = np.ascontiguousarray(robot, np.int32).reshape(-1)
        stamps = np.ascontiguousarray(stamps_ns, np.int64).reshape(-1)
        R, g = _poses(R_rest, g, robot.shape[0])
        if stamps.shape[0] != robot.shape[0]:
            raise ValueError("one stamp per node")
        first = self.n_nodes
        abi.check(self._L.kmx_mesh_add_nodes(self._h, robot.shape[0], abi.iptr(robot), abi.i64ptr(stamps),
                                             abi.fptr(R), abi.fptr(g)), "kmx_mesh_add_nodes")
        ids = np.arange(first, first + robot.shape[0], dtype=np.int64)
        for a in np.unique(robot):
            self._node_ids[int(a)].append(ids[robot == a])
        self.n_nodes += robot.shape[0]
        return first

    def add_keyframes(self, robot: int, stamps_ns, R_odom, t_odom):
        """Keyframes of one robot, in order; their odometry poses are the rest poses."""
        stamps = np.ascontiguousarray(stamps_ns, np.int64).reshape(-1)
        return self.add_nodes(np.full(stamps.shape[0], robot, np.int32), stamps, R_odom, t_odom)

    def set_node_poses(self, first: int, R_cur, p):
        R, p = _poses(R_cur, p)
        abi.check(self._L.kmx_mesh_set_node_poses(self._h, first, R.shape[0], abi.fptr(R), abi.fptr(p)),
                  "kmx_mesh_set_node_poses")

    def update_trajectory(self, robot: int, R_opt, t_opt):
        """Current poses of every keyframe of `robot` added so far, in order."""
        if not 0 <= robot < self.n_robots:
            raise abi.KmxError(f"update_trajectory failed ({abi.KMX_EINVAL}): robot id out of range")
        ids = np.concatenate(self._node_ids[robot]) if self._node_ids[robot] else np.zeros(0, np.int64)
        R, t = _poses(R_opt, t_opt, ids.shape[0])
        # the robot's ids are runs of consecutive ids (one per add_* call, longer when calls were adjacent)
        cut = np.nonzero(np.diff(ids) != 1)[0] + 1
        for run in np.split(np.arange(ids.shape[0]), cut):
            if run.size:
                self.set_node_poses(int(ids[run[0]]), R[run], t[run])

    # -------------------------------------------------------------- vertices
    def add_vertices(self, robot, stamps_ns, xyz):
        """robot: one id or [n]. Returns the first new vertex id."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = xyz.shape[0]
        stamps = np.ascontiguousarray(stamps_ns, np.int64).reshape(-1)
        robot = np.ascontiguousarray(np.broadcast_to(np.asarray(robot, np.int32), (n,)))
        if stamps.shape[0] != n:
            raise ValueError("one stamp per vertex")
        first = C.c_int64(0)
        abi.check(self._L.kmx_mesh_add_vertices(self._h, n, abi.iptr(robot), abi.i64ptr(stamps), abi.f32ptr(xyz),
                                                C.byref(first)), "kmx_mesh_add_vertices")
        self.n_vertices += n
        return first.value

    def bind(self, first: int, n: int):
        abi.check(self._L.kmx_mesh_bind(self._h, first, n), "kmx_mesh_bind")

    def _bind_new(self):
        if self._bound < self.n_vertices:
            self.bind(self._bound, self.n_vertices - self._bound)
            self._bound = self.n_vertices

    def rebind(self):
        """Binds every vertex again, to the nodes present now."""
        self.bind(0, self.n_vertices)
        self._bound = self.n_vertices

    def bindings(self, first: int = 0, n: int | None = None):
        """(idx [n, k] int32, -1 beyond count; w [n, k]; count [n]) of bound vertices."""
        self._bind_new()
        n = self.n_vertices - first if n is None else n
        idx = np.empty((max(n, 0), self.k), np.int32)
        w = np.empty((max(n, 0), self.k), np.float64)
        cnt = np.empty(max(n, 0), np.int32)
        abi.check(self._L.kmx_mesh_get_bindings(self._h, first, n, abi.iptr(idx), abi.fptr(w), abi.iptr(cnt)),
                  "kmx_mesh_get_bindings")
        return idx, w, cnt

    # ---------------------------------------------------------------- deform
    def deform(self, out=None, first: int = 0, n: int | None = None):
        """Binds whatever was added since the last bind, then moves vertices
        [first, first + n) (default: all). Returns (float32 [n, 3], stats).
        With `out` a float32 torch tensor on this device ([n, 3], contiguous)
        the result is written there on the handle's stream and the call
        returns (out, None) without synchronising; `sync()` waits. (torch must
        have taken the device before the process's first kmx handle was made,
        as for kmx.dpgo.driver's exchange buffers.)"""
        self._bind_new()
        n = self.n_vertices - first if n is None else n
        if out is not None:
            import torch
            if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and
                    out.is_contiguous() and out.numel() == 3 * n and out.device.index == self.device):
                raise ValueError("out: a contiguous float32 tensor of n x 3 elements on the handle's device")
            abi.check(self._L.kmx_mesh_deform_device(self._h, first, n, C.c_void_p(out.data_ptr())),
                      "kmx_mesh_deform_device")
            return out, None
        xyz = np.empty((max(n, 0), 3), np.float32)
        st = abi.MeshStats()
        abi.check(self._L.kmx_mesh_deform(self._h, first, n, abi.f32ptr(xyz), C.byref(st)), "kmx_mesh_deform")
        return xyz, {"vertices": st.n_vertices, "unbound": st.n_unbound, "partial": st.n_partial,
                     "max_displacement": st.max_displacement, "sum_sq_displacement": st.sum_sq_displacement}

    # ---------------------------------------------------------------- timing
    def enable_timing(self, on: bool = True):
        abi.check(self._L.kmx_mesh_enable_timing(self._h, int(on)), "kmx_mesh_enable_timing")

    def timing(self) -> dict:
        """Device times (ms) of the last bind and the last deform (0 for one that has not run); waits."""
        b, d = C.c_double(0), C.c_double(0)
        abi.check(self._L.kmx_mesh_read_timing(self._h, C.byref(b), C.byref(d)), "kmx_mesh_read_timing")
        return {"bind_ms": b.value, "deform_ms": d.value}


def corrections_from_atlas(atlas, R_sub, t_sub):
    """Keyframe rest and current poses of one robot from its SubmapAtlas and
    optimised submap poses: rest = the keyframes' odometry poses (the atlas's
    own submap poses), current = atlas.keyframe_trajectory(R_sub, t_sub).
    Returns (stamps_ns [n] int64, R_rest, t_rest, R_cur, t_cur)."""
    n_s = atlas.n_submaps
    R0 = np.stack([p[0] for p in atlas.submap_pose]) if n_s else np.zeros((0, 3, 3))
    t0 = np.stack([p[1] for p in atlas.submap_pose]) if n_s else np.zeros((0, 3))
    R_rest, t_rest = atlas.keyframe_trajectory(R0, t0)
    R_cur, t_cur = atlas.keyframe_trajectory(np.asarray(R_sub, np.float64), np.asarray(t_sub, np.float64))
    return np.asarray(atlas.kf_stamp, np.int64), R_rest, t_rest, R_cur, t_cur
