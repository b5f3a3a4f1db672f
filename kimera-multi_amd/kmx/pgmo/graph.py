"""DeformationGraph: the owner of a kmx_dgraph_* handle (include/kmx_abi.h,
csrc/dgraph.hip), and the host helpers that build a deformation graph from a
mesh: simplify_voxel (the control vertices) and graph_from_mesh (mesh edges
and keyframe links).

The solve runs on the device. The two helpers here run on the host in numpy
and are the reference of the device version, simplify.MeshSimplifier
(csrc/simplify.hip), which returns the same arrays append by append.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import abi

_PARAM_FIELDS = ("lambda_init", "lambda_factor", "lambda_min", "lambda_max", "rel_tol", "abs_tol", "cg_rtol",
                 "max_iterations", "cg_max_iterations", "check_every")


def _opt(a, fn):
    return None if a is None else fn(a)


class DeformationGraph:
    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        self.device = int(device)
        L = abi.lib()
        abi.check(L.kmx_dgraph_create(device, C.byref(self._h)), "kmx_dgraph_create")
        self._L = L
        self.n = 0
        self.m = 0
        self.robot = self.stamp = self.R_rest = self.g = None

    # ------------------------------------------------------------------ life
    def close(self):
        if self._h:
            self._L.kmx_dgraph_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream):
        abi.check(self._L.kmx_dgraph_set_stream(self._h, C.c_void_p(hip_stream)), "kmx_dgraph_set_stream")

    # ----------------------------------------------------------------- graph
    def set_graph(self, R_rest, g, src, dst, w=None, *, robot=None, stamp=None):
        """Nodes (R_rest [n, 3, 3], g [n, 3]) and directed edges src -> dst
        with weights w (default 1). robot and stamp ([n]) are kept for
        `deformer`; default robot 0, stamp 0."""
        R = np.ascontiguousarray(R_rest, np.float64).reshape(-1, 3, 3)
        g = np.ascontiguousarray(g, np.float64).reshape(-1, 3)
        src = np.ascontiguousarray(src, np.int32).reshape(-1)
        dst = np.ascontiguousarray(dst, np.int32).reshape(-1)
        n, m = R.shape[0], src.shape[0]
        if g.shape[0] != n or dst.shape[0] != m:
            raise ValueError("R_rest [n, 3, 3] with g [n, 3], and src [m] with dst [m]")
        w = None if w is None else np.ascontiguousarray(np.broadcast_to(np.asarray(w, np.float64), (m,)))
        robot = np.zeros(n, np.int32) if robot is None else np.ascontiguousarray(robot, np.int32).reshape(-1)
        stamp = np.zeros(n, np.int64) if stamp is None else np.ascontiguousarray(stamp, np.int64).reshape(-1)
        if robot.shape[0] != n or stamp.shape[0] != n:
            raise ValueError("one robot id and one stamp per node")
        abi.check(self._L.kmx_dgraph_set_graph(self._h, n, abi.fptr(R), abi.fptr(g), m, abi.iptr(src), abi.iptr(dst),
                                               _opt(w, abi.fptr)), "kmx_dgraph_set_graph")
        self.n, self.m = n, m
        self.robot, self.stamp, self.R_rest, self.g = robot, stamp, R, g

    def set_weights(self, w=None):
        w = None if w is None else np.ascontiguousarray(np.broadcast_to(np.asarray(w, np.float64), (self.m,)))
        abi.check(self._L.kmx_dgraph_set_weights(self._h, _opt(w, abi.fptr)), "kmx_dgraph_set_weights")

    def set_priors(self, mode, R_hat=None, t_hat=None, kappa=0.0, tau=0.0):
        """mode [n]: 0 none, 1 soft, 2 hard. R_hat and t_hat default to the
        rest poses; kappa and tau broadcast to [n]."""
        n = self.n
        mode = np.ascontiguousarray(mode, np.uint8).reshape(-1)
        if mode.shape[0] != n:
            raise ValueError("one mode per node")
        rest_R = np.zeros((n, 3, 3)) if self.R_rest is None else self.R_rest  # None: no graph yet, the call says so
        rest_g = np.zeros((n, 3)) if self.g is None else self.g
        R = np.ascontiguousarray(rest_R if R_hat is None else R_hat, np.float64).reshape(-1, 3, 3)
        t = np.ascontiguousarray(rest_g if t_hat is None else t_hat, np.float64).reshape(-1, 3)
        if R.shape[0] != n or t.shape[0] != n:
            raise ValueError("R_hat [n, 3, 3] and t_hat [n, 3]")
        kappa = np.ascontiguousarray(np.broadcast_to(np.asarray(kappa, np.float64), (n,)))
        tau = np.ascontiguousarray(np.broadcast_to(np.asarray(tau, np.float64), (n,)))
        abi.check(self._L.kmx_dgraph_set_priors(self._h, abi.u8ptr(mode), abi.fptr(R), abi.fptr(t), abi.fptr(kappa),
                                                abi.fptr(tau)), "kmx_dgraph_set_priors")

    # ----------------------------------------------------------------- poses
    def set_poses(self, R=None, t=None):
        """The start of the next solve; no arguments: the rest poses."""
        if (R is None) != (t is None):
            raise ValueError("R and t: both or neither")
        if R is not None:
            R = np.ascontiguousarray(R, np.float64).reshape(-1, 3, 3)
            t = np.ascontiguousarray(t, np.float64).reshape(-1, 3)
            if R.shape[0] != self.n or t.shape[0] != self.n:
                raise ValueError("R [n, 3, 3] and t [n, 3]")
        abi.check(self._L.kmx_dgraph_set_poses(self._h, _opt(R, abi.fptr), _opt(t, abi.fptr)), "kmx_dgraph_set_poses")

    def poses(self):
        R, t = np.empty((self.n, 3, 3)), np.empty((self.n, 3))
        abi.check(self._L.kmx_dgraph_get_poses(self._h, abi.fptr(R), abi.fptr(t)), "kmx_dgraph_get_poses")
        return R, t

    # ------------------------------------------------------------------ eval
    def eval(self, what: str, v=None):
        """'cost' -> float; 'grad' -> b [n, 6]; 'jtj' -> J^T J v [n, 6] for v
        [n, 6]; 'blocks' -> the upper triangles [n, 21]; at the current point."""
        code = {"cost": abi.KMX_DGRAPH_EVAL_COST, "grad": abi.KMX_DGRAPH_EVAL_GRAD, "jtj": abi.KMX_DGRAPH_EVAL_JTJ,
                "blocks": abi.KMX_DGRAPH_EVAL_BLOCKS}[what]
        out = np.zeros({"cost": (1,), "grad": (self.n, 6), "jtj": (self.n, 6), "blocks": (self.n, 21)}[what])
        if what == "jtj":
            v = np.ascontiguousarray(v, np.float64).reshape(-1, 6)
            if v.shape[0] != self.n:
                raise ValueError("v [n, 6]")
        else:
            v = None
        abi.check(self._L.kmx_dgraph_eval(self._h, code, _opt(v, abi.fptr), abi.fptr(out)), "kmx_dgraph_eval")
        return float(out[0]) if what == "cost" else out

    # ----------------------------------------------------------------- solve
    def solve(self, **params) -> dict:
        """Keywords: kmx_dgraph_params' fields (lambda_init, lambda_factor,
        lambda_min, lambda_max, rel_tol, abs_tol, cg_rtol, max_iterations,
        cg_max_iterations, check_every); the rest take their defaults."""
        unknown = set(params) - set(_PARAM_FIELDS)
        if unknown:
            raise TypeError(f"unknown solve parameter(s) {sorted(unknown)}")
        p = abi.DgraphParams()
        p.rel_tol = -1.0
        for k, v in params.items():
            setattr(p, k, v)
        r = abi.DgraphResult()
        abi.check(self._L.kmx_dgraph_solve(self._h, C.byref(p), C.byref(r)), "kmx_dgraph_solve")
        out = {n: getattr(r, n) for n, _ in abi.DgraphResult._fields_}
        out["stop"] = abi.DGRAPH_STOP.get(r.stop_reason, str(r.stop_reason))
        return out

    def log(self) -> list:
        """Per outer iteration of the last solve: cost, trial_cost, lam, cg_iterations, accepted."""
        n = C.c_int32(0)
        abi.check(self._L.kmx_dgraph_get_log(self._h, 0, None, C.byref(n)), "kmx_dgraph_get_log")
        buf = (abi.DgraphLogEntry * max(n.value, 1))()
        abi.check(self._L.kmx_dgraph_get_log(self._h, n.value, buf, C.byref(n)), "kmx_dgraph_get_log")
        return [{"cost": e.cost, "trial_cost": e.trial_cost, "lam": e.lam, "cg_iterations": e.cg_iterations,
                 "accepted": bool(e.accepted)} for e in buf[:n.value]]

    def timing(self) -> dict:
        """Device times (ms) of the last solve; apply_ms: the product kernel of the last eval('jtj')."""
        ms = np.zeros(5)
        abi.check(self._L.kmx_dgraph_get_timing(self._h, abi.fptr(ms)), "kmx_dgraph_get_timing")
        return {"linearize_ms": ms[0], "cg_ms": ms[1], "trial_ms": ms[2], "total_ms": ms[3], "apply_ms": ms[4]}

    # ------------------------------------------------------------- the mesh
    def node_order(self):
        """The graph's node ids in (robot, stamp, id) order: the order `deformer` holds them in."""
        return np.lexsort((np.arange(self.n), self.stamp, self.robot))

    def deformer(self, k: int = 4, window_s: float = 1.0, *, window_ns=None, n_robots=None):
        """A MeshDeformer holding the graph's nodes, keyframes and control
        vertices alike, at rest; `push` gives them the solved poses."""
        from .deformer import MeshDeformer
        order = self.node_order()
        nr = int(self.robot.max(initial=0)) + 1 if n_robots is None else int(n_robots)
        md = MeshDeformer(k=k, window_s=window_s, n_robots=nr, device=self.device, window_ns=window_ns)
        md.add_nodes(self.robot[order], self.stamp[order], self.R_rest[order], self.g[order])
        return md

    def push(self, deformer):
        """The nodes' current poses (R_i, p_i = t_i) into a deformer made by `deformer`."""
        if deformer.n_nodes != self.n:
            raise ValueError("the deformer does not hold this graph's nodes")
        order = self.node_order()
        R, t = self.poses()
        deformer.set_node_poses(0, R[order], t[order])


def simplify_voxel(xyz, faces, stamp, robot, resolution: float, horizon_s=None):
    """Voxel-grid simplification per robot: a vertex's voxel is
    floor(xyz / resolution); the first vertex seen in a voxel is its
    representative; faces are remapped, and degenerate ones (two corners in one
    voxel) and duplicates (the same three control vertices, in any order) are
    dropped. horizon_s (default None: off) also cuts time into windows of that
    length (floor(stamp / horizon)) and merges inside one window only: on a
    drifting odometry frame, places far apart in time can share coordinates
    without being the same place. Returns (control_xyz float64 [c, 3], control_stamp int64 [c],
    control_robot int32 [c], control_faces int32 [f, 3], vertex_to_control
    int32 [V]); control vertices keep the order of their representatives."""
    if not resolution > 0:
        raise ValueError("resolution must be > 0")
    xyz = np.asarray(xyz).reshape(-1, 3)
    stamp = np.asarray(stamp, np.int64).reshape(-1)
    robot = np.asarray(robot, np.int32).reshape(-1)
    V = xyz.shape[0]
    if stamp.shape[0] != V or robot.shape[0] != V:
        raise ValueError("one stamp and one robot id per vertex")
    key = np.empty((V, 5), np.int64)
    key[:, 0] = robot
    key[:, 1:4] = np.floor(xyz.astype(np.float64) / float(resolution)).astype(np.int64)
    if horizon_s is None:
        key[:, 4] = 0
    else:
        if not horizon_s > 0:
            raise ValueError("horizon_s must be > 0")
        key[:, 4] = np.floor_divide(stamp, int(round(float(horizon_s) * 1e9)))
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    rank = np.empty(first.shape[0], np.int64)
    order = np.argsort(first, kind="stable")
    rank[order] = np.arange(first.shape[0])
    vmap = rank[inv].astype(np.int32)
    rep = first[order]
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    if F.size and (F.min() < 0 or F.max() >= V):
        raise ValueError("face index out of range")
    F = vmap[F].astype(np.int32).reshape(-1, 3)
    F = F[(F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2])]
    if F.shape[0]:
        _, keep = np.unique(np.sort(F, axis=1), axis=0, return_index=True)
        F = F[np.sort(keep)]
    return xyz[rep].astype(np.float64), stamp[rep], robot[rep], np.ascontiguousarray(F, np.int32), vmap


def graph_from_mesh(control_xyz, control_stamp, control_robot, faces, kf_stamp, kf_rest, *, w_mesh: float = 1.0,
                    w_link: float = 1.0) -> dict:
    """The deformation graph of a simplified mesh. Nodes: every robot's
    keyframes (kf_stamp[a] int64 [n_a], kf_rest[a] = (R [n_a, 3, 3], t [n_a,
    3])), robot by robot, then the control vertices (Rrest = I). Edges: the
    unique mesh edges of the faces in both directions (weight w_mesh), then
    every control vertex linked in both directions (w_link) to its robot's
    keyframe whose stamp equals the vertex's stamp (the first such keyframe);
    a vertex without one is an error. Returns R_rest, g, robot, stamp, src,
    dst, w, n_keyframes, kf_offset ([n_robots + 1]) and link ([c]: the node id
    of every control vertex's keyframe)."""
    cx = np.asarray(control_xyz, np.float64).reshape(-1, 3)
    cs = np.asarray(control_stamp, np.int64).reshape(-1)
    cr = np.asarray(control_robot, np.int32).reshape(-1)
    nr = len(kf_stamp)
    off = np.concatenate([[0], np.cumsum([len(s) for s in kf_stamp])]).astype(np.int64)
    nk, c = int(off[-1]), cx.shape[0]
    if c and (cr.min() < 0 or cr.max() >= nr):
        raise ValueError("control vertex robot id out of range")
    R = np.concatenate([np.asarray(kf_rest[a][0], np.float64).reshape(-1, 3, 3) for a in range(nr)] +
                       [np.tile(np.eye(3), (c, 1, 1))])
    g = np.concatenate([np.asarray(kf_rest[a][1], np.float64).reshape(-1, 3) for a in range(nr)] + [cx])
    if R.shape[0] != nk + c or g.shape[0] != nk + c:
        raise ValueError("kf_rest[a]: one pose per keyframe stamp")
    robot = np.concatenate([np.full(len(kf_stamp[a]), a, np.int32) for a in range(nr)] + [cr]).astype(np.int32)
    stamp = np.concatenate([np.asarray(kf_stamp[a], np.int64) for a in range(nr)] + [cs]).astype(np.int64)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    if F.size and (F.min() < 0 or F.max() >= c):
        raise ValueError("face index out of range")
    E = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]) if F.shape[0] else np.zeros((0, 2), np.int64)
    E = np.sort(E, axis=1)
    E = np.unique(E[E[:, 0] != E[:, 1]], axis=0) + nk
    link = np.empty(c, np.int64)
    for a in range(nr):
        sel = np.nonzero(cr == a)[0]
        ks = np.asarray(kf_stamp[a], np.int64)
        pos = np.searchsorted(ks, cs[sel], side="left")  # stamps are non-decreasing within a robot
        ok = (pos < ks.shape[0]) & (ks[np.minimum(pos, max(ks.shape[0] - 1, 0))] == cs[sel]) if ks.shape[0] else \
            np.zeros(sel.shape[0], bool)
        if not ok.all():
            raise ValueError(f"robot {a}: {int((~ok).sum())} control vertices have no keyframe at their stamp")
        link[sel] = off[a] + pos
    v = np.arange(c, dtype=np.int64) + nk
    src = np.concatenate([np.stack([E[:, 0], E[:, 1]], 1).reshape(-1), np.stack([v, link], 1).reshape(-1)])
    dst = np.concatenate([np.stack([E[:, 1], E[:, 0]], 1).reshape(-1), np.stack([link, v], 1).reshape(-1)])
    w = np.concatenate([np.full(2 * E.shape[0], float(w_mesh)), np.full(2 * c, float(w_link))])
    return {"R_rest": R, "g": g, "robot": robot, "stamp": stamp, "src": src.astype(np.int32),
            "dst": dst.astype(np.int32), "w": w, "n_keyframes": nk, "kf_offset": off, "link": link}
