"""Seeded synthetic mesh for the deformation stage (kmx.pgmo): points fixed in
the ground-truth world, each seen from one keyframe and expressed through that
robot's odometry chain, as a mesher running on odometry would place them. The
drift of the chain is what the deformation removes."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .pose_graph import PoseGraphData

KEYFRAME_PERIOD_NS = 100_000_000  # keyframe j of every robot is stamped j * 0.1 s


@dataclass
class MeshData:
    xyz: np.ndarray       # float32 [V, 3] in the robots' odometry frames
    robot: np.ndarray     # int32 [V]
    stamp: np.ndarray     # int64 [V] ns: the stamp of the keyframe the vertex was seen from
    keyframe: np.ndarray  # int32 [V]
    gt_xyz: np.ndarray    # float64 [V, 3] in the ground-truth world
    faces: np.ndarray     # int32 [F, 3]: triangles among one keyframe's vertices
    kf_stamp: list        # per robot int64 [n]
    rest_R: list          # per robot [n, 3, 3]: the odometry chain the vertices are expressed through
    rest_t: list


def make_mesh(g: PoseGraphData, verts_per_keyframe: int = 10, radius: float = 3.0, seed: int = 0, *,
              chain=None) -> MeshData:
    """`chain` {robot: (R [n, 3, 3], t [n, 3])}: the odometry chains; default
    kmx.pipeline.odometry_init(g), every robot in its own frame (first pose =
    identity). numpy PCG64(seed): the same call returns the same bits."""
    if chain is None:
        from ..pipeline import odometry_init
        chain = odometry_init(g)
    rng = np.random.Generator(np.random.PCG64(seed))
    m = int(verts_per_keyframe)
    xyz, rob, stamp, kf, gt, faces, kf_stamp = [], [], [], [], [], [], []
    base = 0
    for a in range(g.n_robots):
        n = int(g.n_poses[a])
        Rg, tg = g.gt_R[a], g.gt_t[a]
        Ro, to = np.asarray(chain[a][0], np.float64), np.asarray(chain[a][1], np.float64)
        d = rng.standard_normal((n, m, 3))
        d *= (radius * rng.random((n, m, 1)) ** (1.0 / 3.0)) / np.linalg.norm(d, axis=2, keepdims=True)
        pw = tg[:, None, :] + d                                  # fixed in the world
        local = np.einsum("nji,nmj->nmi", Rg, pw - tg[:, None, :])  # seen from keyframe n
        po = np.einsum("nij,nmj->nmi", Ro, local) + to[:, None, :]  # through the odometry chain
        st = np.arange(n, dtype=np.int64) * KEYFRAME_PERIOD_NS
        kf_stamp.append(st)
        xyz.append(po.reshape(-1, 3).astype(np.float32))
        gt.append(pw.reshape(-1, 3))
        rob.append(np.full(n * m, a, np.int32))
        kf.append(np.repeat(np.arange(n, dtype=np.int32), m))
        stamp.append(np.repeat(st, m))
        if m >= 3:
            first = base + np.arange(n, dtype=np.int64)[:, None] * m
            tri = np.arange(m - 2, dtype=np.int64)[None, :]
            faces.append(np.stack([first + 0 * tri, first + tri + 1, first + tri + 2], -1).reshape(-1, 3))
        base += n * m
    F = np.concatenate(faces).astype(np.int32) if faces else np.zeros((0, 3), np.int32)
    return MeshData(xyz=np.ascontiguousarray(np.concatenate(xyz)), robot=np.concatenate(rob),
                    stamp=np.concatenate(stamp), keyframe=np.concatenate(kf), gt_xyz=np.concatenate(gt), faces=F,
                    kf_stamp=kf_stamp, rest_R=[np.asarray(chain[a][0], np.float64) for a in range(g.n_robots)],
                    rest_t=[np.asarray(chain[a][1], np.float64) for a in range(g.n_robots)])
