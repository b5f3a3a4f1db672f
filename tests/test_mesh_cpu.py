"""Mesh deformation, the parts that need no GPU: the reference's known
answers (tests/mesh_ref.py is the contract in numpy), the synthetic mesh, the
argument structs, PLY files, corrections_from_atlas and `make mesh_check`."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import mesh_ref as MR

ROOT = Path(__file__).resolve().parents[1]


def _scene(seed=0, n_nodes=60, n_verts=300, n_robots=2):
    from kmx.synth.pose_graph import random_rotations
    rng = np.random.Generator(np.random.PCG64(seed))
    robot = np.sort(rng.integers(0, n_robots, n_nodes)).astype(np.int32)
    stamp = np.zeros(n_nodes, np.int64)
    for a in range(n_robots):
        sel = robot == a
        stamp[sel] = np.arange(sel.sum()) * 100_000_000
    R_rest = random_rotations(rng, n_nodes)
    g = rng.uniform(-20, 20, (n_nodes, 3))
    src = rng.integers(0, n_nodes, n_verts)
    xyz = (g[src] + rng.uniform(-2, 2, (n_verts, 3))).astype(np.float32)
    return dict(robot=robot, stamp=stamp, R_rest=R_rest, g=g, src=src, v_robot=robot[src].astype(np.int32),
                v_stamp=stamp[src].copy(), xyz=xyz, rng=rng)


def _rigid(rng):
    from kmx.synth.pose_graph import random_rotations
    return random_rotations(rng, 1)[0], rng.uniform(-5, 5, 3)


def test_reference_rigid_transform_on_every_node():
    s = _scene(1)
    T_R, T_t = _rigid(s["rng"])
    R_cur = T_R[None] @ s["R_rest"]
    p = s["g"] @ T_R.T + T_t
    out, st, (idx, w, cnt) = MR.deform_all(s["robot"], s["stamp"], s["R_rest"], s["g"], R_cur, p, s["v_robot"],
                                           s["v_stamp"], s["xyz"], 4, 1_000_000_000)
    assert st["unbound"] == 0 and (cnt >= 1).all()
    assert np.abs(w.sum(1) - 1.0).max() < 1e-15
    want = s["xyz"].astype(np.float64) @ T_R.T + T_t
    scale = max(np.abs(s["g"]).max(), np.abs(p).max(), np.abs(s["xyz"]).max())
    # before the final rounding: redo the blend in fp64 through the reference's own pieces
    R = MR.corrections(s["R_rest"], R_cur)
    v = s["xyz"].astype(np.float64)
    acc = np.zeros_like(v)
    for j in range(4):
        use = cnt > j
        jd = np.where(use, idx[:, j], 0)
        y = np.einsum("nij,nj->ni", R[jd], v - s["g"][jd]) + p[jd]
        acc += np.where(use[:, None], w[:, j:j + 1] * y, 0.0)
    assert np.abs(acc - want).max() <= 1e-12 * scale
    assert (np.abs(out.astype(np.float64) - want) <= MR.tolerance(want, scale)).all()


def test_reference_identity_when_current_is_rest():
    s = _scene(2)
    out, st, _ = MR.deform_all(s["robot"], s["stamp"], s["R_rest"], s["g"], s["R_rest"], s["g"], s["v_robot"],
                               s["v_stamp"], s["xyz"], 4, 1_000_000_000)
    assert np.array_equal(out, s["xyz"])
    assert st["max_displacement"] == 0.0 and st["sum_sq_displacement"] == 0.0


def test_reference_k1_w0_follows_its_keyframe():
    from kmx.synth.pose_graph import random_rotations
    s = _scene(3, n_robots=1)
    n = s["g"].shape[0]
    R_cur = random_rotations(s["rng"], n)
    p = s["rng"].uniform(-20, 20, (n, 3))
    out, st, (idx, w, cnt) = MR.deform_all(s["robot"], s["stamp"], s["R_rest"], s["g"], R_cur, p, s["v_robot"],
                                           s["v_stamp"], s["xyz"], 1, 0)
    assert np.array_equal(idx[:, 0], s["src"]) and (cnt == 1).all() and (w[:, 0] == 1.0).all()
    # T_cur T_rest^-1 v
    v = s["xyz"].astype(np.float64)
    local = np.einsum("nji,nj->ni", s["R_rest"][s["src"]], v - s["g"][s["src"]])
    want = np.einsum("nij,nj->ni", R_cur[s["src"]], local) + p[s["src"]]
    scale = max(np.abs(s["g"]).max(), np.abs(p).max(), np.abs(s["xyz"]).max())
    assert (np.abs(out.astype(np.float64) - want) <= MR.tolerance(want, scale)).all()


def test_reference_window_and_ties():
    """The table of the contract on a line of nodes: m = 0, 1, 2, k, k + 1, the
    inclusive window ends, a distance tie, and both fallbacks."""
    g = np.array([[0, 0, 0], [2, 0, 0], [-2, 0, 0], [4, 0, 0], [0, 3, 0], [0, -5, 0]], np.float64)
    stamp = np.arange(6, dtype=np.int64) * 10
    robot = np.zeros(6, np.int32)
    v = np.array([[0.5, 0, 0]], np.float32)

    def one(s, W, k=4, xyz=v):
        idx, w, c = MR.bind(robot, stamp, g, [0], [s], xyz, k, W)
        return idx[0], w[0], int(c[0])
    assert one(1000, 5)[2] == 0                        # m = 0
    i, w, c = one(20, 0)                               # m = 1, exactly at s
    assert (c, i[0], w[0]) == (1, 2, 1.0)
    i, w, c = one(15, 5)                               # s - W and s + W inclusive: nodes 1, 2
    assert c == 1 and i[0] == 1 and w[0] == 1.0        # m = 2: the nearer one, d_max the other's
    i, w, c = one(25, 25)                              # all six: k = 4 used, d_max the fifth's
    assert c == 4 and list(i) == [0, 1, 2, 4]
    assert abs(w.sum() - 1.0) < 1e-15 and (np.diff(w) <= 0).all()
    i, w, c = one(25, 25, xyz=np.array([[0, 0, 0]], np.float32))  # nodes 1 and 2 tie at distance 2: lower id first
    assert list(i[:3]) == [0, 1, 2] and w[1] == w[2]
    i, w, c = one(15, 5, xyz=np.array([[0, 7, 0]], np.float32))   # m = 2, both at the same distance: fallback
    assert (c, i[0], w[0], i[1]) == (1, 1, 1.0, -1)
    gg = np.zeros((3, 3))
    idx, w, c = MR.bind(np.zeros(3, np.int32), np.zeros(3, np.int64), gg, [0], [0], np.zeros((1, 3), np.float32), 4, 0)
    assert (int(c[0]), idx[0, 0], w[0, 0]) == (1, 0, 1.0)        # d_max = 0
    assert MR.window(MR.I64_MIN + 1, 5) == (MR.I64_MIN, MR.I64_MIN + 6)
    assert MR.window(MR.I64_MAX - 1, MR.I64_MAX) == (-1, MR.I64_MAX)


@pytest.fixture(scope="module")
def drifting_team():
    from kmx.synth import make_pose_graph
    from kmx.synth.mesh import make_mesh
    g = make_pose_graph(2, 800, 800, seed=3)
    chain = {a: (g.init_R[a], g.init_t[a]) for a in range(2)}  # odometry chains from the true first poses
    return g, chain, make_mesh(g, 5, 3.0, 1, chain=chain)


def test_synthetic_mesh_follows_ground_truth(drifting_team):
    """The generator's default odometry noise (0.01 rad, 0.1 m per keyframe)
    over 400 keyframes per robot; the ground truth stands in as the optimised
    trajectory. k = 4, W = 1 s. What is left after the deformation is the
    odometry noise between a vertex's keyframe and the keyframes it is blended
    with, d <= 3 steps away: about (0.1 m + 3 m x 0.01 rad) sqrt(d), 0.2 m at
    this noise and radius whatever the length of the chain, while the drift
    grows with the length; 400 keyframes per robot put the drift at several
    metres."""
    g, chain, mesh = drifting_team
    from kmx.synth.mesh import make_mesh
    again = make_mesh(g, 5, 3.0, 1, chain=chain)
    assert np.array_equal(again.xyz, mesh.xyz) and np.array_equal(again.gt_xyz, mesh.gt_xyz)
    assert mesh.xyz.dtype == np.float32 and mesh.xyz.shape == (4000, 3) and mesh.faces.shape == (2400, 3)
    nr = np.concatenate([np.full(400, a, np.int32) for a in range(2)])
    ns = np.concatenate(mesh.kf_stamp)
    out, st, _ = MR.deform_all(nr, ns, np.concatenate(mesh.rest_R), np.concatenate(mesh.rest_t),
                               np.concatenate(g.gt_R), np.concatenate(g.gt_t), mesh.robot, mesh.stamp, mesh.xyz,
                               4, 1_000_000_000)
    before = np.sqrt(((mesh.xyz.astype(np.float64) - mesh.gt_xyz) ** 2).sum(1).mean())
    after = np.sqrt(((out.astype(np.float64) - mesh.gt_xyz) ** 2).sum(1).mean())
    print(f"rmse before {before:.4f} m, after {after:.4f} m")
    assert st["unbound"] == 0
    assert after < before / 10


def test_mesh_rmse_convention(drifting_team):
    from kmx import pipeline as PL
    g, chain, mesh = drifting_team
    gt = {a: (g.gt_R[a], g.gt_t[a]) for a in range(2)}
    assert PL.mesh_rmse(g, mesh.gt_xyz, mesh.gt_xyz, gt) < 1e-12
    assert PL.mesh_rmse(g, mesh.xyz, mesh.gt_xyz, chain) > 0.1
    with pytest.raises(ValueError, match="mesh"):
        PL.run_pipeline(None, None, None, None, world=2, mesh=mesh)


def test_abi_structs_and_error_mapping():
    from kmx import abi
    assert C.sizeof(abi.MeshParams) == 16 and abi.MeshParams.window_ns.offset == 8
    assert C.sizeof(abi.MeshInfo) == 56 and abi.MeshInfo.k.offset == 40
    assert C.sizeof(abi.MeshStats) == 40 and abi.MeshStats.max_displacement.offset == 24
    L = abi.lib()
    for name in ("create", "destroy", "set_stream", "info", "add_nodes", "set_node_poses", "add_vertices", "bind",
                 "get_bindings", "deform", "deform_device", "sync", "enable_timing", "read_timing"):
        assert hasattr(L, "kmx_mesh_" + name)
    # checked before any device call: bad parameters and null handles map to KmxError with the code
    h = C.c_void_p()
    for k, code in ((0, abi.KMX_EUNSUP), (9, abi.KMX_EUNSUP)):
        p = abi.MeshParams(k, 1, 0)
        assert L.kmx_mesh_create(C.byref(p), 0, C.byref(h)) == code
    p = abi.MeshParams(4, 1, -1)
    assert L.kmx_mesh_create(C.byref(p), 0, C.byref(h)) == abi.KMX_EINVAL
    assert L.kmx_mesh_create(None, 0, C.byref(h)) == abi.KMX_EINVAL
    assert L.kmx_mesh_bind(None, 0, 0) == abi.KMX_EINVAL
    with pytest.raises(abi.KmxError, match=r"kmx_mesh_create failed \(-5\)"):
        from kmx.pgmo import MeshDeformer
        MeshDeformer(k=9)


@pytest.mark.parametrize("binary", [True, False])
def test_ply_round_trip(tmp_path, binary):
    from kmx.io import read_ply, write_ply
    rng = np.random.Generator(np.random.PCG64(5))
    xyz = (rng.standard_normal((37, 3)) * 100).astype(np.float32)
    xyz[0] = [1e-30, -3.4e38, 0.1]
    faces = rng.integers(0, 37, (11, 3)).astype(np.int32)
    f = tmp_path / "m.ply"
    write_ply(f, xyz, faces, binary=binary)
    x2, f2 = read_ply(f)
    assert x2.dtype == np.float32 and f2.dtype == np.int32
    assert np.array_equal(x2, xyz) and np.array_equal(f2, faces)
    write_ply(f, xyz, None, binary=binary)  # an empty face list
    x2, f2 = read_ply(f)
    assert np.array_equal(x2, xyz) and f2.shape == (0, 3)
    write_ply(f, np.zeros((0, 3), np.float32), binary=binary)
    x2, f2 = read_ply(f)
    assert x2.shape == (0, 3) and f2.shape == (0, 3)
    with pytest.raises(ValueError):
        write_ply(f, xyz, np.array([[0, 1, 37]]), binary=binary)


def test_corrections_from_atlas():
    from kmx.frontend.submaps import SubmapAtlas
    from kmx.pgmo import corrections_from_atlas
    from kmx.synth.pose_graph import random_rotations
    rng = np.random.Generator(np.random.PCG64(6))
    n = 45
    R_odom = random_rotations(rng, n)
    t_odom = np.cumsum(rng.uniform(0, 0.6, (n, 3)), 0)
    atlas = SubmapAtlas(0, max_distance=4.0, max_keyframes=7)
    for k in range(n):
        atlas.add_keyframe(k, 1000 * k, R_odom[k], t_odom[k])
    assert atlas.n_submaps > 3
    R_sub, t_sub = random_rotations(rng, atlas.n_submaps), rng.uniform(-9, 9, (atlas.n_submaps, 3))
    stamps, R_rest, t_rest, R_cur, t_cur = corrections_from_atlas(atlas, R_sub, t_sub)
    assert stamps.dtype == np.int64 and np.array_equal(stamps, 1000 * np.arange(n))
    assert np.abs(R_rest - R_odom).max() < 1e-13 and np.abs(t_rest - t_odom).max() < 1e-12  # the odometry poses
    Rk, tk = atlas.keyframe_trajectory(R_sub, t_sub)
    assert np.array_equal(R_cur, Rk) and np.array_equal(t_cur, tk)
    # a point rigidly attached to a keyframe follows it through the correction
    x = rng.standard_normal(3)
    R = MR.corrections(R_rest, R_cur)
    for k in (0, 17, n - 1):
        v = R_odom[k] @ x + t_odom[k]
        assert np.abs(R[k] @ (v - t_rest[k]) + t_cur[k] - (Rk[k] @ x + tk[k])).max() < 1e-12


def test_make_mesh_check():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc is missing")
    r = subprocess.run(["make", "-s", "-C", str(ROOT / "kimera-multi_amd" / "csrc"), "mesh_check", f"HIPCC={hipcc}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mesh_check ok" in r.stdout
