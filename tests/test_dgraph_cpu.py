"""Deformation graph optimisation, the parts that need no GPU: the reference
(tests/dgraph_ref.py is the contract in numpy) against finite differences and
a known answer, the mesh helpers (simplify_voxel, graph_from_mesh), the
argument structs and error mapping, and `make dgraph_check`."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import dgraph_ref as DR

ROOT = Path(__file__).resolve().parents[1]


def random_point(P_or_n, rng, rot=0.3, trans=0.5, R_rest=None, g=None):
    """The rest pose of every node moved by a random rotation (angle ~ rot) and offset."""
    if R_rest is None:
        R_rest, g = P_or_n.R_rest, P_or_n.g
    n = g.shape[0]
    return DR.exp_so3(rot * rng.standard_normal((n, 3))) @ R_rest, g + trans * rng.standard_normal((n, 3))


def small_problem(seed=0, modes=True):
    """A 4 x 3 grid with 3 keyframes; with `modes` one of each prior mode and
    a zero-weight edge."""
    rng = np.random.Generator(np.random.PCG64(seed))
    R_rest, g, src, dst, kf = DR.grid_problem(4, 3, 3, seed=seed)
    n = g.shape[0]
    w = rng.uniform(0.5, 2.0, src.shape[0])
    mode = np.zeros(n, np.uint8)
    mode[kf] = 1
    if modes:
        mode[kf[0]] = 2
        w[5] = 0.0
    R_hat, t_hat = random_point(None, rng, R_rest=R_rest, g=g)
    return DR.make_problem(R_rest, g, src, dst, w, mode, R_hat, t_hat, rng.uniform(0.5, 2, n), rng.uniform(0.5, 2, n))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_jacobian_against_central_differences(seed):
    """h = 1e-6: the error of a central difference is O(h^2) times the third
    derivative's scale, so 1e-8 relative to |J|."""
    P = small_problem(seed)
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    R, t = DR.pin(P, *random_point(P, rng))
    J = DR.jacobian(P, R, t).toarray()
    h = 1e-6
    num = np.zeros_like(J)
    for k in range(6 * P.n):
        if P.mode[k // 6] == 2:
            continue  # a hard node has no unknowns: its columns are zero
        x = np.zeros(6 * P.n)
        x[k] = h
        rp = DR.residual(P, *DR.retract(P, R, t, x))
        rm = DR.residual(P, *DR.retract(P, R, t, -x))
        num[:, k] = (rp - rm) / (2 * h)
    assert np.linalg.norm(J) > 1.0
    assert np.abs(J - num).max() <= 1e-8 * np.linalg.norm(J)
    assert not J[:, np.repeat(P.mode == 2, 6)].any()


def test_reference_operators_agree_with_the_jacobian():
    """The closed forms (blocks, and the term-by-term operators the GPU tests
    compare with) against J^T r, J^T J v and the diagonal blocks of J^T J."""
    P = small_problem(3)
    rng = np.random.Generator(np.random.PCG64(7))
    R, t = random_point(P, rng)
    v = rng.standard_normal((P.n, 6))
    J = DR.jacobian(P, R, t)
    r = DR.residual(P, R, t)
    JtJ = (J.T @ J).toarray()
    op = DR.operators(P, R, t, v)
    vm = np.where((P.mode == 2)[:, None], 0.0, v)
    want = {"grad": (J.T @ r).reshape(-1, 6), "jtj": (JtJ @ vm.ravel()).reshape(-1, 6),
            "blocks": np.stack([JtJ[6 * i:6 * i + 6, 6 * i:6 * i + 6][DR.TRIU] for i in range(P.n)])}
    assert abs(op["cost"][0] - r @ r) <= 4 * op["cost"][2] * DR.EPS * op["cost"][1]
    for name, ref in want.items():
        val, ab, nt = op[name]
        assert (np.abs(val - ref) <= 4 * nt * DR.EPS * ab + 1e-300).all(), name
        assert (ab >= np.abs(val)).all() and np.abs(val).max() > 0.1
    B = DR.blocks(P, R, t)
    assert np.abs(B - np.stack([JtJ[6 * i:6 * i + 6, 6 * i:6 * i + 6] for i in range(P.n)])).max() < 1e-12
    assert np.abs(B - B.transpose(0, 2, 1)).max() == 0.0


def rigid_case(seed=0):
    """The 8 x 8 grid with 6 keyframes; soft priors put every keyframe at its
    rest pose moved by one rigid motion (Rm, tm)."""
    R_rest, g, src, dst, kf = DR.grid_problem(8, 8, 6, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 50))
    Rm, tm = DR.exp_so3(0.4 * rng.standard_normal(3)), rng.uniform(-2, 2, 3)
    n = g.shape[0]
    mode = np.zeros(n, np.uint8)
    mode[kf] = 1
    P = DR.make_problem(R_rest, g, src, dst, None, mode, Rm @ R_rest, g @ Rm.T + tm, 1.0, 1.0)
    return P, kf, Rm, tm


def test_reference_rigid_motion_known_answer():
    """Keyframes with soft priors moved by one rigid motion: the minimiser
    moves every node by that motion, at cost 0."""
    P, kf, Rm, tm = rigid_case()
    assert DR.well_posed(P)
    out = DR.solve(P, rel_tol=0.0)
    eR = np.abs(out["R"] - Rm @ P.R_rest).max()
    et = np.abs(out["t"] - (P.g @ Rm.T + tm)).max()
    print(f"rigid: {out['iterations']} outer iterations, {out['accepted']} accepted, stop {out['stop_reason']}, "
          f"cost {out['cost_final']:.3e}, errors {eR:.3e} {et:.3e}")
    assert eR < 1e-10 and et < 1e-10 and out["cost_final"] < 1e-20
    assert out["stop_reason"] in (3, 4) and out["accepted"] >= 3
    costs = [e["cost"] for e in out["log"]]
    assert all(b <= a for a, b in zip(costs, costs[1:]))  # the cost never rises


def test_reference_well_posedness_and_stop_reasons():
    P, kf, _, _ = rigid_case()
    P.mode[:] = 0
    assert not DR.well_posed(P)
    P.mode[kf[0]] = 1
    P.tau[kf[0]] = 0.0
    assert not DR.well_posed(P)
    P.tau[kf[0]] = 1.0
    assert DR.well_posed(P)
    # priors at rest, on coordinates whose differences are exact: the gradient is 0 at the start
    g = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [3, 1, 4]], np.float64)
    P2 = DR.make_problem(np.tile(np.eye(3), (4, 1, 1)), g, [0, 1, 1, 2, 3, 0], [1, 0, 2, 1, 0, 3], None,
                         np.array([1, 0, 0, 2], np.uint8), None, None, 1.0, 1.0)
    out = DR.solve(P2)
    assert out["stop_reason"] == 5 and out["iterations"] == 0 and out["cost_final"] == 0.0
    P3, _, _, _ = rigid_case()
    out = DR.solve(P3, max_iterations=2)
    assert out["stop_reason"] == 3 and out["iterations"] == 2
    assert DR.solve(P3, abs_tol=1e-6)["stop_reason"] == 2


# ------------------------------------------------------------------- helpers
def test_simplify_voxel_first_vertex_per_voxel():
    from kmx.pgmo import simplify_voxel
    xyz = np.array([[0.1, 0.1, 0.1], [0.9, 0.8, 0.2],     # one voxel at resolution 1: vertex 0 represents it
                    [1.5, 0.1, 0.1], [0.2, 1.5, 0.1], [-0.1, 0.1, 0.1], [1.6, 0.2, 0.3]], np.float32)
    stamp = np.arange(6, dtype=np.int64) * 10
    robot = np.zeros(6, np.int32)
    faces = np.array([[0, 2, 3],    # kept
                      [0, 1, 2],    # collapses: 0 and 1 share a voxel
                      [1, 5, 3],    # the same control vertices as the first face: a duplicate
                      [3, 0, 2],    # a duplicate in another order
                      [4, 2, 3]], np.int32)
    cx, cs, cr, cf, vmap = simplify_voxel(xyz, faces, stamp, robot, 1.0)
    assert list(vmap) == [0, 0, 1, 2, 3, 1] and vmap.dtype == np.int32
    assert np.array_equal(cx, xyz[[0, 2, 3, 4]].astype(np.float64)) and cx.dtype == np.float64
    assert list(cs) == [0, 20, 30, 40] and list(cr) == [0, 0, 0, 0]
    assert cf.tolist() == [[0, 1, 2], [3, 1, 2]] and cf.dtype == np.int32
    # negative coordinates floor away from zero: -0.1 and 0.1 are different voxels
    assert vmap[4] != vmap[0]
    # a finer grid keeps every vertex
    _, _, _, cf2, vmap2 = simplify_voxel(xyz, faces, stamp, robot, 0.05)
    assert list(vmap2) == list(range(6)) and cf2.shape[0] == 4  # [3, 0, 2] repeats [0, 2, 3]
    with pytest.raises(ValueError):
        simplify_voxel(xyz, faces, stamp, robot, 0.0)
    with pytest.raises(ValueError):
        simplify_voxel(xyz, np.array([[0, 1, 6]]), stamp, robot, 1.0)
    out = simplify_voxel(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), [], [], 1.0)
    assert out[0].shape == (0, 3) and out[3].shape == (0, 3) and out[4].shape == (0,)


def test_simplify_voxel_horizon():
    """One voxel seen at 0.0, 0.4, 1.2 and 1.3 s: one control vertex without a
    horizon, one per window of 1 s with it."""
    from kmx.pgmo import simplify_voxel
    xyz = np.full((4, 3), 0.5, np.float32)
    stamp = np.array([0, 400_000_000, 1_200_000_000, 1_300_000_000], np.int64)
    none = np.zeros((0, 3), np.int32)
    assert list(simplify_voxel(xyz, none, stamp, np.zeros(4, np.int32), 1.0)[4]) == [0, 0, 0, 0]
    cx, cs, cr, cf, vmap = simplify_voxel(xyz, none, stamp, np.zeros(4, np.int32), 1.0, horizon_s=1.0)
    assert list(vmap) == [0, 0, 1, 1] and list(cs) == [0, 1_200_000_000]
    with pytest.raises(ValueError):
        simplify_voxel(xyz, none, stamp, np.zeros(4, np.int32), 1.0, horizon_s=0.0)


def test_simplify_voxel_keeps_robots_apart():
    from kmx.pgmo import simplify_voxel
    xyz = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.6, 0.5, 0.5]], np.float32)
    cx, cs, cr, cf, vmap = simplify_voxel(xyz, np.zeros((0, 3), np.int32), [5, 6, 7], [0, 1, 0], 1.0)
    assert list(vmap) == [0, 1, 0] and list(cr) == [0, 1] and list(cs) == [5, 6]


def test_graph_from_mesh_edges_and_links():
    from kmx.pgmo import graph_from_mesh
    cx = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], np.float64)
    faces = np.array([[0, 1, 2], [2, 1, 0]])  # two faces over the same three edges
    kf_stamp = [np.array([0, 10], np.int64), np.array([10], np.int64)]
    rot = DR.exp_so3(np.array([[0.1, 0, 0], [0, 0.2, 0], [0, 0, 0.3]]))
    kf_rest = [(rot[:2], np.array([[0, 0, 1.0], [1, 0, 1]])), (rot[2:], np.array([[5.0, 5, 6]]))]
    G = graph_from_mesh(cx, [0, 10, 10, 10], [0, 0, 0, 1], faces, kf_stamp, kf_rest, w_mesh=2.0, w_link=3.0)
    assert G["n_keyframes"] == 3 and list(G["kf_offset"]) == [0, 2, 3]
    assert G["g"].shape == (7, 3) and np.array_equal(G["g"][3:], cx) and np.array_equal(G["R_rest"][:3], rot)
    assert np.array_equal(G["R_rest"][3:], np.tile(np.eye(3), (4, 1, 1)))
    assert list(G["robot"]) == [0, 0, 1, 0, 0, 0, 1] and list(G["stamp"]) == [0, 10, 10, 0, 10, 10, 10]
    edges = list(zip(G["src"].tolist(), G["dst"].tolist(), G["w"].tolist()))
    mesh = [(3, 4), (4, 3), (3, 5), (5, 3), (4, 5), (5, 4)]
    link = [(3, 0), (0, 3), (4, 1), (1, 4), (5, 1), (1, 5), (6, 2), (2, 6)]  # stamp and robot pick the keyframe
    assert edges == [(a, b, 2.0) for a, b in mesh] + [(a, b, 3.0) for a, b in link]
    assert G["src"].dtype == np.int32 and G["dst"].dtype == np.int32 and list(G["link"]) == [0, 1, 1, 2]
    with pytest.raises(ValueError, match="no keyframe"):
        graph_from_mesh(cx, [0, 10, 10, 11], [0, 0, 0, 1], faces, kf_stamp, kf_rest)
    with pytest.raises(ValueError):
        graph_from_mesh(cx, [0, 10, 10, 10], [0, 0, 0, 2], faces, kf_stamp, kf_rest)
    # the graph of a mesh is well posed once its keyframes carry priors
    mode = np.zeros(7, np.uint8)
    mode[:3] = 1
    assert DR.well_posed(DR.make_problem(G["R_rest"], G["g"], G["src"], G["dst"], G["w"], mode, None, None, 1.0, 1.0))


def test_synthetic_mesh_gives_a_well_posed_graph():
    from kmx.pgmo import graph_from_mesh, simplify_voxel
    from kmx.synth import make_pose_graph
    from kmx.synth.mesh import make_mesh
    g = make_pose_graph(2, 60, 60, seed=3)
    mesh = make_mesh(g, 6, 3.0, 1)
    cx, cs, cr, cf, vmap = simplify_voxel(mesh.xyz, mesh.faces, mesh.stamp, mesh.robot, 1.0)
    assert 0 < cx.shape[0] < mesh.xyz.shape[0] and vmap.shape[0] == mesh.xyz.shape[0]
    assert np.array_equal(cr[vmap], mesh.robot)
    G = graph_from_mesh(cx, cs, cr, cf, mesh.kf_stamp, list(zip(mesh.rest_R, mesh.rest_t)))
    n = G["g"].shape[0]
    assert n == 60 + cx.shape[0] and G["src"].shape[0] % 2 == 0
    mode = np.zeros(n, np.uint8)
    mode[:60] = 1
    P = DR.make_problem(G["R_rest"], G["g"], G["src"], G["dst"], G["w"], mode, None, None, 1.0, 1.0)
    assert DR.well_posed(P)


# ----------------------------------------------------------------------- ABI
def test_abi_structs_symbols_and_error_mapping():
    from kmx import abi
    assert C.sizeof(abi.DgraphParams) == 72 and abi.DgraphParams.max_iterations.offset == 56
    assert abi.DgraphParams.cg_rtol.offset == 48 and abi.DgraphParams.reserved.offset == 68
    assert C.sizeof(abi.DgraphResult) == 48 and abi.DgraphResult.iterations.offset == 32
    assert abi.DgraphResult.cg_iterations.offset == 44
    assert C.sizeof(abi.DgraphLogEntry) == 32 and abi.DgraphLogEntry.cg_iterations.offset == 24
    L = abi.lib()
    hdr = (ROOT / "include" / "kmx_abi.h").read_text()
    names = sorted(set(re.findall(r"^\s*int\s+(kmx_dgraph_\w+)\s*\(", hdr, re.M)))
    assert names == sorted("kmx_dgraph_" + s for s in (
        "create", "destroy", "set_stream", "set_graph", "set_weights", "set_priors", "set_poses", "get_poses", "eval",
        "solve", "get_log", "get_timing"))
    for name in names:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    for k, v in enumerate(("COST", "GRAD", "JTJ", "BLOCKS")):
        assert re.search(rf"KMX_DGRAPH_EVAL_{v} = {k}\b", hdr) and getattr(abi, "KMX_DGRAPH_EVAL_" + v) == k
    # checked before any device call
    h = C.c_void_p()
    assert L.kmx_dgraph_create(0, None) == abi.KMX_EINVAL
    assert L.kmx_dgraph_destroy(None) == abi.KMX_OK
    for fn, args in (("set_stream", (None,)), ("set_graph", (0, None, None, 0, None, None, None)),
                     ("set_weights", (None,)), ("set_priors", (None, None, None, None, None)),
                     ("set_poses", (None, None)), ("get_poses", (None, None)), ("solve", (None, None)),
                     ("get_log", (0, None, None)), ("get_timing", (None,))):
        assert getattr(L, "kmx_dgraph_" + fn)(None, *args) == abi.KMX_EINVAL, fn
    out = np.zeros(1)
    assert L.kmx_dgraph_eval(None, 0, None, abi.fptr(out)) == abi.KMX_EINVAL
    assert L.kmx_dgraph_eval(None, 4, None, abi.fptr(out)) == abi.KMX_EUNSUP
    assert L.kmx_dgraph_eval(None, -1, None, abi.fptr(out)) == abi.KMX_EUNSUP
    for field, bad, code in (("lambda_factor", 1.0, abi.KMX_EINVAL), ("lambda_init", -1.0, abi.KMX_EINVAL),
                             ("cg_rtol", float("nan"), abi.KMX_EINVAL), ("abs_tol", float("inf"), abi.KMX_EINVAL),
                             ("max_iterations", -1, abi.KMX_EINVAL), ("check_every", -5, abi.KMX_EINVAL),
                             ("reserved", 1, abi.KMX_EUNSUP)):
        p = abi.DgraphParams()
        setattr(p, field, bad)
        assert L.kmx_dgraph_solve(None, C.byref(p), None) == code, field
    assert b"lambda_factor" in L.kmx_last_error() or b"reserved" in L.kmx_last_error()
    from kmx.pgmo import DeformationGraph  # noqa: F401  (exported)
    if abi.device_count() == 0:
        with pytest.raises(abi.KmxError, match="kmx_dgraph_create"):
            DeformationGraph()


def test_make_dgraph_check():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc is missing")
    r = subprocess.run(["make", "-s", "-C", str(ROOT / "kimera-multi_amd" / "csrc"), "dgraph_check", f"HIPCC={hipcc}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dgraph_check ok" in r.stdout
