"""Mesh deformation on the device (kmx_mesh_*, csrc/mesh.hip) against the
contract in numpy (tests/mesh_ref.py): bindings exactly (ids and counts;
weights within 4 ulp), deformed positions within max(1 fp32 ulp, 1e-12 scale),
streaming, the device-output form, errors, and the pipeline's mesh stage."""
import numpy as np
import pytest

from tests import mesh_ref as MR
from tests.test_mesh_cpu import _rigid, _scene

pytestmark = pytest.mark.gpu

SEC = 1_000_000_000


def _deformer(s, k=4, W=SEC, n_robots=None, vertices=True):
    from kmx.pgmo import MeshDeformer
    R = int(max(s["robot"].max(initial=0), s["v_robot"].max(initial=0)) + 1) if n_robots is None else n_robots
    md = MeshDeformer(k=k, window_ns=W, n_robots=R)
    md.add_nodes(s["robot"], s["stamp"], s["R_rest"], s["g"])
    if vertices:
        md.add_vertices(s["v_robot"], s["v_stamp"], s["xyz"])
    return md


def _ref_bind(s, k=4, W=SEC):
    return MR.bind(s["robot"], s["stamp"], s["g"], s["v_robot"], s["v_stamp"], s["xyz"], k, W)


def _assert_bindings(got, ref):
    (gi, gw, gc), (ri, rw, rc) = got, ref
    assert np.array_equal(gc, rc), np.nonzero(gc != rc)[0][:8]
    assert np.array_equal(gi, ri), np.nonzero((gi != ri).any(1))[0][:8]
    assert (np.abs(gw - rw) <= 4 * np.spacing(rw)).all(), np.abs(gw - rw).max()


def _scale(s, p=None):
    return max(np.abs(s["g"]).max(initial=0), np.abs(s["xyz"]).max(initial=0), 0.0 if p is None else np.abs(p).max())


def _assert_positions(got, ref, scale):
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    tol = MR.tolerance(ref, scale)
    assert (err <= tol).all(), (err / tol).max()


def _moved(s, seed=11):
    """Current poses: every node's rest pose moved by a rigid map of its own."""
    from kmx.synth.pose_graph import random_rotations
    rng = np.random.Generator(np.random.PCG64(seed))
    n = s["g"].shape[0]
    return random_rotations(rng, n), s["g"] + rng.uniform(-1, 1, (n, 3))


def _custom(node_robot, node_stamp, g, v_robot, v_stamp, xyz):
    n = len(node_robot)
    return dict(robot=np.asarray(node_robot, np.int32), stamp=np.asarray(node_stamp, np.int64),
                R_rest=np.tile(np.eye(3), (n, 1, 1)), g=np.asarray(g, np.float64).reshape(n, 3),
                v_robot=np.asarray(v_robot, np.int32), v_stamp=np.asarray(v_stamp, np.int64),
                xyz=np.asarray(xyz, np.float32).reshape(-1, 3))


# ---------------------------------------------------------------- 1. bindings
def test_candidate_counts(gpu):
    """One robot per candidate count m = 0, 1, 2, 4, 5, 6, 40 (k = 4), W = 0."""
    ms = [0, 1, 2, 4, 5, 6, 40]
    rng = np.random.Generator(np.random.PCG64(0))
    robot = np.concatenate([np.full(m, r, np.int32) for r, m in enumerate(ms)])
    n = robot.shape[0]
    v_robot = np.repeat(np.arange(len(ms), dtype=np.int32), 9)
    s = _custom(robot, np.full(n, 7), rng.uniform(-5, 5, (n, 3)), v_robot, np.full(v_robot.shape[0], 7),
                rng.uniform(-5, 5, (v_robot.shape[0], 3)))
    md = _deformer(s, W=0, n_robots=len(ms))
    got, ref = md.bindings(), _ref_bind(s, W=0)
    _assert_bindings(got, ref)
    assert [int(c) for c in got[2][::9]] == [0, 1, 1, 3, 4, 4, 4]
    xyz, st = md.deform()
    assert st["unbound"] == 9 and st["partial"] == 27 and st["vertices"] == 63
    assert np.array_equal(xyz[:9], s["xyz"][:9])  # the unbound ones come back bit for bit
    md.close()


@pytest.mark.parametrize("n_verts", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("n_robots", [1, 2, 3])
def test_wave_and_workgroup_edges(gpu, n_verts, n_robots):
    """Vertices of two and three robots alternate inside one workgroup; their
    stamps are node stamps, so both window ends fall exactly on nodes."""
    s = _scene(20 + n_robots, n_nodes=90, n_verts=n_verts, n_robots=n_robots)
    md = _deformer(s, W=3 * SEC // 10, n_robots=n_robots)
    _assert_bindings(md.bindings(), _ref_bind(s, W=3 * SEC // 10))
    md.close()


@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("W", [0, SEC])
def test_k_and_window(gpu, k, W):
    s = _scene(31, n_nodes=120, n_verts=300, n_robots=2)
    s["stamp"] = (s["stamp"] // (2 * 100_000_000)) * (2 * 100_000_000)  # pairs of nodes share a stamp: m = 2 at W = 0
    s["v_stamp"] = s["stamp"][s["src"]].copy()
    md = _deformer(s, k=k, W=W)
    ref = _ref_bind(s, k=k, W=W)
    _assert_bindings(md.bindings(), ref)
    assert W != 0 or set(ref[2]) == {1}
    md.close()


def test_window_ends_inclusive(gpu):
    stamps = [0, 100, 200, 300, 400, 500, 600]
    g = [[j, 0, 0] for j in range(7)]
    s = _custom([0] * 7, stamps, g, [0, 0, 0], [300, 301, 299], [[3.2, 0, 0]] * 3)
    md = _deformer(s, k=8, W=200)
    got = md.bindings()
    _assert_bindings(got, _ref_bind(s, k=8, W=200))
    assert list(got[2]) == [4, 3, 3]
    assert list(got[0][0][:4]) == [3, 4, 2, 5]  # 100 .. 500: nodes 1 .. 5, m = 5; node 1 is the farthest
    assert list(got[0][1][:3]) == [3, 4, 2]     # 101 .. 501: nodes 2 .. 5
    assert list(got[0][2][:3]) == [3, 4, 2]     # 99 .. 499: nodes 1 .. 4
    assert got[1][1][2] != got[1][2][2]         # not the same d_max
    md.close()


def test_saturating_window(gpu):
    lo, hi = MR.I64_MIN, MR.I64_MAX
    s = _custom([0] * 4, [lo, -5, 5, hi], [[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], [0] * 4, [lo, hi, 0, -1],
                [[0.1, 0, 0]] * 4)
    for W in (10, hi):
        md = _deformer(s, k=2, W=W)
        _assert_bindings(md.bindings(), _ref_bind(s, k=2, W=W))
        md.close()


def test_ties_fallbacks_and_coincident_points(gpu):
    v0 = [10, 20, 30]
    mirrored = [[13, 20, 30], [7, 20, 30], [10, 24, 30], [10, 16, 30], [10, 20, 35], [10, 20, 25], [10, 20, 37]]
    sphere = [[3, 0, 0], [-3, 0, 0], [0, 3, 0], [0, -3, 0], [0, 0, 3], [0, 0, -3]]
    same = [[1, 2, 3]] * 5
    on_node = [[5, 5, 5], [6, 5, 5], [5, 7, 5], [9, 9, 9], [5, 5, 1], [0, 0, 0]]
    groups = [mirrored, sphere, same, on_node]
    robot = np.concatenate([np.full(len(gr), r) for r, gr in enumerate(groups)])
    s = _custom(robot, np.zeros(robot.shape[0]), np.concatenate(groups), [0, 1, 2, 3], [0] * 4,
                [v0, [0, 0, 0], [1, 2, 3], [5, 5, 5]])
    md = _deformer(s, W=0, n_robots=4)
    idx, w, cnt = md.bindings()
    _assert_bindings((idx, w, cnt), _ref_bind(s, W=0))
    assert list(idx[0]) == [0, 1, 2, 3] and w[0, 0] == w[0, 1] and w[0, 2] == w[0, 3]  # ties: the lower id first
    assert (cnt[1], idx[1, 0], w[1, 0], idx[1, 1]) == (1, 7, 1.0, -1)  # all used nodes at d_max
    assert (cnt[2], idx[2, 0], w[2, 0]) == (1, 13, 1.0)                # d_max = 0
    assert cnt[3] == 4 and idx[3, 0] == 18 and w[3, 0] > w[3, 1]       # d = 0: the largest weight
    for k in (1, 8):
        mk = _deformer(s, k=k, W=0, n_robots=4)
        _assert_bindings(mk.bindings(), _ref_bind(s, k=k, W=0))
        mk.close()
    md.close()


def test_global_path_equals_staged_path(gpu):
    """256 vertices of one workgroup whose windows span 3000 nodes: more than
    the workgroup stages, so it reads global memory. The same vertices bound
    eight at a time (neighbours in time: a small union) take the staged path."""
    rng = np.random.Generator(np.random.PCG64(8))
    n = 3000
    stamp = np.arange(n, dtype=np.int64) * 100
    g = np.cumsum(rng.uniform(-1, 1, (n, 3)), 0)
    src = np.sort(rng.integers(0, n, 256))
    s = _custom(np.zeros(n), stamp, g, np.zeros(256), stamp[src] + rng.integers(-50, 50, 256),
                g[src] + rng.uniform(-2, 2, (256, 3)))
    big = _deformer(s, W=2000)
    assert big.info()["lds_nodes"] < n
    got_big = big.bindings()
    info = big.info()
    assert (info["last_bind_blocks"], info["last_bind_global_blocks"]) == (1, 1)
    small = _deformer(s, W=2000)
    for first in range(0, 256, 8):
        small.bind(first, 8)
        assert small.info()["last_bind_global_blocks"] == 0
    small._bound = 256
    got_small = small.bindings()
    for a, b in zip(got_big, got_small):
        assert np.array_equal(a, b)
    _assert_bindings(got_big, _ref_bind(s, W=2000))
    assert (got_big[2] == 4).all()
    big.close()
    small.close()


# --------------------------------------------------------------- 2. positions
@pytest.fixture(scope="module")
def scene():
    s = _scene(41, n_nodes=200, n_verts=1500, n_robots=3)
    s["v_stamp"][:5] += 500 * SEC  # five vertices out of every window: unbound
    s["R_cur"], s["p"] = _moved(s)
    s["ref_bind"] = _ref_bind(s)
    s["ref_out"], s["ref_stats"] = MR.deform(s["xyz"], *s["ref_bind"], s["R_rest"], s["g"], s["R_cur"], s["p"])
    return s


def test_deform_matches_reference(gpu, scene):
    s = scene
    md = _deformer(s)
    md.set_node_poses(0, s["R_cur"], s["p"])
    out, st = md.deform()
    _assert_bindings(md.bindings(), s["ref_bind"])
    _assert_positions(out, s["ref_out"], _scale(s, s["p"]))
    assert st["unbound"] == 5 and np.array_equal(out[:5], s["xyz"][:5])
    assert (st["vertices"], st["unbound"], st["partial"]) == tuple(s["ref_stats"][k] for k in
                                                                   ("vertices", "unbound", "partial"))
    for key in ("max_displacement", "sum_sq_displacement"):
        assert abs(st[key] - s["ref_stats"][key]) <= 1e-12 * s["ref_stats"][key], key
    # again: identical bits, identical statistics
    out2, st2 = md.deform()
    assert np.array_equal(out, out2) and st == st2
    md.update_trajectory(0, s["R_cur"][s["robot"] == 0], s["p"][s["robot"] == 0])
    out3, st3 = md.deform()
    assert np.array_equal(out, out3) and st == st3
    t = md.timing()
    assert t["bind_ms"] > 0 and t["deform_ms"] > 0
    md.close()


def test_rigid_and_identity_on_the_device(gpu, scene):
    s = scene
    md = _deformer(s)
    out, st = md.deform()  # current = rest
    assert np.array_equal(out, s["xyz"]) and st["max_displacement"] == 0.0 and st["sum_sq_displacement"] == 0.0
    T_R, T_t = _rigid(np.random.Generator(np.random.PCG64(3)))
    p = s["g"] @ T_R.T + T_t
    for a in range(3):
        sel = s["robot"] == a
        md.update_trajectory(a, T_R[None] @ s["R_rest"][sel], p[sel])
    out, st = md.deform()
    want = s["xyz"].astype(np.float64) @ T_R.T + T_t
    bound = np.arange(5, s["xyz"].shape[0])
    err = np.abs(out[bound].astype(np.float64) - want[bound])
    assert (err <= MR.tolerance(want[bound], _scale(s, p))).all()
    assert np.array_equal(out[:5], s["xyz"][:5])
    md.close()


# --------------------------------------------------------------- 3. streaming
def test_streaming_vertices_in_five_uneven_calls(gpu, scene):
    s = scene
    one = _deformer(s)
    one.set_node_poses(0, s["R_cur"], s["p"])
    out1, st1 = one.deform()
    b1 = one.bindings()
    five = _deformer(s, vertices=False)
    five.set_node_poses(0, s["R_cur"], s["p"])
    cuts = [0, 1, 64, 321, 1100, 1500]
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert five.add_vertices(s["v_robot"][a:b], s["v_stamp"][a:b], s["xyz"][a:b]) == a
        five.deform(first=a, n=b - a)  # binds this call's vertices
    out5, st5 = five.deform()
    for x, y in zip(b1, five.bindings()):
        assert np.array_equal(x, y)
    assert np.array_equal(out1, out5) and st1 == st5
    inf = five.info()
    assert inf["n_vertices"] == 1500 and inf["n_nodes"] == 200 and inf["vertex_capacity"] >= 1500
    assert list(inf["vertices_per_robot"]) == [int((s["v_robot"] == a).sum()) for a in range(3)]
    assert list(inf["nodes_per_robot"]) == [int((s["robot"] == a).sum()) for a in range(3)]
    one.close()
    five.close()


def test_nodes_appended_after_a_bind(gpu, scene):
    s = scene
    half = {k: (v[s["stamp"] < 3 * SEC] if k in ("robot", "stamp", "R_rest", "g") else v) for k, v in s.items()}
    late = s["stamp"] >= 3 * SEC
    md = _deformer(half, n_robots=3)
    before = md.bindings()
    _assert_bindings(before, _ref_bind(half))
    md.add_nodes(s["robot"][late], s["stamp"][late], s["R_rest"][late], s["g"][late])
    for x, y in zip(before, md.bindings()):  # earlier bindings stand
        assert np.array_equal(x, y)
    md.rebind()
    full = dict(s)
    order = np.concatenate([np.nonzero(~late)[0], np.nonzero(late)[0]])  # the ids the handle gave
    for key in ("robot", "stamp", "R_rest", "g"):
        full[key] = s[key][order]
    fresh = _deformer(full, n_robots=3)
    for x, y in zip(md.bindings(), fresh.bindings()):
        assert np.array_equal(x, y)
    _assert_bindings(md.bindings(), _ref_bind(full))
    assert not np.array_equal(before[0], md.bindings()[0])
    md.close()
    fresh.close()


# ----------------------------------------------------------- 4. device output
_TORCH_CHILD = """
import sys
sys.path[:0] = [{root!r} + "/kimera-multi_amd", {root!r}]
import numpy as np
import torch
torch.cuda.set_device(0)
torch.cuda.init()  # torch takes the device before the first kmx handle, as in kmx.dpgo.driver
from tests.test_mesh_gpu import _deformer, _moved
from tests.test_mesh_cpu import _scene
s = _scene(41, n_nodes=200, n_verts=1500, n_robots=3)
md = _deformer(s)
md.set_node_poses(0, *_moved(s))
host, _ = md.deform()
assert np.abs(host - s["xyz"]).max() > 0.1
t = torch.zeros((1500, 3), dtype=torch.float32, device="cuda:0")
torch.cuda.synchronize()
got, st = md.deform(out=t)
assert got is t and st is None
md.sync()
assert np.array_equal(t.cpu().numpy(), host)
part = torch.zeros((100, 3), dtype=torch.float32, device="cuda:0")
torch.cuda.synchronize()
md.deform(out=part, first=700, n=100)
md.sync()
assert np.array_equal(part.cpu().numpy(), host[700:800])
for bad in (torch.zeros((1500, 3)), torch.zeros((1499, 3), device="cuda:0"),
            torch.zeros((1500, 3), dtype=torch.float64, device="cuda:0")):
    try:
        md.deform(out=bad)
    except ValueError:
        continue
    raise AssertionError("accepted a wrong tensor")
md.close()
print("device output ok")
"""


def test_deform_device_equals_host_form(gpu):
    """In a process of its own: torch has to take the device before the first
    kmx handle of a process does, and this session's earlier tests already
    hold it."""
    import subprocess
    import sys
    from pathlib import Path
    root = str(Path(__file__).resolve().parents[1])
    r = subprocess.run([sys.executable, "-c", _TORCH_CHILD.format(root=root)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "device output ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------ 5. errors
def test_errors_leave_the_handle_usable(gpu, scene):
    from kmx import abi
    from kmx.pgmo import MeshDeformer
    s = scene
    for k in (0, 9):
        with pytest.raises(abi.KmxError, match=r"\(-5\)"):
            MeshDeformer(k=k, n_robots=3)
    md = _deformer(s)
    md.set_node_poses(0, s["R_cur"], s["p"])
    out0, st0 = md.deform()
    eye, zero = np.eye(3)[None], np.zeros((1, 3))
    last0 = int(s["stamp"][s["robot"] == 0].max())
    bad_calls = [
        lambda: md.add_nodes([0], [last0 - 1], eye, zero),                     # stamps go backwards
        lambda: md.add_nodes([1, 1], [10 ** 15, 10 ** 15 - 1], np.tile(eye, (2, 1, 1)), np.zeros((2, 3))),
        lambda: md.add_nodes([3], [10 ** 15], eye, zero),                      # robot out of range
        lambda: md.add_nodes([-1], [10 ** 15], eye, zero),
        lambda: md.add_nodes([0], [10 ** 15], eye * np.nan, zero),
        lambda: md.add_vertices([0, 0], [0, 0], [[0, 0, 0], [0, np.nan, 0]]),   # NaN vertex
        lambda: md.add_vertices([0, 3], [0, 0], np.zeros((2, 3))),
        lambda: md.bind(1499, 2),                                              # range past the end
        lambda: md.bind(-1, 1),
        lambda: md.deform(first=1000, n=501),
        lambda: md.bindings(first=1501, n=0),
        lambda: md.set_node_poses(199, np.tile(eye, (2, 1, 1)), np.zeros((2, 3))),
        lambda: md.set_node_poses(0, eye, np.full((1, 3), np.inf)),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(abi.KmxError, match=r"\(-1\)"):
            call()
        inf = md.info()
        assert (inf["n_nodes"], inf["n_vertices"]) == (200, 1500), i
        out, st = md.deform()
        assert np.array_equal(out, out0) and st == st0, i
    assert md.n_nodes == 200 and md.n_vertices == 1500
    # n = 0 is a legal call everywhere
    md.add_nodes(np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros((0, 3, 3)), np.zeros((0, 3)))
    md.add_vertices(np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros((0, 3), np.float32))
    out, st = md.deform(first=1500, n=0)
    assert out.shape == (0, 3) and st["vertices"] == 0
    md.close()


# ---------------------------------------------------------------- 6. pipeline
def test_pipeline_mesh_stage(gpu):
    from kmx import pipeline as PL
    from kmx.lcd import LcdParams
    from kmx.synth.mesh import make_mesh
    from tests.test_pipeline_gpu import _setup
    g0, st, P = _setup()
    mesh = make_mesh(g0, 2, 3.0, 5)
    out = PL.run_pipeline(g0, st, P, LcdParams(), rounds=10, device=0, mesh=mesh, return_trajectory=True)
    m = out["mesh"]
    print({k: v for k, v in m.items() if k != "xyz"})
    assert m["vertices"] == 6000 and m["unbound"] == 0
    assert m["rmse_after_m"] < m["rmse_before_m"]
    assert m["bind_seconds"] > 0 and m["deform_seconds"] > 0
    traj = out["trajectory"]
    cat = np.concatenate
    node_robot = cat([np.full(int(g0.n_poses[a]), a, np.int32) for a in range(3)])
    R_cur, p = cat([traj[a][0] for a in range(3)]), cat([traj[a][1] for a in range(3)])
    ref, rst, _ = MR.deform_all(node_robot, cat(mesh.kf_stamp), cat(mesh.rest_R), cat(mesh.rest_t), R_cur, p,
                                mesh.robot, mesh.stamp, mesh.xyz, 4, SEC)
    scale = max(np.abs(cat(mesh.rest_t)).max(), np.abs(p).max(), np.abs(mesh.xyz).max())
    _assert_positions(m["xyz"], ref, scale)
    assert rst["unbound"] == 0
