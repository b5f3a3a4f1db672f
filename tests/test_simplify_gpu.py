"""The device simplification (kmx.pgmo.MeshSimplifier, csrc/simplify.hip)
against the numpy reference (kmx.pgmo.simplify_voxel, graph_from_mesh) on the
same input: every array equal value for value, with equal dtype and shape.
There is no tolerance: every output is an integer, a copied input or a given
constant."""
import functools

import numpy as np
import pytest

from kmx.pgmo import MeshSimplifier, graph_from_mesh, simplify_voxel, simplify_voxel_gpu

pytestmark = pytest.mark.gpu

HUB = 32  # simplify.hip's SIMP_HUB: an edge bucket above it takes the wave-per-bucket kernel


def same(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    assert np.array_equal(got, ref), what


def same_five(got, ref):
    for name, a, b in zip(("control_xyz", "control_stamp", "control_robot", "control_faces", "vertex_to_control"),
                          got, ref):
        same(a, b, name)


def same_graph(got, ref):
    assert set(got) == set(ref)
    for k in ref:
        if k == "n_keyframes":
            assert got[k] == ref[k]
        else:
            same(got[k], ref[k], k)


def ref_edges(faces):
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    E = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]) if F.shape[0] else np.zeros((0, 2), np.int64)
    E = np.sort(E, axis=1)
    return np.unique(E[E[:, 0] != E[:, 1]], axis=0).astype(np.int32).reshape(-1, 2)


def five(ms):
    return (*ms.control(), ms.faces(), ms.vertex_map())


def keyframes_of(stamp, robot, n_robots):
    """One keyframe per distinct stamp of every robot, each stamp twice so that 'the first' matters."""
    ks = [np.repeat(np.unique(stamp[robot == a]), 2).astype(np.int64) for a in range(n_robots)]
    rng = np.random.Generator(np.random.PCG64(11))
    rest = [(np.tile(np.eye(3), (k.shape[0], 1, 1)), rng.uniform(-1, 1, (k.shape[0], 3))) for k in ks]
    return ks, rest


@functools.lru_cache(maxsize=None)
def dense(half: float):
    rng = np.random.Generator(np.random.PCG64(3))
    V, F = 20_000, 60_000
    xyz = rng.uniform(-half, half, (V, 3)).astype(np.float32)
    robot = rng.integers(0, 2, V).astype(np.int32)
    stamp = rng.integers(0, 50, V).astype(np.int64) * 100_000_000
    a = rng.integers(0, V, F)
    faces = np.stack([a, (a + rng.integers(0, 40, F)) % V, (a + rng.integers(0, 40, F)) % V], 1).astype(np.int32)
    for arr in (xyz, robot, stamp, faces):
        arr.setflags(write=False)
    return xyz, faces, stamp, robot


@functools.lru_cache(maxsize=None)
def dense_ref(half: float, horizon_s):
    xyz, faces, stamp, robot = dense(half)
    ref = simplify_voxel(xyz, faces, stamp, robot, 1.0, horizon_s=horizon_s)
    for arr in ref:
        arr.setflags(write=False)
    return ref


def check_all(xyz, faces, stamp, robot, resolution, horizon_s, n_robots, w_mesh=1.0, w_link=1.0, ref=None):
    ref = simplify_voxel(xyz, faces, stamp, robot, resolution, horizon_s=horizon_s) if ref is None else ref
    ks, rest = keyframes_of(np.asarray(stamp, np.int64), np.asarray(robot, np.int32), n_robots)
    G = graph_from_mesh(ref[0], ref[1], ref[2], ref[3], ks, rest, w_mesh=w_mesh, w_link=w_link)
    with MeshSimplifier(resolution, horizon_s, n_robots) as ms:
        ms.add(xyz, faces, stamp, robot)
        same_five(five(ms), ref)
        E = ms.edges()
        same(E, ref_edges(ref[3]), "edges")
        same_graph(ms.graph(ks, rest, w_mesh=w_mesh, w_link=w_link), G)
        info = ms.info()
    assert info["n_control"] == ref[0].shape[0] and info["n_faces_kept"] == ref[3].shape[0]
    big = int(np.bincount(E[:, 0]).max()) if E.shape[0] else 0
    return ref, G, big


# ------------------------------------------------------ 1. pipeline-shaped mesh
@pytest.mark.parametrize("horizon_s", [None, 2.0])
def test_pipeline_shaped_mesh(gpu, horizon_s):
    from kmx.synth import make_pose_graph
    from kmx.synth.mesh import make_mesh
    g = make_pose_graph(3, 6000, 0, seed=0)
    mesh = make_mesh(g, 6, 3.0, 1)
    assert mesh.xyz.shape[0] == 36_000 and mesh.faces.shape[0] == 24_000
    ref = simplify_voxel(mesh.xyz, mesh.faces, mesh.stamp, mesh.robot, 0.5, horizon_s=horizon_s)
    rest = list(zip(mesh.rest_R, mesh.rest_t))
    G = graph_from_mesh(ref[0], ref[1], ref[2], ref[3], mesh.kf_stamp, rest)
    print(f"control {ref[0].shape[0]}, faces {ref[3].shape[0]}, directed edges {G['src'].shape[0]}")
    assert 30_000 < ref[0].shape[0] < 36_000 and 20_000 < ref[3].shape[0] < 24_000  # it merges, but little
    with MeshSimplifier(0.5, horizon_s, 3) as ms:
        ms.add(mesh.xyz, mesh.faces, mesh.stamp, mesh.robot)
        same_five(five(ms), ref)
        same_graph(ms.graph(mesh.kf_stamp, rest), G)
    same_five(simplify_voxel_gpu(mesh.xyz, mesh.faces, mesh.stamp, mesh.robot, 0.5, horizon_s=horizon_s), ref)


# ------------------------------------------------------------- 2. dense box
@pytest.mark.parametrize("half,horizon_s", [(4.0, None), (4.0, 1.0), (1.5, None)])
def test_dense_box(gpu, half, horizon_s):
    xyz, faces, stamp, robot = dense(half)
    ref, G, big = check_all(xyz, faces, stamp, robot, 1.0, horizon_s, 2, w_mesh=2.0, w_link=0.5,
                            ref=dense_ref(half, horizon_s))
    vmap = ref[4]
    mapped = vmap[faces]
    degenerate = int(((mapped[:, 0] == mapped[:, 1]) | (mapped[:, 1] == mapped[:, 2]) |
                      (mapped[:, 0] == mapped[:, 2])).sum())
    print(f"control {ref[0].shape[0]}, most vertices per key {int(np.bincount(vmap).max())}, degenerate {degenerate}, "
          f"duplicate {faces.shape[0] - degenerate - ref[3].shape[0]}, kept {ref[3].shape[0]}, "
          f"edges {(G['src'].shape[0] - 2 * ref[0].shape[0]) // 2}, largest bucket {big}")
    if horizon_s is None:
        assert ref[0].shape[0] == (1024 if half == 4.0 else 128)  # 2 robots x 8^3 or 4^3 voxels, all occupied
    assert big > HUB  # the wave-per-bucket kernel ran
    assert faces.shape[0] - degenerate - ref[3].shape[0] > 0  # duplicates were there to drop


# ------------------------------------------------------ 3. online equals batch
def test_online_equals_batch(gpu):
    xyz, faces, stamp, robot = dense(4.0)
    V = xyz.shape[0]
    cuts = np.cumsum([0, 1, 7, 64, 65, 1000])
    cuts = np.append(cuts, V)
    # a face goes with the append that brings its highest vertex
    order = np.argsort(np.searchsorted(cuts[1:], faces.max(1), side="right"), kind="stable")
    fs = faces[order]
    which = np.searchsorted(cuts[1:], fs.max(1), side="right")
    reach_back = 0
    with MeshSimplifier(1.0, None, 2, initial_slots=64) as ms:
        for i in range(len(cuts) - 1):
            v0, v1 = cuts[i], cuts[i + 1]
            f0, f1 = np.searchsorted(which, i, side="left"), np.searchsorted(which, i, side="right")
            reach_back += int((fs[f0:f1].min(1) < v0).sum())
            first, _, _ = ms.add(xyz[v0:v1], fs[f0:f1], stamp[v0:v1], robot[v0:v1])
            assert first == v0
            ref = simplify_voxel(xyz[:v1], fs[:f1], stamp[:v1], robot[:v1], 1.0)
            same(ms.vertex_map(), ref[4], f"vertex map after append {i}")
            same(ms.faces(), ref[3], f"faces after append {i}")
        same_five(five(ms), ref)
        same(ms.edges(), ref_edges(ref[3]), "edges")
        ks, rest = keyframes_of(stamp, robot, 2)
        G = graph_from_mesh(ref[0], ref[1], ref[2], ref[3], ks, rest)
        same_graph(ms.graph(ks, rest), G)
        info = ms.info()
        streamed = five(ms)
    print(info, "faces reaching into earlier appends:", reach_back)
    assert reach_back > 0
    assert info["vertex_rehashes"] >= 2 and info["face_rehashes"] >= 2
    with MeshSimplifier(1.0, None, 2, initial_slots=64) as one:
        one.add(xyz, fs, stamp, robot)
        same_five(five(one), streamed)


# --------------------------------------------------------- 4. arithmetic edges
def test_division_not_reciprocal(gpu):
    ks = np.array([1, 2, 3, 4, 6, 7])
    x = (49.0 * ks).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), 49.0 * ks)  # exact in fp32
    assert np.array_equal(np.floor(x.astype(np.float64) * (1.0 / 49.0)), ks - 1)
    assert np.array_equal(np.floor(x.astype(np.float64) / 49.0), ks)
    # each 49 k beside 49 k - 0.5: the reciprocal would put both in voxel k - 1
    xyz = np.zeros((12, 3), np.float32)
    xyz[0::2, 0] = x
    xyz[1::2, 0] = x - np.float32(0.5)
    stamp, robot = np.zeros(12, np.int64), np.zeros(12, np.int32)
    none = np.zeros((0, 3), np.int32)
    ref = simplify_voxel(xyz, none, stamp, robot, 49.0)
    assert ref[0].shape[0] == 8  # voxels 0 (48.5), 1 (49, 97.5), 2, 3, 4 (196, 244.5) , 5 (293.5), 6, 7
    with MeshSimplifier(49.0) as ms:
        ms.add(xyz, none, stamp, robot)
        vm = ms.vertex_map()
        same_five(five(ms), ref)
    assert (vm[0::2] != vm[1::2]).all()  # 49 k and 49 k - 0.5 are apart


def test_voxel_faces_negative_zero_and_windows(gpu):
    xyz = np.array([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [-0.5, 0.0, 0.0],
                    [-1e-30, 0.0, 0.0], [0.999999, 0.0, 0.0], [2.0, -2.0, 2.0], [1.9999999, -2.0000002, 2.0],
                    [-3.0, -3.0, -3.0], [-3.0000002, -3.0, -3.0], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]], np.float32)
    n = xyz.shape[0]
    robot = np.zeros(n, np.int32)
    robot[-1] = 1  # the same voxel in another robot
    stamp = np.zeros(n, np.int64)
    faces = np.array([[0, 2, 3], [1, 2, 3], [3, 2, 0], [7, 9, 11], [11, 12, 0], [0, 1, 2]], np.int32)
    check_all(xyz, faces, stamp, robot, 1.0, None, 2)
    # windows: -1 ns and 0 are apart, 0 and 999_999_999 together, floor for negative stamps
    p = np.zeros((8, 3), np.float32)
    st = np.array([-1, 0, 999_999_999, 1_000_000_000, -1_000_000_000, -1_000_000_001, -2_000_000_000, 5], np.int64)
    ref, _, _ = check_all(p, np.zeros((0, 3), np.int32), st, np.zeros(8, np.int32), 1.0, 1.0, 1)
    assert list(ref[4]) == [0, 1, 1, 2, 0, 3, 3, 1]
    ref, _, _ = check_all(p, np.zeros((0, 3), np.int32), st, np.zeros(8, np.int32), 1.0, None, 1)
    assert list(ref[4]) == [0] * 8


def test_empty_single_and_faces_only_appends(gpu):
    none = np.zeros((0, 3), np.int32)
    ref = simplify_voxel(np.zeros((0, 3), np.float32), none, [], [], 1.0)
    with MeshSimplifier(1.0) as ms:
        assert ms.add(np.zeros((0, 3), np.float32), none, [], []) == (0, 0, 0)
        same_five(five(ms), ref)
        same(ms.edges(), np.zeros((0, 2), np.int32))
        G = ms.graph([np.array([3, 4], np.int64)], [(np.tile(np.eye(3), (2, 1, 1)), np.zeros((2, 3)))])
        same_graph(G, graph_from_mesh(ref[0], ref[1], ref[2], ref[3], [np.array([3, 4], np.int64)],
                                      [(np.tile(np.eye(3), (2, 1, 1)), np.zeros((2, 3)))]))
    check_all(np.array([[0.2, 0.3, 0.4]], np.float32), np.array([[0, 0, 0]], np.int32), [7], [0], 1.0, None, 1)
    # vertices first, then an append with faces only, then one whose faces name only earlier vertices
    rng = np.random.Generator(np.random.PCG64(5))
    xyz = rng.uniform(-3, 3, (40, 3)).astype(np.float32)
    stamp, robot = np.arange(40, dtype=np.int64), np.zeros(40, np.int32)
    f1, f2 = rng.integers(0, 30, (25, 3)).astype(np.int32), rng.integers(0, 30, (25, 3)).astype(np.int32)
    with MeshSimplifier(2.0) as ms:
        ms.add(xyz[:30], none, stamp[:30], robot[:30])
        assert ms.add(np.zeros((0, 3), np.float32), f1, [], [])[0] == 30
        same_five(five(ms), simplify_voxel(xyz[:30], f1, stamp[:30], robot[:30], 2.0))
        ms.add(xyz[30:], f2, stamp[30:], robot[30:])
        ref = simplify_voxel(xyz, np.concatenate([f1, f2]), stamp, robot, 2.0)
        same_five(five(ms), ref)
        same(ms.edges(), ref_edges(ref[3]), "edges")


# ---------------------------------------------------------------------- 5. hub
def test_hub_fan(gpu):
    n = 300
    ang = 2 * np.pi * np.arange(n) / n
    xyz = np.zeros((n + 1, 3), np.float32)
    xyz[1:, 0], xyz[1:, 1] = 50.0 * np.cos(ang), 50.0 * np.sin(ang)
    k = np.arange(n)
    faces = np.stack([np.zeros(n, np.int64), 1 + k, 1 + (k + 1) % n], 1).astype(np.int32)
    stamp, robot = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int32)
    ref, G, big = check_all(xyz, faces, stamp, robot, 1.0, None, 1)
    print(f"control {ref[0].shape[0]}, faces {ref[3].shape[0]}, hub bucket {big}")
    assert big == ref[0].shape[0] - 1 and big > 8 * HUB  # the hub's bucket holds every rim vertex


# ---------------------------------------------------------- 6. scan boundaries
@functools.lru_cache(maxsize=None)
def scan_spans():
    with MeshSimplifier(1.0) as ms:
        i = ms.info()
    return i["scan_span"], i["scan_span2"]


@pytest.mark.parametrize("which", ["span-1", "span", "span+1", "span2+1"])
def test_scan_boundaries(gpu, which):
    span, span2 = scan_spans()
    assert span == 1024 and span2 == 262_144  # simplify_host.h; a change there moves this test's sizes with it
    n = {"span-1": span - 1, "span": span, "span+1": span + 1, "span2+1": span2 + 1}[which]
    rng = np.random.Generator(np.random.PCG64(n))
    side = 3.0 if n < 5000 else 20.0  # about half the vertices are representatives
    xyz = rng.uniform(-side, side, (n, 3)).astype(np.float32)
    stamp, robot = np.zeros(n, np.int64), rng.integers(0, 2, n).astype(np.int32)
    a = rng.integers(0, n, n)
    faces = np.stack([a, (a + rng.integers(1, 9, n)) % n, (a + rng.integers(1, 9, n)) % n], 1).astype(np.int32)
    ref = simplify_voxel(xyz, faces, stamp, robot, 1.0)
    assert 0 < ref[0].shape[0] < n and 0 < ref[3].shape[0] < n
    with MeshSimplifier(1.0, None, 2) as ms:
        ms.add(xyz, faces, stamp, robot)
        same_five(five(ms), ref)
        same(ms.edges(), ref_edges(ref[3]), "edges")


# ------------------------------------------------------------- 7. rejections
def test_rejections_leave_the_handle_as_it_was(gpu):
    xyz, faces, stamp, robot = dense(4.0)
    xyz, stamp, robot = xyz[:3000], stamp[:3000], robot[:3000]
    faces = faces[(faces < 3000).all(1)][:4000]
    half = 1500
    fa, fb = faces[(faces < half).all(1)], faces[~(faces < half).all(1)]
    ks, rest = keyframes_of(stamp, robot, 2)

    def feed(ms, bad):
        ms.add(xyz[:half], fa, stamp[:half], robot[:half])
        if bad is not None:
            with pytest.raises(ValueError):
                bad(ms)
        ms.add(xyz[half:], fb, stamp[half:], robot[half:])
        return five(ms) + (ms.edges(),), ms.graph(ks, rest)

    with MeshSimplifier(1.0, 1.0, 2) as clean:
        want, want_G = feed(clean, None)
    p1 = np.array([[0.5, 0.5, 0.5]], np.float32)
    tri = np.array([[0, 1, 2]], np.int32)
    bad_calls = {
        "face index": lambda ms: ms.add(p1, np.array([[0, 1, half + 1]], np.int32), [0], [0]),
        "negative face index": lambda ms: ms.add(p1, np.array([[0, -1, 2]], np.int32), [0], [0]),
        "nan": lambda ms: ms.add(np.array([[0.5, np.nan, 0.5]], np.float32), tri, [0], [0]),
        "robot": lambda ms: ms.add(p1, tri, [0], [2]),
        "voxel beyond int32": lambda ms: ms.add(np.array([[3e9, 0, 0]], np.float32), tri, [0], [0]),
    }
    for name, bad in bad_calls.items():
        with MeshSimplifier(1.0, 1.0, 2) as ms:
            got, got_G = feed(ms, bad)
        for a, b in zip(got, want):
            same(a, b, name)
        same_graph(got_G, want_G)
    # the graph's rejections: the handle answers a correct call afterwards, and as before
    with MeshSimplifier(1.0, 1.0, 2) as ms:
        feed(ms, None)
        missing = [ks[0], ks[1][2:]]  # robot 1 loses its first stamp's keyframes
        rest_m = [rest[0], (rest[1][0][2:], rest[1][1][2:])]
        n_missing = int((want[2][want[1] == ks[1][0]] == 1).sum())
        assert n_missing > 0
        with pytest.raises(ValueError, match=rf"robot 1: {n_missing} control vertices have no keyframe"):
            ms.graph(missing, rest_m)
        with pytest.raises(ValueError, match="no keyframe"):  # the reference refuses the same input
            graph_from_mesh(want[0], want[1], want[2], want[3], missing, rest_m)
        dec = [ks[0][::-1].copy(), ks[1]]
        with pytest.raises(ValueError, match="robot 0"):
            ms.graph(dec, rest)
        with pytest.raises(ValueError):
            ms.graph(ks[:1], rest[:1])  # a wrong n_robots
        same_graph(ms.graph(ks, rest), want_G)
        for a, b in zip(five(ms) + (ms.edges(),), want):
            same(a, b, "after the graph rejections")


# -------------------------------------------------------------- 8. run to run
def test_run_to_run(gpu):
    xyz, faces, stamp, robot = dense(4.0)
    ks, rest = keyframes_of(stamp, robot, 2)
    runs = []
    for _ in range(2):
        with MeshSimplifier(1.0, 1.0, 2) as ms:
            ms.add(xyz, faces, stamp, robot)
            runs.append((five(ms) + (ms.edges(),), ms.graph(ks, rest)))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert a.tobytes() == b.tobytes()
    for k in runs[0][1]:
        assert np.asarray(runs[0][1][k]).tobytes() == np.asarray(runs[1][1][k]).tobytes(), k
    same_five(runs[0][0][:5], dense_ref(4.0, 1.0))


# ---------------------------------------------------------------- 9. pipeline
def test_pipeline_graph_simplify_gpu_equals_host(gpu):
    import inspect

    from kmx import pipeline as PL
    from kmx.synth import make_pose_graph
    from kmx.synth.mesh import make_mesh
    assert inspect.signature(PL.deform_mesh).parameters["graph_simplify"].default == "host"
    assert inspect.signature(PL.run_pipeline).parameters["mesh_graph_simplify"].default == "host"
    g0 = make_pose_graph(3, 3000, 12000, f_inter=0.0, outlier_scope="robot", seed=4)  # test_pipeline_gpu's team
    mesh = make_mesh(g0, 3, 3.0, 5)
    rest = PL.odometry_init(g0)
    cur = {a: (g0.gt_R[a], g0.gt_t[a]) for a in range(3)}
    out = {how: PL.deform_mesh(g0, mesh, rest, cur, return_xyz=True, graph_resolution=1.0, graph_simplify=how)
           for how in ("host", "gpu")}
    gh, gg = out["host"]["graph"], out["gpu"]["graph"]
    print(gg)
    assert set(gh) == set(gg) and gg["control_vertices"] > 0
    for k in gh:
        if k != "solve_ms":
            assert gh[k] == gg[k], k
    assert out["host"]["xyz"].tobytes() == out["gpu"]["xyz"].tobytes()
    with pytest.raises(ValueError):
        PL.deform_mesh(g0, mesh, rest, cur, graph_resolution=1.0, graph_simplify="device")
