"""Deformation graph optimisation on the device (kmx_dgraph_*, csrc/dgraph.hip)
against the contract in numpy (tests/dgraph_ref.py): the operators entry by
entry within the bound their summation gives, the Levenberg-Marquardt solve
(flags, counts, stop reason, costs, poses), determinism and independence of
check_every, set_weights, errors, and the pipeline's graph stage."""
import numpy as np
import pytest

from tests import dgraph_ref as DR
from tests import mesh_ref as MR
from tests.test_dgraph_cpu import random_point, rigid_case

pytestmark = pytest.mark.gpu

# The largest pose difference (R entries, t entries) between the device and the
# reference at the tight settings (cg_rtol 1e-12, rel_tol 0) on the bend cases,
# as measured on an MI355X; the tests allow ten times it.
MEASURED_BEND_SOFT = 6.6e-8
MEASURED_BEND_HARD = 2.2e-8


def device_graph(P, priors=True):
    from kmx.pgmo import DeformationGraph
    dg = DeformationGraph()
    dg.set_graph(P.R_rest, P.g, P.src, P.dst, P.w)
    if priors:
        dg.set_priors(P.mode, P.R_hat, P.t_hat, P.kappa, P.tau)
    return dg


def run(P, start=None, **params):
    dg = device_graph(P)
    if start is not None:
        dg.set_poses(*start)
    res = dg.solve(**params)
    R, t = dg.poses()
    log = dg.log()
    dg.close()
    return R, t, log, res


def same_log(a, b):
    return len(a) == len(b) and all(x == y for x, y in zip(a, b))


# -------------------------------------------------------------- 1. operators
def ring_problem(n, seed):
    """A ring in both directions with n / 2 random chords, random weights, a
    hard node, soft nodes (some with kappa or tau 0) and free ones."""
    rng = np.random.Generator(np.random.PCG64(seed))
    i = np.arange(n)
    a = np.concatenate([i, (i + 1) % n, rng.integers(0, n, n // 2)])
    b = np.concatenate([(i + 1) % n, i, rng.integers(0, n, n // 2)])
    keep = a != b
    a, b = a[keep], b[keep]
    R_rest = DR.exp_so3(rng.standard_normal((n, 3)))
    g = rng.uniform(-5, 5, (n, 3))
    mode = rng.choice(np.array([0, 0, 1, 1, 2], np.uint8), n)
    mode[0], mode[n - 1] = 2, 1
    R_hat, t_hat = random_point(None, rng, R_rest=R_rest, g=g)
    kappa, tau = rng.uniform(0, 2, n) * (rng.random(n) < 0.8), rng.uniform(0.1, 2, n)
    return DR.make_problem(R_rest, g, a, b, rng.uniform(0.2, 3, a.shape[0]), mode, R_hat, t_hat, kappa, tau)


def two_node_problem():
    rng = np.random.Generator(np.random.PCG64(2))
    R_rest = DR.exp_so3(rng.standard_normal((2, 3)))
    g = rng.uniform(-5, 5, (2, 3))
    R_hat, t_hat = random_point(None, rng, R_rest=R_rest, g=g)
    return DR.make_problem(R_rest, g, [0, 1], [1, 0], [1.5, 0.5], np.array([0, 2], np.uint8), R_hat, t_hat, 0.0, 0.0)


def big_grid_problem():
    """70 x 70: 4 900 nodes in 77 tiles, so the one-wave sum over the tile partials takes a second pass."""
    R_rest, g, src, dst, _ = DR.grid_problem(70, 70, 0, seed=4)
    rng = np.random.Generator(np.random.PCG64(4))
    n = g.shape[0]
    mode = (rng.random(n) < 0.05).astype(np.uint8)
    mode[0] = 2
    R_hat, t_hat = random_point(None, rng, R_rest=R_rest, g=g)
    return DR.make_problem(R_rest, g, src, dst, rng.uniform(0.5, 2, src.shape[0]), mode, R_hat, t_hat, 1.0, 2.0)


def degree_problem():
    """Out-degrees 300 (node 0, a hub), 65 (node 1), 2 (node 2), 1 (node 3) and 0 (every other node)."""
    rng = np.random.Generator(np.random.PCG64(5))
    n = 301
    src = np.concatenate([np.zeros(300, np.int64), np.ones(65, np.int64), [2, 2], [3]])
    dst = np.concatenate([np.arange(1, 301), np.arange(2, 67), [3, 4], [4]])
    R_rest = DR.exp_so3(rng.standard_normal((n, 3)))
    g = rng.uniform(-5, 5, (n, 3))
    mode = np.zeros(n, np.uint8)
    mode[0], mode[300] = 1, 2
    R_hat, t_hat = random_point(None, rng, R_rest=R_rest, g=g)
    P = DR.make_problem(R_rest, g, src, dst, rng.uniform(0.2, 3, src.shape[0]), mode, R_hat, t_hat, 0.7, 1.3)
    deg = np.bincount(P.src, minlength=n)
    assert {0, 1, 2, 65, 300} == set(deg.tolist())
    return P


def zero_weight_problem():
    P = ring_problem(100, 6)
    rng = np.random.Generator(np.random.PCG64(66))
    P.w[rng.random(P.m) < 0.3] = 0.0
    P.w[:200] = np.where(np.arange(200) % 7 == 0, 0.0, P.w[:200])
    P.mode[P.mode == 0] = 1  # every node holds itself: any set of zero weights is well posed
    P.kappa = np.where(P.mode == 1, 0.5, 0.0)
    P.tau = np.where(P.mode == 1, 0.5, 0.0)
    assert (P.w == 0).sum() > 20
    return P


OPERATOR_CASES = {
    "n2_one_free_one_hard": two_node_problem,
    "n63": lambda: ring_problem(63, 63), "n64": lambda: ring_problem(64, 64), "n65": lambda: ring_problem(65, 65),
    "n129_all_three_modes": lambda: ring_problem(129, 129),
    "grid70_two_reduce_passes": big_grid_problem,
    "degrees_0_1_2_65_300": degree_problem,
    "zero_weights": zero_weight_problem,
}


@pytest.mark.parametrize("case", list(OPERATOR_CASES))
def test_operators_against_reference(gpu, case):
    """Every entry within 4 (number of terms) eps A, A the same sum over
    absolute values (tests/dgraph_ref.py operators): the bound of the
    summation, whatever the order."""
    P = OPERATOR_CASES[case]()
    assert DR.well_posed(P)
    if case == "n129_all_three_modes":
        assert set(P.mode.tolist()) == {0, 1, 2}
    rng = np.random.Generator(np.random.PCG64(99))
    R, t = random_point(P, rng)
    v = rng.standard_normal((P.n, 6))
    ref = DR.operators(P, R, t, v)
    dg = device_graph(P)
    dg.set_poses(R, t)
    got = {"cost": dg.eval("cost"), "grad": dg.eval("grad"), "blocks": dg.eval("blocks"), "jtj": dg.eval("jtj", v)}
    dg.close()
    worst = {}
    for name in ("cost", "grad", "blocks", "jtj"):
        val, ab, nt = ref[name]
        err = np.abs(np.asarray(got[name]) - val)
        bound = 4.0 * np.asarray(nt) * DR.EPS * np.asarray(ab)
        worst[name] = float(np.max(err / np.maximum(bound, 1e-300)))
        assert (err <= bound).all(), (name, worst[name])
        assert np.abs(np.asarray(val)).max() > 0
    print(case, {k: f"{x:.3f} of the bound" for k, x in worst.items()})
    hard = P.mode == 2
    assert not got["grad"][hard].any() and not got["blocks"][hard].any() and not got["jtj"][hard].any()


# ------------------------------------------------------------------ 2. solve
def bend_case(hard, seed=1):
    """The 8 x 8 grid with 6 keyframes, each keyframe's prior at its rest pose
    moved by a rotation and an offset of its own."""
    R_rest, g, src, dst, kf = DR.grid_problem(8, 8, 6, seed=0)
    rng = np.random.Generator(np.random.PCG64(seed))
    n = g.shape[0]
    mode = np.zeros(n, np.uint8)
    mode[kf] = 2 if hard else 1
    R_hat, t_hat = R_rest.copy(), g.copy()
    R_hat[kf] = DR.exp_so3(0.3 * rng.standard_normal((6, 3))) @ R_rest[kf]
    t_hat[kf] = g[kf] + 0.5 * rng.standard_normal((6, 3))
    return DR.make_problem(R_rest, g, src, dst, None, mode, R_hat, t_hat, 1.0, 1.0)


def cost_floor(P, f):
    """How far two evaluations of a cost f = |r|^2 can differ through fp64
    alone. Every residual entry is a sum of coordinates of size S (poses and
    edge vectors), each held and added to 4 eps S at most, so the residual
    carries an error e with |e| <= E = sqrt(entries * largest weight) * 4 eps
    S, and |r + e|^2 - |r|^2 <= 2 sqrt(f) E + E^2. Next to a cost of order 1
    this is 1e-13 relative and plays no part; it is what is left of "relative"
    when the cost itself goes to 0, as in the rigid case."""
    S = max(np.abs(P.t_hat).max(), np.abs(P.g).max()) + np.abs(P.d).max()
    n_res = 3 * P.m + 12 * int((P.mode == 1).sum())
    E = np.sqrt(n_res * max(P.w.max(), P.kappa.max(), P.tau.max(), 1.0)) * 4 * DR.EPS * S
    return 2.0 * np.sqrt(f) * E + E * E


def assert_same_decisions(ref, log, res):
    assert [e["accepted"] for e in log] == [e["accepted"] for e in ref["log"]]
    assert res["iterations"] == ref["iterations"] and res["accepted"] == ref["accepted"]
    assert res["stop_reason"] == ref["stop_reason"]
    for e, r in zip(log, ref["log"]):
        assert e["lam"] == r["lam"]
        assert abs(e["cg_iterations"] - r["cg_iterations"]) <= 1
    print(f"  {res['iterations']} outer iterations ({res['accepted']} accepted), stop {res['stop_reason']}, "
          f"cg {res['cg_iterations']} vs {ref['cg_iterations']}")


def assert_same_costs(P, ref, log):
    """1e-9 relative, per iteration, on the cost and the trial cost, above the
    fp64 floor of a cost's evaluation (cost_floor)."""
    rows = []
    for k, (e, r) in enumerate(zip(log, ref["log"])):
        for name in ("cost", "trial_cost"):
            rows.append((k, name, e[name], r[name], abs(e[name] - r[name]) / max(abs(r[name]), 1e-300)))
    for k, name, a, b, rel in rows:
        print(f"    iteration {k} {name}: device {a:.12e} reference {b:.12e} relative {rel:.2e} "
              f"(floor {cost_floor(P, abs(b)) / max(abs(b), 1e-300):.1e})")
    for k, name, a, b, rel in rows:
        assert abs(a - b) <= 1e-9 * abs(b) + cost_floor(P, abs(b)), (k, name, a, b, rel)


def test_solve_rigid_motion(gpu):
    """Soft priors moved by one rigid motion. abs_tol = 1e-24 ends both runs
    on the accepted step that reaches a cost of 0 to within it, above the
    rounding floor of the cost (about 1e-27 here), where accepting a step
    would depend on the last bits. The minimum has cost 0, so the late costs
    (1.2e-11 after 2.5e-4, then 1e-23) are squares of what the step left
    over and agree to 1e-8 and 1e-4 of themselves, inside cost_floor; the
    reference differs from itself as much when its edges are listed in another
    order."""
    P, kf, Rm, tm = rigid_case()
    ref = DR.solve(P, abs_tol=1e-24)
    R, t, log, res = run(P, abs_tol=1e-24)
    assert_same_decisions(ref, log, res)
    assert_same_costs(P, ref, log)
    assert res["stop_reason"] == 2
    eR, et = np.abs(R - Rm @ P.R_rest).max(), np.abs(t - (P.g @ Rm.T + tm)).max()
    print(f"  rigid: errors {eR:.2e} {et:.2e}, cost {res['cost_final']:.2e}")
    assert eR < 1e-10 and et < 1e-10


@pytest.mark.parametrize("hard", [False, True])
def test_solve_bend(gpu, hard):
    P = bend_case(hard)
    ref = DR.solve(P)
    R, t, log, res = run(P)
    assert_same_decisions(ref, log, res)
    assert_same_costs(P, ref, log)
    assert res["stop_reason"] == 1 and res["cost_final"] < res["cost_initial"]
    if hard:
        kf = P.mode == 2
        assert np.array_equal(R[kf], P.R_hat[kf]) and np.array_equal(t[kf], P.t_hat[kf])
    # the minimiser at the tight settings, both to the end of their own roundings
    tight = dict(cg_rtol=1e-12, rel_tol=0.0)
    rt = DR.solve(P, **tight)
    R, t, log, res = run(P, **tight)
    diff = max(np.abs(R - rt["R"]).max(), np.abs(t - rt["t"]).max())
    measured = MEASURED_BEND_HARD if hard else MEASURED_BEND_SOFT
    print(f"  bend {'hard' if hard else 'soft'}: tight pose difference {diff:.3e} (measured {measured:.3e}); "
          f"device {res['iterations']} iterations stop {res['stop_reason']}, reference {rt['iterations']} "
          f"stop {rt['stop_reason']}; costs {res['cost_final']:.15e} {rt['cost_final']:.15e}")
    assert diff <= 10 * measured


# ------------------------------------------------------------ 3. determinism
def test_deterministic_and_independent_of_check_every(gpu):
    P = bend_case(False)
    R0, t0, log0, res0 = run(P)
    R1, t1, log1, res1 = run(P)
    assert np.array_equal(R0, R1) and np.array_equal(t0, t1) and same_log(log0, log1) and res0 == res1
    assert max(e["cg_iterations"] for e in log0) > 7  # so that check_every = 1 and 7 read the stop word mid-solve
    for ce in (1, 7, 1000):
        R, t, log, res = run(P, check_every=ce)
        assert np.array_equal(R0, R) and np.array_equal(t0, t), ce
        assert same_log(log0, log), ce
        assert res["cg_iterations"] == res0["cg_iterations"] and res["iterations"] == res0["iterations"], ce


# ---------------------------------------------------------------- 4. weights
def test_set_weights_equals_a_graph_without_the_edges(gpu):
    P = bend_case(False)
    rng = np.random.Generator(np.random.PCG64(8))
    w = np.where(rng.random(P.m) < 0.25, 0.0, rng.uniform(0.5, 2, P.m))
    P.w = w
    assert DR.well_posed(P) and (w == 0).sum() > 20
    dg = device_graph(bend_case(False))
    dg.set_weights(w)
    res = dg.solve()
    R, t = dg.poses()
    log = dg.log()
    dg.close()
    keep = w > 0
    Q = DR.make_problem(P.R_rest, P.g, P.src[keep], P.dst[keep], w[keep], P.mode, P.R_hat, P.t_hat, P.kappa, P.tau)
    R2, t2, log2, res2 = run(Q)
    assert np.array_equal(R, R2) and np.array_equal(t, t2) and same_log(log, log2) and res == res2
    assert res["accepted"] >= 2


# ----------------------------------------------------------------- 5. errors
def test_errors_leave_the_handle_as_it_was(gpu):
    from kmx import abi
    from kmx.pgmo import DeformationGraph
    P = bend_case(False)
    R0, t0, log0, res0 = run(P)
    dg = DeformationGraph()
    with pytest.raises(abi.KmxError, match=r"kmx_dgraph_set_priors failed \(-3\)"):  # before set_graph
        dg.set_priors(np.zeros(0, np.uint8))
    with pytest.raises(abi.KmxError, match=r"kmx_dgraph_solve failed \(-3\)"):
        dg.solve()
    dg.set_graph(P.R_rest, P.g, P.src, P.dst, P.w)
    with pytest.raises(abi.KmxError, match=r"kmx_dgraph_solve failed \(-3\)"):  # no priors yet
        dg.solve()
    dg.set_priors(P.mode, P.R_hat, P.t_hat, P.kappa, P.tau)
    with pytest.raises(abi.KmxError, match=r"set_priors failed \(-1\).*component"):  # a component without a prior
        dg.set_priors(np.zeros(P.n, np.uint8))
    tau0 = np.where(P.mode == 1, 0.0, P.tau)
    with pytest.raises(abi.KmxError, match="component"):  # kappa alone holds nothing
        dg.set_priors(P.mode, P.R_hat, P.t_hat, P.kappa, tau0)
    bad = P.t_hat.copy()
    bad[np.nonzero(P.mode == 1)[0][0], 1] = np.nan
    with pytest.raises(abi.KmxError, match="not finite"):
        dg.set_priors(P.mode, P.R_hat, bad, P.kappa, P.tau)
    with pytest.raises(abi.KmxError, match="finite and >= 0"):
        dg.set_priors(P.mode, P.R_hat, P.t_hat, -P.kappa, P.tau)
    with pytest.raises(abi.KmxError, match="endpoint"):
        dg.set_graph(P.R_rest, P.g, P.src, np.where(np.arange(P.m) == 3, P.n, P.dst), P.w)
    wbad = P.w.copy()
    wbad[2] = -1.0
    with pytest.raises(abi.KmxError, match="weight"):
        dg.set_weights(wbad)
    with pytest.raises(abi.KmxError, match="component"):  # every edge off: the free vertices float
        dg.set_weights(np.zeros(P.m))
    with pytest.raises(abi.KmxError, match="not finite"):
        dg.set_poses(np.full((P.n, 3, 3), np.inf), P.g)
    with pytest.raises(abi.KmxError, match=r"kmx_dgraph_solve failed \(-1\)"):
        dg.solve(lambda_factor=0.5)
    res = dg.solve()
    R, t = dg.poses()
    assert np.array_equal(R, R0) and np.array_equal(t, t0) and same_log(dg.log(), log0) and res == res0
    tm = dg.timing()
    assert tm["total_ms"] > 0 and tm["cg_ms"] > 0 and tm["linearize_ms"] > 0 and tm["trial_ms"] > 0
    assert tm["linearize_ms"] + tm["cg_ms"] + tm["trial_ms"] <= tm["total_ms"] * 1.001
    # set_poses(None): back to rest; the same solve again
    dg.set_poses()
    assert np.array_equal(dg.poses()[0], P.R_rest)
    assert dg.solve() == res0
    # n = 0 and m = 0 are legal
    dg.set_graph(np.zeros((0, 3, 3)), np.zeros((0, 3)), [], [])
    dg.set_priors(np.zeros(0, np.uint8))
    assert dg.solve()["stop_reason"] == 5 and dg.eval("cost") == 0.0
    dg.set_graph(np.eye(3)[None], np.ones((1, 3)), [], [])
    dg.set_priors(np.array([1], np.uint8), np.eye(3)[None], np.array([[1.0, 2.0, 4.0]]), 1.0, 1.0)
    res = dg.solve()
    assert res["stop_reason"] in (1, 2) and np.abs(dg.poses()[1] - [1.0, 2.0, 4.0]).max() < 1e-9
    dg.close()


# --------------------------------------------------------------- 6. pipeline
def test_pipeline_graph_stage(gpu):
    import inspect

    from kmx import pipeline as PL
    from kmx.lcd import LcdParams
    from kmx.synth.mesh import make_mesh
    from tests.test_pipeline_gpu import _setup
    assert inspect.signature(PL.run_pipeline).parameters["mesh_graph"].default is None
    assert inspect.signature(PL.deform_mesh).parameters["graph_resolution"].default is None
    g0, st, P = _setup()
    mesh = make_mesh(g0, 3, 3.0, 5)
    out = PL.run_pipeline(g0, st, P, LcdParams(), rounds=10, device=0, mesh=mesh, mesh_graph=1.0,
                          return_trajectory=True)
    m = out["mesh"]
    print({k: v for k, v in m.items() if k != "xyz"})
    gr = m["graph"]
    n_kf = int(np.sum(g0.n_poses))
    assert gr["nodes"] == n_kf + gr["control_vertices"] and 0 < gr["control_vertices"] <= mesh.xyz.shape[0]
    assert gr["edges"] > 2 * gr["control_vertices"] and gr["iterations"] >= 1 and gr["solve_ms"] > 0
    assert gr["cost_after"] < gr["cost_before"]
    assert m["vertices"] == mesh.xyz.shape[0] and m["unbound"] == 0
    assert np.isfinite(m["rmse_after_m"]) and m["rmse_after_m"] < m["rmse_before_m"]
    # off: the entry is today's, vertex for vertex what the keyframe-only contract gives
    traj = out["trajectory"]
    rest = PL.odometry_init(g0)
    m0 = PL.deform_mesh(g0, mesh, rest, traj, return_xyz=True)
    assert set(m0) == {"vertices", "unbound", "bind_seconds", "deform_seconds", "rmse_before_m", "rmse_after_m", "xyz"}
    cat = np.concatenate
    node_robot = cat([np.full(int(g0.n_poses[a]), a, np.int32) for a in range(3)])
    R_cur, p = cat([traj[a][0] for a in range(3)]), cat([traj[a][1] for a in range(3)])
    ref, _, _ = MR.deform_all(node_robot, cat(mesh.kf_stamp), cat(mesh.rest_R), cat(mesh.rest_t), R_cur, p,
                              mesh.robot, mesh.stamp, mesh.xyz, 4, 1_000_000_000)
    scale = max(np.abs(cat(mesh.rest_t)).max(), np.abs(p).max(), np.abs(mesh.xyz).max())
    assert (np.abs(m0["xyz"].astype(np.float64) - ref.astype(np.float64)) <= MR.tolerance(ref, scale)).all()
    assert m0["rmse_before_m"] == m["rmse_before_m"]


def test_graph_path_per_robot_rigid_correction(gpu):
    """Every robot's trajectory moved by a rigid motion of its own: the graph's
    minimiser moves that robot's nodes by the same motion, and so every vertex."""
    from kmx import pipeline as PL
    from kmx.synth import make_pose_graph
    from kmx.synth.mesh import make_mesh
    g = make_pose_graph(3, 240, 240, seed=7)
    mesh = make_mesh(g, 4, 3.0, 2)
    rest = PL.odometry_init(g)
    rng = np.random.Generator(np.random.PCG64(3))
    cur, want = {}, np.empty((mesh.xyz.shape[0], 3))
    for a in range(3):
        Rm, tm = DR.exp_so3(0.3 * rng.standard_normal(3)), rng.uniform(-3, 3, 3)
        cur[a] = (Rm @ rest[a][0], rest[a][1] @ Rm.T + tm)
        sel = mesh.robot == a
        want[sel] = mesh.xyz[sel].astype(np.float64) @ Rm.T + tm
    m = PL.deform_mesh(g, mesh, rest, cur, return_xyz=True, graph_resolution=1.0)
    print({k: v for k, v in m.items() if k != "xyz"})
    assert m["unbound"] == 0 and m["graph"]["control_vertices"] < mesh.xyz.shape[0]
    scale = max(np.abs(want).max(), np.abs(mesh.xyz).max())
    err = np.abs(m["xyz"].astype(np.float64) - want)
    tol = MR.tolerance(want, scale)
    print(f"  worst error / tolerance {np.max(err / tol):.3f}, cost {m['graph']['cost_after']:.2e}")
    assert (err <= tol).all()
