"""Chordal initialisation on the device (kmx_chordal_*, chordal.hip) against
the host's direct solve, kmx.dpgo.init.chordal_initialization, on the same
edges: every entry of R within 1e-8 and t within 1e-7 m at rtol = 1e-10 (a CPU
restatement of the same PCG differs from the direct solve by 5.5e-11 / 1.5e-9 m
at these shapes; a structural mistake shows at 1e-3 or more). Against ground
truth on noise-free graphs: 1e-8 / 1e-6 m, the bounds of
test_agent_chordal_initialization."""
import functools

import numpy as np
import pytest

from kmx import abi
from kmx.dpgo.chordal import ChordalSolver
from kmx.dpgo.init import (chordal_initialization, chordal_initialization_gpu, chordal_initialization_team,
                           project_so3)
from kmx.synth import make_pose_graph
from kmx.synth.pose_graph import _expm_so3

pytestmark = pytest.mark.gpu

TOL_R, TOL_T = 1e-8, 1e-7
RTOL = 1e-10


def _robot_edges(g, a=0):
    own = np.nonzero((g.r1 == a) & (g.r2 == a))[0]
    return [(int(g.p1[e]), int(g.p2[e]), g.R[e], g.t[e], float(g.kappa[e]), float(g.tau[e]), float(g.weight[e]))
            for e in own]


def _relative(Rs, ts):  # gauge: the first pose at the origin
    return np.einsum("ij,njk->nik", Rs[0].T, Rs), (ts - ts[0]) @ Rs[0]


def _arrays(edges):
    return (np.array([e[0] for e in edges]), np.array([e[1] for e in edges]), np.array([e[2] for e in edges]),
            np.array([e[3] for e in edges]), np.array([e[4] for e in edges]), np.array([e[5] for e in edges]),
            np.array([e[6] for e in edges]))


def _close(R, t, Rr, tr, tol_R=TOL_R, tol_t=TOL_T):
    dR, dt = np.abs(R - Rr).max(), np.abs(t - tr).max()
    print(f"max |dR| = {dR:.3e}, max |dt| = {dt:.3e} m")
    assert dR < tol_R and dt < tol_t, (dR, dt)


def _chain(n, seed=11):
    rng = np.random.default_rng(seed)
    Rrel = _expm_so3(rng.normal(0, 0.2, (n - 1, 3)))
    trel = rng.normal(0, 1.0, (n - 1, 3))
    edges = [(k, k + 1, Rrel[k], trel[k], 100.0, 10.0, 1.0) for k in range(n - 1)]
    R, t = np.zeros((n, 3, 3)), np.zeros((n, 3))
    R[0] = np.eye(3)
    for k in range(n - 1):
        R[k + 1] = R[k] @ Rrel[k]
        t[k + 1] = t[k] + R[k] @ trel[k]
    return edges, R, t


@functools.lru_cache(maxsize=None)
def _graph5():
    g = make_pose_graph(1, 400, 1400, outlier_frac=0.0, sigma_R=0.02, seed=5)
    edges = _robot_edges(g)
    return g, edges, chordal_initialization(400, edges), _relative(g.init_R[0], g.init_t[0])


@functools.lru_cache(maxsize=None)
def _gpu5():
    """Graph 5 from a zero start: the result the determinism, weight and
    check_every tests compare with."""
    _, edges, _, _ = _graph5()
    return chordal_initialization_gpu(400, edges, rtol=RTOL, return_info=True)


def test_two_poses_one_edge(gpu):
    Rij = _expm_so3(np.array([[0.3, -0.2, 0.5]]))[0]
    tij = np.array([1.0, -2.0, 0.5])
    R, t, info = chordal_initialization_gpu(2, [(0, 1, Rij, tij, 50.0, 7.0, 1.0)], rtol=RTOL, return_info=True)
    assert np.abs(R[0] - np.eye(3)).max() == 0 and np.abs(t[0]).max() == 0
    assert np.abs(R[1] - Rij).max() < 1e-12 and np.abs(t[1] - tij).max() < 1e-12
    assert info[0]["converged"]


def test_reflection_case_and_parallel_edges(gpu):
    """Three parallel edges whose unconstrained block is diag(-1,-3,-5)/9:
    negative determinant, distinct singular values; the determinant fix must
    land on the smallest singular direction, as project_so3's does."""
    Rs = [np.diag(d) for d in ([1.0, -1, -1], [-1.0, 1, -1], [-1.0, -1, 1])]
    edges = [(0, 1, Rs[k], np.array([0.5, 1.0, -1.0]), kap, 1.0, 1.0) for k, kap in enumerate((4.0, 3.0, 2.0))]
    R, t = chordal_initialization_gpu(2, edges, rtol=RTOL)
    assert np.allclose(project_so3(np.diag([-1.0, -3, -5]) / 9), np.diag([1.0, -1, -1]))
    assert np.abs(R[1] - np.diag([1.0, -1, -1])).max() < 1e-12
    Rr, tr = chordal_initialization(2, edges)
    _close(R, t, Rr, tr)


def test_pure_chain_of_65(gpu):
    edges, Rc, tc = _chain(65)
    R, t, info = chordal_initialization_gpu(65, edges, R_init=Rc, t_init=tc, rtol=RTOL, return_info=True)
    assert info[0]["iterations_rot"] == 0 and info[0]["iterations_trans"] == 0 and info[0]["converged"]
    assert np.abs(R - Rc).max() < 1e-12 and np.abs(t - tc).max() < 1e-12
    Rr, tr = chordal_initialization(65, edges)
    R0, t0, info0 = chordal_initialization_gpu(65, edges, rtol=RTOL, return_info=True)
    assert info0[0]["converged"] and info0[0]["iterations_rot"] > 0
    _close(R0, t0, Rr, tr)


def test_noise_free_graph_is_ground_truth(gpu):
    g = make_pose_graph(1, 300, 900, outlier_frac=0.0, noise_free=True, seed=2)
    R, t = chordal_initialization_gpu(300, _robot_edges(g), rtol=RTOL)
    Rg, tg = _relative(g.gt_R[0], g.gt_t[0])
    _close(R, t, Rg, tg, 1e-8, 1e-6)
    assert np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)).max() < 1e-12
    assert np.abs(np.linalg.det(R) - 1.0).max() < 1e-12


def test_noisy_graph_equals_the_host_solve(gpu):
    g, edges, (Rr, tr), (Ro, to) = _graph5()
    R, t, info = _gpu5()
    _close(R, t, Rr, tr)
    R2, t2, info2 = chordal_initialization_gpu(400, edges, R_init=Ro, t_init=to, rtol=RTOL, return_info=True)
    _close(R2, t2, Rr, tr)
    for i in (info[0], info2[0]):
        print(i)
        assert i["converged"]
        assert 0 < i["iterations_rot"] < 20000 and 0 < i["iterations_trans"] < 20000
        assert max(i["relres_rot"] + i["relres_trans"]) <= RTOL * (1 + 1e-12)  # sqrt of the tested ratio


def test_hub_of_degree_282(gpu):
    """280 loop closures that all touch pose 7 of a 300-pose noisy chain: one
    pose with more incident edges than any wave or tile is wide."""
    g = make_pose_graph(1, 300, 300, outlier_frac=0.0, sigma_R=0.02, seed=6)
    edges = [e for e, f in zip(_robot_edges(g), g.fixed[(g.r1 == 0) & (g.r2 == 0)]) if f]
    assert len(edges) == 299
    rng = np.random.default_rng(8)
    Rg, tg = g.gt_R[0], g.gt_t[0]
    for k, q in enumerate(range(20, 300)):
        i, j = (7, q) if k % 2 else (q, 7)
        Rij = Rg[i].T @ Rg[j] @ _expm_so3(rng.normal(0, 0.02, (1, 3)))[0]
        tij = Rg[i].T @ (tg[j] - tg[i]) + rng.normal(0, 0.1, 3)
        edges.append((i, j, Rij, tij, edges[0][4], edges[0][5], 1.0))
    assert sum(1 for e in edges if 7 in (e[0], e[1])) == 282
    Rr, tr = chordal_initialization(300, edges)
    R, t, info = chordal_initialization_gpu(300, edges, rtol=RTOL, return_info=True)
    assert info[0]["converged"]
    _close(R, t, Rr, tr)


def test_anchor_that_is_not_pose_0(gpu):
    _, edges, _, _ = _graph5()
    Rr, tr = chordal_initialization(400, edges, anchor=123)
    R, t = chordal_initialization_gpu(400, edges, anchor=123, rtol=RTOL)
    assert np.array_equal(R[123], np.eye(3)) and np.array_equal(t[123], np.zeros(3))
    _close(R, t, Rr, tr)


def test_team_batch(gpu):
    g = make_pose_graph(3, 600, 2100, outlier_frac=0.0, f_inter=0.1, seed=3)
    Rl, tl, info = chordal_initialization_team(g, rtol=RTOL, return_info=True)
    assert len(Rl) == len(tl) == len(info) == 3
    for a in range(3):
        n = int(g.n_poses[a])
        edges = _robot_edges(g, a)
        Rr, tr = chordal_initialization(n, edges)
        _close(Rl[a], tl[a], Rr, tr)
        assert info[a]["converged"] and info[a]["iterations_rot"] > 0
        Ro, to = _relative(g.init_R[a], g.init_t[a])
        Rs, ts, si = chordal_initialization_gpu(n, edges, R_init=Ro, t_init=to, rtol=RTOL, return_info=True)
        _close(Rl[a], tl[a], Rs, ts, 1e-10, 1e-10)
        # tiles never span two blocks and a block's partials are summed in an
        # order of its own: the batch changes no bit of a robot's solve
        assert np.array_equal(Rl[a], Rs) and np.array_equal(tl[a], ts)
        assert si[0] == info[a]


def test_set_weights(gpu):
    g, edges, _, _ = _graph5()
    src, dst, R, t, kap, tau, w = _arrays(edges)
    lc = np.nonzero(g.fixed[(g.r1 == 0) & (g.r2 == 0)] == 0)[0]
    drop = lc[::3]
    w2 = w.copy()
    w2[drop] = 0.0
    keep = w2 > 0
    s = ChordalSolver()
    f = ChordalSolver()
    try:
        s.set_graph(400, [0, 400], src, dst, R, t, kap, tau, w)
        Ra, ta, _ = s.solve(rtol=RTOL)
        assert np.array_equal(Ra, _gpu5()[0]) and np.array_equal(ta, _gpu5()[1])
        s.set_weights(w2)
        Rb, tb, ib = s.solve(rtol=RTOL)
        f.set_graph(400, [0, 400], src[keep], dst[keep], R[keep], t[keep], kap[keep], tau[keep], w[keep])
        Rf, tf, i_f = f.solve(rtol=RTOL)
        assert np.array_equal(Rb, Rf) and np.array_equal(tb, tf) and ib == i_f
        assert not np.array_equal(Ra, Rb)
        # cut pose 399 off: refused, the previous weights stay in force
        w3 = w2.copy()
        w3[(src == 399) | (dst == 399)] = 0.0
        with pytest.raises(abi.KmxError, match=r"\(-1\)"):
            s.set_weights(w3)
        Rc, tc, _ = s.solve(rtol=RTOL)
        assert np.array_equal(Rc, Rb) and np.array_equal(tc, tb)
    finally:
        s.close()
        f.close()


def test_determinism_and_check_every(gpu):
    _, edges, _, _ = _graph5()
    R0, t0, i0 = _gpu5()
    R1, t1, i1 = chordal_initialization_gpu(400, edges, rtol=RTOL, return_info=True)
    assert np.array_equal(R0, R1) and np.array_equal(t0, t1) and i0 == i1
    for ce in (1, 7, 1000):
        R, t, info = chordal_initialization_gpu(400, edges, rtol=RTOL, check_every=ce, return_info=True)
        assert np.array_equal(R, R0) and np.array_equal(t, t0), ce
        assert info == i0, ce


def test_iteration_cap(gpu):
    _, edges, _, _ = _graph5()
    R, t, info = chordal_initialization_gpu(400, edges, rtol=RTOL, max_iterations=5, return_info=True)
    assert not info[0]["converged"] and info[0]["iterations_rot"] == 5
    assert np.isfinite(R).all() and np.isfinite(t).all()
    assert np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)).max() < 1e-12
    assert np.abs(np.linalg.det(R) - 1.0).max() < 1e-12


def test_refusals_leave_the_handle_usable(gpu):
    Rij = _expm_so3(np.array([[0.1, 0.2, -0.3]]))[0]
    tij = np.array([1.0, 2.0, 3.0])
    I3 = np.eye(3)[None]
    good = dict(n_poses=2, block_ptr=[0, 2], src=[0], dst=[1], R=Rij[None], t=tij[None], kappa=[5.0], tau=[2.0])

    def usable(s):
        s.set_graph(**good)
        R, t, _ = s.solve(rtol=RTOL)
        assert np.abs(R[1] - Rij).max() < 1e-12 and np.abs(t[1] - tij).max() < 1e-12

    four = dict(n_poses=4, block_ptr=[0, 2, 4], src=[0, 2], dst=[1, 3], R=np.tile(I3, (2, 1, 1)),
                t=np.ones((2, 3)), kappa=[1.0, 1.0], tau=[1.0, 1.0], anchors=[0, 2])
    bad = {
        "an edge across blocks": dict(four, src=[0, 1], dst=[1, 2]),
        "an index out of range": dict(four, dst=[1, 4]),
        "kappa = 0": dict(four, kappa=[1.0, 0.0]),
        "a NaN in t": dict(four, t=np.array([[1.0, 1, 1], [1, np.nan, 1]])),
        "a block without an anchor": dict(four, anchors=[0]),
    }
    s = ChordalSolver()
    try:
        with pytest.raises(abi.KmxError, match=r"\(-3\)"):  # KMX_ESTATE
            s.solve()
        usable(s)
        for what, args in bad.items():
            with pytest.raises(abi.KmxError, match=r"\(-1\)"):  # KMX_EINVAL
                s.set_graph(**args)
            # the previous graph is still in place
            R, t, _ = s.solve(rtol=RTOL)
            assert R.shape == (2, 3, 3) and np.abs(R[1] - Rij).max() < 1e-12, what
            usable(s)
    finally:
        s.close()


def test_agent_chordal_gpu(gpu):
    from kmx.dpgo.agent import PGOAgent
    from kmx.dpgo.messages import RelativeSEMeasurement
    from kmx.dpgo.params import PGOAgentParameters
    g = make_pose_graph(1, 200, 700, outlier_frac=0.0, noise_free=True, seed=4)
    P = PGOAgentParameters(r=5, num_robots=1, localInitializationMethod="chordal_gpu")
    ag = PGOAgent(0, P)  # the real BlockSolver
    for e in range(g.m):
        ag.addMeasurement(RelativeSEMeasurement(0, 0, int(g.p1[e]), int(g.p2[e]), 3, g.R[e], g.t[e],
                                                float(g.kappa[e]), float(g.tau[e]),
                                                fixedWeight=bool(g.fixed[e])))
    ag.initialize()
    T = ag.getTrajectoryInLocalFrame().reshape(3, -1, 4).transpose(1, 0, 2)
    Rg, tg = _relative(g.gt_R[0], g.gt_t[0])
    _close(T[:, :, :3], T[:, :, 3], Rg, tg, 1e-8, 1e-6)
    if hasattr(ag.solver, "close"):
        ag.solver.close()


def test_pipeline_local_init(gpu):
    """run_pipeline(local_init="chordal_gpu") starts every robot from the
    device's chordal relaxation. On an outlier-free team with 0.02 rad of
    odometry noise per keyframe the 300-pose odometry chains drift by metres
    while the relaxation closes every loop, so the team's ATE after the global
    alignment must be lower; the default stays the odometry chain."""
    from kmx import pipeline as PL
    from kmx.dpgo.params import PGOAgentParameters
    from kmx.lcd import LcdParams
    g0 = make_pose_graph(3, 900, 3600, f_inter=0.0, outlier_frac=0.0, sigma_R=0.02, seed=4)
    st = PL.make_lc_stream(g0, 40, 10, n_feats=200, seed=2)
    P = PGOAgentParameters(r=5)
    od = PL.run_pipeline(g0, st, P, LcdParams(), rounds=2, device=0)
    ch = PL.run_pipeline(g0, st, P, LcdParams(), rounds=2, device=0, local_init="chordal_gpu")
    print(od["init"], ch["init"])
    assert od["init"]["local_init"] == "odometry" and ch["init"]["local_init"] == "chordal_gpu"
    assert od["lcd"]["accepted"] == ch["lcd"]["accepted"] > 0
    assert ch["init"]["ate_m"] < od["init"]["ate_m"]
    with pytest.raises(ValueError, match="unknown local_init"):
        PL.run_pipeline(g0, st, P, LcdParams(), rounds=1, device=0, local_init="chordal")
