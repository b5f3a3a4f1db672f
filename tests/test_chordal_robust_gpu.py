"""Robust chordal initialisation on the device (kmx_chordal_residuals,
kmx_chordal_solve_robust; chordal.hip) against its host mirror,
kmx.dpgo.init.robust_chordal_initialization: the same GNC-TLS rule around the
host's direct solve.

Bounds. r^2 is a few dozen fp64 operations per edge with no cancellation
beyond the subtraction itself: 1e-12 relative (about 1e4 ulp of headroom); g
for moderate mu: 1e-12 absolute. The final g is all 0 or 1 and must EQUAL the
mirror's: the test first asserts, on the mirror alone, that no edge's
r^2 / c^2 is within 1e-3 of 1 at the last iterate, so the inlier set is no
rounding matter. R and t: test_chordal_gpu's TOL_R = 1e-8 / TOL_T = 1e-7 m
against the host's direct solve on the kept edges."""
import functools

import numpy as np
import pytest

from kmx import abi
from kmx.dpgo.chordal import ChordalSolver
from kmx.dpgo.init import (chordal_initialization, gnc_tls_factor, measurement_errors,
                           robust_chordal_initialization, robust_chordal_initialization_gpu)
from kmx.synth import make_pose_graph
from kmx.synth.pose_graph import _expm_so3

pytestmark = pytest.mark.gpu

TOL_R, TOL_T = 1e-8, 1e-7
RTOL = 1e-10
BARC = 5.0


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


def _ate(g, R, t):  # mean translation error against ground truth, first pose at the origin
    _, tg = _relative(g.gt_R[0], g.gt_t[0])
    return float(np.linalg.norm(t - tg, axis=1).mean())


@functools.lru_cache(maxsize=None)
def _case(n, m, frac, seed):
    """A one-robot graph with outliers, its odometry start and the host
    mirror's result (computed once, never modified)."""
    g = make_pose_graph(1, n, m, outlier_frac=frac, seed=seed)
    edges = _robot_edges(g)
    fixed = np.asarray(g.fixed) != 0
    ref = robust_chordal_initialization(n, edges, fixed, barc=BARC, return_info=True)
    return g, edges, fixed, _relative(g.init_R[0], g.init_t[0]), ref


@functools.lru_cache(maxsize=None)
def _gpu120():
    """The 120-pose graph from the odometry start: what the consistency,
    determinism and quality tests compare with."""
    g, edges, fixed, (Ro, to), _ = _case(120, 360, 0.2, 3)
    return robust_chordal_initialization_gpu(120, edges, fixed, R_init=Ro, t_init=to, barc=BARC, rtol=RTOL,
                                             return_info=True)


def _solver(n, edges, block_ptr=None, anchors=(0,)):
    s = ChordalSolver()
    src, dst, R, t, kap, tau, w = _arrays(edges)
    s.set_graph(n, [0, n] if block_ptr is None else block_ptr, src, dst, R, t, kap, tau, w, anchors=list(anchors))
    return s


# 1
def test_residual_known_answer(gpu):
    """R_ij = I, t_ij = (1, 0, 0), kappa = 2, tau = 3 between R_0 = I, t_0 = 0
    and R_1 = diag(1, -1, -1), t_1 = (1, 2, 0): |R_1 - R_0 R_ij|_F^2 = 8 and
    |t_1 - t_0 - R_0 t_ij|^2 = 4, so r^2 = 2 * 8 + 3 * 4 = 28 exactly; with
    c = 5 and mu = 1 the thresholds are 12.5 and 50, so g = sqrt(50 / 28) - 1."""
    s = _solver(2, [(0, 1, np.eye(3), np.array([1.0, 0.0, 0.0]), 2.0, 3.0, 1.0)])
    try:
        R = np.stack([np.eye(3), np.diag([1.0, -1.0, -1.0])])
        t = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 0.0]])
        assert s.residuals(R, t).tolist() == [28.0]
        r2, g = s.residuals(R, t, mu=[1.0], barc=5.0)
        assert r2.tolist() == [28.0] and abs(g[0] - (np.sqrt(50.0 / 28.0) - 1.0)) < 1e-15
        assert s.residuals(R, t, mu=[1.0], barc=5.0, fixed=[True])[1].tolist() == [1.0]
        assert s.residuals(R, t, mu=[1.0], barc=10.0)[1].tolist() == [1.0]   # 28 <= 50
        assert s.residuals(R, t, mu=[1.0], barc=3.0)[1].tolist() == [0.0]    # 28 >= 18
        # the inverse measurement from pose 1 to pose 0: t_0 - t_1 - R_1 (-1, 0, 0) = (0, -2, 0), again 28
        s2 = _solver(2, [(1, 0, np.eye(3), np.array([-1.0, 0.0, 0.0]), 2.0, 3.0, 1.0)])
        try:
            assert s2.residuals(R, t).tolist() == [28.0]
        finally:
            s2.close()
    finally:
        s.close()


# 2
def test_residuals_at_tile_and_hub_boundaries(gpu):
    """130 poses (tiles of 64 + 64 + 2), pose 7 with 70 extra edges in both
    directions (a hub wider than a wave) and parallel edges, at poses that are
    no solution (ground truth with per-pose perturbations over 2.5 decades)."""
    g = make_pose_graph(1, 130, 260, outlier_frac=0.2, seed=21)
    edges = _robot_edges(g)
    fixed = list(np.asarray(g.fixed) != 0)
    rng = np.random.default_rng(8)
    Rg, tg = g.gt_R[0], g.gt_t[0]
    for k, q in enumerate(range(40, 110)):
        i, j = (7, q) if k % 2 else (q, 7)
        Rij = Rg[i].T @ Rg[j] @ _expm_so3(rng.normal(0, 0.02, (1, 3)))[0]
        edges.append((i, j, Rij, Rg[i].T @ (tg[j] - tg[i]) + rng.normal(0, 0.1, 3), 5000.0, 70.0, 1.0))
        fixed.append(False)
    for e in (3, 200, 290):  # parallel edges, one of them reversed, with other precisions
        i, j, Rij, tij = edges[e][:4]
        edges += [(i, j, Rij, tij, 300.0, 20.0, 0.5), (j, i, Rij.T, -Rij.T @ tij, 40.0, 9.0, 1.0)]
        fixed += [False, True]
    fixed = np.array(fixed)
    src, dst, Rm, tm, kap, tau, _ = _arrays(edges)
    assert ((src == 7) | (dst == 7)).sum() > 64
    prng = np.random.default_rng(5)
    scale = 10 ** prng.uniform(-3, -0.5, 130)
    Rp = np.einsum("nij,njk->nik", Rg, _expm_so3(prng.normal(0, 1, (130, 3)) * scale[:, None]))
    tp = tg + prng.normal(0, 1, (130, 3)) * (10 * scale[:, None])
    ref = measurement_errors(src, dst, Rm, tm, kap, tau, Rp, tp)
    c2 = float(np.median(ref))
    s = _solver(130, edges)
    try:
        r2 = s.residuals(Rp, tp)
        rel = (np.abs(r2 - ref) / ref).max()
        print(f"max relative error of r^2: {rel:.3e}")
        assert rel < 1e-12
        for mu in (0.05, 1.0, 20.0):
            gr, frac = gnc_tls_factor(ref, mu, c2)
            gr[fixed] = 1.0
            free = ~fixed
            assert (gr[free] == 1).any() and (gr[free] == 0).any() and (frac & free).any(), mu
            r2b, gd = s.residuals(Rp, tp, mu=[mu], barc=np.sqrt(c2), fixed=fixed)
            assert np.array_equal(r2b, r2)
            # an edge within 1e-12 of a threshold could land in the other branch; none is
            lo, hi = mu / (mu + 1.0) * c2, (mu + 1.0) / mu * c2
            assert (np.abs(ref / lo - 1) > 1e-9).all() and (np.abs(ref / hi - 1) > 1e-9).all()
            err = np.abs(gd - gr).max()
            print(f"mu = {mu}: max |g - g_ref| = {err:.3e}")
            assert err < 1e-12
            assert (gd[fixed] == 1.0).all()
    finally:
        s.close()


# 3
@pytest.mark.parametrize("n,m,frac,seed", [(120, 360, 0.2, 3), (300, 900, 0.2, 7)])
def test_end_to_end_equals_the_host_mirror(gpu, n, m, frac, seed):
    g, edges, fixed, (Ro, to), (Rr, tr, gr, updates, ref) = _case(n, m, frac, seed)
    src, dst, Rm, tm, kap, tau, w0 = _arrays(edges)
    # the precondition, on the reference alone: no edge near a threshold at the end
    r2 = measurement_errors(src, dst, Rm, tm, kap, tau, Rr, tr)
    margin = np.abs(r2[~fixed] / BARC ** 2 - 1.0).min()
    print(f"mirror: {updates} updates, {ref}, min |r^2/c^2 - 1| = {margin:.3f}")
    assert margin >= 1e-3 and ref["converged"] and np.all((gr == 0) | (gr == 1))
    if n == 120:
        R, t, gd, upd, info, rinfo = _gpu120()
    else:
        R, t, gd, upd, info, rinfo = robust_chordal_initialization_gpu(n, edges, fixed, R_init=Ro, t_init=to,
                                                                       barc=BARC, rtol=RTOL, return_info=True)
    print(info, rinfo)
    assert np.array_equal(gd, gr)
    assert upd == rinfo["updates"] == updates and rinfo["converged"] == 1
    assert info["converged"]
    # the mirror's last solve is the host's direct solve on the kept edges
    Rk, tk = chordal_initialization(n, [e for e, k in zip(edges, gr) if k > 0])
    assert np.array_equal(Rk, Rr) and np.array_equal(tk, tr)
    _close(R, t, Rk, tk)
    n_lc = int((~fixed).sum())
    assert rinfo["n_kept"] + rinfo["n_rejected"] == n_lc and rinfo["n_fractional"] == 0
    assert rinfo["n_kept"] == int((gd[~fixed] == 1).sum()) == ref["n_kept"]
    assert rinfo["mu"] == pytest.approx(ref["mu"], rel=1e-6)
    assert (gd[np.asarray(g.outlier)[(g.r1 == 0) & (g.r2 == 0)]] == 0).all()  # no outlier is kept


# 4
def test_one_update_equals_the_residual_entry(gpu):
    g, edges, fixed, (Ro, to), _ = _case(120, 360, 0.2, 3)
    s = _solver(120, edges)
    try:
        R1, t1, g1, info, rinfo = s.solve_robust(fixed, Ro, to, barc=BARC, max_updates=1, rtol=RTOL)
        assert rinfo[0]["updates"] == 1 and rinfo[0]["converged"] == 0
        nf = int(((g1 > 0) & (g1 < 1)).sum())
        assert nf > 0 and rinfo[0]["n_fractional"] == nf
        assert rinfo[0]["n_kept"] + rinfo[0]["n_rejected"] + nf == int((~fixed).sum())
        R0, t0, _ = s.solve(Ro, to, rtol=RTOL)
        r2, ge = s.residuals(R0, t0, mu=[rinfo[0]["mu"]], barc=BARC, fixed=fixed)
        assert np.array_equal(g1, ge)
        # mu_0 = c^2 / (2 max r^2 - c^2) over the loop closures
        assert rinfo[0]["mu"] == BARC ** 2 / (2.0 * r2[~fixed].max() - BARC ** 2)
        assert not np.array_equal(R1, R0)  # the returned poses are the update's
    finally:
        s.close()


# 5, 6
def test_set_weights_consistency_and_the_handles_weights_survive(gpu):
    g, edges, fixed, (Ro, to), _ = _case(120, 360, 0.2, 3)
    R, t, gd, _, _, _ = _gpu120()
    w0 = _arrays(edges)[6]
    s = _solver(120, edges)
    try:
        Ra, ta, ia = s.solve(Ro, to, rtol=RTOL)
        Rb, tb, gb, _, _ = s.solve_robust(fixed, Ro, to, barc=BARC, rtol=RTOL)
        assert np.array_equal(Rb, R) and np.array_equal(tb, t) and np.array_equal(gb, gd)
        Rc, tc, ic = s.solve(Ro, to, rtol=RTOL)
        assert np.array_equal(Ra, Rc) and np.array_equal(ta, tc) and ia == ic
        s.set_weights(w0 * gd)
        Rw, tw, iw = s.solve(Ro, to, rtol=RTOL)
        assert iw[0]["converged"]
        _close(Rw, tw, R, t)
    finally:
        s.close()


# 7
def test_team_batch_is_bitwise_solo(gpu):
    """Blocks of 70, 130 and 65 poses with 20 %, 40 % and 10 % outliers, a pure
    chain of 65 (its odometry start is exact: 0 updates) and an empty block.
    The blocks stop after different numbers of updates, so the batch goes on
    while some of its blocks are frozen."""
    parts = [make_pose_graph(1, n, m, outlier_frac=f, seed=sd)
             for n, m, f, sd in ((70, 210, 0.2, 11), (130, 390, 0.4, 12), (65, 195, 0.1, 13))]
    blocks = [(int(p.n_poses[0]), _robot_edges(p), np.asarray(p.fixed) != 0, _relative(p.init_R[0], p.init_t[0]))
              for p in parts]
    rng = np.random.default_rng(11)
    Rrel, trel = _expm_so3(rng.normal(0, 0.2, (64, 3))), rng.normal(0, 1.0, (64, 3))
    Rc, tc = np.zeros((65, 3, 3)), np.zeros((65, 3))
    Rc[0] = np.eye(3)
    for k in range(64):
        Rc[k + 1], tc[k + 1] = Rc[k] @ Rrel[k], tc[k] + Rc[k] @ trel[k]
    blocks.append((65, [(k, k + 1, Rrel[k], trel[k], 100.0, 10.0, 1.0) for k in range(64)], np.ones(64, bool),
                   (Rc, tc)))
    ptr, edges, fixed, R0, t0 = [0], [], [], [], []
    for n, E, f, (Rs, ts) in blocks:
        edges += [(e[0] + ptr[-1], e[1] + ptr[-1]) + e[2:] for e in E]
        fixed.append(f)
        R0.append(Rs)
        t0.append(ts)
        ptr.append(ptr[-1] + n)
    ptr.append(ptr[-1])  # the empty block
    fixed = np.concatenate(fixed)
    s = _solver(ptr[-1], edges, block_ptr=ptr, anchors=ptr[:4])
    try:
        R, t, gt, info, rinfo = s.solve_robust(fixed, np.concatenate(R0), np.concatenate(t0), barc=BARC, rtol=RTOL)
    finally:
        s.close()
    print(rinfo)
    assert len(rinfo) == 5
    e0 = 0
    for b, (n, E, f, (Rs, ts)) in enumerate(blocks):
        one = _solver(n, E)
        try:
            Rb, tb, gb, ib, rb = one.solve_robust(f, Rs, ts, barc=BARC, rtol=RTOL)
        finally:
            one.close()
        assert np.array_equal(R[ptr[b]:ptr[b + 1]], Rb) and np.array_equal(t[ptr[b]:ptr[b + 1]], tb), b
        assert np.array_equal(gt[e0:e0 + len(E)], gb), b
        assert rinfo[b] == rb[0] and info[b] == ib[0], b
        assert rb[0]["converged"] == 1
        e0 += len(E)
    assert rinfo[3]["updates"] == 0 and rinfo[3]["converged"] == 1 and rinfo[3]["n_kept"] == 0
    assert rinfo[4] == {"updates": 0, "converged": 1, "n_kept": 0, "n_rejected": 0, "n_fractional": 0, "mu": 0.0}
    assert len({r["updates"] for r in rinfo[:4]}) >= 3  # frozen blocks while others still run
    for b in range(3):
        assert rinfo[b]["n_rejected"] > 0 and rinfo[b]["n_fractional"] == 0


# 8
def test_determinism_and_check_every(gpu):
    g, edges, fixed, (Ro, to), _ = _case(120, 360, 0.2, 3)
    ref = _gpu120()
    for ce in (0, 1, 7, 1000):
        out = robust_chordal_initialization_gpu(120, edges, fixed, R_init=Ro, t_init=to, barc=BARC, rtol=RTOL,
                                                check_every=ce, return_info=True)
        for a, b in zip(out[:3], ref[:3]):
            assert np.array_equal(a, b), ce
        assert out[3:] == ref[3:], ce


# 9
def test_dpgo_mu_init_reaches_the_same_inliers(gpu):
    g, edges, fixed, (Ro, to), _ = _case(120, 360, 0.2, 3)
    _, _, gd, upd, _, _ = _gpu120()
    _, _, g5, upd5, _, r5 = robust_chordal_initialization_gpu(120, edges, fixed, R_init=Ro, t_init=to, barc=BARC,
                                                              mu_init=1e-5, rtol=RTOL, return_info=True)
    assert r5["converged"] == 1 and np.array_equal(g5, gd)
    assert upd5 > upd


# 10
def test_refusals_leave_the_handle_usable(gpu):
    g, edges, fixed, (Ro, to), _ = _case(120, 360, 0.2, 3)
    R, t, gd, _, _, _ = _gpu120()
    src, dst = _arrays(edges)[:2]
    s = ChordalSolver()
    try:
        with pytest.raises(abi.KmxError, match=r"\(-3\)"):  # KMX_ESTATE
            s.solve_robust(None)
        with pytest.raises(abi.KmxError, match=r"\(-3\)"):
            s.residuals(np.zeros((0, 3, 3)), np.zeros((0, 3)))
    finally:
        s.close()
    s = _solver(120, edges)
    try:
        bad = fixed.copy()
        bad[(src == 57) | (dst == 57)] = False  # nothing fixed holds pose 57
        with pytest.raises(abi.KmxError, match=r"\(-1\).*pose 57"):  # KMX_EINVAL
            s.solve_robust(bad, Ro, to, barc=BARC, rtol=RTOL)
        with pytest.raises(abi.KmxError, match=r"\(-1\)"):  # no fixed edge at all, 119 free poses
            s.solve_robust(None, Ro, to, barc=BARC, rtol=RTOL)
        with pytest.raises(abi.KmxError, match=r"\(-1\)"):
            s.solve_robust(np.zeros(len(edges), bool), Ro, to, barc=BARC, rtol=RTOL)
        Rb, tb, gb, _, _ = s.solve_robust(fixed, Ro, to, barc=BARC, rtol=RTOL)
        assert np.array_equal(Rb, R) and np.array_equal(tb, t) and np.array_equal(gb, gd)
    finally:
        s.close()


# 11
def test_quality_and_the_agent(gpu):
    from kmx.dpgo.agent import PGOAgent
    from kmx.dpgo.init import chordal_initialization_gpu
    from kmx.dpgo.messages import RelativeSEMeasurement
    from kmx.dpgo.params import PGOAgentParameters
    g, edges, fixed, (Ro, to), _ = _case(120, 360, 0.2, 3)
    R, t, _, _, _, _ = _gpu120()
    Rp, tp = chordal_initialization_gpu(120, edges, R_init=Ro, t_init=to, rtol=RTOL)
    ate, ate_odo, ate_l2 = _ate(g, R, t), _ate(g, Ro, to), _ate(g, Rp, tp)
    print(f"ATE: robust chordal {ate:.3f} m, odometry chain {ate_odo:.3f} m, L2 chordal {ate_l2:.3f} m")
    assert ate < 0.5 * ate_odo and ate < ate_l2
    P = PGOAgentParameters(r=5, num_robots=1, localInitializationMethod="robust_chordal_gpu")
    ag = PGOAgent(0, P)  # the real BlockSolver
    for e in range(g.m):
        ag.addMeasurement(RelativeSEMeasurement(0, 0, int(g.p1[e]), int(g.p2[e]), 3, g.R[e], g.t[e],
                                                float(g.kappa[e]), float(g.tau[e]), fixedWeight=bool(g.fixed[e])))
    ag.initialize()
    T = ag.getTrajectoryInLocalFrame().reshape(3, -1, 4).transpose(1, 0, 2)
    # the agent passes its odometry first and then its loop closures: the sums run in another order
    _close(T[:, :, :3], T[:, :, 3], R, t)
    if hasattr(ag.solver, "close"):
        ag.solver.close()
