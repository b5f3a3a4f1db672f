"""The Riemannian staircase on the device (kmx_cert_escape,
kmx_cert_escape_commit, kmx.dpgo.staircase): the lifted
candidates against escape_point and their costs against dense numpy, the
library's refusals, determinism, the escape step and the whole staircase on
the winding ring (known answer: two escapes, ranks 3, 4, 5, the cost halves
and then vanishes), the stop conditions and the pipeline's entry."""
import numpy as np
import pytest

from tests import cert_ref as CR
from tests import stair_ref as SR
from tests.test_cert_gpu import GRAPHS, _check_apply_lambda, _dense, solved_noisy_graph  # noqa: F401

pytestmark = pytest.mark.gpu

LADDERS = {"zero": [0.0], "one": [1.0], "ladder8": [2.0 ** -k for k in range(8)]}

# the level solves of the ring (chosen on the CPU restatement of the solver, where level 1 of the 24-pose ring
# cut into three robots reaches grad_tol in 43 sweeps and level 2 in 45; stationarity ends below 2e-7)
RING_KW = dict(eta=1e-5, grad_tol=1e-7, stat_tol=1e-6, max_rounds=400)


def _ring_params():
    from kmx.dpgo.params import PGOAgentParameters
    P = PGOAgentParameters(r=3)
    P.localOptimizationParams.RTR_iterations = 8  # rejected steps quarter the radius from 100 in every update
    P.localOptimizationParams.RTR_tCG_iterations = 50
    return P


def _cost_and_bound(Q, Z):
    F = CR.flat_X(Z)
    return float(np.trace(F @ Q @ F.T)), 1e-12 * float(np.trace(np.abs(F) @ np.abs(Q) @ np.abs(F).T))


@pytest.mark.parametrize("r", [3, 5, 7])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_lift_and_cost_match_numpy(gpu, name, r):
    from kmx.dpgo.certify import Certifier, escape_point
    g = GRAPHS[name]()
    n = g["n_poses"]
    X = CR.random_point(n, r, 40 + r)
    y = np.random.default_rng(50 + r).standard_normal(4 * n)
    y /= np.linalg.norm(y)
    Q, _ = _dense(g, X)
    c = Certifier()
    c.set_graph(**g)
    for lname, ladder in LADDERS.items():
        for k, a in enumerate(ladder):
            if lname == "ladder8" and k not in (1, 7):  # alpha = 1 and 0 have ladders of their own
                continue
            info0 = c.set_point(X)
            esc = c.escape(y, ladder)
            assert esc["cost"].shape == (len(ladder),) and c.r == r
            Z, info = c.escape_commit(k)
            assert Z.shape == (n, r + 1, 4) and c.r == r + 1
            ref = escape_point(X, y, a)
            YtY = np.einsum("nac,nad->ncd", Z[:, :, :3], Z[:, :, :3])
            want, bound = _cost_and_bound(Q, Z)
            print(name, r, lname, k, "rot", np.abs(Z[:, :, :3] - ref[:, :, :3]).max(), "orth",
                  np.abs(YtY - np.eye(3)).max(), "cost err / bound", abs(esc["cost"][k] - want) / max(bound, 1e-300))
            assert np.abs(Z[:, :, :3] - ref[:, :, :3]).max() <= 1e-13
            assert np.array_equal(Z[:, :, 3], ref[:, :, 3])
            assert np.abs(YtY - np.eye(3)).max() <= 1e-14
            assert abs(esc["cost"][k] - want) <= bound
            assert abs(info["cost"] - esc["cost"][k]) <= bound
            if a == 0.0:
                assert np.array_equal(Z[:, :r], X) and not Z[:, r].any()
                assert abs(esc["cost"][k] - info0["cost"]) <= bound
                assert esc["best"] == -1  # nothing is strictly below
            # the committed point serves the certificate's kernels at rank r + 1
            _check_apply_lambda(c, g, Z, 60 + r)
    c.close()


def test_library_refuses_malformed_escapes(gpu):
    import ctypes as C

    from kmx import abi
    from kmx.dpgo.certify import Certifier
    g = CR.random_graph(65, 60, 4)
    n = 65
    c = Certifier()
    c.set_graph(**g)
    y = np.random.default_rng(1).standard_normal(4 * n)
    al = np.array([1.0, 0.5] + [0.25] * 7)
    cost, best = np.zeros(9), C.c_int32(7)
    Xo = np.zeros((n, 9, 4))

    def esc(yv, k, av):
        return c.L.kmx_cert_escape(c.h, abi.fptr(yv), k, abi.fptr(av), abi.fptr(cost), C.byref(best))

    assert esc(y, 2, al) == abi.KMX_ESTATE  # no point
    assert c.L.kmx_cert_escape_commit(c.h, 0, abi.fptr(Xo), None) == abi.KMX_ESTATE
    c.set_point(CR.random_point(n, 8, 2))
    assert esc(y, 2, al) == abi.KMX_EUNSUP  # no rank 9
    X = CR.random_point(n, 4, 3)
    c.set_point(X)
    assert c.L.kmx_cert_escape_commit(c.h, 0, abi.fptr(Xo), None) == abi.KMX_ESTATE  # no escape yet
    assert esc(y, 0, al) == abi.KMX_EINVAL and esc(y, 9, al) == abi.KMX_EINVAL
    bad = y.copy()
    bad[-1] = np.nan
    assert esc(bad, 2, al) == abi.KMX_EINVAL
    assert esc(y, 2, np.array([1.0, np.nan])) == abi.KMX_EINVAL
    assert esc(y, 2, al) == abi.KMX_OK
    assert c.L.kmx_cert_escape_commit(c.h, 2, abi.fptr(Xo), None) == abi.KMX_EINVAL  # k out of range
    assert c.L.kmx_cert_escape_commit(c.h, -1, abi.fptr(Xo), None) == abi.KMX_EINVAL
    c.set_weights(g["weight"] * 0.5)
    assert c.L.kmx_cert_escape_commit(c.h, 0, abi.fptr(Xo), None) == abi.KMX_ESTATE  # the costs were the old weights'
    # the handle works afterwards: the point is still X at rank 4 with the new weights
    g2 = dict(g, weight=g["weight"] * 0.5)
    _check_apply_lambda(c, g2, X, 5)
    out = c.escape(y, [0.5])
    Q, _ = _dense(g2, X)
    Z, info = c.escape_commit(0)
    want, bound = _cost_and_bound(Q, Z)
    assert abs(out["cost"][0] - want) <= bound and c.r == 5
    with pytest.raises(abi.KmxError, match=r"\(-3\)"):  # a commit consumes the escape
        c.escape_commit(0)
    c.close()


def test_escape_is_deterministic_and_independent_of_the_batch(gpu):
    from kmx.dpgo.certify import Certifier
    g = GRAPHS["n130"]()
    X = CR.random_point(130, 5, 7)
    y = np.random.default_rng(8).standard_normal(4 * 130)
    y /= np.linalg.norm(y)
    ladder = LADDERS["ladder8"]
    c = Certifier()
    c.set_graph(**g)
    c.set_point(X)
    a = c.escape(y, ladder)
    b = c.escape(y, ladder)
    assert np.array_equal(a["cost"], b["cost"]) and a["best"] == b["best"]
    Za, _ = c.escape_commit(3)
    c.set_point(X)
    single = np.array([c.escape(y, [al])["cost"][0] for al in ladder])
    assert np.array_equal(single, a["cost"])
    c.escape(y, ladder[3:4])
    Zb, _ = c.escape_commit(0)
    assert np.array_equal(Za, Zb)
    c.close()


@pytest.mark.parametrize("n", [8, 24])
def test_ring_escape_step(gpu, n):
    from kmx.dpgo.certify import Certifier
    from kmx.dpgo.staircase import DEFAULT_ALPHAS
    g, X = CR.ring(n, 3)
    lam = -(2.0 - 2.0 * np.cos(2.0 * np.pi / n))
    c = Certifier()
    c.set_graph(**g)
    info = c.set_point(X)
    res = c.min_eig(0.5 * abs(lam), want_vector=True)
    assert res["decision"] == "NEGATIVE"
    esc = c.escape(res["y"], DEFAULT_ALPHAS)
    drop = info["cost"] - esc["cost"][7]
    want = DEFAULT_ALPHAS[7] ** 2 * abs(res["theta_min"])
    print("costs", esc["cost"], "cost", info["cost"], "drop", drop, "alpha^2 |theta_min|", want, "rel",
          drop / want - 1.0)
    assert esc["best"] == 0 and esc["cost"][0] < info["cost"]
    assert abs(drop - want) <= 0.01 * want
    c.close()


@pytest.mark.parametrize("n,robots", [(8, 1), (24, 1), (24, 3)])
def test_staircase_climbs_the_ring_to_rank_5(gpu, n, robots):
    """Known answer (numpy: dense Q, Riemannian gradient descent, eigh): cost
    f3 = 2n(2 - 2cos(2pi/n)) at rank 3, f3 / 2 at rank 4, below 1e-13 at rank
    5, lambda_min = -(2 - 2cos(2pi/n)) at ranks 3 and 4."""
    from kmx import pipeline as PL
    from kmx.dpgo.staircase import staircase_team
    g, Xs, gd = SR.ring_team(n, robots)
    out = staircase_team(g, Xs, None, _ring_params(), r_max=6, **RING_KW)
    lv = out["levels"]
    for q in lv:
        print({k: q[k] for k in ("r", "rounds", "block_steps", "cost", "stationarity", "decision", "theta_min",
                                 "steps", "alpha", "solve_seconds", "certify_seconds", "escape_seconds")})
    f3, lam = SR.f3(n), -(2.0 - 2.0 * np.cos(2.0 * np.pi / n))
    assert [q["r"] for q in lv] == [3, 4, 5]
    assert [q["decision"] for q in lv] == ["NEGATIVE", "NEGATIVE", "CERTIFIED"]
    assert out["status"] == "CERTIFIED" and out["r"] == 5
    assert lv[0]["block_steps"] == 0  # exactly stationary: every block update was skipped
    assert abs(lv[0]["cost"] - f3) <= 1e-12 * f3
    assert abs(lv[1]["cost"] - f3 / 2) <= 1e-6 * f3 / 2
    assert lv[2]["cost"] <= 1e-9 * f3
    for q in lv[:2]:
        assert lam - 1e-9 <= q["theta_min"] < -RING_KW["eta"] and q["best"] >= 0 and q["alpha"] > 0
    X = np.concatenate([out["X"][a] for a in range(robots)])
    assert X.shape == (n, 5, 4) and out["lift"].shape == (5, 3)
    # the dense restatement of the final point
    Q = CR.dense_Q(n, gd["src"], gd["dst"], gd["R"], gd["t"], gd["kappa"], gd["tau"], gd["weight"])
    F = CR.flat_X(X)
    assert np.trace(F @ Q @ F.T) <= 1e-9 * f3
    R, _ = PL.rounded(X, out["lift"])
    assert np.abs(SR.relative_rotations(R, gd["src"], gd["dst"]) - np.eye(3)).max() <= 1e-6


def test_staircase_stops_at_the_rank_limit(gpu):
    from kmx.dpgo.staircase import staircase_team
    g, Xs, _ = SR.ring_team(8)
    out = staircase_team(g, Xs, None, _ring_params(), r_max=4, **RING_KW)
    assert out["status"] == "RANK_LIMIT" and out["r"] == 4
    assert [q["r"] for q in out["levels"]] == [3, 4] and out["levels"][-1]["decision"] == "NEGATIVE"
    assert out["levels"][-1]["alpha"] is None and out["X"][0].shape == (8, 4, 4)
    with pytest.raises(ValueError, match="r_max"):
        staircase_team(g, Xs, None, _ring_params(), r_max=2, **RING_KW)


def _one_robot_graph():
    from kmx.synth import make_pose_graph
    return make_pose_graph(1, 60, 119, outlier_frac=0.0, seed=5)  # solved_noisy_graph's


def test_staircase_certifies_a_solved_graph_at_level_0(gpu, solved_noisy_graph):  # noqa: F811
    from kmx.dpgo.params import PGOAgentParameters
    from kmx.dpgo.staircase import staircase_team
    gd, X, _, _ = solved_noisy_graph
    g = _one_robot_graph()
    P = PGOAgentParameters(r=5)
    P.localOptimizationParams.RTR_iterations = 8  # rejected steps quarter the radius from 100 in every update
    P.localOptimizationParams.RTR_tCG_iterations = 50
    out = staircase_team(g, {0: X}, None, P, eta=1e-5, r_max=6, grad_tol=1e-6, stat_tol=1e-3, max_rounds=50)
    print(out["status"], out["levels"])
    assert out["status"] == "CERTIFIED" and out["r"] == 5 and len(out["levels"]) == 1
    assert out["levels"][0]["escape_cost"] is None and out["X"][0].shape == (60, 5, 4)


def test_staircase_does_not_raise_the_rank_of_an_unconverged_iterate(gpu):
    from kmx.dpgo.params import PGOAgentParameters, RobustCostType
    from kmx.dpgo.solver import BlockSolver
    from kmx.dpgo.staircase import staircase_team
    from kmx.synth import lift, lifting_matrix
    g = _one_robot_graph()
    P = PGOAgentParameters(r=5)
    P.robustCostParams.costType = RobustCostType.L2
    s = BlockSolver(P, 0)
    s.set_graph_data(g)
    s.set_iterate(0, lift(g.init_R[0], g.init_t[0], lifting_matrix(5, seed=1)))
    for _ in range(2):
        s.refresh_local()
        s.iterate()
    X = s.get_iterate(0)
    s.close()
    out = staircase_team(g, {0: X}, None, P, eta=1e-5, r_max=6, grad_tol=1e-6, stat_tol=1e-3, max_rounds=0)
    lv = out["levels"]
    print(out["status"], lv)
    assert out["status"] == "NOT_STATIONARY" and out["r"] == 5 and len(lv) == 1
    assert lv[0]["decision"] == "NEGATIVE" and lv[0]["stationarity"] > 1e-3 and lv[0]["rounds"] == 0
    assert np.array_equal(out["X"][0], X)


def test_pipeline_staircase(gpu):
    from kmx import pipeline as PL
    from kmx.dpgo.params import PGOAgentParameters
    from kmx.lcd import LcdParams
    from kmx.synth import make_pose_graph
    g0 = make_pose_graph(3, 600, 2400, f_inter=0.0, outlier_scope="robot", seed=4)
    st = PL.make_lc_stream(g0, 24, 12, n_feats=200, seed=2)
    P = PGOAgentParameters(r=5)
    P.robustOptInnerIters = 10
    out = PL.run_pipeline(g0, st, P, LcdParams(), rounds=30, device=0, certify_eta=1e-5, staircase_rmax=6,
                          staircase_kw=dict(max_rounds=20))
    sc = out["staircase"]
    print(sc["status"], sc["r"], sc["ate_m"], [(q["r"], q["rounds"], q["decision"], q["stationarity"])
                                                for q in sc["levels"]])
    assert sc["status"] in ("CERTIFIED", "UNDECIDED", "RANK_LIMIT", "NOT_STATIONARY", "NO_DESCENT")
    assert len(sc["levels"]) >= 1 and np.isfinite(sc["ate_m"]) and 5 <= sc["r"] <= 6
    cert = out["certificate"]
    assert cert["decision"] in ("CERTIFIED", "NEGATIVE", "UNDECIDED") and cert["steps"] >= 1
    assert abs(cert["cost"] - 2.0 * out["dpgo"]["cost"]) <= 1e-9 * cert["cost"]
