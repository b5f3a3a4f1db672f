"""The dual certificate on the device (kmx_cert_*, cert.hip) against the dense
numpy restatement tests/cert_ref.py: S v and Lambda elementwise, the first
Lanczos coefficients, the known answers (the winding ring: NEGATIVE with
lambda_min = -(2 - 2 cos(2 pi / n)); noise-free and solved noisy graphs:
CERTIFIED), determinism, and the pipeline's certificate entry."""
import numpy as np
import pytest

from tests import cert_ref as CR

pytestmark = pytest.mark.gpu


def _dense(g, X, w=None):
    Q = CR.dense_Q(g["n_poses"], g["src"], g["dst"], g["R"], g["t"], g["kappa"], g["tau"],
                   g["weight"] if w is None else w)
    return Q, CR.dense_S(X, Q)


def _star(hub_incidences=200):
    """Pose 0 with hub_incidences edges, half of them outgoing."""
    g = CR.random_graph(hub_incidences + 1, 0, 11, chain=False)
    rng = np.random.default_rng(12)
    k = hub_incidences
    leaves = np.arange(1, k + 1, dtype=np.int32)
    out = np.arange(k) % 2 == 0
    g.update(src=np.where(out, 0, leaves).astype(np.int32), dst=np.where(out, leaves, 0).astype(np.int32),
             R=CR.random_rotations(rng, k), t=rng.standard_normal((k, 3)), kappa=rng.uniform(0.5, 3.0, k),
             tau=rng.uniform(0.5, 3.0, k), weight=rng.uniform(0.2, 1.5, k))
    return g


def _mixed():
    """Parallel edges (both directions), edges of weight 0 and an isolated pose."""
    g = CR.random_graph(40, 30, 13)
    rng = np.random.default_rng(14)
    src = np.concatenate([g["src"], g["src"][:10], g["dst"][10:20]]).astype(np.int32)
    dst = np.concatenate([g["dst"], g["dst"][:10], g["src"][10:20]]).astype(np.int32)
    k = src.shape[0]
    w = rng.uniform(0.2, 1.5, k)
    w[::7] = 0.0
    return dict(n_poses=42, src=src, dst=dst, R=CR.random_rotations(rng, k), t=rng.standard_normal((k, 3)),
                kappa=rng.uniform(0.5, 3.0, k), tau=rng.uniform(0.5, 3.0, k), weight=w)  # poses 40, 41: no edges


GRAPHS = {
    "n1": lambda: CR.random_graph(1, 0, 1),
    "n63": lambda: CR.random_graph(63, 60, 2),
    "n64": lambda: CR.random_graph(64, 60, 3),
    "n65": lambda: CR.random_graph(65, 60, 4),
    "n130": lambda: CR.random_graph(130, 150, 5),
    "star200": _star,
    "mixed": _mixed,
}


def _check_apply_lambda(c, g, X, seed, termwise=False):
    n = g["n_poses"]
    Q, S = _dense(g, X)
    v = np.random.default_rng(seed).standard_normal(4 * n)
    out = c.apply(v)
    err = np.abs(out - S @ v)
    bound = 1e-12 * (np.abs(S) @ np.abs(v))
    print("apply: max err", err.max(), "max err / bound", (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all()
    L = c.lambda_blocks()
    errL = np.abs(L - CR.lambda_blocks(X, Q))
    boundL = 1e-12 * CR.lambda_bound(X, Q, termwise)
    print("lambda: max err", errL.max(), "max err / bound", (errL / np.maximum(boundL, 1e-300)).max())
    assert (errL <= boundL).all()
    return Q, S


@pytest.mark.parametrize("r", [3, 5, 8])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_apply_and_lambda_match_dense_numpy(gpu, name, r):
    from kmx.dpgo.certify import Certifier
    g = GRAPHS[name]()
    X = CR.random_point(g["n_poses"], r, 20 + r)  # orthonormal Y_i; not stationary
    c = Certifier()
    c.set_graph(**g)
    info = c.set_point(X)
    Q, S = _check_apply_lambda(c, g, X, 30 + r)
    ref = CR.point_info(X, Q)
    print(info, ref)
    for k in ("cost", "trace_lambda", "stationarity"):
        assert abs(info[k] - ref[k]) <= 1e-12 * abs(ref[k]), k
    if name != "n1":
        assert info["stationarity"] > 1e-3 * np.abs(S).max()  # the point is not stationary
    c.close()


def test_apply_and_lambda_at_a_stationary_point(gpu):
    from kmx.dpgo.certify import Certifier
    g, X = CR.consistent_graph(65, 80, 5, 6)
    c = Certifier()
    c.set_graph(**g)
    info = c.set_point(X)
    # X Q = 0 here but for rounding, so Lambda is held to the bound of the terms that cancel
    Q, S = _check_apply_lambda(c, g, X, 7, termwise=True)
    scale = np.abs(Q).max()
    assert info["stationarity"] <= 1e-12 * scale * np.sqrt(4 * 65 * 5) and abs(info["cost"]) <= 1e-12 * scale * 65
    c.close()


def test_library_refuses_malformed_calls(gpu):
    import ctypes as C

    from kmx import abi
    from kmx.dpgo.certify import Certifier
    c = Certifier()
    with pytest.raises(abi.KmxError, match=r"\(-3\)"):  # KMX_ESTATE: no graph
        c.n = 4
        c.set_point(np.zeros((4, 3, 4)))
    g = CR.random_graph(10, 5, 1)
    c.set_graph(**g)
    with pytest.raises(abi.KmxError, match=r"\(-3\)"):  # no point
        c.apply(np.zeros(40))
    X = np.zeros((10, 9, 4))
    assert c.L.kmx_cert_set_point(c.h, 9, abi.fptr(X), None) == abi.KMX_EINVAL
    assert c.L.kmx_cert_set_point(c.h, 2, abi.fptr(X), None) == abi.KMX_EINVAL
    # a refused graph leaves the handle with the one it had
    bad = dict(g)
    bad["kappa"] = g["kappa"].copy()
    bad["kappa"][2] = 0.0
    src, dst = g["src"], g["dst"]
    rc = c.L.kmx_cert_set_graph(c.h, 10, src.shape[0], abi.iptr(src), abi.iptr(dst),
                                abi.fptr(np.ascontiguousarray(g["R"])), abi.fptr(g["t"]), abi.fptr(bad["kappa"]),
                                abi.fptr(g["tau"]), abi.fptr(g["weight"]))
    assert rc == abi.KMX_EINVAL
    Xp = CR.random_point(10, 4, 2)
    c.set_point(Xp)
    _check_apply_lambda(c, g, Xp, 3)
    res = abi.CertResult()
    p = abi.CertParams(0.0, 0, 0, 0, 0, 0)
    assert c.L.kmx_cert_min_eig(c.h, C.byref(p), C.byref(res), None) == abi.KMX_EINVAL  # eta is required
    c.close()


def test_first_lanczos_coefficients_and_set_weights(gpu):
    from kmx.dpgo.certify import Certifier
    g = CR.random_graph(130, 150, 5)
    X = CR.random_point(130, 5, 8)
    c = Certifier()
    c.set_graph(**g)
    c.set_point(X)
    rng = np.random.default_rng(9)
    for w in (None, g["weight"] * rng.uniform(0.0, 2.0, g["weight"].shape[0]), np.ones(g["weight"].shape[0])):
        if w is not None:
            c.set_weights(w)
        _, S = _dense(g, X, w)
        tmax = np.abs(np.linalg.eigvalsh(S)).max()
        res = c.min_eig(1e-30, max_steps=20, test_every=20, seed=42)
        al, be = c.coefficients()
        ar, br = CR.lanczos(S, 20, 42)
        print("alpha err", np.abs(al - ar).max() / tmax, "beta err", np.abs(be - br).max() / tmax)
        assert res["steps"] == 20 and al.shape == (20,)
        assert np.abs(al - ar).max() <= 1e-10 * tmax and np.abs(be - br).max() <= 1e-10 * tmax
        v = rng.standard_normal(4 * 130)  # apply follows the weights too
        assert (np.abs(c.apply(v) - S @ v) <= 1e-12 * (np.abs(S) @ np.abs(v))).all()
    c.close()


@pytest.mark.parametrize("r", [3, 5])
@pytest.mark.parametrize("n", [8, 24, 100])
def test_winding_ring_is_negative_with_the_known_eigenvalue(gpu, n, r):
    from kmx.dpgo.certify import Certifier, escape_point
    g, X = CR.ring(n, r)
    Q, S = _dense(g, X)
    lam = -(2.0 - 2.0 * np.cos(2.0 * np.pi / n))
    assert abs(np.linalg.eigvalsh(S)[0] - lam) < 1e-12
    c = Certifier()
    c.set_graph(**g)
    info = c.set_point(X)
    assert info["stationarity"] <= 1e-12
    res = c.min_eig(1e-5)
    print(res)
    assert res["decision"] == "NEGATIVE" and res["theta_min"] >= lam - 1e-12
    res = c.min_eig(0.5 * abs(lam), want_vector=True)
    y = res["y"]
    print(res["steps"], res["theta_min"], res["residual"], lam)
    assert res["decision"] == "NEGATIVE"
    assert abs(np.linalg.norm(y) - 1.0) <= 1e-12
    assert abs(y @ S @ y - res["theta_min"]) <= res["residual"]
    f = lambda Z: float(np.trace(CR.flat_X(Z) @ Q @ CR.flat_X(Z).T))  # noqa: E731
    drop = f(X) - f(escape_point(X, y, 0.05))
    want = 0.05 ** 2 * abs(res["theta_min"])
    print("drop", drop, "0.05^2 |theta_min|", want, "rel", drop / want - 1.0)
    assert drop > 0 and abs(drop - want) <= 0.01 * want
    c.close()


@pytest.fixture(scope="module")
def noise_free_team():
    from kmx.dpgo.certify import flatten_team
    from kmx.synth import lift, lifting_matrix, make_pose_graph
    g = make_pose_graph(3, 120, 300, outlier_frac=0.0, noise_free=True, seed=3)
    Y = lifting_matrix(5, seed=1)
    Xs = {a: lift(g.gt_R[a], g.gt_t[a], Y) for a in range(3)}
    n, src, dst, X = flatten_team(g, Xs)
    gd = dict(n_poses=n, src=src, dst=dst, R=g.R, t=g.t, kappa=g.kappa, tau=g.tau, weight=g.weight)
    _, S = _dense(gd, X)
    ev = np.linalg.eigvalsh(S)
    return g, Xs, gd, X, S, ev


def test_noise_free_team_is_certified(gpu, noise_free_team):
    from kmx.dpgo.certify import certify_team
    g, Xs, gd, X, S, ev = noise_free_team
    eta = 1e-8 * ev[-1]
    out = certify_team(g, Xs, eta=eta, want_vector=True)
    print({k: v for k, v in out.items() if k != "y"}, "dense lambda_min", ev[0])
    assert out["decision"] == "CERTIFIED"
    assert out["residual"] <= eta and out["theta_min"] - out["residual"] >= -eta
    assert out["stationarity"] <= 1e-12 * ev[-1] * np.sqrt(X.size)
    y = out["y"]
    assert abs(np.linalg.norm(y) - 1.0) <= 1e-12


def test_check_every_changes_no_bit_and_two_calls_agree(gpu, noise_free_team):
    from kmx.dpgo.certify import Certifier
    _, _, gd, X, _, ev = noise_free_team
    eta = 1e-8 * ev[-1]
    c = Certifier()
    c.set_graph(**gd)
    c.set_point(X)
    a = c.min_eig(eta, check_every=50, seed=5, want_vector=True)
    assert a["steps"] > 20  # more than one batch and one test
    for every in (1, 7, 50):  # 50 again: two calls agree
        b = c.min_eig(eta, check_every=every, seed=5, want_vector=True)
        for k in ("decision", "steps", "theta_min", "theta_max", "residual"):
            assert a[k] == b[k], (every, k)
        assert np.array_equal(a["y"], b["y"]), every
    other = c.min_eig(eta, seed=6)
    assert other["decision"] == a["decision"] and other["theta_min"] != a["theta_min"]  # the seed is used
    c.close()


@pytest.fixture(scope="module")
def solved_noisy_graph():
    """A noisy single-robot graph of 60 poses and 60 loop closures, r = 5,
    solved on the device by BlockSolver's RTR steps from the odometry chain."""
    from kmx.dpgo.certify import flatten_team
    from kmx.dpgo.params import PGOAgentParameters, RobustCostType
    from kmx.dpgo.solver import BlockSolver
    from kmx.synth import lift, lifting_matrix, make_pose_graph
    g = make_pose_graph(1, 60, 119, outlier_frac=0.0, seed=5)
    P = PGOAgentParameters(r=5)
    P.robustCostParams.costType = RobustCostType.L2
    P.localOptimizationParams.gradnorm_tol = 1e-12
    P.localOptimizationParams.RTR_iterations = 3
    P.localOptimizationParams.RTR_tCG_iterations = 50
    s = BlockSolver(P, 0)
    s.set_graph_data(g)
    s.set_iterate(0, lift(g.init_R[0], g.init_t[0], lifting_matrix(5, seed=1)))
    gn = np.inf
    for it in range(400):
        s.refresh_local()
        gn = s.iterate()[0]["gradnorm_init"]
        if gn < 1e-9:
            break
    X = s.get_iterate(0)
    s.close()
    n, src, dst, Xf = flatten_team(g, {0: X})
    gd = dict(n_poses=n, src=src, dst=dst, R=g.R, t=g.t, kappa=g.kappa, tau=g.tau, weight=g.weight)
    _, S = _dense(gd, Xf)
    return gd, Xf, S, gn


def test_solved_noisy_graph_is_certified_and_undecided_when_cut_short(gpu, solved_noisy_graph):
    from kmx.dpgo.certify import Certifier
    gd, X, S, gn = solved_noisy_graph
    eta = 1e-5
    ev = np.linalg.eigvalsh(S)
    print("RTR gradient norm", gn, "dense lambda_min", ev[0], "lambda_max", ev[-1])
    assert ev[0] >= -eta / 2, f"the solve was not tight: lambda_min(S) = {ev[0]} at gradient norm {gn}"
    c = Certifier()
    c.set_graph(**gd)
    info = c.set_point(X)
    res = c.min_eig(eta)
    print(info, res)
    assert res["decision"] == "CERTIFIED" and res["theta_min"] - res["residual"] >= -eta
    cut = c.min_eig(eta, max_steps=10)
    assert cut["decision"] == "UNDECIDED" and cut["steps"] == 10 and cut["theta_max"] <= ev[-1] * (1 + 1e-12)
    t = c.timing()
    assert t["set_point_ms"] > 0 and t["lanczos_ms"] > 0 and t["vector_ms"] == 0
    c.close()


def test_pipeline_certificate(gpu):
    from kmx import pipeline as PL
    from kmx.dpgo.params import PGOAgentParameters
    from kmx.lcd import LcdParams
    from kmx.synth import make_pose_graph
    g0 = make_pose_graph(3, 600, 2400, f_inter=0.0, outlier_scope="robot", seed=4)
    st = PL.make_lc_stream(g0, 24, 12, n_feats=200, seed=2)
    P = PGOAgentParameters(r=5)
    P.robustOptInnerIters = 10
    out = PL.run_pipeline(g0, st, P, LcdParams(), rounds=30, device=0, certify_eta=1e-5)
    cert = out["certificate"]
    print(cert, out["dpgo"]["cost"])
    assert cert["decision"] in ("CERTIFIED", "NEGATIVE", "UNDECIDED") and cert["steps"] >= 1
    # tr(X Q X^T) = 2 f. The solver has no team cost: out["dpgo"]["cost"] is its per-robot costs (kmx_pgo_eval)
    # summed, less the second count of the shared edges, and that second count is formed in numpy
    # (pipeline.solver_team_cost). So the device's cost kernel is the reference for the private edges and for
    # one count of the shared ones; the other count of the shared edges is numpy's.
    assert abs(cert["cost"] - 2.0 * out["dpgo"]["cost"]) <= 1e-9 * cert["cost"]
    assert out["lcd"]["accepted"] > 0  # the graph has inter-robot edges
    assert cert["stationarity"] > 0 and cert["theta_max"] > 0
    with pytest.raises(ValueError, match="certify_eta"):
        PL.run_pipeline(g0, st, P, LcdParams(), rounds=1, world=2, certify_eta=1e-5)
