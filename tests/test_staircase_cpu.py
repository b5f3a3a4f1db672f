"""The Riemannian staircase (kmx.dpgo.staircase, kmx_cert_escape), the part that
needs no device: the argument checks, split_team as flatten_team's inverse,
rounding_lift, the pipeline's refusals, and the loop itself on the CPU
restatement of the solver with a dense numpy certifier (tests/stair_ref.py)."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

from tests import cert_ref as CR
from tests import stair_ref as SR

ROOT = Path(__file__).resolve().parents[1]


def test_symbols_declared_exported_and_bound():
    from kmx import abi
    L = abi.lib()
    hdr = (ROOT / "include" / "kmx_abi.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(kmx_\w+)\s*\(", hdr, re.M))
    for name in ("kmx_cert_escape", "kmx_cert_escape_commit", "kmx_cert_get_escape_timing"):
        assert name in declared, name
        assert getattr(L, name).argtypes is not None, name
    assert abi.ABI_VERSION == 10 and L.kmx_abi_version() == 10  # additive


def test_check_escape_refusals():
    from kmx.dpgo.certify import Certifier
    n = 6
    y = np.linspace(-1.0, 1.0, 4 * n)
    yy, aa = Certifier.check_escape(n, 3, y, [1.0, 0.5])
    assert yy.shape == (4 * n,) and yy.dtype == np.float64 and aa.tolist() == [1.0, 0.5]
    assert Certifier.check_escape(n, 7, y.reshape(n, 4), np.ones(8))[0].shape == (4 * n,)
    bad_y = y.copy()
    bad_y[5] = np.nan
    for r, yv, al, what in ((8, y, [1.0], "rank"), (0, y, [1.0], "rank"), (3, y[:-1], [1.0], "y"),
                            (3, bad_y, [1.0], "y"), (3, y, [], "alphas"), (3, y, np.ones(9), "alphas"),
                            (3, y, [1.0, np.inf], "alphas"), (3, y, [[1.0]], "alphas"), (3, y, ["a"], "alphas"),
                            (3, y, 1.0, "alphas")):
        with pytest.raises(ValueError, match=what):
            Certifier.check_escape(n, r, yv, al)


def test_split_team_inverts_flatten_team():
    from kmx.dpgo.certify import flatten_team, split_team
    from kmx.synth import make_pose_graph
    g = make_pose_graph(3, 60, 90, seed=2)
    g.n_poses = np.array([13, 30, 17], np.int32)  # unequal sizes; only n_poses is read
    rng = np.random.default_rng(0)
    Xs = {a: rng.standard_normal((int(g.n_poses[a]), 5, 4)) for a in range(3)}
    X = np.concatenate([Xs[a] for a in range(3)])
    back = split_team(g, X)
    assert sorted(back) == [0, 1, 2]
    for a in range(3):
        assert np.array_equal(back[a], Xs[a]) and back[a].flags.c_contiguous
    g.r1, g.p1, g.r2, g.p2 = (np.zeros(0, np.int32),) * 4
    assert np.array_equal(flatten_team(g, back)[3], X)
    with pytest.raises(ValueError, match="X"):
        split_team(g, X[:-1])


def _exact_lift(r, seed, n=40):
    from kmx.synth import lift, lifting_matrix
    rng = np.random.default_rng(seed)
    R, t = CR.random_rotations(rng, n), rng.standard_normal((n, 3))
    Y0 = lifting_matrix(r, seed=seed)
    return R, t, Y0, lift(R, t, Y0)


@pytest.mark.parametrize("r", [5, 7])
def test_rounding_lift_reproduces_the_relative_trajectory_of_an_exact_lift(r):
    from kmx.dpgo.certify import rounding_lift
    from kmx.pipeline import rounded
    R, t, Y0, X = _exact_lift(r, 3 + r)
    Y = rounding_lift(X)
    assert Y.shape == (r, 3) and np.abs(Y.T @ Y - np.eye(3)).max() <= 1e-14
    Ra, ta = rounded(X, Y0)
    Rb, tb = rounded(X, Y)
    assert np.abs(Ra - R).max() <= 1e-12  # the reference rounds to the trajectory that was lifted
    rel = lambda Rs, ts: (np.einsum("ji,njk->nik", Rs[0], Rs), (ts - ts[0]) @ Rs[0])  # noqa: E731
    (Ra_rel, ta_rel), (Rb_rel, tb_rel) = rel(Ra, ta), rel(Rb, tb)
    print("rotation", np.abs(Ra_rel - Rb_rel).max(), "translation", np.abs(ta_rel - tb_rel).max())
    assert np.abs(Ra_rel - Rb_rel).max() <= 1e-12
    assert np.abs(ta_rel - tb_rel).max() <= 1e-12 * max(1.0, np.abs(ta_rel).max())
    assert (np.linalg.det(np.einsum("ad,nac->ndc", Y, X[:, :, :3])) > 0).all()


def test_rounding_lift_ignores_a_zero_row():
    from kmx.dpgo.certify import rounding_lift
    from kmx.pipeline import rounded
    _, _, _, X = _exact_lift(5, 11)
    Xz = np.concatenate([X, np.zeros((X.shape[0], 1, 4))], axis=1)
    Y, Yz = rounding_lift(X), rounding_lift(Xz)
    assert Yz.shape == (6, 3) and np.abs(Yz[5]).max() <= 1e-15
    Ra, ta = rounded(X, Y)
    Rb, tb = rounded(Xz, Yz)
    # the eigenvectors are fixed up to a rotation of the three-dimensional span: compare relative poses
    assert np.abs(np.einsum("ji,njk->nik", Ra[0], Ra) - np.einsum("ji,njk->nik", Rb[0], Rb)).max() <= 1e-12
    assert np.abs((ta - ta[0]) @ Ra[0] - (tb - tb[0]) @ Rb[0]).max() <= 1e-12 * max(1.0, np.abs(ta).max())
    with pytest.raises(ValueError, match="X"):
        rounding_lift(np.zeros((4, 2, 4)))


def test_pipeline_refuses_a_staircase_without_certificate_or_on_two_ranks():
    from kmx import pipeline as PL
    from kmx.dpgo import staircase as ST
    sig = inspect.signature(PL.run_pipeline)
    assert sig.parameters["staircase_rmax"].default is None and sig.parameters["certify_eta"].default is None
    assert inspect.signature(ST.staircase_team).parameters["alphas"].default is None
    assert ST.DEFAULT_ALPHAS == tuple(2.0 ** -k for k in range(8))
    with pytest.raises(ValueError, match="staircase_rmax"):
        PL.run_pipeline(None, None, None, None, staircase_rmax=6)
    with pytest.raises(ValueError, match="staircase_rmax"):
        PL.run_pipeline(None, None, None, None, world=2, staircase_rmax=6)
    with pytest.raises(ValueError, match="certify_eta"):  # as before
        PL.run_pipeline(None, None, None, None, world=2, certify_eta=1e-5, staircase_rmax=6)


def test_staircase_refuses_bad_arguments_before_any_device_call():
    from kmx.dpgo.staircase import staircase_team
    g, Xs, _ = SR.ring_team(8)
    kw = dict(eta=1e-5, grad_tol=1e-7, stat_tol=1e-6, max_rounds=10, certifier=SR.NumpyCertifier(),
              solver_factory=SR.oracle_solver)
    for r_max in (2, 9, 3.5, True):
        with pytest.raises(ValueError, match="r_max"):
            staircase_team(g, Xs, None, None, r_max=r_max, **kw)
    with pytest.raises(ValueError, match="alphas"):
        staircase_team(g, Xs, None, None, r_max=5, alphas=np.ones(9), **kw)
    with pytest.raises(ValueError, match="weight"):
        staircase_team(g, Xs, -np.ones(8), None, r_max=5, **kw)


@pytest.mark.parametrize("n,robots", [(8, 1), (24, 3)])
def test_staircase_loop_on_the_cpu_restatement_climbs_the_ring(n, robots):
    """The loop's control flow without a device: the CPU restatement of the
    solver and a dense certifier (eigh, escape_point). The winding ring escapes
    twice (St(3,3) and St(3,4) are not simply connected, St(3,5) is)."""
    from kmx import pipeline as PL
    from kmx.dpgo.params import PGOAgentParameters
    from kmx.dpgo.staircase import staircase_team
    g, Xs, gd = SR.ring_team(n, robots)
    P = PGOAgentParameters(r=3)
    P.localOptimizationParams.RTR_iterations = 8  # rejected steps quarter the radius from 100 in every update
    P.localOptimizationParams.RTR_tCG_iterations = 50
    kw = dict(eta=1e-5, grad_tol=1e-7, stat_tol=1e-6, max_rounds=400, solver_factory=SR.oracle_solver)
    out = staircase_team(g, Xs, None, P, r_max=6, certifier=SR.NumpyCertifier(), **kw)
    lv = out["levels"]
    print(out["status"], [(q["r"], q["decision"], q["rounds"], q["cost"], q["alpha"]) for q in lv])
    assert out["status"] == "CERTIFIED" and out["r"] == 5
    assert [q["r"] for q in lv] == [3, 4, 5] and [q["decision"] for q in lv] == ["NEGATIVE", "NEGATIVE", "CERTIFIED"]
    assert lv[0]["block_steps"] == 0 and lv[0]["alpha"] == 1.0 and lv[2]["alpha"] is None
    f3 = SR.f3(n)
    assert abs(lv[1]["cost"] - f3 / 2) <= 1e-6 * f3 / 2 and lv[2]["cost"] <= 1e-9 * f3
    X = np.concatenate([out["X"][a] for a in range(robots)])
    assert X.shape == (n, 5, 4) and out["lift"].shape == (5, 3)
    R, _ = PL.rounded(X, out["lift"])
    assert np.abs(SR.relative_rotations(R, gd["src"], gd["dst"]) - np.eye(3)).max() <= 1e-6
    # the stop conditions that need no second solve
    lim = staircase_team(g, Xs, None, P, r_max=4, certifier=SR.NumpyCertifier(), **kw)
    assert lim["status"] == "RANK_LIMIT" and lim["r"] == 4 and lim["levels"][-1]["decision"] == "NEGATIVE"
    flat = staircase_team(g, Xs, None, P, r_max=6, alphas=[0.0], certifier=SR.NumpyCertifier(), **kw)
    assert flat["status"] == "NO_DESCENT" and flat["r"] == 3 and flat["levels"][0]["best"] == -1
