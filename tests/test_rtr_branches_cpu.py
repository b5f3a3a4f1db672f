"""The RTR failure side on the CPU: what the inputs of rtr_cases.py do, and the
restatement's decisions against an independent reference.

1. Occurrences. Each input of tests/rtr_cases.py is there to send the block
   update down one branch (a rejected step, a negative-curvature stop, a
   radius that shrinks, grows or clamps, a later RTR iteration skipped on the
   gradient norm). The counts below were read from the restatement once and
   are asserted from its statistics, so a change of the graph generator or of
   the defaults cannot hollow out test_rtr_branches_gpu.py silently.

2. Reference. tests/rtr_ref.py states one RTR iteration from the mathematics
   (dense numpy). With one RTR iteration per block update the statistics
   expose the whole update, so each update of the inputs below is recomputed
   from the restatement's iterate before the round:
     C, C', and the first round of A at one RTR iteration (rejected steps:
     boundary and negative-curvature stops; A's first round at one iteration
     is C's, asserted to hold one of each);
     A at radius 1000, F and OK at one iteration, 8 / 4 / 6 rounds (accepted
     steps, so the trial point is visible as the new iterate: boundary,
     negative-curvature and residual stops, radius kept, doubled, clamped).
   Stop reason, tCG count, acceptance equal; radius exactly equal; and every
   decision of the reference at least 1e-6 of its scale away from going the
   other way (<d, Hd> against |d||Hd|, |eta + alpha d|_P^2 against radius^2,
   |r| against the residual stop, rho against 1/4, 3/4 and accept_rho).
   Measured restatement minus reference over these inputs: rho 1.3e-12
   relative to max(1, |rho|) (F, where rho = 1 - 4e-6 is a difference of
   costs of 4e5; 3.1e-15 on C, 4.2e-17 on C', 7.5e-15 on A), new iterate
   6.8e-14 Frobenius per pose (A at radius 1000; 2.1e-14 OK, 9.1e-16 F);
   ten times that is allowed: 1.3e-11 and 6.8e-13. A rejected step's trial
   point is not visible in the statistics; its rho (which holds f at the
   trial point) stands for it.
"""
import collections

import numpy as np
import pytest

from kmx.abi import KMX_EVAL_COST_EGRAD, KMX_EVAL_PRECON, KMX_EVAL_RGRAD, KMX_EVAL_RHESS
from tests import rtr_cases as rc
from tests.rtr_ref import Block, numpy_block, rtr_step

RHO_REF_TOL = 10 * 1.3e-12
X_REF_TOL = 10 * 6.8e-14
MARGIN = 1e-6


def _count(run, key):
    return dict(collections.Counter(s[key] for s in rc.all_stats(run)))


def _common(case):
    g, P, X0, rounds = rc.build(case)
    run = rc.oracle_rounds(case)
    assert len(run) == rounds and all(len(rec["st"]) == 3 for rec in run)
    st = rc.all_stats(run)
    assert all(s["updated"] == 1 for s in st)
    assert all(rc.rho_off_thresholds(s, P.localOptimizationParams.RTR_accept_rho) for s in st), case
    return g, P, X0, run, st


@pytest.mark.parametrize("case", ["A", "A1"])
def test_case_a_moves_then_rejects(case):
    """Three RTR iterations: in round 0 robots 0 and 2 move, then their last
    iteration is rejected; negative-curvature, boundary and residual stops;
    the radius shrinks (2500, 625), grows again (1250) and stays at its cap
    (1e4). The one-sync form gives the same pattern."""
    g, P, X0, run, st = _common(case)
    assert _count(run, "tcg_stop") == {"negative_curvature": 8, "exceeded_trust_region": 5, "linear": 5}
    assert _count(run, "radius") == {625.0: 2, 1250.0: 4, 2500.0: 8, 10000.0: 4}
    assert rc.moved_then(run, "rejected") == [(0, 0), (0, 2)]
    assert rc.moved_then(run, "skipped") == []
    assert sum(s["accepted"] for s in st) == 16
    assert 0.06 < min(s["rho"] for s in st) < 0.065  # below accept_rho 0.1: the rejections of round 0


def test_case_b_rejects_after_a_move_and_twice():
    g, P, X0, run, st = _common("B")
    assert _count(run, "tcg_stop") == {"negative_curvature": 12, "exceeded_trust_region": 8, "linear": 4}
    assert _count(run, "radius") == {5000.0: 2, 2500.0: 15, 625.0: 3, 10000.0: 4}
    assert rc.moved_then(run, "rejected") == [(5, 1)]
    twice = run[7]["st"][1]  # both iterations rejected: 1e4 / 16, nothing moved
    assert (twice["accepted"], twice["rel_change"], twice["radius"]) == (0, 0.0, 625.0)
    assert twice["f_final"] == twice["f_init"]
    assert -3.1 < min(s["rho"] for s in st) < -3.0
    assert sum(s["accepted"] for s in st) == 22


@pytest.mark.parametrize("case", ["C", "Cp"])
def test_case_c_rejects_everything(case):
    g, P, X0, run, st = _common(case)
    if case == "C":
        assert _count(run, "tcg_stop") == {"exceeded_trust_region": 16, "negative_curvature": 8}
        assert sorted({round(s["rho"], 3) for s in st}) == [-1.291, -0.749, -0.311]
    else:
        assert _count(run, "tcg_stop") == {"negative_curvature": 24}
        assert all(-0.02 < s["rho"] < -0.003 for s in st)
    assert _count(run, "radius") == {2500.0: 24}
    assert all(s["accepted"] == 0 and s["rel_change"] == 0.0 and s["f_final"] == s["f_init"] for s in st)
    for a in range(g.n_robots):  # the iterate never moves
        assert np.array_equal(run[-1]["X"][a], X0[a])


def test_case_d_rejects_under_gnc():
    g, P, X0, run, st = _common("D")
    assert _count(run, "tcg_stop") == {"negative_curvature": 8, "exceeded_trust_region": 5, "linear": 5}
    assert rc.moved_then(run, "rejected") == [(0, 0), (0, 1), (0, 2), (2, 2), (3, 1)]
    assert _count(run, "radius") == {1250.0: 5, 2500.0: 6, 625.0: 5, 10000.0: 2}
    assert -0.27 < min(s["rho"] for s in st) < -0.26


def test_case_e_skips_after_a_move_and_at_once():
    g, P, X0, run, st = _common("E")
    assert all(s["accepted"] == 1 and s["tcg_stop"] == "linear" for s in run[0]["st"])
    assert rc.moved_then(run, "skipped") == [(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (3, 1)]
    assert rc.moved_then(run, "rejected") == []
    for it, a in rc.moved_then(run, "skipped"):  # accepted at iteration 0: its rho and radius stand
        s = run[it]["st"][a]
        assert s["accepted"] == 0 and s["tcg_iterations"] == 0 and s["hessvecs"] > 0
        assert s["rho"] > 0.99 and s["radius"] in (100.0, 200.0)
    at_once = [(it, a) for it, rec in enumerate(run) for a, s in enumerate(rec["st"])
               if s["tcg_stop"] == "skipped" and s["rel_change"] == 0.0]
    assert at_once == [(2, 2), (3, 0), (3, 2)] + [(it, a) for it in (4, 5) for a in range(3)]
    for s in (run[it]["st"][a] for it, a in at_once):  # no step taken: the initial radius and rho 0 (kmx_abi.h)
        assert (s["hessvecs"], s["accepted"], s["rho"], s["radius"]) == (0, 0, 0.0, 100.0)
        assert s["f_final"] == s["f_init"]


def test_case_f_grows_and_clamps():
    g, P, X0, run, st = _common("F")
    assert _count(run, "tcg_stop") == {"exceeded_trust_region": 12}
    assert _count(run, "radius") == {1.5: 12}  # 0.5 -> 1 -> min(2, 1.5) -> 1.5 -> 1.5
    assert all(s["accepted"] == 1 and abs(s["rho"] - 1.0) < 1e-4 for s in st)


def test_control_accepts_everything():
    g, P, X0, run, st = _common("OK")
    assert all(s["accepted"] == 1 and s["tcg_stop"] != "skipped" for s in st)
    assert rc.moved_then(run, "rejected") == rc.moved_then(run, "skipped") == []


@pytest.mark.parametrize("case", rc.ALL)
def test_all_cores_variant_takes_the_same_decisions(case):
    """The restatement against itself with its sums grouped differently: the
    same decisions and radii; the largest relative difference in rho (printed)
    is the s of test_rtr_branches_gpu.py's rho tolerance."""
    a_, b_ = rc.oracle_rounds(case), rc.oracle_rounds(case, threads=2, inner=2)
    s = 0.0
    for ra, rb in zip(a_, b_):
        for x, y in zip(ra["st"], rb["st"]):
            for k in ("tcg_iterations", "tcg_stop", "accepted", "hessvecs", "radius"):
                assert x[k] == y[k], (case, k, x, y)
            s = max(s, abs(x["rho"] - y["rho"]) / max(1.0, abs(x["rho"])))
    print(f"{case}: s = {s:.3g}")
    assert s <= 1e-9, s


# ------------------------------------------------------------- reference ---
def _ref_step(g, P, X, a):
    lo = P.localOptimizationParams
    return rtr_step(g, X, a, radius=lo.RTR_initial_radius, max_radius=lo.RTR_max_radius,
                    accept_rho=lo.RTR_accept_rho, tcg_max=lo.RTR_tCG_iterations, kappa=lo.tCG_kappa,
                    theta=lo.tCG_theta, shift=lo.precond_shift, use_preconditioner=lo.use_preconditioner)


REF_INPUTS = {
    # id: (case, overrides, rounds, (stop, accepted, radius) triples that must occur)
    "C": ("C", {}, 1, [("exceeded_trust_region", 0, 2500.0), ("negative_curvature", 0, 2500.0)]),
    "Cp": ("Cp", {}, 1, [("negative_curvature", 0, 2500.0)]),
    "A_round0": ("A", {"RTR_iterations": 1}, 1, [("exceeded_trust_region", 0, 2500.0), ("negative_curvature", 0, 2500.0)]),
    "A_radius1000": ("A", {"RTR_iterations": 1, "RTR_initial_radius": 1000.0}, 8,
                     [("exceeded_trust_region", 1, 2000.0), ("exceeded_trust_region", 1, 1000.0),
                      ("negative_curvature", 1, 2000.0), ("negative_curvature", 1, 1000.0)]),
    "F": ("F", {"RTR_iterations": 1}, 4, [("exceeded_trust_region", 1, 1.0)]),
    "OK": ("OK", {"RTR_iterations": 1}, 6, [("exceeded_trust_region", 1, 200.0), ("linear", 1, 100.0)]),
}


@pytest.mark.parametrize("name", list(REF_INPUTS))
def test_restatement_follows_reference(name):
    case, over, rounds, expect = REF_INPUTS[name]
    g, P, X0, _ = rc.build(case, **over)
    o = rc.oracle(g, P, X0)
    seen, worst_rho, worst_x = set(), 0.0, 0.0
    for it in range(rounds):
        X = {a: o.get_iterate(a) for a in range(g.n_robots)}
        o.refresh()
        st = o.iterate()
        for a in range(g.n_robots):
            ref, s = _ref_step(g, P, X, a), st[a]
            where = (name, it, a, s, {k: v for k, v in ref.items() if k not in ("Xt", "X")})
            m = ref["margins"]
            assert min(m["curvature"]) >= MARGIN, where
            assert min(m["boundary"], default=1.0) >= MARGIN, where
            assert min(m["residual"], default=1.0) >= MARGIN, where
            assert m["rho"] >= MARGIN and m["model_decrease"] >= MARGIN, where
            for k in ("tcg_stop", "tcg_iterations", "accepted"):
                assert s[k] == ref[k], (k,) + where
            assert s["radius"] == ref["radius"], where
            assert abs(s["f_init"] - ref["f_init"]) <= 1e-12 * abs(ref["f_init"]), where
            assert abs(s["gradnorm_init"] - ref["gradnorm_init"]) <= 1e-12 * ref["gradnorm_init"], where
            d_rho = abs(s["rho"] - ref["rho"]) / max(1.0, abs(ref["rho"]))
            Xo = o.get_iterate(a)
            d_x = np.linalg.norm((Xo - ref["X"]).reshape(len(Xo), -1), axis=1).max()
            worst_rho, worst_x = max(worst_rho, d_rho), max(worst_x, d_x)
            assert d_rho <= RHO_REF_TOL, (d_rho,) + where
            assert d_x <= X_REF_TOL, (d_x,) + where
            if ref["accepted"]:
                assert abs(s["f_final"] - ref["f_trial"]) <= 1e-12 * abs(ref["f_trial"]), where
            else:
                assert np.array_equal(Xo, X[a]), where
            seen.add((s["tcg_stop"], s["accepted"], s["radius"]))
    print(f"{name}: restatement - reference: rho {worst_rho:.3g}, iterate {worst_x:.3g}")
    assert set(expect) <= seen, (name, seen)


def test_reference_primitives_against_restatement():
    """The reference's dense pieces against numpy_block and the restatement's
    primitives at A's start: Euclidean and Riemannian gradient, Hessian,
    preconditioner; the Hessian is symmetric on tangent vectors."""
    g, P, X0, _ = rc.build("A")
    o = rc.oracle(g, P, X0)
    rng = np.random.default_rng(5)
    for a in range(g.n_robots):
        B = Block(g, X0, a, shift=P.localOptimizationParams.precond_shift)
        f, Gn = numpy_block(g, X0, a)
        G = B.egrad(X0[a])
        assert np.abs(G - Gn).max() <= 1e-12 * np.abs(Gn).max()
        M = X0[a].transpose(1, 0, 2).reshape(P.r, -1)
        assert abs(0.5 * np.sum((M @ B.Q) * M) + np.sum(M * B.B) + B.c - f) <= 1e-12 * f
        eg, fo = o.eval(a, KMX_EVAL_COST_EGRAD, X0[a])
        assert abs(fo - f) <= 1e-12 * f and np.abs(eg - G).max() <= 1e-12 * np.abs(G).max()
        rg, _ = o.eval(a, KMX_EVAL_RGRAD)
        assert np.abs(rg - B.proj(X0[a], G)).max() <= 1e-12 * np.abs(G).max()
        U, V = (B.proj(X0[a], rng.standard_normal(X0[a].shape)) for _ in range(2))
        HU, HV = B.rhess(X0[a], G, U), B.rhess(X0[a], G, V)
        assert abs(np.sum(U * HV) - np.sum(V * HU)) <= 1e-10 * abs(np.sum(U * HV))
        Ho, _ = o.eval(a, KMX_EVAL_RHESS, U)
        assert np.abs(Ho - HU).max() <= 1e-12 * np.abs(HU).max()
        Po, _ = o.eval(a, KMX_EVAL_PRECON, U)
        assert np.abs(Po - B.precon(X0[a], U)).max() <= 1e-12 * np.abs(Po).max()
