"""The certificate's decisions held to what they claim: the smallest
eigenvalue of the dense S (numpy.linalg.eigvalsh), on points where it sits near
-eta. The numpy restatement of the scan (tests/cert_ref.py) runs over all of
family F, 1350 Lanczos runs on almost stationary points of noise-free graphs,
and every decision must be true: NEGATIVE only with lambda_min < -eta,
CERTIFIED only with lambda_min >= -eta. The same coefficients go through
kmx_cert_ritz (the host's C++ rule) at the same test steps, and its decisions
must be the restatement's. No device is needed.

With rho <= eta as the residual condition 20 of the 668 certificates on F
were false (lambda_min / eta from -1.02 to -2.74: Lanczos had converged onto
the kernel of S, the rows of X, before it resolved the negative eigenvalue
below it). CERT_C = 1/10 is the largest of 1, 1/2, 1/4, 1/10, 1/100 that leaves
none (scripts/cert_rule_table.py prints the table)."""
import numpy as np
import pytest

from tests import cert_ref as CR

EPS = np.finfo(float).eps
_cache = {}


def _host_decision(al, be, k, eta):
    from kmx.dpgo.certify import ritz
    return ritz(al[:k], be[:k], eta)


def _runs(graph):
    """Every run of F on one graph: (point, seed, the scan's result, its tests)."""
    if graph not in _cache:
        out = []
        for pt in CR.family_points(graphs=(graph,)):
            for seed in CR.F_SEEDS:
                tests = []
                res = CR.scan(pt["S"], pt["eta"], seed, pt["max_steps"], CR.F_TEST_EVERY, tests=tests)
                out.append((pt, seed, res, tests))
        _cache[graph] = out
    return _cache[graph]


def check_sound(decision, ev, eta, where):
    """The two implications, and that rounding of the dense solver cannot
    decide: lambda_min is at least 1e-9 lambda_max away from -eta."""
    assert abs(ev[0] + eta) >= 1e-9 * ev[-1], where
    if decision == "NEGATIVE":
        assert ev[0] < -eta, (where, "false NEGATIVE", ev[0] / eta)
    if decision == "CERTIFIED":
        assert ev[0] >= -eta, (where, "false CERTIFIED", ev[0] / eta)


@pytest.mark.parametrize("graph", CR.F_GRAPHS, ids=lambda g: "n%d_m%d_r%d" % g)
def test_every_decision_on_family_F_is_true(graph):
    runs = _runs(graph)
    assert len(runs) == len(CR.F_DSEEDS) * len(CR.F_DELTAS) * len(CR.F_SEEDS) == 270
    false, count = [], {"CERTIFIED": 0, "NEGATIVE": 0, "UNDECIDED": 0}
    for pt, seed, res, tests in runs:
        ev, eta = pt["ev"], pt["eta"]
        where = (graph, pt["dseed"], pt["delta"], seed)
        assert abs(ev[0] + eta) >= 1e-9 * ev[-1], where
        count[res["decision"]] += 1
        if res["decision"] == "CERTIFIED" and ev[0] < -eta:
            false.append(where + (ev[0] / eta, res["residual"] / eta, res["steps"]))
        # the host's rule on the same coefficients at the same steps
        assert [t["steps"] for t in tests][-1] == res["steps"] == len(res["alpha"])
        for t in tests:
            got = _host_decision(res["alpha"], res["beta"], t["steps"], eta)
            want = t["decision"] if t["decides"] else CR.rule(t["theta_min"], t["residual"], eta)
            assert got["decision"] == want, (where, t["steps"], got, t["theta_min"], t["residual"])
            assert abs(got["theta_min"] - t["theta_min"]) <= 1e-12 * ev[-1], (where, t["steps"])
        assert all(t["decision"] == "UNDECIDED" for t in tests[:-1]), where
    print(graph, count, "false certificates (graph, dseed, delta, seed, lambda_min/eta, rho/eta, steps):", false)
    assert not false
    for pt, seed, res, _ in runs:
        check_sound(res["decision"], pt["ev"], pt["eta"], (graph, pt["dseed"], pt["delta"], seed))
    # the family decides: nothing is left UNDECIDED at 40 n + 200 steps, and both answers occur
    assert count["UNDECIDED"] == 0 and count["CERTIFIED"] > 0 and count["NEGATIVE"] > 0
    # an exactly stationary point and one moved by 1e-7 are certified from every start
    assert all(res["decision"] == "CERTIFIED" for pt, _, res, _ in runs if pt["delta"] <= 1e-7)


def test_the_yardsticks_of_the_device_tests():
    """Over all 1350 runs: how far Ritz values leave the spectrum, and how far
    the Ritz vector's true residual exceeds rho. tests/test_cert_sound_gpu.py
    allows the device ten times the figures recorded in cert_ref."""
    below = above = ratio = ratio_all = 0.0
    n_runs = certified = 0
    for graph in CR.F_GRAPHS:
        for pt, seed, res, tests in _runs(graph):
            lmax = pt["ev"][-1]
            n_runs += 1
            certified += res["decision"] == "CERTIFIED"
            for t in tests:
                below = max(below, (pt["ev"][0] - t["theta_min"]) / lmax)
                above = max(above, (t["theta_max"] - lmax) / lmax)
                ratio_all = max(ratio_all, (t["true_residual"] - t["residual"]) / (t["steps"] * EPS * lmax))
            ratio = max(ratio, (res["true_residual"] - res["residual"]) / (res["steps"] * EPS * lmax))
            assert abs(np.linalg.norm(res["y"]) - 1.0) <= 1e-12
    print(f"runs {n_runs}, certified {certified}; (lambda_min - theta_min) / lambda_max <= {below:.3e}; "
          f"(theta_max - lambda_max) / lambda_max <= {above:.3e}; (|S y - theta y| - rho) / (k eps lambda_max) <= "
          f"{ratio:.3e} at the returned step, {ratio_all:.3e} over every test")
    assert n_runs == 1350
    assert below <= CR.F_RITZ_BELOW and above <= CR.F_RITZ_ABOVE and ratio <= CR.F_RESIDUAL_RATIO


def test_the_residual_factor_is_needed():
    """The finding behind CERT_C: with rho <= eta the same runs hold false
    certificates (20 when this was written; 7 at 1/2, 1 at 1/4, which rests on a
    single run and is printed, not asserted), with CERT_C none. The runs of a
    larger factor are the runs of CERT_C cut short, so they are read from its
    tests."""
    assert CR.CERT_C in CR.CERT_C_CANDIDATES
    false = {c: 0 for c in CR.CERT_C_CANDIDATES if c >= CR.CERT_C}
    for graph in CR.F_GRAPHS:
        for pt, seed, res, tests in _runs(graph):
            for c in false:
                d, _ = CR.first_decision(tests, pt["eta"], c)
                false[c] += d == "CERTIFIED" and pt["ev"][0] < -pt["eta"]
    print("false certificates per factor:", false)
    assert false[CR.CERT_C] == 0 and false[1.0] >= 10


@pytest.mark.parametrize("graph", CR.SMALL_GRAPHS, ids=lambda g: "n%d_m%d_r%d" % g)
def test_past_the_dimension_the_restatement_stays_sound(graph):
    """Graphs of 2 to 5 poses (dimension 8 to 20) decide at 20 to 30 steps:
    beta has dipped to 1e-7 or 1e-8 of |T| and the iteration has restarted from
    rounding noise. The decisions must still be true, for the restatement and
    for the host's rule on its coefficients."""
    n, m, r = graph
    g, X0 = CR.consistent_graph(n, m, r, 6)
    for delta in CR.SMALL_DELTAS:
        X = CR.perturbed_point(X0, delta, 1)
        _, S = CR.dense_of(g, X)
        ev = np.linalg.eigvalsh(S)
        eta = 1e-6 * ev[-1]
        for every in CR.SMALL_TEST_EVERY:
            tests = []
            res = CR.scan(S, eta, 1, CR.SMALL_MAX_STEPS, every, tests=tests)
            where = (graph, delta, every, res["decision"], res["steps"])
            check_sound(res["decision"], ev, eta, where)
            assert res["theta_min"] >= ev[0] - 10 * CR.F_RITZ_BELOW * ev[-1], where
            assert res["theta_max"] <= ev[-1] + 10 * CR.F_RITZ_ABOVE * ev[-1], where
            for t in tests:
                got = _host_decision(res["alpha"], res["beta"], t["steps"], eta)
                want = t["decision"] if t["decides"] else CR.rule(t["theta_min"], t["residual"], eta)
                assert got["decision"] == want, (where, t["steps"], got, t)


@pytest.mark.parametrize("n,r", CR.RINGS)
def test_graded_ring_in_the_restatement(n, r):
    """eta on either side of the ring's known |lambda_min|."""
    g, X = CR.ring(n, r)
    _, S = CR.dense_of(g, X)
    lam = CR.ring_lambda_min(n)
    for ratio in CR.RING_ETA_RATIOS:
        res = CR.scan(S, ratio * abs(lam), 1, 40 * n + 200, 10)
        assert res["decision"] == ("NEGATIVE" if ratio < 1 else "CERTIFIED"), (ratio, res["decision"], res["steps"])
        assert res["theta_min"] >= lam - 10 * CR.F_RITZ_BELOW * 4.0
