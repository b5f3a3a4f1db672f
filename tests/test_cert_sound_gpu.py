"""kmx_cert_min_eig's decisions on the device held to what they claim, the
smallest eigenvalue of the dense S from tests/cert_ref.py (never the device):
a subset of family F (almost stationary points with lambda_min near -eta), the
Ritz vector's true residual, runs past the dimension on graphs of 2 to 5
poses, an exact breakdown (S = 0) and the NaNs it leaves behind in the batch,
the winding ring with eta graded around |lambda_min|, and the scaling of the
whole computation by a power of two. The slacks are ten times what the numpy
restatement needed over all of F (cert_ref.F_*; tests/test_cert_sound_cpu.py)."""
import numpy as np
import pytest

from tests import cert_ref as CR

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
GRAPHS = ((5, 3, 5), (17, 20, 5), (65, 80, 5), (130, 150, 8))
_ids = lambda g: "n%d_m%d_r%d" % g  # noqa: E731
_points = {}


def points(graph):
    """F's points of one graph at dseed 1 (all 15 delta), computed once."""
    if graph not in _points:
        _points[graph] = list(CR.family_points(graphs=(graph,), dseeds=(1,)))
    return _points[graph]


def certifier(g, X=None):
    from kmx.dpgo.certify import Certifier
    c = Certifier()
    c.set_graph(**g)
    if X is not None:
        c.set_point(X)
    return c


def check_sound(res, ev, eta, where):
    """The two implications, lambda_min at least 1e-9 lambda_max from -eta,
    and the Ritz values inside the spectrum to the slack."""
    lmin, lmax, k = ev[0], ev[-1], res["steps"]
    report = (where, res["decision"], "lambda_min/eta", lmin / eta, "rho/eta", res["residual"] / eta, "steps", k)
    assert abs(lmin + eta) >= 1e-9 * lmax, report
    if res["decision"] == "NEGATIVE":
        assert lmin < -eta, report
    if res["decision"] == "CERTIFIED":
        assert lmin >= -eta, report
    # every returned number is finite (theta_max is left out only at tests that return nothing)
    assert np.isfinite([res["theta_min"], res["theta_max"], res["residual"]]).all() and res["residual"] >= 0, report
    assert res["theta_min"] >= lmin - max(10 * CR.F_RITZ_BELOW, k * EPS) * lmax, report
    assert res["theta_max"] <= lmax + max(10 * CR.F_RITZ_ABOVE, k * EPS) * lmax, report
    return ((lmin - res["theta_min"]) / lmax, (res["theta_max"] - lmax) / lmax)


@pytest.mark.parametrize("graph", GRAPHS, ids=_ids)
def test_decisions_on_family_F_are_true(gpu, graph):
    pts = points(graph)
    assert len(pts) == 15
    c = certifier(pts[0]["g"])
    worst = np.array([-np.inf, -np.inf])
    count = {"CERTIFIED": 0, "NEGATIVE": 0, "UNDECIDED": 0}
    for pt in pts:
        ev, eta = pt["ev"], pt["eta"]
        c.set_point(pt["X"])
        for seed in (1, 2):
            res = c.min_eig(eta, max_steps=pt["max_steps"], test_every=CR.F_TEST_EVERY, seed=seed)
            where = (graph, pt["delta"], seed)
            worst = np.maximum(worst, check_sound(res, ev, eta, where))
            count[res["decision"]] += 1
            if pt["delta"] <= 1e-7:
                assert res["decision"] == "CERTIFIED", (where, res)
            if ev[0] < -10 * eta:
                assert res["decision"] == "NEGATIVE", (where, res, ev[0] / eta)
    c.close()
    print(graph, count, "Ritz values outside the spectrum / lambda_max: below", worst[0], "above", worst[1])
    assert count["CERTIFIED"] > 0 and count["NEGATIVE"] > 0


@pytest.mark.parametrize("graph", GRAPHS, ids=_ids)
def test_ritz_vector_has_the_residual_it_reports(gpu, graph):
    pts = points(graph)
    c = certifier(pts[0]["g"])
    C = max(10 * CR.F_RESIDUAL_RATIO, 1.0)
    worst = [-np.inf, -np.inf]
    for pt in pts:
        ev, eta, S = pt["ev"], pt["eta"], pt["S"]
        c.set_point(pt["X"])
        res = c.min_eig(eta, max_steps=pt["max_steps"], test_every=CR.F_TEST_EVERY, seed=1, want_vector=True)
        y, th, rho, k = res["y"], res["theta_min"], res["residual"], res["steps"]
        unit = k * EPS * ev[-1]
        where = (graph, pt["delta"], res["decision"], k)
        assert np.isfinite(y).all() and abs(np.linalg.norm(y) - 1.0) <= 1e-12, where
        rq = abs(y @ S @ y - th)
        tr = np.linalg.norm(S @ y - th * y)
        worst = [max(worst[0], (rq - rho) / unit), max(worst[1], (tr - rho) / unit)]
        assert rq <= rho + C * unit, (where, rq, rho, (rq - rho) / unit)
        assert tr <= rho + C * unit, (where, tr, rho, (tr - rho) / unit)
    c.close()
    print(graph, "in units of steps eps lambda_max (allowed", C, "): |y'Sy - theta| - rho <=", worst[0],
          "|Sy - theta y| - rho <=", worst[1])


@pytest.mark.parametrize("graph", CR.SMALL_GRAPHS, ids=_ids)
def test_past_the_dimension(gpu, graph):
    """Dimension 8 to 20 and up to 200 steps: beta dips towards the breakdown
    level and the iteration restarts from rounding noise."""
    n, m, r = graph
    g, X0 = CR.consistent_graph(n, m, r, 6)
    c = certifier(g)
    seen = []
    for delta in CR.SMALL_DELTAS:
        X = CR.perturbed_point(X0, delta, 1)
        _, S = CR.dense_of(g, X)
        ev = np.linalg.eigvalsh(S)
        eta = 1e-6 * ev[-1]
        c.set_point(X)
        for every in CR.SMALL_TEST_EVERY:
            res = c.min_eig(eta, max_steps=CR.SMALL_MAX_STEPS, test_every=every, seed=1)
            where = (graph, delta, every)
            check_sound(res, ev, eta, where)
            assert 1 <= res["steps"] <= CR.SMALL_MAX_STEPS, where
            al, be = c.coefficients()
            assert al.shape == be.shape == (res["steps"],), (where, al.shape, res["steps"])
            assert np.isfinite(al).all() and np.isfinite(be).all() and (be >= 0).all(), where
            seen.append((delta, every, res["decision"], res["steps"], float(be.min() / ev[-1])))
    c.close()
    print(graph, "(delta, test_every, decision, steps, min beta / lambda_max):", seen)
    assert any(s[3] > 4 * n for s in seen)  # some run did go past the dimension


def _same(a, b, what):
    for k in ("decision", "steps", "theta_min", "theta_max", "residual"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    if "y" in a:
        assert np.array_equal(a["y"], b["y"]), what


@pytest.mark.parametrize("check_every", [1, 50])
@pytest.mark.parametrize("want_vector", [False, True])
def test_exact_breakdown_of_one_pose(gpu, want_vector, check_every):
    """S = 0: beta_1 = 0 and the rest of the batch divides by it. The host stops
    at step 1 and the NaNs stay behind."""
    g = CR.random_graph(1, 0, 1)
    c = certifier(g, CR.random_point(1, 3, 2))
    first = c.min_eig(1e-6, check_every=check_every, seed=3, want_vector=want_vector)
    assert first["decision"] == "CERTIFIED" and first["steps"] == 1, first
    assert first["theta_min"] == 0.0 and first["theta_max"] == 0.0 and first["residual"] == 0.0, first
    al, be = c.coefficients()
    assert al.tolist() == [0.0] and be.tolist() == [0.0]
    if want_vector:
        y = first["y"]
        assert np.isfinite(y).all() and abs(np.linalg.norm(y) - 1.0) <= 1e-12
    _same(c.min_eig(1e-6, check_every=check_every, seed=3, want_vector=want_vector), first, "second call")
    c.close()


@pytest.mark.parametrize("check_every", [1, 50])
@pytest.mark.parametrize("want_vector", [False, True])
def test_exact_breakdown_of_zero_weights_leaves_no_nan_behind(gpu, want_vector, check_every):
    g = CR.random_graph(10, 5, 1)
    X = CR.random_point(10, 4, 2)
    m = g["weight"].shape[0]
    c = certifier(g, X)
    c.set_weights(np.zeros(m))
    res = c.min_eig(1e-6, check_every=check_every, seed=3, want_vector=want_vector)
    assert res["decision"] == "CERTIFIED" and res["steps"] == 1, res
    assert res["theta_min"] == 0.0 and res["theta_max"] == 0.0 and res["residual"] == 0.0, res
    if want_vector:
        y = res["y"]
        assert np.isfinite(y).all() and abs(np.linalg.norm(y) - 1.0) <= 1e-12
    # the graph's weights again: the handle that broke down against a fresh one, bit for bit
    _, S = CR.dense_of(g, X)
    ev = np.linalg.eigvalsh(S)
    eta = 1e-6 * ev[-1]
    kw = dict(max_steps=120, test_every=10, check_every=check_every, seed=3, want_vector=True)
    c.set_weights(g["weight"])
    again = c.min_eig(eta, **kw)
    coef = c.coefficients()
    fresh = certifier(g, X)
    want = fresh.min_eig(eta, **kw)
    coef_want = fresh.coefficients()
    _same(again, want, "after the breakdown")
    assert np.array_equal(coef[0], coef_want[0]) and np.array_equal(coef[1], coef_want[1])
    assert np.isfinite(again["y"]).all() and np.isfinite(coef[0]).all() and np.isfinite(coef[1]).all()
    check_sound(again, ev, eta, "after the breakdown")
    v = np.random.default_rng(4).standard_normal(40)
    assert np.array_equal(c.apply(v), fresh.apply(v))
    c.close()
    fresh.close()


@pytest.mark.parametrize("n,r", CR.RINGS)
def test_graded_ring(gpu, n, r):
    """eta on either side of the known |lambda_min| = 2 - 2 cos(2 pi / n). At
    n = 8 the Krylov space is exhausted at step 8 and beta may or may not fall
    under the breakdown level: either path must decide the same."""
    g, X = CR.ring(n, r)
    _, S = CR.dense_of(g, X)
    ev = np.linalg.eigvalsh(S)
    lam = CR.ring_lambda_min(n)
    assert abs(ev[0] - lam) < 1e-12
    c = certifier(g, X)
    seen = []
    for ratio in CR.RING_ETA_RATIOS:
        eta = ratio * abs(lam)
        for seed in (1, 2):
            res = c.min_eig(eta, max_steps=40 * n + 200, test_every=10, seed=seed)
            where = (n, r, ratio, seed)
            check_sound(res, ev, eta, where)
            assert res["decision"] == ("NEGATIVE" if eta < abs(lam) else "CERTIFIED"), (where, res)
            seen.append((ratio, seed, res["decision"], res["steps"], res["residual"] / eta))
    c.close()
    print((n, r), "(eta/|lambda_min|, seed, decision, steps, rho/eta):", seen)


@pytest.mark.parametrize("exponent", [20, -20])
def test_scaling_by_a_power_of_two_is_exact(gpu, exponent):
    """kappa, tau and eta times 2^e: every operation from the records to the
    coefficients is homogeneous, so the run is the same run, scaled."""
    pt = points((65, 80, 5))[8]  # delta = 1e-4
    f = 2.0 ** exponent
    g = pt["g"]
    gs = dict(g, kappa=g["kappa"] * f, tau=g["tau"] * f)
    kw = dict(max_steps=pt["max_steps"], test_every=10, seed=1, want_vector=True)
    a = certifier(g, pt["X"])
    b = certifier(gs, pt["X"])
    ra, rb = a.min_eig(pt["eta"], **kw), b.min_eig(pt["eta"] * f, **kw)
    (ala, bea), (alb, beb) = a.coefficients(), b.coefficients()
    a.close()
    b.close()
    print(ra["decision"], ra["steps"], rb["decision"], rb["steps"])
    assert ra["steps"] == rb["steps"] >= 20 and ra["decision"] == rb["decision"] != "UNDECIDED"
    assert np.array_equal(ala * f, alb) and np.array_equal(bea * f, beb)
    for k in ("theta_min", "theta_max", "residual"):
        assert ra[k] * f == rb[k], (k, ra[k] * f, rb[k])
    assert np.array_equal(ra["y"], rb["y"])
