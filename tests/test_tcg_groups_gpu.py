"""Robot groups of the launched-reduction round (KMX_TCG_GROUPS).

Between a round's begin launch and its final commit a robot's launches read its
own rows and the public table only, so the handle runs contiguous groups of
robots on streams of their own. A robot's arithmetic depends on its tiles and on
the order in which its tile partials are summed, and grouping changes neither:
every comparison here is np.array_equal against a fresh handle with
KMX_TCG_GROUPS=1, and every grouped handle must report more than one group.
KMX_RED=0 makes these small graphs run the launched form.
"""
import numpy as np
import pytest

from kmx.dpgo.params import PGOAgentParameters, RobustCostType
from kmx.dpgo.solver import BlockSolver
from kmx.synth import lift, lifting_matrix, make_pose_graph
from kmx.synth.pose_graph import _expm_so3

pytestmark = pytest.mark.gpu

R_LIFT = 5


def _graph(sizes, seed=0, edges_per_pose=3, outlier=0.2):
    """A make_pose_graph team cut down to `sizes` poses per robot (a robot keeps
    its first poses; measurements that touch a dropped pose go). Size 0: a robot
    without poses, hence without tiles."""
    nr, big = len(sizes), max(sizes)
    g = make_pose_graph(nr, nr * big, nr * big * edges_per_pose, outlier_frac=outlier, seed=seed)
    sz = np.asarray(sizes, dtype=np.int32)
    keep = (g.p1 < sz[g.r1]) & (g.p2 < sz[g.r2])
    for f in ("r1", "p1", "r2", "p2", "R", "t", "kappa", "tau", "weight", "fixed", "outlier"):
        setattr(g, f, np.ascontiguousarray(getattr(g, f)[keep]))
    g.n_poses = sz
    for f in ("gt_R", "gt_t", "init_R", "init_t"):
        setattr(g, f, [x[:n] for x, n in zip(getattr(g, f), sizes)])
    return g


def _start(g, seed=0, perturb=0.05):
    Y = lifting_matrix(R_LIFT, seed=1)
    rng = np.random.default_rng(seed + 7)
    X0 = {}
    for a in range(g.n_robots):
        k = int(g.n_poses[a])
        Rp = g.init_R[a] @ _expm_so3(rng.normal(0, perturb, (k, 3)))
        X0[a] = lift(Rp, g.init_t[a] + rng.normal(0, 5 * perturb, (k, 3)), Y)
    return X0


def _params(robust=True, tcg=10, rtr=1):
    P = PGOAgentParameters(r=R_LIFT)
    if not robust:
        P.robustCostParams.costType = RobustCostType.L2
    P.localOptimizationParams.RTR_tCG_iterations = tcg
    P.localOptimizationParams.RTR_iterations = rtr
    return P


def _incidences(g):
    """Incidences per robot: one per local endpoint of every measurement."""
    inc = np.zeros(g.n_robots, dtype=np.int64)
    np.add.at(inc, g.r1, 1)
    np.add.at(inc, g.r2, 1)
    return inc


def _check_cut(g, bounds, asked):
    """The cut is ordered, covers every robot once, has as many groups as asked
    for (clamped to the robots with poses), gives every group a robot with
    poses, and no other contiguous cut into that many groups has a smaller
    worst distance of a boundary's incidence prefix from its even share."""
    inc, nr = _incidences(g), g.n_robots
    tiled = int((np.asarray(g.n_poses) > 0).sum())
    G = len(bounds) - 1
    assert G == min(asked, tiled), (bounds, asked, tiled)
    assert bounds[0] == 0 and bounds[-1] == nr and all(a < b for a, b in zip(bounds, bounds[1:])), bounds
    for a, b in zip(bounds, bounds[1:]):
        assert (np.asarray(g.n_poses[a:b]) > 0).any(), bounds
    pre = np.concatenate([[0], np.cumsum(inc)])
    for k in range(1, G):  # each boundary is the feasible cut nearest to k / G of the incidences
        here = abs(G * pre[bounds[k]] - k * pre[nr])
        for c in (bounds[k] - 1, bounds[k] + 1):
            lo, hi = bounds[k - 1], bounds[k + 1]
            if c <= lo or c >= hi:
                continue
            if not (np.asarray(g.n_poses[lo:c]) > 0).any() or not (np.asarray(g.n_poses[c:hi]) > 0).any():
                continue
            assert here <= abs(G * pre[c] - k * pre[nr]), (bounds, k, c)


def _run(monkeypatch, groups, g, P, X0, *, rounds=6, poll=-1, gnc=True, per_call=None, active=None,
         timing=False, stream=None, expect=None, stats=None):
    """Rounds on a fresh handle; returns every robot's iterate, the GNC
    weights, the status words and the work counters."""
    monkeypatch.setenv("KMX_RED", "0")
    monkeypatch.setenv("KMX_TCG_GROUPS", str(groups))
    s = BlockSolver(P, 0)
    try:
        if stream is not None:
            s.set_stream(stream)
        s.set_tcg_poll(poll)
        s.set_graph_data(g)
        if gnc:
            s.set_gnc_schedule(True, 3, 50, P.relChangeTol)
        for a in range(g.n_robots):
            if g.n_poses[a]:
                s.set_iterate(a, X0[a])
        want = (min(groups, int((np.asarray(g.n_poses) > 0).sum())) if expect is None else expect)
        assert s.tcg_groups() == want, (s.tcg_groups(), want)
        if groups > 1:
            assert s.tcg_groups() > 1  # the grouped path must really run
            _check_cut(g, s.tcg_group_bounds(), groups)
        if timing:
            s.enable_timing(True)
            assert s.tcg_groups() == 1
            s.enable_timing(False)
            assert s.tcg_groups() == want
            s.enable_timing(True)
        s.read_counters()
        if active is not None or stats is not None:
            s.refresh_local()
            for _ in range(rounds):
                st = s.iterate(active)
                if stats is not None:
                    stats.append([x["tcg_iterations"] for x in st])
        else:
            left, first = rounds, True
            while left > 0:
                n = min(left, per_call or rounds)
                s.iterate_async(n, refresh_local=first)
                s.sync()
                left, first = left - n, False
        c = s.read_counters()
        out = [s.get_iterate(a) for a in range(g.n_robots) if g.n_poses[a]]
        out += [s.get_weights(), s.status(),
                np.array([c["hessvecs"], c["edges_iters"], c["block_updates"], c["gnc_updates"]])]
        return out
    finally:
        s.close()


def _same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), k


@pytest.fixture(scope="module")
def team3():
    g = _graph([300, 300, 300], seed=6)
    return g, _start(g, seed=6)


@pytest.fixture(scope="module")
def team5():
    g = _graph([300, 150, 150, 300, 200], seed=2)
    return g, _start(g, seed=2)


@pytest.mark.parametrize("asked", [2, 4])
def test_three_robots_gnc_rounds(gpu, monkeypatch, team3, asked):
    """3 robots in 2 groups (2 + 1 or 1 + 2) and with 4 asked for (clamped to
    3), robust GNC-TLS on the device schedule over 14 rounds that cross weight
    updates: the gated k_grad and its GNC store run in the group of tile 0."""
    g, X0 = team3
    P = _params()
    ref = _run(monkeypatch, 1, g, P, X0, rounds=14)
    assert ref[-1][3] >= 2, ref[-1]  # at least two weight updates
    _same(ref, _run(monkeypatch, asked, g, P, X0, rounds=14))


@pytest.mark.parametrize("asked", [2, 4])
def test_five_unequal_robots(gpu, monkeypatch, team5, asked):
    g, X0 = team5
    P = _params()
    ref = _run(monkeypatch, 1, g, P, X0, rounds=9)
    _same(ref, _run(monkeypatch, asked, g, P, X0, rounds=9))


@pytest.mark.parametrize("tcg,rtr", [(1, 1), (3, 1), (10, 2)])
def test_tcg_caps_and_rtr_iterations(gpu, monkeypatch, team3, tcg, rtr):
    """tCG caps 1, 3 and 10; two RTR iterations put a non-final commit of each
    group's own X between them, on the group's stream."""
    g, X0 = team3
    P = _params(tcg=tcg, rtr=rtr)
    ref = _run(monkeypatch, 1, g, P, X0, rounds=6)
    _same(ref, _run(monkeypatch, 2, g, P, X0, rounds=6))


@pytest.fixture(scope="module")
def team3_clean():
    g = _graph([300, 300, 300], seed=6, outlier=0.0)
    return g, _start(g, seed=6, perturb=0.01)


@pytest.mark.parametrize("poll", [1, 0, -1])
def test_poll_modes_with_uneven_groups(gpu, monkeypatch, team3_clean, poll):
    """Polled, blind and adaptive enqueueing per group. No outliers, L2 cost
    and a residual stop at kappa 0.3: tCG stops on its residual test after 2 to
    8 steps, differently per robot (chosen on the CPU restatement: the per-robot
    step counts of the six rounds are 2 2 2, 4 3 4, 3 5 3, 6 8 6, 4 3 4, 6 5 4),
    so a polled group stops being enqueued while the other goes on. The
    one-group run's step counts must differ by two or more between the groups
    in some round, wherever the cut falls."""
    g, X0 = team3_clean
    P = _params(robust=False, tcg=10)
    lo = P.localOptimizationParams
    lo.tCG_kappa = 0.3
    lo.RTR_initial_radius, lo.RTR_max_radius = 1e4, 1e6  # no stop at the trust-region boundary
    steps, got_steps = [], []
    ref = _run(monkeypatch, 1, g, P, X0, rounds=6, poll=poll, gnc=False, stats=steps)
    got = _run(monkeypatch, 2, g, P, X0, rounds=6, poll=poll, gnc=False, stats=got_steps)
    _same(ref, got)
    assert steps == got_steps
    for cut in (1, 2):  # group 0 holds robot 0, or robots 0 and 1
        assert max(abs(max(r[:cut]) - max(r[cut:])) for r in steps) >= 2, steps


def test_inactive_robot_and_robot_without_tiles(gpu, monkeypatch):
    """Robot 1 has no poses (no tiles: it belongs to a group and launches
    nothing) and robot 2 is inactive in every round."""
    g = _graph([300, 0, 250, 300], seed=3)
    X0 = _start(g, seed=3)
    P = _params()
    act = np.array([1, 1, 0, 1], np.uint8)
    ref = _run(monkeypatch, 1, g, P, X0, rounds=6, active=act)
    _same(ref, _run(monkeypatch, 2, g, P, X0, rounds=6, active=act))
    _same(ref, _run(monkeypatch, 4, g, P, X0, rounds=6, active=act))


def test_timing_turns_groups_off(gpu, monkeypatch, team3):
    """With timing on the handle runs one group (the evented replay wants
    launches that do not overlap); the getter says so, reports the groups again
    once timing is off, and the results equal the untimed grouped run."""
    g, X0 = team3
    P = _params()
    ref = _run(monkeypatch, 1, g, P, X0, rounds=6)
    _same(ref, _run(monkeypatch, 2, g, P, X0, rounds=6))
    _same(ref, _run(monkeypatch, 2, g, P, X0, rounds=6, timing=True))


def test_several_rounds_per_call(gpu, monkeypatch, team5):
    """iterate_async with several rounds per call: round k + 1's begin launch
    and its groups start behind round k's final commit on the handle's stream."""
    g, X0 = team5
    P = _params()
    ref = _run(monkeypatch, 1, g, P, X0, rounds=12, per_call=1)
    _same(ref, _run(monkeypatch, 2, g, P, X0, rounds=12, per_call=12))
    _same(ref, _run(monkeypatch, 4, g, P, X0, rounds=12, per_call=5))


def test_caller_stream(gpu, monkeypatch, team3):
    """A caller-supplied main stream (created through the HIP runtime that
    serves libkmx): group 0 and the fork / join run on it."""
    import ctypes as C

    from kmx import abi
    g, X0 = team3
    P = _params()
    ref = _run(monkeypatch, 1, g, P, X0, rounds=6)
    hip = C.CDLL(abi.runtime_info()["hip_path"])
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    st = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(st)) == 0 and st.value
    try:
        _same(ref, _run(monkeypatch, 2, g, P, X0, rounds=6, stream=st.value))
    finally:
        assert hip.hipStreamDestroy(st) == 0


def test_consumer_form_runs_one_group(gpu, monkeypatch, team3):
    """Groups are for the launched form: the consumer form reports 1."""
    g, X0 = team3
    monkeypatch.setenv("KMX_RED", "2")
    monkeypatch.setenv("KMX_TCG_GROUPS", "2")
    s = BlockSolver(_params(), 0)
    s.set_graph_data(g)
    assert s.tcg_groups() == 1
    assert len(s.tcg_group_bounds()) == 3  # the cut exists, not in effect
    s.close()
