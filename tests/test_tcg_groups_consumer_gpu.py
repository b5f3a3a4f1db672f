"""The grouped round in the consumer reduction form (KMX_GROUP_RED=2).

With robot groups in effect every group's launch chain can run without a
k_reduce launch: the gradient's sums are taken by the group's first k_hess,
k_update and k_hess reduce each other's partials, k_retract takes the last
update's and the final all-robot k_commit the trial cost's. A robot's sums are
taken over its own tiles in the same order in either form, so every comparison
here is np.array_equal against a fresh single-chain handle in the launched form
(KMX_RED=0 KMX_TCG_GROUPS=1): every robot's iterate, the GNC weights, the
status words and the work counters. Every grouped handle must report more than
one group and the consumer grouped form.

A tile is at most 48 poses at r = 5: the team below has a robot without
tiles, one with the poses of a single full tile and robots with those of 2 to
5, in groups of unequal robot counts.
"""
import numpy as np
import pytest

from kmx.dpgo.params import PGOAgentParameters, RobustCostType
from kmx.dpgo.solver import BlockSolver
from kmx.synth import lift, lifting_matrix, make_pose_graph
from kmx.synth.pose_graph import _expm_so3

pytestmark = pytest.mark.gpu

R_LIFT = 5
SIZES = (150, 0, 97, 210, 48)
CONSUMER = 2


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
    """perturb: one value, or one per robot."""
    Y = lifting_matrix(R_LIFT, seed=1)
    rng = np.random.default_rng(seed + 7)
    pr = np.broadcast_to(np.asarray(perturb, dtype=np.float64), (g.n_robots,))
    X0 = {}
    for a in range(g.n_robots):
        k = int(g.n_poses[a])
        Rp = g.init_R[a] @ _expm_so3(rng.normal(0, 1.0, (k, 3)) * pr[a])
        X0[a] = lift(Rp, g.init_t[a] + rng.normal(0, 5.0, (k, 3)) * pr[a], Y)
    return X0


def _params(robust=True, tcg=10, rtr=1):
    P = PGOAgentParameters(r=R_LIFT)
    if not robust:
        P.robustCostParams.costType = RobustCostType.L2
    P.localOptimizationParams.RTR_tCG_iterations = tcg
    P.localOptimizationParams.RTR_iterations = rtr
    return P


def _run(monkeypatch, groups, g, P, X0, *, rounds=6, poll=-1, gnc=True, per_call=None, idle_group=None,
         timing_calls=(), stream=None, stats=None, unequal=True):
    """Rounds on a fresh handle: groups == 1 is the reference (the launched
    form on a single chain), groups > 1 the grouped consumer form. Returns
    every robot's iterate, the GNC weights, the status words and the work
    counters.
    idle_group: the robots of this group of the two-group cut are inactive in
    every round. timing_calls: the iterate_async calls (by index) that run
    with timing switched on."""
    monkeypatch.setenv("KMX_RED", "0")
    monkeypatch.setenv("KMX_TCG_GROUPS", str(groups))
    monkeypatch.setenv("KMX_GROUP_RED", str(CONSUMER) if groups > 1 else "0")
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
        tiled = int((np.asarray(g.n_poses) > 0).sum())
        assert s.tcg_groups() == min(groups, tiled), (s.tcg_groups(), groups)
        if groups > 1:  # the grouped consumer path must really run
            assert s.tcg_groups() > 1
            assert s.group_reduction() == CONSUMER
            b = s.tcg_group_bounds()
            assert not unequal or len({hi - lo for lo, hi in zip(b, b[1:])}) > 1, b  # unequal robot counts
        else:
            assert s.group_reduction() == 0
        active = None
        if idle_group is not None:
            active = np.ones(g.n_robots, np.uint8)
            active[idle_group[0]:idle_group[1]] = 0
        s.read_counters()
        if active is not None or stats is not None:
            s.refresh_local()
            for _ in range(rounds):
                st = s.iterate(active)
                if stats is not None:
                    stats.append([x["tcg_iterations"] for x in st])
        else:
            left, first, call = rounds, True, 0
            while left > 0:
                n = min(left, per_call or rounds)
                on = call in timing_calls
                s.enable_timing(on)
                if on:  # one group in the single chain's form while timing is on
                    assert s.tcg_groups() == 1 and s.group_reduction() == 0
                elif groups > 1:
                    assert s.tcg_groups() > 1 and s.group_reduction() == CONSUMER
                s.iterate_async(n, refresh_local=first)
                s.sync()
                left, first, call = left - n, False, call + 1
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
def team():
    g = _graph(SIZES, seed=2)
    return g, _start(g, seed=2)


@pytest.fixture(scope="module")
def refs():
    """Reference results, computed once per case and left unchanged."""
    return {}


def _ref(refs, key, monkeypatch, g, P, X0, **kw):
    if key not in refs:
        refs[key] = _run(monkeypatch, 1, g, P, X0, **kw)
    return refs[key]


@pytest.mark.parametrize("poll", [1, 0, -1])
@pytest.mark.parametrize("groups", [2, 4])
def test_groups_and_poll_modes(gpu, monkeypatch, team, refs, groups, poll):
    """2 and 4 groups, polled, blind and adaptive enqueueing per group (the
    reference is polled adaptively: the mode does not change the results)."""
    g, X0 = team
    P = _params()
    ref = _ref(refs, "base", monkeypatch, g, P, X0, rounds=6)
    _same(ref, _run(monkeypatch, groups, g, P, X0, rounds=6, poll=poll))


@pytest.mark.parametrize("groups", [2, 4])
def test_gnc_schedule_fires_inside_the_run(gpu, monkeypatch, team, refs, groups):
    """14 rounds cross weight updates: the gated k_grad (the GNC commit by the
    group that holds tile 0, the preconditioner rebuild in every group) with
    the gradient's sums folded into the groups' first k_hess."""
    g, X0 = team
    P = _params()
    ref = _ref(refs, "gnc", monkeypatch, g, P, X0, rounds=14)
    assert ref[-1][3] >= 2, ref[-1]  # at least two weight updates
    _same(ref, _run(monkeypatch, groups, g, P, X0, rounds=14))


@pytest.mark.parametrize("groups", [2, 4])
def test_two_rtr_iterations(gpu, monkeypatch, team, refs, groups):
    """RTR_iterations = 2: the trial cost keeps its per-group k_reduce and a
    non-final commit of the group's own X runs on the group's stream."""
    g, X0 = team
    P = _params(rtr=2)
    ref = _ref(refs, "rtr2", monkeypatch, g, P, X0, rounds=5)
    _same(ref, _run(monkeypatch, groups, g, P, X0, rounds=5))


@pytest.mark.parametrize("groups,poll", [(2, 1), (4, 0)])
def test_25_tcg_steps(gpu, monkeypatch, team, refs, groups, poll):
    """RTR_tCG_iterations = 25: more steps than kept directions, so k_hess
    folds the oldest directions into eta."""
    g, X0 = team
    P = _params(tcg=25)
    ref = _ref(refs, "tcg25", monkeypatch, g, P, X0, rounds=4)
    _same(ref, _run(monkeypatch, groups, g, P, X0, rounds=4, poll=poll))


@pytest.fixture(scope="module")
def team_clean():
    """No outliers; robots 0-2 (group 0 of the two-group cut) start 300 times
    nearer to the odometry than robots 3 and 4."""
    g = _graph(SIZES, seed=2, outlier=0.0)
    return g, _start(g, seed=2, perturb=[1e-4, 1e-4, 1e-4, 3e-2, 3e-2])


@pytest.mark.parametrize("groups,poll", [(2, 1), (2, -1), (4, 1)])
def test_one_group_leaves_tcg_first(gpu, monkeypatch, team_clean, refs, groups, poll):
    """L2 cost from a nearly converged start, residual stop at kappa 0.3
    (relative to the gradient norm, so the robots far from the optimum meet it
    first). Chosen on the CPU restatement, whose per-robot step counts are
    2 0 4 1 1, 4 0 3 2 3, 7 0 6 6 3, 5 0 4 5 4, 10 0 3 6 3: in the first round
    the robots of the second group leave tCG in their first step while those
    of the first go on, so a polled group stops being enqueued (and skips its
    k_retract) while the other chain runs on."""
    g, X0 = team_clean
    P = _params(robust=False, tcg=10)
    lo = P.localOptimizationParams
    lo.tCG_kappa = 0.3
    lo.RTR_initial_radius, lo.RTR_max_radius = 1e4, 1e6  # no stop at the trust-region boundary
    if "l2" not in refs:
        st = []
        refs["l2"] = (_run(monkeypatch, 1, g, P, X0, rounds=5, poll=1, gnc=False, stats=st), st)
    (ref, steps), got_steps = refs["l2"], []
    first = steps[0]
    assert max(first[3:]) == 1 and min(first[0], first[2]) >= 2, steps
    _same(ref, _run(monkeypatch, groups, g, P, X0, rounds=5, poll=poll, gnc=False, stats=got_steps))
    assert steps == got_steps


def test_idle_group(gpu, monkeypatch, team, refs):
    """An active mask that idles a whole group, each group in turn: its chain
    runs launches that every tile leaves at the phase test."""
    g, X0 = team
    P = _params()
    monkeypatch.setenv("KMX_TCG_GROUPS", "2")
    s = BlockSolver(P, 0)
    s.set_graph_data(g)
    b = s.tcg_group_bounds()
    s.close()
    assert len(b) == 3
    for k in range(2):
        idle = (b[k], b[k + 1])
        ref = _run(monkeypatch, 1, g, P, X0, rounds=5, idle_group=idle)
        for poll in (1, -1):
            _same(ref, _run(monkeypatch, 2, g, P, X0, rounds=5, idle_group=idle, poll=poll))


def test_caller_stream(gpu, monkeypatch, team, refs):
    """A caller-supplied main stream (created through the HIP runtime that
    serves libkmx): group 0 and the fork / join run on it."""
    import ctypes as C

    from kmx import abi
    g, X0 = team
    P = _params()
    ref = _ref(refs, "base", monkeypatch, g, P, X0, rounds=6)
    hip = C.CDLL(abi.runtime_info()["hip_path"])
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    st = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(st)) == 0 and st.value
    try:
        _same(ref, _run(monkeypatch, 2, g, P, X0, rounds=6, stream=st.value))
    finally:
        assert hip.hipStreamDestroy(st) == 0


@pytest.mark.parametrize("groups", [2, 4])
def test_timing_on_and_off_between_rounds(gpu, monkeypatch, team, refs, groups):
    """Timing switched on for the second and fourth of six one-round calls:
    those rounds run one group in the launched form between grouped consumer
    rounds, and the results are unchanged."""
    g, X0 = team
    P = _params()
    ref = _ref(refs, "base", monkeypatch, g, P, X0, rounds=6)
    _same(ref, _run(monkeypatch, groups, g, P, X0, rounds=6, per_call=1, timing_calls=(1, 3)))


def test_default_form_by_tiles_per_robot(gpu, monkeypatch, team):
    """Without KMX_GROUP_RED the grouped form is the consumer one while every
    robot has at most 384 tiles (up to there it measured faster), else
    the launched one. 16 incidences per tile give the 2000-pose robot about
    700 tiles: the default is the launched form there, and the forced consumer
    form, whose workgroups then sum the robot's partials in a loop, still
    gives the reference's bits."""
    g, X0 = team
    monkeypatch.setenv("KMX_RED", "0")
    monkeypatch.setenv("KMX_TCG_GROUPS", "2")
    monkeypatch.delenv("KMX_GROUP_RED", raising=False)
    s = BlockSolver(_params(), 0)
    try:
        s.set_graph_data(g)
        assert s.tcg_groups() == 2 and s.group_reduction() == CONSUMER
    finally:
        s.close()
    gb = _graph((2000, 300), seed=5)
    Xb = _start(gb, seed=5)
    P = _params()
    P.tileIncidences = 16
    s = BlockSolver(P, 0)
    try:
        s.set_graph_data(gb)
        assert s.tcg_groups() == 2 and s.group_reduction() == 0
    finally:
        s.close()
    ref = _run(monkeypatch, 1, gb, P, Xb, rounds=4, unequal=False)
    _same(ref, _run(monkeypatch, 2, gb, P, Xb, rounds=4, unequal=False))


def test_repeatable(gpu, monkeypatch, team):
    """The same grouped consumer run twice, several rounds per call."""
    g, X0 = team
    P = _params()
    a = _run(monkeypatch, 2, g, P, X0, rounds=8, per_call=4)
    _same(a, _run(monkeypatch, 2, g, P, X0, rounds=8, per_call=4))
