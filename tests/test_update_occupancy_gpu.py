"""k_update at seven or eight waves per SIMD: the shapes at which it can go wrong.

The second half of a tCG step (pgo.hip body_update) no longer holds the
preconditioner block across the projection, reads the group's Y^T G products
back from LDS two members at a time (group_symYtG, shared with k_grad,
k_retract and k_step), and in the consumer form publishes the robot's state
with 32 lanes instead of one thread. Nothing in the arithmetic moves, so every
form of the round gives the bits of every other one, and the restatement's
results to the project's bar: equal tCG counts, acceptance and update flags,
poses within 1e-6, GNC weights within 1e-9.

The team: robots of 150, 97, 1 and 0 poses and one of 400 (tiles with fewer
poses than a tile holds, a tile of one pose without an edge, a robot without
tiles). tCG capped at 1, 2, 3 and 10 steps with robots leaving at different
steps (step 0 reads g in place of r; a robot that stops has its trial point
formed inside the consumer k_update, the rest by k_retract's fold 2); a
trust-region radius at which tCG ends on the boundary (no z, no partials);
the preconditioner on and off; a robot of more than 1,024 tiles, which the
register form of the consumer's robot sum (four tiles per thread) does not
hold; r = 3, 5 and 6.

Forms crossed: KMX_RED 0 / 2 and KMX_TCG_GROUPS 1 / 2 with KMX_GROUP_RED 2.
"""
import numpy as np
import pytest

from kmx.dpgo.params import PGOAgentParameters
from kmx.synth import lift, lifting_matrix
from kmx.synth.pose_graph import PoseGraphData, _expm_so3

pytestmark = pytest.mark.gpu

ISOLATED, EMPTY = 2, 3
# (KMX_RED, KMX_TCG_GROUPS): the launched single chain, the consumer single
# chain, the grouped consumer round
REFERENCE = ("0", "1")
FORMS = [("2", "1"), ("0", "2")]
ROBOT_SUM_TILES = 4 * 256  # RobotSum<1, 4> in k_update: four tiles per thread of a 256-thread workgroup


def team_graph(sizes, seed=0, ring=None):
    """Robots of the given sizes: an odometry chain and random loop closures
    inside each robot with more than one pose, 25 closures between each pair
    of such robots, 15 % outliers. ring = (robot, k): every pose of that robot
    also closes loops with its next k successors but one (mod the robot's
    size), so that each pose has at least 2 k + 1 incidences."""
    rng = np.random.default_rng(seed)
    n = np.array(sizes, np.int32)
    gt_R = [_expm_so3(rng.normal(0, 0.3, (int(k), 3))) for k in n]
    gt_t = [np.cumsum(rng.normal(0, 1.0, (int(k), 3)), axis=0) for k in n]
    chains = [(a, int(k)) for a, k in enumerate(n) if k > 1]
    E = []  # (r1, p1, r2, p2, fixed)
    for a, k in chains:
        E += [(a, i, a, i + 1, 1) for i in range(k - 1)]
        if ring is None or ring[0] != a:
            E += [(a, int(i), a, int(j), 0) for i, j in rng.integers(0, k, (k, 2)) if abs(int(i) - int(j)) > 1]
        else:
            E += [(a, i, a, (i + s) % k, 0) for i in range(k) for s in range(2, 2 + ring[1])]
    for x, (a, ka) in enumerate(chains):
        for b, kb in chains[x + 1:]:
            E += [(a, int(i), b, int(j), 0) for i, j in zip(rng.integers(0, ka, 25), rng.integers(0, kb, 25))]
    E = np.array(E, dtype=np.int64)
    r1, p1, r2, p2 = (E[:, k].astype(np.int32) for k in range(4))
    m = len(E)
    R = np.empty((m, 3, 3))
    t = np.empty((m, 3))
    outlier = rng.random(m) < 0.15
    outlier[E[:, 4] == 1] = False
    for e in range(m):
        Ra, ta = gt_R[r1[e]][p1[e]], gt_t[r1[e]][p1[e]]
        Rb, tb = gt_R[r2[e]][p2[e]], gt_t[r2[e]][p2[e]]
        Rr, tr = Ra.T @ Rb, Ra.T @ (tb - ta)
        if outlier[e]:
            Rr, tr = _expm_so3(rng.normal(0, 2.0, (1, 3)))[0], rng.uniform(-10, 10, 3)
        R[e] = Rr @ _expm_so3(rng.normal(0, 0.01, (1, 3)))[0]
        t[e] = tr + rng.normal(0, 0.1, 3)
    init_R = [gt_R[a] @ _expm_so3(rng.normal(0, 0.05, (int(k), 3))) if k else np.zeros((0, 3, 3))
              for a, k in enumerate(n)]
    init_t = [gt_t[a] + rng.normal(0, 0.3, (int(k), 3)) if k else np.zeros((0, 3)) for a, k in enumerate(n)]
    return PoseGraphData(n_robots=len(n), n_poses=n, r1=r1, p1=p1, r2=r2, p2=p2, R=R, t=t,
                         kappa=np.full(m, 1e4), tau=np.full(m, 1e2), weight=np.ones(m),
                         fixed=E[:, 4].astype(np.uint8), outlier=outlier, gt_R=gt_R, gt_t=gt_t,
                         init_R=init_R, init_t=init_t)


def tile_cut(g, r, tile_incidences=0):
    """set_graph's cut, restated: (robot, first pose, poses, incidences) per
    tile. A tile holds at most TP = 4 * (64 / r) poses of one robot and closes
    when the next pose would take it past the cap: the smaller of the handle's
    (two chunks of TP * r incidences, or for a small problem about 736 tiles
    but at least 180 incidences; tile_incidences overrides it, 16 at least)
    and 1.05 x the robot's mean per full tile."""
    TP = 4 * (64 // r)
    deg = [np.zeros(int(k), np.int64) for k in g.n_poses]
    for rr, pp in ((g.r1, g.p1), (g.r2, g.p2)):
        for a, p in zip(rr, pp):
            deg[a][p] += 1
    inc_all = int(sum(d.sum() for d in deg))
    cap_all = min(2 * TP * r, max(180, -(-inc_all // 736)))
    if tile_incidences > 0:
        cap_all = max(16, tile_incidences)
    tiles = []
    for a, d in enumerate(deg):
        k = len(d)
        full = max(1, -(-k // TP))
        cap = min(cap_all, max(1, (int(d.sum()) * 21 // 20 + full - 1) // full))
        p0 = 0
        while p0 < k:
            np_, cum = 0, 0
            while p0 + np_ < k and np_ < TP:
                if np_ > 0 and cum + d[p0 + np_] > cap:
                    break
                cum += int(d[p0 + np_])
                np_ += 1
            tiles.append((a, p0, np_, cum))
            p0 += np_
    return tiles


def params(r=5, tcg=10, radius=1e3, precond=True, tile_incidences=0, gradnorm_tol=None):
    P = PGOAgentParameters(r=r)
    lo = P.localOptimizationParams
    lo.RTR_tCG_iterations = tcg
    lo.RTR_initial_radius, lo.RTR_max_radius = radius, 1e6
    lo.use_preconditioner = precond
    P.tileIncidences = tile_incidences
    if gradnorm_tol is not None:
        lo.gradnorm_tol = gradnorm_tol
    return P


def start(g, r):
    Y = lifting_matrix(r, seed=1)
    return {a: lift(g.init_R[a], g.init_t[a], Y) for a in range(g.n_robots) if g.n_poses[a]}


def set_form(monkeypatch, form):
    red, groups = form
    monkeypatch.setenv("KMX_RED", red)
    monkeypatch.setenv("KMX_TCG_GROUPS", groups)
    monkeypatch.setenv("KMX_GROUP_RED", "2" if groups != "1" else "0")


def run(monkeypatch, form, g, P, X0, rounds, weights_every=4):
    """Rounds on a fresh handle in the given form, a GNC weight update every
    `weights_every` rounds: the iterates, the weights, the status words, the
    work counters, every round's per-robot (tCG steps, accepted, updated) and
    the stop reasons. The robot without poses is left out of the active set
    (at a gradient tolerance of 0 the launched form runs a block update over
    nothing for it and the consumer form has no tile to run it on; at any
    positive tolerance both skip it, which the oracle tests cover)."""
    from kmx.dpgo.solver import BlockSolver
    set_form(monkeypatch, form)
    s = BlockSolver(P, 0)
    try:
        s.set_graph_data(g)
        red, groups = form
        assert s.tcg_groups() == int(groups)
        assert s.group_reduction() == (2 if groups != "1" else int(red))
        for a, X in X0.items():
            s.set_iterate(a, X)
        s.read_counters()
        steps, stops = [], []
        active = (np.asarray(g.n_poses) > 0).astype(np.uint8)
        for it in range(rounds):
            s.refresh_local()
            st = s.iterate(active)
            steps.append([(x["tcg_iterations"], x["accepted"], x["updated"]) for x in st])
            stops.append([x["tcg_stop"] for x in st])
            if it % weights_every == weights_every - 1:
                s.refresh_local()
                s.update_weights()
        c = s.read_counters()
        out = [s.get_iterate(a) for a in sorted(X0)]
        out += [s.get_weights(), s.status(),
                np.array([c["hessvecs"], c["edges_iters"], c["block_updates"], c["gnc_updates"]]), np.array(steps),
                np.array(stops)]
        return out
    finally:
        s.close()


def same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), (what, k)


def against_oracle(monkeypatch, form, g, P, rounds):
    """One handle in `form` next to the restatement, checked after every
    round; returns every round's stop reasons."""
    from kmx.dpgo.solver import BlockSolver
    from oracle.oracle import OraclePGO
    set_form(monkeypatch, form)
    X0 = start(g, P.r)
    s = BlockSolver(P, 0)
    stops = []
    try:
        s.set_graph_data(g)
        o = OraclePGO(P.to_c(), g)
        for a, X in X0.items():
            s.set_iterate(a, X)
            o.set_iterate(a, X)
        s.refresh_local()
        o.refresh()
        for it in range(rounds):
            s.refresh_local()
            sg, so = s.iterate(), o.iterate()
            stops.append([x["tcg_stop"] for x in sg])
            for a in range(g.n_robots):
                assert sg[a]["updated"] == so[a]["updated"], (it, a)
                assert sg[a]["tcg_iterations"] == so[a]["tcg_iterations"], (it, a, sg[a], so[a])
                assert sg[a]["accepted"] == so[a]["accepted"], (it, a)
                if g.n_poses[a]:
                    d = np.linalg.norm((s.get_iterate(a) - o.get_iterate(a)).reshape(-1, 4 * P.r), axis=1).max()
                    assert d <= 1e-6, (it, a, d)
            if it % 4 == 3:
                s.refresh_local()
                assert s.update_weights() == o.update_weights()
                assert np.abs(s.get_weights() - o.get_weights()).max() <= 1e-9
    finally:
        s.close()
    return stops


BOUNDARY = ("exceeded_trust_region", "negative_curvature")


@pytest.fixture(scope="module")
def team():
    g = team_graph([150, 97, 1, 0, 400])
    tiles = tile_cut(g, 5)
    assert (ISOLATED, 0, 1, 0) in tiles              # a tile of one pose, without incidences
    assert all(a != EMPTY for a, _, _, _ in tiles)    # the robot without poses has no tile
    assert min(k for _, _, k, _ in tiles) == 1 and max(k for _, _, k, _ in tiles) <= 48
    assert any(1 < k < 48 for _, _, k, _ in tiles)    # tiles that fill only part of the workgroup
    assert len(tiles) > 8                             # more than one workgroup per XCD slot
    return g


@pytest.fixture(scope="module")
def refs():
    """The launched single chain's results, computed once per case and left unchanged."""
    return {}


def reference(refs, key, monkeypatch, *a, **kw):
    if key not in refs:
        refs[key] = run(monkeypatch, REFERENCE, *a, **kw)
    return refs[key]


@pytest.mark.parametrize("precond", [True, False])
@pytest.mark.parametrize("form", [REFERENCE] + FORMS)
def test_team_matches_oracle(gpu, monkeypatch, team, form, precond):
    """Interior steps with the preconditioner's block and without it, a
    weight update inside the run, every robot active (the robot without poses
    and, at the default tolerance, the pose without edges are skipped)."""
    against_oracle(monkeypatch, form, team, params(precond=precond), rounds=8)


@pytest.mark.parametrize("tcg", [1, 2, 3, 10])
def test_forms_agree(gpu, monkeypatch, team, refs, tcg):
    """tCG capped at 1, 2, 3 and 10 steps with the gradient tolerance at 0, so
    that the one-pose tile runs its update too. At a cap of 1 every robot's
    only update reads g; at 10 robots stop at different steps, so one launch
    of the consumer k_update forms a stopped robot's trial point while another
    robot's tiles run a step, and robots still in tCG at the cap are left to
    k_retract's fold 2."""
    g = team
    P = params(tcg=tcg, gradnorm_tol=0.0)
    X0 = start(g, 5)
    ref = reference(refs, ("r5", tcg), monkeypatch, g, P, X0, rounds=8)
    steps = ref[-2][:, :, 0]
    tiled = [a for a in range(g.n_robots) if a not in (ISOLATED, EMPTY)]
    assert (steps[:, ISOLATED] > 0).all(), steps
    assert steps.max() == tcg
    if tcg == 10:
        assert sum(len(set(row[tiled])) > 1 for row in steps) >= 3, steps
        assert steps[:, tiled].min() < 10, steps
    for form in FORMS:
        same(ref, run(monkeypatch, form, g, P, X0, rounds=8), form)


@pytest.mark.parametrize("precond", [True, False])
def test_boundary_steps(gpu, monkeypatch, team, precond):
    """A radius of 1: tCG ends on the trust-region boundary, the update
    without z and without partials. The status says that it happened, for a
    robot with tiles, and that other robots' steps were interior."""
    g = team
    stops = against_oracle(monkeypatch, ("2", "1"), g, params(radius=1.0, precond=precond), rounds=6)
    tiled = [a for a in range(g.n_robots) if a not in (ISOLATED, EMPTY)]
    assert any(stops[it][a] in BOUNDARY for it in range(len(stops)) for a in tiled), stops
    P = params(radius=1.0, precond=precond, gradnorm_tol=0.0)
    X0 = start(g, 5)
    ref = run(monkeypatch, REFERENCE, g, P, X0, rounds=6)
    st, steps = ref[-1], ref[-2][:, :, 0]
    assert np.isin(st[:, tiled], BOUNDARY).any(), st
    assert (steps[np.isin(st, BOUNDARY)] >= 1).all()
    for form in FORMS:
        same(ref, run(monkeypatch, form, g, P, X0, rounds=6), form)


def test_precond_off_forms_agree(gpu, monkeypatch, team):
    g = team
    P = params(precond=False, gradnorm_tol=0.0)
    X0 = start(g, 5)
    ref = run(monkeypatch, REFERENCE, g, P, X0, rounds=6)
    for form in FORMS:
        same(ref, run(monkeypatch, form, g, P, X0, rounds=6), form)


def test_robot_of_many_tiles(gpu, monkeypatch):
    """A robot of 1,100 poses with 9 or more incidences each at 16 incidences
    per tile: every pose a tile of its own, more tiles than the consumer
    k_update's register form of the robot sum holds (it falls back to the
    loop); next to it robots of 150 and 97 poses in a few tiles each."""
    g = team_graph([150, 1100, 97], seed=5, ring=(1, 4))
    tiles = tile_cut(g, 5, 16)
    per_robot = [sum(1 for a, _, _, _ in tiles if a == b) for b in range(3)]
    assert per_robot[1] == 1100 > ROBOT_SUM_TILES, per_robot
    assert max(per_robot[0], per_robot[2]) <= ROBOT_SUM_TILES
    against_oracle(monkeypatch, ("2", "1"), g, params(tile_incidences=16), rounds=5)
    P = params(tile_incidences=16, gradnorm_tol=0.0)
    X0 = start(g, 5)
    ref = run(monkeypatch, REFERENCE, g, P, X0, rounds=5)
    assert ref[-2][:, :, 0].max() > 1
    for form in FORMS:
        same(ref, run(monkeypatch, form, g, P, X0, rounds=5), form)


@pytest.mark.parametrize("r", [3, 6])
def test_other_lifts(gpu, monkeypatch, r):
    """r = 3 (21 poses per wave, one idle lane) and r = 6 (10 per wave, four
    idle lanes): against the restatement and across forms."""
    g = team_graph([150, 97, 1, 0, 400], seed=r)
    assert (ISOLATED, 0, 1, 0) in tile_cut(g, r)
    against_oracle(monkeypatch, ("2", "1"), g, params(r=r), rounds=6)
    P = params(r=r, gradnorm_tol=0.0)
    X0 = start(g, r)
    ref = run(monkeypatch, REFERENCE, g, P, X0, rounds=6)
    for form in FORMS:
        same(ref, run(monkeypatch, form, g, P, X0, rounds=6), form)
