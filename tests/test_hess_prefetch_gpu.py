"""k_hess with the next chunk's rows and the epilogue's loads issued ahead.

The Hessian gather (pgo.hip hinc_gather_src) walks a tile's incidences in
chunks of CH = TP * r lanes (240 at r = 5). It issues the next chunk's records
and neighbour rows once the current chunk's contributions are in LDS, and on
the tile's last chunk -- peeled out of the loop -- the epilogue's loads in
their place; a tile without incidences issues the epilogue's loads at once.
The word that holds a row's address is fetched a chunk before the row. Nothing
in the arithmetic moves, so every form of the round must give the bits of every other
one, and the restatement's results to the project's bar: equal tCG counts,
acceptance and update flags, poses within 1e-6, GNC weights within 1e-9.

The team: hub poses at the end of the last robot, each a tile of its own with
1, 239, 240, 241, 479, 480, 481 and 721 incidences (no loop iteration, the
loop's exit at exactly one and two chunks, a second or third chunk with one
incidence, four chunks), the last of them on the last pose of the last robot
so that its tile ends the record array; a robot of one pose without an edge
and a robot without poses. The cut is restated from set_graph's rule and the
hub tiles are asserted to be there.

Forms crossed: KMX_RED 0 / 2, KMX_TCG_GROUPS 1 / 2 with KMX_GROUP_RED 2,
KMX_HESS_DECIDE 0 / 1 (the stop decision after / before the gather; the size
rule takes "after" only above 80,000 poses), KMX_HESS_GATE 0 / 1.
"""
import numpy as np
import pytest

from kmx.dpgo.params import PGOAgentParameters
from kmx.synth import lift, lifting_matrix
from kmx.synth.pose_graph import PoseGraphData, _expm_so3

pytestmark = pytest.mark.gpu

HUBS_R5 = (721, 1, 481, 239, 480, 240, 479, 241)  # any two neighbours exceed a two-chunk tile
LEAVES = 400
ISOLATED, EMPTY, LAST = 1, 2, 4

# (KMX_RED, KMX_TCG_GROUPS, KMX_HESS_DECIDE): the launched single chain, the
# consumer single chain and the grouped consumer round with either decision
REFERENCE = ("0", "1", None)
FORMS = [("2", "1", "0"), ("2", "1", "1"), ("0", "2", "0"), ("0", "2", "1")]


def chunk(r):
    return 4 * (64 // r) * r  # SmemH<R>::CH at four waves per workgroup


def hub_team(hubs, seed=0, off_so3=False):
    """Robots of 150, 1, 0, 97 and LEAVES + len(hubs) poses. The last robot is
    an odometry chain of LEAVES poses followed by the hub poses, which have no
    odometry: hub k has exactly hubs[k] incidences, loop closures to the leaves
    in alternating direction (so a hub is tail and head)."""
    rng = np.random.default_rng(seed)
    n = np.array([150, 1, 0, 97, LEAVES + len(hubs)], np.int32)
    gt_R = [_expm_so3(rng.normal(0, 0.3, (int(k), 3))) for k in n]
    gt_t = [np.cumsum(rng.normal(0, 1.0, (int(k), 3)), axis=0) for k in n]
    E = []  # (r1, p1, r2, p2, fixed)
    for a, k in ((0, 150), (3, 97), (LAST, LEAVES)):
        E += [(a, i, a, i + 1, 1) for i in range(k - 1)]
        E += [(a, int(i), a, int(j), 0) for i, j in rng.integers(0, k, (k, 2)) if abs(int(i) - int(j)) > 1]
    for a, ka, b, kb in ((0, 150, 3, 97), (0, 150, LAST, LEAVES), (3, 97, LAST, LEAVES)):
        E += [(a, int(i), b, int(j), 0) for i, j in zip(rng.integers(0, ka, 25), rng.integers(0, kb, 25))]
    for k, deg in enumerate(hubs):
        for i in range(deg):
            leaf = (37 * k + i) % LEAVES  # more incidences than leaves: parallel edges
            E.append((LAST, LEAVES + k, LAST, leaf, 0) if i % 2 == 0 else (LAST, leaf, LAST, LEAVES + k, 0))
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
    if off_so3:  # one measurement rotation off SO(3) by 1e-9: the full 128-B records
        R[m // 2] *= 1.0 + 1e-9
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
    (two chunks, or for a small problem about 736 tiles but at least 180
    incidences; tile_incidences overrides it) and 1.05 x the robot's mean per
    full tile."""
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


def assert_hub_tiles(g, r, hubs, tile_incidences=0):
    tiles = tile_cut(g, r, tile_incidences)
    tail = tiles[-len(hubs):]
    assert [(a, p0, k) for a, p0, k, _ in tail] == [(LAST, LEAVES + i, 1) for i in range(len(hubs))], tail
    assert [c for _, _, _, c in tail] == list(hubs), tail
    assert tiles[-1][1] + 1 == int(g.n_poses[LAST]) and LAST == g.n_robots - 1  # the last tile ends the records
    return tiles


def params(r=5, tcg=10, tile_incidences=0, gradnorm_tol=None):
    P = PGOAgentParameters(r=r)
    lo = P.localOptimizationParams
    lo.RTR_tCG_iterations = tcg
    # (at the default radius of 100 this team's tCG ends at the trust-region
    # boundary in its first step for the first rounds; at 1000 the restatement's
    # step counts are 2 4 1, 5 5 1, 7 6 4, 7 6 10, ... for the robots with tiles)
    lo.RTR_initial_radius, lo.RTR_max_radius = 1e3, 1e6
    P.tileIncidences = tile_incidences
    if gradnorm_tol is not None:
        P.localOptimizationParams.gradnorm_tol = gradnorm_tol
    return P


def start(g, r):
    Y = lifting_matrix(r, seed=1)
    return {a: lift(g.init_R[a], g.init_t[a], Y) for a in range(g.n_robots) if g.n_poses[a]}


def set_form(monkeypatch, form, gate="1"):
    red, groups, decide = form
    monkeypatch.setenv("KMX_RED", red)
    monkeypatch.setenv("KMX_TCG_GROUPS", groups)
    monkeypatch.setenv("KMX_GROUP_RED", "2" if groups != "1" else "0")
    monkeypatch.setenv("KMX_HESS_GATE", gate)
    if decide is None:
        monkeypatch.delenv("KMX_HESS_DECIDE", raising=False)
    else:
        monkeypatch.setenv("KMX_HESS_DECIDE", decide)


def run(monkeypatch, form, g, P, X0, rounds, gate="1", weights_every=4, record_bytes=None):
    """Rounds on a fresh handle in the given form, a GNC weight update every
    `weights_every` rounds: the iterates, the weights, the status words, the
    work counters and every round's per-robot (tCG steps, accepted, updated).
    The robot without poses is left out of the active set: these runs have the
    gradient tolerance at 0, where the forms have always differed about a
    block update over nothing (the launched form's k_reduce runs it and
    reports a status word of NaN, a mean over zero poses; the consumer form
    has no tile to run it on). At any positive tolerance it is skipped in
    every form, which test_hubs_match_oracle covers with the robot active."""
    from kmx.dpgo.solver import BlockSolver
    set_form(monkeypatch, form, gate)
    s = BlockSolver(P, 0)
    try:
        s.set_graph_data(g)
        red, groups, _ = form
        assert s.tcg_groups() == int(groups)
        assert s.group_reduction() == (2 if groups != "1" else int(red))
        if record_bytes is not None:
            assert s.memory()[1] == record_bytes
        for a, X in X0.items():
            s.set_iterate(a, X)
        s.read_counters()
        steps = []
        active = (np.asarray(g.n_poses) > 0).astype(np.uint8)
        for it in range(rounds):
            s.refresh_local()
            st = s.iterate(active)
            steps.append([(x["tcg_iterations"], x["accepted"], x["updated"]) for x in st])
            if it % weights_every == weights_every - 1:
                s.refresh_local()
                s.update_weights()
        c = s.read_counters()
        out = [s.get_iterate(a) for a in sorted(X0)]
        out += [s.get_weights(), s.status(),
                np.array([c["hessvecs"], c["edges_iters"], c["block_updates"], c["gnc_updates"]]), np.array(steps)]
        return out
    finally:
        s.close()


def same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), (what, k)


def against_oracle(monkeypatch, form, g, P, rounds, record_bytes=None):
    """One handle in `form` next to the restatement, checked after every round."""
    from kmx.dpgo.solver import BlockSolver
    from oracle.oracle import OraclePGO
    set_form(monkeypatch, form)
    X0 = start(g, P.r)
    s = BlockSolver(P, 0)
    try:
        s.set_graph_data(g)
        if record_bytes is not None:
            assert s.memory()[1] == record_bytes
        o = OraclePGO(P.to_c(), g)
        for a, X in X0.items():
            s.set_iterate(a, X)
            o.set_iterate(a, X)
        s.refresh_local()
        o.refresh()
        for it in range(rounds):
            s.refresh_local()
            sg, so = s.iterate(), o.iterate()
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


@pytest.fixture(scope="module")
def team():
    g = hub_team(HUBS_R5)
    tiles = assert_hub_tiles(g, 5, HUBS_R5)
    assert_hub_tiles(g, 5, HUBS_R5, 480)
    assert (ISOLATED, 0, 1, 0) in tiles                   # the pose without incidences: a tile with n = 0
    assert all(a != EMPTY for a, _, _, _ in tiles)         # the robot without poses has no tile
    # with 480 incidences per tile the leaves' tiles take two chunks, as the flagship's
    assert max(c for a, _, k, c in tile_cut(g, 5, 480) if k > 1) > chunk(5)
    return g


@pytest.fixture(scope="module")
def refs():
    """The launched single chain's results, computed once per case and left unchanged."""
    return {}


def reference(refs, key, monkeypatch, *a, **kw):
    if key not in refs:
        refs[key] = run(monkeypatch, REFERENCE, *a, **kw)
    return refs[key]


@pytest.mark.parametrize("form", [REFERENCE, ("2", "1", "0"), ("0", "2", "1")])
@pytest.mark.parametrize("tile_incidences", [0, 480])
def test_hubs_match_oracle(gpu, monkeypatch, team, form, tile_incidences):
    """Every hub tile, the empty tile and (480 per tile) two-chunk tiles of
    many poses against the restatement, a weight update inside the run."""
    against_oracle(monkeypatch, form, team, params(tile_incidences=tile_incidences), rounds=10, record_bytes=68)


@pytest.mark.parametrize("tcg", [1, 2, 3, 10])
def test_forms_agree(gpu, monkeypatch, team, refs, tcg):
    """tCG capped at 1, 2, 3 and 10 steps (a first step without delta_old, the
    eta fold at every second step) with the gradient tolerance at 0, so that
    the pose without incidences runs its block update and its tile takes the
    n = 0 path of the epilogue's loads. Every form and both gate settings give
    the launched single chain's bits."""
    g = team
    P = params(tcg=tcg, gradnorm_tol=0.0)
    X0 = start(g, 5)
    ref = reference(refs, ("r5", tcg), monkeypatch, g, P, X0, rounds=8)
    steps = ref[-1][:, :, 0]
    assert (steps[:, ISOLATED] > 0).all(), steps          # the isolated pose's Hess-vec ran in every round
    assert steps.max() == tcg
    if tcg == 10:
        # rounds in which some robots' tCG has stopped while others' runs on:
        # their tiles leave a launch at the gated test or at the decision
        tiled = [a for a in range(g.n_robots) if a not in (ISOLATED, EMPTY)]
        assert sum(len(set(row[tiled])) > 1 for row in steps) >= 3, steps
        assert steps[:, tiled].min() < 10, steps
    same(ref, run(monkeypatch, REFERENCE, g, P, X0, rounds=8, gate="0"), (REFERENCE, "0"))
    for form in FORMS:
        for gate in ("1", "0"):
            same(ref, run(monkeypatch, form, g, P, X0, rounds=8, gate=gate), (form, gate))


@pytest.fixture(scope="module")
def team_full():
    g = hub_team(HUBS_R5, seed=3, off_so3=True)
    assert_hub_tiles(g, 5, HUBS_R5)
    return g


def test_full_records_match_oracle(gpu, monkeypatch, team_full):
    """A measurement rotation off SO(3) by 1e-9 (> 1e-12): the 128-B records,
    whose gather keeps the rows' loads at the top of the chunk."""
    against_oracle(monkeypatch, ("2", "1", "0"), team_full, params(), rounds=6, record_bytes=128)


def test_full_records_forms_agree(gpu, monkeypatch, team_full):
    g = team_full
    P = params(gradnorm_tol=0.0)
    X0 = start(g, 5)
    ref = run(monkeypatch, REFERENCE, g, P, X0, rounds=6, record_bytes=128)
    for form in FORMS:
        same(ref, run(monkeypatch, form, g, P, X0, rounds=6, record_bytes=128), form)


@pytest.mark.parametrize("r", [3, 6])
def test_other_lifts(gpu, monkeypatch, r):
    """r = 3 (a chunk of 252) and r = 6 (240): hubs of exactly one chunk and
    one chunk plus one incidence, against the restatement and across forms."""
    ch = chunk(r)
    assert ch == {3: 252, 6: 240}[r]
    hubs = (ch, ch + 1)
    g = hub_team(hubs, seed=r)
    assert_hub_tiles(g, r, hubs)
    against_oracle(monkeypatch, ("2", "1", "0"), g, params(r=r), rounds=6, record_bytes=68)
    P = params(r=r, gradnorm_tol=0.0)
    X0 = start(g, r)
    ref = run(monkeypatch, REFERENCE, g, P, X0, rounds=6)
    for form in FORMS:
        same(ref, run(monkeypatch, form, g, P, X0, rounds=6), form)
