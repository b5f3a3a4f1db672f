"""The consumer round's tail without k_retract: the shapes at which it can go wrong.

In the consumer reduction form the k_update of the host's launch tcg_max - 1
(pgo.hip k_update_last, body_update's LAST) finds a robot still in tCG at the
step cap. It forms no z, goes on to the robot's trial point with this launch's
coefficient as the last direction's, and leaves the stop reason from ||r||^2
to k_cost, whose first tile of the robot writes it. KMX_TCG_TAIL=0 keeps the
earlier launches (an ordinary last k_update, k_retract's fold 2). Nothing in
the arithmetic moves, so each case is checked two ways:

* against the restatement at the project's bar: equal tCG step counts, stop
  reasons, acceptance and update flags, poses within 1e-6, weights within 1e-9;
* bit for bit (np.array_equal on iterates, weights, status, counters, steps
  and stop reasons) against the launched single chain (KMX_RED=0,
  KMX_TCG_GROUPS=1), which keeps k_retract, and between KMX_TCG_TAIL=0 and the
  default.

Forms crossed: the consumer single chain (KMX_RED=2) and the grouped consumer
round (KMX_TCG_GROUPS=2, KMX_GROUP_RED=2), each blind (set_tcg_poll 0), polled
(1) and adaptive (-1) with the new tail, and adaptive with KMX_TCG_TAIL=0.

The team is test_update_occupancy_gpu's: robots of 150, 97, 1, 0 and 400 poses
(short tiles, a one-pose tile without edges, a robot without tiles). The
settings at which a stop lands exactly on the cap were found with the
restatement on the CPU and are fixed here; each test asserts from the stop
reasons that its run shows what it is about.
"""
import numpy as np
import pytest

from kmx.dpgo.params import PGOAgentParameters  # noqa: F401  (the helpers' parameters)
from tests.test_update_occupancy_gpu import (BOUNDARY, EMPTY, ISOLATED, REFERENCE, same, set_form, start, team_graph,
                                             tile_cut)
from tests.test_update_occupancy_gpu import params as base_params

pytestmark = pytest.mark.gpu

CONSUMER = [("2", "1"), ("0", "2")]  # (KMX_RED, KMX_TCG_GROUPS): single chain, two groups
POLLS = (0, 1, -1)                   # blind, polled, adaptive
RESIDUAL = ("linear", "superlinear")
COST_SUM_TILES = 2 * 256             # RobotSum<2> in k_cost: two tiles per thread of a 256-thread workgroup


def params(kappa=None, rtr=1, **kw):
    P = base_params(**kw)
    if kappa is not None:
        P.localOptimizationParams.tCG_kappa = kappa
    P.localOptimizationParams.RTR_iterations = rtr
    return P


def run(monkeypatch, form, tail, poll, g, P, X0, rounds):
    """test_update_occupancy_gpu.run with the tail switch and the polling
    mode: rounds on a fresh handle, a weight update every fourth round."""
    from kmx.dpgo.solver import BlockSolver
    set_form(monkeypatch, form)
    if tail is None:
        monkeypatch.delenv("KMX_TCG_TAIL", raising=False)
    else:
        monkeypatch.setenv("KMX_TCG_TAIL", tail)
    s = BlockSolver(P, 0)
    try:
        s.set_tcg_poll(poll)
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
            if it % 4 == 3:
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


def bitwise(monkeypatch, g, P, r, rounds):
    """The launched single chain's results, and every consumer form, polling
    mode and tail equal to them bit for bit. Returns the reference's per-round
    steps and stop reasons."""
    X0 = start(g, r)
    ref = run(monkeypatch, REFERENCE, None, -1, g, P, X0, rounds)
    for form in CONSUMER:
        for poll in POLLS:
            same(ref, run(monkeypatch, form, None, poll, g, P, X0, rounds), (form, "tail", poll))
        same(ref, run(monkeypatch, form, "0", -1, g, P, X0, rounds), (form, "KMX_TCG_TAIL=0"))
    return ref[-2][:, :, 0], ref[-1]


def oracle_rounds(g, P, rounds):
    """The restatement's rounds from the lifted start: its state after every
    round (iterates, weights where updated) and the per-robot statistics.
    Runs on the CPU; computed once per case."""
    from oracle.oracle import OraclePGO
    o = OraclePGO(P.to_c(), g)
    for a, X in start(g, P.r).items():
        o.set_iterate(a, X)
    o.refresh()
    out = []
    for it in range(rounds):
        st = o.iterate()
        rec = {"st": st, "X": {a: o.get_iterate(a).copy() for a in range(g.n_robots) if g.n_poses[a]}}
        if it % 4 == 3:
            rec["mu"] = o.update_weights()
            rec["w"] = o.get_weights().copy()
        out.append(rec)
    return out


def against_oracle(monkeypatch, form, poll, g, P, ora):
    """One handle in `form` (new tail) next to the restatement's recorded
    rounds, checked after every round, stop reasons included."""
    from kmx.dpgo.solver import BlockSolver
    set_form(monkeypatch, form)
    monkeypatch.delenv("KMX_TCG_TAIL", raising=False)
    s = BlockSolver(P, 0)
    try:
        s.set_tcg_poll(poll)
        s.set_graph_data(g)
        for a, X in start(g, P.r).items():
            s.set_iterate(a, X)
        s.refresh_local()
        for it, rec in enumerate(ora):
            s.refresh_local()
            sg, so = s.iterate(), rec["st"]
            for a in range(g.n_robots):
                assert sg[a]["updated"] == so[a]["updated"], (it, a)
                assert sg[a]["tcg_iterations"] == so[a]["tcg_iterations"], (it, a, sg[a], so[a])
                assert sg[a]["accepted"] == so[a]["accepted"], (it, a)
                if g.n_poses[a]:
                    # (a robot without poses has no tile, so no launch writes a
                    # reason for it: the handle reports "none" where the
                    # restatement says "skipped", in every form)
                    assert sg[a]["tcg_stop"] == so[a]["tcg_stop"], (it, a, sg[a], so[a])
                    d = np.linalg.norm((s.get_iterate(a) - rec["X"][a]).reshape(-1, 4 * P.r), axis=1).max()
                    assert d <= 1e-6, (it, a, d)
            if "w" in rec:
                s.refresh_local()
                assert s.update_weights() == rec["mu"]
                assert np.abs(s.get_weights() - rec["w"]).max() <= 1e-9
    finally:
        s.close()


def oracle_case(monkeypatch, g, P, rounds):
    """Both consumer forms against the restatement (the single chain blind,
    the groups adaptive); returns its per-round (steps, stop) per robot."""
    ora = oracle_rounds(g, P, rounds)
    against_oracle(monkeypatch, CONSUMER[0], 0, g, P, ora)
    against_oracle(monkeypatch, CONSUMER[1], -1, g, P, ora)
    return [[(x["tcg_iterations"], x["tcg_stop"]) for x in rec["st"]] for rec in ora]


TILED = (0, 1, 4)  # the robots with more than one pose


@pytest.fixture(scope="module")
def team():
    g = team_graph([150, 97, 1, 0, 400])
    tiles = tile_cut(g, 5)
    assert (ISOLATED, 0, 1, 0) in tiles
    assert all(a != EMPTY for a, _, _, _ in tiles)
    assert any(1 < k < 48 for _, _, k, _ in tiles) and len(tiles) > 8
    return g


@pytest.mark.parametrize("tcg", [1, 2, 3, 10])
def test_caps(gpu, monkeypatch, team, tcg):
    """tCG capped at 1 (the last launch is also the first, which reads g for
    r), 2 and 3 (the eta fold on either parity) and 10 (the workload's), the
    gradient tolerance at 0 so that the one-pose tile runs too. In each run a
    robot reaches the cap without passing a stop test (the trial point of
    k_update_last, the reason from k_cost) and a robot ends at a stop test
    (the trial point of the k_update behind the k_hess that stopped it, or of
    k_update_last on the boundary). For caps above 1 some robot stops before
    the cap and the robots of one round leave at different steps; at a cap of
    1 every robot's only step is the cap, so there the stop test is the
    boundary test of that step."""
    g = team
    oracle_case(monkeypatch, g, params(tcg=tcg), rounds=8)
    steps, stops = bitwise(monkeypatch, g, params(tcg=tcg, gradnorm_tol=0.0), 5, rounds=8)
    tiled = list(TILED)
    at_cap = (steps[:, tiled] == tcg) & (stops[:, tiled] == "max_iterations")
    tested = np.isin(stops[:, tiled], BOUNDARY + RESIDUAL)
    assert at_cap.any(), (steps, stops)
    assert tested.any(), (steps, stops)
    if tcg > 1:
        assert (tested & (steps[:, tiled] < tcg)).any(), (steps, stops)
        assert any(len(set(row)) > 1 and row.max() == tcg for row in steps[:, tiled]), steps


def test_boundary_at_the_cap(gpu, monkeypatch, team):
    """A radius of 1e3 and a cap of 3: in the first round robot 1's third step,
    its last allowed one, ends on the trust-region boundary (found with the
    restatement). k_update_last then takes tau as the last direction's
    coefficient and writes no ||r||^2; k_cost keeps the boundary reason."""
    g = team
    ora = oracle_case(monkeypatch, g, params(tcg=3, radius=1e3), rounds=4)
    assert ora[0][1] == (3, "exceeded_trust_region"), ora
    steps, stops = bitwise(monkeypatch, g, params(tcg=3, radius=1e3, gradnorm_tol=0.0), 5, rounds=4)
    assert ((steps == 3) & np.isin(stops, BOUNDARY)).any(), (steps, stops)


def test_residual_test_passes_at_the_cap(gpu, monkeypatch, team):
    """tCG kappa 0.2 and a cap of 3: in the fifth round robots 0 and 1 pass the
    residual test exactly at step 3 (found with the restatement). The reason
    is then the residual test's, not the iteration limit: upd_step tests the
    residual first, and k_cost's decision must keep that order."""
    g = team
    P = params(tcg=3, kappa=0.2)
    ora = oracle_case(monkeypatch, g, P, rounds=6)
    assert ora[4][0] == (3, "linear") and ora[4][1] == (3, "linear"), ora
    assert any(n == 3 and s == "max_iterations" for row in ora for n, s in row), ora
    steps, stops = bitwise(monkeypatch, g, P, 5, rounds=6)
    assert ((steps == 3) & np.isin(stops, RESIDUAL)).any(), (steps, stops)
    assert ((steps == 3) & (stops == "max_iterations")).any(), (steps, stops)


def test_precond_off(gpu, monkeypatch, team):
    """Without the preconditioner z = r: the ordinary update stores z and
    <z, r>, the last one neither."""
    g = team
    ora = oracle_case(monkeypatch, g, params(tcg=3, precond=False), rounds=5)
    assert any(n == 3 and s == "max_iterations" for row in ora for n, s in row), ora
    bitwise(monkeypatch, g, params(tcg=3, precond=False, gradnorm_tol=0.0), 5, rounds=5)


@pytest.mark.parametrize("r", [3, 6])
def test_other_lifts(gpu, monkeypatch, r):
    """r = 3 (21 poses per wave, one idle lane) and r = 6 (10 per wave, four
    idle lanes) at a cap of 3."""
    g = team_graph([150, 97, 1, 0, 400], seed=r)
    ora = oracle_case(monkeypatch, g, params(r=r, tcg=3), rounds=5)
    assert any(n == 3 and s == "max_iterations" for row in ora for n, s in row), ora
    bitwise(monkeypatch, g, params(r=r, tcg=3, gradnorm_tol=0.0), r, rounds=5)


def test_two_rtr_iterations(gpu, monkeypatch, team):
    """Two RTR iterations per block update: k_cost is followed by k_reduce
    (which reads the phase k_cost's first tile wrote) and a non-final commit,
    and the second iteration's tCG starts from a state k_update_last left."""
    g = team
    ora = oracle_case(monkeypatch, g, params(tcg=3, rtr=2), rounds=4)
    assert any(n == 3 and s == "max_iterations" for row in ora for n, s in row), ora
    bitwise(monkeypatch, g, params(tcg=3, rtr=2, gradnorm_tol=0.0), 5, rounds=4)


def test_robot_of_many_tiles(gpu, monkeypatch):
    """A robot of 1,100 one-pose tiles at the cap: more tiles than the
    register form of k_cost's robot sum (two per thread) and of k_update's
    (four per thread) hold, so both fall back to the loop. Over six rounds
    that robot ends at the cap on the boundary, by the residual test and by
    the iteration limit (found with the restatement)."""
    g = team_graph([150, 1100, 97], seed=5, ring=(1, 4))
    tiles = tile_cut(g, 5, 16)
    per_robot = [sum(1 for a, _, _, _ in tiles if a == b) for b in range(3)]
    assert per_robot[1] == 1100 > 2 * COST_SUM_TILES, per_robot
    ora = oracle_case(monkeypatch, g, params(tcg=3, tile_incidences=16), rounds=6)
    assert [row[1] for row in ora[3:]] == [(3, "exceeded_trust_region"), (3, "linear"), (3, "max_iterations")], ora
    steps, stops = bitwise(monkeypatch, g, params(tcg=3, tile_incidences=16, gradnorm_tol=0.0), 5, rounds=6)
    assert ((steps[:, 1] == 3) & (stops[:, 1] == "max_iterations")).any(), (steps, stops)
