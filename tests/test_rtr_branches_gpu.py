"""The failure side of the dpgo round on the GPU: rejected and skipped RTR steps.

The inputs of tests/rtr_cases.py make the restatement reject steps, leave tCG
through negative curvature, shrink, grow and clamp the radius, and skip a later
RTR iteration on the gradient norm (test_rtr_branches_cpu.py asserts that they
do). Here the HIP path runs them, in synchronous rounds (refresh_local +
iterate) next to the restatement, per round and robot:

  tcg_iterations, tcg_stop, accepted, updated, hessvecs   equal
  radius                                                  equal (x 0.25, x 2 and
                                                          fmin are exact)
  f_init, f_final                                         1e-9 max(1, |f|)
  rel_change                                              1e-9
  poses                                                   1e-6 Frobenius per pose
  rho                                                     RHO_TOL max(1, |rho|)

RHO_TOL: the restatement against itself, serial against its all-cores variant
(iterate(threads=2, inner=2), whose sums are grouped differently), differs in
rho by at most s = 6.2e-11 relative to max(1, |rho|) over A-F (A: 6.2e-11, D:
3.9e-12, F: 4.4e-13, B: 2.0e-13, the others below 1e-13); RHO_TOL =
max(100 s, 1e-9) = 6.2e-9. No decision sits on a threshold: every rho the
restatement reports is at least 1e-3 away from 0.25, 0.75 and RTR_accept_rho.

Public rows: kmx_pgo_iterate_async promises that every round republishes the
rows it commits. After each synchronous round the public table is read, then
refresh_local() is called and the table read again: bitwise equal, on the
inputs where a block update moves and its last RTR iteration is rejected (A,
B, D) or skipped (E), and on an all-accepted control. The asynchronous form
(one iterate_async call for all rounds) must reach the restatement's and the
synchronous rounds' poses.

Forms: A and C under the default form, KMX_RED=0, KMX_TCG_TAIL=0 and two robot
groups with launched and with consumer reductions; groups only take effect
where the single chain would be launched, so those two set KMX_RED=0 as
test_tcg_tail_gpu does, and the handle's getters say which form ran (KMX_RED=0
alone leaves the number of chains to the handle). A also in the one-sync tCG
form.
"""
import numpy as np
import pytest

from kmx.dpgo.solver import BlockSolver
from tests import rtr_cases as rc

pytestmark = pytest.mark.gpu

RHO_TOL = rc.RHO_TOL

ENV = ("KMX_RED", "KMX_TCG_TAIL", "KMX_TCG_GROUPS", "KMX_GROUP_RED")
FORMS = {
    "default": {},
    "launched": {"KMX_RED": "0"},
    "tail0": {"KMX_TCG_TAIL": "0"},
    "groups_launched": {"KMX_RED": "0", "KMX_TCG_GROUPS": "2", "KMX_GROUP_RED": "0"},
    "groups_consumer": {"KMX_RED": "0", "KMX_TCG_GROUPS": "2", "KMX_GROUP_RED": "2"},
}
MOVED = ("A", "B", "D", "E")  # a move, then a rejected or skipped last iteration


def _handle(monkeypatch, form, g, P, X0):
    env = FORMS[form]
    for k in ENV:
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)
    s = BlockSolver(P, 0)
    s.set_graph_data(g)
    if "KMX_TCG_GROUPS" in env:
        assert s.tcg_groups() == 2, s.tcg_groups()
        assert s.group_reduction() == int(env["KMX_GROUP_RED"]), s.group_reduction()
    elif "KMX_RED" not in env:  # 90 poses: by default one chain in the consumer form
        assert s.tcg_groups() == 1, s.tcg_groups()
    for a in range(g.n_robots):
        s.set_iterate(a, X0[a])
    return s


def _pose_diff(X, Y, r):
    return np.linalg.norm((X - Y).reshape(-1, 4 * r), axis=1).max()


def _sync_rounds(monkeypatch, case, form, public=False):
    """Synchronous rounds of one handle next to the restatement's recorded
    ones; with `public`, the republished rows after every round instead of
    the statistics. Returns the final iterates."""
    g, P, X0, rounds = rc.build(case)
    ora = rc.oracle_rounds(case)
    accept = P.localOptimizationParams.RTR_accept_rho
    s = _handle(monkeypatch, form, g, P, X0)
    try:
        s.refresh_local()
        for it, rec in enumerate(ora):
            sg, so = s.iterate(), rec["st"]
            if public:
                before = s.get_public()[0].copy()
                assert before.size > 0
            s.refresh_local()
            if public:
                assert np.array_equal(before, s.get_public()[0]), (case, it, np.abs(before - s.get_public()[0]).max())
                continue
            for a in range(g.n_robots):
                x, o = sg[a], so[a]
                where = (case, form, it, a, x, o)
                assert rc.rho_off_thresholds(o, accept), where
                for k in ("tcg_iterations", "tcg_stop", "accepted", "updated", "hessvecs"):
                    assert x[k] == o[k], (k,) + where
                assert x["radius"] == o["radius"], where
                for k in ("f_init", "f_final"):
                    assert abs(x[k] - o[k]) <= 1e-9 * max(1.0, abs(o[k])), (k,) + where
                assert abs(x["rel_change"] - o["rel_change"]) <= 1e-9, where
                assert abs(x["rho"] - o["rho"]) <= RHO_TOL * max(1.0, abs(o["rho"])), where
                d = _pose_diff(s.get_iterate(a), rec["X"][a], P.r)
                assert d <= 1e-6, (d,) + where
                if case in ("C", "Cp"):
                    assert x["rel_change"] == 0.0 and x["f_final"] == x["f_init"], where
        out = [s.get_iterate(a) for a in range(g.n_robots)]
        if case in ("C", "Cp"):  # every step rejected: the iterate never moves
            for a in range(g.n_robots):
                assert np.array_equal(out[a], X0[a]), (case, form, a)
        return out
    finally:
        s.close()


@pytest.mark.parametrize("case", rc.ALL + ("A1",))
def test_sync_rounds_match_restatement(gpu, monkeypatch, case):
    _sync_rounds(monkeypatch, case, "default")


@pytest.mark.parametrize("form", [f for f in FORMS if f != "default"])
@pytest.mark.parametrize("case", ["A", "C"])
def test_forms_match_restatement(gpu, monkeypatch, case, form):
    """C matters most under the consumer forms: with one RTR iteration the
    folded k_commit takes the reject decision per tile."""
    _sync_rounds(monkeypatch, case, form)


@pytest.mark.parametrize("case", MOVED + ("OK",))
def test_round_republishes_moved_rows(gpu, monkeypatch, case):
    """A robot whose block update moved X in an earlier RTR iteration and whose
    last iteration was rejected or skipped still publishes its rows."""
    _sync_rounds(monkeypatch, case, "default", public=True)


@pytest.mark.parametrize("form", ["default", "groups_launched"])
@pytest.mark.parametrize("case", MOVED)
def test_async_rounds_match_restatement(gpu, monkeypatch, case, form):
    """All rounds in one iterate_async call: from round 2 on the robots read
    what the round before published, with no refresh_local in between."""
    g, P, X0, rounds = rc.build(case)
    ora = rc.oracle_rounds(case)
    s = _handle(monkeypatch, form, g, P, X0)
    try:
        s.iterate_async(rounds, refresh_local=True)
        s.sync()
        got = [s.get_iterate(a) for a in range(g.n_robots)]
    finally:
        s.close()
    sync = _final_sync(monkeypatch, case, form)
    for a in range(g.n_robots):
        d = _pose_diff(got[a], ora[-1]["X"][a], P.r)
        assert d <= 1e-6, (case, "restatement", a, d)
        d = _pose_diff(got[a], sync[a], P.r)
        assert d <= 1e-6, (case, "sync", a, d)


def _final_sync(monkeypatch, case, form):
    """The synchronous rounds' final iterates (refresh_local before each)."""
    g, P, X0, rounds = rc.build(case)
    s = _handle(monkeypatch, form, g, P, X0)
    try:
        for _ in range(rounds):
            s.refresh_local()
            s.iterate()
        return [s.get_iterate(a) for a in range(g.n_robots)]
    finally:
        s.close()
