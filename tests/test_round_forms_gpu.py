"""Combinations of the round's forms that share one enqueue function.

A round is enqueued over one launch chain or over several robot groups, in
the launched or the consumer reduction form; timing, RGD and the one-sync tCG
run on one chain only, whatever KMX_TCG_GROUPS asks for. Neither the number of
chains nor the reduction form changes a robot's arithmetic, so every
comparison here is np.array_equal against a fresh handle of the plain form:
every robot's iterate, the GNC weights, the status words and the work
counters. Blind enqueueing wherever the polling mode is not the subject.
"""
import numpy as np
import pytest

from kmx.dpgo.params import ROptMethod
from kmx.dpgo.solver import BlockSolver
from tests.test_tcg_groups_gpu import _graph, _params, _same, _start

pytestmark = pytest.mark.gpu

ENV = ("KMX_RED", "KMX_TCG_GROUPS", "KMX_GROUP_RED")


def _run(monkeypatch, env, g, P, X0, *, calls=((5, False),), poll=0, groups=1):
    """Rounds on a fresh handle created under `env` (a switch it does not name
    is unset). calls: (rounds, timing on) per iterate_async call; an untimed
    call must run `groups` chains, a timed one runs one and must report k_hess
    launches. Returns what test_tcg_groups_gpu._run returns, the counters
    summed over the calls."""
    for k in ENV:
        if k in env:
            monkeypatch.setenv(k, str(env[k]))
        else:
            monkeypatch.delenv(k, raising=False)
    s = BlockSolver(P, 0)
    try:
        s.set_tcg_poll(poll)
        s.set_graph_data(g)
        s.set_gnc_schedule(True, 3, 50, P.relChangeTol)
        for a in range(g.n_robots):
            if g.n_poses[a]:
                s.set_iterate(a, X0[a])
        s.read_counters()
        work = np.zeros(4, dtype=np.int64)
        for k, (n, timed) in enumerate(calls):
            s.enable_timing(timed)
            assert s.tcg_groups() == (1 if timed else groups), (s.tcg_groups(), timed, groups)
            s.iterate_async(n, refresh_local=k == 0)
            s.sync()
            c = s.read_counters()
            assert not timed or c["hessvec_launches"] > 0, c
            work += [c["hessvecs"], c["edges_iters"], c["block_updates"], c["gnc_updates"]]
        assert work[0] > 0 or P.localOptimizationParams.method == ROptMethod.RGD, work
        assert work[2] > 0, work
        out = [s.get_iterate(a) for a in range(g.n_robots) if g.n_poses[a]]
        return out + [s.get_weights(), s.status(), work]
    finally:
        s.close()


@pytest.fixture(scope="module")
def team3():
    g = _graph([300, 210, 260], seed=6)
    return g, _start(g, seed=6)


@pytest.fixture(scope="module")
def refs():
    """Reference results, computed once per case and left unchanged."""
    return {}


def _ref(refs, key, *a, **kw):
    if key not in refs:
        refs[key] = _run(*a, **kw)
    return refs[key]


@pytest.mark.parametrize("red", [0, 2])
def test_rgd_with_groups_asked_for(gpu, monkeypatch, team3, red):
    """RGD has no tCG to overlap: one chain in either reduction form, and the
    bits of the handle that was asked for one."""
    g, X0 = team3
    P = _params()
    P.localOptimizationParams.method = ROptMethod.RGD
    P.localOptimizationParams.RGD_stepsize = 1e-4
    ref = _run(monkeypatch, {"KMX_RED": red, "KMX_TCG_GROUPS": 1}, g, P, X0)
    _same(ref, _run(monkeypatch, {"KMX_RED": red, "KMX_TCG_GROUPS": 2}, g, P, X0))


@pytest.mark.parametrize("group_red", [0, 2])
def test_onesync_with_groups_asked_for(gpu, monkeypatch, team3, refs, group_red):
    """The one-sync tCG runs its k_step loop on one chain, whatever form the
    groups would take."""
    g, X0 = team3
    P = _params()
    P.localOptimizationParams.tCG_form = "onesync"
    ref = _ref(refs, "onesync", monkeypatch, {"KMX_TCG_GROUPS": 1}, g, P, X0)
    _same(ref, _run(monkeypatch, {"KMX_TCG_GROUPS": 2, "KMX_GROUP_RED": group_red}, g, P, X0))


@pytest.mark.parametrize("group_red", [0, 2])
def test_timing_toggled_on_one_handle(gpu, monkeypatch, team3, refs, group_red):
    """Two grouped rounds, two timed ones (one chain, launched form), two
    grouped again, polled adaptively with a tCG cap of 3: the polled loops run
    to the cap and open blind windows, in the groups' polling states and in
    the single chain's, which are kept apart."""
    g, X0 = team3
    P = _params(tcg=3)
    ref = _ref(refs, "timing", monkeypatch, {"KMX_RED": 0, "KMX_TCG_GROUPS": 1}, g, P, X0, calls=((6, False),),
               poll=-1)
    got = _run(monkeypatch, {"KMX_RED": 0, "KMX_TCG_GROUPS": 2, "KMX_GROUP_RED": group_red}, g, P, X0,
               calls=((2, False), (2, True), (2, False)), poll=-1, groups=2)
    _same(ref, got)


@pytest.mark.parametrize("tcg", [1, 10])
def test_two_rtr_iterations_on_one_chain(gpu, monkeypatch, team3, tcg):
    """RTR_iterations = 2 on one chain: a non-final k_commit over all tiles
    between the iterations, and the trial cost keeps its reduction (a k_reduce
    launch in either form); launched against consumer."""
    g, X0 = team3
    P = _params(tcg=tcg, rtr=2)
    ref = _run(monkeypatch, {"KMX_RED": 0, "KMX_TCG_GROUPS": 1}, g, P, X0)
    _same(ref, _run(monkeypatch, {"KMX_RED": 2, "KMX_TCG_GROUPS": 1}, g, P, X0))


def test_robot_without_tiles_on_one_chain(gpu, monkeypatch):
    """Robot 1 has no poses, hence no tiles: the polled single chain never
    waits for it, in either reduction form."""
    g = _graph([300, 0, 250], seed=3)
    X0 = _start(g, seed=3)
    P = _params()
    ref = _run(monkeypatch, {"KMX_RED": 0, "KMX_TCG_GROUPS": 1}, g, P, X0, poll=1)
    _same(ref, _run(monkeypatch, {"KMX_RED": 2, "KMX_TCG_GROUPS": 1}, g, P, X0, poll=1))
