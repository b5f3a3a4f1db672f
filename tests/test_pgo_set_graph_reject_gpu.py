"""kmx_pgo_set_graph plans the graph on the host before it touches the handle:
a rejected graph leaves the handle's graph, iterate and public table as they
were, and the rounds after it produce the bits of a handle that never saw it."""
import numpy as np
import pytest

from kmx import abi
from kmx.abi import fptr, iptr, u8ptr
from kmx.dpgo.params import PGOAgentParameters
from kmx.dpgo.solver import BlockSolver
from kmx.synth import lift, lifting_matrix, make_pose_graph

pytestmark = pytest.mark.gpu


def _raw_set_graph(s, g, local, p1=None):
    """The ABI call itself (BlockSolver.set_graph records the team before it
    calls), so the Python object keeps describing the graph in force."""
    i32 = [np.ascontiguousarray(x, dtype=np.int32) for x in (g.n_poses, g.r1, g.p1 if p1 is None else p1, g.r2, g.p2)]
    f64 = [np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1)) for x in (g.R, g.t, g.kappa, g.tau, g.weight)]
    lo = np.ascontiguousarray(local, dtype=np.uint8)
    fx = np.ascontiguousarray(g.fixed, dtype=np.uint8)
    return s.L.kmx_pgo_set_graph(s.h, int(g.n_robots), iptr(i32[0]), u8ptr(lo), int(g.m), iptr(i32[1]), iptr(i32[2]),
                                 iptr(i32[3]), iptr(i32[4]), *[fptr(x) for x in f64], u8ptr(fx))


def _state(s, n_robots):
    return [s.get_iterate(a) for a in range(n_robots)], s.public_count(), s.memory()


def test_rejected_graph_leaves_the_handle_alone(gpu):
    g = make_pose_graph(2, 100, 300, seed=3)
    P = PGOAgentParameters(r=5)
    Y = lifting_matrix(5, seed=1)
    pair = [BlockSolver(P, 0), BlockSolver(P, 0)]  # [0] sees the bad calls, [1] never does
    for s in pair:
        s.set_graph_data(g)
        for a in range(2):
            s.set_iterate(a, lift(g.init_R[a], g.init_t[a], Y))
        for _ in range(2):
            s.refresh_local()
            s.iterate()
    s = pair[0]
    X, pub, mem = _state(s, 2)
    assert pub[0] > 0

    p1 = np.array(g.p1, dtype=np.int32)
    p1[g.m // 2] = g.n_poses[g.r1[g.m // 2]]  # one pose id out of range
    g3 = make_pose_graph(3, 150, 450, seed=4)
    assert all(np.any((g3.r1 != g3.r2) & ((g3.r1 == a) | (g3.r2 == a))) for a in range(3))  # each holds public poses
    for call, want, text in ((lambda: _raw_set_graph(s, g, [1, 1], p1=p1), abi.KMX_EINVAL, "edge pose id out of range"),
                             (lambda: _raw_set_graph(s, g3, [1, 0, 1]), abi.KMX_EUNSUP,
                              "contiguous range of the public table")):
        assert call() == want
        assert text in s.L.kmx_last_error().decode()
        X1, pub1, mem1 = _state(s, 2)
        assert pub1 == pub and mem1 == mem
        assert all(np.array_equal(a, b) for a, b in zip(X, X1))

    for q in pair:
        q.refresh_local()
        q.iterate()
    for a in range(2):
        assert np.array_equal(pair[0].get_iterate(a), pair[1].get_iterate(a))
    assert np.array_equal(pair[0].get_public()[0], pair[1].get_public()[0])
    assert np.array_equal(pair[0].get_weights(), pair[1].get_weights())
    for q in pair:
        q.close()
