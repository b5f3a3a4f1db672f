"""k_traj (kmx_pgo_get_trajectory) and the Stiefel projection of the accelerated
rounds (group_project, through KMX_EVAL_PROJECT) against the mpmath SVD truth of
tests/golden/rounding_ref.npz, under the bounds of tests/rounding_ref.py: every
singular value ratio down to 1e-16, both determinant signs, off-manifold
scales, and exact rank 2, 1 and 0.

Worst device ratios observed on an MI355X (of the allowed K_R = 48.7,
K_O = 44, K_P = 27.5, translation 1): rotation 3.6, orthogonality 7, polar
factor 1.02, translation 0.02.
"""
import numpy as np
import pytest

from kmx import abi
from kmx.dpgo.params import PGOAgentParameters
from kmx.dpgo.solver import BlockSolver
from tests import rounding_ref as REF

pytestmark = pytest.mark.gpu


def _handle(r, X):
    s = BlockSolver(PGOAgentParameters(r=r), 0)
    s.set_graph_data(REF.chain_graph(X.shape[0]))
    s.set_iterate(0, X)
    return s


def _trajectory(s, c, n, K):
    """The first n poses' rounding, each against its own anchor; every anchor
    is applied to every pose (the rotation property holds for all of them), and
    a second call returns the same bits."""
    traj = np.empty((n, 12))
    for g in range(c.anchors.shape[0]):
        full = s.trajectory(0, c.anchors[g])
        REF.assert_rotations(full, K, f"device, anchor {g}")
        assert np.array_equal(full, s.trajectory(0, c.anchors[g]))
        traj[c.aid[:n] == g] = full[c.aid[:n] == g]
    return traj


@pytest.mark.parametrize("r,n", [(3, None), (4, None), (5, None), (8, None), (5, 1), (5, 127), (5, 128), (5, 129)])
def test_trajectory_against_svd(gpu, r, n):
    """n = None: all of the rank's poses (300 at r = 5); k_traj runs 128
    threads per block, hence 1, 127, 128, 129."""
    cases, K = REF.load()
    c = cases[r]
    n = c.n if n is None else n
    s = _handle(r, c.X[:n])
    traj = _trajectory(s, c, n, K)
    s.close()
    sub = c if n == c.n else REF.Case(r, _first(c, n))
    REF.check_trajectory(sub, traj, K, "device")


def _first(c, n):
    keep = c.deg < n
    out = {k: getattr(c, k)[:n] for k in REF.FIELDS if k not in ("anchors", "deg", "deg_U", "deg_V", "deg_pV")}
    out.update(anchors=c.anchors, deg=c.deg[keep], deg_U=c.deg_U[keep], deg_V=c.deg_V[keep], deg_pV=c.deg_pV[keep])
    return out


@pytest.mark.parametrize("r", REF.RANKS)
def test_projection_against_svd(gpu, r):
    """KMX_EVAL_PROJECT runs the device function the accelerated rounds run
    (group_project in k_accel and in k_eval): the fixture's Yi as V."""
    cases, K = REF.load()
    c = cases[r]
    s = _handle(r, c.X)
    out, _ = s.eval(0, abi.KMX_EVAL_PROJECT, c.X)
    again, _ = s.eval(0, abi.KMX_EVAL_PROJECT, c.X)
    s.close()
    assert np.array_equal(out, again)
    REF.check_projection(c, out, K, "device")
