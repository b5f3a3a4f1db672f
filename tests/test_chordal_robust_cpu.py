"""Robust chordal initialisation (kmx_chordal_residuals,
kmx_chordal_solve_robust), the part that needs no device: the header declares
the entry points, the library exports them and kmx/abi.py binds them, the
structs have the header's size, the ABI version is unchanged, the wrappers
refuse wrong shapes and dtypes before the library is called, and the host
mirror kmx.dpgo.init.robust_chordal_initialization (the rule the device
implements, and the reference of its tests) rejects the outliers of the
project's own generator."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]

SYMBOLS = ("kmx_chordal_residuals", "kmx_chordal_solve_robust")


def test_symbols_declared_exported_and_bound():
    from kmx import abi
    L = abi.lib()
    hdr = (ROOT / "include" / "kmx_abi.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(kmx_\w+)\s*\(", hdr, re.M))
    for name in SYMBOLS + ("kmx_chordal_get_robust_stats",):
        assert name in declared, name
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name  # bound in kmx/abi.py


def test_structs_match_the_header_and_the_abi_version_is_10():
    import ctypes as C

    from kmx import abi
    assert C.sizeof(abi.ChordalRobustParams) == 32
    assert C.sizeof(abi.ChordalRobustInfo) == 32
    assert abi.ChordalRobustParams.max_updates.offset == 24 and abi.ChordalRobustInfo.mu.offset == 24
    hdr = (ROOT / "include" / "kmx_abi.h").read_text()
    assert int(re.search(r"#define\s+KMX_ABI_VERSION\s+(\d+)", hdr).group(1)) == 10
    assert abi.ABI_VERSION == 10
    assert abi.lib().kmx_abi_version() == 10


class _NoLibrary:
    """A ChordalSolver's fields without a handle: any library call fails."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def _solver(n=4, m=3, nb=1):
    from kmx.dpgo.chordal import ChordalSolver
    s = ChordalSolver.__new__(ChordalSolver)
    s.L, s.h, s.n, s.n_blocks, s.m = _NoLibrary(), None, n, nb, m
    return s


@pytest.mark.parametrize("kw", [
    dict(R=np.zeros((4, 9))),
    dict(R=np.zeros((3, 3, 3))),
    dict(R=np.zeros((4, 3, 3), np.complex128)),
    dict(t=np.zeros((4, 4))),
    dict(t=np.zeros(12)),
    dict(mu=np.ones(2)),
    dict(mu=np.array(["a"])),
    dict(fixed=np.zeros(4, bool)),
    dict(fixed=np.zeros((3, 1), bool)),
    dict(fixed=np.zeros(3)),           # floats are no mask
    dict(barc=-1.0),
    dict(barc=float("nan")),
])
def test_residuals_refuses_without_a_device(kw):
    a = dict(R=np.zeros((4, 3, 3)), t=np.zeros((4, 3)), mu=np.ones(1), barc=5.0, fixed=np.zeros(3, bool))
    a.update(kw)
    with pytest.raises(ValueError):
        _solver().residuals(**a)


@pytest.mark.parametrize("kw", [
    dict(fixed=np.zeros(2, bool)),
    dict(fixed=np.zeros(3, np.float64)),
    dict(fixed=np.zeros((1, 3), np.uint8)),
    dict(R_init=np.zeros((4, 9))),
    dict(t_init=np.zeros((3, 3))),
    dict(R_init=np.zeros((4, 3, 3), np.complex128)),
    dict(barc=-5.0),
    dict(barc=float("nan")),
    dict(mu_init=-1e-5),
    dict(mu_init=float("inf")),
    dict(mu_step=1.0),
    dict(mu_step=0.9),
    dict(mu_step=float("nan")),
    dict(max_updates=-1),
    dict(max_updates=2.5),
    dict(rtol=-1e-10),
    dict(check_every=-1),
])
def test_solve_robust_refuses_without_a_device(kw):
    a = dict(fixed=np.ones(3, bool), R_init=np.zeros((4, 3, 3)), t_init=np.zeros((4, 3)))
    a.update(kw)
    with pytest.raises(ValueError):
        _solver().solve_robust(**a)


def test_check_fixed_converts():
    from kmx.dpgo.chordal import ChordalSolver
    assert ChordalSolver.check_fixed(3, None) is None
    for mask in (np.array([True, False, True]), np.array([2, 0, 1]), [1, 0, 1], np.array([1, 0, 1], np.uint8)):
        f = ChordalSolver.check_fixed(3, mask)
        assert f.dtype == np.uint8 and f.tolist() == [1, 0, 1] and f.flags.c_contiguous


# ---- the host mirror

def _edges(g):
    return [(int(g.p1[e]), int(g.p2[e]), g.R[e], g.t[e], float(g.kappa[e]), float(g.tau[e]), float(g.weight[e]))
            for e in range(g.m)]


def _ate(g, R, t):  # mean translation error against ground truth, first pose at the origin
    Rg, tg = g.gt_R[0], g.gt_t[0]
    return float(np.linalg.norm(t - (tg - tg[0]) @ Rg[0], axis=1).mean())


@functools.lru_cache(maxsize=None)
def _mirror120():
    from kmx.dpgo.init import robust_chordal_initialization
    from kmx.synth import make_pose_graph
    g = make_pose_graph(1, 120, 360, outlier_frac=0.2, seed=3)
    return g, robust_chordal_initialization(120, _edges(g), g.fixed, return_info=True)


def test_mirror_rejects_the_outliers():
    g, (R, t, w, updates, info) = _mirror120()
    lc = g.fixed == 0
    inl = lc & ~g.outlier
    kept_outliers, dropped = int((w[g.outlier] != 0).sum()), int((w[inl] == 0).sum())
    Ro = np.einsum("ij,njk->nik", g.init_R[0][0].T, g.init_R[0])
    to = (g.init_t[0] - g.init_t[0][0]) @ g.init_R[0][0]
    ate, ate_odo = _ate(g, R, t), _ate(g, Ro, to)
    print(f"updates {updates}, {info}; outliers kept {kept_outliers} of {int(g.outlier.sum())}, inliers dropped "
          f"{dropped} of {int(inl.sum())}; ATE {ate:.3f} m, odometry chain {ate_odo:.3f} m")
    assert info["converged"] and 0 < updates < 100
    assert np.all((w == 0) | (w == 1)) and np.all(w[g.fixed != 0] == 1)
    assert kept_outliers == 0
    assert dropped <= 0.05 * inl.sum()
    assert ate < 0.5 * ate_odo
    assert info["n_kept"] + info["n_rejected"] == int(lc.sum()) and info["n_fractional"] == 0
    assert info["n_kept"] == int((w[lc] == 1).sum())


def test_mirror_with_dpgo_mu_init_gives_the_same_inliers():
    from kmx.dpgo.init import robust_chordal_initialization
    g, (_, _, w, updates, _) = _mirror120()
    _, _, w2, updates2 = robust_chordal_initialization(120, _edges(g), g.fixed, mu_init=1e-5)
    assert np.array_equal(w, w2)
    assert updates2 > updates  # mu starts far lower and climbs by the same factor


def test_mirror_on_a_clean_graph_is_the_plain_chordal_result():
    from kmx.dpgo.init import chordal_initialization, robust_chordal_initialization
    from kmx.synth import make_pose_graph
    g = make_pose_graph(1, 60, 180, outlier_frac=0.0, noise_free=True, seed=2)
    R, t, w, updates = robust_chordal_initialization(60, _edges(g), g.fixed)
    Rc, tc = chordal_initialization(60, _edges(g))
    assert updates == 0 and np.array_equal(w, np.ones(g.m))
    assert np.array_equal(R, Rc) and np.array_equal(t, tc)


def test_mirror_stops_at_max_updates():
    from kmx.dpgo.init import robust_chordal_initialization
    g, (_, _, w, _, _) = _mirror120()
    R, t, w1, updates, info = robust_chordal_initialization(120, _edges(g), g.fixed, max_updates=1, return_info=True)
    assert updates == 1 and not info["converged"] and info["n_fractional"] > 0
    assert ((w1 > 0) & (w1 < 1)).sum() == info["n_fractional"]


def test_tls_factor_branches():
    from kmx.dpgo.init import gnc_tls_factor
    c2, mu = 25.0, 1.0
    r2 = np.array([0.0, 12.5, 12.5 + 1e-9, 25.0, 50.0 - 1e-9, 50.0, 1e6])
    w, frac = gnc_tls_factor(r2, mu, c2)
    assert w[:2].tolist() == [1.0, 1.0] and w[5:].tolist() == [0.0, 0.0]
    assert frac.tolist() == [False, False, True, True, True, False, False]
    assert abs(w[3] - (np.sqrt(2.0) - 1.0)) < 1e-15 and 0 < w[4] < w[3] < w[2] < 1


def test_agent_and_pipeline_know_the_method_and_keep_their_defaults():
    import inspect

    from kmx import pipeline as PL
    from kmx.dpgo import agent
    from kmx.dpgo.params import PGOAgentParameters
    assert PGOAgentParameters().localInitializationMethod == "odometry"
    assert PGOAgentParameters().robustInitMinInliers == 0
    assert inspect.signature(PL.run_pipeline).parameters["local_init"].default == "odometry"
    assert '"robust_chordal_gpu"' in inspect.getsource(agent.PGOAgent.initialize)
    assert '"robust_chordal_gpu"' in inspect.getsource(PL.run_pipeline)
