"""Chordal initialisation on the device (kmx_chordal_*), the part that needs no
device: the header declares the entry points, the library exports them and
kmx/abi.py binds them, the ABI version is unchanged, there is no CPU fallback,
and the Python wrapper refuses wrong shapes and dtypes before the library is
called."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]

SYMBOLS = ("kmx_chordal_create", "kmx_chordal_destroy", "kmx_chordal_set_stream", "kmx_chordal_set_graph",
           "kmx_chordal_set_weights", "kmx_chordal_solve")


def test_symbols_declared_exported_and_bound():
    from kmx import abi
    L = abi.lib()
    hdr = (ROOT / "include" / "kmx_abi.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(kmx_\w+)\s*\(", hdr, re.M))
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name  # bound in kmx/abi.py


def test_abi_version_is_still_10_on_both_sides():
    from kmx import abi
    hdr = (ROOT / "include" / "kmx_abi.h").read_text()
    assert int(re.search(r"#define\s+KMX_ABI_VERSION\s+(\d+)", hdr).group(1)) == 10
    assert abi.ABI_VERSION == 10
    assert abi.lib().kmx_abi_version() == 10


def test_structs_match_the_header():
    import ctypes as C

    from kmx import abi
    assert C.sizeof(abi.ChordalParams) == 16
    assert C.sizeof(abi.ChordalBlockInfo) == 64
    assert abi.ChordalBlockInfo.relres_rot.offset == 16 and abi.ChordalBlockInfo.relres_trans.offset == 40


def test_chordal_solver_needs_a_device():
    """An ordinal past the visible devices (all of them on a host without a
    GPU): no CPU fallback."""
    from kmx import abi
    from kmx.dpgo.chordal import ChordalSolver
    with pytest.raises(abi.KmxError):
        ChordalSolver(device=abi.device_count())


def _good(m=3, n=4):
    return dict(n_poses=n, block_ptr=np.array([0, n]), src=np.arange(m), dst=np.arange(m) + 1,
                R=np.tile(np.eye(3), (m, 1, 1)), t=np.zeros((m, 3)), kappa=np.ones(m), tau=np.ones(m),
                weight=np.ones(m), anchors=[0])


def test_check_graph_accepts_and_converts():
    from kmx.dpgo.chordal import ChordalSolver
    n, bp, src, dst, R, t, kappa, tau, w, anchors = ChordalSolver.check_graph(**_good())
    assert n == 4 and bp.dtype == np.int32 and src.dtype == np.int32 and dst.dtype == np.int32
    assert R.dtype == np.float64 and R.shape == (3, 3, 3) and R.flags.c_contiguous
    assert anchors.dtype == np.int32 and anchors.tolist() == [0]
    a = _good()
    a["weight"] = None
    a["kappa"] = np.ones(3, np.int64)  # integers are real numbers
    assert ChordalSolver.check_graph(**a)[8] is None


@pytest.mark.parametrize("field,value", [
    ("src", np.zeros(3)),                      # float indices
    ("dst", np.arange(4)),                     # length differs from src
    ("dst", np.zeros((3, 1), np.int64)),       # not one-dimensional
    ("R", np.zeros((3, 9))),                   # flat rotations
    ("R", np.zeros((2, 3, 3))),                # wrong count
    ("R", np.zeros((3, 3, 3), np.complex128)),  # not real
    ("t", np.zeros((3, 2))),
    ("kappa", np.ones(4)),
    ("tau", np.array(["a", "b", "c"])),
    ("weight", np.ones((3, 1))),
    ("block_ptr", np.array([0.0, 4.0])),
    ("block_ptr", np.array([4])),
    ("anchors", [0.5]),
    ("src", np.array([0, 1, 2**40])),          # does not fit int32
    ("n_poses", 0),
])
def test_check_graph_refuses(field, value):
    from kmx.dpgo.chordal import ChordalSolver
    a = _good()
    a[field] = value
    with pytest.raises(ValueError):
        ChordalSolver.check_graph(**a)


@pytest.mark.parametrize("R_init,t_init", [
    (np.zeros((4, 9)), None),
    (np.zeros((3, 3, 3)), None),
    (None, np.zeros((4, 4))),
    (None, np.zeros(12)),
    (np.zeros((4, 3, 3), np.complex128), None),
])
def test_check_start_refuses(R_init, t_init):
    from kmx.dpgo.chordal import ChordalSolver
    with pytest.raises(ValueError):
        ChordalSolver.check_start(4, R_init, t_init)
    assert ChordalSolver.check_start(4, None, None) == (None, None)
    R, t = ChordalSolver.check_start(4, np.zeros((4, 3, 3), np.float32), np.zeros((4, 3)))
    assert R.dtype == np.float64 and t.shape == (4, 3)


def test_agent_and_pipeline_keep_their_unknown_method_errors():
    from kmx import pipeline as PL
    from kmx.dpgo.agent import PGOAgent
    from kmx.dpgo.messages import RelativeSEMeasurement
    from kmx.dpgo.params import PGOAgentParameters
    from kmx.synth import make_pose_graph
    from tests.mock_solver import OracleBlockSolver
    assert PGOAgentParameters().localInitializationMethod == "odometry"
    g = make_pose_graph(1, 20, 40, outlier_frac=0.0, seed=1)
    P = PGOAgentParameters(r=5, num_robots=1, localInitializationMethod="cholesky")
    ag = PGOAgent(0, P, solver=OracleBlockSolver(P))
    for e in range(g.m):
        ag.addMeasurement(RelativeSEMeasurement(0, 0, int(g.p1[e]), int(g.p2[e]), 3, g.R[e], g.t[e],
                                                float(g.kappa[e]), float(g.tau[e]), fixedWeight=bool(g.fixed[e])))
    with pytest.raises(ValueError, match="unknown localInitializationMethod"):
        ag.initialize()
    import inspect
    assert inspect.signature(PL.run_pipeline).parameters["local_init"].default == "odometry"
