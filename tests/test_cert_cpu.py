"""The dual certificate (kmx_cert_*), the part that needs no device: the header
declares the entry points, the library exports them and kmx/abi.py binds them,
struct sizes match, the ABI version is unchanged, the host-only decision rule
(kmx_cert_ritz) agrees with numpy.linalg.eigh on Lanczos tridiagonals, the
start vector equals the restatement's bit for bit, and the Python wrapper
refuses malformed graphs before the library is called."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import cert_ref as CR

ROOT = Path(__file__).resolve().parents[1]

SYMBOLS = ("kmx_cert_create", "kmx_cert_destroy", "kmx_cert_set_stream", "kmx_cert_set_graph",
           "kmx_cert_set_weights", "kmx_cert_set_point", "kmx_cert_get_lambda", "kmx_cert_apply", "kmx_cert_min_eig",
           "kmx_cert_get_coefficients", "kmx_cert_ritz", "kmx_cert_start_vector", "kmx_cert_get_timing",
           "kmx_cert_get_host_timing")


def test_symbols_declared_exported_and_bound():
    from kmx import abi
    L = abi.lib()
    hdr = (ROOT / "include" / "kmx_abi.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(kmx_\w+)\s*\(", hdr, re.M))
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name  # bound in kmx/abi.py


def test_abi_version_is_still_10_and_structs_match_the_header():
    import ctypes as C

    from kmx import abi
    hdr = (ROOT / "include" / "kmx_abi.h").read_text()
    assert int(re.search(r"#define\s+KMX_ABI_VERSION\s+(\d+)", hdr).group(1)) == 10
    assert abi.ABI_VERSION == 10 and abi.lib().kmx_abi_version() == 10
    assert C.sizeof(abi.CertParams) == 32 and abi.CertParams.seed.offset == 24
    assert C.sizeof(abi.CertResult) == 32 and abi.CertResult.theta_min.offset == 8
    assert C.sizeof(abi.CertPointInfo) == 24
    for k, name in enumerate(abi.CERT_DECISION):
        assert int(re.search(rf"#define\s+KMX_CERT_{name}\s+(\d+)", hdr).group(1)) == k


def test_certifier_needs_a_device():
    from kmx import abi
    from kmx.dpgo.certify import Certifier
    with pytest.raises(abi.KmxError):
        Certifier(device=abi.device_count())


@pytest.fixture(scope="module")
def tridiagonals():
    """Lanczos coefficients of the restatement. The long one is a noise-free
    chain of 400 poses at the lifted ground truth: S is positive semidefinite
    with a dense small end, so 300 steps have not converged and the smallest
    Ritz value is simple. (Once a Ritz value has converged, Lanczos without
    reorthogonalisation grows copies of it; the eigenvector of a cluster, and
    with it rho, is then not determined, in numpy's eigh either.)"""
    g, X = CR.consistent_graph(400, 0, 5, 1)
    Q = CR.dense_Q(400, g["src"], g["dst"], g["R"], g["t"], g["kappa"], g["tau"], g["weight"])
    chain = CR.lanczos(CR.dense_S(X, Q), 300, 7)
    gr, Xr = CR.ring(24, 3)
    Qr = CR.dense_Q(24, gr["src"], gr["dst"], gr["R"], gr["t"], gr["kappa"], gr["tau"], gr["weight"])
    ring = CR.lanczos(CR.dense_S(Xr, Qr), 10, 7)
    return {"chain": chain, "ring": ring}


@pytest.mark.parametrize("k", [1, 2, 10, 300])
def test_ritz_matches_eigh(tridiagonals, k):
    from kmx.dpgo.certify import ritz
    al, be = tridiagonals["chain"]
    assert len(al) == 300
    if k > 2:  # the reference's eigenvector is determined: the smallest Ritz value is simple
        T = np.diag(al[:k]) + np.diag(be[:k - 1], 1) + np.diag(be[:k - 1], -1)
        ev = np.linalg.eigvalsh(T)
        assert ev[1] - ev[0] > 1e-3
    for eta in (1e-5, 1.0):
        ref = CR.ritz(al[:k], be[:k], eta)
        got = ritz(al[:k], be[:k], eta)
        tol = 1e-12 * abs(ref["theta_max"])
        assert abs(got["theta_min"] - ref["theta_min"]) <= tol
        assert abs(got["theta_max"] - ref["theta_max"]) <= tol
        assert abs(got["residual"] - ref["residual"]) <= tol
        assert got["decision"] == ref["decision"] and got["steps"] == k


def test_ritz_reaches_all_three_decisions(tridiagonals):
    from kmx.dpgo.certify import ritz
    al, be = tridiagonals["chain"]
    assert ritz(al, be, 1e-5)["decision"] == "UNDECIDED"  # theta_min > 0, rho ~ 1e-2
    assert ritz(al, be, 1.0)["decision"] == "CERTIFIED"
    ar, br = tridiagonals["ring"]
    ref = CR.ritz(ar, br, 1e-5)
    got = ritz(ar, br, 1e-5)
    assert got["decision"] == ref["decision"] == "NEGATIVE"
    assert got["theta_min"] >= -(2 - 2 * np.cos(2 * np.pi / 24)) - 1e-12  # Ritz values lie inside the spectrum
    # an invariant subspace (beta_k = 0): the Ritz values are eigenvalues, rho = 0
    one = ritz(np.array([2.0, 3.0]), np.array([0.5, 0.0]), 1e-9)
    assert one["decision"] == "CERTIFIED" and one["residual"] == 0.0


def test_ritz_certifies_only_below_a_tenth_of_eta():
    """One step has s = (1) and rho = beta_1: CERTIFIED needs rho <= CERT_C eta
    (and theta_min - rho >= -eta as before), in the library, in the restatement
    and in the header's words."""
    from kmx.dpgo.certify import ritz
    assert CR.CERT_C == 0.1
    for a, b, want in ((1.0, 0.1, "CERTIFIED"), (1.0, 0.1000001, "UNDECIDED"), (1.0, 0.9, "UNDECIDED"),
                       (-0.95, 0.1, "UNDECIDED"), (-0.5, 0.1, "CERTIFIED"), (-1.01, 0.0, "NEGATIVE")):
        got, ref = ritz(np.array([a]), np.array([b]), 1.0), CR.ritz(np.array([a]), np.array([b]), 1.0)
        assert got["decision"] == ref["decision"] == want, (a, b, got, ref)
        assert got["residual"] == b and got["theta_min"] == a
    hdr = (ROOT / "include" / "kmx_abi.h").read_text()
    assert re.search(r"#define\s+KMX_CERT_CERTIFIED\s+1\s*/\*\s*rho <= eta / 10 and theta_min - rho >= -eta", hdr)


@pytest.mark.parametrize("eta", [0.0, -1e-5, float("nan"), float("inf")])
def test_ritz_refuses_bad_eta(eta):
    import ctypes as C

    from kmx import abi
    L = abi.lib()
    a, b = np.array([1.0, 2.0]), np.array([0.5, 0.5])
    res = abi.CertResult()
    assert L.kmx_cert_ritz(2, abi.fptr(a), abi.fptr(b), eta, C.byref(res)) == abi.KMX_EINVAL
    assert L.kmx_cert_ritz(0, abi.fptr(a), abi.fptr(b), 1e-5, C.byref(res)) == abi.KMX_EINVAL


@pytest.mark.parametrize("seed,count", [(0, 1), (7, 260), (2**64 - 1, 33), (123456789, 4 * 130)])
def test_start_vector_bit_for_bit(seed, count):
    from kmx.dpgo.certify import start_vector
    got = start_vector(seed, count)
    ref = CR.start_vector(seed, count)
    assert got.shape == ref.shape and np.array_equal(got, ref)
    assert (got >= -1).all() and (got < 1).all()
    if count > 1:
        assert np.unique(got).size == count


def _good(m=3, n=4):
    return dict(n_poses=n, src=np.arange(m), dst=np.arange(m) + 1, R=np.tile(np.eye(3), (m, 1, 1)),
                t=np.zeros((m, 3)), kappa=np.ones(m), tau=np.ones(m), weight=np.ones(m))


def test_check_graph_accepts_and_converts():
    from kmx.dpgo.certify import Certifier
    n, src, dst, R, t, kappa, tau, w = Certifier.check_graph(**_good())
    assert n == 4 and src.dtype == np.int32 and dst.dtype == np.int32
    assert R.dtype == np.float64 and R.shape == (3, 3, 3) and R.flags.c_contiguous
    a = _good()
    a["weight"] = None
    a["kappa"] = np.ones(3, np.int64)  # integers are real numbers
    assert Certifier.check_graph(**a)[7] is None
    # legal: weight 0, parallel edges, poses without edges, no edges at all
    a = _good()
    a["weight"] = np.array([0.0, 1.0, 1.0])
    a["src"], a["dst"] = np.array([0, 0, 1]), np.array([1, 1, 0])
    a["n_poses"] = 9
    Certifier.check_graph(**a)
    Certifier.check_graph(3, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 3, 3)), np.zeros((0, 3)),
                          np.zeros(0), np.zeros(0))


@pytest.mark.parametrize("field,value", [
    ("src", np.array([0, 1, 4])),              # index out of range
    ("dst", np.array([1, 2, -1])),
    ("dst", np.array([1, 1, 3])),              # src == dst (edge 1)
    ("R", np.full((3, 3, 3), np.nan)),         # not finite
    ("t", np.array([[0, 0, 0], [0, np.inf, 0], [0, 0, 0.0]])),
    ("kappa", np.array([1.0, 0.0, 1.0])),      # kappa <= 0
    ("kappa", np.array([1.0, np.nan, 1.0])),
    ("tau", np.array([1.0, 1.0, -2.0])),       # tau <= 0
    ("weight", np.array([1.0, -0.1, 1.0])),    # w < 0
    ("weight", np.array([1.0, np.inf, 1.0])),
    ("src", np.zeros(3)),                      # float indices
    ("dst", np.arange(4)),                     # length differs from src
    ("R", np.zeros((3, 9))),                   # flat rotations
    ("t", np.zeros((3, 2))),
    ("tau", np.array(["a", "b", "c"])),
    ("weight", np.ones((3, 1))),
    ("src", np.array([0, 1, 2**40])),          # does not fit int32
    ("n_poses", 0),
])
def test_check_graph_refuses(field, value):
    from kmx.dpgo.certify import Certifier
    a = _good()
    a[field] = value
    with pytest.raises(ValueError):
        Certifier.check_graph(**a)


@pytest.mark.parametrize("X", [np.zeros((4, 2, 4)), np.zeros((4, 9, 4)), np.zeros((3, 5, 4)), np.zeros((4, 5, 3)),
                               np.full((4, 5, 4), np.nan), np.zeros((4, 20))])
def test_check_point_refuses(X):
    from kmx.dpgo.certify import Certifier
    with pytest.raises(ValueError):
        Certifier.check_point(4, X)
    assert Certifier.check_point(4, np.zeros((4, 8, 4), np.float32)).dtype == np.float64


def test_escape_point_is_on_the_manifold_and_flatten_team_offsets():
    from kmx.dpgo.certify import escape_point, flatten_team
    from kmx.synth import make_pose_graph
    X = CR.random_point(7, 4, 3)
    y = np.random.default_rng(0).standard_normal(28)
    Xp = escape_point(X, y, 0.05)
    assert Xp.shape == (7, 5, 4)
    G = np.einsum("nac,nad->ncd", Xp[:, :, :3], Xp[:, :, :3])
    assert np.abs(G - np.eye(3)).max() < 1e-14
    assert np.array_equal(Xp[:, :4, 3], X[:, :, 3]) and np.allclose(Xp[:, 4, 3], 0.05 * y.reshape(7, 4)[:, 3])
    assert np.abs(escape_point(X, y, 0.0)[:, :4] - X).max() < 1e-14  # alpha = 0: X with a zero row
    g = make_pose_graph(3, 30, 50, seed=2)
    Xs = {a: np.full((int(g.n_poses[a]), 3, 4), float(a)) for a in range(3)}
    n, src, dst, Xf = flatten_team(g, Xs)
    off = np.concatenate([[0], np.cumsum(g.n_poses)])
    assert n == 30 and Xf.shape == (30, 3, 4)
    assert np.array_equal(src, off[g.r1] + g.p1) and np.array_equal(dst, off[g.r2] + g.p2)
    assert all((Xf[off[a]:off[a + 1]] == a).all() for a in range(3))


def test_pipeline_refuses_a_certificate_across_ranks():
    from kmx import pipeline as PL
    with pytest.raises(ValueError, match="certify_eta"):
        PL.run_pipeline(None, None, None, None, world=2, certify_eta=1e-5)
    import inspect
    assert inspect.signature(PL.run_pipeline).parameters["certify_eta"].default is None
