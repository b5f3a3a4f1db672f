"""Rounding (k_traj) and Stiefel projection (group_project) against an SVD:
the fixture's loader, the bounds and a plain numpy fp64 route.

tests/golden/rounding_ref.npz (written by tests/golden/make_rounding_ref.py)
holds, for each r in RANKS, a set of lifted poses with the truth computed by
mpmath at 60 digits on the exact product of the fp64 inputs.

Contract ("Rounding and projection against an SVD"),
eps = 2^-52, M = Ya^T Yi with singular values s1 >= s2 >= s3, d = sign det M
(+1 where s3 = 0):

  rotation   |R - U diag(1,1,d) V^T|max <= K_R eps A / (s2 + d s3),
             A = || |Ya|^T |Yi| ||_F   (what fp64 loses in forming M, over the
             perturbation bound of the nearest rotation)
             |R^T R - I|max <= K_O eps and det R > 0 on every pose
             rank 1: only R v1 = u1, with s2 + d s3 replaced by s1
             rank 0: any finite proper rotation
  translation |t - Ya^T (pi - pa)| <= 4 * 2r * eps * sum_k |Ya[k,x]| (|pi[k]| + |pa[k]|)
  polar      |Y - U V^T|max <= K_P eps ||Yi||_F / s3  (s of the r x 3 block Yi)
             |Y^T Y - I|max <= K_O eps
             s3 = 0: Y finite with orthonormal columns; (Y - U V^T) [v1 v2]
             within the bound with s3 replaced by s2. The same rule one rank
             down (the issue leaves it open): rank 1 agrees on v1 with s1,
             rank 0 is any finite orthonormal frame.

The constants are 4 x the worst ratio of the numpy fp64 route below
(numpy.linalg.svd) to the mpmath truth over the fixture's inputs, measured by
the generator and stored in the fixture ("ratio_*", "K_*"):

  ratio_R = 12.19   K_R = 48.75    (rotation value)
  ratio_O = 11.00   K_O = 44.00    (orthogonality, rotation and polar factor)
  ratio_P =  6.88   K_P = 27.53    (polar factor value)

A correct fp64 algorithm with another rotation or summation order may differ
from LAPACK by a small factor, not by orders of magnitude. Measured on an
MI355X: the one-sided Jacobi of so3_project.h and group_project stays at 3.6
(rotation), 7 eps (orthogonality), 1.02 (polar) and 0.02 of the translation
bound; the Gram-matrix recipe they replace reached 3e2 at sigma3/sigma1 = 1e-2,
1e5 at 1e-4, 5e7 at 1e-6, 4e15 at 1e-8 and stored Inf or NaN from 1e-12 down
and on the exact rank-2, rank-1 and zero blocks.
"""
from pathlib import Path

import numpy as np

EPS = 2.0 ** -52
RANKS = (3, 4, 5, 8)
FIXTURE = Path(__file__).resolve().parent / "golden" / "rounding_ref.npz"
FIELDS = ("anchors", "aid", "X", "sig", "d", "R", "t", "psig", "pY", "deg", "deg_U", "deg_V", "deg_pV")

_cache = {}


class Case:
    """The poses of one rank r; arrays as the generator's docstring lists them."""

    def __init__(self, r, arrays):
        self.r = r
        for k in FIELDS:
            setattr(self, k, arrays[k])
        self.n = self.X.shape[0]
        self.rank = (self.sig > 0).sum(1)    # of M = Ya^T Yi
        self.prank = (self.psig > 0).sum(1)  # of the r x 3 block Yi
        self._deg = {int(p): k for k, p in enumerate(self.deg)}

    def anchor(self, i):
        return self.anchors[self.aid[i]]

    def uv(self, i):
        """(U, V, pV) of a pose with a zero singular value (rows of deg_*)."""
        k = self._deg[int(i)]
        return self.deg_U[k], self.deg_V[k], self.deg_pV[k]


def load():
    """{r: Case}, {name: constant}; read once and left unchanged."""
    if not _cache:
        z = np.load(FIXTURE)
        _cache["cases"] = {r: Case(r, {k: z[f"r{r}_{k}"] for k in FIELDS}) for r in RANKS}
        _cache["K"] = {k: float(z[k][0]) for k in ("ratio_R", "ratio_O", "ratio_P", "K_R", "K_O", "K_P")}
        for c in _cache["cases"].values():
            for k in FIELDS:
                getattr(c, k).setflags(write=False)
    return _cache["cases"], _cache["K"]


def chain_graph(n):
    """A one-robot chain of n poses (n - 1 identity odometry edges): what the
    handles are built on; its content plays no part in rounding."""
    from kmx.synth.pose_graph import PoseGraphData
    m = n - 1
    z = np.zeros(m, np.int32)
    return PoseGraphData(n_robots=1, n_poses=np.array([n], np.int32), r1=z, p1=np.arange(m, dtype=np.int32), r2=z.copy(),
                         p2=np.arange(1, n, dtype=np.int32), R=np.tile(np.eye(3), (m, 1, 1)), t=np.zeros((m, 3)),
                         kappa=np.full(m, 1e4), tau=np.full(m, 1e2), weight=np.ones(m), fixed=np.ones(m, np.uint8),
                         outlier=np.zeros(m, bool))


# ------------------------------------------------------------- numpy route --
def np_rotation(Ya, Yi):
    """Nearest rotation to Ya^T Yi in fp64: U diag(1, 1, det(U V^T)) V^T."""
    U, _, Vt = np.linalg.svd(Ya.T @ Yi)
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U @ Vt) >= 0 else -1.0])
    return U @ D @ Vt


def np_translation(anchor, Xi):
    return anchor[:, :3].T @ (Xi[:, 3] - anchor[:, 3])


def np_polar(Yi):
    U, _, Vt = np.linalg.svd(Yi, full_matrices=False)
    return U @ Vt


def np_trajectory(case):
    out = np.empty((case.n, 12))
    for i in range(case.n):
        a = case.anchor(i)
        out[i, :9] = np_rotation(a[:, :3], case.X[i, :, :3]).reshape(-1)
        out[i, 9:] = np_translation(a, case.X[i])
    return out


def np_project(case):
    out = case.X.copy()
    for i in range(case.n):
        out[i, :, :3] = np_polar(case.X[i, :, :3])
    return out


# ------------------------------------------------------------------ bounds --
def rotation_unit(case, i):
    """The rotation value bound of pose i over K_R (inf for the zero block)."""
    a = case.anchor(i)
    A = np.linalg.norm(np.abs(a[:, :3]).T @ np.abs(case.X[i, :, :3]))
    s = case.sig[i]
    den = s[1] + case.d[i] * s[2] if case.rank[i] >= 2 else s[0]
    return EPS * A / den if den > 0 else np.inf


def rotation_ratios(case, traj):
    """Per pose: (value error / unit bound, |R^T R - I|max / eps, det R,
    translation error / its bound). The rank-0 pose's value ratio is 0."""
    val, orth, det, tr = (np.zeros(case.n) for _ in range(4))
    for i in range(case.n):
        R = traj[i, :9].reshape(3, 3)
        orth[i] = np.abs(R.T @ R - np.eye(3)).max() / EPS
        det[i] = np.linalg.det(R)
        if case.rank[i] >= 2:
            val[i] = np.abs(R - case.R[i]).max() / rotation_unit(case, i)
        elif case.rank[i] == 1:
            U, V, _ = case.uv(i)
            val[i] = np.abs(R @ V[:, 0] - U[:, 0]).max() / rotation_unit(case, i)
        a, Xi = case.anchor(i), case.X[i]
        tb = 4 * 2 * case.r * EPS * (np.abs(a[:, :3]).T @ (np.abs(Xi[:, 3]) + np.abs(a[:, 3])))
        tr[i] = (np.abs(traj[i, 9:] - case.t[i]) / tb).max()
    return val, orth, det, tr


def assert_rotations(traj, K, what=""):
    """The rotation property alone (every input has it, whatever the anchor)."""
    assert np.isfinite(traj).all(), f"{what}: non-finite output at poses {np.unique(np.nonzero(~np.isfinite(traj))[0])[:8]}"
    R = traj[:, :9].reshape(-1, 3, 3)
    orth = np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max((1, 2)) / EPS
    assert (orth <= K["K_O"]).all(), f"{what}: |R^T R - I| = {orth.max():.3g} eps at pose {orth.argmax()}"
    assert (np.linalg.det(R) > 0).all(), what


def polar_unit(case, i):
    s = case.psig[i]
    den = s[case.prank[i] - 1] if case.prank[i] else 0.0
    return EPS * np.linalg.norm(case.X[i, :, :3]) / den if den > 0 else np.inf


def polar_ratios(case, out):
    """Per pose: (value error / unit bound, |Y^T Y - I|max / eps)."""
    val, orth = np.zeros(case.n), np.zeros(case.n)
    for i in range(case.n):
        Y = out[i, :, :3]
        orth[i] = np.abs(Y.T @ Y - np.eye(3)).max() / EPS
        k = case.prank[i]
        if k == 3:
            val[i] = np.abs(Y - case.pY[i]).max() / polar_unit(case, i)
        elif k > 0:
            pV = case.uv(i)[2]
            val[i] = np.abs((Y - case.pY[i]) @ pV[:, :k]).max() / polar_unit(case, i)
    return val, orth


def check_trajectory(case, traj, K, what=""):
    """Applies the rotation, rotation-property and translation bounds to every
    pose; returns the worst ratios (value / K_R-unit, orthogonality / eps,
    translation / bound) for the record."""
    assert np.isfinite(traj).all(), f"{what}: non-finite output at poses {np.unique(np.nonzero(~np.isfinite(traj))[0])[:8]}"
    val, orth, det, tr = rotation_ratios(case, traj)
    print(f"{what} r={case.r} n={case.n}: rotation {val.max():.3g} of K_R={K['K_R']:.3g}, "
          f"orthogonality {orth.max():.3g} of K_O={K['K_O']:.3g}, translation {tr.max():.3g} of 1")
    assert (det > 0).all(), f"{what}: det R <= 0 at poses {np.nonzero(det <= 0)[0][:8]}"
    assert (orth <= K["K_O"]).all(), f"{what}: |R^T R - I| = {orth.max():.3g} eps at pose {orth.argmax()}"
    assert (val <= K["K_R"]).all(), f"{what}: rotation {val.max():.3g} x unit bound at pose {val.argmax()} " \
                                     f"(sigma {case.sig[val.argmax()]}, d {case.d[val.argmax()]})"
    assert (tr <= 1.0).all(), f"{what}: translation {tr.max():.3g} x bound at pose {tr.argmax()}"
    return val.max(), orth.max(), tr.max()


def check_projection(case, out, K, what=""):
    assert np.isfinite(out).all(), f"{what}: non-finite output at poses {np.unique(np.nonzero(~np.isfinite(out))[0])[:8]}"
    assert np.array_equal(out[:, :, 3], case.X[:, :, 3]), f"{what}: translation column changed"
    val, orth = polar_ratios(case, out)
    print(f"{what} r={case.r} n={case.n}: polar {val.max():.3g} of K_P={K['K_P']:.3g}, "
          f"orthogonality {orth.max():.3g} of K_O={K['K_O']:.3g}")
    assert (orth <= K["K_O"]).all(), f"{what}: |Y^T Y - I| = {orth.max():.3g} eps at pose {orth.argmax()}"
    assert (val <= K["K_P"]).all(), f"{what}: polar {val.max():.3g} x unit bound at pose {val.argmax()} " \
                                     f"(sigma {case.psig[val.argmax()]})"
    return val.max(), orth.max()
