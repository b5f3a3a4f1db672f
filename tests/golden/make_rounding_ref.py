"""Writes tests/golden/rounding_ref.npz: the truth for the rounding of
kmx_pgo_get_trajectory (nearest rotation to M = Ya^T Yi, t = Ya^T (pi - pa))
and for the Stiefel projection (polar factor of the r x 3 block Yi), computed
by mpmath at 60 digits on the exact product of the stored fp64 inputs. Needs
no GPU. tests/rounding_ref.py holds the loader and the bounds.

Per r in (3, 4, 5, 8), n = 93, 93, 300, 93 poses (keys "r{r}_{name}"):

  anchors [G, r, 4]  the anchors [Ya pa] in use; aid [n] is each pose's
  X       [n, r, 4]  the lifted pose [Yi pi]
  sig     [n, 3]     singular values of M (exact zeros where the rank is < 3)
  d       [n]        sign det M, +1 where sig[2] = 0
  R       [n, 3, 3]  U diag(1, 1, d) V^T (rank 1: one completion; rank 0: I)
  t       [n, 3]     Ya^T (pi - pa)
  psig    [n, 3]     singular values of the r x 3 block Yi
  pY      [n, r, 3]  its U V^T (over the non-zero singular values only)
  deg     [k]        the poses with a zero singular value, and for them
  deg_U, deg_V [k, 3, 3]  U and V of M;  deg_pV [k, 3, 3]  V of Yi

and ratio_R, ratio_O, ratio_P, K_R, K_O, K_P: the worst ratio of the numpy
fp64 route to this truth for each bound, and 4 x it (the tests' constants).

The cases cycle (31 of them, so that each lands on several thread positions):
20 constructed (ten singular value triples, det > 0 and det < 0, a new draw
each cycle) and 11 exact ones with Ya = e1..e3.

    python tests/golden/make_rounding_ref.py
"""
import io
import sys
import zipfile
from pathlib import Path

import mpmath as mp
import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import rounding_ref as REF  # noqa: E402

mp.mp.dps = 60
ZERO = mp.mpf(10) ** -40  # relative: below it a singular value of the exact product is an exact zero
N_POSES = {3: 93, 4: 93, 5: 300, 8: 93}
SEED = 20261
TRIPLES = [(1, .9, .8), (1, .5, 1e-2), (1, 1e-2, 1e-4), (1, 1e-3, 1e-6), (1, .5, 1e-8), (1, .5, 1e-12),
           (1, .3, 1e-16), (1, 1e-5, 1e-6), (3e3, 2e3, 1e3), (1e-3, 5e-4, 1e-7)]


def _perm(p, s):
    P = np.zeros((3, 3))
    for i, (j, sg) in enumerate(zip(p, s)):
        P[i, j] = sg
    return P


_D = np.diag([1.0, 0.5, 0.0])
_A = np.array([[1.0, 2, 3], [2, 4, 6], [1, 0, 1]])
EXACT = [
    _D,
    _perm((1, 2, 0), (1, -1, 1)) @ _D @ _perm((2, 0, 1), (1, 1, 1)),
    _perm((2, 1, 0), (-1, 1, 1)) @ _D @ _perm((0, 2, 1), (1, -1, -1)),
    _perm((0, 2, 1), (1, 1, -1)) @ _D @ _perm((1, 0, 2), (-1, 1, 1)),
    _A, -_A,                                               # rank 2
    np.array([[1.0, 2, 3], [2, 4, 6], [3, 6, 9]]),         # rank 1
    np.zeros((3, 3)),                                      # rank 0
    np.eye(3),
    np.diag([-1.0, -3, -5]) / 9,                           # the reflection of test_chordal_gpu.py
    np.diag([1.0, -1, -1]) @ np.diag([1.0, 3, 5]) / 9,
]
N_CASES = 2 * len(TRIPLES) + len(EXACT)


def _orth(rng, k):
    Q, Rq = np.linalg.qr(rng.standard_normal((k, k)))
    return Q * np.sign(np.diag(Rq))


def _rot(rng):
    Q = _orth(rng, 3)
    return Q * np.linalg.det(Q)


def _mpm(a):
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in np.atleast_2d(a)])


def _np(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


def _cross(a, b):
    return mp.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _svd(A):
    """mpmath SVD with the singular values below ZERO * s1 set to an exact 0."""
    U, S, Vt = mp.svd_r(A, full_matrices=False)
    s = [S[k] for k in range(3)]
    s = [x if (s[0] > mp.mpf(10) ** -300 and x > ZERO * s[0]) else mp.mpf(0) for x in s]
    return U, s, Vt.T


def truth(anchor, Xi):
    """One pose's record (the arrays of the file) from its fp64 inputs."""
    r = anchor.shape[0]
    Ya, Yi = _mpm(anchor[:, :3]), _mpm(Xi[:, :3])
    M = Ya.T * Yi
    U, s, V = _svd(M)
    rank = sum(1 for x in s if x > 0)
    d = 1
    if rank == 3:
        d = 1 if mp.det(M) > 0 else -1
        assert (mp.det(U) * mp.det(V) > 0) == (d > 0)
    u = [U[:, k] for k in range(3)]
    v = [V[:, k] for k in range(3)]
    if rank >= 2:
        # U diag(1, 1, d) V^T: d u3 v3^T = (u1 x u2)(v1 x v2)^T whatever the signs of u3 and v3
        R = u[0] * v[0].T + u[1] * v[1].T + _cross(u[0], u[1]) * _cross(v[0], v[1]).T
        if rank == 3:
            assert mp.norm(R - U * mp.diag([1, 1, d]) * V.T) < mp.mpf(10) ** -45
    elif rank == 1:
        R = U * mp.diag([1, 1, mp.det(U) * mp.det(V)]) * V.T
    else:
        R = mp.eye(3)
    t = Ya.T * (_mpm(Xi[:, 3]).T - _mpm(anchor[:, 3]).T)
    pU, ps, pV = _svd(Yi)
    pY = mp.zeros(r, 3)
    for k in range(3):
        if ps[k] > 0:
            pY += pU[:, k] * pV[:, k].T
    return {"sig": np.array([float(x) for x in s]), "d": d, "R": _np(R), "t": _np(t).reshape(3),
            "psig": np.array([float(x) for x in ps]), "pY": _np(pY), "U": _np(U), "V": _np(V), "pV": _np(pV)}


def inputs(r, rng):
    """anchors, aid, X for rank r: anchor 0 a random frame with |pa| ~ 1,
    anchor 1 another with |pa| ~ 1e3 (and pi - pa ~ 1), anchor 2 the unit
    vectors e1..e3 of the exact cases."""
    n = N_POSES[r]
    Q = [_orth(rng, r), _orth(rng, r), np.eye(r)]
    pa = [rng.standard_normal(r), 1e3 * rng.standard_normal(r), np.array(([0.5, -1.25, 2.0] * 3)[:r])]
    anchors = np.stack([np.concatenate([Q[g][:, :3], pa[g][:, None]], 1) for g in range(3)])
    aid, X = np.zeros(n, np.int8), np.zeros((n, r, 4))
    for i in range(n):
        c = i % N_CASES
        if c < 2 * len(TRIPLES):
            g = (i // N_CASES + c) % 2
            s, sign = TRIPLES[c // 2], 1.0 if c % 2 == 0 else -1.0
            core = _rot(rng) @ np.diag([s[0], s[1], sign * s[2]]) @ _rot(rng).T
            B = 0.5 * s[0] * rng.standard_normal((r - 3, 3))  # the part outside the anchor's 3-plane
            X[i, :, :3] = Q[g][:, :3] @ core + Q[g][:, 3:] @ B
            X[i, :, 3] = pa[g] + rng.standard_normal(r)
        else:
            g = 2
            X[i, :3, :3] = EXACT[c - 2 * len(TRIPLES)]
            X[i, :, 3] = pa[g] + np.round(8 * rng.standard_normal(r)) / 8
        aid[i] = g
    return anchors, aid, X


def main():
    rng = np.random.Generator(np.random.PCG64(SEED))
    out, cases = {}, {}
    for r in REF.RANKS:
        anchors, aid, X = inputs(r, rng)
        recs = []
        for i in range(X.shape[0]):
            for _ in range(20):
                rec = truth(anchors[aid[i]], X[i])
                rank = int((rec["sig"] > 0).sum())
                ok = True
                if rank >= 2:  # passing must mean something: a provisional K_R of 400, asserted with the final one below
                    A = np.linalg.norm(np.abs(anchors[aid[i]][:, :3]).T @ np.abs(X[i, :, :3]))
                    ok = 400 * REF.EPS * A / (rec["sig"][1] + rec["d"] * rec["sig"][2]) < 1e-3
                if ok:
                    break
                X[i, :, :3] = X[i, :, :3] @ _rot(rng)  # another draw of the same triple
            assert ok
            recs.append(rec)
        deg = np.array([i for i, q in enumerate(recs) if q["sig"][2] == 0 or q["psig"][2] == 0], np.int32)
        arr = {"anchors": anchors, "aid": aid, "X": X, "deg": deg, "d": np.array([q["d"] for q in recs], np.int8)}
        for k in ("sig", "R", "t", "psig", "pY"):
            arr[k] = np.stack([q[k] for q in recs])
        for k in ("U", "V", "pV"):
            arr["deg_" + k] = np.stack([recs[i][k] for i in deg])
        for k, v in arr.items():
            out[f"r{r}_{k}"] = v
        cases[r] = REF.Case(r, arr)
        print(f"r={r}: {X.shape[0]} poses, {len(deg)} with a zero singular value", flush=True)
    # the constants: 4 x the numpy fp64 route's worst ratio to the truth
    rR = rO = rP = rT = 0.0
    for r, c in cases.items():
        val, orth, det, tr = REF.rotation_ratios(c, REF.np_trajectory(c))
        pval, porth = REF.polar_ratios(c, REF.np_project(c))
        assert (det > 0).all()
        rR, rO, rP, rT = max(rR, val.max()), max(rO, orth.max(), porth.max()), max(rP, pval.max()), max(rT, tr.max())
    K = {"ratio_R": rR, "ratio_O": rO, "ratio_P": rP, "K_R": 4 * rR, "K_O": 4 * rO, "K_P": 4 * rP}
    for r, c in cases.items():
        for i in range(c.n):
            if c.rank[i] >= 2:
                assert K["K_R"] * REF.rotation_unit(c, i) < 1e-3, (r, i)
    for k, v in K.items():
        out[k] = np.array([v])
    print({k: round(float(v), 3) for k, v in K.items()}, "numpy translation ratio", round(float(rT), 3))
    save(REF.FIXTURE, out)
    print(REF.FIXTURE.stat().st_size, "bytes")


def save(path, arrays):
    """An .npz as numpy.savez_compressed writes it, but with a fixed time stamp
    on every member, so that the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    main()
