"""Degenerate and ill-conditioned loop-closure scenes for the LCD tests.

Every other LCD test draws from kmx.synth.lcd.make_lcd_pool's one family (a
general 3D cloud 1-20 m ahead, rotation <= 30 deg, baseline 0.2-2 m). A real
loop closure is a revisit: (almost) no baseline, pure forward motion, a wall, a
far scene, a rolled camera. There the 5-point systems are rank-deficient or
nearly so, the triangulation's 2x2 system is singular, EPnP's PCA has a zero
eigenvalue.

One function per family. Each returns an LcdPool from make_lcd_pool (its
descriptors, look-alikes, random features and candidate list unchanged) whose
planted true correspondences (pool.true_idx) have their points and bearings
overwritten with the family's scene under the family's pose
(p_query = R p_match + t). Fixed seeds; F = 8 frames (4 planted pairs) and
N = 200 features by default. `noise_free=False` adds make_lcd_pool's noise
(bearing sigma 1e-4, point sigma 0.05 m) to the overwritten entries too.
"""
from __future__ import annotations

import numpy as np

from kmx.synth.lcd import LcdPool, make_lcd_pool
from kmx.synth.pose_graph import _expm_so3

BEARING_SIGMA = 1e-4
POINT_SIGMA = 0.05


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _cloud(rng, n, zlo=2.0, zhi=20.0):
    z = rng.uniform(zlo, zhi, n)
    xy = rng.uniform(-0.6, 0.6, (n, 2)) * z[:, None]
    return np.c_[xy, z]


def _rot(rng, P, angle=None):
    axis = _unit(rng.normal(size=(P, 3)))
    ang = rng.uniform(-np.pi / 6, np.pi / 6, P) if angle is None else np.full(P, angle)
    return _expm_so3(axis * ang[:, None])


def _trans(rng, P, lo=0.2, hi=1.5):
    return _unit(rng.normal(size=(P, 3))) * rng.uniform(lo, hi, P)[:, None]


def _build(seed, F, N, noise_free, pose, scene) -> LcdPool:
    """pose(rng, P) -> (R [P, 3, 3], t [P, 3]); scene(rng, n) -> match-frame
    points [n, 3] (drawn per pair)."""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    P = F // 2
    R, t = pose(rng, P)
    pool = make_lcd_pool(F, N, noise_free=noise_free, bearing_sigma=BEARING_SIGMA, point_sigma=POINT_SIGMA,
                         seed=seed, R_qm=R, t_qm=t)
    sb = 0.0 if noise_free else BEARING_SIGMA
    sp = 0.0 if noise_free else POINT_SIGMA
    nt = pool.true_idx.shape[1]
    for k in range(P):
        pm = np.ascontiguousarray(scene(rng, nt), np.float64)
        pq = pm @ pool.R_qm[k].T + pool.t_qm[k]
        assert pm[:, 2].min() > 0.5 and pq[:, 2].min() > 0.5, "scene behind a camera"
        iq, im = pool.true_idx[k, :, 0], pool.true_idx[k, :, 1]
        for f, idx, p in ((2 * k, iq, pq), (2 * k + 1, im, pm)):
            b = _unit(p)
            if sb > 0:
                b = _unit(b + rng.normal(0, sb, b.shape))
            pool.bearings[f, idx] = b
            pool.points[f, idx] = p + (rng.normal(0, sp, p.shape) if sp > 0 else 0.0)
    return pool


def _pose_general(rng, P):
    return _rot(rng, P), _trans(rng, P)


def _fixed(R, t):
    def pose(rng, P):
        return np.tile(np.asarray(R, np.float64), (P, 1, 1)), np.tile(np.asarray(t, np.float64), (P, 1))
    return pose


def general(noise_free=True, F=8, N=200, seed=40):
    """The well-conditioned family in this module's form (cloud 2-20 m, rotation <= 30 deg, baseline 0.2-1.5 m)."""
    return _build(seed, F, N, noise_free, _pose_general, _cloud)


def zero_baseline_rotation(noise_free=True, F=8, N=200, seed=41):
    """(a) t = 0 with a 0.27 rad rotation about a random axis."""
    return _build(seed, F, N, noise_free, lambda rng, P: (_rot(rng, P, 0.27), np.zeros((P, 3))), _cloud)


def identity(noise_free=True, F=8, N=200, seed=42):
    """(b) R = I, t = 0: the same view twice."""
    return _build(seed, F, N, noise_free, _fixed(np.eye(3), np.zeros(3)), _cloud)


def baseline_1e6(noise_free=True, F=8, N=200, seed=43):
    """(c) baseline 1e-6 m, rotation <= 30 deg."""
    return _build(seed, F, N, noise_free, lambda rng, P: (_rot(rng, P), _trans(rng, P, 1e-6, 1e-6)), _cloud)


def baseline_1e3(noise_free=True, F=8, N=200, seed=44):
    """(d) baseline 1e-3 m, rotation <= 30 deg."""
    return _build(seed, F, N, noise_free, lambda rng, P: (_rot(rng, P), _trans(rng, P, 1e-3, 1e-3)), _cloud)


def forward(noise_free=True, F=8, N=200, seed=45):
    """(e) t = (0, 0, 1), R = I: the epipole is in the image."""
    return _build(seed, F, N, noise_free, _fixed(np.eye(3), [0.0, 0.0, 1.0]), _cloud)


def sideways(noise_free=True, F=8, N=200, seed=46):
    """(f) t = (1, 0, 0), R = I: the epipole at infinity."""
    return _build(seed, F, N, noise_free, _fixed(np.eye(3), [1.0, 0.0, 0.0]),
                  lambda rng, n: _cloud(rng, n, 3.0, 20.0))


def roll_pi(noise_free=True, F=8, N=200, seed=47):
    """(g) roll of pi about the optical axis, baseline 0.2-1.5 m."""
    return _build(seed, F, N, noise_free,
                  lambda rng, P: (np.tile(np.diag([-1.0, -1.0, 1.0]), (P, 1, 1)), _trans(rng, P)),
                  lambda rng, n: _cloud(rng, n, 3.0, 20.0))


def _plane(a, b):
    def scene(rng, n):
        xy = rng.uniform(-0.6 * 8, 0.6 * 8, (n, 2))
        return np.c_[xy, 8.0 + a * xy[:, 0] + b * xy[:, 1]]
    return scene


def tilted_plane(noise_free=True, F=8, N=200, seed=74):
    """(h) every planted point on the plane z = 8 + 0.3 x - 0.2 y. A plane admits a second essential matrix that
    fits every point on it (the homography's other decomposition); on about a third of the seeds the 2D-2D RANSAC
    returns that twin for one of the four pairs and the 1-point recovery then keeps only part of the planted set.
    Seed 74 is one where all four pairs resolve to the planted pose."""
    return _build(seed, F, N, noise_free, _pose_general, _plane(0.3, -0.2))


def fronto_plane(noise_free=True, F=8, N=200, seed=49):
    """(i) every planted point on the plane z = 8 exactly (match frame)."""
    return _build(seed, F, N, noise_free, _pose_general, _plane(0.0, 0.0))


def far_scene(noise_free=True, F=8, N=200, seed=50):
    """(j) depth 1e4-2e4 m."""
    return _build(seed, F, N, noise_free, _pose_general, lambda rng, n: _cloud(rng, n, 1e4, 2e4))


def collinear(noise_free=True, F=8, N=200, seed=51):
    """(k) every planted point on one line."""
    def scene(rng, n):
        p0 = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), 9.0])
        d = _unit(np.array([1.0, rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3)]))
        return p0 + rng.uniform(-4.0, 4.0, n)[:, None] * d
    return _build(seed, F, N, noise_free, _pose_general, scene)


def three_points(noise_free=True, F=8, N=200, seed=52):
    """(l) three distinct scene points, repeated."""
    def scene(rng, n):
        return _cloud(rng, 3, 5.0, 15.0)[np.arange(n) % 3]
    return _build(seed, F, N, noise_free, _pose_general, scene)


FAMILIES = {
    "a": zero_baseline_rotation, "b": identity, "c": baseline_1e6, "d": baseline_1e3, "e": forward, "f": sideways,
    "g": roll_pi, "h": tilted_plane, "i": fronto_plane, "j": far_scene, "k": collinear, "l": three_points,
}


def planted_correspondences(pool: LcdPool, K: int):
    """Exact correspondence lists for verify_matches / O.lcd_verify_pairs: the
    planted candidates (even indices) with the first K planted pairs each.
    Returns (cand_query, cand_match, [(iq, im), ...])."""
    cq = np.ascontiguousarray(pool.cand_query[0::2])
    cm = np.ascontiguousarray(pool.cand_match[0::2])
    corr = [(np.ascontiguousarray(pool.true_idx[k, :K, 0]), np.ascontiguousarray(pool.true_idx[k, :K, 1]))
            for k in range(cq.shape[0])]
    return cq, cm, corr


def planted_samples(pool: LcdPool, n: int, seed: int):
    """n planted 5-samples (f_query [5, 3], f_match [5, 3], pair index) for the
    5-point solvers, drawn over the pool's pairs in turn."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    P, nt = pool.true_idx.shape[:2]
    for s in range(n):
        k = s % P
        sel = rng.choice(nt, 5, replace=False)
        iq, im = pool.true_idx[k, sel, 0], pool.true_idx[k, sel, 1]
        out.append((pool.bearings[2 * k, iq].copy(), pool.bearings[2 * k + 1, im].copy(), k))
    return out


def as_dict(r):
    """A result record (the detector's dict or the restatement's struct) as a dict."""
    if isinstance(r, dict):
        return r
    return {"n_matches": r.n_matches, "mono_inliers": r.mono_inliers, "stereo_inliers": r.stereo_inliers,
            "pnp_inliers": r.pnp_inliers, "iterations_2d2d": r.iterations_2d2d, "accepted": bool(r.accepted),
            "T_query_match": np.array(r.T_query_match[:])}


def check_invariants(results, masks, max_iterations, pnp, stages=3):
    """Properties of a verification result that hold whatever the geometry,
    checked without the restatement: the inlier counts are the masks'
    popcounts, no mask bit at or beyond n_matches, the iteration cap, and an
    accepted candidate has a finite, proper rotation and a finite translation."""
    for i, r in enumerate(results):
        r = as_dict(r)
        m = masks[i]
        n = r["n_matches"]
        assert 0 <= n <= m.shape[0], i
        assert not m[n:].any(), i
        assert not (m & ~np.uint8(3)).any(), i
        if stages & 1:
            assert int(np.count_nonzero(m & 1)) == r["mono_inliers"], i
            assert 0 <= r["iterations_2d2d"] <= max_iterations + 1, i
        if stages & 2:
            assert int(np.count_nonzero(m & 2)) == (r["pnp_inliers"] if pnp else r["stereo_inliers"]), i
            assert (r["stereo_inliers"] if pnp else r["pnp_inliers"]) == 0, i
        if r["accepted"]:
            T = np.asarray(r["T_query_match"], np.float64)
            assert np.isfinite(T).all(), i
            R = T[:9].reshape(3, 3)
            assert np.abs(R.T @ R - np.eye(3)).max() < 1e-9, i
            assert np.linalg.det(R) > 0, i
