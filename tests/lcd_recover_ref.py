"""A plain reference of the 1-point 3D-3D recovery, and scenes that put its
answer where a kernel can lose it.

recover_1point is numpy float64 and shares nothing with oracle/lcd_oracle.c:
given the 2D-2D rotation and the stereo points of the K pairs in pair order it
forms T_j = p_q - R p_m, counts for every valid i the valid j within thr3d of
it, takes the first maximum and averages the T_j of its inliers in pair order.
Every operation is written in the order the restatement and lcd.hip use, none
is fused, so counts, indices and masks are equal as integers and the
translation bit for bit: no tolerance belongs to a comparison against it.

The scenes build an LcdPool directly (no make_lcd_pool): one pair of frames
per scene, N feature slots, identity correspondences iq = im = arange(K). The
bearings of every pair are exact under the scene's pose (p_q = R p_m + t), so
the 2D-2D stage finds every pair an inlier; only the query stereo points say
which pairs are 3D-consistent. A pair's translation T_j is either a cluster
member (centre + N(0, 1e-3) per axis) or an outlier on a 3 m lattice that
starts 30 m from every cluster: with thr3d 0.3 no outlier is consistent with
another pair. Without the 2D-2D stage the rotation is passed as T_prior
(t = 0). Seeds are fixed.

    all_consistent  one cluster over every pair (the whole j range)
    last_block      only indices >= 64 (ceil(K / 64) - 1): the final,
                    partly filled block of 64
    late            only indices >= 520 (K > 525)
    nan_front       one cluster over every pair; pairs 0..514 have a NaN in
                    the query point (even index) or the match point (odd)
    bigger_late     clusters of s and s + 1: the smaller from index 10, the
                    larger in the last s + 1 indices, all >= 512
    tie_late        two equal clusters in alternating runs of five from index
                    700: their first members are 700 (lane 60 of block 10)
                    and 705 (lane 1 of block 11); 700 must win
    interleaved{0,1,2}  clusters of s and s + 1 over a random permutation of
                    all indices (K even: one outlier); the larger must win
    all_invalid     every pair has a NaN: best -1, translation 0
    wrong_depth     (wrong_depth_pool) the first 520 query points scaled by a
                    factor in [1.5, 3] along their ray, as a wrong disparity
                    does: 2D-2D inliers all, 3D inliers only from 520 on
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from kmx.synth.lcd import LcdPool
from kmx.synth.pose_graph import _expm_so3

THR3D = 0.3   # LcdParams.ransac_threshold_3d3d
MIN3D = 5     # LcdParams.min_nr_3d3d_inliers
BLOCK = 64    # the wavefront: k_rs_finish counts blocks of 64 inliers i
LATE = 520
NAN_FRONT = 515

# n3 = K without the 2D-2D stage: every change of the count's wave assignment
# (1, 2, 4, 8 j-ranges; 5, 7, 8, 9, 10, 16 i-blocks) and every n3 mod 4
K_GRID = (1, 4, 5, 63, 64, 65, 128, 129, 256, 257, 320, 321, 448, 449, 511, 512, 513, 515, 576, 577, 640, 1021, 1023,
          1024)

Recovery = namedtuple("Recovery", "T valid cnt best mask stereo_inliers accepted t")


def recover_1point(R, p_query, p_match, thr3d=THR3D, min3d=MIN3D) -> Recovery:
    """R: the rotation (row-major 3x3); p_query / p_match [K, 3]: the stereo
    points of the pairs in pair order (NaN: no stereo depth)."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    pq = np.asarray(p_query, np.float64).reshape(-1, 3)
    pm = np.asarray(p_match, np.float64).reshape(-1, 3)
    K = pq.shape[0]
    T = np.empty((K, 3))
    for i in range(3):
        T[:, i] = pq[:, i] - (R[i, 0] * pm[:, 0] + R[i, 1] * pm[:, 1] + R[i, 2] * pm[:, 2])
    valid = ~(np.isnan(pq).any(axis=1) | np.isnan(pm).any(axis=1))
    thr2 = thr3d * thr3d
    with np.errstate(invalid="ignore"):
        dx = T[None, :, 0] - T[:, None, 0]  # [i, j]: T_j - T_i
        dy = T[None, :, 1] - T[:, None, 1]
        dz = T[None, :, 2] - T[:, None, 2]
        near = (dx * dx + dy * dy + dz * dz < thr2) & valid[None, :] & valid[:, None]
    cnt = near.sum(axis=1).astype(np.int64)
    best = int(np.argmax(cnt)) if K and cnt.max() > 0 else -1  # argmax: the first maximum
    mask = np.zeros(K, bool)
    t = np.zeros(3)
    cc = 0
    if best >= 0:
        mask = near[best].copy()
        s = np.zeros(3)
        for j in np.flatnonzero(mask):  # in pair order
            s = s + T[j]
        cc = int(mask.sum())
        t = s / float(cc)
    return Recovery(T, valid, cnt, best, mask, cc, cc >= min3d, t)


# ------------------------------------------------------------------ scenes --
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _pose(rng):
    axis = _unit(rng.normal(size=3))
    R = _expm_so3((axis * rng.uniform(-np.pi / 6, np.pi / 6))[None])[0]
    t = _unit(rng.normal(size=3)) * rng.uniform(0.2, 1.5)
    return np.ascontiguousarray(R), t


def _cloud(rng, n):
    z = rng.uniform(3.0, 20.0, n)
    return np.c_[rng.uniform(-0.6, 0.6, (n, 2)) * z[:, None], z]


def _lattice(k):
    """Outlier k's translation offset: 3 m apart, 30 m from the clusters."""
    k = np.asarray(k)
    return 30.0 + 3.0 * np.stack([k % 11, (k // 11) % 11, k // 121], axis=-1).astype(np.float64)


CLUSTER_B = np.array([0.0, 10.0, 0.0])  # the second cluster's centre, from the first


def _labels(scene, K, rng):
    """Per pair: 0 / 1 the cluster it belongs to, -1 an outlier; and the pairs
    that get a NaN."""
    lab = np.full(K, -1)
    nan = np.zeros(K, bool)
    idx = np.arange(K)
    if scene == "all_consistent":
        lab[:] = 0
    elif scene == "last_block":
        lab[BLOCK * ((K + BLOCK - 1) // BLOCK - 1):] = 0
    elif scene == "late":
        lab[LATE:] = 0
    elif scene == "nan_front":
        lab[:] = 0
        nan[:NAN_FRONT] = True
    elif scene == "bigger_late":
        s = min(100, K - 513)
        lab[10:10 + s] = 1
        lab[K - (s + 1):] = 0
    elif scene == "tie_late":
        runs = (K - 700) // 10  # runs of five per cluster
        m = idx[700:700 + 10 * runs]
        lab[m] = ((m - 700) // 5) % 2
    elif scene.startswith("interleaved"):
        s = (K - 1) // 2
        perm = rng.permutation(K)
        lab[perm[:s]] = 1
        lab[perm[s:2 * s + 1]] = 0
    elif scene == "all_invalid":
        lab[:] = 0
        nan[:] = True
    else:
        raise KeyError(scene)
    return lab, nan


def fits(scene, K):
    if scene == "late":
        return K > LATE + 5
    if scene == "nan_front":
        return K > NAN_FRONT
    if scene == "bigger_late":
        return K >= 515
    if scene == "tie_late":
        return K >= 710
    if scene.startswith("interleaved"):
        return K >= 3
    return K >= 1


SCENES = ("all_consistent", "last_block", "late", "nan_front", "bigger_late", "tie_late", "interleaved0", "interleaved1",
          "interleaved2", "all_invalid")


def scenes_for(K):
    return [s for s in SCENES if fits(s, K)]


def _empty_pool(F, N, K):
    bearings = np.zeros((F, N, 3))
    bearings[..., 2] = 1.0
    cq = np.arange(0, F, 2, dtype=np.int32)
    ident = np.stack([np.arange(K), np.arange(K)], axis=-1).astype(np.int32)
    return LcdPool(n_frames=F, max_feats=N, n_feats=np.full(F, K, np.int32), desc=np.zeros((F, N, 32), np.uint8),
                   bearings=bearings, points=np.full((F, N, 3), np.nan), cand_query=cq, cand_match=cq + 1,
                   R_qm=np.zeros((F // 2, 3, 3)), t_qm=np.zeros((F // 2, 3)),
                   true_idx=np.ascontiguousarray(np.tile(ident, (F // 2, 1, 1))))


def _plant(pool, k, rng, K):
    """Pair k's pose, match cloud and exact bearings; returns the exact query points."""
    R, t = _pose(rng)
    pm = _cloud(rng, K)
    pq = pm @ R.T + t
    assert pq[:, 2].min() > 0.5, "scene behind the query camera"
    pool.R_qm[k], pool.t_qm[k] = R, t
    pool.bearings[2 * k, :K] = _unit(pq)
    pool.bearings[2 * k + 1, :K] = _unit(pm)
    pool.points[2 * k + 1, :K] = pm
    return pq


def recover_pool(K, N) -> LcdPool:
    """The scenes that fit K (scenes_for(K), in that order) as frame pairs
    (2k, 2k + 1) of one pool of N feature slots; candidate k is scene k."""
    names = scenes_for(K)
    pool = _empty_pool(2 * len(names), N, K)
    for k, name in enumerate(names):
        rng = np.random.Generator(np.random.PCG64([SCENES.index(name), K, 7]))
        pq = _plant(pool, k, rng, K)
        lab, nan = _labels(name, K, rng)
        R, t = pool.R_qm[k], pool.t_qm[k]
        off = np.where((lab >= 0)[:, None], rng.normal(0.0, 1e-3, (K, 3)) + np.where((lab == 1)[:, None], CLUSTER_B, 0.0),
                       _lattice(np.arange(K)))
        pool.points[2 * k, :K] = pq + off  # T_j = t + off_j (to rounding)
        i = np.flatnonzero(nan)
        pool.points[2 * k, i[i % 2 == 0], rng.integers(0, 3)] = np.nan
        pool.points[2 * k + 1, i[i % 2 == 1], rng.integers(0, 3)] = np.nan
    return pool


def wrong_depth_pool(K, N=1024, descriptors=False) -> LcdPool:
    """One pair of frames: bearings exact under one pose, the first 520 query
    points at 1.5 to 3 times their depth. descriptors: both frames carry the
    same K distinct random 256-bit descriptors, so computeMatchedIndices
    yields the identity pairs itself."""
    assert K > LATE
    rng = np.random.Generator(np.random.PCG64([99, K]))
    pool = _empty_pool(2, N, K)
    pq = _plant(pool, 0, rng, K)
    scale = np.ones(K)
    scale[:LATE] = rng.uniform(1.5, 3.0, LATE)
    pool.points[0, :K] = pq * scale[:, None]
    if descriptors:
        d = rng.integers(0, 256, (K, 32), dtype=np.uint8)
        assert np.unique(d, axis=0).shape[0] == K
        pool.desc[0, :K] = d
        pool.desc[1, :K] = d
    return pool


def prior(pool, k):
    """T_prior of candidate k: its planted rotation (row-major), t = 0."""
    return np.r_[pool.R_qm[k].reshape(9), np.zeros(3)]


def identity_pairs(pool, K):
    a = np.arange(K, dtype=np.int32)
    return [(a, a)] * (pool.n_frames // 2)


def reference(pool, k, K, thr3d=THR3D, min3d=MIN3D) -> Recovery:
    """recover_1point on candidate k of a pool with identity pairs and the planted rotation."""
    return recover_1point(pool.R_qm[k], pool.points[2 * k, :K], pool.points[2 * k + 1, :K], thr3d, min3d)


def pool_sizes(K):
    """Feature strides a K is run at: 1024 above 512; below, 1024 and K
    rounded up to 64 (a smaller dynamic LDS size)."""
    return (1024,) if K > 512 else (1024, BLOCK * ((K + BLOCK - 1) // BLOCK))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_against_reference(r, mask, pool, k, K, ref=None):
    """A result record (the restatement's struct or the detector's dict) and
    its mask row against recover_1point on candidate k, refine_pose off."""
    ref = ref or reference(pool, k, K)
    if isinstance(r, dict):
        stereo, acc, T = r["stereo_inliers"], bool(r["accepted"]), np.asarray(r["T_query_match"])
        nm, mono = r["n_matches"], r["mono_inliers"]
    else:
        stereo, acc, T = r.stereo_inliers, bool(r.accepted), np.array(r.T_query_match[:])
        nm, mono = r.n_matches, r.mono_inliers
    assert (nm, mono) == (K, K)
    assert stereo == ref.stereo_inliers, (stereo, ref.stereo_inliers, ref.best)
    assert acc == bool(ref.accepted)
    assert np.array_equal((mask[:K] & 2) != 0, ref.mask), (np.flatnonzero(mask[:K] & 2)[:4], ref.best)
    assert np.array_equal(mask[:K] & 1, np.ones(K, np.uint8))
    assert not mask[K:].any()
    assert np.array_equal(bits(T[9:]), bits(ref.t)), (T[9:], ref.t)
    assert np.array_equal(bits(T[:9]), bits(pool.R_qm[k].reshape(9)))
