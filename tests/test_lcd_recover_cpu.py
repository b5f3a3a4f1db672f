"""The 1-point 3D-3D recovery of the LCD restatement (oracle/lcd_oracle.c)
against a plain numpy reference (tests/lcd_recover_ref.py) at every size
class of the GPU's multi-wave count, without a GPU: 1 to 1024 pairs, the
answer placed late in the list, in the final partly filled block of 64, behind
NaN points, in the larger of two clusters, and on a tie.

All comparisons are exact: inlier counts, acceptance and masks as integers,
the translation bit for bit (the reference keeps the restatement's operation
order; nothing is fused on either side).

Each scene is also checked from the reference alone to be what it claims (the
first maximum at an index >= 512, inside the last block, a tie), so a change
to a builder cannot quietly turn a case into an easy one. last_block with a
single pair in its final block (K = 64 b + 1, K > 1) cannot claim that: the
lone member's count of 1 ties with every outlier's and the first index wins;
there the claim checked is that tie."""
from functools import lru_cache

import numpy as np
import pytest

import lcd_recover_ref as RR
from kmx.lcd.detector import LcdParams
from oracle import oracle as O


@lru_cache(maxsize=None)
def _pool(K, N):
    return RR.recover_pool(K, N)


def check_scene_claim(name, K, ref):
    """What the scene is there for, stated from the reference alone."""
    last0 = RR.BLOCK * ((K + RR.BLOCK - 1) // RR.BLOCK - 1)
    top = int(ref.cnt.max()) if K else 0
    if name == "all_consistent":
        assert ref.best == 0 and ref.stereo_inliers == K
    elif name == "last_block":
        if K - last0 >= 2 or K == 1:
            assert ref.best == last0 and ref.stereo_inliers == K - last0
        else:  # a lone member ties with every outlier
            assert ref.best == 0 and top == 1 and ref.cnt[last0] == 1
    elif name == "late":
        assert ref.best == RR.LATE >= 512 and ref.stereo_inliers == K - RR.LATE
        assert ref.cnt[:RR.LATE].max() == 1
    elif name == "nan_front":
        assert ref.best == RR.NAN_FRONT >= 512 and ref.stereo_inliers == K - RR.NAN_FRONT
        assert not ref.valid[:RR.NAN_FRONT].any() and ref.valid[RR.NAN_FRONT:].all()
    elif name == "bigger_late":
        s = min(100, K - 513)
        assert ref.best == K - (s + 1) >= 512 and ref.stereo_inliers == s + 1
        assert ref.cnt[:512].max() == s and ref.cnt[10] == s  # the smaller cluster starts in block 0
    elif name == "tie_late":
        assert ref.best == 700 and ref.cnt[700] == ref.cnt[705] == top
        assert (700 % RR.BLOCK, 705 % RR.BLOCK) == (60, 1)
        assert not ref.mask[705] and ref.cnt[:700].max() == 1
    elif name.startswith("interleaved"):
        s = (K - 1) // 2
        assert ref.stereo_inliers == top == s + 1
        assert np.count_nonzero(ref.cnt == s) >= s  # the smaller cluster is there (s = 1: and the outlier)
    elif name == "all_invalid":
        assert ref.best == -1 and ref.stereo_inliers == 0 and not ref.accepted
        assert np.array_equal(RR.bits(ref.t), RR.bits(np.zeros(3)))
    else:
        raise KeyError(name)


def test_grid_holds_every_scene_above_512():
    """The grid reaches each scene at a size above 512 pairs."""
    for name in RR.SCENES:
        assert any(RR.fits(name, K) and K > 512 for K in RR.K_GRID), name
    assert RR.scenes_for(1024) == list(RR.SCENES)


def test_reference_on_a_known_answer():
    """recover_1point by hand: R = I, three pairs at t = (1, 2, 3), one far, one NaN."""
    pm = np.array([[0, 0, 5], [1, 0, 6], [0, 1, 7], [2, 2, 8], [1, 1, 9]], np.float64)
    pq = pm + np.array([1.0, 2.0, 3.0])
    pq[0] += 50.0
    pq[3, 1] = np.nan
    r = RR.recover_1point(np.eye(3), pq, pm, 0.3, 3)
    assert r.cnt.tolist() == [1, 3, 3, 0, 3] and r.best == 1
    assert r.mask.tolist() == [False, True, True, False, True] and r.accepted
    assert np.array_equal(r.t, [1.0, 2.0, 3.0])
    assert not RR.recover_1point(np.eye(3), pq, pm, 0.3, 4).accepted


@pytest.mark.parametrize("K", RR.K_GRID)
def test_restatement_equals_numpy_reference(K):
    p = LcdParams(refine_pose=0)
    for N in RR.pool_sizes(K):
        pool = _pool(K, N)
        names = RR.scenes_for(K)
        n = len(names)
        pr = np.stack([RR.prior(pool, k) for k in range(n)])
        res, masks = O.lcd_verify_pairs(p.to_c(), pool, pool.cand_query, pool.cand_match, RR.identity_pairs(pool, K),
                                        stages=2, T_prior=pr)
        for k, name in enumerate(names):
            ref = RR.reference(pool, k, K)
            check_scene_claim(name, K, ref)
            RR.check_against_reference(res[k], masks[k], pool, k, K, ref)


@pytest.mark.parametrize("algo", [0, 1], ids=["stewenius", "nister"])
@pytest.mark.parametrize("K", [600, 1024])
def test_wrong_depth_full_chain(K, algo):
    """stages = 3 on plain inputs: every pair a 2D-2D inlier, the 3D inliers
    only from index 520 on."""
    pool = RR.wrong_depth_pool(K)
    p = LcdParams(refine_pose=0, ransac_2d2d_algorithm=algo)
    res, masks = O.lcd_verify_pairs(p.to_c(), pool, pool.cand_query, pool.cand_match, RR.identity_pairs(pool, K),
                                    stages=3)
    r, m = res[0], masks[0]
    assert r.mono_inliers > 512 and r.mono_inliers == K
    in3 = np.flatnonzero(m & 2)
    assert in3.size == r.stereo_inliers and r.accepted
    assert in3[0] >= 512 and in3[0] == RR.LATE
    assert r.stereo_inliers == K - RR.LATE
    # the numpy reference on the restatement's own rotation
    ref = RR.recover_1point(np.array(r.T_query_match[:9]), pool.points[0, :K], pool.points[1, :K])
    assert ref.best == RR.LATE and np.array_equal(ref.mask, (m[:K] & 2) != 0)
    assert np.array_equal(RR.bits(np.array(r.T_query_match[9:])), RR.bits(ref.t))
