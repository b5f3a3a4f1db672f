"""GPU parity of the LCD verification path on degenerate and ill-conditioned
geometry (tests/lcd_scenes.py: zero and tiny baselines, forward and sideways
motion, a roll of pi, planes, a far scene, collinear and repeated points),
noisy and noise-free.

There the 5-point systems are rank-deficient or nearly so, the elimination
meets exact zero pivots (a, b, f: a scratch kernel that treats pivots below
1e-12 as zero fails 18 of these cases and none of the earlier tests) and the
3D fits see rank-deficient cross-covariances (k, l). Not every branch the
families were meant for is separated from the general pool by them: mutating,
in the restatement, the NaN handling of the inlier comparisons, hqr's
zero-diagonal fallback and second exceptional shift, the Sturm remainder
cut-off or the isolation depth changes no result on any family, so a port
difference there would still pass (open gap).

Bar: bit-exact against the restatement (test_verify_bit_exact's: counts,
iterations_2d2d, accepted, masks, T_query_match with equal_nan), through the
work queue (KMX_LCD_SPREAD=0) and the spread form (64), both 2D-2D algorithms,
the three recoveries, and verify_matches at K = 5, 6, 7, 12 planted pairs in
stages 1, 2, 3. Beside it, invariants that do not pass through the
restatement (lcd_scenes.check_invariants) and the rejection of the unrelated
odd candidates."""
from functools import lru_cache

import numpy as np
import pytest

import lcd_scenes as S
from kmx.lcd import LcdParams, LoopClosureDetector

pytestmark = pytest.mark.gpu

FIELDS = ("n_matches", "mono_inliers", "stereo_inliers", "pnp_inliers", "iterations_2d2d", "accepted")
RECOVERY = {"1point": 0, "pnp": 1, "arun": 2}
CASES = [pytest.param(f, nf, id=f"{f}-{'exact' if nf else 'noisy'}") for f in S.FAMILIES for nf in (True, False)]


def _params(algo, recovery, **kw):
    return LcdParams(ransac_2d2d_algorithm=algo, pose_recovery_type=int(recovery == 1),
                     ransac_use_1point_3d3d=int(recovery != 2), refine_pose=int(recovery != 1), **kw)


@lru_cache(maxsize=None)
def _pool(fam, noise_free):
    return S.FAMILIES[fam](noise_free=noise_free)


def _same(got, gm, ref, rm, what):
    for i, (g, r) in enumerate(zip(got, ref)):
        r = S.as_dict(r)
        assert tuple(g[k] for k in FIELDS) == tuple(r[k] for k in FIELDS), (what, i, g, r)
        assert np.array_equal(g["T_query_match"], r["T_query_match"], equal_nan=True), (what, i)
    assert np.array_equal(gm, rm), what


@pytest.mark.parametrize("recovery", list(RECOVERY))
@pytest.mark.parametrize("fam,noise_free", CASES)
def test_verify_bit_exact_on_family(gpu, monkeypatch, fam, noise_free, recovery):
    from oracle import oracle as O
    pool = _pool(fam, noise_free)
    rec = RECOVERY[recovery]
    for algo in (0, 1):
        p = _params(algo, rec)
        ref, rm = O.lcd_verify(p.to_c(), pool)
        for spread in (0, 64):
            monkeypatch.setenv("KMX_LCD_SPREAD", str(spread))
            det = LoopClosureDetector(p)
            try:
                det.set_pool(pool)
                got, gm = det.verify(pool.cand_query, pool.cand_match, with_masks=True)
            finally:
                det.close()
            S.check_invariants(got, gm, p.ransac_max_iterations, rec == 1)
            assert not any(g["accepted"] for g in got[1::2]), (algo, spread)
            _same(got, gm, ref, rm, (algo, spread))


@pytest.mark.parametrize("recovery", list(RECOVERY))
@pytest.mark.parametrize("fam,noise_free", CASES)
def test_verify_matches_bit_exact_on_family(gpu, monkeypatch, fam, noise_free, recovery):
    """Exact correspondence lists of K planted pairs: K = 5 (the sample is
    the list), 6, 7 (a handful of distinct samples) and 12 (enough for the
    2D-2D gate), each stage alone and both; the recovery alone takes the
    restatement's 2D-2D pose as its prior. Under EPnP ransac_max_iterations
    is 60 (the default 500 otherwise): on these short lists its loops run to
    the cap, and the restatement's share of a case would be several seconds."""
    from oracle import oracle as O
    pool = _pool(fam, noise_free)
    rec = RECOVERY[recovery]
    for algo in (0, 1):
        p = _params(algo, rec, **({"ransac_max_iterations": 60} if rec == 1 else {}))
        ref = {}
        for K in (5, 6, 7, 12):
            cq, cm, corr = S.planted_correspondences(pool, K)
            r1 = O.lcd_verify_pairs(p.to_c(), pool, cq, cm, corr, stages=1)
            prior = np.array([S.as_dict(r)["T_query_match"] for r in r1[0]])
            ref[K] = {1: (None, r1), 2: (prior, O.lcd_verify_pairs(p.to_c(), pool, cq, cm, corr, stages=2,
                                                                     T_prior=prior)),
                      3: (None, O.lcd_verify_pairs(p.to_c(), pool, cq, cm, corr, stages=3))}
        for spread in (0, 64):
            monkeypatch.setenv("KMX_LCD_SPREAD", str(spread))
            det = LoopClosureDetector(p)
            try:
                det.set_pool(pool)
                for K in (5, 6, 7, 12):
                    cq, cm, corr = S.planted_correspondences(pool, K)
                    for st in (1, 2, 3):
                        prior, (rr, rm) = ref[K][st]
                        got, gm = det.verify_matches(cq, cm, corr, stages=st, T_prior=prior, with_masks=True)
                        S.check_invariants(got, gm, p.ransac_max_iterations, rec == 1, stages=st)
                        assert all(g["n_matches"] == K for g in got)
                        _same(got, gm, rr, rm, (algo, spread, K, st))
            finally:
                det.close()
