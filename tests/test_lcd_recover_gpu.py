"""Pose recovery above 512 inliers (lcd.hip k_rs_finish / fin_count, the
work-queue tail ransac_tail<false>, k_recover) on the scenes of
tests/lcd_recover_ref.py: 1 to 1024 pairs with the largest consistent set
late in the list, in the final partly filled block of 64, behind NaN points,
in the larger of two clusters, on a tie.

k_rs_finish divides the n3 x n3 count over its workgroup's eight waves; above
512 entries there are more blocks of 64 inliers i than waves, and every block
has to be counted all the same. The 1-point recovery is run in three forms:

    one    one candidate per call (the reference's verification thread):
           k_rs_finish and its completion word
    batch  the scenes of a K in calls of up to 8 candidates: k_rs_finish,
           several workgroups
    queue  KMX_LCD_SPREAD=0: the work-queue kernel's serial tail

Each is compared bit for bit with the restatement (oracle/lcd_oracle.c) and,
with refine_pose off, with the numpy reference, which shares nothing with the
restatement. The EPnP and Arun recoveries (k_recover) and the full chain
(stages = 3, verify()) go above 512 entries as well, against the
restatement.

Before fin_count counted every block, 21 of these failed, all in the spread
forms and none in the work queue: test_recover_1point[one-..] and [batch-..]
at K = 515, 576, 577, 640, 1021, 1023, 1024 (the scenes last_block, late,
nan_front, bigger_late, tie_late: e.g. `late` at K = 1024 came back with 1
inlier, rejected, against 504, accepted), test_recover_1point_refine_pose
[one-1024], test_recover_pose_call_late_1024, the four
test_wrong_depth_full_chain cases and test_wrong_depth_through_verify."""
from functools import lru_cache

import numpy as np
import pytest

import lcd_recover_ref as RR
from kmx import abi
from kmx.lcd import LcdParams, LoopClosureDetector

pytestmark = pytest.mark.gpu

FIELDS = ("n_matches", "mono_inliers", "stereo_inliers", "pnp_inliers", "iterations_2d2d")
RECOVER = abi.KMX_LCD_STAGE_RECOVER
GRID = [(K, N) for K in RR.K_GRID for N in RR.pool_sizes(K)]


def _same_as_oracle(got, gm, ref, rm):
    for i, (g, r) in enumerate(zip(got, ref)):
        assert tuple(g[k] for k in FIELDS) == tuple(getattr(r, k) for k in FIELDS), (i, g, r.iterations_2d2d)
        assert g["accepted"] == bool(r.accepted), i
        assert np.array_equal(g["T_query_match"], np.array(r.T_query_match[:])), i
    assert np.array_equal(gm, rm)


class _Det:
    """A detector in one form (KMX_LCD_SPREAD is read when it is created) that
    re-uploads only when the pool changes."""

    def __init__(self, p, spread):
        with pytest.MonkeyPatch.context() as mp:
            if spread is None:
                mp.delenv("KMX_LCD_SPREAD", raising=False)
            else:
                mp.setenv("KMX_LCD_SPREAD", str(spread))
            self.d = LoopClosureDetector(p)
        self.loaded = None

    def on(self, pool):
        if self.loaded is not pool:
            self.d.set_pool(pool)
            self.loaded = pool
        return self.d

    def close(self):
        self.d.close()


@pytest.fixture(scope="module")
def dets(gpu):
    p = LcdParams(refine_pose=0)
    d = {"spread": _Det(p, None), "queue": _Det(p, 0)}
    yield d
    for x in d.values():
        x.close()


@lru_cache(maxsize=None)
def _pool(K, N):
    return RR.recover_pool(K, N)


@lru_cache(maxsize=None)
def _priors(K, N):
    pool = _pool(K, N)
    return np.stack([RR.prior(pool, k) for k in range(pool.n_frames // 2)])


@lru_cache(maxsize=None)
def _oracle(K, N, refine=0):
    """The restatement on every scene of (K, N), stages = RECOVER."""
    from oracle import oracle as O
    pool = _pool(K, N)
    return O.lcd_verify_pairs(LcdParams(refine_pose=refine).to_c(), pool, pool.cand_query, pool.cand_match,
                              RR.identity_pairs(pool, K), stages=RECOVER, T_prior=_priors(K, N))


@lru_cache(maxsize=None)
def _numpy_ref(K, N, k):
    return RR.reference(_pool(K, N), k, K)


def _run(det, pool, K, N, sel, chunk):
    """verify_matches on the candidates `sel`, `chunk` per call."""
    a = np.arange(K, dtype=np.int32)
    pr = _priors(K, N)
    got, gm = [], []
    for i in range(0, len(sel), chunk):
        s = sel[i:i + chunk]
        g, m = det.verify_matches(pool.cand_query[s], pool.cand_match[s], [(a, a)] * len(s), stages=RECOVER,
                                  T_prior=pr[s], with_masks=True)
        got += g
        gm.append(m)
    return got, np.concatenate(gm)


FORMS = {"one": ("spread", 1), "batch": ("spread", 8), "queue": ("queue", 1 << 20)}


@pytest.mark.parametrize("K,N", GRID, ids=[f"K{K}-N{N}" for K, N in GRID])
@pytest.mark.parametrize("form", list(FORMS))
def test_recover_1point(dets, form, K, N):
    which, chunk = FORMS[form]
    pool = _pool(K, N)
    n = pool.n_frames // 2
    got, gm = _run(dets[which].on(pool), pool, K, N, np.arange(n), chunk)
    ref, rm = _oracle(K, N)
    bad = []
    for k, name in enumerate(RR.scenes_for(K)):
        try:
            _same_as_oracle(got[k:k + 1], gm[k:k + 1], [ref[k]], rm[k:k + 1])
            RR.check_against_reference(got[k], gm[k], pool, k, K, _numpy_ref(K, N, k))
        except AssertionError as e:
            bad.append((name, got[k]["stereo_inliers"], ref[k].stereo_inliers, str(e).split("\n")[0][:80]))
    assert not bad, bad  # (scene, kernel's 3D inliers, restatement's, first difference)


@pytest.mark.parametrize("K", [513, 1024])
@pytest.mark.parametrize("form", ["one", "queue"])
def test_recover_1point_refine_pose(gpu, form, K):
    """refine_pose on: the refit sums over up to 1024 staged inliers (Pc)."""
    pool = _pool(K, 1024)
    names = RR.scenes_for(K)
    sel = np.array([names.index(s) for s in ("late", "all_consistent") if s in names])
    ref, rm = _oracle(K, 1024, 1)
    det = _Det(LcdParams(refine_pose=1), None if form == "one" else 0)
    try:
        got, gm = _run(det.on(pool), pool, K, 1024, sel, 1 if form == "one" else 8)
        _same_as_oracle(got, gm, [ref[k] for k in sel], rm[sel])
        assert all(g["accepted"] and g["pose_refined"] for g in got)
        assert max(g["stereo_inliers"] for g in got) == K
    finally:
        det.close()


def test_recover_pose_call_late_1024(dets):
    """recoverPose itself (one candidate, the completion word) on `late` at K = 1024."""
    K = 1024
    pool = _pool(K, 1024)
    k = RR.scenes_for(K).index("late")
    ref = _numpy_ref(K, 1024, k)
    T0 = np.eye(4)
    T0[:3, :3] = pool.R_qm[k]
    a = np.arange(K, dtype=np.int32)
    ok, T, inl = dets["spread"].on(pool).recoverPose(2 * k, 2 * k + 1, a, a, T0)
    assert ok and ref.accepted and ref.best == RR.LATE
    assert np.array_equal(inl, ref.mask)
    assert np.array_equal(T[:3, 3].view(np.uint64), ref.t.view(np.uint64))
    assert np.array_equal(T[:3, :3], pool.R_qm[k])


def _recovery_params(recovery, algo=0, refine=None):
    return LcdParams(ransac_2d2d_algorithm=algo, pose_recovery_type=int(recovery == "pnp"),
                     ransac_use_1point_3d3d=int(recovery != "arun"),
                     refine_pose=int(recovery == "arun") if refine is None else refine)


@pytest.mark.parametrize("K", [513, 1024])
@pytest.mark.parametrize("recovery", ["pnp", "arun"])
def test_k_recover_above_512(gpu, recovery, K):
    """EPnP and Arun RANSAC (k_recover) over more than 512 stereo-valid 2D-2D
    inliers, stages = 3: the spread form one candidate per call and the work
    queue, against the restatement."""
    from oracle import oracle as O
    pool = _pool(K, 1024)
    names = RR.scenes_for(K)
    scenes = [s for s in ("all_consistent", "nan_front", "late") if s in names]
    sel = np.array([names.index(s) for s in scenes])
    p = _recovery_params(recovery)
    a = np.arange(K, dtype=np.int32)
    cq, cm, corr = pool.cand_query[sel], pool.cand_match[sel], [(a, a)] * len(sel)
    ref, rm = O.lcd_verify_pairs(p.to_c(), pool, cq, cm, corr, stages=3)
    for s, k, r, m in zip(scenes, sel, ref, rm):
        valid = ~(np.isnan(pool.points[2 * k, :K]).any(1) | np.isnan(pool.points[2 * k + 1, :K]).any(1))
        seen = int(np.count_nonzero((m[:K] & 1).astype(bool) & valid))  # what the recovery sampled from
        if s == "nan_front":
            assert seen == K - RR.NAN_FRONT == 509
        else:
            assert seen > 512, (s, seen)
        assert r.accepted and (r.pnp_inliers if recovery == "pnp" else r.stereo_inliers) >= 400, s
    for spread in (None, 0):
        det = _Det(p, spread)
        try:
            d = det.on(pool)
            got, gm = [], []
            for ix in [slice(i, i + 1) for i in range(len(sel))] if spread is None else [slice(None)]:
                g, mk = d.verify_matches(cq[ix], cm[ix], corr[ix], stages=3, with_masks=True)
                got += g
                gm.append(mk)
            _same_as_oracle(got, np.concatenate(gm), ref, rm)
        finally:
            det.close()


@pytest.mark.parametrize("algo", [0, 1], ids=["stewenius", "nister"])
@pytest.mark.parametrize("K", [600, 1024])
def test_wrong_depth_full_chain(gpu, K, algo):
    """Plain inputs, stages = 3: every pair a 2D-2D inlier, the first 520 with
    a wrong stereo depth; as a spread call and through the work queue."""
    from oracle import oracle as O
    pool = RR.wrong_depth_pool(K)
    p = _recovery_params("1point", algo, refine=0)
    corr = RR.identity_pairs(pool, K)
    ref, rm = O.lcd_verify_pairs(p.to_c(), pool, pool.cand_query, pool.cand_match, corr, stages=3)
    assert ref[0].mono_inliers > 512 and np.flatnonzero(rm[0] & 2)[0] >= 512 and ref[0].accepted
    for spread in (None, 0):
        det = _Det(p, spread)
        try:
            got, gm = det.on(pool).verify_matches(pool.cand_query, pool.cand_match, corr, stages=3, with_masks=True)
            _same_as_oracle(got, gm, ref, rm)
            # and the numpy reference, given the kernel's own 2D-2D rotation
            r1 = RR.recover_1point(got[0]["T_query_match"][:9], pool.points[0, :K], pool.points[1, :K])
            assert r1.best == RR.LATE and got[0]["stereo_inliers"] == r1.stereo_inliers == K - RR.LATE
            assert np.array_equal((gm[0, :K] & 2) != 0, r1.mask)
            assert np.array_equal(got[0]["T_query_match"][9:].view(np.uint64), r1.t.view(np.uint64))
        finally:
            det.close()


def test_wrong_depth_through_verify(gpu):
    """The same scene through verify(): both frames carry the same 1024
    distinct random descriptors, so computeMatchedIndices yields the pairs."""
    from oracle import oracle as O
    K = 1024
    pool = RR.wrong_depth_pool(K, descriptors=True)
    p = LcdParams(refine_pose=0)
    ref, rm = O.lcd_verify(p.to_c(), pool)
    assert ref[0].n_matches > 512 and ref[0].mono_inliers > 512
    assert ref[0].accepted and np.flatnonzero(rm[0] & 2)[0] >= 512
    for spread in (None, 0):
        det = _Det(p, spread)
        try:
            got, gm = det.on(pool).verify(pool.cand_query, pool.cand_match, with_masks=True)
            _same_as_oracle(got, gm, ref, rm)
        finally:
            det.close()
