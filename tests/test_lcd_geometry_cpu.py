"""The LCD restatement (oracle/lcd_oracle.c) on degenerate and ill-conditioned
geometry (tests/lcd_scenes.py), without a GPU.

Known answers. Families a-h, noise-free, under the 1-point and the Arun
recoveries and both 2D-2D algorithms: every planted pair is accepted with the
planted pose (R within 1e-7, t within 1e-6: test_verify_noise_free_pool's
bars), the planted correspondences that passed Lowe's test are a subset of the
2D-2D inliers and are exactly the 3D inliers. The tilted plane (h) under EPnP
holds test_verify_pnp_noise_free_pool's 1e-9 / 1e-8.

Recorded behaviour where the geometry does not decide the pose (i under EPnP,
j under the 1-point recovery, k, l): pinned as it is, see DESIGN.md.

5-point solvers against a 40-digit reference (tests/lcd_fivept_ref.py; 80
digits on a and c, where 40 are not converged; its results are read from
tests/golden/lcd_fivept_ref.npz and two samples per family recomputed), 30
planted samples per family (general, a, c, d, e, h, i, j), both algorithms.
A sample is dropped where a real reference solution's eigenvalue lies within
1e-6 of another eigenvalue (no sample is: 0 of 30 in every family). On the
kept samples every real reference solution must have an O.fivept solution
within 100 kappa 2^-52 (kappa: the reference's condition estimate; 100 = n^2
of the 10 x 10 eigen stage and the elimination), Nister must return as many
solutions as the reference has real ones and Stewenius real ones plus complex
pairs.

Measured (worst err / (kappa 2^-52) per family; Stewenius / Nister; bound 100):

    general  1.4e5 / 9.3e8      e  1.7e3 / 2.6e7
    a        4.1e4 / 5.8e4      h  8.9e6 / 1.8e11
    c        3.4e10 / 4.2e10    i  1.8e5 / 1.9e9
    d        4.3e11 / 1.5e13    j  1.1e12 / 7.0e12

No family meets the bound. The medians on the general family are 5.9
(Stewenius) and 16 (Nister); 17 % / 38 % of its solutions are above 100. The
loss is the published methods', not a defect of the restatement: the same
formulation (lcd_fivept_ref) run at 16 digits instead of 40 has errors of the
same size, sample by sample (general: median 5e-15, worst 3e-11, against the
restatement's 4e-14 / 3e-10, log-correlation 0.87; c: both O(1)). The
elimination of the 10 x 20 system and the eigenvectors of the action matrix
have their own conditioning, which is not the solution's: at baseline 1e-6 the
planted solution has kappa ~ 1e7 (an error of 1e-9 would be backward stable)
while the system is within 1e-7 of one with a three-parameter family of
solutions. So the bound tests are strict xfails whose reasons carry the ratios;
the counts hold on general, e, h, i and are strict xfails on a, c, d, j (near
double roots decided differently in double precision), with the recorded
number of misses as an upper bound. What does pin the solvers:
test_stewenius_loses_no_more_than_its_method (within 100 times the 16-digit
run, every family) and test_fivept_typical_solution_within_conditioning
(median ratio within 100 and every solution to 1e-5 on general and e)."""
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import lcd_fivept_ref as REF
import lcd_scenes as S
from kmx.lcd.detector import LcdParams
from oracle import oracle as O

EPS = 2.0 ** -52
N_SAMPLES = 30


def _params(algo, recovery):
    return LcdParams(ransac_2d2d_algorithm=algo, pose_recovery_type=int(recovery == 1),
                     ransac_use_1point_3d3d=int(recovery != 2), refine_pose=int(recovery != 1))


@lru_cache(maxsize=None)
def _pool(fam):
    return S.general() if fam == "general" else S.FAMILIES[fam]()


def _verify(fam, algo, recovery):
    """Per planted pair: (result, pose errors, planted set that passed Lowe, 2D-2D inliers, 3D inliers)."""
    pool = _pool(fam)
    res, masks = O.lcd_verify(_params(algo, recovery).to_c(), pool)
    out = []
    for c in range(0, len(res), 2):
        k = c // 2
        T = np.array(res[c].T_query_match[:])
        eR = np.abs(T[:9].reshape(3, 3) - pool.R_qm[k]).max()
        et = np.abs(T[9:] - pool.t_qm[k]).max()
        pairs = O.knn2(0, 0.7, pool.desc[c], pool.desc[c + 1])
        true = {tuple(x) for x in pool.true_idx[k].tolist()} & {tuple(x) for x in pairs.tolist()}
        in2 = {tuple(pairs[j]) for j in range(len(pairs)) if masks[c, j] & 1}
        in3 = {tuple(pairs[j]) for j in range(len(pairs)) if masks[c, j] & 2}
        out.append((res[c], eR, et, true, in2, in3))
    assert not any(res[c].accepted for c in range(1, len(res), 2))  # the unrelated pairs
    return out


@pytest.mark.parametrize("algo", [0, 1], ids=["stewenius", "nister"])
@pytest.mark.parametrize("recovery", [0, 2], ids=["1point", "arun"])
@pytest.mark.parametrize("fam", list("abcdefgh"))
def test_known_answers(fam, recovery, algo):
    for k, (r, eR, et, true, in2, in3) in enumerate(_verify(fam, algo, recovery)):
        print(f"{fam} pair {k}: mono {r.mono_inliers} stereo {r.stereo_inliers} |dR| {eR:.1e} |dt| {et:.1e}")
        assert r.accepted, k
        assert eR < 1e-7 and et < 1e-6, (k, eR, et)
        assert len(true) >= 95
        assert true <= in2, k
        assert in3 == true, k
        assert r.mono_inliers == len(in2) and r.stereo_inliers == len(in3)


@pytest.mark.parametrize("algo", [0, 1], ids=["stewenius", "nister"])
def test_tilted_plane_epnp(algo):
    for k, (r, eR, et, true, in2, in3) in enumerate(_verify("h", algo, 1)):
        print(f"h pair {k}: mono {r.mono_inliers} pnp {r.pnp_inliers} |dR| {eR:.1e} |dt| {et:.1e}")
        assert r.accepted and r.stereo_inliers == 0, k
        assert eR < 1e-9 and et < 1e-8, (k, eR, et)
        assert true <= in2 and in3 == true, k
        assert r.pnp_inliers == len(in3)


@pytest.mark.parametrize("algo", [0, 1], ids=["stewenius", "nister"])
def test_recorded_behaviour_where_geometry_does_not_decide(algo):
    """Not known answers: what the path does today ("LCD on
    degenerate geometry"). Every planted pair still passes the 2D-2D stage
    with the planted set among its inliers."""
    for fam, rec in (("i", 1), ("j", 0), ("k", 0), ("k", 1), ("k", 2), ("l", 0), ("l", 1), ("l", 2)):
        for r, eR, et, true, in2, in3 in _verify(fam, algo, rec):
            assert true <= in2 or fam == "i", fam
            assert r.mono_inliers >= 95
    # i, EPnP: the control points' PCA has an exact zero eigenvalue; no pair recovers the planted pose
    got = _verify("i", algo, 1)
    assert sum(bool(r.accepted) for r, *_ in got) <= 1
    assert all(eR > 0.05 for _, eR, *_ in got)
    assert sum(r.pnp_inliers == 0 for r, *_ in got) >= 3
    # j, 1-point: accepted with the planted pose (the refit), but the recovery keeps a fraction of the planted set
    got = _verify("j", algo, 0)
    assert all(r.accepted and eR < 1e-7 and et < 1e-9 for r, eR, et, *_ in got)
    assert min(r.stereo_inliers for r, *_ in got) < 30
    # j, Arun and EPnP: the planted set exactly
    for rec in (1, 2):
        assert all(r.accepted and in3 == true for r, _, _, true, _, in3 in _verify("j", algo, rec))
    # k (collinear), l (three points): accepted with a pose that is not the planted one
    for fam in "kl":
        got = _verify(fam, algo, 0)
        assert all(r.accepted for r, *_ in got)
        assert all(eR > 0.05 for _, eR, *_ in got)
    # l under Arun: three distinct points do determine the rigid motion
    assert all(r.accepted and eR < 1e-12 and et < 1e-12 and in3 == true
               for r, eR, et, true, _, in3 in _verify("l", algo, 2))


# ------------------------------------------------- 5-point vs the reference --
FIVEPT_FAMILIES = ["general", "a", "c", "d", "e", "h", "i", "j"]
# worst err / (kappa 2^-52), (Stewenius, Nister), measured on this restatement
RATIO = {"general": (1.4e5, 9.3e8), "a": (4.1e4, 5.8e4), "c": (3.4e10, 4.2e10), "d": (4.3e11, 1.5e13),
         "e": (1.7e3, 2.6e7), "h": (8.9e6, 1.8e11), "i": (1.8e5, 1.9e9), "j": (1.1e12, 7.0e12)}
# samples of 30 whose solution count differs from the reference's (Stewenius, Nister)
COUNT_MISSES = {"a": (17, 24), "c": (20, 26), "d": (5, 18), "j": (12, 15)}


GOLDEN = Path(__file__).parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_lcd_fivept_ref as MK  # noqa: E402  (the fixture's generator: its sample list and record())


@lru_cache(maxsize=None)
def _fixture():
    return np.load(GOLDEN / "lcd_fivept_ref.npz")


@lru_cache(maxsize=None)
def _reference(fam):
    """[(f1, f2, solutions with kappa and the 16-digit run's E16)] for the family's planted samples, from
    tests/golden/lcd_fivept_ref.npz (made by make_lcd_fivept_ref.py; test_reference_fixture_is_current)."""
    z = _fixture()
    samples = MK.samples(fam)
    out = []
    for s, (f1, f2, _) in enumerate(samples):
        assert np.array_equal(f1, z[f"{fam}_f1"][s]) and np.array_equal(f2, z[f"{fam}_f2"][s]), "stale fixture"
        sols = [REF.Solution(E=z[f"{fam}_E"][s, i], eig=complex(z[f"{fam}_eig"][s, i]), real=bool(z[f"{fam}_real"][s, i]),
                             sep=float(z[f"{fam}_sep"][s, i]), kappa=float(z[f"{fam}_kappa"][s, i])) for i in range(10)]
        out.append((f1, f2, sols, z[f"{fam}_E16"][s]))
    return out


@pytest.mark.parametrize("fam", FIVEPT_FAMILIES)
def test_reference_fixture_is_current(fam):
    """Two samples per family recomputed with the reference (40 / 80 digits,
    kappa, and the 16-digit run) equal the stored record."""
    z = _fixture()
    samples = MK.samples(fam)
    for s in (0, 17):
        rec = MK.record(fam, s, samples[s][0], samples[s][1])
        assert np.array_equal(rec["real"], z[f"{fam}_real"][s])
        assert np.allclose(rec["E"], z[f"{fam}_E"][s], rtol=0, atol=1e-15)
        assert np.allclose(rec["eig"], z[f"{fam}_eig"][s], rtol=1e-12, atol=0)
        assert np.allclose(rec["sep"], z[f"{fam}_sep"][s], rtol=1e-12, atol=0)
        assert np.allclose(rec["kappa"], z[f"{fam}_kappa"][s], rtol=1e-9, atol=0, equal_nan=True)
        assert np.allclose(rec["E16"], z[f"{fam}_E16"][s], rtol=0, atol=1e-15)


def _kept(fam):
    return [r for r in _reference(fam) if all(x.sep > 1e-6 for x in r[2] if x.real)]


def _dist(A, B):
    return min(np.abs(A - B).max(), np.abs(A + B).max())


@pytest.mark.parametrize("fam", FIVEPT_FAMILIES)
def test_fivept_separation_rule_drops_few(fam):
    ref = _reference(fam)
    assert len(ref) == N_SAMPLES and all(len(sols) == 10 for _, _, sols, _ in ref)
    for _, _, sols, _ in ref:  # complex solutions come in conjugate pairs
        assert (10 - sum(x.real for x in sols)) % 2 == 0
    dropped = N_SAMPLES - len(_kept(fam))
    print(f"{fam}: dropped {dropped} of {N_SAMPLES}")
    assert dropped <= N_SAMPLES // 10


def _count_marks():
    out = []
    for fam in FIVEPT_FAMILIES:
        for algo, name in ((0, "stewenius"), (1, "nister")):
            marks = []
            if fam in COUNT_MISSES:
                marks = [pytest.mark.xfail(strict=True, reason=f"{COUNT_MISSES[fam][algo]} of 30 samples differ in "
                                           "count: near-double roots decided differently in double precision")]
            out.append(pytest.param(fam, algo, id=f"{fam}-{name}", marks=marks))
    return out


@pytest.mark.parametrize("fam,algo", _count_marks())
def test_fivept_solution_counts(fam, algo):
    miss = 0
    for f1, f2, sols, _ in _kept(fam):
        nreal = sum(x.real for x in sols)
        want = nreal + ((10 - nreal) // 2 if algo == 0 else 0)
        miss += len(O.fivept(f1, f2, algo)) != want
    print(f"{fam} algo {algo}: {miss} of {len(_kept(fam))} samples differ in count")
    assert miss == 0


def _bound_marks():
    out = []
    for fam in FIVEPT_FAMILIES:
        for algo, name in ((0, "stewenius"), (1, "nister")):
            out.append(pytest.param(fam, algo, id=f"{fam}-{name}", marks=pytest.mark.xfail(
                strict=True, reason=f"worst err / (kappa 2^-52) = {RATIO[fam][algo]:.1e} > 100: the method's loss "
                "(elimination and eigenvector conditioning), see the module docstring")))
    return out


@pytest.mark.parametrize("fam,algo", _bound_marks())
def test_fivept_within_conditioning(fam, algo):
    worst, ratios = 0.0, []
    for f1, f2, sols, _ in _kept(fam):
        Es = [E / np.linalg.norm(E) for E in O.fivept(f1, f2, algo)]
        for x in sols:
            if x.real:
                err = min((_dist(E, x.E) for E in Es), default=2.0)
                ratios.append(err / (x.kappa * EPS))
    worst = max(ratios)
    print(f"{fam} algo {algo}: worst err / (kappa 2^-52) = {worst:.3g}, median {np.median(ratios):.3g}, "
          f"{np.mean(np.array(ratios) > 100):.0%} above 100")
    assert worst <= 100.0


def _errors(fam, algo):
    """Per real reference solution of the kept samples: (error of O.fivept's nearest solution, error of the
    16-digit run's nearest solution, kappa)."""
    out = []
    for f1, f2, sols, E16 in _kept(fam):
        Es = [E / np.linalg.norm(E) for E in O.fivept(f1, f2, algo)]
        for x in sols:
            if x.real:
                out.append((min((_dist(E, x.E) for E in Es), default=2.0), min(_dist(E, x.E) for E in E16), x.kappa))
    return np.array(out)


@pytest.mark.parametrize("fam", FIVEPT_FAMILIES)
def test_stewenius_loses_no_more_than_its_method(fam):
    """The claim behind the xfails above, checked: the restatement's Stewenius
    errs like the published formulation itself does in double precision. The
    yardstick is lcd_fivept_ref run at 16 digits (the same null space, cubics,
    elimination and action matrix; mpmath's own QR eigen-solver) against the
    40-digit solutions. Two correct implementations of one pipeline differ by
    the rounding of their stages, for which the issue's factor is n^2 = 100
    (the 10 x 10 eigen stage and the elimination); so over a family's real
    reference solutions the median and the worst error of O.fivept stay
    within 100 times the 16-digit run's (floored at 2^-52). A wrong constant,
    a lost pivot or an unconverged eigenvalue in the restatement puts it
    orders of magnitude outside; measured factors are 1 to 7 (median) and 1
    to 16 (worst) on the eight families."""
    e = _errors(fam, 0)
    med, med16 = np.median(e[:, 0]), max(np.median(e[:, 1]), EPS)
    worst, worst16 = e[:, 0].max(), max(e[:, 1].max(), EPS)
    print(f"{fam}: median {med:.1e} vs {med16:.1e} at 16 digits, worst {worst:.1e} vs {worst16:.1e}")
    assert med <= 100.0 * med16
    assert worst <= 100.0 * worst16


@pytest.mark.parametrize("algo", [0, 1], ids=["stewenius", "nister"])
@pytest.mark.parametrize("fam", ["general", "e"])
def test_fivept_typical_solution_within_conditioning(fam, algo):
    """Where the problem is well conditioned (general, e: median kappa ~ 20)
    the issue's bound holds for the typical solution, if not for the worst:
    the median of err / (kappa 2^-52) is within 100 (measured 5.9 / 16 and
    6.5 / 9.8), and every real reference solution is found to 1e-5, the bar
    of test_fivept_stewenius_contains_every_real_solution. Nister's
    degree-10 polynomial loses more than that on the other families (h:
    median 2e4, worst error 3e-3); there only the GPU parity pins it."""
    e = _errors(fam, algo)
    ratio = e[:, 0] / (e[:, 2] * EPS)
    print(f"{fam} algo {algo}: median ratio {np.median(ratio):.3g}, worst error {e[:, 0].max():.1e}")
    assert np.median(ratio) <= 100.0
    assert e[:, 0].max() < 1e-5


@pytest.mark.parametrize("fam", sorted(COUNT_MISSES))
@pytest.mark.parametrize("algo", [0, 1], ids=["stewenius", "nister"])
def test_fivept_count_misses_do_not_grow(fam, algo):
    """The count xfails above would stay xfailed if every sample miscounted:
    the recorded number of miscounting samples is an upper bound."""
    miss = 0
    for f1, f2, sols, _ in _kept(fam):
        nreal = sum(x.real for x in sols)
        want = nreal + ((10 - nreal) // 2 if algo == 0 else 0)
        miss += len(O.fivept(f1, f2, algo)) != want
    assert miss <= COUNT_MISSES[fam][algo]
