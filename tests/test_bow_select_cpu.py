"""The inputs of the top-K selection tests (tests/bow_query_ref.py), checked
without a device, so that a later change of an input cannot hollow out
test_bow_select_gpu.py:

  * every family reaches the selection depth it claims under every kernel
    form, computed from the reference's results and the grid's constants alone
    (bow_query_ref.levels_needed / base_depth): DEPTH below, per form, for
    K = 1, 50, 256; X = no level under 6 fits the buffer = KMX_EUNSUP;
  * query_l1 equals oracle.OracleBowDb.query with == on n, ids and scores (the
    oracle orders ties by (acc, id) too: qsort_r on exactly that key);
  * query_l1 agrees with score_exact within 4 * c * 2**-52 (c common words:
    three roundings per term on magnitudes up to 2, one per accumulation on
    magnitudes below 4). Largest |acc_ref - acc_exact| / (c * 2**-52) seen:
    0.0 on the two-word and dyadic families (every operation is exact there)
    and 0.17 on the random real-valued vectors of test_rounding_bound;
  * oracle.OracleBowDb refuses weights that are not finite and > 0.
"""
import numpy as np
import pytest

from tests import bow_query_ref as R
from oracle import oracle as O

X = None
# (family, cap): {form: depth for K = 1, 50, 256}; "stream" is the LDS form over
# the first 2000 entries (the rest are the tail, which has no cap)
DEPTH = {
    ("spread", 2048): dict(lds=(0, 0, 0), chunk1100=(0, 0, 0), chunk97=(0, 0, 0), hbm=(0, 0, 0), stream=(0, 0, 0)),
    ("L1", 2048): dict(lds=(1, 1, 1), chunk1100=(1, 1, 1), chunk97=(0, 0, 0), hbm=(1, 1, 1), stream=(1, 1, 1)),
    ("L2", 2048): dict(lds=(2, 2, 2), chunk1100=(2, 2, 2), chunk97=(0, 0, 0), hbm=(2, 2, 2), stream=(2, 2, 2)),
    ("L3", 2048): dict(lds=(3, 3, 3), chunk1100=(3, 3, 3), chunk97=(0, 0, 0), hbm=(3, 3, 3), stream=(3, 3, 3)),
    ("L4", 2048): dict(lds=(4, 4, 4), chunk1100=(4, 4, 4), chunk97=(0, 0, 0), hbm=(4, 4, 4), stream=(4, 4, 4)),
    # a chunk of 1104 holds ~966 entries in the best value's level-0 cell: it fits at once
    ("L5", 2048): dict(lds=(5, 5, 5), chunk1100=(0, 0, 0), chunk97=(0, 0, 0), hbm=(5, 5, 5), stream=(5, 5, 5)),
    ("tied_at_cap", 2048): dict(lds=(X, X, X), chunk1100=(0, 0, 0), chunk97=(0, 0, 0), hbm=(0, 0, 0), stream=(X, X, X)),
    ("tied_at_cap", 1024): dict(lds=(0, 0, 0), chunk1100=(0, 0, 0), chunk97=(0, 0, 0), hbm=(0, 0, 0), stream=(0, 0, 0)),
    ("tied_over_cap", 2048): dict(lds=(X, X, X), chunk1100=(0, 0, 0), chunk97=(0, 0, 0), hbm=(X, X, X),
                                  stream=(X, X, X)),
    ("tied_over_cap", 1024): dict(lds=(X, X, X), chunk1100=(0, 0, 0), chunk97=(0, 0, 0), hbm=(0, 0, 0),
                                  stream=(0, 0, 0)),
    # the cap is per chunk: a chunk of 1104 holds ~22 of the 60 better entries, so K = 50 cuts inside its tie group
    ("past_cut", 2048): dict(lds=(0, 0, X), chunk1100=(0, X, X), chunk97=(0, 0, 0), hbm=(0, 0, X), stream=(0, X, X)),
    # K = 256 takes 60 certain entries at level 0 (need -= cb) and ends at level 1
    ("two_step", 2048): dict(lds=(0, 0, 1), chunk1100=(0, 1, X), chunk97=(0, 0, 0), hbm=(0, 0, 1), stream=(0, 1, X)),
    ("one_chunk_1025", 2048): dict(lds=(X, X, X), chunk1100=(X, X, X), chunk97=(0, 0, 0), hbm=(0, 0, 0),
                                   stream=(X, X, X)),
    ("split_1025", 2048): dict(lds=(X, X, X), chunk1100=(0, 0, 0), chunk97=(0, 0, 0), hbm=(0, 0, 0), stream=(X, X, X)),
    ("dyadic", 2048): dict(lds=(0, 0, 0), chunk1100=(0, 0, 0), chunk97=(0, 0, 0), hbm=(0, 0, 0), stream=(0, 0, 0)),
    # K = 1: the planted best entries have a level-1 cell of their own
    ("lch_edge_14335", 2048): dict(lds=(1, 2, 2), hbm=(1, 2, 2)),
    ("lch_edge_14336", 2048): dict(lds=(1, 2, 2), hbm=(1, 2, 2)),
    ("lch_edge_14337", 2048): dict(lds=(1, 2, 2), hbm=(1, 2, 2)),
}
FORM_DEPTH = dict({k: v["depth"] for k, v in R.FORMS.items()}, stream=dict(lds=True, n_sealed=R.STREAM_SEALED))


def test_every_family_has_its_claims():
    assert set(DEPTH) == set(R.FAMILIES + R.LCH_EDGE)
    for key in R.FAMILIES:
        assert set(DEPTH[key]) == set(FORM_DEPTH), key


@pytest.mark.parametrize("name,cap", R.FAMILIES + R.LCH_EDGE, ids=lambda v: str(v))
def test_family_reaches_its_depth(name, cap):
    f = R.family(name, cap)
    assert f.n == (int(name[9:]) if name.startswith("lch_edge_") else 3000)
    assert (f.weights > 0).all() and np.isfinite(f.weights).all()
    for form, claim in DEPTH[(name, cap)].items():
        got = tuple(R.call_depth(R.expected(name, cap, K), K, **FORM_DEPTH[form]) for K in R.KS)
        assert got == claim, (name, cap, form)
    # the selection grid is exact on these inputs: acc + 2 does not round
    for ids, acc in R.expected(name, cap, 256):
        assert ((acc + 2.0) - 2.0 == acc).all()
    # the queries that follow a refusal are answered by every form
    for K in R.KS:
        for form, fd in FORM_DEPTH.items():
            if f.good:
                assert R.call_depth(R.expected(name, cap, K, good=True), K, **fd) is not None, (name, form, K)


def test_the_hbm_form_reaches_every_level():
    """Levels 0..5 of k_bow_query each end the narrowing of some family, at every K."""
    for K_i in range(3):
        assert {DEPTH[(n, 2048)]["hbm"][K_i] for n in ("spread", "L1", "L2", "L3", "L4", "L5")} == set(range(6))
    assert {d for n in ("spread", "L1", "L2", "L3", "L4", "L5") for d in DEPTH[(n, 2048)]["lds"]} == set(range(6))


def test_two_word_scores_are_placed_to_the_ulp():
    """acc_i == -2 * a_i exactly, for every two-word family."""
    for name, cap in R.FAMILIES + R.LCH_EDGE:
        f = R.family(name, cap)
        if f.n_words != 8:
            continue
        ids, acc = R.all_results(name, cap, 0, -1)
        assert ids.shape[0] == f.n
        assert np.array_equal(acc, -2.0 * f.weights[0::2][ids]), name


def test_tie_structure():
    ids, acc = R.all_results("L4", 2048, 0, -1)
    assert np.unique(acc).shape[0] < 3000  # natural ties
    ids, acc = R.all_results("L5", 2048, 0, -1)
    vals, counts = np.unique(acc, return_counts=True)
    assert vals.shape[0] == 8 and counts.min() > 300
    best = np.sort(np.nonzero(R.family("L5").weights[0::2] == 0.75 + 7 * 2.0 ** -53)[0])
    assert np.array_equal(ids[:256], best[:256])  # the lowest ids of the best value
    for cap in (1024, 2048):
        for name, m in (("tied_at_cap", cap), ("tied_over_cap", cap + 1)):
            ids, acc = R.all_results(name, cap, 0, -1)
            assert int((acc == -2.0 * R.TIED).sum()) == m and (acc[:m] == -2.0 * R.TIED).all()
            assert (np.diff(ids[:m]) > 0).all()
    ids, acc = R.all_results("past_cut", 2048, 0, -1)
    assert (acc[:60] < -2.0 * R.TIED).all() and (acc[60:] == -2.0 * R.TIED).all()
    ch = R.chunk_size(1100)
    assert ch == 1104 and R.chunk_size(97) == 112 and R.chunk_size() == 14336
    for name, per_chunk in (("one_chunk_1025", [1025]), ("split_1025", [512, 513])):
        ids, acc = R.all_results(name, 2048, 0, -1)
        tied = ids[acc == -2.0 * R.TIED]
        assert np.bincount(tied // ch).tolist()[:len(per_chunk)] == per_chunk and tied.shape[0] == 1025
    for K in R.KS:  # dyadic: a handful of distinct scores, ties of hundreds
        for ids, acc in R.expected("dyadic", 2048, K):
            vals, counts = np.unique(acc, return_counts=True)
            assert vals.shape[0] <= 16 and counts.max() >= 200
    for name, cap in R.LCH_EDGE:  # the 16 best lie at the chunk limit and at the end
        n = R.family(name, cap).n
        ids, acc = R.all_results(name, cap, 0, -1)
        assert all(i >= n - 20 or 14330 <= i <= 14340 for i in ids[:16].tolist())
        assert acc[15] < acc[16]


def test_max_id_slots():
    for name, cap in R.FAMILIES + R.LCH_EDGE:
        m = R.max_ids(name, cap)
        assert m.shape == (8,) and m[0] == -1 and m[1] == 0
    for name in ("L5", "tied_at_cap", "tied_over_cap", "past_cut", "dyadic"):
        ids, acc = R.all_results(name, 2048, 0, -1)
        vals, counts = np.unique(acc, return_counts=True)
        group = ids[acc == vals[np.argmax(counts)]]
        cut = R.max_ids(name)[2]
        assert 0 < int((group < cut).sum()) < group.shape[0], name  # the group is cut in two


def _oracle_equal(f, qs, K, mids):
    D = O.OracleBowDb(f.n_words, f.vptr, f.words, f.weights)
    qptr, qw, qv = R.csr(qs)
    n, ids, sc = D.query(qptr, qw, qv, K, mids)
    for q, (w, v) in enumerate(qs):
        n0, ids0, sc0 = R.query_l1(f.n_words, f.vptr, f.words, f.weights, w, v, K, -1 if mids is None else int(mids[q]))
        assert n[q] == n0, (f.name, K, q)
        assert np.array_equal(ids[q, :n0], ids0), (f.name, K, q)
        assert np.array_equal(sc[q, :n0], sc0), (f.name, K, q)


@pytest.mark.parametrize("name,cap", R.FAMILIES + R.LCH_EDGE, ids=lambda v: str(v))
def test_query_l1_equals_the_oracle(name, cap):
    f = R.family(name, cap)
    for K in R.KS:
        _oracle_equal(f, R.batch(name, cap)[0], K, None)
        _oracle_equal(f, *((lambda b: (b[0], K, b[1]))(R.batch(name, cap, with_max_id=True))))
        if f.good:
            _oracle_equal(f, f.good, K, None)


def test_detection_database():
    """The detection case: entry 1400 as a query fails the LDS form at K = 256
    with recent_frames_window 50; the other queries of the test succeed."""
    f = R.detect_family()
    vec = lambda i: (f.words[2 * i:2 * i + 2], f.weights[2 * i:2 * i + 2])
    for i in list(range(100, 108)) + [350, 351] + list(range(352, 360)) + [1400]:
        ids, acc = R.results_l1(f.n_words, f.vptr, f.words, f.weights, *vec(i), max_id=max(i - 50, 0))
        assert ids.shape[0] > 0
        d = R.base_depth(ids, acc, 256, lds=True)
        assert (d is None) == (i == 1400), i


def test_rounding_bound():
    """query_l1 against score_exact, on the families and on real-valued vectors."""
    worst = 0.0
    rng = np.random.default_rng(5)
    cases = []
    for name in ("spread", "L3", "L5", "dyadic"):
        f = R.family(name)
        for w, v in f.queries[:2]:
            cases.append((f.n_words, f.vptr[:201], f.words, f.weights, w, v))
    for _ in range(4):  # 200 vectors of 5-40 of 64 words, L1-normalised in floating point
        vecs = []
        for _ in range(201):
            k = int(rng.integers(5, 41))
            x = rng.random(k) + 1e-3
            vecs.append((np.sort(rng.choice(64, k, replace=False)), x / x.sum()))
        ptr, w, v = R.csr(vecs[:200])
        cases.append((64, ptr, w, v, *vecs[200]))
    for n_words, vptr, words, weights, qw, qv in cases:
        ids, acc = R.results_l1(n_words, vptr, words, weights, qw, qv)
        for e, a in zip(ids.tolist(), acc.tolist()):
            s, c = R.score_exact(words[vptr[e]:vptr[e + 1]], weights[vptr[e]:vptr[e + 1]], qw, qv)
            assert c >= 1
            err = abs(a - (-2.0 * s))  # -2 * s is exact
            assert err <= 4 * c * 2.0 ** -52
            worst = max(worst, err / (c * 2.0 ** -52))
    print("largest |acc_ref - acc_exact| / (c * 2^-52):", worst)


@pytest.mark.parametrize("bad", [0.0, -0.0, -0.25, float("nan"), float("inf")])
def test_oracle_refuses_bad_weights(bad):
    f = R.family("spread")
    vptr, words, weights = f.db(0, 5)
    O.OracleBowDb(f.n_words, vptr, words, weights)
    w = weights.copy()
    w[-1] = bad
    with pytest.raises(ValueError, match="finite and > 0"):
        O.OracleBowDb(f.n_words, vptr, words, w)
    w[-1] = 5e-324  # a denormal is legal
    O.OracleBowDb(f.n_words, vptr, words, w)
