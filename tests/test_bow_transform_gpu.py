"""kmx_voc_* (voc.hip): DBoW2's vocabulary transform on the GPU against the CPU
restatement tests/bow_transform_ref.py, bit for bit — vptr, words and weights
compared with np.array_equal, no tolerance. Descriptor slots beyond a frame's
n_feats hold 0xFF and must not influence anything. The shapes are the smallest
at which each failure mode exists."""
import functools

import numpy as np
import pytest

from tests import bow_transform_ref as ref

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _voc(k, L, seed=1, irregular=0.0, zero_weight=0.0, weighting=0):
    from kmx.synth.vocab import make_vocabulary
    return make_vocabulary(k, L, seed=seed, flip_bits=24, irregular=irregular, zero_weight=zero_weight,
                           weighting=weighting)


def _frames(voc, n_feats, max_feats, seed, noise_bits=20):
    """Padded frames: features near random words, 0xFF beyond n_feats."""
    from kmx.synth.vocab import make_descriptors
    nf = np.asarray(n_feats, np.int32)
    desc = make_descriptors(voc, nf.shape[0], max_feats, noise_bits=noise_bits, seed=seed)
    for f, n in enumerate(nf):
        desc[f, n:] = 0xFF
    return nf, desc


def _check(voc, nf, desc):
    from kmx.lcd.vocabulary import GpuVocabulary
    gv = GpuVocabulary(voc)
    try:
        got = gv.transform(nf, desc)
    finally:
        gv.close()
    want = ref.transform(voc, nf, desc)
    for name, g, w in zip(("vptr", "words", "weights"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    return got


def test_known_answer(gpu):
    """The hand-built tree of tests/test_vocabulary_cpu.py: a word hit twice, an
    exact tie between siblings at both levels, a zero-weight word."""
    voc, nf, feats = ref.hand_tree(weighting=0)
    vptr, words, weights = _check(voc, nf, feats)
    assert (vptr.tolist(), words.tolist(), weights.tolist()) == ([0, 2], [1, 2], [0.4, 0.6])
    voc, nf, feats = ref.hand_tree(weighting=2)
    vptr, words, weights = _check(voc, nf, feats)
    assert weights.tolist() == [0.5714285714285714, 0.42857142857142855]


def test_regular_tree_empty_frame_and_padding(gpu):
    voc = _voc(10, 3)
    assert voc.n_nodes == 1111
    nf, desc = _frames(voc, [0, 1, 2, 63, 64, 64, 17, 5], 64, seed=2)
    vptr, _, _ = _check(voc, nf, desc)
    assert vptr[1] == 0  # the empty frame
    # the padding does not matter: other bytes there, same vectors
    desc2 = desc.copy()
    for f, n in enumerate(nf):
        desc2[f, n:] = 0x00
    again = _check(voc, nf, desc2)
    assert np.array_equal(again[1], ref.transform(voc, nf, desc)[1])


def test_tree_larger_than_the_lds_stage(gpu):
    """k = 10, L = 4: 11,111 nodes (355 KB); the top of the tree is read from
    LDS, the deeper child blocks from global memory."""
    from kmx.lcd.vocabulary import GpuVocabulary
    voc = _voc(10, 4)
    gv = GpuVocabulary(voc)
    info = gv.info()
    gv.close()
    assert info["n_nodes"] == 11111 and info["max_children"] == 10 and info["max_depth"] == 4
    assert 0 < info["lds_nodes"] < info["n_nodes"]
    nf, desc = _frames(voc, [128, 128, 100, 128], 128, seed=3)
    _check(voc, nf, desc)


def test_deep_tree(gpu):
    voc = _voc(4, 6)
    nf, desc = _frames(voc, [128, 128, 128, 77], 128, seed=4)
    _check(voc, nf, desc)


@pytest.mark.parametrize("k", [7, 17])
def test_odd_child_counts(gpu, k):
    voc = _voc(k, 3)
    nf, desc = _frames(voc, [64, 64, 64, 33], 64, seed=5)
    _check(voc, nf, desc)


def test_irregular_tree(gpu):
    """1..k children per node, leaves at depths 1..L."""
    voc = _voc(10, 4, seed=6, irregular=0.4)
    cnt = np.bincount(voc.parent[1:], minlength=voc.n_nodes)
    assert cnt[cnt > 0].min() == 1 and cnt.max() == 10
    nf, desc = _frames(voc, [128, 128, 128, 128], 128, seed=6, noise_bits=40)
    _check(voc, nf, desc)


def test_ties_first_child_wins(gpu):
    """Two identical siblings at every level of one path, the features equal to
    that path's descriptors: distance 0 to both, the first is taken."""
    import copy
    voc = copy.deepcopy(_voc(10, 3))
    kids = ref.children_of(voc)
    path, node = [], 0
    for pick in (2, 4, 0):
        a, twin = kids[node][pick], kids[node][pick + 1]
        voc.descriptor[twin] = voc.descriptor[a]
        path.append(a)
        node = a
    desc = np.zeros((1, 32, 32), np.uint8)
    for i in range(32):
        desc[0, i] = voc.descriptor[path[i % 3]]
    leaves = ref.descend_numpy(voc, desc[0])
    assert leaves[2] == path[2] and all(ref.descend(voc, kids, desc[0, i]) == leaves[i] for i in range(3))
    _check(voc, np.array([32], np.int32), desc)


def test_duplicates_are_added_one_at_a_time(gpu):
    """1024 identical features: the weight is 1023 sequential additions, which
    differs from 1024 * w in the last bits; 513 features from 3 descriptors:
    the sort at an odd size."""
    voc = _voc(10, 3)
    one = voc.descriptor[voc.word_node[123]]
    w = float(voc.weight[voc.word_node[123]])
    acc = w
    for _ in range(1023):
        acc += w
    assert acc != 1024 * w  # the case can tell the two apart
    desc = np.broadcast_to(one, (1, 1024, 32)).copy()
    vptr, words, weights = _check(voc, np.array([1024], np.int32), desc)
    assert words.tolist() == [123] and weights.tolist() == [1.0]
    three = voc.descriptor[voc.word_node[[5, 700, 31]]]
    desc = np.full((1, 1024, 32), 0xFF, np.uint8)
    desc[0, :513] = three[np.arange(513) % 3]
    _, words, _ = _check(voc, np.array([513], np.int32), desc)
    assert words.tolist() == [5, 31, 700]


@pytest.mark.parametrize("zero_weight", [1.0, 0.3])
def test_zero_weight_words(gpu, zero_weight):
    voc = _voc(10, 3, seed=8, zero_weight=zero_weight)
    nf, desc = _frames(voc, [64, 40], 64, seed=8)
    vptr, _, weights = _check(voc, nf, desc)
    if zero_weight == 1.0:
        assert vptr.tolist() == [0, 0, 0]
    else:
        assert np.all(weights > 0) and vptr[-1] > 0


@pytest.mark.parametrize("weighting", [0, 1, 2, 3])
def test_weightings(gpu, weighting):
    """TF_IDF / TF add per occurrence, IDF / BINARY store once: few words, many hits."""
    voc = _voc(3, 3, seed=9, weighting=weighting)
    nf, desc = _frames(voc, [64, 50], 64, seed=9, noise_bits=5)
    vptr, _, _ = _check(voc, nf, desc)
    assert vptr[1] < 64  # words repeat


def test_pool_transform_equals_host_transform(gpu):
    """Descriptors appended to a LoopClosureDetector in two add_frames calls
    that cross a capacity doubling; transform_pool on shuffled ids with
    repeats equals transform on the same host descriptors."""
    from kmx import abi
    from kmx.lcd import LoopClosureDetector
    from kmx.lcd.vocabulary import GpuVocabulary
    voc = _voc(10, 3)
    rng = np.random.Generator(np.random.PCG64(10))
    F, N = 70, 64
    nf, desc = _frames(voc, rng.integers(0, N + 1, F), N, seed=10)
    zeros = np.zeros((F, N, 3))
    det = LoopClosureDetector()
    gv = GpuVocabulary(voc)
    try:
        assert det.add_frames(nf[:60], desc[:60], zeros[:60], zeros[:60]) == 0
        cap0 = det.pool_info()["capacity"]
        assert det.add_frames(nf[60:], desc[60:], zeros[60:], zeros[60:]) == 60
        assert det.pool_info()["capacity"] > cap0 >= 60
        ids = rng.integers(0, F, 100).astype(np.int32)
        ids[:3] = [69, 0, 69]
        got = det.bow_vectors(gv, ids)
        want = gv.transform(nf[ids], desc[ids])
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        for g, w in zip(got, ref.transform(voc, nf[ids], desc[ids])):
            assert np.array_equal(g, w)
        for bad in ([0, F], [-1]):
            with pytest.raises(abi.KmxError, match=r"\(-1\).*outside the pool"):
                gv.transform_pool(det, np.array(bad, np.int32))
    finally:
        gv.close()
        det.close()


E2E_SEED = 21  # chosen so that the REFERENCE vectors give the copied frame as top-1 for all 16 queries


def e2e_case():
    """64 database frames x 200 features; 16 queries, each a copy of a database
    frame with 3 bits flipped in a tenth of its descriptors."""
    from kmx.synth.vocab import _flip
    voc = _voc(10, 4)
    nf, desc = _frames(voc, [200] * 64, 200, seed=E2E_SEED)
    rng = np.random.Generator(np.random.PCG64(E2E_SEED + 1))
    src = rng.permutation(64)[:16]
    q = desc[src].copy()
    for i in range(16):
        hit = rng.permutation(200)[:20]
        d = q[i, hit]
        _flip(d, 3, rng)
        q[i, hit] = d
    return voc, nf, desc, src, q


def l1_top1(n_words, db, qv):
    """argmax over database entries of the L1 score 1 - |q - d|_1 / 2 (dense, CPU)."""
    def dense(v):
        vptr, words, weights = v
        m = np.zeros((vptr.shape[0] - 1, n_words))
        rows = np.repeat(np.arange(vptr.shape[0] - 1), np.diff(vptr))
        m[rows, words] = weights
        return m
    D, Q = dense(db), dense(qv)
    return np.array([int(np.argmin(np.abs(D - Q[i]).sum(axis=1))) for i in range(Q.shape[0])])


def test_end_to_end_vectors_through_the_bow_database(gpu):
    from kmx.lcd import BowDetector
    from kmx.lcd.bow import BowDatabase
    voc, nf, desc, src, q = e2e_case()
    ref_db = ref.transform(voc, nf, desc)
    ref_q = ref.transform(voc, nf[:16], q)
    assert np.array_equal(l1_top1(voc.n_words, ref_db, ref_q), src)  # the condition on the seed
    det = BowDetector(vocabulary=voc)
    assert det.n_words == voc.n_words == 10000
    db_v = det.transform(nf, desc)
    q_v = det.transform(nf[:16], q)
    for g, w in zip(db_v + q_v, ref_db + ref_q):
        assert np.array_equal(g, w)
    db = BowDatabase(det.n_words)
    try:
        db.set_entries(*db_v)
        n, ids, sc = db.query(*q_v, max_results=4)
    finally:
        db.close()
    assert np.all(n >= 1) and np.array_equal(ids[:, 0], src)
