"""Streaming BoW database on MI355X (Database::add restated for the GPU): a
database grown by add / add_transformed answers every query bit for bit like
the CPU restatement (oracle/bow_oracle.c) built on the same prefix, and like
kmx_bow_set_database of the same entries.

Shared input: robot 0's 320 frames followed by its first 40 again (360
entries, 117,483 postings; the last 40 tie exactly with entries 0..39, so the
id decides); the queries are robot 1's first 64 frames. Expected values come
from OracleBowDb on the current prefix, never from the code under test."""
import functools

import numpy as np
import pytest

from kmx import abi
from kmx.lcd import LcdParams
from kmx.lcd.bow import BowDatabase, BowDetector
from kmx.synth.bow import make_bow_stream
from oracle import oracle as O

pytestmark = pytest.mark.gpu

BATCHES = [1, 1, 1, 7, 0, 3, 64, 1, 2, 33, 150, 1, 1, 40, 55]


@functools.lru_cache(maxsize=None)
def _input():
    st = make_bow_stream(2, 320, n_words=20000, seed=11)
    r0 = np.nonzero(st.robot == 0)[0]
    db = st.subset(np.concatenate([r0, r0[:40]]))
    qs = st.subset(np.nonzero(st.robot == 1)[0][:64])
    assert db.n == 360 and int(db.vptr[-1]) == 117483
    return st, db, qs


def _prefix(db, a, b):
    """Entries [a, b) of db as CSR."""
    return db.vptr[a:b + 1] - db.vptr[a], db.words[db.vptr[a]:db.vptr[b]], db.weights[db.vptr[a]:db.vptr[b]]


def _max_id(n, nq, seed):
    return np.random.default_rng(seed).integers(-1, n + 1, nq).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _expected(n, K, mid_seed):
    """The oracle's answer on the first n entries (mid_seed None: no max_id)."""
    _, db, qs = _input()
    D = O.OracleBowDb(db.n_words, *_prefix(db, 0, n))
    mid = None if mid_seed is None else _max_id(n, qs.n, mid_seed)
    return D.query(qs.vptr, qs.words, qs.weights, K, mid)


def _same(got, want, what):
    n, ids, sc = got
    n0, ids0, sc0 = want
    assert np.array_equal(n, n0), what
    for q in range(n.shape[0]):
        assert np.array_equal(ids[q, :n[q]], ids0[q, :n[q]]), (what, q)
        assert np.array_equal(sc[q, :n[q]], sc0[q, :n[q]]), (what, q)


def _check_queries(G, n, what):
    _, _, qs = _input()
    for K, seed in ((50, None), (256, None), (7, 1000 + n)):
        mid = None if seed is None else _max_id(n, qs.n, seed)
        _same(G.query(qs.vptr, qs.words, qs.weights, K, mid), _expected(n, K, seed), (what, n, K))


def _grown(tail=None):
    """A database over the shared input's words, empty."""
    _, db, _ = _input()
    G = BowDatabase(db.n_words)
    G.reset()
    if tail is not None:
        G.set_tail_cap(tail)
    return G


ENVS = [dict(t, **e) for t in ({}, {"KMX_BOW_TAIL": "1"}, {"KMX_BOW_TAIL": "5"}, {"KMX_BOW_TAIL": "1024"})
        for e in ({}, {"KMX_BOW_CHUNK": "97"}, {"KMX_BOW_LDS": "0"})]


@pytest.mark.parametrize("env", ENVS, ids=lambda e: ",".join(f"{k[8:]}={v}" for k, v in e.items()) or "default")
def test_adds_equal_a_rebuild_at_every_step(gpu, env, monkeypatch):
    for k in ("KMX_BOW_TAIL", "KMX_BOW_CHUNK", "KMX_BOW_LDS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _, db, _ = _input()
    G = _grown()
    n, mixed = 0, False
    for b in BATCHES:
        first = G.add(*_prefix(db, n, n + b))
        assert first == n
        n += b
        assert G.n == n
        info = G.info()
        assert info["n_entries"] == n and info["n_postings"] == int(db.vptr[n])
        assert 0 <= info["n_sealed"] <= n and n - info["n_sealed"] <= info["tail_cap"]
        mixed = mixed or 0 < info["n_sealed"] < n
        if env.get("KMX_BOW_TAIL") == "1024":
            assert info["n_sealed"] == 0
        _check_queries(G, n, "add")
    assert n == 360
    if env.get("KMX_BOW_TAIL") == "5":
        assert mixed, "no step had a sealed base and an unsealed tail"
    G.close()


@pytest.mark.parametrize("base,tail", [(8, 5), (100, 13), (224, 1), (320, 40), (0, 12), (113, 111)])
def test_explicit_splits(gpu, base, tail, monkeypatch):
    monkeypatch.delenv("KMX_BOW_TAIL", raising=False)
    _, db, qs = _input()
    G = _grown(tail=1024)
    if base:
        G.add(*_prefix(db, 0, base))
        G.seal()
    G.add(*_prefix(db, base, base + tail))
    info = G.info()
    assert (info["n_sealed"], info["n_entries"]) == (base, base + tail)
    want = _expected(base + tail, 50, None)
    got = G.query(qs.vptr, qs.words, qs.weights, 50)
    _same(got, want, "split")
    if (base, tail) == (320, 40):  # every duplicate ties with its original, which comes first
        n, ids, sc = got
        for q in range(qs.n):
            for k in np.nonzero(ids[q, :n[q]] >= 320)[0]:
                assert k > 0 and ids[q, k - 1] == ids[q, k] - 320 and sc[q, k - 1] == sc[q, k]
    G.seal()
    assert G.info()["n_sealed"] == base + tail
    again = G.query(qs.vptr, qs.words, qs.weights, 50)
    _same(again, want, "sealed")
    _same(got, again, "equal")
    G.close()


def test_same_answers_as_set_entries(gpu, monkeypatch):
    monkeypatch.setenv("KMX_BOW_TAIL", "5")
    _, db, qs = _input()
    G = _grown()
    n = 0
    for b in BATCHES[:-1] + [52, 3]:  # the last 3 stay unsealed
        G.add(*_prefix(db, n, n + b))
        n += b
    assert n == 360 and G.info()["n_sealed"] == 357
    S = BowDatabase(db.n_words)
    S.set_entries(db.vptr, db.words, db.weights)
    for K in (50, 256):
        got, want = G.query(qs.vptr, qs.words, qs.weights, K), S.query(qs.vptr, qs.words, qs.weights, K)
        _same(got, want, "equal")
        _same(got, _expected(360, K, None), "grown")
        G.query_async(qs.vptr, qs.words, qs.weights, K)
        G.sync()
        _same(G.fetch(qs.n, K), want, "equal")
    # set_entries on the grown handle replaces everything, all sealed
    G.set_entries(db.vptr, db.words, db.weights)
    info = G.info()
    assert G.n == 360 and (info["n_entries"], info["n_sealed"]) == (360, 360)
    w, v = db.vector(3)
    assert G.add(np.array([0, w.shape[0]], np.int64), w, v) == 360
    G.close()
    S.close()


def test_resident_forms(gpu, monkeypatch):
    monkeypatch.setenv("KMX_BOW_TAIL", "5")
    _, db, qs = _input()
    G = _grown()
    G.add(*_prefix(db, 0, 200))
    G.add(*_prefix(db, 200, 203))  # 3 entries unsealed
    assert G.info()["n_sealed"] == 200
    # entries() returns what was added
    for a, b in ((0, 203), (37, 1), (199, 4), (203, 0)):
        for g, w in zip(G.entries(a, b), _prefix(db, a, a + b)):
            assert g.dtype == w.dtype and np.array_equal(g, w)
    # queries by entry id of the database itself: sealed and unsealed ids, repeated, unordered
    ids = np.array([202, 0, 5, 5, 201, 199, 77], np.int32)
    sub = db.subset(ids)
    mid = np.array([-1, 203, 5, 0, 201, 100, -1], np.int32)
    for K, m in ((50, None), (9, mid)):
        got, want = G.query_entries(ids, K, m), G.query(sub.vptr, sub.words, sub.weights, K, m)
        _same(got, want, "equal")
        D = O.OracleBowDb(db.n_words, *_prefix(db, 0, 203))
        _same(got, D.query(sub.vptr, sub.words, sub.weights, K, m), "query_entries")
    # queries taken from another handle (robot 1's frames), also enqueue-only
    R = _grown()
    R.add(qs.vptr, qs.words, qs.weights)
    qid = np.arange(qs.n, dtype=np.int32)[::-1].copy()
    rsub = qs.subset(qid)
    want = G.query(rsub.vptr, rsub.words, rsub.weights, 50)
    _same(G.query_entries(qid, 50, src=R), want, "equal")
    G.query_entries_async(qid, 50, src=R)
    G.sync()
    _same(G.fetch(qid.shape[0], 50), want, "equal")
    # score_entries == score_pairs, with an id of -1 and an empty vector (entry 203)
    G.add(np.array([0, 0], np.int64), np.zeros(0, np.uint32), np.zeros(0))
    assert G.n == 204 and np.array_equal(G.entries(203, 1)[0], [0, 0])
    a_ids = np.array([1, 2, 202, 203, 50, -1, 7, 203], np.int32)
    b_ids = np.array([0, 1, 201, 5, -1, 3, 7, 203], np.int32)

    def vec(ids):  # -1 and the empty entry: an empty vector
        keep = [i for i in ids if 0 <= i < 203]
        s = db.subset(np.array(keep, np.int64))
        lens = np.array([db.vptr[i + 1] - db.vptr[i] if 0 <= i < 203 else 0 for i in ids], np.int64)
        return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), s.words, s.weights

    got = G.score_entries(a_ids, b_ids)
    assert np.array_equal(got, G.score_pairs(vec(a_ids), vec(b_ids)))
    assert abs(got[6] - 1.0) < 1e-12 and np.all(got[[3, 4, 5, 7]] == 0.0) and np.all(got[:3] > 0.0)
    # set_entries fills the resident vectors too
    S = BowDatabase(db.n_words)
    S.set_entries(db.vptr, db.words, db.weights)
    for g, w in zip(S.entries(350, 10), _prefix(db, 350, 360)):
        assert np.array_equal(g, w)
    _same(S.query_entries(np.array([3], np.int32), 50), S.query(*_prefix(db, 3, 4), 50), "set_entries, by id")
    for h in (G, R, S):
        h.close()


def test_transform_to_database_without_host_hop(gpu, monkeypatch):
    monkeypatch.setenv("KMX_BOW_TAIL", "5")
    from kmx.lcd.vocabulary import GpuVocabulary
    from kmx.synth.vocab import make_descriptors, make_vocabulary
    voc = make_vocabulary(10, 3, seed=1, flip_bits=24)
    nf = np.array([64, 0, 33, 64, 1, 17], np.int32)  # a frame without features, full frames
    desc = make_descriptors(voc, nf.shape[0], 64, noise_bits=20, seed=3)
    for f, n in enumerate(nf):
        desc[f, n:] = 0xFF
    gv = GpuVocabulary(voc)
    vptr, words, weights = gv.transform(nf, desc)
    assert vptr[2] == vptr[1]  # the zero-word frame
    G = BowDatabase(voc.n_words)
    G.reset()
    H = BowDatabase(voc.n_words)
    H.reset()
    for rep in range(2):  # the second batch crosses tail_cap: a seal of device-added entries
        gv.transform_async(nf, desc)
        assert G.add_transformed(gv) == (6 * rep, 6)
        assert H.add(vptr, words, weights) == 6 * rep
    gi, hi = G.info(), H.info()
    assert G.n == 12 and gi["n_sealed"] == 12
    assert all(gi[k] == hi[k] for k in ("n_words", "n_entries", "n_sealed", "tail_cap", "n_postings"))
    for first in (0, 6):
        for g, w in zip(G.entries(first, 6), (vptr, words, weights)):
            assert g.dtype == w.dtype and np.array_equal(g, w)
    gv.transform_async(nf[:3], desc[:3])
    assert G.add_transformed(gv) == (12, 3)  # unsealed, the zero-word frame is entry 13
    H.add(vptr[:4], words[:vptr[3]], weights[:vptr[3]])
    assert G.info()["n_sealed"] == 12 and np.array_equal(G.entries(13, 1)[0], [0, 0])
    qd = make_descriptors(voc, 5, 64, noise_bits=20, seed=4)
    q = gv.transform(np.full(5, 64, np.int32), qd)
    D = O.OracleBowDb(voc.n_words, *H.entries(0, 15))
    for K in (10, 256):
        got = G.query(*q, K)
        _same(got, H.query(*q, K), "equal")
        _same(got, D.query(*q, K), "voc")
        assert got[0].max() > 0
        assert all(13 not in got[1][i, :got[0][i]] for i in range(5))  # the empty entry is never a result
    # a vocabulary over another word count is refused, the database unchanged
    voc2 = make_vocabulary(4, 3, seed=2, flip_bits=24)
    gv2 = GpuVocabulary(voc2)
    gv2.transform_async(np.array([8], np.int32), make_descriptors(voc2, 1, 8, noise_bits=4, seed=5))
    before = G.info()
    with pytest.raises(abi.KmxError):
        G.add_transformed(gv2)
    assert G.info() == before and G.n == 15
    for h in (G, H, gv, gv2):
        h.close()


def test_detect_loop_resident(gpu, monkeypatch):
    monkeypatch.setenv("KMX_BOW_TAIL", "5")
    st, _, _ = _input()
    r0 = np.nonzero(st.robot == 0)[0]
    allf = st.subset(np.concatenate([r0, r0[:120]]))
    p = LcdParams()
    det = BowDetector(p, n_words=st.n_words)
    for i in range(allf.n):
        ids = det.add_vectors(0, *_prefix(allf, i, i + 1))
        assert ids.tolist() == [i]
    assert 0 < det.db[0].info()["n_sealed"] <= 440
    got = det.detectLoopResident(0, 0, 440)
    ref_det = BowDetector(p, n_words=st.n_words)
    ref_det.set_robot_database(0, allf.vptr, allf.words, allf.weights)
    assert got == ref_det.detectLoop(0, (allf.vptr, allf.words, allf.weights), 0)
    D = O.OracleBowDb(st.n_words, allf.vptr, allf.words, allf.weights)
    assert got == O.detect_loop_stream(D, allf.vptr, allf.words, allf.weights, 0, p)
    assert sum(1 for g in got if g[1] == "LOOP_DETECTED") >= 50
    # a later window of the same stream
    assert det.detectLoopResident(0, 300, 140) == ref_det.detectLoop(0, _prefix(allf, 300, 440), 300)


def test_detect_loop_with_robot_resident(gpu, monkeypatch):
    monkeypatch.setenv("KMX_BOW_TAIL", "5")
    st, _, _ = _input()
    db = st.subset(np.nonzero(st.robot == 0)[0])
    r1 = st.subset(np.nonzero(st.robot == 1)[0])
    det = BowDetector(LcdParams(), n_words=st.n_words)
    for a in range(0, 320, 10):  # other robots' vectors arrive in batches of bow_batch_size = 10
        det.add_vectors(0, *_prefix(db, a, a + 10))
        det.add_vectors(1, *_prefix(r1, a, a + 10))
    qids = np.arange(320, dtype=np.int32)
    m, s, nss = det.detectLoopWithRobotResident(0, 1, qids)
    # the host form: prev = the frame before each query, an empty vector for frame 0
    pv = _prefix(r1, 0, 319)
    prev = (np.concatenate([[0], pv[0]]).astype(np.int64), pv[1], pv[2])
    query = (r1.vptr, r1.words, r1.weights)
    m1, s1, nss1 = det.detectLoopWithRobot(0, query, prev)
    assert np.array_equal(m, m1) and np.array_equal(s, s1) and np.array_equal(nss, nss1)
    D = O.OracleBowDb(st.n_words, db.vptr, db.words, db.weights)
    m0, s0, nss0 = D.detect_batch(*query, *prev)
    assert np.array_equal(nss, nss0) and np.array_equal(m, m0) and np.array_equal(s, s0)
    assert m[0] == -1 and nss[0] == 0.0 and (m >= 0).sum() > 320 // 4


def test_refusals(gpu, monkeypatch):
    monkeypatch.setenv("KMX_BOW_TAIL", "5")
    _, db, qs = _input()
    G = BowDatabase(db.n_words)
    with pytest.raises(abi.KmxError):  # no database yet
        G.add(*_prefix(db, 0, 1))
    assert G.L.kmx_bow_add_entries(G.h, 0, None, None, None, None) == abi.KMX_ESTATE
    assert G.n == 0
    G.reset()
    G.add(*_prefix(db, 0, 23))
    before = G.info()
    want = G.query(qs.vptr, qs.words, qs.weights, 50)
    vptr, words, weights = (x.copy() for x in _prefix(db, 23, 26))
    bad = []
    w = words.copy()
    w[vptr[1] + 4] = w[vptr[1] + 3]  # a repeated word
    bad.append((vptr, w, weights))
    w = words.copy()
    w[vptr[2] - 1] = db.n_words  # a word >= n_words
    bad.append((vptr, w, weights))
    v = vptr.copy()
    v[2] = v[1] - 1  # a decreasing vptr
    bad.append((v, words, weights))
    for args in bad:
        a, b, c = (np.ascontiguousarray(x) for x in args)
        rc = G.L.kmx_bow_add_entries(G.h, 3, abi.i64ptr(a), abi.u32ptr(b), abi.fptr(c), None)
        assert rc == abi.KMX_EINVAL
        with pytest.raises(abi.KmxError):
            G.add(*args)
        assert G.info() == before and G.n == 23
        _same(G.query(qs.vptr, qs.words, qs.weights, 50), want, "equal")
    assert G.add(vptr, words, weights) == 23  # the same batch, intact, is taken
    _same(G.query(qs.vptr, qs.words, qs.weights, 50), _expected(26, 50, None), "after refusals")
    G.close()
