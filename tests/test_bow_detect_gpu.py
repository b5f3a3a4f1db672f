"""detectLoop decided on the device (kmx_bow_detect_entries, kmx_bow_decide_results;
k_bow_decide and k_bow_temporal in bow.hip): the nss gate, the alpha cut,
computeIslands and checkTemporalConstraint give, record for record, what the
CPU restatement gives (oracle/oracle.py detect_loop_stream, orc_bow_islands,
orc_bow_temporal, OracleBowDb.detect_batch), in one call or in any split of the
stream into calls, one keyframe per call included.

Shared input, as test_bow_stream_gpu.py::test_detect_loop_resident builds it:
robot 0's 320 frames followed by its first 120 again (440 entries). Expected
values come from the oracle, never from the code under test: _oracle_decide
restates detect_loop_stream's control around the oracle's own islands and
temporal functions so that the whole record and the state after every keyframe
are known, and is itself checked against detect_loop_stream."""
import ctypes as C
import functools

import numpy as np
import pytest

from kmx import abi
from kmx.lcd import LcdParams
from kmx.lcd.bow import BowDatabase, BowDetector
from kmx.synth.bow import make_bow_stream
from oracle import oracle as O

pytestmark = pytest.mark.gpu

BATCHES = [1, 1, 1, 7, 0, 3, 64, 1, 2, 33, 150, 1, 1, 40, 55, 17, 0, 63]  # test_bow_stream_gpu's, then the rest of 440
N = 440

# (parameters, the oracle's status counts on the shared stream)
PARAM_SETS = {
    "default": ({}, dict(NO_MATCHES=101, LOW_NSS_FACTOR=84, LOOP_DETECTED=89, FAILED_TEMPORAL_CONSTRAINT=1,
                         LOW_SCORE=165)),
    "no_groups": (dict(max_intraisland_gap=1, min_matches_per_island=2),
                  dict(NO_MATCHES=101, LOW_NSS_FACTOR=84, NO_GROUPS=90)),
    "no_nss": (dict(use_nss=0), dict(NO_MATCHES=101, LOW_NSS_FACTOR=0, LOOP_DETECTED=119)),
    "k256_alpha05": (dict(max_db_results=256, alpha=0.05),
                     dict(NO_MATCHES=101, LOW_NSS_FACTOR=84, FAILED_TEMPORAL_CONSTRAINT=51, LOOP_DETECTED=106)),
    "no_nss_alpha02": (dict(use_nss=0, alpha=0.02), dict(NO_MATCHES=101, LOW_NSS_FACTOR=0)),
    "full_width": (dict(use_nss=0, alpha=0.0, max_db_results=256), dict(NO_MATCHES=101, LOW_NSS_FACTOR=0)),
    # fewer keyframes without a match, so more of them reach the nss test: 107, not the other sets' 84
    "window10": (dict(recent_frames_window=10), dict(NO_MATCHES=11, LOW_NSS_FACTOR=107)),
    "min_temporal0": (dict(min_temporal_matches=0),
                      dict(NO_MATCHES=101, LOW_NSS_FACTOR=84, LOOP_DETECTED=90, FAILED_TEMPORAL_CONSTRAINT=0)),
    "min_temporal3": (dict(min_temporal_matches=3),
                      dict(NO_MATCHES=101, LOW_NSS_FACTOR=84, LOOP_DETECTED=87, FAILED_TEMPORAL_CONSTRAINT=3)),
    "between_queries0": (dict(max_nrFrames_between_queries=0),
                         dict(NO_MATCHES=101, LOW_NSS_FACTOR=84, LOOP_DETECTED=0, FAILED_TEMPORAL_CONSTRAINT=90)),
    "between_islands0": (dict(max_nrFrames_between_islands=0, max_intraisland_gap=2),
                         dict(NO_MATCHES=101, LOW_NSS_FACTOR=84, FAILED_TEMPORAL_CONSTRAINT=30, LOOP_DETECTED=60)),
}


@functools.lru_cache(maxsize=None)
def _input():
    st = make_bow_stream(2, 320, n_words=20000, seed=11)
    r0 = np.nonzero(st.robot == 0)[0]
    allf = st.subset(np.concatenate([r0, r0[:120]]))
    assert allf.n == N
    return st, allf


def _prefix(db, a, b):
    """Entries [a, b) of db as CSR."""
    return db.vptr[a:b + 1] - db.vptr[a], db.words[db.vptr[a]:db.vptr[b]], db.weights[db.vptr[a]:db.vptr[b]]


@functools.lru_cache(maxsize=None)
def _oracle_db():
    st, allf = _input()
    return O.OracleBowDb(st.n_words, allf.vptr, allf.words, allf.weights)


@functools.lru_cache(maxsize=None)
def _oracle_query(K, window):
    """The oracle's query results for every keyframe of the stream, and the
    nss factor of each against the keyframe before it (0.0 for keyframe 0)."""
    _, allf = _input()
    fids = np.arange(N)
    n, ids, sc = _oracle_db().query(allf.vptr, allf.words, allf.weights, K, np.maximum(fids - window, 0))
    nss = np.zeros(N)
    for q in range(1, N):
        a, b = slice(allf.vptr[q], allf.vptr[q + 1]), slice(allf.vptr[q - 1], allf.vptr[q])
        nss[q] = O.bow_score(allf.words[a], allf.weights[a], allf.words[b], allf.weights[b])
    for a in (n, ids, sc, nss):
        a.setflags(write=False)
    return n, ids, sc, nss


def _oracle_decide(qids, n, ids, sc, nss, has_prev, p, state=None):
    """detect_loop_stream's control (oracle/oracle.py) on given query results,
    around the oracle's orc_bow_islands / orc_bow_temporal. Returns the records
    (abi.BOW_RECORD_DTYPE), the state after every query [nq, 4], and per query
    (number of kept islands, most members in one, whether the best island holds
    the top result)."""
    L = O.lib()
    nq = len(qids)
    rec = np.zeros(nq, abi.BOW_RECORD_DTYPE)
    states = np.zeros((nq, 4), np.int32)
    shape = np.zeros((nq, 3), np.int32)
    state = np.zeros(4, np.int32) if state is None else np.array(state, np.int32)
    isl = (O._Island * max(ids.shape[1], 1))()
    for q in range(nq):
        hp = bool(has_prev[q])
        f = float(nss[q]) if p.use_nss else 1.0
        r = dict(query_id=int(qids[q]), status=None, match_id=-1, n_kept=0, island_start=-1, island_end=-1,
                 score=0.0, nss=f if hp else 0.0, island_score=0.0)
        k = 0
        if n[q] == 0:
            r["status"] = "NO_MATCHES"
        elif p.use_nss and (not hp or f < p.min_nss_factor):
            r["status"] = "LOW_NSS_FACTOR"
        else:
            while k < n[q] and sc[q, k] >= p.alpha * f:
                k += 1
            r["n_kept"] = k
            if k == 0:
                r["status"] = "LOW_SCORE"
        if r["status"] is None:
            qi, qs = np.ascontiguousarray(ids[q, :k], np.int32), np.ascontiguousarray(sc[q, :k], np.float64)
            ni = L.orc_bow_islands(k, O._i(qi), O._f(qs), p.max_intraisland_gap, p.min_matches_per_island,
                                   C.byref(isl))
            if ni == 0:
                r["status"] = "NO_GROUPS"
            else:
                best = max(range(ni), key=lambda j: isl[j].score)  # first maximum, like std::max_element
                b = isl[best]
                ok = L.orc_bow_temporal(O._i(state), int(qids[q]), b.start, b.end, p.max_nrFrames_between_queries,
                                        p.max_nrFrames_between_islands, p.min_temporal_matches)
                r.update(status="LOOP_DETECTED" if ok else "FAILED_TEMPORAL_CONSTRAINT", match_id=b.best_id,
                         island_start=b.start, island_end=b.end, score=b.best_score, island_score=b.score)
                members = max(int(((qi >= isl[j].start) & (qi <= isl[j].end)).sum()) for j in range(ni))
                shape[q] = (ni, members, b.start <= qi[0] <= b.end)
        r["status"] = abi.BOW_STATUS.index(r["status"])
        rec[q] = tuple(r[name] for name in abi.BOW_RECORD_DTYPE.names)
        states[q] = state
    return rec, states, shape


def _tuples(rec):
    return [(int(r["query_id"]), abi.BOW_STATUS[r["status"]], int(r["match_id"]), float(r["score"])) for r in rec]


def _cands(rec):
    loop = rec["status"] == abi.BOW_STATUS.index("LOOP_DETECTED")
    return np.stack([rec["query_id"][loop], rec["match_id"][loop]], axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _expected(name):
    """The oracle's records, states and island shapes for a parameter set."""
    p = LcdParams(**PARAM_SETS[name][0])
    n, ids, sc, nss = _oracle_query(p.max_db_results, p.recent_frames_window)
    rec, states, shape = _oracle_decide(np.arange(N), n, ids, sc, nss, np.arange(N) > 0, p)
    rec.setflags(write=False)
    states.setflags(write=False)
    return p, rec, states, shape


def _same_records(got, want, what):
    """Equality on every field; doubles compare with ==."""
    for name in abi.BOW_RECORD_DTYPE.names:
        bad = np.nonzero(got[name] != want[name])[0]
        assert bad.size == 0, (what, name, bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


def _detector(p, monkeypatch, tail="5", upto=N):
    """A detector whose robot 0 holds the first `upto` keyframes, added one at a time."""
    monkeypatch.setenv("KMX_BOW_TAIL", tail)
    st, allf = _input()
    det = BowDetector(p, n_words=st.n_words)
    det._robot_db(0)
    if upto:
        det.add_vectors(0, *_prefix(allf, 0, upto))
    return det


@pytest.mark.parametrize("name", list(PARAM_SETS))
def test_whole_stream_in_one_call(gpu, name, monkeypatch):
    p, want, states, shape = _expected(name)
    _, allf = _input()
    # the oracle's own counts on this stream, so a change of input cannot hollow the test out
    ref = O.detect_loop_stream(_oracle_db(), allf.vptr, allf.words, allf.weights, 0, p)
    assert _tuples(want) == ref
    counts = {s: sum(1 for r in ref if r[1] == s) for s in abi.BOW_STATUS}
    for s, c in PARAM_SETS[name][1].items():
        assert counts[s] == c, (name, s, counts)
    if name == "default":
        reached = shape[:, 0] > 0
        assert reached.sum() == 90 and (shape[reached, 1] == 4).all()
    if name == "k256_alpha05":
        assert shape[:, 0].max() == 6 and (shape[:, 0] > 1).sum() == 76
    if name == "no_nss_alpha02":
        reached = shape[:, 0] > 0
        assert reached.sum() == 317 and want["n_kept"].max() == 50
        assert shape[:, 0].max() == 25 and shape[:, 1].max() == 18 and (reached & (shape[:, 2] == 0)).sum() == 81
    if name == "full_width":
        assert (want["n_kept"] == 256).sum() >= 1
    det = _detector(p, monkeypatch)
    got, cand = det.db[0].detect_entries(np.arange(N, dtype=np.int32), det.detect_params())
    _same_records(got, want, name)
    assert np.array_equal(cand, _cands(want))
    assert np.array_equal(det.db[0].temporal_state, states[-1])
    out, cand2 = det.detectLoopStream(0, 0, N, reset=True, candidates=True)
    assert out == ref and np.array_equal(cand2, cand)
    assert out == det.detectLoopResident(0, 0, N)
    assert np.array_equal(det.detectLoopStreamCandidates(0, 0, N, reset=True), cand)


def test_between_the_sets_every_status_occurs():
    seen = set()
    for name in PARAM_SETS:
        seen |= set(np.unique(_expected(name)[1]["status"]).tolist())
    assert seen == set(range(len(abi.BOW_STATUS)))


def test_one_keyframe_per_call_equals_the_batch(gpu, monkeypatch):
    """Kimera's form: Database::add of one keyframe, then detectLoop of it. Also
    the state after every keyframe against the oracle's."""
    p, want, states, _ = _expected("default")
    _, allf = _input()
    det = _detector(p, monkeypatch, upto=0)
    out, cands = [], []
    for i in range(N):
        assert det.add_vectors(0, *_prefix(allf, i, i + 1)).tolist() == [i]
        o, c = det.detectLoopStream(0, i, 1, candidates=True)
        assert np.array_equal(det.db[0].temporal_state, states[i]), i
        out += o
        cands.append(c)
    assert out == _tuples(want)
    assert sum(1 for o in out if o[1] == "LOOP_DETECTED") == 89
    assert np.array_equal(np.concatenate(cands), _cands(want))


@pytest.mark.parametrize("tail", ["1", "5", "1024"])
@pytest.mark.parametrize("name", ["default", "k256_alpha05"])
def test_ragged_batches_equal_the_batch(gpu, name, tail, monkeypatch):
    p, want, states, _ = _expected(name)
    _, allf = _input()
    assert sum(BATCHES) == N
    det = _detector(p, monkeypatch, tail=tail, upto=0)
    recs, cands, a = [], [], 0
    for b in BATCHES:
        det.add_vectors(0, *_prefix(allf, a, a + b))
        r, c = det.db[0].detect_entries(np.arange(a, a + b, dtype=np.int32), det.detect_params())
        recs.append(r)
        cands.append(c)
        a += b
        if b:
            assert np.array_equal(det.db[0].temporal_state, states[a - 1]), a
    _same_records(np.concatenate(recs), want, (name, tail))
    assert np.array_equal(np.concatenate(cands), _cands(want))


def test_entry_ids_need_not_be_consecutive(gpu, monkeypatch):
    """Every second keyframe, then a few out of order: each query still has the
    entry before it as its previous keyframe and max_id from its own id."""
    p, _, _, _ = _expected("default")
    n, ids, sc, nss = _oracle_query(p.max_db_results, p.recent_frames_window)
    det = _detector(p, monkeypatch)
    for sub in (np.arange(1, N, 2), np.array([400, 401, 0, 403, 403, 405, 120, 406])):
        want, states, _ = _oracle_decide(sub, n[sub], ids[sub], sc[sub], nss[sub], sub > 0, p)
        det.db[0].temporal_state = np.zeros(4, np.int32)
        got, cand = det.db[0].detect_entries(sub.astype(np.int32), det.detect_params())
        _same_records(got, want, sub[:3])
        assert np.array_equal(cand, _cands(want)) and np.array_equal(det.db[0].temporal_state, states[-1])
        assert (want["status"] == abi.BOW_STATUS.index("LOOP_DETECTED")).sum() >= 2


def test_temporal_state(gpu, monkeypatch):
    p, want, states, _ = _expected("default")
    det = _detector(p, monkeypatch)
    db = det.db[0]
    assert np.array_equal(db.temporal_state, np.zeros(4, np.int32))
    # set the state of an interrupted stream, then continue it
    cut = 371  # inside the run of detections: the state matters for what follows
    assert states[cut - 1][0] > 0 and want["status"][cut] == abi.BOW_STATUS.index("LOOP_DETECTED")
    db.temporal_state = states[cut - 1]
    assert np.array_equal(db.temporal_state, states[cut - 1])
    assert det.detectLoopStream(0, cut, N - cut) == _tuples(want)[cut:]
    assert np.array_equal(db.temporal_state, states[-1])
    # without the state the continuation differs (the first detection has no predecessor)
    assert det.detectLoopStream(0, cut, N - cut, reset=True) != _tuples(want)[cut:]
    # reset=True, kmx_bow_reset and set_entries zero the state
    assert det.detectLoopStream(0, 0, N, reset=True) == _tuples(want)
    assert db.temporal_state[0] > 0
    _, allf = _input()
    db.set_entries(allf.vptr, allf.words, allf.weights)
    assert np.array_equal(db.temporal_state, np.zeros(4, np.int32))
    assert det.detectLoopStream(0, 0, N) == _tuples(want)
    db.reset()
    assert np.array_equal(db.temporal_state, np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        db.temporal_state = [1, 2, 3]


def test_inter_robot_mode(gpu, monkeypatch):
    monkeypatch.setenv("KMX_BOW_TAIL", "5")
    st, _ = _input()
    db = st.subset(np.nonzero(st.robot == 0)[0])
    r1 = st.subset(np.nonzero(st.robot == 1)[0])
    det = BowDetector(LcdParams(), n_words=st.n_words)
    for a in range(0, 320, 10):
        det.add_vectors(0, *_prefix(db, a, a + 10))
        det.add_vectors(1, *_prefix(r1, a, a + 10))
    qids = np.arange(320, dtype=np.int32)
    m, s, nss = det.detectLoopWithRobotDevice(0, 1, qids)
    pv = _prefix(r1, 0, 319)
    prev = (np.concatenate([[0], pv[0]]).astype(np.int64), pv[1], pv[2])
    D = O.OracleBowDb(st.n_words, db.vptr, db.words, db.weights)
    m0, s0, nss0 = D.detect_batch(r1.vptr, r1.words, r1.weights, *prev)
    assert np.array_equal(nss, nss0) and np.array_equal(m, m0) and np.array_equal(s, s0)
    m1, s1, nss1 = det.detectLoopWithRobotResident(0, 1, qids)
    assert np.array_equal(m, m1) and np.array_equal(s, s1) and np.array_equal(nss, nss1)
    assert m[0] == -1 and nss[0] == 0.0 and (m >= 0).sum() > 80
    # no temporal stage: the state of the queried database is untouched
    assert np.array_equal(det.db[0].temporal_state, np.zeros(4, np.int32))
    # a shuffled subset with repeats, entry 0 in the middle
    sub = np.array([17, 0, 319, 5, 5, 200, 1], np.int32)
    m2, s2, nss2 = det.detectLoopWithRobotDevice(0, 1, sub)
    assert np.array_equal(m2, m0[sub]) and np.array_equal(s2, s0[sub]) and np.array_equal(nss2, nss0[sub])


def _rows(K, seed, nq=2048):
    """Seeded query results [nq, K]: unique ids from a range small enough for
    multi-member islands, scores descending with the lower id first on ties,
    and hand-made rows in front (those that fit K)."""
    rng = np.random.default_rng(seed)
    n = np.zeros(nq, np.int32)
    ids = np.full((nq, K), -1, np.int32)
    sc = np.zeros((nq, K))
    nss = rng.choice([0.03, 0.06, 0.1, 0.5, 1.0, 1.2], nq) * rng.uniform(0.9, 1.1, nq)
    has_prev = (rng.random(nq) < 0.95).astype(np.int32)
    qids = np.cumsum(rng.integers(1, 5, nq)).astype(np.int32)
    base = 2000 + np.cumsum(rng.integers(-4, 5, nq))  # a slow walk: consecutive queries' islands often overlap

    def put(q, pairs, f=0.1):
        pairs = sorted(pairs, key=lambda t: (-t[1], t[0]))
        if len(pairs) > K:
            return
        n[q] = len(pairs)
        ids[q, :len(pairs)] = [t[0] for t in pairs]
        sc[q, :len(pairs)] = [t[1] for t in pairs]
        nss[q], has_prev[q] = f, 1

    for q in range(nq):
        m = int(rng.choice([0, 1, K // 2, K, rng.integers(0, K + 1)], p=[0.03, 0.05, 0.12, 0.3, 0.5]))
        span = max(m, 1) * int(rng.choice([1, 2, 3, 6]))
        i = rng.choice(span, m, replace=False) + int(base[q])
        s = rng.uniform(rng.choice([0.0, 0.05, 0.5]), 1.0, m)
        if rng.random() < 0.4:
            s = np.ceil(s * 8) / 8  # many exact ties
        o = np.lexsort((i, -s))
        n[q] = m
        ids[q, :m], sc[q, :m] = i[o], s[o]
    a, b, c = 0.8125, 0.3, 0.7
    put(0, [])                                                       # n = 0
    put(1, [(40, 0.9), (3, 0.01), (4, 0.01)])                        # k = 1 after the cut
    put(2, [(7, 0.9)])                                               # n = k = 1
    put(3, [(100 + i, 0.1 + 0.013 * ((i * 7) % 11)) for i in range(min(K, 40))])  # one island spanning everything
    put(4, [(10 * i, 0.2 + 0.01 * i) for i in range(min(K, 30))])    # all singletons
    put(5, [(20, a), (21, a), (22, a), (23, b)])                     # ties inside an island: the lowest id is best
    put(6, [(40, a), (41, b), (42, c), (10, a), (11, b), (12, c)])   # equal sums in the same order: the first wins
    put(7, [(10, 0.6), (12, 0.5), (50, 0.9)])                        # span 3 with 2 members; a singleton beside it
    put(8, [(5, 0.5), (7, 0.5), (30, 0.25), (32, 0.75)])             # 0.5 + 0.5 == 0.25 + 0.75: the first wins
    put(9, [(9, 0.9), (8, 0.9)], f=1.2)                              # the cut is alpha * nss = 0.48
    for a_ in (n, ids, sc, nss, has_prev, qids):
        a_.setflags(write=False)
    return qids, n, ids, sc, nss, has_prev


@pytest.mark.parametrize("K,over", [(1, dict(use_nss=0)), (2, dict(min_matches_per_island=3)), (7, {}),
                                    (7, dict(min_matches_per_island=3)), (50, {}),
                                    (50, dict(min_matches_per_island=3, max_intraisland_gap=2)),
                                    (64, dict(min_matches_per_island=3)), (65, dict(alpha=0.1)),
                                    (256, dict(min_matches_per_island=2, alpha=0.1))],
                         ids=lambda v: str(v) if isinstance(v, int) else ",".join(f"{k}={x}" for k, x in v.items()))
def test_decide_caller_supplied_results(gpu, K, over):
    p = LcdParams(**over)
    qids, n, ids, sc, nss, has_prev = _rows(K, 100 + K)
    want, states, shape = _oracle_decide(qids, n, ids, sc, nss, has_prev, p)
    st = want["status"]
    if K >= 7:  # the rows reach what they are meant to
        assert set(np.unique(st).tolist()) >= {0, 1, 2, 4, 5}
        assert shape[:, 0].max() > 1 and shape[:, 1].max() > 1 and (want["n_kept"] == K).any()
        assert want["match_id"][5] == 20 and want["match_id"][6] == 10
        if p.max_intraisland_gap > 2:
            assert (want["island_start"][7], want["island_end"][7], want["island_start"][8]) == (10, 12, 5)
        else:  # ids two apart are islands of their own, each too short to keep
            assert st[7] == st[8] == abi.BOW_STATUS.index("NO_GROUPS")
    assert st[0] == 0 and want["n_kept"][2] == 1
    det = BowDetector(p, n_words=1000)
    db = det._robot_db(0)
    got = db.decide_results(n, ids, sc, det.detect_params(), nss=nss, has_prev=has_prev, query_ids=qids)
    _same_records(got, want, (K, over))
    assert np.array_equal(db.temporal_state, np.zeros(4, np.int32))  # a pass of its own
    # on the handle's state, in two calls: the second continues the first
    h = 1000
    g1 = db.decide_results(n[:h], ids[:h], sc[:h], det.detect_params(), nss=nss[:h], has_prev=has_prev[:h],
                           query_ids=qids[:h], use_state=True)
    assert np.array_equal(db.temporal_state, states[h - 1])
    g2 = db.decide_results(n[h:], ids[h:], sc[h:], det.detect_params(), nss=nss[h:], has_prev=has_prev[h:],
                           query_ids=qids[h:], use_state=True)
    _same_records(np.concatenate([g1, g2]), want, (K, over, "two calls"))
    assert np.array_equal(db.temporal_state, states[-1])
    db.close()


def test_refusals(gpu, monkeypatch):
    p = LcdParams()
    _, allf = _input()
    G = BowDatabase(allf.n_words)
    ids = np.arange(4, dtype=np.int32)
    rec = np.zeros(4, abi.BOW_RECORD_DTYPE)
    recp = rec.ctypes.data_as(C.POINTER(abi.BowDetectRecord))
    nc = C.c_int32(0)
    good = BowDetector(p, n_words=allf.n_words).detect_params()

    def call(params, ids_=ids, nq=4):
        return G.L.kmx_bow_detect_entries(G.h, G.h, nq, abi.iptr(ids_), 0, params, recp, None, C.byref(nc))

    assert call(C.byref(good)) == abi.KMX_ESTATE  # before any database
    with pytest.raises(abi.KmxError):
        G.detect_entries(ids, good)
    monkeypatch.setenv("KMX_BOW_TAIL", "5")
    G.reset()
    G.add(*_prefix(allf, 0, 130))
    want = G.detect_entries(np.arange(130, dtype=np.int32), good)[0]
    G.temporal_state = np.zeros(4, np.int32)
    assert call(None) == abi.KMX_EINVAL  # a null params pointer
    for k in (0, 257, -1):
        bad = BowDetector(LcdParams(max_db_results=k), n_words=allf.n_words).detect_params()
        assert call(C.byref(bad)) == abi.KMX_EINVAL
        with pytest.raises(abi.KmxError):
            G.detect_entries(ids, bad)
        n1 = np.ones(4, np.int32)
        assert G.L.kmx_bow_decide_results(G.h, 4, 1, None, abi.iptr(n1), abi.iptr(n1), abi.fptr(np.ones(4)), None,
                                          None, 0, C.byref(bad), 0, recp) == abi.KMX_EINVAL
    bad = BowDetector(LcdParams(alpha=float("inf")), n_words=allf.n_words).detect_params()
    assert call(C.byref(bad)) == abi.KMX_EINVAL
    for e in (130, -1, 1 << 30):  # an entry id out of range
        assert call(C.byref(good), np.array([0, 1, e, 2], np.int32)) == abi.KMX_EINVAL
    assert G.L.kmx_bow_detect_entries(G.h, G.h, 4, abi.iptr(ids), 2, C.byref(good), recp, None, None) == abi.KMX_EINVAL
    # decide_results: a count beyond K, K beyond 256
    n5 = np.array([1, 5, 0, 2], np.int32)
    z = np.zeros((4, 4), np.int32)
    assert G.L.kmx_bow_decide_results(G.h, 4, 4, None, abi.iptr(n5), abi.iptr(z), abi.fptr(np.zeros((4, 4))), None,
                                      None, 0, C.byref(good), 0, recp) == abi.KMX_EINVAL
    assert G.L.kmx_bow_decide_results(G.h, 4, 257, None, abi.iptr(n5), abi.iptr(z), abi.fptr(np.zeros((4, 4))), None,
                                      None, 0, C.byref(good), 0, recp) == abi.KMX_EINVAL
    # the handle is as it was: the same stream gives the same records
    assert np.array_equal(G.temporal_state, np.zeros(4, np.int32))
    _same_records(G.detect_entries(np.arange(130, dtype=np.int32), good)[0], want, "after refusals")
    p0, want0, _, _ = _expected("default")
    _same_records(want, want0[:130], "prefix")
    G.close()
