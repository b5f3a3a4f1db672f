"""The top-K selection of kmx_bow_query* on MI355X under ties and clustered
scores: k_bow_query (KMX_BOW_LDS=0, one sort buffer of 2048), k_bow_query_lds
(a buffer of 1024 per chunk; chunks of 14336, 1104 and 112 entries), k_bow_tail
(1000 unsealed entries that tie with sealed ones) and the resident form
(query_entries of a stored copy of the query).

Every expected value is tests/bow_query_ref.py's: n, every id and every score
are compared with ==, for K = 1, 50, 256, without max_id and with one seeded
max_id array (-1, 0, a value that cuts the largest tie group in two, random
ones). Whether a call succeeds is derived from the reference's results and the
selection grid's constants (bow_query_ref.base_depth): where no level fits the
form's buffer the call must return KMX_EUNSUP, the next call on the handle must
answer a good query like the reference, and a later async call and its fetch
must succeed. test_bow_select_cpu.py pins the depth every family reaches under
every form (levels 0..5 of both kernels), so the inputs cannot hollow out.

No test hands a query kernel a vector outside its contract: the weight tests
exercise the host's refusal only.
"""
import ctypes as C

import numpy as np
import pytest

from kmx import abi
from kmx.lcd.bow import BowDatabase
from tests import bow_query_ref as R

pytestmark = pytest.mark.gpu

FAILED_TEMPORAL = abi.BOW_STATUS.index("FAILED_TEMPORAL_CONSTRAINT")
ENV_KEYS = ("KMX_BOW_TAIL", "KMX_BOW_CHUNK", "KMX_BOW_LDS")


def _setenv(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _same(got, res, K, what):
    n, ids, sc = got
    assert n.shape[0] == len(res), what
    for q, (ids0, acc0) in enumerate(res):
        n0 = min(K, ids0.shape[0])
        assert n[q] == n0, (what, q)
        assert np.array_equal(ids[q, :n0], ids0[:n0]), (what, q)
        assert np.array_equal(sc[q, :n0], -acc0[:n0] / 2.0), (what, q)


def _refused(call, what):
    with pytest.raises(abi.KmxError) as e:
        call()
    assert f"({abi.KMX_EUNSUP})" in str(e.value), (what, str(e.value))


def _host_query(G):
    return lambda qs, K, mids: G.query(*R.csr(qs), K, mids)


def _resident_query(G, src):
    """query_entries of stored copies of the query vectors (held by src)."""
    def run(qs, K, mids):
        src.set_entries(*R.csr(qs))
        return G.query_entries(np.arange(len(qs), dtype=np.int32), K, mids, src=src)
    return run


def _run_family(G, name, cap, query, form, what):
    """Every call of the family on handle G through `query`; `form` is how
    bow_query_ref.base_depth sees G. Returns (calls answered, calls refused)."""
    f = R.family(name, cap)
    answered = refused = 0
    for K in R.KS:
        for with_max_id in (False, True):
            qs, mids = R.batch(name, cap, with_max_id)
            res = R.expected(name, cap, K, with_max_id)
            tag = (what, name, cap, K, with_max_id)
            if R.call_depth(res, K, **form) is not None:
                _same(query(qs, K, mids), res, K, tag)
                answered += 1
                continue
            _refused(lambda: query(qs, K, mids), tag)
            # the handle stays usable: the next call answers a good query ...
            good = R.expected(name, cap, K, good=True)
            assert R.call_depth(good, K, **form) is not None
            _same(query(f.good, K, None), good, K, tag + ("after",))
            if refused == 0:  # ... and so does a later async call, after a refused fetch
                G.query_async(*R.csr(qs), K, mids)
                _refused(lambda: G.fetch(len(qs), K), tag + ("fetch",))
                G.query_async(*R.csr(f.good), K, None)
                _same(G.fetch(len(f.good), K), good, K, tag + ("async after",))
            refused += 1
    return answered, refused


@pytest.mark.parametrize("name,cap", R.FAMILIES, ids=lambda v: str(v))
@pytest.mark.parametrize("form", list(R.FORMS))
def test_every_family_under_every_form(gpu, form, name, cap, monkeypatch):
    _setenv(monkeypatch, R.FORMS[form]["env"])
    f = R.family(name, cap)
    G = BowDatabase(f.n_words)
    G.set_entries(f.vptr, f.words, f.weights)
    answered, refused = _run_family(G, name, cap, _host_query(G), R.FORMS[form]["depth"], form)
    assert answered + refused == 6
    G.close()


@pytest.mark.parametrize("name,cap", R.FAMILIES, ids=lambda v: str(v))
def test_streaming_tail_ties_with_the_base(gpu, name, cap, monkeypatch):
    """2000 entries sealed, 1000 in the tail (k_bow_tail merges them, ties with
    sealed entries included); then all sealed: the same answers."""
    _setenv(monkeypatch, {})
    f = R.family(name, cap)
    G = BowDatabase(f.n_words)
    G.set_tail_cap(1024)
    G.reset()
    assert G.add(*f.db(0, R.STREAM_SEALED)) == 0
    G.seal()
    assert G.add(*f.db(R.STREAM_SEALED, f.n)) == R.STREAM_SEALED
    info = G.info()
    assert (info["n_entries"], info["n_sealed"], info["tail_cap"]) == (f.n, R.STREAM_SEALED, 1024)
    _run_family(G, name, cap, _host_query(G), dict(lds=True, n_sealed=R.STREAM_SEALED), "tail")
    G.seal()
    assert G.info()["n_sealed"] == f.n
    _run_family(G, name, cap, _host_query(G), dict(lds=True), "sealed")
    G.close()


@pytest.mark.parametrize("name,cap", R.FAMILIES, ids=lambda v: str(v))
def test_resident_query(gpu, name, cap, monkeypatch):
    _setenv(monkeypatch, {})
    f = R.family(name, cap)
    G, src = BowDatabase(f.n_words), BowDatabase(f.n_words)
    G.set_entries(f.vptr, f.words, f.weights)
    _run_family(G, name, cap, _resident_query(G, src), dict(lds=True), "resident")
    G.close()
    src.close()


@pytest.mark.parametrize("name,cap", R.LCH_EDGE, ids=lambda v: str(v))
def test_default_chunk_limit(gpu, name, cap, monkeypatch):
    """14335, 14336 and 14337 entries: below, at and above the default chunk;
    the best entries sit at the limit and at the end."""
    _setenv(monkeypatch, {})
    f = R.family(name, cap)
    G = BowDatabase(f.n_words)
    G.set_entries(f.vptr, f.words, f.weights)
    answered, refused = _run_family(G, name, cap, _host_query(G), dict(lds=True), "lch")
    assert (answered, refused) == (6, 0)
    G.close()


# (family, cap, form, K) -> refused? Stated outright; the reference must agree.
CAP_EDGES = [
    ("tied_at_cap", 2048, "hbm", 256, False), ("tied_at_cap", 1024, "lds", 256, False),
    ("tied_over_cap", 2048, "hbm", 1, True), ("tied_over_cap", 2048, "hbm", 256, True),
    ("tied_over_cap", 1024, "lds", 1, True), ("tied_over_cap", 1024, "lds", 256, True),
    ("past_cut", 2048, "hbm", 1, False), ("past_cut", 2048, "hbm", 50, False), ("past_cut", 2048, "hbm", 256, True),
    ("past_cut", 2048, "lds", 1, False), ("past_cut", 2048, "lds", 50, False), ("past_cut", 2048, "lds", 256, True),
    # certain entries from level 0, the cut found at level 1 just before a tie group of 2740
    ("two_step", 2048, "hbm", 256, False), ("two_step", 2048, "lds", 256, False),
    # the LDS cap is per chunk: 1025 tied entries in one chunk of 1104, or 512 + 513 over two
    ("one_chunk_1025", 2048, "chunk1100", 50, True), ("split_1025", 2048, "chunk1100", 50, False),
    ("split_1025", 2048, "chunk1100", 256, False),
]


@pytest.mark.parametrize("name,cap,form,K,refused", CAP_EDGES, ids=lambda v: str(v))
def test_cap_edges(gpu, name, cap, form, K, refused, monkeypatch):
    _setenv(monkeypatch, R.FORMS[form]["env"])
    f = R.family(name, cap)
    qs, _ = R.batch(name, cap)
    res = R.expected(name, cap, K)
    assert (R.call_depth(res, K, **R.FORMS[form]["depth"]) is None) == refused
    G = BowDatabase(f.n_words)
    G.set_entries(f.vptr, f.words, f.weights)
    if refused:
        _refused(lambda: G.query(*R.csr(qs), K), (name, form, K))
        _same(G.query(*R.csr(f.good), K), R.expected(name, cap, K, good=True), K, (name, form, K, "after"))
    else:
        got = G.query(*R.csr(qs), K)
        _same(got, res, K, (name, form, K))
        if name.startswith("tied_at_cap") or name == "split_1025":  # the lowest ids of the tied value
            tied = np.sort(np.nonzero(f.weights[0::2] == R.TIED)[0])
            assert np.array_equal(got[1][0, :K], tied[:K])
    G.close()


def test_refused_detection_leaves_the_temporal_state(gpu, monkeypatch):
    """detect_entries whose query selection fails returns KMX_EUNSUP and leaves
    the temporal state as it was; the next call gives what a fresh handle
    brought to that state gives."""
    _setenv(monkeypatch, {})
    f = R.detect_family()
    p = abi.BowDetectParams(0, 0.0, 0.0, 256, 50, 3, 1, 2, 3, 1)
    G = BowDatabase(f.n_words)
    G.set_entries(f.vptr, f.words, f.weights)
    rec, _ = G.detect_entries(np.arange(100, 108, dtype=np.int32), p)
    assert (rec["status"] >= FAILED_TEMPORAL).all()  # every query reached the temporal pass
    before = G.temporal_state.copy()
    assert before[0] >= 1 and before[1] == 107
    # entry 1400 ties with 1157 eligible entries at the cut (test_bow_select_cpu.py)
    bad_ids = np.array([350, 1400, 351], np.int32)
    _refused(lambda: G.detect_entries(bad_ids, p), "detect")
    assert np.array_equal(G.temporal_state, before)
    # the same through kmx_bow_detect_entries_async / kmx_bow_detect_fetch
    L = abi.lib()
    abi.check(L.kmx_bow_detect_entries_async(G.h, G.h, 3, abi.iptr(bad_ids), abi.BOW_MODE_INTRA, C.byref(p)),
              "kmx_bow_detect_entries_async")
    out, cand, nc = np.zeros(3, abi.BOW_RECORD_DTYPE), np.zeros((3, 2), np.int32), C.c_int32(0)
    assert L.kmx_bow_detect_fetch(G.h, 3, out.ctypes.data_as(C.POINTER(abi.BowDetectRecord)), abi.iptr(cand),
                                  C.byref(nc)) == abi.KMX_EUNSUP
    assert np.array_equal(G.temporal_state, before)
    good_ids = np.arange(352, 360, dtype=np.int32)
    rec1, cand1 = G.detect_entries(good_ids, p)
    H = BowDatabase(f.n_words)
    H.set_entries(f.vptr, f.words, f.weights)
    H.temporal_state = before
    rec0, cand0 = H.detect_entries(good_ids, p)
    assert rec1.tobytes() == rec0.tobytes()
    assert np.array_equal(cand1, cand0)
    assert np.array_equal(G.temporal_state, H.temporal_state)
    assert (rec1["status"] >= FAILED_TEMPORAL).all() and (rec1["query_id"] == good_ids).all()
    G.close()
    H.close()


BAD_WEIGHTS = [0.0, -0.0, -0.25, float("nan"), float("inf"), float("-inf")]


@pytest.mark.parametrize("form", ["lds", "hbm"])
def test_bad_weights_are_refused_on_the_host(gpu, form, monkeypatch):
    """add and set_entries return KMX_EINVAL for a weight that is not finite
    and > 0; info() and the next query are unchanged. The vectors never reach
    a kernel."""
    _setenv(monkeypatch, R.FORMS[form]["env"])
    f = R.family("spread")
    G = BowDatabase(f.n_words)
    G.set_entries(*f.db(0, 500))
    info0 = G.info()
    want = [R.results_l1(f.n_words, *f.db(0, 500), *f.queries[0])]
    _same(G.query(*R.csr(f.queries), 50), want, 50, "before")
    vptr, words, weights = f.db(500, 520)
    for bad in BAD_WEIGHTS:
        for k in (0, weights.shape[0] - 1):  # the first word of the batch, the last word of its last vector
            w = weights.copy()
            w[k] = bad
            for call in (lambda: G.add(vptr, words, w), lambda: G.set_entries(vptr, words, w)):
                with pytest.raises(abi.KmxError) as e:
                    call()
                assert f"({abi.KMX_EINVAL})" in str(e.value) and "finite and > 0" in str(e.value)
                assert G.info() == info0
            _same(G.query(*R.csr(f.queries), 50), want, 50, ("after", bad, k))
    w = weights.copy()
    w[0] = 5e-324  # a denormal is legal
    assert G.add(vptr, words, w) == 500
    assert G.info()["n_entries"] == 520
    G.close()
