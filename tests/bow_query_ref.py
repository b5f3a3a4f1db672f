"""Plain restatement of DBoW2 Database::queryL1 and of the grid the top-K
selection of kmx_bow_query* narrows on, used ONLY by the selection tests
(test_bow_select_cpu.py, test_bow_select_gpu.py). numpy and the standard
library, nothing from kmx or oracle.

  query_l1        dense float64 accumulator; the query's words in increasing
                  word id, for every entry holding the word
                  acc[e] += fabs(q - d) - fabs(q) - fabs(d) (three float64
                  operations, then one addition: DBoW2's order, so results
                  compare with ==); a result holds >= 1 query word and has
                  id < max_id (or max_id == -1); order (acc ascending, id
                  ascending), the first K, score = -acc / 2.0
  score_exact     the same score from math.fsum over exactly representable
                  terms (a bound on query_l1's own rounding)
  levels_needed   the selection grid stated from its constants: NBINS = 1024
                  bins per level, LEVELS = 6 levels over [-2, 0], so a level-l
                  cell of acc is floor((acc + 2) * 2**(10 * (l + 1) - 1))
                  (widths 2^-9, 2^-19, ..., 2^-59). The narrowing stops at the
                  first level at which the results whose cell is <= the cell
                  of the K-th best fit the sort buffer (`cap`); None if no
                  level under 6 does (the call returns KMX_EUNSUP).
  base_depth      levels_needed per kernel form: one buffer of SEL_CAP = 2048
                  over all sealed entries (KMX_BOW_LDS=0), or LSEL = 1024 per
                  chunk of `chunk` consecutive ids rounded up to a multiple of
                  16 (default LCH = 14336); the unsealed tail has no cap.

The input families are built here too (seeded, small); see `family`.
"""
import functools
import math
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

NBINS, LEVELS = 1024, 6
SEL_CAP, LSEL, LCH, LW_WAVES = 2048, 1024, 14336, 16
KS = (1, 50, 256)


# ---------------------------------------------------------------- queryL1 ---
def results_l1(n_words, vptr, words, weights, qwords, qweights, max_id=-1):
    """All results of one query in (acc, id) order: (ids int64, acc float64)."""
    vptr = np.asarray(vptr, np.int64)
    words = np.asarray(words, np.int64)
    weights = np.asarray(weights, np.float64)
    n = vptr.shape[0] - 1
    ent = np.repeat(np.arange(n, dtype=np.int64), np.diff(vptr))
    w_db, d_db = words[vptr[0]:vptr[-1]], weights[vptr[0]:vptr[-1]]
    acc = np.zeros(n, np.float64)
    hit = np.zeros(n, bool)
    qwords, qweights = np.asarray(qwords, np.int64), np.asarray(qweights, np.float64)
    assert (np.diff(qwords) > 0).all(), "query words must be strictly increasing"
    for w, q in zip(qwords.tolist(), qweights.tolist()):
        if w >= n_words:
            continue
        sel = np.nonzero(w_db == w)[0]  # ascending posting = ascending entry id
        e, d = ent[sel], d_db[sel]
        if max_id != -1:
            keep = e < max_id
            e, d = e[keep], d[keep]
        v = np.fabs(q - d) - math.fabs(q) - np.fabs(d)  # left to right, each rounded to float64
        acc[e] = acc[e] + v  # an entry holds a word once: no repeated index
        hit[e] = True
    ids = np.nonzero(hit)[0]
    order = np.lexsort((ids, acc[ids]))  # acc ascending, then id ascending
    ids = ids[order]
    return ids, acc[ids]


def query_l1(n_words, vptr, words, weights, qwords, qweights, K, max_id=-1):
    """DBoW2 queryL1 of one query -> (n, ids int32 [n], scores float64 [n])."""
    ids, acc = results_l1(n_words, vptr, words, weights, qwords, qweights, max_id)
    ids, acc = ids[:K], acc[:K]
    return ids.shape[0], ids.astype(np.int32), -acc / 2.0


def score_exact(vwords, vweights, wwords, wweights):
    """(score, c): -1/2 sum over the c common words of (|v - w| - |v| - |w|),
    the sum taken by math.fsum over the terms max(v, w), -min(v, w), -|v|, -|w|,
    each a float64 as given, so the only rounding is fsum's final one. For
    L1-normalised vectors this is 1 - 0.5 * |v - w|_1."""
    common, iv, iw = np.intersect1d(np.asarray(vwords), np.asarray(wwords), return_indices=True)
    terms = []
    for a, b in zip(np.asarray(vweights, np.float64)[iv].tolist(), np.asarray(wweights, np.float64)[iw].tolist()):
        terms += [max(a, b), -min(a, b), -abs(a), -abs(b)]
    return -math.fsum(terms) / 2.0, int(common.shape[0])


# --------------------------------------------------------- selection grid ---
def cells(acc, level):
    """The level-`level` cell of every acc, exactly: floor((acc + 2) * 2**(10 * (level + 1) - 1))."""
    acc = np.asarray(acc, np.float64)
    y = acc + 2.0
    if ((y - 2.0) == acc).all() and (y >= 0).all() and (y < 2.0).all():
        # acc + 2 is exact, a scaling by 2**59 is exact and stays below 2**63
        c5 = np.floor(np.ldexp(y, 10 * LEVELS - 1)).astype(np.int64)
        return c5 >> (10 * (LEVELS - 1 - level))
    out = [math.floor((Fraction(x) + 2) * (1 << (10 * (level + 1) - 1))) for x in acc.tolist()]
    return np.array(out, dtype=object)


def levels_needed(acc_of_results, K, cap):
    """Smallest level l < LEVELS at which #{results: cell_l <= cell_l of the K-th
    best} <= cap; None if there is none. No results or K == 0: level 0."""
    acc = np.sort(np.asarray(acc_of_results, np.float64))
    k = min(K, acc.shape[0])
    if k == 0:
        return 0
    for level in range(LEVELS):
        c = cells(acc, level)
        if int((c <= c[k - 1]).sum()) <= cap:
            return level
    return None


def chunk_size(chunk=None):
    """Entries per chunk of the LDS form for KMX_BOW_CHUNK=chunk (None: unset)."""
    ch = LCH if chunk is None else max(1, min(LCH, int(chunk)))
    return (ch + LW_WAVES - 1) // LW_WAVES * LW_WAVES


def base_depth(ids, acc, K, lds=True, chunk=None, n_sealed=None):
    """The deepest level the base kernel reaches for results (ids, acc) of one
    query, None if it fails. Results with id >= n_sealed are the tail's."""
    ids, acc = np.asarray(ids), np.asarray(acc)
    if n_sealed is not None:
        acc, ids = acc[ids < n_sealed], ids[ids < n_sealed]
    if not lds:
        return levels_needed(acc, K, SEL_CAP)
    ch = chunk_size(chunk)
    deepest = 0
    for c in np.unique(ids // ch).tolist():
        d = levels_needed(acc[ids // ch == c], K, LSEL)
        if d is None:
            return None
        deepest = max(deepest, d)
    return deepest


# The kernel forms the GPU test runs: the environment, and how base_depth sees them.
FORMS = {
    "lds": dict(env={}, depth=dict(lds=True)),
    "chunk1100": dict(env={"KMX_BOW_CHUNK": "1100"}, depth=dict(lds=True, chunk=1100)),
    "chunk97": dict(env={"KMX_BOW_CHUNK": "97"}, depth=dict(lds=True, chunk=97)),
    "hbm": dict(env={"KMX_BOW_LDS": "0"}, depth=dict(lds=False)),
}
STREAM_SEALED = 2000  # the streaming form: this many entries sealed, the rest in the tail


# ----------------------------------------------------------------- inputs ---
@dataclass(eq=False)
class Family:
    name: str
    n_words: int
    vptr: np.ndarray
    words: np.ndarray
    weights: np.ndarray
    queries: list            # [(words, weights)], the call under test
    good: list = field(default_factory=list)  # queries that succeed where `queries` is refused

    @property
    def n(self):
        return self.vptr.shape[0] - 1

    def db(self, a=0, b=None):
        """Entries [a, b) as CSR."""
        b = self.n if b is None else b
        return self.vptr[a:b + 1] - self.vptr[a], self.words[self.vptr[a]:self.vptr[b]], \
            self.weights[self.vptr[a]:self.vptr[b]]


def csr(vectors):
    """[(words, weights)] -> (ptr int64, words uint32, weights float64)."""
    ptr = np.zeros(len(vectors) + 1, np.int64)
    ptr[1:] = np.cumsum([len(w) for w, _ in vectors])
    words = np.concatenate([np.asarray(w, np.uint32) for w, _ in vectors]) if vectors else np.zeros(0, np.uint32)
    wts = np.concatenate([np.asarray(v, np.float64) for _, v in vectors]) if vectors else np.zeros(0)
    return ptr, words, wts


def two_word(name, a, perm=None):
    """Entry i = {word 0: a_i, word 1 + (i % 7): 1 - a_i} over 8 words, a_i in
    [0.5, 1); the query {word 0: 1.0} gives acc_i == -2 * a_i exactly (1 - a is
    exact, |1 - a| - 1 == -a, -a - a == -2a). perm: the values in the order
    given land on entry ids perm[0], perm[1], ... (None: in place). The `good`
    queries {word k: 1.0}, k = 1..7, each see one entry in seven."""
    a = np.asarray(a, np.float64)
    assert ((a >= 0.5) & (a < 1.0)).all()
    n = a.shape[0]
    if perm is not None:
        placed = np.empty(n)
        placed[perm] = a
        a = placed
    i = np.arange(n)
    words = np.stack([np.zeros(n, np.uint32), (1 + i % 7).astype(np.uint32)], 1).reshape(-1)
    weights = np.stack([a, 1.0 - a], 1).reshape(-1)
    assert (weights > 0).all()
    one = lambda k: (np.array([k], np.uint32), np.array([1.0]))
    return Family(name, 8, 2 * np.arange(n + 1, dtype=np.int64), words, weights, [one(0)],
                  [one(k) for k in range(1, 8)])


N = 3000
TIED = 0.8125
TIED2 = 0.8125 - 2.0 ** -12  # inside a level-0 cell, at the start of a level-1 cell
L_EXP = {"L1": 10, "L2": 20, "L3": 30, "L4": 40}


def _dyadic_vector(rng, n_words=32):
    k = int(rng.integers(3, 9))
    w = np.sort(rng.choice(n_words, k, replace=False)).astype(np.uint32)
    parts = np.ones(k, np.int64)  # 8 eighths over k words, each >= 1/8
    for _ in range(8 - k):
        parts[rng.integers(0, k)] += 1
    return w, parts / 8.0


@functools.lru_cache(maxsize=None)
def family(name, cap=SEL_CAP):
    """The seeded input families (n = 3000 unless stated):
      spread          a = 0.5 + 0.5 u                               depth 0
      L1 .. L4        a = 0.75 + 2^-e u, e = 10, 20, 30, 40         depth 1 .. 4
      L5              a in the 8 doubles 0.75 + k 2^-53             depth 5, ~375-way ties
      tied_at_cap     `cap` entries on a = 0.8125, the rest 0.5 + 0.25 u
      tied_over_cap   cap + 1 of them
      past_cut        60 entries 0.9 + 0.05 u, then 2940 tied
      two_step        60 entries 0.9 + 0.05 u, 200 entries one or two level-1
                      cells better than 2740 tied ones in the same level-0
                      cell: K = 256 takes 60 certain entries at level 0 and
                      must look for the 196th, not the 256th, at level 1
      one_chunk_1025  1025 tied entries at ids 0..1024 (one chunk of 1104)
      split_1025      the same 1025 at ids 592..1616 (512 + 513 over two chunks of 1104)
      dyadic          3-8 words of 32, weights k/8 summing to 1, 8 queries alike
      lch_edge_<n>    n two-word entries, L2-style, the 16 best in the last 20
                      ids and in ids 14330..14340
    Entry ids are a seeded permutation of the value order unless the ids are
    placed on purpose."""
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + cap)
    u = rng.random(N)
    perm = rng.permutation(N)
    if name == "spread":
        return two_word(name, 0.5 + 0.5 * u, perm)
    if name in L_EXP:
        return two_word(name, 0.75 + 2.0 ** -L_EXP[name] * u, perm)
    if name == "L5":
        return two_word(name, 0.75 + rng.integers(0, 8, N) * 2.0 ** -53, perm)
    if name in ("tied_at_cap", "tied_over_cap"):
        m = cap + (name == "tied_over_cap")
        return two_word(f"{name}_{cap}", np.concatenate([np.full(m, TIED), 0.5 + 0.25 * u[m:]]), perm)
    if name == "past_cut":
        return two_word(name, np.concatenate([0.9 + 0.05 * u[:60], np.full(N - 60, TIED)]), perm)
    if name == "two_step":
        return two_word(name, np.concatenate([0.9 + 0.05 * u[:60], TIED2 + 2.0 ** -20 * (1.0 + u[60:260]),
                                              np.full(N - 260, TIED2)]), perm)
    if name in ("one_chunk_1025", "split_1025"):
        first = 0 if name == "one_chunk_1025" else 592
        a = 0.5 + 0.25 * u
        a[first:first + 1025] = TIED
        return two_word(name, a)
    if name == "dyadic":
        vecs = [_dyadic_vector(rng) for _ in range(N)]
        ptr, w, v = csr(vecs)
        return Family(name, 32, ptr, w, v, [_dyadic_vector(rng) for _ in range(8)])
    if name.startswith("lch_edge_"):
        n = int(name[9:])
        a = 0.75 + 2.0 ** -20 * rng.random(n)
        spots = np.unique(np.concatenate([np.arange(n - 20, n), np.arange(14330, min(14341, n))]))
        best = rng.choice(spots, 16, replace=False)
        a[best] = 0.75 + 2.0 ** -20 * (1.0 + (1 + rng.permutation(16)) / 32.0)
        return two_word(name, a)
    raise KeyError(name)


def detect_family():
    """The detection case's database: tied_over_cap for the LDS form (1025
    entries on a = 0.8125, the rest 0.5 + 0.25 u) with the ids placed: the tied
    entries are ids 300..1324, and entry 1400 has the least a (0.5), so as a
    query it ties with every entry on word 0."""
    rng = np.random.default_rng(20240607)
    a = 0.5 + 0.25 * rng.random(N)
    a[300:1325] = TIED
    a[1400] = 0.5
    return two_word("tied_over_cap_placed", a)


FAMILIES = [("spread", SEL_CAP), ("L1", SEL_CAP), ("L2", SEL_CAP), ("L3", SEL_CAP), ("L4", SEL_CAP),
            ("L5", SEL_CAP), ("tied_at_cap", SEL_CAP), ("tied_at_cap", LSEL), ("tied_over_cap", SEL_CAP),
            ("tied_over_cap", LSEL), ("past_cut", SEL_CAP), ("two_step", SEL_CAP), ("one_chunk_1025", SEL_CAP), ("split_1025", SEL_CAP),
            ("dyadic", SEL_CAP)]
LCH_EDGE = [("lch_edge_14335", SEL_CAP), ("lch_edge_14336", SEL_CAP), ("lch_edge_14337", SEL_CAP)]


@functools.lru_cache(maxsize=None)
def max_ids(name, cap=SEL_CAP):
    """One seeded max_id per query slot (8): -1, 0, a value that cuts the
    largest tie group of the first query's results in two, then random ones."""
    f = family(name, cap)
    ids, acc = all_results(name, cap, 0, -1)
    vals, counts = np.unique(acc, return_counts=True)
    group = np.sort(ids[acc == vals[np.argmax(counts)]])
    cut = int(group[group.shape[0] // 2])
    rng = np.random.default_rng(f.n + cap)
    return np.array([-1, 0, cut] + rng.integers(1, f.n + 1, 5).tolist(), np.int32)


def batch(name, cap=SEL_CAP, with_max_id=False, good=False):
    """The queries of a call and its max_id array (None without one): the
    family's queries, cycled over the 8 max_id slots when with_max_id."""
    f = family(name, cap)
    qs = f.good if good else f.queries
    if not with_max_id:
        return qs, None
    return [qs[i % len(qs)] for i in range(8)], max_ids(name, cap)


@functools.lru_cache(maxsize=None)
def all_results(name, cap, q, max_id, good=False):
    """results_l1 of the family's query q (of `good` if set), cached and read-only."""
    f = family(name, cap)
    qw, qv = (f.good if good else f.queries)[q]
    ids, acc = results_l1(f.n_words, f.vptr, f.words, f.weights, qw, qv, max_id)
    ids.flags.writeable = acc.flags.writeable = False
    return ids, acc


def expected(name, cap, K, with_max_id=False, good=False):
    """What a call must return: [(ids, acc)] of all results per query (the
    answer is the first K of each) and the queries' (index, max_id) list."""
    f = family(name, cap)
    nq0 = len(f.good if good else f.queries)
    if with_max_id:
        slots = [(i % nq0, int(m)) for i, m in enumerate(max_ids(name, cap).tolist())]
    else:
        slots = [(i, -1) for i in range(nq0)]
    return [all_results(name, cap, q, m, good) for q, m in slots]


def call_depth(res, K, **form):
    """base_depth over a call's queries: the deepest, None if any query fails."""
    ds = [base_depth(ids, acc, K, **form) for ids, acc in res]
    return None if any(d is None for d in ds) else max(ds)
