"""BoW candidate stage of Kimera-Multi-LCD on MI355X.

Mirrors the reference's detection calls (drawio:2574-2580, 2612-2633,
drawio:1565) on top of kmx_bow_* (C ABI, bow.hip):

  BowDatabase.query          DBoW2 Database::queryL1 (batched; GPU)
  BowDatabase.score_pairs    L1Scoring::score (the nss factor; GPU)
  BowDatabase.add / add_transformed   DBoW2 Database::add, one keyframe or
                             batch at a time: the vectors stay resident on
                             the device (from host CSR, or straight from a
                             GpuVocabulary's last transform)
  BowDatabase.query_entries / score_entries   the same query / score with the
                             vectors named by entry id (nothing uploaded)
  BowDetector.detectLoopWithRobot   nss vs the previous keyframe of the query
                             robot, min_nss_factor gate, max_db_results query,
                             alpha * nss cut, best result (batched)
  BowDetector.add_vectors / add_frames / detectLoopResident /
  detectLoopWithRobotResident   the streaming forms: keyframes are added as
                             they arrive and detection runs by entry id
  BowDetector.detectLoop     single-robot stream: query with
                             max_id = frame - recent_frames_window, nss / alpha
                             cut, computeIslands, checkTemporalConstraint
                             (sequential control on the host, queries batched)
  BowDatabase.detect_entries / decide_results / temporal_state,
  BowDetector.detectLoopStream / detectLoopStreamCandidates /
  detectLoopWithRobotDevice  the same decisions made on the device
                             (kmx_bow_detect_entries): one record per keyframe
                             comes back, the temporal constraint's state stays
                             in the database across calls, so one keyframe per
                             call gives what one call over the stream gives

Constants are LcdParams (params/D455/LcdParams.yaml:3-12). DBoW2 and
kimera_multi_lcd are not vendored: the restatement is "parity unpinned" and
checked bit-exact against oracle/bow_oracle.c (tests/test_bow_gpu.py).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from .. import abi
from ..abi import check, fptr, i64ptr, iptr, u32ptr
from .detector import LcdParams


def _csr(vptr, words, weights):
    return (np.ascontiguousarray(vptr, np.int64), np.ascontiguousarray(words, np.uint32),
            np.ascontiguousarray(weights, np.float64))


class BowDatabase:
    """An L1 DBoW2 database of BowVectors (entry id = insertion index) on one GPU."""

    def __init__(self, n_words: int, device: int = 0):
        L = abi.lib()
        if abi.device_count() <= device:
            raise abi.KmxError(f"no HIP device {device} visible (kmx has no CPU fallback)")
        h = C.c_void_p()
        check(L.kmx_bow_create(device, C.byref(h)), "kmx_bow_create")
        self.L, self.h, self.n_words, self.n = L, h, int(n_words), 0

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.L.kmx_bow_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_entries(self, vptr, words, weights):
        """Database::add of every vector, in order (replaces the database)."""
        vptr, words, weights = _csr(vptr, words, weights)
        n = vptr.shape[0] - 1
        check(self.L.kmx_bow_set_database(self.h, self.n_words, n, i64ptr(vptr), u32ptr(words),
                                          fptr(weights)), "kmx_bow_set_database")
        self.n = n  # a refused database leaves the old one in place

    # ---- streaming: Database::add, the vectors resident on the device
    def reset(self):
        """An empty database (the state set_entries of no vectors leaves)."""
        check(self.L.kmx_bow_reset(self.h, self.n_words), "kmx_bow_reset")
        self.n = 0

    def add(self, vptr, words, weights) -> int:
        """Database::add of each vector, in order -> the first new entry id."""
        vptr, words, weights = _csr(vptr, words, weights)
        first = C.c_int32(-1)
        check(self.L.kmx_bow_add_entries(self.h, vptr.shape[0] - 1, i64ptr(vptr), u32ptr(words), fptr(weights),
                                         C.byref(first)), "kmx_bow_add_entries")
        self.n += vptr.shape[0] - 1
        return first.value

    def add_transformed(self, gpu_voc):
        """Append the vectors gpu_voc's last transform / transform_async left on
        the device (no host copy) -> (first new entry id, count)."""
        first, n = C.c_int32(-1), C.c_int32(0)
        check(self.L.kmx_bow_add_from_voc(self.h, gpu_voc.h, C.byref(first), C.byref(n)), "kmx_bow_add_from_voc")
        self.n += n.value
        return first.value, n.value

    def seal(self):
        """Move the unsealed tail into the inverted file now (on the device)."""
        check(self.L.kmx_bow_seal(self.h), "kmx_bow_seal")

    def set_tail_cap(self, cap: int):
        check(self.L.kmx_bow_set_tail_cap(self.h, int(cap)), "kmx_bow_set_tail_cap")

    def info(self) -> dict:
        v = [C.c_int32() for _ in range(4)] + [C.c_int64(), C.c_int64()]
        check(self.L.kmx_bow_info(self.h, *[C.byref(x) for x in v]), "kmx_bow_info")
        return dict(zip(("n_words", "n_entries", "n_sealed", "tail_cap", "n_postings", "device_bytes"),
                        (x.value for x in v)))

    def lengths(self, first: int, n: int):
        """Word counts of stored vectors [first, first + n) (no device access)."""
        vptr = np.zeros(n + 1, np.int64)
        check(self.L.kmx_bow_get_entries(self.h, first, n, i64ptr(vptr), None, None, 0), "kmx_bow_get_entries")
        return np.diff(vptr)

    def entries(self, first: int, n: int):
        """Stored vectors [first, first + n) read back as CSR (vptr, words, weights)."""
        vptr = np.zeros(n + 1, np.int64)
        check(self.L.kmx_bow_get_entries(self.h, first, n, i64ptr(vptr), None, None, 0), "kmx_bow_get_entries")
        tot = int(vptr[-1])
        words, weights = np.zeros(max(tot, 1), np.uint32), np.zeros(max(tot, 1))
        check(self.L.kmx_bow_get_entries(self.h, first, n, i64ptr(vptr), u32ptr(words), fptr(weights), tot),
              "kmx_bow_get_entries")
        return vptr, words[:tot], weights[:tot]

    def query_entries(self, ids, max_results: int = 50, max_id=None, src=None):
        """query with the query vectors taken from stored entries `ids` of
        `src` (another BowDatabase on the same device; None: this one)."""
        ids = np.ascontiguousarray(ids, np.int32)
        nq = ids.shape[0]
        mid = None if max_id is None else np.ascontiguousarray(max_id, np.int32)
        n = np.zeros(nq, np.int32)
        out = np.full((nq, max_results), -1, np.int32)
        sc = np.zeros((nq, max_results))
        check(self.L.kmx_bow_query_entries(self.h, (src or self).h, nq, iptr(ids),
                                           iptr(mid) if mid is not None else None, max_results, iptr(n), iptr(out),
                                           fptr(sc)), "kmx_bow_query_entries")
        return n, out, sc

    def query_entries_async(self, ids, max_results: int = 50, max_id=None, src=None):
        ids = np.ascontiguousarray(ids, np.int32)
        mid = None if max_id is None else np.ascontiguousarray(max_id, np.int32)
        self._keep = (ids, mid)
        check(self.L.kmx_bow_query_entries_async(self.h, (src or self).h, ids.shape[0], iptr(ids),
                                                 iptr(mid) if mid is not None else None, max_results),
              "kmx_bow_query_entries_async")

    def fetch(self, nq: int, max_results: int = 50):
        """Results of the last query_async / query_entries_async (nq queries, same max_results)."""
        n = np.zeros(nq, np.int32)
        ids = np.full((nq, max_results), -1, np.int32)
        sc = np.zeros((nq, max_results))
        check(self.L.kmx_bow_fetch(self.h, nq, max_results, iptr(n), iptr(ids), fptr(sc)), "kmx_bow_fetch")
        return n, ids, sc

    def score_entries(self, a_ids, b_ids):
        """L1 scores of pairs of stored entries; an id of -1 scores 0."""
        a, b = np.ascontiguousarray(a_ids, np.int32), np.ascontiguousarray(b_ids, np.int32)
        if a.shape != b.shape or a.ndim != 1:
            raise ValueError("a_ids and b_ids must be 1-d and of the same length")
        out = np.zeros(a.shape[0])
        check(self.L.kmx_bow_score_entries(self.h, a.shape[0], iptr(a), iptr(b), fptr(out)), "kmx_bow_score_entries")
        return out

    # ---- detectLoop / detectLoopWithRobot decided on the device
    def detect_entries(self, ids, params: "abi.BowDetectParams", mode: int = abi.BOW_MODE_INTRA, src=None):
        """kmx_bow_detect_entries: query, nss gate, alpha cut, islands and (intra
        mode) the temporal constraint for stored entries `ids` of `src` (None:
        this database), decided on the device. Returns (records, candidates):
        a numpy array of abi.BOW_RECORD_DTYPE, one per query, and the int32
        [n, 2] (query id, match id) pairs of the LOOP_DETECTED records (intra
        mode). The temporal state stays in the database across calls."""
        ids = np.ascontiguousarray(ids, np.int32)
        nq = ids.shape[0]
        rec = np.zeros(nq, abi.BOW_RECORD_DTYPE)
        cand = np.zeros((max(nq, 1), 2), np.int32)
        nc = C.c_int32(0)
        check(self.L.kmx_bow_detect_entries(self.h, (src or self).h, nq, iptr(ids), int(mode), C.byref(params),
                                            rec.ctypes.data_as(C.POINTER(abi.BowDetectRecord)), iptr(cand),
                                            C.byref(nc)), "kmx_bow_detect_entries")
        return rec, cand[:nc.value].copy()

    def decide_results(self, n, ids, scores, params: "abi.BowDetectParams", nss=None, has_prev=None,
                       query_ids=None, mode: int = abi.BOW_MODE_INTRA, use_state: bool = False):
        """kmx_bow_decide_results: the same decision on query results the caller
        holds (n [nq], ids / scores [nq, K] sorted by score descending, lower id
        first on ties). use_state: run the temporal pass on the database's
        state instead of from zeros. Returns the records."""
        n = np.ascontiguousarray(n, np.int32)
        ids = np.ascontiguousarray(ids, np.int32)
        scores = np.ascontiguousarray(scores, np.float64)
        nq = n.shape[0]
        if ids.ndim != 2 or ids.shape != scores.shape or ids.shape[0] != nq:
            raise ValueError("ids and scores must be [nq, K]")
        opt = [None if a is None else np.ascontiguousarray(a, t)
               for a, t in ((query_ids, np.int32), (nss, np.float64), (has_prev, np.int32))]
        if any(a is not None and a.shape != (nq,) for a in opt):
            raise ValueError("query_ids, nss and has_prev must be [nq]")
        qid, ns, hp = opt
        rec = np.zeros(nq, abi.BOW_RECORD_DTYPE)
        check(self.L.kmx_bow_decide_results(self.h, nq, ids.shape[1], iptr(qid) if qid is not None else None, iptr(n),
                                            iptr(ids), fptr(scores), fptr(ns) if ns is not None else None,
                                            iptr(hp) if hp is not None else None, int(mode), C.byref(params),
                                            1 if use_state else 0,
                                            rec.ctypes.data_as(C.POINTER(abi.BowDetectRecord))),
              "kmx_bow_decide_results")
        return rec

    @property
    def temporal_state(self):
        """The temporal constraint's state on the device: int32 [4] =
        (temporal entries, latest query id, latest island start, end)."""
        st = np.zeros(4, np.int32)
        check(self.L.kmx_bow_get_temporal_state(self.h, iptr(st)), "kmx_bow_get_temporal_state")
        return st

    @temporal_state.setter
    def temporal_state(self, state):
        st = np.ascontiguousarray(state, np.int32)
        if st.shape != (4,):
            raise ValueError("the temporal state is 4 integers")
        check(self.L.kmx_bow_set_temporal_state(self.h, iptr(st)), "kmx_bow_set_temporal_state")

    def enable_timing(self, on: bool = True):
        check(self.L.kmx_bow_enable_timing(self.h, 1 if on else 0), "kmx_bow_enable_timing")

    def detect_timing(self):
        """Milliseconds of the last detection call with timing on:
        (gather + query + nss, k_bow_decide, k_bow_temporal)."""
        ms = np.zeros(3)
        check(self.L.kmx_bow_read_detect_timing(self.h, fptr(ms)), "kmx_bow_read_detect_timing")
        return ms

    def query(self, qptr, words, weights, max_results: int = 50, max_id=None):
        """queryL1 of each query vector -> (n [nq], ids [nq, K], scores [nq, K])."""
        qptr, words, weights = _csr(qptr, words, weights)
        nq = qptr.shape[0] - 1
        mid = None if max_id is None else np.ascontiguousarray(max_id, np.int32)
        n = np.zeros(nq, np.int32)
        ids = np.full((nq, max_results), -1, np.int32)
        sc = np.zeros((nq, max_results))
        check(self.L.kmx_bow_query(self.h, nq, i64ptr(qptr), u32ptr(words), fptr(weights),
                                   iptr(mid) if mid is not None else None, max_results, iptr(n), iptr(ids),
                                   fptr(sc)), "kmx_bow_query")
        return n, ids, sc

    def query_async(self, qptr, words, weights, max_results: int = 50, max_id=None):
        qptr, words, weights = _csr(qptr, words, weights)
        self._keep = (qptr, words, weights)
        mid = None if max_id is None else np.ascontiguousarray(max_id, np.int32)
        check(self.L.kmx_bow_query_async(self.h, qptr.shape[0] - 1, i64ptr(qptr), u32ptr(words), fptr(weights),
                                         iptr(mid) if mid is not None else None, max_results),
              "kmx_bow_query_async")

    def sync(self):
        check(self.L.kmx_bow_sync(self.h), "kmx_bow_sync")

    def score_pairs(self, a, b):
        """L1 scores of pairs: a, b = (vptr, words, weights) with the same count."""
        aptr, aw, av = _csr(*a)
        bptr, bw, bv = _csr(*b)
        n = aptr.shape[0] - 1
        out = np.zeros(n)
        check(self.L.kmx_bow_score_pairs(self.h, n, i64ptr(aptr), u32ptr(aw), fptr(av), i64ptr(bptr),
                                         u32ptr(bw), fptr(bv), fptr(out)), "kmx_bow_score_pairs")
        return out


@dataclass
class MatchIsland:
    start_id: int
    end_id: int
    island_score: float
    best_id: int
    best_score: float


def compute_islands(ids, scores, p: LcdParams) -> list[MatchIsland]:
    """LcdThirdPartyWrapper::computeIslands (DLoopDetector islands) [U]."""
    n = len(ids)
    if n == 0:
        return []
    if n == 1:
        return [MatchIsland(int(ids[0]), int(ids[0]), float(scores[0]), int(ids[0]), float(scores[0]))]
    order = np.argsort(np.asarray(ids), kind="stable")
    ids = [int(ids[i]) for i in order]
    sc = [float(scores[i]) for i in order]
    out = []
    first = last = ids[0]
    i_first = i_last = 0
    best_s, best_e = sc[0], ids[0]
    for idx in range(1, n + 1):
        if idx < n and ids[idx] - last < p.max_intraisland_gap:
            last, i_last = ids[idx], idx
            if sc[idx] > best_s:
                best_s, best_e = sc[idx], ids[idx]
            continue
        if last - first + 1 >= p.min_matches_per_island:
            s = 0.0
            for k in range(i_first, i_last + 1):
                s += sc[k]
            out.append(MatchIsland(first, last, s, best_e, best_s))
        if idx < n:
            first = last = ids[idx]
            i_first = i_last = idx
            best_s, best_e = sc[idx], ids[idx]
    return out


class TemporalConstraint:
    """LcdThirdPartyWrapper::checkTemporalConstraint state [U]."""

    def __init__(self, p: LcdParams):
        self.p = p
        self.entries = 0
        self.latest_query = 0
        self.latest = None

    def check(self, query_id: int, island: MatchIsland) -> bool:
        p = self.p
        if self.entries == 0 or query_id - self.latest_query > p.max_nrFrames_between_queries:
            self.entries = 1
        else:
            a1, a2 = self.latest.start_id, self.latest.end_id
            b1, b2 = island.start_id, island.end_id
            if (b1 <= a1 <= b2) or (a1 <= b1 <= a2) or (b1 <= a2 <= b2) or (a1 <= b2 <= a2):
                self.entries += 1
            else:
                gap = max(a1 - b2, b1 - a2)
                self.entries = self.entries + 1 if gap <= p.max_nrFrames_between_islands else 1
        self.latest, self.latest_query = island, query_id
        return self.entries > p.min_temporal_matches


class BowDetector:
    """Loop-candidate detection on BowVectors (one database per robot)."""

    def __init__(self, params: LcdParams | None = None, n_words: int = 1_000_000, device: int = 0,
                 vocabulary=None):
        """vocabulary: a kmx.lcd.vocabulary.Vocabulary. When given, n_words is
        the vocabulary's and `transform` turns ORB descriptors into the
        BowVectors the detection calls take; None (the default) leaves the
        detector on caller-made BowVectors over `n_words` words."""
        self.p = params or LcdParams()
        self.n_words = n_words if vocabulary is None else vocabulary.n_words
        self.device = device
        self.db: dict[int, BowDatabase] = {}
        self.vocabulary = vocabulary
        self._gpu_voc = None

    def transform(self, n_feats, desc):
        """DBoW2 transform of frames (desc uint8 [F, N, 32], n_feats [F]) with
        the detector's vocabulary: CSR (vptr, words, weights)."""
        if self.vocabulary is None:
            raise ValueError("BowDetector.transform needs a vocabulary (BowDetector(..., vocabulary=...))")
        if self._gpu_voc is None:
            from .vocabulary import GpuVocabulary
            self._gpu_voc = GpuVocabulary(self.vocabulary, self.device)
        return self._gpu_voc.transform(n_feats, desc)

    def set_robot_database(self, robot: int, vptr, words, weights):
        db = self.db.get(robot) or BowDatabase(self.n_words, self.device)
        db.set_entries(vptr, words, weights)
        self.db[robot] = db

    def detectLoopWithRobot(self, robot: int, query, prev):
        """Batched detectLoopWithRobot: query / prev = (vptr, words, weights) of the
        query keyframes and of their robots' previous keyframes (empty vector =
        no previous keyframe). Returns (match entry id or -1, score, nss)."""
        p = self.p
        db = self.db[robot]
        nq = len(query[0]) - 1
        nss = db.score_pairs(query, prev) if p.use_nss else np.ones(nq)
        has_prev = np.diff(np.asarray(prev[0])) > 0
        ok = has_prev & (nss >= p.min_nss_factor) if p.use_nss else np.ones(nq, bool)
        n, ids, sc = db.query(*query, max_results=p.max_db_results)
        match = np.full(nq, -1, np.int32)
        score = np.zeros(nq)
        thr = p.alpha * nss
        good = ok & (n > 0) & (sc[:, 0] >= thr)
        match[good] = ids[good, 0]
        score[good] = sc[good, 0]
        return match, score, np.where(has_prev, nss, 0.0)

    def detectLoop(self, robot: int, frames, first_frame: int = 0):
        """Single-robot detectLoop over keyframes first_frame.. of `robot`'s
        database (frames = (vptr, words, weights) of the same keyframes, in
        order). The queries run as one GPU batch with max_id = frame -
        recent_frames_window (entries added after their own query are invisible,
        as in the sequential loop); nss, islands and the temporal constraint are
        the sequential host logic. Returns a list of (frame, status, match, score)."""
        p = self.p
        db = self.db[robot]
        vptr, words, weights = _csr(*frames)
        nq = vptr.shape[0] - 1
        fids = np.arange(first_frame, first_frame + nq)
        max_id = np.maximum(fids - p.recent_frames_window, 0).astype(np.int32)
        n, ids, sc = db.query(vptr, words, weights, p.max_db_results, max_id)
        # nss of keyframe q against keyframe q - 1 (the latest BoW vector)
        if nq > 1:
            a = (vptr[1:] - vptr[1], words[vptr[1]:vptr[-1]], weights[vptr[1]:vptr[-1]])
            b = (vptr[:-1] - vptr[0], words[vptr[0]:vptr[-2]], weights[vptr[0]:vptr[-2]])
            nss_tail = db.score_pairs(a, b)
        else:
            nss_tail = np.zeros(0)
        return self._stream_decisions(fids, n, ids, sc, nss_tail)

    def _stream_decisions(self, fids, n, ids, sc, nss_tail):
        """detectLoop's sequential host control over the batched query results."""
        p = self.p
        nq = len(fids)
        tc = TemporalConstraint(p)
        out = []
        for q in range(nq):
            fid = int(fids[q])
            if n[q] == 0:
                out.append((fid, "NO_MATCHES", -1, 0.0))
                continue
            nss = 1.0
            if p.use_nss:
                nss = nss_tail[q - 1] if q > 0 else 0.0
                if q == 0 or nss < p.min_nss_factor:
                    out.append((fid, "LOW_NSS_FACTOR", -1, 0.0))
                    continue
            keep = sc[q, :n[q]] >= p.alpha * nss
            if not keep.any():
                out.append((fid, "LOW_SCORE", -1, 0.0))
                continue
            k = int(np.argmin(keep)) if not keep.all() else int(n[q])  # results are sorted: a prefix
            islands = compute_islands(ids[q, :k], sc[q, :k], p)
            if not islands:
                out.append((fid, "NO_GROUPS", -1, 0.0))
                continue
            best = max(islands, key=lambda isl: isl.island_score)
            if not tc.check(fid, best):
                out.append((fid, "FAILED_TEMPORAL_CONSTRAINT", best.best_id, best.best_score))
                continue
            out.append((fid, "LOOP_DETECTED", best.best_id, best.best_score))
        return out

    # ---- streaming forms: keyframes are added as they arrive, detection runs by entry id
    def _robot_db(self, robot: int) -> BowDatabase:
        db = self.db.get(robot)
        if db is None:
            db = self.db[robot] = BowDatabase(self.n_words, self.device)
            db.reset()
        return db

    def add_vectors(self, robot: int, vptr, words, weights):
        """Database::add of BowVectors to `robot`'s database (created empty on
        first use) -> the new entry ids."""
        db = self._robot_db(robot)
        first = db.add(vptr, words, weights)
        return np.arange(first, db.n, dtype=np.int32)

    def add_frames(self, robot: int, n_feats, desc):
        """Transform frames (desc uint8 [F, N, 32], n_feats [F]) with the
        detector's vocabulary and add their vectors to `robot`'s database; the
        vectors go from the transform to the database on the device -> the
        new entry ids."""
        if self.vocabulary is None:
            raise ValueError("BowDetector.add_frames needs a vocabulary (BowDetector(..., vocabulary=...))")
        if self._gpu_voc is None:
            from .vocabulary import GpuVocabulary
            self._gpu_voc = GpuVocabulary(self.vocabulary, self.device)
        db = self._robot_db(robot)
        if len(n_feats) == 0:
            return np.zeros(0, np.int32)
        self._gpu_voc.transform_async(n_feats, desc)
        first, n = db.add_transformed(self._gpu_voc)
        return np.arange(first, first + n, dtype=np.int32)

    def detectLoopResident(self, robot: int, first_frame: int, n_frames: int):
        """detectLoop over entries first_frame .. first_frame + n_frames - 1 of
        `robot`'s database, the queries and the nss factors taken by entry id:
        the list detectLoop(robot, frames, first_frame) returns for the same
        vectors."""
        p = self.p
        db = self.db[robot]
        fids = np.arange(first_frame, first_frame + n_frames, dtype=np.int32)
        max_id = np.maximum(fids - p.recent_frames_window, 0).astype(np.int32)
        n, ids, sc = db.query_entries(fids, p.max_db_results, max_id)
        nss_tail = db.score_entries(fids[1:], fids[:-1]) if n_frames > 1 else np.zeros(0)
        return self._stream_decisions(fids, n, ids, sc, nss_tail)

    # ---- decided on the device: one record per keyframe comes back
    def detect_params(self) -> "abi.BowDetectParams":
        """The BoW detection fields of the detector's LcdParams as kmx_bow_detect_params."""
        p = self.p
        return abi.BowDetectParams(int(p.use_nss), float(p.alpha), float(p.min_nss_factor), int(p.max_db_results),
                                   int(p.recent_frames_window), int(p.max_intraisland_gap),
                                   int(p.min_matches_per_island), int(p.max_nrFrames_between_queries),
                                   int(p.max_nrFrames_between_islands), int(p.min_temporal_matches))

    def detectLoopStream(self, robot: int, first_frame: int, n_frames: int, reset: bool = False,
                         candidates: bool = False):
        """detectLoop over entries first_frame .. first_frame + n_frames - 1 of
        `robot`'s database, decided on the device (kmx_bow_detect_entries): the
        list of (frame, status, match, score) detectLoopResident returns, from
        one 48-byte record per keyframe. The temporal constraint's state lives
        in the database and carries across calls, and a keyframe's previous
        keyframe is the entry before it, so a stream fed in any split, one
        keyframe per call included, gets the answers of one call over all of
        it. reset=True starts a new stream (zero state) first.

        The one difference from detectLoopResident: there, the first keyframe
        of every call has no previous keyframe and is LOW_NSS_FACTOR when
        use_nss is set; here only entry 0 is, since the previous keyframe of a
        window starting at first_frame > 0 is entry first_frame - 1 of the
        database. candidates=True returns (list, int32 [n, 2] array of the
        LOOP_DETECTED (query, match) pairs) instead."""
        db = self.db[robot]
        if reset:
            db.temporal_state = np.zeros(4, np.int32)
        fids = np.arange(first_frame, first_frame + n_frames, dtype=np.int32)
        rec, cand = db.detect_entries(fids, self.detect_params(), abi.BOW_MODE_INTRA)
        out = [(int(q), abi.BOW_STATUS[s], int(m), float(sc))
               for q, s, m, sc in zip(rec["query_id"], rec["status"], rec["match_id"], rec["score"])]
        return (out, cand) if candidates else out

    def detectLoopStreamCandidates(self, robot: int, first_frame: int, n_frames: int, reset: bool = False):
        """detectLoopStream's compact result: the (query, match) pairs of the
        LOOP_DETECTED keyframes, in order (what the verification stage takes)."""
        return self.detectLoopStream(robot, first_frame, n_frames, reset, candidates=True)[1]

    def detectLoopWithRobotDevice(self, robot: int, query_robot: int, query_ids):
        """detectLoopWithRobotResident decided on the device: the same
        (match entry id or -1, score, nss) arrays from one record per query."""
        db, src = self.db[robot], self.db[query_robot]
        rec, _ = db.detect_entries(query_ids, self.detect_params(), abi.BOW_MODE_INTER, src=src)
        return rec["match_id"].copy(), rec["score"].copy(), rec["nss"].copy()

    def detectLoopWithRobotResident(self, robot: int, query_robot: int, query_ids):
        """detectLoopWithRobot with the queries = entries `query_ids` of
        `query_robot`'s database and prev = the entry before each (none for
        id 0). Returns (match entry id or -1, score, nss)."""
        p = self.p
        db, src = self.db[robot], self.db[query_robot]
        qids = np.ascontiguousarray(query_ids, np.int32)
        nq = qids.shape[0]
        prev = qids - 1
        has_prev = prev >= 0
        if has_prev.any():
            lo = int(prev[has_prev].min())
            ln = src.lengths(lo, int(prev.max()) - lo + 1)
            has_prev[has_prev] = ln[prev[has_prev] - lo] > 0
        nss = src.score_entries(qids, prev) if p.use_nss else np.ones(nq)
        ok = has_prev & (nss >= p.min_nss_factor) if p.use_nss else np.ones(nq, bool)
        n, ids, sc = db.query_entries(qids, p.max_db_results, src=src)
        match = np.full(nq, -1, np.int32)
        score = np.zeros(nq)
        good = ok & (n > 0) & (sc[:, 0] >= p.alpha * nss)
        match[good] = ids[good, 0]
        score[good] = sc[good, 0]
        return match, score, np.where(has_prev, nss, 0.0)
