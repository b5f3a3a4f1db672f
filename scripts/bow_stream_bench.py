"""Cost of the streaming BoW database (kmx_bow_add_entries / kmx_bow_query_entries,
bow.hip) on the shape of bench.py's BoW leg: make_bow_stream(2, 25_000,
n_words=100_000, seed=0), robot 0 as the database.

  (a) one frame at a time from 0 to N entries: add of one vector, then
      query_entries of it with max_id = id - recent_frames_window, results
      copied out (a host clock around calls that end in a synchronise), for
      each tail_cap; total, per-frame median, p99 and max (the seals live in
      the tail of the distribution), and the per-frame median around the
      sampled prefix sizes;
  (b) what a caller could do before the streaming interface: set_entries of
      the whole prefix, then query of the frame's vector, at sampled prefixes;
  (c) the batched query rate (robot 1's frames, enqueue-only query + sync)
      with the tail empty, half full and full, beside the same queries on a
      set_entries database;
  (d) batches of 10 frames x 500 descriptors: transform_async +
      add_transformed (no host hop) against transform + add;
  (e) the tail-scoring mapping: one is built (a wave per entry), so (c)'s
      full-tail line is its figure.

Warm-up runs, then medians over repeated runs, all in one process on one
device. Nothing here is a pass mark.

  python scripts/bow_stream_bench.py [--frames 25000] [--runs 3] [--out profiles/bow_stream.json]
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "kimera-multi_amd"))
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402


def one_at_a_time(st_db, n_words, tail_cap, window, K):
    """(a): per-frame seconds of add + query_entries over the whole stream."""
    from kmx.lcd.bow import BowDatabase
    G = BowDatabase(n_words)
    G.reset()
    G.set_tail_cap(tail_cap)
    vptr, words, weights = st_db.vptr, st_db.words, st_db.weights
    dt = np.zeros(st_db.n)
    one = np.zeros(2, np.int64)
    for i in range(st_db.n):
        a, b = vptr[i], vptr[i + 1]
        one[1] = b - a
        w, v = words[a:b], weights[a:b]
        t = time.perf_counter()
        fid = G.add(one, w, v)
        G.query_entries(np.array([fid], np.int32), K, np.array([max(fid - window, 0)], np.int32))
        dt[i] = time.perf_counter() - t
    info = G.info()
    G.close()
    return dt, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=25000)
    ap.add_argument("--words", type=int, default=100_000)
    ap.add_argument("--caps", default="16,32,64,256,1024")
    ap.add_argument("--prefixes", default="1000,5000,25000")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--voc-L", type=int, default=5)
    ap.add_argument("--commit", default="", help="the commit the tree under test is based on (recorded in the result)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    from kmx.lcd import LcdParams
    from kmx.lcd.bow import BowDatabase
    from kmx.synth.bow import make_bow_stream
    p = LcdParams()
    K, window = p.max_db_results, p.recent_frames_window
    t = time.time()
    st = make_bow_stream(2, a.frames, n_words=a.words, seed=0)
    db = st.subset(np.nonzero(st.robot == 0)[0])
    qs = st.subset(np.nonzero(st.robot == 1)[0])
    print(f"generated {st.n} BowVectors in {time.time() - t:.1f} s", flush=True)
    caps = [int(c) for c in a.caps.split(",")]
    prefixes = [min(int(x), db.n) for x in a.prefixes.split(",")]
    res = {"what": "streaming BoW database: add + query_entries one frame at a time, and what surrounds it",
           "frames": db.n, "n_words": st.n_words, "postings": int(db.vptr[-1]), "max_db_results": K,
           "recent_frames_window": window, "warmup": a.warmup, "runs": a.runs}

    # ---- (a)
    res["one_at_a_time"] = {}
    for i in range(a.warmup):
        one_at_a_time(db.subset(np.arange(min(db.n, 2000))), st.n_words, caps[0], window, K)
    for cap in caps:
        tot, runs = [], []
        for r in range(a.runs):
            dt, info = one_at_a_time(db, st.n_words, cap, window, K)
            tot.append(float(dt.sum()))
            runs.append(dt)
            print(f"(a) tail_cap {cap} run {r}: total {dt.sum():.3f} s, median {1e6 * np.median(dt):.1f} us, "
                  f"p99 {1e6 * np.percentile(dt, 99):.1f} us, max {1e3 * dt.max():.2f} ms", flush=True)
        dt = runs[int(np.argsort(tot)[len(tot) // 2])]  # the run with the median total
        near = {}
        for n in prefixes:
            lo, hi = max(n - 500, 0), min(n, db.n)
            near[str(n)] = {"median_us": float(1e6 * np.median(dt[lo:hi])), "mean_us": float(1e6 * dt[lo:hi].mean())}
        res["one_at_a_time"][str(cap)] = {
            "total_s_median": float(np.median(tot)), "total_s_all": tot,
            "per_frame_median_us": float(1e6 * np.median(dt)), "per_frame_p99_us": float(1e6 * np.percentile(dt, 99)),
            "per_frame_max_ms": float(1e3 * dt.max()), "per_frame_near_prefix": near,
            "n_sealed_at_end": info["n_sealed"], "device_bytes_at_end": info["device_bytes"]}

    # ---- (b)
    res["rebuild_baseline"] = {}
    S = BowDatabase(st.n_words)
    for n in prefixes:
        pre_vptr, pre_words, pre_weights = _slice(db, 0, n)
        w, v = db.vector(n - 1)
        qp = np.array([0, w.shape[0]], np.int64)
        mid = np.array([max(n - 1 - window, 0)], np.int32)
        ts = []
        for r in range(a.warmup + a.runs):
            t = time.perf_counter()
            S.set_entries(pre_vptr, pre_words, pre_weights)
            S.query(qp, w, v, K, mid)
            if r >= a.warmup:
                ts.append(time.perf_counter() - t)
        res["rebuild_baseline"][str(n)] = {"per_frame_ms_median": float(1e3 * np.median(ts)),
                                           "per_frame_ms_all": [1e3 * x for x in ts]}
        print(f"(b) prefix {n}: set_entries + query {1e3 * np.median(ts):.2f} ms", flush=True)
    for cap in caps:
        for n in prefixes:
            a_us = res["one_at_a_time"][str(cap)]["per_frame_near_prefix"][str(n)]["mean_us"]
            res["rebuild_baseline"][str(n)][f"ratio_to_streaming_cap{cap}"] = \
                1e3 * res["rebuild_baseline"][str(n)]["per_frame_ms_median"] / a_us

    # ---- (c)
    def rate(G, label):
        ts = []
        for r in range(a.warmup + a.runs + 2):
            t = time.perf_counter()
            G.query_async(qs.vptr, qs.words, qs.weights, K)
            G.sync()
            if r >= a.warmup:
                ts.append(time.perf_counter() - t)
        out = {"queries_per_s_median": qs.n / float(np.median(ts)), "seconds_all": ts, **G.info()}
        print(f"(c) {label}: {out['queries_per_s_median']:.4g} queries/s", flush=True)
        return out
    res["batched_query"] = {}
    S.set_entries(db.vptr, db.words, db.weights)
    res["batched_query"]["set_entries"] = rate(S, "set_entries")
    for label, tail in (("tail_empty", 0), ("tail_half", 512), ("tail_full", 1024)):
        G = BowDatabase(st.n_words)
        G.reset()
        G.set_tail_cap(1024)
        G.add(*_slice(db, 0, db.n - tail))
        G.seal()
        if tail:
            G.add(*_slice(db, db.n - tail, db.n))
        assert G.info()["n_sealed"] == db.n - tail
        res["batched_query"][label] = rate(G, label)
        G.close()
    res["batched_query"]["set_entries_again"] = rate(S, "set_entries again")
    S.close()

    # ---- (d)
    from kmx.lcd.vocabulary import GpuVocabulary
    from kmx.synth.vocab import make_descriptors, make_vocabulary
    voc = make_vocabulary(10, a.voc_L, seed=0, flip_bits=24)
    nb, bf, feats = 100, 10, 500
    desc = make_descriptors(voc, nb * bf, feats, noise_bits=20, seed=1).reshape(nb, bf, feats, 32)
    nf = np.full(bf, feats, np.int32)
    gv = GpuVocabulary(voc)
    tt = {"resident": [], "host_hop": []}
    for r in range(a.warmup + a.runs):
        for mode in ("resident", "host_hop"):
            G = BowDatabase(voc.n_words)
            G.reset()
            t = time.perf_counter()
            for b in range(nb):
                if mode == "resident":
                    gv.transform_async(nf, desc[b])
                    G.add_transformed(gv)
                else:
                    G.add(*gv.transform(nf, desc[b]))
            G.sync()
            if r >= a.warmup:
                tt[mode].append((time.perf_counter() - t) / nb)
            G.close()
    gv.close()
    res["transform_and_add"] = {"batch": f"{bf} frames x {feats} descriptors, {voc.n_words} words, {nb} batches",
                                "resident_ms_per_batch": float(1e3 * np.median(tt["resident"])),
                                "host_hop_ms_per_batch": float(1e3 * np.median(tt["host_hop"])),
                                "resident_all_ms": [1e3 * x for x in tt["resident"]],
                                "host_hop_all_ms": [1e3 * x for x in tt["host_hop"]]}
    print(f"(d) {res['transform_and_add']}", flush=True)
    res["tail_mapping"] = "a wave per tail entry (the only mapping built); its figure is batched_query.tail_full"

    commit = a.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "HEAD"], capture_output=True, text=True,
                                    check=True).stdout.strip()
        except Exception:
            commit = "unknown"
    res["measured_on_commit"] = commit
    print(json.dumps(res), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


def _slice(db, a, b):
    return db.vptr[a:b + 1] - db.vptr[a], db.words[db.vptr[a]:db.vptr[b]], db.weights[db.vptr[a]:db.vptr[b]]


if __name__ == "__main__":
    main()
