"""Cost of detectLoop decided on the device (kmx_bow_detect_entries: k_bow_decide,
k_bow_temporal, bow.hip) on the shape of bench.py's BoW leg: make_bow_stream(2,
25_000, n_words=100_000, seed=0), robot 0's keyframes as both the database and
the stream of queries (max_id = id - recent_frames_window), K = 50: 25k queries
on 25k entries. The last --revisit (5000) keyframes are the first ones again,
so that there are loops to detect.

  (a) the whole stream in one call: keyframes per second of detectLoopResident
      (query results copied out, the decision a per-query host loop) and of
      detectLoopStream (the decision on the device, one record per keyframe),
      alternating; detect_entries alone (the records, no Python list); and the
      evented time of the query stage, k_bow_decide and k_bow_temporal, with
      the sequential stage's cost per keyframe;
  (b) the online form, one keyframe per call on the full database: median and
      p95 of the per-call latency of detectLoopStream(robot, i, 1) and, as a
      time reference only (its answers differ: every call starts a fresh
      temporal constraint), of detectLoopResident(robot, i, 1), alternating;
  (c) with --parent-lib: kmx_bow_query_entries alone at the same shape in child
      processes that load the parent commit's library and this one's in turn,
      three runs each (the query path is untouched, so they should overlap).

Before timing, the first 512 records are compared with the CPU restatement
(oracle.detect_loop_stream); a mismatch, or no GPU, exits non-zero. Host wall
time around calls that end in a synchronise; warm-up, then medians of --runs
(>= 7). Nothing here is a pass mark.

  python scripts/bow_detect_bench.py [--frames 25000] [--runs 7] [--parent-lib PATH] [--out profiles/bow_detect.json]
"""
import argparse
import ctypes as C
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "kimera-multi_amd"))
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402


def _stream(frames, words, revisit):
    """Robot 0's first frames - revisit keyframes, then its first `revisit`
    again: the loops detectLoop is there to find (without them every keyframe
    of this stream ends at the alpha cut and no island is ever built)."""
    from kmx.synth.bow import make_bow_stream
    st = make_bow_stream(2, frames, n_words=words, seed=0)
    r0 = np.nonzero(st.robot == 0)[0]
    revisit = max(0, min(revisit, frames // 2))
    return st, st.subset(np.concatenate([r0[:frames - revisit], r0[:revisit]]))


def child_query_entries(a):
    """(c): kmx_bow_query_entries_async + sync through plain ctypes, so that a
    library without the newer entry points loads too. Prints seconds per call."""
    st, db = _stream(a.frames, a.words, a.revisit)
    L = C.CDLL(a.child_lib)
    P, i32 = C.c_void_p, C.c_int32
    pi32 = C.POINTER(i32)
    L.kmx_bow_create.argtypes = [C.c_int, C.POINTER(P)]
    L.kmx_bow_set_database.argtypes = [P, i32, i32, C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    L.kmx_bow_query_entries_async.argtypes = [P, P, i32, pi32, pi32, i32]
    L.kmx_bow_sync.argtypes = [P]
    L.kmx_bow_destroy.argtypes = [P]
    h = P()
    assert L.kmx_bow_create(0, C.byref(h)) == 0
    vptr, w, v = (np.ascontiguousarray(db.vptr, np.int64), np.ascontiguousarray(db.words, np.uint32),
                  np.ascontiguousarray(db.weights, np.float64))
    assert L.kmx_bow_set_database(h, st.n_words, db.n, vptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                  w.ctypes.data_as(C.POINTER(C.c_uint32)), v.ctypes.data_as(C.POINTER(C.c_double))) == 0
    ids = np.arange(db.n, dtype=np.int32)
    mid = np.maximum(ids - a.window, 0).astype(np.int32)
    ts = []
    for r in range(a.warmup + a.runs):
        t = time.perf_counter()
        assert L.kmx_bow_query_entries_async(h, h, db.n, ids.ctypes.data_as(pi32), mid.ctypes.data_as(pi32), a.K) == 0
        assert L.kmx_bow_sync(h) == 0
        if r >= a.warmup:
            ts.append(time.perf_counter() - t)
    L.kmx_bow_destroy(h)
    print("CHILD " + json.dumps(ts), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=25000)
    ap.add_argument("--words", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--revisit", type=int, default=5000, help="the last keyframes of the stream repeat the first ones")
    ap.add_argument("--online", type=int, default=2000, help="(b): keyframes timed one per call (the last of the stream)")
    ap.add_argument("--parent-lib", default="", help="(c): the parent commit's libkmx.so")
    ap.add_argument("--commit", default="", help="the commit the tree under test is based on (recorded in the result)")
    ap.add_argument("--out", default="")
    ap.add_argument("--child-lib", default="", help=argparse.SUPPRESS)
    ap.add_argument("--K", type=int, default=50, help=argparse.SUPPRESS)
    ap.add_argument("--window", type=int, default=100, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_lib:
        return child_query_entries(a)
    if a.runs < 7:
        ap.error("--runs must be at least 7")

    from kmx import abi
    from kmx.lcd import LcdParams
    from kmx.lcd.bow import BowDetector
    from oracle import oracle as O
    try:
        ndev = abi.device_count()
    except abi.KmxError:
        ndev = 0
    if ndev < 1:
        print("no GPU found", file=sys.stderr)
        return 2
    p = LcdParams()
    t = time.time()
    st, db = _stream(a.frames, a.words, a.revisit)
    print(f"generated {st.n} BowVectors in {time.time() - t:.1f} s", flush=True)
    N = db.n
    det = BowDetector(p, n_words=st.n_words)
    det.set_robot_database(0, db.vptr, db.words, db.weights)
    G = det.db[0]
    res = {"what": "detectLoop decided on the device: whole stream in one call, one keyframe per call, query regression",
           "frames": N, "revisit": a.revisit, "n_words": st.n_words, "postings": int(db.vptr[-1]), "max_db_results": p.max_db_results,
           "recent_frames_window": p.recent_frames_window, "warmup": a.warmup, "runs": a.runs}

    # ---- the first 512 records against the CPU restatement
    m = min(512, N)
    pre = (db.vptr[:m + 1] - db.vptr[0], db.words[:db.vptr[m]], db.weights[:db.vptr[m]])
    want = O.detect_loop_stream(O.OracleBowDb(st.n_words, *pre), *pre, 0, p)
    got = det.detectLoopStream(0, 0, m, reset=True)
    if got != want:
        bad = [i for i in range(m) if got[i] != want[i]]
        print(f"MISMATCH against the oracle at {bad[:5]}: {[got[i] for i in bad[:5]]} != {[want[i] for i in bad[:5]]}",
              file=sys.stderr)
        return 1
    counts = {s: sum(1 for g in got if g[1] == s) for s in abi.BOW_STATUS}
    print(f"first {m} records equal the oracle's: {counts}", flush=True)
    res["checked_against_oracle"] = {"records": m, "status_counts": counts}

    # ---- (a) the whole stream in one call, the forms alternating
    fids = np.arange(N, dtype=np.int32)
    dp = det.detect_params()

    def resident():
        return det.detectLoopResident(0, 0, N)

    def stream():
        return det.detectLoopStream(0, 0, N, reset=True)

    def records():
        G.temporal_state = np.zeros(4, np.int32)
        return G.detect_entries(fids, dp)

    forms = {"detectLoopResident": resident, "detectLoopStream": stream, "detect_entries": records}
    ts = {k: [] for k in forms}
    outs = {}
    for r in range(a.warmup + a.runs):
        for k, fn in forms.items():
            t = time.perf_counter()
            outs[k] = fn()
            if r >= a.warmup:
                ts[k].append(time.perf_counter() - t)
    if outs["detectLoopResident"] != outs["detectLoopStream"]:
        print("MISMATCH: detectLoopStream differs from detectLoopResident on the whole stream", file=sys.stderr)
        return 1
    full = {s: sum(1 for g in outs["detectLoopStream"] if g[1] == s) for s in abi.BOW_STATUS}
    res["batched_stream"] = {k: {"keyframes_per_s_median": N / float(np.median(v)), "seconds_median": float(np.median(v)),
                                 "seconds_all": v} for k, v in ts.items()}
    res["batched_stream"]["status_counts"] = full
    res["batched_stream"]["candidates"] = int(outs["detect_entries"][1].shape[0])
    G.enable_timing(True)
    ev = []
    for r in range(a.runs):
        records()
        ev.append(G.detect_timing().tolist())
    G.enable_timing(False)
    ev = np.median(np.array(ev), axis=0)
    res["batched_stream"]["evented_ms"] = {
        "gather_query_nss": float(ev[0]), "k_bow_decide": float(ev[1]), "k_bow_temporal": float(ev[2]),
        "k_bow_temporal_ns_per_keyframe": float(1e6 * ev[2] / N), "k_bow_decide_ns_per_keyframe": float(1e6 * ev[1] / N)}
    for k, v in res["batched_stream"].items():
        print(f"(a) {k}: {v if not isinstance(v, dict) or 'seconds_all' not in v else {x: y for x, y in v.items() if x != 'seconds_all'}}",
              flush=True)

    # ---- (b) one keyframe per call on the full database
    first = max(N - a.online, 1)
    lat = {"detectLoopStream": [], "detectLoopResident": []}
    for i in range(first - min(50, first - 1), N):  # the first 50 warm up
        for k in lat:
            t = time.perf_counter()
            if k == "detectLoopStream":
                det.detectLoopStream(0, i, 1)
            else:
                det.detectLoopResident(0, i, 1)
            if i >= first:
                lat[k].append(time.perf_counter() - t)
    res["online"] = {"entries": N, "calls": N - first,
                     **{k: {"median_us": float(1e6 * np.median(v)), "p95_us": float(1e6 * np.percentile(v, 95))}
                        for k, v in lat.items()}}
    print(f"(b) {res['online']}", flush=True)
    for h in det.db.values():
        h.close()

    # ---- (c) kmx_bow_query_entries alone, the parent's library and this one's in turn
    if a.parent_lib:
        libs = {"parent": str(Path(a.parent_lib).resolve()), "this": str(Path(abi.__file__).resolve().parent / "libkmx.so")}
        runs = {k: [] for k in libs}
        for r in range(3):
            for k, path in libs.items():
                out = subprocess.run([sys.executable, __file__, "--child-lib", path, "--frames", str(a.frames),
                                      "--words", str(a.words), "--revisit", str(a.revisit), "--runs", str(a.runs), "--warmup", str(a.warmup),
                                      "--K", str(p.max_db_results), "--window", str(p.recent_frames_window)],
                                     capture_output=True, text=True, timeout=600)
                line = [x for x in out.stdout.splitlines() if x.startswith("CHILD ")]
                if out.returncode or not line:
                    print(f"(c) the {k} child failed ({out.returncode}): {out.stderr[-400:]}", file=sys.stderr)
                    return 1
                v = json.loads(line[0][6:])
                runs[k].append({"queries_per_s_median": N / float(np.median(v)), "seconds_all": v})
                print(f"(c) {k} run {r}: {runs[k][-1]['queries_per_s_median']:.4g} queries/s", flush=True)
        res["query_entries_regression"] = runs
    else:
        res["query_entries_regression"] = "not run (no --parent-lib)"

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
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
