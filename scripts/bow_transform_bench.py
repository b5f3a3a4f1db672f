"""Throughput of the DBoW2 vocabulary transform (kmx_voc_*, voc.hip).

Shape: a synthetic k = 10, L = 6 vocabulary (1,111,111 nodes, 35.6 MB of node
descriptors) and 25,000 frames x 500 features, the BoW leg's 25k keyframes at
configs[2]'s feature count. The descriptors are uploaded once per run by the
enqueue-only call (kmx_voc_transform_async); the handle brackets its two
kernels with HIP events (kmx_voc_enable_timing), so the figures are device
times of the descent and of the per-frame reduction, upload excluded. Warm-up
runs, then the median of the timed runs.

Reported: frames/s and descriptors/s over both kernels, and the descent's
gathered bytes/s: the algorithmic bytes are sum(child_count * 32 B) over the
nodes a descriptor visits (k * L * 32 = 1,920 B on the regular tree; counted
on a sample of frames with the CPU restatement when the tree is irregular),
in all and for the levels the kernel reads from global memory (the top levels
come from LDS). The ceiling the fraction is stated against is the rate of
uniformly random rows of a 38 MB table served from the Infinity Cache (8.6
TB/s chip-wide on MI355X); only the global-memory levels count against it. It
is a ceiling, not a pass mark.

  python scripts/bow_transform_bench.py [--frames 25000] [--feats 500] [--runs 7]
      [--out profiles/bow_transform.json]
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

CEILING_BPS = 8.6e12  # uniformly random rows of a 38 MB table, Infinity Cache, chip-wide


def gathered_bytes_per_descriptor(voc, desc_sample, lds_nodes):
    """Algorithmic bytes the descent gathers per descriptor, 32 B per child of
    every visited node: (all levels, the levels read from global memory, how).
    The device holds the tree breadth first with its first lds_nodes nodes in
    LDS, so the children of the nodes at depth d come from LDS when the levels
    0..d+1 together have at most lds_nodes nodes (a level cut by the stage is
    counted as global)."""
    cnt = np.bincount(voc.parent[1:], minlength=voc.n_nodes)
    depth = np.zeros(voc.n_nodes, np.int64)
    for i in range(1, voc.n_nodes):  # ids are in creation order: a parent precedes its children
        depth[i] = depth[voc.parent[i]] + 1
    cum = np.cumsum(np.bincount(depth))
    from_global = np.array([d + 1 >= cum.shape[0] or cum[d + 1] > lds_nodes for d in range(cum.shape[0])])
    inner = cnt[cnt > 0]
    if inner.min() == inner.max() == voc.k and np.all(depth[cnt == 0] == voc.L):
        return (float(voc.k * voc.L * 32), float(voc.k * 32 * int(from_global[:voc.L].sum())),
                "exact (regular tree)")
    from tests import bow_transform_ref as ref
    leaves = ref.descend_numpy(voc, desc_sample.reshape(-1, 32))
    total = glob = 0
    node = leaves.copy()
    while np.any(node > 0):
        up = node > 0
        node[up] = voc.parent[node[up]]
        total += int(cnt[node[up]].sum())
        glob += int((cnt[node[up]] * from_global[depth[node[up]]]).sum())
    n = leaves.shape[0]
    return 32.0 * total / n, 32.0 * glob / n, f"sampled on {desc_sample.shape[0]} frames (CPU restatement)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=25000)
    ap.add_argument("--feats", type=int, default=500)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--L", type=int, default=6)
    ap.add_argument("--irregular", type=float, default=0.0)
    ap.add_argument("--noise-bits", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--check", type=int, default=4, help="frames compared with the CPU restatement (0: none)")
    ap.add_argument("--commit", default="", help="the commit the tree under test is based on (recorded in the result)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    from kmx.lcd.vocabulary import GpuVocabulary
    from kmx.synth.vocab import make_descriptors, make_vocabulary
    t = time.time()
    voc = make_vocabulary(a.k, a.L, seed=a.seed, flip_bits=24, irregular=a.irregular)
    desc = make_descriptors(voc, a.frames, a.feats, noise_bits=a.noise_bits, seed=a.seed + 1)
    nf = np.full(a.frames, a.feats, np.int32)
    print(f"generated {voc.n_nodes} nodes, {voc.n_words} words, {a.frames} x {a.feats} descriptors "
          f"in {time.time() - t:.1f} s", flush=True)
    gv = GpuVocabulary(voc)
    info = gv.info()
    bpd, gbpd, how = gathered_bytes_per_descriptor(voc, desc[:min(a.frames, 16)], info["lds_nodes"])
    if a.check:
        from tests import bow_transform_ref as ref
        n = min(a.check, a.frames)
        got = gv.transform(nf[:n], desc[:n])
        want = ref.transform(voc, nf[:n], desc[:n])
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), "GPU vectors differ from the CPU restatement"
        print(f"checked {n} frames against the CPU restatement: bit-exact", flush=True)
    gv.enable_timing(True)
    runs = []
    for i in range(a.warmup + a.runs):
        gv.transform_async(nf, desc)
        gv.sync()
        tm = gv.read_timing()
        if i >= a.warmup:
            runs.append(tm)
        print(f"run {i}{' (warm-up)' if i < a.warmup else ''}: descend {tm['descend_ms']:.3f} ms, "
              f"reduce {tm['reduce_ms']:.3f} ms", flush=True)
    gv.close()
    d_ms = float(np.median([r["descend_ms"] for r in runs]))
    r_ms = float(np.median([r["reduce_ms"] for r in runs]))
    n_desc = a.frames * a.feats
    commit = a.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "HEAD"], capture_output=True, text=True,
                                    check=True).stdout.strip()
        except Exception:
            commit = "unknown"
    res = {
        "what": "DBoW2 vocabulary transform (kmx_voc_transform_async), device time of its two kernels",
        "vocabulary": {"k": a.k, "L": a.L, "irregular": a.irregular, **info,
                       "descriptor_table_MB": voc.n_nodes * 32 / 1e6},
        "frames": a.frames, "feats_per_frame": a.feats, "descriptors": n_desc,
        "warmup": a.warmup, "runs": a.runs,
        "descend_ms_median": d_ms, "reduce_ms_median": r_ms,
        "descend_ms_all": [r["descend_ms"] for r in runs], "reduce_ms_all": [r["reduce_ms"] for r in runs],
        "frames_per_s": a.frames / ((d_ms + r_ms) * 1e-3),
        "descriptors_per_s": n_desc / ((d_ms + r_ms) * 1e-3),
        "gathered_bytes_per_descriptor": bpd, "gathered_bytes_how": how,
        "descend_gathered_bytes_per_s": bpd * n_desc / (d_ms * 1e-3),
        "global_gathered_bytes_per_descriptor": gbpd,
        "descend_global_gathered_bytes_per_s": gbpd * n_desc / (d_ms * 1e-3),
        "ceiling_bytes_per_s": CEILING_BPS,
        "ceiling": "uniformly random rows of a 38 MB table from the Infinity Cache, chip-wide",
        "mapping": "one lane per descriptor, top of the tree in LDS",
        "measured_on_commit": commit,
    }
    # the ceiling is a rate of global-memory rows: the levels served from LDS do not count against it
    res["fraction_of_ceiling"] = res["descend_global_gathered_bytes_per_s"] / CEILING_BPS
    print(json.dumps(res), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
