"""Times of the voxel simplification and the deformation-graph build on the
device (kmx_simplify_*, simplify.hip) next to the numpy reference.

Shape: dgraph_bench.py's (8 robots x 20,000 keyframes, `--verts-per-keyframe`
mesh vertices per keyframe, resolution `--resolution`), with or without
`--horizon-s`. One result per horizon is written: run the script once without
and once with `--horizon-s 2` and both land in the output file, under
"horizon_off" and "horizon_2s".

* numpy: simplify_voxel and graph_from_mesh on this machine's host clock.
* device, batch: one add of the whole mesh, the edge formation and the graph
  (links and emit), each by the handle's HIP events on a fresh handle per run:
  warm-up runs, then the median of the timed runs. Uploads and downloads are
  outside the events.
* device, streamed: the same mesh one keyframe's vertices and faces per add,
  `--stream-runs` times (default 1: the stream is 160,000 appends): the host
  clock over all appends, that per append, and the median and maximum of the
  appends' own event times.
* downloads (control rows, faces, vertex map; src, dst, w, link) on the host
  clock; slots, rehashes and device bytes from info().
* the equality of every array with numpy's.

Nothing is thresholded.

  python scripts/simplify_bench.py [--horizon-s 2] [--out profiles/simplify.json]
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


def med(x):
    return float(np.median(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=8)
    ap.add_argument("--poses", type=int, default=20_000, help="keyframes per robot")
    ap.add_argument("--verts-per-keyframe", type=int, default=6)
    ap.add_argument("--resolution", type=float, default=0.5)
    ap.add_argument("--horizon-s", type=float, default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--stream-runs", type=int, default=1)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "simplify.json"))
    a = ap.parse_args()

    from kmx.pgmo import MeshSimplifier, graph_from_mesh, simplify_voxel
    from kmx.synth import make_pose_graph
    from kmx.synth.mesh import make_mesh

    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else None

    g = make_pose_graph(a.robots, a.robots * a.poses, 0, seed=0)
    rest = [(g.init_R[r], g.init_t[r]) for r in range(a.robots)]
    mesh = make_mesh(g, a.verts_per_keyframe, 3.0, 1, chain=dict(enumerate(rest)))
    V, F = mesh.xyz.shape[0], mesh.faces.shape[0]

    # numpy on this host
    t0 = time.perf_counter()
    ref = simplify_voxel(mesh.xyz, mesh.faces, mesh.stamp, mesh.robot, a.resolution, horizon_s=a.horizon_s)
    t_simplify = time.perf_counter() - t0
    t0 = time.perf_counter()
    G = graph_from_mesh(ref[0], ref[1], ref[2], ref[3], mesh.kf_stamp, rest)
    t_graph = time.perf_counter() - t0
    print(f"{V} vertices, {F} faces -> {ref[0].shape[0]} control vertices, {ref[3].shape[0]} faces, "
          f"{G['src'].shape[0]} directed edges; numpy simplify_voxel {t_simplify:.2f} s, graph_from_mesh "
          f"{t_graph:.2f} s", flush=True)

    def equal(ms):
        got = (*ms.control(), ms.faces(), ms.vertex_map())
        Gd = ms.graph(mesh.kf_stamp, rest)
        return bool(all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(got, ref)) and
                    all(np.asarray(Gd[k]).dtype == np.asarray(G[k]).dtype and np.array_equal(Gd[k], G[k]) for k in G))

    # batch
    add_ms, edges_ms, graph_ms, wall_ms = [], [], [], []
    for _ in range(a.warmup + a.runs):
        with MeshSimplifier(a.resolution, a.horizon_s, a.robots) as ms:
            t0 = time.perf_counter()
            ms.add(mesh.xyz, mesh.faces, mesh.stamp, mesh.robot)
            ms.edges()
            ms.graph_arrays(mesh.kf_stamp)
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            tm = ms.timing()
            add_ms.append(tm["add_ms"])
            edges_ms.append(tm["edges_ms"])
            graph_ms.append(tm["graph_ms"])
    w = a.warmup
    with MeshSimplifier(a.resolution, a.horizon_s, a.robots) as ms:
        ms.add(mesh.xyz, mesh.faces, mesh.stamp, mesh.robot)
        ms.edges()
        t0 = time.perf_counter()
        ms.control(), ms.faces(), ms.vertex_map()
        t_down_simplify = time.perf_counter() - t0
        ms.graph_arrays(mesh.kf_stamp)  # sizes the buffers and forms everything once
        t0 = time.perf_counter()
        ms.graph_arrays(mesh.kf_stamp)
        t_down_graph = time.perf_counter() - t0  # the link and emit kernels again, and the four downloads
        info = ms.info()
        batch_equal = equal(ms)
    batch = {"add_ms_median": med(add_ms[w:]), "add_ms_min": float(min(add_ms[w:])),
             "edges_ms_median": med(edges_ms[w:]), "graph_ms_median": med(graph_ms[w:]),
             "host_clock_ms_median_with_uploads_and_graph_downloads": med(wall_ms[w:]),
             "download_simplify_s": t_down_simplify, "graph_call_with_downloads_s": t_down_graph,
             "info": info, "equals_numpy": batch_equal}
    print(json.dumps(batch), flush=True)

    # streamed: one keyframe per append; a keyframe's vertices and faces are contiguous in make_mesh's output
    vpk = a.verts_per_keyframe
    n_kf = V // vpk
    fmax = mesh.faces.max(1) // vpk
    assert (np.diff(fmax) >= 0).all() and (mesh.faces.min(1) // vpk == fmax).all()
    f_lo = np.searchsorted(fmax, np.arange(n_kf), side="left")
    f_hi = np.searchsorted(fmax, np.arange(n_kf), side="right")
    stream = []
    for _ in range(a.stream_runs):
        with MeshSimplifier(a.resolution, a.horizon_s, a.robots) as ms:
            per = np.empty(n_kf)
            t0 = time.perf_counter()
            for k in range(n_kf):
                v0 = k * vpk
                ms.add(mesh.xyz[v0:v0 + vpk], mesh.faces[f_lo[k]:f_hi[k]], mesh.stamp[v0:v0 + vpk],
                       mesh.robot[v0:v0 + vpk])
                per[k] = ms.timing()["add_ms"]
            total = time.perf_counter() - t0
            stream.append({"appends": n_kf, "host_clock_total_s": total, "host_clock_per_append_us": total / n_kf * 1e6,
                           "add_event_ms_median": med(per), "add_event_ms_max": float(per.max()),
                           "add_event_ms_sum": float(per.sum()), "info": ms.info(), "equals_numpy": equal(ms)})
            print(json.dumps(stream[-1]), flush=True)

    key = "horizon_off" if a.horizon_s is None else f"horizon_{a.horizon_s:g}s"
    out_path = Path(a.out)
    out = json.loads(out_path.read_text()) if out_path.exists() else {}
    out.update({"commit": commit, "device": "MI355X"})
    out[key] = {
        "robots": a.robots, "keyframes": a.robots * a.poses, "verts_per_keyframe": vpk, "vertices": V, "faces": F,
        "resolution_m": a.resolution, "horizon_s": a.horizon_s, "control_vertices": int(ref[0].shape[0]),
        "faces_kept": int(ref[3].shape[0]), "directed_edges": int(G["src"].shape[0]),
        "numpy_host": {"simplify_voxel_s": t_simplify, "graph_from_mesh_s": t_graph},
        "warmup": a.warmup, "runs": a.runs, "batch": batch, "stream_runs": a.stream_runs, "streamed": stream,
    }
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
