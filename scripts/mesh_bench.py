"""Bind and deform times of the mesh deformation (kmx_mesh_*, mesh.hip).

Shape: the keyframes of the configs[4] team (8 robots x 20,000 poses; the
generator's odometry chains are the rest poses, its ground truth stands in as
the optimised trajectory) as control nodes, and 52 vertices per keyframe
(8.32 M vertices, kmx.synth.mesh.make_mesh), k = 4, a window of 1 s (21
keyframes at 10 Hz).

The handle brackets its kernels with HIP events, so the figures are device
times, uploads excluded: warm-up runs, then the median of the timed runs, for
the bind kernel (every vertex bound again: rebind) and for the deformation
(k_mesh_deform and the one-wave reduction of its statistics, written to device
memory). Derived figures:

* bind: candidate visits per second. A visit is one (vertex, node in its
  window) pair, counted on the host from the stamps.
* deform: bytes per vertex by the layout (position in 12, count 4, k ids 4k,
  k weights 8k, position out 12; the gathered node rows, 120 B each, are 19 MB
  in all and come from the caches) and that over the time as a fraction of
  6.3 TB/s, the achievable HBM rate. A ceiling, not a pass mark.
* one re-deformation after update_trajectory, host clock around the upload of
  160,000 poses, the node kernel, the deformation and the wait.
* the numpy reference (tests/mesh_ref.py) on the first `--ref-vertices`
  vertices, for scale, and the device result on them against it.

Nothing is thresholded.

  python scripts/mesh_bench.py [--verts-per-keyframe 52] [--runs 20] [--out profiles/mesh_deform.json]
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

HBM_BPS = 6.3e12


def candidate_visits(mesh, W):
    total = 0
    for a, st in enumerate(mesh.kf_stamp):
        s = mesh.stamp[mesh.robot == a]
        total += int((np.searchsorted(st, s + W, "right") - np.searchsorted(st, s - W, "left")).sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=8)
    ap.add_argument("--poses", type=int, default=20_000, help="keyframes per robot")
    ap.add_argument("--verts-per-keyframe", type=int, default=52)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--ref-vertices", type=int, default=20_000)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mesh_deform.json"))
    a = ap.parse_args()

    import torch
    torch.cuda.set_device(0)
    torch.cuda.init()  # before the first kmx handle of the process
    from kmx.pgmo import MeshDeformer
    from kmx.pipeline import mesh_rmse
    from kmx.synth import make_pose_graph
    from kmx.synth.mesh import make_mesh
    from tests import mesh_ref as MR

    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else None

    t0 = time.perf_counter()
    n = a.robots * a.poses
    # the team's keyframes and odometry do not depend on the loop closures: none are generated
    g = make_pose_graph(a.robots, n, 0, seed=0)
    # the odometry chains from the true first poses, so the error before is the drift alone
    mesh = make_mesh(g, a.verts_per_keyframe, 3.0, 1, chain={r: (g.init_R[r], g.init_t[r]) for r in range(a.robots)})
    V = mesh.xyz.shape[0]
    gen = time.perf_counter() - t0
    W = int(round(a.window_s * 1e9))
    visits = candidate_visits(mesh, W)

    md = MeshDeformer(k=a.k, window_s=a.window_s, n_robots=a.robots)
    t0 = time.perf_counter()
    for r in range(a.robots):
        md.add_keyframes(r, mesh.kf_stamp[r], mesh.rest_R[r], mesh.rest_t[r])
        md.update_trajectory(r, g.gt_R[r], g.gt_t[r])
    md.add_vertices(mesh.robot, mesh.stamp, mesh.xyz)
    upload = time.perf_counter() - t0

    bind_ms = []
    for i in range(a.warmup + a.runs):
        md.rebind()
        bind_ms.append(md.timing()["bind_ms"])
    bind_ms = bind_ms[a.warmup:]
    info = md.info()

    out = torch.empty((V, 3), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    deform_ms = []
    for i in range(a.warmup + a.runs):
        md.deform(out=out)
        deform_ms.append(md.timing()["deform_ms"])
    deform_ms = deform_ms[a.warmup:]
    xyz, stats = md.deform()
    assert np.array_equal(out.cpu().numpy(), xyz)

    # one new trajectory: the rest poses again (the identity correction), then back
    t0 = time.perf_counter()
    for r in range(a.robots):
        md.update_trajectory(r, mesh.rest_R[r], mesh.rest_t[r])
    md.deform(out=out)
    md.sync()
    redeform = time.perf_counter() - t0
    redeform_dev = md.timing()["deform_ms"]
    identity_max_abs = float(np.abs(out.cpu().numpy() - mesh.xyz).max())

    # the reference on a subset, and the device against it
    m = min(a.ref_vertices, V)
    cat = np.concatenate
    node_robot = cat([np.full(a.poses, r, np.int32) for r in range(a.robots)])
    t0 = time.perf_counter()
    idx, w, cnt = MR.bind(node_robot, cat(mesh.kf_stamp), cat(mesh.rest_t), mesh.robot[:m], mesh.stamp[:m],
                          mesh.xyz[:m], a.k, W)
    t_ref_bind = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref, _ = MR.deform(mesh.xyz[:m], idx, w, cnt, cat(mesh.rest_R), cat(mesh.rest_t), cat(g.gt_R), cat(g.gt_t))
    t_ref_deform = time.perf_counter() - t0
    scale = max(np.abs(cat(mesh.rest_t)).max(), np.abs(cat(g.gt_t)).max(), float(np.abs(mesh.xyz).max()))
    err = np.abs(xyz[:m].astype(np.float64) - ref.astype(np.float64))
    ratio = float((err / MR.tolerance(ref, scale)).max())

    rest = {r: (mesh.rest_R[r], mesh.rest_t[r]) for r in range(a.robots)}
    gt = {r: (g.gt_R[r], g.gt_t[r]) for r in range(a.robots)}
    b, d = float(np.median(bind_ms)), float(np.median(deform_ms))
    bytes_per_vertex = 12 + 4 + 4 * a.k + 8 * a.k + 12
    res = {
        "what": "mesh deformation: bind and deform, device times (HIP events), MI355X",
        "commit": commit,
        "config": {"robots": a.robots, "keyframes": n, "vertices": V, "k": a.k, "window_s": a.window_s,
                   "warmup": a.warmup, "runs": a.runs, "generation_s": round(gen, 1), "upload_s": round(upload, 3),
                   "device_bytes": int(info["device_bytes"]), "lds_nodes": int(info["lds_nodes"]),
                   "bind_blocks": int(info["last_bind_blocks"]),
                   "bind_global_blocks": int(info["last_bind_global_blocks"])},
        "bind": {"median_ms": b, "min_ms": float(min(bind_ms)), "max_ms": float(max(bind_ms)),
                 "vertices_per_s": V / (b * 1e-3), "candidate_visits": visits,
                 "candidate_visits_per_s": visits / (b * 1e-3)},
        "deform": {"median_ms": d, "min_ms": float(min(deform_ms)), "max_ms": float(max(deform_ms)),
                   "vertices_per_s": V / (d * 1e-3), "bytes_per_vertex": bytes_per_vertex,
                   "bytes_per_s": bytes_per_vertex * V / (d * 1e-3),
                   "fraction_of_6.3TBps": bytes_per_vertex * V / (d * 1e-3) / HBM_BPS},
        "redeform_after_update_trajectory": {"host_s": redeform, "deform_device_ms": redeform_dev,
                                             "identity_correction_max_abs_m": identity_max_abs},
        "stats": stats,
        "rmse_before_m": mesh_rmse(g, mesh.xyz, mesh.gt_xyz, rest),
        "rmse_after_m": mesh_rmse(g, xyz, mesh.gt_xyz, gt),
        "numpy_reference": {"vertices": m, "bind_s": t_ref_bind, "deform_s": t_ref_deform,
                            "device_max_error_over_tolerance": ratio},
    }
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
