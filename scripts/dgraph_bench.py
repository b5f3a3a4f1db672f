"""Times of the deformation graph's optimisation (kmx_dgraph_*, dgraph.hip).

Shape: the keyframes of the configs[4] team (8 robots x 20,000 poses; the
generator's odometry chains are the rest poses, its ground truth stands in as
the optimised trajectory) and `--verts-per-keyframe` mesh vertices per
keyframe (kmx.synth.mesh.make_mesh), simplified on a voxel grid of
`--resolution` metres (kmx.pgmo.simplify_voxel); the graph is
kmx.pgmo.graph_from_mesh's (mesh edges and keyframe links, both directions,
weight 1) with soft priors on the keyframes, started as kmx.pipeline's graph
stage starts it. The resolution and the counts are written to the result.

The handle brackets its kernels with HIP events, so the figures are device
times, uploads excluded: warm-up runs, then the median of the timed runs.

* one k_dg_apply (the matrix-free product behind eval('jtj')), with its bytes
  by the layout: per record `other` 4, w 8, a 24, and the other node's v, 48
  (from the caches: 6 n doubles in all), per node v 48 in, q 48 out, mode 1,
  ptr 4; that over the time as a fraction of 6.3 TB/s, the achievable HBM
  rate. A ceiling, not a pass mark.
* one outer iteration (max_iterations = 1) from the start, and its parts.
* the whole solve at the default parameters from the start.
* vertex RMSE against the ground truth through the graph's nodes, next to the
  keyframe-only deformation (kmx.pipeline.deform_mesh).
* the numpy / scipy reference (tests/dgraph_ref.py) on the same shape at 1/100
  of the keyframes, host clock, for scale.

Nothing is thresholded.

  python scripts/dgraph_bench.py [--verts-per-keyframe 6] [--resolution 0.5] [--horizon-s S] [--out profiles/dgraph.json]
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


def build(robots, poses, vpk, resolution, kappa, tau, horizon_s=None):
    from kmx.pgmo import graph_from_mesh, simplify_voxel
    from kmx.synth import make_pose_graph
    from kmx.synth.mesh import make_mesh
    g = make_pose_graph(robots, robots * poses, 0, seed=0)
    rest = {r: (g.init_R[r], g.init_t[r]) for r in range(robots)}
    cur = {r: (g.gt_R[r], g.gt_t[r]) for r in range(robots)}
    mesh = make_mesh(g, vpk, 3.0, 1, chain=rest)
    cx, cs, cr, cf, _ = simplify_voxel(mesh.xyz, mesh.faces, mesh.stamp, mesh.robot, resolution, horizon_s=horizon_s)
    G = graph_from_mesh(cx, cs, cr, cf, mesh.kf_stamp, [rest[r] for r in range(robots)])
    nk, n = G["n_keyframes"], G["g"].shape[0]
    mode = np.zeros(n, np.uint8)
    mode[:nk] = 1
    R_hat, t_hat = G["R_rest"].copy(), G["g"].copy()
    R_hat[:nk] = np.concatenate([cur[r][0] for r in range(robots)])
    t_hat[:nk] = np.concatenate([cur[r][1] for r in range(robots)])
    C = R_hat[:nk] @ G["R_rest"][:nk].transpose(0, 2, 1)
    lk = G["link"]
    R0, t0 = R_hat.copy(), t_hat.copy()
    R0[nk:] = C[lk]
    t0[nk:] = np.einsum("nij,nj->ni", C[lk], G["g"][nk:] - G["g"][lk]) + t_hat[lk]
    return dict(g=g, mesh=mesh, rest=rest, cur=cur, G=G, mode=mode, R_hat=R_hat, t_hat=t_hat, R0=R0, t0=t0,
                kappa=kappa, tau=tau, n=n, nk=nk)


def med(x):
    return float(np.median(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=8)
    ap.add_argument("--poses", type=int, default=20_000, help="keyframes per robot")
    ap.add_argument("--verts-per-keyframe", type=int, default=6)
    ap.add_argument("--resolution", type=float, default=0.5)
    ap.add_argument("--horizon-s", type=float, default=None,
                    help="simplify_voxel's horizon_s: merge only vertices seen in one window of this length")
    ap.add_argument("--kappa", type=float, default=100.0)
    ap.add_argument("--tau", type=float, default=100.0)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dgraph.json"))
    a = ap.parse_args()

    from kmx.pgmo import DeformationGraph
    from kmx.pipeline import deform_mesh, mesh_rmse
    from tests import dgraph_ref as DR

    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else None

    t0 = time.perf_counter()
    B = build(a.robots, a.poses, a.verts_per_keyframe, a.resolution, a.kappa, a.tau, a.horizon_s)
    G, n, nk = B["G"], B["n"], B["nk"]
    m = int(G["src"].shape[0])
    prep = time.perf_counter() - t0
    print(f"graph: {n} nodes ({nk} keyframes, {n - nk} control vertices of {B['mesh'].xyz.shape[0]} vertices), "
          f"{m} directed edges, host preparation {prep:.1f} s", flush=True)

    dg = DeformationGraph()
    t0 = time.perf_counter()
    dg.set_graph(G["R_rest"], G["g"], G["src"], G["dst"], G["w"], robot=G["robot"], stamp=G["stamp"])
    dg.set_priors(B["mode"], B["R_hat"], B["t_hat"], a.kappa, a.tau)
    upload = time.perf_counter() - t0

    # one product
    rng = np.random.Generator(np.random.PCG64(0))
    v = rng.standard_normal((n, 6))
    dg.set_poses(B["R0"], B["t0"])
    apply_ms = []
    for _ in range(a.warmup + a.runs):
        dg.eval("jtj", v)
        apply_ms.append(dg.timing()["apply_ms"])
    apply_ms = apply_ms[a.warmup:]
    rec = 2 * m
    apply_bytes = rec * (4 + 8 + 24 + 48) + n * (48 + 48 + 1 + 4)
    stream_bytes = rec * (4 + 8 + 24) + n * (48 + 48 + 48 + 1 + 4)  # the gathered v counted once per node

    # one outer iteration
    one = {"total_ms": [], "linearize_ms": [], "cg_ms": [], "trial_ms": []}
    cg1 = 0
    for _ in range(a.warmup + a.runs):
        dg.set_poses(B["R0"], B["t0"])
        r1 = dg.solve(max_iterations=1)
        cg1 = r1["cg_iterations"]
        tm = dg.timing()
        for k in one:
            one[k].append(tm[k])
    one = {k: med(x[a.warmup:]) for k, x in one.items()}

    # the whole solve
    dg.set_poses(B["R0"], B["t0"])
    t0 = time.perf_counter()
    res = dg.solve()
    first_wall = time.perf_counter() - t0
    runs = a.runs if first_wall < 1.5 else 5
    solve_ms, wall_ms = [], []
    for _ in range(a.warmup + runs):
        dg.set_poses(B["R0"], B["t0"])
        t0 = time.perf_counter()
        res = dg.solve()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        solve_ms.append(dg.timing()["total_ms"])
    parts = dg.timing()
    log = dg.log()

    # the mesh through the graph, and through the keyframes alone
    mesh, g = B["mesh"], B["g"]
    md = dg.deformer(a.k, a.window_s, n_robots=a.robots)
    dg.push(md)
    md.add_vertices(mesh.robot, mesh.stamp, mesh.xyz)
    xyz, st = md.deform()
    md.close()
    dg.close()
    rmse_graph = mesh_rmse(g, xyz, mesh.gt_xyz, B["cur"])
    kf_only = deform_mesh(g, mesh, B["rest"], B["cur"], k=a.k, window_s=a.window_s)

    # the reference at 1/100 of the keyframes
    S = build(a.robots, max(a.poses // 100, 2), a.verts_per_keyframe, a.resolution, a.kappa, a.tau, a.horizon_s)
    P = DR.make_problem(S["G"]["R_rest"], S["G"]["g"], S["G"]["src"], S["G"]["dst"], S["G"]["w"], S["mode"], S["R_hat"],
                        S["t_hat"], a.kappa, a.tau)
    t0 = time.perf_counter()
    ref = DR.solve(P, S["R0"], S["t0"])
    ref_s = time.perf_counter() - t0
    sd = DeformationGraph()
    sd.set_graph(P.R_rest, P.g, P.src, P.dst, P.w)
    sd.set_priors(P.mode, P.R_hat, P.t_hat, P.kappa, P.tau)
    sd.set_poses(S["R0"], S["t0"])
    sres = sd.solve()
    small_ms = sd.timing()["total_ms"]
    Rs, ts = sd.poses()
    sd.close()

    out = {
        "commit": commit, "device": "MI355X", "robots": a.robots, "keyframes": nk,
        "verts_per_keyframe": a.verts_per_keyframe, "vertices": int(mesh.xyz.shape[0]), "resolution_m": a.resolution,
        "horizon_s": a.horizon_s,
        "nodes": n, "control_vertices": n - nk, "directed_edges": m, "records": rec, "tiles": (n + 63) // 64,
        "prior_kappa": a.kappa, "prior_tau": a.tau, "host_prepare_s": prep, "upload_s": upload,
        "warmup": a.warmup, "runs": a.runs,
        "apply": {"ms_median": med(apply_ms), "ms_min": float(min(apply_ms)), "bytes_by_layout": apply_bytes,
                  "bytes_streamed_once": stream_bytes,
                  "fraction_of_6p3_TBps": apply_bytes / (med(apply_ms) * 1e-3) / HBM_BPS,
                  "fraction_of_6p3_TBps_streamed_once": stream_bytes / (med(apply_ms) * 1e-3) / HBM_BPS},
        "one_outer_iteration": dict(one, cg_iterations=cg1),
        "solve": {"ms_median": med(solve_ms[a.warmup:]), "wall_ms_median": med(wall_ms[a.warmup:]), "runs": runs,
                  "iterations": res["iterations"], "accepted": res["accepted"], "stop": res["stop"],
                  "cg_iterations": res["cg_iterations"], "cost_initial": res["cost_initial"],
                  "cost_final": res["cost_final"], "linearize_ms": parts["linearize_ms"], "cg_ms": parts["cg_ms"],
                  "trial_ms": parts["trial_ms"],
                  "log": [[e["cost"], e["trial_cost"], e["lam"], e["cg_iterations"], int(e["accepted"])] for e in log]},
        "mesh": {"rmse_before_m": kf_only["rmse_before_m"], "rmse_keyframes_only_m": kf_only["rmse_after_m"],
                 "rmse_graph_m": rmse_graph, "unbound": int(st["unbound"])},
        "reference_1_100": {"nodes": P.n, "directed_edges": P.m, "numpy_scipy_solve_s": ref_s,
                            "iterations": ref["iterations"], "cg_iterations": ref["cg_iterations"],
                            "device_solve_ms": small_ms, "device_iterations": sres["iterations"],
                            "max_pose_difference": float(max(np.abs(Rs - ref["R"]).max(), np.abs(ts - ref["t"]).max()))},
    }
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({k: v for k, v in out.items() if k != "solve"}, indent=1))
    print(json.dumps({k: v for k, v in out["solve"].items() if k != "log"}))


if __name__ == "__main__":
    main()
