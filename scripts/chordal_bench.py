#!/usr/bin/env python
"""Measures the device chordal initialisation (kmx_chordal_*)
and writes profiles/chordal.json. Reports, gates nothing.

  (a) one robot, 20,000 poses / 100,000 edges: device vs the host's direct
      solve on the same box (the host run once), and check_every tried at
      several values;
  (b) the configs[4] base graph, outlier-free, as one team batch;
  (c) make_pose_graph(8, 100_000, 500_000) (and --million: 1M poses);
  (d) what it buys the optimiser: cost at round 0 and rounds to relChangeTol
      from the odometry start and from chordal_initialization_team, L2 on an
      outlier-free graph and GNC-TLS on the default 20 %-outlier graph.

Every solve is one warm-up and the median of 5: HIP events around the stages
(kmx_chordal_get_timing), the host clock around the whole call; set_graph (the
host's CSR build and the upload) is stated apart. --kernel-stats merges the
per-kernel totals of a `rocprofv3 --kernel-trace --stats` run of this script
(run with --only a --profile-run, so that it holds one graph and no skipped launch).
"""
from __future__ import annotations

import argparse
import csv
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "kimera-multi_amd"))
sys.path.insert(0, str(ROOT))

HBM_BYTES_PER_S = 8e12  # the figure the project quotes for MI355X


def team_arrays(g):
    n_poses = np.asarray(g.n_poses, np.int64)
    ptr = np.concatenate([[0], np.cumsum(n_poses)])
    own = np.nonzero(g.r1 == g.r2)[0]
    off = ptr[g.r1[own]]
    R0 = np.concatenate([np.einsum("ij,njk->nik", g.init_R[a][0].T, g.init_R[a]) for a in range(g.n_robots)])
    t0 = np.concatenate([(g.init_t[a] - g.init_t[a][0]) @ g.init_R[a][0] for a in range(g.n_robots)])
    return dict(n_poses=int(ptr[-1]), block_ptr=ptr, src=off + g.p1[own], dst=off + g.p2[own], R=g.R[own],
                t=g.t[own], kappa=g.kappa[own], tau=g.tau[own], weight=g.weight[own], anchors=ptr[:-1]), R0, t0


def apply_bytes(n, m, W):
    """Algorithmic bytes of one k_ch_apply launch: per record the other
    endpoint, the weight, the rotation (W = 3) and the gathered block; per pose
    the CSR pointer, D, the anchor flag, its own block and the output."""
    rec = 4 + 8 + (72 if W == 3 else 0) + 8 * 3 * W
    pose = 4 + 8 + 1 + 2 * 8 * 3 * W
    return 2 * m * rec + n * pose


def measure(graph_args, R0, t0, *, check_every=0, reps=5, label=""):
    from kmx.dpgo.chordal import ChordalSolver
    s = ChordalSolver()
    try:
        t = time.perf_counter()
        s.set_graph(**graph_args)
        t_graph = time.perf_counter() - t
        runs = []
        for k in range(reps + 1):
            t = time.perf_counter()
            R, tt, info = s.solve(R0, t0, check_every=check_every)
            wall = time.perf_counter() - t
            if k:  # the first is the warm-up
                runs.append(dict(s.timing(), solve_wall_ms=1e3 * wall))
    finally:
        s.close()
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    it_r = max(b["iterations_rot"] for b in info)
    it_t = max(b["iterations_trans"] for b in info)
    n, m = graph_args["n_poses"], int(np.asarray(graph_args["src"]).shape[0])
    out = {"poses": n, "edges": m, "blocks": len(info), "all_converged": all(b["converged"] for b in info),
           "iterations_rot": it_r, "iterations_trans": it_t,
           "iterations_rot_per_block": [b["iterations_rot"] for b in info],
           "set_graph_wall_ms": 1e3 * t_graph, **med,
           "us_per_iteration_rot": 1e3 * med["rotation_ms"] / max(it_r, 1),
           "us_per_iteration_trans": 1e3 * med["translation_ms"] / max(it_t, 1),
           "total_wall_ms_with_set_graph": 1e3 * t_graph + med["solve_wall_ms"],
           "apply_bytes_rot": apply_bytes(n, m, 3), "apply_bytes_trans": apply_bytes(n, m, 1)}
    print(label, json.dumps({k: v for k, v in out.items() if k != "iterations_rot_per_block"}), flush=True)
    return out, R, tt


def team_cost(g, traj, w=None):
    """0.5 sum w (kappa |R_j - R_i R_ij|_F^2 + tau |t_j - t_i - R_i t_ij|^2) over the team graph."""
    ptr = np.concatenate([[0], np.cumsum(np.asarray(g.n_poses, np.int64))])
    R = np.concatenate([traj[a][0] for a in range(g.n_robots)])
    t = np.concatenate([traj[a][1] for a in range(g.n_robots)])
    i, j = ptr[g.r1] + g.p1, ptr[g.r2] + g.p2
    w = g.weight if w is None else w
    dR = R[j] - R[i] @ g.R
    dt = t[j] - t[i] - np.einsum("eab,eb->ea", R[i], g.t)
    return float(0.5 * (w * (g.kappa * (dR ** 2).sum((1, 2)) + g.tau * (dt ** 2).sum(1))).sum())


def optimiser_gain(g, robust: bool, max_rounds: int):
    from kmx import pipeline as PL
    from kmx.dpgo.driver import RBCDDriver
    from kmx.dpgo.init import chordal_initialization_team
    from kmx.dpgo.params import PGOAgentParameters, RobustCostType
    from kmx.synth import lift, lifting_matrix
    P = PGOAgentParameters(r=5)
    if not robust:
        P.robustCostParams.costType = RobustCostType.L2
    P.maxNumIters = max_rounds
    Y = lifting_matrix(P.r, seed=1)
    out = {}
    for name in ("odometry", "chordal_gpu"):
        t = time.perf_counter()
        if name == "odometry":
            own = PL.odometry_init(g)
        else:
            Rl, tl = chordal_initialization_team(g)
            own = {a: (Rl[a], tl[a]) for a in range(g.n_robots)}
        t_local = time.perf_counter() - t
        traj0, _ = PL.global_init(g, own)
        drv = RBCDDriver(P, g)
        drv.initialize({a: lift(traj0[a][0], traj0[a][1], Y) for a in drv.robots})
        rounds = drv.run(max_rounds=max_rounds, check_every=10)
        final = {a: PL.rounded(drv.iterate_of(a), Y) for a in drv.robots}
        out[name] = {"local_init_s": t_local, "cost_round_0": team_cost(g, traj0), "ate_round_0_m": PL.ate_rmse(g, traj0),
                     "rounds_to_stop": rounds, "hit_round_limit": rounds >= max_rounds,
                     "cost_final_weight_1": team_cost(g, final), "ate_final_m": PL.ate_rmse(g, final)}
        drv.solver.close()
        print("(d)", "robust" if robust else "L2", name, json.dumps(out[name]), flush=True)
    return out


def robust_device(s, fixed, R0, t0, **kw):
    t = time.perf_counter()
    R, tt, g, info, rinfo = s.solve_robust(fixed, R0, t0, **kw)
    wall = time.perf_counter() - t
    st = s.robust_stats()
    return dict(st, wall_ms=1e3 * wall, updates=max(r["updates"] for r in rinfo),
                updates_per_block=[r["updates"] for r in rinfo], all_converged=all(r["converged"] for r in rinfo),
                kept=sum(r["n_kept"] for r in rinfo), rejected=sum(r["n_rejected"] for r in rinfo)), g


def robust_host_driven(s, args, fixed, R0, t0, *, barc=5.0, mu_step=1.4, max_updates=100):
    """The same loop through the entry points the library had before
    kmx_chordal_solve_robust: solve, the residuals and weights in numpy,
    set_weights (which runs the host's connectivity check and uploads), solve
    again from the last poses. Per block mu and stop test as on the device; a
    block that is done keeps its g, but its CGs start again in every solve
    (the API cannot freeze it)."""
    from kmx.dpgo.init import gnc_tls_factor, measurement_errors
    src, dst, w0 = np.asarray(args["src"]), np.asarray(args["dst"]), np.asarray(args["weight"], np.float64)
    ptr = np.asarray(args["block_ptr"])
    nb = ptr.shape[0] - 1
    blk = np.searchsorted(ptr, src, side="right") - 1
    counted = ~fixed & (w0 > 0)
    c2 = barc * barc
    t_start = time.perf_counter()
    s.set_weights(w0)
    R, t, _ = s.solve(R0, t0)
    r2 = measurement_errors(src, dst, args["R"], args["t"], args["kappa"], args["tau"], R, t)
    mx = np.zeros(nb)
    np.maximum.at(mx, blk[counted], r2[counted])
    done = 2.0 * mx <= c2
    mu = np.where(done, 1.0, c2 / np.where(done, 1.0, 2.0 * mx - c2))
    g = np.ones(src.shape[0])
    updates = np.zeros(nb, np.int64)
    solves = 1
    while not done.all() and solves <= max_updates:
        g_new = g.copy()
        stop = np.zeros(nb, bool)
        for b in np.nonzero(~done)[0]:
            sel = (blk == b) & ~fixed
            gb, frac = gnc_tls_factor(r2[sel], mu[b], c2)
            stop[b] = not frac[counted[sel]].any() and np.array_equal(gb[counted[sel]], g[sel][counted[sel]])
            g_new[sel] = gb
        g = g_new
        done |= stop
        if done.all():
            break
        s.set_weights(w0 * g)
        R, t, _ = s.solve(R, t)
        solves += 1
        updates[~done] += 1
        r2 = measurement_errors(src, dst, args["R"], args["t"], args["kappa"], args["tau"], R, t)
        mu[~done] *= mu_step
    wall = time.perf_counter() - t_start
    s.set_weights(w0)
    return {"wall_ms": 1e3 * wall, "updates": int(updates.max()), "solves": solves}, g


def robust_part(g, label, reps=5, host_reps=5):
    """(R1) / (R2): solve_robust with both warm starts and the host-driven loop, alternating, one warm-up each."""
    from kmx.dpgo.chordal import ChordalSolver
    args, R0, t0 = team_arrays(g)
    own = np.nonzero(g.r1 == g.r2)[0]
    fixed = np.asarray(g.fixed)[own] != 0
    outl = np.asarray(g.outlier)[own]
    s = ChordalSolver()
    runs = {"unprojected": [], "projected": [], "host_driven": []}
    try:
        s.set_graph(**args)
        for k in range(max(reps, host_reps) + 1):
            for name in runs:
                if name == "host_driven":
                    if k > host_reps:
                        continue
                    r, gg = robust_host_driven(s, args, fixed, R0, t0)
                else:
                    if k > reps:
                        continue
                    r, gg = robust_device(s, fixed, R0, t0, start_projected=name == "projected")
                r["outliers_kept"] = int((gg[outl] > 0).sum())
                r["inliers_dropped"] = int((gg[~outl & ~fixed] == 0).sum())
                if k:  # the first is the warm-up
                    runs[name].append(r)
    finally:
        s.close()
    out = {"poses": args["n_poses"], "edges": int(own.shape[0]), "outliers": int(outl.sum()),
           "loop_closures": int((~fixed).sum())}
    for name, rr in runs.items():
        med = {k: statistics.median(r[k] for r in rr) for k in rr[0] if not isinstance(rr[0][k], (list, bool))}
        med.update({k: rr[0][k] for k in rr[0] if isinstance(rr[0][k], (list, bool))})
        if "gnc_passes" in med:
            med["gnc_pass_and_decision_us"] = 1e3 * med["gnc_ms"] / max(med["gnc_passes"], 1)
        out[name] = med
    out["host_driven_over_device"] = out["host_driven"]["wall_ms"] / out["unprojected"]["wall_ms"]
    print(label, json.dumps(out), flush=True)
    return out


def robust_optimiser_row(g, max_rounds):
    """§14's table, the third GNC-TLS row: start robust_chordal_initialization_team."""
    from kmx import pipeline as PL
    from kmx.dpgo.driver import RBCDDriver
    from kmx.dpgo.init import robust_chordal_initialization_team
    from kmx.dpgo.params import PGOAgentParameters
    from kmx.synth import lift, lifting_matrix
    P = PGOAgentParameters(r=5)
    P.maxNumIters = max_rounds
    Y = lifting_matrix(P.r, seed=1)
    t = time.perf_counter()
    Rl, tl, gl, _, rinfo = robust_chordal_initialization_team(g, return_info=True)
    t_local = time.perf_counter() - t
    own = {a: (Rl[a], tl[a]) for a in range(g.n_robots)}
    traj0, _ = PL.global_init(g, own)
    drv = RBCDDriver(P, g)
    drv.initialize({a: lift(traj0[a][0], traj0[a][1], Y) for a in drv.robots})
    rounds = drv.run(max_rounds=max_rounds, check_every=10)
    final = {a: PL.rounded(drv.iterate_of(a), Y) for a in drv.robots}
    out = {"local_init_s": t_local, "updates_per_robot": [r["updates"] for r in rinfo],
           "cost_round_0": team_cost(g, traj0), "ate_round_0_m": PL.ate_rmse(g, traj0), "rounds_to_stop": rounds,
           "hit_round_limit": rounds >= max_rounds, "cost_final_weight_1": team_cost(g, final),
           "ate_final_m": PL.ate_rmse(g, final)}
    drv.solver.close()
    print("(d) robust robust_chordal_gpu", json.dumps(out), flush=True)
    return out


def kernel_stats(path):
    """Per-kernel totals of the k_ch_* kernels from a rocprofv3 kernel-stats CSV."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            if "k_ch_" not in name:
                continue
            key = name[name.index("k_ch_"):].split("(")[0]
            out[key] = {"calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) / 1e6,
                        "average_us": float(row["AverageNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="abcd", help="which parts to run (letters of a, b, c, d)")
    ap.add_argument("--no-host", action="store_true", help="skip the host reference of (a)")
    ap.add_argument("--million", action="store_true", help="(c) also on 1M poses")
    ap.add_argument("--profile-run", action="store_true", help="one warm-up and one solve of (a) only (under rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel-stats CSV of a --profile-run to merge")
    ap.add_argument("--max-rounds", type=int, default=1500)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "chordal.json"))
    ap.add_argument("--robust", default=None, metavar="PARTS",
                    help="measure kmx_chordal_solve_robust instead (letters of 1: (R1), 2: (R2), d: the optimiser row) "
                         "and write profiles/chordal_robust.json")
    a = ap.parse_args()
    from kmx.dpgo.init import chordal_initialization
    from kmx.synth import make_pose_graph
    if a.robust is not None and a.out == str(ROOT / "profiles" / "chordal.json"):
        a.out = str(ROOT / "profiles" / "chordal_robust.json")
    outp = Path(a.out)
    res = json.loads(outp.read_text()) if outp.exists() else {}  # parts run apart are merged

    def save():
        outp.parent.mkdir(parents=True, exist_ok=True)
        outp.write_text(json.dumps(res, indent=1) + "\n")

    if a.robust is not None:
        if "1" in a.robust:
            res["R1_20k_one_robot_20pct_outliers"] = robust_part(
                make_pose_graph(1, 20000, 100000, outlier_frac=0.2, f_inter=0, seed=1), "(R1)")
            save()
        if "2" in a.robust:
            res["R2_configs4_team_with_outliers"] = robust_part(
                make_pose_graph(8, 160_000, 800_000, f_inter=0, seed=0), "(R2)")
            save()
        if "d" in a.robust:
            res["d_optimiser_gnc_tls_20pct_outliers_robust_chordal"] = robust_optimiser_row(
                make_pose_graph(6, 6000, 30000), a.max_rounds)
            save()
        return

    if a.kernel_stats:
        ks = kernel_stats(a.kernel_stats)
        res["a_kernel_split"] = {"kernels": ks, "note": "rocprofv3 --kernel-trace --stats of one warm-up and one solve of (a) "
                                                        "with check_every = 1 (every launch a full one)"}
        ga = res.get("a_20k_one_robot", {}).get("gpu")
        for W, name in ((3, "k_ch_apply<3, false>"), (1, "k_ch_apply<1, false>")):
            if ga and name in ks:
                b = ga["apply_bytes_rot" if W == 3 else "apply_bytes_trans"]
                rate = b / (ks[name]["average_us"] * 1e-6)
                res["a_kernel_split"][f"apply_W{W}_bytes_per_s"] = rate
                res["a_kernel_split"][f"apply_W{W}_fraction_of_8TBps"] = rate / HBM_BYTES_PER_S
        save()
        return
    if "a" in a.only:
        g = make_pose_graph(1, 20000, 100000, outlier_frac=0, f_inter=0, seed=1)
        args, R0, t0 = team_arrays(g)
        if a.profile_run:
            # check_every = 1: no launch is enqueued past convergence, so every traced launch is a full one
            measure(args, R0, t0, check_every=1, reps=1, label="(a, profiled)")
            return
        part = {}
        part["gpu"], R, t = measure(args, R0, t0, label="(a)")
        part["check_every"] = {}
        for ce in (10, 50, 200):
            m, _, _ = measure(args, R0, t0, check_every=ce, label=f"(a) check_every={ce}")
            part["check_every"][str(ce)] = {k: m[k] for k in ("solve_wall_ms", "rotation_ms", "translation_ms")}
        if not a.no_host:
            edges = [(int(i), int(j), g.R[e], g.t[e], float(g.kappa[e]), float(g.tau[e]), float(g.weight[e]))
                     for e, (i, j) in enumerate(zip(g.p1, g.p2))]
            tt = time.perf_counter()
            Rr, tr = chordal_initialization(20000, edges)
            part["host_reference_s"] = time.perf_counter() - tt
            part["max_abs_dR_vs_host"] = float(np.abs(R - Rr).max())
            part["max_abs_dt_vs_host_m"] = float(np.abs(t - tr).max())
            print("(a) host", part["host_reference_s"], part["max_abs_dR_vs_host"], part["max_abs_dt_vs_host_m"],
                  flush=True)
        res["a_20k_one_robot"] = part
        save()
    if "b" in a.only:
        g = make_pose_graph(8, 160_000, 800_000, outlier_frac=0, f_inter=0, seed=0)
        args, R0, t0 = team_arrays(g)
        res["b_configs4_team"], _, _ = measure(args, R0, t0, label="(b)")
        save()
    if "c" in a.only:
        sizes = [(100_000, 500_000)] + ([(1_000_000, 5_000_000)] if a.million else [])
        for (n, m) in sizes:
            g = make_pose_graph(8, n, m, outlier_frac=0, f_inter=0)
            args, R0, t0 = team_arrays(g)
            res[f"c_{n}_poses_team"], _, _ = measure(args, R0, t0, label=f"(c) {n}")
            save()
    if "d" in a.only:
        res["d_optimiser_L2_outlier_free"] = optimiser_gain(make_pose_graph(6, 6000, 30000, outlier_frac=0), False,
                                                            a.max_rounds)
        save()
        res["d_optimiser_gnc_tls_20pct_outliers"] = optimiser_gain(make_pose_graph(6, 6000, 30000), True, a.max_rounds)
        save()


if __name__ == "__main__":
    main()
