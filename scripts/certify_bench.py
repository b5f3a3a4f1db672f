#!/usr/bin/env python
"""Measures the dual certificate (kmx_cert_*) and writes
profiles/certify.json. Reports, gates nothing.

configs[1] (campus6) and configs[3] (synth100k) are solved with bench.py's own
parameters (GNC on) for --rounds RBCD rounds from the odometry start, then
certify_team runs on the final iterate and the final weights: decision, steps,
device ms per Lanczos step (HIP events around the launches only), the host's
decision time apart, and the algorithmic bytes of one S v over the device step
time as a fraction of 8 TB/s. At configs[1] only, scipy.sparse.linalg.eigsh(S, which="SA")
on the same S is timed on the host as the CPU figure.
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "kimera-multi_amd"))
sys.path.insert(0, str(ROOT))

HBM_BYTES_PER_S = 8e12  # the figure the project quotes for MI355X


def apply_bytes(n, m):
    """Algorithmic bytes of one k_ct_apply launch: per incidence its 128-byte
    record and the other endpoint's 32-byte row; per pose the CSR pointer,
    D - Lambda (80), its own row, the previous vector's row and the output."""
    return 2 * m * (128 + 32) + n * (4 + 80 + 3 * 32)


def sparse_S(n, src, dst, R, t, kappa, tau, w, X):
    """S = Q - Lambda as a scipy CSR matrix (the host's restatement, vectorised)."""
    import scipy.sparse as sp
    m = src.shape[0]
    A = np.zeros((m, 4, 4))
    A[:, :3, :3] = kappa[:, None, None] * np.eye(3) + tau[:, None, None] * t[:, :, None] * t[:, None, :]
    A[:, :3, 3] = A[:, 3, :3] = tau[:, None] * t
    A[:, 3, 3] = tau
    B = np.zeros((m, 4, 4))
    B[:, 0, 0] = B[:, 1, 1] = B[:, 2, 2] = kappa
    B[:, 3, 3] = tau
    Cm = np.zeros((m, 4, 4))
    Cm[:, :3, :3] = kappa[:, None, None] * R
    Cm[:, :3, 3] = tau[:, None] * t
    Cm[:, 3, 3] = tau
    a4 = np.arange(4)

    def blocks(bi, bj, V):
        rows = (4 * bi[:, None, None] + a4[None, :, None]) + 0 * a4[None, None, :]
        cols = (4 * bj[:, None, None] + a4[None, None, :]) + 0 * a4[None, :, None]
        return rows.ravel(), cols.ravel(), V.ravel()

    parts = [blocks(src, src, w[:, None, None] * A), blocks(dst, dst, w[:, None, None] * B),
             blocks(src, dst, -w[:, None, None] * Cm), blocks(dst, src, -w[:, None, None] * Cm.transpose(0, 2, 1))]
    Q = sp.coo_matrix((np.concatenate([p[2] for p in parts]),
                       (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))),
                      shape=(4 * n, 4 * n)).tocsr()
    r = X.shape[1]
    Xf = np.ascontiguousarray(X.transpose(1, 0, 2).reshape(r, 4 * n))
    G = (Q @ Xf.T).T.reshape(r, n, 4).transpose(1, 0, 2)
    M = np.einsum("nac,nad->ncd", X[:, :, :3], G[:, :, :3])
    L = np.zeros((n, 4, 4))
    L[:, :3, :3] = 0.5 * (M + M.transpose(0, 2, 1))
    p = np.arange(n)
    lr, lc, lv = blocks(p, p, L)
    return (Q - sp.coo_matrix((lv, (lr, lc)), shape=(4 * n, 4 * n)).tocsr()).tocsr()


def run(name, rounds, eta, max_steps, with_eigsh):
    import bench
    from kmx.dpgo.certify import certify_team, flatten_team
    from kmx.dpgo.driver import RBCDDriver
    from kmx.synth import config, lift, lifting_matrix
    g = config(name, seed=0)
    P = bench.params()
    Y = lifting_matrix(P.r, seed=1)
    drv = RBCDDriver(P, g)
    drv.initialize({a: lift(g.init_R[a], g.init_t[a], Y) for a in drv.robots})
    t0 = time.perf_counter()
    drv.run_async(rounds)
    drv.solver.sync()
    t_solve = time.perf_counter() - t0
    Xs = {a: drv.iterate_of(a) for a in range(g.n_robots)}
    w = drv.solver.get_weights()
    drv.solver.close()
    n = int(np.sum(g.n_poses))
    certify_team(g, Xs, w, eta=eta, max_steps=20)  # warm-up: the kernels' first launch
    t0 = time.perf_counter()
    cert = certify_team(g, Xs, w, eta=eta, max_steps=max_steps)
    wall = time.perf_counter() - t0
    ms_step = cert["timing"]["lanczos_ms"] / max(cert["steps"], 1)
    nbytes = apply_bytes(n, int(g.m))
    out = {"config": name, "poses": n, "edges": int(g.m), "r": P.r, "rounds": rounds, "solve_seconds": t_solve,
           "eta": eta, "max_steps": max_steps, "decision": cert["decision"], "steps": cert["steps"],
           "theta_min": cert["theta_min"], "theta_max": cert["theta_max"], "rho": cert["residual"],
           "cost": cert["cost"], "stationarity": cert["stationarity"], "timing_ms": cert["timing"],
           "certify_wall_ms": 1e3 * wall,
           # lanczos_ms is the device's: an event pair around every batch's launches, summed; the host's
           # decisions between the batches (timing_ms.host_rule_ms) and the read-backs are not in it
           "device_ms_per_step": ms_step, "host_rule_ms_per_test": cert["timing"]["host_rule_ms"] /
           max(cert["steps"] // 10, 1), "apply_bytes": nbytes,
           # a step is one S v and the vector update with two one-wave reductions; the bytes are S v's alone
           "apply_bytes_over_device_step_time_fraction_of_8TBps": nbytes / (1e-3 * ms_step) / HBM_BYTES_PER_S}
    if with_eigsh:
        import scipy.sparse.linalg as spla
        _, src, dst, X = flatten_team(g, Xs)
        S = sparse_S(n, src, dst, g.R, g.t, g.kappa, g.tau, np.asarray(w, float), X)
        t0 = time.perf_counter()
        try:
            ev = spla.eigsh(S, k=1, which="SA", return_eigenvectors=False, tol=1e-9, maxiter=20_000)
            out["cpu_eigsh_SA_lambda_min"] = float(ev[0])
        except spla.ArpackNoConvergence as ex:  # the time is still the CPU figure; say that it did not converge
            out["cpu_eigsh_SA_lambda_min"] = None
            out["cpu_eigsh_SA_note"] = f"no convergence in 20000 restarts: {ex}"
        out["cpu_eigsh_SA_seconds"] = time.perf_counter() - t0
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=300, help="RBCD rounds before the certificate")
    ap.add_argument("--eta", type=float, default=1e-5)
    ap.add_argument("--max-steps", type=int, default=5000)
    ap.add_argument("--only", choices=("campus6", "synth100k"), default=None)
    ap.add_argument("--no-eigsh", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "certify.json"))
    a = ap.parse_args()
    try:
        commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    res = {"commit": commit, "note": "reports, thresholds nothing; decision UNDECIDED means max_steps was reached "
                                     "with the theta_min and rho stated", "runs": []}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    for name in ("synth100k", "campus6"):  # the host's eigsh comes last; the file is written after every run
        if a.only in (None, name):
            res["runs"].append(run(name, a.rounds, a.eta, a.max_steps, name == "campus6" and not a.no_eigsh))
            Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
