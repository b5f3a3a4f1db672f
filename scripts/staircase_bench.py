#!/usr/bin/env python
"""Measures the Riemannian staircase (kmx.dpgo.staircase, kmx_cert_escape;
DESIGN.md §17) and writes profiles/staircase.json. Reports, gates nothing.

The winding ring (tests/cert_ref.py's: identity measurements, exactly
stationary at rank 3, lambda_min(S) = -(2 - 2 cos(2 pi / n))) at n = 100 and
10 000 poses, one robot, from r = 3 with eta = min(1e-5, |lambda_min| / 100).
Per level:
the solver's rounds and host time, the Lanczos steps and their device time
(HIP events), and kmx_cert_escape's device time for the 8 candidates of the
default ladder (HIP events around its three launches; its transfers apart).
The same eight costs by the route the library had before kmx_cert_escape --
numpy escape_point on the host and eight kmx_cert_set_point uploads -- are
timed in the same run on the host clock and compared.
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


def ring_graph(n):
    """The winding ring of n poses as a one-robot PoseGraphData and its
    stationary point at rank 3 (Y_i = Rz(2 pi i / n), p_i = 0)."""
    from kmx.synth.pose_graph import PoseGraphData
    src = np.arange(n, dtype=np.int32)
    dst = ((src + 1) % n).astype(np.int32)
    zero = np.zeros(n, np.int32)
    eye, z3 = [np.tile(np.eye(3), (n, 1, 1))], [np.zeros((n, 3))]
    g = PoseGraphData(n_robots=1, n_poses=np.array([n], np.int32), r1=zero, p1=src, r2=zero, p2=dst,
                      R=np.tile(np.eye(3), (n, 1, 1)), t=np.zeros((n, 3)), kappa=np.ones(n), tau=np.ones(n),
                      weight=np.ones(n), fixed=(dst == src + 1).astype(np.uint8), outlier=np.zeros(n, bool),
                      gt_R=eye, gt_t=z3, init_R=eye, init_t=z3)
    X = np.zeros((n, 3, 4))
    a = 2.0 * np.pi * np.arange(n) / n
    X[:, 0, 0], X[:, 0, 1] = np.cos(a), -np.sin(a)
    X[:, 1, 0], X[:, 1, 1] = np.sin(a), np.cos(a)
    X[:, 2, 2] = 1.0
    return g, {0: X}


def run(n, max_rounds, max_steps, device):
    from kmx.dpgo.certify import Certifier, escape_point
    from kmx.dpgo.params import PGOAgentParameters
    from kmx.dpgo.staircase import staircase_team

    extra = []  # per level: the device's times, and the host route to the same costs

    class Timed(Certifier):
        def set_point(self, X):
            self._X = np.array(X, np.float64)
            return super().set_point(X)

        def min_eig(self, eta, **kw):
            res = super().min_eig(eta, **kw)
            t = self.timing()
            extra.append({"lanczos_device_ms": t["lanczos_ms"], "vector_device_ms": t["vector_ms"],
                          "min_eig_host_wall_ms": t["host_wall_ms"]})
            return res

        def escape(self, y, alphas):
            X = self._X
            t0 = time.perf_counter()
            cands = [escape_point(X, y, a) for a in alphas]
            t1 = time.perf_counter()
            ref = [Certifier.set_point(self, Z)["cost"] for Z in cands]
            t2 = time.perf_counter()
            Certifier.set_point(self, X)  # the point the escape starts from
            super().escape(y, alphas)  # warm-up: the kernels' first launch at this rank
            t3 = time.perf_counter()
            out = super().escape(y, alphas)
            t4 = time.perf_counter()
            extra[-1].update(self.escape_timing())
            extra[-1].update(escape_host_wall_ms=1e3 * (t4 - t3), numpy_escape_point_ms=1e3 * (t1 - t0),
                             eight_set_point_ms=1e3 * (t2 - t1), host_route_ms=1e3 * (t2 - t0),
                             max_cost_difference_to_host_route=float(np.abs(np.array(ref) - out["cost"]).max()))
            return out

    g, Xs = ring_graph(n)
    lam = 2.0 - 2.0 * np.cos(2.0 * np.pi / n)
    P = PGOAgentParameters(r=3)
    P.localOptimizationParams.RTR_iterations = 8  # rejected steps quarter the radius from 100 in every update
    P.localOptimizationParams.RTR_tCG_iterations = 50
    c = Timed(device)
    t0 = time.perf_counter()
    # eta well below the gap: at eta = |lambda_min| / 4 the 100-pose ring was CERTIFIED at rank 4 with
    # theta_min = -8e-6 and rho = 9e-4 (lambda_min is -3.9e-3 there): the rule's residual bound says an
    # eigenvalue lies within rho of theta_min, not that it is the smallest
    eta = min(1e-5, 0.01 * lam)
    out = staircase_team(g, Xs, None, P, eta=eta, r_max=6, grad_tol=1e-7, stat_tol=1e-5,
                         max_rounds=max_rounds, certifier=c, max_steps=max_steps)
    wall = time.perf_counter() - t0
    c.close()
    levels = []
    for lv, ex in zip(out["levels"], extra):
        q = {k: lv[k] for k in ("r", "rounds", "block_steps", "solve_seconds", "cost", "stationarity", "decision",
                                "steps", "theta_min", "residual", "certify_seconds", "escape_cost", "alpha", "best")}
        q.update(ex)
        levels.append(q)
    res = {"poses": n, "lambda_min_known": -lam, "eta": eta, "max_rounds": max_rounds, "max_steps": max_steps,
           "status": out["status"], "r": out["r"], "wall_seconds": wall, "levels": levels}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100, 10_000])
    ap.add_argument("--max-rounds", type=int, default=1000, help="solver rounds per level at most")
    ap.add_argument("--max-steps", type=int, default=40_000, help="Lanczos steps per certificate at most")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "staircase.json"))
    a = ap.parse_args()
    try:
        commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    res = {"commit": commit,
           "note": "reports, thresholds nothing. escape_ms / transfer_ms: HIP events inside kmx_cert_escape "
                   "(8 candidates: lift, cost and reduction launches; the upload of y and alpha and the download "
                   "of the costs). host_route_ms: numpy escape_point for the 8 candidates plus 8 kmx_cert_set_point "
                   "calls, the host clock. A level whose solve hit max_rounds above stat_tol ends the run as "
                   "NOT_STATIONARY.", "runs": []}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    for n in a.sizes:
        res["runs"].append(run(n, a.max_rounds, a.max_steps, a.device))
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
