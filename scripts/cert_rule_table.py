#!/usr/bin/env python3
"""The table behind the certificate's residual factor (DESIGN.md 16;
cert_host.h CT_RESIDUAL_FACTOR, tests/cert_ref.py CERT_C): the numpy restatement
of the Lanczos scan over family F (tests/cert_ref.py: 1350 runs on almost
stationary points), decided under rho <= c eta for every candidate c, each
decision held to numpy.linalg.eigvalsh of the dense S. Host only; no device.

  python scripts/cert_rule_table.py [--out table.json]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tests import cert_ref as CR  # noqa: E402


def ring_example(n=100, seeds=200):
    """DESIGN.md 17's event: the winding ring solved at rank 4 (the CPU
    restatement of the solver, a dense certifier), then the scan at
    eta = |lambda_min| / 4 and / 2 from many start vectors, under rho <= eta
    and under the rule's factor."""
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "kimera-multi_amd"))
    from kmx.dpgo.params import PGOAgentParameters
    from kmx.dpgo.staircase import staircase_team
    from tests import stair_ref as SR
    g, Xs, gd = SR.ring_team(n, 1)
    P = PGOAgentParameters(r=3)
    P.localOptimizationParams.RTR_iterations = 8
    P.localOptimizationParams.RTR_tCG_iterations = 50
    lim = staircase_team(g, Xs, None, P, r_max=4, certifier=SR.NumpyCertifier(), eta=1e-5, grad_tol=1e-7,
                         stat_tol=1e-5, max_rounds=1000, solver_factory=SR.oracle_solver)
    X = lim["X"][0]
    Q, S = CR.dense_of(gd, X)
    ev = np.linalg.eigvalsh(S)
    stat = CR.point_info(X, Q)["stationarity"]
    print(f"ring of {n} at rank {X.shape[1]}: lambda_min {ev[0]:.6e}, |X S|_F {stat:.1e}")
    for frac in (4, 2):
        eta = abs(ev[0]) / frac
        for c in (1.0, CR.CERT_C):
            count, steps = {}, 0
            for seed in range(seeds):
                tests = []
                CR.scan(S, eta, seed, 5000, 10, c=c, tests=tests)
                t = tests[-1]
                count[t["decision"]] = count.get(t["decision"], 0) + 1
                steps += t["steps"]
                if t["decision"] == "CERTIFIED":
                    print(f"  false certificate: eta = |lambda_min| / {frac}, c = {c:g}, seed {seed}, "
                          f"step {t['steps']}, "
                          f"theta_min {t['theta_min']:.2e}, rho / eta {t['residual'] / eta:.3f}")
            print(f"eta = |lambda_min| / {frac}, c = {c:g}: {count}, {steps} steps")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ring", action="store_true", help="the ring example of DESIGN.md 17 instead of the table")
    a = ap.parse_args()
    if a.ring:
        return ring_example()
    cands = CR.CERT_C_CANDIDATES
    stat = {c: dict(false=[], certified=0, negative=0, undecided=0, steps_true=0) for c in cands}
    two = dict(false=0, steps_true=0)  # c = 1 at two consecutive tests
    below = above = ratio = 0.0
    runs = 0
    eps = np.finfo(float).eps
    for pt in CR.family_points():
        ev, eta = pt["ev"], pt["eta"]
        for seed in CR.F_SEEDS:
            tests = []
            CR.scan(pt["S"], eta, seed, pt["max_steps"], CR.F_TEST_EVERY, c=min(cands), tests=tests)
            runs += 1
            for t in tests:
                below = max(below, (ev[0] - t["theta_min"]) / ev[-1])
                above = max(above, (t["theta_max"] - ev[-1]) / ev[-1])
                ratio = max(ratio, (t["true_residual"] - t["residual"]) / (t["steps"] * eps * ev[-1]))
            for c in cands:
                d, k = CR.first_decision(tests, eta, c)
                s = stat[c]
                s[d.lower()] += 1
                if d == "CERTIFIED":
                    if ev[0] < -eta:
                        t = next(t for t in tests if t["steps"] == k)
                        s["false"].append(dict(graph=pt["graph"], dseed=pt["dseed"], delta=pt["delta"], seed=seed,
                                               lambda_min_over_eta=ev[0] / eta, rho_over_eta=t["residual"] / eta,
                                               theta_min_over_eta=t["theta_min"] / eta, steps=k))
                    else:
                        s["steps_true"] += k
                if d == "NEGATIVE":
                    assert ev[0] < -eta
            prev = None
            for t in tests:
                d = CR.rule(t["theta_min"], t["residual"], eta, 1.0)
                if d == "NEGATIVE":
                    break
                if d == "CERTIFIED" and prev == "CERTIFIED":
                    if ev[0] < -eta:
                        two["false"] += 1
                    else:
                        two["steps_true"] += t["steps"]
                    break
                prev = d
    print(f"{runs} runs")
    print("| c | certified | negative | undecided | false certificates | steps summed over true certificates |")
    print("|---|---|---|---|---|---|")
    for c in cands:
        s = stat[c]
        print(f"| {c:g} | {s['certified']} | {s['negative']} | {s['undecided']} | {len(s['false'])} | "
              f"{s['steps_true']} |")
    print(f"| 1, at two consecutive tests | | | | {two['false']} | {two['steps_true']} |")
    print(f"(lambda_min - theta_min) / lambda_max <= {below:.3e}")
    print(f"(theta_max - lambda_max) / lambda_max <= {above:.3e}")
    print(f"(|S y - theta_min y| - rho) / (k eps lambda_max) <= {ratio:.3e}")
    for c in cands:
        for f in stat[c]["false"]:
            print("false certificate at c =", c, f)
    if a.out:
        Path(a.out).write_text(json.dumps(dict(runs=runs, per_c={str(c): stat[c] for c in cands}, two_tests=two,
                                               ritz_below=below, ritz_above=above, residual_ratio=ratio), indent=1))


if __name__ == "__main__":
    main()
