"""Inputs on which the RTR block update rejects, skips, shrinks, grows and clamps.

Shared by test_rtr_branches_cpu.py (which asserts, from the restatement's
statistics, that each input does what it is here for) and
test_rtr_branches_gpu.py (which runs the HIP path on them).

Every input is test_dpgo_gpu._setup's construction at 3 robots x 30 poses and
270 edges: make_pose_graph(3, 90, 270, outlier_frac, seed=0), r = 5,
lifting_matrix(5, seed=1), the start `init` perturbed by default_rng(7)
(rotation normal(0, perturb), translation normal(0, 5 perturb)). Rounds are
concurrent, with refresh() before each round of the restatement.

  A   perturb 1.5, 3 RTR iterations, radius = max radius = 1e4, tCG cap 25, L2
  B   A with 2 RTR iterations
  C   A with 1 RTR iteration: every update is rejected
  C'  C without the preconditioner: every stop is negative curvature
  D   A with GNC-TLS and 20 % outliers
  E   perturb 0.05, 2 RTR iterations, gradnorm_tol 3000: accepted, then skipped
  F   perturb 0.3, 4 RTR iterations, radius 0.5, max radius 1.5: grows, clamps
  A1  A's one-sync tCG form
  OK  the control: E's input at the default gradient tolerance, all accepted
"""
import numpy as np

from kmx.dpgo.params import PGOAgentParameters, RobustCostType
from kmx.synth import lift, lifting_matrix, make_pose_graph
from kmx.synth.pose_graph import _expm_so3

R_LIFT = 5
BOUNDARY = ("negative_curvature", "exceeded_trust_region")

# rho, HIP path against restatement: the restatement's serial round against its
# all-cores variant (sums grouped differently) differs by at most S_SELF
# relative to max(1, |rho|) over A-F (test_rtr_branches_cpu.py prints it); a
# hundred times that, and no less than the suite's 1e-9 for the costs rho is
# formed from.
S_SELF = 6.2e-11
RHO_TOL = max(100 * S_SELF, 1e-9)

# id: (perturb, outlier_frac, robust, rounds, ROptParameters fields)
_HARD = dict(RTR_initial_radius=1e4, RTR_max_radius=1e4, RTR_tCG_iterations=25)
CASES = {
    "A": (1.5, 0.0, False, 6, dict(_HARD, RTR_iterations=3)),
    "B": (1.5, 0.0, False, 8, dict(_HARD, RTR_iterations=2)),
    "C": (1.5, 0.0, False, 8, dict(_HARD, RTR_iterations=1)),
    "Cp": (1.5, 0.0, False, 8, dict(_HARD, RTR_iterations=1, use_preconditioner=False)),
    "D": (1.5, 0.2, True, 6, dict(_HARD, RTR_iterations=3)),
    "E": (0.05, 0.0, False, 6, dict(RTR_iterations=2, gradnorm_tol=3000.0)),
    "F": (0.3, 0.0, False, 4, dict(RTR_iterations=4, RTR_initial_radius=0.5, RTR_max_radius=1.5)),
    "A1": (1.5, 0.0, False, 6, dict(_HARD, RTR_iterations=3, tCG_form="onesync")),
    "OK": (0.05, 0.0, False, 6, dict(RTR_iterations=2)),
}
ALL = ("A", "B", "C", "Cp", "D", "E", "F")


def build(case, **override):
    """(graph, parameters, start {robot: X}, rounds) of one input; `override`
    replaces ROptParameters fields (the reference comparison runs A with one
    RTR iteration)."""
    perturb, outlier, robust, rounds, lo_fields = CASES[case]
    g = make_pose_graph(3, 90, 270, outlier_frac=outlier, seed=0)
    P = PGOAgentParameters(r=R_LIFT)
    if not robust:
        P.robustCostParams.costType = RobustCostType.L2
    for k, v in {**lo_fields, **override}.items():
        assert hasattr(P.localOptimizationParams, k), k
        setattr(P.localOptimizationParams, k, v)
    Y = lifting_matrix(R_LIFT, seed=1)
    rng = np.random.default_rng(7)
    X0 = {}
    for a in range(g.n_robots):
        k = int(g.n_poses[a])
        Rp = g.init_R[a] @ _expm_so3(rng.normal(0, perturb, (k, 3)))
        X0[a] = lift(Rp, g.init_t[a] + rng.normal(0, 5 * perturb, (k, 3)), Y)
    return g, P, X0, rounds


def oracle(g, P, X0):
    from oracle.oracle import OraclePGO
    o = OraclePGO(P.to_c(), g)
    for a in range(g.n_robots):
        o.set_iterate(a, X0[a])
    o.refresh()
    return o


_RUNS = {}


def oracle_rounds(case, threads=1, inner=1):
    """The restatement's rounds on one input, computed once per process and
    left unchanged: per round {"st": statistics per robot, "X": iterates}."""
    key = (case, threads, inner)
    if key not in _RUNS:
        g, P, X0, rounds = build(case)
        o = oracle(g, P, X0)
        out = []
        for _ in range(rounds):
            o.refresh()
            st = o.iterate(threads=threads, inner=inner)
            out.append({"st": st, "X": [o.get_iterate(a).copy() for a in range(g.n_robots)]})
        _RUNS[key] = out
    return _RUNS[key]


def all_stats(run):
    return [s for rec in run for s in rec["st"]]


def moved_then(run, what):
    """(round, robot) of the block updates that moved the iterate in an
    earlier RTR iteration and whose last iteration was `what`: "rejected" (a
    step was tried and not accepted) or "skipped" (the gradient norm test)."""
    out = []
    for it, rec in enumerate(run):
        for a, s in enumerate(rec["st"]):
            last = "skipped" if s["tcg_stop"] == "skipped" else "accepted" if s["accepted"] else "rejected"
            if s["rel_change"] > 0 and last == what:
                out.append((it, a))
    return out


def rho_off_thresholds(s, accept_rho, margin=1e-3):
    """No decision of this update sits on a threshold of rho."""
    return all(abs(s["rho"] - t) >= margin for t in (0.25, 0.75, accept_rho))
