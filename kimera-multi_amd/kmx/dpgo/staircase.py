"""The Riemannian staircase around the dual certificate (SURVEY.md §9.1;
DESIGN.md §17): solve at rank r, certify, and while S(X) has an eigenvalue
below -eta at a stationary point, escape along its Ritz vector to rank r + 1
(kmx_cert_escape: a line search over a ladder of step lengths, on the device),
descend there and certify again.

The team is on one device (world == 1), as certify_team has it. The weights
are fixed: the staircase asks whether the L2 problem of the weights a run
ended with is solved, so GNC is off in the level solves.
"""
from __future__ import annotations

import copy
import time

import numpy as np

from .certify import Certifier, flatten_team, rounding_lift, split_team
from .params import RobustCostType

DEFAULT_ALPHAS = tuple(2.0 ** -k for k in range(8))


def _level_params(params, r, grad_tol):
    """params for a level solve: rank r, the L2 cost of fixed weights, and a
    skip threshold no larger than grad_tol (a block whose gradient is below
    the solver's threshold is skipped, so a larger one could never reach
    grad_tol)."""
    P = copy.deepcopy(params)
    P.r = int(r)
    P.robustCostParams.costType = RobustCostType.L2
    P.acceleration = False
    lo = P.localOptimizationParams
    lo.gradnorm_tol = min(float(lo.gradnorm_tol), float(grad_tol))
    return P


def _default_solver(P, g, device):
    from .solver import BlockSolver
    s = BlockSolver(P, device)
    s.set_graph_data(g)  # every robot is local
    s.set_gnc_schedule(False)
    return s


def staircase_team(g, X_by_robot, weights=None, params=None, *, eta: float, r_max: int, grad_tol: float,
                   stat_tol: float, max_rounds: int, alphas=None, device: int = 0, solver_factory=None,
                   certifier=None, **cert_kw) -> dict:
    """The staircase from the team's iterate X_by_robot ({robot: [n_a, r, 4]}
    or a list) on the graph g (PoseGraphData) with the fixed `weights` ([m];
    None: g.weight) and the solver parameters `params` (PGOAgentParameters;
    its rank, cost type and GNC settings are replaced per level).

    Per level: a fresh BlockSolver at the level's rank runs rounds until every
    robot's gradnorm_init <= grad_tol or max_rounds is reached (a round is a
    sweep, the robots updating one after the other: from an escape point the
    concurrent round, all blocks at once, can climb in cost); then set_point
    and min_eig(eta, want_vector=True). The run stops with status "CERTIFIED",
    "UNDECIDED", "RANK_LIMIT" (NEGATIVE at r == r_max), "NOT_STATIONARY"
    (NEGATIVE with stationarity > stat_tol: away from a stationary point S is
    indefinite as a rule, so the rank is not raised on an unconverged iterate)
    or "NO_DESCENT" (no candidate of the ladder is below the point's cost).
    Otherwise the best candidate is committed and the next level starts from
    it. alphas: the ladder of step lengths (1..8; default 2^-k, k = 0..7).
    cert_kw: min_eig's max_steps, test_every, check_every, seed.
    block_steps counts the block updates that ran a tCG step at all. An
    escape point lies next to a saddle, where tCG meets negative curvature and
    a step to the boundary of the initial trust region is rejected; the radius
    starts again at RTR_initial_radius in every block update and a rejection
    quarters it, so params should allow several RTR iterations per update
    (with 3, a 24-pose block repeated the same three rejected steps for 400
    rounds on the CPU restatement; with 6 or more it converged in 3).
    solver_factory(P, g, device) and certifier replace the BlockSolver and the
    Certifier (the CPU tests inject restatements).

    -> {"status", "r", "X": {robot: [n_a, r, 4]}, "lift": rounding_lift(X),
    "levels": [{r, rounds, block_steps, cost, trace_lambda, stationarity,
    decision, theta_min, residual, steps, escape_cost, alpha, best,
    solve_seconds, certify_seconds, escape_seconds}, ...]}."""
    if params is None:
        from .params import PGOAgentParameters
        params = PGOAgentParameters()
    n, src, dst, X = flatten_team(g, X_by_robot)
    r = int(X.shape[1])
    if isinstance(r_max, bool) or int(r_max) != r_max or not r <= int(r_max) <= 8:
        raise ValueError(f"r_max: expected an integer in {r}..8 (the iterate's rank .. 8), got {r_max!r}")
    r_max = int(r_max)
    if int(max_rounds) < 0:
        raise ValueError(f"max_rounds: expected >= 0, got {max_rounds!r}")
    for name, v in (("grad_tol", grad_tol), ("stat_tol", stat_tol)):
        if not np.isfinite(v) or not v >= 0:
            raise ValueError(f"{name}: expected a finite number >= 0, got {v!r}")
    alphas = np.asarray(DEFAULT_ALPHAS if alphas is None else alphas, np.float64)
    Certifier.check_escape(n, 3, np.zeros(4 * n), alphas)  # the ladder alone
    w = np.ascontiguousarray(g.weight if weights is None else weights, np.float64)
    Certifier.check_weights(int(g.m), w)
    make_solver = solver_factory or _default_solver

    c = certifier if certifier is not None else Certifier(device)
    levels = []
    status = None
    Xs = split_team(g, X)
    try:
        c.set_graph(n, src, dst, g.R, g.t, g.kappa, g.tau, w)
        while status is None:
            lv = {"r": r}
            # 1. descend at rank r
            t0 = time.perf_counter()
            s = make_solver(_level_params(params, r, grad_tol), g, device)
            try:
                s.set_weights(w)
                for a in range(int(g.n_robots)):
                    s.set_iterate(a, Xs[a])
                rounds = block_steps = 0
                nr = int(g.n_robots)
                while rounds < int(max_rounds):
                    # a round is a sweep: the robots update in turn, each against the others' new rows
                    # (an accepted step then lowers the team's cost; updating all blocks at once need not)
                    gn = []
                    for a in range(nr):
                        act = np.zeros(nr, np.uint8)
                        act[a] = 1
                        s.refresh_local()
                        q = s.iterate(act)[a]
                        gn.append(q["gradnorm_init"])
                        block_steps += int(q["hessvecs"] > 0)  # 0: its first RTR iteration was skipped
                    rounds += 1
                    if all(v <= grad_tol for v in gn):
                        break
                Xs = {a: s.get_iterate(a) for a in range(int(g.n_robots))}
            finally:
                if hasattr(s, "close"):
                    s.close()
            lv.update(rounds=rounds, block_steps=block_steps, solve_seconds=time.perf_counter() - t0)
            # 2. certify
            t0 = time.perf_counter()
            X = flatten_team(g, Xs)[3]
            info = c.set_point(X)
            res = c.min_eig(eta, want_vector=True, **cert_kw)
            lv.update(info)
            lv.update({k: res[k] for k in ("decision", "theta_min", "theta_max", "residual", "steps")})
            lv["certify_seconds"] = time.perf_counter() - t0
            lv.update(escape_cost=None, alpha=None, best=None, escape_seconds=0.0)
            levels.append(lv)
            # 3. stop, or escape to rank r + 1
            if res["decision"] != "NEGATIVE":
                status = res["decision"]
            elif r == r_max:
                status = "RANK_LIMIT"
            elif info["stationarity"] > stat_tol:
                status = "NOT_STATIONARY"
            else:
                t0 = time.perf_counter()
                esc = c.escape(res["y"], alphas)
                lv["escape_cost"] = [float(v) for v in esc["cost"]]
                lv["best"] = esc["best"]
                if esc["best"] < 0:
                    status = "NO_DESCENT"
                else:
                    lv["alpha"] = float(alphas[esc["best"]])
                    X, _ = c.escape_commit(esc["best"])
                    Xs = split_team(g, X)
                    r += 1
                lv["escape_seconds"] = time.perf_counter() - t0
    finally:
        if certifier is None:
            c.close()
    return {"status": status, "r": r, "X": Xs, "lift": rounding_lift(X), "levels": levels}
