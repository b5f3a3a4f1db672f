"""kmx.pipeline — configs[4]: the multi-robot back end end to end on MI355X.

Reference flow (Kimera-Multi, images/kimera-multi.drawio):
  * Kimera-Distributed's verification thread takes inter-robot loop-closure
    candidates and runs computeMatchedIndices -> geometricVerificationNister ->
    recoverPose (drawio:246, 405, 2583-2598); accepted loop closures become
    shared loop closures of the pose graph (addSharedLoopClosure, drawio:2817);
  * dpgo_ros requests the pose graph (drawio:557-574, 623-632), initialises
    every robot in its own frame and aligns it to the global frame over the
    shared loop closures (INITIALIZE, drawio:2271-2307; kmx.dpgo.init), then
    runs synchronous RBCD rounds with GNC-TLS (drawio:2058-2066, 2212-2215).

Here every stage runs on the MI355X path of this package: the candidates are
verified in one batched kmx_lcd_verify call per rank (candidates sharded by
query robot, no collective), the accepted loop closures are gathered to every
rank (one small all_gather), and the RBCD rounds run through RBCDDriver
(robot blocks dealt to ranks, one all_to_all of public poses per round).

Synthetic inputs (the Campus bags are unavailable offline): a team pose graph
without inter-robot loop closures (kmx.synth.make_pose_graph with f_inter = 0
and outlier_scope = "robot": its outlier loop closures join poses of one
robot), and a loop-closure stream whose
keyframe pairs observe a common scene under the GROUND-TRUTH relative pose of
the two robot poses (true candidates) or are unrelated frames (false ones).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from .dpgo.init import align_to_world, transform_trajectory
from .synth.lcd import LcdPool, make_lcd_pool
from .synth.pose_graph import PoseGraphData, _compose_scan


@dataclass
class LcStream:
    """Inter-robot loop-closure candidates. Candidate c asks whether keyframe
    (r_q[c], p_q[c]) sees the place of (r_m[c], p_m[c]); its frames in `pool`
    are cand_query[c] / cand_match[c]; truth[c] marks a planted loop closure."""
    pool: LcdPool
    r_q: np.ndarray
    p_q: np.ndarray
    r_m: np.ndarray
    p_m: np.ndarray
    cand_query: np.ndarray
    cand_match: np.ndarray
    truth: np.ndarray


def _flat(g: PoseGraphData):
    rob = np.concatenate([np.full(int(n), a, np.int32) for a, n in enumerate(g.n_poses)])
    idx = np.concatenate([np.arange(int(n), dtype=np.int32) for n in g.n_poses])
    return rob, idx, np.concatenate(g.gt_R), np.concatenate(g.gt_t)


def make_lc_stream(g: PoseGraphData, n_true: int, n_false: int, *, n_feats: int = 500, radius: float = 3.0,
                   max_angle: float = np.pi / 6, seed: int = 1) -> LcStream:
    """`n_true` true candidates: pose pairs of different robots whose ground
    truth positions are within `radius` and whose relative rotation is below
    `max_angle` (the views overlap); the keyframe pair plants the ground-truth
    relative pose T_q^-1 T_m. `n_false` false candidates pair the query frame
    of one true candidate with the match frame of another candidate of a
    different robot (unrelated scenes)."""
    from scipy.spatial import cKDTree
    rng = np.random.Generator(np.random.PCG64(seed))
    rob, idx, Rw, tw = _flat(g)
    pairs = cKDTree(tw).query_pairs(radius, output_type="ndarray")
    pairs = pairs[rob[pairs[:, 0]] != rob[pairs[:, 1]]]
    Rrel = np.einsum("kji,kjl->kil", Rw[pairs[:, 0]], Rw[pairs[:, 1]])
    cosang = np.clip((np.trace(Rrel, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)
    pairs = pairs[np.arccos(cosang) <= max_angle]
    if pairs.shape[0] < n_true:
        raise ValueError(f"only {pairs.shape[0]} overlapping inter-robot pose pairs for {n_true} true candidates")
    sel = pairs[np.sort(rng.choice(pairs.shape[0], n_true, replace=False))]
    swap = rng.random(n_true) < 0.5
    q = np.where(swap, sel[:, 1], sel[:, 0])
    m = np.where(swap, sel[:, 0], sel[:, 1])
    R_qm = np.einsum("kji,kjl->kil", Rw[q], Rw[m])
    t_qm = np.einsum("kji,kj->ki", Rw[q], tw[m] - tw[q])
    pool = make_lcd_pool(2 * n_true, n_feats, R_qm=R_qm, t_qm=t_qm, seed=seed)
    # false candidates: query frame of pair k with the match frame of pair k2 (other robot)
    fk = rng.integers(0, n_true, n_false)
    fk2 = rng.integers(0, n_true, n_false)
    for _ in range(64):
        bad = (fk2 == fk) | (rob[m[fk2]] == rob[q[fk]])
        if not bad.any():
            break
        fk2[bad] = rng.integers(0, n_true, int(bad.sum()))
    keep = (fk2 != fk) & (rob[m[fk2]] != rob[q[fk]])
    fk, fk2 = fk[keep], fk2[keep]
    k = np.arange(n_true)
    cq = np.concatenate([2 * k, 2 * fk]).astype(np.int32)
    cm = np.concatenate([2 * k + 1, 2 * fk2 + 1]).astype(np.int32)
    qq = np.concatenate([q, q[fk]])
    mm = np.concatenate([m, m[fk2]])
    order = np.argsort(rob[qq], kind="stable")  # grouped by query robot (sharding)
    truth = np.concatenate([np.ones(n_true, bool), np.zeros(fk.shape[0], bool)])
    return LcStream(pool=pool, r_q=rob[qq][order], p_q=idx[qq][order], r_m=rob[mm][order], p_m=idx[mm][order],
                    cand_query=cq[order], cand_match=cm[order], truth=truth[order])


@dataclass
class Accepted:
    """Verified loop closures (query -> match): T_q^-1 T_m = (R, t)."""
    r1: np.ndarray
    p1: np.ndarray
    r2: np.ndarray
    p2: np.ndarray
    R: np.ndarray
    t: np.ndarray
    truth: np.ndarray
    n_verified: int = 0
    stats: dict = field(default_factory=dict)


def accepted_from_results(stream: LcStream, sel: np.ndarray, results) -> Accepted:
    """Turn kmx_lcd_result records of the candidates `sel` into loop-closure
    measurements: the structured array of LoopClosureDetector.verify_arrays,
    or a list of result dicts (LoopClosureDetector.verify, the CPU tests'
    restatement)."""
    if isinstance(results, np.ndarray) and results.dtype.names:
        ok = results["accepted"] != 0
        T = np.asarray(results["T_query_match"], np.float64).reshape(-1, 12)
    else:
        ok = np.array([r["accepted"] for r in results], bool)
        T = np.array([r["T_query_match"] for r in results], np.float64).reshape(-1, 12)
    s = sel[ok]
    return Accepted(r1=stream.r_q[s], p1=stream.p_q[s], r2=stream.r_m[s], p2=stream.p_m[s],
                    R=T[ok, :9].reshape(-1, 3, 3), t=T[ok, 9:].reshape(-1, 3), truth=stream.truth[s],
                    n_verified=int(sel.shape[0]))


def merge_accepted(parts) -> Accepted:
    parts = list(parts)
    cat = lambda name: np.concatenate([getattr(a, name) for a in parts])  # noqa: E731
    out = Accepted(r1=cat("r1"), p1=cat("p1"), r2=cat("r2"), p2=cat("p2"), R=cat("R").reshape(-1, 3, 3),
                   t=cat("t").reshape(-1, 3), truth=cat("truth"), n_verified=sum(a.n_verified for a in parts))
    order = np.lexsort((out.p2, out.r2, out.p1, out.r1))
    for k in ("r1", "p1", "r2", "p2", "R", "t", "truth"):
        setattr(out, k, getattr(out, k)[order])
    return out


def team_graph(g0: PoseGraphData, acc: Accepted, kappa: float, tau: float) -> PoseGraphData:
    """The base graph plus the accepted loop closures as shared loop closures
    (weight 1, not fixed: GNC may reject them)."""
    k = acc.r1.shape[0]
    cat = np.concatenate
    return PoseGraphData(
        n_robots=g0.n_robots, n_poses=g0.n_poses,
        r1=cat([g0.r1, acc.r1]).astype(np.int32), p1=cat([g0.p1, acc.p1]).astype(np.int32),
        r2=cat([g0.r2, acc.r2]).astype(np.int32), p2=cat([g0.p2, acc.p2]).astype(np.int32),
        R=np.ascontiguousarray(cat([g0.R, acc.R])), t=np.ascontiguousarray(cat([g0.t, acc.t])),
        kappa=cat([g0.kappa, np.full(k, kappa)]), tau=cat([g0.tau, np.full(k, tau)]),
        weight=cat([g0.weight, np.ones(k)]), fixed=cat([g0.fixed, np.zeros(k, np.uint8)]),
        outlier=cat([g0.outlier, ~acc.truth]), gt_R=g0.gt_R, gt_t=g0.gt_t, init_R=g0.init_R, init_t=g0.init_t)


def odometry_init(g: PoseGraphData):
    """Each robot's odometry chain in its own frame (first pose = identity),
    from the graph's odometry edges (fixed, same robot, p -> p + 1)."""
    out = {}
    for a in range(g.n_robots):
        n = int(g.n_poses[a])
        sel = np.nonzero((g.r1 == a) & (g.r2 == a) & (g.p2 == g.p1 + 1) & (g.fixed == 1))[0]
        sel = sel[np.argsort(g.p1[sel], kind="stable")]
        if sel.shape[0] != n - 1 or not np.array_equal(g.p1[sel], np.arange(n - 1)):
            raise ValueError(f"robot {a}: odometry chain incomplete")
        out[a] = _compose_scan(g.R[sel], g.t[sel], np.eye(3), np.zeros(3))
    return out


@dataclass
class _Lc:
    r1: int
    p1: int
    r2: int
    p2: int
    R: np.ndarray
    t: np.ndarray
    kappa: float
    tau: float


def global_init(g: PoseGraphData, own: dict, *, first: int = 0):
    """Distributed initialisation: robot `first` defines the
    world frame; the others are aligned in breadth-first order over the
    robot graph of shared loop closures by GNC-TLS robust single-pose
    averaging (kmx.dpgo.init.align_to_world). Returns ({robot: (R, t)} in the
    world frame, {robot: (R_WA, t_WA, inlier weights)})."""
    sh = np.nonzero(g.r1 != g.r2)[0]
    lcs = [_Lc(int(g.r1[e]), int(g.p1[e]), int(g.r2[e]), int(g.p2[e]), g.R[e], g.t[e], float(g.kappa[e]),
               float(g.tau[e])) for e in sh]
    world = {first: own[first]}
    frames = {first: (np.eye(3), np.zeros(3), None)}
    nbr_global = {}

    def publish(a):
        R, t = world[a]
        for lc in lcs:
            for (r, p) in ((lc.r1, lc.p1), (lc.r2, lc.p2)):
                if r == a:
                    nbr_global[(r, p)] = (R[p], t[p])

    publish(first)
    pending = [a for a in range(g.n_robots) if a != first]
    while pending:
        progress = False
        for a in list(pending):
            mine = [lc for lc in lcs if lc.r1 == a or lc.r2 == a]
            res = align_to_world(mine, a, own[a][0], own[a][1], nbr_global)
            if res is None:
                continue
            R_WA, t_WA, w = res
            world[a] = transform_trajectory(R_WA, t_WA, *own[a])
            frames[a] = (R_WA, t_WA, w)
            publish(a)
            pending.remove(a)
            progress = True
        if not progress:
            raise ValueError(f"robots {pending} share no loop closure with the initialised team")
    return world, frames


def rounded(X: np.ndarray, YLift: np.ndarray):
    """dpgo rounding: T_i = YLift^T X_i, R projected to SO(3)."""
    T = np.einsum("ad,nac->ndc", YLift, X)
    U, _, Vt = np.linalg.svd(T[:, :, :3])
    D = np.ones((X.shape[0], 3))
    D[:, 2] = np.sign(np.linalg.det(U @ Vt))
    return (U * D[:, None, :]) @ Vt, T[:, :, 3].copy()


def ate_rmse(g: PoseGraphData, traj: dict, *, anchor_robot: int = 0) -> float:
    """Position RMSE over the team after expressing both the estimate and the
    ground truth relative to `anchor_robot`'s first pose."""
    Re0, te0 = traj[anchor_robot][0][0], traj[anchor_robot][1][0]
    Rg0, tg0 = g.gt_R[anchor_robot][0], g.gt_t[anchor_robot][0]
    err = []
    for a, (R, t) in traj.items():
        pe = (t - te0) @ Re0
        pg = (g.gt_t[a] - tg0) @ Rg0
        err.append(((pe - pg) ** 2).sum(1))
    return float(np.sqrt(np.concatenate(err).mean()))


def run_pipeline(g0: PoseGraphData, stream: LcStream, params, lcd_params, *, rank: int = 0, world: int = 1,
                 device: int = 0, rounds: int = 100, verifier=None, solver=None, exchange_device=None,
                 return_trajectory: bool = False, local_init: str = "odometry", certify_eta=None,
                 staircase_rmax=None, staircase_kw=None, mesh=None, mesh_k: int = 4,
                 mesh_window_s: float = 1.0, mesh_graph=None, mesh_graph_simplify: str = "host") -> dict:
    """One team run: LCD verification of this rank's candidates (query robot
    in the rank's robot range) -> all_gather of the accepted loop closures ->
    team graph -> global initialisation -> `rounds` concurrent RBCD rounds
    with GNC. `verifier(cand_query, cand_match) -> result dicts` and `solver`
    replace the HIP LoopClosureDetector / BlockSolver (the CPU tests inject
    the restatement). local_init: how every robot is initialised in its own
    frame before the global alignment: "odometry" (its odometry chain, the
    default) or "chordal_gpu" (kmx.dpgo.init.chordal_initialization_team: the
    chordal relaxation over its private measurements, one batch on the device;
    an L2 method, so outlier loop closures at weight 1 can make it worse than
    the odometry chain) or "robust_chordal_gpu"
    (robust_chordal_initialization_team: GNC-TLS around that solve, decided on
    the device, which rejects outlier loop closures). certify_eta (one rank
    only: the team's X must be on one device): the result gets a "certificate"
    entry, kmx.dpgo.certify.certify_team on the final iterate and the final GNC
    weights at tolerance certify_eta, and out["dpgo"]["cost"], the solver's
    cost of that iterate (half the certificate's tr(X Q X^T)). staircase_rmax
    (needs certify_eta, one rank only): after the rounds the Riemannian
    staircase (kmx.dpgo.staircase.staircase_team) runs from the final iterate
    with the final GNC weights fixed, up to rank staircase_rmax, at tolerance
    certify_eta; the result gets a "staircase" entry (status, r, levels) with
    "ate_m", the error of the trajectory rounded with the result's own lift
    (rounding_lift). staircase_kw: staircase_team's grad_tol, stat_tol,
    max_rounds, alphas and min_eig's keywords (defaults: 1e-6, 1e-3, 200).
    "certificate" stays the RBCD iterate's. mesh (one rank only; a
    kmx.synth.mesh.MeshData, or anything with its xyz, robot, stamp, kf_stamp
    and gt_xyz): after the rounds the mesh follows the result on the device
    (kmx.pgmo.MeshDeformer, mesh_k nodes per vertex in a window of
    mesh_window_s): every robot's odometry chain is the rest trajectory and
    the rounded RBCD trajectory the current one. The result gets a "mesh"
    entry: vertices, unbound, bind_seconds and deform_seconds (device times),
    rmse_before_m and rmse_after_m against mesh.gt_xyz, both expressed
    relative to the anchor robot's first pose as ate_rmse does (before: the
    vertices as given, in their robots' odometry frames), and with
    return_trajectory "xyz", the deformed vertices. mesh_graph (needs mesh; a
    voxel resolution in metres): the mesh is simplified at that resolution,
    the deformation graph over keyframes and control vertices is solved on the
    device with soft priors on the keyframes at the rounded RBCD trajectory
    (kmx.pgmo.DeformationGraph), and the vertices are bound to and moved by
    the graph's nodes; the "mesh" entry gains "graph" (see deform_mesh).
    mesh_graph_simplify: deform_mesh's graph_simplify ("host", the default, or
    "gpu"). Returns stage timings and metrics (identical on every rank)."""
    import time

    if certify_eta is not None and world > 1:
        raise ValueError("certify_eta needs world == 1: the team's iterate is not on one rank")
    if staircase_rmax is not None and certify_eta is None:
        raise ValueError("staircase_rmax needs certify_eta: the staircase decides at that tolerance")
    if staircase_rmax is not None and world > 1:
        raise ValueError("staircase_rmax needs world == 1: the team's iterate is not on one rank")
    if mesh is not None and world > 1:
        raise ValueError("mesh needs world == 1: the team's trajectory and the mesh are on one rank")
    if mesh_graph is not None and mesh is None:
        raise ValueError("mesh_graph needs mesh: the graph is built from the mesh")

    from .dpgo.driver import RBCDDriver, robot_ranges
    from .synth.pose_graph import lift, lifting_matrix
    dist = None
    if world > 1:
        import torch.distributed as dist
    lo, hi = robot_ranges(g0.n_robots, world)[rank]
    sel = np.nonzero((stream.r_q >= lo) & (stream.r_q < hi))[0]
    out = {"rank": rank, "world": world, "candidates": int(stream.truth.shape[0])}
    # 1. LCD (candidates of this rank's query robots; pool upload and a warm-up call outside the timed region)
    if verifier is None:
        from .lcd import LoopClosureDetector
        det = LoopClosureDetector(lcd_params, device=device)
        det.set_pool(stream.pool)
        if sel.size:  # one small untimed call: the kernels' first launch (code-object load, scratch)
            det.verify(stream.cand_query[sel[:64]], stream.cand_match[sel[:64]])
        det.sync()
        verifier = det.verify_arrays
    t0 = time.perf_counter()
    results = verifier(stream.cand_query[sel], stream.cand_match[sel])
    t_lcd = time.perf_counter() - t0
    acc = accepted_from_results(stream, sel, results)
    if dist is not None:
        parts = [None] * world
        dist.all_gather_object(parts, (acc, t_lcd))
        acc = merge_accepted([p[0] for p in parts])
        t_lcd = max(p[1] for p in parts)
    else:
        acc = merge_accepted([acc])
    out["lcd"] = {"verified": acc.n_verified, "accepted": int(acc.r1.shape[0]),
                  "true_positives": int(acc.truth.sum()), "planted": int(stream.truth.sum()),
                  "seconds": t_lcd, "candidates_per_s": acc.n_verified / max(t_lcd, 1e-12)}
    # 2. team graph + distributed initialisation (host control, identical on every rank)
    t0 = time.perf_counter()
    rc = lcd_params
    g = team_graph(g0, acc, getattr(rc, "kappa", 1e4), getattr(rc, "tau", 1e2))
    if local_init == "odometry":
        own0 = odometry_init(g)
    elif local_init == "chordal_gpu":
        from .dpgo.init import chordal_initialization_team
        Rl, tl = chordal_initialization_team(g, device=device)
        own0 = {a: (Rl[a], tl[a]) for a in range(g.n_robots)}
    elif local_init == "robust_chordal_gpu":
        from .dpgo.init import robust_chordal_initialization_team
        Rl, tl, _ = robust_chordal_initialization_team(g, device=device, barc=params.robustCostParams.GNCBarc,
                                                       min_inliers=params.robustInitMinInliers)
        own0 = {a: (Rl[a], tl[a]) for a in range(g.n_robots)}
    else:
        raise ValueError(f"unknown local_init {local_init!r}")
    traj0, frames = global_init(g, own0)
    out["init"] = {"seconds": time.perf_counter() - t0, "ate_m": ate_rmse(g, traj0), "local_init": local_init,
                   "edges": g.m, "shared_loop_closures": int((g.r1 != g.r2).sum())}
    # 3. RBCD + GNC rounds
    Y = lifting_matrix(params.r, seed=1)
    drv = RBCDDriver(params, g, rank=rank, world=world, device=device, solver=solver,
                     exchange_device=exchange_device)
    drv.initialize({a: lift(traj0[a][0], traj0[a][1], Y) for a in drv.robots})
    counters = getattr(drv.solver, "read_counters", None)
    if counters:
        drv.solver.sync()
        counters()
    t0 = time.perf_counter()
    drv.run_async(rounds)
    drv.solver.sync()
    t_pgo = time.perf_counter() - t0
    ei = float(counters()["edges_iters"]) if counters else float("nan")
    mine = {a: rounded(drv.iterate_of(a), Y) for a in drv.robots}
    if dist is not None:
        parts = [None] * world
        dist.all_gather_object(parts, (mine, t_pgo, ei))
        mine = {k: v for p in parts for k, v in p[0].items()}
        t_pgo = max(p[1] for p in parts)
        ei = sum(p[2] for p in parts)
    w = drv.solver.get_weights() if hasattr(drv.solver, "get_weights") else None
    out["dpgo"] = {"rounds": rounds, "seconds": t_pgo, "edges_iters_per_s": ei / max(t_pgo, 1e-12),
                   "ate_m": ate_rmse(g, mine)}
    if return_trajectory:  # the team's rounded trajectories (identical on every rank)
        out["trajectory"] = mine
    if w is not None and world == 1:
        lc = g.fixed == 0
        out["dpgo"]["gnc_weight_mean_inlier_lc"] = float(w[lc & ~g.outlier].mean()) if (lc & ~g.outlier).any() else None
        out["dpgo"]["gnc_weight_mean_outlier_lc"] = float(w[lc & g.outlier].mean()) if (lc & g.outlier).any() else None
    if certify_eta is not None:
        from .dpgo.certify import certify_team
        Xs = {a: drv.iterate_of(a) for a in range(g.n_robots)}
        out["dpgo"]["cost"] = solver_team_cost(drv.solver, g, Xs, w)
        out["certificate"] = certify_team(g, Xs, w, eta=certify_eta, device=device)
        if staircase_rmax is not None:
            from .dpgo.staircase import staircase_team
            kw = dict(grad_tol=1e-6, stat_tol=1e-3, max_rounds=200)
            kw.update(staircase_kw or {})
            sc = staircase_team(g, Xs, w, params, eta=certify_eta, r_max=staircase_rmax, device=device, **kw)
            off = np.concatenate([[0], np.cumsum(np.asarray(g.n_poses, np.int64))])
            Xf = np.concatenate([sc["X"][a] for a in range(g.n_robots)])
            Rr, tr = rounded(Xf, sc["lift"])
            traj = {a: (Rr[off[a]:off[a + 1]], tr[off[a]:off[a + 1]]) for a in range(g.n_robots)}
            out["staircase"] = {"status": sc["status"], "r": sc["r"], "levels": sc["levels"],
                                "ate_m": ate_rmse(g, traj)}
            if return_trajectory:
                out["staircase"]["trajectory"] = traj
    if mesh is not None:
        out["mesh"] = deform_mesh(g, mesh, odometry_init(g), mine, k=mesh_k, window_s=mesh_window_s, device=device,
                                  return_xyz=return_trajectory, graph_resolution=mesh_graph,
                                  graph_simplify=mesh_graph_simplify)
    if hasattr(drv.solver, "close"):
        drv.solver.close()
    return out


def mesh_rmse(g: PoseGraphData, xyz, gt_xyz, traj: dict, *, anchor_robot: int = 0) -> float:
    """Vertex RMSE after expressing the vertices relative to traj's first pose
    of `anchor_robot` and the ground truth relative to its ground-truth first
    pose (ate_rmse's convention)."""
    Re0, te0 = traj[anchor_robot][0][0], traj[anchor_robot][1][0]
    Rg0, tg0 = g.gt_R[anchor_robot][0], g.gt_t[anchor_robot][0]
    pe = (np.asarray(xyz, np.float64) - te0) @ Re0
    pg = (np.asarray(gt_xyz, np.float64) - tg0) @ Rg0
    return float(np.sqrt(((pe - pg) ** 2).sum(1).mean()))


def deform_mesh(g: PoseGraphData, mesh, rest: dict, current: dict, *, k: int = 4, window_s: float = 1.0,
                device: int = 0, return_xyz: bool = False, graph_resolution=None, graph_kappa: float = 100.0,
                graph_tau: float = 100.0, graph_solve=None, graph_horizon_s=None,
                graph_simplify: str = "host") -> dict:
    """The mesh stage of run_pipeline: keyframes of every robot as control
    nodes (rest[a] -> current[a]), one bind and one deformation on the device.
    graph_resolution (metres; default None: off): the mesh is simplified on a
    voxel grid of that size (kmx.pgmo.simplify_voxel; graph_horizon_s: its
    horizon_s), the deformation graph of
    keyframes and control vertices (graph_from_mesh, all edge weights 1) is
    solved on the device with soft priors (graph_kappa, graph_tau) on the
    keyframes at current[a] (graph_solve: DeformationGraph.solve's keywords),
    starting from every control vertex moved by its keyframe's correction, and
    the vertices are bound to and moved by the graph's nodes. The result
    then has "graph": nodes, edges, control_vertices, iterations, accepted,
    stop, cost_before, cost_after and solve_ms (device time). graph_simplify:
    where the simplification and the graph's edge arrays are formed: "host"
    (numpy, the default) or "gpu" (kmx.pgmo.MeshSimplifier); the arrays are
    equal, and so is everything after them."""
    from .pgmo import MeshDeformer
    if graph_simplify not in ("host", "gpu"):
        raise ValueError(f"unknown graph_simplify {graph_simplify!r}")
    graph = None
    if graph_resolution is None:
        md = MeshDeformer(k=k, window_s=window_s, n_robots=g.n_robots, device=device)
    else:
        from .pgmo import DeformationGraph, MeshSimplifier, graph_from_mesh, simplify_voxel
        if graph_simplify == "gpu":
            with MeshSimplifier(graph_resolution, graph_horizon_s, g.n_robots, device) as ms:
                ms.add(mesh.xyz, mesh.faces, mesh.stamp, mesh.robot)
                G = ms.graph(mesh.kf_stamp, [rest[a] for a in range(g.n_robots)])
        else:
            cx, cs, cr, cf, _ = simplify_voxel(mesh.xyz, mesh.faces, mesh.stamp, mesh.robot, graph_resolution,
                                               horizon_s=graph_horizon_s)
            G = graph_from_mesh(cx, cs, cr, cf, mesh.kf_stamp, [rest[a] for a in range(g.n_robots)])
        nk, n = G["n_keyframes"], G["g"].shape[0]
        mode = np.zeros(n, np.uint8)
        mode[:nk] = 1
        R_hat, t_hat = G["R_rest"].copy(), G["g"].copy()
        R_hat[:nk] = np.concatenate([current[a][0] for a in range(g.n_robots)])
        t_hat[:nk] = np.concatenate([current[a][1] for a in range(g.n_robots)])
        dg = DeformationGraph(device)
        try:
            dg.set_graph(G["R_rest"], G["g"], G["src"], G["dst"], G["w"], robot=G["robot"], stamp=G["stamp"])
            dg.set_priors(mode, R_hat, t_hat, graph_kappa, graph_tau)
            # the start: every control vertex follows its keyframe's rigid correction C = Rcur Rrest^T. A vertex
            # with fewer than two non-parallel outgoing edges keeps the part of C its edges do not determine.
            C_kf = R_hat[:nk] @ G["R_rest"][:nk].transpose(0, 2, 1)
            lk = G["link"]
            R0, t0 = R_hat.copy(), t_hat.copy()
            R0[nk:] = C_kf[lk]
            t0[nk:] = np.einsum("nij,nj->ni", C_kf[lk], G["g"][nk:] - G["g"][lk]) + t_hat[lk]
            dg.set_poses(R0, t0)
            res = dg.solve(**(graph_solve or {}))
            graph = {"nodes": n, "edges": int(G["src"].shape[0]), "control_vertices": n - nk,
                     "iterations": res["iterations"], "accepted": res["accepted"], "stop": res["stop"],
                     "cost_before": res["cost_initial"], "cost_after": res["cost_final"],
                     "solve_ms": dg.timing()["total_ms"]}
            md = dg.deformer(k, window_s, n_robots=g.n_robots)
            dg.push(md)
        finally:
            dg.close()
    try:
        if graph is None:
            for a in range(g.n_robots):
                md.add_keyframes(a, mesh.kf_stamp[a], rest[a][0], rest[a][1])
                md.update_trajectory(a, current[a][0], current[a][1])
        md.add_vertices(mesh.robot, mesh.stamp, mesh.xyz)
        xyz, st = md.deform()
        tm = md.timing()
    finally:
        md.close()
    res = {"vertices": int(st["vertices"]), "unbound": int(st["unbound"]), "bind_seconds": tm["bind_ms"] * 1e-3,
           "deform_seconds": tm["deform_ms"] * 1e-3,
           "rmse_before_m": mesh_rmse(g, mesh.xyz, mesh.gt_xyz, rest),
           "rmse_after_m": mesh_rmse(g, xyz, mesh.gt_xyz, current)}
    if graph is not None:
        res["graph"] = graph
    if return_xyz:
        res["xyz"] = xyz
    return res


def solver_team_cost(solver, g: PoseGraphData, X_by_robot: dict, w=None) -> float:
    """The team's cost f = 1/2 sum_e w_e r_e^2 at X_by_robot as the solver
    evaluates it: every robot's local cost (its private edges and its shared
    edges, neighbours at their current iterates) summed, less the shared
    edges' second count, which is formed here from the same iterates."""
    from .abi import KMX_EVAL_COST_EGRAD
    solver.refresh_local()
    f = sum(solver.eval(a, KMX_EVAL_COST_EGRAD, X_by_robot[a])[1] for a in range(g.n_robots))
    sh = np.nonzero(g.r1 != g.r2)[0]
    if sh.size:
        ws = np.asarray(g.weight if w is None else w, np.float64)[sh]
        Xi = np.stack([X_by_robot[int(a)][int(p)] for a, p in zip(g.r1[sh], g.p1[sh])])
        Xj = np.stack([X_by_robot[int(a)][int(p)] for a, p in zip(g.r2[sh], g.p2[sh])])
        eR = Xj[:, :, :3] - np.einsum("kad,kdc->kac", Xi[:, :, :3], g.R[sh])
        et = Xj[:, :, 3] - Xi[:, :, 3] - np.einsum("kad,kd->ka", Xi[:, :, :3], g.t[sh])
        f -= 0.5 * float((ws * (g.kappa[sh] * (eR ** 2).sum((1, 2)) + g.tau[sh] * (et ** 2).sum(1))).sum())
    return float(f)
