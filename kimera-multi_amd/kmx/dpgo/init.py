"""Distributed initialisation: robust alignment of each
robot's locally initialised trajectory to the global frame.

Reference flow (drawio:2271-2307, 2490-2510; images/system_arch.png "Global
Frame Estimation"): every robot first initialises its own block (odometry
chain / local solve) in its own frame; then, once a neighbour that is already
in the global frame publishes the poses at the ends of their shared loop
closures, the robot estimates the rigid transform between the two frames
from every such loop closure and fuses the candidates with GNC-TLS robust
single-pose averaging [U: dpgo's robustSinglePoseAveraging; restated from
the published GNC algorithm]. Robot 0 defines the global frame.

This is host-side control (O(#shared loop closures) per robot, once), like
the reference's.
"""
from __future__ import annotations

import numpy as np

from .params import error_threshold_at_quantile


def project_so3(M: np.ndarray) -> np.ndarray:
    U, _, Vt = np.linalg.svd(M)
    D = np.eye(3)
    D[2, 2] = np.sign(np.linalg.det(U @ Vt))
    return U @ D @ Vt


def single_pose_averaging(R, t, kappa, tau, w):
    """argmin_{R,t} sum_i w_i (kappa_i |R - R_i|_F^2 + tau_i |t - t_i|^2)."""
    Rm = project_so3(np.einsum("i,ijk->jk", w * kappa, R))
    wt = w * tau
    tm = (wt[:, None] * t).sum(0) / max(wt.sum(), 1e-300)
    return Rm, tm


def robust_single_pose_averaging(R, t, kappa, tau, *, barc: float | None = None, mu_step: float = 1.4,
                                 max_iters: int = 1000):
    """GNC-TLS robust averaging of SE(3) candidates (R_i, t_i) with precisions
    (kappa_i, tau_i). Returns (R, t, weights in [0, 1]).
    barc default: chi-square 0.999 quantile of SE(3)'s 6 dof (error_threshold_at_quantile): with
    dpgo's precisions kappa |dR|_F^2 is ~2x a chi-square(3) variable, so tighter quantiles reject
    inliers."""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    t = np.asarray(t, np.float64).reshape(-1, 3)
    n = R.shape[0]
    kappa = np.broadcast_to(np.asarray(kappa, np.float64), (n,)).copy()
    tau = np.broadcast_to(np.asarray(tau, np.float64), (n,)).copy()
    if n == 0:
        raise ValueError("no candidates")
    barc = error_threshold_at_quantile(0.999, 3) if barc is None else barc
    c2 = barc * barc
    w = np.ones(n)
    Rm, tm = single_pose_averaging(R, t, kappa, tau, w)
    if n == 1:
        return Rm, tm, w
    r2 = kappa * ((R - Rm) ** 2).sum((1, 2)) + tau * ((t - tm) ** 2).sum(1)
    mu = c2 / max(2.0 * r2.max() - c2, 1e-12)  # GNC-TLS initial mu (Yang et al. 2020)
    mu = max(mu, 1e-12)
    for _ in range(max_iters):
        lo, hi = mu / (mu + 1.0) * c2, (mu + 1.0) / mu * c2
        w_new = np.where(r2 <= lo, 1.0, np.where(r2 >= hi, 0.0, np.sqrt(c2 * mu * (mu + 1.0) / np.maximum(r2, 1e-300)) - mu))
        if w_new.sum() == 0:  # everything rejected: keep the best single candidate
            w_new = (r2 == r2.min()).astype(float)
        Rm, tm = single_pose_averaging(R, t, kappa, tau, w_new)
        r2 = kappa * ((R - Rm) ** 2).sum((1, 2)) + tau * ((t - tm) ** 2).sum(1)
        converged = np.all((w_new == 0.0) | (w_new == 1.0)) and np.array_equal(w_new, w)
        w = w_new
        if converged:
            break
        mu *= mu_step
    return Rm, tm, w


def alignment_candidates(shared_lcs, own_robot, own_R, own_t, nbr_global):
    """One candidate T_world_own per shared loop closure whose neighbour end is
    known in the world frame.

    shared_lcs: RelativeSEMeasurement-like objects ((r1, p1) -> (r2, p2), R, t,
    kappa, tau) with T_{r1,p1}^{-1} T_{r2,p2} = (R, t).
    own_R / own_t: this robot's trajectory in its own frame ([n, 3, 3], [n, 3]).
    nbr_global: {(robot, pose): (R, t)} neighbour poses in the world frame."""
    Rs, ts, ks, taus = [], [], [], []
    for m in shared_lcs:
        if m.r1 == own_robot and (m.r2, m.p2) in nbr_global:
            # T_W_own(p1) = T_W_nbr(p2) meas^{-1};  T_W_A = T_W_own(p1) T_A_own(p1)^{-1}
            Rn, tn = nbr_global[(m.r2, m.p2)]
            Rw = Rn @ m.R.T
            tw = tn - Rw @ m.t
            Ra, ta = own_R[m.p1], own_t[m.p1]
        elif m.r2 == own_robot and (m.r1, m.p1) in nbr_global:
            # T_W_own(p2) = T_W_nbr(p1) meas
            Rn, tn = nbr_global[(m.r1, m.p1)]
            Rw = Rn @ m.R
            tw = tn + Rn @ m.t
            Ra, ta = own_R[m.p2], own_t[m.p2]
        else:
            continue
        R_WA = Rw @ Ra.T
        Rs.append(R_WA)
        ts.append(tw - R_WA @ ta)
        ks.append(m.kappa)
        taus.append(m.tau)
    return np.array(Rs).reshape(-1, 3, 3), np.array(ts).reshape(-1, 3), np.array(ks), np.array(taus)


def align_to_world(shared_lcs, own_robot, own_R, own_t, nbr_global, **kw):
    """Robust T_world_own = (R, t) and the per-loop-closure inlier weights."""
    Rs, ts, ks, taus = alignment_candidates(shared_lcs, own_robot, own_R, own_t, nbr_global)
    if Rs.shape[0] == 0:
        return None
    return robust_single_pose_averaging(Rs, ts, ks, taus, **kw)


def transform_trajectory(R_WA, t_WA, R, t):
    """Express a trajectory given in frame A in the world frame."""
    return np.einsum("ij,njk->nik", R_WA, R), t @ R_WA.T + t_WA


def chordal_initialization(n: int, edges, anchor: int = 0):
    """Local chordal initialisation of one robot's trajectory (SURVEY.md §8
    row D10; dpgo's local initialisation method Chordal [U: restated from the
    SE-Sync chordal relaxation it uses]).

    edges: iterable of (i, j, R_ij [3x3], t_ij [3], kappa, tau, weight) for the
    robot's own measurements (odometry and private loop closures), with
    R_j = R_i R_ij and t_j = t_i + R_i t_ij. Step 1 minimises
    sum w kappa |R_j - R_i R_ij|_F^2 over unconstrained 3x3 blocks with
    R_anchor = I (sparse normal equations), then projects every block to SO(3);
    step 2 minimises sum w tau |t_j - t_i - R_i t_ij|^2 with t_anchor = 0 for
    the rotations of step 1. Returns (R [n,3,3], t [n,3])."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    E = list(edges)
    if n == 1:
        return np.eye(3)[None], np.zeros((1, 3))
    free = np.array([k for k in range(n) if k != anchor])
    col = -np.ones(n, np.int64)
    col[free] = np.arange(n - 1)
    # rotations: unknowns are the 3x3 blocks of the free poses, row-major, and
    # every edge gives R_j - R_i R_ij = 0, i.e. for each row a of R:
    # R_j[a, :] - R_i[a, :] R_ij = 0 (3 equations per row, same structure per row)
    # row a of every block is an independent problem with the same matrix:
    # s (R_j[a, c] - sum_b R_i[a, b] R_ij[b, c]) = 0 for c = 0..2; the anchor's
    # known row (R_anchor = I) moves to the right-hand side
    rows, cols, vals, rhs = [], [], [], []
    r = 0
    for (i, j, Rij, _t, kap, _tau, w) in E:
        s = np.sqrt(max(w * kap, 0.0))
        Rij = np.asarray(Rij, np.float64)
        for c in range(3):
            if col[j] >= 0:
                rows.append(r); cols.append(3 * col[j] + c); vals.append(s)
            if col[i] >= 0:
                for b in range(3):
                    rows.append(r); cols.append(3 * col[i] + b); vals.append(-s * Rij[b, c])
            rhs.append((c, i, j, s, Rij))
            r += 1
    A = sp.csr_matrix((vals, (rows, cols)), shape=(r, 3 * (n - 1)))
    AtA = (A.T @ A).tocsc()
    solve = spla.factorized(AtA)
    Rs = np.zeros((n, 3, 3))
    Rs[anchor] = np.eye(3)
    for a in range(3):  # one solve per row of the rotation blocks, same matrix
        bvec = np.zeros(r)
        for k, (c, i, j, s, Rij) in enumerate(rhs):
            v = 0.0
            if i == anchor:
                v += s * Rij[a, c]
            if j == anchor:
                v -= s * (1.0 if a == c else 0.0)
            bvec[k] = v
        x = solve(A.T @ bvec)
        Rs[free, a, :] = x.reshape(n - 1, 3)
    for k in free:
        Rs[k] = project_so3(Rs[k])
    # translations
    rows, cols, vals, b = [], [], [], []
    r = 0
    for (i, j, Rij, tij, _kap, tau, w) in E:
        s = np.sqrt(max(w * tau, 0.0))
        d = Rs[i] @ np.asarray(tij, np.float64)
        for c in range(3):
            if col[j] >= 0:
                rows.append(r); cols.append(3 * col[j] + c); vals.append(s)
            if col[i] >= 0:
                rows.append(r); cols.append(3 * col[i] + c); vals.append(-s)
            b.append(s * d[c])
            r += 1
    A = sp.csr_matrix((vals, (rows, cols)), shape=(r, 3 * (n - 1)))
    x = spla.spsolve((A.T @ A).tocsc(), A.T @ np.asarray(b))
    ts = np.zeros((n, 3))
    ts[free] = np.asarray(x).reshape(n - 1, 3)
    return Rs, ts


def _edge_arrays(edges):
    E = list(edges)
    m = len(E)
    src = np.array([e[0] for e in E], np.int64).reshape(m)
    dst = np.array([e[1] for e in E], np.int64).reshape(m)
    R = np.array([np.asarray(e[2], np.float64) for e in E], np.float64).reshape(m, 3, 3)
    t = np.array([np.asarray(e[3], np.float64) for e in E], np.float64).reshape(m, 3)
    kap = np.array([e[4] for e in E], np.float64).reshape(m)
    tau = np.array([e[5] for e in E], np.float64).reshape(m)
    w = np.array([e[6] for e in E], np.float64).reshape(m)
    return src, dst, R, t, kap, tau, w


def chordal_initialization_gpu(n: int, edges, anchor: int = 0, R_init=None, t_init=None, *, device: int = 0,
                               return_info: bool = False, **solver_kw):
    """chordal_initialization on the device (kmx.dpgo.chordal.ChordalSolver,
    DESIGN.md §14): the same arguments, the same problem and the same return
    values, the two linear systems solved by preconditioned conjugate
    gradients to solver_kw's rtol (default 1e-10) instead of a sparse
    factorisation. R_init / t_init: the start vectors ([n,3,3], [n,3]; None:
    zero), e.g. the odometry chain. There is no CPU fallback.

    Like the host function this is an L2 method: loop closures that are
    outliers pull at full weight, and the result can then be worse than the
    odometry chain; robust_chordal_initialization_gpu is the robust form."""
    from .chordal import ChordalSolver
    src, dst, R, t, kap, tau, w = _edge_arrays(edges)
    s = ChordalSolver(device)
    try:
        s.set_graph(n, [0, n], src, dst, R, t, kap, tau, w, anchors=[anchor])
        Rs, ts, info = s.solve(R_init, t_init, **solver_kw)
    finally:
        s.close()
    return (Rs, ts, info) if return_info else (Rs, ts)


def chordal_initialization_team(g, weights=None, *, device: int = 0, return_info: bool = False, **solver_kw):
    """Chordal initialisation of every robot of the team graph g
    (kmx.synth.PoseGraphData) in one batch on the device: each robot's private
    measurements (r1 == r2) form one block, pose 0 of each robot is its anchor
    (every robot in its own frame), and the start vector is the robot's
    odometry chain g.init_R / g.init_t relative to its pose 0. weights: per
    edge of g ([g.m]; None: g.weight). Returns (list of R [n_a,3,3], list of
    t [n_a,3]) per robot, and the per-robot solver info with return_info.
    An L2 method: see chordal_initialization_gpu; under outliers use
    robust_chordal_initialization_team."""
    from .chordal import ChordalSolver
    n_poses = np.asarray(g.n_poses, np.int64)
    ptr = np.concatenate([[0], np.cumsum(n_poses)])
    own = np.nonzero(g.r1 == g.r2)[0]
    w = np.asarray(g.weight if weights is None else weights, np.float64)
    if w.shape != (g.m,):
        raise ValueError(f"weights: expected shape ({g.m},), got {w.shape}")
    off = ptr[g.r1[own]]
    R0, t0 = [], []
    for a in range(g.n_robots):
        Ra, ta = np.asarray(g.init_R[a], np.float64), np.asarray(g.init_t[a], np.float64)
        R0.append(np.einsum("ij,njk->nik", Ra[0].T, Ra))
        t0.append((ta - ta[0]) @ Ra[0])
    n = int(ptr[-1])
    s = ChordalSolver(device)
    try:
        s.set_graph(n, ptr, off + g.p1[own], off + g.p2[own], g.R[own], g.t[own], g.kappa[own], g.tau[own], w[own],
                    anchors=ptr[:-1][n_poses > 0])
        Rs, ts, info = s.solve(np.concatenate(R0).reshape(n, 3, 3), np.concatenate(t0).reshape(n, 3), **solver_kw)
    finally:
        s.close()
    Rl = [Rs[ptr[a]:ptr[a + 1]] for a in range(g.n_robots)]
    tl = [ts[ptr[a]:ptr[a + 1]] for a in range(g.n_robots)]
    return (Rl, tl, info) if return_info else (Rl, tl)


# ---- robust chordal initialisation: GNC-TLS around the chordal solve

def measurement_errors(src, dst, R, t, kappa, tau, Rs, ts):
    """dpgo's computeMeasurementError [U] for every edge at the poses (Rs, ts):
    r^2 = kappa |R_j - R_i R_ij|_F^2 + tau |t_j - t_i - R_i t_ij|^2."""
    dR = Rs[dst] - np.einsum("eab,ebc->eac", Rs[src], R)
    dt = ts[dst] - ts[src] - np.einsum("eab,eb->ea", Rs[src], t)
    return kappa * (dR ** 2).sum((1, 2)) + tau * (dt ** 2).sum(1)


def gnc_tls_factor(r2, mu: float, c2: float):
    """The GNC-TLS factor of every residual for one mu (Yang et al. 2020,
    "Graduated Non-Convexity for Robust Spatial Perception"): 1 for
    r^2 <= mu/(mu+1) c^2, 0 for r^2 >= (mu+1)/mu c^2, sqrt(c^2 mu (mu+1) / r^2)
    - mu in between. Returns (g, fractional mask); the operations are in the
    order chordal.hip states them."""
    r2 = np.asarray(r2, np.float64)
    lo, hi = mu / (mu + 1.0) * c2, (mu + 1.0) / mu * c2
    one, zero = r2 <= lo, (r2 >= hi) & ~(r2 <= lo)
    frac = ~one & ~zero
    g = np.where(one, 1.0, 0.0)
    g[frac] = np.sqrt(c2 * mu * (mu + 1.0) / r2[frac]) - mu
    return g, frac


def robust_chordal_initialization(n: int, edges, fixed, anchor: int = 0, *, barc: float = 5.0, mu_init: float = 0.0,
                                  mu_step: float = 1.4, max_updates: int = 100, return_info: bool = False):
    """Robust local chordal initialisation of one robot's trajectory: GNC-TLS
    around chordal_initialization (dpgo's robust local initialisation [U: dpgo
    is not vendored; restated from the published GNC algorithm]). This is the
    host mirror of kmx_chordal_solve_robust (chordal.hip): the
    same rule around the host's direct solve, the reference of the device's
    tests.

    edges as chordal_initialization's; fixed [m]: the edges that keep their
    weight (the odometry; they must connect every pose to the anchor by
    themselves). Every other edge of weight w0 > 0 enters a solve with w0 g:
      1. solve at g = 1; r^2 of every edge (measurement_errors).
      2. mu_0 = mu_init, or (mu_init = 0) c^2 / (2 max r^2 - c^2) over the
         counted edges (Yang et al. 2020); with 2 max r^2 <= c^2 nothing can be
         an outlier: done, 0 updates.
      3. g = gnc_tls_factor(r^2, mu). Done (converged) when every g is 0 or 1
         and none differs from the g of the last solve.
      4. Otherwise solve with w0 g (an update), new r^2, mu <- mu mu_step, and
         back to 3; after max_updates updates it stops as it is.
    Returns (R [n,3,3], t [n,3], g [m], updates), and with return_info a dict
    (converged, mu, n_kept, n_rejected, n_fractional) as a fifth value."""
    src, dst, Rm, tm, kap, tau, w0 = _edge_arrays(edges)
    m = src.shape[0]
    fixed = np.asarray(fixed).astype(bool).reshape(m)
    counted = ~fixed & (w0 > 0)
    c2 = float(barc) * float(barc)
    E = list(edges)

    def solve(g):
        w = w0 * g
        return chordal_initialization(n, [(e[0], e[1], e[2], e[3], e[4], e[5], w[k])
                                          for k, e in enumerate(E) if w[k] > 0], anchor)

    g = np.ones(m)
    frac = np.zeros(m, bool)
    Rs, ts = solve(g)
    r2 = measurement_errors(src, dst, Rm, tm, kap, tau, Rs, ts)
    mx = float(r2[counted].max()) if counted.any() else 0.0
    updates, converged, mu = 0, False, 0.0
    if mu_init > 0:
        mu_next = float(mu_init)
    elif 2.0 * mx <= c2:
        converged, mu_next = True, 0.0
    else:
        mu_next = c2 / (2.0 * mx - c2)
    while not converged:
        mu = mu_next
        g_new, frac = gnc_tls_factor(r2, mu, c2)
        g_new[fixed] = 1.0
        frac = frac & ~fixed
        changed = bool((g_new[counted] != g[counted]).any())
        g = g_new
        if not frac[counted].any() and not changed:
            converged = True
            break
        Rs, ts = solve(g)
        updates += 1
        if updates >= max_updates:
            break
        r2 = measurement_errors(src, dst, Rm, tm, kap, tau, Rs, ts)
        mu_next = mu * mu_step
    if not return_info:
        return Rs, ts, g, updates
    info = {"converged": converged, "mu": mu, "n_kept": int((counted & ~frac & (g == 1.0)).sum()),
            "n_rejected": int((counted & ~frac & (g == 0.0)).sum()), "n_fractional": int((counted & frac).sum())}
    return Rs, ts, g, updates, info


def robust_chordal_initialization_gpu(n: int, edges, fixed, anchor: int = 0, R_init=None, t_init=None, *,
                                      barc: float = 5.0, mu_init: float = 0.0, mu_step: float = 1.4,
                                      max_updates: int = 100, device: int = 0, return_info: bool = False,
                                      **solver_kw):
    """robust_chordal_initialization on the device
    (ChordalSolver.solve_robust, kmx_chordal_solve_robust): the same
    arguments and the same rule, the solves by warm-started preconditioned
    conjugate gradients, the residuals, weights, mu and the stop test on the
    device. Returns (R, t, g, updates), and with return_info the solver's
    info and rinfo of the one block as well. There is no CPU fallback."""
    from .chordal import ChordalSolver
    src, dst, R, t, kap, tau, w = _edge_arrays(edges)
    s = ChordalSolver(device)
    try:
        s.set_graph(n, [0, n], src, dst, R, t, kap, tau, w, anchors=[anchor])
        Rs, ts, g, info, rinfo = s.solve_robust(fixed, R_init, t_init, barc=barc, mu_init=mu_init, mu_step=mu_step,
                                                max_updates=max_updates, **solver_kw)
    finally:
        s.close()
    if return_info:
        return Rs, ts, g, rinfo[0]["updates"], info[0], rinfo[0]
    return Rs, ts, g, rinfo[0]["updates"]


def robust_chordal_initialization_team(g, weights=None, *, min_inliers: int = 0, barc: float = 5.0,
                                       mu_init: float = 0.0, mu_step: float = 1.4, max_updates: int = 100,
                                       device: int = 0, return_info: bool = False, **solver_kw):
    """Robust chordal initialisation of every robot of the team graph g in one
    batch on the device: blocks, anchors and the odometry start as in
    chordal_initialization_team, fixed = g.fixed (the odometry), every robot
    with a mu, an update count and a stop test of its own. A robot that keeps
    fewer than min_inliers loop closures gets its odometry chain (dpgo's
    robustInitMinInliers [U]). Returns (list of R, list of t, list of g over
    the robot's private edges in g's order), and the per-robot info and rinfo
    with return_info."""
    from .chordal import ChordalSolver
    n_poses = np.asarray(g.n_poses, np.int64)
    ptr = np.concatenate([[0], np.cumsum(n_poses)])
    own = np.nonzero(g.r1 == g.r2)[0]
    w = np.asarray(g.weight if weights is None else weights, np.float64)
    if w.shape != (g.m,):
        raise ValueError(f"weights: expected shape ({g.m},), got {w.shape}")
    off = ptr[g.r1[own]]
    R0, t0 = [], []
    for a in range(g.n_robots):
        Ra, ta = np.asarray(g.init_R[a], np.float64), np.asarray(g.init_t[a], np.float64)
        R0.append(np.einsum("ij,njk->nik", Ra[0].T, Ra))
        t0.append((ta - ta[0]) @ Ra[0])
    n = int(ptr[-1])
    s = ChordalSolver(device)
    try:
        s.set_graph(n, ptr, off + g.p1[own], off + g.p2[own], g.R[own], g.t[own], g.kappa[own], g.tau[own], w[own],
                    anchors=ptr[:-1][n_poses > 0])
        Rs, ts, gf, info, rinfo = s.solve_robust(
            np.asarray(g.fixed)[own] != 0, np.concatenate(R0).reshape(n, 3, 3), np.concatenate(t0).reshape(n, 3),
            barc=barc, mu_init=mu_init, mu_step=mu_step, max_updates=max_updates, **solver_kw)
    finally:
        s.close()
    Rl, tl, gl = [], [], []
    for a in range(g.n_robots):
        keep = rinfo[a]["n_kept"] >= min_inliers
        Rl.append(Rs[ptr[a]:ptr[a + 1]] if keep else R0[a])
        tl.append(ts[ptr[a]:ptr[a + 1]] if keep else t0[a])
        gl.append(gf[g.r1[own] == a])
    return (Rl, tl, gl, info, rinfo) if return_info else (Rl, tl, gl)
