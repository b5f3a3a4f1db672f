"""An independent reference of one robot's RTR block update (numpy, float64, dense).

The restatement (oracle/dpgo_oracle.c) is written line by line like the
kernels; a mistake both share in the boundary step tau, in the radius rule or
in the acceptance rule would pass every kernel-against-restatement test. This
module states the same update from the mathematics instead, with the robot's
neighbours held fixed:

  f(X)   = 1/2 sum_e w (kappa |Y_j - Y_i R|^2 + tau |p_j - p_i - Y_i t|^2)
         = 1/2 <X Q, X> + <X, B> + const     (X: r x 4n, Q: 4n x 4n dense)
  grad   = P_X(X Q + B),   Hess[V] = P_X(V Q - V sym(Y^T (XQ + B)_Y))
  P_X    : per pose, Z_Y - Y sym(Y^T Z_Y) on the rotation block (Stiefel)
  precon : per pose, V_i (Q_ii + shift I)^-1, projected
  tCG    : Steihaug-Toint (Conn, Gould, Toint, Trust-Region Methods, Alg.
           7.5.1; stopping rule of Absil, Baker, Gallivan 2007)
  Retr   : per pose, the Q factor of Y + V_Y with a positive diagonal of R
  rho    = (f(X) - f(Retr(eta))) / -(<eta, grad> + 1/2 <eta, Hess[eta]>)
  radius : x 1/4 if not rho >= 1/4; min(2 radius, max) if rho > 3/4 on the
           boundary; accepted if rho > accept_rho

Dense linear algebra (np.linalg.inv, np.linalg.qr, matrix products), no
recurrence for H eta, no per-incidence loops: nothing of the restatement's
program text. Every decision's margin is returned, so a caller can require
that no decision of its input sits on a threshold.
"""
import numpy as np


def numpy_block(g, X, a, V=None, hess=False):
    """Independent restatement: f = 1/2 sum_e w(k|Y_j - Y_i R|^2 + t|p_j - p_i - Y_i t|^2)."""
    off = np.concatenate([[0], np.cumsum(g.n_poses)])
    allX = np.concatenate([X[b] for b in range(g.n_robots)])
    Vb = X[a] if V is None else V
    sel = (g.r1 == a) | (g.r2 == a)
    e = np.nonzero(sel)[0]
    gi, gj = off[g.r1[e]] + g.p1[e], off[g.r2[e]] + g.p2[e]
    Xi, Xj = allX[gi].copy(), allX[gj].copy()
    ti, tj = g.r1[e] == a, g.r2[e] == a
    Xi[ti] = Vb[g.p1[e][ti]]
    Xj[tj] = Vb[g.p2[e][tj]]
    if hess:
        Xi[~ti] = 0.0
        Xj[~tj] = 0.0
    wk = (g.weight * g.kappa)[e][:, None, None]
    wt = (g.weight * g.tau)[e][:, None]
    ER = Xj[:, :, :3] - Xi[:, :, :3] @ g.R[e]
    Et = Xj[:, :, 3] - Xi[:, :, 3] - np.einsum("nac,nc->na", Xi[:, :, :3], g.t[e])
    cost = 0.5 * (np.sum(wk * ER ** 2) + np.sum(wt * Et ** 2))
    G = np.zeros_like(Vb)
    np.add.at(G, (g.p2[e][tj], slice(None), slice(0, 3)), (wk * ER)[tj])
    np.add.at(G, (g.p2[e][tj], slice(None), 3), (wt * Et)[tj])
    gi_Y = -(wk * np.einsum("nac,nkc->nak", ER, g.R[e])) - (wt * Et)[:, :, None] * g.t[e][:, None, :]
    np.add.at(G, (g.p1[e][ti], slice(None), slice(0, 3)), gi_Y[ti])
    np.add.at(G, (g.p1[e][ti], slice(None), 3), -(wt * Et)[ti])
    return cost, G


def _flat(X):
    """[n, r, 4] -> r x 4n."""
    return X.transpose(1, 0, 2).reshape(X.shape[1], -1)


def _unflat(M):
    return M.reshape(M.shape[0], -1, 4).transpose(1, 0, 2)


def quadratic(g, X, a):
    """Dense (Q [4n, 4n], B [r, 4n], c) of robot a's local cost with the other
    robots' poses fixed at X: f(M) = 1/2 <M Q, M> + <M, B> + c, M = _flat(X[a])."""
    n, r = int(g.n_poses[a]), X[a].shape[1]
    Q = np.zeros((4 * n, 4 * n))
    B = np.zeros((r, 4 * n))
    c = 0.0
    for e in np.nonzero((g.r1 == a) | (g.r2 == a))[0]:
        A = np.zeros((8, 4))  # the row [Y_i p_i Y_j p_j] times A: rotation (3) and translation residual
        A[0:3, 0:3] = -g.R[e]
        A[4:7, 0:3] = np.eye(3)
        A[0:3, 3] = -g.t[e]
        A[3, 3], A[7, 3] = -1.0, 1.0
        W = g.weight[e] * np.diag([g.kappa[e]] * 3 + [g.tau[e]])
        Qe = A @ W @ A.T
        ends = ((g.r1[e], g.p1[e]), (g.r2[e], g.p2[e]))
        for s, (rs, ps_) in enumerate(ends):
            for t, (rt, pt) in enumerate(ends):
                blk = Qe[4 * s:4 * s + 4, 4 * t:4 * t + 4]
                if rs == a and rt == a:
                    Q[4 * ps_:4 * ps_ + 4, 4 * pt:4 * pt + 4] += blk
                elif rs != a and rt == a:  # fixed row times the cross block: linear in the local row
                    B[:, 4 * pt:4 * pt + 4] += X[rs][ps_] @ blk
                elif rs != a and rt != a:
                    c += 0.5 * np.sum((X[rs][ps_] @ blk) * X[rt][pt])
    return Q, B, c


class Block:
    """Robot a's block problem at the team iterate X (neighbours fixed)."""

    def __init__(self, g, X, a, shift=0.1, use_preconditioner=True):
        self.g, self.a = g, a
        self.X = {b: np.array(X[b], dtype=np.float64) for b in X}
        self.Q, self.B, self.c = quadratic(g, self.X, a)
        self.n = int(g.n_poses[a])
        self.precond = use_preconditioner
        D = np.stack([self.Q[4 * i:4 * i + 4, 4 * i:4 * i + 4] for i in range(self.n)])
        self.Dinv = np.linalg.inv(D + shift * np.eye(4))

    def cost(self, Xa):
        X = dict(self.X)
        X[self.a] = Xa
        return numpy_block(self.g, X, self.a)[0]

    def egrad(self, Xa):
        return _unflat(_flat(Xa) @ self.Q + self.B)

    @staticmethod
    def proj(Xa, Z):
        Y = Xa[:, :, :3]
        S = np.einsum("nac,nak->nck", Y, Z[:, :, :3])
        S = 0.5 * (S + S.transpose(0, 2, 1))
        T = Z.copy()
        T[:, :, :3] -= Y @ S
        return T

    def rhess(self, Xa, G, V):
        """Riemannian Hessian at Xa (Euclidean gradient G) applied to a tangent V."""
        S = np.einsum("nac,nak->nck", Xa[:, :, :3], G[:, :, :3])
        S = 0.5 * (S + S.transpose(0, 2, 1))
        H = _unflat(_flat(V) @ self.Q)
        H[:, :, :3] -= V[:, :, :3] @ S
        return self.proj(Xa, H)

    def precon(self, Xa, V):
        return self.proj(Xa, V @ self.Dinv) if self.precond else V.copy()

    @staticmethod
    def retract(Xa, V):
        out = Xa + V
        for i in range(Xa.shape[0]):
            q, rr = np.linalg.qr(out[i, :, :3])
            out[i, :, :3] = q * np.sign(np.diag(rr))
        return out


def _rel(x, y):
    """Distance of x from the threshold y relative to their scale."""
    return abs(x - y) / max(abs(x), abs(y), np.finfo(float).tiny)


def rtr_step(g, X, a, *, radius, max_radius, accept_rho=0.1, tcg_max=10, kappa=0.1, theta=1.0, shift=0.1,
             use_preconditioner=True):
    """One RTR iteration of robot a's block update from the team iterate X.
    Returns the decisions (stop, tcg_iterations, accepted, radius), rho, the
    costs, the trial point Xt, the new iterate, and `margins`: for every
    decision taken, how far it was from going the other way, relative to scale."""
    P = Block(g, X, a, shift, use_preconditioner)
    Xa = P.X[a]
    ip = lambda U, V: float(np.sum(U * V))  # noqa: E731
    f = P.cost(Xa)
    G = P.egrad(Xa)
    grad = P.proj(Xa, G)
    margins = {"curvature": [], "boundary": [], "residual": [], "rho": None}
    eta = np.zeros_like(Xa)
    r = grad.copy()
    norm_r0 = np.sqrt(ip(r, r))
    r_stop = norm_r0 * min(norm_r0 ** theta, kappa)
    z = P.precon(Xa, r)
    z_r = ip(z, r)
    delta = -z
    e_Pe, e_Pd, d_Pd = 0.0, 0.0, z_r
    stop, j = "max_iterations", 0
    for j in range(1, tcg_max + 1):
        Hd = P.rhess(Xa, G, delta)
        d_Hd = ip(delta, Hd)
        margins["curvature"].append(abs(d_Hd) / (np.sqrt(ip(delta, delta)) * np.sqrt(ip(Hd, Hd))))
        alpha = z_r / d_Hd
        e_Pe_new = e_Pe + 2.0 * alpha * e_Pd + alpha * alpha * d_Pd
        if d_Hd > 0.0:
            margins["boundary"].append(_rel(e_Pe_new, radius ** 2))
        if d_Hd <= 0.0 or e_Pe_new >= radius ** 2:
            # the positive root of |eta + tau delta|_P = radius
            tau = (-e_Pd + np.sqrt(e_Pd ** 2 + d_Pd * (radius ** 2 - e_Pe))) / d_Pd
            eta = eta + tau * delta
            stop = "negative_curvature" if d_Hd <= 0.0 else "exceeded_trust_region"
            break
        e_Pe = e_Pe_new
        eta = eta + alpha * delta
        r = r + alpha * Hd
        norm_r = np.sqrt(ip(r, r))
        margins["residual"].append(_rel(norm_r, r_stop))
        if norm_r <= r_stop:
            stop = "linear" if kappa < norm_r0 ** theta else "superlinear"
            break
        if j == tcg_max:
            break
        z = P.precon(Xa, r)
        z_r, z_r_old = ip(z, r), z_r
        beta = z_r / z_r_old
        delta = -z + beta * delta
        e_Pd = beta * (e_Pd + alpha * d_Pd)
        d_Pd = z_r + beta * beta * d_Pd
    Xt = P.retract(Xa, eta)
    ft = P.cost(Xt)
    model_dec = -(ip(eta, grad) + 0.5 * ip(eta, P.rhess(Xa, G, eta)))
    rho = (f - ft) / model_dec if model_dec > 0.0 else -1.0
    new_radius = radius
    if not rho >= 0.25:
        new_radius = 0.25 * radius
    elif rho > 0.75 and stop in ("negative_curvature", "exceeded_trust_region"):
        new_radius = min(2.0 * radius, max_radius)
    accepted = rho > accept_rho
    margins["rho"] = min(abs(rho - t) / max(1.0, abs(rho)) for t in (0.25, 0.75, accept_rho))
    margins["model_decrease"] = model_dec / (abs(ip(eta, grad)) + 1e-300)
    return {"tcg_stop": stop, "tcg_iterations": j, "accepted": int(accepted), "radius": new_radius, "rho": rho,
            "f_init": f, "f_trial": ft, "gradnorm_init": norm_r0, "Xt": Xt, "X": Xt if accepted else Xa,
            "margins": margins}
