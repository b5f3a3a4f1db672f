"""Test infrastructure of the Riemannian staircase (kmx.dpgo.staircase): the
winding ring as a team graph (PoseGraphData, one robot or cut into several),
and dense numpy stand-ins for the Certifier (numpy.linalg.eigh, escape_point)
and an adapter of the CPU restatement of the solver (oracle.OraclePGO), so the
loop can run without a device. Small graphs only (everything is dense)."""
import numpy as np

from tests import cert_ref as CR


def ring_team(n, robots=1):
    """cert_ref.ring(n, 3) as a PoseGraphData of `robots` robots of n / robots
    consecutive poses each, and its stationary point by robot. Edges inside a
    robot between consecutive poses are odometry; the closing edge, and with
    several robots every edge that crosses two of them, is a loop closure."""
    from kmx.synth.pose_graph import PoseGraphData
    assert n % robots == 0
    per = n // robots
    gd, X = CR.ring(n, 3)
    src, dst = gd["src"].astype(np.int64), gd["dst"].astype(np.int64)
    r1, p1, r2, p2 = src // per, src % per, dst // per, dst % per
    fixed = ((r1 == r2) & (p2 == p1 + 1)).astype(np.uint8)
    eye = [np.tile(np.eye(3), (per, 1, 1)) for _ in range(robots)]
    zero = [np.zeros((per, 3)) for _ in range(robots)]
    g = PoseGraphData(n_robots=robots, n_poses=np.full(robots, per, np.int32), r1=r1.astype(np.int32),
                      p1=p1.astype(np.int32), r2=r2.astype(np.int32), p2=p2.astype(np.int32), R=gd["R"], t=gd["t"],
                      kappa=gd["kappa"], tau=gd["tau"], weight=gd["weight"], fixed=fixed,
                      outlier=np.zeros(n, bool), gt_R=eye, gt_t=zero, init_R=eye, init_t=zero)
    return g, {a: np.ascontiguousarray(X[a * per:(a + 1) * per]) for a in range(robots)}, gd


def f3(n):
    """The ring's cost tr(X Q X^T) at its rank-3 stationary point."""
    return 2.0 * n * (2.0 - 2.0 * np.cos(2.0 * np.pi / n))


def relative_rotations(R, src, dst):
    """R_i^T R_j over the edges."""
    return np.einsum("kji,kjl->kil", R[src], R[dst])


class NumpyCertifier:
    """Certifier's staircase surface on dense numpy: min_eig by eigh, escape by
    escape_point and tr(Z Q Z^T)."""

    def __init__(self):
        self.r = 0

    def set_graph(self, n, src, dst, R, t, kappa, tau, weight=None):
        self.n = n
        self.Q = CR.dense_Q(n, src, dst, R, t, kappa, tau, np.ones(len(src)) if weight is None else weight)

    def _cost(self, Z):
        F = CR.flat_X(Z)
        return float(np.trace(F @ self.Q @ F.T))

    def set_point(self, X):
        self.X, self.r = np.array(X, np.float64), X.shape[1]
        self.S = CR.dense_S(self.X, self.Q)
        self.info = CR.point_info(self.X, self.Q)
        return dict(self.info)

    def min_eig(self, eta, want_vector=False, **kw):
        ev, V = np.linalg.eigh(self.S)
        d = "NEGATIVE" if ev[0] < -eta else "CERTIFIED"
        out = {"decision": d, "steps": 0, "theta_min": float(ev[0]), "theta_max": float(ev[-1]), "residual": 0.0}
        if want_vector:
            out["y"] = V[:, 0].copy()
        return out

    def escape(self, y, alphas):
        from kmx.dpgo.certify import escape_point
        # alpha = 0 is [X; 0] itself, as the device has it (numpy's QR would move X by a rounding error)
        zero = np.concatenate([self.X, np.zeros((self.n, 1, 4))], axis=1)
        self.cand = [escape_point(self.X, y, a) if a != 0 else zero for a in alphas]
        cost = np.array([self._cost(Z) for Z in self.cand])
        ok = np.isfinite(cost) & (cost < self.info["cost"])
        best = int(np.flatnonzero(ok)[np.argmin(cost[ok])]) if ok.any() else -1
        return {"cost": cost, "best": best}

    def escape_commit(self, k):
        return self.cand[k], self.set_point(self.cand[k])

    def close(self):
        pass


def oracle_solver(P, g, device):
    """staircase_team's solver_factory over the CPU restatement."""
    from oracle.oracle import OraclePGO

    class _S(OraclePGO):
        refresh_local = OraclePGO.refresh

    return _S(P.to_c(), g)
