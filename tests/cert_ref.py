"""Dense numpy restatement of the dual certificate (cert.hip):
the connection Laplacian Q of a flattened team graph, Lambda(X), S = Q - Lambda,
the Lanczos start vector, plain Lanczos on S and the decision rule. Test
infrastructure: small graphs only (everything is dense)."""
import numpy as np

MASK = (1 << 64) - 1


def dense_Q(n, src, dst, R, t, kappa, tau, w):
    Q = np.zeros((4 * n, 4 * n))
    for e in range(len(src)):
        i, j = int(src[e]), int(dst[e])
        ka, ta, te = float(kappa[e]), float(tau[e]), np.asarray(t[e], float)
        A = np.zeros((4, 4))
        A[:3, :3] = ka * np.eye(3) + ta * np.outer(te, te)
        A[:3, 3] = A[3, :3] = ta * te
        A[3, 3] = ta
        B = np.diag([ka, ka, ka, ta])
        Cm = np.zeros((4, 4))
        Cm[:3, :3] = ka * np.asarray(R[e], float)
        Cm[:3, 3] = ta * te
        Cm[3, 3] = ta
        ii, jj = slice(4 * i, 4 * i + 4), slice(4 * j, 4 * j + 4)
        Q[ii, ii] += w[e] * A
        Q[jj, jj] += w[e] * B
        Q[ii, jj] -= w[e] * Cm
        Q[jj, ii] -= w[e] * Cm.T
    return Q


def flat_X(X):
    """[n, r, 4] -> r x 4n (pose i in columns 4i .. 4i+3)."""
    n, r, _ = X.shape
    return np.ascontiguousarray(X.transpose(1, 0, 2).reshape(r, 4 * n))


def lambda_blocks(X, Q):
    """Lambda_i = sym(Y_i^T (X Q)_{i,Y}) [n, 3, 3]."""
    n = X.shape[0]
    G = (flat_X(X) @ Q).reshape(X.shape[1], n, 4).transpose(1, 0, 2)  # [n, r, 4]
    M = np.einsum("nac,nad->ncd", X[:, :, :3], G[:, :, :3])
    return 0.5 * (M + M.transpose(0, 2, 1))


def lambda_bound(X, Q, termwise=False):
    """|Y_i^T| |(X Q)_{i,Y}|, symmetrised like Lambda ([n, 3, 3]). termwise:
    |X| |Q| in place of |X Q|, the bound of a point where X Q itself cancels
    (a stationary point of a noise-free graph has X Q = 0)."""
    n = X.shape[0]
    G = np.abs(flat_X(X)) @ np.abs(Q) if termwise else np.abs(flat_X(X) @ Q)
    G = G.reshape(X.shape[1], n, 4).transpose(1, 0, 2)
    M = np.einsum("nac,nad->ncd", np.abs(X[:, :, :3]), G[:, :, :3])
    return 0.5 * (M + M.transpose(0, 2, 1))


def dense_S(X, Q):
    S = Q.copy()
    L = lambda_blocks(X, Q)
    for i in range(X.shape[0]):
        S[4 * i:4 * i + 3, 4 * i:4 * i + 3] -= L[i]
    return S


def point_info(X, Q):
    Xf = flat_X(X)
    S = dense_S(X, Q)
    return {"cost": float(np.trace(Xf @ Q @ Xf.T)), "trace_lambda": float(np.trace(Q - S)),
            "stationarity": float(np.linalg.norm(Xf @ S))}


def start_vector(seed, count):
    """z = seed + (i+1) 0x9E3779B97F4A7C15 mod 2^64, the splitmix64 finaliser,
    u_i = (z >> 11) 2^-52 - 1 (not normalised)."""
    out = np.empty(count)
    for i in range(count):
        z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & MASK
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        z = z ^ (z >> 31)
        out[i] = float(z >> 11) * 2.0 ** -52 - 1.0
    return out


def lanczos(S, k, seed):
    """k steps of plain Lanczos from the start vector -> (alpha [k], beta [k])."""
    v = start_vector(seed, S.shape[0])
    v /= np.linalg.norm(v)
    vp = np.zeros_like(v)
    b = 0.0
    al, be = [], []
    for _ in range(k):
        w = S @ v - b * vp
        a = float(v @ w)
        w -= a * v
        b = float(np.linalg.norm(w))
        al.append(a)
        be.append(b)
        if b == 0.0:
            break
        vp, v = v, w / b
    return np.array(al), np.array(be)


def lanczos_steps(S, seed):
    """The same iteration one step at a time: yields (alpha_j, beta_j, v_j)
    with v_j the unit vector step j started from, for as long as the caller
    asks (after beta = 0 it yields zeros)."""
    v = start_vector(seed, S.shape[0])
    v /= np.linalg.norm(v)
    vp = np.zeros_like(v)
    b = 0.0
    while True:
        w = S @ v - b * vp
        a = float(v @ w)
        w -= a * v
        b = float(np.linalg.norm(w))
        yield a, b, v
        vp, v = v, (w / b if b > 0.0 else np.zeros_like(w))


# CERTIFIED needs rho <= CERT_C eta (cert_host.h: CT_RESIDUAL_FACTOR): the
# largest of CERT_C_CANDIDATES with no false certificate on family F (below;
# tests/test_cert_sound_cpu.py).
CERT_C_CANDIDATES = (1.0, 0.5, 0.25, 0.1, 0.01)
CERT_C = 0.1


def rule(theta_min, rho, eta, c=CERT_C):
    if theta_min < -eta:
        return "NEGATIVE"
    if rho <= c * eta and theta_min - rho >= -eta:
        return "CERTIFIED"
    return "UNDECIDED"


def ritz(alpha, beta, eta, c=CERT_C, vector=False):
    """The rule on the first k = len(alpha) steps, with numpy.linalg.eigh.
    vector: also "s", the unit eigenvector of theta_min in the tridiagonal."""
    k = len(alpha)
    T = np.diag(alpha) + np.diag(beta[:k - 1], 1) + np.diag(beta[:k - 1], -1)
    ev, V = np.linalg.eigh(T)
    rho = abs(beta[k - 1] * V[k - 1, 0])
    out = {"decision": rule(ev[0], rho, eta, c), "steps": k, "theta_min": float(ev[0]), "theta_max": float(ev[-1]),
           "residual": float(rho)}
    if vector:
        out["s"] = V[:, 0].copy()
    return out


def scan(S, eta, seed, max_steps, test_every, c=CERT_C, tests=None):
    """Lanczos with the rule applied as cert_scan_step applies it: in step
    order, at multiples of test_every, at a breakdown (beta <= 1e-14 of the
    running bound of |T|) and at the last step (which decides only if it is a
    multiple of test_every). -> ritz()'s result with "alpha", "beta" (the steps
    taken), "breakdown", and the unit Ritz vector "y" = V s / |V s| with its
    "true_residual" |S y - theta_min y|; the basis is kept for that.
    tests (a list): gets a copy of that result, without the coefficients, for
    every application of the rule."""
    al, be, V = [], [], []
    scale = 0.0
    res = None
    for a, b, v in lanczos_steps(S, seed):
        al.append(a)
        be.append(b)
        V.append(v)
        j = len(al)
        scale = max(scale, abs(a) + b + (be[-2] if j > 1 else 0.0))
        brk = b <= 1e-14 * scale
        last = j == max_steps
        if not (brk or last or j % test_every == 0):
            continue
        res = ritz(np.array(al), np.array(be), eta, c, vector=True)
        y = np.array(V).T @ res.pop("s")
        y /= np.linalg.norm(y)
        res.update(y=y, true_residual=float(np.linalg.norm(S @ y - res["theta_min"] * y)), breakdown=bool(brk),
                   decides=bool(brk or j % test_every == 0))
        if not res["decides"]:  # the last step, not a test step: reported, not decided
            res["decision"] = "UNDECIDED"
        if tests is not None:
            tests.append(dict(res))
        if brk or last or res["decision"] != "UNDECIDED":
            break
    res.update(alpha=np.array(al), beta=np.array(be))
    return res


def first_decision(tests, eta, c):
    """What scan(..., c) returns, read from the tests a scan with a smaller c
    recorded: the runs are the same up to c's decision. -> (decision, steps)."""
    for t in tests:
        d = rule(t["theta_min"], t["residual"], eta, c) if t["decides"] else "UNDECIDED"
        if d != "UNDECIDED" or t["breakdown"]:
            return d, t["steps"]
    return "UNDECIDED", tests[-1]["steps"]


def random_rotations(rng, k):
    q, r = np.linalg.qr(rng.standard_normal((k, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 2] *= np.linalg.det(q)[:, None]
    return q


def random_graph(n, m, seed, *, chain=True):
    """A connected random graph of n poses: a chain plus m random edges."""
    rng = np.random.default_rng(seed)
    src = list(range(n - 1)) if chain else []
    dst = list(range(1, n)) if chain else []
    while n > 1 and len(src) < (n - 1 if chain else 0) + m:
        i, j = (int(x) for x in rng.integers(0, n, 2))
        if i != j:
            src.append(i)
            dst.append(j)
    k = len(src)
    return dict(n_poses=n, src=np.array(src, np.int32), dst=np.array(dst, np.int32), R=random_rotations(rng, k),
                t=rng.standard_normal((k, 3)), kappa=rng.uniform(0.5, 3.0, k), tau=rng.uniform(0.5, 3.0, k),
                weight=rng.uniform(0.2, 1.5, k))


def consistent_graph(n, m, r, seed):
    """random_graph with noise-free measurements of random absolute poses, and
    the lifted ground truth X [n, r, 4]: S is positive semidefinite with the
    rows of X in its kernel."""
    g = random_graph(n, m, seed)
    rng = np.random.default_rng(seed + 5)
    Ra, ta = random_rotations(rng, n), rng.standard_normal((n, 3))
    i, j = g["src"], g["dst"]
    g["R"] = np.einsum("kji,kjl->kil", Ra[i], Ra[j])
    g["t"] = np.einsum("kji,kj->ki", Ra[i], ta[j] - ta[i])
    YL, _ = np.linalg.qr(rng.standard_normal((r, 3)))
    X = np.empty((n, r, 4))
    X[:, :, :3] = np.einsum("ad,ndc->nac", YL, Ra)
    X[:, :, 3] = ta @ YL.T
    return g, X


def random_point(n, r, seed):
    """X [n, r, 4] with orthonormal Y_i."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((n, r, 3)))
    X = np.empty((n, r, 4))
    X[:, :, :3] = q
    X[:, :, 3] = rng.standard_normal((n, r))
    return X


def ring(n, r):
    """The winding ring: identity measurements, kappa = tau = w = 1, and the
    point Y_i = Rz(2 pi i / n) in the first three rows, p_i = 0: exactly
    stationary, not optimal, lambda_min(S) = -(2 - 2 cos(2 pi / n))."""
    src = np.arange(n, dtype=np.int32)
    dst = ((src + 1) % n).astype(np.int32)
    g = dict(n_poses=n, src=src, dst=dst, R=np.tile(np.eye(3), (n, 1, 1)), t=np.zeros((n, 3)), kappa=np.ones(n),
             tau=np.ones(n), weight=np.ones(n))
    X = np.zeros((n, r, 4))
    a = 2.0 * np.pi * np.arange(n) / n
    X[:, 0, 0], X[:, 0, 1] = np.cos(a), -np.sin(a)
    X[:, 1, 0], X[:, 1, 1] = np.sin(a), np.cos(a)
    X[:, 2, 2] = 1.0
    return g, X


# ---- the points the soundness tests decide on (tests/test_cert_sound_*.py)

def dense_of(g, X, w=None):
    """(Q, S) of a graph dict and a point."""
    Q = dense_Q(g["n_poses"], g["src"], g["dst"], g["R"], g["t"], g["kappa"], g["tau"], g["weight"] if w is None else w)
    return Q, dense_S(X, Q)


def perturbed_point(X, delta, dseed):
    """X + delta D with D standard normal from dseed, every pose's r x 3 block
    replaced by the Q factor of its QR with a positive diagonal (the
    translation is kept): almost stationary for a small delta."""
    Z = X + delta * np.random.default_rng(dseed).standard_normal(X.shape)
    q, rr = np.linalg.qr(Z[:, :, :3])
    d = np.sign(np.diagonal(rr, axis1=1, axis2=2))
    d[d == 0] = 1.0
    Z[:, :, :3] = q * d[:, None, :]
    return Z


F_GRAPHS = ((5, 3, 5), (17, 20, 5), (33, 10, 3), (65, 80, 5), (130, 150, 8))
F_DELTAS = (0.0, 1e-7) + tuple(float(x) for x in np.geomspace(1e-5, 1e-3, 13))
F_DSEEDS = (1, 2, 3)
F_SEEDS = (1, 2, 3, 4, 5, 6)
F_TEST_EVERY = 10


def family_points(graphs=F_GRAPHS, dseeds=F_DSEEDS, deltas=F_DELTAS, eta_rel=1e-6):
    """Family F, one entry per point: consistent_graph(n, m, r, 6) at
    perturbed_point(X, delta, dseed), with the dense S, its eigenvalues ev,
    eta = eta_rel lambda_max and max_steps = 40 n + 200. Every point is run
    from the Lanczos seeds F_SEEDS with test_every = F_TEST_EVERY."""
    for (n, m, r) in graphs:
        g, X0 = consistent_graph(n, m, r, 6)
        for dseed in dseeds:
            for delta in deltas:
                X = perturbed_point(X0, delta, dseed)
                _, S = dense_of(g, X)
                ev = np.linalg.eigvalsh(S)
                yield dict(graph=(n, m, r), dseed=dseed, delta=delta, g=g, X=X, S=S, ev=ev, eta=eta_rel * ev[-1],
                           max_steps=40 * n + 200)


# What the restatement's scan showed over all 1350 runs of F, rounded up
# (tests/test_cert_sound_cpu.py measures them again and holds them under these
# figures; the device tests take ten times them): Ritz values below lambda_min
# (measured 4.3e-16) and above lambda_max (5.2e-15 to 8.0e-15, with the BLAS
# thread count), over every application of the rule, in units of lambda_max;
# and the true residual |S y - theta_min y| of the unit Ritz vector above rho
# at the step a run returns, the only step whose vector the device forms, in
# units of k eps lambda_max at k steps (measured 2.11; over the undecided tests
# too it is 55, at a step past the dimension where rho is still 9e-6 lambda_max).
F_RITZ_BELOW = 1e-15
F_RITZ_ABOVE = 2e-14
F_RESIDUAL_RATIO = 2.5

SMALL_GRAPHS = ((2, 0, 3), (3, 1, 4), (5, 3, 5))
SMALL_DELTAS = (0.0, 1e-6, 1e-4, 1e-2)
SMALL_TEST_EVERY = (1, 10, 64)
SMALL_MAX_STEPS = 200

RINGS = ((8, 3), (24, 5), (100, 3))
RING_ETA_RATIOS = (0.5, 0.99, 1.01, 2.0, 10.0)


def ring_lambda_min(n):
    return -(2.0 - 2.0 * np.cos(2.0 * np.pi / n))
