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


def ritz(alpha, beta, eta):
    """The rule on the first k = len(alpha) steps, with numpy.linalg.eigh."""
    k = len(alpha)
    T = np.diag(alpha) + np.diag(beta[:k - 1], 1) + np.diag(beta[:k - 1], -1)
    ev, V = np.linalg.eigh(T)
    rho = abs(beta[k - 1] * V[k - 1, 0])
    if ev[0] < -eta:
        d = "NEGATIVE"
    elif rho <= eta and ev[0] - rho >= -eta:
        d = "CERTIFIED"
    else:
        d = "UNDECIDED"
    return {"decision": d, "steps": k, "theta_min": float(ev[0]), "theta_max": float(ev[-1]), "residual": float(rho)}


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
