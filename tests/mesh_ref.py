"""The mesh deformation contract (include/kmx_abi.h, "Mesh deformation") in
plain numpy, with the loops, summation orders and the tie rule exactly as
stated there. The reference of tests/test_mesh_cpu.py and test_mesh_gpu.py.

Every product and sum below is a separate numpy operation (no fused
multiply-add), in the order the contract names.
"""
import numpy as np

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def window(s: int, W: int):
    """[s - W, s + W], saturating at the int64 limits."""
    return max(int(s) - int(W), I64_MIN), min(int(s) + int(W), I64_MAX)


def bind(node_robot, node_stamp, node_g, v_robot, v_stamp, v_xyz, k: int, W: int):
    """idx [n, k] (node ids in rank order, -1 beyond count), w [n, k] (0 beyond
    count), count [n]."""
    node_robot = np.asarray(node_robot, np.int64)
    node_stamp = np.asarray(node_stamp, np.int64)
    g = np.asarray(node_g, np.float64).reshape(-1, 3)
    xyz = np.asarray(v_xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    idx = np.full((n, k), -1, np.int32)
    w = np.zeros((n, k), np.float64)
    count = np.zeros(n, np.int32)
    # a robot's node ids in increasing order; its stamps are non-decreasing, so
    # the candidates lo <= s_j <= hi are one run of that list
    by_robot = {int(a): np.nonzero(node_robot == a)[0] for a in np.unique(node_robot)}
    st_of = {a: node_stamp[ids] for a, ids in by_robot.items()}
    assert all((np.diff(st) >= 0).all() for st in st_of.values())
    none = np.zeros(0, np.int64)
    for i in range(n):
        lo, hi = window(int(v_stamp[i]), W)
        ids = by_robot.get(int(v_robot[i]), none)
        st = st_of.get(int(v_robot[i]), none)
        cand = ids[np.searchsorted(st, np.int64(lo), "left"):np.searchsorted(st, np.int64(hi), "right")]
        m = cand.shape[0]
        if m == 0:
            continue
        v = xyz[i].astype(np.float64)
        dx, dy, dz = v[0] - g[cand, 0], v[1] - g[cand, 1], v[2] - g[cand, 2]
        d2 = dx * dx + dy * dy + dz * dz
        order = np.lexsort((cand, d2))  # by squared distance, ties to the lower node id
        cand, d2 = cand[order], d2[order]
        if m == 1:
            idx[i, 0], w[i, 0], count[i] = cand[0], 1.0, 1
            continue
        used = min(m, k + 1) - 1
        dmax = np.sqrt(d2[used])
        with np.errstate(invalid="ignore", divide="ignore"):
            t = 1.0 - np.sqrt(d2[:used]) / dmax
        wj = t * t
        s = 0.0
        for j in range(used):  # in rank order
            s = s + wj[j]
        if s > 0.0:
            idx[i, :used], w[i, :used], count[i] = cand[:used], wj / s, used
        else:  # d_max == 0, or every used node at d_max: the nearest alone
            idx[i, 0], w[i, 0], count[i] = cand[0], 1.0, 1
    return idx, w, count


def corrections(R_rest, R_cur):
    """R_j = Rcur_j Rrest_j^T, each entry summed over the inner index in order."""
    A = np.asarray(R_cur, np.float64).reshape(-1, 3, 3)
    B = np.asarray(R_rest, np.float64).reshape(-1, 3, 3)
    R = np.empty_like(A)
    for r in range(3):
        for c in range(3):
            R[:, r, c] = A[:, r, 0] * B[:, c, 0] + A[:, r, 1] * B[:, c, 1] + A[:, r, 2] * B[:, c, 2]
    return R


def deform(v_xyz, idx, w, count, R_rest, g, R_cur, p):
    """(out float32 [n, 3], stats): v' = sum_j w_j (R_j (v - g_j) + p_j) in
    rank order, rounded to fp32 once; an unbound vertex passes through."""
    xyz = np.asarray(v_xyz, np.float32).reshape(-1, 3)
    g = np.asarray(g, np.float64).reshape(-1, 3)
    p = np.asarray(p, np.float64).reshape(-1, 3)
    R = corrections(R_rest, R_cur)
    v = xyz.astype(np.float64)
    n, k = idx.shape
    acc = np.zeros((n, 3))
    for j in range(k):
        use = count > j
        jd = np.where(use, idx[:, j], 0)
        d = v - g[jd]
        y = np.empty((n, 3))
        for c in range(3):
            y[:, c] = R[jd, c, 0] * d[:, 0] + R[jd, c, 1] * d[:, 1] + R[jd, c, 2] * d[:, 2] + p[jd, c]
        acc = np.where(use[:, None], acc + w[:, j:j + 1] * y, acc)
    out = np.where((count > 0)[:, None], acc.astype(np.float32), xyz).astype(np.float32)
    e = out.astype(np.float64) - v
    d2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]
    d2 = np.where(count > 0, d2, 0.0)
    stats = {"vertices": n, "unbound": int((count == 0).sum()), "partial": int(((count > 0) & (count < k)).sum()),
             "max_displacement": float(np.sqrt(d2.max())) if n else 0.0, "sum_sq_displacement": float(d2.sum())}
    return out, stats


def deform_all(node_robot, node_stamp, R_rest, g, R_cur, p, v_robot, v_stamp, v_xyz, k, W):
    idx, w, count = bind(node_robot, node_stamp, g, v_robot, v_stamp, v_xyz, k, W)
    out, stats = deform(v_xyz, idx, w, count, R_rest, g, R_cur, p)
    return out, stats, (idx, w, count)


def tolerance(ref, scale):
    """Per coordinate: max(1 fp32 ulp at |ref|, 1e-12 * scale). The fp64 sum
    has <= 8 terms of ~10 operations, about 2e-14 * scale."""
    return np.maximum(np.spacing(np.abs(np.asarray(ref, np.float32))).astype(np.float64), 1e-12 * scale)
