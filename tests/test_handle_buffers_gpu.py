"""A handle that replaces or grows its device buffers answers like a fresh one.

Every comparison is bitwise (np.array_equal) against a fresh handle given the
same inputs: what is checked is that a buffer replaced by a larger one, by a
smaller one again, or grown with contents to carry, holds exactly what a
first allocation would. The graphs are a 65-pose chain with loop closures (two
64-lane tiles) and a 130-pose one (every buffer larger); the mesh, the BoW
forward store and the vocabulary's batch buffers cross their first growth."""
import numpy as np
import pytest

from kmx import abi
from tests import cert_ref as CR

pytestmark = pytest.mark.gpu

SEC = 1_000_000_000


def _same(a, b, what=""):
    """Bitwise equality of two results: arrays, scalars, or tuples / lists / dicts of them."""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], f"{what}.{k}")
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), what


def _self_loop(g):
    bad = dict(g)
    bad["dst"] = g["dst"].copy()
    bad["dst"][0] = g["src"][0]
    return bad


# ------------------------------------------------------------------- chordal
def _chordal_graph(n, seed):
    g = CR.random_graph(n, 6, seed)  # the chain first, then six loop closures
    g.pop("weight")
    return g


def _chordal_set(c, g):
    c.set_graph(g["n_poses"], [0, g["n_poses"]], g["src"], g["dst"], g["R"], g["t"], g["kappa"], g["tau"])


def _chordal_fixed(g):
    return np.arange(g["src"].shape[0]) < g["n_poses"] - 1  # the chain


def _chordal_fresh(g, robust=False):
    from kmx.dpgo.chordal import ChordalSolver
    c = ChordalSolver()
    _chordal_set(c, g)
    out = c.solve_robust(_chordal_fixed(g), max_updates=5) if robust else c.solve()
    c.close()
    return out


def test_chordal_set_graph_larger_smaller_and_refused(gpu):
    from kmx.dpgo.chordal import ChordalSolver
    A, B = _chordal_graph(65, 1), _chordal_graph(130, 2)
    want_A, want_B, want_rob = _chordal_fresh(A), _chordal_fresh(B), _chordal_fresh(A, robust=True)
    assert np.abs(want_A[0] - want_B[0][:65]).max() > 1e-3  # two different problems
    c = ChordalSolver()
    _chordal_set(c, A)
    _same(c.solve(), want_A, "A")
    _same(c.solve_robust(_chordal_fixed(A), max_updates=5), want_rob, "A robust")  # allocates the robust group
    _chordal_set(c, B)  # every buffer, the robust group included, gives way to a larger one
    _same(c.solve(), want_B, "B")
    _chordal_set(c, A)
    _same(c.solve(), want_A, "A again")
    bad = _self_loop(A)
    with pytest.raises(abi.KmxError):
        _chordal_set(c, bad)
    _same(c.solve(), want_A, "A after a refused graph")
    _same(c.solve_robust(_chordal_fixed(A), max_updates=5), want_rob, "A robust after a refused graph")
    c.close()


# ---------------------------------------------------------------------- cert
def _cert_run(c, g, r, seed):
    """set_point, S v, Lambda, 30 Lanczos steps with the vector, and the escape step's candidates."""
    n = g["n_poses"]
    info = c.set_point(CR.random_point(n, r, seed))
    sv = c.apply(np.random.default_rng(seed + 1).standard_normal(4 * n))
    lam = c.lambda_blocks()
    res = c.min_eig(1e-30, max_steps=30, test_every=30, seed=7, want_vector=True)
    coef = c.coefficients()
    esc = c.escape(res["y"], np.array([1.0, 0.5, 0.25]))
    return info, sv, lam, res, coef, esc


def _cert_fresh(g, r, seed):
    from kmx.dpgo.certify import Certifier
    c = Certifier()
    c.set_graph(**g)
    out = _cert_run(c, g, r, seed)
    c.close()
    return out


def test_cert_set_graph_larger_smaller_and_refused(gpu):
    from kmx.dpgo.certify import Certifier
    A, B = CR.random_graph(65, 6, 3), CR.random_graph(130, 6, 4)
    want_A, want_B = _cert_fresh(A, 4, 10), _cert_fresh(B, 5, 11)
    c = Certifier()
    c.set_graph(**A)
    _same(_cert_run(c, A, 4, 10), want_A, "A")
    c.set_graph(**B)  # larger, and the candidates grow with it
    _same(_cert_run(c, B, 5, 11), want_B, "B")
    c.set_graph(**A)
    _same(_cert_run(c, A, 4, 10), want_A, "A again")
    bad = _self_loop(A)  # Certifier.check_graph would stop it: straight to the library
    rc = c.L.kmx_cert_set_graph(c.h, 65, bad["src"].shape[0], abi.iptr(bad["src"]), abi.iptr(bad["dst"]),
                                abi.fptr(np.ascontiguousarray(bad["R"])), abi.fptr(bad["t"]), abi.fptr(bad["kappa"]),
                                abi.fptr(bad["tau"]), abi.fptr(bad["weight"]))
    assert rc == abi.KMX_EINVAL
    _same(_cert_run(c, A, 4, 10), want_A, "A after a refused graph")
    c.close()


# -------------------------------------------------------------------- dgraph
def _dgraph_set(dg, P):
    dg.set_graph(P.R_rest, P.g, P.src, P.dst, P.w)
    dg.set_priors(P.mode, P.R_hat, P.t_hat, P.kappa, P.tau)


def _dgraph_run(dg):
    res = dg.solve(max_iterations=6)
    return res, dg.poses(), dg.log()


def _dgraph_fresh(P):
    from kmx.pgmo import DeformationGraph
    dg = DeformationGraph()
    _dgraph_set(dg, P)
    out = _dgraph_run(dg)
    dg.close()
    return out


def test_dgraph_set_graph_larger_smaller_and_refused(gpu):
    from kmx.pgmo import DeformationGraph
    from tests.test_dgraph_gpu import ring_problem
    A, B = ring_problem(65, 65), ring_problem(130, 130)
    want_A, want_B = _dgraph_fresh(A), _dgraph_fresh(B)
    assert want_A[0]["iterations"] > 0 and want_A[0]["accepted"] > 0
    dg = DeformationGraph()
    _dgraph_set(dg, A)
    _same(_dgraph_run(dg), want_A, "A")
    _dgraph_set(dg, B)
    _same(_dgraph_run(dg), want_B, "B")
    _dgraph_set(dg, A)
    _same(_dgraph_run(dg), want_A, "A again")
    dst = A.dst.copy()
    dst[0] = A.src[0]
    with pytest.raises(abi.KmxError):
        dg.set_graph(A.R_rest, A.g, A.src, dst, A.w)
    dg.set_poses()  # back to the rest poses, where a fresh handle starts
    _same(_dgraph_run(dg), want_A, "A after a refused graph")
    dg.close()


# ---------------------------------------------------------------------- mesh
def test_mesh_appends_across_the_first_doubling(gpu):
    """Nodes in calls of 1000, 24 and 1 (the last one doubles the node buffers
    from 1024 with rest poses, current poses and rows to carry), vertices in
    calls of 1000 and 25 after a bind (their buffers double with positions and
    bindings to carry)."""
    from kmx.pgmo import MeshDeformer
    from tests.test_mesh_cpu import _scene
    from tests.test_mesh_gpu import _moved
    s = _scene(7, n_nodes=1025, n_verts=1025, n_robots=2)
    R_cur, p = _moved(s)
    node = lambda a, b: (s["robot"][a:b], s["stamp"][a:b], s["R_rest"][a:b], s["g"][a:b])  # noqa: E731
    vert = lambda a, b: (s["v_robot"][a:b], s["v_stamp"][a:b], s["xyz"][a:b])  # noqa: E731

    fresh = MeshDeformer(k=4, window_ns=SEC, n_robots=2)
    fresh.add_nodes(*node(0, 1025))
    fresh.add_vertices(*vert(0, 1025))
    fresh.set_node_poses(0, R_cur, p)
    want = fresh.deform()
    want_b = fresh.bindings()
    fresh.close()
    assert want[1]["max_displacement"] > 0.1

    md = MeshDeformer(k=4, window_ns=SEC, n_robots=2)
    assert md.info()["node_capacity"] == 1024 and md.info()["vertex_capacity"] == 1024
    md.add_nodes(*node(0, 1000))
    md.set_node_poses(0, R_cur[:1000], p[:1000])  # rows that the doubling has to carry
    md.add_nodes(*node(1000, 1024))
    assert md.info()["node_capacity"] == 1024
    md.add_nodes(*node(1024, 1025))
    assert md.info()["node_capacity"] == 2048
    md.set_node_poses(1000, R_cur[1000:], p[1000:])
    assert md.add_vertices(*vert(0, 1000)) == 0
    md.deform(first=0, n=1000)  # binds them
    assert md.add_vertices(*vert(1000, 1025)) == 1000
    assert md.info()["vertex_capacity"] == 2048
    _same(md.bindings(), want_b, "bindings")  # binds the 25 new ones; the first 1000 were carried
    _same(md.deform(), want, "deform")
    md.close()


# ----------------------------------------------------------------------- bow
def _bow_vectors(n, n_words, per, seed):
    rng = np.random.default_rng(seed)
    words = np.concatenate([np.sort(rng.choice(n_words, per, replace=False)) for _ in range(n)]).astype(np.uint32)
    w = rng.uniform(0.5, 1.5, (n, per))
    weights = (w / w.sum(1, keepdims=True)).reshape(-1)
    return np.arange(n + 1, dtype=np.int64) * per, words, weights


def _bow_prefix(db, a, b):
    vptr, words, weights = db
    return vptr[a:b + 1] - vptr[a], words[vptr[a]:vptr[b]], weights[vptr[a]:vptr[b]]


def test_bow_forward_store_grows_past_both_floors(gpu, monkeypatch):
    """1100 entries of 60 words: more than the forward store's first 1024
    entries and its first 65 536 postings, added while it holds entries; the
    queries run on an unsealed tail, on a sealed base with a tail, and after
    the last seal."""
    from kmx.lcd.bow import BowDatabase
    for k in ("KMX_BOW_TAIL", "KMX_BOW_CHUNK", "KMX_BOW_LDS"):
        monkeypatch.delenv(k, raising=False)
    NW = 5000
    db = _bow_vectors(1100, NW, 60, 21)
    q = _bow_vectors(32, NW, 60, 22)
    assert int(db[0][-1]) == 66000

    def rebuilt(n):
        S = BowDatabase(NW)
        S.set_entries(*_bow_prefix(db, 0, n))
        out = S.query(*q, 50)
        S.close()
        return out

    want_500, want_1100 = rebuilt(500), rebuilt(1100)
    G = BowDatabase(NW)
    G.reset()
    G.set_tail_cap(1024)
    assert G.add(*_bow_prefix(db, 0, 500)) == 0
    assert G.info()["n_sealed"] == 0
    _same(G.query(*q, 50), want_500, "before the seal")
    G.seal()
    assert G.add(*_bow_prefix(db, 500, 1100)) == 500  # the store grows with 500 entries held
    info = G.info()
    assert (info["n_sealed"], info["n_entries"], info["n_postings"]) == (500, 1100, 66000)
    _same(G.entries(0, 1100), db, "the stored vectors")
    _same(G.query(*q, 50), want_1100, "across the seal")
    G.seal()
    assert G.info()["n_sealed"] == 1100
    _same(G.query(*q, 50), want_1100, "after the seal")
    _same(G.entries(0, 1100), db, "the stored vectors after the seal")
    G.close()


# ----------------------------------------------------------------------- voc
def test_voc_batches_grow_and_shrink_on_one_handle(gpu):
    from kmx.lcd.vocabulary import GpuVocabulary
    from tests.test_bow_transform_gpu import _frames, _voc
    voc = _voc(10, 3)
    batches = [_frames(voc, [64, 17], 64, seed=31), _frames(voc, [128, 0, 99, 1, 128], 128, seed=32),
               _frames(voc, [5, 64], 64, seed=33)]
    want = []
    for nf, desc in batches:
        gv = GpuVocabulary(voc)
        want.append(gv.transform(nf, desc))
        gv.close()
    assert all(w[0][-1] > 0 for w in want)
    gv = GpuVocabulary(voc)
    for k, (nf, desc) in enumerate(batches):
        _same(gv.transform(nf, desc), want[k], f"batch {k}")
    gv.close()
