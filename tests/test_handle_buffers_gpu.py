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


# ------------------------------------------------------- with torch tensors
_TORCH_CHILD = """
import sys
sys.path[:0] = [{root!r} + "/kimera-multi_amd", {root!r}]
import torch
torch.cuda.set_device(0)
torch.cuda.init()  # torch takes the device before the first kmx handle, as in kmx.dpgo.driver
from tests import test_handle_buffers_gpu as T
T.{body}()
print("child ok")
"""


def _in_torch_child(body):
    """Runs this module's `body` in a process of its own: torch has to take the
    device before the first kmx handle of a process does, and this session's
    earlier tests already hold it."""
    import subprocess
    import sys
    from pathlib import Path
    root = str(Path(__file__).resolve().parents[1])
    r = subprocess.run([sys.executable, "-c", _TORCH_CHILD.format(root=root, body=body)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ----------------------------------------------------------------------- lcd
def _lcd_fresh(pool, call):
    from kmx.lcd import LcdParams, LoopClosureDetector
    det = LoopClosureDetector(LcdParams())
    det.set_pool(pool)
    out = call(det)
    det.close()
    return out


def test_lcd_slot_grows_past_its_floor_while_slots_are_warm(gpu):
    """A synchronous call of 1500 candidates lands on a slot whose buffers hold
    the floor of 1024, after async calls have warmed the other slots; the
    small calls before and after it use what it left."""
    from kmx.lcd import LcdParams, LoopClosureDetector
    from kmx.synth.lcd import make_lcd_pool
    pool = make_lcd_pool(16, 64, seed=41)
    small = (pool.cand_query, pool.cand_match)
    big = (np.tile(pool.cand_query, 94)[:1500], np.tile(pool.cand_match, 94)[:1500])
    want_small = _lcd_fresh(pool, lambda d: d.verify(*small, with_masks=True))
    want_big = _lcd_fresh(pool, lambda d: d.verify(*big, with_masks=True))
    assert sum(r["accepted"] for r in want_small[0]) > 0
    det = LoopClosureDetector(LcdParams())
    det.set_pool(pool)
    _same(det.verify(*small, with_masks=True), want_small, "small")
    for _ in range(3):
        det.verify_async(*small)
    _same(det.verify(*big, with_masks=True), want_big, "1500 candidates")
    _same(det.verify(*small, with_masks=True), want_small, "small again")
    det.close()


def test_lcd_frame_staging_grows(gpu):
    """add_frames of one frame, then of four, at max_feats = 1024: 81 KB, then
    327 KB, past the staging area's 256 KiB floor."""
    from kmx.lcd import LcdParams, LoopClosureDetector
    from kmx.synth.lcd import make_lcd_pool
    pool = make_lcd_pool(6, 1024, seed=43)
    F = 5
    cq, cm = np.array([0, 2, 4, 1], np.int32), np.array([1, 3, 0, 2], np.int32)
    fr = lambda a, b: (pool.n_feats[a:b], pool.desc[a:b], pool.bearings[a:b], pool.points[a:b])  # noqa: E731

    ref = LoopClosureDetector(LcdParams())
    ref.set_frames(*fr(0, F))
    want = ref.verify(cq, cm, with_masks=True)
    ref.close()
    assert sum(r["accepted"] for r in want[0]) > 0
    det = LoopClosureDetector(LcdParams())
    assert det.add_frames(*fr(0, 1)) == 0
    assert det.add_frames(*fr(1, F)) == 1
    _same(det.verify(cq, cm, with_masks=True), want, "verify")
    det.close()


def test_lcd_borrowed_stream_is_used_and_left_alive(gpu):
    _in_torch_child("_lcd_borrowed_stream")


def _lcd_borrowed_stream():
    import torch
    from kmx.lcd import LcdParams, LoopClosureDetector
    from kmx.synth.lcd import make_lcd_pool
    pool = make_lcd_pool(16, 64, seed=47)
    cq, cm = pool.cand_query, pool.cand_match

    def run(det):
        v = det.verify(cq, cm, with_masks=True)
        pairs, k = det.match(cq, cm)
        corr = [(pairs[i, :k[i], 0], pairs[i, :k[i], 1]) for i in range(len(k))]
        return v, [pairs[i, :k[i]] for i in range(len(k))], k, det.verify_matches(cq, cm, corr, with_masks=True)

    want = _lcd_fresh(pool, run)
    st = torch.cuda.Stream()
    det = LoopClosureDetector(LcdParams())
    det.set_pool(pool)
    _same(det.verify(cq, cm, with_masks=True), want[0], "own stream")
    det.set_stream(st.cuda_stream)
    _same(run(det), want, "borrowed stream")
    det.close()
    with torch.cuda.stream(st):  # the stream was not the detector's to destroy
        x = torch.arange(8, device="cuda") * 2
    st.synchronize()
    assert x.sum().item() == 56


def test_lcd_timing_events_made_on_first_use(gpu):
    from kmx.lcd import LcdParams, LoopClosureDetector
    from kmx.synth.lcd import make_lcd_pool
    pool = make_lcd_pool(16, 64, seed=53)
    det = LoopClosureDetector(LcdParams())
    det.set_pool(pool)
    det.enable_timing(True)
    det.verify(pool.cand_query, pool.cand_match)
    t = det.read_timing()
    assert np.isfinite(t["knn_ms"]) and t["knn_ms"] >= 0 and np.isfinite(t["ransac_ms"]) and t["ransac_ms"] >= 0
    det.close()
    det = LoopClosureDetector(LcdParams())  # closed with its events never made
    det.set_pool(pool)
    det.enable_timing(True)
    det.close()


# ----------------------------------------------------------------------- pgo
def _pgo_params(kind):
    from kmx.dpgo.params import PGOAgentParameters, ROptParameters
    if kind == "accelerated":
        return PGOAgentParameters(r=5, acceleration=True)
    if kind == "two_rtr":
        return PGOAgentParameters(r=5, localOptimizationParams=ROptParameters(RTR_iterations=2))
    return PGOAgentParameters(r=5)


def _pgo_load(s, g):
    from kmx.synth import lift, lifting_matrix
    s.set_graph_data(g)
    Y = lifting_matrix(5, seed=1)
    for a in range(g.n_robots):
        s.set_iterate(a, lift(g.init_R[a], g.init_t[a], Y))


def _pgo_rounds(s, g):
    for _ in range(2):
        s.refresh_local()
        s.iterate()
    return [s.get_iterate(a) for a in range(g.n_robots)], s.get_public()[0], s.get_weights(), s.memory()


@pytest.mark.parametrize("kind", ["plain", "accelerated", "two_rtr"])
def test_pgo_set_graph_larger_smaller_and_again(gpu, kind):
    """accelerated and two_rtr hold the optional buffers (momentum V and Y; X at the round's start)."""
    from kmx.dpgo.solver import BlockSolver
    from kmx.synth import make_pose_graph
    P = _pgo_params(kind)
    A, B = make_pose_graph(2, 100, 300, seed=3), make_pose_graph(3, 150, 450, seed=4)
    want = []
    for g in (A, B):
        f = BlockSolver(P, 0)
        _pgo_load(f, g)
        want.append(_pgo_rounds(f, g))
        f.close()
    assert want[0][3] != want[1][3]  # two sizes
    s = BlockSolver(P, 0)
    for g, w, what in ((A, want[0], "A"), (B, want[1], "B"), (A, want[0], "A again")):
        _pgo_load(s, g)
        _same(_pgo_rounds(s, g), w, what)
    s.close()


def test_pgo_scratch_and_status_words_grow(gpu):
    """The scratch grows from a trajectory's (620 doubles) to an eval's (4000)
    and the peers' status words from 8 to 100 (past the first 64). The status
    words are zero: a peer whose last block update changed nothing."""
    _in_torch_child("_pgo_scratch_and_status_words")


def _pgo_scratch_and_status_words():
    import torch
    from kmx.dpgo.solver import BlockSolver
    from kmx.synth import make_pose_graph
    g = make_pose_graph(2, 100, 300, seed=3)
    P = _pgo_params("plain")
    seg = torch.zeros(101, dtype=torch.int32, device="cuda")
    rows = torch.zeros(100, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def unpack_and_round(s, sizes):
        for n_seg in sizes:
            s.exchange_unpack(0, 0, seg.data_ptr(), n_seg, rows.data_ptr())
        out = _pgo_rounds(s, g)
        return out[:3], s.get_public(100)[1]

    ref = BlockSolver(P, 0)
    _pgo_load(ref, g)
    want = unpack_and_round(ref, [100])
    ref.close()
    s = BlockSolver(P, 0)
    _pgo_load(s, g)
    anchor = s.get_iterate(0)[0]
    t0 = s.trajectory(0, anchor)
    grad, _ = s.eval(0, abi.KMX_EVAL_RGRAD)
    assert np.abs(grad).max() > 0
    _same(s.trajectory(0, anchor), t0, "trajectory after the scratch grew")
    _same(unpack_and_round(s, [8, 100]), want, "round after the status words grew")
    s.close()
