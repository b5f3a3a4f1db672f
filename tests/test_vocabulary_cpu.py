"""DBoW2 vocabulary: the CPU restatement's known answer, the file round trips,
kmx_voc_create's tree validation (host code, runs before any device call) and
the synthetic generator. No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from tests import bow_transform_ref as ref


def test_known_answer_tf_idf():
    voc, nf, feats = ref.hand_tree(weighting=0)
    kids = ref.children_of(voc)
    assert [ref.descend(voc, kids, feats[0, i]) for i in range(4)] == [5, 4, 3, 5]
    vptr, words, weights = ref.transform(voc, nf, feats, literal=True)
    # word 1: 1.0; word 2: 0.75 + 0.75 = 1.5; word 0 has weight 0; s = 1.0 + 1.5 = 2.5
    assert vptr.tolist() == [0, 2]
    assert words.tolist() == [1, 2]
    assert weights.tolist() == [0.4, 0.6]


def test_known_answer_idf_stores_the_weight_once():
    voc, nf, feats = ref.hand_tree(weighting=2)
    vptr, words, weights = ref.transform(voc, nf, feats, literal=True)
    # word 1: 1.0; word 2: 0.75 (the second hit adds nothing); s = 1.75
    assert vptr.tolist() == [0, 2] and words.tolist() == [1, 2]
    assert weights.tolist() == [0.5714285714285714, 0.42857142857142855]


def test_vectorised_descent_equals_the_literal_one():
    from kmx.synth.vocab import make_descriptors, make_vocabulary
    voc = make_vocabulary(4, 3, seed=3, flip_bits=40, irregular=0.4, zero_weight=0.2)
    desc = make_descriptors(voc, 2, 24, noise_bits=30, seed=4)
    kids = ref.children_of(voc)
    lit = [ref.descend(voc, kids, d) for d in desc.reshape(-1, 32)]
    assert ref.descend_numpy(voc, desc.reshape(-1, 32)).tolist() == lit
    a = ref.transform(voc, [24, 7], desc, literal=True)
    b = ref.transform(voc, [24, 7], desc)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    hv, nf, feats = ref.hand_tree()
    assert ref.descend_numpy(hv, feats[0]).tolist() == [5, 4, 3, 5]  # the ties included


YAML = """%YAML:1.0
---
vocabulary:
   k: 3
   L: 2
   scoringType: 0
   weightingType: 0
   nodes:
      - { nodeId:1, parentId:0, weight:0., descriptor:"252 188 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 7 1 " }
      - { nodeId:2, parentId:0, weight:0., descriptor:"255 255 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 " }
      - { nodeId:3, parentId:0, weight:2.5000000000000000e-01,
          descriptor:"0 0 255 255 255 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 " }
      - { nodeId:4, parentId:1, weight:1., descriptor:"0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 15 " }
      - { nodeId:5, parentId:1, weight:7.2346980520501352e+00, descriptor:"0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 240 0 " }
      - { nodeId:6, parentId:2, weight:2., descriptor:"255 255 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 9 " }
   words:
      - { wordId:0, nodeId:3 }
      - { wordId:1, nodeId:4 }
      - { wordId:2, nodeId:5 }
      - { wordId:3, nodeId:6 }
"""


def _same(a, b):
    assert (a.k, a.L, a.weighting, a.scoring) == (b.k, b.L, b.weighting, b.scoring)
    for f in ("parent", "descriptor", "weight", "word_node"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and np.array_equal(x, y), f


def test_yaml_round_trip(tmp_path):
    from kmx.lcd.vocabulary import Vocabulary
    src = tmp_path / "voc.yml"
    src.write_text(YAML)
    a = Vocabulary.from_dbow2_yaml(src)
    assert (a.k, a.L, a.scoring, a.weighting, a.n_nodes, a.n_words) == (3, 2, 0, 0, 7, 4)
    assert a.parent.tolist() == [-1, 0, 0, 0, 1, 1, 2] and a.word_node.tolist() == [3, 4, 5, 6]
    assert a.descriptor[1, :2].tolist() == [252, 188] and a.descriptor[1, 30:].tolist() == [7, 1]
    assert a.weight.tolist() == [0.0, 0.0, 0.0, 0.25, 1.0, 7.2346980520501352, 2.0]
    out = tmp_path / "again.yml"
    a.to_dbow2_yaml(out)
    text = out.read_text()
    assert text.startswith("%YAML:1.0\n")
    assert '- { nodeId:1, parentId:0, weight:0., descriptor:"252 188 0 ' in text and ' 7 1 " }' in text
    assert "- { wordId:3, nodeId:6 }" in text
    _same(a, Vocabulary.from_dbow2_yaml(out))


def test_yaml_and_npz_round_trip_of_a_generated_tree(tmp_path):
    from kmx.lcd.vocabulary import Vocabulary
    from kmx.synth.vocab import make_vocabulary
    voc = make_vocabulary(3, 3, seed=11, flip_bits=20, irregular=0.3, zero_weight=0.2, weighting=2)
    voc.to_dbow2_yaml(tmp_path / "v.yml")
    _same(voc, Vocabulary.from_dbow2_yaml(tmp_path / "v.yml"))   # weights survive as text, bit for bit
    voc.save_npz(tmp_path / "v.npz")
    _same(voc, Vocabulary.load_npz(tmp_path / "v.npz"))


def test_gpu_class_rejects_other_scorings():
    from kmx.lcd.vocabulary import GpuVocabulary
    voc, _, _ = ref.hand_tree()
    voc.scoring = 1
    with pytest.raises(ValueError, match="scoringType"):
        GpuVocabulary(voc)


def _create(parent, word_node, weighting=0, n_nodes=None):
    from kmx import abi
    L = abi.lib()
    parent = np.ascontiguousarray(parent, np.int32)
    word_node = np.ascontiguousarray(word_node, np.int32)
    n = parent.shape[0] if n_nodes is None else n_nodes
    desc = np.zeros((max(parent.shape[0], 1), 32), np.uint8)
    weight = np.ones(max(parent.shape[0], 1))
    h = C.c_void_p()
    rc = L.kmx_voc_create(0, n, abi.iptr(parent), abi.u8ptr(desc), abi.fptr(weight), word_node.shape[0],
                          abi.iptr(word_node), weighting, C.byref(h))
    msg = L.kmx_last_error().decode() if rc else ""
    if rc == 0:
        L.kmx_voc_destroy(h)
    return rc, msg


GOOD_PARENT = [-1, 0, 0, 0, 1, 1, 2]
GOOD_WORDS = [3, 4, 5, 6]
_CHAIN = [-1] + list(range(70))  # node i hangs below node i - 1: depth 70


@pytest.mark.parametrize("parent,words,msg", [
    ([-1, 0, 0, 99, 1, 1, 2], GOOD_WORDS, "parent id out of range"),
    ([-1, 0, 0, -1, 1, 1, 2], GOOD_WORDS, "parent id out of range"),
    ([-1, 0, 0, 3, 1, 1, 2], GOOD_WORDS, "parent id out of range"),       # its own parent
    ([-1, 0, 0, 0, 5, 4, 2], GOOD_WORDS, "cycle"),
    (_CHAIN, [70], "deeper than 64"),
    (GOOD_PARENT, [3, 4, 5, 2], "inner node"),
    (GOOD_PARENT, [3, 4, 5], "no word"),
    (GOOD_PARENT, [3, 4, 5, 5], "two words"),
    (GOOD_PARENT, [3, 4, 5, 7], "out of range"),
    ([-1], [0], "n_nodes >= 2"),
], ids=["parent-high", "parent-negative", "parent-self", "cycle", "too-deep", "word-inner", "leaf-no-word",
        "leaf-two-words", "word-range", "one-node"])
def test_create_rejects_malformed_trees_before_any_device_call(parent, words, msg):
    from kmx import abi
    rc, text = _create(parent, words)
    assert rc == abi.KMX_EINVAL and msg in text, (rc, text)


def test_create_rejects_unknown_weighting_and_takes_a_good_tree():
    from kmx import abi
    rc, text = _create(GOOD_PARENT, GOOD_WORDS, weighting=4)
    assert rc == abi.KMX_EUNSUP and "weighting" in text
    # a well-formed tree passes the checks: with a GPU it is created, without
    # one the failure is the device's, not the tree's
    rc, text = _create(GOOD_PARENT, GOOD_WORDS)
    if abi.device_count() > 0:
        assert rc == 0, text
    else:
        assert rc != 0 and ("HIP" in text or "hip" in text), (rc, text)


def test_generator_is_deterministic_and_every_leaf_is_one_word():
    from kmx.synth.vocab import make_descriptors, make_vocabulary
    kw = dict(seed=7, flip_bits=24, irregular=0.4, zero_weight=0.3)
    a, b = make_vocabulary(5, 4, **kw), make_vocabulary(5, 4, **kw)
    for f in ("parent", "descriptor", "weight", "word_node"):
        assert np.array_equal(getattr(a, f), getattr(b, f))
    c = make_vocabulary(5, 4, **dict(kw, seed=8))
    assert not np.array_equal(a.descriptor[:20], c.descriptor[:20])
    n = a.n_nodes
    cnt = np.bincount(a.parent[1:], minlength=n)
    leaves = np.flatnonzero(cnt == 0)
    assert np.array_equal(np.sort(a.word_node), leaves) and np.all(np.diff(a.word_node) > 0)
    assert cnt.max() == 5 and 0 < cnt[cnt > 0].min() < 5          # 1..k children
    depth = np.zeros(n, int)
    for i in range(1, n):                                           # creation order: parents come first
        assert a.parent[i] < i
        depth[i] = depth[a.parent[i]] + 1
    assert depth.max() == 4 and depth[leaves].min() < 4             # leaves above level L
    w = a.weight[a.word_node]
    assert 0.15 < np.mean(w == 0.0) < 0.45 and np.all(w[w != 0.0] >= 0.5)
    assert not np.array_equal(np.arange(1, n), np.argsort(depth[1:], kind="stable") + 1)  # ids are not breadth first
    r = make_vocabulary(10, 3, seed=1, flip_bits=24)
    assert (r.n_nodes, r.n_words) == (1111, 1000)
    d1 = make_descriptors(r, 3, 16, noise_bits=3, seed=2)
    assert d1.shape == (3, 16, 32) and d1.dtype == np.uint8
    assert np.array_equal(d1, make_descriptors(r, 3, 16, noise_bits=3, seed=2))
