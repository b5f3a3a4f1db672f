"""Seeded synthetic DBoW2 vocabularies and ORB-like descriptors near their words.

The reference's vocabulary (mit_voc.yml, kimera_vio_jackal.launch:40) is an
offline download, so trees of the same structure are generated: a k-ary tree
of depth L whose nodes carry 256-bit descriptors, a child's being its
parent's with a few bits flipped (so a descriptor near a leaf descends to
it, as with a k-means tree), leaves numbered as words in increasing node id
with idf-like weights. Node ids follow DBoW2's creation order (HKmeansStep:
a node's children get consecutive ids, then each child's subtree is built in
turn), so they are not breadth first and the device renumbering has work to do.
Both generators build level by level with vectorised numpy.
"""
from __future__ import annotations

import numpy as np

from ..lcd.vocabulary import Vocabulary


def _flip(desc: np.ndarray, bits: int, rng) -> None:
    """Flip `bits` bit positions (drawn with replacement) in every row of desc [n, 32]."""
    n = desc.shape[0]
    rows = np.arange(n)
    for _ in range(int(bits)):
        pos = rng.integers(0, 256, n)
        desc[rows, pos >> 3] ^= (1 << (pos & 7)).astype(np.uint8)


def make_vocabulary(k: int, L: int, *, seed: int, flip_bits: int, irregular: float = 0.0,
                    zero_weight: float = 0.0, weighting: int = 0) -> Vocabulary:
    """A depth-L tree with k children per inner node. `irregular`: the share
    of inner nodes below the root that get 1..k-1 children or become leaves
    early (equal odds for 0..k-1); `zero_weight`: the share of words with
    weight 0.0; the other weights are uniform in [0.5, 12), the range of
    log(N / n_i)."""
    if k < 1 or L < 1:
        raise ValueError("need k >= 1 and L >= 1")
    rng = np.random.Generator(np.random.PCG64(seed))
    # breadth first: per level the parent (index into the previous level) and descriptor
    level_parent = [np.zeros(0, np.int64)]
    level_desc = [rng.integers(0, 256, (1, 32)).astype(np.uint8)]
    level_cnt = []
    for depth in range(L):
        n = level_desc[depth].shape[0]
        cnt = np.full(n, k, np.int64)
        if irregular > 0.0 and depth > 0:
            odd = rng.random(n) < irregular
            cnt[odd] = rng.integers(0, k, int(odd.sum()))
        level_cnt.append(cnt)
        par = np.repeat(np.arange(n), cnt)
        d = level_desc[depth][par].copy()
        _flip(d, flip_bits, rng)
        level_parent.append(par)
        level_desc.append(d)
    level_cnt.append(np.zeros(level_desc[L].shape[0], np.int64))
    sizes = [d.shape[0] for d in level_desc]
    off = np.concatenate([[0], np.cumsum(sizes)])
    n_nodes = int(off[-1])
    bfs_parent = np.full(n_nodes, -1, np.int64)
    for depth in range(1, L + 1):
        bfs_parent[off[depth]:off[depth + 1]] = off[depth - 1] + level_parent[depth]
    bfs_cnt = np.concatenate(level_cnt)
    bfs_first = np.zeros(n_nodes, np.int64)  # first child of a node, breadth-first ids
    for depth in range(L):
        c = level_cnt[depth]
        bfs_first[off[depth]:off[depth + 1]] = off[depth + 1] + np.cumsum(c) - c
    # DBoW2 ids: creation order (one step per inner node)
    new_id = np.zeros(n_nodes, np.int64)
    nxt = 1
    stack = [0]
    while stack:
        b = stack.pop()
        c = int(bfs_cnt[b])
        if c == 0:
            continue
        f = int(bfs_first[b])
        new_id[f:f + c] = np.arange(nxt, nxt + c)
        nxt += c
        stack.extend(range(f + c - 1, f - 1, -1))
    parent = np.full(n_nodes, -1, np.int32)
    parent[new_id[1:]] = new_id[bfs_parent[1:]]
    desc = np.zeros((n_nodes, 32), np.uint8)
    desc[new_id] = np.concatenate(level_desc)
    desc[0] = 0  # the root's descriptor is never compared (DBoW2 does not save it)
    is_leaf = np.zeros(n_nodes, bool)
    is_leaf[new_id] = bfs_cnt == 0
    word_node = np.flatnonzero(is_leaf).astype(np.int32)  # createWords: leaves in increasing node id
    weight = np.zeros(n_nodes, np.float64)
    w = rng.uniform(0.5, 12.0, word_node.shape[0])
    if zero_weight > 0.0:
        w[rng.random(word_node.shape[0]) < zero_weight] = 0.0
    weight[word_node] = w
    return Vocabulary(k, L, int(weighting), 0, parent, desc, weight, word_node)


def make_descriptors(voc: Vocabulary, n_frames: int, n_feats: int, *, noise_bits: int, seed: int) -> np.ndarray:
    """desc uint8 [n_frames, n_feats, 32]: every descriptor is a random word's
    leaf descriptor with `noise_bits` bit positions (drawn with replacement) flipped."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(n_frames) * int(n_feats)
    leaf = voc.word_node[rng.integers(0, voc.n_words, n)]
    d = voc.descriptor[leaf].copy()
    _flip(d, noise_bits, rng)
    return d.reshape(int(n_frames), int(n_feats), 32)
