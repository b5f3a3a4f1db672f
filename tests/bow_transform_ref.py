"""CPU restatement of DBoW2's TemplatedVocabulary::transform(features,
BowVector&) for the ORB vocabulary, used ONLY by the vocabulary tests. It is a
literal reading of the published algorithm (DBoW2 is not vendored: [U], parity
unpinned):

  word of a descriptor   from the root, among the node's children in stored
                         order (increasing node id) the one of least Hamming
                         distance, a later child only on a strictly smaller
                         distance; repeat until a node without children
  vector of a frame      features in order; weight <= 0 contributes nothing;
                         TF_IDF / TF: v[word] += weight (one f64 addition per
                         occurrence); IDF / BINARY: v[word] = weight if absent;
                         then s = sum |v| in increasing word id, v /= s if s > 0

All sums are Python float `+=` in the stated order (np.sum is pairwise and
rounds differently). `descend_numpy` is a vectorised descent for the larger
cases; tests/test_vocabulary_cpu.py asserts it equal to the literal one.
"""
import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def children_of(voc):
    """Per node the list of its children in increasing node id."""
    kids = [[] for _ in range(voc.n_nodes)]
    for i in range(1, voc.n_nodes):
        kids[int(voc.parent[i])].append(i)
    return kids


def word_of_node(voc):
    w = np.full(voc.n_nodes, -1, np.int64)
    w[voc.word_node] = np.arange(voc.n_words)
    return w


def hamming(a, b) -> int:
    return int(_POP[np.bitwise_xor(a, b)].sum())


def descend(voc, kids, d) -> int:
    """Leaf node (DBoW2 id) of one descriptor d [32] uint8."""
    node = 0
    while kids[node]:
        best, best_d = -1, None
        for c in kids[node]:
            dist = hamming(voc.descriptor[c], d)
            if best_d is None or dist < best_d:
                best, best_d = c, dist
        node = best
    return node


def descend_numpy(voc, desc):
    """Leaf nodes of desc [n, 32]: all descriptors level by level; the j-th
    children of every current node are compared in turn with strict <."""
    desc = np.ascontiguousarray(desc, np.uint8)
    n = desc.shape[0]
    nn = voc.n_nodes
    cnt = np.bincount(voc.parent[1:], minlength=nn).astype(np.int64)
    order = np.argsort(voc.parent[1:], kind="stable") + 1   # children grouped by parent, increasing id
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    node = np.zeros(n, np.int64)
    active = cnt[node] > 0
    while active.any():
        idx = np.flatnonzero(active)
        cur = node[idx]
        best = np.full(idx.shape[0], 1 << 30, np.int64)
        pick = np.zeros(idx.shape[0], np.int64)
        for j in range(int(cnt[cur].max())):
            has = cnt[cur] > j
            c = order[first[cur[has]] + j]
            dist = _POP[np.bitwise_xor(voc.descriptor[c], desc[idx[has]])].sum(axis=1)
            better = dist < best[has]
            h = np.flatnonzero(has)[better]
            best[h] = dist[better]
            pick[h] = c[better]
        node[idx] = pick
        active = cnt[node] > 0
    return node


def bow_vector(voc, leaves, wid=None):
    """(words, weights) of one frame from its features' leaf nodes, in feature order."""
    if wid is None:
        wid = word_of_node(voc)
    additive = int(voc.weighting) in (0, 1)
    v = {}
    for leaf in leaves:
        w = float(voc.weight[int(leaf)])
        if not w > 0:
            continue
        word = int(wid[int(leaf)])
        if word in v:
            if additive:
                v[word] += w
        else:
            v[word] = w
    words = sorted(v)
    s = 0.0
    for word in words:
        s += abs(v[word])
    if s > 0:
        for word in words:
            v[word] = v[word] / s
    return np.array(words, np.uint32), np.array([v[word] for word in words], np.float64)


def transform(voc, n_feats, desc, literal=False):
    """CSR (vptr int64, words uint32, weights float64) of frames desc
    [F, N, 32] with n_feats[f] features each. literal: the per-descriptor
    Python descent instead of the vectorised one."""
    desc = np.asarray(desc, np.uint8)
    F = desc.shape[0]
    kids = children_of(voc) if literal else None
    wid = word_of_node(voc)
    vptr = np.zeros(F + 1, np.int64)
    W, V = [], []
    for f in range(F):
        n = int(n_feats[f])
        if literal:
            leaves = [descend(voc, kids, desc[f, i]) for i in range(n)]
        else:
            leaves = descend_numpy(voc, desc[f, :n]) if n else []
        w, v = bow_vector(voc, leaves, wid)
        W.append(w)
        V.append(v)
        vptr[f + 1] = vptr[f] + w.shape[0]
    words = np.concatenate(W) if W else np.zeros(0, np.uint32)
    weights = np.concatenate(V) if V else np.zeros(0, np.float64)
    return vptr, words.astype(np.uint32), weights.astype(np.float64)


def hand_tree(weighting=0):
    """The hand-built vocabulary of the known-answer tests and a 4-feature
    frame. Root 0 has children 1, 2, 3; node 1 has children 4, 5; node 2 has
    child 6; node 3 is a leaf. Words (leaves in increasing node id): 0 = node
    3 (weight 0), 1 = node 4 (1.0), 2 = node 5 (0.75), 3 = node 6 (2.0).

      feature 0 = node 5's descriptor            -> node 1 (4 bits) -> node 5: word 2
      feature 1 = byte 0 set: 8 bits from node 1 and from node 2 (a tie: the
                  first wins), then 12 bits from node 4 and from node 5 (a
                  tie again)                     -> word 1
      feature 2 = node 3's descriptor            -> word 0, weight 0: dropped
      feature 3 = node 5's plus one bit          -> word 2 again
    """
    from kmx.lcd.vocabulary import Vocabulary
    parent = np.array([-1, 0, 0, 0, 1, 1, 2], np.int32)
    desc = np.zeros((7, 32), np.uint8)
    desc[2, 0:2] = 0xFF
    desc[3, 2:5] = 0xFF
    desc[4, 31] = 0x0F
    desc[5, 30] = 0xF0
    desc[6, 0:2] = 0xFF
    weight = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 0.75, 2.0])
    word_node = np.array([3, 4, 5, 6], np.int32)
    voc = Vocabulary(3, 2, weighting, 0, parent, desc, weight, word_node)
    feats = np.zeros((1, 4, 32), np.uint8)
    feats[0, 0] = desc[5]
    feats[0, 1, 0] = 0xFF
    feats[0, 2] = desc[3]
    feats[0, 3] = desc[5]
    feats[0, 3, 29] = 0x01
    return voc, np.array([4], np.int32), feats
