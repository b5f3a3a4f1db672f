"""DBoW2 ORB vocabulary and its transform on MI355X.

  Vocabulary        the tree in DBoW2's node ids: load / save in DBoW2's
                    `save()` YAML layout and as npz
  GpuVocabulary     TemplatedVocabulary::transform(features, BowVector&) on
                    the GPU (kmx_voc_*, voc.hip): ORB descriptors, from host
                    arrays or from a LoopClosureDetector's resident frame
                    pool, to the L1-normalised CSR BowVectors kmx.lcd.bow reads

DBoW2 is not vendored and no upstream vocabulary file (`mit_voc.yml`,
launch/kimera_vio_jackal.launch:40) is at hand: the YAML layout is restated
from DBoW2's `TemplatedVocabulary::save` [U] and pinned only by the round trip
(tests/test_vocabulary_cpu.py); the transform is "parity unpinned" like the
query and is checked bit for bit against tests/bow_transform_ref.py.
"""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass

import numpy as np

from .. import abi
from ..abi import check, iptr, u8ptr, u32ptr, fptr

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3   # DBoW2 WeightingType
L1_NORM = 0                            # DBoW2 ScoringType L1_NORM

_NODE_RE = re.compile(r'nodeId:\s*(\d+)\s*,\s*parentId:\s*(\d+)\s*,\s*weight:\s*([^,\s]+)\s*,\s*'
                      r'descriptor:\s*"([^"]*)"')
_WORD_RE = re.compile(r"wordId:\s*(\d+)\s*,\s*nodeId:\s*(\d+)")
_KEY_RE = re.compile(r"^\s*(k|L|scoringType|weightingType)\s*:\s*(-?\d+)\s*$")


@dataclass
class Vocabulary:
    """A DBoW2 vocabulary tree in DBoW2's node ids. Node 0 is the root; node
    i > 0 has parent[i]; a node's children are the nodes naming it, in
    increasing id (DBoW2's load order). descriptor [n_nodes, 32] uint8 (the
    root's is unused), weight [n_nodes] float64 (read at leaves),
    word_node [n_words] int32: the leaf of each word."""
    k: int
    L: int
    weighting: int
    scoring: int
    parent: np.ndarray
    descriptor: np.ndarray
    weight: np.ndarray
    word_node: np.ndarray

    def __post_init__(self):
        self.parent = np.ascontiguousarray(self.parent, np.int32)
        self.descriptor = np.ascontiguousarray(self.descriptor, np.uint8)
        self.weight = np.ascontiguousarray(self.weight, np.float64)
        self.word_node = np.ascontiguousarray(self.word_node, np.int32)
        n = self.parent.shape[0]
        if self.descriptor.shape != (n, 32) or self.weight.shape != (n,) or self.word_node.ndim != 1:
            raise ValueError("vocabulary shapes must be parent [n], descriptor [n, 32], weight [n], word_node [w]")

    @property
    def n_nodes(self) -> int:
        return int(self.parent.shape[0])

    @property
    def n_words(self) -> int:
        return int(self.word_node.shape[0])

    # ------------------------------------------------------------------ npz --
    def save_npz(self, path) -> None:
        np.savez_compressed(path, k=self.k, L=self.L, weighting=self.weighting, scoring=self.scoring,
                            parent=self.parent, descriptor=self.descriptor, weight=self.weight,
                            word_node=self.word_node)

    @classmethod
    def load_npz(cls, path) -> "Vocabulary":
        with np.load(path) as z:
            return cls(int(z["k"]), int(z["L"]), int(z["weighting"]), int(z["scoring"]), z["parent"],
                       z["descriptor"], z["weight"], z["word_node"])

    # ----------------------------------------------------------------- YAML --
    def to_dbow2_yaml(self, path) -> None:
        """DBoW2 TemplatedVocabulary::save through cv::FileStorage [U]: the
        %YAML:1.0 header, a `vocabulary` map with k, L, scoringType,
        weightingType, the nodes (all but the root) and the words as flow
        maps. A descriptor is its 32 bytes in decimal, each followed by a
        space (FORB::toString). Weights are written with repr(), which
        reads back to the same double."""
        with open(path, "w") as f:
            f.write("%YAML:1.0\n---\nvocabulary:\n")
            f.write(f"   k: {int(self.k)}\n   L: {int(self.L)}\n   scoringType: {int(self.scoring)}\n"
                    f"   weightingType: {int(self.weighting)}\n   nodes:\n")
            desc = self.descriptor
            for i in range(1, self.n_nodes):
                d = "".join(f"{b} " for b in desc[i].tolist())
                f.write(f'      - {{ nodeId:{i}, parentId:{int(self.parent[i])}, weight:{_fmt(self.weight[i])}, '
                        f'descriptor:"{d}" }}\n')
            f.write("   words:\n")
            for w in range(self.n_words):
                f.write(f"      - {{ wordId:{w}, nodeId:{int(self.word_node[w])} }}\n")

    @classmethod
    def from_dbow2_yaml(cls, path) -> "Vocabulary":
        """Read DBoW2's save() layout with a line / regex reader: OpenCV
        writes `key:value` without a space inside flow maps, which a YAML
        parser does not take for a mapping. A node entry may span lines."""
        text = open(path).read()
        head = {}
        for line in text.split("\n"):
            m = _KEY_RE.match(line)
            if m and m.group(1) not in head:
                head[m.group(1)] = int(m.group(2))
            if line.strip().startswith("nodes:"):
                break
        for key in ("k", "L", "scoringType", "weightingType"):
            if key not in head:
                raise ValueError(f"{path}: no `{key}` in the vocabulary header")
        nodes = _NODE_RE.findall(text)
        words = _WORD_RE.findall(text[text.rfind("words:"):] if "words:" in text else "")
        if not nodes or not words:
            raise ValueError(f"{path}: no nodes / words entries in DBoW2's save() layout")
        n = len(nodes) + 1
        parent = np.full(n, -1, np.int32)
        desc = np.zeros((n, 32), np.uint8)
        weight = np.zeros(n, np.float64)
        seen = np.zeros(n, bool)
        for nid, pid, w, d in nodes:
            i = int(nid)
            if not 1 <= i < n or seen[i]:
                raise ValueError(f"{path}: node ids must be 1..{n - 1}, each once (got {i})")
            seen[i] = True
            parent[i] = int(pid)
            weight[i] = float(w)
            b = d.split()
            if len(b) != 32:
                raise ValueError(f"{path}: node {i}: an ORB descriptor has 32 bytes, got {len(b)}")
            desc[i] = [int(x) for x in b]
        word_node = np.full(len(words), -1, np.int32)
        for wid, nid in words:
            w = int(wid)
            if not 0 <= w < len(words) or word_node[w] >= 0:
                raise ValueError(f"{path}: word ids must be 0..{len(words) - 1}, each once (got {w})")
            word_node[w] = int(nid)
        return cls(head["k"], head["L"], head["weightingType"], head["scoringType"], parent, desc, weight, word_node)


def _fmt(x) -> str:
    """A double as cv::FileStorage writes reals: a trailing '.' on integers
    (`0.`), otherwise the shortest text that reads back to the same double."""
    x = float(x)
    if np.isfinite(x) and x == int(x) and abs(x) < 1e15:
        return f"{int(x)}."
    return repr(x)


class GpuVocabulary:
    """A Vocabulary resident on one GPU (kmx_voc_*): descriptors -> BowVectors."""

    def __init__(self, voc: Vocabulary, device: int = 0):
        if int(voc.scoring) != L1_NORM:
            raise ValueError(f"scoringType {voc.scoring}: only 0 (L1_NORM) is built — kmx_bow_* scores L1 only")
        L = abi.lib()
        if abi.device_count() <= device:
            raise abi.KmxError(f"no HIP device {device} visible (kmx has no CPU fallback)")
        h = C.c_void_p()
        check(L.kmx_voc_create(device, voc.n_nodes, iptr(voc.parent), u8ptr(voc.descriptor), fptr(voc.weight),
                               voc.n_words, iptr(voc.word_node), int(voc.weighting), C.byref(h)), "kmx_voc_create")
        self.L, self.h, self.voc, self.n_words = L, h, voc, voc.n_words

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.L.kmx_voc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream: int):
        check(self.L.kmx_voc_set_stream(self.h, C.c_void_p(hip_stream)), "kmx_voc_set_stream")

    def info(self) -> dict:
        v = [C.c_int32() for _ in range(6)]
        check(self.L.kmx_voc_info(self.h, *[C.byref(x) for x in v]), "kmx_voc_info")
        return dict(zip(("n_nodes", "n_words", "max_children", "max_depth", "lds_nodes", "descend_grid"), (x.value for x in v)))

    @staticmethod
    def _frames(n_feats, desc):
        nf = np.ascontiguousarray(n_feats, np.int32)
        de = np.ascontiguousarray(desc, np.uint8)
        if de.ndim != 3 or de.shape[2] != 32 or nf.shape != (de.shape[0],):
            raise ValueError("frames must be desc [F, N, 32] uint8 and n_feats [F]")
        return nf, de

    @staticmethod
    def _compact(nnz, words, weights):
        """Strided device output -> CSR (vptr int64, words uint32, weights float64)."""
        n, N = words.shape
        vptr = np.zeros(n + 1, np.int64)
        np.cumsum(nnz, out=vptr[1:])
        keep = np.arange(N)[None, :] < nnz[:, None]
        return vptr, np.ascontiguousarray(words[keep]), np.ascontiguousarray(weights[keep])

    def transform(self, n_feats, desc):
        """BowVectors of frames given as host arrays: desc uint8 [F, N, 32]
        (N <= 1024), n_feats [F]. Returns CSR (vptr, words, weights)."""
        nf, de = self._frames(n_feats, desc)
        F, N = de.shape[0], de.shape[1]
        nnz = np.zeros(max(F, 1), np.int32)
        words = np.zeros((max(F, 1), max(N, 1)), np.uint32)
        weights = np.zeros((max(F, 1), max(N, 1)), np.float64)
        check(self.L.kmx_voc_transform(self.h, F, N, iptr(nf), u8ptr(de), iptr(nnz), u32ptr(words), fptr(weights)),
              "kmx_voc_transform")
        return self._compact(nnz[:F], words[:F], weights[:F])

    def transform_pool(self, detector, frame_ids):
        """BowVectors of frames resident in a LoopClosureDetector's device pool
        (no second upload). frame_ids may repeat and come in any order."""
        ids = np.ascontiguousarray(frame_ids, np.int32)
        n, N = ids.shape[0], max(int(detector.max_feats), 1)
        nnz = np.zeros(max(n, 1), np.int32)
        words = np.zeros((max(n, 1), N), np.uint32)
        weights = np.zeros((max(n, 1), N), np.float64)
        check(self.L.kmx_voc_transform_pool(self.h, detector.h, n, iptr(ids), iptr(nnz), u32ptr(words),
                                            fptr(weights)), "kmx_voc_transform_pool")
        return self._compact(nnz[:n], words[:n], weights[:n])

    # enqueue-only forms (benchmark path): the vectors stay on the device
    def transform_async(self, n_feats, desc):
        nf, de = self._frames(n_feats, desc)
        self._keep = (nf, de)
        check(self.L.kmx_voc_transform_async(self.h, de.shape[0], de.shape[1], iptr(nf), u8ptr(de)),
              "kmx_voc_transform_async")

    def transform_pool_async(self, detector, frame_ids):
        ids = np.ascontiguousarray(frame_ids, np.int32)
        self._keep = (ids,)
        check(self.L.kmx_voc_transform_pool_async(self.h, detector.h, ids.shape[0], iptr(ids)),
              "kmx_voc_transform_pool_async")

    def sync(self):
        check(self.L.kmx_voc_sync(self.h), "kmx_voc_sync")

    def enable_timing(self, on: bool = True):
        check(self.L.kmx_voc_enable_timing(self.h, 1 if on else 0), "kmx_voc_enable_timing")

    def read_timing(self) -> dict:
        """Device times (ms) of the descent and the per-frame reduction of the last transform."""
        a, b = C.c_double(), C.c_double()
        check(self.L.kmx_voc_read_timing(self.h, C.byref(a), C.byref(b)), "kmx_voc_read_timing")
        return {"descend_ms": a.value, "reduce_ms": b.value}
