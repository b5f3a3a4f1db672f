"""LoopClosureDetector — Kimera-Multi-LCD verification API on MI355X.

Mirrors the verification half of Kimera-Multi-LCD's LoopClosureDetector
(drawio:2550-2609) as called by Kimera-Distributed's verifyLoopSpin
(drawio:2638-2657): computeMatchedIndices -> geometricVerificationNister ->
recoverPose, batched over candidates on the GPU through kmx_lcd_* (C ABI).
Parameters are read with the keys of params/D455/LcdParams.yaml.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from .. import abi
from ..abi import check


@dataclass
class LcdParams:
    """LcdParams (params/D455/LcdParams.yaml). matcher_type 3 is BruteForce-L1
    in the reference build (docker/copy/kimera_multi_lcd.patch:33-35); the
    north_star's Hamming matcher is `norm="hamming"`."""
    lowe_ratio: float = 0.7
    norm: str = "l1"
    min_nr_2d2d_inliers: int = 10
    min_nr_3d3d_inliers: int = 5
    ransac_threshold_2d2d: float = 1e-6
    ransac_threshold_3d3d: float = 0.3
    ransac_max_iterations: int = 500
    ransac_probability: float = 0.995
    ransac_randomize: int = 0
    ransac_seed: int = 12345
    rng_variant: str = "gcc9"           # libstdc++ of ROS Noetic (SURVEY.md §0 finding 5)
    ransac_use_1point_3d3d: int = 1     # 1: translation given the 2D-2D rotation; 0: Arun 3-point RANSAC
    # opengv CentralRelativePoseSacProblem::algorithm_t (LcdParams.yaml:73):
    # 0 STEWENIUS (the reference config), 1 NISTER
    ransac_2d2d_algorithm: int = 0
    # opengv AbsolutePoseSacProblem::algorithm_t (LcdParams.yaml:74): 3 EPNP
    ransac_2d3d_algorithm: int = 3
    # PnP pose recovery (pose_recovery_type 1: EPnP RANSAC, LcdParams.yaml:53,57,63,74)
    pose_recovery_type: int = 0
    min_nr_2d3d_inliers: int = 20
    ransac_threshold_2d3d: float = 1.0   # pixels
    # px: converts the 2D-3D threshold to (1 - cos), as Kimera-VIO's LCD does
    # with the left camera's fu. The default is the D455 left camera's fu
    # (params/D455/LeftCameraParams.yaml:18, intrinsics[0]); from_yaml(...,
    # camera_yaml=...) reads it from a camera file
    focal_length: float = 377.229220831
    # BoW detection (LcdParams.yaml:3-12)
    use_nss: int = 1
    alpha: float = 0.4
    min_temporal_matches: int = 1
    recent_frames_window: int = 100
    max_db_results: int = 50
    min_nss_factor: float = 0.05
    min_matches_per_island: int = 1
    max_intraisland_gap: int = 3
    max_nrFrames_between_islands: int = 3
    max_nrFrames_between_queries: int = 2
    # stereo pose refinement after an accepted 3D-3D recovery (LcdParams.yaml:14,
    # the reference config): least-squares T over the 3D-3D inliers
    # (include/kmx_abi.h refine_pose), a restated substitute for Kimera-VIO's
    # GTSAM stereo refinement [U, parity unpinned]. Results it touched carry
    # "pose_refined": True. Measured on 20 planted candidates it is not more
    # accurate than the unrefined pose (translation error 0.0158 vs 0.0149 m,
    # rotation 1.17e-3 vs 1.11e-3; tests/test_golden_cpu.py
    # test_refine_pose_delta_on_planted_pool); 0 keeps the recovered pose.
    refine_pose: int = 1
    # ORB keypoints per frame (LcdParams.yaml:19): the feature-slot stride of
    # the frame pool that addVLCFrame fills
    nfeatures: int = 700
    # LC5 sampler reading (include/kmx_abi.h rng_stream): 0 every RANSAC
    # problem seeds its own engine (opengv's constructor, the default); 1 the
    # fork's thread_local engine continued from problem to problem (ordered,
    # candidate-serial path)
    rng_stream: int = 0

    @classmethod
    def from_yaml(cls, path: str, camera_yaml: str | None = None, **overrides) -> "LcdParams":
        """Read an OpenCV-FileStorage LcdParams.yaml (the %YAML:1.0 header is
        skipped). `camera_yaml`: a Kimera camera file (LeftCameraParams.yaml)
        whose `intrinsics` fu sets focal_length (the PnP threshold's pixel to
        angle conversion). `overrides` replace yaml keys (by yaml name) or
        dataclass fields before validation. Every key is accounted for: verification
        and BoW keys map onto fields, keys of stages outside the hot path
        (ORB extraction, the PGO back end, the tracker) are ignored by name,
        and anything else, or a value that selects an algorithm this build
        does not have, raises ValueError (no silent fallback)."""
        import yaml
        text = open(path).read()
        if text.startswith("%YAML"):
            text = text.split("\n", 1)[1] if "\n" in text else ""
        y = dict(yaml.safe_load(text) or {})
        if camera_yaml is not None:
            y["focal_length"] = camera_focal_length(camera_yaml)
        y.update(overrides)
        p = cls()
        for k, v in y.items():
            if k in _YAML_FIELDS:
                setattr(p, k, type(getattr(p, k))(v))
            elif k == "matcher_type":
                # OpenCV DescriptorMatcher::MatcherType; 3 is built as BruteForce-L1
                # (docker/copy/kimera_multi_lcd.patch:33-35)
                mt = int(v)
                if mt not in _MATCHER_NORM:
                    raise ValueError(f"matcher_type {mt} is not built (3: L1, 4/5: Hamming)")
                p.norm = _MATCHER_NORM[mt]
            elif k in _YAML_SELECTORS:
                allowed, field = _YAML_SELECTORS[k]
                if int(v) not in allowed:
                    raise ValueError(f"{k}: {v} is not built (supported: {sorted(allowed)})")
                if field:
                    setattr(p, field, int(v))
            elif k in _YAML_IGNORED:
                continue
            elif k in cls.__dataclass_fields__:
                setattr(p, k, v)
            else:
                raise ValueError(f"unknown LcdParams key {k!r}")
        p.validate()
        return p

    def validate(self):
        if self.norm not in ("l1", "hamming"):
            raise ValueError(f"norm {self.norm!r}")
        if self.ransac_2d2d_algorithm not in (ALGO_STEWENIUS, ALGO_NISTER):
            raise ValueError(f"ransac_2d2d_algorithm {self.ransac_2d2d_algorithm} is not built (0 Stewenius, 1 Nister)")
        if self.ransac_2d3d_algorithm != 3:
            raise ValueError("ransac_2d3d_algorithm: only 3 (EPnP) is built")
        if self.pose_recovery_type not in (0, 1):
            raise ValueError(f"pose_recovery_type {self.pose_recovery_type}")
        if self.ransac_use_1point_3d3d not in (0, 1):
            raise ValueError("ransac_use_1point_3d3d is 0 (Arun 3-point) or 1 (given rotation)")
        if self.rng_variant not in ("gcc9", "gcc11"):
            raise ValueError(f"rng_variant {self.rng_variant!r}")
        if self.rng_stream not in (0, 1):
            raise ValueError(f"rng_stream {self.rng_stream}")
        if not 5 <= int(self.nfeatures) <= 1024:
            raise ValueError(f"nfeatures {self.nfeatures}: the frame pool holds 5..1024 features per frame")
        if self.refine_pose not in (0, 1):
            raise ValueError(f"refine_pose {self.refine_pose}")
        if self.refine_pose and self.pose_recovery_type == 1:
            raise ValueError("refine_pose: 1 with pose_recovery_type 1 (PnP) is not built (refinement follows the "
                             "3D-3D recovery); set refine_pose 0")

    def to_c(self) -> abi.LcdParams:
        self.validate()
        c = abi.LcdParams()
        c.norm = abi.KMX_NORM_HAMMING if self.norm == "hamming" else abi.KMX_NORM_L1
        c.lowe_ratio = float(self.lowe_ratio)
        c.min_2d2d_inliers = int(self.min_nr_2d2d_inliers)
        c.min_3d3d_inliers = int(self.min_nr_3d3d_inliers)
        c.ransac_threshold_2d2d = float(self.ransac_threshold_2d2d)
        c.ransac_threshold_3d3d = float(self.ransac_threshold_3d3d)
        c.ransac_max_iterations = int(self.ransac_max_iterations)
        c.ransac_probability = float(self.ransac_probability)
        c.ransac_randomize = int(self.ransac_randomize)
        c.ransac_seed = int(self.ransac_seed)
        c.rng_variant = abi.KMX_RNG_GCC11 if self.rng_variant == "gcc11" else abi.KMX_RNG_GCC9
        c.use_1point_3d3d = int(self.ransac_use_1point_3d3d)
        c.algorithm_2d2d = int(self.ransac_2d2d_algorithm)
        c.refine_pose = int(self.refine_pose)
        c.rng_stream = int(self.rng_stream)
        c.pose_recovery_type = int(self.pose_recovery_type)
        c.min_2d3d_inliers = int(self.min_nr_2d3d_inliers)
        c.ransac_threshold_2d3d = 1.0 - np.cos(np.arctan(float(self.ransac_threshold_2d3d) / float(self.focal_length)))
        return c


ALGO_STEWENIUS = 0
ALGO_NISTER = 1


def camera_focal_length(path: str) -> float:
    """fu of a Kimera camera file (`intrinsics: [fu, fv, cu, cv]`,
    params/D455/LeftCameraParams.yaml:18), the focal length Kimera-VIO's LCD
    converts the PnP pixel threshold with."""
    import yaml
    text = open(path).read()
    if text.startswith("%YAML"):
        text = text.split("\n", 1)[1] if "\n" in text else ""
    y = yaml.safe_load(text) or {}
    intr = y.get("intrinsics")
    if not isinstance(intr, (list, tuple)) or len(intr) < 1:
        raise ValueError(f"{path}: no `intrinsics: [fu, fv, cu, cv]`")
    fu = float(intr[0])
    if not fu > 0.0:
        raise ValueError(f"{path}: fu = {fu}")
    return fu

# yaml keys that are dataclass fields of the same name
_YAML_FIELDS = (
    "lowe_ratio", "min_nr_2d2d_inliers", "min_nr_3d3d_inliers", "ransac_threshold_2d2d",
    "ransac_threshold_3d3d", "ransac_max_iterations", "ransac_probability", "ransac_randomize",
    "ransac_use_1point_3d3d", "pose_recovery_type", "min_nr_2d3d_inliers", "ransac_threshold_2d3d",
    "ransac_2d2d_algorithm", "ransac_2d3d_algorithm",
    "use_nss", "alpha", "min_temporal_matches", "recent_frames_window", "max_db_results",
    "min_nss_factor", "min_matches_per_island", "max_intraisland_gap",
    "max_nrFrames_between_islands", "max_nrFrames_between_queries", "nfeatures")
_MATCHER_NORM = {3: "l1", 4: "hamming", 5: "hamming"}
# switches of verification stages: yaml key -> (built values, field or None)
_YAML_SELECTORS = {
    "refine_pose": ({0, 1}, "refine_pose"),           # stereo pose refinement (LcdParams.yaml:14)
    "ransac_use_2point_2d2d": ({0}, None),            # 2-point 2D-2D given rotation (:59)
    "optimize_2d2d_pose_from_inliers": ({0}, None),   # nonlinear refits (:67-69)
    "optimize_3d3d_pose_from_inliers": ({0}, None),
    "optimize_2d3d_pose_from_inliers": ({0}, None),
}
# keys of stages outside the verification hot path (SURVEY.md §8 out of scope):
# ORB extraction (:19-27), the PGO back end (:29-37), the stereo tracker (:48)
_YAML_IGNORED = frozenset((
    "scale_factor", "nlevels", "edge_threshold", "first_level", "WTA_K", "score_type_id",
    "patch_sze", "fast_threshold", "betweenRotationPrecision", "betweenTranslationPrecision",
    "odom_rot_threshold", "odom_trans_threshold", "pcm_rot_threshold", "pcm_trans_threshold", "gnc_alpha",
    "max_lc_cached_before_optimize", "disparity_threshold"))


@dataclass
class VLCFrame:
    """The visual-loop-closure frame Kimera-Distributed exchanges and hands to
    LoopClosureDetector::addVLCFrame (drawio:2601; pose_graph_tools VLCFrame,
    drawio:441-505), reduced to what verification reads [U field names:
    Kimera-Multi-LCD is not vendored]: its (robot_id, pose_id) vertex, the ORB
    descriptors [n, 32] uint8, the unit bearing vectors ("versors") [n, 3]
    and the stereo keypoints [n, 3] (NaN where a keypoint has no stereo
    depth)."""
    robot_id: int
    pose_id: int
    descriptors: np.ndarray
    versors: np.ndarray
    keypoints: np.ndarray


class _BatchDesc(C.Structure):
    _fields_ = [
        ("n_frames", C.c_int32), ("max_feats", C.c_int32), ("n_feats", C.POINTER(C.c_int32)),
        ("desc", C.POINTER(C.c_uint8)), ("bearings", C.POINTER(C.c_double)), ("points", C.POINTER(C.c_double)),
        ("n_cand", C.c_int32), ("cand_query", C.POINTER(C.c_int32)), ("cand_match", C.POINTER(C.c_int32)),
    ]


class LoopClosureDetector:
    """GPU verification of loop-closure candidates over a resident frame pool
    (the VLC frames Kimera-Distributed holds, drawio:441-505)."""

    def __init__(self, params: LcdParams | None = None, device: int = 0):
        self.params = params or LcdParams()
        L = abi.lib()
        if abi.device_count() <= device:
            raise abi.KmxError(f"no HIP device {device} visible (kmx has no CPU fallback)")
        self._c = self.params.to_c()
        h = C.c_void_p()
        check(L.kmx_lcd_create(C.byref(self._c), device, C.byref(h)), "kmx_lcd_create")
        self.h, self.L = h, L
        self.max_feats = 0
        self.n_frames = 0
        self._vertex = {}  # (robot_id, pose_id) -> frame id in the pool

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.L.kmx_lcd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream: int):
        check(self.L.kmx_lcd_set_stream(self.h, C.c_void_p(hip_stream)), "kmx_lcd_set_stream")

    def set_frames(self, n_feats, desc, bearings, points):
        """Upload the frame pool: desc uint8 [F, N, 32], bearings / points float64 [F, N, 3]."""
        nf = np.ascontiguousarray(n_feats, dtype=np.int32)
        de = np.ascontiguousarray(desc, dtype=np.uint8)
        be = np.ascontiguousarray(bearings, dtype=np.float64)
        pt = np.ascontiguousarray(points, dtype=np.float64)
        F, N = de.shape[0], de.shape[1]
        if de.shape != (F, N, 32) or be.shape != (F, N, 3) or pt.shape != (F, N, 3) or nf.shape != (F,):
            raise ValueError("frame pool shapes must be desc [F,N,32], bearings/points [F,N,3], n_feats [F]")
        d = _BatchDesc()
        d.n_frames, d.max_feats = F, N
        d.n_feats = nf.ctypes.data_as(C.POINTER(C.c_int32))
        d.desc = de.ctypes.data_as(C.POINTER(C.c_uint8))
        d.bearings = be.ctypes.data_as(C.POINTER(C.c_double))
        d.points = pt.ctypes.data_as(C.POINTER(C.c_double))
        check(self.L.kmx_lcd_set_frames(self.h, C.byref(d)), "kmx_lcd_set_frames")
        self.max_feats = N
        self.n_frames = F
        self._vertex = {}

    def set_pool(self, pool):
        self.set_frames(pool.n_feats, pool.desc, pool.bearings, pool.points)

    # ------------------------------------------------ streaming frame pool --
    def add_frames(self, n_feats, desc, bearings, points) -> int:
        """Append frames to the resident pool (kmx_lcd_add_frames: capacity
        doubling on the device, resident frames never re-uploaded, the sampler
        table kept). Arrays as set_frames; the stride N must equal the pool's
        (on an empty detector it sets it). Returns the first new frame id."""
        nf = np.ascontiguousarray(n_feats, dtype=np.int32)
        de = np.ascontiguousarray(desc, dtype=np.uint8)
        be = np.ascontiguousarray(bearings, dtype=np.float64)
        pt = np.ascontiguousarray(points, dtype=np.float64)
        F, N = de.shape[0], de.shape[1]
        if de.shape != (F, N, 32) or be.shape != (F, N, 3) or pt.shape != (F, N, 3) or nf.shape != (F,):
            raise ValueError("frame shapes must be desc [F,N,32], bearings/points [F,N,3], n_feats [F]")
        first = C.c_int32()
        check(self.L.kmx_lcd_add_frames(self.h, F, N, abi.iptr(nf), abi.u8ptr(de), abi.fptr(be), abi.fptr(pt),
                                        C.byref(first)), "kmx_lcd_add_frames")
        self.max_feats = N
        self.n_frames = first.value + F
        return first.value

    def pool_info(self) -> dict:
        f, cap, n = C.c_int32(), C.c_int32(), C.c_int32()
        check(self.L.kmx_lcd_pool_info(self.h, C.byref(f), C.byref(cap), C.byref(n)), "kmx_lcd_pool_info")
        return {"n_frames": f.value, "capacity": cap.value, "max_feats": n.value}

    def bow_vectors(self, gpu_vocabulary, frame_ids):
        """BowVectors (CSR vptr, words, weights) of resident frames, made on
        the device from the pool's descriptors by a
        kmx.lcd.vocabulary.GpuVocabulary (no second upload)."""
        return gpu_vocabulary.transform_pool(self, frame_ids)

    def addVLCFrame(self, frame: VLCFrame) -> int:
        """LoopClosureDetector::addVLCFrame (drawio:2601): the frame joins the
        device pool (padded to the pool's feature stride, `nfeatures` of
        LcdParams on an empty detector) and its (robot_id, pose_id) vertex
        maps to the returned frame id."""
        N = self.max_feats or int(self.params.nfeatures)
        d = np.asarray(frame.descriptors, np.uint8)
        n = d.shape[0]
        if n > N:
            raise ValueError(f"frame has {n} features, the pool's stride is {N}")
        de = np.zeros((1, N, 32), np.uint8)
        be = np.zeros((1, N, 3))
        pt = np.full((1, N, 3), np.nan)
        de[0, :n] = d
        be[0, :n] = np.asarray(frame.versors, np.float64)
        pt[0, :n] = np.asarray(frame.keypoints, np.float64)
        fid = self.add_frames(np.array([n], np.int32), de, be, pt)
        self._vertex[(int(frame.robot_id), int(frame.pose_id))] = fid
        return fid

    def frame_id(self, vertex) -> int:
        """Pool id of a vertex: an int frame id, or a (robot_id, pose_id) added
        by addVLCFrame."""
        if isinstance(vertex, (tuple, list)):
            return self._vertex[(int(vertex[0]), int(vertex[1]))]
        return int(vertex)

    # ------------------------------------------- reference-shaped single calls --
    # the one-candidate entry points with raw-address arguments (ctypes'
    # data_as costs ~6 us per array, more than the kernels it feeds)
    _VP = C.c_void_p
    _VM1 = C.CFUNCTYPE(C.c_int, _VP, C.c_int32, _VP, _VP, _VP, _VP, _VP, C.c_int, _VP, _VP, _VP)
    _M1 = C.CFUNCTYPE(C.c_int, _VP, C.c_int32, _VP, _VP, _VP, _VP)

    def _one(self):
        """Buffers, addresses and call objects of the one-candidate calls, made
        once per pool stride: the reference's verification thread makes three
        calls per candidate (verifyLoopSpin, drawio:2638-2657), so their host
        side is kept to filling two ids, a count and the pairs."""
        N = max(self.max_feats, 1)
        o = getattr(self, "_one_bufs", None)
        if o is None or o["N"] != N:
            o = {"N": N, "cq": np.zeros(1, np.int32), "cm": np.zeros(1, np.int32),
                 "mptr": np.zeros(2, np.int64), "pairs": np.zeros((1, N, 2), np.int32), "k": np.zeros(1, np.int32),
                 "masks": np.zeros((1, N), np.uint8), "res": (abi.LcdResult * 1)(),
                 "iq": np.zeros(N, np.int32), "im": np.zeros(N, np.int32), "prior": np.zeros(12, np.float64),
                 "T": np.eye(4)}
            a = {k: o[k].ctypes.data for k in ("cq", "cm", "mptr", "pairs", "k", "masks", "iq", "im", "prior")}
            a["res"] = C.addressof(o["res"])
            o["a"] = a
            o["vm"] = self._VM1(("kmx_lcd_verify_matches", self.L))
            o["m"] = self._M1(("kmx_lcd_match", self.L))
            o["t12"] = np.frombuffer(o["res"][0].T_query_match, np.float64)
            self._one_bufs = o
        return o

    def _verify_one(self, vertex_query, vertex_match, iq, im, stages, prior=None):
        """kmx_lcd_verify_matches for one candidate through the _one buffers:
        (result record, inlier-mask row over the given pairs; both views of
        the buffers, valid until the next call)."""
        o = self._one()
        n = len(iq)
        if len(im) != n:
            raise ValueError("i_query and i_match differ in length")
        if n > o["N"]:
            raise ValueError("more pairs than the pool's max_feats")
        o["cq"][0], o["cm"][0] = self.frame_id(vertex_query), self.frame_id(vertex_match)
        o["mptr"][1] = n
        o["iq"][:n] = iq
        o["im"][:n] = im
        a = o["a"]
        pa = None
        if prior is not None:
            o["prior"][:] = prior
            pa = a["prior"]
        check(o["vm"](self.h, 1, a["cq"], a["cm"], a["mptr"], a["iq"], a["im"], int(stages), pa, a["res"], a["masks"]),
              "kmx_lcd_verify_matches")
        return o["res"][0], o["masks"][0, :n]

    _T4_POS = np.array([0, 1, 2, 4, 5, 6, 8, 9, 10, 3, 7, 11])  # (R row-major, t) -> [R | t] rows

    def _T4_one(self):
        """T_query_match of the last one-candidate result as a fresh 4x4."""
        o = self._one_bufs
        T = o["T"].copy()
        T.ravel()[self._T4_POS] = o["t12"]
        return T

    def computeMatchedIndices(self, vertex_query, vertex_match):
        """LoopClosureDetector::computeMatchedIndices (drawio:2583-2586) on two
        resident frames: (i_query, i_match) int32 arrays in query order."""
        o = self._one()
        o["cq"][0], o["cm"][0] = self.frame_id(vertex_query), self.frame_id(vertex_match)
        a = o["a"]
        check(o["m"](self.h, 1, a["cq"], a["cm"], a["pairs"], a["k"]), "kmx_lcd_match")
        k = int(o["k"][0])
        return o["pairs"][0, :k, 0].copy(), o["pairs"][0, :k, 1].copy()

    def geometricVerificationNister(self, vertex_query, vertex_match, i_query, i_match):
        """geometricVerificationNister (drawio:2589-2592): the 2D-2D RANSAC on
        the given correspondences. Returns (ok, i_query_inliers,
        i_match_inliers, T_query_match 4x4 with unit-norm t); ok = at least
        min_nr_2d2d_inliers inliers. The inlier lists are what the reference
        writes back into i_query / i_match."""
        iq = np.asarray(i_query, np.int32)
        im = np.asarray(i_match, np.int32)
        r, mask = self._verify_one(vertex_query, vertex_match, iq, im, abi.KMX_LCD_STAGE_2D2D)
        keep = (mask & 1).view(bool)
        return bool(r.accepted), iq[keep], im[keep], self._T4_one()

    def recoverPose(self, vertex_query, vertex_match, i_query, i_match, T_query_match_mono=None):
        """recoverPose (drawio:2595-2598) on geometricVerificationNister's
        inliers: the 3D-3D recovery (1-point given the 2D-2D rotation of
        T_query_match_mono, or Arun) or EPnP, per LcdParams. Returns (ok,
        T_query_match 4x4, inlier mask over the given pairs)."""
        iq = np.asarray(i_query, np.int32)
        im = np.asarray(i_match, np.int32)
        prior = None
        if T_query_match_mono is not None:
            T = np.asarray(T_query_match_mono, np.float64)
            prior = self._one()["prior"]
            prior[:] = T[:3].ravel()[self._T4_POS]
        r, mask = self._verify_one(vertex_query, vertex_match, iq, im, abi.KMX_LCD_STAGE_RECOVER, prior)
        return bool(r.accepted), self._T4_one(), (mask & 2) != 0

    # --------------------------------------------------------------- batched --
    def match(self, cand_query, cand_match):
        """Batched computeMatchedIndices on resident frames (kmx_lcd_match):
        pairs [n, max_feats, 2] int32 and k [n]."""
        cq = np.ascontiguousarray(cand_query, dtype=np.int32)
        cm = np.ascontiguousarray(cand_match, dtype=np.int32)
        n = cq.shape[0]
        pairs = np.zeros((max(n, 1), max(self.max_feats, 1), 2), np.int32)
        k = np.zeros(max(n, 1), np.int32)
        check(self.L.kmx_lcd_match(self.h, n, abi.iptr(cq), abi.iptr(cm), abi.iptr(pairs), abi.iptr(k)),
              "kmx_lcd_match")
        return pairs[:n], k[:n]

    def verify_matches(self, cand_query, cand_match, correspondences, stages: int = 3, T_prior=None,
                       with_masks: bool = False):
        """geometricVerificationNister and / or recoverPose on caller-supplied
        correspondences (kmx_lcd_verify_matches), batched: correspondences[i] =
        (i_query, i_match) of candidate i; stages a mask of
        abi.KMX_LCD_STAGE_2D2D / _RECOVER; T_prior [n, 12] (R row-major, t) is
        the rotation source of the 1-point recovery without the 2D-2D stage.
        Returns (results, masks) as verify, masks indexed by pair position."""
        n = len(cand_query)
        if len(correspondences) != n:
            raise ValueError("one (i_query, i_match) pair list per candidate")
        lens = [len(np.asarray(a)) for a, _ in correspondences]
        for (a, b), k in zip(correspondences, lens):
            if len(np.asarray(b)) != k:
                raise ValueError("i_query and i_match differ in length")
        mptr = np.zeros(n + 1, np.int64)
        mptr[1:] = np.cumsum(lens)
        iq = np.concatenate([np.asarray(a, np.int32) for a, _ in correspondences]) if n else np.zeros(0, np.int32)
        im = np.concatenate([np.asarray(b, np.int32) for _, b in correspondences]) if n else np.zeros(0, np.int32)
        return self.verify_matches_csr(cand_query, cand_match, mptr, iq, im, stages, T_prior, with_masks)

    def verify_matches_csr(self, cand_query, cand_match, mptr, i_query, i_match, stages: int = 3, T_prior=None,
                           with_masks: bool = False, as_arrays: bool = False):
        """verify_matches with the correspondences already in CSR form: candidate
        i's pairs are (i_query[k], i_match[k]) for k in [mptr[i], mptr[i+1])
        (kmx_lcd_verify_matches' own layout; no per-candidate Python lists).
        as_arrays: the results as one structured array (verify_arrays' form)
        instead of a list of dicts."""
        cq = np.ascontiguousarray(cand_query, dtype=np.int32)
        cm = np.ascontiguousarray(cand_match, dtype=np.int32)
        n = cq.shape[0]
        mptr = np.ascontiguousarray(mptr, np.int64)
        if mptr.shape != (n + 1,):
            raise ValueError("mptr must have n_cand + 1 entries")
        iq = np.ascontiguousarray(i_query, np.int32)
        im = np.ascontiguousarray(i_match, np.int32)
        if iq.shape != im.shape:
            raise ValueError("i_query and i_match differ in length")
        if iq.size == 0:
            iq = np.zeros(1, np.int32)
            im = np.zeros(1, np.int32)
        pr = None
        if T_prior is not None:
            pr = np.ascontiguousarray(T_prior, np.float64).reshape(n, 12)
        res = (abi.LcdResult * max(n, 1))()
        masks = np.zeros((max(n, 1), max(self.max_feats, 1)), np.uint8) if with_masks else None
        check(self.L.kmx_lcd_verify_matches(self.h, n, abi.iptr(cq), abi.iptr(cm), abi.i64ptr(mptr), abi.iptr(iq),
                                            abi.iptr(im), int(stages), abi.fptr(pr) if pr is not None else None,
                                            res, abi.u8ptr(masks) if with_masks else None),
              "kmx_lcd_verify_matches")
        out = np.frombuffer(res, dtype=_RES_DT, count=n).copy() if as_arrays else _results(res, n, self._refines(stages))
        return out, (masks[:n] if with_masks else None)

    def verify(self, cand_query, cand_match, with_masks: bool = False):
        """Verify candidates; returns (list of result dicts, masks or None).
        masks[c, j]: bit0 = 2D-2D inlier, bit1 = 3D-3D inlier, j = position in
        the candidate's match list (computeMatchedIndices order)."""
        cq = np.ascontiguousarray(cand_query, dtype=np.int32)
        cm = np.ascontiguousarray(cand_match, dtype=np.int32)
        n = cq.shape[0]
        res = (abi.LcdResult * max(n, 1))()
        masks = np.zeros((n, self.max_feats), np.uint8) if with_masks else None
        check(self.L.kmx_lcd_verify(self.h, n, cq.ctypes.data_as(C.POINTER(C.c_int32)),
                                    cm.ctypes.data_as(C.POINTER(C.c_int32)), res,
                                    masks.ctypes.data_as(C.POINTER(C.c_uint8)) if with_masks else None),
              "kmx_lcd_verify")
        return _results(res, n, self._refines(3)), masks

    def verify_arrays(self, cand_query, cand_match):
        """verify without per-candidate Python objects: the kmx_lcd_result
        records as one numpy structured array (fields as kmx_lcd_result:
        n_matches, mono_inliers, stereo_inliers, accepted, iterations_2d2d,
        pnp_inliers, T_query_match [12]) — the form for large batches, whose
        dicts would cost more host time than the verification itself."""
        cq = np.ascontiguousarray(cand_query, dtype=np.int32)
        cm = np.ascontiguousarray(cand_match, dtype=np.int32)
        n = cq.shape[0]
        res = (abi.LcdResult * max(n, 1))()
        check(self.L.kmx_lcd_verify(self.h, n, cq.ctypes.data_as(C.POINTER(C.c_int32)),
                                    cm.ctypes.data_as(C.POINTER(C.c_int32)), res, None), "kmx_lcd_verify")
        return np.frombuffer(res, dtype=_RES_DT, count=n).copy()

    def _refines(self, stages: int) -> bool:
        p = self.params
        return bool(p.refine_pose) and p.pose_recovery_type == 0 and bool(stages & abi.KMX_LCD_STAGE_RECOVER)

    def verify_async(self, cand_query, cand_match):
        cq = np.ascontiguousarray(cand_query, dtype=np.int32)
        cm = np.ascontiguousarray(cand_match, dtype=np.int32)
        check(self.L.kmx_lcd_verify_async(self.h, cq.shape[0], cq.ctypes.data_as(C.POINTER(C.c_int32)),
                                          cm.ctypes.data_as(C.POINTER(C.c_int32))), "kmx_lcd_verify_async")

    def sync(self):
        check(self.L.kmx_lcd_sync(self.h), "kmx_lcd_sync")

    def enable_timing(self, on: bool = True):
        check(self.L.kmx_lcd_enable_timing(self.h, 1 if on else 0), "kmx_lcd_enable_timing")

    def read_timing(self) -> dict:
        """Device times (ms) of the kNN2 and RANSAC launches of the last evented
        verification."""
        a, b = C.c_double(), C.c_double()
        check(self.L.kmx_lcd_read_timing(self.h, C.byref(a), C.byref(b)), "kmx_lcd_read_timing")
        return {"knn_ms": a.value, "ransac_ms": b.value}

    # computeMatchedIndices on two descriptor sets (single pair)
    @staticmethod
    def compute_matched_indices(desc_query, desc_match, lowe_ratio: float = 0.7, norm: str = "l1"):
        q = np.ascontiguousarray(desc_query, dtype=np.uint8)
        m = np.ascontiguousarray(desc_match, dtype=np.uint8)
        pairs = np.empty((max(q.shape[0], 1), 2), np.int32)
        k = C.c_int32()
        nrm = abi.KMX_NORM_HAMMING if norm == "hamming" else abi.KMX_NORM_L1
        check(abi.lib().kmx_lcd_knn2(nrm, float(lowe_ratio), q.ctypes.data_as(C.POINTER(C.c_uint8)), q.shape[0],
                                     m.ctypes.data_as(C.POINTER(C.c_uint8)), m.shape[0],
                                     pairs.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(k)),
              "kmx_lcd_knn2")
        return pairs[: k.value, 0].copy(), pairs[: k.value, 1].copy()


_RES_DT = np.dtype(abi.LcdResult)


def _results(res, n: int, refines: bool = False) -> list:
    """Result records; pose_refined marks an accepted 3D-3D pose that went
    through the restated refine_pose refit (a substitute, parity unpinned).
    Read column by column from a numpy view of the records (a ctypes field
    access per value cost ~2 us per candidate)."""
    a = np.frombuffer(res, dtype=_RES_DT, count=n)
    T = a["T_query_match"].copy()
    cols = [a[k].tolist() for k in ("n_matches", "mono_inliers", "stereo_inliers", "pnp_inliers", "accepted",
                                     "iterations_2d2d")]
    return [{"n_matches": nm, "mono_inliers": mo, "stereo_inliers": st, "pnp_inliers": pn, "accepted": bool(ac),
             "iterations_2d2d": it, "T_query_match": t, "pose_refined": bool(refines and ac)}
            for nm, mo, st, pn, ac, it, t in zip(*cols, list(T))]


def _T4(t12) -> np.ndarray:
    T = np.eye(4)
    T[:3, :4] = np.ctypeslib.as_array(t12, (12,))[[0, 1, 2, 9, 3, 4, 5, 10, 6, 7, 8, 11]].reshape(3, 4)
    return T
