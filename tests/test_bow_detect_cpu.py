"""detectLoop decided on the device, the part that needs no device: the header
declares the new entry points, the library exports them, kmx/abi.py binds them,
and both sides agree on the record, the parameters and the status order. The
ABI version stays 10: everything here is additive."""
import ctypes as C
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

NEW_SYMBOLS = ("kmx_bow_detect_entries", "kmx_bow_detect_entries_async", "kmx_bow_detect_fetch",
               "kmx_bow_decide_results", "kmx_bow_get_temporal_state", "kmx_bow_set_temporal_state",
               "kmx_bow_enable_timing", "kmx_bow_read_detect_timing")


def test_detect_symbols_declared_exported_and_bound():
    from kmx import abi
    L = abi.lib()
    hdr = (ROOT / "include" / "kmx_abi.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(kmx_\w+)\s*\(", hdr, re.M))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name  # bound in kmx/abi.py
    assert int(re.search(r"#define\s+KMX_ABI_VERSION\s+(\d+)", hdr).group(1)) == abi.ABI_VERSION == 10


def test_record_params_and_status_order_match_the_header():
    from kmx import abi
    hdr = (ROOT / "include" / "kmx_abi.h").read_text()
    for struct, cls in (("kmx_bow_detect_params", abi.BowDetectParams), ("kmx_bow_detect_record", abi.BowDetectRecord)):
        body = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", hdr).group(1)
        fields = re.findall(r"^\s*(int32_t|double)\s+(\w+);", body, re.M)
        assert [(n, C.c_int32 if t == "int32_t" else C.c_double) for t, n in fields] == list(cls._fields_), struct
    assert C.sizeof(abi.BowDetectRecord) == 48 == abi.BOW_RECORD_DTYPE.itemsize
    assert [abi.BOW_RECORD_DTYPE.fields[n][1] for n, _ in abi.BowDetectRecord._fields_] == \
        [getattr(abi.BowDetectRecord, n).offset for n, _ in abi.BowDetectRecord._fields_]
    status = re.findall(r"KMX_BOW_(\w+) = (\d)", hdr)
    order = [n for n, _ in sorted(((n, int(v)) for n, v in status if not n.startswith("MODE_")), key=lambda t: t[1])]
    assert tuple(order) == abi.BOW_STATUS
    assert ("MODE_INTRA", "0") in status and ("MODE_INTER", "1") in status
    assert (abi.BOW_MODE_INTRA, abi.BOW_MODE_INTER) == (0, 1)


def test_detector_params_come_from_lcdparams():
    from kmx.lcd import LcdParams
    from kmx.lcd.bow import BowDetector
    p = LcdParams(alpha=0.25, max_db_results=77, use_nss=0, min_temporal_matches=3)
    c = BowDetector(p, n_words=100).detect_params()
    assert (c.alpha, c.max_db_results, c.use_nss, c.min_temporal_matches) == (0.25, 77, 0, 3)
    assert (c.min_nss_factor, c.recent_frames_window, c.max_intraisland_gap, c.min_matches_per_island,
            c.max_nrFrames_between_queries, c.max_nrFrames_between_islands) == (0.05, 100, 3, 1, 2, 3)
