"""Streaming BoW database (ABI 10), the part that needs no device: the library
exports the new entry points and both sides agree on the ABI version."""
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

NEW_SYMBOLS = ("kmx_bow_reset", "kmx_bow_add_entries", "kmx_bow_add_from_voc", "kmx_bow_seal",
               "kmx_bow_set_tail_cap", "kmx_bow_info", "kmx_bow_get_entries", "kmx_bow_query_entries",
               "kmx_bow_query_entries_async", "kmx_bow_fetch", "kmx_bow_score_entries")


def test_new_symbols_declared_and_exported():
    from kmx import abi
    L = abi.lib()
    hdr = (ROOT / "include" / "kmx_abi.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(kmx_\w+)\s*\(", hdr, re.M))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name  # bound in kmx/abi.py


def test_abi_version_is_10_on_both_sides():
    from kmx import abi
    hdr = (ROOT / "include" / "kmx_abi.h").read_text()
    assert int(re.search(r"#define\s+KMX_ABI_VERSION\s+(\d+)", hdr).group(1)) == 10
    assert abi.ABI_VERSION == 10
    assert abi.lib().kmx_abi_version() == 10


def test_bow_database_needs_a_device():
    """An ordinal past the visible devices (all of them on a host without a
    GPU): no CPU fallback."""
    from kmx import abi
    from kmx.lcd.bow import BowDatabase
    with pytest.raises(abi.KmxError):
        BowDatabase(1000, device=abi.device_count())
