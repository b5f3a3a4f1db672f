"""The owning device buffer every handle is made of (devbuf.h: move, swap,
reset, alloc, put, grow_keep and the commit by move of the set_graph-style
calls) needs no GPU: `make devbuf_check` runs it over a host backend under the
host sanitizers."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_make_devbuf_check():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc is missing")
    r = subprocess.run(["make", "-s", "-C", str(ROOT / "kimera-multi_amd" / "csrc"), "devbuf_check", f"HIPCC={hipcc}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "devbuf_check ok" in r.stdout
