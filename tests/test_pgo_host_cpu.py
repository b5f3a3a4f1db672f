"""pgo.hip's host code (pgo_host.h: the graph checks and the plan of
kmx_pgo_set_graph) needs no GPU: `make pgo_check` runs it under the host
sanitizers."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_make_pgo_check():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc is missing")
    r = subprocess.run(["make", "-s", "-C", str(ROOT / "kimera-multi_amd" / "csrc"), "pgo_check", f"HIPCC={hipcc}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pgo_check ok" in r.stdout
