"""The host side of the device simplification (simplify_host.h: the parameter,
append and keyframe checks, the voxel division, the window's floor division,
the table-size rule) needs no GPU: `make simplify_check` runs it under the
host sanitizers. And the names the feature adds import without a device."""
import inspect
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_make_simplify_check():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc is missing")
    r = subprocess.run(["make", "-s", "-C", str(ROOT / "kimera-multi_amd" / "csrc"), "simplify_check",
                        f"HIPCC={hipcc}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "simplify_check ok" in r.stdout


def test_new_names_import():
    from kmx import abi, pipeline
    from kmx.pgmo import MeshSimplifier, simplify_voxel_gpu
    from kmx.pgmo.simplify import horizon_to_ns
    assert {"add", "control", "vertex_map", "faces", "edges", "graph", "info", "timing", "close"} <= set(dir(MeshSimplifier))
    assert callable(simplify_voxel_gpu)
    assert [n for n, _ in abi.SimplifyParams._fields_] == ["resolution", "horizon_ns", "n_robots", "initial_slots"]
    assert inspect.signature(pipeline.deform_mesh).parameters["graph_simplify"].default == "host"
    assert inspect.signature(pipeline.run_pipeline).parameters["mesh_graph_simplify"].default == "host"
    assert horizon_to_ns(None) == 0 and horizon_to_ns(2.0) == 2_000_000_000
    with pytest.raises(ValueError):
        horizon_to_ns(0.0)
