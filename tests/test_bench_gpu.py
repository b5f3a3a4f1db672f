"""bench.py's plain run: the headline figure alone, and --dump-outputs."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_plain_run_is_the_default():
    sys.path.insert(0, str(ROOT))
    import bench
    old = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
        a = bench.parse()
    finally:
        sys.argv = old
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)


@pytest.mark.gpu
def test_plain_run_result_line_and_outputs(gpu, tmp_path):
    """One plain run (3 timed rounds of configs[3]): the result line holds the
    headline keys and none of the --full legs, and --dump-outputs writes every
    robot's iterate, the GNC weights and the status words as finite float64
    arrays of the graph's sizes."""
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert (d["unit"], d["higher_is_better"], d["dtype"], d["steps"], d["warmup"]) == \
        ("edges*iters/s", True, "f64", 3, 1)
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert not {"roofline", "parity", "cpu_baseline", "lcd"} & set(d)
    names = sorted(f.name for f in out.glob("*.npy"))
    assert names == sorted([f"iterate_robot{a}.npy" for a in range(8)] + ["gnc_weights.npy", "status.npy"])
    total = 0
    for a in range(8):
        X = np.load(out / f"iterate_robot{a}.npy")
        assert X.dtype == np.float64 and X.shape == (12500, 5, 4) and np.isfinite(X).all()
        # the rotation part of every lifted pose stays on the Stiefel manifold
        # (a retraction in fp64: a few ulp of entries of size <= 1)
        Yr = X[:, :, :3]
        assert np.abs(np.einsum("nji,njk->nik", Yr, Yr) - np.eye(3)).max() < 1e-12
        total += X.nbytes
    w = np.load(out / "gnc_weights.npy")
    assert w.dtype == np.float64 and w.shape == (500000,) and ((w >= 0) & (w <= 1)).all()
    s = np.load(out / "status.npy")
    assert s.dtype == np.float64 and s.shape == (8,)
    assert total + w.nbytes + s.nbytes <= 64 * 2**20
