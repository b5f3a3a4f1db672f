"""The rounding fixture (tests/golden/rounding_ref.npz) and the CPU restatement
of the rounding and of the Stiefel projection against it; no GPU needed. The
bounds are those of tests/rounding_ref.py."""
from pathlib import Path

import numpy as np
import pytest

from tests import rounding_ref as REF

ROOT = Path(__file__).resolve().parents[1]


def test_fixture_is_self_consistent():
    """The numpy fp64 route is within the measured (unscaled) ratios on every
    pose, the constants are 4 x them, and every case of the generator is there."""
    cases, K = REF.load()
    assert sorted(cases) == list(REF.RANKS) and cases[5].n == 300
    for k in "ROP":
        assert K["K_" + k] == 4 * K["ratio_" + k] and 1 <= K["ratio_" + k] < 100
    for r, c in cases.items():
        assert c.X.shape == (c.n, r, 4) and c.anchors.shape[1:] == (r, 4)
        assert {0, 1, 2, 3} == set(c.rank.tolist()) and set(c.d.tolist()) == {-1, 1}
        assert (np.diff(c.sig, axis=1) <= 0).all() and (np.diff(c.psig, axis=1) <= 0).all()
        assert np.abs(c.anchors[:, :, 3]).min() > 0
        val, orth, det, tr = REF.rotation_ratios(c, REF.np_trajectory(c))
        pval, porth = REF.polar_ratios(c, REF.np_project(c))
        assert val.max() <= K["ratio_R"] and pval.max() <= K["ratio_P"]
        assert max(orth.max(), porth.max()) <= K["ratio_O"]
        assert (det > 0).all() and tr.max() <= 1
        # passing means something: the bound is below 1e-3 wherever the answer is unique
        for i in range(c.n):
            if c.rank[i] >= 2:
                assert K["K_R"] * REF.rotation_unit(c, i) < 1e-3


def test_fixture_follows_the_generator():
    """A sample of poses, recomputed with mpmath, equals the stored truth."""
    pytest.importorskip("mpmath")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_rounding_ref", REF.FIXTURE.with_name("make_rounding_ref.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    cases, _ = REF.load()
    for r, c in cases.items():
        for i in list(range(0, c.n, 17)) + [int(p) for p in c.deg[:4]]:
            rec = gen.truth(c.anchor(i), c.X[i])
            for k in ("sig", "R", "t", "psig", "pY"):
                assert np.array_equal(rec[k], getattr(c, k)[i]), (r, i, k)
            assert rec["d"] == c.d[i]
            if i in c.deg:
                U, V, pV = c.uv(i)
                assert np.array_equal(rec["U"], U) and np.array_equal(rec["V"], V) and np.array_equal(rec["pV"], pV)


@pytest.mark.parametrize("r", REF.RANKS)
def test_oracle_meets_the_contract(r):
    """The CPU restatement (oracle/dpgo_oracle.c: proj_so3, proj_stiefel) is the
    same algorithm as the device's: it meets the bounds before any GPU run."""
    from kmx import abi
    from kmx.dpgo.params import PGOAgentParameters
    from oracle.oracle import OraclePGO
    cases, K = REF.load()
    c = cases[r]
    o = OraclePGO(PGOAgentParameters(r=r).to_c(), REF.chain_graph(c.n))
    o.set_iterate(0, c.X)
    traj = np.empty((c.n, 12))
    for g in range(c.anchors.shape[0]):
        full = o.trajectory(0, c.anchors[g])
        REF.assert_rotations(full, K, f"oracle, anchor {g}")
        traj[c.aid == g] = full[c.aid == g]
    REF.check_trajectory(c, traj, K, "oracle")
    out, _ = o.eval(0, abi.KMX_EVAL_PROJECT, c.X)
    REF.check_projection(c, out, K, "oracle")


def test_make_project_check():
    """so3_project.h on the CPU under the host sanitizers (`make project_check`)."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc is missing")
    r = subprocess.run(["make", "-s", "-C", str(ROOT / "kimera-multi_amd" / "csrc"), "project_check", f"HIPCC={hipcc}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "project_check ok" in r.stdout
