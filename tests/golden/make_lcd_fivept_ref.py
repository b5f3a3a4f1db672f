"""Writes tests/golden/lcd_fivept_ref.npz: the high-precision 5-point reference
(tests/lcd_fivept_ref.py) on the planted samples of tests/lcd_scenes.py, so the
suite reads four minutes of mpmath from a file. Per family (general, a, c, d,
e, h, i, j), 30 samples:

  f1, f2  [30, 5, 3]      the sample's bearings (the test checks they are the scenes')
  E       [30, 10, 3, 3]  the reference's ten solutions (40 digits; 80 on a and c)
  eig     [30, 10]        complex: their eigenvalues
  real    [30, 10]        bool
  sep     [30, 10]        distance of eig to the nearest other eigenvalue
  kappa   [30, 10]        condition estimate (NaN for complex solutions)
  E16     [30, 10, 3, 3]  the same formulation run at 16 digits

tests/test_lcd_geometry_cpu.py recomputes two samples per family and fails if
the file no longer follows the reference or the scenes.

    python tests/golden/make_lcd_fivept_ref.py
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parents[1] / "kimera-multi_amd"))

import lcd_fivept_ref as REF  # noqa: E402
import lcd_scenes as S  # noqa: E402

FAMILIES = ["general", "a", "c", "d", "e", "h", "i", "j"]
# 40 digits reproduce the 120-digit solutions to the last bit of a double on every family but a (zero baseline:
# first-digit differences at 40, none at 80) and c (baseline 1e-6: 1e-15 at 40, none at 80)
REF_DPS = {"a": 80, "c": 80}
N_SAMPLES = 30
SAMPLE_SEED = 7


def samples(fam):
    pool = S.general() if fam == "general" else S.FAMILIES[fam]()
    return S.planted_samples(pool, N_SAMPLES, seed=SAMPLE_SEED)


def record(fam, s, f1, f2):
    """One sample's record, as the arrays of the file."""
    sols = REF.solve_with_condition(f1, f2, seed=s, dps=REF_DPS.get(fam, 40))
    lo = REF.solve(f1, f2, dps=16)
    return {"f1": f1, "f2": f2, "E": np.array([x.E for x in sols]), "eig": np.array([x.eig for x in sols]),
            "real": np.array([x.real for x in sols]), "sep": np.array([x.sep for x in sols]),
            "kappa": np.array([x.kappa for x in sols]), "E16": np.array([x.E for x in lo])}


def main():
    out = {}
    for fam in FAMILIES:
        recs = [record(fam, s, f1, f2) for s, (f1, f2, _) in enumerate(samples(fam))]
        for k in recs[0]:
            out[f"{fam}_{k}"] = np.stack([r[k] for r in recs])
        print(fam, "done", flush=True)
    np.savez_compressed(HERE / "lcd_fivept_ref.npz", **out)


if __name__ == "__main__":
    main()
