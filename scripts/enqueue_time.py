"""Host enqueue time per round against the GPU's round time (configs[3], 1 GPU).

iterate_async(n) returns once the host has enqueued n rounds; the handle's
stream drains later. With robot groups (KMX_TCG_GROUPS) the host launches each
group's kernels, so its time per round grows with the group count and must stay
below the GPU's, or the streams run dry. Blind tCG enqueueing (set_tcg_poll(0)):
the host never waits inside a round, so the first figure is launch cost alone.
usage: KMX_TCG_GROUPS=g python scripts/enqueue_time.py [rounds]
"""
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "kimera-multi_amd"))
sys.path.insert(0, str(ROOT))

import bench
from kmx.dpgo.solver import BlockSolver
from kmx.synth import config, lift, lifting_matrix

n_rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 40  # few enough that no queue fills and throttles the host
g = config("synth100k", seed=0)
P = bench.params()
Y = lifting_matrix(P.r, seed=1)
s = BlockSolver(P, 0)
s.set_tcg_poll(0)
s.set_graph_data(g)
s.set_gnc_schedule(True, P.robustOptInnerIters, P.robustOptNumWeightUpdates, P.relChangeTol)
for a in range(g.n_robots):
    s.set_iterate(a, lift(g.init_R[a], g.init_t[a], Y))
s.iterate_async(45, refresh_local=True)
s.sync()
for rep in range(3):
    t0 = time.perf_counter()
    s.iterate_async(n_rounds, refresh_local=False)
    t1 = time.perf_counter()
    s.sync()
    t2 = time.perf_counter()
    print(f"groups {s.tcg_groups()} (KMX_TCG_GROUPS={os.environ.get('KMX_TCG_GROUPS', 'default')}): "
          f"host enqueue {1e6 * (t1 - t0) / n_rounds:7.1f} us/round, "
          f"enqueue to drained {1e6 * (t2 - t0) / n_rounds:7.1f} us/round", flush=True)
s.close()
