"""The tail of the dpgo round in a rocprofv3 kernel trace (all complete rounds
after the first, rounds delimited by k_begin): launch counts and mean
durations of the tail's kernels (k_retract, the k_update at the step cap,
k_cost, k_commit) next to the ordinary k_update, and per round the launch
chain (queue) whose k_cost ends last — the one the final k_commit waits for —
with whether it carried a k_retract or a k_update_last. That share of rounds
is what removing the launch can shorten.

  python scripts/round_tail.py run_kernel_trace.csv
"""
import csv
import sys
from collections import defaultdict

rows = list(csv.DictReader(open(sys.argv[1])))
qcol = "Queue_Id" if "Queue_Id" in rows[0] else "Stream_Id"
ts = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r[qcol]) for r in rows)


def nm(n):
    for k in ("k_update_last", "k_step", "k_hess", "k_update", "k_reduce", "k_grad", "k_cost", "k_retract", "k_commit",
              "k_begin"):
        if k in n:
            return k
    return n[:16]


begins = [i for i, t in enumerate(ts) if nm(t[2]) == "k_begin"]
rounds = [ts[begins[i]:begins[i + 1]] for i in range(1, len(begins) - 1)]
dur = defaultdict(list)
last_has = defaultdict(int)
wall = []
chains = with_retract = 0
for rd in rounds:
    for a, b, n, q in rd:
        dur[nm(n)].append((b - a) / 1e3)
    byq = defaultdict(list)
    for a, b, n, q in rd:
        byq[q].append((a, b, nm(n)))
    ends = {q: max(b for a, b, k in v if k == "k_cost") for q, v in byq.items() if any(k == "k_cost" for _, _, k in v)}
    for q in ends:
        chains += 1
        with_retract += any(k == "k_retract" for _, _, k in byq[q])
    if ends:
        q = max(ends, key=ends.get)
        kinds = {k for _, _, k in byq[q]}
        last_has["k_retract" if "k_retract" in kinds else "k_update_last" if "k_update_last" in kinds else "neither"] += 1
wall = [(ts[begins[i + 1]][0] - ts[begins[i]][0]) / 1e3 for i in range(1, len(begins) - 1)]
print(f"rounds {len(rounds)}, wall {sum(wall) / len(wall):.1f} us/round (k_begin to k_begin)")
for k in ("k_grad", "k_hess", "k_update", "k_update_last", "k_retract", "k_cost", "k_commit"):
    v = dur.get(k, [])
    print(f"{k:>14s} n/round {len(v) / len(rounds):5.2f}" + (f"  mean {sum(v) / len(v):6.2f} us" if v else ""))
print(f"chains {chains}, with a k_retract {with_retract} ({100.0 * with_retract / max(chains, 1):.0f} %)")
print("the chain whose k_cost ends last carried: " +
      ", ".join(f"{k} {v} ({100.0 * v / len(rounds):.0f} % of rounds)" for k, v in sorted(last_has.items())))
