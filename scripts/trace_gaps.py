"""Per-round wall time, busy time and inter-kernel gaps from a rocprofv3
kernel trace (last 10 complete rounds, rounds delimited by k_begin: one per
round, also when robot groups run a k_grad each). With robot groups the
kernels of different streams overlap: busy (the sum of kernel durations) then
exceeds the wall time, gaps between start-ordered neighbours go negative, and
the last lines count the k_reduce launches that ran wholly inside another
group's k_hess / k_update."""
import csv
import sys
from collections import defaultdict

rows = list(csv.DictReader(open(sys.argv[1])))
ts = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows)
g = [t for t in ts if "k_begin" in t[2]] or [t for t in ts if "k_grad" in t[2]]
s0, s1 = g[-11][0], g[-1][0]
seq = [t for t in ts if t[0] >= s0 and t[1] <= s1]
busy = sum(b - a for a, b, _ in seq)
print(f"wall {(s1 - s0) / 10e3:.1f} us/round, busy {busy / 10e3:.1f} us/round, kernels/round {len(seq) / 10:.1f}")


def nm(n):
    for k in ("k_step", "k_hess", "k_update", "k_reduce", "k_grad", "k_cost", "k_retract", "k_commit", "k_begin", "k_precond",
              "k_publish", "k_accel"):
        if k in n:
            return k
    return n[:16]


gap = defaultdict(list)
for i in range(len(seq) - 1):
    gap[(nm(seq[i][2]), nm(seq[i + 1][2]))].append((seq[i + 1][0] - seq[i][1]) / 1e3)
for k, v in sorted(gap.items(), key=lambda kv: -sum(kv[1])):
    print(f"{k[0]:>10s} -> {k[1]:10s} n={len(v):4d} mean gap {sum(v) / len(v):6.2f} us, total/round {sum(v) / 10:7.1f} us")

kt = defaultdict(list)
for a, b, n in seq:
    kt[nm(n)].append((b - a) / 1e3)
for k, v in sorted(kt.items(), key=lambda kv: -sum(kv[1])):
    print(f"{k:>10s} n/round={len(v) / 10:5.1f} mean {sum(v) / len(v):6.2f} us, total/round {sum(v) / 10:7.1f} us")

big = [(a, b, nm(n)) for a, b, n in seq if nm(n) in ("k_hess", "k_update")]
red = [(a, b) for a, b, n in seq if nm(n) == "k_reduce"]
inside = defaultdict(int)
for a, b in red:
    for c, d, k in big:
        if c <= a and b <= d:
            inside[k] += 1
            break
print(f"k_reduce launches/round {len(red) / 10:.1f}: inside a k_hess {inside['k_hess'] / 10:.1f}, "
      f"inside a k_update {inside['k_update'] / 10:.1f}")
# fork and join per round: k_begin's end to the first k_grad's start, and the
# last kernel's end before the round's final k_commit to that k_commit's start
fork, join = [], []
for r in range(10):
    lo, hi = g[-11 + r][0], g[-10 + r][0]
    rk = [t for t in ts if lo <= t[0] < hi]
    kb = [t for t in rk if "k_begin" in t[2]]
    kg = [t for t in rk if "k_grad" in t[2]]
    kc = [t for t in rk if "k_commit" in t[2]]
    if not (kb and kg and kc):
        continue
    fork.append((min(t[0] for t in kg) - kb[0][1]) / 1e3)
    c0 = kc[-1][0]
    join.append((c0 - max(t[1] for t in rk if t[0] < c0)) / 1e3)
if fork:
    print(f"k_begin end -> first k_grad start: mean {sum(fork) / len(fork):.2f} us; "
          f"last kernel end -> final k_commit start: mean {sum(join) / len(join):.2f} us")
