"""k_update in a rocprofv3 kernel trace (last 10 complete rounds, delimited by
k_begin as in trace_gaps.py): its mean duration, the mean of the launches that
no other kernel overlaps, and how much of its span runs beside a k_hess (the
other robot group's). The same three figures for k_hess against k_update, and
the slot-time account of DESIGN.md section 13 (round 10) with these lives."""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
ts = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows)
g = [t for t in ts if "k_begin" in t[2]] or [t for t in ts if "k_grad" in t[2]]
s0, s1 = g[-11][0], g[-1][0]
seq = [t for t in ts if t[0] >= s0 and t[1] <= s1]
print(f"wall {(s1 - s0) / 10e3:.1f} us/round, kernels/round {len(seq) / 10:.1f}")


def report(name, other):
    mine = [t for t in seq if name in t[2]]
    if not mine:
        print(f"{name}: none")
        return
    dur, alone, ov_other, ov_any = [], [], [], []
    for a, b, n in mine:
        o_other = o_any = 0
        for c, e, m in seq:
            if e <= a or c >= b or (c, e, m) == (a, b, n):
                continue
            x = min(b, e) - max(a, c)
            o_any += x
            if other in m:
                o_other += x
        dur.append(b - a)
        ov_other.append(o_other)
        ov_any.append(o_any)
        if o_any == 0:
            alone.append(b - a)
    n = len(dur)
    m_alone = f"{sum(alone) / len(alone) / 1e3:6.2f} us (n={len(alone)})" if alone else "none"
    print(f"{name:>9s} n/round {n / 10:5.1f}: mean {sum(dur) / n / 1e3:6.2f} us, total/round {sum(dur) / 10e3:7.1f} us; "
          f"with no kernel beside it: mean {m_alone}; "
          f"share of its span beside a {other}: {100.0 * sum(ov_other) / sum(dur):5.1f} %, beside any kernel: "
          f"{100.0 * min(sum(ov_any), sum(dur)) / sum(dur):5.1f} %")
    # duration by how much of the launch ran beside `other`
    for lo, hi in ((0.0, 0.1), (0.1, 0.5), (0.5, 0.9), (0.9, 1.01)):
        sel = [d for d, o in zip(dur, ov_other) if lo <= o / d < hi]
        if sel:
            print(f"{'':>9s}   {int(lo * 100):3d}-{min(int(hi * 100), 100):3d} % beside {other}: n={len(sel):4d} "
                  f"mean {sum(sel) / len(sel) / 1e3:6.2f} us")


report("k_update", "k_hess")
report("k_hess", "k_update")
