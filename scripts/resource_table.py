"""Tabulate hipcc's -Rpass-analysis=kernel-resource-usage remarks (stderr of a
device-only compile of one .hip file): one line per function with its VGPRs,
scratch bytes per lane and waves per SIMD. With two files, side by side
(parent, new). Optional last argument: a substring filter on the name.

  hipcc ... --cuda-device-only -Rpass-analysis=kernel-resource-usage -c pgo.hip -o /dev/null 2> new.txt
  python scripts/resource_table.py parent.txt new.txt k_update
"""
import re
import subprocess
import sys


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur:
            out[cur][m.group(1).split()[0]] = int(m.group(2))
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


files = [a for a in sys.argv[1:] if a.endswith(".txt")]
flt = [a for a in sys.argv[1:] if not a.endswith(".txt")]
tabs = [parse(f) for f in files]
names = sorted(set().union(*[t.keys() for t in tabs]))
dm = demangle(names)
for n in names:
    short = re.sub(r"\(anonymous namespace\)::|kmx_pgo::|void ", "", dm[n]).split("(")[0]
    if [f for f in flt if f != "changed"] and not any(f in short for f in flt):
        continue
    cells = []
    for t in tabs:
        r = t.get(n)
        cells.append(f"{r['VGPRs']:4d} VGPRs {r['ScratchSize']:4d} B {r['Occupancy']} w" if r and "VGPRs" in r else "-")
    if "changed" in flt and len(set(cells)) == 1:
        continue
    print(f"{short:34s} " + "  |  ".join(cells))
