# Round time and k_hess roofline against the tile cut (bench.py --tile-incidences:
# incidences per workgroup tile; the default cut gives 2,084 tiles at configs[3], i.e. two
# generations of the 1,024 resident k_hess workgroups plus 36 tiles).
# usage: bash scripts/gpu_tile_sweep.sh TAG cap...   (results under ${OUT_DIR:-out}/TAG/)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
T=${1:-tiles}; shift
O=${OUT_DIR:-out}/$T
mkdir -p "$O"
for cap in "$@"; do
  if [ "$cap" = default ]; then ti=0; else ti=$cap; fi
  timeout -k 10 300 python bench.py --full --no-cpu --no-lcd --steps 200 --tile-incidences $ti > "$O/cap_$cap.json" 2> "$O/cap_$cap.err" \
    || { echo "cap $cap failed"; tail -5 "$O/cap_$cap.err"; exit 1; }
  python3 - "$O" "$cap" <<'PY' | tee -a "$O/summary.txt"
import json, sys
o, cap = sys.argv[1], sys.argv[2]
d = json.loads(open(f"{o}/cap_{cap}.json").read().strip().splitlines()[-1])
r = d["roofline"]
print(f"cap {cap}: {d['value']:.4g} edges*iters/s, {d['ms_per_step']*1e3:.1f} us/round, k_hess {r['avg_launch_us']:.1f} us frac {r['frac']:.3f}, hessvecs/round {d['work']['hessvecs_per_round']:.2f}, parity {d.get('parity', {}).get('ok')}")
PY
done
