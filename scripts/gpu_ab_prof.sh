# Same-box A/B of library builds by rocprofv3 kernel stats of the dpgo bench: bash scripts/gpu_ab_prof.sh TAG lib1.so [lib2.so ...] (diag/ names; two reps each, alternating)
# (results under ${OUT_DIR:-out}/TAG/)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
T=$1; shift
O=${OUT_DIR:-out}/$T
mkdir -p "$O"
for rep in 1 2; do
  for L in "" "$@"; do
    tag=${L:-intree}_$rep
    if [ -n "$L" ]; then export KMX_LIB=$PWD/diag/$L; else unset KMX_LIB; fi
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$O/$tag" -o run --output-format csv -- python3 bench.py --full --no-cpu --no-lcd --steps 10 > "$O/$tag.json" 2> "$O/$tag.err" || { tail "$O/$tag.err"; exit 1; }
    echo "$tag done"
  done
done
