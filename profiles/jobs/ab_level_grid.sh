# A/B of the trace grids sized by queue length (EXPERIMENTS R13.1) against a library built from the PARENT commit, in one session, one process per run, the libraries
# alternating: parent / this tree / this tree with BHRAY_LEVEL_GRID=0 (the prologue store without the rule) / this tree with BHRAY_LEVEL_GRID_GEN=512.
# usage: bash profiles/jobs/ab_level_grid.sh <parent libbhray.so> <output directory> [seconds the whole job may take]
# Lines: label, bench arguments, steps, value (Mrays/s), ms_per_step (and, of a --full run, the latency of one frame at a time).  Legs are run in order of importance; a leg that would start after the deadline is skipped and said so.
PARENT=$1; OUT=$2; DEADLINE=$(( $(date +%s) + ${3:-1000} ))
ROOT=$(cd "$(dirname "$0")/../.." && pwd); cd $ROOT; mkdir -p $OUT
RAW=$OUT/ab_level_grid_raw.txt
one() {  # $1 = label, $2 = bench arguments; environment from the caller
  if [ $(date +%s) -ge $DEADLINE ]; then echo "$1 | $2 | skipped: deadline" >> $RAW; return 0; fi
  timeout -k 10 ${TLIMIT:-240} python bench.py $2 --no-cpu-baseline > $OUT/last_stdout.txt 2>$OUT/last_stderr.txt
  rc=$?; if [ $rc -ne 0 ]; then echo "$1 | $2 | FAILED: bench.py rc=$rc" >> $RAW; tail -5 $OUT/last_stderr.txt; return 1; fi
  python -c "
import json,sys
d=json.loads(open('$OUT/last_stdout.txt').read().strip().splitlines()[-1])
def find(o, k):
    if isinstance(o, dict):
        if k in o: return o[k]
        for v in o.values():
            r = find(v, k)
            if r is not None: return r
    return None
lat=find(d, 'latency_ms_one_frame_in_flight')
print('$1 | $2 |', d['steps'], d['value'], d['ms_per_step'], *([] if lat is None else ['one frame at a time ms', lat]))" >> $RAW || { echo "$1 | $2 | FAILED: no result line" >> $RAW; return 1; }
}
legs() {  # $1 = bench arguments, $2 = rounds, $3 = rounds that also run the 512-ray generation
  for r in $(seq 1 $2); do
    BHRAY_LIB=$PARENT BHRAY_AB_OLD_BUILD=1 one parent "$1" || exit 1
    one new "$1" || exit 1
    BHRAY_LEVEL_GRID=0 one new_rule_off "$1" || exit 1
    if [ $r -le $3 ]; then BHRAY_LEVEL_GRID_GEN=512 one new_gen512 "$1" || exit 1; fi
  done
}
LEGS=${LEGS:-"flagship steps20 euler mesh rank8 full"}          # LEGS="full" bash ab_level_grid.sh ...: some of the legs only
for leg in $LEGS; do
  case $leg in
    flagship) legs "" 7 5 ;;
    steps20) legs "--steps 20 --warmup 5" 5 5 ;;
    euler) legs "--integrator euler" 5 0 ;;
    mesh) legs "--workload mesh" 5 0 ;;
    rank8) legs "--emulate-world 8 --emulate-rank 3 --partition balanced --steps 20 --warmup 5" 5 0 ;;
    full) TLIMIT=600 legs "--full" 2 0 ;;          # one frame at a time (latency builds): must not move
  esac
done
python - $RAW <<'PY'
import sys, statistics as st
rows = {}
for l in open(sys.argv[1]):
    p = [x.strip() for x in l.split('|')]
    if len(p) == 3 and p[2][:1].isdigit():
        rows.setdefault((p[1], p[0]), []).append(float(p[2].split()[1]))
        if 'one frame at a time ms' in p[2]:
            rows.setdefault((p[1] + ': ms, one frame at a time', p[0]), []).append(float(p[2].split()[-1]))
for (args, label), v in rows.items():
    m = st.median(v)
    print(f"{args or '(flagship)':60s} {label:14s} n={len(v)} median {m:10.5g} min {min(v):10.5g} max {max(v):10.5g} spread {(max(v) - min(v)) / m * 100:5.2f} %")
PY
