#!/bin/bash
# The camera solve's forward-inverse form (default) against the backward pass inside the launch (PTAM_LDLT_BACKWARD_IN_LAUNCH=1),
# alternating in one call: the solve alone (tools/ldlt), per-trial times by outcome at the headline, bench.py's value and
# deterministic_mode.value; then bench.py --full once, and the ldlt_chain_kernel row of a kernel trace for both forms.
# PARENT=path/to/ldlt_bench of the parent commit adds that build to the first part: the switch's old form is ~1.4 us slower
# than the parent's own build.
# SOLVE_ONLY=1 stops after the first part.
#   usage: [OUT_DIR=dir] [PARENT=binary] [SOLVE_ONLY=1] bash tools/dev/solve_forward_inverse_ab.sh   (from the repository root, library and tools/ldlt/ldlt_bench built)
R=$(cd "$(dirname "$0")/../.." && pwd)
cd $R
O=${OUT_DIR:-$R/tools/_ab}   # (where the results go: kept out of git)
mkdir -p $O
OUT=$O/solve_forward_inverse_ab.txt
LOG=$O/solve_forward_inverse_ab_log.txt
: > $OUT
# Every program that uses the device runs HERE, at the script's top level (never inside $( ) or a subshell, whose `exit` would
# end only itself), under a time limit, its output in $LOG; any status but 0 ends the script: nothing more is started on a
# device after a fault, an abort or a hang — and bench.py's legs run in child processes, whose fault may come back as 1.
step() {
  "$@" > $LOG 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then echo "stopped: rc $rc from: $*" | tee -a $OUT; tail -5 $LOG | tee -a $OUT; exit 1; fi
}
form() { if [ $1 = old ]; then export PTAM_LDLT_BACKWARD_IN_LAUNCH=1; else unset PTAM_LDLT_BACKWARD_IN_LAUNCH; fi; }
first_line() { echo "$1: $(head -1 $LOG)" >> $OUT; }
summary() {
  python3 - "$1" "$LOG" >> $OUT <<PY
import json, sys
b = json.loads([l for l in open(sys.argv[2]) if l.startswith("{")][-1])
l, g, d = b.get("local_ba_config4", {}), b.get("global_ba_single_gpu", {}), b.get("deterministic_mode", {})
k = b.get("kernel_ms_per_trial", {})
print("%s: value %.0f mix %s | deterministic %.0f | solve %.1f us | accepted trial %.1f us | local %.0f it/s (solve %.1f us) | global %.0f it/s (solve %.1f us)" % (
    sys.argv[1], b["value"], list(b["trial_mix"].values()), d.get("value", 0), 1e3 * k.get("solve", 0), b.get("accepted_trial_us", 0),
    l.get("value", 0), 1e3 * l.get("kernel_ms_per_trial", {}).get("solve", 0), g.get("value", 0), 1e3 * g.get("kernel_ms_per_trial", {}).get("solve", 0)))
PY
}
echo "== the solve alone (tools/ldlt/ldlt_bench, us per solve incl. the device copy of the system)" >> $OUT
for rep in 1 2 3; do
  for a in 49 19; do
    for f in new old; do
      form $f
      step timeout -k 10 60 tools/ldlt/ldlt_bench $a
      first_line $f
    done
    if [ -n "$PARENT" ]; then
      step timeout -k 10 60 $PARENT $a
      first_line parent
    fi
  done
done
if [ -n "$SOLVE_ONLY" ]; then cat $OUT; exit 0; fi
echo "== per-trial times by outcome (tools/dev/r06_trial_times.py 12), bench.py --full without the global leg" >> $OUT
for rep in 1 2 3; do
  for f in new old; do
    form $f
    step timeout -k 10 120 python tools/dev/r06_trial_times.py 12
    first_line $f
    if head -1 $LOG | grep -q "accepted nan"; then echo "stopped: the trial-times run printed no trials" | tee -a $OUT; exit 1; fi   # (it does not pass its child's status on)
    step timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-tracking --no-global
    summary $f
  done
done
echo "== bench.py --full with the global leg, once per form" >> $OUT
for f in new old; do
  form $f
  step timeout -k 10 400 python bench.py --full --no-cpu-baseline --no-tracking
  summary $f
done
echo "== rocprofv3 --kernel-trace --stats of a plain bench.py run: the ldlt_chain_kernel row" >> $OUT
export TMPDIR=/tmp
for f in old new; do
  form $f
  D=$O/solve_forward_inverse_trace_$f
  mkdir -p $D
  cd /tmp   # (the profiler's scratch files)
  step timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $D -o ba -- python $R/bench.py
  cd $R
  python3 - "$f" "$D" >> $OUT <<PY
import csv, glob, sys
for p in glob.glob(sys.argv[2] + "/**/ba_kernel_stats.csv", recursive=True):
    for r in csv.DictReader(open(p)):
        if "ldlt_" in r["Name"]:
            print(f'{sys.argv[1]}: {r["Name"].split("(")[0][:44]:44s} calls {r["Calls"]:>5s} avg {float(r["AverageNs"])/1e3:8.2f} us  min {float(r["MinNs"])/1e3:7.2f} max {float(r["MaxNs"])/1e3:7.2f}')
PY
done
cat $OUT
