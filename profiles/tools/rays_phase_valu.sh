# dynamic VALU/SALU instructions of the ray kernel by phase: builds that stop after phase k (variants_stopK.so, -DFTL_RAYS_STOP=K;
# variants_stop6.so = the full kernel).  0: loads + windows, 1: + corridor staging, 2: + table (phase 1), 3: + ray ends (phase 2),
# 5: + phase 3 without the ray tests but with the rows, 4: all of phase 3 without the rows, 6: everything.
# Counters and a trace are never collected in one run: MODE=pmc (default) prints the counters per env-step, MODE=trace the ray kernel's
# duration per launch.  OUT = directory that receives the runs' files (default rays_phase_out).
# Every run has its own time limit, and the first one that fails ends the script: nothing more is started on a card that has just faulted.
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${OUT:-rays_phase_out}; mkdir -p $O
MODE=${MODE:-pmc}
B="python3 bench.py --parts 1 --steps 10 --warmup 5 --no-cpu-baseline --kernel-steps 0 --gen-sample 0"
for v in ${STOPS:-0 1 2 3 4 5 6}; do
  if [ "$MODE" = trace ]; then
    FTL_LIB=$PWD/variants_stop$v.so timeout -k 10 200 rocprofv3 --kernel-trace --output-format csv -d $O/trace_stop$v -- $B > $O/trace_stop$v.log 2>&1 || { echo "stop $v: exit status $?"; exit 1; }
  else
    FTL_LIB=$PWD/variants_stop$v.so timeout -k 10 200 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_SMEM --output-format csv -d $O/stop$v -- $B > $O/stop$v.log 2>&1 || { echo "stop $v: exit status $?"; exit 1; }
  fi
  python3 - <<PY
import csv,glob,collections
acc=collections.defaultdict(list)
if "$MODE" == "trace":
    for f in glob.glob("$O/trace_stop$v/*/*_kernel_trace.csv"):
        for r in csv.DictReader(open(f)):
            if "rays" in r["Kernel_Name"]: acc["ns"].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    print("stop after $v: %.1f us per launch" % (sum(d for _, d in sorted(acc["ns"])[-10:])/10/1e3))
else:
    for f in glob.glob("$O/stop$v/*/*_counter_collection.csv"):
        for r in csv.DictReader(open(f)):
            if "rays" in r["Kernel_Name"]: acc[r["Counter_Name"]].append(float(r["Counter_Value"]))
    print("stop after $v:", {k: round(sum(x[-10:])/10/65536,1) for k,x in sorted(acc.items())})
PY
done
