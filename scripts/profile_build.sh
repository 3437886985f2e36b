# per-kernel times of the device build (rocprofv3 kernel trace of scripts/build_timing.py for one size) -> $RESULTS/prof_build_<n>/,
# $RESULTS/build_kernel_stats_<n>.csv (RESULTS: default results/ in the repo root)
N=${1:-10000000}
R=$(cd "$(dirname "$0")/.." && pwd)
D=$(cd "$R" && mkdir -p "${RESULTS:-results}/prof_build_$N" && cd "${RESULTS:-results}/prof_build_$N" && pwd)
cd /tmp && export TMPDIR=/tmp
timeout -k 10 500 rocprofv3 --kernel-trace --stats -d $D --output-format csv -- python3 $R/scripts/build_timing.py $N > $D/out.log 2>&1
echo "rc=$?"
f=$(find $D -name '*kernel_stats.csv' | head -1)
python3 - "$f" <<'PY'
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
for r in rows[:28]:
    print('%-70s calls %5s avg_us %9.1f total_us %10.1f' % (r['Name'][:70], r['Calls'], float(r['AverageNs']) / 1e3, float(r['TotalDurationNs']) / 1e3))
PY
cp "$f" $D/../build_kernel_stats_$N.csv
