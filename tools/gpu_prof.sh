# Full measurement set for one tag (run on the GPU box via gpurun): rocprofv3 trace + HBM
# counters (tools/profile.sh), one SQ counter pass (tools/profile_sq.sh), the default bench
# line.  Summaries: python tools/prof_summary.py TAG; python tools/sq_summary.py TAG.
set -o pipefail
TAG=${TAG:-r02h}
bash tools/profile.sh $TAG || exit 1
bash tools/profile_sq.sh $TAG || exit 2
OUT=${ZH_OUT:-bench_out}  # where the result line goes
mkdir -p $OUT
timeout -k 10 300 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || exit 3
echo all-done
