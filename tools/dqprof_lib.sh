# decoder kernel trace of a variant library (gpurun): usage bash tools/dqprof_lib.sh TAG LIB
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${ZH_OUT:-$R/bench_out}  # where the logs and result lines go
TAG=$1
mkdir -p $OUT/$TAG
cd /tmp && export TMPDIR=/tmp
CUDA_ZSTD_HIP_LIB=$R/$2 timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/$TAG/trace -o run --output-format csv -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-verify --no-legs > $OUT/$TAG/trace.log 2>&1 || exit 2
echo prof-done
