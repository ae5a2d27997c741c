# Developer tool (GPU box): decoder tests, then the decode leg of the bench with the block kernel (NHW_DEC_L2Q=0: k_dec_luma_l2, one
# workgroup a file) and with the quarters (NHW_DEC_L2Q=1: k_dec_luma_l2q, the default).  Each step under its own time limit; the first
# that fails ends the script.  Usage: tools/dev/dec_l2q.sh [output directory, default: dec_l2q_out in the repository root]
cd "$(dirname "$0")/../.." || exit 1
OUT=${1:-dec_l2q_out}
mkdir -p "$OUT" || exit 1
timeout -k 10 900 python -m pytest tests/test_decode.py tests/test_gpu_schedule.py -x -q -m gpu > "$OUT/dec_tests.txt" 2>&1; rc=$?
tail -1 "$OUT/dec_tests.txt"
[ $rc -eq 0 ] || exit $rc
for v in 0 1; do
	NHW_DEC_L2Q=$v timeout -k 10 300 python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-host-path --no-config4-shape --no-chroma-l1 --sweep= > "$OUT/dec_l2q_$v.txt" 2>&1 || exit $?
	echo "== NHW_DEC_L2Q=$v $(python -c "
import json,sys
for l in open(sys.argv[1]):
    if l.startswith('{'):
        print('decode ms', json.loads(l)['decode']['ms_per_step'])" "$OUT/dec_l2q_$v.txt")"
done
