#!/bin/bash
# Runs on the GPU box: un-profiled bench line, kernel trace + stats, PMC passes, all of `bench.py --full`.
# The program sits directly behind `--` (python3), as the pool requires.
# Output folder: $OUT (default profile_out/ in the repo root); then python tools/make_profiles.py rNN "$OUT"
R="$(cd "$(dirname "$0")/.." && pwd)"
[ -n "$R" ] && [ -f "$R/bench.py" ] || { echo "cannot locate the repo root from $0" >&2; exit 1; }
cd /tmp && export TMPDIR=/tmp
cd "$R"
O="${OUT:-profile_out}"
mkdir -p "$O"
rm -rf "$O/kt" "$O/pmc_f" "$O/pmc_w" "$O/pmc_sq"
python3 bench.py --full > "$O/bench_line.json" 2> "$O/bench_line.err"; echo "bench rc=$?"
rocprofv3 --kernel-trace --stats --output-format csv -d "$O/kt" -- python3 bench.py --full --steps 20 --warmup 3 --no-cpu-baseline --no-other-configs > "$O/kt.log" 2>&1; echo "kt rc=$?"
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d "$O/pmc_f" -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-other-configs > "$O/pmc_f.log" 2>&1; echo "f rc=$?"
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d "$O/pmc_w" -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-other-configs > "$O/pmc_w.log" 2>&1; echo "w rc=$?"
rocprofv3 --pmc SQ_BUSY_CU_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d "$O/pmc_sq" -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-other-configs > "$O/pmc_sq.log" 2>&1; echo "sq rc=$?"
grep -a '^{' "$O/kt.log" | head -1 | cut -c1-200
