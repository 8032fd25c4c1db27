#!/bin/bash
# Collect the round's profiling artefacts on an MI355X box:  bash tools/profile_round.sh [OUTDIR]
#   kernel trace + stats of the default bench command, FETCH_SIZE / WRITE_SIZE and the instruction counters in separate
#   PMC passes (never together with a trace), the per-unit routing cycles, and the calibration bench line.
# Outputs land in OUTDIR (default profile_out/ under the repository root); copy what is to be judged into
# profiles/<round>/ (README there).
export TMPDIR=/tmp
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R
OUT=$(mkdir -p "${1:-profile_out}" && cd "${1:-profile_out}" && pwd)
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_trace -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-end-to-end --no-secondary > $OUT/bench_under_rocprof.json 2> $OUT/bench_under_rocprof.log
# (counter passes serialise the kernels of a process: the fed order's routing kernel would wait for months that cannot be
#  produced beside it -- the passes run the stages one after the other, which is also what per-kernel counters are about)
timeout 600 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/prof_fetch -- python3 bench.py --steps 2 --warmup 1 --order staged --no-cpu-baseline --no-end-to-end --no-secondary > /dev/null 2>&1
timeout 600 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/prof_write -- python3 bench.py --steps 2 --warmup 1 --order staged --no-cpu-baseline --no-end-to-end --no-secondary > /dev/null 2>&1
# counter calibration on the streams' own access shapes: 1 GiB (past the Infinity Cache) and 128 MiB
for sz in 1024 128; do
  timeout 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/cal_fetch_$sz -- tools/micro/sc1_traffic.bin $sz > $OUT/cal_bytes_$sz.txt 2>&1
  timeout 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/cal_write_$sz -- tools/micro/sc1_traffic.bin $sz > /dev/null 2>&1
done
BYTES=$(grep bytes_per_launch $OUT/cal_bytes_1024.txt | cut -d" " -f2)
python3 tools/pmc_to_json.py $OUT/prof_fetch $OUT/prof_write $OUT/pmc_traffic.json $OUT/cal_fetch_1024 $OUT/cal_write_1024 $BYTES > /dev/null
BYTES2=$(grep bytes_per_launch $OUT/cal_bytes_128.txt | cut -d" " -f2)
python3 tools/pmc_to_json.py $OUT/prof_fetch $OUT/prof_write $OUT/pmc_traffic_cal128.json $OUT/cal_fetch_128 $OUT/cal_write_128 $BYTES2 > /dev/null
cp $OUT/prof_trace/*/*kernel_stats.csv $OUT/kernel_stats.csv
timeout 600 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES --output-format csv -d $OUT/prof_insts -- python3 bench.py --steps 2 --warmup 1 --order staged --no-cpu-baseline --no-end-to-end --no-secondary > /dev/null 2>&1
timeout 600 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY --output-format csv -d $OUT/prof_cyc -- python3 bench.py --steps 2 --warmup 1 --order staged --no-cpu-baseline --no-end-to-end --no-secondary > /dev/null 2>&1
# the calibration marches (config 5): instruction counts for the measured issue fraction of bench.py's `calib` lines
timeout 600 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES --output-format csv -d $OUT/prof_insts_calib -- python3 bench.py --workload calib --steps 2 --warmup 1 --no-cpu-baseline > /dev/null 2>&1
timeout 600 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY --output-format csv -d $OUT/prof_cyc_calib -- python3 bench.py --workload calib --steps 2 --warmup 1 --no-cpu-baseline > /dev/null 2>&1
python3 tools/pmc_insts_json.py $OUT/pmc_insts.json $OUT/prof_insts $OUT/prof_cyc $OUT/prof_insts_calib $OUT/prof_cyc_calib > /dev/null
(python3 tools/pmc_summary.py $OUT/prof_insts; python3 tools/pmc_summary.py $OUT/prof_cyc) | grep -E "k_pm_pet|k_abcd|k_mrtm_wave|k_mrtm_rsum|k_mrtm_units" > $OUT/pmc_insts.txt
(python3 tools/pmc_summary.py $OUT/prof_insts_calib; python3 tools/pmc_summary.py $OUT/prof_cyc_calib) | grep -E "k_calib" >> $OUT/pmc_insts.txt
timeout 900 python3 bench.py --full --steps 20 --warmup 5 > $OUT/bench.json 2> $OUT/bench.log
timeout 300 python3 bench.py --full --workload pm_abcd --steps 10 --warmup 2 > $OUT/bench_pm_abcd.json 2> $OUT/bench_pm_abcd.log
timeout 600 python3 bench.py --full --workload calib --steps 5 --warmup 1 > $OUT/bench_calib.json 2> $OUT/bench_calib.log
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_trace_calib -- python3 bench.py --workload calib --steps 5 --warmup 1 --no-cpu-baseline > /dev/null 2>&1
cp $OUT/prof_trace_calib/*/*kernel_stats.csv $OUT/kernel_stats_calib.csv
timeout 300 python3 bench.py --full --steps 20 --warmup 5 --order staged --no-end-to-end --no-cpu-baseline > $OUT/bench_staged.json 2> /dev/null
timeout 300 python3 tools/feed_interference.py 2>&1 | grep -E "stage by stage|fed" > $OUT/feed_interference.txt
timeout 600 python3 tools/feed_stress.py 150 2>&1 | tail -3 > $OUT/feed_stress.txt
XH_FLOW_STATS=1 timeout 300 python3 tools/flow_stats.py 720 > $OUT/flow_unit_cycles.txt 2>&1
XH_STATS_ROUTE_SPIN=120 XH_STATS_ABCD_SPIN=120 XH_STATS_LOOP=5 timeout 300 python3 tools/flow_stats.py 600 2>&1 | grep -E "back-to-back|histogram|wave\(s\)" > $OUT/flow_pipelined.txt
head -c 600 $OUT/bench.json; echo; head -8 $OUT/kernel_stats.csv | cut -c1-160; cat $OUT/pmc_traffic.json | head -50
# the N = 2 dry run on this box's one GPU (both ranks on device 0, gloo process group, RCCL stand-in named by path)
make -C tests/fake_rccl > /dev/null 2>&1
XH_BENCH_ONE_DEVICE=1 XH_BENCH_BACKEND=gloo XH_RCCL_LIBRARY=$R/tests/fake_rccl/librccl.so.1 XH_FAKE_RCCL_DIR=/tmp timeout 900 python3 bench.py --gpus 2 --steps 3 --warmup 1 --route-flags 4 --check-gather --no-replica-figure > $OUT/bench_2rank_dryrun.json 2> $OUT/bench_2rank_dryrun.log
head -c 400 $OUT/bench_2rank_dryrun.json; echo
