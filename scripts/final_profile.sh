#!/bin/bash
# GPU box: the judged artefacts — the driver's bench command, rocprofv3 --kernel-trace --stats of the SAME command, the
# HBM-traffic PMC passes (FETCH_SIZE / WRITE_SIZE in separate runs, counters only) for the history kernel in both policies
# and for the two full_trace routes, and SQ counters of the IEEE kernel.
set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd /root/repo
OUT=/root/repo/gpurun_out/final
rm -rf $OUT; mkdir -p $OUT
timeout -k 10 500 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench.json 2> $OUT/bench.err || { tail -5 $OUT/bench.err; exit 1; }
cd /tmp && export TMPDIR=/tmp
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats -- python3 $ROOT/bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/stats.log 2>&1 || { tail -5 $OUT/stats.log; exit 1; }
Q="--steps 5 --warmup 1 --no-cpu-baseline --no-extras --no-verify --sustain-s 0"
for pol in fast ieee; do
  timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/fetch_$pol -- python3 /root/repo/bench.py $Q --policy $pol > $OUT/fetch_$pol.log 2>&1 || exit 1
  timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/write_$pol -- python3 /root/repo/bench.py $Q --policy $pol > $OUT/write_$pol.log 2>&1 || exit 1
done
for route in place lookback fused; do
  extra=""; [ $route = lookback ] && extra="--ft-lookback"; [ $route = fused ] && extra="--ft-fused"
  timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/ft_fetch_$route -- python3 /root/repo/bench.py $Q --mode full_trace $extra > $OUT/ft_fetch_$route.log 2>&1 || exit 1
  timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/ft_write_$route -- python3 /root/repo/bench.py $Q --mode full_trace $extra > $OUT/ft_write_$route.log 2>&1 || exit 1
done
timeout -k 10 300 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CU_CYCLES SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY --kernel-trace --output-format csv -d $OUT/sq_both -- python3 $ROOT/bench.py $Q --full --policy fast > $OUT/sq_both.log 2>&1 || exit 1
ORT_ROUND=${ORT_ROUND:-r04} python3 /root/repo/scripts/collect_final.py
# the rest of the round's judged artefacts, same box: config 3 / config 1 kernel statistics, the plain-C caller's wall time, the
# counter + clock pass of the config-3 trace kernel, the 2-rank rehearsal of `bench.py --gpus 2` (gloo; both ranks on this GPU)
T=${ORT_ROUND:-r04}
cd /root/repo
bash scripts/config3_kernels.sh ${T}_c3k > /dev/null 2>&1; cp gpurun_out/${T}_c3k.log profiles/${T}_config3_kernels.log 2>/dev/null
bash scripts/config1_kernels.sh > gpurun_out/${T}_c1k.log 2>&1; cp gpurun_out/${T}_c1k.log profiles/${T}_config1_kernels.log
gcc -O2 -Wall -Iinclude examples/cooke_full_trace.c -o build/cooke_full_trace -Lopticalraytracing.jl_amd/csrc -lort_hip -Wl,-rpath,$PWD/opticalraytracing.jl_amd/csrc -Wl,-rpath,/opt/rocm/lib -Wl,-rpath-link,/opt/rocm/lib -lm
[ -x build/cooke_full_trace ] && (./build/cooke_full_trace --time 0.0; ./build/cooke_full_trace --time 1.0; ./build/cooke_full_trace --time 0.0 fast; ./build/cooke_full_trace --time 1.0 fast) > gpurun_out/${T}_c1_cabi.log 2>&1
bash scripts/clock_config3.sh ${T}_clk > gpurun_out/${T}_clk.log 2>&1
bash scripts/clock_fused.sh ${T}_clock_fused > gpurun_out/${T}_clock_fused.log 2>&1     # default / fused / statistics-only: kernel times, clocks, board power
cd /root/repo
ORT_BENCH_BACKEND=gloo timeout -k 10 600 python bench.py --gpus 2 --steps 5 --warmup 2 --full > $OUT/${T}_n2_gloo.json 2> $OUT/${T}_n2_gloo.err || echo "n2 rehearsal rc=$?"
# round 4: counter + clock pass of the Float32 kernels of config 5 (statistics kernel and summary kernel), the kernel statistics of
# one ort_spot_batch_f32 call, the GPU suite with its parity report, one parity soak of the final build
bash scripts/clock_config5.sh ${T}_clk5 > gpurun_out/${T}_clk5.log 2>&1; cp gpurun_out/${T}_clk5/summary.json profiles/${T}_sq_config5_final.json 2>/dev/null
(cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d /root/repo/gpurun_out/${T}_c5_kstats -- python3 /root/repo/scripts/run_workload.py config5 --mode stats --reps 6 > /root/repo/gpurun_out/${T}_c5_kstats.log 2>&1)
cp $(ls -t gpurun_out/${T}_c5_kstats/*/*kernel_stats.csv | head -1) profiles/${T}_config5_kernel_stats.csv 2>/dev/null
python -m pytest tests -m gpu -q > gpurun_out/${T}_gpu_suite.log 2>&1; cp gpurun_out/${T}_gpu_suite.log profiles/${T}_gpu_suite_parity_report.log
timeout -k 10 600 python scripts/soak_parity.py 900 4242 > gpurun_out/${T}_soak_parity_seed4242.log 2>&1; cp gpurun_out/${T}_soak_parity_seed4242.log profiles/
timeout -k 10 300 python scripts/soak_fused.py 60 7 > gpurun_out/${T}_soak_fused_seed7.log 2>&1
# the exchange leg alone with the native RCCL communicator of the C ABI (ort_comm_*), one rank: the code path the N > 1 line takes
timeout -k 10 300 python bench.py --workload config4 --steps 5 --warmup 2 > gpurun_out/${T}_config4_world1_native_rccl.json 2> gpurun_out/${T}_config4_world1.err || echo "config4 world1 rc=$?"
