export TMPDIR=/tmp; mkdir -p gpurun_out
timeout -k 10 500 python -u -m pytest ${TESTS:-tests/test_x3_gpu.py} -q --timeout 200 --timeout-method thread > gpurun_out/t2.log 2>&1; rc=$?; echo "pytest rc=$rc"; tail -4 gpurun_out/t2.log
case $rc in 124|134|137|139) exit $rc;; esac
timeout -k 10 200 python -u tools/x3_ab.py build_abl/r03_base.so build_abl/r03_new.so --ops ${ABOPS:-dgc1,dgrad,c1x3} --rounds 30 > gpurun_out/ab.log 2>&1; rc=$?; echo "ab rc=$rc"; cat gpurun_out/ab.log | tail -8
case $rc in 124|134|137|139) exit $rc;; esac
export SLK_BENCH_FULL=1   # = bench.py --full: the per-kernel pass ("kernels") runs only there
timeout -k 10 300 python -u bench.py --steps 30 --warmup 5 --no-cpu-baseline --no-k5 --no-conv-compare > gpurun_out/b2.log 2>&1; echo "bench rc=$?"; grep -o '"value": [0-9.]*\|"ms_per_step": [0-9.]*\|"kernels": {[^}]*}' gpurun_out/b2.log
