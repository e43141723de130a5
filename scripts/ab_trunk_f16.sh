# fp16 trunk copy (VF_TRUNK16=f16, default) against the fp32 trunk (VF_TRUNK16=0): op test, model parity subset, bench A/B
O=${1:?usage: bash scripts/ab_trunk_f16.sh OUT_DIR}
mkdir -p $O
timeout 900 python -m pytest tests/test_ops_gpu.py -x -q -m gpu -k "fp16_trunk or gemm_ln_producer" > $O/pytest_ops.log 2>&1; echo "rc=$?" >> $O/pytest_ops.log; tail -4 $O/pytest_ops.log
timeout 1500 python -m pytest tests/test_model_gpu.py tests/test_configs_gpu.py -x -q -m gpu > $O/pytest_model.log 2>&1; echo "rc=$?" >> $O/pytest_model.log; tail -15 $O/pytest_model.log
for m in 0 f16 0 f16; do VF_TRUNK16=$m python bench.py --full --no-cpu-baseline --no-cfg3 --no-pipelined 2>/dev/null | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('trunk16=$m', d['value'], d['ms_per_step'], d['roofline']['achieved'], d['batch_of_8']['value'])"; done > $O/bench_ab.log 2>&1
cat $O/bench_ab.log
