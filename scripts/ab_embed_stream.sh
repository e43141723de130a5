O=${1:?usage: bash scripts/ab_embed_stream.sh OUT_DIR}
mkdir -p $O
timeout 900 python -m pytest tests/test_ops_gpu.py -x -q -m gpu -k "embed" > $O/pytest_ops.log 2>&1; echo "rc=$?" >> $O/pytest_ops.log; tail -4 $O/pytest_ops.log
timeout 1500 python -m pytest tests/test_model_gpu.py -x -q -m gpu -k "seq2reg or golden or production_dims or full_depth or trunk" > $O/pytest_model.log 2>&1; echo "rc=$?" >> $O/pytest_model.log; tail -6 $O/pytest_model.log
python bench.py --full --no-cpu-baseline --no-cfg3 --no-pipelined 2>/dev/null | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['roofline']['achieved'], d['batch_of_8']['value'], {k:v['ms_per_step'] for k,v in d['kernel_families'].items() if 'layernorm' in k})" > $O/bench.log 2>&1; cat $O/bench.log
