O=${1:?usage: bash scripts/ab_genes_per_step.sh OUT_DIR}
mkdir -p $O
for g in ${GPS:-8 12 16 8}; do python bench.py --full --steps 4 --warmup 2 --genes-per-step $g --no-cpu-baseline --no-cfg3 --no-pipelined 2>/dev/null | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('genes_per_step=$g', d['value'], d['ms_per_step'], d['roofline']['achieved'])"; done > $O/gps.log 2>&1
cat $O/gps.log
