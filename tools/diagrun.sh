set -u
O=${1:-build/diag_out}; mkdir -p $O
for d in base 1 2 3 4 32; do
  if [ $d = base ]; then L=recommendation-models_amd/csrc/librmx.so; else L=build/diag$d/librmx.so; fi
  RMX_LIB=$L timeout -k 10 120 python bench.py --full --steps 50 --warmup 5 --no-companion --no-cpu-baseline --settle-ms 300 > $O/$d.json 2> $O/$d.err || exit 1
  python3 -c "
import json; d=json.load(open('$O/$d.json')); print('$d', d['ms_per_step'], {k: v['avg_ms'] for k, v in d['stages'].items()})"
done
