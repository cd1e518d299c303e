R=${GRAFT_REPO_ROOT:-$(pwd)}; cd $R
for rep in 1 2; do
  line=$(timeout 300 python bench.py --config c3 --full --no-cpu-baseline --steps 10 --parity-rows 50000 2>&1 | tail -1)
  echo "$line" | python -c "
import json, sys; l=json.load(sys.stdin); print('step', round(l['ms_per_step'],4), 'kernel', round(l['roofline']['launch_ms'],4), 'err', l['parity']['max_rel_err'], 'one-shot', l['config'].get('one_shot_ms'))"
done
