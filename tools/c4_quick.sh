R=${GRAFT_REPO_ROOT:-$(pwd)}; cd $R
for lib in "" $R/geopolars_amd/variants/*.so; do
  [ -e "$lib" ] || [ -z "$lib" ] || continue
  line=$(GPK_LIB_PATH=$lib timeout 300 python bench.py --config c4 --full --no-cpu-baseline --steps 6 --parity-rows 50000 2>&1 | tail -1)
  echo "$line" | python -c "
import json, sys; l=json.load(sys.stdin); print('$lib', 'step', round(l['ms_per_step'],4), 'kernel', round(l['roofline']['launch_ms'],4), l['parity'].get('bit_exact'), json.dumps(l['config'])[-900:])"
done
