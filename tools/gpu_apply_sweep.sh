# apply-launch geometry sweep (SWT_EXTRA_FLAGS rebuilds on the box)
export TMPDIR=/tmp
OUT=${OUT:-$(mktemp -d)}  # the bench lines and their stderr
for v in "${@}"; do
  export SWT_EXTRA_FLAGS="$v"
  python -c "import importlib; importlib.import_module('subword-tokenizers_amd._build').build()" || exit 1
  for c in open lex; do
    timeout -k 10 300 python bench.py --workload bpe_train --corpus $c --full > $OUT/sweep_$c.json 2> $OUT/sweep.err || { tail -5 $OUT/sweep.err; exit 1; }
    python - <<PY
import json
d=json.load(open("$OUT/sweep_$c.json"))
print("$v $c:", d["value"], "s/1k  merge_us", d["roofline"]["kernel_us"], flush=True)
PY
  done
done
