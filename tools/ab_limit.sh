#!/bin/bash
# A/B of the default-limit batch (params == NULL => 1000) inside one session: "name:ENV=val,ENV=val" per argument
out=${OUT:-out}/ab
mkdir -p "$out"
for spec in "$@"; do
  name=${spec%%:*}; kv=${spec#*:}
  (
    IFS=','; for e in $kv; do case "$e" in ?*=*) export "$e";; esac; done
    timeout -k 10 300 python bench.py --full --limit 1000 --depth 4 --cpu-seconds 0 --no-extras --steps 30 > "$out/L.$name.json" 2>"$out/L.$name.err"
  )
  python - "$name" "$out/L.$name.json" <<'PY'
import json, sys
try:
    d = json.load(open(sys.argv[2]))
    print("%-12s %9.0f q/s %.4f ms/step  %s" % (sys.argv[1], d["value"], d["ms_per_step"], [(k["kernel"][:24], k["ms"]) for k in d["roofline"]["per_kernel"]][:4]))
except Exception as e:
    print(sys.argv[1], "failed", e)
PY
done
