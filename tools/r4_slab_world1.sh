#!/bin/bash
# world-1 overhead of the slab-decomposed drivers when every message goes through uammd_comm_* (RCCL, the ring closing on the rank itself)
R=${REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}; cd $R; OUT=${OUT:-bench_out}; mkdir -p $OUT
timeout 900 python bench.py --gpus 1 --force-distributed --steps 200 --warmup 20 --fcm-steps 100 --no-cpu-baseline --full > $OUT/r4_bench_slab_world1.json 2> $OUT/r4_bench_slab_world1.err; echo "rc=$?"; tail -3 $OUT/r4_bench_slab_world1.err
timeout 900 python bench.py --gpus 1 --steps 200 --warmup 20 --fcm-steps 100 --no-cpu-baseline --full > $OUT/r4_bench_single.json 2>/dev/null
OUT=$OUT python - <<'PY'
import json, os
a = json.load(open(os.environ["OUT"] + "/r4_bench_slab_world1.json")); b = json.load(open(os.environ["OUT"] + "/r4_bench_single.json"))
print("comm:", a["comm"])
print("LJ   slab world 1 %.4f ms  single %.4f ms  (+%.1f %%)" % (a["ms_per_step"], b["ms_per_step"], 100 * (a["ms_per_step"] / b["ms_per_step"] - 1)))
print("FCM  slab world 1 %.4f ms  single %.4f ms  (+%.1f %%)" % (a["fcm"]["ms_per_step"], b["fcm"]["ms_per_step"], 100 * (a["fcm"]["ms_per_step"] / b["fcm"]["ms_per_step"] - 1)))
print("C5   slab world 1 %.4f ms  single %.4f ms  (+%.1f %%)" % (a["fcm_c5"]["ms_per_step"], b["fcm_c5"]["ms_per_step"], 100 * (a["fcm_c5"]["ms_per_step"] / b["fcm_c5"]["ms_per_step"] - 1)))
print(a["config"]["workload"])
PY
