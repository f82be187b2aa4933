#!/bin/bash
# Full evidence pass of a round on an MI355X (bash profiles/collect_all.sh from the repo root): the GPU suite, the --full bench line
# of every BASELINE.json config, then profiles/collect.sh (rocprofv3 kernel traces and PMC passes); outputs under
# $PROFILE_OUT/{final,prof}/ (default profile_out/ in the repo root), copied into profiles/ as r<round>_* by hand.
R=${GRAFT_REPO_ROOT:-$(pwd)}
F=${PROFILE_OUT:-$R/profile_out}/final
mkdir -p $F
cd $R
python -m pytest tests -m gpu -x -q 2>&1 | tail -5 > $F/gputest.txt
python bench.py --full --steps 20 --warmup 5 --full-record $F/bench_default_full.json > $F/bench_default.json 2> $F/bench_default.err
python bench.py --full --steps 20 --warmup 5 --all-heads --no-cpu-baseline --no-secondary --full-line --full-record "" > $F/bench_all_heads.json 2>/dev/null
for c in c3 c5; do python bench.py --full --steps 20 --warmup 5 --config $c --no-cpu-baseline --no-secondary --full-line --full-record "" > $F/bench_$c.json 2>/dev/null; done
python bench.py --full --config c4 --full-line --full-record "" > $F/bench_c4.json 2>/dev/null     # (with the oracle check of 8 records)
# two ranks on this box's one GPU (gloo rendezvous, shared device: a code-path run, not a scaling measurement) -- the line must prove
# itself: every rank's objects against the oracle, per-rank times, CPU binding, cpu_baseline (bench.py, bench_dist.py)
python bench.py --full --gpus 2 --no-secondary --min-seconds 1 --full-record "" > $F/bench_gpus2_shared.json 2>/dev/null
python bench.py --full --gpus 2 --config c4 --full-record "" > $F/bench_c4_gpus2_shared.json 2>/dev/null
python bench.py --full --config c1 --full-line --full-record "" > $F/bench_c1.json 2>/dev/null
bash profiles/collect.sh > $F/collect.log 2>&1
cat $F/gputest.txt
F=$F python - <<'PY'
import json,glob,os
for f in sorted(glob.glob(os.path.join(os.environ["F"], "bench_*.json"))):
    try:
        d=json.loads(open(f).read().strip().splitlines()[-1])
        print(f.split("/")[-1], "value %.4g"%d["value"], "ms %.5f"%d["ms_per_step"], (d.get("roofline") or {}).get("frac"), (d.get("roofline") or {}).get("launch_ms"))
    except Exception as e: print(f, "failed", e)
PY
