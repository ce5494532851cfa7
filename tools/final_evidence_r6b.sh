#!/bin/bash
# Round-6 evidence after the last kernel change (K2 score prefetch by 32-byte sectors): GPU suite, rocprofv3 passes, the default bench
# line with the counter summary of the same sources in place, time-boxed sweeps of the K2 paths.
cd "$GRAFT_REPO_ROOT"
OUT=${1:?usage: bash tools/final_evidence_r6b.sh OUT_DIR}
mkdir -p "$OUT"
python -m pytest tests -m gpu -q > "$OUT"/r6_gpu_tests.log 2>&1; tail -n 2 "$OUT"/r6_gpu_tests.log
bash tools/profile_r6.sh > "$OUT"/r6_profile.log 2>&1
python tools/summarize_prof.py gpurun_out/prof_r6 r6 > /dev/null 2>&1
python bench.py --full > "$OUT"/r6_bench_default.json 2> "$OUT"/r6_bench_default.err
python - > "$OUT"/r6_fuzz_graphs.txt 2>&1 <<'PY'
import sys
sys.path.insert(0, "tests")
import fuzzlib
from kaldi_hmm_gmm_amd import Context
ctx = Context(0)
print("graph fuzz ok:", fuzzlib.fuzz_graphs(ctx, budget=330.0, seed=9702))
PY
python - > "$OUT"/r6_fuzz_parity.txt 2>&1 <<'PY'
import sys
sys.path.insert(0, "tests")
import fuzzlib
from kaldi_hmm_gmm_amd import Context
ctx = Context(0)
print("fuzz ok:", fuzzlib.fuzz_parity(ctx, budget=270.0, seed=9701))
PY
tail -n 1 "$OUT"/r6_fuzz_graphs.txt "$OUT"/r6_fuzz_parity.txt
OUT="$OUT" python - <<'PY'
import json, os
d = json.loads(open(os.environ["OUT"] + "/r6_bench_default.json").read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], d["kernel_ms_per_step"], d["roofline"].get("traffic"), d["check"]["ali_mismatch_utts"], d["check"]["oracle_utts"], (d.get("flat_start_line") or {}).get("ms_per_step"))
PY
