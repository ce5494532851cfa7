#!/bin/bash
# A/B of K1 builds and launch shapes on ONE GPU, in one go: every variant is timed by a short bench run (K1 kernel ms by HIP events),
# ROUNDS times round-robin (default 2), "base" first -- its own spread is the noise floor the others are read against.
#   base            the library as built, default options
#   chunk           the same library with KHG_K1_LAUNCH=chunk (one workgroup per chunk)
#   persistent      ... with KHG_K1_LAUNCH=persistent
#   prof-chunk, prof-persistent   ... with KHG_K1_PROF=1: the boundary-stamp line of each K1 launch (timings of these runs include the download)
#   ko<mask>        tools/bin/libkhg_ko<mask>.so (tools/build_k1_variants.sh; WRONG results, time only), one workgroup per chunk
#   <name>          tools/bin/libkhg_<name>.so with default options (e.g. a build of the parent commit)
# usage: [ROUNDS=3] [BENCH_ARGS="--utts 12500"] tools/ab_k1.sh name1 name2 ...
set -e
cd "$(dirname "$0")/.."
lib=kaldi_hmm_gmm_amd/libkhg_hip.so
mkdir -p tools/bin
cp $lib tools/bin/libkhg_base.so
trap 'cp tools/bin/libkhg_base.so '$lib EXIT
for round in $(seq 1 ${ROUNDS:-2}); do
for v in base "$@"; do
  env_launch=; env_prof=; src=tools/bin/libkhg_base.so
  case $v in
    base) ;;
    chunk|persistent) env_launch=$v ;;
    prof-chunk|prof-persistent) env_launch=${v#prof-}; env_prof=1 ;;
    ko*) src=tools/bin/libkhg_$v.so; env_launch=chunk ;;
    *) src=tools/bin/libkhg_$v.so ;;
  esac
  cp $src $lib
  KHG_K1_LAUNCH=$env_launch KHG_K1_PROF=$env_prof timeout -k 10 400 python bench.py --steps 3 --warmup 1 --no-fp32-line --no-cpu-baseline --per-call-utts 0 --no-recipe-beam-line $BENCH_ARGS 2>tools/bin/ab_k1.stderr | python -c "
import json,sys
d=json.loads(sys.stdin.read().splitlines()[-1]); k=d['kernel_ms_per_step']
print('%-16s k1 %.2f  step %.2f' % ('$v', k['k1_loglikes'], d['ms_per_step']))"
  grep -h "KHG_K1_PROF" tools/bin/ab_k1.stderr | tail -1 || true
done; done
