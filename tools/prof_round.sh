# Round profile: the full bench line (bench.py --full), rocprofv3 kernel stats of the same command, PMC traffic passes, Kron MFMA counters.
# usage (on the GPU box): bash tools/prof_round.sh <tag>      outputs under $PROF_OUT/<tag>/ (default prof_out/<tag>/) ; copy into profiles/
TAG=${1:-v6}
O=${PROF_OUT:-prof_out}/$TAG
set -x
mkdir -p $O
O=$(cd $O && pwd)
python bench.py --full --detail-json $O/bench_detail.json > $O/bench.json.log 2>$O/bench.err
R=$PWD
cd /tmp && export TMPDIR=/tmp
# (the profiled passes skip the exchange_overhead leg: it runs the same r = 20 kernels at 12.5M rows, which would be averaged into the
#  per-kernel figures of the N = 100M workload; tools/sharded_step_trace.sh profiles that leg on its own)
rocprofv3 --kernel-trace --stats -d $O/stats -- python3 $R/bench.py --full --no-cpu-baseline --no-exchange-leg > $O/stats.log 2>&1
# (round 6: the counter passes run on the packed layout -- bytes do not depend on where the streams live, and the placement probe's
#  13M-row launches of the same kernels would be averaged into the per-launch figures; the stats pass above keeps the probe and
#  tools/rocpd_stats.py adds a row per sweep kernel for its full-size launches only)
rocprofv3 --pmc FETCH_SIZE -d $O/pmc_f -- python3 $R/bench.py --full --placement packed --no-cpu-baseline --no-kron --no-wide-rank --no-exchange-leg --steps 3 --warmup 1 > $O/pmc_f.log 2>&1
rocprofv3 --pmc WRITE_SIZE -d $O/pmc_w -- python3 $R/bench.py --full --placement packed --no-cpu-baseline --no-kron --no-wide-rank --no-exchange-leg --steps 3 --warmup 1 > $O/pmc_w.log 2>&1
cd $R
python tools/rocpd_stats.py $O/stats > $O/kernel_stats.csv
python tools/pmc_traffic.py $O/pmc_f $O/pmc_w > $O/pmc_traffic.json
rm -rf $O/stats $O/pmc_f $O/pmc_w
tail -c 400 $O/bench.json.log
# afterwards, in the repo: cp the three files into profiles/ as r03_bench_*_$TAG and run  python tools/curate_pmc_traffic.py $O/pmc_traffic.json $TAG  (never copy the raw table over profiles/pmc_traffic.json: bench.py reads the curated form)
