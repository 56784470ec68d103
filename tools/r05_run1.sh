O=${1:?usage: bash tools/r05_run1.sh OUTDIR}; mkdir -p $O
export TMPDIR=/tmp
timeout 900 python -m pytest tests -m gpu -x -q > $O/pytest.log 2>&1; echo "pytest rc $?" >> $O/pytest.log
timeout 600 python bench.py --full > $O/bench.json 2> $O/bench.err
for i in 1 2 3; do timeout 300 python tools/train_bench.py --iters 30 2>/dev/null | tail -1; done > $O/train_step.json
(cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_train -- python $GRAFT_REPO_ROOT/tools/train_bench.py > /dev/null 2>&1)
find /tmp/prof_train -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $O/kernel_stats_train.csv
tail -3 $O/pytest.log; cat $O/train_step.json
