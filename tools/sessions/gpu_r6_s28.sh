# Round 6, GPU session 28 (last): after the heuristic fix for tap-subset convolutions (gemm.hip) the kernel-source hash changed: the HBM traffic
# passes once more (the bench line quotes them only for the sources they were measured on), the tests that touch the change, the default bench line.
set -u
REPO=$PWD
OUT=$REPO/gpurun_out/r6_s28
mkdir -p $OUT
export TMPDIR=/tmp
(timeout 900 python -m pytest tests/test_kernels.py tests/test_unet.py tests/test_unet_ctx.py -q -m gpu 2>&1 | tail -3) > $OUT/tests.txt
cd /tmp
timeout 200 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -- python $REPO/tools/profile_step.py > /dev/null 2>&1
timeout 200 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -- python $REPO/tools/profile_step.py > /dev/null 2>&1
cd $REPO
python tools/pmc_traffic.py $OUT/pmc_fetch $OUT/pmc_write $OUT/gemm_traffic.json > $OUT/kernel_traffic.json 2> $OUT/kernel_traffic.err
rm -rf $OUT/pmc_fetch $OUT/pmc_write
cp $OUT/gemm_traffic.json profiles/gemm_traffic.json
(timeout 500 python bench.py --full) > $OUT/bench.json 2> $OUT/bench.err
cat $OUT/tests.txt; cut -c1-200 $OUT/bench.json; grep -o '"traffic": [0-9a-z]*' $OUT/bench.json
