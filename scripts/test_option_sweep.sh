#!/bin/bash
# Runs the GPU parity suite under non-default tunables (each must give the same answers) and
# EXITS NON-ZERO if any option set fails.  Tests that assert on path-specific statistics are
# deselected; the full-size and fuzz files are left to the plain suite (time).
set -o pipefail
out=$GRAFT_REPO_ROOT/gpurun_out/option_sweep.log
: > $out
failed=0
run() {  # $1 = label, rest = pytest arguments
  label=$1; shift
  echo "== $label" >> $out
  # (straight into a file of its own: behind a pipe into tail nothing would be written for the whole run)
  SZG_OPTIONS=$opts timeout -k 10 900 python -m pytest "$@" > $out.run 2>&1
  rc=$?
  tail -3 $out.run >> $out
  if [ $rc -ne 0 ]; then failed=$((failed + 1)); echo "FAILED ($rc): $label" >> $out; fi
}
# (test_refused_allocation_leaves_the_handle_working is about automatic mode, which steps aside on a refused allocation: a
# set that forces sketch=1 turns the refusal into the error the option documents.)
# (tie_mode=1 changes the contract -- any valid top-k among equal distances -- and has its own test,
# tests/test_gpu_parity.py::test_tie_mode_1_returns_a_valid_topk.)
# SWEEP_SETS="a=1 b=2,c=3" restricts the first loop to those sets (re-checking a fix)
# SWEEP_SKIP_MAIN=1 skips this loop (a box allows 20 minutes per call and this loop takes more than that by now: give the
# first call ten of the sets through SWEEP_SETS, the second the eleventh and everything below; formerly: first call
# `SWEEP_MQ_SETS="" SWEEP_SKIP_NORMS=1`, second call `SWEEP_SKIP_MAIN=1`)
[ -n "$SWEEP_SKIP_MAIN" ] || for opts in ${SWEEP_SETS:-serialize_scans=0 queries_per_launch=1 queries_per_launch=3,query_batch=5 \
            force_matrix=1 multi_query=0 contexts=1,mask_dense=0,coalesce=0 mq_min=8,mq_hits=256 \
            sketch=1,sketch_min_rows=1 sketch=1,multi_query=0,sketch_extra=0,sketch_min_rows=1 force_no_refine=1 \
            finish_thread=0,radius_mq=0 scan_group=1 scan_group=2 sketch_planes=3,scan_norms=1 scan_group_ring=4 sketch_matrix=1 \
            sketch_select=1 sketch_wide=1 sketch_f64=1,sketch=1,sketch_min_rows=1 \
            sketch_topk_collect=1,sketch=1,sketch_min_rows=1,multi_query=0}; do
  run "$opts" tests -m gpu -q -x --ignore=tests/test_gpu_fullsize.py --ignore=tests/test_gpu_bench_launch.py \
      --deselect tests/test_gpu_multiquery.py::test_shared_sweep_matches_oracle \
      --deselect tests/test_gpu_multiquery.py::test_shared_sweep_quantized_rows \
      --deselect tests/test_gpu_multiquery.py::test_shared_sweep_euclidean \
      --deselect tests/test_gpu_multiquery.py::test_shared_sweep_euclidean_far_from_origin \
      --deselect tests/test_gpu_multiquery.py::test_shared_sweep_int8_mfma \
      --deselect tests/test_gpu_multiquery.py::test_fused_selection_overflow_falls_back \
      --deselect tests/test_gpu_collection.py::test_concurrent_single_queries_are_coalesced \
      --deselect tests/test_gpu_radius_batch.py::test_concurrent_radius_callers_are_coalesced \
      --deselect tests/test_gpu_collection.py::test_search_batch_equals_search_by_search \
      --deselect tests/test_gpu_sketch_default.py::test_refused_allocation_leaves_the_handle_working \
      --deselect tests/test_gpu_fullsize.py \
      --ignore=tests/test_gpu_comm.py
done
# shared-sweep variants on the shared-sweep tests (their statistics do not depend on these)
for opts in ${SWEEP_MQ_SETS-force_matrix=1,serialize_scans=0 force_no_refine=1 finish_thread=0,mq_hits=256}; do
  run "multiquery tests, $opts" tests/test_gpu_multiquery.py -q -x \
      --deselect tests/test_gpu_multiquery.py::test_fused_selection_overflow_falls_back
done
# the row lists' whole-tile merge off (1) and on every tile that selects (2), on the files that open sketched handles
# (SWEEP_BULK_SETS="" skips them)
for opts in ${SWEEP_BULK_SETS-sketch_bulk=1 sketch_bulk=2}; do
  run "sketched handles, $opts" tests/test_gpu_sketch.py tests/test_gpu_sketch_default.py tests/test_gpu_sketch_lists.py \
      tests/test_gpu_sketch_state.py tests/test_gpu_sketch_planes.py tests/test_gpu_sketch_matrix.py \
      tests/test_gpu_sketch_select.py tests/test_gpu_sketch_wide.py tests/test_gpu_sketch_bulk.py \
      tests/test_gpu_certificates.py -m gpu -q -x
done
# the matrix sweep's shared form off (1) and in every sketch call of more than 32 queries (2), on the same files and its
# own (SWEEP_SHARE_SETS="" skips them)
for opts in ${SWEEP_SHARE_SETS-sketch_share=1 sketch_share=2}; do
  run "sketched handles, $opts" tests/test_gpu_sketch.py tests/test_gpu_sketch_default.py tests/test_gpu_sketch_lists.py \
      tests/test_gpu_sketch_state.py tests/test_gpu_sketch_planes.py tests/test_gpu_sketch_matrix.py \
      tests/test_gpu_sketch_select.py tests/test_gpu_sketch_wide.py tests/test_gpu_sketch_bulk.py \
      tests/test_gpu_sketch_share.py tests/test_gpu_certificates.py -m gpu -q -x
done
# a sketch batch's queries prepared on the card, every batch from one query on (2), on the same files, the masked, float64
# and device-query files and its own (SWEEP_PREP_SETS="" skips them)
for opts in ${SWEEP_PREP_SETS-query_prep=2}; do
  run "sketched handles, $opts" tests/test_gpu_sketch.py tests/test_gpu_sketch_default.py tests/test_gpu_sketch_lists.py \
      tests/test_gpu_sketch_state.py tests/test_gpu_sketch_planes.py tests/test_gpu_sketch_matrix.py \
      tests/test_gpu_sketch_select.py tests/test_gpu_sketch_wide.py tests/test_gpu_sketch_bulk.py \
      tests/test_gpu_sketch_share.py tests/test_gpu_sketch_masked.py tests/test_gpu_sketch_f64.py \
      tests/test_gpu_search_dev.py tests/test_gpu_coincident.py tests/test_gpu_certificates.py \
      tests/test_gpu_query_prep.py -m gpu -q -x
done
# the shared sweeps without the resident row norms (a test hook of its own: an environment variable read once per process)
if [ -z "$SWEEP_SKIP_NORMS" ]; then
  opts=""
  export SZG_NO_ROW_NORMS=1
  run "SZG_NO_ROW_NORMS=1 (int8 any-shape kernels, staged 16-bit sweep)" tests/test_gpu_multiquery.py tests/test_gpu_radius_batch.py -m gpu -q -x
  unset SZG_NO_ROW_NORMS
  export SZG_BF16_8BIT=0
  run "SZG_BF16_8BIT=0 (top-k batches on tiled 8-bit rows through the exact int8 sweep)" tests/test_gpu_multiquery.py -m gpu -q -x -k "8 or quantized or int8 or long_calls"
  unset SZG_BF16_8BIT
fi
cat $out
echo "option sets failed: $failed"
exit $failed
