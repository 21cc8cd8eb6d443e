// options.cpp -- the option table (options.h).  Plain C++.
#include "options.h"

#include "scan_plan.h"

#include <cstring>

namespace szgi {

namespace {
template <int64_t lo, int64_t hi> bool in_range(int64_t v) { return v >= lo && v <= hi; }
bool any_value(int64_t) { return true; }
bool zero_or_one(int64_t v) { return v == 0 || v == 1; }
bool scan_group_known(int64_t v) { return v == 0 || v == 1 || v == 2 || v == 4; }
bool sketch_planes_known(int64_t v) { return v == 0 || v == 2 || v == 3; }
bool at_least_one(int64_t v) { return v >= 1; }
bool carry_stage_known(int64_t v) { return v >= 0 && v % 16 == 0 && (uint64_t)v <= kCarryStageMax; }

constexpr OptionStore kInt = OptionStore::kInt, kBool = OptionStore::kBool;
constexpr bool kScan = true, kFwd = true;  // (the two flags, where a row sets them)
// name, member, accepted values, refusal, store, known to szg_debug_option_check, forwarded to the sketch index.
// The six rows that are not forwarded govern the sketch index from outside (whether there is one, how it is asked) or
// are hooks of the handle's own paths; the sketch index keeps their defaults.
const OptionRow kRows[] = {
    {"sketch", &Options::sketch_on, in_range<0, 2>, "sketch is 0, 1 or 2", kInt, false, false},
    {"force_sketch_nomem", &Options::force_sketch_nomem, any_value, "", kBool, false, false},
    {"carry_stage_bytes", nullptr, carry_stage_known, "carry_stage_bytes is 0 or a multiple of 16 up to 64 MiB",
     OptionStore::kBytes, false, false},
    {"sketch_min_rows", &Options::sketch_min_rows, at_least_one, "sketch_min_rows out of range", OptionStore::kClamp30, false, false},
    {"sketch_list", &Options::sketch_list, in_range<0, 4096>, "sketch_list out of range", kInt, false, false},
    {"sketch_extra", &Options::sketch_extra, in_range<0, 900>, "sketch_extra out of range", kInt, false, false},
    {"slack", &Options::slack_min, in_range<0, 4096>, "slack out of range", kInt, false, kFwd},
    {"queries_per_launch", &Options::queries_per_launch, in_range<1, szg::kMaxSweepsPerLaunch>, "queries_per_launch out of range",
     kInt, false, kFwd},
    {"scan_group", &Options::scan_group, scan_group_known, "scan_group is 0, 1, 2 or 4", kInt, kScan, kFwd},
    {"scan_group_ring", &Options::scan_group_ring, szg::scan_group_ring_known,
     "scan_group_ring is 0 or a ring depth the library carries", kInt, kScan, kFwd},
    {"scan_norms", &Options::scan_norms, zero_or_one, "scan_norms is 0 or 1", kInt, kScan, kFwd},
    {"sketch_planes", &Options::sketch_planes, sketch_planes_known, "sketch_planes is 0, 2 or 3", kInt, kScan, kFwd},
    {"sketch_matrix", &Options::sketch_matrix, szg::sketch_matrix_known, "sketch_matrix is 0, 1 or 2", kInt, kScan, kFwd},
    {"sketch_select", &Options::sketch_select, szg::sketch_select_known, "sketch_select is 0 or 1", kInt, kScan, kFwd},
    {"sketch_wide", &Options::sketch_wide, szg::sketch_wide_known, "sketch_wide is 0, 1 or 2", kInt, kScan, kFwd},
    {"sketch_share", &Options::sketch_share, szg::sketch_share_known, "sketch_share is 0, 1 or 2", kInt, kScan, kFwd},
    {"sketch_bulk", &Options::sketch_bulk, szg::sketch_bulk_known, "sketch_bulk is 0 to 1024", kInt, kScan, kFwd},
    {"sketch_radius", &Options::sketch_radius, zero_or_one, "sketch_radius is 0 or 1", kInt, kScan, kFwd},
    {"sketch_masked", &Options::sketch_masked, szg::sketch_masked_known, "sketch_masked is 0 or 1", kInt, kScan, kFwd},
    {"sketch_f64", &Options::sketch_f64, zero_or_one, "sketch_f64 is 0 or 1", kInt, kScan, kFwd},
    {"sketch_topk_collect", &Options::sketch_topk_collect, zero_or_one, "sketch_topk_collect is 0 or 1", kInt, kScan, kFwd},
    {"query_prep", &Options::query_prep, in_range<0, 2>, "query_prep is 0, 1 or 2", kInt, kScan, kFwd},
    {"query_batch", &Options::query_batch, in_range<1, kMaxBatch>, "query_batch out of range", kInt, false, kFwd},
    {"radius_mq", &Options::radius_mq, zero_or_one, "radius_mq is 0 or 1", kInt, false, kFwd},
    {"finish_thread", &Options::finish_thread, zero_or_one, "finish_thread is 0 or 1", kInt, false, kFwd},
    {"contexts", nullptr, at_least_one, "contexts out of range", OptionStore::kContexts, false, kFwd},
    {"multi_query", &Options::multi_query, any_value, "", kBool, false, kFwd},
    {"mask_dense", &Options::mask_dense, any_value, "", kBool, false, kFwd},
    {"coalesce", &Options::coalesce, any_value, "", kBool, false, kFwd},
    {"force_matrix", &Options::force_matrix, any_value, "", kBool, false, kFwd},
    {"force_no_refine", &Options::force_no_refine, any_value, "", kBool, false, kFwd},
    {"mq_hits", &Options::mq_hits, in_range<64, 65536>, "mq_hits out of range", kInt, false, kFwd},
    {"mq_min", &Options::mq_min, in_range<1, 32>, "mq_min out of range", kInt, false, kFwd},
    {"serialize_scans", &Options::serialize_scans, any_value, "", kBool, false, kFwd},
    {"tie_mode", &Options::tie_mode, zero_or_one, "tie_mode must be 0 or 1", kInt, false, kFwd},
    {"force_escalate", &Options::force_escalate, any_value, "", kBool, false, kFwd},
};
constexpr int kRowCount = (int)(sizeof(kRows) / sizeof(kRows[0]));
static_assert(kRowCount <= 64, "one mark per row in a 64-bit word");
}  // namespace

const OptionRow *option_rows(int *n)
{
    *n = kRowCount;
    return kRows;
}

const OptionRow *option_find(const char *name)
{
    for (const OptionRow &r : kRows)
        if (strcmp(r.name, name) == 0) return &r;
    return nullptr;
}

const OptionRow *option_of(int Options::*member)
{
    for (const OptionRow &r : kRows)
        if (r.member == member) return &r;
    return nullptr;
}

const char *option_refusal(const OptionRow *row, int64_t value) { return row->accepts(value) ? nullptr : row->refusal; }

void option_store(const OptionRow *row, Options *o, int64_t value)
{
    switch (row->store) {
    case OptionStore::kInt: o->*row->member = (int)value; break;
    case OptionStore::kBool: o->*row->member = value != 0; break;
    case OptionStore::kClamp30: o->*row->member = (int)(value < (1 << 30) ? value : (1 << 30)); break;
    case OptionStore::kBytes: o->carry_stage_bytes = (uint64_t)value; break;
    case OptionStore::kContexts: break;
    }
}

int64_t option_load(const OptionRow *row, const Options &o)
{
    if (row->store == OptionStore::kBytes) return (int64_t)o.carry_stage_bytes;
    return row->member ? o.*row->member : 0;
}

}  // namespace szgi
