// The option table (syzgydb_amd/csrc/options.h + options.cpp) without HIP and without a GPU, against a list written out
// by hand from the two if-chains szg_set_option was before the table: per name the default, the two flags, accepted edge
// values with what they store, refused edge values and the refusal's text.  tests/test_options_cpu.py builds it from
// options.cpp and scan_plan.cpp with -fsanitize=address,undefined and runs it: argv[1] = include/syzgy_scan.h, whose
// option comment must name every option; argv[2] = --list prints the list (tests/option_cases.py holds the same one).
#include "../../syzgydb_amd/csrc/options.h"

#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

using namespace szgi;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
            exit(1);                                      \
        }                                                 \
    } while (0)

namespace {

constexpr int kCtx = 4;  // contexts per shard: "contexts" is held against it by the handle, not by the table
constexpr int64_t kMiB64 = 64ll << 20;
using Stores = std::vector<std::pair<int64_t, int64_t>>;

struct Expect {
    const char *name;
    int64_t def;
    bool check, forwarded;
    Stores accepted;                // value, what is stored
    std::vector<int64_t> refused;
    const char *text;               // "" where nothing is refused
};

const Stores kBool = {{7, 1}, {-1, 1}, {0, 0}, {1, 1}};  // every value is accepted; value != 0 is stored
Stores same(std::initializer_list<int64_t> vs)
{
    Stores s;
    for (int64_t v : vs) s.emplace_back(v, v);
    return s;
}

const std::vector<Expect> kExpect = {
    // not forwarded
    {"sketch", 2, false, false, same({0, 1, 2}), {-1, 3}, "sketch is 0, 1 or 2"},
    {"force_sketch_nomem", 0, false, false, kBool, {}, ""},
    {"carry_stage_bytes", 0, false, false, same({16, kMiB64, 0}), {8, -16, kMiB64 + 16},
     "carry_stage_bytes is 0 or a multiple of 16 up to 64 MiB"},
    {"sketch_min_rows", 4096, false, false, {{1, 1}, {1ll << 40, 1 << 30}, {1 << 30, 1 << 30}, {5000, 5000}}, {0, -1},
     "sketch_min_rows out of range"},
    {"sketch_list", 0, false, false, same({4096, 0}), {-1, 4097}, "sketch_list out of range"},
    {"sketch_extra", 30, false, false, same({0, 900}), {-1, 901}, "sketch_extra out of range"},
    // forwarded
    {"slack", 16, false, true, same({0, 4096}), {-1, 4097}, "slack out of range"},
    {"queries_per_launch", 16, false, true, same({1, 16}), {0, 17}, "queries_per_launch out of range"},
    {"scan_group", 0, true, true, same({1, 2, 4, 0}), {-1, 3, 5}, "scan_group is 0, 1, 2 or 4"},
    {"scan_group_ring", 0, true, true, same({4, 6, 0}), {-1, 1, 5, 7, 12}, "scan_group_ring is 0 or a ring depth the library carries"},
    {"scan_norms", 0, true, true, same({1, 0}), {-1, 2}, "scan_norms is 0 or 1"},
    {"sketch_planes", 0, true, true, same({2, 3, 0}), {-1, 1, 4}, "sketch_planes is 0, 2 or 3"},
    {"sketch_matrix", 0, true, true, same({1, 2, 0}), {-1, 3}, "sketch_matrix is 0, 1 or 2"},
    {"sketch_select", 0, true, true, same({1, 0}), {-1, 2}, "sketch_select is 0 or 1"},
    {"sketch_wide", 0, true, true, same({1, 2, 0}), {-1, 3}, "sketch_wide is 0, 1 or 2"},
    {"sketch_share", 0, true, true, same({1, 2, 0}), {-1, 3}, "sketch_share is 0, 1 or 2"},
    {"sketch_bulk", 0, true, true, same({1024, 0}), {-1, 1025}, "sketch_bulk is 0 to 1024"},
    {"sketch_radius", 0, true, true, same({1, 0}), {-1, 2}, "sketch_radius is 0 or 1"},
    {"sketch_masked", 0, true, true, same({1, 0}), {-1, 2}, "sketch_masked is 0 or 1"},
    {"sketch_f64", 0, true, true, same({1, 0}), {-1, 2}, "sketch_f64 is 0 or 1"},
    {"sketch_topk_collect", 0, true, true, same({1, 0}), {-1, 2}, "sketch_topk_collect is 0 or 1"},
    {"query_prep", 0, true, true, same({1, 2, 0}), {-1, 3}, "query_prep is 0, 1 or 2"},
    {"query_batch", 16, false, true, same({1, 96}), {0, 97}, "query_batch out of range"},
    {"radius_mq", 1, false, true, same({0, 1}), {-1, 2}, "radius_mq is 0 or 1"},
    {"finish_thread", 1, false, true, same({0, 1}), {-1, 2}, "finish_thread is 0 or 1"},
    {"contexts", kCtx, false, true, same({1, kCtx}), {0, kCtx + 1}, "contexts out of range"},
    {"multi_query", 1, false, true, kBool, {}, ""},
    {"mask_dense", 1, false, true, kBool, {}, ""},
    {"coalesce", 1, false, true, kBool, {}, ""},
    {"force_matrix", 0, false, true, kBool, {}, ""},
    {"force_no_refine", 0, false, true, kBool, {}, ""},
    {"mq_hits", 1024, false, true, same({64, 65536}), {63, 65537}, "mq_hits out of range"},
    {"mq_min", 2, false, true, same({1, 32}), {0, 33}, "mq_min out of range"},
    {"serialize_scans", 1, false, true, kBool, {}, ""},
    {"tie_mode", 0, false, true, same({1, 0}), {2, -1}, "tie_mode must be 0 or 1"},
    {"force_escalate", 0, false, true, kBool, {}, ""},
};

void print_list()
{
    std::vector<std::string> lines;
    for (const Expect &e : kExpect) {
        std::ostringstream o;
        o << e.name << " default=" << e.def << " check=" << e.check << " forwarded=" << e.forwarded << " accepted=";
        for (size_t i = 0; i < e.accepted.size(); i++) o << (i ? "," : "") << e.accepted[i].first << ":" << e.accepted[i].second;
        o << " refused=";
        for (size_t i = 0; i < e.refused.size(); i++) o << (i ? "," : "") << e.refused[i];
        o << " text=" << e.text;
        lines.push_back(o.str());
    }
    for (const std::string &l : std::set<std::string>(lines.begin(), lines.end())) puts(l.c_str());
}

}  // namespace

int main(int argc, char **argv)
{
    CHECK(argc >= 2, "usage: test_options include/syzgy_scan.h [--list]");
    if (argc > 2 && !strcmp(argv[2], "--list")) {
        print_list();
        return 0;
    }

    // the table has exactly the expected names, each once
    int n = 0;
    const OptionRow *rows = option_rows(&n);
    CHECK(n == (int)kExpect.size() && n <= 64, "%d rows, %zu expected", n, kExpect.size());
    std::set<std::string> names;
    for (int i = 0; i < n; i++) {
        CHECK(names.insert(rows[i].name).second, "%s: twice in the table", rows[i].name);
        CHECK(option_find(rows[i].name) == &rows[i], "%s: not found where it is", rows[i].name);
        if (rows[i].member) CHECK(option_of(rows[i].member) == &rows[i], "%s: two rows store into one member", rows[i].name);
    }
    CHECK(!option_find("nonsense") && !option_find("") && !option_find("sketch_") && !option_find("slack_min"), "a name too many");

    int n_check = 0, n_forwarded = 0;
    const Options defaults;
    for (const Expect &e : kExpect) {
        const OptionRow *r = option_find(e.name);
        CHECK(r, "%s: not in the table", e.name);
        CHECK(r->scan_check == e.check && r->forwarded == e.forwarded, "%s: flags", e.name);
        n_check += r->scan_check;
        n_forwarded += r->forwarded;
        const bool contexts = r->store == OptionStore::kContexts;
        CHECK(contexts == !strcmp(e.name, "contexts"), "%s: the handler's row", e.name);
        if (!contexts) CHECK(option_load(r, defaults) == e.def, "%s: default %lld", e.name, (long long)option_load(r, defaults));
        Options o;
        for (const auto &a : e.accepted) {
            CHECK(!option_refusal(r, a.first), "%s = %lld refused", e.name, (long long)a.first);
            option_store(r, &o, a.first);
            if (!contexts)
                CHECK(option_load(r, o) == a.second, "%s = %lld stores %lld", e.name, (long long)a.first, (long long)option_load(r, o));
        }
        for (int64_t v : e.refused) {
            if (contexts && v > kCtx) continue;  // (the handle refuses it, with the row's text: tests/test_gpu_options.py)
            const char *why = option_refusal(r, v);
            CHECK(why && !strcmp(why, e.text), "%s = %lld: %s", e.name, (long long)v, why ? why : "accepted");
        }
        if (e.refused.empty())  // the Booleans: nothing is refused
            for (int64_t v : {INT64_MIN, (int64_t)-2, (int64_t)2, (int64_t)1 << 40, INT64_MAX}) {
                CHECK(!option_refusal(r, v), "%s = %lld refused", e.name, (long long)v);
                option_store(r, &o, v);
                CHECK(option_load(r, o) == 1, "%s = %lld is not stored as 1", e.name, (long long)v);
            }
        else
            CHECK(!strcmp(r->refusal, e.text), "%s: text", e.name);
        // a store touches its own member alone
        Options p, q;
        option_store(r, &p, e.accepted[0].first);
        for (int i = 0; i < n; i++)
            if (&rows[i] != r) CHECK(option_load(&rows[i], p) == option_load(&rows[i], q), "%s moved %s", e.name, rows[i].name);
    }
    CHECK(n_check == 14 && n_forwarded == 30, "%d known to the check hook, %d forwarded", n_check, n_forwarded);

    // every name occurs in the option comment above szg_set_option
    std::ifstream in(argv[1]);
    CHECK(in.good(), "cannot read %s", argv[1]);
    std::stringstream ss;
    ss << in.rdbuf();
    const std::string text = ss.str();
    const size_t end = text.find("int szg_set_option(");
    CHECK(end != std::string::npos, "no szg_set_option in %s", argv[1]);
    const size_t begin = text.rfind("/*", end);
    CHECK(begin != std::string::npos, "no comment above szg_set_option");
    const std::string comment = text.substr(begin, end - begin);
    for (const Expect &e : kExpect) {
        bool found = false;
        for (size_t at = comment.find(e.name); at != std::string::npos && !found; at = comment.find(e.name, at + 1)) {
            auto word = [](char c) { return isalnum((unsigned char)c) || c == '_'; };
            found = (at == 0 || !word(comment[at - 1])) && !word(comment[at + strlen(e.name)]);
        }
        CHECK(found, "%s: not in the option comment of %s", e.name, argv[1]);
    }
    puts("options ok");
    return 0;
}
