// The bulk upsert and RemoveDocuments of the C++ host mirror (include/syzgy_collection.hpp) against the same mirror
// brought to the same state by AddDocument / removeDocument in a loop.  Built and run by tests/test_gpu_bulk.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "syzgy_collection.hpp"

using namespace syzgydb;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "CHECK failed at %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

static void same(Collection &a, Collection &b, const std::vector<std::vector<double>> &queries)
{
    CHECK(a.GetAllIDs() == b.GetAllIDs());
    for (uint64_t id : a.GetAllIDs()) {
        const Document x = a.GetDocument(id), y = b.GetDocument(id);
        CHECK(x.Vector == y.Vector && x.Metadata == y.Metadata);
    }
    for (const auto &q : queries) {
        SearchArgs s;
        s.Vector = q;
        s.K = 7;
        const SearchResults x = a.Search(s), y = b.Search(s);
        CHECK(x.Results.size() == y.Results.size() && !x.Results.empty());
        for (size_t i = 0; i < x.Results.size(); i++)
            CHECK(x.Results[i].ID == y.Results[i].ID && x.Results[i].Distance == y.Results[i].Distance &&
                  x.Results[i].Metadata == y.Results[i].Metadata);
    }
}

int main()
{
    const int dim = 17, n = 300;
    CollectionOptions o;
    o.DistanceMethod = Cosine;
    o.DimensionCount = dim;
    o.Quantization = 8;
    auto bulk = Collection::NewCollection(o), loop = Collection::NewCollection(o);
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> u(-1, 1);
    auto block = [&](size_t count) {
        std::vector<double> v(count * dim);
        for (double &x : v) x = u(rng);
        return v;
    };
    auto feed_loop = [&](const std::vector<uint64_t> &ids, const std::vector<double> &v, const std::vector<std::string> &m) {
        for (size_t j = 0; j < ids.size(); j++)
            loop->AddDocument(ids[j], std::vector<double>(v.begin() + j * dim, v.begin() + (j + 1) * dim), m[j]);
    };
    std::vector<std::vector<double>> queries;
    for (int i = 0; i < 3; i++) queries.push_back(block(1));

    // new ids only
    std::vector<uint64_t> ids;
    std::vector<std::string> metas;
    for (int i = 0; i < n; i++) ids.push_back(100 + i), metas.push_back("m" + std::to_string(i));
    std::vector<double> v = block(n);
    bulk->AddDocuments(ids, v, metas);
    feed_loop(ids, v, metas);
    same(*bulk, *loop, queries);

    // a mix of existing ids, new ids and ids listed twice (new and existing): the last entry stays
    ids = {100, 5000, 163, 164, 5001, 5000, 399, 163, 5002, 115};
    metas.clear();
    for (size_t j = 0; j < ids.size(); j++) metas.push_back("second" + std::to_string(j));
    v = block(ids.size());
    bulk->AddDocuments(ids, v, metas);
    feed_loop(ids, v, metas);
    CHECK(bulk->GetDocumentCount() == n + 3);
    same(*bulk, *loop, queries);

    // removals: an unknown id throws before anything changes
    bool threw = false;
    try {
        bulk->RemoveDocuments({101, 102, 9999});
    } catch (const std::runtime_error &) {
        threw = true;
    }
    CHECK(threw && bulk->GetDocumentCount() == n + 3);
    same(*bulk, *loop, queries);
    const std::vector<uint64_t> gone = {100, 163, 164, 227, 5001, 399};
    CHECK(bulk->RemoveDocuments(gone) == gone.size());
    for (uint64_t id : gone) loop->removeDocument(id);
    CHECK(bulk->GetDocumentCount() == n + 3 - (int)gone.size());
    CHECK(bulk->RemoveDocuments({}) == 0);
    same(*bulk, *loop, queries);
    std::puts("CPP_BULK_OK");
    return 0;
}
