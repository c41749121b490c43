// The C++ host layer's item-to-item similarity (ImplicitSequenceModel::similar_items over sbr_similar_items), driven from
// tests/test_similar_cpp.py: the reference protocol's MovieLens split (seed [42;16], user_based_split 0.2), an LSTM fitted on
// the train part, then the k nearest neighbours of every seventh item, by cosine without the query and by dot product with it.
// The items and score bits of both go to a binary file the harness compares with the Python calls on the same model.
//
// Usage: similar_tests <movielens csv> <k> <out file>; exit code 0 = assertions held.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "sbr.hpp"

using namespace sbr;

#define CHECK(cond)                                                                               \
    do {                                                                                          \
        if (!(cond)) {                                                                            \
            std::fprintf(stderr, "%s:%d: assertion failed: %s\n", __FILE__, __LINE__, #cond);     \
            std::exit(1);                                                                         \
        }                                                                                         \
    } while (0)

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s <movielens csv> <k> <out file>\n", argv[0]);
        return 2;
    }
    const std::size_t k = (std::size_t)std::stoul(argv[2]);
    try {
        data::Interactions data = datasets::download_movielens_100k(argv[1]);
        std::array<std::uint8_t, 16> seed;
        seed.fill(42);
        XorShiftRng rng = XorShiftRng::from_seed(seed);
        auto [train, test] = data::user_based_split(data, rng, 0.2f);
        const data::CompressedInteractions tr = train.to_compressed();
        auto model = models::lstm::Hyperparameters::new_(data.num_items(), 32)
                         .embedding_dim(32)
                         .learning_rate(0.16f)
                         .l2_penalty(0.0004f)
                         .loss(models::Loss::WARP)
                         .num_epochs(1)
                         .batch_sequences(64)
                         .rng(rng)
                         .build();
        model.fit(tr).unwrap();
        std::vector<ItemId> queries;
        for (std::size_t i = 0; i < data.num_items(); i += 7) queries.push_back((ItemId)i);
        const models::Recommendations cosine = model.similar_items(queries, k).unwrap();
        const models::Recommendations dot = model.similar_items(queries, k, models::Similarity::Dot, true).unwrap();
        for (const models::Recommendations* r : {&cosine, &dot}) {
            CHECK(r->num_users == queries.size() && r->k == k && r->items.size() == queries.size() * k && r->scores.size() == r->items.size());
            for (std::size_t j = 0; j < r->num_users; ++j)
                for (std::size_t x = 1; x < k; ++x) CHECK(r->scores[j * k + x - 1] >= r->scores[j * k + x]);
        }
        // a cosine row leaves its query out and stays within [-1, 1] up to rounding
        for (std::size_t j = 0; j < cosine.num_users; ++j)
            for (std::size_t x = 0; x < k; ++x) {
                CHECK(cosine.items[j * k + x] != (std::uint32_t)queries[j]);
                CHECK(std::fabs(cosine.scores[j * k + x]) <= 1.00001f);
            }
        CHECK(model.similar_items({}, k).unwrap().items.empty());
        std::FILE* f = std::fopen(argv[3], "wb");
        CHECK(f);
        for (const models::Recommendations* r : {&cosine, &dot}) {
            CHECK(std::fwrite(r->items.data(), 4, r->items.size(), f) == r->items.size());
            CHECK(std::fwrite(r->scores.data(), 4, r->scores.size(), f) == r->scores.size());
        }
        std::fclose(f);
        std::printf("queries=%zu k=%zu\n", queries.size(), k);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
