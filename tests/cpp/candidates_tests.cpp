// The C++ host layer's recommend-within-a-subset and batched candidate scoring (ImplicitSequenceModel::recommend with `among`,
// score_candidates, user_representations), driven from tests/test_candidates_cpp.py: the reference protocol's MovieLens split
// (seed [42;16], user_based_split 0.2), an LSTM fitted on the train part, then for the train histories the k best among every
// seventh item and the scores of items 0..99 for the first 50 users.  The items and score bits go to a binary file the harness
// compares with the Python calls on the same model.
//
// Usage: candidates_tests <movielens csv> <k> <out file>; exit code 0 = assertions held.
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
        const std::size_t nu = tr.num_users();
        CHECK(nu >= 50 && data.num_items() >= 100);
        std::vector<ItemId> among;
        for (std::size_t i = 0; i < data.num_items(); i += 7) among.push_back((ItemId)i);
        const models::Recommendations rec = model.recommend(tr, k, true, among).unwrap();
        CHECK(rec.num_users == nu && rec.k == k && rec.items.size() == nu * k && rec.scores.size() == rec.items.size());
        for (std::size_t u = 0; u < nu; ++u)
            for (std::size_t x = 0; x < k; ++x) {
                const std::uint32_t it = rec.items[u * k + x];
                CHECK(it == 0xFFFFFFFFu || it % 7 == 0);
                if (x) CHECK(rec.scores[u * k + x - 1] >= rec.scores[u * k + x]);
            }
        // an empty set: rows of padding
        const models::Recommendations none = model.recommend(tr, k, true, {}).unwrap();
        for (std::size_t e = 0; e < none.items.size(); ++e) CHECK(none.items[e] == 0xFFFFFFFFu && std::isinf(none.scores[e]) && none.scores[e] < 0);
        // items 0..99 for the first 50 users, nothing for the others
        std::vector<std::uint64_t> cand_ptr(nu + 1);
        std::vector<std::uint32_t> cand_items;
        for (std::size_t u = 0; u < nu; ++u) {
            cand_ptr[u] = cand_items.size();
            if (u < 50)
                for (std::uint32_t i = 0; i < 100; ++i) cand_items.push_back(i);
        }
        cand_ptr[nu] = cand_items.size();
        const std::vector<float> scores = model.score_candidates(tr, cand_ptr, cand_items).unwrap();
        CHECK(scores.size() == 50 * 100);
        // the batched representations are the single calls'
        const std::vector<float> reps = model.user_representations(tr);
        const std::size_t d = model.hparams().embedding_dim;
        CHECK(reps.size() == nu * d);
        for (std::size_t u : {std::size_t(0), std::size_t(49), nu - 1}) {
            const auto& ptr = tr.user_pointers();
            std::vector<ItemId> h(tr.item_ids().begin() + ptr[u], tr.item_ids().begin() + ptr[u + 1]);
            const models::ImplicitUser one = model.user_representation(h).unwrap();
            CHECK(std::memcmp(one.user_embedding.data(), reps.data() + u * d, d * 4) == 0);
        }
        std::FILE* f = std::fopen(argv[3], "wb");
        CHECK(f);
        CHECK(std::fwrite(rec.items.data(), 4, rec.items.size(), f) == rec.items.size());
        CHECK(std::fwrite(rec.scores.data(), 4, rec.scores.size(), f) == rec.scores.size());
        CHECK(std::fwrite(scores.data(), 4, scores.size(), f) == scores.size());
        std::fclose(f);
        std::printf("users=%zu among=%zu k=%zu\n", nu, among.size(), k);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
