// The C++ host layer's top-k recommendation (ImplicitSequenceModel::recommend over sbr_recommend), driven from
// tests/test_recommend_cpp.py: the reference protocol's MovieLens split (seed [42;16], user_based_split 0.2), an LSTM fitted
// on the train part, then the top k of every test user.  The items and score bits go to a binary file the harness compares
// with the Python call on the same model.
//
// Usage: recommend_tests <movielens csv> <k> <out file>; exit code 0 = assertions held.
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
        const data::CompressedInteractions tr = train.to_compressed(), te = test.to_compressed();
        auto model = models::lstm::Hyperparameters::new_(data.num_items(), 32)
                         .embedding_dim(32)
                         .learning_rate(0.16f)
                         .l2_penalty(0.0004f)
                         .loss(models::Loss::WARP)
                         .num_epochs(2)
                         .batch_sequences(8)
                         .rng(rng)
                         .build();
        model.fit(tr).unwrap();
        const models::Recommendations r = model.recommend(te, k).unwrap();
        CHECK(r.num_users == te.num_users() && r.items.size() == r.num_users * k && r.scores.size() == r.items.size());
        // rows are ordered and hold no history item; the first entry of a user equals predict's score
        for (std::size_t u = 0; u < r.num_users; ++u) {
            const std::uint64_t b = te.user_pointers()[u], e = te.user_pointers()[u + 1];
            for (std::size_t j = 0; j < k; ++j) {
                const std::uint32_t it = r.items[u * k + j];
                if (it == 0xFFFFFFFFu) continue;
                for (std::uint64_t x = b; x < e; ++x) CHECK(te.item_ids()[x] != it);
                if (j) CHECK(r.scores[u * k + j - 1] >= r.scores[u * k + j]);
            }
            if (u < 4 && r.items[u * k] != 0xFFFFFFFFu) {
                std::vector<ItemId> hist(te.item_ids().begin() + b, te.item_ids().begin() + e);
                const auto user = model.user_representation(hist).unwrap();
                const auto s = model.predict(user, {(ItemId)r.items[u * k]}).unwrap();
                std::uint32_t a, c;
                std::memcpy(&a, &s[0], 4);
                std::memcpy(&c, &r.scores[u * k], 4);
                CHECK(a == c);
            }
        }
        std::FILE* f = std::fopen(argv[3], "wb");
        CHECK(f);
        CHECK(std::fwrite(r.items.data(), 4, r.items.size(), f) == r.items.size());
        CHECK(std::fwrite(r.scores.data(), 4, r.scores.size(), f) == r.scores.size());
        std::fclose(f);
        std::printf("users=%zu k=%zu\n", r.num_users, k);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
