// The C++ host layer's diversified top-k (ImplicitSequenceModel::recommend_diverse over sbr_recommend_diverse, and
// Sessions::recommend_diverse), driven from tests/test_diverse_cpp.py: the reference protocol's MovieLens split (seed [42;16],
// user_based_split 0.2), an LSTM fitted on the train part, then k picks from a pool of 64 for every test user's history, by cosine at
// trade_off 0.3 and by dot product at 0.7 with the history kept, and by cosine from a session store that holds the same histories.
// The items and score bits of the three go to a binary file the harness compares with the Python calls on the same model.
//
// Usage: diverse_tests <movielens csv> <k> <out file>; exit code 0 = assertions held.
#include <algorithm>
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
    const std::size_t pool = 64;
    try {
        data::Interactions data = datasets::download_movielens_100k(argv[1]);
        std::array<std::uint8_t, 16> seed;
        seed.fill(42);
        XorShiftRng rng = XorShiftRng::from_seed(seed);
        auto [train, test] = data::user_based_split(data, rng, 0.2f);
        const data::CompressedInteractions tr = train.to_compressed();
        const data::CompressedInteractions te = test.to_compressed();
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
        CHECK(model.diverse_max_pool() == 1024);
        const models::Recommendations cosine = model.recommend_diverse(te, k, pool, 0.3f).unwrap();
        const models::Recommendations dot = model.recommend_diverse(te, k, pool, 0.7f, models::Similarity::Dot, false).unwrap();
        const models::Recommendations plain = model.recommend(te, k).unwrap();
        const models::Recommendations wide = model.recommend(te, pool).unwrap();
        for (const models::Recommendations* r : {&cosine, &dot})
            CHECK(r->num_users == te.num_users() && r->k == k && r->items.size() == r->num_users * k && r->scores.size() == r->items.size());
        for (std::size_t u = 0; u < cosine.num_users; ++u) {
            // the first pick is the best item, and every pick is an entry of the pool with the pool's score bits
            CHECK(cosine.items[u * k] == plain.items[u * k]);
            for (std::size_t x = 0; x < k; ++x) {
                const std::uint32_t* row = &wide.items[u * pool];
                const std::uint32_t* at = std::find(row, row + pool, cosine.items[u * k + x]);
                CHECK(at != row + pool);
                CHECK(std::memcmp(&wide.scores[u * pool + (std::size_t)(at - row)], &cosine.scores[u * k + x], 4) == 0);
            }
        }
        // trade_off 1 is recommend; the default pool is min(4 k, the largest)
        const models::Recommendations one = model.recommend_diverse(te, k, pool, 1.0f).unwrap();
        CHECK(one.items == plain.items && std::memcmp(one.scores.data(), plain.scores.data(), 4 * plain.scores.size()) == 0);
        const models::Recommendations dflt = model.recommend_diverse(te, k).unwrap();
        const models::Recommendations four = model.recommend_diverse(te, k, std::min<std::size_t>(4 * k, 1024)).unwrap();
        CHECK(dflt.items == four.items);
        // a session store that holds the test histories (whole: a session does not truncate to max_sequence_length)
        std::vector<std::uint32_t> slots(te.num_users());
        for (std::size_t u = 0; u < slots.size(); ++u) slots[u] = (std::uint32_t)u;
        Sessions st = model.sessions(slots.size());
        st.append(slots, te.user_pointers(), te.item_ids());
        const models::Recommendations sess = st.recommend_diverse(slots, k, pool, 0.3f, models::Similarity::Cosine, te.user_pointers(), te.item_ids()).unwrap();
        const models::Recommendations sess_one = st.recommend_diverse(slots, k, pool, 1.0f, models::Similarity::Cosine, te.user_pointers(), te.item_ids()).unwrap();
        const models::Recommendations sess_plain = st.recommend(slots, k, te.user_pointers(), te.item_ids()).unwrap();
        CHECK(sess_one.items == sess_plain.items && std::memcmp(sess_one.scores.data(), sess_plain.scores.data(), 4 * sess_plain.scores.size()) == 0);
        for (std::size_t u = 0; u < sess.num_users; ++u) CHECK(sess.items[u * k] == sess_plain.items[u * k]);
        for (std::size_t bad_pool : {k - 1, (std::size_t)(2 * SBR_DIVERSE_MAX_POOL)}) {
            bool threw = false;
            try {
                (void)model.recommend_diverse(te, k, bad_pool);
            } catch (const EngineError&) {
                threw = true;
            }
            CHECK(threw || bad_pool == 0);
        }
        std::FILE* f = std::fopen(argv[3], "wb");
        CHECK(f);
        for (const models::Recommendations* r : {&cosine, &dot, &sess}) {
            CHECK(std::fwrite(r->items.data(), 4, r->items.size(), f) == r->items.size());
            CHECK(std::fwrite(r->scores.data(), 4, r->scores.size(), f) == r->scores.size());
        }
        std::fclose(f);
        std::printf("users=%zu k=%zu pool=%zu\n", cosine.num_users, k, pool);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
