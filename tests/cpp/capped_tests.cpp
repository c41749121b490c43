// The C++ host layer's capped top-k (ImplicitSequenceModel::recommend_capped over sbr_recommend_capped, and Sessions::recommend_capped),
// driven from tests/test_capped_cpp.py: the reference protocol's MovieLens split (seed [42;16], user_based_split 0.2), an LSTM fitted on
// the train part, then for every test user's history
//   A  groups = id % 400, cap 2, k = 10 from a pool of 256: the pool settles every row, no completion;
//   B  one large group (every id that is no multiple of 10) and every other item alone, cap 1, k from a pool of 32: the pool settles
//      no row, first as the library returns it (exact = false), then finished through recommend_top, then the same from a session
//      store that holds the histories.
// Items, score bits and flags of the four go to a binary file the harness compares with the Python calls on the same model.
//
// Usage: capped_tests <movielens csv> <k> <out file>; exit code 0 = assertions held.
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
        const std::size_t ni = data.num_items();
        std::vector<std::uint32_t> ga(ni), gb(ni);
        for (std::size_t i = 0; i < ni; ++i) {
            ga[i] = (std::uint32_t)(i % 400);
            gb[i] = i % 10 ? 0u : (std::uint32_t)i;
        }
        bool threw = false; /* no groups yet */
        try {
            (void)model.recommend_capped(te, k);
        } catch (const EngineError&) {
            threw = true;
        }
        CHECK(threw);
        model.set_item_groups(ga);
        CHECK(model.item_groups() == ga);
        models::CapArgs ca;
        ca.cap = 2; ca.pool = 256; ca.exact = false;
        const models::CappedRecommendations a = model.recommend_capped(te, 10, ca).unwrap();
        CHECK(a.num_users == te.num_users() && a.k == 10 && a.items.size() == a.num_users * 10 && a.complete.size() == a.num_users);
        for (std::uint8_t c : a.complete) CHECK(c == 1);
        // cap >= k is recommend
        ca.cap = (std::uint32_t)k; ca.pool = 0;
        const models::CappedRecommendations same = model.recommend_capped(te, k, ca).unwrap();
        const models::Recommendations plain = model.recommend(te, k).unwrap();
        CHECK(same.items == plain.items && std::memcmp(same.scores.data(), plain.scores.data(), 4 * plain.scores.size()) == 0);
        model.set_item_groups(gb);
        models::CapArgs cb;
        cb.cap = 1; cb.pool = 32; cb.exact = false;
        const models::CappedRecommendations b0 = model.recommend_capped(te, k, cb).unwrap();
        cb.exact = true;
        const models::CappedRecommendations b1 = model.recommend_capped(te, k, cb).unwrap();
        std::size_t short_rows = 0;
        for (std::size_t u = 0; u < b0.num_users; ++u) {
            short_rows += b0.complete[u] ? 0 : 1;
            CHECK(b1.complete[u] == 1);
            std::size_t big = 0; /* the finished row: b0's entries lead it, and the large group appears once at the most */
            for (std::size_t x = 0; x < k; ++x) {
                const std::uint32_t id = b1.items[u * k + x];
                if (b0.items[u * k + x] != 0xFFFFFFFFu) CHECK(b0.items[u * k + x] == id);
                if (id != 0xFFFFFFFFu && gb[id] == 0) ++big;
            }
            CHECK(big <= 1);
        }
        CHECK(short_rows > 0);
        // a session store that holds the test histories
        std::vector<std::uint32_t> slots(te.num_users());
        for (std::size_t u = 0; u < slots.size(); ++u) slots[u] = (std::uint32_t)u;
        Sessions st = model.sessions(slots.size());
        st.append(slots, te.user_pointers(), te.item_ids());
        const models::CappedRecommendations sess = st.recommend_capped(slots, k, cb, gb, {}, te.user_pointers(), te.item_ids()).unwrap();
        for (models::CapArgs bad : {models::CapArgs{0, 0, true}, models::CapArgs{1, (std::uint32_t)k - 1, true}, models::CapArgs{1, 1025, true}}) {
            threw = false;
            try {
                (void)model.recommend_capped(te, k, bad);
            } catch (const EngineError&) {
                threw = true;
            }
            CHECK(threw || (bad.cap == 1 && bad.pool == 0)); /* k = 1: pool k - 1 names the default */
        }
        std::FILE* f = std::fopen(argv[3], "wb");
        CHECK(f);
        for (const models::CappedRecommendations* r : {&a, &b0, &b1, &sess}) {
            CHECK(std::fwrite(r->items.data(), 4, r->items.size(), f) == r->items.size());
            CHECK(std::fwrite(r->scores.data(), 4, r->scores.size(), f) == r->scores.size());
            CHECK(std::fwrite(r->complete.data(), 1, r->complete.size(), f) == r->complete.size());
        }
        std::fclose(f);
        std::printf("users=%zu k=%zu short_rows=%zu\n", b0.num_users, k, short_rows);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
