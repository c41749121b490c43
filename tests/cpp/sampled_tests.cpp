// The C++ host layer's sampling calls (ImplicitSequenceModel::recommend_sampled / recommend_sampled_reps and
// Sessions::recommend_sampled, over the sbr_*_sampled entry points), driven from tests/test_sampled_cpp.py: the reference protocol's
// MovieLens split (seed [42;16], user_based_split 0.2), an LSTM as built from that rng (not fitted: the harness builds the same
// model), tags[i] = (i * 2654435761) & 0x8000FFFF, and for every test user's history
//   recommend_sampled        T = 0.75, seed 7, default streams, the history excluded, any_of[u] = 1 << (u % 5)
//   recommend_sampled_reps   on user_representations of the histories, T = 2, seed 8, streams[u] = 1000003 u + (1 << 40), the
//                            histories as exclusion lists, no filter
//   Sessions::recommend_sampled  on a store with remember = 8 that holds the same histories, T = 1, seed 9, default streams (the
//                            slot ids), nothing excluded but what the store remembers
// The items, score bits and key bits of the three go to a binary file the harness compares with the Python calls on the same model.
//
// Usage: sampled_tests <movielens csv> <k> <out file>; exit code 0 = assertions held.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
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

template <class F>
static bool refused(F&& call) {
    try {
        call();
    } catch (const EngineError& e) {
        return e.status == SBR_ERR_INVALID_ARGUMENT;
    }
    return false;
}

static bool same(const models::SampledRecommendations& a, const models::SampledRecommendations& b) {
    return a.items == b.items && a.scores.size() == b.scores.size() && a.keys.size() == b.keys.size() &&
           std::memcmp(a.scores.data(), b.scores.data(), 4 * a.scores.size()) == 0 &&
           std::memcmp(a.keys.data(), b.keys.data(), 4 * a.keys.size()) == 0;
}

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
        const data::CompressedInteractions te = test.to_compressed();
        auto model = models::lstm::Hyperparameters::new_(data.num_items(), 32).embedding_dim(32).rng(rng).build();
        const std::size_t items = data.num_items(), users = te.num_users();
        models::TagFilter per_user;
        for (std::size_t u = 0; u < users; ++u) per_user.any_of.push_back(1u << (u % 5));
        models::SampleArgs a;
        a.temperature = 0.75f;
        a.seed = 7;
        // bad arguments: the temperature, k, the number of streams, masks before any tags
        for (float t : {0.0f, -1.0f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), 1e-39f}) {
            models::SampleArgs bad = a;
            bad.temperature = t;
            CHECK(refused([&] { (void)model.recommend_sampled(te, k, bad); }));
        }
        CHECK(refused([&] { (void)model.recommend_sampled(te, 0, a); }));
        CHECK(refused([&] { (void)model.recommend_sampled(te, SBR_RECOMMEND_MAX_K + 1, a); }));
        models::SampleArgs short_streams = a;
        short_streams.streams.assign(users - 1, 0);
        CHECK(refused([&] { (void)model.recommend_sampled(te, k, short_streams); }));
        CHECK(refused([&] { (void)model.recommend_sampled(te, k, a, true, per_user); }));
        std::vector<std::uint32_t> tags(items);
        for (std::size_t i = 0; i < items; ++i) tags[i] = ((std::uint32_t)i * 2654435761u) & 0x8000FFFFu;
        model.set_item_tags(tags);

        const models::SampledRecommendations rec = model.recommend_sampled(te, k, a, true, per_user).unwrap();
        CHECK(rec.num_users == users && rec.k == k && rec.items.size() == users * k && rec.scores.size() == users * k && rec.keys.size() == users * k);
        CHECK(same(rec, model.recommend_sampled(te, k, a, true, per_user).unwrap()));  // the same (seed, streams): the same bits
        models::SampleArgs other = a;
        other.seed = 70;
        CHECK(!same(rec, model.recommend_sampled(te, k, other, true, per_user).unwrap()));
        for (std::size_t u = 0; u < users; ++u)
            for (std::size_t x = 0; x < k; ++x) {
                const std::uint32_t i = rec.items[u * k + x];
                if (i == 0xFFFFFFFFu) {
                    CHECK(std::isinf(rec.keys[u * k + x]) && std::isinf(rec.scores[u * k + x]));
                    continue;
                }
                CHECK((tags[i] & per_user.any_of[u]) != 0);
                CHECK(x == 0 || rec.keys[u * k + x] <= rec.keys[u * k + x - 1]);
            }

        const std::vector<float> reps = model.user_representations(te);
        models::SampleArgs b;
        b.temperature = 2.0f;
        b.seed = 8;
        for (std::size_t u = 0; u < users; ++u) b.streams.push_back(1000003ull * u + (1ull << 40));
        const models::SampledRecommendations by_reps = model.recommend_sampled_reps(reps, k, b, te.user_pointers(), te.item_ids()).unwrap();
        CHECK(by_reps.items.size() == users * k);

        std::vector<std::uint32_t> slots(users);
        for (std::size_t u = 0; u < users; ++u) slots[u] = (std::uint32_t)u;
        Sessions st = model.sessions(users, 8);
        st.append(slots, te.user_pointers(), te.item_ids());
        models::SampleArgs c;
        c.temperature = 1.0f;
        c.seed = 9;
        const models::SampledRecommendations sess = st.recommend_sampled(slots, k, c).unwrap();
        models::SampleArgs c_explicit = c;
        for (std::size_t u = 0; u < users; ++u) c_explicit.streams.push_back(u);
        CHECK(same(sess, st.recommend_sampled(slots, k, c_explicit).unwrap()));  // the default stream is the slot id
        CHECK(!same(sess, st.recommend_sampled(slots, k, c, {}, {}, {}, true).unwrap()));  // the memory excluded something

        std::FILE* f = std::fopen(argv[3], "wb");
        CHECK(f);
        for (const models::SampledRecommendations* r : {&rec, &by_reps, &sess}) {
            CHECK(std::fwrite(r->items.data(), 4, r->items.size(), f) == r->items.size());
            CHECK(std::fwrite(r->scores.data(), 4, r->scores.size(), f) == r->scores.size());
            CHECK(std::fwrite(r->keys.data(), 4, r->keys.size(), f) == r->keys.size());
        }
        std::fclose(f);
        std::printf("users=%zu items=%zu k=%zu\n", users, items, k);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
