// The C++ host layer's partition calls (ImplicitSequenceModel::log_partition / log_partition_reps and Sessions::log_partition, over
// the sbr_*log_partition* entry points, and models::Partition over sbr_softmax_weights), driven from tests/test_partition_cpp.py: the
// reference protocol's MovieLens split (seed [42;16], user_based_split 0.2), an LSTM as built from that rng (not fitted: the harness
// builds the same model), tags[i] = (i * 2654435761) & 0x8000FFFF, and for every test user's history
//   log_partition        T = 0.75, the history excluded, any_of[u] = 1 << (u % 5)
//   log_partition_reps   on user_representations of the histories, T = 2, the histories as exclusion lists, no filter
//   Sessions::log_partition  on a store with remember = 8 that holds the same histories, T = 1, nothing excluded but what the
//                        store remembers
// and, beside each, recommend_sampled with the same arguments (seeds 7, 8, 9).  Per call the shifts' bits, the masses, and
// Partition::slate_log_prob of the draws' scores go to a binary file the harness compares with the Python calls on the same model.
//
// Usage: partition_tests <movielens csv> <k> <out file>; exit code 0 = assertions held.
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

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s <movielens csv> <k> <out file>\n", argv[0]);
        return 2;
    }
    const std::size_t k = (std::size_t)std::stoul(argv[2]);
    try {
        // the host helpers need no model
        CHECK(sbr_softmax_frac_bits(1) == 40 && sbr_softmax_frac_bits(1u << 23) == 39 && sbr_softmax_frac_bits(0xFFFFFFFFu) == 31);
        models::Partition hand;
        hand.frac_bits = 40;
        hand.shift = {0.0f};
        hand.mass = {3ull << 40};
        const std::vector<double> lp = hand.slate_log_prob({0.0f, 0.0f, 0.0f, 0.0f, -std::numeric_limits<float>::infinity()});
        CHECK(std::fabs(lp[0] - std::log(1.0 / 3.0)) < 1e-12 && std::fabs(lp[1] - std::log(0.5)) < 1e-12 && lp[2] == 0.0);
        CHECK(std::isnan(lp[3]) && std::isnan(lp[4]));  // the mass is used up; padding
        CHECK(std::fabs(hand.log_z()[0] - std::log(3.0)) < 1e-12 && std::isinf(hand.log_prob({-100.0f})[0]));

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
        // bad arguments: the temperature, masks before any tags
        for (float t : {0.0f, -1.0f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), 1e-39f})
            CHECK(refused([&] { (void)model.log_partition(te, t); }));
        CHECK(refused([&] { (void)model.log_partition(te, 1.0f, true, per_user); }));
        std::vector<std::uint32_t> tags(items);
        for (std::size_t i = 0; i < items; ++i) tags[i] = ((std::uint32_t)i * 2654435761u) & 0x8000FFFFu;
        model.set_item_tags(tags);

        models::SampleArgs a;
        a.temperature = 0.75f;
        a.seed = 7;
        const models::Partition p1 = model.log_partition(te, 0.75f, true, per_user).unwrap();
        const models::SampledRecommendations d1 = model.recommend_sampled(te, k, a, true, per_user).unwrap();
        CHECK(p1.num_users() == users && p1.mass.size() == users && p1.frac_bits == sbr_softmax_frac_bits((std::uint32_t)items));
        const std::vector<double> z1 = p1.log_z();
        for (std::size_t u = 0; u < users; ++u) CHECK(p1.mass[u] >= (1ull << p1.frac_bits) && std::isfinite(z1[u]) && z1[u] >= (double)p1.shift[u]);

        const std::vector<float> reps = model.user_representations(te);
        models::SampleArgs b;
        b.temperature = 2.0f;
        b.seed = 8;
        const models::Partition p2 = model.log_partition_reps(reps, 2.0f, te.user_pointers(), te.item_ids()).unwrap();
        const models::SampledRecommendations d2 = model.recommend_sampled_reps(reps, k, b, te.user_pointers(), te.item_ids()).unwrap();

        std::vector<std::uint32_t> slots(users);
        for (std::size_t u = 0; u < users; ++u) slots[u] = (std::uint32_t)u;
        Sessions st = model.sessions(users, 8);
        st.append(slots, te.user_pointers(), te.item_ids());
        models::SampleArgs c;
        c.temperature = 1.0f;
        c.seed = 9;
        const models::Partition p3 = st.log_partition(slots, 1.0f).unwrap();
        const models::SampledRecommendations d3 = st.recommend_sampled(slots, k, c).unwrap();
        const models::Partition p3_all = st.log_partition(slots, 1.0f, {}, {}, {}, true).unwrap();
        bool grew = false;
        for (std::size_t u = 0; u < users; ++u) {
            CHECK(p3_all.shift[u] > p3.shift[u] || (p3_all.shift[u] == p3.shift[u] && p3_all.mass[u] >= p3.mass[u]));
            grew = grew || p3_all.mass[u] != p3.mass[u] || p3_all.shift[u] != p3.shift[u];
        }
        CHECK(grew);  // the memory excluded something

        std::FILE* f = std::fopen(argv[3], "wb");
        CHECK(f);
        const models::Partition* parts[3] = {&p1, &p2, &p3};
        const models::SampledRecommendations* draws[3] = {&d1, &d2, &d3};
        for (int j = 0; j < 3; ++j) {
            const std::vector<double> slate = parts[j]->slate_log_prob(draws[j]->scores);
            CHECK(slate.size() == users * k);
            for (std::size_t e = 0; e < slate.size(); ++e) CHECK(std::isnan(slate[e]) || slate[e] <= 0.0);
            CHECK(std::fwrite(parts[j]->shift.data(), 4, users, f) == users);
            CHECK(std::fwrite(parts[j]->mass.data(), 8, users, f) == users);
            CHECK(std::fwrite(slate.data(), 8, slate.size(), f) == slate.size());
        }
        std::fclose(f);
        std::printf("users=%zu items=%zu k=%zu frac_bits=%u\n", users, items, k, p1.frac_bits);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
