// The C++ host layer's tag filter (ImplicitSequenceModel::set_item_tags recommend_filtered, recommend_diverse_filtered,
// similar_items_filtered and the Sessions forms, over the sbr_*_filtered entry points), driven from tests/test_filtered_cpp.py: the reference
// protocol's MovieLens split (seed [42;16], user_based_split 0.2), an LSTM as built from that rng (not fitted: the filter does not
// care, and the harness builds the same model), tags[i] = (i * 2654435761) & 0x8000FFFF, and for every test user's history
//   recommend          any_of[u] = 1 << (u % 5), none_of[u] = 0x80000000 for every third user
//   recommend_diverse  pool 64, dot product, trade_off 0.7, the history kept, one any_of mask (0x00F0) for every user
//   similar_items      of items 0 .. 49, cosine, any_of[j] = the query's own tag word ("the same category")
//   Sessions::recommend  on a store that holds the same histories, the histories excluded, recommend's masks
// The items and score bits of the four go to a binary file the harness compares with the Python calls on the same model.
//
// Usage: filtered_tests <movielens csv> <k> <out file>; exit code 0 = assertions held.
#include <cinttypes>
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

template <class F>
static bool refused(F&& call) {
    try {
        call();
    } catch (const EngineError& e) {
        return e.status == SBR_ERR_INVALID_ARGUMENT;
    }
    return false;
}

static bool same(const models::Recommendations& a, const models::Recommendations& b) {
    return a.items == b.items && a.scores.size() == b.scores.size() && std::memcmp(a.scores.data(), b.scores.data(), 4 * a.scores.size()) == 0;
}

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
        const data::CompressedInteractions te = test.to_compressed();
        auto model = models::lstm::Hyperparameters::new_(data.num_items(), 32).embedding_dim(32).rng(rng).build();
        const std::size_t items = data.num_items(), users = te.num_users();
        models::TagFilter per_user;
        for (std::size_t u = 0; u < users; ++u) {
            per_user.any_of.push_back(1u << (u % 5));
            per_user.none_of.push_back(u % 3 == 0 ? 0x80000000u : 0u);
        }
        // no tags yet: the filtered forms are refused, the plain ones are not
        CHECK(refused([&] { (void)model.recommend_filtered(te, k, true, per_user); }));
        CHECK(refused([&] { (void)model.item_tags(); }));
        const models::Recommendations plain = model.recommend(te, k).unwrap();
        std::vector<std::uint32_t> tags(items);
        for (std::size_t i = 0; i < items; ++i) tags[i] = ((std::uint32_t)i * 2654435761u) & 0x8000FFFFu;
        CHECK(refused([&] { model.set_item_tags(std::vector<std::uint32_t>(items - 1)); }));
        model.set_item_tags(tags);
        CHECK(model.item_tags() == tags);
        CHECK(same(model.recommend(te, k).unwrap(), plain));
        CHECK(same(model.recommend_filtered(te, k, true, models::TagFilter{}).unwrap(), plain));  // all-zero masks filter nothing
        CHECK(refused([&] { (void)model.recommend_filtered(te, k, true, models::TagFilter{{1u, 2u}, {}}); }));  // neither one mask nor one per user

        const models::Recommendations rec = model.recommend_filtered(te, k, true, per_user).unwrap();
        CHECK(rec.num_users == users && rec.k == k && rec.items.size() == users * k && rec.scores.size() == rec.items.size());
        CHECK(!same(rec, plain));
        for (std::size_t u = 0; u < users; ++u)
            for (std::size_t x = 0; x < k; ++x) {
                const std::uint32_t i = rec.items[u * k + x];
                if (i == 0xFFFFFFFFu) continue;
                CHECK((tags[i] & per_user.none_of[u]) == 0 && (tags[i] & per_user.any_of[u]) != 0);
            }
        const models::TagFilter one_mask{{0x00F0u}, {}};
        const models::Recommendations div = model.recommend_diverse_filtered(te, k, pool, 0.7f, models::Similarity::Dot, false, one_mask).unwrap();
        const models::Recommendations div_one = model.recommend_diverse_filtered(te, k, pool, 1.0f, models::Similarity::Dot, false, one_mask).unwrap();
        CHECK(same(div_one, model.recommend_filtered(te, k, false, one_mask).unwrap()));  // trade_off 1 is the filtered recommend
        std::vector<ItemId> queries;
        models::TagFilter category;
        for (std::size_t j = 0; j < 50; ++j) {
            queries.push_back((ItemId)j);
            category.any_of.push_back(tags[j]);
        }
        const models::Recommendations sim = model.similar_items_filtered(queries, k, models::Similarity::Cosine, false, category).unwrap();
        for (std::size_t j = 0; j < queries.size(); ++j)
            for (std::size_t x = 0; x < k; ++x) {
                const std::uint32_t i = sim.items[j * k + x];
                CHECK(i == 0xFFFFFFFFu || (i != j && (tags[j] == 0 || (tags[i] & tags[j]) != 0)));
            }
        std::vector<std::uint32_t> slots(users);
        for (std::size_t u = 0; u < users; ++u) slots[u] = (std::uint32_t)u;
        Sessions st = model.sessions(users);
        st.append(slots, te.user_pointers(), te.item_ids());
        const models::Recommendations sess = st.recommend_filtered(slots, k, per_user, te.user_pointers(), te.item_ids()).unwrap();
        const models::Recommendations sess_div = st.recommend_diverse_filtered(slots, k, pool, 1.0f, models::Similarity::Cosine, per_user, te.user_pointers(), te.item_ids()).unwrap();
        CHECK(same(sess_div, sess));
        model.clear_item_tags();
        CHECK(refused([&] { (void)st.recommend_filtered(slots, k, per_user); }));
        CHECK(same(model.recommend(te, k).unwrap(), plain));
        std::FILE* f = std::fopen(argv[3], "wb");
        CHECK(f);
        for (const models::Recommendations* r : {&rec, &div, &sim, &sess}) {
            CHECK(std::fwrite(r->items.data(), 4, r->items.size(), f) == r->items.size());
            CHECK(std::fwrite(r->scores.data(), 4, r->scores.size(), f) == r->scores.size());
        }
        std::fclose(f);
        std::printf("users=%zu items=%zu k=%zu pool=%zu\n", users, items, k, pool);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
