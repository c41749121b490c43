// The C++ host layer's threshold calls (ImplicitSequenceModel::recommend_above / recommend_above_reps / audience_above /
// audience_above_reps, Sessions::recommend_above / audience_above and their count forms, over the sbr_*_above entry points, and
// models::Above), driven from tests/test_above_cpp.py: the reference protocol's MovieLens split (seed [42;16], user_based_split 0.2),
// an LSTM as built from that rng (not fitted: the harness builds the same model), tags[i] = (i * 2654435761) & 0x8000FFFF, and for
// the test users' histories, with t[u] = the k-th score of recommend(k) for user u and the query items 0 .. 11:
//   recommend_above        t, the history excluded, any_of[u] = 1 << (u % 5), both orders
//   recommend_above_reps   on user_representations of the histories, t, the histories as exclusion lists, both orders
//   audience_above         the queries against the histories, one threshold (the median of t) for all, both orders
//   audience_above_reps    the same over the representations, thresholds t[j], nothing excluded, id order
//   Sessions::recommend_above / audience_above  on a store with remember = 8 that holds the same histories, score order
// Each result goes to a binary file — rows, total, ptr, ids, scores — that the harness compares with the Python calls on the same
// model.  Here: the score order is the id order sorted (score descending, ties to the lower id), the first k entries of a row are
// recommend(k)'s row, the count forms give the pointers, and a max_results below the total is an EngineError that names the total.
//
// Usage: above_tests <movielens csv> <k> <out file>; exit code 0 = assertions held.
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

static std::uint32_t bits(float x) {
    std::uint32_t b;
    std::memcpy(&b, &x, 4);
    return b;
}

// the same set in both orders: every row of `by_score` is the row of `by_id` sorted by (score descending, id ascending)
static void check_orders(const models::Above& by_score, const models::Above& by_id) {
    CHECK(by_score.order == models::AboveOrder::Score && by_id.order == models::AboveOrder::Id);
    CHECK(by_score.ptr == by_id.ptr && by_score.ids.size() == by_id.ids.size() && by_id.ids.size() == by_id.total());
    models::Above again = by_id;
    again.sort_by_score();
    CHECK(again.ids == by_score.ids);
    for (std::size_t e = 0; e < again.scores.size(); ++e) CHECK(bits(again.scores[e]) == bits(by_score.scores[e]));
    for (std::size_t r = 0; r < by_id.rows(); ++r)
        for (std::uint64_t e = by_id.ptr[r]; e + 1 < by_id.ptr[r + 1]; ++e) {
            CHECK(by_id.ids[e] < by_id.ids[e + 1]);
            CHECK(by_score.scores[e] > by_score.scores[e + 1] || (by_score.scores[e] == by_score.scores[e + 1] && by_score.ids[e] < by_score.ids[e + 1]));
        }
}

static void dump(std::FILE* f, const models::Above& a) {
    const std::uint64_t head[2] = {(std::uint64_t)a.rows(), a.total()};
    CHECK(std::fwrite(head, 8, 2, f) == 2);
    CHECK(std::fwrite(a.ptr.data(), 8, a.ptr.size(), f) == a.ptr.size());
    CHECK(std::fwrite(a.ids.data(), 4, a.ids.size(), f) == a.ids.size());
    CHECK(std::fwrite(a.scores.data(), 4, a.scores.size(), f) == a.scores.size());
}

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s <movielens csv> <k> <out file>\n", argv[0]);
        return 2;
    }
    const std::size_t k = (std::size_t)std::stoul(argv[2]);
    try {
        // models::Above needs no model: a hand-made CSR in id order, ties and signed zeros
        models::Above hand;
        hand.ptr = {0, 5, 5, 8};
        hand.ids = {2, 3, 7, 9, 11, 1, 4, 6};
        hand.scores = {1.0f, 2.0f, 1.0f, -0.0f, 0.0f, 0.5f, 0.5f, 3.0f};
        hand.order = models::AboveOrder::Id;
        hand.sort_by_score();
        CHECK((hand.ids == std::vector<std::uint32_t>{3, 2, 7, 9, 11, 6, 1, 4}) && std::signbit(hand.scores[3]) && !std::signbit(hand.scores[4]));
        CHECK(hand.rows() == 3 && hand.count(0) == 5 && hand.count(1) == 0 && hand.total() == 8);

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
        const models::Recommendations top = model.recommend(te, k).unwrap();
        std::vector<float> t(users);
        for (std::size_t u = 0; u < users; ++u) t[u] = top.scores[u * k + k - 1];
        std::vector<float> sorted_t = t;
        std::sort(sorted_t.begin(), sorted_t.end());
        const std::vector<float> mid = {sorted_t[users / 2]};
        std::vector<ItemId> queries;
        for (std::size_t j = 0; j < 12; ++j) queries.push_back((ItemId)j);
        using models::AboveOrder;

        // bad arguments: a NaN threshold, a wrong number of thresholds, masks before any tags
        CHECK(refused([&] { (void)model.recommend_above(te, {std::numeric_limits<float>::quiet_NaN()}); }));
        CHECK(refused([&] { (void)model.recommend_above(te, {1.0f, 2.0f}); }));
        CHECK(refused([&] { (void)model.recommend_above(te, t, true, per_user); }));
        std::vector<std::uint32_t> tags(items);
        for (std::size_t i = 0; i < items; ++i) tags[i] = ((std::uint32_t)i * 2654435761u) & 0x8000FFFFu;
        model.set_item_tags(tags);

        // the first k entries of a row in score order are recommend(k)'s row, bit for bit
        const models::Above plain = model.recommend_above(te, t).unwrap();
        for (std::size_t u = 0; u < users; ++u) {
            CHECK(plain.count(u) >= k);
            for (std::size_t j = 0; j < k; ++j) {
                CHECK(plain.ids[plain.ptr[u] + j] == top.items[u * k + j]);
                CHECK(bits(plain.scores[plain.ptr[u] + j]) == bits(top.scores[u * k + j]));
            }
        }
        CHECK(model.count_above(te, t).unwrap().ptr == plain.ptr && model.count_above(te, t).unwrap().ids.empty());
        bool named_total = false;
        try {
            (void)model.recommend_above(te, t, true, {}, plain.total() - 1);
        } catch (const EngineError& e) {
            named_total = e.status == SBR_ERR_INVALID_ARGUMENT && std::string(e.what()).find(std::to_string(plain.total())) != std::string::npos;
        }
        CHECK(named_total);
        CHECK(model.recommend_above(te, t, true, {}, plain.total()).unwrap().ids == plain.ids);
        const float inf = std::numeric_limits<float>::infinity();
        CHECK(model.recommend_above(te, {inf}).unwrap().total() == 0);
        CHECK(model.count_above(te, {-inf}, false).unwrap().total() == (std::uint64_t)users * items);

        const models::Above a1 = model.recommend_above(te, t, true, per_user).unwrap();
        const models::Above a1i = model.recommend_above(te, t, true, per_user, models::ABOVE_MAX_RESULTS, AboveOrder::Id).unwrap();
        check_orders(a1, a1i);
        const std::vector<float> reps = model.user_representations(te);
        const models::Above a2 = model.recommend_above_reps(reps, t, te.user_pointers(), te.item_ids()).unwrap();
        const models::Above a2i = model.recommend_above_reps(reps, t, te.user_pointers(), te.item_ids(), {}, models::ABOVE_MAX_RESULTS, AboveOrder::Id).unwrap();
        check_orders(a2, a2i);
        CHECK(a2.ptr == plain.ptr && a2.ids == plain.ids);  // the histories as lists are the histories excluded
        CHECK(model.count_above_reps(reps, t, te.user_pointers(), te.item_ids()).unwrap().ptr == a2.ptr);
        const models::Above a3 = model.audience_above(te, queries, mid).unwrap();
        const models::Above a3i = model.audience_above(te, queries, mid, true, models::ABOVE_MAX_RESULTS, AboveOrder::Id).unwrap();
        check_orders(a3, a3i);
        CHECK(model.count_audience_above(te, queries, mid).unwrap().ptr == a3.ptr);
        const std::vector<float> tq(t.begin(), t.begin() + (std::ptrdiff_t)queries.size());
        const models::Above a4 = model.audience_above_reps(reps, queries, tq, {}, {}, models::ABOVE_MAX_RESULTS, AboveOrder::Id).unwrap();
        CHECK(model.count_audience_above_reps(reps, queries, tq).unwrap().ptr == a4.ptr && a4.rows() == queries.size());

        std::vector<std::uint32_t> slots(users);
        for (std::size_t u = 0; u < users; ++u) slots[u] = (std::uint32_t)u;
        Sessions st = model.sessions(users, 8);
        st.append(slots, te.user_pointers(), te.item_ids());
        const models::Above a5 = st.recommend_above(slots, t).unwrap();
        CHECK(st.count_above(slots, t).unwrap().ptr == a5.ptr);
        const models::Above a5_all = st.recommend_above(slots, t, {}, {}, {}, true).unwrap();
        CHECK(a5_all.total() > a5.total());  // the memory excluded something that passes
        std::vector<std::uint32_t> q32(queries.begin(), queries.end());
        const models::Above a6 = st.audience_above(q32, mid).unwrap();
        CHECK(st.count_audience_above(q32, mid).unwrap().ptr == a6.ptr && a6.rows() == q32.size());

        std::FILE* f = std::fopen(argv[3], "wb");
        CHECK(f);
        for (const models::Above* a : {&a1, &a1i, &a2, &a2i, &a3, &a3i, &a4, &a5, &a6}) dump(f, *a);
        std::fclose(f);
        std::printf("users=%zu items=%zu k=%zu pairs=%" PRIu64 "\n", users, items, k, plain.total());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
