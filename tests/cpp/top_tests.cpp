// The C++ host layer's budget calls (ImplicitSequenceModel::recommend_top / recommend_top_reps / audience_top / audience_top_reps,
// Sessions::recommend_top / audience_top, over the sbr_*_top entry points, and models::Above::cuts), driven from
// tests/test_top_cpp.py: the reference protocol's MovieLens split (seed [42;16], user_based_split 0.2), an LSTM as built from that
// rng (not fitted: the harness builds the same model), tags[i] = (i * 2654435761) & 0x8000FFFF, and for the test users' histories,
// with n[u] = 1 + 37 u (most of them past the 1 024 a top-k call stops at, the last ones past the catalogue) and the query items
// 0 .. 11:
//   recommend_top        n, the history excluded, any_of[u] = 1 << (u % 5), both orders
//   recommend_top_reps   on user_representations of the histories, n, the histories as exclusion lists, both orders
//   audience_top         the queries against the histories, one budget (1 500) for all, both orders
//   audience_top_reps    the same over the representations, budgets 5 j, nothing excluded, id order
//   Sessions::recommend_top / audience_top  on a store with remember = 8 that holds the same histories, score order
// Each result goes to a binary file — rows, total, ptr, ids, scores, cuts — that the harness compares with the Python calls on the
// same model.  Here: the score order is the id order sorted, a row at n = k is recommend(k)'s row, a row is the first n of
// recommend_above at its cut, count_only gives the cuts and the pointers without pairs, and a max_results below the total is an
// EngineError that names the total.
//
// Usage: top_tests <movielens csv> <k> <out file>; exit code 0 = assertions held.
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

// the same rows in both orders, and the cuts: the last score of a full row, -inf for a short one, +inf for an empty budget
static void check_orders(const models::Above& by_score, const models::Above& by_id, const std::vector<std::uint64_t>& n) {
    CHECK(by_score.order == models::AboveOrder::Score && by_id.order == models::AboveOrder::Id);
    CHECK(by_score.ptr == by_id.ptr && by_score.ids.size() == by_id.ids.size() && by_id.ids.size() == by_id.total());
    CHECK(by_score.cuts.size() == by_score.rows() && by_id.cuts.size() == by_id.rows());
    models::Above again = by_id;
    again.sort_by_score();
    CHECK(again.ids == by_score.ids);
    for (std::size_t e = 0; e < again.scores.size(); ++e) CHECK(bits(again.scores[e]) == bits(by_score.scores[e]));
    for (std::size_t r = 0; r < by_id.rows(); ++r) {
        const std::uint64_t want = n.size() == 1 ? n[0] : n[r];
        CHECK(by_id.count(r) <= want && bits(by_id.cuts[r]) == bits(by_score.cuts[r]));
        if (want == 0) CHECK(by_score.cuts[r] == std::numeric_limits<float>::infinity());
        else if (by_score.count(r) < want) CHECK(by_score.cuts[r] == -std::numeric_limits<float>::infinity());
        else CHECK(by_score.cuts[r] == by_score.scores[by_score.ptr[r + 1] - 1]);
        for (std::uint64_t e = by_id.ptr[r]; e + 1 < by_id.ptr[r + 1]; ++e) {
            CHECK(by_id.ids[e] < by_id.ids[e + 1]);
            CHECK(by_score.scores[e] > by_score.scores[e + 1] || (by_score.scores[e] == by_score.scores[e + 1] && by_score.ids[e] < by_score.ids[e + 1]));
        }
    }
}

static void dump(std::FILE* f, const models::Above& a) {
    const std::uint64_t head[2] = {(std::uint64_t)a.rows(), a.total()};
    CHECK(a.cuts.size() == a.rows());
    CHECK(std::fwrite(head, 8, 2, f) == 2);
    CHECK(std::fwrite(a.ptr.data(), 8, a.ptr.size(), f) == a.ptr.size());
    CHECK(std::fwrite(a.ids.data(), 4, a.ids.size(), f) == a.ids.size());
    CHECK(std::fwrite(a.scores.data(), 4, a.scores.size(), f) == a.scores.size());
    CHECK(std::fwrite(a.cuts.data(), 4, a.cuts.size(), f) == a.cuts.size());
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
        std::vector<std::uint64_t> n(users);
        for (std::size_t u = 0; u < users; ++u) n[u] = 1 + 37 * (std::uint64_t)u;
        CHECK(n[users - 1] > items && n[users / 2] > SBR_RECOMMEND_MAX_K);
        std::vector<ItemId> queries;
        for (std::size_t j = 0; j < 12; ++j) queries.push_back((ItemId)j);
        using models::AboveOrder;

        // bad arguments: a wrong number of budgets, masks before any tags
        CHECK(refused([&] { (void)model.recommend_top(te, {1, 2}); }));
        CHECK(refused([&] { (void)model.recommend_top(te, n, true, per_user); }));
        std::vector<std::uint32_t> tags(items);
        for (std::size_t i = 0; i < items; ++i) tags[i] = ((std::uint32_t)i * 2654435761u) & 0x8000FFFFu;
        model.set_item_tags(tags);

        // n = k for all: recommend(k)'s rows, bit for bit, and the cut is the k-th score
        const models::Recommendations top = model.recommend(te, k).unwrap();
        const models::Above at_k = model.recommend_top(te, {(std::uint64_t)k}).unwrap();
        CHECK(at_k.total() == (std::uint64_t)users * k);
        for (std::size_t u = 0; u < users; ++u) {
            CHECK(at_k.count(u) == k && at_k.cuts[u] == top.scores[u * k + k - 1]);
            for (std::size_t j = 0; j < k; ++j) {
                CHECK(at_k.ids[at_k.ptr[u] + j] == top.items[u * k + j]);
                CHECK(bits(at_k.scores[at_k.ptr[u] + j]) == bits(top.scores[u * k + j]));
            }
        }
        // per-row budgets: each row is the first n of recommend_above at its cut
        const models::Above plain = model.recommend_top(te, n).unwrap();
        const models::Above over = model.recommend_above(te, plain.cuts).unwrap();
        for (std::size_t u = 0; u < users; ++u) {
            CHECK(over.count(u) >= plain.count(u) && plain.count(u) <= n[u]);
            for (std::uint64_t j = 0; j < plain.count(u); ++j) {
                CHECK(plain.ids[plain.ptr[u] + j] == over.ids[over.ptr[u] + j]);
                CHECK(bits(plain.scores[plain.ptr[u] + j]) == bits(over.scores[over.ptr[u] + j]));
            }
        }
        const models::Above select_only = model.recommend_top(te, n, true, {}, 0, AboveOrder::Id, true).unwrap();
        CHECK(select_only.ptr == plain.ptr && select_only.ids.empty() && select_only.cuts.size() == users);
        for (std::size_t u = 0; u < users; ++u) CHECK(bits(select_only.cuts[u]) == bits(plain.cuts[u]));
        bool named_total = false;
        try {
            (void)model.recommend_top(te, n, true, {}, plain.total() - 1);
        } catch (const EngineError& e) {
            named_total = e.status == SBR_ERR_INVALID_ARGUMENT && std::string(e.what()).find(std::to_string(plain.total())) != std::string::npos;
        }
        CHECK(named_total);
        CHECK(model.recommend_top(te, n, true, {}, plain.total()).unwrap().ids == plain.ids);
        CHECK(model.recommend_top(te, {0}).unwrap().total() == 0);
        CHECK(model.recommend_top(te, {(std::uint64_t)items + 5}, false).unwrap().total() == (std::uint64_t)users * items);

        const models::Above a1 = model.recommend_top(te, n, true, per_user).unwrap();
        const models::Above a1i = model.recommend_top(te, n, true, per_user, models::ABOVE_MAX_RESULTS, AboveOrder::Id).unwrap();
        check_orders(a1, a1i, n);
        const std::vector<float> reps = model.user_representations(te);
        const models::Above a2 = model.recommend_top_reps(reps, n, te.user_pointers(), te.item_ids()).unwrap();
        const models::Above a2i = model.recommend_top_reps(reps, n, te.user_pointers(), te.item_ids(), {}, models::ABOVE_MAX_RESULTS, AboveOrder::Id).unwrap();
        check_orders(a2, a2i, n);
        CHECK(a2.ptr == plain.ptr && a2.ids == plain.ids);  // the histories as lists are the histories excluded
        const std::vector<std::uint64_t> reach = {1500};
        const models::Above a3 = model.audience_top(te, queries, reach).unwrap();
        const models::Above a3i = model.audience_top(te, queries, reach, true, models::ABOVE_MAX_RESULTS, AboveOrder::Id).unwrap();
        check_orders(a3, a3i, reach);
        std::vector<std::uint64_t> nq;
        for (std::size_t j = 0; j < queries.size(); ++j) nq.push_back(5 * j);
        const models::Above a4 = model.audience_top_reps(reps, queries, nq, {}, {}, models::ABOVE_MAX_RESULTS, AboveOrder::Id).unwrap();
        CHECK(a4.rows() == queries.size() && a4.count(0) == 0 && a4.count(11) == 55);

        std::vector<std::uint32_t> slots(users);
        for (std::size_t u = 0; u < users; ++u) slots[u] = (std::uint32_t)u;
        Sessions st = model.sessions(users, 8);
        st.append(slots, te.user_pointers(), te.item_ids());
        const models::Above a5 = st.recommend_top(slots, n).unwrap();
        const models::Above a5_all = st.recommend_top(slots, n, {}, {}, {}, true).unwrap();
        CHECK(a5.cuts.size() == users && a5_all.total() >= a5.total());
        std::vector<std::uint32_t> q32(queries.begin(), queries.end());
        const models::Above a6 = st.audience_top(q32, reach).unwrap();
        CHECK(a6.rows() == q32.size() && a6.cuts.size() == q32.size());

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
