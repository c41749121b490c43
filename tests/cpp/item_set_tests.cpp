// The C++ host layer's item sets (sbr::ItemSet over sbr_item_set_*, from ImplicitSequenceModel::item_set), driven from
// tests/test_item_set_cpp.py: the reference protocol's MovieLens split (seed [42;16], user_based_split 0.2), an LSTM fitted on the
// train part, S = every seventh item.  For every test user's history each family through the set equals, items and bits, the
// model's own call on the user's representation with the history and the complement of S as its exclusion list — recommend (plain
// and under a tag filter), recommend_sampled, log_partition, recommend_above, recommend_top, recommend_capped (device rows and
// finished rows) and recommend_diverse — and on(store) equals the histories form for the slots that hold at most
// min(W, max_sequence_length) items.  The program checks itself.
//
// Usage: item_set_tests <movielens csv> <k>; exit code 0 = assertions held.
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

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), 4 * a.size()) == 0);
}
template <class R>
static bool same_rows(const R& a, const R& b) {
    return a.num_users == b.num_users && a.k == b.k && a.items == b.items && same_bits(a.scores, b.scores);
}
static bool same_above(const models::Above& a, const models::Above& b) {
    return a.ptr == b.ptr && a.ids == b.ids && same_bits(a.scores, b.scores) && same_bits(a.cuts, b.cuts);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <movielens csv> <k>\n", argv[0]);
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
        const std::size_t T = 32, W = 24;
        auto model = models::lstm::Hyperparameters::new_(data.num_items(), T)
                         .embedding_dim(32)
                         .learning_rate(0.16f)
                         .l2_penalty(0.0004f)
                         .loss(models::Loss::WARP)
                         .num_epochs(1)
                         .batch_sequences(64)
                         .rng(rng)
                         .build();
        model.fit(tr).unwrap();
        const std::size_t ni = data.num_items(), n = te.num_users();
        std::vector<std::uint32_t> S, given, tags(ni), groups(ni);
        std::vector<char> in_s(ni, 0);
        for (std::size_t i = 0; i < ni; ++i) {
            tags[i] = (std::uint32_t)(1u << (i % 5));
            groups[i] = i % 10 ? 0u : (std::uint32_t)i; /* one large group, every tenth item alone */
            if (i % 7 == 0) { S.push_back((std::uint32_t)i); in_s[i] = 1; }
        }
        given.assign(S.rbegin(), S.rend()); /* any order, duplicates allowed */
        given.push_back(S[0]);
        model.set_item_tags(tags);
        model.set_item_groups(groups);
        models::ItemSet set = model.item_set(given);
        CHECK(set.size() == S.size() && set.items() == S);
        bool threw = false;
        try {
            (void)model.item_set({(std::uint32_t)ni});
        } catch (const EngineError&) {
            threw = true;
        }
        CHECK(threw);
        // the model's route: representations, with the history and the complement of S excluded
        const std::vector<float> reps = model.user_representations(te);
        std::vector<std::uint64_t> ep(1, 0);
        std::vector<std::uint32_t> ei;
        for (std::size_t u = 0; u < n; ++u) {
            ei.insert(ei.end(), te.item_ids().begin() + (std::ptrdiff_t)te.user_pointers()[u], te.item_ids().begin() + (std::ptrdiff_t)te.user_pointers()[u + 1]);
            for (std::size_t i = 0; i < ni; ++i)
                if (!in_s[i]) ei.push_back((std::uint32_t)i);
            ep.push_back(ei.size());
        }
        models::TagFilter f;
        f.any_of = {0x0Bu};
        f.none_of = {0x10u};
        const std::vector<std::uint32_t> any(n, 0x0Bu), none_of(n, 0x10u);
        // top-k, plain and filtered
        const models::Recommendations a = set.recommend(te, k).unwrap();
        models::Recommendations ref;
        ref.num_users = n; ref.k = k; ref.items.resize(n * k); ref.scores.resize(n * k);
        CHECK(sbr_recommend_reps(model.handle(), reps.data(), n, (std::uint32_t)k, ep.data(), ei.data(), ref.items.data(), ref.scores.data()) == SBR_OK);
        CHECK(same_rows(a, ref));
        for (std::uint32_t id : a.items) CHECK(id == 0xFFFFFFFFu || in_s[id]);
        const models::Recommendations af = set.recommend(te, k, true, f).unwrap();
        CHECK(sbr_recommend_filtered_reps(model.handle(), reps.data(), n, (std::uint32_t)k, ep.data(), ei.data(), any.data(), none_of.data(),
                                          ref.items.data(), ref.scores.data()) == SBR_OK);
        CHECK(same_rows(af, ref) && af.items != a.items);
        CHECK(same_rows(set.recommend_reps(reps, k, ep, ei, f).unwrap(), af));
        // sampled: the same (seed, stream) through the set and through the model
        models::SampleArgs sa;
        sa.temperature = 0.7f; sa.seed = 99;
        for (std::size_t u = 0; u < n; ++u) sa.streams.push_back(1000 + 3 * u);
        const models::SampledRecommendations sm = set.recommend_sampled(te, k, sa).unwrap();
        const models::SampledRecommendations sr = model.recommend_sampled_reps(reps, k, sa, ep, ei).unwrap();
        CHECK(same_rows(sm, sr) && same_bits(sm.keys, sr.keys));
        // log_partition: the model's F, the same integers
        const models::Partition pa = set.log_partition(te, 0.7f, true, f).unwrap();
        const models::Partition pr = model.log_partition_reps(reps, 0.7f, ep, ei, f).unwrap();
        CHECK(pa.frac_bits == pr.frac_bits && pa.mass == pr.mass && same_bits(pa.shift, pr.shift));
        // above at each row's k-th score, and top
        std::vector<float> th(n);
        for (std::size_t u = 0; u < n; ++u) th[u] = a.scores[u * k + k - 1];
        const models::Above ab = set.recommend_above(te, th).unwrap();
        CHECK(same_above(ab, model.recommend_above_reps(reps, th, ep, ei).unwrap()));
        for (std::size_t u = 0; u < n; ++u) CHECK(ab.count(u) >= k && ab.ids[(std::size_t)ab.ptr[u]] == a.items[u * k]);
        CHECK(same_above(set.recommend_above(te, th, true, {}, models::ABOVE_MAX_RESULTS, models::AboveOrder::Id).unwrap(),
                         model.recommend_above_reps(reps, th, ep, ei, {}, models::ABOVE_MAX_RESULTS, models::AboveOrder::Id).unwrap()));
        const models::Above tp = set.recommend_top(te, {37}, true, f).unwrap();
        CHECK(same_above(tp, model.recommend_top_reps(reps, {37}, ep, ei, f).unwrap()) && tp.cuts.size() == n);
        // capped: the device's rows and the finished ones
        models::CapArgs cb;
        cb.cap = 1; cb.pool = 32; cb.exact = false;
        const models::CappedRecommendations c0 = set.recommend_capped(te, k, cb).unwrap();
        const models::CappedRecommendations r0 = model.recommend_capped_reps(reps, k, cb, ep, ei).unwrap();
        CHECK(same_rows(c0, r0) && c0.complete == r0.complete);
        cb.exact = true;
        const models::CappedRecommendations c1 = set.recommend_capped(te, k, cb).unwrap();
        const models::CappedRecommendations r1 = model.recommend_capped_reps(reps, k, cb, ep, ei).unwrap();
        CHECK(same_rows(c1, r1) && c1.complete == r1.complete);
        std::size_t short_rows = 0;
        for (std::size_t u = 0; u < n; ++u) {
            short_rows += c0.complete[u] ? 0 : 1;
            CHECK(c1.complete[u] == 1);
        }
        CHECK(short_rows > 0);
        // diverse
        const models::Recommendations dv = set.recommend_diverse(te, 10, 40, 0.5f).unwrap();
        models::Recommendations dref;
        dref.num_users = n; dref.k = 10; dref.items.resize(n * 10); dref.scores.resize(n * 10);
        CHECK(sbr_recommend_diverse_reps(model.handle(), reps.data(), n, 10, 40, 0.5f, SBR_SIMILAR_COSINE, ep.data(), ei.data(), dref.items.data(),
                                         dref.scores.data()) == SBR_OK);
        CHECK(same_rows(dv, dref));
        CHECK(same_rows(set.recommend_diverse(te, k, 40, 1.0f).unwrap(), set.recommend(set.of(te), k).unwrap()) || k > 40);
        // a store: the slots that hold at most min(W, T) items answer as their histories do
        std::vector<std::uint32_t> slots;
        std::vector<std::size_t> users;
        std::vector<std::uint64_t> sp(1, 0);
        std::vector<std::uint32_t> si;
        for (std::size_t u = 0; u < n; ++u) {
            const std::size_t len = (std::size_t)(te.user_pointers()[u + 1] - te.user_pointers()[u]);
            if (len > std::min(W, T)) continue;
            users.push_back(u);
            slots.push_back((std::uint32_t)slots.size());
            si.insert(si.end(), te.item_ids().begin() + (std::ptrdiff_t)te.user_pointers()[u], te.item_ids().begin() + (std::ptrdiff_t)te.user_pointers()[u + 1]);
            sp.push_back(si.size());
        }
        CHECK(!slots.empty());
        Sessions st = model.sessions(slots.size(), W);
        st.append(slots, sp, si);
        const auto on = set.on(st);
        const models::Recommendations so = on.recommend(slots, k).unwrap();
        const models::SampledRecommendations ss = on.recommend_sampled(slots, k, models::SampleArgs{0.7f, 5, {}}).unwrap();
        models::SampleArgs by_slot{0.7f, 5, {}};
        for (std::uint32_t s : slots) by_slot.streams.push_back(s);
        const ItemSet::Rows hist_rows = set.of(te).take(users);
        const models::SampledRecommendations sh = set.recommend_sampled(hist_rows, k, by_slot).unwrap();
        CHECK(same_rows(ss, sh) && same_bits(ss.keys, sh.keys));
        const models::Partition po = on.log_partition(slots, 0.7f).unwrap(), ph = set.log_partition(hist_rows, 0.7f).unwrap();
        CHECK(po.mass == ph.mass && same_bits(po.shift, ph.shift) && po.frac_bits == ph.frac_bits);
        CHECK(same_above(on.recommend_top(slots, {12}).unwrap(), set.recommend_top(hist_rows, {12}).unwrap()));
        cb.exact = true;
        CHECK(same_rows(on.recommend_capped(slots, k, cb).unwrap(), set.recommend_capped(hist_rows, k, cb).unwrap()));
        for (std::size_t j = 0; j < users.size(); ++j)
            for (std::size_t x = 0; x < k; ++x) {
                CHECK(so.items[j * k + x] == a.items[users[j] * k + x]);
                CHECK(std::memcmp(&so.scores[j * k + x], &a.scores[users[j] * k + x], 4) == 0);
            }
        // stale after a fit, current again after refresh
        model.fit(tr).unwrap();
        threw = false;
        try {
            (void)set.recommend(te, k);
        } catch (const EngineError& e) {
            threw = e.status == SBR_ERR_INVALID_ARGUMENT;
        }
        CHECK(threw);
        set.refresh();
        CHECK(set.recommend(te, k).unwrap().items.size() == n * k);
        std::printf("users=%zu set=%zu store_slots=%zu short_rows=%zu\n", n, S.size(), slots.size(), short_rows);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
