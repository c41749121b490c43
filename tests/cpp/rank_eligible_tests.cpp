// The C++ host layer's rank_targets under a serving policy (include/sbr.hpp over sbr_rank_targets_rows / sbr_item_set_rank_targets;
// ELIGIBLE RANKS in sbr_hip.h), driven from tests/test_rank_eligible_cpp.py.  A small LSTM over 229 items is fitted for one epoch on
// synthetic sequences; every item carries one of five tag bits and S holds the items with i % 3 != 0.  For 40 histories the C++
// overloads — the model's with a TagFilter, ItemSet::rank_targets, Sessions::rank_targets, ItemSet::on(store).rank_targets — return
// the ranks of the C call the contract names: sbr_rank_targets_reps on the rows' representations with the mask list
// M = history ∪ forbidden ∪ complement of S.  ranking_metrics under a policy skips exactly the targets of rank num_items.
// The program checks itself.
//
// Usage: rank_eligible_tests; exit code 0 = assertions held.
#include <algorithm>
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

int main() {
    try {
        const std::size_t ni = 229, n = 40, T = 16, W = 12;
        std::array<std::uint8_t, 16> seed;
        seed.fill(7);
        XorShiftRng rng = XorShiftRng::from_seed(seed);
        std::uint32_t x = 12345u;
        auto next = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
        std::vector<std::uint64_t> hp(1, 0), tp(1, 0), ts;
        std::vector<std::uint32_t> hi, ti;
        for (std::size_t u = 0; u < n; ++u) {
            for (std::size_t j = 0; j < 3 + u % 10; ++j) hi.push_back(next() % ni);  // at most 12 items: the memory below holds a whole history
            hp.push_back(hi.size());
            for (std::size_t j = 0; j < u % 20; ++j) ti.push_back(next() % ni);  // 0 .. 19 targets: past one scan row's 16
            if (u % 20 > 2) {
                ti[tp.back()] = hi[hp[u]];          // a target in its own history
                ti[tp.back() + 1] = ti[tp.back() + 2];  // a duplicate
            }
            tp.push_back(ti.size());
        }
        ts.assign(hi.size(), 0);
        const data::CompressedInteractions hist(n, ni, hp, hi, ts);
        auto model = models::lstm::Hyperparameters::new_(ni, T).embedding_dim(32).loss(models::Loss::Hinge).num_epochs(1).batch_sequences(8).rng(rng).build();
        model.fit(hist).unwrap();
        std::vector<std::uint32_t> tags(ni), S;
        std::vector<char> in_s(ni, 0);
        for (std::size_t i = 0; i < ni; ++i) {
            tags[i] = (std::uint32_t)(1u << (i % 5));
            if (i % 3) { S.push_back((std::uint32_t)i); in_s[i] = 1; }
        }
        model.set_item_tags(tags);
        models::ItemSet set = model.item_set(S);
        models::TagFilter f;
        f.any_of = {0x0Bu};
        f.none_of = {0x10u};
        auto allowed = [&](std::uint32_t i) { return (tags[i] & 0x10u) == 0 && (tags[i] & 0x0Bu) != 0; };
        // the contract's call: the plain rank_targets_reps with the mask list M
        const std::vector<float> reps = model.user_representations(hist);
        auto reference = [&](bool history, bool filter, bool within) {
            std::vector<std::uint64_t> ep(1, 0);
            std::vector<std::uint32_t> ei;
            for (std::size_t u = 0; u < n; ++u) {
                if (history) ei.insert(ei.end(), hi.begin() + (std::ptrdiff_t)hp[u], hi.begin() + (std::ptrdiff_t)hp[u + 1]);
                for (std::uint32_t i = 0; i < ni; ++i)
                    if ((filter && !allowed(i)) || (within && !in_s[i])) ei.push_back(i);
                ep.push_back(ei.size());
            }
            std::vector<std::uint32_t> ranks(ti.size() + 1), none(1, 0);
            CHECK(sbr_rank_targets_reps(model.handle(), reps.data(), n, ep.data(), ei.empty() ? none.data() : ei.data(), tp.data(), ti.data(),
                                        ranks.data()) == SBR_OK);
            ranks.pop_back();
            return ranks;
        };
        const std::vector<std::uint32_t> plain = model.rank_targets(hist, tp, ti).unwrap();
        CHECK(plain == reference(true, false, false));
        // the model under a filter; an empty filter is the plain call
        const std::vector<std::uint32_t> filtered = model.rank_targets(hist, tp, ti, f).unwrap();
        CHECK(filtered == reference(true, true, false) && filtered != plain);
        CHECK(model.rank_targets(hist, tp, ti, models::TagFilter{}) .unwrap() == plain);
        CHECK(model.rank_targets(hist, tp, ti, f, false).unwrap() == reference(false, true, false));
        // through the set, with and without the filter
        CHECK(set.rank_targets(set.of(hist), tp, ti).unwrap() == reference(true, false, true));
        const std::vector<std::uint32_t> both = set.rank_targets(set.of(hist, true, f), tp, ti).unwrap();
        CHECK(both == reference(true, true, true));
        CHECK(set.rank_targets(set.of_reps(reps, {}, {}, f), tp, ti).unwrap() == reference(false, true, true));
        for (std::size_t e = 0; e < ti.size(); ++e)
            if (!in_s[ti[e]] || !allowed(ti[e])) CHECK(both[e] == ni);
        // a store whose memory holds each whole history: its seen items are the history
        models::Sessions store = model.sessions(n + 3, W);
        std::vector<std::uint32_t> slots(n);
        for (std::size_t u = 0; u < n; ++u) slots[u] = (std::uint32_t)(n + 2 - u);
        store.append(slots, hp, hi);
        CHECK(store.rank_targets(slots, tp, ti).unwrap() == plain);
        CHECK(store.rank_targets(slots, tp, ti, {}, {}, false, f).unwrap() == filtered);
        CHECK(store.rank_targets(slots, tp, ti, {}, {}, true, f).unwrap() == reference(false, true, false));
        CHECK(store.rank_targets(slots, tp, ti, hp, hi, true).unwrap() == plain);  // the caller's lists in the memory's place
        CHECK(set.on(store).rank_targets(slots, tp, ti, {}, {}, false, f).unwrap() == both);
        // refusals: a target id out of range, one target range too few
        bool threw = false;
        std::vector<std::uint32_t> bad = ti;
        bad[3] = (std::uint32_t)ni;
        try {
            (void)model.rank_targets(hist, tp, bad, f);
        } catch (const EngineError&) {
            threw = true;
        }
        CHECK(threw);
        threw = false;
        try {
            (void)set.rank_targets(set.of(hist), std::vector<std::uint64_t>(tp.begin(), tp.end() - 1), ti);
        } catch (const EngineError&) {
            threw = true;
        }
        CHECK(threw);
        // ranking_metrics under the policy: "skip" leaves out exactly the targets the policy can never show
        const std::vector<std::size_t> ks{10, 100};
        evaluation::RankingPolicy policy;
        policy.filter = f;
        policy.item_set = &set;
        std::vector<std::uint32_t> r_miss, r_skip;
        const evaluation::RankingMetrics miss = evaluation::ranking_metrics(model, hist, policy, ks, 2, &r_miss).unwrap();
        policy.ineligible = evaluation::Ineligible::Skip;
        const evaluation::RankingMetrics skip = evaluation::ranking_metrics(model, hist, policy, ks, 2, &r_skip).unwrap();
        CHECK(r_miss == r_skip && miss.targets_skipped == 0);
        CHECK(skip.targets_skipped == (std::size_t)std::count(r_miss.begin(), r_miss.end(), (std::uint32_t)ni) && skip.targets_skipped > 0);
        CHECK(skip.num_users_ranked <= miss.num_users_ranked && skip.mean_rank < miss.mean_rank);
        std::vector<std::uint32_t> r_plain;
        const evaluation::RankingMetrics base = evaluation::ranking_metrics(model, hist, ks, 2, &r_plain).unwrap();
        CHECK(base.targets_skipped == 0 && r_plain.size() == r_miss.size() && r_plain != r_miss);
        std::printf("targets=%zu filtered!=plain skipped=%zu\n", ti.size(), skip.targets_skipped);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
