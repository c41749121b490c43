// The audience scan of the C++ host layer (Sessions::audience, ImplicitSequenceModel::audience_reps / audience in include/sbr.hpp),
// driven from tests/test_audience_cpp.py: models of 300 items with every parameter block set to seeded random values, 70 sessions
// with histories of 1..8 items drawn from 30 ids, 40 queries with repeats.  Every facade call must give the rows of the C call it
// wraps, bit for bit: sbr_sessions_audience on a store with and without memory (all live slots, a named subset, caller exclusions,
// include_seen), sbr_audience_reps on the store's representations (where rows are positions), and sbr_audience on the histories;
// and a few rows are checked against ImplicitSequenceModel::predict.
//
// Usage: audience_tests; exit code 0 = assertions held.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
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

namespace {

constexpr std::size_t kItems = 300, kT = 8, kSessions = 70, kSeen = 8, kQueries = 40, kK = 6;

template <class Model>
void randomize(const Model& model, std::mt19937& gen) {
    std::normal_distribution<float> nd(0.0f, 0.4f);
    for (sbr_param which : {SBR_PARAM_ITEM_EMBEDDING, SBR_PARAM_ITEM_BIAS, SBR_PARAM_LSTM_W, SBR_PARAM_LSTM_B, SBR_PARAM_EWMA_ALPHA}) {
        std::uint64_t count = 0;
        CHECK(sbr_model_param_count(model.handle(), which, &count) == SBR_OK);
        if (!count) continue;
        std::vector<float> v(count);
        for (float& x : v) x = nd(gen);
        CHECK(sbr_model_set_param(model.handle(), which, v.data(), count) == SBR_OK);
    }
}

struct Rows {
    std::vector<std::uint32_t> ids;
    std::vector<float> scores;
    explicit Rows(std::size_t n) : ids(n * kK, 7u), scores(n * kK, 7.0f) {}
};

bool same(const models::Recommendations& a, const Rows& b) {
    return a.items == b.ids && a.scores.size() == b.scores.size() && std::memcmp(a.scores.data(), b.scores.data(), a.scores.size() * sizeof(float)) == 0;
}

template <class Model>
void run(const Model& model, const char* name, unsigned seed) {
    std::mt19937 gen(seed);
    randomize(model, gen);
    std::vector<std::uint64_t> ptr(kSessions + 1, 0);
    std::vector<std::uint32_t> items;
    for (std::size_t u = 0; u < kSessions; ++u) {
        const std::size_t len = 1 + u % kT;
        for (std::size_t t = 0; t < len; ++t) items.push_back((std::uint32_t)(gen() % 30));
        ptr[u + 1] = items.size();
    }
    const data::CompressedInteractions hist(kSessions, kItems, ptr, items, std::vector<std::uint64_t>(items.size(), 0));
    std::vector<std::uint32_t> all(kSessions);
    for (std::size_t u = 0; u < kSessions; ++u) all[u] = (std::uint32_t)u;
    std::vector<std::uint32_t> queries(kQueries);
    std::vector<ItemId> query_ids(kQueries);
    for (std::size_t j = 0; j < kQueries; ++j) {
        queries[j] = j < 30 ? (std::uint32_t)(gen() % 30) : (std::uint32_t)(gen() % kItems);
        if (j >= 35) queries[j] = queries[j - 35];
        query_ids[j] = (ItemId)queries[j];
    }
    std::vector<std::uint64_t> eptr(kQueries + 1, 0);
    std::vector<std::uint32_t> eslots;
    for (std::size_t j = 0; j < kQueries; ++j) {
        for (std::size_t e = 0; e < j % 3; ++e) eslots.push_back((std::uint32_t)(gen() % kSessions));
        eptr[j + 1] = eslots.size();
    }
    std::vector<std::uint32_t> subset = all;
    std::shuffle(subset.begin(), subset.end(), gen);
    subset.resize(25);
    subset.push_back((std::uint32_t)kSessions + 1);  // an empty slot

    Sessions plain = model.sessions(kSessions + 3);
    Sessions mem = model.sessions(kSessions + 3, kSeen);
    plain.append(all, ptr, items);
    mem.append(all, ptr, items);
    sbr_model* h = model.handle();
    for (Sessions* st : {&plain, &mem}) {
        Rows c(kQueries);
        CHECK(sbr_sessions_audience(st->handle(), queries.data(), kQueries, kK, nullptr, 0, nullptr, nullptr, 0, c.ids.data(), c.scores.data()) == SBR_OK);
        CHECK(same(st->audience(queries, kK).unwrap(), c));
        CHECK(sbr_sessions_audience(st->handle(), queries.data(), kQueries, kK, subset.data(), subset.size(), eptr.data(), eslots.data(), 0, c.ids.data(),
                                    c.scores.data()) == SBR_OK);
        CHECK(same(st->audience(queries, kK, subset, false, eptr, eslots).unwrap(), c));
        for (std::uint32_t s : c.ids) CHECK(s == 0xFFFFFFFFu || std::find(subset.begin(), subset.end(), s) != subset.end());
    }
    const models::Recommendations with_memory = mem.audience(queries, kK).unwrap();
    const models::Recommendations free = mem.audience(queries, kK, {}, true, {}, {}, true).unwrap();
    const models::Recommendations plain_rows = plain.audience(queries, kK).unwrap();
    CHECK(free.items == plain_rows.items && free.scores == plain_rows.scores);
    CHECK(with_memory.items != free.items);  // the memory excludes something
    bool refused = false;
    try { (void)plain.audience(queries, kK, {}, true, {}, {}, true); } catch (const EngineError&) { refused = true; }
    CHECK(refused);

    // caller-supplied rows: the store's representations, where slot u is row u
    const std::vector<float> reps = plain.representations(all);
    {
        Rows c(kQueries);
        CHECK(sbr_audience_reps(h, reps.data(), kSessions, queries.data(), kQueries, kK, eptr.data(), eslots.data(), c.ids.data(), c.scores.data()) == SBR_OK);
        CHECK(same(model.audience_reps(reps, query_ids, kK, eptr, eslots).unwrap(), c));
        const models::Recommendations r = model.audience_reps(reps, query_ids, kK).unwrap();
        CHECK(r.items == plain_rows.items && r.scores == plain_rows.scores);
        // predict's bits
        for (std::size_t j : {std::size_t(0), kQueries - 1})
            for (std::size_t c2 = 0; c2 < 2; ++c2) {
                const std::uint32_t u = r.items[j * kK + c2];
                models::ImplicitUser user;
                user.user_embedding.assign(reps.begin() + u * (reps.size() / kSessions), reps.begin() + (u + 1) * (reps.size() / kSessions));
                const std::vector<float> p = model.predict(user, {query_ids[j]}).unwrap();
                CHECK(std::memcmp(&p[0], &r.scores[j * kK + c2], sizeof(float)) == 0);
            }
    }
    // the histories
    for (bool exclude_history : {true, false}) {
        Rows c(kQueries);
        CHECK(sbr_audience(h, ptr.data(), items.data(), kSessions, queries.data(), kQueries, kK, exclude_history ? 0u : SBR_RECOMMEND_INCLUDE_HISTORY,
                           c.ids.data(), c.scores.data()) == SBR_OK);
        CHECK(same(model.audience(hist, query_ids, kK, exclude_history).unwrap(), c));
        if (exclude_history) CHECK(same(with_memory, c));  // histories of at most kSeen = kT items: the memory is the history
    }
    std::printf("%s: sessions=%zu queries=%zu audience ok\n", name, kSessions, kQueries);
}

}  // namespace

int main() {
    try {
        std::array<std::uint8_t, 16> seed;
        seed.fill(7);
        auto normal = models::lstm::Hyperparameters::new_(kItems, kT).embedding_dim(48).lstm_variant(models::lstm::LSTMVariant::Normal).from_seed(seed).build();
        run(normal, "lstm normal d=48", 1);
        auto ewma = models::ewma::Hyperparameters::new_(kItems, kT).embedding_dim(20).from_seed(seed).build();
        run(ewma, "ewma d=20", 3);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
