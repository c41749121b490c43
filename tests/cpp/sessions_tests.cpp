// The C++ host layer's session store (sbr::Sessions, include/sbr.hpp), driven from tests/test_sessions_cpp.py: models of 300
// items and max_sequence_length 8 with every parameter block set to seeded random values, 70 sessions with histories of 0..8
// items appended three ways — one item per call, all at once, in ragged splits over shuffled slots — and compared, bit for bit,
// with ImplicitSequenceModel::user_representations of the histories; then Sessions::recommend with each history as the exclusion
// list against ImplicitSequenceModel::recommend of the histories, and Sessions::score_candidates against score_candidates.
//
// Usage: sessions_tests; exit code 0 = assertions held.
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

constexpr std::size_t kItems = 300, kT = 8, kSessions = 70;

// every non-empty parameter block (not the optimiser state) to seeded normal values: gates and biases are non-trivial
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

bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

template <class Model>
void run(const Model& model, const char* name, unsigned seed) {
    std::mt19937 gen(seed);
    randomize(model, gen);
    // histories of 0 .. 8 items, every length present
    std::vector<std::uint64_t> ptr(kSessions + 1, 0);
    std::vector<std::uint32_t> items;
    for (std::size_t u = 0; u < kSessions; ++u) {
        const std::size_t len = u % (kT + 1);
        for (std::size_t t = 0; t < len; ++t) items.push_back((std::uint32_t)(gen() % kItems));
        ptr[u + 1] = items.size();
    }
    const data::CompressedInteractions hist(kSessions, kItems, ptr, items, std::vector<std::uint64_t>(items.size(), 0));
    const std::vector<float> want = model.user_representations(hist);
    std::vector<std::uint32_t> all(kSessions);
    for (std::size_t u = 0; u < kSessions; ++u) all[u] = (std::uint32_t)u;

    Sessions st = model.sessions(kSessions + 3);  // some slots stay unused
    CHECK(st.capacity() == kSessions + 3);
    // (a) one item per call
    for (std::size_t t = 0; t < kT; ++t) {
        std::vector<std::uint32_t> slots, one;
        for (std::size_t u = 0; u < kSessions; ++u)
            if (ptr[u] + t < ptr[u + 1]) { slots.push_back((std::uint32_t)u); one.push_back(items[ptr[u] + t]); }
        st.append(slots, one);
    }
    CHECK(same_bits(st.representations(all), want));
    const std::vector<std::uint64_t> lens = st.lengths(all);
    for (std::size_t u = 0; u < kSessions; ++u) CHECK(lens[u] == ptr[u + 1] - ptr[u]);
    // (b) all at once
    st.reset(all);
    st.append(all, ptr, items);
    CHECK(same_bits(st.representations(all), want));
    // (c) ragged splits of 0 .. 5 items per call over shuffled slots
    st.reset_all();
    std::vector<std::uint64_t> done(kSessions, 0);
    for (bool more = true; more;) {
        more = false;
        std::vector<std::uint32_t> slots = all, ids;
        std::shuffle(slots.begin(), slots.end(), gen);
        slots.resize(kSessions - 7);  // not every slot in every call
        std::vector<std::uint64_t> p(1, 0);
        for (std::uint32_t u : slots) {
            const std::uint64_t left = ptr[u + 1] - ptr[u] - done[u];
            const std::uint64_t take = std::min<std::uint64_t>(left, gen() % 6);
            for (std::uint64_t j = 0; j < take; ++j) ids.push_back(items[ptr[u] + done[u] + j]);
            done[u] += take;
            p.push_back(ids.size());
        }
        st.append(slots, p, ids);
        for (std::size_t u = 0; u < kSessions; ++u) more = more || done[u] < ptr[u + 1] - ptr[u];
    }
    CHECK(same_bits(st.representations(all), want));
    {  // checkpoint into another store, reversed slot order
        const bool lstm = model.hparams().model != SBR_MODEL_EWMA;
        const std::vector<std::uint32_t> back(all.rbegin(), all.rend());
        Sessions other = model.sessions(kSessions);
        other.set_state(back, st.get_state(back, lstm));
        CHECK(same_bits(other.representations(all), want) && other.lengths(all) == st.lengths(all));
    }

    // the scans read the store in place: recommend with each history excluded = recommend of the histories
    for (std::size_t k : {std::size_t(1), std::size_t(10)}) {
        const models::Recommendations a = st.recommend(all, k, ptr, items).unwrap();
        const models::Recommendations b = model.recommend(hist, k).unwrap();
        CHECK(a.items == b.items && same_bits(a.scores, b.scores));
    }
    std::vector<std::uint32_t> rev(all.rbegin(), all.rend());  // a slot order that is not ascending, nothing excluded
    const models::Recommendations r = st.recommend(rev, 10).unwrap();
    const models::Recommendations f = model.recommend(hist, 10, false).unwrap();
    for (std::size_t u = 0; u < kSessions; ++u)
        for (std::size_t x = 0; x < 10; ++x) {
            CHECK(r.items[u * 10 + x] == f.items[(kSessions - 1 - u) * 10 + x]);
            CHECK(std::memcmp(&r.scores[u * 10 + x], &f.scores[(kSessions - 1 - u) * 10 + x], 4) == 0);
        }
    std::vector<std::uint64_t> cptr(kSessions + 1, 0);
    std::vector<std::uint32_t> cand;
    for (std::size_t u = 0; u < kSessions; ++u) {
        for (std::size_t j = 0; j < u % 4; ++j) cand.push_back((std::uint32_t)(gen() % kItems));
        cptr[u + 1] = cand.size();
    }
    CHECK(same_bits(st.score_candidates(all, cptr, cand).unwrap(), model.score_candidates(hist, cptr, cand).unwrap()));
    std::printf("%s: sessions=%zu items=%zu ok\n", name, kSessions, items.size());
}

}  // namespace

int main() {
    try {
        std::array<std::uint8_t, 16> seed;
        seed.fill(7);
        auto normal = models::lstm::Hyperparameters::new_(kItems, kT).embedding_dim(48).lstm_variant(models::lstm::LSTMVariant::Normal).from_seed(seed).build();
        run(normal, "lstm normal d=48", 1);
        auto coupled = models::lstm::Hyperparameters::new_(kItems, kT).embedding_dim(128).lstm_variant(models::lstm::LSTMVariant::Coupled).from_seed(seed).build();
        run(coupled, "lstm coupled d=128", 2);
        auto ewma = models::ewma::Hyperparameters::new_(kItems, kT).embedding_dim(20).from_seed(seed).build();
        run(ewma, "ewma d=20", 3);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
