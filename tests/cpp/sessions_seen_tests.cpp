// The seen-item memory of the C++ host layer's session store (sbr::Sessions with a seen_capacity, include/sbr.hpp), driven from
// tests/test_sessions_seen_cpp.py: models of 300 items and max_sequence_length 8 with every parameter block set to seeded random
// values, 40 sessions with histories of 0..8 items (drawn from 30 ids, so items repeat) appended three ways — all at once, one item
// per call, in ragged splits — into a store that remembers 8 items per slot.  Sessions::recommend of the store, with no lists
// given, must equal ImplicitSequenceModel::recommend of the histories bit for bit and differ from the call with include_seen;
// Sessions::seen must return the histories; and get_state + seen -> set_state + set_seen into a second store must give the same
// recommend bits.
//
// Usage: sessions_seen_tests; exit code 0 = assertions held.
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

constexpr std::size_t kItems = 300, kT = 8, kSessions = 40, kSeen = 8;

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

bool same(const models::Recommendations& a, const models::Recommendations& b) { return a.items == b.items && same_bits(a.scores, b.scores); }

template <class Model>
void run(const Model& model, const char* name, unsigned seed) {
    std::mt19937 gen(seed);
    randomize(model, gen);
    std::vector<std::uint64_t> ptr(kSessions + 1, 0);
    std::vector<std::uint32_t> items;
    for (std::size_t u = 0; u < kSessions; ++u) {
        const std::size_t len = u % (kT + 1);
        for (std::size_t t = 0; t < len; ++t) items.push_back((std::uint32_t)(gen() % 30));
        ptr[u + 1] = items.size();
    }
    const data::CompressedInteractions hist(kSessions, kItems, ptr, items, std::vector<std::uint64_t>(items.size(), 0));
    std::vector<std::uint32_t> all(kSessions);
    for (std::size_t u = 0; u < kSessions; ++u) all[u] = (std::uint32_t)u;

    for (int way = 0; way < 3; ++way) {
        Sessions st = model.sessions(kSessions + 3, kSeen);
        CHECK(st.capacity() == kSessions + 3 && st.seen_capacity() == kSeen);
        if (way == 0) {
            st.append(all, ptr, items);
        } else if (way == 1) {
            for (std::size_t t = 0; t < kT; ++t) {
                std::vector<std::uint32_t> slots, one;
                for (std::size_t u = 0; u < kSessions; ++u)
                    if (ptr[u] + t < ptr[u + 1]) { slots.push_back((std::uint32_t)u); one.push_back(items[ptr[u] + t]); }
                st.append(slots, one);
            }
        } else {
            std::vector<std::uint64_t> done(kSessions, 0);
            for (bool more = true; more;) {
                more = false;
                std::vector<std::uint32_t> slots = all, ids;
                std::shuffle(slots.begin(), slots.end(), gen);
                slots.resize(kSessions - 7);
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
        }
        // the memory holds the histories, in order, repeats kept
        const Sessions::Seen seen = st.seen(all);
        CHECK(seen.ptr == ptr && seen.items == items);
        // the two oracles
        for (std::size_t k : {std::size_t(1), std::size_t(10)}) {
            const models::Recommendations a = st.recommend(all, k).unwrap();
            CHECK(same(a, model.recommend(hist, k).unwrap()));
            const models::Recommendations free = st.recommend(all, k, {}, {}, true).unwrap();
            CHECK(same(free, model.recommend(hist, k, false).unwrap()));
            if (k == 10) CHECK(a.items != free.items);  // excluding nothing would not pass
        }
        // the round trip: state + seen -> set_state + set_seen, reversed slot order, into a store whose slots had other occupants
        const bool lstm = model.hparams().model != SBR_MODEL_EWMA;
        const std::vector<std::uint32_t> back(all.rbegin(), all.rend());
        Sessions other = model.sessions(kSessions, kSeen);
        other.append(all, std::vector<std::uint32_t>(kSessions, 5u));
        other.set_state(back, st.get_state(back, lstm));
        CHECK(other.seen(all).items.empty());  // set_state empties the memory
        other.set_seen(back, st.seen(back));
        CHECK(same(other.recommend(all, 10).unwrap(), st.recommend(all, 10).unwrap()));
        const Sessions::Seen again = other.seen(all);
        CHECK(again.ptr == ptr && again.items == items);
        st.reset(all);
        CHECK(st.seen(all).items.empty());
    }
    {  // a store without memory refuses include_seen and has no memory to read
        Sessions plain = model.sessions(4);
        CHECK(plain.seen_capacity() == 0);
        bool refused = false;
        try { (void)plain.recommend({0, 1}, 5, {}, {}, true); } catch (const EngineError&) { refused = true; }
        CHECK(refused);
    }
    std::printf("%s: sessions=%zu items=%zu seen ok\n", name, kSessions, items.size());
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
