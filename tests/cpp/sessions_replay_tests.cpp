// Replay of the C++ host layer's session store (sbr::Sessions::replay, include/sbr.hpp), driven from
// tests/test_sessions_replay_cpp.py: models of 300 items and max_sequence_length 8 with every parameter block set to seeded random
// values; a store of 70 slots that remember 8 items, its slots chosen out of order to hold 0, 1, 7, 8, 9 and 29 items (the last in
// three calls: the ring wraps more than once), one slot with a state and no memory (set_state only), one with a memory and no
// state (set_seen only).  After every parameter block is set anew the store must refuse lengths and recommend; replay() must
// return the number of slots with a memory, leave seen() as it was, and leave every slot with the bits — state, length,
// recommend — of a new store after append of what seen() returned.
//
// Usage: sessions_replay_tests; exit code 0 = assertions held.
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

constexpr std::size_t kItems = 300, kT = 8, kSlots = 70, kSeen = 8;
constexpr std::uint32_t kStateOnly = 50, kSeenOnly = 12;

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

template <class F>
bool refuses(F&& call) {
    try { call(); } catch (const EngineError&) { return true; }
    return false;
}

template <class Model>
void run(const Model& model, const char* name, unsigned seed) {
    std::mt19937 gen(seed);
    randomize(model, gen);
    const bool lstm = model.hparams().model != SBR_MODEL_EWMA;
    std::vector<std::uint32_t> all(kSlots);
    for (std::size_t u = 0; u < kSlots; ++u) all[u] = (std::uint32_t)u;
    const std::pair<std::uint32_t, std::size_t> told[] = {{63, 0}, {5, 1}, {41, kSeen - 1}, {2, kSeen}, {17, kSeen + 1}, {33, 3 * kSeen + 5}};

    Sessions st = model.sessions(kSlots, kSeen);
    for (const auto& [slot, n] : told) {
        const std::size_t calls = n > kSeen + 1 ? 3 : 1;
        for (std::size_t c = 0; c < calls; ++c) {
            const std::size_t a = n * c / calls, b = n * (c + 1) / calls;
            std::vector<std::uint32_t> ids;
            for (std::size_t t = a; t < b; ++t) ids.push_back((std::uint32_t)(gen() % kItems));
            st.append(std::vector<std::uint32_t>{slot}, std::vector<std::uint64_t>{0, ids.size()}, ids.empty() ? std::vector<std::uint32_t>{0} : ids);
        }
    }
    {
        auto donor = st.get_state({2u}, lstm);
        donor.len[0] = 3;
        st.set_state({kStateOnly}, donor);
        st.set_seen({kSeenOnly}, std::vector<std::uint64_t>{0, 4}, std::vector<std::uint32_t>{7, 8, 9, 7});
    }
    const Sessions::Seen before = st.seen(all);
    std::size_t with_memory = 0;
    for (std::size_t u = 0; u < kSlots; ++u) with_memory += before.ptr[u + 1] > before.ptr[u];
    CHECK(with_memory == 6);
    CHECK(before.ptr[34] - before.ptr[33] == kSeen && before.ptr[18] - before.ptr[17] == kSeen);

    randomize(model, gen);  // the store goes stale
    CHECK(refuses([&] { (void)st.lengths(all); }));
    CHECK(refuses([&] { (void)st.recommend(all, 10); }));
    CHECK(refuses([&] { (void)st.replay({33u, 41u}); }));  // the subset form needs a current store
    CHECK(st.replay() == with_memory);

    const Sessions::Seen after = st.seen(all);
    CHECK(after.ptr == before.ptr && after.items == before.items);
    const std::vector<std::uint64_t> len = st.lengths(all);
    for (std::size_t u = 0; u < kSlots; ++u) CHECK(len[u] == before.ptr[u + 1] - before.ptr[u]);

    Sessions fresh = model.sessions(kSlots, kSeen);
    fresh.append(all, before.ptr, before.items.empty() ? std::vector<std::uint32_t>{0} : before.items);
    const auto a = st.get_state(all, lstm), b = fresh.get_state(all, lstm);
    CHECK(same_bits(a.h, b.h) && a.len == b.len);
    if (lstm) CHECK(same_bits(a.c, b.c));
    CHECK(same_bits(st.representations(all), fresh.representations(all)));
    CHECK(same_bits(st.representations({kStateOnly}), fresh.representations({63u})));  // emptied: the empty-history row
    CHECK(len[kStateOnly] == 0);
    CHECK(same(st.recommend(all, 10).unwrap(), fresh.recommend(all, 10).unwrap()));

    // the subset form on the now current store: a slot named twice counts once, the result is the same store
    CHECK(st.replay({33u, 41u, 33u}) == 2);
    const auto c = st.get_state(all, lstm);
    CHECK(same_bits(c.h, b.h) && c.len == b.len);

    {  // a store without memory has nothing to replay from
        Sessions plain = model.sessions(4);
        CHECK(refuses([&] { (void)plain.replay(); }));
    }
    std::printf("%s: slots=%zu replayed=%zu replay ok\n", name, kSlots, with_memory);
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
