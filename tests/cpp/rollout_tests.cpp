// The rollout calls of the C++ host layer (sbr::Sessions::rollout and ImplicitSequenceModel::rollout, include/sbr.hpp), driven from
// tests/test_rollout_cpp.py: models of 300 items and max_sequence_length 8 with every parameter block set to seeded random values,
// 40 sessions with histories of 0..11 items.  Sessions::rollout must return what the C entry point sbr_sessions_rollout returns for
// the same arguments, bit for bit, in both modes, with the partition and the final state; its greedy rows must be what the host loop
// of Sessions::recommend(k = 1) + append + a rebuilt exclusion list gives on a second store, whose state the final state then equals;
// the store it ran on must hold every bit it held; and ImplicitSequenceModel::rollout must equal its defining sequence of calls.
//
// Usage: rollout_tests; exit code 0 = assertions held.
#include <algorithm>
#include <cmath>
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

constexpr std::size_t kItems = 300, kT = 8, kSessions = 40, kSteps = 6;

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

template <class T>
bool same_bits(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

bool same(const models::Rollout& a, const models::Rollout& b) {
    return a.num_rows == b.num_rows && a.steps == b.steps && a.items == b.items && a.lengths == b.lengths && same_bits(a.scores, b.scores) &&
           same_bits(a.keys, b.keys) && same_bits(a.partition.shift, b.partition.shift) && a.partition.mass == b.partition.mass &&
           a.partition.frac_bits == b.partition.frac_bits && same_bits(a.log_prob, b.log_prob) && same_bits(a.h, b.h) && same_bits(a.c, b.c) &&
           a.len == b.len;
}

template <class Model>
void run(const Model& model, const char* name, unsigned seed) {
    std::mt19937 gen(seed);
    randomize(model, gen);
    const bool lstm = model.hparams().model != SBR_MODEL_EWMA;
    const std::size_t dim = model.hparams().embedding_dim;
    std::vector<std::uint64_t> ptr(kSessions + 1, 0);
    std::vector<std::uint32_t> items;
    for (std::size_t u = 0; u < kSessions; ++u) {
        const std::size_t len = u % (kT + 4);  // some longer than max_sequence_length
        for (std::size_t t = 0; t < len; ++t) items.push_back((std::uint32_t)(gen() % kItems));
        ptr[u + 1] = items.size();
    }
    const data::CompressedInteractions hist(kSessions, kItems, ptr, items, std::vector<std::uint64_t>(items.size(), 0));
    std::vector<std::uint32_t> all(kSessions);
    for (std::size_t u = 0; u < kSessions; ++u) all[u] = (std::uint32_t)u;
    // caller lists: row 1 is left with three items, row 2 with none
    std::vector<std::uint64_t> eptr(1, 0);
    std::vector<std::uint32_t> eitems;
    for (std::size_t u = 0; u < kSessions; ++u) {
        for (std::uint32_t i = 0; i < kItems; ++i) {
            const bool bar = u == 1 ? i >= 3 : u == 2 ? true : gen() % 40 == 0;
            if (bar) eitems.push_back(i);
        }
        eptr.push_back(eitems.size());
    }

    Sessions st = model.sessions(kSessions + 2);
    st.append(all, ptr, items);
    const Sessions::State before = st.get_state(all, lstm);

    for (int mode = 0; mode < 2; ++mode) {
        models::RolloutArgs a;
        a.steps = kSteps;
        a.sample = mode == 1;
        a.log_prob = a.final_state = true;
        a.lstm = lstm;
        a.noise.temperature = 0.75f;
        a.noise.seed = 0xFFFFFFFFFFFFFFFEull;  // wraps at step 2
        a.excl_ptr = eptr;
        a.excl_items = eitems;
        const models::Rollout r = st.rollout(all, a).unwrap();
        // the C entry point, same arguments
        const std::size_t cells = kSessions * kSteps;
        models::Rollout c;
        c.num_rows = kSessions; c.steps = kSteps;
        c.items.resize(cells); c.scores.resize(cells); c.lengths.resize(kSessions);
        if (a.sample) c.keys.resize(cells);
        c.partition.temperature = a.noise.temperature;
        c.partition.shift.resize(cells); c.partition.mass.resize(cells);
        c.h.resize(kSessions * dim);
        if (lstm) c.c.resize(kSessions * dim);
        sbr_rollout_args ra{};
        ra.steps = (std::uint32_t)kSteps;
        ra.flags = a.sample ? SBR_ROLLOUT_SAMPLE : 0u;
        ra.sample.temperature = a.noise.temperature;
        ra.sample.seed = a.noise.seed;
        ra.sample.streams = nullptr;
        CHECK(sbr_sessions_rollout(st.handle(), all.data(), kSessions, &ra, eptr.data(), eitems.data(), nullptr, nullptr, c.items.data(),
                                   c.scores.data(), a.sample ? c.keys.data() : nullptr, c.lengths.data(), c.partition.shift.data(),
                                   c.partition.mass.data(), &c.partition.frac_bits, c.h.data(), lstm ? c.c.data() : nullptr) == SBR_OK);
        CHECK(r.items == c.items && r.lengths == c.lengths && same_bits(r.scores, c.scores) && same_bits(r.keys, c.keys));
        CHECK(same_bits(r.partition.shift, c.partition.shift) && r.partition.mass == c.partition.mass && r.partition.frac_bits == c.partition.frac_bits);
        CHECK(same_bits(r.h, c.h) && same_bits(r.c, c.c));
        CHECK(r.lengths[1] == 3 && r.lengths[2] == 0 && r.lengths[0] == kSteps);
        for (std::size_t p = 0; p < cells; ++p) {
            const bool pad = p % kSteps >= r.lengths[p / kSteps];
            CHECK(pad == (r.items[p] == 0xFFFFFFFFu) && pad == std::isnan(r.log_prob[p]));
            if (pad) CHECK(std::isinf(r.scores[p]) && std::isinf(r.partition.shift[p]) && r.partition.mass[p] == 0);
            else CHECK(r.log_prob[p] <= 0.0 && (a.sample || r.log_prob[p] > -1e300));
        }
        // nothing was written
        const Sessions::State after = st.get_state(all, lstm);
        CHECK(same_bits(before.h, after.h) && same_bits(before.c, after.c) && before.len == after.len);
        if (mode == 0) {  // the host loop it replaces, on a second store
            Sessions loop = model.sessions(kSessions);
            loop.append(all, ptr, items);
            std::vector<std::vector<std::uint32_t>> barred(kSessions);
            for (std::size_t u = 0; u < kSessions; ++u) barred[u].assign(eitems.begin() + (std::ptrdiff_t)eptr[u], eitems.begin() + (std::ptrdiff_t)eptr[u + 1]);
            for (std::size_t j = 0; j < kSteps; ++j) {
                std::vector<std::uint64_t> lp(1, 0), ap(1, 0);
                std::vector<std::uint32_t> li, ai;
                for (std::size_t u = 0; u < kSessions; ++u) {
                    std::sort(barred[u].begin(), barred[u].end());
                    li.insert(li.end(), barred[u].begin(), barred[u].end());
                    lp.push_back(li.size());
                }
                const models::Recommendations one = loop.recommend(all, 1, lp, li).unwrap();
                for (std::size_t u = 0; u < kSessions; ++u) {
                    const std::size_t p = u * kSteps + j;
                    CHECK(one.items[u] == r.items[p] && std::memcmp(&one.scores[u], &r.scores[p], 4) == 0);
                    if (one.items[u] != 0xFFFFFFFFu) { ai.push_back(one.items[u]); barred[u].push_back(one.items[u]); }
                    ap.push_back(ai.size());
                }
                if (ai.empty()) ai.push_back(0);
                loop.append(all, ap, ai);
            }
            const Sessions::State fin = loop.get_state(all, lstm);
            CHECK(same_bits(fin.h, r.h) && same_bits(fin.c, r.c) && fin.len == r.len);
        }
        // the model-level convenience is its defining sequence of calls
        models::RolloutArgs b = a;
        b.excl_ptr.clear();
        b.excl_items.clear();
        const models::Rollout conv = model.rollout(hist, b).unwrap();
        Sessions tmp = model.sessions(kSessions);
        std::vector<std::uint64_t> tp(1, 0);
        std::vector<std::uint32_t> ti;
        for (std::size_t u = 0; u < kSessions; ++u) {
            const std::uint64_t keep = std::min<std::uint64_t>(ptr[u + 1] - ptr[u], kT);
            ti.insert(ti.end(), items.begin() + (std::ptrdiff_t)(ptr[u + 1] - keep), items.begin() + (std::ptrdiff_t)ptr[u + 1]);
            tp.push_back(ti.size());
        }
        tmp.append(all, tp, ti);
        b.excl_ptr = ptr;
        b.excl_items = items;
        CHECK(same(conv, tmp.rollout(all, b).unwrap()));
        b.excl_ptr.clear();
        b.excl_items.clear();
        CHECK(same(model.rollout(hist, b, false).unwrap(), tmp.rollout(all, b).unwrap()));
    }
    {  // refusals of the C++ layer and of the library
        bool refused = false;
        models::RolloutArgs a;
        a.steps = 0;
        try { (void)st.rollout(all, a); } catch (const EngineError&) { refused = true; }
        CHECK(refused);
        refused = false;
        a.steps = 2;
        a.include_seen = true;  // a store without memory
        try { (void)st.rollout(all, a); } catch (const EngineError&) { refused = true; }
        CHECK(refused);
    }
    std::printf("%s: sessions=%zu steps=%zu rollout ok\n", name, kSessions, kSteps);
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
