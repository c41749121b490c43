// Rollout and beam search within an item set through the C++ host layer (sbr::ItemSet::OnSessions::rollout / beam_search and
// sbr::ItemSet::rollout / beam_search over histories, include/sbr.hpp), driven from tests/test_item_set_rollout_cpp.py: an LSTM
// (d = 48) and an EWMA model (d = 20) of 300 items, max_sequence_length 8, every parameter block set to seeded random values, 40
// sessions with histories of 0..7 items, a set of every third item and a few others.  The OnSessions methods must return what the C
// entry points sbr_item_set_rollout / sbr_item_set_beam_search return for the same arguments, bit for bit, and that must equal the
// store's own call with every item outside the set appended to each row's exclusion list; the histories forms must equal their
// defining sequence of calls.
//
// Usage: item_set_rollout_tests; exit code 0 = assertions held.
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

constexpr std::size_t kItems = 300, kT = 8, kSessions = 40, kSteps = 5, kWidth = 4;

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

bool same(const models::Beams& a, const models::Beams& b) {
    return a.num_rows == b.num_rows && a.width == b.width && a.steps == b.steps && a.items == b.items && a.lengths == b.lengths &&
           a.beams == b.beams && same_bits(a.scores, b.scores) && same_bits(a.step_lp, b.step_lp) && same_bits(a.cum, b.cum) &&
           same_bits(a.partition.shift, b.partition.shift) && a.partition.mass == b.partition.mass && a.partition.frac_bits == b.partition.frac_bits;
}

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

/// each row's list with every item outside the set appended
void with_complement(const std::vector<std::uint64_t>& ptr, const std::vector<std::uint32_t>& items, const std::vector<std::uint32_t>& set,
                     std::vector<std::uint64_t>* out_ptr, std::vector<std::uint32_t>* out_items) {
    std::vector<std::uint32_t> comp;
    for (std::uint32_t i = 0; i < kItems; ++i)
        if (!std::binary_search(set.begin(), set.end(), i)) comp.push_back(i);
    out_ptr->assign(1, 0);
    out_items->clear();
    for (std::size_t u = 0; u + 1 < ptr.size(); ++u) {
        out_items->insert(out_items->end(), items.begin() + (std::ptrdiff_t)ptr[u], items.begin() + (std::ptrdiff_t)ptr[u + 1]);
        out_items->insert(out_items->end(), comp.begin(), comp.end());
        out_ptr->push_back(out_items->size());
    }
}

template <class Model>
void run(const Model& model, const char* name, bool lstm, unsigned seed) {
    std::mt19937 gen(seed);
    randomize(model, gen);
    std::vector<std::uint64_t> ptr(kSessions + 1, 0);
    std::vector<std::uint32_t> items;
    for (std::size_t u = 0; u < kSessions; ++u) {
        const std::size_t len = u % kT;
        for (std::size_t t = 0; t < len; ++t) items.push_back((std::uint32_t)(gen() % kItems));
        ptr[u + 1] = items.size();
    }
    const data::CompressedInteractions hist(kSessions, kItems, ptr, items, std::vector<std::uint64_t>(items.size(), 0));
    std::vector<std::uint32_t> all(kSessions), ids;
    for (std::size_t u = 0; u < kSessions; ++u) all[u] = (std::uint32_t)u;
    for (std::uint32_t i = 0; i < kItems; ++i)
        if (i % 3 == 0 || i == 50 || i == 52 || i == 299) ids.push_back(i);
    // caller lists: row 1 is left with three set items, row 2 with none
    std::vector<std::uint64_t> eptr(1, 0);
    std::vector<std::uint32_t> eitems;
    for (std::size_t u = 0; u < kSessions; ++u) {
        for (std::uint32_t i = 0; i < kItems; ++i) {
            const bool bar = u == 1 ? i > 6 : u == 2 ? true : gen() % 40 == 0;
            if (bar) eitems.push_back(i);
        }
        eptr.push_back(eitems.size());
    }
    std::vector<std::uint64_t> cptr;
    std::vector<std::uint32_t> citems;
    with_complement(eptr, eitems, ids, &cptr, &citems);

    ItemSet set = model.item_set(ids);
    Sessions st = model.sessions(kSessions + 2);
    st.append(all, ptr, items);
    const auto on = set.on(st);
    for (int mode = 0; mode < 2; ++mode) {  // greedy, then sampled
        models::RolloutArgs a;
        a.steps = kSteps;
        a.sample = mode == 1;
        a.noise.temperature = 0.8f;
        a.noise.seed = 11;
        a.log_prob = true;
        a.final_state = true;
        a.lstm = lstm;
        a.excl_ptr = eptr;
        a.excl_items = eitems;
        const models::Rollout r = on.rollout(all, a).unwrap();
        // the C entry point, same arguments
        models::Rollout c = r;
        std::fill(c.items.begin(), c.items.end(), 7u);
        std::fill(c.scores.begin(), c.scores.end(), 7.0f);
        std::fill(c.keys.begin(), c.keys.end(), 7.0f);
        std::fill(c.h.begin(), c.h.end(), 7.0f);
        std::fill(c.c.begin(), c.c.end(), 7.0f);
        std::fill(c.partition.shift.begin(), c.partition.shift.end(), 7.0f);
        std::fill(c.partition.mass.begin(), c.partition.mass.end(), 7u);
        sbr_rollout_args ra{};
        ra.steps = (std::uint32_t)kSteps;
        ra.flags = a.sample ? SBR_ROLLOUT_SAMPLE : 0u;
        ra.sample.temperature = a.noise.temperature;
        ra.sample.seed = a.noise.seed;
        sbr_scan_rows d{};
        d.store = st.handle();
        d.slots = all.data();
        d.excl_ptr = eptr.data();
        d.excl_items = eitems.data();
        CHECK(sbr_item_set_rollout(set.handle(), &d, kSessions, &ra, c.items.data(), c.scores.data(), a.sample ? c.keys.data() : nullptr,
                                   c.lengths.data(), c.partition.shift.data(), c.partition.mass.data(), &c.partition.frac_bits, c.h.data(),
                                   lstm ? c.c.data() : nullptr) == SBR_OK);
        CHECK(c.items == r.items && same_bits(c.scores, r.scores) && same_bits(c.keys, r.keys) && c.lengths == r.lengths &&
              same_bits(c.partition.shift, r.partition.shift) && c.partition.mass == r.partition.mass &&
              c.partition.frac_bits == r.partition.frac_bits && same_bits(c.h, r.h) && same_bits(c.c, r.c));
        d.flags = SBR_RECOMMEND_INCLUDE_HISTORY;  // include_seen is said in the args, never in the descriptor
        CHECK(sbr_item_set_rollout(set.handle(), &d, kSessions, &ra, c.items.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   nullptr, nullptr) == SBR_ERR_INVALID_ARGUMENT);
        // the complement route
        models::RolloutArgs b = a;
        b.excl_ptr = cptr;
        b.excl_items = citems;
        CHECK(same(r, st.rollout(all, b).unwrap()));
        CHECK(r.lengths[1] == 3 && r.lengths[2] == 0 && r.partition.frac_bits == sbr_softmax_frac_bits((std::uint32_t)kItems));
        for (std::uint32_t x : r.items) CHECK(x == 0xFFFFFFFFu || std::binary_search(ids.begin(), ids.end(), x));
        // the histories form is its defining sequence of calls
        models::RolloutArgs h = a;
        h.excl_ptr.clear();
        h.excl_items.clear();
        const models::Rollout conv = set.rollout(hist, h).unwrap();
        Sessions tmp = model.sessions(kSessions);
        tmp.append(all, ptr, items);  // every history is within max_sequence_length
        h.excl_ptr = ptr;
        h.excl_items = items;
        CHECK(same(conv, set.on(tmp).rollout(all, h).unwrap()));
    }
    models::BeamArgs a;
    a.steps = kSteps;
    a.width = kWidth;
    a.temperature = 0.75f;
    a.partitions = true;
    a.excl_ptr = eptr;
    a.excl_items = eitems;
    const models::Beams r = on.beam_search(all, a).unwrap();
    models::Beams c = r;
    std::fill(c.items.begin(), c.items.end(), 7u);
    std::fill(c.scores.begin(), c.scores.end(), 7.0f);
    std::fill(c.step_lp.begin(), c.step_lp.end(), 7.0f);
    std::fill(c.cum.begin(), c.cum.end(), 7.0f);
    sbr_beam_args ba{};
    ba.steps = (std::uint32_t)kSteps;
    ba.width = (std::uint32_t)kWidth;
    ba.temperature = a.temperature;
    sbr_scan_rows d{};
    d.store = st.handle();
    d.slots = all.data();
    d.excl_ptr = eptr.data();
    d.excl_items = eitems.data();
    CHECK(sbr_item_set_beam_search(set.handle(), &d, kSessions, &ba, c.items.data(), c.scores.data(), c.step_lp.data(), c.cum.data(),
                                   c.lengths.data(), c.beams.data(), c.partition.shift.data(), c.partition.mass.data(), &c.partition.frac_bits) == SBR_OK);
    CHECK(same(r, c));
    models::BeamArgs b = a;
    b.excl_ptr = cptr;
    b.excl_items = citems;
    CHECK(same(r, st.beam_search(all, b).unwrap()));
    CHECK(r.lengths[1] == 3 && r.lengths[2] == 0 && r.beams[1] == kWidth && r.beams[2] == 0);
    for (std::uint32_t x : r.items) CHECK(x == 0xFFFFFFFFu || std::binary_search(ids.begin(), ids.end(), x));
    models::BeamArgs h = a;
    h.excl_ptr.clear();
    h.excl_items.clear();
    const models::Beams conv = set.beam_search(hist, h).unwrap();
    Sessions tmp = model.sessions(kSessions);
    tmp.append(all, ptr, items);
    h.excl_ptr = ptr;
    h.excl_items = items;
    CHECK(same(conv, set.on(tmp).beam_search(all, h).unwrap()));
    {  // refusals of the C++ layer
        bool refused = false;
        models::BeamArgs z;
        z.width = 33;
        try { (void)on.beam_search(all, z); } catch (const EngineError&) { refused = true; }
        CHECK(refused);
        refused = false;
        models::RolloutArgs y;
        y.include_seen = true;  // a store without memory
        try { (void)on.rollout(all, y); } catch (const EngineError&) { refused = true; }
        CHECK(refused);
    }
    std::printf("%s: sessions=%zu set=%zu rollout and beam_search within the set ok\n", name, kSessions, ids.size());
}

}  // namespace

int main() {
    try {
        std::array<std::uint8_t, 16> seed;
        seed.fill(7);
        auto normal = models::lstm::Hyperparameters::new_(kItems, kT).embedding_dim(48).lstm_variant(models::lstm::LSTMVariant::Normal).from_seed(seed).build();
        run(normal, "lstm normal d=48", true, 5);
        auto ewma = models::ewma::Hyperparameters::new_(kItems, kT).embedding_dim(20).from_seed(seed).build();
        run(ewma, "ewma d=20", false, 6);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
