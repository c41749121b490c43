// The beam-search calls of the C++ host layer (sbr::Sessions::beam_search and ImplicitSequenceModel::beam_search, include/sbr.hpp),
// driven from tests/test_beam_cpp.py: an LSTM of 300 items, max_sequence_length 8 and d = 48 with every parameter block set to seeded
// random values, 40 sessions with histories of 0..11 items, W = 4, 5 steps.  Sessions::beam_search must return what the C entry point
// sbr_sessions_beam_search returns for the same arguments, bit for bit; the store it ran on must hold every bit it held; and
// ImplicitSequenceModel::beam_search must equal its defining sequence of calls.  The program then writes the model's parameters, the
// histories, the exclusion lists and its result as raw little-endian arrays into the directory named by its argument, so that the
// Python test can hold the Python binding's result to them.
//
// Usage: beam_tests OUT_DIR; exit code 0 = assertions held.
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

bool same(const models::Beams& a, const models::Beams& b) {
    return a.num_rows == b.num_rows && a.width == b.width && a.steps == b.steps && a.items == b.items && a.lengths == b.lengths &&
           a.beams == b.beams && same_bits(a.scores, b.scores) && same_bits(a.step_lp, b.step_lp) && same_bits(a.cum, b.cum) &&
           same_bits(a.partition.shift, b.partition.shift) && a.partition.mass == b.partition.mass && a.partition.frac_bits == b.partition.frac_bits;
}

template <class T>
void dump(const std::string& dir, const char* name, const std::vector<T>& v) {
    const std::string path = dir + "/" + name;
    std::FILE* f = std::fopen(path.c_str(), "wb");
    CHECK(f != nullptr);
    if (!v.empty()) CHECK(std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size());
    std::fclose(f);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: beam_tests OUT_DIR\n");
        return 2;
    }
    const std::string out = argv[1];
    try {
        std::array<std::uint8_t, 16> seed;
        seed.fill(7);
        auto model = models::lstm::Hyperparameters::new_(kItems, kT).embedding_dim(48).lstm_variant(models::lstm::LSTMVariant::Normal).from_seed(seed).build();
        std::mt19937 gen(5);
        std::normal_distribution<float> nd(0.0f, 0.4f);
        for (sbr_param which : {SBR_PARAM_ITEM_EMBEDDING, SBR_PARAM_ITEM_BIAS, SBR_PARAM_LSTM_W, SBR_PARAM_LSTM_B}) {
            std::uint64_t count = 0;
            CHECK(sbr_model_param_count(model.handle(), which, &count) == SBR_OK);
            std::vector<float> v(count);
            for (float& x : v) x = nd(gen);
            CHECK(sbr_model_set_param(model.handle(), which, v.data(), count) == SBR_OK);
            std::vector<float> back(count);
            CHECK(sbr_model_get_param(model.handle(), which, back.data(), count) == SBR_OK);
            dump(out, which == SBR_PARAM_ITEM_EMBEDDING ? "E.f32" : which == SBR_PARAM_ITEM_BIAS ? "b.f32" : which == SBR_PARAM_LSTM_W ? "W.f32" : "B.f32", back);
        }
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
        const Sessions::State before = st.get_state(all, true);
        models::BeamArgs a;
        a.steps = kSteps;
        a.width = kWidth;
        a.temperature = 0.75f;
        a.partitions = true;
        a.excl_ptr = eptr;
        a.excl_items = eitems;
        const models::Beams r = st.beam_search(all, a).unwrap();
        // the C entry point, same arguments
        const std::size_t cells = kSessions * kWidth * kSteps;
        models::Beams c;
        c.num_rows = kSessions; c.width = kWidth; c.steps = kSteps;
        c.items.resize(cells); c.scores.resize(cells); c.step_lp.resize(cells); c.cum.resize(kSessions * kWidth);
        c.lengths.resize(kSessions); c.beams.resize(kSessions);
        c.partition.temperature = a.temperature;
        c.partition.shift.resize(cells); c.partition.mass.resize(cells);
        sbr_beam_args ba{};
        ba.steps = (std::uint32_t)kSteps;
        ba.width = (std::uint32_t)kWidth;
        ba.flags = 0u;
        ba.temperature = a.temperature;
        CHECK(sbr_sessions_beam_search(st.handle(), all.data(), kSessions, &ba, eptr.data(), eitems.data(), nullptr, nullptr, c.items.data(),
                                       c.scores.data(), c.step_lp.data(), c.cum.data(), c.lengths.data(), c.beams.data(), c.partition.shift.data(),
                                       c.partition.mass.data(), &c.partition.frac_bits) == SBR_OK);
        CHECK(same(r, c));
        CHECK(r.lengths[1] == 3 && r.lengths[2] == 0 && r.lengths[0] == kSteps && r.beams[1] == kWidth && r.beams[2] == 0);
        for (std::size_t i = 0; i < kSessions; ++i)
            for (std::size_t b = 0; b < kWidth; ++b)
                for (std::size_t j = 0; j < kSteps; ++j) {
                    const std::size_t p = (i * kWidth + b) * kSteps + j;
                    const bool pad = b >= r.beams[i] || j >= r.lengths[i];
                    CHECK(pad == (r.items[p] == 0xFFFFFFFFu));
                    if (pad) CHECK(std::isinf(r.step_lp[p]) && std::isinf(r.partition.shift[p]) && r.partition.mass[p] == 0);
                    else CHECK(r.step_lp[p] <= 0.0f && std::isfinite(r.step_lp[p]));
                }
        CHECK(r.best(0).size() == kSteps && r.best(2).empty());
        // nothing was written
        const Sessions::State after = st.get_state(all, true);
        CHECK(same_bits(before.h, after.h) && same_bits(before.c, after.c) && before.len == after.len);
        // the model-level convenience is its defining sequence of calls
        models::BeamArgs b = a;
        b.excl_ptr.clear();
        b.excl_items.clear();
        const models::Beams conv = model.beam_search(hist, b).unwrap();
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
        CHECK(same(conv, tmp.beam_search(all, b).unwrap()));
        {  // refusals of the C++ layer and of the library
            bool refused = false;
            models::BeamArgs z;
            z.width = 33;
            try { (void)st.beam_search(all, z); } catch (const EngineError&) { refused = true; }
            CHECK(refused);
            refused = false;
            z.width = 2;
            z.include_seen = true;  // a store without memory
            try { (void)st.beam_search(all, z); } catch (const EngineError&) { refused = true; }
            CHECK(refused);
        }
        dump(out, "hist_ptr.u64", ptr);
        dump(out, "hist_items.u32", items);
        dump(out, "excl_ptr.u64", eptr);
        dump(out, "excl_items.u32", eitems);
        dump(out, "items.u32", r.items);
        dump(out, "scores.f32", r.scores);
        dump(out, "step_lp.f32", r.step_lp);
        dump(out, "cum.f32", r.cum);
        dump(out, "lengths.u32", r.lengths);
        dump(out, "beams.u32", r.beams);
        dump(out, "shift.f32", r.partition.shift);
        dump(out, "mass.u64", r.partition.mass);
        std::printf("lstm normal d=48: sessions=%zu width=%zu steps=%zu beam_search ok\n", kSessions, kWidth, kSteps);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
