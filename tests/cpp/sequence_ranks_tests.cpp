// The C++ host layer's sequence_ranks / sequence_metrics (include/sbr.hpp over sbr_sequence_ranks), driven from
// tests/test_sequence_ranks_cpp.py: the reference protocol's MovieLens split (seed [42;16], user_based_split 0.2), an LSTM fitted
// on the train part (the model of ranking_tests.cpp), then the next-item rank at every position of the test part's windows, or at
// their last <last> positions, and the metrics at k = 10 and 100.  ptr (u64), the ranks (u32) and the metrics (f64) go to a binary
// file the harness compares with the Python call on the same model.
//
// Usage: sequence_ranks_tests <movielens csv> <last, 0 = all> <out file>; exit code 0 = assertions held.
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

static void push(std::vector<double>& m, const evaluation::PositionMetrics& p) {
    m.push_back((double)p.count);
    m.push_back(p.mrr);
    m.push_back(p.mean_rank);
    for (double x : p.hit_rate) m.push_back(x);
    for (double x : p.ndcg) m.push_back(x);
}

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s <movielens csv> <last> <out file>\n", argv[0]);
        return 2;
    }
    const std::size_t last = (std::size_t)std::stoul(argv[2]);
    try {
        data::Interactions data = datasets::download_movielens_100k(argv[1]);
        std::array<std::uint8_t, 16> seed;
        seed.fill(42);
        XorShiftRng rng = XorShiftRng::from_seed(seed);
        auto [train, test] = data::user_based_split(data, rng, 0.2f);
        const data::CompressedInteractions tr = train.to_compressed(), te = test.to_compressed();
        const std::size_t T = 32;
        auto model = models::lstm::Hyperparameters::new_(data.num_items(), T)
                         .embedding_dim(32)
                         .learning_rate(0.16f)
                         .l2_penalty(0.0004f)
                         .loss(models::Loss::WARP)
                         .num_epochs(2)
                         .batch_sequences(8)
                         .rng(rng)
                         .build();
        model.fit(tr).unwrap();
        const std::vector<std::size_t> ks{10, 100};
        models::SequenceRanks r;
        const evaluation::SequenceMetrics m = evaluation::sequence_metrics(model, te, ks, true, last, &r).unwrap();
        CHECK(r.num_users() == te.num_users() && r.ptr[0] == 0 && r.ptr.back() == r.ranks.size() && m.num_positions == r.ranks.size());
        const std::vector<std::uint64_t>& ptr = te.user_pointers();
        for (std::size_t u = 0; u < te.num_users(); ++u) {
            const std::uint64_t n = ptr[u + 1] - ptr[u];
            std::uint64_t want = n < 2 ? 0 : std::min<std::uint64_t>(n, T + 1) - 1;
            if (last) want = std::min<std::uint64_t>(want, last);
            CHECK(r.ptr[u + 1] - r.ptr[u] == want);
        }
        for (std::uint32_t x : r.ranks) CHECK(x >= 1 && x <= data.num_items());
        CHECK(m.by_history_length.size() == T + 1 && m.by_history_length[0].count == 0 && m.macro.count > 0);
        CHECK(m.micro.mrr > 0.0 && m.micro.mrr <= 1.0 && m.micro.mean_rank >= 1.0 && m.micro.hit_rate[1] >= m.micro.hit_rate[0]);
        if (last == 0) {  // the last position of a user whose sequence fits the window is mrr_score's rank
            std::vector<std::uint32_t> mrr_ranks;
            evaluation::mrr_score(model, te, &mrr_ranks).unwrap();
            std::size_t j = 0, compared = 0;
            for (std::size_t u = 0; u < te.num_users(); ++u) {
                const std::uint64_t n = ptr[u + 1] - ptr[u];
                if (n < 2) continue;
                if (n <= T + 1) {
                    CHECK(r.ranks[r.ptr[u + 1] - 1] == mrr_ranks[j]);
                    compared += 1;
                }
                j += 1;
            }
            CHECK(j == mrr_ranks.size() && compared > 0);
            // the kept positions of a call with `last` are the tail of the full call's rows
            const models::SequenceRanks r3 = model.sequence_ranks(te, true, 3).unwrap();
            for (std::size_t u = 0; u < te.num_users(); ++u) {
                const std::uint64_t k3 = r3.ptr[u + 1] - r3.ptr[u];
                CHECK(k3 == std::min<std::uint64_t>(3, r.ptr[u + 1] - r.ptr[u]));
                for (std::uint64_t e = 0; e < k3; ++e) CHECK(r3.ranks[r3.ptr[u + 1] - 1 - e] == r.ranks[r.ptr[u + 1] - 1 - e]);
            }
        }
        std::vector<double> f64;
        push(f64, m.micro);
        push(f64, m.macro);
        for (const evaluation::PositionMetrics& p : m.by_history_length) push(f64, p);
        const std::uint64_t np = r.ptr.size(), nr = r.ranks.size(), nm = f64.size();
        std::FILE* f = std::fopen(argv[3], "wb");
        CHECK(f);
        CHECK(std::fwrite(&np, 8, 1, f) == 1 && std::fwrite(&nr, 8, 1, f) == 1 && std::fwrite(&nm, 8, 1, f) == 1);
        CHECK(std::fwrite(r.ptr.data(), 8, r.ptr.size(), f) == r.ptr.size());
        CHECK(std::fwrite(f64.data(), 8, f64.size(), f) == f64.size());
        CHECK(std::fwrite(r.ranks.data(), 4, r.ranks.size(), f) == r.ranks.size());
        std::fclose(f);
        std::printf("positions=%zu users=%zu mrr=%.4f hit@10=%.4f\n", m.num_positions, m.macro.count, m.micro.mrr, m.micro.hit_rate[0]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
