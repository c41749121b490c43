// The C++ host layer's sequence_partition / sequence_log_probs / sequence_log_likelihood (include/sbr.hpp over
// sbr_sequence_partition), driven from tests/test_sequence_partition_cpp.py: the reference protocol's MovieLens split (seed
// [42;16], user_based_split 0.2), an LSTM fitted on the train part (the model of sequence_ranks_tests.cpp), then shift, mass, target
// score, mask flag and log-probability at every position of the test part's windows, or at their last <last> positions, at
// temperature 0.5.  Everything goes to a binary file the harness compares with the Python call on the same model.
//
// Usage: sequence_partition_tests <movielens csv> <last, 0 = all> <out file>; exit code 0 = assertions held.
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

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s <movielens csv> <last> <out file>\n", argv[0]);
        return 2;
    }
    const std::size_t last = (std::size_t)std::stoul(argv[2]);
    const float temperature = 0.5f;
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
        const models::SequencePartition r = model.sequence_partition(te, temperature, true, last).unwrap();
        const std::size_t n = r.scores.size();
        CHECK(r.num_users() == te.num_users() && r.ptr[0] == 0 && r.ptr.back() == n);
        CHECK(r.partition.shift.size() == n && r.partition.mass.size() == n && r.masked.size() == n);
        CHECK(r.partition.frac_bits == sbr_softmax_frac_bits((std::uint32_t)data.num_items()) && r.partition.temperature == temperature);
        const std::vector<std::uint64_t>& ptr = te.user_pointers();
        for (std::size_t u = 0; u < te.num_users(); ++u) {
            const std::uint64_t len = ptr[u + 1] - ptr[u];
            std::uint64_t want = len < 2 ? 0 : std::min<std::uint64_t>(len, T + 1) - 1;
            if (last) want = std::min<std::uint64_t>(want, last);
            CHECK(r.ptr[u + 1] - r.ptr[u] == want);
        }
        evaluation::SequenceLogProbs lp;
        const evaluation::SequenceLogLikelihood ll = evaluation::sequence_log_likelihood(model, te, temperature, true, last, &lp).unwrap();
        CHECK(lp.ptr == r.ptr && lp.log_probs.size() == n);
        const std::vector<double> own = r.log_probs();
        std::size_t masked = 0;
        for (std::size_t p = 0; p < n; ++p) {
            CHECK(r.masked[p] <= 1 && lp.log_probs[p] <= 0.0 && r.partition.mass[p] > 0);
            CHECK(lp.log_probs[p] == own[p]);
            if (r.masked[p]) {
                CHECK(std::isinf(lp.log_probs[p]));
                masked += 1;
            }
        }
        CHECK(ll.positions + ll.masked_positions == n && ll.masked_positions >= masked && ll.positions > 0);
        CHECK(ll.mean_log_prob < 0.0 && ll.perplexity > 1.0 && ll.macro_users > 0);
        if (last == 0) {  // the kept positions of a call with `last` are the tail of the full call's rows
            const models::SequencePartition r3 = model.sequence_partition(te, temperature, true, 3).unwrap();
            for (std::size_t u = 0; u < te.num_users(); ++u) {
                const std::uint64_t k3 = r3.ptr[u + 1] - r3.ptr[u];
                CHECK(k3 == std::min<std::uint64_t>(3, r.ptr[u + 1] - r.ptr[u]));
                for (std::uint64_t e = 0; e < k3; ++e) {
                    const std::uint64_t a = r3.ptr[u + 1] - 1 - e, b = r.ptr[u + 1] - 1 - e;
                    CHECK(std::memcmp(&r3.partition.shift[a], &r.partition.shift[b], 4) == 0 && r3.partition.mass[a] == r.partition.mass[b]);
                    CHECK(std::memcmp(&r3.scores[a], &r.scores[b], 4) == 0 && r3.masked[a] == r.masked[b]);
                }
            }
        }
        const double summary[7] = {(double)ll.positions, (double)ll.masked_positions, (double)ll.macro_users, ll.mean_log_prob,
                                   ll.perplexity,        ll.macro_mean_log_prob,      ll.macro_perplexity};
        const std::uint64_t np = r.ptr.size(), nn = n;
        std::FILE* f = std::fopen(argv[3], "wb");
        CHECK(f);
        CHECK(std::fwrite(&np, 8, 1, f) == 1 && std::fwrite(&nn, 8, 1, f) == 1);
        CHECK(std::fwrite(r.ptr.data(), 8, np, f) == np);
        CHECK(std::fwrite(summary, 8, 7, f) == 7);
        CHECK(std::fwrite(r.partition.mass.data(), 8, n, f) == n);
        CHECK(std::fwrite(lp.log_probs.data(), 8, n, f) == n);
        CHECK(std::fwrite(r.partition.shift.data(), 4, n, f) == n);
        CHECK(std::fwrite(r.scores.data(), 4, n, f) == n);
        CHECK(std::fwrite(r.masked.data(), 1, n, f) == n);
        std::fclose(f);
        std::printf("positions=%zu masked=%zu mean_log_prob=%.4f perplexity=%.2f\n", ll.positions, ll.masked_positions, ll.mean_log_prob,
                    ll.perplexity);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
