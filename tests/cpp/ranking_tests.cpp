// The C++ host layer's rank_targets / ranking_metrics (include/sbr.hpp over sbr_rank_targets), driven from
// tests/test_ranking_cpp.py: the reference protocol's MovieLens split (seed [42;16], user_based_split 0.2), an LSTM fitted on
// the train part (the model of recommend_tests.cpp), then the ranking metrics of the test part at k = 10 and 100 over a
// hold-out of <holdout> items.  The ranks (u32) and the metrics (f64) go to a binary file the harness compares with the Python
// call on the same model.
//
// Usage: ranking_tests <movielens csv> <holdout> <out file>; exit code 0 = assertions held.
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
        std::fprintf(stderr, "usage: %s <movielens csv> <holdout> <out file>\n", argv[0]);
        return 2;
    }
    const std::size_t holdout = (std::size_t)std::stoul(argv[2]);
    try {
        data::Interactions data = datasets::download_movielens_100k(argv[1]);
        std::array<std::uint8_t, 16> seed;
        seed.fill(42);
        XorShiftRng rng = XorShiftRng::from_seed(seed);
        auto [train, test] = data::user_based_split(data, rng, 0.2f);
        const data::CompressedInteractions tr = train.to_compressed(), te = test.to_compressed();
        auto model = models::lstm::Hyperparameters::new_(data.num_items(), 32)
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
        std::vector<std::uint32_t> ranks;
        const evaluation::RankingMetrics r = evaluation::ranking_metrics(model, te, ks, holdout, &ranks).unwrap();
        CHECK(r.num_users_ranked > 0 && r.users.size() == r.num_users_ranked && r.per_user_ndcg.size() == 2 * r.num_users_ranked);
        CHECK(ranks.size() >= r.num_users_ranked && ranks.size() <= holdout * r.num_users_ranked);
        for (std::uint32_t x : ranks) CHECK(x >= 1 && x <= data.num_items());
        for (std::size_t j = 0; j < ks.size(); ++j) {
            CHECK(r.ndcg[j] >= 0.0 && r.ndcg[j] <= 1.0 && r.recall[j] >= 0.0 && r.recall[j] <= 1.0);
            CHECK(r.hit_rate[j] >= r.recall[j] && r.precision[j] <= r.hit_rate[j]);
        }
        CHECK(r.recall[1] >= r.recall[0] && r.mrr > 0.0 && r.mrr <= 1.0 && r.mean_rank >= 1.0);
        if (holdout == 1) {  // one target per user, the rest the history: mrr_score's ranks
            std::vector<std::uint32_t> mrr_ranks;
            evaluation::mrr_score(model, te, &mrr_ranks).unwrap();
            CHECK(mrr_ranks == ranks);
        }
        std::vector<double> m;
        m.push_back((double)r.num_users_ranked);
        for (std::size_t j = 0; j < ks.size(); ++j) {
            m.push_back(r.precision[j]);
            m.push_back(r.recall[j]);
            m.push_back(r.hit_rate[j]);
            m.push_back(r.ndcg[j]);
        }
        m.push_back(r.mrr);
        m.push_back(r.mean_rank);
        const std::uint64_t nr = ranks.size(), nm = m.size();
        std::FILE* f = std::fopen(argv[3], "wb");
        CHECK(f);
        CHECK(std::fwrite(&nr, 8, 1, f) == 1 && std::fwrite(&nm, 8, 1, f) == 1);
        CHECK(std::fwrite(m.data(), 8, m.size(), f) == m.size());
        CHECK(std::fwrite(r.per_user_ndcg.data(), 8, r.per_user_ndcg.size(), f) == r.per_user_ndcg.size());
        CHECK(std::fwrite(ranks.data(), 4, ranks.size(), f) == ranks.size());
        std::fclose(f);
        std::printf("users=%zu ranks=%zu recall@10=%.4f ndcg@10=%.4f\n", r.num_users_ranked, ranks.size(), r.recall[0], r.ndcg[0]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 3;
    }
    return 0;
}
