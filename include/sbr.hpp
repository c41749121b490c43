// sbr.hpp — C++17 host side of the MI355X sequence-recommender engine.
//
// The reference crate (maciejkula/sbr-rs) is Rust; no Rust toolchain exists in this image, so the
// host layer above the C-ABI (include/sbr_hip.h, libsbr_hip.so) is written in C++ and mirrors the
// crate's public interface for the sequence-model path: same module layout (sbr::data,
// sbr::models::lstm, sbr::models::ewma, sbr::evaluation, sbr::datasets), same names, same
// argument meaning, same error behaviour, so that the reference's own tests read the same here
// (tests/cpp/facade_tests.cpp).  Header-only; needs nothing but sbr_hip.h and libsbr_hip.so.
//
//   reference                                  here
//   Result<T, E>                               sbr::Result<T, E>  (is_ok / is_err / unwrap / unwrap_err)
//   panic!                                     sbr::EngineError (std::runtime_error)
//   rand::XorShiftRng                          sbr::XorShiftRng   (the engine's documented stream)
//   Vec<f32>, &[ItemId]                        std::vector<float>, const std::vector<ItemId>&
//
// Everything numeric runs on the GPU through the C-ABI.  There is no CPU fallback: without a
// gfx950 device `build()` throws EngineError(SBR_ERR_NO_DEVICE).
#ifndef SBR_HPP
#define SBR_HPP

#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <limits>
#include <memory>
#include <numeric>
#include <optional>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <variant>
#include <vector>

#include "sbr_hip.h"

namespace sbr {

// ---- lib.rs:77-116 ---------------------------------------------------------------------------
using UserId = std::size_t;    // lib.rs:77
using ItemId = std::size_t;    // lib.rs:79
using Timestamp = std::size_t; // lib.rs:81

/// Prediction error types (lib.rs:84-89).
enum class PredictionError { InvalidPredictionValue };
/// Fitting error types (lib.rs:93-97).
enum class FittingError { NoInteractions };

inline const char* to_string(PredictionError) { return "Invalid prediction value: non-finite or not a number."; }
inline const char* to_string(FittingError) { return "No interactions were supplied."; }

/// Anything the reference would `panic!` on, plus ABI-level failures (no device, HIP error, out
/// of memory, unsupported configuration).
struct EngineError : std::runtime_error {
    sbr_status status;
    EngineError(sbr_status st, const std::string& where)
        : std::runtime_error(where + ": " + sbr_status_string(st)), status(st) {}
};

/// The engine keeps the scratch of a fit call (device and pinned-host blocks up to 64 MiB) for the next call — the reference's
/// own bench re-fits one model in a loop (benches/benchmark.rs:40-42).  A long-lived process that is done fitting gives it back.
inline void release_cached_memory() { sbr_release_cached_memory(); }

/// Minimal Result: holds either a value or an error enum.
template <class T, class E>
class Result {
  public:
    static Result Ok(T value) { return Result(std::in_place_index<0>, std::move(value)); }
    static Result Err(E error) { return Result(std::in_place_index<1>, error); }
    bool is_ok() const { return v_.index() == 0; }
    bool is_err() const { return v_.index() == 1; }
    /// The value; throws std::runtime_error with the error text otherwise (≙ `unwrap` panicking).
    T& unwrap() {
        if (is_err()) throw std::runtime_error(std::string("called unwrap() on an Err value: ") + to_string(std::get<1>(v_)));
        return std::get<0>(v_);
    }
    const T& unwrap() const { return const_cast<Result*>(this)->unwrap(); }
    E unwrap_err() const {
        if (is_ok()) throw std::runtime_error("called unwrap_err() on an Ok value");
        return std::get<1>(v_);
    }

  private:
    template <std::size_t I, class U>
    Result(std::in_place_index_t<I> tag, U&& u) : v_(tag, std::forward<U>(u)) {}
    std::variant<T, E> v_;
};

// ---- the index RNG --------------------------------------------------------------------------
/// rand 0.5's `XorShiftRng` as recalled: Marsaglia xorshift128, next_u64 = low word
/// first, gen_range / shuffle / Uniform with the crate's widening-multiply rejection zones — the
/// object handed to `Hyperparameters::rng` / `from_seed` (lstm.rs:122-132).  Identical in the library
/// (sbr_numerics.h: sbr_xorshift, sbr_rand_*), the Python host layer and here; the crate's source is not
/// in this image and no reference test pins a stream.
class XorShiftRng {
  public:
    static XorShiftRng from_seed(const std::array<std::uint8_t, 16>& seed) {
        XorShiftRng r;
        bool any = false;
        for (int i = 0; i < 4; ++i) {
            r.s_[i] = (std::uint32_t)seed[4 * i] | ((std::uint32_t)seed[4 * i + 1] << 8) |
                      ((std::uint32_t)seed[4 * i + 2] << 16) | ((std::uint32_t)seed[4 * i + 3] << 24);
            any = any || r.s_[i] != 0;
        }
        if (!any) r.s_ = {0x193A6754u, 0xA8A7D469u, 0x97830E05u, 0x113BA7BBu};
        return r;
    }
    /// `XorShiftRng::from_seed(rand::thread_rng().gen())` (lstm.rs:67)
    static XorShiftRng from_entropy() {
        std::random_device rd;
        std::array<std::uint8_t, 16> seed;
        for (auto& b : seed) b = (std::uint8_t)rd();
        return from_seed(seed);
    }
    /// The 16 bytes that re-create the current state through from_seed.
    std::array<std::uint8_t, 16> state_seed() const {
        std::array<std::uint8_t, 16> out;
        for (int i = 0; i < 4; ++i)
            for (int b = 0; b < 4; ++b) out[4 * i + b] = (std::uint8_t)(s_[i] >> (8 * b));
        return out;
    }
    std::uint32_t next_u32() {
        const std::uint32_t t = s_[0] ^ (s_[0] << 11);
        s_[0] = s_[1];
        s_[1] = s_[2];
        s_[2] = s_[3];
        s_[3] = s_[3] ^ (s_[3] >> 19) ^ (t ^ (t >> 8));
        return s_[3];
    }
    std::uint64_t next_u64() {
        const std::uint64_t lo = next_u32();
        const std::uint64_t hi = next_u32();
        return lo | (hi << 32);
    }
    /// `Rng::gen_range(low, high)` (rand 0.5 `UniformInt::sample_single`): zone = range << leading_zeros(range),
    /// accept when the low half of next_u64() * range is <= zone, result = low + high half.
    /// Panics in the crate when low >= high (`assert!(low < high)`); here: std::invalid_argument.
    std::uint64_t gen_range(std::uint64_t low, std::uint64_t high) {
        if (low >= high) throw std::invalid_argument("gen_range: low must be below high");
        const std::uint64_t range = high - low;
        const std::uint64_t zone = range << __builtin_clzll(range);
        for (;;) {
            const unsigned __int128 m = (unsigned __int128)next_u64() * range;
            if ((std::uint64_t)m <= zone) return low + (std::uint64_t)(m >> 64);
        }
    }
    /// `Uniform::new(low, high).sample(rng)`: zone = MAX - (MAX - range + 1) % range (data.rs:77-78).
    std::uint64_t uniform(std::uint64_t low, std::uint64_t high) {
        if (low >= high) throw std::invalid_argument("Uniform::new: low must be below high");
        const std::uint64_t range = high - low, max = std::numeric_limits<std::uint64_t>::max();
        const std::uint64_t zone = max - (max - range + 1) % range;
        for (;;) {
            const unsigned __int128 m = (unsigned __int128)next_u64() * range;
            if ((std::uint64_t)m <= zone) return low + (std::uint64_t)(m >> 64);
        }
    }
    /// gen_range(0, n)
    std::uint64_t below(std::uint64_t n) { return gen_range(0, n); }
    /// `rng.gen::<f64>()` (rand 0.5 `Standard`): 53 random bits scaled to [0, 1).
    double unit() { return (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }
    /// `Rng::shuffle`: i = len; while i >= 2 { i -= 1; swap(i, gen_range(0, i + 1)) }.
    template <class T>
    void shuffle(std::vector<T>& v) {
        for (std::size_t i = v.size(); i >= 2;) {
            i -= 1;
            std::swap(v[i], v[gen_range(0, i + 1)]);
        }
    }

  private:
    std::array<std::uint32_t, 4> s_{};
};

// =============================================================================================
// sbr::data  (src/data.rs)
// =============================================================================================
namespace data {

/// Basic interaction type (data.rs:17-51).
class Interaction {
  public:
    Interaction(UserId user_id, ItemId item_id, Timestamp timestamp)
        : user_id_(user_id), item_id_(item_id), timestamp_(timestamp) {}
    UserId user_id() const { return user_id_; }
    ItemId item_id() const { return item_id_; }
    float weight() const { return 1.0f; }
    Timestamp timestamp() const { return timestamp_; }
    bool operator==(const Interaction& o) const {
        return user_id_ == o.user_id_ && item_id_ == o.item_id_ && timestamp_ == o.timestamp_;
    }

  private:
    UserId user_id_;
    ItemId item_id_;
    Timestamp timestamp_;
};

class CompressedInteractions;
class TripletInteractions;

/// A collection of individual interactions (data.rs:92-211).
class Interactions {
  public:
    Interactions(std::size_t num_users, std::size_t num_items) : num_users_(num_users), num_items_(num_items) {}
    /// `impl From<Vec<Interaction>>` (data.rs:200-211): num_users / num_items = max id + 1.
    static Interactions from(std::vector<Interaction> interactions) {
        std::size_t nu = 0, ni = 0;
        for (const auto& x : interactions) {
            nu = std::max(nu, x.user_id() + 1);
            ni = std::max(ni, x.item_id() + 1);
        }
        Interactions out(nu, ni);
        out.interactions_ = std::move(interactions);
        return out;
    }
    void push(const Interaction& interaction) { interactions_.push_back(interaction); }
    const std::vector<Interaction>& data() const { return interactions_; }
    std::size_t len() const { return interactions_.size(); }
    bool is_empty() const { return interactions_.empty(); }
    void shuffle(XorShiftRng& rng) { rng.shuffle(interactions_); }
    std::pair<Interactions, Interactions> split_at(std::size_t idx) const {
        Interactions head(num_users_, num_items_), tail(num_users_, num_items_);
        head.interactions_.assign(interactions_.begin(), interactions_.begin() + (std::ptrdiff_t)idx);
        tail.interactions_.assign(interactions_.begin() + (std::ptrdiff_t)idx, interactions_.end());
        return {std::move(head), std::move(tail)};
    }
    /// (those for which func is true, the rest) — data.rs:149-172
    template <class F>
    std::pair<Interactions, Interactions> split_by(F func) const {
        Interactions head(num_users_, num_items_), tail(num_users_, num_items_);
        for (const auto& x : interactions_) (func(x) ? head : tail).interactions_.push_back(x);
        return {std::move(head), std::move(tail)};
    }
    inline CompressedInteractions to_compressed() const;
    inline TripletInteractions to_triplet() const;
    std::size_t num_users() const { return num_users_; }
    std::size_t num_items() const { return num_items_; }
    std::pair<std::size_t, std::size_t> shape() const { return {num_users_, num_items_}; }

  private:
    std::size_t num_users_, num_items_;
    std::vector<Interaction> interactions_;
};

/// Random split (data.rs:54-64): shuffles `interactions` in place; the first test_fraction of the
/// shuffled data is the test set.  Returns (train, test).
inline std::pair<Interactions, Interactions> train_test_split(Interactions& interactions, XorShiftRng& rng,
                                                              float test_fraction) {
    interactions.shuffle(rng);
    const std::size_t cut = (std::size_t)(test_fraction * (float)interactions.len());
    auto parts = interactions.split_at(cut);
    return {std::move(parts.second), std::move(parts.first)};
}

namespace detail {
/// SipHash-2-4 of one u64 written as 8 little-endian bytes (`Hasher::write_usize` on a 64-bit
/// target, data.rs:81-84; siphasher 0.2's SipHasher is SipHash-2-4).
inline std::uint64_t siphash24_u64(std::uint64_t k0, std::uint64_t k1, std::uint64_t m) {
    auto rotl = [](std::uint64_t x, int b) { return (x << b) | (x >> (64 - b)); };
    std::uint64_t v0 = k0 ^ 0x736F6D6570736575ull, v1 = k1 ^ 0x646F72616E646F6Dull;
    std::uint64_t v2 = k0 ^ 0x6C7967656E657261ull, v3 = k1 ^ 0x7465646279746573ull;
    auto round = [&]() {
        v0 += v1; v1 = rotl(v1, 13); v1 ^= v0; v0 = rotl(v0, 32);
        v2 += v3; v3 = rotl(v3, 16); v3 ^= v2;
        v0 += v3; v3 = rotl(v3, 21); v3 ^= v0;
        v2 += v1; v1 = rotl(v1, 17); v1 ^= v2; v2 = rotl(v2, 32);
    };
    v3 ^= m; round(); round(); v0 ^= m;
    const std::uint64_t tail = (std::uint64_t)8 << 56; // message length in the top byte, no tail bytes
    v3 ^= tail; round(); round(); v0 ^= tail;
    v2 ^= 0xFF;
    round(); round(); round(); round();
    return v0 ^ v1 ^ v2 ^ v3;
}
} // namespace detail

/// Split so that no user is in both sets (data.rs:69-88): two u64 keys from rng, SipHash-2-4 of
/// the user id, train iff hash % 100000 > (test_fraction * 100000) as u64.  Returns (train, test).
inline std::pair<Interactions, Interactions> user_based_split(Interactions& interactions, XorShiftRng& rng,
                                                              float test_fraction) {
    const std::uint64_t denominator = 100000;
    const std::uint64_t train_cutoff = (std::uint64_t)(test_fraction * (float)denominator);
    const std::uint64_t key_0 = rng.uniform(0, std::numeric_limits<std::uint64_t>::max());
    const std::uint64_t key_1 = rng.uniform(0, std::numeric_limits<std::uint64_t>::max());
    return interactions.split_by([&](const Interaction& x) {
        return detail::siphash24_u64(key_0, key_1, (std::uint64_t)x.user_id()) % denominator > train_cutoff;
    });
}

/// A single user's data, earliest to latest (data.rs:339-371).  A view into CompressedInteractions.
struct CompressedInteractionsUser {
    UserId user_id;
    const std::uint32_t* item_ids;
    const std::uint64_t* timestamps;
    std::size_t length;

    std::size_t len() const { return length; }
    bool is_empty() const { return length == 0; }
    /// One chunk of at most chunk_size interactions: (item_ids, timestamps).
    using Chunk = std::pair<std::vector<ItemId>, std::vector<Timestamp>>;
    /// Chunked view: the FIRST chunk is the short one, all the others have chunk_size elements
    /// (data.rs:363-370, 406-431).
    std::vector<Chunk> chunks(std::size_t chunk_size) const {
        std::vector<Chunk> out;
        std::size_t idx = 0;
        while (idx < length) {
            const std::size_t rem = (length - idx) % chunk_size;
            const std::size_t size = rem == 0 ? chunk_size : rem;
            out.emplace_back(std::vector<ItemId>(item_ids + idx, item_ids + idx + size),
                             std::vector<Timestamp>(timestamps + idx, timestamps + idx + size));
            idx += size;
        }
        return out;
    }
};

/// CSR by user, time-sorted (data.rs:227-329).  Storage is exactly what the C-ABI takes:
/// user_pointers u64 [num_users + 1], item_ids u32 [nnz] (sbr_model_fit / sbr_mrr_score).
class CompressedInteractions {
  public:
    CompressedInteractions(std::size_t num_users, std::size_t num_items, std::vector<std::uint64_t> user_pointers,
                           std::vector<std::uint32_t> item_ids, std::vector<std::uint64_t> timestamps)
        : num_users_(num_users), num_items_(num_items), user_pointers_(std::move(user_pointers)),
          item_ids_(std::move(item_ids)), timestamps_(std::move(timestamps)) {}

    /// `impl From<&Interactions>` (data.rs:236-265): stable sort by (user, timestamp).
    static CompressedInteractions from(const Interactions& interactions) {
        std::vector<Interaction> data = interactions.data();
        std::stable_sort(data.begin(), data.end(), [](const Interaction& a, const Interaction& b) {
            return a.user_id() != b.user_id() ? a.user_id() < b.user_id() : a.timestamp() < b.timestamp();
        });
        std::vector<std::uint64_t> ptr(interactions.num_users() + 1, 0);
        std::vector<std::uint32_t> items;
        std::vector<std::uint64_t> ts;
        items.reserve(data.size());
        ts.reserve(data.size());
        for (const auto& x : data) {
            ptr[x.user_id() + 1] += 1;
            items.push_back((std::uint32_t)x.item_id());
            ts.push_back((std::uint64_t)x.timestamp());
        }
        for (std::size_t u = 0; u < interactions.num_users(); ++u) ptr[u + 1] += ptr[u];
        return CompressedInteractions(interactions.num_users(), interactions.num_items(), std::move(ptr), std::move(items),
                                      std::move(ts));
    }

    std::optional<CompressedInteractionsUser> get_user(UserId user_id) const {
        if (user_id >= num_users_) return std::nullopt;
        const std::size_t start = (std::size_t)user_pointers_[user_id], stop = (std::size_t)user_pointers_[user_id + 1];
        return CompressedInteractionsUser{user_id, item_ids_.data() + start, timestamps_.data() + start, stop - start};
    }
    /// Iterate over users (data.rs:269-274).
    std::vector<CompressedInteractionsUser> iter_users() const {
        std::vector<CompressedInteractionsUser> out;
        out.reserve(num_users_);
        for (UserId u = 0; u < num_users_; ++u) out.push_back(*get_user(u));
        return out;
    }
    std::size_t num_users() const { return num_users_; }
    std::size_t num_items() const { return num_items_; }
    std::pair<std::size_t, std::size_t> shape() const { return {num_users_, num_items_}; }
    Interactions to_interactions() const {
        Interactions out(num_users_, num_items_);
        for (UserId u = 0; u < num_users_; ++u)
            for (std::uint64_t k = user_pointers_[u]; k < user_pointers_[u + 1]; ++k)
                out.push(Interaction(u, item_ids_[k], (Timestamp)timestamps_[k]));
        return out;
    }
    const std::vector<std::uint64_t>& user_pointers() const { return user_pointers_; }
    const std::vector<std::uint32_t>& item_ids() const { return item_ids_; }
    const std::vector<std::uint64_t>& timestamps() const { return timestamps_; }

  private:
    std::size_t num_users_, num_items_;
    std::vector<std::uint64_t> user_pointers_;
    std::vector<std::uint32_t> item_ids_;
    std::vector<std::uint64_t> timestamps_;
};

inline CompressedInteractions Interactions::to_compressed() const { return CompressedInteractions::from(*this); }

/// A minibatch of triplet interactions: views into the three arrays (data.rs:502-520).
struct TripletMinibatch {
    const UserId* user_ids;
    const ItemId* item_ids;
    const Timestamp* timestamps;
    std::size_t size;
    std::size_t len() const { return size; }
    bool is_empty() const { return size == 0; }
};

/// Interactions in COO form (data.rs:435-481).  Not consumed by the sequence models; kept for API parity.
class TripletInteractions {
  public:
    /// Minibatches of exactly minibatch_size interactions over [idx, stop_idx): a shorter remainder is never
    /// yielded (data.rs:522-545).  next() returns false at the end.
    class MinibatchIterator {
      public:
        MinibatchIterator(const TripletInteractions* interactions, std::size_t idx, std::size_t stop_idx, std::size_t minibatch_size)
            : interactions_(interactions), idx_(idx), stop_idx_(stop_idx), minibatch_size_(minibatch_size) {}
        /// The same data and minibatch size over [start, stop) (data.rs:491-499).
        MinibatchIterator slice(std::size_t start, std::size_t stop) const { return {interactions_, start, stop, minibatch_size_}; }
        bool next(TripletMinibatch& out) {
            const std::size_t start = idx_, stop = idx_ + minibatch_size_;
            idx_ = stop;
            if (stop > stop_idx_) return false;
            out = {interactions_->user_ids_.data() + start, interactions_->item_ids_.data() + start,
                   interactions_->timestamps_.data() + start, minibatch_size_};
            return true;
        }

      private:
        const TripletInteractions* interactions_;
        std::size_t idx_, stop_idx_, minibatch_size_;
    };

    /// `impl From<&Interactions>` (data.rs:558-575): the interactions' own order.
    static TripletInteractions from(const Interactions& interactions) {
        TripletInteractions out;
        out.num_users_ = interactions.num_users();
        out.num_items_ = interactions.num_items();
        out.user_ids_.reserve(interactions.len());
        out.item_ids_.reserve(interactions.len());
        out.timestamps_.reserve(interactions.len());
        for (const auto& x : interactions.data()) {
            out.user_ids_.push_back(x.user_id());
            out.item_ids_.push_back(x.item_id());
            out.timestamps_.push_back(x.timestamp());
        }
        return out;
    }
    std::size_t len() const { return user_ids_.size(); }
    bool is_empty() const { return user_ids_.empty(); }
    MinibatchIterator iter_minibatch(std::size_t minibatch_size) const { return {this, 0, len(), minibatch_size}; }
    /// num_partitions iterators over consecutive slices of len / num_partitions interactions (integer division:
    /// the remainder belongs to no partition, data.rs:463-475).
    std::vector<MinibatchIterator> iter_minibatch_partitioned(std::size_t minibatch_size, std::size_t num_partitions) const {
        const MinibatchIterator iterator = iter_minibatch(minibatch_size);
        const std::size_t chunk_size = len() / num_partitions;
        std::vector<MinibatchIterator> out;
        for (std::size_t x = 0; x < num_partitions; ++x) out.push_back(iterator.slice(x * chunk_size, (x + 1) * chunk_size));
        return out;
    }
    std::size_t num_users() const { return num_users_; }
    std::size_t num_items() const { return num_items_; }
    std::pair<std::size_t, std::size_t> shape() const { return {num_users_, num_items_}; }

  private:
    std::size_t num_users_ = 0, num_items_ = 0;
    std::vector<UserId> user_ids_;
    std::vector<ItemId> item_ids_;
    std::vector<Timestamp> timestamps_;
};

inline TripletInteractions Interactions::to_triplet() const { return TripletInteractions::from(*this); }

} // namespace data

// =============================================================================================
// OnlineRankingModel (lib.rs:101-116)
// =============================================================================================
template <class UserRepresentation>
class OnlineRankingModel {
  public:
    virtual ~OnlineRankingModel() = default;
    /// From a chronologically ordered sequence of items compute a user representation.
    virtual Result<UserRepresentation, PredictionError> user_representation(const std::vector<ItemId>& item_ids) const = 0;
    /// Scores of `item_ids` for that user representation.
    virtual Result<std::vector<float>, PredictionError> predict(const UserRepresentation& user,
                                                                const std::vector<ItemId>& item_ids) const = 0;
};

// =============================================================================================
// sbr::models  (src/models/mod.rs, sequence_model.rs, lstm.rs, ewma.rs)
// =============================================================================================
namespace models {

/// The user representation used by implicit sequence models (mod.rs:9-12).
struct ImplicitUser {
    std::vector<float> user_embedding;
};
/// Top-k recommendations of ImplicitSequenceModel::recommend: row-major [num_users][k] (similar_items: a row per query item).
struct Recommendations {
    std::size_t num_users = 0, k = 0;
    std::vector<std::uint32_t> items;
    std::vector<float> scores;
};
/// The per-position ranks of ImplicitSequenceModel::sequence_ranks, CSR: user u's are ranks[ptr[u] .. ptr[u + 1]), positions ascending.
struct SequenceRanks {
    std::vector<std::uint64_t> ptr;
    std::vector<std::uint32_t> ranks;
    std::size_t num_users() const { return ptr.empty() ? 0 : ptr.size() - 1; }
};
/// The per-user tag filter of the *_filtered top-k calls (named methods, so that no braced argument of a plain form changes its
/// meaning), against the model's item tags (ImplicitSequenceModel::set_item_tags): user u may see
/// item i iff (tags[i] & none_of[u]) == 0 && (any_of[u] == 0 || (tags[i] & any_of[u]) != 0).  Each vector is empty (all zeros), holds
/// one mask for every user, or one mask per user (query, slot) of the call.
struct TagFilter {
    std::vector<std::uint32_t> any_of, none_of;
};
/// The rule of the recommend_capped calls (struct sbr_cap_args; CAPPED in sbr_hip.h): at most `cap` items of one item group per row
/// (ImplicitSequenceModel::set_item_groups), applied on the device to each row's best `pool` (0: min(1 024, max(64, 4 k))).  exact:
/// the rows the pool did not settle are finished through recommend_top at a growing n with the rule on the host.
struct CapArgs {
    std::uint32_t cap = 1;
    std::uint32_t pool = 0;
    bool exact = true;
};
/// Rows of the recommend_capped calls, row-major [num_users][k], padded with (0xFFFFFFFF, -inf), and one flag per row: 1 where the
/// row is the exact answer over the whole catalogue (always, with CapArgs::exact), 0 where it is a short prefix of it.
struct CappedRecommendations {
    std::size_t num_users = 0, k = 0;
    std::vector<std::uint32_t> items;
    std::vector<float> scores;
    std::vector<std::uint8_t> complete;
};
/// The noise of the recommend_sampled calls (struct sbr_sample_args): k draws without replacement from softmax(score / temperature);
/// the noise of (row, item) is a function of (seed, streams[row], item) alone.  streams: empty (the row's index in the call; for a
/// session store the slot id) or one per row.
struct SampleArgs {
    float temperature = 1.0f;
    std::uint64_t seed = 0;
    std::vector<std::uint64_t> streams;
};
/// Rows of the recommend_sampled calls, row-major [num_users][k]: the drawn items in draw order, their plain scores (predict's bits,
/// not sorted) and their keys (descending); short rows padded with (0xFFFFFFFF, -inf, -inf).
struct SampledRecommendations {
    std::size_t num_users = 0, k = 0;
    std::vector<std::uint32_t> items;
    std::vector<float> scores, keys;
};
/// What the log_partition calls return (PARTITION in sbr_hip.h): per row the shift (the largest score / temperature over the items
/// the row may see; -inf: none), the fixed-point mass (the sum of the items' weights w = floor(exp32(score / T - shift) 2^frac_bits),
/// exact and independent of the batch and of how the scan is cut up) and the catalogue's frac_bits.  The model's probability of an
/// item is w / mass; the weights come from sbr_softmax_weights, the library's one host statement of them.
struct Partition {
    float temperature = 1.0f;
    std::uint32_t frac_bits = 0;
    std::vector<float> shift;
    std::vector<std::uint64_t> mass;
    std::size_t num_users() const { return shift.size(); }
    /// shift + log(mass / 2^frac_bits) per row; -inf for a row that may see nothing.
    std::vector<double> log_z() const {
        std::vector<double> z(shift.size());
        for (std::size_t u = 0; u < z.size(); ++u)
            z[u] = mass[u] ? (double)shift[u] + std::log(std::ldexp((double)mass[u], -(int)frac_bits)) : -std::numeric_limits<double>::infinity();
        return z;
    }
    /// The weights of plain scores, row-major [num_users][m].
    std::vector<std::uint64_t> weights(const std::vector<float>& scores) const {
        const std::size_t n = shift.size();
        if (n == 0 ? !scores.empty() : scores.size() % n != 0) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Partition: scores [num_users][m]");
        const std::size_t m = n ? scores.size() / n : 0;
        std::vector<std::uint64_t> w(scores.size());
        const sbr_status st = sbr_softmax_weights_rows(scores.data(), (std::uint64_t)n, (std::uint64_t)m, temperature, shift.data(), frac_bits, w.data());
        if (st != SBR_OK) throw EngineError(st, "sbr_softmax_weights_rows");
        return w;
    }
    /// log(w / mass) of items with the plain scores [num_users][m]: the log-probability of one draw; -inf where w == 0.
    std::vector<double> log_prob(const std::vector<float>& scores) const {
        const std::vector<std::uint64_t> w = weights(scores);
        const std::size_t m = shift.empty() ? 0 : scores.size() / shift.size();
        std::vector<double> out(w.size());
        for (std::size_t p = 0; p < w.size(); ++p)
            out[p] = w[p] ? std::log((double)w[p]) - std::log((double)mass[p / m]) : -std::numeric_limits<double>::infinity();
        return out;
    }
    /// The Plackett-Luce conditional log-probabilities of draws without replacement with the plain scores [num_users][k] in draw
    /// order (SampledRecommendations::scores): log(w_j) - log(mass - the w before j), the remaining mass an exact integer; NaN at
    /// padding (-inf score) and where w_j == 0.  Meaningful only for a partition taken with the draws' exclusions and masks.
    std::vector<double> slate_log_prob(const std::vector<float>& scores) const {
        const std::vector<std::uint64_t> w = weights(scores);
        const std::size_t k = shift.empty() ? 0 : scores.size() / shift.size();
        std::vector<double> out(w.size(), std::numeric_limits<double>::quiet_NaN());
        for (std::size_t u = 0; u < shift.size(); ++u) {
            std::uint64_t rest = mass[u];
            for (std::size_t j = 0; j < k; ++j) {
                const std::uint64_t wj = w[u * k + j];
                if (wj == 0 || std::isinf(scores[u * k + j])) continue;
                if (rest == 0 || wj > rest) { rest = 0; continue; }
                out[u * k + j] = std::log((double)wj) - std::log((double)rest);
                rest -= wj;
            }
        }
        return out;
    }
};
/// The arguments of the rollout calls (struct sbr_rollout_args and the lists around it; ROLLOUT in sbr_hip.h).  `sample`: each pick is
/// the one draw of recommend_sampled(k = 1) at noise.seed + step, else the top-1; noise.temperature is also the per-step partition's
/// (`log_prob`), in either mode; noise.streams default to the slot ids.  `final_state`: the states after all picks are returned too —
/// `lstm` says whether the model has cell states (ImplicitSequenceModel::rollout sets it itself).
struct RolloutArgs {
    std::size_t steps = 1;
    bool sample = false, allow_repeats = false, include_seen = false, log_prob = false, final_state = false, lstm = true;
    SampleArgs noise;
    TagFilter filter;
    std::vector<std::uint64_t> excl_ptr;
    std::vector<std::uint32_t> excl_items;
};
/// What the rollout calls return, row-major [num_rows][steps]: row i's picks in pick order with their plain scores, padded with
/// (0xFFFFFFFF, -inf) from the step at which the row had nothing left to choose from, and lengths [num_rows], its real steps.  keys:
/// the winning keys of a sampled rollout, else empty.  With log_prob: `partition` holds one row per (row, step) — shift -inf and mass 0
/// at padding — and log_prob = partition.log_prob of the picks' scores, NaN at padding.  With final_state: h, c (empty for EWMA)
/// [num_rows][embedding_dim] and len, in Sessions::State's format, after all picks.
struct Rollout {
    std::size_t num_rows = 0, steps = 0;
    std::vector<std::uint32_t> items, lengths;
    std::vector<float> scores, keys;
    Partition partition;
    std::vector<double> log_prob;
    std::vector<float> h, c;
    std::vector<std::uint64_t> len;
};
/// The arguments of the beam-search calls (struct sbr_beam_args and the lists around it; BEAM SEARCH in sbr_hip.h): `width` beams
/// per row, `temperature` the per-step partition's; `partitions`: each (beam, step)'s shift and mass are returned too.
struct BeamArgs {
    std::size_t steps = 1, width = 4;
    float temperature = 1.0f;
    bool allow_repeats = false, include_seen = false, partitions = false;
    TagFilter filter;
    std::vector<std::uint64_t> excl_ptr;
    std::vector<std::uint32_t> excl_items;
};
/// What the beam-search calls return, beams in selection order at each row's last real step: items, scores and step_lp
/// [num_rows][width][steps] (padding (0xFFFFFFFF, -inf), -inf in step_lp), cum [num_rows][width] (-inf for a missing beam), lengths
/// (the real steps) and beams (the live beams) [num_rows].  With partitions: `partition` holds one row per (row, beam, step) — shift
/// -inf and mass 0 at padding.
struct Beams {
    std::size_t num_rows = 0, width = 0, steps = 0;
    std::vector<std::uint32_t> items, lengths, beams;
    std::vector<float> scores, step_lp, cum;
    Partition partition;
    /// beam 0 of row i, its real picks
    std::vector<std::uint32_t> best(std::size_t i) const {
        const std::size_t n = beams[i] ? lengths[i] : 0;
        return std::vector<std::uint32_t>(items.begin() + (std::ptrdiff_t)(i * width * steps), items.begin() + (std::ptrdiff_t)(i * width * steps + n));
    }
};
/// What ImplicitSequenceModel::sequence_partition returns (SEQUENCE PARTITION in sbr_hip.h), CSR over the kept positions: user u's
/// are entries ptr[u] .. ptr[u + 1), positions ascending, of the partition's rows, of `scores` (the targets' plain scores) and of
/// `masked` (1 where the policy masks the target: its log-probability is -inf).
struct SequencePartition {
    std::vector<std::uint64_t> ptr;
    Partition partition;
    std::vector<float> scores;
    std::vector<std::uint8_t> masked;
    std::size_t num_users() const { return ptr.empty() ? 0 : ptr.size() - 1; }
    /// log(w / mass) of every position's target, Partition::log_prob of its score; -inf where it is masked or its weight is 0.
    std::vector<double> log_probs() const {
        std::vector<double> lp = partition.log_prob(scores);
        for (std::size_t p = 0; p < lp.size(); ++p)
            if (masked[p]) lp[p] = -std::numeric_limits<double>::infinity();
        return lp;
    }
};
/// The order of each row of an Above: by score descending with ties to the lower id (the total order of every top-k call), or by
/// ascending id (as the library writes it).
enum class AboveOrder { Score, Id };
/// What the *_above calls return (ABOVE in sbr_hip.h): every (row, id, score) pair whose score is >= the row's threshold, as CSR —
/// row i's pairs are entries ptr[i] .. ptr[i + 1] of ids / scores.  A set, not a list of k: a row may hold far more than
/// SBR_RECOMMEND_MAX_K entries.  The *_top calls return the same with `cuts`: each row its exact best n.
struct Above {
    std::vector<std::uint64_t> ptr;  ///< [rows + 1]
    std::vector<std::uint32_t> ids;
    std::vector<float> scores;
    AboveOrder order = AboveOrder::Score;
    /// [rows] from a *_top call (TOP in sbr_hip.h): the score of a row's last entry, -inf where the row holds everything eligible,
    /// +inf for n = 0; empty from an *_above call.
    std::vector<float> cuts;
    std::size_t rows() const { return ptr.empty() ? 0 : ptr.size() - 1; }
    std::uint64_t count(std::size_t i) const { return ptr[i + 1] - ptr[i]; }
    std::uint64_t total() const { return ptr.empty() ? 0 : ptr.back(); }
    /// Rows in ascending id order -> score order: a stable sort on top of the id order (-0.0 and +0.0 tie), so ties go to the lower id.
    void sort_by_score() {
        std::vector<std::size_t> at;
        std::vector<std::uint32_t> ti;
        std::vector<float> ts;
        for (std::size_t r = 0; r < rows(); ++r) {
            const std::size_t a = (std::size_t)ptr[r], n = (std::size_t)(ptr[r + 1] - ptr[r]);
            at.resize(n);
            for (std::size_t j = 0; j < n; ++j) at[j] = j;
            std::stable_sort(at.begin(), at.end(), [&](std::size_t x, std::size_t y) { return scores[a + x] > scores[a + y]; });
            ti.assign(ids.begin() + (std::ptrdiff_t)a, ids.begin() + (std::ptrdiff_t)(a + n));
            ts.assign(scores.begin() + (std::ptrdiff_t)a, scores.begin() + (std::ptrdiff_t)(a + n));
            for (std::size_t j = 0; j < n; ++j) {
                ids[a + j] = ti[at[j]];
                scores[a + j] = ts[at[j]];
            }
        }
        order = AboveOrder::Score;
    }
};
/// The default max_results of the *_above calls: the entries of the one buffer they call with (2^24 pairs).
constexpr std::uint64_t ABOVE_MAX_RESULTS = 1ull << 24;
/// What ImplicitSequenceModel::similar_items ranks by: the cosine of two item embeddings, or their plain dot product.
enum class Similarity { Cosine = SBR_SIMILAR_COSINE, Dot = SBR_SIMILAR_DOT };
/// The loss used for training the model (mod.rs:15-23).
enum class Loss { BPR = SBR_LOSS_BPR, Hinge = SBR_LOSS_HINGE, WARP = SBR_LOSS_WARP };
/// Optimizer used to train the model (mod.rs:26-32).
enum class Optimizer { Adagrad = SBR_OPT_ADAGRAD, Adam = SBR_OPT_ADAM };
/// Type of parallelism (mod.rs:35-41).  Synchronous: every replica sees every update before its
/// next minibatch.  Asynchronous: the deterministic analogue of Hogwild — with more than one replica,
/// minibatch k+1 is computed on parameters that lack update k (staleness exactly one step), so the
/// exchange runs underneath the computation.
enum class Parallelism { Asynchronous = SBR_PAR_ASYNCHRONOUS, Synchronous = SBR_PAR_SYNCHRONOUS };

namespace detail {

inline void check(sbr_status st, const char* where) {
    if (st != SBR_OK) throw EngineError(st, where);
}

/// One mask vector of a TagFilter as the n words a *_filtered call takes (n == 0: one word, never read).
inline std::vector<std::uint32_t> tag_masks(const std::vector<std::uint32_t>& mask, std::size_t n, const char* where) {
    if (mask.size() > 1 && mask.size() != n) throw EngineError(SBR_ERR_INVALID_ARGUMENT, where);
    if (mask.size() == n && n > 0) return mask;
    return std::vector<std::uint32_t>(n ? n : 1, mask.empty() ? 0u : mask[0]);
}

/// The eligible-ranks call (ELIGIBLE RANKS in sbr_hip.h) over a descriptor's `rows` rows, on the model (set null) or through a set of
/// it: one rank per target, in target order; Err(InvalidPredictionValue) on a non-finite score of a scanned pair.
inline Result<std::vector<std::uint32_t>, PredictionError> eligible_ranks(sbr_model* model, sbr_item_set* set, const sbr_scan_rows& d, std::size_t rows,
                                                                          const std::vector<std::uint64_t>& target_ptr,
                                                                          const std::vector<std::uint32_t>& target_items, const char* where) {
    using R = Result<std::vector<std::uint32_t>, PredictionError>;
    if (target_ptr.size() != rows + 1 || target_ptr.back() < target_ptr.front() || target_ptr.back() > target_items.size())
        throw EngineError(SBR_ERR_INVALID_ARGUMENT, where);
    static const std::uint32_t none = 0;
    std::vector<std::uint32_t> ranks((std::size_t)(target_ptr.back() - target_ptr.front()) + 1);
    const std::uint32_t* items = target_items.empty() ? &none : target_items.data();
    const sbr_status st = set ? sbr_item_set_rank_targets(set, &d, (std::uint64_t)rows, target_ptr.data(), items, ranks.data())
                              : sbr_rank_targets_rows(model, &d, (std::uint64_t)rows, target_ptr.data(), items, ranks.data());
    if (st == SBR_ERR_INVALID_PREDICTION) return R::Err(PredictionError::InvalidPredictionValue);
    check(st, where);
    ranks.pop_back();
    return R::Ok(std::move(ranks));
}

/// The pool a *_capped call scans at, and its refusals ahead of the library: cap < 1, k < 1, pool < k, pool > SBR_RECOMMEND_MAX_K.
inline sbr_cap_args cap_args(const CapArgs& a, std::size_t k, const char* me) {
    const std::uint64_t pool = a.pool ? a.pool : std::min<std::uint64_t>(1024, std::max<std::uint64_t>(64, 4 * (std::uint64_t)k));
    if (a.cap < 1 || k < 1 || pool < k || pool > SBR_RECOMMEND_MAX_K)
        throw EngineError(SBR_ERR_INVALID_ARGUMENT, std::string(me) + ": cap >= 1 and 1 <= k <= pool <= SBR_RECOMMEND_MAX_K");
    return sbr_cap_args{a.cap, (std::uint32_t)pool};
}

/// The rule R(L, cap, k) of CAPPED on one row: ids[0 .. n) in the total order -> the positions of the first k kept entries.
inline std::vector<std::size_t> capped_keep(const std::uint32_t* ids, std::size_t n, const std::vector<std::uint32_t>& groups, std::uint32_t cap,
                                            std::size_t k) {
    std::vector<std::size_t> kept;
    std::unordered_map<std::uint32_t, std::uint32_t> seen;
    for (std::size_t j = 0; j < n && kept.size() < k; ++j) {
        const std::uint32_t g = groups[ids[j]];
        if (g != SBR_NO_GROUP && seen[g]++ >= cap) continue;
        kept.push_back(j);
    }
    return kept;
}

/// Finishes the rows of `r` whose flag is 0, in place.  top(rows, n) is the matching recommend_top* over those rows of the call only
/// (same exclusions, masks and include_seen, score order).  n starts at 4 pool and grows fourfold per round up to the catalogue;
/// a row is done when k are kept or its returned row is shorter than n; the rows of a round go in batches whose rows x n stay
/// within ABOVE_MAX_RESULTS.  False when a top call met a non-finite score.
template <class Top>
inline bool capped_complete(Top top, CappedRecommendations* r, const std::vector<std::uint32_t>& groups, std::uint32_t cap, std::uint32_t pool) {
    std::vector<std::size_t> todo;
    for (std::size_t u = 0; u < r->num_users; ++u)
        if (!r->complete[u]) todo.push_back(u);
    const std::uint64_t num_items = std::max<std::uint64_t>(groups.size(), 1);
    for (std::uint64_t n = 4ull * pool; !todo.empty(); n *= 4) {
        n = std::min(n, num_items);
        const std::size_t per = (std::size_t)std::max<std::uint64_t>(1, ABOVE_MAX_RESULTS / n);
        std::vector<std::size_t> left;
        for (std::size_t b0 = 0; b0 < todo.size(); b0 += per) {
            const std::vector<std::size_t> rows(todo.begin() + (std::ptrdiff_t)b0, todo.begin() + (std::ptrdiff_t)std::min(todo.size(), b0 + per));
            auto res = top(rows, n);
            if (res.is_err()) return false;
            const Above& a = res.unwrap();
            for (std::size_t i = 0; i < rows.size(); ++i) {
                const std::size_t at = (std::size_t)a.ptr[i], len = (std::size_t)a.count(i), u = rows[i];
                const std::vector<std::size_t> kept = capped_keep(a.ids.data() + at, len, groups, cap, r->k);
                if (kept.size() < r->k && len >= n && n < num_items) {
                    left.push_back(u);
                    continue;
                }
                for (std::size_t j = 0; j < r->k; ++j) {
                    r->items[u * r->k + j] = j < kept.size() ? a.ids[at + kept[j]] : 0xFFFFFFFFu;
                    r->scores[u * r->k + j] = j < kept.size() ? a.scores[at + kept[j]] : -std::numeric_limits<float>::infinity();
                }
                r->complete[u] = 1;
            }
        }
        todo.swap(left);
    }
    return true;
}

/// The exclusion CSR of the named rows of a call's (both empty: none).
inline void csr_rows(const std::vector<std::uint64_t>& ptr, const std::vector<std::uint32_t>& items, const std::vector<std::size_t>& rows,
                     std::vector<std::uint64_t>* out_ptr, std::vector<std::uint32_t>* out_items) {
    out_ptr->clear();
    out_items->clear();
    if (ptr.empty()) return;
    out_ptr->push_back(0);
    for (std::size_t r : rows) {
        out_items->insert(out_items->end(), items.begin() + (std::ptrdiff_t)ptr[r], items.begin() + (std::ptrdiff_t)ptr[r + 1]);
        out_ptr->push_back(out_items->size());
    }
}

/// The tag filter of the named rows of a call's: a vector with one mask per row is cut down, anything else applies as it is.
inline TagFilter filter_rows(const TagFilter& f, std::size_t n, const std::vector<std::size_t>& rows) {
    TagFilter out = f;
    for (auto pair : {std::make_pair(&f.any_of, &out.any_of), std::make_pair(&f.none_of, &out.none_of)})
        if (pair.first->size() == n && n > 1) {
            pair.second->clear();
            for (std::size_t r : rows) pair.second->push_back((*pair.first)[r]);
        }
    return out;
}

/// The thresholds of an *_above call over n rows: one value for every row, or one per row; a NaN is refused.
inline std::vector<float> above_thresholds(const std::vector<float>& t, std::size_t n, const char* where) {
    if (t.size() != 1 && t.size() != n) throw EngineError(SBR_ERR_INVALID_ARGUMENT, where);
    std::vector<float> out(n ? n : 1, t.empty() ? 0.0f : t[0]);
    if (t.size() == n) std::copy(t.begin(), t.end(), out.begin());
    for (float x : out)
        if (std::isnan(x)) throw EngineError(SBR_ERR_INVALID_ARGUMENT, where);
    return out;
}
/// What an *_above / *_top method holds its rows to: thresholds (Bar::above) or budgets (Bar::best: the entry point is then the
/// *_top sibling, which takes n where the thresholds stand and out_cuts ahead of out_counts).  fit() makes one value per row
/// (`method` and `unit` word the refusal).
struct Bar {
    std::vector<float> th;          ///< above: one threshold for all rows or one per row
    std::vector<std::uint64_t> n;   ///< top: one budget for all rows or one per row
    std::vector<float> cuts;        ///< top: the entry point's out_cuts
    bool top = false;
    static Bar above(const std::vector<float>& t) {
        Bar b;
        b.th = t;
        return b;
    }
    static Bar best(const std::vector<std::uint64_t>& n) {
        Bar b;
        b.n = n;
        b.top = true;
        return b;
    }
    void fit(std::size_t rows, const char* method, const char* unit) {
        if (!top) {
            th = above_thresholds(th, rows, (std::string(method) + ": one threshold, or one per " + unit + "; no NaN").c_str());
            return;
        }
        if (n.size() != 1 && n.size() != rows) throw EngineError(SBR_ERR_INVALID_ARGUMENT, std::string(method) + ": one n, or one per " + unit);
        if (n.size() != rows || rows == 0) n.assign(rows ? rows : 1, n.empty() ? 0 : n[0]);
        cuts.assign(rows ? rows : 1, 0.0f);
    }
};

/// The shared tail of the *_above / *_top methods.  call(out_counts, out_total, capacity, out_ids, out_scores) invokes the entry
/// point with the method's leading arguments (and, for a budget, bar.n and bar.cuts, which end up in out->cuts).  One call with
/// buffers of max_results entries that are allocated but not touched; a total above max_results throws an EngineError that states the total, never a truncated result.  count_only: the counts alone (ids / scores
/// stay empty), one scan.  Returns the call's status when it is SBR_ERR_INVALID_PREDICTION, for the caller's Result.
template <class Call>
inline sbr_status above_call(Call&& call, std::size_t n, std::uint64_t max_results, AboveOrder order, bool count_only, const char* where,
                             const Bar& bar, Above* out) {
    std::vector<std::uint64_t> counts(n ? n : 1, 0);
    std::uint64_t total = 0;
    std::unique_ptr<std::uint32_t[]> ids;
    std::unique_ptr<float[]> scores;
    if (!count_only) {
        ids.reset(new std::uint32_t[max_results ? max_results : 1]);
        scores.reset(new float[max_results ? max_results : 1]);
    }
    const sbr_status st = call(counts.data(), &total, count_only ? 0 : max_results, ids.get(), scores.get());
    if (st == SBR_ERR_INVALID_PREDICTION) return st;
    check(st, where);
    if (!count_only && total > max_results)
        throw EngineError(SBR_ERR_INVALID_ARGUMENT, std::string(where) + ": " + std::to_string(total) +
                                                        (bar.top ? " pairs make up the rows' best n, above max_results = "
                                                                 : " pairs pass the threshold, above max_results = ") +
                                                        std::to_string(max_results));
    if (bar.top) out->cuts.assign(bar.cuts.begin(), bar.cuts.begin() + (std::ptrdiff_t)n);
    out->ptr.assign(n + 1, 0);
    for (std::size_t i = 0; i < n; ++i) out->ptr[i + 1] = out->ptr[i] + counts[i];
    out->order = AboveOrder::Id;
    if (!count_only) {
        out->ids.assign(ids.get(), ids.get() + total);
        out->scores.assign(scores.get(), scores.get() + total);
        if (order == AboveOrder::Score) out->sort_by_score();
    }
    return SBR_OK;
}

/// A SampleArgs as the struct a *_sampled call takes, over n rows; a non-empty `filter` vector as tag_masks makes it (null: none).
inline sbr_sample_args sample_args(const SampleArgs& a, std::size_t n, const char* where) {
    if (!a.streams.empty() && a.streams.size() != n) throw EngineError(SBR_ERR_INVALID_ARGUMENT, where);
    sbr_sample_args s;
    s.temperature = a.temperature;
    s.seed = a.seed;
    s.streams = a.streams.empty() || n == 0 ? nullptr : a.streams.data();
    return s;
}
inline SampledRecommendations sampled_rows(std::size_t n, std::size_t k) {
    SampledRecommendations r;
    r.num_users = n;
    r.k = k;
    r.items.resize(n * k);
    r.scores.resize(n * k);
    r.keys.resize(n * k);
    return r;
}

inline std::vector<std::uint32_t> narrow(const std::vector<ItemId>& ids) {
    std::vector<std::uint32_t> out(ids.size());
    for (std::size_t i = 0; i < ids.size(); ++i) out[i] = (std::uint32_t)ids[i];
    return out;
}

/// A session store on one model (sbr_sessions_*): `capacity` slots of recurrent state on the device — h, c of the LSTM, s of
/// EWMA — each advanced by the items appended to it, one cell step per item, and read in place by `recommend` /
/// `score_candidates`.  A slot's representation has the bits of `user_representation` of the items appended since its last reset
/// (an empty slot: of the empty history) while they are at most max_sequence_length; beyond that a session keeps the recurrence
/// over everything appended where the windowed call truncates.  After the model's parameters change (`fit`, a restored
/// checkpoint) every call but `reset_all` — and, with a seen-item memory, `replay()` of the whole store, which recomputes every
/// state from the remembered items — throws EngineError(SBR_ERR_INVALID_ARGUMENT) until one of the two re-binds the store.
/// With a seen-item memory (`seen_capacity` > 0) a slot also remembers, on the device, the last seen_capacity items appended
/// to it since its last reset, in append order with repeats; `reset`, `reset_all` and `set_state` empty it, `set_seen` restores it.
/// The recommend calls of such a store exclude each slot's remembered items, united with the caller's lists, as
/// ImplicitSequenceModel::recommend excludes the history; `score_candidates` masks nothing.
/// Obtained from ImplicitSequenceModel::sessions; the model must outlive it.  Movable, not copyable.
class Sessions {
  public:
    Sessions(sbr_model* model, std::size_t capacity, std::size_t embedding_dim, std::size_t seen_capacity = 0) : m_(model), dim_(embedding_dim) {
        if (seen_capacity > SBR_SESSIONS_MAX_SEEN) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions: seen_capacity above SBR_SESSIONS_MAX_SEEN");
        check(sbr_sessions_create_seen(model, (std::uint64_t)capacity, (std::uint32_t)seen_capacity, &h_), "sbr_sessions_create_seen");
    }
    Sessions(const Sessions&) = delete;
    Sessions& operator=(const Sessions&) = delete;
    Sessions(Sessions&& o) noexcept : h_(o.h_), m_(o.m_), dim_(o.dim_) { o.h_ = nullptr; }
    Sessions& operator=(Sessions&& o) noexcept {
        if (this != &o) { release(); h_ = o.h_; m_ = o.m_; dim_ = o.dim_; o.h_ = nullptr; }
        return *this;
    }
    ~Sessions() { release(); }

    std::size_t capacity() const {
        std::uint64_t c = 0;
        check(sbr_sessions_capacity(h_, &c), "sbr_sessions_capacity");
        return (std::size_t)c;
    }
    /// Items each slot remembers (0: a store without seen-item memory).
    std::size_t seen_capacity() const {
        std::uint32_t w = 0;
        check(sbr_sessions_seen_capacity(h_, &w), "sbr_sessions_seen_capacity");
        return (std::size_t)w;
    }
    /// The named slots' remembered items, oldest first, repeats kept (sbr_sessions_get_seen): slot i's are items[ptr[i] .. ptr[i + 1]).
    struct Seen {
        std::vector<std::uint64_t> ptr;
        std::vector<std::uint32_t> items;
    };
    Seen seen(const std::vector<std::uint32_t>& slots) const {
        Seen s;
        s.ptr.assign(slots.size() + 1, 0);
        s.items.resize(slots.size() * seen_capacity() + 1);
        check(sbr_sessions_get_seen(h_, slots.data(), (std::uint64_t)slots.size(), s.ptr.data(), s.items.data()), "sbr_sessions_get_seen");
        s.items.resize((std::size_t)s.ptr.back());
        return s;
    }
    /// Replaces the named slots' memory with the last seen_capacity() items of each list (sbr_sessions_set_seen); after `set_state`
    /// it completes the restore of a checkpoint taken with `get_state` + `seen`.
    void set_seen(const std::vector<std::uint32_t>& slots, const std::vector<std::uint64_t>& ptr, const std::vector<std::uint32_t>& items) {
        if (ptr.size() != slots.size() + 1 || ptr.back() > items.size())
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::set_seen: one item range per slot");
        const std::uint32_t none = 0;
        check(sbr_sessions_set_seen(h_, slots.data(), (std::uint64_t)slots.size(), ptr.data(), items.empty() ? &none : items.data()),
              "sbr_sessions_set_seen");
    }
    void set_seen(const std::vector<std::uint32_t>& slots, const Seen& s) { set_seen(slots, s.ptr, s.items); }
    /// Appends item_ids[item_ptr[i] .. item_ptr[i + 1]), in order, to slot slots[i].
    void append(const std::vector<std::uint32_t>& slots, const std::vector<std::uint64_t>& item_ptr, const std::vector<std::uint32_t>& item_ids) {
        if (item_ptr.size() != slots.size() + 1 || item_ptr.back() > item_ids.size())
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::append: one item range per slot");
        check(sbr_sessions_append(h_, slots.data(), (std::uint64_t)slots.size(), item_ptr.data(), item_ids.data()), "sbr_sessions_append");
    }
    /// One item for each of `slots`.
    void append(const std::vector<std::uint32_t>& slots, const std::vector<std::uint32_t>& one_item_each) {
        std::vector<std::uint64_t> ptr(slots.size() + 1);
        std::iota(ptr.begin(), ptr.end(), (std::uint64_t)0);
        append(slots, ptr, one_item_each);
    }
    std::vector<std::uint64_t> lengths(const std::vector<std::uint32_t>& slots) const {
        std::vector<std::uint64_t> out(slots.size());
        check(sbr_sessions_lengths(h_, slots.data(), (std::uint64_t)slots.size(), out.data()), "sbr_sessions_lengths");
        return out;
    }
    /// Row-major [slots.size()][embedding_dim].
    std::vector<float> representations(const std::vector<std::uint32_t>& slots) const {
        std::vector<float> out(slots.size() * dim_);
        check(sbr_sessions_representations(h_, slots.data(), (std::uint64_t)slots.size(), out.data()), "sbr_sessions_representations");
        return out;
    }
    void reset(const std::vector<std::uint32_t>& slots) { check(sbr_sessions_reset(h_, slots.data(), (std::uint64_t)slots.size()), "sbr_sessions_reset"); }
    /// Every slot emptied and the store re-bound to the model's current parameters.
    void reset_all() { check(sbr_sessions_reset_all(h_), "sbr_sessions_reset_all"); }
    /// Every slot's state recomputed on the device from its remembered items under the model's current parameters, and the store
    /// re-bound to them (sbr_sessions_replay): the second call, beside reset_all, that a stale store accepts.  A slot with an empty
    /// memory becomes empty; one whose memory has wrapped keeps the recurrence over its last seen_capacity() items.  Returns the
    /// number of slots that had a non-empty memory.  A store without seen-item memory refuses the call.
    std::size_t replay() {
        std::uint64_t n = 0;
        check(sbr_sessions_replay(h_, nullptr, 0, &n), "sbr_sessions_replay");
        return (std::size_t)n;
    }
    /// The same for the named slots of a current store (a slot named twice counts once); every other slot keeps its bits.
    std::size_t replay(const std::vector<std::uint32_t>& slots) {
        std::uint64_t n = 0;
        const std::uint32_t none = 0;
        check(sbr_sessions_replay(h_, slots.empty() ? &none : slots.data(), (std::uint64_t)slots.size(), &n), "sbr_sessions_replay");
        return (std::size_t)n;
    }
    /// The k best items of the whole catalogue for each slot's state, read in place (sbr_sessions_recommend): ordered and padded as
    /// ImplicitSequenceModel::recommend's rows.  Slot i's excluded items are excl_items[excl_ptr[i] .. excl_ptr[i + 1]) (both
    /// empty: none), united with the slot's remembered items on a store with seen-item memory unless `include_seen` (which a
    /// store without memory refuses).
    Result<Recommendations, PredictionError> recommend(const std::vector<std::uint32_t>& slots, std::size_t k,
                                                       const std::vector<std::uint64_t>& excl_ptr = {},
                                                       const std::vector<std::uint32_t>& excl_items = {}, bool include_seen = false) const {
        if (k < 1 || k > SBR_RECOMMEND_MAX_K) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::recommend: k outside 1..SBR_RECOMMEND_MAX_K");
        if (!excl_ptr.empty() && (excl_ptr.size() != slots.size() + 1 || excl_ptr.back() > excl_items.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::recommend: one exclusion range per slot");
        Recommendations r;
        r.num_users = slots.size();
        r.k = k;
        r.items.resize(r.num_users * k);
        r.scores.resize(r.num_users * k);
        const std::uint32_t none = 0;
        const sbr_status st = sbr_sessions_recommend(h_, slots.data(), (std::uint64_t)slots.size(), (std::uint32_t)k,
                                                     excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                     excl_ptr.empty() ? nullptr : (excl_items.empty() ? &none : excl_items.data()),
                                                     include_seen ? SBR_RECOMMEND_INCLUDE_HISTORY : 0u, r.items.data(), r.scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Recommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_sessions_recommend");
        return Result<Recommendations, PredictionError>::Ok(std::move(r));
    }
    /// `recommend` without the near-duplicates (sbr_sessions_recommend_diverse): from each slot's `pool` best items, k picked
    /// greedily by maximal marginal relevance, as ImplicitSequenceModel::recommend_diverse picks them; rows in pick order.
    Result<Recommendations, PredictionError> recommend_diverse(const std::vector<std::uint32_t>& slots, std::size_t k, std::size_t pool,
                                                               float trade_off = 0.5f, Similarity metric = Similarity::Cosine,
                                                               const std::vector<std::uint64_t>& excl_ptr = {},
                                                               const std::vector<std::uint32_t>& excl_items = {}) const {
        if (k < 1 || pool < k || pool > SBR_DIVERSE_MAX_POOL)
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::recommend_diverse: 1 <= k <= pool <= SBR_DIVERSE_MAX_POOL");
        if (!excl_ptr.empty() && (excl_ptr.size() != slots.size() + 1 || excl_ptr.back() > excl_items.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::recommend_diverse: one exclusion range per slot");
        Recommendations r;
        r.num_users = slots.size();
        r.k = k;
        r.items.resize(r.num_users * k);
        r.scores.resize(r.num_users * k);
        const std::uint32_t none = 0;
        const sbr_status st = sbr_sessions_recommend_diverse(h_, slots.data(), (std::uint64_t)slots.size(), (std::uint32_t)k, (std::uint32_t)pool,
                                                             trade_off, (std::uint32_t)metric, excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                             excl_ptr.empty() ? nullptr : (excl_items.empty() ? &none : excl_items.data()),
                                                             r.items.data(), r.scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Recommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_sessions_recommend_diverse");
        return Result<Recommendations, PredictionError>::Ok(std::move(r));
    }
    /// `recommend` under a tag filter, one mask pair per slot of the call (sbr_sessions_recommend_filtered).
    Result<Recommendations, PredictionError> recommend_filtered(const std::vector<std::uint32_t>& slots, std::size_t k, const TagFilter& filter,
                                                       const std::vector<std::uint64_t>& excl_ptr = {},
                                                       const std::vector<std::uint32_t>& excl_items = {}, bool include_seen = false) const {
        if (k < 1 || k > SBR_RECOMMEND_MAX_K) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::recommend: k outside 1..SBR_RECOMMEND_MAX_K");
        if (!excl_ptr.empty() && (excl_ptr.size() != slots.size() + 1 || excl_ptr.back() > excl_items.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::recommend: one exclusion range per slot");
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, slots.size(), "Sessions::recommend: one any_of mask per slot");
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, slots.size(), "Sessions::recommend: one none_of mask per slot");
        Recommendations r;
        r.num_users = slots.size();
        r.k = k;
        r.items.resize(r.num_users * k);
        r.scores.resize(r.num_users * k);
        const std::uint32_t none = 0;
        const sbr_status st = sbr_sessions_recommend_filtered(h_, slots.data(), (std::uint64_t)slots.size(), (std::uint32_t)k,
                                                              excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                              excl_ptr.empty() ? nullptr : (excl_items.empty() ? &none : excl_items.data()),
                                                              include_seen ? SBR_RECOMMEND_INCLUDE_HISTORY : 0u, any.data(), none_of.data(),
                                                              r.items.data(), r.scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Recommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_sessions_recommend_filtered");
        return Result<Recommendations, PredictionError>::Ok(std::move(r));
    }
    /// `recommend` with a dice (sbr_sessions_recommend_sampled): k draws without replacement from softmax(score / temperature) over
    /// what each slot may see — exclusion lists, the seen-item memory unless include_seen, and `filter` unless both its vectors are
    /// empty.  Streams default to the slot ids.
    Result<SampledRecommendations, PredictionError> recommend_sampled(const std::vector<std::uint32_t>& slots, std::size_t k,
                                                                      const SampleArgs& sample, const TagFilter& filter = {},
                                                                      const std::vector<std::uint64_t>& excl_ptr = {},
                                                                      const std::vector<std::uint32_t>& excl_items = {},
                                                                      bool include_seen = false) const {
        if (k < 1 || k > SBR_RECOMMEND_MAX_K) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::recommend_sampled: k outside 1..SBR_RECOMMEND_MAX_K");
        if (!excl_ptr.empty() && (excl_ptr.size() != slots.size() + 1 || excl_ptr.back() > excl_items.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::recommend_sampled: one exclusion range per slot");
        const bool filtered = !filter.any_of.empty() || !filter.none_of.empty();
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, slots.size(), "Sessions::recommend_sampled: one any_of mask per slot");
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, slots.size(), "Sessions::recommend_sampled: one none_of mask per slot");
        const sbr_sample_args sa = sample_args(sample, slots.size(), "Sessions::recommend_sampled: one stream per slot");
        SampledRecommendations r = sampled_rows(slots.size(), k);
        const std::uint32_t none = 0;
        const sbr_status st = sbr_sessions_recommend_sampled(h_, slots.data(), (std::uint64_t)slots.size(), (std::uint32_t)k,
                                                             excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                             excl_ptr.empty() ? nullptr : (excl_items.empty() ? &none : excl_items.data()),
                                                             include_seen ? SBR_RECOMMEND_INCLUDE_HISTORY : 0u, &sa,
                                                             filtered ? any.data() : nullptr, filtered ? none_of.data() : nullptr, r.items.data(),
                                                             r.scores.data(), r.keys.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<SampledRecommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_sessions_recommend_sampled");
        return Result<SampledRecommendations, PredictionError>::Ok(std::move(r));
    }
    /// The exact fixed-point mass of softmax(score / temperature) over what each slot may see (sbr_sessions_log_partition), with
    /// `recommend_sampled`'s eligibility: the propensities of its draws are `Partition::slate_log_prob` of their scores.
    Result<Partition, PredictionError> log_partition(const std::vector<std::uint32_t>& slots, float temperature, const TagFilter& filter = {},
                                                     const std::vector<std::uint64_t>& excl_ptr = {},
                                                     const std::vector<std::uint32_t>& excl_items = {}, bool include_seen = false) const {
        if (!excl_ptr.empty() && (excl_ptr.size() != slots.size() + 1 || excl_ptr.back() > excl_items.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::log_partition: one exclusion range per slot");
        const bool filtered = !filter.any_of.empty() || !filter.none_of.empty();
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, slots.size(), "Sessions::log_partition: one any_of mask per slot");
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, slots.size(), "Sessions::log_partition: one none_of mask per slot");
        Partition r;
        r.temperature = temperature;
        r.shift.resize(slots.size());
        r.mass.resize(slots.size());
        const std::uint32_t none = 0;
        const sbr_status st = sbr_sessions_log_partition(h_, slots.data(), (std::uint64_t)slots.size(), excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                         excl_ptr.empty() ? nullptr : (excl_items.empty() ? &none : excl_items.data()),
                                                         include_seen ? SBR_RECOMMEND_INCLUDE_HISTORY : 0u, temperature,
                                                         filtered ? any.data() : nullptr, filtered ? none_of.data() : nullptr, r.shift.data(),
                                                         r.mass.data(), &r.frac_bits);
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Partition, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_sessions_log_partition");
        return Result<Partition, PredictionError>::Ok(std::move(r));
    }
    /// Each slot's next a.steps items, each chosen given the ones before it, picked and fed back on the device
    /// (sbr_sessions_rollout): what a host loop of recommend(k = 1) + append + a rebuilt exclusion list returns, WITHOUT writing the
    /// store — a rollout is hypothetical; append its rows to make it happen.  Step j picks among what `recommend` would offer at
    /// call time minus picks 0 .. j - 1 (with allow_repeats: the picks stay eligible), scored against the state after those picks.
    /// The insert of a pick into its row's exclusion list costs O(list) per step; steps <= SBR_ROLLOUT_MAX_STEPS.
    Result<Rollout, PredictionError> rollout(const std::vector<std::uint32_t>& slots, const RolloutArgs& a) const { return rollout_in(nullptr, slots, a); }
    /// rollout, or (set non-null) the same within an item set: sbr_item_set_rollout through a store descriptor of these slots
    /// (ItemSet::OnSessions::rollout).
    Result<Rollout, PredictionError> rollout_in(sbr_item_set* set, const std::vector<std::uint32_t>& slots, const RolloutArgs& a) const {
        using R = Result<Rollout, PredictionError>;
        if (a.steps < 1 || a.steps > SBR_ROLLOUT_MAX_STEPS) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::rollout: steps outside 1..SBR_ROLLOUT_MAX_STEPS");
        if (!a.excl_ptr.empty() && (a.excl_ptr.size() != slots.size() + 1 || a.excl_ptr.back() > a.excl_items.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::rollout: one exclusion range per slot");
        const std::size_t n = slots.size(), cells = n * a.steps;
        const bool filtered = !a.filter.any_of.empty() || !a.filter.none_of.empty();
        const std::vector<std::uint32_t> any = tag_masks(a.filter.any_of, n, "Sessions::rollout: one any_of mask per slot");
        const std::vector<std::uint32_t> none_of = tag_masks(a.filter.none_of, n, "Sessions::rollout: one none_of mask per slot");
        sbr_rollout_args ra{};
        ra.steps = (std::uint32_t)a.steps;
        ra.flags = (a.sample ? SBR_ROLLOUT_SAMPLE : 0u) | (a.allow_repeats ? SBR_ROLLOUT_ALLOW_REPEATS : 0u) |
                   (a.include_seen ? SBR_ROLLOUT_INCLUDE_SEEN : 0u);
        ra.sample = sample_args(a.noise, n, "Sessions::rollout: one stream per slot");
        Rollout r;
        r.num_rows = n;
        r.steps = a.steps;
        r.items.resize(cells);
        r.scores.resize(cells);
        r.lengths.resize(n);
        if (a.sample) r.keys.resize(cells);
        if (a.log_prob) {
            r.partition.temperature = a.noise.temperature;
            r.partition.shift.resize(cells);
            r.partition.mass.resize(cells);
        }
        if (a.final_state) {
            r.h.resize(n * dim_);
            if (a.lstm) r.c.resize(n * dim_);
        }
        const std::uint32_t none = 0;
        const sbr_scan_rows d = store_rows(slots, a.excl_ptr, a.excl_items, filtered ? any.data() : nullptr, filtered ? none_of.data() : nullptr);
        const sbr_status st =
            set ? sbr_item_set_rollout(set, &d, (std::uint64_t)n, &ra, r.items.data(), r.scores.data(), a.sample ? r.keys.data() : nullptr, r.lengths.data(),
                                       a.log_prob ? r.partition.shift.data() : nullptr, a.log_prob ? r.partition.mass.data() : nullptr,
                                       a.log_prob ? &r.partition.frac_bits : nullptr, a.final_state ? r.h.data() : nullptr,
                                       a.final_state && a.lstm ? r.c.data() : nullptr)
                : sbr_sessions_rollout(h_, slots.data(), (std::uint64_t)n, &ra, a.excl_ptr.empty() ? nullptr : a.excl_ptr.data(),
                                       a.excl_ptr.empty() ? nullptr : (a.excl_items.empty() ? &none : a.excl_items.data()),
                                       filtered ? any.data() : nullptr, filtered ? none_of.data() : nullptr, r.items.data(),
                                       r.scores.data(), a.sample ? r.keys.data() : nullptr, r.lengths.data(),
                                       a.log_prob ? r.partition.shift.data() : nullptr, a.log_prob ? r.partition.mass.data() : nullptr,
                                       a.log_prob ? &r.partition.frac_bits : nullptr, a.final_state ? r.h.data() : nullptr,
                                       a.final_state && a.lstm ? r.c.data() : nullptr);
        if (st == SBR_ERR_INVALID_PREDICTION) return R::Err(PredictionError::InvalidPredictionValue);
        check(st, set ? "sbr_item_set_rollout" : "sbr_sessions_rollout");
        if (a.log_prob) { /* one partition row per (row, step): the library's one host statement of the weights */
            r.log_prob = r.partition.log_prob(r.scores);
            for (std::size_t p = 0; p < cells; ++p)
                if (r.items[p] == 0xFFFFFFFFu) r.log_prob[p] = std::numeric_limits<double>::quiet_NaN();
        }
        if (a.final_state) {
            r.len.resize(n);
            check(sbr_sessions_lengths(h_, slots.data(), (std::uint64_t)n, r.len.data()), "sbr_sessions_lengths");
            for (std::size_t i = 0; i < n; ++i) r.len[i] += r.lengths[i];
        }
        return R::Ok(std::move(r));
    }
    /// The a.width most likely next-a.steps continuations of each slot, searched on the device (sbr_sessions_beam_search; greedy,
    /// deterministic) WITHOUT writing the store.  Eligibility is rollout's, minus each beam's own path unless allow_repeats; each
    /// live beam offers its first width eligible items per step, and the row keeps the width best offers by (cumulative f32 lp
    /// descending, parent beam ascending, offer position ascending).  width <= SBR_BEAM_MAX_WIDTH, steps <= SBR_ROLLOUT_MAX_STEPS.
    Result<Beams, PredictionError> beam_search(const std::vector<std::uint32_t>& slots, const BeamArgs& a) const { return beam_search_in(nullptr, slots, a); }
    /// beam_search, or (set non-null) the same within an item set: sbr_item_set_beam_search through a store descriptor of these
    /// slots (ItemSet::OnSessions::beam_search).
    Result<Beams, PredictionError> beam_search_in(sbr_item_set* set, const std::vector<std::uint32_t>& slots, const BeamArgs& a) const {
        using R = Result<Beams, PredictionError>;
        if (a.steps < 1 || a.steps > SBR_ROLLOUT_MAX_STEPS) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::beam_search: steps outside 1..SBR_ROLLOUT_MAX_STEPS");
        if (a.width < 1 || a.width > SBR_BEAM_MAX_WIDTH) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::beam_search: width outside 1..SBR_BEAM_MAX_WIDTH");
        if (!a.excl_ptr.empty() && (a.excl_ptr.size() != slots.size() + 1 || a.excl_ptr.back() > a.excl_items.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::beam_search: one exclusion range per slot");
        const std::size_t n = slots.size(), cells = n * a.width * a.steps;
        const bool filtered = !a.filter.any_of.empty() || !a.filter.none_of.empty();
        const std::vector<std::uint32_t> any = tag_masks(a.filter.any_of, n, "Sessions::beam_search: one any_of mask per slot");
        const std::vector<std::uint32_t> none_of = tag_masks(a.filter.none_of, n, "Sessions::beam_search: one none_of mask per slot");
        sbr_beam_args ba{};
        ba.steps = (std::uint32_t)a.steps;
        ba.width = (std::uint32_t)a.width;
        ba.flags = (a.allow_repeats ? SBR_ROLLOUT_ALLOW_REPEATS : 0u) | (a.include_seen ? SBR_ROLLOUT_INCLUDE_SEEN : 0u);
        ba.temperature = a.temperature;
        Beams r;
        r.num_rows = n;
        r.width = a.width;
        r.steps = a.steps;
        r.items.resize(cells);
        r.scores.resize(cells);
        r.step_lp.resize(cells);
        r.cum.resize(n * a.width);
        r.lengths.resize(n);
        r.beams.resize(n);
        if (a.partitions) {
            r.partition.temperature = a.temperature;
            r.partition.shift.resize(cells);
            r.partition.mass.resize(cells);
        }
        const std::uint32_t none = 0;
        const sbr_scan_rows d = store_rows(slots, a.excl_ptr, a.excl_items, filtered ? any.data() : nullptr, filtered ? none_of.data() : nullptr);
        const sbr_status st =
            set ? sbr_item_set_beam_search(set, &d, (std::uint64_t)n, &ba, r.items.data(), r.scores.data(), r.step_lp.data(), r.cum.data(),
                                           r.lengths.data(), r.beams.data(), a.partitions ? r.partition.shift.data() : nullptr,
                                           a.partitions ? r.partition.mass.data() : nullptr, a.partitions ? &r.partition.frac_bits : nullptr)
                : sbr_sessions_beam_search(h_, slots.data(), (std::uint64_t)n, &ba, a.excl_ptr.empty() ? nullptr : a.excl_ptr.data(),
                                           a.excl_ptr.empty() ? nullptr : (a.excl_items.empty() ? &none : a.excl_items.data()),
                                           filtered ? any.data() : nullptr, filtered ? none_of.data() : nullptr, r.items.data(),
                                           r.scores.data(), r.step_lp.data(), r.cum.data(), r.lengths.data(), r.beams.data(),
                                           a.partitions ? r.partition.shift.data() : nullptr, a.partitions ? r.partition.mass.data() : nullptr,
                                           a.partitions ? &r.partition.frac_bits : nullptr);
        if (st == SBR_ERR_INVALID_PREDICTION) return R::Err(PredictionError::InvalidPredictionValue);
        check(st, set ? "sbr_item_set_beam_search" : "sbr_sessions_beam_search");
        return R::Ok(std::move(r));
    }
    /// The store descriptor (struct sbr_scan_rows) of these slots with the caller's lists and masks, flags 0: the rows of
    /// rollout_in / beam_search_in through a set.  The arrays must outlive the call.
    sbr_scan_rows store_rows(const std::vector<std::uint32_t>& slots, const std::vector<std::uint64_t>& excl_ptr,
                             const std::vector<std::uint32_t>& excl_items, const std::uint32_t* any_of, const std::uint32_t* none_of) const {
        static const std::uint32_t none = 0;
        sbr_scan_rows d{};
        d.store = h_;
        d.slots = slots.empty() ? &none : slots.data();
        if (!excl_ptr.empty()) { d.excl_ptr = excl_ptr.data(); d.excl_items = excl_items.empty() ? &none : excl_items.data(); }
        d.any_of = any_of;
        d.none_of = none_of;
        return d;
    }
    /// `recommend_diverse` under a tag filter: the pool holds eligible items only (sbr_sessions_recommend_diverse_filtered).
    Result<Recommendations, PredictionError> recommend_diverse_filtered(const std::vector<std::uint32_t>& slots, std::size_t k, std::size_t pool,
                                                               float trade_off, Similarity metric, const TagFilter& filter,
                                                               const std::vector<std::uint64_t>& excl_ptr = {},
                                                               const std::vector<std::uint32_t>& excl_items = {}) const {
        if (k < 1 || pool < k || pool > SBR_DIVERSE_MAX_POOL)
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::recommend_diverse: 1 <= k <= pool <= SBR_DIVERSE_MAX_POOL");
        if (!excl_ptr.empty() && (excl_ptr.size() != slots.size() + 1 || excl_ptr.back() > excl_items.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::recommend_diverse: one exclusion range per slot");
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, slots.size(), "Sessions::recommend_diverse: one any_of mask per slot");
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, slots.size(), "Sessions::recommend_diverse: one none_of mask per slot");
        Recommendations r;
        r.num_users = slots.size();
        r.k = k;
        r.items.resize(r.num_users * k);
        r.scores.resize(r.num_users * k);
        const std::uint32_t none = 0;
        const sbr_status st = sbr_sessions_recommend_diverse_filtered(
            h_, slots.data(), (std::uint64_t)slots.size(), (std::uint32_t)k, (std::uint32_t)pool, trade_off, (std::uint32_t)metric,
            excl_ptr.empty() ? nullptr : excl_ptr.data(), excl_ptr.empty() ? nullptr : (excl_items.empty() ? &none : excl_items.data()),
            any.data(), none_of.data(), r.items.data(), r.scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Recommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_sessions_recommend_diverse_filtered");
        return Result<Recommendations, PredictionError>::Ok(std::move(r));
    }
    /// Which sessions for this item (sbr_sessions_audience): row j of the result holds, for query item items[j], the k candidate
    /// slots whose states score it highest — `items` of the result are SLOT ids, the scores have the bits of `score_candidates`,
    /// score descending, ties to the lower slot, short rows padded with (0xFFFFFFFF, -inf).  Candidates: `slots`, or with
    /// `all_live_slots` (and `slots` empty) every slot of length > 0.  Query j's excluded slots are excl_slots[excl_ptr[j] ..
    /// excl_ptr[j + 1]) (both empty: none); on a store with seen-item memory a candidate whose memory holds the query item is left
    /// out as well unless `include_seen` (which a store without memory refuses).
    Result<Recommendations, PredictionError> audience(const std::vector<std::uint32_t>& items, std::size_t k,
                                                      const std::vector<std::uint32_t>& slots = {}, bool all_live_slots = true,
                                                      const std::vector<std::uint64_t>& excl_ptr = {},
                                                      const std::vector<std::uint32_t>& excl_slots = {}, bool include_seen = false) const {
        if (k < 1 || k > SBR_RECOMMEND_MAX_K) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::audience: k outside 1..SBR_RECOMMEND_MAX_K");
        if (!excl_ptr.empty() && (excl_ptr.size() != items.size() + 1 || excl_ptr.back() > excl_slots.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::audience: one exclusion range per query");
        if (all_live_slots && !slots.empty()) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::audience: slots together with all_live_slots");
        Recommendations r;
        r.num_users = items.size();
        r.k = k;
        r.items.resize(r.num_users * k);
        r.scores.resize(r.num_users * k);
        const std::uint32_t none = 0;
        const sbr_status st = sbr_sessions_audience(h_, items.data(), (std::uint64_t)items.size(), (std::uint32_t)k,
                                                    all_live_slots ? nullptr : (slots.empty() ? &none : slots.data()),
                                                    (std::uint64_t)slots.size(), excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                    excl_ptr.empty() ? nullptr : (excl_slots.empty() ? &none : excl_slots.data()),
                                                    include_seen ? SBR_RECOMMEND_INCLUDE_HISTORY : 0u, r.items.data(), r.scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Recommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_sessions_audience");
        return Result<Recommendations, PredictionError>::Ok(std::move(r));
    }
  private:
    /// The body the *_above and *_top forms share: `me` names the calling method in refusals, `bar` holds the thresholds or the
    /// budgets.
    Result<Above, PredictionError> recommend_bar(const char* me, const std::vector<std::uint32_t>& slots, detail::Bar bar,
                                                   const TagFilter& filter, const std::vector<std::uint64_t>& excl_ptr,
                                                   const std::vector<std::uint32_t>& excl_items, bool include_seen,
                                                   std::uint64_t max_results, AboveOrder order,
                                                   bool count_only) const {
        if (!excl_ptr.empty() && (excl_ptr.size() != slots.size() + 1 || excl_ptr.back() > excl_items.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, (std::string(me) + ": one exclusion range per slot").c_str());
        const bool filtered = !filter.any_of.empty() || !filter.none_of.empty();
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, slots.size(), (std::string(me) + ": one any_of mask per slot").c_str());
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, slots.size(), (std::string(me) + ": one none_of mask per slot").c_str());
        bar.fit(slots.size(), me, "slot");
        const std::uint32_t none = 0;
        Above r;
        const sbr_status st = detail::above_call(
            [&](std::uint64_t* counts, std::uint64_t* total, std::uint64_t cap, std::uint32_t* ids, float* scores) {
                if (bar.top)
                    return sbr_sessions_recommend_top(h_, slots.data(), (std::uint64_t)slots.size(), bar.n.data(), excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                        excl_ptr.empty() ? nullptr : (excl_items.empty() ? &none : excl_items.data()),
                                                        include_seen ? SBR_RECOMMEND_INCLUDE_HISTORY : 0u, filtered ? any.data() : nullptr,
                                                        filtered ? none_of.data() : nullptr, bar.cuts.data(), counts, total, cap, ids, scores);
                return sbr_sessions_recommend_above(h_, slots.data(), (std::uint64_t)slots.size(), bar.th.data(), excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                    excl_ptr.empty() ? nullptr : (excl_items.empty() ? &none : excl_items.data()),
                                                    include_seen ? SBR_RECOMMEND_INCLUDE_HISTORY : 0u, filtered ? any.data() : nullptr,
                                                    filtered ? none_of.data() : nullptr, counts, total, cap, ids, scores);
            },
            slots.size(), max_results, order, count_only, bar.top ? "sbr_sessions_recommend_top" : "sbr_sessions_recommend_above", bar, &r);
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Above, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        return Result<Above, PredictionError>::Ok(std::move(r));
    }
  public:
    /// `recommend` without a k (sbr_sessions_recommend_above): for each slot EVERY eligible item whose score is >= its threshold —
    /// `thresholds`: one value for all slots or one per slot; ties at the bar all pass, -inf returns every eligible item.  Eligibility
    /// (the lists, the filter, the seen-item memory unless `include_seen`) is `recommend`'s.  More than `max_results` pairs throw an
    /// EngineError that states the total; `count_above` costs one scan and says how many to expect.
    Result<Above, PredictionError> recommend_above(const std::vector<std::uint32_t>& slots, const std::vector<float>& thresholds,
                                                   const TagFilter& filter = {}, const std::vector<std::uint64_t>& excl_ptr = {},
                                                   const std::vector<std::uint32_t>& excl_items = {}, bool include_seen = false,
                                                   std::uint64_t max_results = ABOVE_MAX_RESULTS, AboveOrder order = AboveOrder::Score,
                                                   bool count_only = false) const {
        return recommend_bar("Sessions::recommend_above",
                             slots, detail::Bar::above(thresholds), filter, excl_ptr, excl_items, include_seen, max_results, order, count_only);
    }
    /// `recommend` with a budget in place of k (sbr_sessions_recommend_top): each slot's exact best n eligible items — `n`: one value
    /// for all slots or one per slot, any size (no SBR_RECOMMEND_MAX_K); an Above with `cuts`.  count_only: the select alone — cuts
    /// and counts, no pair.  Everything else as `recommend_above`.
    Result<Above, PredictionError> recommend_top(const std::vector<std::uint32_t>& slots, const std::vector<std::uint64_t>& n,
                                                 const TagFilter& filter = {}, const std::vector<std::uint64_t>& excl_ptr = {},
                                                 const std::vector<std::uint32_t>& excl_items = {}, bool include_seen = false,
                                                 std::uint64_t max_results = ABOVE_MAX_RESULTS, AboveOrder order = AboveOrder::Score,
                                                 bool count_only = false) const {
        return recommend_bar("Sessions::recommend_top",
                             slots, detail::Bar::best(n), filter, excl_ptr, excl_items, include_seen, max_results, order, count_only);
    }
    /// `recommend` under the group cap (sbr_sessions_recommend_capped; CAPPED in sbr_hip.h): at most cap.cap items of one item group
    /// per row, with the seen-item memory excluded exactly as in `recommend`.  `groups`: the model's group words on the host
    /// (ImplicitSequenceModel::item_groups), which the completion of cap.exact applies the rule with.
    Result<CappedRecommendations, PredictionError> recommend_capped(const std::vector<std::uint32_t>& slots, std::size_t k, const CapArgs& cap,
                                                                    const std::vector<std::uint32_t>& groups, const TagFilter& filter = {},
                                                                    const std::vector<std::uint64_t>& excl_ptr = {},
                                                                    const std::vector<std::uint32_t>& excl_items = {},
                                                                    bool include_seen = false) const {
        const sbr_cap_args ca = detail::cap_args(cap, k, "Sessions::recommend_capped");
        const std::size_t n = slots.size();
        if (!excl_ptr.empty() && (excl_ptr.size() != n + 1 || excl_ptr.back() > excl_items.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::recommend_capped: one exclusion range per slot");
        const bool filtered = !filter.any_of.empty() || !filter.none_of.empty();
        const std::vector<std::uint32_t> any = detail::tag_masks(filter.any_of, n, "Sessions::recommend_capped: one any_of mask per slot");
        const std::vector<std::uint32_t> none_of = detail::tag_masks(filter.none_of, n, "Sessions::recommend_capped: one none_of mask per slot");
        CappedRecommendations r;
        r.num_users = n;
        r.k = k;
        r.items.resize(n * k);
        r.scores.resize(n * k);
        r.complete.assign(n ? n : 1, 0);
        const std::uint32_t none = 0;
        const sbr_status st = sbr_sessions_recommend_capped(h_, n ? slots.data() : &none, (std::uint64_t)n, (std::uint32_t)k,
                                                            excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                            excl_ptr.empty() ? nullptr : (excl_items.empty() ? &none : excl_items.data()),
                                                            include_seen ? SBR_RECOMMEND_INCLUDE_HISTORY : 0u, &ca, filtered ? any.data() : nullptr,
                                                            filtered ? none_of.data() : nullptr, r.items.data(), r.scores.data(), r.complete.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<CappedRecommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_sessions_recommend_capped");
        r.complete.resize(n);
        if (cap.exact) {
            const bool ok = detail::capped_complete(
                [&](const std::vector<std::size_t>& rows, std::uint64_t top_n) {
                    std::vector<std::uint32_t> sl;
                    for (std::size_t i : rows) sl.push_back(slots[i]);
                    std::vector<std::uint64_t> ep;
                    std::vector<std::uint32_t> ei;
                    detail::csr_rows(excl_ptr, excl_items, rows, &ep, &ei);
                    return recommend_top(sl, {top_n}, detail::filter_rows(filter, n, rows), ep, ei, include_seen);
                },
                &r, groups, ca.cap, ca.pool);
            if (!ok) return Result<CappedRecommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        }
        return Result<CappedRecommendations, PredictionError>::Ok(std::move(r));
    }
    /// The rows' counts of `recommend_above` (its `ptr`; `ids` / `scores` stay empty) without writing any pair: one scan.
    Result<Above, PredictionError> count_above(const std::vector<std::uint32_t>& slots, const std::vector<float>& thresholds,
                                               const TagFilter& filter = {}, const std::vector<std::uint64_t>& excl_ptr = {},
                                               const std::vector<std::uint32_t>& excl_items = {}, bool include_seen = false) const {
        return recommend_above(slots, thresholds, filter, excl_ptr, excl_items, include_seen, 0, AboveOrder::Id, true);
    }
  private:
    /// The body the *_above and *_top forms share: `me` names the calling method in refusals, `bar` holds the thresholds or the
    /// budgets.
    Result<Above, PredictionError> audience_bar(const char* me, const std::vector<std::uint32_t>& items, detail::Bar bar,
                                                  const std::vector<std::uint32_t>& slots, bool all_live_slots,
                                                  const std::vector<std::uint64_t>& excl_ptr, const std::vector<std::uint32_t>& excl_slots,
                                                  bool include_seen, std::uint64_t max_results,
                                                  AboveOrder order, bool count_only) const {
        if (!excl_ptr.empty() && (excl_ptr.size() != items.size() + 1 || excl_ptr.back() > excl_slots.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, (std::string(me) + ": one exclusion range per query").c_str());
        if (all_live_slots && !slots.empty()) throw EngineError(SBR_ERR_INVALID_ARGUMENT, (std::string(me) + ": slots together with all_live_slots").c_str());
        bar.fit(items.size(), me, "query");
        const std::uint32_t none = 0;
        Above r;
        const sbr_status st = detail::above_call(
            [&](std::uint64_t* counts, std::uint64_t* total, std::uint64_t cap, std::uint32_t* ids, float* scores) {
                if (bar.top)
                    return sbr_sessions_audience_top(h_, items.data(), (std::uint64_t)items.size(), bar.n.data(),
                                                       all_live_slots ? nullptr : (slots.empty() ? &none : slots.data()), (std::uint64_t)slots.size(),
                                                       excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                       excl_ptr.empty() ? nullptr : (excl_slots.empty() ? &none : excl_slots.data()),
                                                       include_seen ? SBR_RECOMMEND_INCLUDE_HISTORY : 0u, bar.cuts.data(), counts, total, cap, ids, scores);
                return sbr_sessions_audience_above(h_, items.data(), (std::uint64_t)items.size(), bar.th.data(),
                                                   all_live_slots ? nullptr : (slots.empty() ? &none : slots.data()), (std::uint64_t)slots.size(),
                                                   excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                   excl_ptr.empty() ? nullptr : (excl_slots.empty() ? &none : excl_slots.data()),
                                                   include_seen ? SBR_RECOMMEND_INCLUDE_HISTORY : 0u, counts, total, cap, ids, scores);
            },
            items.size(), max_results, order, count_only, bar.top ? "sbr_sessions_audience_top" : "sbr_sessions_audience_above", bar, &r);
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Above, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        return Result<Above, PredictionError>::Ok(std::move(r));
    }
  public:
    /// Who should hear about this item (sbr_sessions_audience_above): for each query item EVERY candidate slot whose state scores it
    /// >= its threshold (`thresholds`: one for all queries or one per query) — `ids` of the result are SLOT ids.  Candidates, the
    /// lists and the seen-item memory as in `audience`; no k.
    Result<Above, PredictionError> audience_above(const std::vector<std::uint32_t>& items, const std::vector<float>& thresholds,
                                                  const std::vector<std::uint32_t>& slots = {}, bool all_live_slots = true,
                                                  const std::vector<std::uint64_t>& excl_ptr = {}, const std::vector<std::uint32_t>& excl_slots = {},
                                                  bool include_seen = false, std::uint64_t max_results = ABOVE_MAX_RESULTS,
                                                  AboveOrder order = AboveOrder::Score, bool count_only = false) const {
        return audience_bar("Sessions::audience_above",
                            items, detail::Bar::above(thresholds), slots, all_live_slots, excl_ptr, excl_slots, include_seen, max_results, order,
                            count_only);
    }
    /// We can reach n people: which n (sbr_sessions_audience_top)?  For each query item its exact best n candidate slots — `n`: one
    /// value for all queries or one per query, any size; an Above with `cuts`, SLOT ids.  count_only: the select alone.
    Result<Above, PredictionError> audience_top(const std::vector<std::uint32_t>& items, const std::vector<std::uint64_t>& n,
                                                const std::vector<std::uint32_t>& slots = {}, bool all_live_slots = true,
                                                const std::vector<std::uint64_t>& excl_ptr = {}, const std::vector<std::uint32_t>& excl_slots = {},
                                                bool include_seen = false, std::uint64_t max_results = ABOVE_MAX_RESULTS,
                                                AboveOrder order = AboveOrder::Score, bool count_only = false) const {
        return audience_bar("Sessions::audience_top",
                            items, detail::Bar::best(n), slots, all_live_slots, excl_ptr, excl_slots, include_seen, max_results, order, count_only);
    }
    /// The rows' counts of `audience_above` without writing any pair: one scan.
    Result<Above, PredictionError> count_audience_above(const std::vector<std::uint32_t>& items, const std::vector<float>& thresholds,
                                                        const std::vector<std::uint32_t>& slots = {}, bool all_live_slots = true,
                                                        const std::vector<std::uint64_t>& excl_ptr = {},
                                                        const std::vector<std::uint32_t>& excl_slots = {}, bool include_seen = false) const {
        return audience_above(items, thresholds, slots, all_live_slots, excl_ptr, excl_slots, include_seen, 0, AboveOrder::Id, true);
    }
    /// One score per candidate, in candidate order, slot i's candidates cand_items[cand_ptr[i] .. cand_ptr[i + 1]) (sbr_sessions_score_candidates).
    Result<std::vector<float>, PredictionError> score_candidates(const std::vector<std::uint32_t>& slots, const std::vector<std::uint64_t>& cand_ptr,
                                                                 const std::vector<std::uint32_t>& cand_items) const {
        using R = Result<std::vector<float>, PredictionError>;
        if (cand_ptr.size() != slots.size() + 1 || cand_ptr.back() < cand_ptr.front() || cand_ptr.back() > cand_items.size())
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::score_candidates: one candidate range per slot");
        std::vector<float> scores(cand_ptr.back() - cand_ptr.front());
        const sbr_status st = sbr_sessions_score_candidates(h_, slots.data(), (std::uint64_t)slots.size(), cand_ptr.data(), cand_items.data(),
                                                            scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return R::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_sessions_score_candidates");
        return R::Ok(std::move(scores));
    }
    /// Checkpoint of the named slots (sbr_sessions_get_state): h and c row-major [slots.size()][embedding_dim] (c stays empty for
    /// EWMA, `lstm` false), len per slot.
    struct State {
        std::vector<float> h, c;
        std::vector<std::uint64_t> len;
    };
    State get_state(const std::vector<std::uint32_t>& slots, bool lstm) const {
        State s;
        s.h.resize(slots.size() * dim_);
        if (lstm) s.c.resize(slots.size() * dim_);
        s.len.resize(slots.size());
        check(sbr_sessions_get_state(h_, slots.data(), (std::uint64_t)slots.size(), s.h.data(), lstm ? s.c.data() : nullptr, s.len.data()),
              "sbr_sessions_get_state");
        return s;
    }
    /// Restores a checkpoint into the named slots of this store (sbr_sessions_set_state); `state.c` empty for EWMA.
    void set_state(const std::vector<std::uint32_t>& slots, const State& state) {
        if (state.h.size() != slots.size() * dim_ || state.len.size() != slots.size() || (!state.c.empty() && state.c.size() != state.h.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::set_state: one state per slot");
        check(sbr_sessions_set_state(h_, slots.data(), (std::uint64_t)slots.size(), state.h.data(), state.c.empty() ? nullptr : state.c.data(),
                                     state.len.data()),
              "sbr_sessions_set_state");
    }
    /// Exact ranks of each slot's targets target_items[target_ptr[i] .. target_ptr[i + 1]) among what the slot may be shown
    /// (sbr_rank_targets_rows): the model's rank_targets for representations(slots) with the slot's seen items (unless
    /// `include_seen`), the caller's lists and every item the filter forbids masked to f32::MIN — a masked target has rank
    /// num_items.  The scan reads the store's rows in place.  "Rank the next event, then append it" is this call and `append`.
    Result<std::vector<std::uint32_t>, PredictionError> rank_targets(const std::vector<std::uint32_t>& slots, const std::vector<std::uint64_t>& target_ptr,
                                                                     const std::vector<std::uint32_t>& target_items,
                                                                     const std::vector<std::uint64_t>& excl_ptr = {},
                                                                     const std::vector<std::uint32_t>& excl_items = {}, bool include_seen = false,
                                                                     const TagFilter& filter = {}) const {
        if (!excl_ptr.empty() && (excl_ptr.size() != slots.size() + 1 || excl_ptr.back() > excl_items.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "Sessions::rank_targets: one exclusion range per slot");
        const bool filtered = !filter.any_of.empty() || !filter.none_of.empty();
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, slots.size(), "Sessions::rank_targets: one any_of mask per slot");
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, slots.size(), "Sessions::rank_targets: one none_of mask per slot");
        static const std::uint32_t none = 0;
        sbr_scan_rows d{};
        d.store = h_;
        d.slots = slots.empty() ? &none : slots.data();
        d.flags = include_seen ? SBR_RECOMMEND_INCLUDE_HISTORY : 0u;
        if (!excl_ptr.empty()) { d.excl_ptr = excl_ptr.data(); d.excl_items = excl_items.empty() ? &none : excl_items.data(); }
        if (filtered) { d.any_of = any.data(); d.none_of = none_of.data(); }
        return detail::eligible_ranks(m_, nullptr, d, slots.size(), target_ptr, target_items, "sbr_rank_targets_rows");
    }
    sbr_sessions* handle() const { return h_; }

  private:
    void release() {
        if (h_) sbr_sessions_destroy(h_);
        h_ = nullptr;
    }
    sbr_sessions* h_ = nullptr;
    sbr_model* m_ = nullptr;
    std::size_t dim_;
};

/// An item set of one model (sbr_item_set_*; ITEM SETS in sbr_hip.h): the sorted, unique ids S — a category, a territory, what is in
/// stock — and a device copy of their rows, gathered once, so that every catalogue call restricted to S scans the set's rows and not
/// the catalogue's.  Every method returns, bit for bit, what the model's method of the same name returns with every item outside S
/// added to each row's exclusions: catalogue ids, predict's bits, the same noise per (seed, stream, item), the model's frac_bits.
/// Histories, exclusion lists and a session's seen items stay catalogue ids; entries outside S are ignored.  After the model's
/// parameters change (`fit`, a restored checkpoint) every call throws EngineError(SBR_ERR_INVALID_ARGUMENT) until `refresh()`;
/// set_item_tags / set_item_groups take effect without one.  An empty set is legal.
/// A call's rows are an ItemSet::Rows — of(interactions), of_reps(reps) or of(store, slots) — and every family has the Rows form
/// plus the model's own signatures for histories and representations; `on(store)` offers Sessions' signatures.
/// Obtained from ImplicitSequenceModel::item_set; the model (and a store it is used with) must outlive it.  Movable, not copyable.
class ItemSet {
  public:
    /// max_sequence_length / lstm: the model's, for rollout and beam_search over histories (0: not known, those two refuse).
    ItemSet(sbr_model* model, const std::vector<std::uint32_t>& item_ids, std::size_t embedding_dim, std::size_t num_items,
            std::size_t max_sequence_length = 0, bool lstm = true)
        : m_(model), dim_(embedding_dim), num_items_(num_items), max_len_(max_sequence_length), lstm_(lstm) {
        check(sbr_item_set_create(model, item_ids.empty() ? nullptr : item_ids.data(), (std::uint64_t)item_ids.size(), &h_), "sbr_item_set_create");
    }
    ItemSet(const ItemSet&) = delete;
    ItemSet& operator=(const ItemSet&) = delete;
    ItemSet(ItemSet&& o) noexcept : h_(o.h_), m_(o.m_), dim_(o.dim_), num_items_(o.num_items_), max_len_(o.max_len_), lstm_(o.lstm_) { o.h_ = nullptr; }
    ItemSet& operator=(ItemSet&& o) noexcept {
        if (this != &o) {
            release();
            h_ = o.h_; m_ = o.m_; dim_ = o.dim_; num_items_ = o.num_items_; max_len_ = o.max_len_; lstm_ = o.lstm_;
            o.h_ = nullptr;
        }
        return *this;
    }
    ~ItemSet() { release(); }

    std::size_t size() const {
        std::uint64_t n = 0;
        check(sbr_item_set_size(h_, &n), "sbr_item_set_size");
        return (std::size_t)n;
    }
    /// The set's ids, sorted and unique.
    std::vector<std::uint32_t> items() const {
        std::vector<std::uint32_t> out(size() + 1);
        check(sbr_item_set_items(h_, out.data()), "sbr_item_set_items");
        out.pop_back();
        return out;
    }
    /// Gathers the set's rows again from the model's current parameters.
    void refresh() { check(sbr_item_set_refresh(h_), "sbr_item_set_refresh"); }
    sbr_item_set* handle() const { return h_; }

    /// The rows of one call (struct sbr_scan_rows with the arrays it points into): histories, representations or a store's slots,
    /// with the caller's exclusion lists (representations, slots) and a tag filter.
    class Rows {
      public:
        std::size_t size() const { return n_; }
        /// The same source restricted to some rows of the call.
        Rows take(const std::vector<std::size_t>& rows) const {
            Rows r;
            r.n_ = rows.size();
            r.flags_ = flags_;
            r.store_ = store_;
            r.dim_ = dim_;
            r.kind_ = kind_;
            if (kind_ == 0) detail::csr_rows(ptr_, ids_, rows, &r.ptr_, &r.ids_);
            for (std::size_t i : rows) {
                if (kind_ == 1) r.reps_.insert(r.reps_.end(), reps_.begin() + (std::ptrdiff_t)(i * dim_), reps_.begin() + (std::ptrdiff_t)((i + 1) * dim_));
                if (kind_ == 2) r.ids_.push_back(ids_[i]);
            }
            detail::csr_rows(excl_ptr_, excl_items_, rows, &r.excl_ptr_, &r.excl_items_);
            r.filtered_ = filtered_;
            if (filtered_)
                for (std::size_t i : rows) {
                    r.any_.push_back(any_[i]);
                    r.none_.push_back(none_[i]);
                }
            return r;
        }
        sbr_scan_rows desc() const {
            static const std::uint32_t none = 0;
            static const float zero = 0.0f;
            sbr_scan_rows d{};
            d.flags = flags_;
            if (kind_ == 0) { d.user_ptr = ptr_.data(); d.item_ids = ids_.empty() ? &none : ids_.data(); }
            if (kind_ == 1) d.reps = reps_.empty() ? &zero : reps_.data();
            if (kind_ == 2) { d.store = store_; d.slots = ids_.empty() ? &none : ids_.data(); }
            if (!excl_ptr_.empty()) { d.excl_ptr = excl_ptr_.data(); d.excl_items = excl_items_.empty() ? &none : excl_items_.data(); }
            if (filtered_) { d.any_of = any_.empty() ? &none : any_.data(); d.none_of = none_.empty() ? &none : none_.data(); }
            return d;
        }

      private:
        friend class ItemSet;
        void finish(const std::vector<std::uint64_t>& excl_ptr, const std::vector<std::uint32_t>& excl_items, const TagFilter& filter) {
            if (!excl_ptr.empty() && (excl_ptr.size() != n_ + 1 || excl_ptr.back() > excl_items.size()))
                throw EngineError(SBR_ERR_INVALID_ARGUMENT, "ItemSet: one exclusion range per row");
            excl_ptr_ = excl_ptr;
            excl_items_ = excl_items;
            filtered_ = !filter.any_of.empty() || !filter.none_of.empty();
            if (filtered_) {
                any_ = tag_masks(filter.any_of, n_, "ItemSet: one any_of mask per row");
                none_ = tag_masks(filter.none_of, n_, "ItemSet: one none_of mask per row");
                any_.resize(n_);
                none_.resize(n_);
            }
        }
        int kind_ = 0;  // 0: histories (ptr_, ids_), 1: representations (reps_), 2: a store's slots (store_, ids_)
        std::size_t n_ = 0, dim_ = 0;
        std::uint32_t flags_ = 0;
        sbr_sessions* store_ = nullptr;
        std::vector<std::uint64_t> ptr_, excl_ptr_;
        std::vector<std::uint32_t> ids_, excl_items_, any_, none_;
        std::vector<float> reps_;
        bool filtered_ = false;
    };
    /// Histories: every item of a history is excluded unless `exclude_history` is false.
    Rows of(const data::CompressedInteractions& interactions, bool exclude_history = true, const TagFilter& filter = {}) const {
        Rows r;
        r.kind_ = 0;
        r.n_ = interactions.num_users();
        r.ptr_ = interactions.user_pointers();
        r.ids_ = interactions.item_ids();
        r.flags_ = exclude_history ? 0u : SBR_RECOMMEND_INCLUDE_HISTORY;
        r.finish({}, {}, filter);
        return r;
    }
    /// Representations, row-major [rows][embedding_dim], with per-row exclusion lists as a CSR (both empty: none).
    Rows of_reps(const std::vector<float>& reps, const std::vector<std::uint64_t>& excl_ptr = {}, const std::vector<std::uint32_t>& excl_items = {},
                 const TagFilter& filter = {}) const {
        if (reps.size() % dim_) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "ItemSet: rows of embedding_dim floats");
        Rows r;
        r.kind_ = 1;
        r.dim_ = dim_;
        r.n_ = reps.size() / dim_;
        r.reps_ = reps;
        r.finish(excl_ptr, excl_items, filter);
        return r;
    }
    /// Slots of a current store of this set's model; its seen items are excluded unless `include_seen`.
    Rows of(const Sessions& store, const std::vector<std::uint32_t>& slots, const std::vector<std::uint64_t>& excl_ptr = {},
            const std::vector<std::uint32_t>& excl_items = {}, bool include_seen = false, const TagFilter& filter = {}) const {
        Rows r;
        r.kind_ = 2;
        r.n_ = slots.size();
        r.store_ = store.handle();
        r.ids_ = slots;
        r.flags_ = include_seen ? SBR_RECOMMEND_INCLUDE_HISTORY : 0u;
        r.finish(excl_ptr, excl_items, filter);
        return r;
    }

    // ---- the families over any rows ----
    /// Exact ranks of each row's targets among the set's items the row may be shown (sbr_item_set_rank_targets): the model's
    /// rank_targets with every item outside the set masked as well — a target outside it has rank num_items, the catalogue's.
    Result<std::vector<std::uint32_t>, PredictionError> rank_targets(const Rows& rows, const std::vector<std::uint64_t>& target_ptr,
                                                                     const std::vector<std::uint32_t>& target_items) const {
        const sbr_scan_rows d = rows.desc();
        return detail::eligible_ranks(m_, h_, d, rows.size(), target_ptr, target_items, "sbr_item_set_rank_targets");
    }
    Result<Recommendations, PredictionError> recommend(const Rows& rows, std::size_t k) const {
        if (k < 1 || k > SBR_RECOMMEND_MAX_K) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "ItemSet::recommend: k outside 1..SBR_RECOMMEND_MAX_K");
        Recommendations r = top_rows(rows.size(), k);
        const sbr_scan_rows d = rows.desc();
        const sbr_status st = sbr_item_set_recommend(h_, &d, (std::uint64_t)rows.size(), (std::uint32_t)k, r.items.data(), r.scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Recommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_item_set_recommend");
        return Result<Recommendations, PredictionError>::Ok(std::move(r));
    }
    Result<Recommendations, PredictionError> recommend_diverse(const Rows& rows, std::size_t k, std::size_t pool, float trade_off = 0.5f,
                                                               Similarity metric = Similarity::Cosine) const {
        if (k < 1 || pool < k || pool > SBR_DIVERSE_MAX_POOL)
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "ItemSet::recommend_diverse: 1 <= k <= pool <= SBR_DIVERSE_MAX_POOL");
        Recommendations r = top_rows(rows.size(), k);
        const sbr_scan_rows d = rows.desc();
        const sbr_status st = sbr_item_set_recommend_diverse(h_, &d, (std::uint64_t)rows.size(), (std::uint32_t)k, (std::uint32_t)pool, trade_off,
                                                             (std::uint32_t)metric, r.items.data(), r.scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Recommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_item_set_recommend_diverse");
        return Result<Recommendations, PredictionError>::Ok(std::move(r));
    }
    Result<SampledRecommendations, PredictionError> recommend_sampled(const Rows& rows, std::size_t k, const SampleArgs& sample) const {
        if (k < 1 || k > SBR_RECOMMEND_MAX_K) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "ItemSet::recommend_sampled: k outside 1..SBR_RECOMMEND_MAX_K");
        const sbr_sample_args sa = sample_args(sample, rows.size(), "ItemSet::recommend_sampled: one stream per row");
        SampledRecommendations r = sampled_rows(rows.size(), k);
        const sbr_scan_rows d = rows.desc();
        const sbr_status st = sbr_item_set_recommend_sampled(h_, &d, (std::uint64_t)rows.size(), (std::uint32_t)k, &sa, r.items.data(), r.scores.data(),
                                                             r.keys.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<SampledRecommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_item_set_recommend_sampled");
        return Result<SampledRecommendations, PredictionError>::Ok(std::move(r));
    }
    /// The mass over the set's items the rows may see; frac_bits is the model's.
    Result<Partition, PredictionError> log_partition(const Rows& rows, float temperature = 1.0f) const {
        Partition r;
        r.temperature = temperature;
        r.shift.resize(rows.size() ? rows.size() : 1);
        r.mass.resize(rows.size() ? rows.size() : 1);
        const sbr_scan_rows d = rows.desc();
        const sbr_status st = sbr_item_set_log_partition(h_, &d, (std::uint64_t)rows.size(), temperature, r.shift.data(), r.mass.data(), &r.frac_bits);
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Partition, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_item_set_log_partition");
        r.shift.resize(rows.size());
        r.mass.resize(rows.size());
        return Result<Partition, PredictionError>::Ok(std::move(r));
    }
    Result<Above, PredictionError> recommend_above(const Rows& rows, const std::vector<float>& thresholds, std::uint64_t max_results = ABOVE_MAX_RESULTS,
                                                   AboveOrder order = AboveOrder::Score, bool count_only = false) const {
        return bar("ItemSet::recommend_above", rows, detail::Bar::above(thresholds), max_results, order, count_only);
    }
    Result<Above, PredictionError> count_above(const Rows& rows, const std::vector<float>& thresholds) const {
        return recommend_above(rows, thresholds, 0, AboveOrder::Id, true);
    }
    Result<Above, PredictionError> recommend_top(const Rows& rows, const std::vector<std::uint64_t>& n, std::uint64_t max_results = ABOVE_MAX_RESULTS,
                                                 AboveOrder order = AboveOrder::Score, bool count_only = false) const {
        return bar("ItemSet::recommend_top", rows, detail::Bar::best(n), max_results, order, count_only);
    }
    /// cap.exact finishes the rows the pool did not settle with the set's own recommend_top and the rule on the host.
    Result<CappedRecommendations, PredictionError> recommend_capped(const Rows& rows, std::size_t k, const CapArgs& cap = {}) const {
        const sbr_cap_args ca = detail::cap_args(cap, k, "ItemSet::recommend_capped");
        const std::size_t n = rows.size();
        CappedRecommendations r;
        r.num_users = n;
        r.k = k;
        r.items.resize(n * k);
        r.scores.resize(n * k);
        r.complete.assign(n ? n : 1, 0);
        const sbr_scan_rows d = rows.desc();
        const sbr_status st = sbr_item_set_recommend_capped(h_, &d, (std::uint64_t)n, (std::uint32_t)k, &ca, r.items.data(), r.scores.data(),
                                                            r.complete.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<CappedRecommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_item_set_recommend_capped");
        r.complete.resize(n);
        if (cap.exact && std::find(r.complete.begin(), r.complete.end(), 0) != r.complete.end()) {
            std::vector<std::uint32_t> groups(num_items_);
            check(sbr_model_get_item_groups(m_, groups.data()), "sbr_model_get_item_groups");
            const bool ok = detail::capped_complete(
                [&](const std::vector<std::size_t>& some, std::uint64_t top_n) { return recommend_top(rows.take(some), {top_n}); }, &r, groups, ca.cap,
                ca.pool);
            if (!ok) return Result<CappedRecommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        }
        return Result<CappedRecommendations, PredictionError>::Ok(std::move(r));
    }

    // ---- the model's signatures: histories and representations ----
    Result<Recommendations, PredictionError> recommend(const data::CompressedInteractions& interactions, std::size_t k, bool exclude_history = true,
                                                       const TagFilter& filter = {}) const {
        return recommend(of(interactions, exclude_history, filter), k);
    }
    Result<Recommendations, PredictionError> recommend_reps(const std::vector<float>& reps, std::size_t k, const std::vector<std::uint64_t>& excl_ptr = {},
                                                            const std::vector<std::uint32_t>& excl_items = {}, const TagFilter& filter = {}) const {
        return recommend(of_reps(reps, excl_ptr, excl_items, filter), k);
    }
    Result<SampledRecommendations, PredictionError> recommend_sampled(const data::CompressedInteractions& interactions, std::size_t k,
                                                                      const SampleArgs& sample, bool exclude_history = true,
                                                                      const TagFilter& filter = {}) const {
        return recommend_sampled(of(interactions, exclude_history, filter), k, sample);
    }
    Result<SampledRecommendations, PredictionError> recommend_sampled_reps(const std::vector<float>& reps, std::size_t k, const SampleArgs& sample,
                                                                           const std::vector<std::uint64_t>& excl_ptr = {},
                                                                           const std::vector<std::uint32_t>& excl_items = {},
                                                                           const TagFilter& filter = {}) const {
        return recommend_sampled(of_reps(reps, excl_ptr, excl_items, filter), k, sample);
    }
    Result<Partition, PredictionError> log_partition(const data::CompressedInteractions& interactions, float temperature = 1.0f,
                                                     bool exclude_history = true, const TagFilter& filter = {}) const {
        return log_partition(of(interactions, exclude_history, filter), temperature);
    }
    Result<Partition, PredictionError> log_partition_reps(const std::vector<float>& reps, float temperature, const std::vector<std::uint64_t>& excl_ptr = {},
                                                          const std::vector<std::uint32_t>& excl_items = {}, const TagFilter& filter = {}) const {
        return log_partition(of_reps(reps, excl_ptr, excl_items, filter), temperature);
    }
    Result<Above, PredictionError> recommend_above(const data::CompressedInteractions& interactions, const std::vector<float>& thresholds,
                                                   bool exclude_history = true, const TagFilter& filter = {}, std::uint64_t max_results = ABOVE_MAX_RESULTS,
                                                   AboveOrder order = AboveOrder::Score, bool count_only = false) const {
        return recommend_above(of(interactions, exclude_history, filter), thresholds, max_results, order, count_only);
    }
    Result<Above, PredictionError> recommend_above_reps(const std::vector<float>& reps, const std::vector<float>& thresholds,
                                                        const std::vector<std::uint64_t>& excl_ptr = {}, const std::vector<std::uint32_t>& excl_items = {},
                                                        const TagFilter& filter = {}, std::uint64_t max_results = ABOVE_MAX_RESULTS,
                                                        AboveOrder order = AboveOrder::Score, bool count_only = false) const {
        return recommend_above(of_reps(reps, excl_ptr, excl_items, filter), thresholds, max_results, order, count_only);
    }
    Result<Above, PredictionError> recommend_top(const data::CompressedInteractions& interactions, const std::vector<std::uint64_t>& n,
                                                 bool exclude_history = true, const TagFilter& filter = {}, std::uint64_t max_results = ABOVE_MAX_RESULTS,
                                                 AboveOrder order = AboveOrder::Score, bool count_only = false) const {
        return recommend_top(of(interactions, exclude_history, filter), n, max_results, order, count_only);
    }
    Result<Above, PredictionError> recommend_top_reps(const std::vector<float>& reps, const std::vector<std::uint64_t>& n,
                                                      const std::vector<std::uint64_t>& excl_ptr = {}, const std::vector<std::uint32_t>& excl_items = {},
                                                      const TagFilter& filter = {}, std::uint64_t max_results = ABOVE_MAX_RESULTS,
                                                      AboveOrder order = AboveOrder::Score, bool count_only = false) const {
        return recommend_top(of_reps(reps, excl_ptr, excl_items, filter), n, max_results, order, count_only);
    }
    Result<CappedRecommendations, PredictionError> recommend_capped(const data::CompressedInteractions& interactions, std::size_t k, const CapArgs& cap = {},
                                                                    bool exclude_history = true, const TagFilter& filter = {}) const {
        return recommend_capped(of(interactions, exclude_history, filter), k, cap);
    }
    Result<CappedRecommendations, PredictionError> recommend_capped_reps(const std::vector<float>& reps, std::size_t k, const CapArgs& cap = {},
                                                                         const std::vector<std::uint64_t>& excl_ptr = {},
                                                                         const std::vector<std::uint32_t>& excl_items = {},
                                                                         const TagFilter& filter = {}) const {
        return recommend_capped(of_reps(reps, excl_ptr, excl_items, filter), k, cap);
    }
    Result<Recommendations, PredictionError> recommend_diverse(const data::CompressedInteractions& interactions, std::size_t k, std::size_t pool,
                                                               float trade_off = 0.5f, Similarity metric = Similarity::Cosine,
                                                               bool exclude_history = true, const TagFilter& filter = {}) const {
        return recommend_diverse(of(interactions, exclude_history, filter), k, pool, trade_off, metric);
    }
    Result<Recommendations, PredictionError> recommend_diverse_reps(const std::vector<float>& reps, std::size_t k, std::size_t pool, float trade_off = 0.5f,
                                                                    Similarity metric = Similarity::Cosine, const std::vector<std::uint64_t>& excl_ptr = {},
                                                                    const std::vector<std::uint32_t>& excl_items = {}, const TagFilter& filter = {}) const {
        return recommend_diverse(of_reps(reps, excl_ptr, excl_items, filter), k, pool, trade_off, metric);
    }

    /// `on(store)`: Sessions' scan signatures through the set.
    class OnSessions {
      public:
        OnSessions(const ItemSet& set, const Sessions& store) : set_(set), store_(store) {}
        Result<std::vector<std::uint32_t>, PredictionError> rank_targets(const std::vector<std::uint32_t>& slots, const std::vector<std::uint64_t>& target_ptr,
                                                                         const std::vector<std::uint32_t>& target_items,
                                                                         const std::vector<std::uint64_t>& excl_ptr = {},
                                                                         const std::vector<std::uint32_t>& excl_items = {}, bool include_seen = false,
                                                                         const TagFilter& filter = {}) const {
            return set_.rank_targets(set_.of(store_, slots, excl_ptr, excl_items, include_seen, filter), target_ptr, target_items);
        }
        Result<Recommendations, PredictionError> recommend(const std::vector<std::uint32_t>& slots, std::size_t k, const std::vector<std::uint64_t>& excl_ptr = {},
                                                           const std::vector<std::uint32_t>& excl_items = {}, bool include_seen = false,
                                                           const TagFilter& filter = {}) const {
            return set_.recommend(set_.of(store_, slots, excl_ptr, excl_items, include_seen, filter), k);
        }
        Result<SampledRecommendations, PredictionError> recommend_sampled(const std::vector<std::uint32_t>& slots, std::size_t k, const SampleArgs& sample,
                                                                          const TagFilter& filter = {}, const std::vector<std::uint64_t>& excl_ptr = {},
                                                                          const std::vector<std::uint32_t>& excl_items = {}, bool include_seen = false) const {
            return set_.recommend_sampled(set_.of(store_, slots, excl_ptr, excl_items, include_seen, filter), k, sample);
        }
        Result<Partition, PredictionError> log_partition(const std::vector<std::uint32_t>& slots, float temperature, const TagFilter& filter = {},
                                                         const std::vector<std::uint64_t>& excl_ptr = {}, const std::vector<std::uint32_t>& excl_items = {},
                                                         bool include_seen = false) const {
            return set_.log_partition(set_.of(store_, slots, excl_ptr, excl_items, include_seen, filter), temperature);
        }
        Result<Above, PredictionError> recommend_above(const std::vector<std::uint32_t>& slots, const std::vector<float>& thresholds, const TagFilter& filter = {},
                                                       const std::vector<std::uint64_t>& excl_ptr = {}, const std::vector<std::uint32_t>& excl_items = {},
                                                       bool include_seen = false, std::uint64_t max_results = ABOVE_MAX_RESULTS,
                                                       AboveOrder order = AboveOrder::Score, bool count_only = false) const {
            return set_.recommend_above(set_.of(store_, slots, excl_ptr, excl_items, include_seen, filter), thresholds, max_results, order, count_only);
        }
        Result<Above, PredictionError> recommend_top(const std::vector<std::uint32_t>& slots, const std::vector<std::uint64_t>& n, const TagFilter& filter = {},
                                                     const std::vector<std::uint64_t>& excl_ptr = {}, const std::vector<std::uint32_t>& excl_items = {},
                                                     bool include_seen = false, std::uint64_t max_results = ABOVE_MAX_RESULTS,
                                                     AboveOrder order = AboveOrder::Score, bool count_only = false) const {
            return set_.recommend_top(set_.of(store_, slots, excl_ptr, excl_items, include_seen, filter), n, max_results, order, count_only);
        }
        Result<CappedRecommendations, PredictionError> recommend_capped(const std::vector<std::uint32_t>& slots, std::size_t k, const CapArgs& cap = {},
                                                                        const TagFilter& filter = {}, const std::vector<std::uint64_t>& excl_ptr = {},
                                                                        const std::vector<std::uint32_t>& excl_items = {}, bool include_seen = false) const {
            return set_.recommend_capped(set_.of(store_, slots, excl_ptr, excl_items, include_seen, filter), k, cap);
        }
        Result<Recommendations, PredictionError> recommend_diverse(const std::vector<std::uint32_t>& slots, std::size_t k, std::size_t pool, float trade_off = 0.5f,
                                                                   Similarity metric = Similarity::Cosine, const std::vector<std::uint64_t>& excl_ptr = {},
                                                                   const std::vector<std::uint32_t>& excl_items = {}, const TagFilter& filter = {}) const {
            return set_.recommend_diverse(set_.of(store_, slots, excl_ptr, excl_items, false, filter), k, pool, trade_off, metric);
        }
        /// Sessions::rollout within the set (sbr_item_set_rollout): the store's own rollout with every item outside the set added
        /// to each row's exclusion list, bit for bit; frac_bits is the model's.
        Result<Rollout, PredictionError> rollout(const std::vector<std::uint32_t>& slots, const RolloutArgs& a) const {
            return store_.rollout_in(set_.h_, slots, a);
        }
        /// Sessions::beam_search within the set (sbr_item_set_beam_search), under rollout's rule.
        Result<Beams, PredictionError> beam_search(const std::vector<std::uint32_t>& slots, const BeamArgs& a) const {
            return store_.beam_search_in(set_.h_, slots, a);
        }

      private:
        const ItemSet& set_;
        const Sessions& store_;
    };
    OnSessions on(const Sessions& store) const { return OnSessions(*this, store); }

    /// ImplicitSequenceModel::rollout within the set, DEFINED as that call is: a temporary store of one slot per user, `append` of
    /// each history's last max_sequence_length items, and on(store).rollout of all slots — with exclude_history each history's
    /// items as its exclusion list, replacing a.excl_ptr / a.excl_items; a.lstm is set from the model.
    Result<Rollout, PredictionError> rollout(const data::CompressedInteractions& histories, RolloutArgs a, bool exclude_history = true) const {
        std::vector<std::uint32_t> slots;
        Sessions store = histories_store("ItemSet::rollout", histories, exclude_history, &slots, &a.excl_ptr, &a.excl_items);
        a.lstm = lstm_;
        a.include_seen = false;
        return on(store).rollout(slots, a);
    }
    /// ImplicitSequenceModel::beam_search within the set, DEFINED as rollout's histories form is.
    Result<Beams, PredictionError> beam_search(const data::CompressedInteractions& histories, BeamArgs a, bool exclude_history = true) const {
        std::vector<std::uint32_t> slots;
        Sessions store = histories_store("ItemSet::beam_search", histories, exclude_history, &slots, &a.excl_ptr, &a.excl_items);
        a.include_seen = false;
        return on(store).beam_search(slots, a);
    }

  private:
    static Recommendations top_rows(std::size_t n, std::size_t k) {
        Recommendations r;
        r.num_users = n;
        r.k = k;
        r.items.resize(n * k);
        r.scores.resize(n * k);
        return r;
    }
    Result<Above, PredictionError> bar(const char* me, const Rows& rows, detail::Bar b, std::uint64_t max_results, AboveOrder order, bool count_only) const {
        b.fit(rows.size(), me, "row");
        const sbr_scan_rows d = rows.desc();
        Above r;
        const sbr_status st = detail::above_call(
            [&](std::uint64_t* counts, std::uint64_t* total, std::uint64_t cap, std::uint32_t* ids, float* scores) {
                if (b.top)
                    return sbr_item_set_recommend_top(h_, &d, (std::uint64_t)rows.size(), b.n.data(), b.cuts.data(), counts, total, cap, ids, scores);
                return sbr_item_set_recommend_above(h_, &d, (std::uint64_t)rows.size(), b.th.data(), counts, total, cap, ids, scores);
            },
            rows.size(), max_results, order, count_only, b.top ? "sbr_item_set_recommend_top" : "sbr_item_set_recommend_above", b, &r);
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Above, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        return Result<Above, PredictionError>::Ok(std::move(r));
    }
    void release() {
        if (h_) sbr_item_set_destroy(h_);
        h_ = nullptr;
    }
    /// ImplicitSequenceModel::rollout's temporary store: one slot per user, each history's last max_sequence_length items appended;
    /// with exclude_history each history's items become the exclusion list (replacing excl_ptr / excl_items).
    Sessions histories_store(const char* me, const data::CompressedInteractions& histories, bool exclude_history, std::vector<std::uint32_t>* slots,
                             std::vector<std::uint64_t>* excl_ptr, std::vector<std::uint32_t>* excl_items) const {
        const std::vector<std::uint64_t>& up = histories.user_pointers();
        const std::vector<std::uint32_t>& ids = histories.item_ids();
        const std::size_t n = histories.num_users();
        if (n == 0) throw EngineError(SBR_ERR_INVALID_ARGUMENT, std::string(me) + ": at least one history");
        if (max_len_ == 0) throw EngineError(SBR_ERR_INVALID_ARGUMENT, std::string(me) + ": a set made by ImplicitSequenceModel::item_set");
        std::vector<std::uint32_t> tail;
        std::vector<std::uint64_t> tail_ptr(n + 1, 0);
        slots->resize(n);
        for (std::size_t u = 0; u < n; ++u) {
            (*slots)[u] = (std::uint32_t)u;
            const std::uint64_t keep = std::min<std::uint64_t>(up[u + 1] - up[u], max_len_);
            tail.insert(tail.end(), ids.begin() + (std::ptrdiff_t)(up[u + 1] - keep), ids.begin() + (std::ptrdiff_t)up[u + 1]);
            tail_ptr[u + 1] = tail.size();
        }
        Sessions store(m_, n, dim_);
        store.append(*slots, tail_ptr, tail);
        if (exclude_history) {
            excl_ptr->assign(up.begin(), up.end());
            for (std::uint64_t& p : *excl_ptr) p -= up.front();
            excl_items->assign(ids.begin() + (std::ptrdiff_t)up.front(), ids.begin() + (std::ptrdiff_t)up.back());
        }
        return store;
    }
    sbr_item_set* h_ = nullptr;
    sbr_model* m_ = nullptr;
    std::size_t dim_ = 0, num_items_ = 0, max_len_ = 0;
    bool lstm_ = true;
};

/// Owner of the device replicas behind one model object: `num_threads` replicas (≙ the worker
/// threads of sequence_model.rs:90-102), replica r on HIP device r mod device_count
/// (sbr_group_create).
class Replicas {
  public:
    Replicas(sbr_hparams hp, bool partition_item_table) : hp_(hp), partitioned_(partition_item_table) {
        handles_.assign(hp.num_devices, nullptr);
        const sbr_status st = sbr_group_create(&hp, hp.num_devices, partition_item_table ? SBR_GROUP_PARTITION_ITEM_TABLE : 0u,
                                               handles_.data());
        if (st != SBR_OK) {
            handles_.clear();
            throw EngineError(st, "sbr_group_create");
        }
    }
    Replicas(const Replicas&) = delete;
    Replicas& operator=(const Replicas&) = delete;
    ~Replicas() { release(); }

    sbr_model* primary() const { return handles_[0]; }
    const sbr_hparams& hparams() const { return hp_; }
    const std::vector<sbr_model*>& handles() const { return handles_; }
    bool partitioned() const { return partitioned_; }

    Result<float, FittingError> fit(const data::CompressedInteractions& interactions) {
        float loss = 0.0f;
        const sbr_status st =
            sbr_group_fit(handles_.data(), (std::uint32_t)handles_.size(), interactions.user_pointers().data(),
                          interactions.item_ids().data(), (std::uint64_t)interactions.num_users(), &loss);
        if (st == SBR_ERR_NO_INTERACTIONS) return Result<float, FittingError>::Err(FittingError::NoInteractions);
        check(st, "sbr_group_fit");
        return Result<float, FittingError>::Ok(loss);
    }

  private:
    void release() {
        for (sbr_model* h : handles_)
            if (h) sbr_model_destroy(h);
        handles_.clear();
    }
    sbr_hparams hp_;
    bool partitioned_ = false;
    std::vector<sbr_model*> handles_;
};

/// fit + OnlineRankingModel over the C-ABI, shared by both model types
/// (lstm.rs:391-416, ewma.rs:404-429 → sequence_model.rs:70-232).
class ImplicitSequenceModel : public OnlineRankingModel<ImplicitUser> {
  public:
    ImplicitSequenceModel(const sbr_hparams& hp, bool partition_item_table)
        : replicas_(std::make_unique<Replicas>(hp, partition_item_table)) {}

    /// Fit the model; re-callable (training continues).  Err(NoInteractions) when no subsequence
    /// of more than two items exists (sequence_model.rs:86-88).
    Result<float, FittingError> fit(const data::CompressedInteractions& interactions) { return replicas_->fit(interactions); }

    /// The crate's own ORDER of work at one subsequence per step (`batch_sequences(1)`, embedding_dim <= 32): a step's negatives
    /// from the worker's sequential XorShiftRng stream (sequence_model.rs:58-65, :137) and, with `num_threads(n)`, one optimiser
    /// application per worker in worker order (:163-166) — instead of the engine's counter-keyed draws and summed gradients.
    /// Call before `fit`.  Throws EngineError(SBR_ERR_UNSUPPORTED) outside the mode's shapes.
    void set_reference_order(bool on) {
        for (sbr_model* h : replicas_->handles()) {
            const sbr_status st = sbr_model_set_reference_order(h, on ? 1 : 0);
            if (st != SBR_OK) throw EngineError(st, "sbr_model_set_reference_order");
        }
    }

    /// The number the reference's `fit` would have returned for the last `fit` call: sequence_model.rs:157 reads the
    /// loss node BEFORE :160 runs its forward pass; the nodes are shared running sums (lstm.rs:322-328), so a subsequence
    /// of s steps contributes L_{s-1} of the worker's most recent earlier subsequence with at least s steps.  `fit` itself returns the true mean loss.
    float last_fit_lagged_loss() const {
        float v = 0.0f;
        check(sbr_model_last_fit_lagged_loss(replicas_->primary(), &v), "sbr_model_last_fit_lagged_loss");
        return v;
    }

    Result<ImplicitUser, PredictionError> user_representation(const std::vector<ItemId>& item_ids) const override {
        const std::vector<std::uint32_t> ids = narrow(item_ids);
        ImplicitUser user{std::vector<float>(replicas_->hparams().embedding_dim)};
        const sbr_status st = sbr_user_representation(replicas_->primary(), ids.data(), ids.size(), user.user_embedding.data());
        if (st == SBR_ERR_INVALID_PREDICTION)
            return Result<ImplicitUser, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_user_representation");
        return Result<ImplicitUser, PredictionError>::Ok(std::move(user));
    }

    Result<std::vector<float>, PredictionError> predict(const ImplicitUser& user,
                                                        const std::vector<ItemId>& item_ids) const override {
        if (user.user_embedding.size() != replicas_->hparams().embedding_dim)
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "predict: user embedding has the wrong dimension");
        const std::vector<std::uint32_t> ids = narrow(item_ids);
        std::vector<float> out(ids.size());
        const sbr_status st = sbr_predict(replicas_->primary(), user.user_embedding.data(), ids.data(), ids.size(), out.data());
        if (st == SBR_ERR_INVALID_PREDICTION)
            return Result<std::vector<float>, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_predict");
        return Result<std::vector<float>, PredictionError>::Ok(std::move(out));
    }

    /// The k best items of the whole catalogue for each user's history in `interactions` (sbr_recommend): score descending,
    /// ties to the lower item id, the scores bit-equal to `predict`'s.  Every item of a history is excluded unless
    /// `exclude_history` is false; a row with fewer than k eligible items is padded with (0xFFFFFFFF, -inf).
    /// Err(InvalidPredictionValue) on a non-finite score.
    Result<Recommendations, PredictionError> recommend(const data::CompressedInteractions& interactions, std::size_t k,
                                                       bool exclude_history = true) const {
        if (k < 1 || k > SBR_RECOMMEND_MAX_K) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "recommend: k outside 1..SBR_RECOMMEND_MAX_K");
        Recommendations r;
        r.num_users = interactions.num_users();
        r.k = k;
        r.items.resize(r.num_users * k);
        r.scores.resize(r.num_users * k);
        const sbr_status st = sbr_recommend(replicas_->primary(), interactions.user_pointers().data(), interactions.item_ids().data(),
                                            (std::uint64_t)r.num_users, (std::uint32_t)k, exclude_history ? 0u : SBR_RECOMMEND_INCLUDE_HISTORY,
                                            r.items.data(), r.scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Recommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_recommend");
        return Result<Recommendations, PredictionError>::Ok(std::move(r));
    }

    /// One 32-bit tag word per item, kept on the device for `recommend_filtered`, `recommend_diverse_filtered`,
    /// `similar_items_filtered` and the Sessions forms (sbr_model_set_item_tags).  Serving metadata: `fit` leaves the tags alone, a session store stays usable,
    /// and they are not part of a saved model — set them again after a restore.
    void set_item_tags(const std::vector<std::uint32_t>& tags) {
        if (tags.size() != (std::size_t)replicas_->hparams().num_items)
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "set_item_tags: one tag word per item");
        check(sbr_model_set_item_tags(replicas_->primary(), tags.data()), "sbr_model_set_item_tags");
    }
    /// The model has no tags again: the *_filtered calls throw EngineError(SBR_ERR_INVALID_ARGUMENT) until they are set.
    void clear_item_tags() { check(sbr_model_set_item_tags(replicas_->primary(), nullptr), "sbr_model_set_item_tags"); }
    /// The tag words last set; throws EngineError(SBR_ERR_INVALID_ARGUMENT) while the model has none.
    std::vector<std::uint32_t> item_tags() const {
        std::vector<std::uint32_t> out((std::size_t)replicas_->hparams().num_items);
        check(sbr_model_get_item_tags(replicas_->primary(), out.data()), "sbr_model_get_item_tags");
        return out;
    }

    /// One u32 group word per item — a series, a seller, a category; SBR_NO_GROUP: never capped — kept on the device for the
    /// recommend_capped calls (sbr_model_set_item_groups).  Serving metadata as the tags: `fit` leaves them alone, a session store
    /// stays usable, and they are not part of a saved model.
    void set_item_groups(const std::vector<std::uint32_t>& groups) {
        if (groups.size() != (std::size_t)replicas_->hparams().num_items)
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "set_item_groups: one group word per item");
        check(sbr_model_set_item_groups(replicas_->primary(), groups.data()), "sbr_model_set_item_groups");
    }
    /// The model has no groups again: the recommend_capped calls throw EngineError(SBR_ERR_INVALID_ARGUMENT) until they are set.
    void clear_item_groups() { check(sbr_model_set_item_groups(replicas_->primary(), nullptr), "sbr_model_set_item_groups"); }
    /// The group words last set; throws EngineError(SBR_ERR_INVALID_ARGUMENT) while the model has none.
    std::vector<std::uint32_t> item_groups() const {
        std::vector<std::uint32_t> out((std::size_t)replicas_->hparams().num_items);
        check(sbr_model_get_item_groups(replicas_->primary(), out.data()), "sbr_model_get_item_groups");
        return out;
    }

    /// `recommend` under the hard slate rule "at most cap.cap items of one item group" (sbr_recommend_capped; CAPPED in sbr_hip.h):
    /// each row is `recommend`'s order walked from the top, an entry kept while fewer than cap kept entries share its group, k kept
    /// in all, with predict's bits.  The device applies the rule to each row's best cap.pool; with cap.exact the rows that pool did
    /// not settle are finished through `recommend_top` and every flag is 1.  `filter`: a tag filter unless both its vectors are empty.
    Result<CappedRecommendations, PredictionError> recommend_capped(const data::CompressedInteractions& interactions, std::size_t k,
                                                                    const CapArgs& cap = {}, bool exclude_history = true,
                                                                    const TagFilter& filter = {}) const {
        const sbr_cap_args ca = detail::cap_args(cap, k, "recommend_capped");
        const std::size_t n = interactions.num_users();
        const bool filtered = !filter.any_of.empty() || !filter.none_of.empty();
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, n, "recommend_capped: one any_of mask per user");
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, n, "recommend_capped: one none_of mask per user");
        CappedRecommendations r = capped_rows(n, k);
        const sbr_status st = sbr_recommend_capped(replicas_->primary(), interactions.user_pointers().data(), interactions.item_ids().data(),
                                                   (std::uint64_t)n, (std::uint32_t)k, exclude_history ? 0u : SBR_RECOMMEND_INCLUDE_HISTORY, &ca,
                                                   filtered ? any.data() : nullptr, filtered ? none_of.data() : nullptr, r.items.data(),
                                                   r.scores.data(), r.complete.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<CappedRecommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_recommend_capped");
        r.complete.resize(n);
        if (cap.exact && std::find(r.complete.begin(), r.complete.end(), 0) != r.complete.end()) {
            const std::vector<std::uint64_t>& up = interactions.user_pointers();
            const bool ok = detail::capped_complete(
                [&](const std::vector<std::size_t>& rows, std::uint64_t top_n) {
                    std::vector<std::uint64_t> sp, ts;
                    std::vector<std::uint32_t> si;
                    detail::csr_rows(up, interactions.item_ids(), rows, &sp, &si);
                    ts.assign(si.size(), 0);
                    const data::CompressedInteractions sub(rows.size(), interactions.num_items(), sp, si, ts);
                    return recommend_top(sub, {top_n}, exclude_history, detail::filter_rows(filter, n, rows));
                },
                &r, item_groups(), ca.cap, ca.pool);
            if (!ok) return Result<CappedRecommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        }
        return Result<CappedRecommendations, PredictionError>::Ok(std::move(r));
    }
    /// recommend_capped from representations, reps [num_users][embedding_dim] (sbr_recommend_capped_reps); excl_ptr / excl_items:
    /// per-user exclusion lists as a CSR (both empty: none).
    Result<CappedRecommendations, PredictionError> recommend_capped_reps(const std::vector<float>& reps, std::size_t k, const CapArgs& cap = {},
                                                                         const std::vector<std::uint64_t>& excl_ptr = {},
                                                                         const std::vector<std::uint32_t>& excl_items = {},
                                                                         const TagFilter& filter = {}) const {
        const sbr_cap_args ca = detail::cap_args(cap, k, "recommend_capped_reps");
        const std::size_t dim = (std::size_t)replicas_->hparams().embedding_dim;
        if (reps.size() % dim) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "recommend_capped_reps: rows of embedding_dim floats");
        const std::size_t n = reps.size() / dim;
        if (!excl_ptr.empty() && (excl_ptr.size() != n + 1 || excl_ptr.back() > excl_items.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "recommend_capped_reps: one exclusion range per user");
        const bool filtered = !filter.any_of.empty() || !filter.none_of.empty();
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, n, "recommend_capped_reps: one any_of mask per user");
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, n, "recommend_capped_reps: one none_of mask per user");
        CappedRecommendations r = capped_rows(n, k);
        const std::uint32_t none = 0;
        const float zero = 0.0f;
        const sbr_status st = sbr_recommend_capped_reps(replicas_->primary(), reps.empty() ? &zero : reps.data(), (std::uint64_t)n, (std::uint32_t)k,
                                                        excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                        excl_ptr.empty() ? nullptr : (excl_items.empty() ? &none : excl_items.data()), &ca,
                                                        filtered ? any.data() : nullptr, filtered ? none_of.data() : nullptr, r.items.data(),
                                                        r.scores.data(), r.complete.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<CappedRecommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_recommend_capped_reps");
        r.complete.resize(n);
        if (cap.exact && std::find(r.complete.begin(), r.complete.end(), 0) != r.complete.end()) {
            const bool ok = detail::capped_complete(
                [&](const std::vector<std::size_t>& rows, std::uint64_t top_n) {
                    std::vector<float> sub;
                    for (std::size_t i : rows) sub.insert(sub.end(), reps.begin() + (std::ptrdiff_t)(i * dim), reps.begin() + (std::ptrdiff_t)((i + 1) * dim));
                    std::vector<std::uint64_t> ep;
                    std::vector<std::uint32_t> ei;
                    detail::csr_rows(excl_ptr, excl_items, rows, &ep, &ei);
                    return recommend_top_reps(sub, {top_n}, ep, ei, detail::filter_rows(filter, n, rows));
                },
                &r, item_groups(), ca.cap, ca.pool);
            if (!ok) return Result<CappedRecommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        }
        return Result<CappedRecommendations, PredictionError>::Ok(std::move(r));
    }
  private:
    static CappedRecommendations capped_rows(std::size_t n, std::size_t k) {
        CappedRecommendations r;
        r.num_users = n;
        r.k = k;
        r.items.resize(n * k);
        r.scores.resize(n * k);
        r.complete.assign(n ? n : 1, 0);
        return r;
    }
  public:

    /// `recommend` under a per-user tag filter (sbr_recommend_filtered): the exact top k of the items each user's masks allow, the
    /// bits of `recommend` with every other item added to the user's exclusions; tested inside the scan.  Not with `among`.
    Result<Recommendations, PredictionError> recommend_filtered(const data::CompressedInteractions& interactions, std::size_t k,
                                                                bool exclude_history, const TagFilter& filter) const {
        if (k < 1 || k > SBR_RECOMMEND_MAX_K) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "recommend: k outside 1..SBR_RECOMMEND_MAX_K");
        Recommendations r;
        r.num_users = interactions.num_users();
        r.k = k;
        r.items.resize(r.num_users * k);
        r.scores.resize(r.num_users * k);
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, r.num_users, "recommend: one any_of mask per user");
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, r.num_users, "recommend: one none_of mask per user");
        const sbr_status st = sbr_recommend_filtered(replicas_->primary(), interactions.user_pointers().data(), interactions.item_ids().data(),
                                                     (std::uint64_t)r.num_users, (std::uint32_t)k,
                                                     exclude_history ? 0u : SBR_RECOMMEND_INCLUDE_HISTORY, any.data(), none_of.data(),
                                                     r.items.data(), r.scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Recommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_recommend_filtered");
        return Result<Recommendations, PredictionError>::Ok(std::move(r));
    }

    /// `recommend` with a dice (sbr_recommend_sampled): k draws without replacement from softmax(score / temperature) over the items
    /// each user may see, inside the catalogue scan; rows in draw order with the plain scores and the keys.  The same (seed, stream)
    /// gives the same row bit for bit; vary `sample.seed` per request.  `filter`: a tag filter unless both its vectors are empty.
    Result<SampledRecommendations, PredictionError> recommend_sampled(const data::CompressedInteractions& interactions, std::size_t k,
                                                                      const SampleArgs& sample, bool exclude_history = true,
                                                                      const TagFilter& filter = {}) const {
        if (k < 1 || k > SBR_RECOMMEND_MAX_K) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "recommend_sampled: k outside 1..SBR_RECOMMEND_MAX_K");
        const std::size_t n = interactions.num_users();
        const bool filtered = !filter.any_of.empty() || !filter.none_of.empty();
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, n, "recommend_sampled: one any_of mask per user");
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, n, "recommend_sampled: one none_of mask per user");
        const sbr_sample_args sa = sample_args(sample, n, "recommend_sampled: one stream per user");
        SampledRecommendations r = sampled_rows(n, k);
        const sbr_status st = sbr_recommend_sampled(replicas_->primary(), interactions.user_pointers().data(), interactions.item_ids().data(),
                                                    (std::uint64_t)n, (std::uint32_t)k, exclude_history ? 0u : SBR_RECOMMEND_INCLUDE_HISTORY, &sa,
                                                    filtered ? any.data() : nullptr, filtered ? none_of.data() : nullptr, r.items.data(),
                                                    r.scores.data(), r.keys.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<SampledRecommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_recommend_sampled");
        return Result<SampledRecommendations, PredictionError>::Ok(std::move(r));
    }
    /// recommend_sampled from representations, reps [num_users][embedding_dim] (sbr_recommend_sampled_reps); excl_ptr / excl_items:
    /// per-user exclusion lists as a CSR (both empty: none).
    Result<SampledRecommendations, PredictionError> recommend_sampled_reps(const std::vector<float>& reps, std::size_t k, const SampleArgs& sample,
                                                                           const std::vector<std::uint64_t>& excl_ptr = {},
                                                                           const std::vector<std::uint32_t>& excl_items = {},
                                                                           const TagFilter& filter = {}) const {
        if (k < 1 || k > SBR_RECOMMEND_MAX_K) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "recommend_sampled_reps: k outside 1..SBR_RECOMMEND_MAX_K");
        const std::size_t dim = (std::size_t)replicas_->hparams().embedding_dim;
        if (reps.size() % dim) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "recommend_sampled_reps: rows of embedding_dim floats");
        const std::size_t n = reps.size() / dim;
        if (!excl_ptr.empty() && (excl_ptr.size() != n + 1 || excl_ptr.back() > excl_items.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "recommend_sampled_reps: one exclusion range per user");
        const bool filtered = !filter.any_of.empty() || !filter.none_of.empty();
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, n, "recommend_sampled_reps: one any_of mask per user");
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, n, "recommend_sampled_reps: one none_of mask per user");
        const sbr_sample_args sa = sample_args(sample, n, "recommend_sampled_reps: one stream per user");
        SampledRecommendations r = sampled_rows(n, k);
        const std::uint32_t none = 0;
        const sbr_status st = sbr_recommend_sampled_reps(replicas_->primary(), reps.data(), (std::uint64_t)n, (std::uint32_t)k,
                                                         excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                         excl_ptr.empty() ? nullptr : (excl_items.empty() ? &none : excl_items.data()), &sa,
                                                         filtered ? any.data() : nullptr, filtered ? none_of.data() : nullptr, r.items.data(),
                                                         r.scores.data(), r.keys.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<SampledRecommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_recommend_sampled_reps");
        return Result<SampledRecommendations, PredictionError>::Ok(std::move(r));
    }

    /// The softmax normaliser of `recommend_sampled`'s distribution, exactly (sbr_log_partition): per user the fixed-point mass of
    /// softmax(score / temperature) over the items `recommend` would choose from, summed on the device as integers.
    Result<Partition, PredictionError> log_partition(const data::CompressedInteractions& interactions, float temperature = 1.0f,
                                                     bool exclude_history = true, const TagFilter& filter = {}) const {
        const std::size_t n = interactions.num_users();
        const bool filtered = !filter.any_of.empty() || !filter.none_of.empty();
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, n, "log_partition: one any_of mask per user");
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, n, "log_partition: one none_of mask per user");
        Partition r;
        r.temperature = temperature;
        r.shift.resize(n);
        r.mass.resize(n);
        const sbr_status st = sbr_log_partition(replicas_->primary(), interactions.user_pointers().data(), interactions.item_ids().data(),
                                                (std::uint64_t)n, exclude_history ? 0u : SBR_RECOMMEND_INCLUDE_HISTORY, temperature,
                                                filtered ? any.data() : nullptr, filtered ? none_of.data() : nullptr, r.shift.data(),
                                                r.mass.data(), &r.frac_bits);
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Partition, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_log_partition");
        return Result<Partition, PredictionError>::Ok(std::move(r));
    }
    /// log_partition from representations, reps [num_users][embedding_dim] (sbr_log_partition_reps); excl_ptr / excl_items: per-user
    /// exclusion lists as a CSR (both empty: none).
    Result<Partition, PredictionError> log_partition_reps(const std::vector<float>& reps, float temperature,
                                                          const std::vector<std::uint64_t>& excl_ptr = {},
                                                          const std::vector<std::uint32_t>& excl_items = {}, const TagFilter& filter = {}) const {
        const std::size_t dim = (std::size_t)replicas_->hparams().embedding_dim;
        if (reps.size() % dim) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "log_partition_reps: rows of embedding_dim floats");
        const std::size_t n = reps.size() / dim;
        if (!excl_ptr.empty() && (excl_ptr.size() != n + 1 || excl_ptr.back() > excl_items.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "log_partition_reps: one exclusion range per user");
        const bool filtered = !filter.any_of.empty() || !filter.none_of.empty();
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, n, "log_partition_reps: one any_of mask per user");
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, n, "log_partition_reps: one none_of mask per user");
        Partition r;
        r.temperature = temperature;
        r.shift.resize(n);
        r.mass.resize(n);
        const std::uint32_t none = 0;
        const sbr_status st = sbr_log_partition_reps(replicas_->primary(), reps.data(), (std::uint64_t)n, excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                     excl_ptr.empty() ? nullptr : (excl_items.empty() ? &none : excl_items.data()), temperature,
                                                     filtered ? any.data() : nullptr, filtered ? none_of.data() : nullptr, r.shift.data(),
                                                     r.mass.data(), &r.frac_bits);
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Partition, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_log_partition_reps");
        return Result<Partition, PredictionError>::Ok(std::move(r));
    }

    /// `recommend` with every item outside `among` ineligible (sbr_recommend_among): the exact top k of that item set — ids in any
    /// order, duplicates allowed — as catalogue ids, ordered and padded as `recommend`'s rows.  Only the set's rows are scanned: an
    /// empty set gives rows of padding, and a non-finite score outside the set does not fail the call.
    Result<Recommendations, PredictionError> recommend(const data::CompressedInteractions& interactions, std::size_t k, bool exclude_history,
                                                       const std::vector<ItemId>& among) const {
        if (k < 1 || k > SBR_RECOMMEND_MAX_K) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "recommend: k outside 1..SBR_RECOMMEND_MAX_K");
        const std::vector<std::uint32_t> subset = narrow(among);
        Recommendations r;
        r.num_users = interactions.num_users();
        r.k = k;
        r.items.resize(r.num_users * k);
        r.scores.resize(r.num_users * k);
        const sbr_status st = sbr_recommend_among(replicas_->primary(), interactions.user_pointers().data(), interactions.item_ids().data(),
                                                  (std::uint64_t)r.num_users, (std::uint32_t)k, exclude_history ? 0u : SBR_RECOMMEND_INCLUDE_HISTORY,
                                                  subset.data(), (std::uint64_t)subset.size(), r.items.data(), r.scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Recommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_recommend_among");
        return Result<Recommendations, PredictionError>::Ok(std::move(r));
    }

    /// The largest `pool` of recommend_diverse on this model (sbr_recommend_diverse_max_pool): a user's pool lives in one
    /// workgroup's LDS, min(1024, 32768 / storage width) rows.
    std::size_t diverse_max_pool() const {
        std::uint32_t p = 0;
        check(sbr_recommend_diverse_max_pool(replicas_->primary(), &p), "sbr_recommend_diverse_max_pool");
        return (std::size_t)p;
    }

    /// `recommend` without the near-duplicates (sbr_recommend_diverse): from each user's `pool` best items — recommend's row at
    /// k = pool — k are picked greedily by maximal marginal relevance, trade_off * score - (1 - trade_off) * (the largest
    /// similarity to an item already picked), similarity as `similar_items` measures it; the first pick is the best item.  Rows
    /// in pick order with `recommend`'s score bits, padded with (0xFFFFFFFF, -inf).  pool = 0: min(4 k, diverse_max_pool()).
    /// trade_off = 1 is recommend(k).  Err(InvalidPredictionValue) on a non-finite score, norm or similarity the selection uses.
    Result<Recommendations, PredictionError> recommend_diverse(const data::CompressedInteractions& interactions, std::size_t k,
                                                               std::size_t pool = 0, float trade_off = 0.5f,
                                                               Similarity metric = Similarity::Cosine, bool exclude_history = true) const {
        if (pool == 0) pool = std::min<std::size_t>(4 * k, diverse_max_pool());
        if (k < 1 || pool < k || pool > SBR_DIVERSE_MAX_POOL)
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "recommend_diverse: 1 <= k <= pool <= SBR_DIVERSE_MAX_POOL");
        Recommendations r;
        r.num_users = interactions.num_users();
        r.k = k;
        r.items.resize(r.num_users * k);
        r.scores.resize(r.num_users * k);
        const sbr_status st = sbr_recommend_diverse(replicas_->primary(), interactions.user_pointers().data(), interactions.item_ids().data(),
                                                    (std::uint64_t)r.num_users, (std::uint32_t)k, (std::uint32_t)pool, trade_off,
                                                    (std::uint32_t)metric, exclude_history ? 0u : SBR_RECOMMEND_INCLUDE_HISTORY,
                                                    r.items.data(), r.scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Recommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_recommend_diverse");
        return Result<Recommendations, PredictionError>::Ok(std::move(r));
    }

    /// `recommend_diverse` under a per-user tag filter (sbr_recommend_diverse_filtered): the pool is the filtered row at k = pool.
    Result<Recommendations, PredictionError> recommend_diverse_filtered(const data::CompressedInteractions& interactions, std::size_t k,
                                                                        std::size_t pool, float trade_off, Similarity metric,
                                                                        bool exclude_history, const TagFilter& filter) const {
        if (pool == 0) pool = std::min<std::size_t>(4 * k, diverse_max_pool());
        if (k < 1 || pool < k || pool > SBR_DIVERSE_MAX_POOL)
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "recommend_diverse: 1 <= k <= pool <= SBR_DIVERSE_MAX_POOL");
        Recommendations r;
        r.num_users = interactions.num_users();
        r.k = k;
        r.items.resize(r.num_users * k);
        r.scores.resize(r.num_users * k);
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, r.num_users, "recommend_diverse: one any_of mask per user");
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, r.num_users, "recommend_diverse: one none_of mask per user");
        const sbr_status st = sbr_recommend_diverse_filtered(replicas_->primary(), interactions.user_pointers().data(),
                                                             interactions.item_ids().data(), (std::uint64_t)r.num_users, (std::uint32_t)k,
                                                             (std::uint32_t)pool, trade_off, (std::uint32_t)metric,
                                                             exclude_history ? 0u : SBR_RECOMMEND_INCLUDE_HISTORY, any.data(), none_of.data(),
                                                             r.items.data(), r.scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Recommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_recommend_diverse_filtered");
        return Result<Recommendations, PredictionError>::Ok(std::move(r));
    }

    /// `user_representation` of every history of `histories` in one device pass (sbr_user_representations): row-major
    /// [num_users][embedding_dim], row u with the bits of the single call on history u.
    std::vector<float> user_representations(const data::CompressedInteractions& histories) const {
        std::vector<float> reps(histories.num_users() * (std::size_t)replicas_->hparams().embedding_dim);
        check(sbr_user_representations(replicas_->primary(), histories.user_pointers().data(), histories.item_ids().data(),
                                       (std::uint64_t)histories.num_users(), reps.data()),
              "sbr_user_representations");
        return reps;
    }

    /// The reverse of `recommend` over caller-supplied representations (sbr_audience_reps): row j of the result holds, for query
    /// item items[j], the k rows of `reps` (row-major [num_rows][embedding_dim]) that score it highest — `items` of the result are
    /// ROW indices, the scores have the bits of `predict`, score descending, ties to the lower row, short rows padded with
    /// (0xFFFFFFFF, -inf).  Query j's excluded rows are excl_rows[excl_ptr[j] .. excl_ptr[j + 1]) (both empty: none).
    Result<Recommendations, PredictionError> audience_reps(const std::vector<float>& reps, const std::vector<ItemId>& items, std::size_t k,
                                                           const std::vector<std::uint64_t>& excl_ptr = {},
                                                           const std::vector<std::uint32_t>& excl_rows = {}) const {
        const std::size_t dim = (std::size_t)replicas_->hparams().embedding_dim;
        if (k < 1 || k > SBR_RECOMMEND_MAX_K) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "audience_reps: k outside 1..SBR_RECOMMEND_MAX_K");
        if (reps.size() % dim) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "audience_reps: rows of embedding_dim floats");
        if (!excl_ptr.empty() && (excl_ptr.size() != items.size() + 1 || excl_ptr.back() > excl_rows.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "audience_reps: one exclusion range per query");
        const std::vector<std::uint32_t> q = narrow(items);
        Recommendations r;
        r.num_users = q.size();
        r.k = k;
        r.items.resize(r.num_users * k);
        r.scores.resize(r.num_users * k);
        const std::uint32_t none = 0;
        const float zero = 0.0f;
        const sbr_status st = sbr_audience_reps(replicas_->primary(), reps.empty() ? &zero : reps.data(), (std::uint64_t)(reps.size() / dim),
                                                q.data(), (std::uint64_t)q.size(), (std::uint32_t)k, excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                excl_ptr.empty() ? nullptr : (excl_rows.empty() ? &none : excl_rows.data()), r.items.data(),
                                                r.scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Recommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_audience_reps");
        return Result<Recommendations, PredictionError>::Ok(std::move(r));
    }

    /// `audience_reps` on `user_representations` of `histories` (sbr_audience): `items` of the result are USER indices.  With
    /// `exclude_history` a user whose history holds the query item is left out of that item's row.
    Result<Recommendations, PredictionError> audience(const data::CompressedInteractions& histories, const std::vector<ItemId>& items,
                                                      std::size_t k, bool exclude_history = true) const {
        if (k < 1 || k > SBR_RECOMMEND_MAX_K) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "audience: k outside 1..SBR_RECOMMEND_MAX_K");
        const std::vector<std::uint32_t> q = narrow(items);
        Recommendations r;
        r.num_users = q.size();
        r.k = k;
        r.items.resize(r.num_users * k);
        r.scores.resize(r.num_users * k);
        const sbr_status st = sbr_audience(replicas_->primary(), histories.user_pointers().data(), histories.item_ids().data(),
                                           (std::uint64_t)histories.num_users(), q.data(), (std::uint64_t)q.size(), (std::uint32_t)k,
                                           exclude_history ? 0u : SBR_RECOMMEND_INCLUDE_HISTORY, r.items.data(), r.scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Recommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_audience");
        return Result<Recommendations, PredictionError>::Ok(std::move(r));
    }

  private:
    /// The body the *_above and *_top forms share: `me` names the calling method in refusals, `bar` holds the thresholds or the
    /// budgets.
    Result<Above, PredictionError> recommend_bar(const char* me, const data::CompressedInteractions& interactions, detail::Bar bar,
                                                   bool exclude_history, const TagFilter& filter,
                                                   std::uint64_t max_results, AboveOrder order,
                                                   bool count_only) const {
        const std::size_t n = interactions.num_users();
        const bool filtered = !filter.any_of.empty() || !filter.none_of.empty();
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, n, (std::string(me) + ": one any_of mask per user").c_str());
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, n, (std::string(me) + ": one none_of mask per user").c_str());
        bar.fit(n, me, "user");
        Above r;
        const sbr_status st = detail::above_call(
            [&](std::uint64_t* counts, std::uint64_t* total, std::uint64_t cap, std::uint32_t* ids, float* scores) {
                if (bar.top)
                    return sbr_recommend_top(replicas_->primary(), interactions.user_pointers().data(), interactions.item_ids().data(), (std::uint64_t)n,
                                               bar.n.data(), exclude_history ? 0u : SBR_RECOMMEND_INCLUDE_HISTORY, filtered ? any.data() : nullptr,
                                               filtered ? none_of.data() : nullptr, bar.cuts.data(), counts, total, cap, ids, scores);
                return sbr_recommend_above(replicas_->primary(), interactions.user_pointers().data(), interactions.item_ids().data(), (std::uint64_t)n,
                                           bar.th.data(), exclude_history ? 0u : SBR_RECOMMEND_INCLUDE_HISTORY, filtered ? any.data() : nullptr,
                                           filtered ? none_of.data() : nullptr, counts, total, cap, ids, scores);
            },
            n, max_results, order, count_only, bar.top ? "sbr_recommend_top" : "sbr_recommend_above", bar, &r);
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Above, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        return Result<Above, PredictionError>::Ok(std::move(r));
    }
  public:
    /// `recommend` without a k (sbr_recommend_above): for each user's history EVERY eligible item whose score is >= its threshold
    /// — `thresholds`: one value for all users or one per user; the f32 compare, so ties at the bar all pass, -0.0 == +0.0, -inf
    /// returns every eligible item and +inf none.  An Above over the users, item ids with `predict`'s score bits, each row by score
    /// descending with ties to the lower id (AboveOrder::Id: ascending id): with the threshold at `recommend(k)`'s k-th score a row
    /// starts with that call's row.  Eligibility (`exclude_history`, `filter`) is `recommend`'s.  More than `max_results` pairs throw
    /// an EngineError that states the total; `count_above` costs one scan and says how many to expect.
    Result<Above, PredictionError> recommend_above(const data::CompressedInteractions& interactions, const std::vector<float>& thresholds,
                                                   bool exclude_history = true, const TagFilter& filter = {},
                                                   std::uint64_t max_results = ABOVE_MAX_RESULTS, AboveOrder order = AboveOrder::Score,
                                                   bool count_only = false) const {
        return recommend_bar("recommend_above",
                             interactions, detail::Bar::above(thresholds), exclude_history, filter, max_results, order, count_only);
    }
    /// `recommend` with a budget in place of k (sbr_recommend_top): each user's exact best n eligible items — `n`: one value for all
    /// users or one per user, any size (no SBR_RECOMMEND_MAX_K; 0: an empty row; past the eligible items: all of them).  An Above
    /// with `cuts`: for n <= SBR_RECOMMEND_MAX_K a row is `recommend(k = n)`'s without padding, for any n the first n of
    /// `recommend_above(cuts[row])`'s; of a tie group that straddles the cut exactly the lowest ids are kept.  count_only: the select
    /// alone — cuts and counts, no pair.  max_results is held against the pairs returned.
    Result<Above, PredictionError> recommend_top(const data::CompressedInteractions& interactions, const std::vector<std::uint64_t>& n,
                                                 bool exclude_history = true, const TagFilter& filter = {},
                                                 std::uint64_t max_results = ABOVE_MAX_RESULTS, AboveOrder order = AboveOrder::Score,
                                                 bool count_only = false) const {
        return recommend_bar("recommend_top",
                             interactions, detail::Bar::best(n), exclude_history, filter, max_results, order, count_only);
    }
    /// The rows' counts of `recommend_above` (its `ptr`; `ids` / `scores` stay empty) without writing any pair: one scan.
    Result<Above, PredictionError> count_above(const data::CompressedInteractions& interactions, const std::vector<float>& thresholds,
                                               bool exclude_history = true, const TagFilter& filter = {}) const {
        return recommend_above(interactions, thresholds, exclude_history, filter, 0, AboveOrder::Id, true);
    }
  private:
    /// The body the *_above and *_top forms share: `me` names the calling method in refusals, `bar` holds the thresholds or the
    /// budgets.
    Result<Above, PredictionError> recommend_reps_bar(const char* me, const std::vector<float>& reps, detail::Bar bar,
                                                        const std::vector<std::uint64_t>& excl_ptr,
                                                        const std::vector<std::uint32_t>& excl_items, const TagFilter& filter,
                                                        std::uint64_t max_results, AboveOrder order,
                                                        bool count_only) const {
        const std::size_t dim = (std::size_t)replicas_->hparams().embedding_dim;
        if (reps.size() % dim) throw EngineError(SBR_ERR_INVALID_ARGUMENT, (std::string(me) + ": rows of embedding_dim floats").c_str());
        const std::size_t n = reps.size() / dim;
        if (!excl_ptr.empty() && (excl_ptr.size() != n + 1 || excl_ptr.back() > excl_items.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, (std::string(me) + ": one exclusion range per user").c_str());
        const bool filtered = !filter.any_of.empty() || !filter.none_of.empty();
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, n, (std::string(me) + ": one any_of mask per user").c_str());
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, n, (std::string(me) + ": one none_of mask per user").c_str());
        bar.fit(n, me, "user");
        const std::uint32_t none = 0;
        const float zero = 0.0f;
        Above r;
        const sbr_status st = detail::above_call(
            [&](std::uint64_t* counts, std::uint64_t* total, std::uint64_t cap, std::uint32_t* ids, float* scores) {
                if (bar.top)
                    return sbr_recommend_top_reps(replicas_->primary(), reps.empty() ? &zero : reps.data(), (std::uint64_t)n, bar.n.data(),
                                                    excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                    excl_ptr.empty() ? nullptr : (excl_items.empty() ? &none : excl_items.data()),
                                                    filtered ? any.data() : nullptr, filtered ? none_of.data() : nullptr, bar.cuts.data(), counts, total, cap, ids, scores);
                return sbr_recommend_above_reps(replicas_->primary(), reps.empty() ? &zero : reps.data(), (std::uint64_t)n, bar.th.data(),
                                                excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                excl_ptr.empty() ? nullptr : (excl_items.empty() ? &none : excl_items.data()),
                                                filtered ? any.data() : nullptr, filtered ? none_of.data() : nullptr, counts, total, cap, ids, scores);
            },
            n, max_results, order, count_only, bar.top ? "sbr_recommend_top_reps" : "sbr_recommend_above_reps", bar, &r);
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Above, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        return Result<Above, PredictionError>::Ok(std::move(r));
    }
  public:
    /// recommend_above from representations, reps [num_users][embedding_dim] (sbr_recommend_above_reps); excl_ptr / excl_items:
    /// per-user exclusion lists as a CSR (both empty: none).
    Result<Above, PredictionError> recommend_above_reps(const std::vector<float>& reps, const std::vector<float>& thresholds,
                                                        const std::vector<std::uint64_t>& excl_ptr = {},
                                                        const std::vector<std::uint32_t>& excl_items = {}, const TagFilter& filter = {},
                                                        std::uint64_t max_results = ABOVE_MAX_RESULTS, AboveOrder order = AboveOrder::Score,
                                                        bool count_only = false) const {
        return recommend_reps_bar("recommend_above_reps",
                                  reps, detail::Bar::above(thresholds), excl_ptr, excl_items, filter, max_results, order, count_only);
    }
    /// recommend_top from representations, reps [num_users][embedding_dim] (sbr_recommend_top_reps).
    Result<Above, PredictionError> recommend_top_reps(const std::vector<float>& reps, const std::vector<std::uint64_t>& n,
                                                      const std::vector<std::uint64_t>& excl_ptr = {},
                                                      const std::vector<std::uint32_t>& excl_items = {}, const TagFilter& filter = {},
                                                      std::uint64_t max_results = ABOVE_MAX_RESULTS, AboveOrder order = AboveOrder::Score,
                                                      bool count_only = false) const {
        return recommend_reps_bar("recommend_top_reps",
                                  reps, detail::Bar::best(n), excl_ptr, excl_items, filter, max_results, order, count_only);
    }
    /// The rows' counts of `recommend_above_reps` without writing any pair: one scan.
    Result<Above, PredictionError> count_above_reps(const std::vector<float>& reps, const std::vector<float>& thresholds,
                                                    const std::vector<std::uint64_t>& excl_ptr = {},
                                                    const std::vector<std::uint32_t>& excl_items = {}, const TagFilter& filter = {}) const {
        return recommend_above_reps(reps, thresholds, excl_ptr, excl_items, filter, 0, AboveOrder::Id, true);
    }
  private:
    /// The body the *_above and *_top forms share: `me` names the calling method in refusals, `bar` holds the thresholds or the
    /// budgets.
    Result<Above, PredictionError> audience_reps_bar(const char* me, const std::vector<float>& reps, const std::vector<ItemId>& items,
                                                       detail::Bar bar, const std::vector<std::uint64_t>& excl_ptr,
                                                       const std::vector<std::uint32_t>& excl_rows,
                                                       std::uint64_t max_results, AboveOrder order,
                                                       bool count_only) const {
        const std::size_t dim = (std::size_t)replicas_->hparams().embedding_dim;
        if (reps.size() % dim) throw EngineError(SBR_ERR_INVALID_ARGUMENT, (std::string(me) + ": rows of embedding_dim floats").c_str());
        if (!excl_ptr.empty() && (excl_ptr.size() != items.size() + 1 || excl_ptr.back() > excl_rows.size()))
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, (std::string(me) + ": one exclusion range per query").c_str());
        const std::vector<std::uint32_t> q = narrow(items);
        bar.fit(q.size(), me, "query");
        const std::uint32_t none = 0;
        const float zero = 0.0f;
        Above r;
        const sbr_status st = detail::above_call(
            [&](std::uint64_t* counts, std::uint64_t* total, std::uint64_t cap, std::uint32_t* ids, float* scores) {
                if (bar.top)
                    return sbr_audience_top_reps(replicas_->primary(), reps.empty() ? &zero : reps.data(), (std::uint64_t)(reps.size() / dim), q.data(),
                                                   (std::uint64_t)q.size(), bar.n.data(), excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                                   excl_ptr.empty() ? nullptr : (excl_rows.empty() ? &none : excl_rows.data()), bar.cuts.data(), counts, total, cap, ids,
                                                   scores);
                return sbr_audience_above_reps(replicas_->primary(), reps.empty() ? &zero : reps.data(), (std::uint64_t)(reps.size() / dim), q.data(),
                                               (std::uint64_t)q.size(), bar.th.data(), excl_ptr.empty() ? nullptr : excl_ptr.data(),
                                               excl_ptr.empty() ? nullptr : (excl_rows.empty() ? &none : excl_rows.data()), counts, total, cap, ids,
                                               scores);
            },
            q.size(), max_results, order, count_only, bar.top ? "sbr_audience_top_reps" : "sbr_audience_above_reps", bar, &r);
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Above, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        return Result<Above, PredictionError>::Ok(std::move(r));
    }
  public:
    /// `audience_reps` without a k (sbr_audience_above_reps): for each query item EVERY row of `reps` that scores it >= its threshold
    /// (`thresholds`: one for all queries or one per query) — `ids` of the result are ROW indices.
    Result<Above, PredictionError> audience_above_reps(const std::vector<float>& reps, const std::vector<ItemId>& items,
                                                       const std::vector<float>& thresholds, const std::vector<std::uint64_t>& excl_ptr = {},
                                                       const std::vector<std::uint32_t>& excl_rows = {},
                                                       std::uint64_t max_results = ABOVE_MAX_RESULTS, AboveOrder order = AboveOrder::Score,
                                                       bool count_only = false) const {
        return audience_reps_bar("audience_above_reps",
                                 reps, items, detail::Bar::above(thresholds), excl_ptr, excl_rows, max_results, order, count_only);
    }
    /// `audience_reps` with a budget in place of k (sbr_audience_top_reps): for each query item its exact best n rows of `reps` —
    /// `n`: one value for all queries or one per query, any size; an Above with `cuts`, ROW indices.
    Result<Above, PredictionError> audience_top_reps(const std::vector<float>& reps, const std::vector<ItemId>& items,
                                                     const std::vector<std::uint64_t>& n, const std::vector<std::uint64_t>& excl_ptr = {},
                                                     const std::vector<std::uint32_t>& excl_rows = {},
                                                     std::uint64_t max_results = ABOVE_MAX_RESULTS, AboveOrder order = AboveOrder::Score,
                                                     bool count_only = false) const {
        return audience_reps_bar("audience_top_reps",
                                 reps, items, detail::Bar::best(n), excl_ptr, excl_rows, max_results, order, count_only);
    }
    /// The rows' counts of `audience_above_reps` without writing any pair: one scan.
    Result<Above, PredictionError> count_audience_above_reps(const std::vector<float>& reps, const std::vector<ItemId>& items,
                                                             const std::vector<float>& thresholds, const std::vector<std::uint64_t>& excl_ptr = {},
                                                             const std::vector<std::uint32_t>& excl_rows = {}) const {
        return audience_above_reps(reps, items, thresholds, excl_ptr, excl_rows, 0, AboveOrder::Id, true);
    }
  private:
    /// The body the *_above and *_top forms share: `me` names the calling method in refusals, `bar` holds the thresholds or the
    /// budgets.
    Result<Above, PredictionError> audience_bar(const char* me, const data::CompressedInteractions& histories, const std::vector<ItemId>& items,
                                                  detail::Bar bar, bool exclude_history,
                                                  std::uint64_t max_results, AboveOrder order,
                                                  bool count_only) const {
        const std::vector<std::uint32_t> q = narrow(items);
        bar.fit(q.size(), me, "query");
        Above r;
        const sbr_status st = detail::above_call(
            [&](std::uint64_t* counts, std::uint64_t* total, std::uint64_t cap, std::uint32_t* ids, float* scores) {
                if (bar.top)
                    return sbr_audience_top(replicas_->primary(), histories.user_pointers().data(), histories.item_ids().data(),
                                              (std::uint64_t)histories.num_users(), q.data(), (std::uint64_t)q.size(), bar.n.data(),
                                              exclude_history ? 0u : SBR_RECOMMEND_INCLUDE_HISTORY, bar.cuts.data(), counts, total, cap, ids, scores);
                return sbr_audience_above(replicas_->primary(), histories.user_pointers().data(), histories.item_ids().data(),
                                          (std::uint64_t)histories.num_users(), q.data(), (std::uint64_t)q.size(), bar.th.data(),
                                          exclude_history ? 0u : SBR_RECOMMEND_INCLUDE_HISTORY, counts, total, cap, ids, scores);
            },
            q.size(), max_results, order, count_only, bar.top ? "sbr_audience_top" : "sbr_audience_above", bar, &r);
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Above, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        return Result<Above, PredictionError>::Ok(std::move(r));
    }
  public:
    /// `audience_above_reps` on `user_representations` of `histories` (sbr_audience_above): `ids` of the result are USER indices.
    /// With `exclude_history` a user whose history holds the query item is left out of that item's row.
    Result<Above, PredictionError> audience_above(const data::CompressedInteractions& histories, const std::vector<ItemId>& items,
                                                  const std::vector<float>& thresholds, bool exclude_history = true,
                                                  std::uint64_t max_results = ABOVE_MAX_RESULTS, AboveOrder order = AboveOrder::Score,
                                                  bool count_only = false) const {
        return audience_bar("audience_above",
                            histories, items, detail::Bar::above(thresholds), exclude_history, max_results, order, count_only);
    }
    /// `audience_top_reps` on `user_representations` of `histories` (sbr_audience_top): USER indices.
    Result<Above, PredictionError> audience_top(const data::CompressedInteractions& histories, const std::vector<ItemId>& items,
                                                const std::vector<std::uint64_t>& n, bool exclude_history = true,
                                                std::uint64_t max_results = ABOVE_MAX_RESULTS, AboveOrder order = AboveOrder::Score,
                                                bool count_only = false) const {
        return audience_bar("audience_top",
                            histories, items, detail::Bar::best(n), exclude_history, max_results, order, count_only);
    }
    /// The rows' counts of `audience_above` without writing any pair.
    Result<Above, PredictionError> count_audience_above(const data::CompressedInteractions& histories, const std::vector<ItemId>& items,
                                                        const std::vector<float>& thresholds, bool exclude_history = true) const {
        return audience_above(histories, items, thresholds, exclude_history, 0, AboveOrder::Id, true);
    }

    /// `predict` for many users in one device pass (sbr_score_candidates): user u's history is row u of `histories`, its
    /// candidates cand_items[cand_ptr[u] .. cand_ptr[u + 1]) (any order, duplicates allowed, none included).  One score per
    /// candidate, in candidate order, with the bits of `predict`; nothing is masked.  Err(InvalidPredictionValue) on a
    /// non-finite score.
    Result<std::vector<float>, PredictionError> score_candidates(const data::CompressedInteractions& histories,
                                                                 const std::vector<std::uint64_t>& cand_ptr,
                                                                 const std::vector<std::uint32_t>& cand_items) const {
        using R = Result<std::vector<float>, PredictionError>;
        if (cand_ptr.size() != histories.num_users() + 1 || cand_ptr.back() < cand_ptr.front() || cand_ptr.back() > cand_items.size())
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "score_candidates: one candidate range per user");
        std::vector<float> scores(cand_ptr.back() - cand_ptr.front());
        const sbr_status st = sbr_score_candidates(replicas_->primary(), histories.user_pointers().data(), histories.item_ids().data(),
                                                   (std::uint64_t)histories.num_users(), cand_ptr.data(), cand_items.data(), scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return R::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_score_candidates");
        return R::Ok(std::move(scores));
    }

    /// The k items most like each of `items` among the whole catalogue (sbr_similar_items): row j of the result is query
    /// items[j]'s, by the cosine of the item embeddings (or their dot product; the item bias takes no part), score descending,
    /// ties to the lower item id.  The query is left out of its own row unless `include_self`; a row with fewer than k eligible
    /// items is padded with (0xFFFFFFFF, -inf).  Err(InvalidPredictionValue) on a non-finite norm or score.
    Result<Recommendations, PredictionError> similar_items(const std::vector<ItemId>& items, std::size_t k,
                                                           Similarity metric = Similarity::Cosine, bool include_self = false) const {
        if (k < 1 || k > SBR_RECOMMEND_MAX_K) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "similar_items: k outside 1..SBR_RECOMMEND_MAX_K");
        const std::vector<std::uint32_t> ids = narrow(items);
        Recommendations r;
        r.num_users = ids.size();
        r.k = k;
        r.items.resize(r.num_users * k);
        r.scores.resize(r.num_users * k);
        const sbr_status st = sbr_similar_items(replicas_->primary(), ids.data(), (std::uint64_t)ids.size(), (std::uint32_t)k,
                                                (std::uint32_t)metric, include_self ? SBR_SIMILAR_INCLUDE_SELF : 0u, nullptr, nullptr,
                                                r.items.data(), r.scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Recommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_similar_items");
        return Result<Recommendations, PredictionError>::Ok(std::move(r));
    }

    /// `similar_items` under a tag filter with one mask pair per query (sbr_similar_items_filtered): "similar items of the same
    /// category" is any_of[j] = the tag word of items[j].
    Result<Recommendations, PredictionError> similar_items_filtered(const std::vector<ItemId>& items, std::size_t k, Similarity metric,
                                                                    bool include_self, const TagFilter& filter) const {
        if (k < 1 || k > SBR_RECOMMEND_MAX_K) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "similar_items: k outside 1..SBR_RECOMMEND_MAX_K");
        const std::vector<std::uint32_t> ids = narrow(items);
        Recommendations r;
        r.num_users = ids.size();
        r.k = k;
        r.items.resize(r.num_users * k);
        r.scores.resize(r.num_users * k);
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, ids.size(), "similar_items: one any_of mask per query");
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, ids.size(), "similar_items: one none_of mask per query");
        const sbr_status st = sbr_similar_items_filtered(replicas_->primary(), ids.data(), (std::uint64_t)ids.size(), (std::uint32_t)k,
                                                         (std::uint32_t)metric, include_self ? SBR_SIMILAR_INCLUDE_SELF : 0u, nullptr, nullptr,
                                                         any.data(), none_of.data(), r.items.data(), r.scores.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return Result<Recommendations, PredictionError>::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_similar_items_filtered");
        return Result<Recommendations, PredictionError>::Ok(std::move(r));
    }

    /// Exact ranks of each user's targets among the whole catalogue from ONE device scan (sbr_rank_targets): user u's history is
    /// row u of `histories`, its targets target_items[target_ptr[u] .. target_ptr[u + 1]).  rank = #{items whose masked score >=
    /// the target's}: the target counts itself, ties count against it, the WHOLE history is masked to f32::MIN unless
    /// `mask_history` is false (a target inside it then has rank num_items).  One rank per target, in target order.
    /// Err(InvalidPredictionValue) on a non-finite score.
    Result<std::vector<std::uint32_t>, PredictionError> rank_targets(const data::CompressedInteractions& histories,
                                                                     const std::vector<std::uint64_t>& target_ptr,
                                                                     const std::vector<std::uint32_t>& target_items,
                                                                     bool mask_history = true) const {
        using R = Result<std::vector<std::uint32_t>, PredictionError>;
        if (target_ptr.size() != histories.num_users() + 1 || target_ptr.back() - target_ptr.front() > target_items.size())
            throw EngineError(SBR_ERR_INVALID_ARGUMENT, "rank_targets: one target range per user");
        std::vector<std::uint32_t> ranks(target_ptr.back() - target_ptr.front());
        const sbr_status st = sbr_rank_targets(replicas_->primary(), histories.user_pointers().data(), histories.item_ids().data(),
                                               (std::uint64_t)histories.num_users(), target_ptr.data(), target_items.data(),
                                               mask_history ? 0u : SBR_RANK_INCLUDE_HISTORY, ranks.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return R::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_rank_targets");
        return R::Ok(std::move(ranks));
    }

    /// rank_targets among what each user may be shown (sbr_rank_targets_rows): every item the filter forbids is masked to f32::MIN
    /// as the history is, so a forbidden target has rank num_items; an empty filter is the call above.  Needs set_item_tags.
    Result<std::vector<std::uint32_t>, PredictionError> rank_targets(const data::CompressedInteractions& histories,
                                                                     const std::vector<std::uint64_t>& target_ptr,
                                                                     const std::vector<std::uint32_t>& target_items, const TagFilter& filter,
                                                                     bool mask_history = true) const {
        if (filter.any_of.empty() && filter.none_of.empty()) return rank_targets(histories, target_ptr, target_items, mask_history);
        const std::size_t n = histories.num_users();
        const std::vector<std::uint32_t> any = tag_masks(filter.any_of, n, "rank_targets: one any_of mask per user");
        const std::vector<std::uint32_t> none_of = tag_masks(filter.none_of, n, "rank_targets: one none_of mask per user");
        static const std::uint32_t none = 0;
        sbr_scan_rows d{};
        d.user_ptr = histories.user_pointers().data();
        d.item_ids = histories.item_ids().empty() ? &none : histories.item_ids().data();
        d.flags = mask_history ? 0u : SBR_RECOMMEND_INCLUDE_HISTORY;
        d.any_of = any.data();
        d.none_of = none_of.data();
        return detail::eligible_ranks(replicas_->primary(), nullptr, d, n, target_ptr, target_items, "sbr_rank_targets_rows");
    }

    /// Exact next-item rank at every position of every sequence from one forward pass per sequence (sbr_sequence_ranks): with
    /// W = min(n, max_sequence_length + 1) and w the last W items of user u, position p = 1 .. W - 1 ranks w[p] against the state
    /// after w[0 .. p), the distinct items of that prefix masked to f32::MIN unless `mask_history` is false — the number
    /// rank_targets(history = w[0 .. p), targets = { w[p] }) gives.  `last` (0 = all) keeps only the last `last` positions of each
    /// window.  Row u of the result holds its positions ascending and is empty for n < 2.  Err(InvalidPredictionValue) on a
    /// non-finite score.
    Result<SequenceRanks, PredictionError> sequence_ranks(const data::CompressedInteractions& test, bool mask_history = true,
                                                          std::size_t last = 0) const {
        using R = Result<SequenceRanks, PredictionError>;
        if (last > 0xFFFFFFFFull) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "sequence_ranks: last does not fit 32 bits");
        const std::uint32_t flags = mask_history ? 0u : SBR_RANK_INCLUDE_HISTORY;
        SequenceRanks r;
        r.ptr.assign(test.num_users() + 1, 0);
        check(sbr_sequence_ranks(replicas_->primary(), test.user_pointers().data(), test.item_ids().data(), (std::uint64_t)test.num_users(),
                                 flags, (std::uint32_t)last, r.ptr.data(), nullptr), "sbr_sequence_ranks");  // sizing: no device work
        r.ranks.assign(r.ptr.back() + 1, 0);
        const sbr_status st = sbr_sequence_ranks(replicas_->primary(), test.user_pointers().data(), test.item_ids().data(),
                                                 (std::uint64_t)test.num_users(), flags, (std::uint32_t)last, r.ptr.data(), r.ranks.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return R::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_sequence_ranks");
        r.ranks.resize(r.ptr.back());
        return R::Ok(std::move(r));
    }

    /// What softmax(score / temperature) needs to price the next item at every position of every sequence, from one forward pass
    /// per sequence (sbr_sequence_partition): windows, positions, `last` and the rows are sequence_ranks'; per kept position p the
    /// shift and mass are log_partition's for the explicit history w[0 .. p) bit for bit, `scores` the plain score of w[p] and
    /// `masked` 1 where the prefix is masked and w[p] occurs in it.  SequencePartition::log_probs gives the log-probabilities.
    /// Err(InvalidPredictionValue) on a non-finite score.
    Result<SequencePartition, PredictionError> sequence_partition(const data::CompressedInteractions& test, float temperature = 1.0f,
                                                                  bool mask_history = true, std::size_t last = 0) const {
        using R = Result<SequencePartition, PredictionError>;
        if (last > 0xFFFFFFFFull) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "sequence_partition: last does not fit 32 bits");
        const std::uint32_t flags = mask_history ? 0u : SBR_RANK_INCLUDE_HISTORY;
        SequencePartition r;
        r.ptr.assign(test.num_users() + 1, 0);
        check(sbr_sequence_partition(replicas_->primary(), test.user_pointers().data(), test.item_ids().data(), (std::uint64_t)test.num_users(),
                                     temperature, flags, (std::uint32_t)last, r.ptr.data(), nullptr, nullptr, nullptr, nullptr),
              "sbr_sequence_partition");  // sizing: no device work
        const std::size_t n = (std::size_t)r.ptr.back();
        r.partition.temperature = temperature;
        r.partition.frac_bits = sbr_softmax_frac_bits((std::uint32_t)replicas_->hparams().num_items);
        r.partition.shift.assign(n + 1, 0.0f);
        r.partition.mass.assign(n + 1, 0);
        r.scores.assign(n + 1, 0.0f);
        r.masked.assign(n + 1, 0);
        const sbr_status st = sbr_sequence_partition(replicas_->primary(), test.user_pointers().data(), test.item_ids().data(),
                                                     (std::uint64_t)test.num_users(), temperature, flags, (std::uint32_t)last, r.ptr.data(),
                                                     r.partition.shift.data(), r.partition.mass.data(), r.scores.data(), r.masked.data());
        if (st == SBR_ERR_INVALID_PREDICTION) return R::Err(PredictionError::InvalidPredictionValue);
        check(st, "sbr_sequence_partition");
        r.partition.shift.resize(n);
        r.partition.mass.resize(n);
        r.scores.resize(n);
        r.masked.resize(n);
        return R::Ok(std::move(r));
    }

    /// Sessions::beam_search from histories, DEFINED as rollout's form is: a temporary store of one slot per user, `append` of each
    /// history's last max_sequence_length items, and the store's beam_search of all slots — with exclude_history each history's items
    /// as its exclusion list, replacing a.excl_ptr / a.excl_items.
    Result<Beams, PredictionError> beam_search(const data::CompressedInteractions& histories, BeamArgs a, bool exclude_history = true) const {
        const std::vector<std::uint64_t>& up = histories.user_pointers();
        const std::vector<std::uint32_t>& ids = histories.item_ids();
        const std::size_t n = histories.num_users(), T = (std::size_t)replicas_->hparams().max_sequence_length;
        if (n == 0) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "beam_search: at least one history");
        std::vector<std::uint32_t> slots(n), tail;
        std::vector<std::uint64_t> tail_ptr(n + 1, 0);
        for (std::size_t u = 0; u < n; ++u) {
            slots[u] = (std::uint32_t)u;
            const std::uint64_t keep = std::min<std::uint64_t>(up[u + 1] - up[u], T);
            tail.insert(tail.end(), ids.begin() + (std::ptrdiff_t)(up[u + 1] - keep), ids.begin() + (std::ptrdiff_t)up[u + 1]);
            tail_ptr[u + 1] = tail.size();
        }
        Sessions store = sessions(n);
        store.append(slots, tail_ptr, tail);
        a.include_seen = false;
        if (exclude_history) {
            a.excl_ptr.assign(up.begin(), up.end());
            for (std::uint64_t& p : a.excl_ptr) p -= up.front();
            a.excl_items.assign(ids.begin() + (std::ptrdiff_t)up.front(), ids.begin() + (std::ptrdiff_t)up.back());
        }
        return store.beam_search(slots, a);
    }

    /// Sessions::rollout from histories, DEFINED as this sequence of calls: a temporary store of one slot per user, `append` of each
    /// history's last max_sequence_length items, and the store's rollout of all slots — with exclude_history each history's items as
    /// its exclusion list, replacing a.excl_ptr / a.excl_items.  Streams default to the user's index, the slot id; a.lstm is set
    /// from the model.
    Result<Rollout, PredictionError> rollout(const data::CompressedInteractions& histories, RolloutArgs a, bool exclude_history = true) const {
        const std::vector<std::uint64_t>& up = histories.user_pointers();
        const std::vector<std::uint32_t>& ids = histories.item_ids();
        const std::size_t n = histories.num_users(), T = (std::size_t)replicas_->hparams().max_sequence_length;
        if (n == 0) throw EngineError(SBR_ERR_INVALID_ARGUMENT, "rollout: at least one history");
        std::vector<std::uint32_t> slots(n), tail;
        std::vector<std::uint64_t> tail_ptr(n + 1, 0);
        for (std::size_t u = 0; u < n; ++u) {
            slots[u] = (std::uint32_t)u;
            const std::uint64_t keep = std::min<std::uint64_t>(up[u + 1] - up[u], T);
            tail.insert(tail.end(), ids.begin() + (std::ptrdiff_t)(up[u + 1] - keep), ids.begin() + (std::ptrdiff_t)up[u + 1]);
            tail_ptr[u + 1] = tail.size();
        }
        Sessions store = sessions(n);
        store.append(slots, tail_ptr, tail);
        a.lstm = replicas_->hparams().model != 2;
        a.include_seen = false;
        if (exclude_history) {
            a.excl_ptr.assign(up.begin(), up.end());
            for (std::uint64_t& p : a.excl_ptr) p -= up.front();
            a.excl_items.assign(ids.begin() + (std::ptrdiff_t)up.front(), ids.begin() + (std::ptrdiff_t)up.back());
        }
        return store.rollout(slots, a);
    }

    /// A session store of `capacity` slots on the primary replica: device-resident user states advanced one appended item at a
    /// time (see Sessions).  Destroy it before this model.
    Sessions sessions(std::size_t capacity) const { return Sessions(replicas_->primary(), capacity, replicas_->hparams().embedding_dim); }
    /// The same with a seen-item memory of `seen_capacity` items per slot (1 .. SBR_SESSIONS_MAX_SEEN; 0: the store above), which
    /// the store's recommend calls exclude.
    Sessions sessions(std::size_t capacity, std::size_t seen_capacity) const {
        return Sessions(replicas_->primary(), capacity, replicas_->hparams().embedding_dim, seen_capacity);
    }

    /// An item set of this model on the primary replica (see ItemSet): `item_ids` in any order, duplicates allowed, each below
    /// num_items.  Destroy it before this model; call its refresh() after `fit`.
    ItemSet item_set(const std::vector<std::uint32_t>& item_ids) const {
        return ItemSet(replicas_->primary(), item_ids, replicas_->hparams().embedding_dim, replicas_->hparams().num_items,
                       replicas_->hparams().max_sequence_length, replicas_->hparams().model != 2);
    }

    /// The engine handle (replica 0), for evaluation's fused path and for parameter access.
    sbr_model* handle() const { return replicas_->primary(); }
    const sbr_hparams& hparams() const { return replicas_->hparams(); }

    /// One parameter block (sbr_param) — what the serde derives at lstm.rs:204,386 expose.
    std::vector<float> parameter(sbr_param which) const {
        std::uint64_t count = 0;
        check(sbr_model_param_count(handle(), which, &count), "sbr_model_param_count");
        std::vector<float> out(count);
        if (count) check(sbr_model_get_param(handle(), which, out.data(), count), "sbr_model_get_param");
        return out;
    }

    /// ≙ the serde derives on Hyperparameters / Parameters / the models (lstm.rs:38,204,386; ewma.rs:44,208,401; `bincode`
    /// in Cargo.toml:18): hyper-parameters, every parameter and optimiser-state block, the two counters and the state of
    /// the model RNG — everything the next `fit` depends on — in one little-endian file:
    ///   "SBRM" u32 version  u32 sizeof(sbr_hparams)  sbr_hparams  u8 partitioned  u64 epoch  u64 optimiser steps
    ///   u8 rng[16]  u32 blocks  { i32 which  u64 count  f32[count] } ...
    /// A model built with num_threads(n) stores ONE copy (replicas are bit-identical by construction).
    void save(const std::string& path) const {
        std::ofstream f(path, std::ios::binary);
        if (!f) throw std::runtime_error("save: cannot open " + path);
        auto put = [&](const void* p, std::size_t n) { f.write(reinterpret_cast<const char*>(p), (std::streamsize)n); };
        const std::uint32_t version = 1, hp_bytes = (std::uint32_t)sizeof(sbr_hparams);
        put("SBRM", 4); put(&version, 4); put(&hp_bytes, 4);
        const sbr_hparams hp = replicas_->hparams();
        put(&hp, sizeof hp);
        const std::uint8_t part = replicas_->partitioned() ? 1 : 0;
        put(&part, 1);
        std::uint64_t epoch = 0, steps = 0;
        check(sbr_model_get_counters(handle(), &epoch, &steps), "sbr_model_get_counters");
        put(&epoch, 8); put(&steps, 8);
        std::uint8_t rng[16];
        check(sbr_model_get_rng(handle(), rng), "sbr_model_get_rng");
        put(rng, 16);
        std::vector<std::pair<std::int32_t, std::vector<float>>> blocks;
        for (int w = SBR_PARAM_ITEM_EMBEDDING; w <= SBR_PARAM_EWMA_ALPHA_M; ++w) {
            std::vector<float> v = parameter((sbr_param)w);
            if (!v.empty()) blocks.emplace_back((std::int32_t)w, std::move(v));
        }
        const std::uint32_t nb = (std::uint32_t)blocks.size();
        put(&nb, 4);
        for (const auto& b : blocks) {
            const std::uint64_t count = b.second.size();
            put(&b.first, 4); put(&count, 8); put(b.second.data(), count * sizeof(float));
        }
        if (!f) throw std::runtime_error("save: write failed: " + path);
    }

  protected:
    /// Rebuilds the replicas of a saved model (one copy of a partitioned table, never n full tables) and restores the
    /// saved state into every one of them: the next `fit` is the one the saved model would have run.
    explicit ImplicitSequenceModel(const std::string& path, int expect_ewma) {
        std::ifstream f(path, std::ios::binary);
        if (!f) throw std::runtime_error("load: cannot open " + path);
        auto get = [&](void* p, std::size_t n) {
            f.read(reinterpret_cast<char*>(p), (std::streamsize)n);
            if (!f) throw std::runtime_error("load: truncated file: " + path);
        };
        char magic[4];
        std::uint32_t version = 0, hp_bytes = 0;
        get(magic, 4); get(&version, 4); get(&hp_bytes, 4);
        if (std::string(magic, 4) != "SBRM" || version != 1 || hp_bytes != sizeof(sbr_hparams))
            throw std::runtime_error("load: not a model file of this library version: " + path);
        sbr_hparams hp;
        get(&hp, sizeof hp);
        if ((hp.model == SBR_MODEL_EWMA) != (expect_ewma != 0)) throw std::runtime_error("load: the file holds the other model type: " + path);
        // a corrupt header must not size allocations or build replicas (sbr_model_create re-checks the rest)
        if (hp.num_items == 0 || hp.embedding_dim == 0 || hp.embedding_dim > 256 || hp.num_devices == 0 || hp.num_devices > 16 ||
            hp.device_rank != 0 || hp.batch_sequences == 0 || hp.max_sequence_length < 3 || hp.model < 0 || hp.model > 2)
            throw std::runtime_error("load: implausible hyper-parameters in " + path);
        std::uint8_t part = 0;
        get(&part, 1);
        std::uint64_t epoch = 0, steps = 0;
        get(&epoch, 8); get(&steps, 8);
        std::uint8_t rng[16];
        get(rng, 16);
        replicas_ = std::make_unique<Replicas>(hp, part != 0);
        std::uint32_t nb = 0;
        get(&nb, 4);
        if (nb > SBR_PARAM_EWMA_ALPHA_M + 1) throw std::runtime_error("load: implausible block count in " + path);
        std::uint32_t seen = 0;
        for (std::uint32_t i = 0; i < nb; ++i) {
            std::int32_t which = 0;
            std::uint64_t count = 0, expect = 0;
            get(&which, 4); get(&count, 8);
            // the engine says how many elements block `which` of THIS model has: a corrupt count never sizes an allocation
            if (which < 0 || which > SBR_PARAM_EWMA_ALPHA_M || (seen >> which & 1u) ||
                sbr_model_param_count(replicas_->primary(), which, &expect) != SBR_OK || expect == 0 || count != expect)
                throw std::runtime_error("load: parameter block " + std::to_string(which) + " does not fit the model in " + path);
            seen |= 1u << which;
            std::vector<float> v(count);
            get(v.data(), count * sizeof(float));
            const bool table = which == SBR_PARAM_ITEM_EMBEDDING || which == SBR_PARAM_ITEM_EMBEDDING_ACC || which == SBR_PARAM_ITEM_BIAS ||
                               which == SBR_PARAM_ITEM_BIAS_ACC || which == SBR_PARAM_ITEM_EMBEDDING_M || which == SBR_PARAM_ITEM_BIAS_M;
            for (std::size_t r = 0; r < replicas_->handles().size(); ++r) {
                if (part && table && r > 0) continue;  // a partitioned table exists once: written through replica 0
                check(sbr_model_set_param(replicas_->handles()[r], (sbr_param)which, v.data(), count), "sbr_model_set_param");
            }
        }
        for (std::int32_t which = 0; which <= SBR_PARAM_EWMA_ALPHA_M; ++which) {  // every non-empty block of the model must have been in the file
            std::uint64_t expect = 0;
            if (sbr_model_param_count(replicas_->primary(), which, &expect) == SBR_OK && expect != 0 && !(seen >> which & 1u))
                throw std::runtime_error("load: parameter block " + std::to_string(which) + " is missing from " + path);
        }
        for (sbr_model* h : replicas_->handles()) {
            check(sbr_model_set_counters(h, epoch, steps), "sbr_model_set_counters");
            check(sbr_model_set_rng(h, rng), "sbr_model_set_rng");
        }
    }

  private:
    std::unique_ptr<Replicas> replicas_;
};

/// Builder state common to lstm::Hyperparameters (lstm.rs:39-202) and ewma::Hyperparameters
/// (ewma.rs:45-206); defaults are those of `new` (lstm.rs:56-71, ewma.rs:61-75).
template <class Derived>
class HyperparametersBase {
  public:
    HyperparametersBase(std::size_t num_items, std::size_t max_sequence_length)
        : num_items_(num_items), max_sequence_length_(max_sequence_length), rng_(XorShiftRng::from_entropy()) {}

    /// Set the learning rate.
    Derived& learning_rate(float v) { learning_rate_ = v; return self(); }
    /// Set the L2 penalty.
    Derived& l2_penalty(float v) { l2_penalty_ = v; return self(); }
    /// Set the embedding dimensionality (the engine supports 16, 32, 64, 128, 256).
    Derived& embedding_dim(std::size_t v) { item_embedding_dim_ = v; return self(); }
    /// Set the number of epochs to run per each `fit` call.
    Derived& num_epochs(std::size_t v) { num_epochs_ = v; return self(); }
    /// Set the loss function.
    Derived& loss(Loss v) { loss_ = v; return self(); }
    /// Number of parallel workers = device replicas (≙ rayon threads, lstm.rs:110-113).  The
    /// reference default is one per core; here the default is one replica.
    Derived& num_threads(std::size_t v) { num_threads_ = v; return self(); }
    /// Set the type of parallelism.
    Derived& parallelism(Parallelism v) { parallelism_ = v; return self(); }
    /// Set the random number generator (moved in, as in the reference).
    Derived& rng(XorShiftRng v) { rng_ = v; return self(); }
    /// Set the random number generator from seed.
    Derived& from_seed(const std::array<std::uint8_t, 16>& seed) { rng_ = XorShiftRng::from_seed(seed); return self(); }
    /// Set the optimizer type.
    Derived& optimizer(Optimizer v) { optimizer_ = v; return self(); }
    /// Subsequences per optimiser step and device (engine extension; 1 = the reference's
    /// per-sequence SGD).
    Derived& batch_sequences(std::size_t v) { batch_sequences_ = v; return self(); }
    /// With num_threads(n) > 1: store the item table once, row range r on replica r's device, instead
    /// of n full copies (engine extension for catalogues in the 1e7 range; results are identical).
    Derived& partition_item_table(bool v) { partition_item_table_ = v; return self(); }

  protected:
    Derived& self() { return static_cast<Derived&>(*this); }

    sbr_hparams hparams(sbr_model_kind kind) const {
        sbr_hparams hp{};
        hp.num_items = (std::uint32_t)num_items_;
        hp.max_sequence_length = (std::uint32_t)max_sequence_length_;
        hp.embedding_dim = (std::uint32_t)item_embedding_dim_;
        hp.learning_rate = learning_rate_;
        hp.l2_penalty = l2_penalty_;
        hp.model = kind;
        hp.loss = (std::int32_t)loss_;
        hp.optimizer = (std::int32_t)optimizer_;
        hp.parallelism = (std::int32_t)parallelism_;
        const auto seed = rng_.state_seed();
        std::copy(seed.begin(), seed.end(), hp.seed);
        hp.num_epochs = (std::uint32_t)num_epochs_;
        hp.num_devices = (std::uint32_t)num_threads_;
        hp.device_rank = 0;
        hp.batch_sequences = (std::uint32_t)batch_sequences_;
        return hp;
    }

    /// The parts of `random` the two models share (lstm.rs:141-172, ewma.rs:141-165): same ranges
    /// as the reference; the draws come from this engine's RNG.
    void randomize_common(XorShiftRng& rng) {
        auto uniform = [&](double lo, double hi) { return lo + (hi - lo) * rng.unit(); };
        max_sequence_length_ = (std::size_t)1 << (4 + rng.below(4));
        item_embedding_dim_ = (std::size_t)1 << (4 + rng.below(4));
        learning_rate_ = std::pow(10.0f, (float)uniform(-3.0, 0.5));
        l2_penalty_ = std::pow(10.0f, (float)uniform(-7.0, -3.0));
        loss_ = uniform(0.0, 1.0) < 0.5 ? Loss::BPR : Loss::Hinge;
        optimizer_ = uniform(0.0, 1.0) < 0.5 ? Optimizer::Adam : Optimizer::Adagrad;
    }

    std::size_t num_items_;
    std::size_t max_sequence_length_;
    std::size_t item_embedding_dim_ = 16;
    float learning_rate_ = 0.01f;
    float l2_penalty_ = 0.0f;
    Loss loss_ = Loss::BPR;
    Optimizer optimizer_ = Optimizer::Adam;
    Parallelism parallelism_ = Parallelism::Synchronous;
    XorShiftRng rng_;
    std::size_t num_threads_ = 1;
    std::size_t num_epochs_ = 10;
    std::size_t batch_sequences_ = 32;
    bool partition_item_table_ = false;
};

} // namespace detail

// ---- sbr::models::lstm (lstm.rs) ---------------------------------------------------------------
namespace lstm {

/// Type of LSTM layer (lstm.rs:28-35).
enum class LSTMVariant { Normal, Coupled };

/// An LSTM-based sequence model for implicit feedback (lstm.rs:386-416).
class ImplicitLSTMModel : public detail::ImplicitSequenceModel {
    using detail::ImplicitSequenceModel::ImplicitSequenceModel;

  public:
    /// A model written by `save` (≙ deserialising the serde-derived ImplicitLSTMModel, lstm.rs:386).
    static ImplicitLSTMModel load(const std::string& path) { return ImplicitLSTMModel(path, 0); }
};

/// Hyperparameters for the ImplicitLSTMModel (lstm.rs:39-202).
class Hyperparameters : public detail::HyperparametersBase<Hyperparameters> {
  public:
    /// Build new hyperparameters.
    static Hyperparameters new_(std::size_t num_items, std::size_t max_sequence_length) {
        return Hyperparameters(num_items, max_sequence_length);
    }
    Hyperparameters(std::size_t num_items, std::size_t max_sequence_length)
        : detail::HyperparametersBase<Hyperparameters>(num_items, max_sequence_length) {}
    /// Set the LSTM variant.
    Hyperparameters& lstm_variant(LSTMVariant v) { lstm_type_ = v; return *this; }
    /// Generate a random point of the search space (lstm.rs:141-172).
    static Hyperparameters random(std::size_t num_items, XorShiftRng& rng) {
        Hyperparameters h(num_items, 16);
        h.randomize_common(rng);
        auto uniform = [&]() { return rng.unit(); };
        h.lstm_type_ = uniform() < 0.5 ? LSTMVariant::Normal : LSTMVariant::Coupled;
        h.parallelism_ = uniform() < 0.5 ? Parallelism::Asynchronous : Parallelism::Synchronous;
        h.num_epochs_ = (std::size_t)1 << (3 + rng.below(4));
        return h;
    }
    /// Build a model out of the chosen hyperparameters: parameters are initialised on the device
    /// from the builder's RNG (lstm.rs:174-201).
    ImplicitLSTMModel build() const {
        return ImplicitLSTMModel(hparams(lstm_type_ == LSTMVariant::Normal ? SBR_MODEL_LSTM_NORMAL : SBR_MODEL_LSTM_COUPLED),
                                 partition_item_table_);
    }

  private:
    LSTMVariant lstm_type_ = LSTMVariant::Coupled;
};

} // namespace lstm

// ---- sbr::models::ewma (ewma.rs) ---------------------------------------------------------------
namespace ewma {

/// Implicit EWMA model (ewma.rs:401-429).  State recurrence as coded at ewma.rs:302-313.
class ImplicitEWMAModel : public detail::ImplicitSequenceModel {
    using detail::ImplicitSequenceModel::ImplicitSequenceModel;

  public:
    /// A model written by `save` (≙ deserialising the serde-derived ImplicitEWMAModel, ewma.rs:401).
    static ImplicitEWMAModel load(const std::string& path) { return ImplicitEWMAModel(path, 1); }
};

/// Hyperparameters describing the EWMA model (ewma.rs:45-206).
class Hyperparameters : public detail::HyperparametersBase<Hyperparameters> {
  public:
    static Hyperparameters new_(std::size_t num_items, std::size_t max_sequence_length) {
        return Hyperparameters(num_items, max_sequence_length);
    }
    Hyperparameters(std::size_t num_items, std::size_t max_sequence_length)
        : detail::HyperparametersBase<Hyperparameters>(num_items, max_sequence_length) {}
    static Hyperparameters random(std::size_t num_items, XorShiftRng& rng) {
        Hyperparameters h(num_items, 16);
        h.randomize_common(rng);
        h.parallelism_ = rng.unit() < 0.5 ? Parallelism::Asynchronous : Parallelism::Synchronous;
        h.num_epochs_ = (std::size_t)1 << (3 + rng.below(4));
        return h;
    }
    /// Build the implicit EWMA model (ewma.rs:201-205).
    ImplicitEWMAModel build() const { return ImplicitEWMAModel(hparams(SBR_MODEL_EWMA), partition_item_table_); }
};

} // namespace ewma
using Sessions = detail::Sessions;
using ItemSet = detail::ItemSet;
} // namespace models
using Sessions = models::Sessions;
using ItemSet = models::ItemSet;

// =============================================================================================
// sbr::evaluation  (src/evaluation.rs)
// =============================================================================================
namespace evaluation {

/// MRR of the last item of every test sequence, the items before it being the inputs
/// (evaluation.rs:12-48), through the model's OnlineRankingModel interface — the reference's loop:
/// one user_representation + one full-catalogue predict per user, history masked to f32::MIN,
/// rank = #{score >= score[test item]}.
template <class Model>
Result<float, PredictionError> mrr_score_generic(const Model& model, const data::CompressedInteractions& test) {
    std::vector<ItemId> item_ids(test.num_items());
    std::iota(item_ids.begin(), item_ids.end(), (ItemId)0);
    float sum = 0.0f;
    std::size_t count = 0;
    for (const auto& user : test.iter_users()) {
        if (user.len() < 2) continue;
        const std::vector<ItemId> train_items(user.item_ids, user.item_ids + user.len() - 1);
        const ItemId test_item = user.item_ids[user.len() - 1];
        auto representation = model.user_representation(train_items);
        if (representation.is_err()) return Result<float, PredictionError>::Err(representation.unwrap_err());
        auto scored = model.predict(representation.unwrap(), item_ids);
        if (scored.is_err()) return Result<float, PredictionError>::Err(scored.unwrap_err());
        std::vector<float>& predictions = scored.unwrap();
        for (ItemId seen : train_items) predictions[seen] = std::numeric_limits<float>::lowest();
        const float test_score = predictions[test_item];
        std::size_t rank = 0;
        for (float p : predictions) rank += p >= test_score;
        sum += 1.0f / (float)rank;
        count += 1;
    }
    return Result<float, PredictionError>::Ok(sum / (float)count);
}

/// mrr_score for the engine's models: the whole evaluation in one device call (sbr_mrr_score:
/// batched user representations, MFMA score GEMM with the rank count in its epilogue).  Integer
/// ranks are identical to mrr_score_generic's.
inline Result<float, PredictionError> mrr_score(const models::detail::ImplicitSequenceModel& model,
                                                const data::CompressedInteractions& test,
                                                std::vector<std::uint32_t>* out_ranks = nullptr) {
    float mrr = 0.0f;
    std::uint64_t ranked = 0;
    std::vector<std::uint32_t> ranks(test.num_users());
    const sbr_status st = sbr_mrr_score(model.handle(), test.user_pointers().data(), test.item_ids().data(),
                                        (std::uint64_t)test.num_users(), &mrr, ranks.data(), &ranked);
    if (st == SBR_ERR_INVALID_PREDICTION) return Result<float, PredictionError>::Err(PredictionError::InvalidPredictionValue);
    models::detail::check(st, "sbr_mrr_score");
    if (out_ranks) {
        ranks.resize(ranked);
        *out_ranks = std::move(ranks);
    }
    return Result<float, PredictionError>::Ok(mrr);
}

/// Ranking metrics at several k over a hold-out of one or more items per user (no counterpart in the reference crate).
/// The means are over the ranked users (NaN without one, as mrr_score's 0 / 0); `per_user_*` hold one value per ranked user,
/// the at-k ones row-major [num_users_ranked][ks.size()].
struct RankingMetrics {
    std::vector<std::size_t> ks;
    std::size_t targets_skipped = 0;  ///< ranking_metrics under a policy with Ineligible::Skip: the targets left out of every mean
    std::size_t num_users_ranked = 0;
    std::vector<std::size_t> users;  ///< the ranked users' indices
    std::vector<double> precision, recall, hit_rate, ndcg;  ///< one mean per k
    double mrr = 0.0, mean_rank = 0.0;
    std::vector<double> per_user_precision, per_user_recall, per_user_hit_rate, per_user_ndcg, per_user_mrr, per_user_mean_rank;
};

/// precision / recall / hit rate / NDCG at every k, MRR (1 / best rank) and mean rank from the catalogue ranks of each user's
/// DISTINCT relevant items, user u's being ranks[ranks_ptr[u] .. ranks_ptr[u + 1]) (r of them):
///   hits_k = #{t : rank_t <= k}, precision = hits_k / k, recall = hits_k / r, hit_rate = hits_k > 0,
///   ndcg = sum_{rank_t <= k} 1 / log2(1 + rank_t)  /  sum_{j = 1..min(r, k)} 1 / log2(1 + j).
/// Users without ranks are left out.  Host only, float64.
inline RankingMetrics ranking_metrics_from_ranks(const std::vector<std::uint64_t>& ranks_ptr, const std::vector<std::uint32_t>& ranks,
                                                 const std::vector<std::size_t>& ks) {
    RankingMetrics out;
    out.ks = ks;
    const std::size_t nk = ks.size();
    std::size_t kmax = 0;
    for (std::size_t k : ks) {
        if (k < 1) throw std::invalid_argument("ranking_metrics: every k must be >= 1");
        kmax = std::max(kmax, k);
    }
    std::vector<double> ideal(kmax + 1, 0.0);
    for (std::size_t j = 1; j <= kmax; ++j) ideal[j] = ideal[j - 1] + 1.0 / std::log2(1.0 + (double)j);
    for (std::size_t u = 0; u + 1 < ranks_ptr.size(); ++u) {
        std::vector<std::uint32_t> r(ranks.begin() + (std::ptrdiff_t)ranks_ptr[u], ranks.begin() + (std::ptrdiff_t)ranks_ptr[u + 1]);
        if (r.empty()) continue;
        std::sort(r.begin(), r.end());
        out.users.push_back(u);
        out.per_user_mrr.push_back(1.0 / (double)r[0]);
        double sum = 0.0;
        for (std::uint32_t x : r) sum += (double)x;
        out.per_user_mean_rank.push_back(sum / (double)r.size());
        for (std::size_t k : ks) {
            const std::size_t hits = (std::size_t)(std::upper_bound(r.begin(), r.end(), (std::uint32_t)std::min<std::size_t>(k, 0xFFFFFFFFu)) - r.begin());
            double dcg = 0.0;
            for (std::size_t j = 0; j < hits; ++j) dcg += 1.0 / std::log2(1.0 + (double)r[j]);
            out.per_user_precision.push_back((double)hits / (double)k);
            out.per_user_recall.push_back((double)hits / (double)r.size());
            out.per_user_hit_rate.push_back(hits ? 1.0 : 0.0);
            out.per_user_ndcg.push_back(dcg / ideal[std::min(r.size(), k)]);
        }
    }
    const std::size_t n = out.num_users_ranked = out.users.size();
    auto mean_at = [&](const std::vector<double>& v, std::size_t j, std::size_t stride) {
        double s = 0.0;
        for (std::size_t i = 0; i < n; ++i) s += v[i * stride + j];
        return s / (double)n;
    };
    for (std::size_t j = 0; j < nk; ++j) {
        out.precision.push_back(mean_at(out.per_user_precision, j, nk));
        out.recall.push_back(mean_at(out.per_user_recall, j, nk));
        out.hit_rate.push_back(mean_at(out.per_user_hit_rate, j, nk));
        out.ndcg.push_back(mean_at(out.per_user_ndcg, j, nk));
    }
    out.mrr = mean_at(out.per_user_mrr, 0, 1);
    out.mean_rank = mean_at(out.per_user_mean_rank, 0, 1);
    return out;
}

/// precision@k, recall@k, hit-rate@k, NDCG@k at every k of `ks`, MRR and mean rank over a hold-out: the last `holdout` items of
/// each test sequence are the targets (de-duplicated, first occurrence kept), the rest the history; users with fewer than
/// holdout + 1 items are skipped (the reference's >= 2 at holdout = 1).  The exact ranks come from one device scan
/// (ImplicitSequenceModel::rank_targets), whose cost does not depend on k; `out_ranks` (optional) receives them, one per
/// distinct target in user order.  `users` of the result index the test set's users.
/// What a target the serving policy can never show — in its own history, forbidden by the masks, outside the set — counts as: Miss
/// keeps it at rank num_items (the reference's rule for a target in its own history), Skip leaves it out of every mean.
enum class Ineligible { Miss, Skip };
/// The serving policy the ranks are taken under: tag masks (one per user of the TEST SET, or one for all; needs set_item_tags) and an
/// item set of the model; both empty: the plain evaluation.
struct RankingPolicy {
    models::TagFilter filter;
    const models::ItemSet* item_set = nullptr;
    Ineligible ineligible = Ineligible::Miss;
};
inline Result<RankingMetrics, PredictionError> ranking_metrics(const models::detail::ImplicitSequenceModel& model,
                                                               const data::CompressedInteractions& test, const RankingPolicy& policy,
                                                               const std::vector<std::size_t>& ks = {10, 100}, std::size_t holdout = 1,
                                                               std::vector<std::uint32_t>* out_ranks = nullptr);
inline Result<RankingMetrics, PredictionError> ranking_metrics(const models::detail::ImplicitSequenceModel& model,
                                                               const data::CompressedInteractions& test,
                                                               const std::vector<std::size_t>& ks = {10, 100}, std::size_t holdout = 1,
                                                               std::vector<std::uint32_t>* out_ranks = nullptr) {
    return ranking_metrics(model, test, RankingPolicy{}, ks, holdout, out_ranks);
}
/// The same under a serving policy (ELIGIBLE RANKS in sbr_hip.h); `out_ranks` receives every rank, skipped targets included.
inline Result<RankingMetrics, PredictionError> ranking_metrics(const models::detail::ImplicitSequenceModel& model,
                                                               const data::CompressedInteractions& test, const RankingPolicy& policy,
                                                               const std::vector<std::size_t>& ks, std::size_t holdout,
                                                               std::vector<std::uint32_t>* out_ranks) {
    if (holdout < 1) throw std::invalid_argument("ranking_metrics: holdout must be >= 1");
    std::vector<std::size_t> users;
    std::vector<std::uint64_t> hist_ptr{0}, target_ptr{0}, timestamps;
    std::vector<std::uint32_t> hist_items, target_items;
    const std::vector<std::uint64_t>& ptr = test.user_pointers();
    for (std::size_t u = 0; u < test.num_users(); ++u) {
        const std::uint64_t b = ptr[u], e = ptr[u + 1];
        if (e - b < holdout + 1) continue;
        users.push_back(u);
        hist_items.insert(hist_items.end(), test.item_ids().begin() + (std::ptrdiff_t)b, test.item_ids().begin() + (std::ptrdiff_t)(e - holdout));
        hist_ptr.push_back(hist_items.size());
        for (std::uint64_t x = e - holdout; x < e; ++x) {
            const std::uint32_t t = test.item_ids()[x];
            if (std::find(target_items.begin() + (std::ptrdiff_t)target_ptr.back(), target_items.end(), t) == target_items.end())
                target_items.push_back(t);
        }
        target_ptr.push_back(target_items.size());
    }
    timestamps.assign(hist_items.size(), 0);
    const data::CompressedInteractions histories(users.size(), test.num_items(), hist_ptr, hist_items, timestamps);
    auto per_user = [&](const std::vector<std::uint32_t>& mask) {  // a per-user mask of the test set follows the users the split kept
        if (mask.size() <= 1) return mask;
        if (mask.size() != test.num_users()) throw std::invalid_argument("ranking_metrics: one mask per user of the test set");
        std::vector<std::uint32_t> kept;
        for (std::size_t u : users) kept.push_back(mask[u]);
        return kept;
    };
    const models::TagFilter filter{per_user(policy.filter.any_of), per_user(policy.filter.none_of)};
    const bool filtered = !filter.any_of.empty() || !filter.none_of.empty();
    auto ranks = policy.item_set ? policy.item_set->rank_targets(policy.item_set->of(histories, true, filter), target_ptr, target_items)
                                 : model.rank_targets(histories, target_ptr, target_items, filter);
    if (ranks.is_err()) return Result<RankingMetrics, PredictionError>::Err(ranks.unwrap_err());
    std::vector<std::uint64_t> kept_ptr = target_ptr;
    std::vector<std::uint32_t> kept_ranks = ranks.unwrap();
    std::size_t skipped = 0;
    if (policy.ineligible == Ineligible::Skip) {  // the host statement of "the policy can show it": in the set, allowed, not in the history
        const std::vector<std::uint32_t> tags = filtered ? model.item_tags() : std::vector<std::uint32_t>();
        const std::vector<std::uint32_t> members = policy.item_set ? policy.item_set->items() : std::vector<std::uint32_t>();
        kept_ptr.assign(1, 0);
        kept_ranks.clear();
        for (std::size_t i = 0; i < users.size(); ++i) {
            const std::uint32_t any = filter.any_of.empty() ? 0u : filter.any_of[filter.any_of.size() == 1 ? 0 : i];
            const std::uint32_t none = filter.none_of.empty() ? 0u : filter.none_of[filter.none_of.size() == 1 ? 0 : i];
            for (std::uint64_t e = target_ptr[i]; e < target_ptr[i + 1]; ++e) {
                const std::uint32_t t = target_items[e];
                bool ok = !policy.item_set || std::binary_search(members.begin(), members.end(), t);
                if (ok && filtered) ok = (tags[t] & none) == 0 && (any == 0 || (tags[t] & any) != 0);
                if (ok) ok = std::find(hist_items.begin() + (std::ptrdiff_t)hist_ptr[i], hist_items.begin() + (std::ptrdiff_t)hist_ptr[i + 1], t) ==
                             hist_items.begin() + (std::ptrdiff_t)hist_ptr[i + 1];
                if (ok) kept_ranks.push_back(ranks.unwrap()[e]);
                else ++skipped;
            }
            kept_ptr.push_back(kept_ranks.size());
        }
    }
    RankingMetrics out = ranking_metrics_from_ranks(kept_ptr, kept_ranks, ks);
    out.targets_skipped = skipped;
    for (std::size_t& u : out.users) u = users[u];
    if (out_ranks) *out_ranks = ranks.unwrap();
    return Result<RankingMetrics, PredictionError>::Ok(std::move(out));
}

/// One set of next-item metrics over some positions (each has ONE relevant item, of rank r): the means of 1 / r, r, [r <= k] and
/// (r <= k ? 1 / log2(1 + r) : 0), the last two one per k.  NaN where `count` is 0.
struct PositionMetrics {
    std::size_t count = 0;
    double mrr = 0.0, mean_rank = 0.0;
    std::vector<double> hit_rate, ndcg;
};

/// The result of sequence_metrics: `micro` over all positions, `macro` the mean of the per-user means (users without positions
/// left out; its count is the number of such users), and `by_history_length`[p] over the positions whose history has p items,
/// p = 1 .. max_sequence_length (entry 0 unused) — the j-th entry of a row counts as history length j + 1, which holds for a full
/// call (last = 0) on sequences of at most max_sequence_length + 1 items.
struct SequenceMetrics {
    std::vector<std::size_t> ks;
    std::size_t num_positions = 0;
    PositionMetrics micro, macro;
    std::vector<PositionMetrics> by_history_length;
};

/// sequence_metrics from the ranks (ImplicitSequenceModel::sequence_ranks).  Host only, float64.
inline SequenceMetrics sequence_metrics_from_ranks(const models::SequenceRanks& r, const std::vector<std::size_t>& ks,
                                                   std::size_t max_sequence_length) {
    for (std::size_t k : ks)
        if (k < 1) throw std::invalid_argument("sequence_metrics: every k must be >= 1");
    const std::size_t nk = ks.size();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    struct Sums {
        std::size_t n = 0;
        double rr = 0.0, rank = 0.0;
        std::vector<double> hit, dcg;
    };
    auto fresh = [&] { Sums s; s.hit.assign(nk, 0.0); s.dcg.assign(nk, 0.0); return s; };
    auto add = [&](Sums& s, std::uint32_t rank) {
        const double x = (double)rank;
        s.n += 1; s.rr += 1.0 / x; s.rank += x;
        for (std::size_t j = 0; j < nk; ++j)
            if (x <= (double)ks[j]) { s.hit[j] += 1.0; s.dcg[j] += 1.0 / std::log2(1.0 + x); }
    };
    auto means = [&](const Sums& s) {
        PositionMetrics m;
        m.count = s.n;
        const double n = (double)s.n;
        m.mrr = s.n ? s.rr / n : nan;
        m.mean_rank = s.n ? s.rank / n : nan;
        for (std::size_t j = 0; j < nk; ++j) {
            m.hit_rate.push_back(s.n ? s.hit[j] / n : nan);
            m.ndcg.push_back(s.n ? s.dcg[j] / n : nan);
        }
        return m;
    };
    SequenceMetrics out;
    out.ks = ks;
    Sums all = fresh();
    std::vector<Sums> by(max_sequence_length + 1, fresh());
    std::size_t users = 0;
    double mrr = 0.0, mean_rank = 0.0;
    std::vector<double> hit(nk, 0.0), ndcg(nk, 0.0);
    for (std::size_t u = 0; u < r.num_users(); ++u) {
        if (r.ptr[u + 1] == r.ptr[u]) continue;
        if (r.ptr[u + 1] - r.ptr[u] > max_sequence_length) throw std::invalid_argument("sequence_metrics: a row has more positions than max_sequence_length");
        Sums mine = fresh();
        for (std::uint64_t e = r.ptr[u]; e < r.ptr[u + 1]; ++e) {
            if (r.ranks[e] < 1) throw std::invalid_argument("sequence_metrics: ranks start at 1");
            add(all, r.ranks[e]);
            add(mine, r.ranks[e]);
            add(by[(std::size_t)(e - r.ptr[u]) + 1], r.ranks[e]);
        }
        const PositionMetrics m = means(mine);
        users += 1; mrr += m.mrr; mean_rank += m.mean_rank;
        for (std::size_t j = 0; j < nk; ++j) { hit[j] += m.hit_rate[j]; ndcg[j] += m.ndcg[j]; }
    }
    out.num_positions = all.n;
    out.micro = means(all);
    out.macro.count = users;
    out.macro.mrr = users ? mrr / (double)users : nan;
    out.macro.mean_rank = users ? mean_rank / (double)users : nan;
    for (std::size_t j = 0; j < nk; ++j) {
        out.macro.hit_rate.push_back(users ? hit[j] / (double)users : nan);
        out.macro.ndcg.push_back(users ? ndcg[j] / (double)users : nan);
    }
    for (const Sums& s : by) out.by_history_length.push_back(means(s));
    return out;
}

/// MRR, mean rank, hit-rate@k and NDCG@k of next-item prediction at EVERY position of every test sequence — how good the model is
/// after 1, 5 or 50 events — from one forward pass per sequence and one scan row per position
/// (ImplicitSequenceModel::sequence_ranks).  `last` (0 = all) keeps each window's last positions only (by_history_length is then
/// indexed from the first kept position); `out_ranks` (optional) receives the ranks.
inline Result<SequenceMetrics, PredictionError> sequence_metrics(const models::detail::ImplicitSequenceModel& model,
                                                                 const data::CompressedInteractions& test,
                                                                 const std::vector<std::size_t>& ks = {10, 100}, bool mask_history = true,
                                                                 std::size_t last = 0, models::SequenceRanks* out_ranks = nullptr) {
    auto ranks = model.sequence_ranks(test, mask_history, last);
    if (ranks.is_err()) return Result<SequenceMetrics, PredictionError>::Err(ranks.unwrap_err());
    SequenceMetrics out = sequence_metrics_from_ranks(ranks.unwrap(), ks, (std::size_t)model.hparams().max_sequence_length);
    if (out_ranks) *out_ranks = ranks.unwrap();
    return Result<SequenceMetrics, PredictionError>::Ok(std::move(out));
}

/// The per-position log-probabilities of sequence_log_probs, CSR: user u's are log_probs[ptr[u] .. ptr[u + 1]), positions ascending;
/// -inf where the policy masks the target.
struct SequenceLogProbs {
    std::vector<std::uint64_t> ptr;
    std::vector<double> log_probs;
    std::size_t num_users() const { return ptr.empty() ? 0 : ptr.size() - 1; }
};

/// The exact log-probability of the item that came next at every position of every test sequence under softmax(score / temperature)
/// over the items the user may see (ImplicitSequenceModel::sequence_partition; `last` 0 = all positions).
inline Result<SequenceLogProbs, PredictionError> sequence_log_probs(const models::detail::ImplicitSequenceModel& model,
                                                                    const data::CompressedInteractions& test, float temperature = 1.0f,
                                                                    bool mask_history = true, std::size_t last = 0) {
    auto part = model.sequence_partition(test, temperature, mask_history, last);
    if (part.is_err()) return Result<SequenceLogProbs, PredictionError>::Err(part.unwrap_err());
    SequenceLogProbs out;
    out.log_probs = part.unwrap().log_probs();
    out.ptr = part.unwrap().ptr;
    return Result<SequenceLogProbs, PredictionError>::Ok(std::move(out));
}

/// The result of sequence_log_likelihood.  Positions with log-probability -inf (the masked ones) are left out of every mean and
/// counted in `masked_positions`; `mean_log_prob` / `perplexity` = exp(-mean) over the `positions` counted, `macro_*` the mean of
/// the per-user means over `macro_users` users; NaN where nothing is counted.
struct SequenceLogLikelihood {
    std::size_t positions = 0, masked_positions = 0, macro_users = 0;
    double mean_log_prob = 0.0, perplexity = 0.0, macro_mean_log_prob = 0.0, macro_perplexity = 0.0;
};

/// sequence_log_likelihood from the log-probabilities.  Host only, float64.
inline SequenceLogLikelihood sequence_log_likelihood_from_log_probs(const SequenceLogProbs& lp) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    SequenceLogLikelihood out;
    double sum = 0.0, user_means = 0.0;
    for (std::size_t u = 0; u < lp.num_users(); ++u) {
        double mine = 0.0;
        std::size_t n = 0;
        for (std::uint64_t e = lp.ptr[u]; e < lp.ptr[u + 1]; ++e) {
            if (std::isinf(lp.log_probs[e])) { out.masked_positions += 1; continue; }
            mine += lp.log_probs[e];
            n += 1;
        }
        if (!n) continue;
        sum += mine;
        out.positions += n;
        user_means += mine / (double)n;
        out.macro_users += 1;
    }
    out.mean_log_prob = out.positions ? sum / (double)out.positions : nan;
    out.perplexity = std::exp(-out.mean_log_prob);
    out.macro_mean_log_prob = out.macro_users ? user_means / (double)out.macro_users : nan;
    out.macro_perplexity = std::exp(-out.macro_mean_log_prob);
    return out;
}

/// Mean log-likelihood and perplexity of next-item prediction under softmax(score / temperature) at every position of every test
/// sequence; `out_log_probs` (optional) receives the log-probabilities.
inline Result<SequenceLogLikelihood, PredictionError> sequence_log_likelihood(const models::detail::ImplicitSequenceModel& model,
                                                                              const data::CompressedInteractions& test, float temperature = 1.0f,
                                                                              bool mask_history = true, std::size_t last = 0,
                                                                              SequenceLogProbs* out_log_probs = nullptr) {
    auto lp = sequence_log_probs(model, test, temperature, mask_history, last);
    if (lp.is_err()) return Result<SequenceLogLikelihood, PredictionError>::Err(lp.unwrap_err());
    SequenceLogLikelihood out = sequence_log_likelihood_from_log_probs(lp.unwrap());
    if (out_log_probs) *out_log_probs = lp.unwrap();
    return Result<SequenceLogLikelihood, PredictionError>::Ok(std::move(out));
}

} // namespace evaluation

// =============================================================================================
// sbr::datasets  (src/datasets.rs) — the part that needs no network
// =============================================================================================
namespace datasets {

/// Reads the MovieLens CSV the reference downloads (datasets.rs:57-60: header
/// `user_id,item_id,rating,timestamp`, deserialised into Interaction{user_id,item_id,timestamp}).
inline data::Interactions read_csv(const std::string& path) {
    std::ifstream f(path);
    if (!f) throw std::runtime_error(path + ": cannot open");
    std::string line;
    if (!std::getline(f, line)) throw std::runtime_error(path + ": empty file");
    std::vector<std::string> header;
    {
        std::stringstream ss(line);
        std::string cell;
        while (std::getline(ss, cell, ',')) {
            while (!cell.empty() && (cell.back() == '\r' || cell.back() == ' ')) cell.pop_back();
            header.push_back(cell);
        }
    }
    auto column = [&](const char* name) {
        const auto it = std::find(header.begin(), header.end(), name);
        if (it == header.end()) throw std::runtime_error(path + ": no column " + name);
        return (std::size_t)(it - header.begin());
    };
    const std::size_t cu = column("user_id"), ci = column("item_id"), ct = column("timestamp");
    std::vector<data::Interaction> rows;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::vector<std::string> cells;
        std::stringstream ss(line);
        std::string cell;
        while (std::getline(ss, cell, ',')) cells.push_back(cell);
        if (cells.size() <= std::max(cu, std::max(ci, ct))) throw std::runtime_error(path + ": short row");
        rows.emplace_back((UserId)std::stoull(cells[cu]), (ItemId)std::stoull(cells[ci]), (Timestamp)std::stoull(cells[ct]));
    }
    return data::Interactions::from(std::move(rows));
}

/// Same name as the reference entry point (datasets.rs:66-71); reads a local copy (argument, or
/// $SBR_MOVIELENS_PATH) instead of downloading — there is no egress on the GPU hosts.
inline data::Interactions download_movielens_100k(const std::string& path = "") {
    std::string p = path;
    if (p.empty())
        if (const char* env = std::getenv("SBR_MOVIELENS_PATH")) p = env;
    if (p.empty()) throw std::runtime_error("download_movielens_100k: no network here; set SBR_MOVIELENS_PATH to data.csv");
    return read_csv(p);
}

} // namespace datasets
} // namespace sbr

#endif // SBR_HPP
