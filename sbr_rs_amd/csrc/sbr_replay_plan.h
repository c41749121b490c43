// sbr_replay_plan.h — the host's planning of sbr_sessions_replay (sbr_engine.hip) and the ring arithmetic it shares with the feed
// kernels (sbr_sessions.hip).  Nothing here needs a device or a HIP header: the file compiles with any C++17 compiler, which is how
// its bounds are checked under the host sanitizers.
//
// A replay recomputes slots' states from their seen-item memories.  The plan orders the slots by remembered items descending (so
// that step t of the recurrence covers a prefix, as an append call's sessions are ordered), cuts that order into chunks of at most
// `chunk_cap` sessions, and gives each chunk the offsets of the feed array the step kernels read (SessionAppend, sbr_kernels.h).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define SBR_REPLAY_HD __host__ __device__
#else
#define SBR_REPLAY_HD
#endif

namespace sbr {

/* entries of a ring of w that are valid after cnt items were remembered */
SBR_REPLAY_HD inline uint32_t seen_valid(unsigned long long cnt, uint32_t w) { return cnt < w ? (uint32_t)cnt : w; }

/* ring position of the t-th oldest valid entry, t < seen_valid(cnt, w): the q-th remembered item lies at q % w, and the oldest
 * one still held is q = cnt - seen_valid(cnt, w) */
SBR_REPLAY_HD inline uint32_t seen_ring_base(unsigned long long cnt, uint32_t w) { return cnt < w ? 0u : (uint32_t)(cnt % w); }
SBR_REPLAY_HD inline uint32_t seen_ring_pos(unsigned long long cnt, uint32_t w, uint32_t t) {
    const uint32_t p = seen_ring_base(cnt, w) + t; /* cnt < w ? t : (cnt + t) % w, with one 64-bit division per slot: p < 2 w */
    return p >= w ? p - w : p;
}

struct ReplayChunk {
    size_t first = 0, n = 0;  /* sessions [first, first + n) of the plan's order */
    int tm = 0;               /* steps of the chunk: the count of its first session */
    uint64_t total = 0;       /* items of the chunk = off[tm] */
    std::vector<int> off;     /* [tm + 1] time-major feed: the item of (step t, session b) at off[t] + b, b < off[t + 1] - off[t] */
    std::vector<unsigned long long> start; /* [n] session-major feed: session b's items at [start[b], start[b] + count) */
};

struct ReplayPlan {
    std::vector<uint32_t> slot, count; /* the slots with a non-empty memory, count = seen_valid descending, equal counts in input order */
    std::vector<uint32_t> empty;       /* the slots whose memory is empty: they become empty slots */
    std::vector<ReplayChunk> chunks;
};

/* slots [n] (null: slot i = i), each named once, cnt[i] = the remembered-item count of slots[i]; 1 <= w <= 1024, chunk_cap >= 1
 * with chunk_cap * w < 2^31 (a chunk's feed is addressed with an int). */
inline void plan_replay(const uint32_t* slots, const unsigned long long* cnt, size_t n, uint32_t w, size_t chunk_cap, ReplayPlan* out) {
    ReplayPlan& p = *out;
    p = ReplayPlan();
    /* counting sort by count descending: below[c] = sessions with a count above c */
    std::vector<size_t> at((size_t)w + 2, 0);
    for (size_t i = 0; i < n; ++i) ++at[seen_valid(cnt[i], w)];
    const size_t live = n - at[0];
    size_t run = 0;
    for (uint32_t c = w; c >= 1; --c) { /* at[c] becomes the first position of count c */
        const size_t have = at[c];
        at[c] = run;
        run += have;
    }
    p.slot.resize(live);
    p.count.resize(live);
    p.empty.reserve(n - live);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t c = seen_valid(cnt[i], w);
        const uint32_t s = slots ? slots[i] : (uint32_t)i;
        if (c == 0) { p.empty.push_back(s); continue; }
        const size_t q = at[c]++;
        p.slot[q] = s;
        p.count[q] = c;
    }
    for (size_t first = 0; first < live; first += chunk_cap) {
        ReplayChunk ch;
        ch.first = first;
        ch.n = live - first < chunk_cap ? live - first : chunk_cap;
        ch.tm = (int)p.count[first];
        /* sessions alive at step t = those with a count above t: from the chunk's count histogram, largest count first */
        std::vector<size_t> hist((size_t)ch.tm + 1, 0);
        ch.start.resize(ch.n);
        for (size_t b = 0; b < ch.n; ++b) {
            ch.start[b] = ch.total;
            ch.total += p.count[first + b];
            ++hist[p.count[first + b]];
        }
        std::vector<size_t> alive((size_t)ch.tm, 0);
        size_t above = 0;
        for (int t = ch.tm - 1; t >= 0; --t) {
            above += hist[(size_t)t + 1];
            alive[(size_t)t] = above;
        }
        ch.off.assign((size_t)ch.tm + 1, 0);
        for (int t = 0; t < ch.tm; ++t) ch.off[(size_t)t + 1] = ch.off[(size_t)t] + (int)alive[(size_t)t];
        p.chunks.push_back(std::move(ch));
    }
}

}  // namespace sbr
