// sbr_sessions.hip — gfx950 kernels of the session store (sbr_sessions_*, include/sbr_hip.h): device-resident recurrent states,
// one row per slot, advanced by appended items and read in place by the catalogue scans (sbr_catalogue.hip).
//
// A store is H [capacity + 1][D] (h of the LSTM, s of EWMA), C [capacity + 1][D] (LSTM cell states) and len [capacity + 1]; row
// `capacity` is the empty-history row: the state after one step of item 0 from zero (lstm.rs:262-264), which the scans read for a
// slot with len == 0.  The arithmetic of a step is the forward pass's (sbr_kernels.hip: lstm_fwd_step_kernel,
// ewma_forward_kernel), operation for operation, so a slot's state has the bits of sbr_user_representation of the items appended
// to it, however they were split across calls.
//
//   session_lstm_step_kernel : one LSTM cell step of the sessions that still have an item at step t of a call
//   session_commit_kernel    : the call's final h, c into the store's rows and len += items appended (the ONLY writer of the store
//                              on the LSTM append path)
//   session_ewma_step_kernel : all of a call's items of a session, in place
//   session_reset_kernel / session_set_state_kernel / session_get_state_kernel : zero / scatter / gather of slots' rows and len
//
// A store with seen-item memory (SeenView: w > 0) also has ring [capacity][w] and cnt [capacity]; nothing above reads or writes them:
//   session_seen_append_kernel : an append call's ring writes and cnt += items appended, behind the kernels above
//   session_seen_lists_kernel  : per scan chunk, the exclusion CSR the catalogue scan binary-searches (sbr_catalogue.hip)
//   audience_seen_match_kernel : the audience scan's inverted lists: (query, candidate position) keys of the candidates whose memory holds
//                                a query item, counted in one pass and written in a second; audience_seen_csr_kernel turns the sorted
//                                keys into the CSR over queries the scan binary-searches
//   session_seen_clear_kernel / session_seen_get_kernel / session_seen_set_kernel : cnt = 0 / the ring oldest first / restore
//   session_replay_feed_steps_kernel / session_replay_feed_rows_kernel : a replay chunk's items out of the rings, in the order the
//                                step kernels above read an append call's (LSTM time-major through an LDS transpose / EWMA session-major)
//   session_seen_count_kernel  : cnt of named slots, for the host's replay plan
//
// A rollout (sbr_sessions_rollout) reads a store and writes scratch only:
//   rollout_begin_kernel / rollout_segments_kernel : a chunk's scratch state and its exclusion CSR with one entry of slack per step
//   rollout_advance_kernel     : per step, the scan's pick into the outputs, the row's exclusion segment and the next step's feed
//   rollout_carry_kernel       : an ended row's state kept across the LSTM step
//
// A beam search (sbr_sessions_beam_search) reads a store and writes scratch only; per step, behind the k = W scan and its partition:
//   beam_select_kernel         : one workgroup per row: the W best of the live beams' offers, in the three-key order
//   beam_segments_kernel       : each child beam's exclusion segment, its parent's with the pick merged in, into the other parity
//   beam_gather_rows_kernel    : EWMA: the parents' rows copied into the other parity, ahead of the in-place cell step
//   beam_backtrack_kernel      : at the chunk's end, the parent pointers walked back into the [n][W][steps] outputs
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see sbr_rs_amd/build.py).

#include "sbr_kernels.h"

#include "../../include/sbr_hip.h"
#include "sbr_device.h"
#include "sbr_numerics.h"
#include "sbr_replay_plan.h"

namespace sbr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// LSTM step of a session store.  FORM: the STEP form — grid = (32-session tiles of step t) x (16-unit tiles), one wave per gate,
// one launch per step of the call — writing the new h, c into SCRATCH rows, never into the rows it reads; session_commit_kernel,
// next on the stream, copies each session's final state into the store.  Why: a workgroup of unit tile ut reads ALL of a row's h
// while the workgroups of the other unit tiles write their units of the same row, so writing h in place would race; the
// sequence-resident form (one workgroup per session tile for all units and steps) avoids that too but needs a workgroup of D / 16
// waves with every gate's accumulators live, which does not exist at D = 256 (the forward pass itself takes per-step launches
// there), and a call appends one item far more often than many.  The sequence-resident form is not built here: this kernel is the
// only one that steps a store's LSTM state.
//
// Arithmetic = lstm_fwd_step_kernel: wave g computes z_g = [E[item] ; h] Wp_g + b_g for 32 sessions x 16 units on
// v_mfma_f32_16x16x4_f32 (accumulator seeded with the bias, k ascending, the x half then the h half), the gate pre-activations
// meet in LDS and sbr_lstm_cell_fwd is applied by all threads.  No G, no X: nothing here trains.
//
// Rows: session b of the step (b < bt; the host orders a call's sessions by item count descending, so step t covers a prefix)
// reads h, c from Hin / Cin row (in_row ? in_row[b] : b) — the store's rows through the slot index at the call's first step, the
// scratch rows of the step before afterwards — as zeros where len is given and len[row] == 0 (an empty slot starts from
// h = c = 0), and writes row b of Hout / Cout.
// ------------------------------------------------------------------------------------------------
template <int D, int NG>
__global__ __launch_bounds__(NG * 64) void session_lstm_step_kernel(ModelView m, const uint32_t* __restrict__ items, int bt,
                                                                    const uint32_t* __restrict__ in_row,
                                                                    const unsigned long long* __restrict__ len,
                                                                    const float* __restrict__ Hin, const float* __restrict__ Cin,
                                                                    float* __restrict__ Hout, float* __restrict__ Cout) {
    constexpr int LDA = D + 2;
    constexpr int NSH = D / 16;       // weight k-blocks (16 k each) per half
    constexpr int RT = 2;             // 16-row tiles per workgroup
    constexpr int ROWS = 16 * RT;
    constexpr int NT = NG * 64;
    constexpr int LDZ = NG * 16 + 1;
    constexpr int PF = NSH < 8 ? NSH : 8;
    constexpr int LDS_FLOATS = ROWS * (LDA > LDZ ? LDA : LDZ);  // A halves and the gate exchange share one buffer
    __shared__ float As[LDS_FLOATS];
    __shared__ int src_row[ROWS];     // row of Hin / Cin of the tile's sessions; -1: zero state (or past the tile's end)
    float* Zs = As;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int g = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j16 = lane & 15;
    const int kq = lane >> 4;
    const int ut = blockIdx.y;
    const int b0 = blockIdx.x * ROWS;
    const int nrows = bt - b0 < ROWS ? bt - b0 : ROWS;
    if (tid < ROWS) {
        int r = -1;
        if (tid < nrows) {
            r = in_row ? (int)in_row[b0 + tid] : b0 + tid;
            if (len && len[r] == 0ull) r = -1;
        }
        src_row[tid] = r;
    }
    const float* wp = m.Wp + (((size_t)(ut * NG + g) * (2 * NSH)) * 64 + lane) * 4;
    float4 bf[PF];
#pragma unroll
    for (int S = 0; S < PF; ++S) bf[S] = ld4(wp + (size_t)S * 256);
    const float bias = m.bW[g * D + ut * 16 + j16];
    __syncthreads();
    // both halves of the A tile are requested up front
    constexpr int NV = ROWS * (D / 4);
    constexpr int ITER = (NV + NT - 1) / NT;
    float4 xv[ITER], hv[ITER];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int idx = tid + it * NT;
        const int i = idx / (D / 4);
        const int c4 = (idx % (D / 4)) * 4;
        xv[it] = make_float4(0.f, 0.f, 0.f, 0.f);
        hv[it] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (idx < NV && i < nrows) {
            xv[it] = ld4(m.E + (size_t)items[b0 + i] * D + c4);
            const int r = src_row[i];
            if (r >= 0) hv[it] = ld4(Hin + (size_t)r * D + c4);
        }
    }
    auto stage = [&](const float4* v) {
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int idx = tid + it * NT;
            if (idx < NV) {
                const int i = idx / (D / 4);
                const int c4 = (idx % (D / 4)) * 4;
                float2* dst = reinterpret_cast<float2*>(&As[i * LDA + c4]);
                dst[0] = make_float2(v[it].x, v[it].y);
                dst[1] = make_float2(v[it].z, v[it].w);
            }
        }
    };
    f32x4 acc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[rt] = (f32x4){bias, bias, bias, bias};
    auto mma_half = [&](int half) {
#pragma unroll
        for (int S0 = 0; S0 < NSH; S0 += PF) {
            float4 cur[PF];
#pragma unroll
            for (int S = 0; S < PF; ++S) cur[S] = bf[S];
            // request the next group of weight k-blocks (possibly of the other half)
            const int nextS = half * NSH + S0 + PF;
            if (nextS < 2 * NSH) {
#pragma unroll
                for (int S = 0; S < PF; ++S) bf[S] = ld4(wp + (size_t)(nextS + S) * 256);
            }
#pragma unroll
            for (int S = 0; S < PF; ++S) {
                float av[RT][4];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const float* arow = &As[(rt * 16 + j16) * LDA + 16 * (S0 + S) + kq];
                    av[rt][0] = arow[0]; av[rt][1] = arow[4]; av[rt][2] = arow[8]; av[rt][3] = arow[12];
                }
                // independent accumulators alternate so that no MFMA waits on its predecessor
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][0], cur[S].x, acc[rt], 0, 0, 0);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][1], cur[S].y, acc[rt], 0, 0, 0);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][2], cur[S].z, acc[rt], 0, 0, 0);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][3], cur[S].w, acc[rt], 0, 0, 0);
            }
        }
    };
    stage(xv);
    __syncthreads();
    mma_half(0);
    __syncthreads();
    stage(hv);
    __syncthreads();
    mma_half(1);
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) Zs[(rt * 16 + kq * 4 + reg) * LDZ + g * 16 + j16] = acc[rt][reg];
    __syncthreads();
    for (int e = tid; e < ROWS * 16; e += NT) {
        const int i = e >> 4;
        const int uu = e & 15;
        if (i < nrows) {
            const int u = ut * 16 + uu;
            const int r = src_row[i];
            const float cprev = r >= 0 ? Cin[(size_t)r * D + u] : 0.0f;
            const float* z = &Zs[i * LDZ + uu];
            float zi, zf, zg, zo;
            if (NG == 4) { zi = z[0]; zf = z[16]; zg = z[32]; zo = z[(NG - 1) * 16]; }
            else { zi = 0.0f; zf = z[0]; zg = z[16]; zo = z[32]; }
            float gi, gf, gg, go, cc, hh;
            sbr_lstm_cell_fwd(zi, zf, zg, zo, cprev, NG == 3, &gi, &gf, &gg, &go, &cc, &hh);
            Cout[(size_t)(b0 + i) * D + u] = cc;
            Hout[(size_t)(b0 + i) * D + u] = hh;
        }
    }
}

// The append's commit: session b (count[b] items this call, final state in the scratch rows of parity (count[b] - 1) & 1) ->
// the store's row slot[b]; len[slot[b]] += count[b] * advance (advance = 0: the empty-history row, which has no length).  Sessions
// with no items are left alone.  16 B per lane.
template <int D>
__global__ __launch_bounds__(256) void session_commit_kernel(const uint32_t* __restrict__ slot, const uint32_t* __restrict__ count, int n,
                                                             const float* __restrict__ Hs, const float* __restrict__ Cs, size_t parity_stride,
                                                             float* __restrict__ H, float* __restrict__ C, unsigned long long* __restrict__ len,
                                                             int advance) {
    constexpr int L = D / 4;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t b = idx / L;
    if (b >= (size_t)n) return;
    const uint32_t cnt = count[b];
    if (cnt == 0) return;
    const int c4 = (int)(idx % L) * 4;
    const size_t src = (size_t)((cnt - 1) & 1u) * parity_stride + b * D + c4;
    const size_t dst = (size_t)slot[b] * D + c4;
    st4(H + dst, ld4(Hs + src));
    st4(C + dst, ld4(Cs + src));
    if (c4 == 0 && advance) len[slot[b]] += cnt;
}

// ------------------------------------------------------------------------------------------------
// EWMA step of a session store: one D/4-lane group per session, 16 B per lane, walks the call's items of its session —
// ids[start[b] .. start[b] + count[b]) — from the slot's stored s and writes s and len back IN PLACE (each element depends only on
// itself and one lane group owns a row).  The first item ever appended to a slot (len == 0) sets s = E[x] (ewma.rs:306); every
// other one is ewma_forward_kernel's expression s = fma(a, s, (1 - a) * E[x]), a = sbr_sigmoidf(alpha).
// ------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void session_ewma_step_kernel(ModelView m, const uint32_t* __restrict__ slot,
                                                                const unsigned long long* __restrict__ start,
                                                                const uint32_t* __restrict__ count, int n, const uint32_t* __restrict__ ids,
                                                                float* __restrict__ S, unsigned long long* __restrict__ len, int advance) {
    constexpr int L = D / 4;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t b = idx / L;
    if (b >= (size_t)n) return;
    const int lg = (int)(idx % L);
    const uint32_t cnt = count[b];
    if (cnt == 0) return;
    float a[4], oma[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a[j] = sbr_sigmoidf(m.alpha[4 * lg + j]);
        oma[j] = 1.0f - a[j];
    }
    const uint32_t sl = slot[b];
    const unsigned long long have = len[sl];
    float* row = S + (size_t)sl * D + 4 * lg;
    float4 s = ld4(row);
    const uint32_t* it = ids + start[b];
    for (uint32_t t = 0; t < cnt; ++t) {
        const float4 x = ld4(m.E + (size_t)it[t] * D + 4 * lg);
        if (have == 0ull && t == 0) {
            s = x;
        } else {
            s.x = sbr_fma(a[0], s.x, oma[0] * x.x);
            s.y = sbr_fma(a[1], s.y, oma[1] * x.y);
            s.z = sbr_fma(a[2], s.z, oma[2] * x.z);
            s.w = sbr_fma(a[3], s.w, oma[3] * x.w);
        }
    }
    st4(row, s);
    if (lg == 0 && advance) len[sl] = have + cnt;
}

// rows slot[i] of H (and C) zeroed, len = 0
__global__ __launch_bounds__(256) void session_reset_kernel(const uint32_t* __restrict__ slot, int n, int d, float* __restrict__ H,
                                                            float* __restrict__ C, unsigned long long* __restrict__ len) {
    const int L = d / 4;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t i = idx / L;
    if (i >= (size_t)n) return;
    const int c4 = (int)(idx % L) * 4;
    const size_t at = (size_t)slot[i] * d + c4;
    st4(H + at, make_float4(0.f, 0.f, 0.f, 0.f));
    if (C) st4(C + at, make_float4(0.f, 0.f, 0.f, 0.f));
    if (c4 == 0) len[slot[i]] = 0ull;
}

// restore: row slot[i] of H (C) = h_in[i] (c_in[i]), embedding_dim floats each, the columns past it zero; len[slot[i]] = len_in[i].
// A restored length of 0 is the empty slot: its state is zero whatever h_in holds.
__global__ __launch_bounds__(256) void session_set_state_kernel(const uint32_t* __restrict__ slot, int n, int d, int dl,
                                                                const float* __restrict__ h_in, const float* __restrict__ c_in,
                                                                const unsigned long long* __restrict__ len_in, float* __restrict__ H,
                                                                float* __restrict__ C, unsigned long long* __restrict__ len) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t i = idx / d;
    if (i >= (size_t)n) return;
    const int c = (int)(idx % d);
    const bool live = c < dl && len_in[i] != 0ull;
    const size_t at = (size_t)slot[i] * d + c;
    H[at] = live ? h_in[i * dl + c] : 0.0f;
    if (C) C[at] = live ? c_in[i * dl + c] : 0.0f;
    if (c == 0) len[slot[i]] = len_in[i];
}

// checkpoint: h_out[i] (c_out[i]) = the first embedding_dim columns of row slot[i] of H (C), len_out[i] = len[slot[i]]; any output
// may be null
__global__ __launch_bounds__(256) void session_get_state_kernel(const uint32_t* __restrict__ slot, int n, int d, int dl,
                                                                const float* __restrict__ H, const float* __restrict__ C,
                                                                const unsigned long long* __restrict__ len, float* __restrict__ h_out,
                                                                float* __restrict__ c_out, unsigned long long* __restrict__ len_out) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t i = idx / dl;
    if (i >= (size_t)n) return;
    const int c = (int)(idx % dl);
    const size_t at = (size_t)slot[i] * d + c;
    if (h_out) h_out[i * dl + c] = H[at];
    if (c_out) c_out[i * dl + c] = C[at];
    if (c == 0 && len_out) len_out[i] = len[slot[i]];
}

// ------------------------------------------------------------------------------------------------
// Seen-item memory.  The q-th item remembered by a slot since its reset lies at ring[slot][q % w]; cnt[slot] counts them all, so
// the valid entries are [0, cnt) while cnt < w and the whole ring afterwards, the oldest at (cnt - min(cnt, w)) % w.
// ------------------------------------------------------------------------------------------------

// One wave per session of an append call: its last min(count, w) items into the ring — lane j the j-th of them, so a wave's
// stores are consecutive words of the slot's segment (split once where the ring wraps) and no two land on one entry — then
// cnt += count by lane 0.  Every lane has read cnt before lane 0 stores it (one instruction stream), and no other wave touches
// the slot: a call names a slot once.
__global__ __launch_bounds__(256) void session_seen_append_kernel(const uint32_t* __restrict__ slot, const unsigned long long* __restrict__ start,
                                                                  const uint32_t* __restrict__ count, const uint32_t* __restrict__ ids, int n,
                                                                  uint32_t w, uint32_t* __restrict__ ring, unsigned long long* cnt) {
    const int b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (b >= n) return;
    const uint32_t c = count[b];
    if (c == 0) return;
    const uint32_t sl = slot[b];
    const unsigned long long have = cnt[sl];
    const uint32_t keep = c < w ? c : w;
    const uint32_t* src = ids + start[b] + (c - keep);
    uint32_t* dst = ring + (size_t)sl * w;
    const uint32_t at = (uint32_t)((have + (unsigned long long)(c - keep)) % w);
    for (uint32_t j = lane; j < keep; j += 64u) {
        uint32_t p = at + j; /* < 2 w */
        if (p >= w) p -= w;
        dst[p] = src[j];
    }
    if (lane == 0) cnt[sl] = have + c;
}

__global__ __launch_bounds__(256) void session_seen_clear_kernel(const uint32_t* __restrict__ slot, int n, unsigned long long* __restrict__ cnt) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) cnt[slot[i]] = 0ull;
}

// out_n[i] = min(cnt, w) of slot[i]; out_items[i * w + j] = its j-th oldest remembered item: the ring unrolled
__global__ __launch_bounds__(256) void session_seen_get_kernel(const uint32_t* __restrict__ slot, int n, uint32_t w,
                                                               const uint32_t* __restrict__ ring, const unsigned long long* __restrict__ cnt,
                                                               uint32_t* __restrict__ out_n, uint32_t* __restrict__ out_items) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t i = idx / w;
    if (i >= (size_t)n) return;
    const uint32_t j = (uint32_t)(idx % w);
    const uint32_t sl = slot[i];
    const unsigned long long c = cnt[sl];
    const uint32_t nv = c < w ? (uint32_t)c : w;
    if (j == 0) out_n[i] = nv;
    if (j < nv) out_items[i * w + j] = ring[(size_t)sl * w + (size_t)((c - nv + j) % w)];
}

// slot[i]'s memory = the last min(len, w) of ids[ptr[i] - ptr[0] .. ptr[i + 1] - ptr[0]) at entries [0, that many), cnt = that many
__global__ __launch_bounds__(256) void session_seen_set_kernel(const uint32_t* __restrict__ slot, int n, uint32_t w,
                                                               const uint64_t* __restrict__ ptr, const uint32_t* __restrict__ ids,
                                                               uint32_t* __restrict__ ring, unsigned long long* __restrict__ cnt) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t i = idx / w;
    if (i >= (size_t)n) return;
    const uint32_t j = (uint32_t)(idx % w);
    const uint32_t sl = slot[i];
    const uint64_t len = ptr[i + 1] - ptr[i];
    const uint32_t keep = len < (uint64_t)w ? (uint32_t)len : w;
    if (j == 0) cnt[sl] = keep;
    if (j < keep) ring[(size_t)sl * w + j] = ids[ptr[i + 1] - ptr[0] - keep + j];
}

// out[i] = cnt[slot[i]]: what a replay of named slots reads of their memories on the host
__global__ __launch_bounds__(256) void session_seen_count_kernel(const uint32_t* __restrict__ slot, int n, const unsigned long long* __restrict__ cnt,
                                                                 unsigned long long* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) out[i] = cnt[slot[i]];
}

// ------------------------------------------------------------------------------------------------
// Replay: the feed of the step kernels straight from the rings (sbr_sessions_replay).  Session b of a replay chunk is slot slot[b]
// with count[b] = min(cnt, w) remembered items (the host's plan, sbr_replay_plan.h: count descending); its t-th oldest lies at ring
// position seen_ring_pos(cnt, w, t).  Neither kernel writes the ring or cnt.
//
// session_replay_feed_steps_kernel (LSTM): the time-major array session_lstm_step_kernel reads, items[off[t] + b] for b below
// off[t + 1] - off[t] = the sessions with more than t items.  A workgroup takes 64 sessions x 64 steps: each wave reads 64
// consecutive steps of one session — consecutive ring words but for the one place the ring wraps — into a row of an LDS tile, and
// after the barrier writes one step of 64 consecutive sessions, the tile read down a column (rows padded to 65 words: no bank
// shared).  Lanes walking a step across 64 rings instead would touch one 64-byte sector per word read, w words apart, as
// item_rnorm_kernel's rows would without its transpose.  Bounds: b < n, t < count[b] <= w on the read; on the write t < tm and
// b < off[t + 1] - off[t], so the index is below off[t + 1] <= off[tm] = the array's length.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void session_replay_feed_steps_kernel(const uint32_t* __restrict__ slot, const uint32_t* __restrict__ count, int n,
                                                                        int tm, const int* __restrict__ off, uint32_t w,
                                                                        const uint32_t* __restrict__ ring, const unsigned long long* __restrict__ cnt,
                                                                        uint32_t* __restrict__ items) {
    __shared__ uint32_t tile[64][65];
    const int b0 = (int)blockIdx.x * 64, t0 = (int)blockIdx.y * 64;
    if (count[b0] <= (uint32_t)t0) return; /* counts descend: no session of this tile reaches step t0 (the whole workgroup leaves) */
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    for (int r = wave; r < 64; r += 4) {
        const int b = b0 + r;
        if (b >= n) break;
        const uint32_t t = (uint32_t)(t0 + lane);
        if (t < count[b]) {
            const uint32_t sl = slot[b];
            uint32_t p = seen_ring_base(cnt[sl], w) + t;
            if (p >= w) p -= w;
            tile[r][lane] = ring[(size_t)sl * w + p];
        }
    }
    __syncthreads();
    for (int r = wave; r < 64; r += 4) {
        const int t = t0 + r;
        if (t >= tm) break;
        const int o = off[t], bt = off[t + 1] - o;
        const int b = b0 + lane;
        if (b < bt) items[o + b] = tile[lane][r]; /* b < bt: count[b] > t, so the tile entry was written above */
    }
}

// session_replay_feed_rows_kernel (EWMA): the session-major array session_ewma_step_kernel reads, session b's items at
// [start[b], start[b] + count[b]).  One wave per session; reads and writes are consecutive words.
__global__ __launch_bounds__(256) void session_replay_feed_rows_kernel(const uint32_t* __restrict__ slot, const unsigned long long* __restrict__ start,
                                                                       const uint32_t* __restrict__ count, int n, uint32_t w,
                                                                       const uint32_t* __restrict__ ring, const unsigned long long* __restrict__ cnt,
                                                                       uint32_t* __restrict__ items) {
    const int b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (b >= n) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t c = count[b], sl = slot[b];
    const uint32_t base = seen_ring_base(cnt[sl], w);
    uint32_t* dst = items + start[b];
    for (uint32_t t = lane; t < c; t += 64u) {
        uint32_t p = base + t;
        if (p >= w) p -= w;
        dst[t] = ring[(size_t)sl * w + p];
    }
}

// The exclusion CSR of a scan chunk.  A group of G threads per user (G = 64: four users per workgroup, for p <= 64; G = 256: one)
// brings the slot's valid ring entries into LDS, padded with 0xFFFFFFFF to p = the power of two >= w, sorts them ascending there
// (bitonic; every thread of the workgroup walks the same p, so the barriers are uniform) and merges them with the caller's list
// straight into the user's segment [eptr[i], eptr[i + 1]) of out, whose length is w + (the caller's entries): sorted entry r goes to
// r + (caller entries below it), caller entry q to q + (ring entries not above it) — a merge without collisions, equal ids the
// ring's first — and 0xFFFFFFFF fills the rest.  The caller's list of user i is caller[eptr[i] - i w ..), any length.
//
// What topk_gemm_kernel needs of a segment (sbr_catalogue.hip, the excl_ptr block of its merge): it takes the lower bound of a
// real id (< num_items) and tests that entry for equality, so the segment must be NON-DECREASING — nothing more.  Repeated ids
// (an item seen twice, or seen and also in the caller's list) leave the lower bound on the first of them, which is equal; the
// 0xFFFFFFFF tail is above every real id and so keeps the order, and is never equal to one.  Hence no de-duplication here.
template <int G>
__global__ __launch_bounds__(256) void session_seen_lists_kernel(const uint32_t* __restrict__ slot, int n, uint32_t w, uint32_t p,
                                                                 const uint32_t* __restrict__ ring, const unsigned long long* __restrict__ cnt,
                                                                 const uint64_t* __restrict__ eptr, const uint32_t* __restrict__ caller,
                                                                 uint32_t* __restrict__ out) {
    constexpr int UPB = 256 / G;                       // users per workgroup
    constexpr uint32_t PMAX = G == 64 ? 64u : 1024u;   // the largest p of this form
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    __shared__ uint32_t buf[UPB * PMAX];
    const uint32_t grp = threadIdx.x / G, g = threadIdx.x % G;
    const size_t i = (size_t)blockIdx.x * UPB + grp;
    const bool live = i < (size_t)n;
    uint32_t* b = buf + grp * PMAX;
    uint32_t nv = 0, sl = 0;
    uint64_t e0 = 0, e1 = 0;
    if (live) {
        sl = slot[i];
        const unsigned long long c = cnt[sl];
        nv = c < w ? (uint32_t)c : w;
        e0 = eptr[i];
        e1 = eptr[i + 1];
    }
    for (uint32_t j = g; j < p; j += G) b[j] = j < nv ? ring[(size_t)sl * w + j] : NONE;
    __syncthreads();
    for (uint32_t k = 2; k <= p; k <<= 1)
        for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
            for (uint32_t t = g; t < (p >> 1); t += G) {
                const uint32_t lo = 2 * t - (t & (jj - 1)), hi = lo + jj; /* the pair whose indices differ in bit jj */
                const bool asc = (lo & k) == 0;
                const uint32_t x = b[lo], y = b[hi];
                if ((x > y) == asc) { b[lo] = y; b[hi] = x; }
            }
            __syncthreads();
        }
    if (!live) return;
    const uint64_t nc = e1 - e0 - w;
    const uint32_t* cl = caller + (e0 - i * w); /* not read where nc == 0 (caller may be null then) */
    uint32_t* o = out + e0;
    for (uint32_t r = g; r < nv; r += G) {
        const uint32_t v = b[r];
        uint64_t lo = 0, hi = nc;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (cl[mid] < v) lo = mid + 1; else hi = mid;
        }
        o[r + lo] = v;
    }
    for (uint64_t q = g; q < nc; q += G) {
        const uint32_t v = cl[q];
        uint32_t lo = 0, hi = nv;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (b[mid] <= v) lo = mid + 1; else hi = mid;
        }
        o[q + lo] = v;
    }
    for (uint64_t j = nv + nc + g; j < w + nc; j += G) o[j] = NONE;
}

// ------------------------------------------------------------------------------------------------
// The audience scan's inverted seen lists: per QUERY item, the candidate positions whose slot remembers it.
//
// A workgroup holds the chunk's queries' items, sorted ascending with repeats, in LDS (at most 8 192: 32 KB) and walks candidate
// positions p = wave, wave + (waves of the grid), ...: lane j of a position's wave takes ring entries j, j + 64, ... of the
// min(cnt, w) valid ones, finds the first query of that item by binary search and — where there is one, and no EARLIER valid entry
// of the ring holds the same item (a repeat counts once: the walk over the entries before it runs only for the few that matched) —
// produces one key (query << 32 | p) per query of that item.  FILL = false counts the keys (one atomic per wave); FILL = true writes
// them through a cursor, in no particular order: launch_pair_sort orders them.  Bounds: a ring read is below min(cnt, w) <= w of
// a slot below capacity (the host validated the slots), a key is written only at an index below cap.
// ------------------------------------------------------------------------------------------------
template <bool FILL>
__global__ __launch_bounds__(256) void audience_seen_match_kernel(const uint32_t* __restrict__ cand_slot, uint32_t num_cand, uint32_t w,
                                                                  const uint32_t* __restrict__ ring, const unsigned long long* __restrict__ cnt,
                                                                  const uint32_t* __restrict__ qs_item, const uint32_t* __restrict__ qs_idx,
                                                                  uint32_t nq, uint64_t* __restrict__ keys, unsigned long long cap,
                                                                  unsigned long long* counter) {
    __shared__ uint32_t qs[8192];
    for (uint32_t i = threadIdx.x; i < nq; i += 256) qs[i] = qs_item[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave0 = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t nwaves = gridDim.x * 4u;
    unsigned long long mine = 0;
    for (uint32_t p = wave0; p < num_cand; p += nwaves) {
        const uint32_t sl = cand_slot[p];
        const unsigned long long c = cnt[sl];
        const uint32_t nv = c < w ? (uint32_t)c : w;
        const uint32_t* rg = ring + (size_t)sl * w;
        for (uint32_t j = lane; j < nv; j += 64u) {
            const uint32_t item = rg[j];
            uint32_t lo = 0, hi = nq;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (qs[mid] < item) lo = mid + 1; else hi = mid;
            }
            if (lo >= nq || qs[lo] != item) continue;
            bool repeat = false;
            for (uint32_t e = 0; e < j && !repeat; ++e) repeat = rg[e] == item;
            if (repeat) continue;
            for (uint32_t t = lo; t < nq && qs[t] == item; ++t) {
                if (FILL) {
                    const unsigned long long at = atomicAdd(counter, 1ull);
                    if (at < cap) keys[at] = ((uint64_t)qs_idx[t] << 32) | (uint64_t)p;
                } else {
                    ++mine;
                }
            }
        }
    }
    if (!FILL) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off, 64);
        if (lane == 0 && mine) atomicAdd(counter, mine);
    }
}

// eptr[j] = the number of sorted keys below (j << 32), j = 0 .. nq; excl[e] = the position half of key e
__global__ __launch_bounds__(256) void audience_seen_csr_kernel(const uint64_t* __restrict__ keys, uint32_t n, uint32_t nq,
                                                                uint64_t* __restrict__ eptr, uint32_t* __restrict__ excl) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < (size_t)n) excl[t] = (uint32_t)keys[t];
    if (t <= (size_t)nq) {
        const uint64_t bound = (uint64_t)t << 32;
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (keys[mid] < bound) lo = mid + 1; else hi = mid;
        }
        eptr[t] = lo;
    }
}

// ------------------------------------------------------------------------------------------------
// Rollout (sbr_sessions_rollout; the contract: ROLLOUT in include/sbr_hip.h): a chunk's sessions advanced by their own picks, step
// after step, on SCRATCH rows — none of these kernels is given a pointer into the store that it writes through.  Per step the
// unchanged k = 1 scan leaves row i's pick in stride-1 arrays, rollout_advance_kernel below turns it into column j of the outputs,
// the next scan's exclusion and the next cell step's item, and the step kernels above advance the scratch state.
// ------------------------------------------------------------------------------------------------

// The chunk's start: ended = 0 and lengths = steps for every row (a row that never ends keeps that), and for EWMA — whose step
// kernel works in place — the scratch rows S[i] = H[slot[i]] at the storage width with slen[i] = len[slot[i]].  S null (LSTM): the
// first cell step reads the store's rows itself, through the slot index, as an append's first step does.
__global__ __launch_bounds__(256) void rollout_begin_kernel(const uint32_t* __restrict__ slot, int n, int d, uint32_t steps,
                                                            const float* __restrict__ H, const unsigned long long* __restrict__ len,
                                                            float* __restrict__ S, unsigned long long* __restrict__ slen,
                                                            uint32_t* __restrict__ ended, uint32_t* __restrict__ lengths) {
    const int L = d / 4;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t i = idx / L;
    if (i >= (size_t)n) return;
    const int c4 = (int)(idx % L) * 4;
    if (S) st4(S + i * d + c4, ld4(H + (size_t)slot[i] * d + c4));
    if (c4 == 0) {
        if (S) slen[i] = len[slot[i]];
        ended[i] = 0u;
        lengths[i] = steps;
    }
}

// The chunk's exclusion CSR with slack: row i's tight segment src[src_ptr[i], src_ptr[i + 1]) — non-decreasing, a 0xFFFFFFFF tail
// allowed: the caller's sorted list, or session_seen_lists_kernel's merge — to out[src_ptr[i] + i * slack ..), followed by `slack`
// entries of 0xFFFFFFFF: the room rollout_advance_kernel's inserts take.  One wave per row; every entry of the output is written.
__global__ __launch_bounds__(256) void rollout_segments_kernel(const uint64_t* __restrict__ src_ptr, const uint32_t* __restrict__ src, int n,
                                                               uint32_t slack, uint32_t* __restrict__ out) {
    const int i = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (i >= n) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t s0 = src_ptr[i], have = src_ptr[i + 1] - s0;
    uint32_t* o = out + s0 + (uint64_t)i * slack;
    for (uint64_t q = lane; q < have + slack; q += 64u) o[q] = q < have ? src[s0 + q] : 0xFFFFFFFFu;
}

// One wave per row, step j of a rollout.  The row's merged pick (pick_items[i]; 0xFFFFFFFF: nothing was eligible) becomes
//   column j of the outputs: the pick with its plain score, and where asked for its key and the step's shift and mass — or, for a
//     row that has ended, (0xFFFFFFFF, -inf, -inf, -inf, 0);
//   the row's end: the first padding sets ended[i] and lengths[i] = j, once — an ended row stays ended whatever its scans return;
//   the next cell step's feed: feed[i] = the pick and count[i] = 1, or item 0 (any valid row of E) and count[i] = 0 for an ended row,
//     whose state the step leaves alone (EWMA) or rollout_carry_kernel restores (LSTM);
//   the next scan's exclusion, where ins_ptr is given: the pick inserted into the row's sorted segment [ins_ptr[i], ins_ptr[i + 1]).
//     The segment is non-decreasing with a 0xFFFFFFFF tail at least one entry long (rollout_segments_kernel's slack: one entry per
//     step), and does not hold the pick — the scan has just offered it — so its place is the number of entries below it, counted by
//     the wave; the tail from there moves up by one entry, 64 at a time from the top, each round's loads complete (its stores carry
//     the loaded values) before its stores and so before the next round's stores, which land below it; then lane 0 writes the pick.
//     O(segment) per row and step.
// Within an item set (ids non-null: its num_ids sorted catalogue ids, the scan ran over its sub-table) the segments hold positions of
// the set while the outputs and the feed are catalogue ids: a pick that arrives as a position (pick_is_id == 0: the plain scan's) leaves
// as ids[pick] and is inserted as itself; one that arrives as a catalogue id (the sampled launch maps its rows) leaves as itself and is
// inserted at its position, found by the wave's binary search over ids (every lane the same probes: one load per probe).  An ended
// row's stand-in feed is then ids[0], so no row outside the set is read.
// No atomics; rows are independent and a row is one wave's.
__global__ __launch_bounds__(256) void rollout_advance_kernel(int n, uint32_t steps, uint32_t j, const uint32_t* __restrict__ pick_items,
                                                              const float* __restrict__ pick_scores, const float* __restrict__ pick_keys,
                                                              const float* __restrict__ pick_shift,
                                                              const unsigned long long* __restrict__ pick_mass,
                                                              const uint32_t* __restrict__ ids, uint32_t num_ids, uint32_t pick_is_id,
                                                              const uint64_t* __restrict__ ins_ptr, uint32_t* excl, uint32_t* ended,
                                                              uint32_t* __restrict__ lengths, uint32_t* __restrict__ feed,
                                                              uint32_t* __restrict__ count, uint32_t* __restrict__ out_items,
                                                              float* __restrict__ out_scores, float* __restrict__ out_keys,
                                                              float* __restrict__ out_shift, unsigned long long* __restrict__ out_mass) {
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    const int i = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (i >= n) return;
    const uint32_t lane = threadIdx.x & 63u;
    const bool was = ended[i] != 0u;
    const uint32_t picked = was ? NONE : pick_items[i];
    const bool live = picked != NONE;
    uint32_t id = picked, v = picked; /* what leaves and feeds; what the segment takes */
    if (ids && live) {
        if (pick_is_id) {
            uint32_t lo = 0, hi = num_ids;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (ids[mid] < picked) lo = mid + 1; else hi = mid;
            }
            v = lo;
        } else {
            id = ids[picked];
        }
    }
    if (lane == 0) {
        const size_t o = (size_t)i * steps + j;
        out_items[o] = id;
        out_scores[o] = live ? pick_scores[i] : -INFINITY;
        if (out_keys) out_keys[o] = live ? pick_keys[i] : -INFINITY;
        if (out_shift) {
            out_shift[o] = live ? pick_shift[i] : -INFINITY;
            out_mass[o] = live ? pick_mass[i] : 0ull;
        }
        feed[i] = live ? id : ids ? ids[0] : 0u;
        count[i] = live ? 1u : 0u;
        if (!live && !was) {
            ended[i] = 1u;
            lengths[i] = j;
        }
    }
    if (!live || !ins_ptr) return;
    const uint64_t e0 = ins_ptr[i], len = ins_ptr[i + 1] - e0;
    uint32_t* seg = excl + e0;
    uint32_t below = 0;
    for (uint64_t q = lane; q < len; q += 64u) below += seg[q] < v ? 1u : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) below += __shfl_xor(below, off, 64);
    const uint64_t pos = below; /* < len: the segment's last entry is 0xFFFFFFFF, above every pick */
    for (uint64_t hi = len; hi > pos + 1;) {
        const uint64_t lo = hi - (pos + 1) > 64u ? hi - 64u : pos + 1;
        const uint64_t dst = lo + lane;
        uint32_t x = 0;
        if (dst < hi) x = seg[dst - 1];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (dst < hi) seg[dst] = x;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        hi = lo;
    }
    if (lane == 0) seg[pos] = v;
}

// Behind an LSTM cell step of a rollout: an ended row's state, which the step has just advanced by the feed's stand-in item, is put
// back — row b of Hout / Cout = the row the step read (session_lstm_step_kernel's in_row / len rule: zeros for an empty slot at the
// rollout's first step).  So the next scan reads finite data and the final state is the row's last real one.  16 B per lane.
__global__ __launch_bounds__(256) void rollout_carry_kernel(const uint32_t* __restrict__ ended, int n, int d, const uint32_t* __restrict__ in_row,
                                                            const unsigned long long* __restrict__ len, const float* __restrict__ Hin,
                                                            const float* __restrict__ Cin, float* __restrict__ Hout, float* __restrict__ Cout) {
    const int L = d / 4;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t b = idx / L;
    if (b >= (size_t)n || !ended[b]) return;
    const int c4 = (int)(idx % L) * 4;
    const size_t r = in_row ? (size_t)in_row[b] : b;
    const bool zero = len && len[r] == 0ull;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    st4(Hout + b * d + c4, zero ? z : ld4(Hin + r * d + c4));
    st4(Cout + b * d + c4, zero ? z : ld4(Cin + r * d + c4));
}

// ------------------------------------------------------------------------------------------------
// Beam search (sbr_sessions_beam_search; the contract: BEAM SEARCH in include/sbr_hip.h): W beams per row advanced step after step on
// SCRATCH rows — beam b of row i is scan row i * W + b — the store read only.  Per step the unchanged top-k scan at k = W leaves
// each parent's first W eligible items and the partition sum its (shift, mass); beam_select_kernel keeps the row's W best offers,
// beam_segments_kernel and the cell step (or beam_gather_rows_kernel + the in-place EWMA step) make the children's exclusion
// segments and states from their parents'.  Parities: the children of step j are written into parity j & 1; the scan of step j + 1
// reads them.  The per-step record [steps][n W] holds what beam_backtrack_kernel needs to write the paths at the end.
// ------------------------------------------------------------------------------------------------

// The chunk's start: no row has ended, lengths = steps (a row that never ends keeps that), beams = 0.
__global__ __launch_bounds__(256) void beam_begin_kernel(int n, uint32_t steps, uint32_t* __restrict__ row_ended, uint32_t* __restrict__ lengths,
                                                         uint32_t* __restrict__ beams) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    row_ended[i] = 0u;
    lengths[i] = steps;
    beams[i] = 0u;
}

// One workgroup per row, step j.  Parents: the slot itself at j == 0 (scan row i), else beams p < W of the row (scan rows i W + p)
// that are alive.  Parent p offers its scan row's entries q < nv[p] (the scan's non-padding prefix), each with
//   t = fl(score * inv_t), d = fl(t - shift[p]), lp = fl(d - L[p]), cum = fl(cum[p] + lp)   (cum[p] = 0 at j == 0)
// where L[p] = sbr_log32(x), x = f32(mass >> s) 2^(s - F) exactly, s = max(0, bit_length(mass) - 24): one log per parent.  The row
// keeps the W best offers ordered by (cum descending, p ascending, q ascending).  lp never increases along q (fl is monotone and L[p]
// is constant), so an offer's rank is q plus, for every other parent, the length of that parent's prefix of offers that beat it —
// counted until it reaches W.  Ranks are distinct, so child c = the offer of rank c; no atomics, no dependence on dispatch order.
// Children c >= K = min(W, offers) are DEAD: they mirror child 0 (its parent and its pick) so that their state and segment are
// finite copies of a live beam's, and alive = 0.  No offer at all: the row ends at j (lengths = j; beams keep the last count), and
// every beam row is carried: parent itself (the slot at j == 0), no pick, ended = 1.  Per child, into the step's record: parent,
// item, plain score, lp, cum and the PARENT's shift and mass; and for the next kernels in_row (the state row the cell step reads:
// slot[i] at j == 0, else i W + parent), src_row (the segment the child's is copied from: i at j == 0, else i W + parent), feed /
// count (the cell step's item; count 0 on ended rows), pick (merged into the segment; 0xFFFFFFFF: nothing).  A row's parents are
// read into LDS before any of its children is written, so alive / cum are updated in place.
// Within an item set (ids non-null: its sorted catalogue ids, the scan ran over its sub-table) the scan's items are positions of the
// set: pick stays the position (the segments are positions), feed and the record's item become ids[position], and the stand-in feed
// of a carried beam is ids[0], so no row outside the set is read.
__global__ __launch_bounds__(256) void beam_select_kernel(int n, uint32_t w, uint32_t j, const uint32_t* __restrict__ slot,
                                                          const uint32_t* __restrict__ ids,
                                                          const uint32_t* __restrict__ scan_items, const float* __restrict__ scan_scores,
                                                          const float* __restrict__ shift, const unsigned long long* __restrict__ mass,
                                                          float inv_t, uint32_t fbits, uint32_t* row_ended, uint32_t* __restrict__ lengths,
                                                          uint32_t* __restrict__ beams, uint32_t* alive, float* cum, uint32_t* __restrict__ ended,
                                                          uint32_t* __restrict__ in_row, uint32_t* __restrict__ src_row,
                                                          uint32_t* __restrict__ feed, uint32_t* __restrict__ count, uint32_t* __restrict__ pick,
                                                          uint32_t* __restrict__ rec_parent, uint32_t* __restrict__ rec_item,
                                                          float* __restrict__ rec_score, float* __restrict__ rec_lp, float* __restrict__ rec_cum,
                                                          float* __restrict__ rec_shift, unsigned long long* __restrict__ rec_mass) {
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    __shared__ uint32_t p_nv[32];
    __shared__ float p_L[32], p_cum[32];
    __shared__ float o_cum[32 * 32], o_lp[32 * 32];
    __shared__ int ch[32];
    __shared__ uint32_t total;
    const int i = (int)blockIdx.x;
    if (i >= n) return; /* the whole workgroup */
    const uint32_t tid = threadIdx.x;
    const uint32_t P = j == 0 ? 1u : w;
    const bool was = row_ended[i] != 0u;
    const size_t b0 = (size_t)i * w;
    for (uint32_t p = tid; p < P; p += 256u) {
        const size_t srow = j == 0 ? (size_t)i : b0 + p;
        const bool live = !was && (j == 0 || alive[b0 + p] != 0u);
        uint32_t nv = 0;
        if (live)
            while (nv < w && scan_items[srow * w + nv] != NONE) ++nv;
        float L = 0.0f;
        if (nv) { /* mass >= 2^F: the best offer's weight alone is 2^F */
            const unsigned long long ms = mass[srow];
            const int s = ms >> 24 ? 40 - __clzll((long long)ms) : 0; /* = max(0, bit_length(mass) - 24) */
            L = sbr_log32(ldexpf((float)(ms >> s), s - (int)fbits));
        }
        p_nv[p] = nv;
        p_L[p] = L;
        p_cum[p] = j == 0 || !live ? 0.0f : cum[b0 + p];
    }
    if (tid < w) ch[tid] = -1;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;
        for (uint32_t p = 0; p < P; ++p) t += p_nv[p];
        total = t;
    }
    for (uint32_t o = tid; o < P * w; o += 256u) {
        const uint32_t p = o / w, q = o % w;
        if (q >= p_nv[p]) continue;
        const size_t srow = j == 0 ? (size_t)i : b0 + p;
        const float t = __fmul_rn(scan_scores[srow * w + q], inv_t);
        const float d = __fsub_rn(t, shift[srow]);
        const float lp = __fsub_rn(d, p_L[p]);
        o_lp[o] = lp;
        o_cum[o] = __fadd_rn(p_cum[p], lp);
    }
    __syncthreads();
    for (uint32_t o = tid; o < P * w; o += 256u) {
        const uint32_t p = o / w, q = o % w;
        if (q >= p_nv[p]) continue;
        const float c = o_cum[o];
        uint32_t rank = q;
        for (uint32_t p2 = 0; p2 < P && rank < w; ++p2) {
            if (p2 == p) continue;
            for (uint32_t q2 = 0; q2 < p_nv[p2]; ++q2) {
                const float c2 = o_cum[p2 * w + q2];
                if (!(c2 > c || (c2 == c && p2 < p))) break;
                if (++rank >= w) break;
            }
        }
        if (rank < w) ch[rank] = (int)o;
    }
    __syncthreads();
    if (tid >= w) return;
    const uint32_t c = tid;
    const size_t b = b0 + c;
    if (was || total == 0u) { /* the row has ended (or ends now): every beam row carried, nothing recorded */
        if (!was && c == 0) {
            row_ended[i] = 1u;
            lengths[i] = j;
        }
        in_row[b] = j == 0 ? slot[i] : (uint32_t)b;
        src_row[b] = j == 0 ? (uint32_t)i : (uint32_t)b;
        feed[b] = ids ? ids[0] : 0u;
        count[b] = 0u;
        pick[b] = NONE;
        ended[b] = 1u;
        alive[b] = 0u;
        cum[b] = -INFINITY;
        return;
    }
    const uint32_t K = total < w ? total : w;
    const bool live = c < K;
    int o = ch[live ? c : 0];
    if (o < 0) o = ch[0] < 0 ? 0 : ch[0]; /* only where the scores are not numbers (the call fails): keep every index in range */
    const uint32_t p = (uint32_t)o / w, q = (uint32_t)o % w;
    const size_t srow = j == 0 ? (size_t)i : b0 + p;
    const uint32_t item = scan_items[srow * w + q];
    const uint32_t it = item == NONE ? 0u : item;
    const uint32_t id = ids ? ids[it] : it; /* a position of the set < its size: the scan offered it, or 0 */
    in_row[b] = j == 0 ? slot[i] : (uint32_t)(b0 + p);
    src_row[b] = j == 0 ? (uint32_t)i : (uint32_t)(b0 + p);
    feed[b] = id;
    count[b] = 1u;
    pick[b] = it;
    ended[b] = 0u;
    alive[b] = live ? 1u : 0u;
    cum[b] = live ? o_cum[o] : -INFINITY;
    const size_t r = (size_t)j * n * w + b;
    rec_parent[r] = live ? p : 0u;
    rec_item[r] = live ? id : NONE;
    rec_score[r] = live ? scan_scores[srow * w + q] : -INFINITY;
    rec_lp[r] = live ? o_lp[o] : -INFINITY;
    rec_cum[r] = live ? o_cum[o] : -INFINITY;
    if (rec_shift) {
        rec_shift[r] = live ? shift[srow] : -INFINITY;
        rec_mass[r] = live ? mass[srow] : 0ull;
    }
    if (c == 0) beams[i] = K;
}

// One wave per child beam c: its exclusion segment [dst_ptr[c], dst_ptr[c + 1]) of dst = the source segment s = src_row[c] of the
// other CSR — src_row null: s = c / w, the row's tight list — with pick[c] merged in (pick null or 0xFFFFFFFF: a plain copy), then
// 0xFFFFFFFF to the end.  The source is non-decreasing with a 0xFFFFFFFF tail allowed and does not hold the pick (the scan has just
// offered it), so the pick's place is the number of entries below it, counted by the wave; the merged sequence is written in one
// pass.  The destination has room: a child's segment has one entry of slack per step beyond its row's list.
__global__ __launch_bounds__(256) void beam_segments_kernel(int nc, uint32_t w, const uint64_t* __restrict__ src_ptr, const uint32_t* __restrict__ src,
                                                            const uint32_t* __restrict__ src_row, const uint32_t* __restrict__ pick,
                                                            const uint64_t* __restrict__ dst_ptr, uint32_t* __restrict__ dst) {
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    const int c = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (c >= nc) return;
    const uint32_t lane = threadIdx.x & 63u;
    const size_t s = src_row ? (size_t)src_row[c] : (size_t)c / w;
    const uint64_t s0 = src_ptr[s], have = src_ptr[s + 1] - s0;
    const uint64_t d0 = dst_ptr[c], room = dst_ptr[c + 1] - d0;
    const uint32_t v = pick ? pick[c] : NONE;
    uint64_t pos = have; /* the pick's place: past every entry when there is none to merge */
    if (v != NONE) {
        uint32_t below = 0;
        for (uint64_t q = lane; q < have; q += 64u) below += src[s0 + q] < v ? 1u : 0u;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) below += __shfl_xor(below, off, 64);
        pos = below;
    }
    const uint64_t merged = have + (v != NONE ? 1u : 0u);
    for (uint64_t q = lane; q < room; q += 64u) {
        uint32_t x = NONE;
        if (q < merged) x = q < pos ? src[s0 + q] : q == pos ? v : src[s0 + q - 1];
        dst[d0 + q] = x;
    }
}

// EWMA ahead of the in-place cell step: row b of Sout / lout = row in_row[b] of Sin / lin, 16 B per lane
__global__ __launch_bounds__(256) void beam_gather_rows_kernel(const uint32_t* __restrict__ in_row, int n, int d, const float* __restrict__ Sin,
                                                               const unsigned long long* __restrict__ lin, float* __restrict__ Sout,
                                                               unsigned long long* __restrict__ lout) {
    const int L = d / 4;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t b = idx / L;
    if (b >= (size_t)n) return;
    const int c4 = (int)(idx % L) * 4;
    const size_t r = in_row[b];
    st4(Sout + b * d + c4, ld4(Sin + r * d + c4));
    if (c4 == 0) lout[b] = lin[r];
}

// One wave per (row i, beam b) at the chunk's end: beam b < beams[i] of the row's last real step lengths[i] - 1 is walked back by
// the record's parent pointers, lane 0 writing entry j of out [n][w][steps] for j = lengths[i] - 1 .. 0; the other lanes write the
// padding (0xFFFFFFFF, -inf, -inf, -inf, 0) — every entry of a beam b >= beams[i] and every j >= lengths[i].  out_cum [n][w]: the
// beam's cum at the last real step, -inf for a missing beam.
__global__ __launch_bounds__(256) void beam_backtrack_kernel(int n, uint32_t w, uint32_t steps, const uint32_t* __restrict__ lengths,
                                                             const uint32_t* __restrict__ beams, const uint32_t* __restrict__ rec_parent,
                                                             const uint32_t* __restrict__ rec_item, const float* __restrict__ rec_score,
                                                             const float* __restrict__ rec_lp, const float* __restrict__ rec_cum,
                                                             const float* __restrict__ rec_shift, const unsigned long long* __restrict__ rec_mass,
                                                             uint32_t* __restrict__ out_items, float* __restrict__ out_scores,
                                                             float* __restrict__ out_lp, float* __restrict__ out_cum, float* __restrict__ out_shift,
                                                             unsigned long long* __restrict__ out_mass) {
    const size_t g = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= (size_t)n * w) return;
    const uint32_t lane = threadIdx.x & 63u;
    const size_t i = g / w;
    const uint32_t b = (uint32_t)(g % w);
    const uint32_t len = b < beams[i] ? lengths[i] : 0u;
    const size_t o = g * steps;
    for (uint32_t j = len + lane; j < steps; j += 64u) {
        out_items[o + j] = 0xFFFFFFFFu;
        out_scores[o + j] = -INFINITY;
        out_lp[o + j] = -INFINITY;
        if (out_shift) {
            out_shift[o + j] = -INFINITY;
            out_mass[o + j] = 0ull;
        }
    }
    if (lane != 0) return;
    const size_t nw = (size_t)n * w;
    out_cum[g] = len ? rec_cum[(size_t)(len - 1) * nw + g] : -INFINITY;
    uint32_t c = b;
    for (uint32_t j = len; j-- > 0;) {
        const size_t r = (size_t)j * nw + i * w + c;
        out_items[o + j] = rec_item[r];
        out_scores[o + j] = rec_score[r];
        out_lp[o + j] = rec_lp[r];
        if (out_shift) {
            out_shift[o + j] = rec_shift[r];
            out_mass[o + j] = rec_mass[r];
        }
        c = rec_parent[r];
        if (c >= w) c = 0; /* never, from beam_select_kernel: an index stays in range */
    }
}

namespace {

inline unsigned blocks_for(size_t threads) { return (unsigned)((threads + 255) / 256); }

template <int D>
void lstm_append_d(const ModelView& m, const SessionView& sv, const SessionAppend& a, hipStream_t s) {
    const size_t parity_stride = (size_t)a.n * D;
    for (int t = 0; t < a.tm; ++t) {
        const int bt = a.off_host[t + 1] - a.off_host[t];
        const uint32_t* items = a.items + a.off_host[t];
        const float* Hin = t == 0 ? sv.H : a.Hs + (size_t)((t - 1) & 1) * parity_stride;
        const float* Cin = t == 0 ? sv.C : a.Cs + (size_t)((t - 1) & 1) * parity_stride;
        float* Hout = a.Hs + (size_t)(t & 1) * parity_stride;
        float* Cout = a.Cs + (size_t)(t & 1) * parity_stride;
        const dim3 grid((unsigned)((bt + 31) / 32), D / 16);
        if (m.ng == 4)
            hipLaunchKernelGGL((session_lstm_step_kernel<D, 4>), grid, dim3(256), 0, s, m, items, bt, t == 0 ? a.slot : nullptr,
                               t == 0 ? sv.len : nullptr, Hin, Cin, Hout, Cout);
        else
            hipLaunchKernelGGL((session_lstm_step_kernel<D, 3>), grid, dim3(192), 0, s, m, items, bt, t == 0 ? a.slot : nullptr,
                               t == 0 ? sv.len : nullptr, Hin, Cin, Hout, Cout);
    }
    if (a.tm > 0)
        hipLaunchKernelGGL((session_commit_kernel<D>), dim3(blocks_for((size_t)a.n * (D / 4))), dim3(256), 0, s, a.slot, a.count, a.n, a.Hs,
                           a.Cs, parity_stride, sv.H, sv.C, sv.len, a.advance);
}

template <int D>
void ewma_append_d(const ModelView& m, const SessionView& sv, const SessionAppend& a, hipStream_t s) {
    if (a.tm > 0)
        hipLaunchKernelGGL((session_ewma_step_kernel<D>), dim3(blocks_for((size_t)a.n * (D / 4))), dim3(256), 0, s, m, a.slot, a.start, a.count,
                           a.n, a.items, sv.H, sv.len, a.advance);
}

}  // namespace

int launch_session_append(const ModelView& m, const SessionView& sv, const SessionAppend& a, hipStream_t s) {
#define SBR_SESSION_D(DD)                                  \
    case DD:                                               \
        if (m.ng) lstm_append_d<DD>(m, sv, a, s);          \
        else ewma_append_d<DD>(m, sv, a, s);               \
        break;
    switch (m.d) {
        SBR_SESSION_D(16)
        SBR_SESSION_D(32)
        SBR_SESSION_D(64)
        SBR_SESSION_D(128)
        SBR_SESSION_D(256)
        default: return -1; /* no such storage width: the caller fails the call */
    }
#undef SBR_SESSION_D
    return a.tm > 0 ? (m.ng ? a.tm + 1 : 1) : 0;
}

namespace {

/* step j of a rollout's LSTM chunk: every row one cell step by its feed item into the scratch rows of parity j & 1 — from the store's
 * rows through the slot index at j == 0, as an append's first step, from the other parity afterwards — then the ended rows' carry */
template <int D>
void rollout_lstm_step_d(const ModelView& m, const SessionView& sv, const RolloutRows& r, uint32_t j, hipStream_t s) {
    const size_t parity_stride = (size_t)r.n * D;
    const float* Hin = j == 0 ? sv.H : r.Hs + (size_t)((j - 1) & 1u) * parity_stride;
    const float* Cin = j == 0 ? sv.C : r.Cs + (size_t)((j - 1) & 1u) * parity_stride;
    float* Hout = r.Hs + (size_t)(j & 1u) * parity_stride;
    float* Cout = r.Cs + (size_t)(j & 1u) * parity_stride;
    const uint32_t* in_row = j == 0 ? r.slot : nullptr;
    const unsigned long long* len = j == 0 ? sv.len : nullptr;
    const dim3 grid((unsigned)((r.n + 31) / 32), D / 16);
    if (m.ng == 4)
        hipLaunchKernelGGL((session_lstm_step_kernel<D, 4>), grid, dim3(256), 0, s, m, r.feed, r.n, in_row, len, Hin, Cin, Hout, Cout);
    else
        hipLaunchKernelGGL((session_lstm_step_kernel<D, 3>), grid, dim3(192), 0, s, m, r.feed, r.n, in_row, len, Hin, Cin, Hout, Cout);
    hipLaunchKernelGGL(rollout_carry_kernel, dim3(blocks_for((size_t)r.n * (D / 4))), dim3(256), 0, s, r.ended, r.n, D, in_row, len, Hin, Cin, Hout,
                       Cout);
}

/* step j of a rollout's EWMA chunk, in place on the scratch rows: row i's feed item where count[i] == 1, nothing where it is 0 */
template <int D>
void rollout_ewma_step_d(const ModelView& m, const RolloutRows& r, hipStream_t s) {
    hipLaunchKernelGGL((session_ewma_step_kernel<D>), dim3(blocks_for((size_t)r.n * (D / 4))), dim3(256), 0, s, m, r.ident, r.start, r.count, r.n,
                       r.feed, r.Hs, r.len, 1);
}

}  // namespace

int launch_rollout_begin(const ModelView& m, const SessionView& sv, const RolloutRows& r, hipStream_t s) {
    if (r.n <= 0) return 0;
    hipLaunchKernelGGL(rollout_begin_kernel, dim3(blocks_for((size_t)r.n * (m.d / 4))), dim3(256), 0, s, r.slot, r.n, m.d, r.steps, sv.H, sv.len,
                       m.ng ? nullptr : r.Hs, r.len, r.ended, r.lengths);
    return 1;
}

int launch_rollout_segments(const uint64_t* src_ptr, const uint32_t* src, int n, uint32_t slack, uint32_t* out, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(rollout_segments_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, src_ptr, src, n, slack, out);
    return 1;
}

int launch_rollout_advance(const RolloutRows& r, uint32_t j, const RolloutPick& p, const uint64_t* ins_ptr, uint32_t* excl, const RolloutOut& o,
                           hipStream_t s) {
    if (r.n <= 0) return 0;
    hipLaunchKernelGGL(rollout_advance_kernel, dim3((unsigned)((r.n + 3) / 4)), dim3(256), 0, s, r.n, r.steps, j, p.items, p.scores, p.keys, p.shift,
                       p.mass, p.ids, p.num_ids, p.is_id ? 1u : 0u, ins_ptr, excl, r.ended, r.lengths, r.feed, r.count, o.items, o.scores, o.keys, o.shift, o.mass);
    return 1;
}

int launch_rollout_step(const ModelView& m, const SessionView& sv, const RolloutRows& r, uint32_t j, hipStream_t s) {
    if (r.n <= 0) return 0;
#define SBR_ROLLOUT_D(DD)                                          \
    case DD:                                                       \
        if (m.ng) rollout_lstm_step_d<DD>(m, sv, r, j, s);         \
        else rollout_ewma_step_d<DD>(m, r, s);                     \
        break;
    switch (m.d) {
        SBR_ROLLOUT_D(16)
        SBR_ROLLOUT_D(32)
        SBR_ROLLOUT_D(64)
        SBR_ROLLOUT_D(128)
        SBR_ROLLOUT_D(256)
        default: return -1; /* no such storage width: the caller fails the call */
    }
#undef SBR_ROLLOUT_D
    return m.ng ? 2 : 1;
}

namespace {

/* step j of a beam chunk: every beam row one cell step by its feed item into parity j & 1 from its parent's row in_row — the store's
 * rows through the slot at j == 0 — LSTM by the unchanged step kernel and the ended rows' carry, EWMA by the gather and the unchanged
 * in-place step */
template <int D>
void beam_step_d(const ModelView& m, const SessionView& sv, const BeamRows& r, uint32_t j, hipStream_t s) {
    const int nb = r.n * (int)r.w;
    const size_t parity_stride = (size_t)nb * D;
    const float* Hin = j == 0 ? sv.H : r.Hs + (size_t)((j - 1) & 1u) * parity_stride;
    float* Hout = r.Hs + (size_t)(j & 1u) * parity_stride;
    const unsigned long long* len = j == 0 ? sv.len : nullptr;
    if (m.ng) {
        const float* Cin = j == 0 ? sv.C : r.Cs + (size_t)((j - 1) & 1u) * parity_stride;
        float* Cout = r.Cs + (size_t)(j & 1u) * parity_stride;
        const dim3 grid((unsigned)((nb + 31) / 32), D / 16);
        if (m.ng == 4)
            hipLaunchKernelGGL((session_lstm_step_kernel<D, 4>), grid, dim3(256), 0, s, m, r.feed, nb, r.in_row, len, Hin, Cin, Hout, Cout);
        else
            hipLaunchKernelGGL((session_lstm_step_kernel<D, 3>), grid, dim3(192), 0, s, m, r.feed, nb, r.in_row, len, Hin, Cin, Hout, Cout);
        hipLaunchKernelGGL(rollout_carry_kernel, dim3(blocks_for((size_t)nb * (D / 4))), dim3(256), 0, s, r.ended, nb, D, r.in_row, len, Hin, Cin,
                           Hout, Cout);
        return;
    }
    const unsigned long long* lin = j == 0 ? sv.len : r.len + (size_t)((j - 1) & 1u) * nb;
    unsigned long long* lout = r.len + (size_t)(j & 1u) * nb;
    hipLaunchKernelGGL(beam_gather_rows_kernel, dim3(blocks_for((size_t)nb * (D / 4))), dim3(256), 0, s, r.in_row, nb, D, Hin, lin, Hout, lout);
    hipLaunchKernelGGL((session_ewma_step_kernel<D>), dim3(blocks_for((size_t)nb * (D / 4))), dim3(256), 0, s, m, r.ident, r.start, r.count, nb,
                       r.feed, Hout, lout, 1);
}

}  // namespace

int launch_beam_begin(const BeamRows& r, hipStream_t s) {
    if (r.n <= 0) return 0;
    hipLaunchKernelGGL(beam_begin_kernel, dim3(blocks_for((size_t)r.n)), dim3(256), 0, s, r.n, r.steps, r.row_ended, r.lengths, r.beams);
    return 1;
}

int launch_beam_select(const BeamRows& r, uint32_t j, const BeamScan& sc, const BeamRecord& rec, hipStream_t s) {
    if (r.n <= 0) return 0;
    hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)r.n), dim3(256), 0, s, r.n, r.w, j, r.slot, sc.ids, sc.items, sc.scores, sc.shift, sc.mass, sc.inv_t,
                       sc.fbits, r.row_ended, r.lengths, r.beams, r.alive, r.cum, r.ended, r.in_row, r.src_row, r.feed, r.count, r.pick,
                       rec.parent, rec.item, rec.score, rec.lp, rec.cum, rec.shift, rec.mass);
    return 1;
}

int launch_beam_segments(int nc, uint32_t w, const uint64_t* src_ptr, const uint32_t* src, const uint32_t* src_row, const uint32_t* pick,
                         const uint64_t* dst_ptr, uint32_t* dst, hipStream_t s) {
    if (nc <= 0) return 0;
    hipLaunchKernelGGL(beam_segments_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, s, nc, w, src_ptr, src, src_row, pick, dst_ptr, dst);
    return 1;
}

int launch_beam_step(const ModelView& m, const SessionView& sv, const BeamRows& r, uint32_t j, hipStream_t s) {
    if (r.n <= 0) return 0;
#define SBR_BEAM_D(DD)                         \
    case DD:                                   \
        beam_step_d<DD>(m, sv, r, j, s);       \
        break;
    switch (m.d) {
        SBR_BEAM_D(16)
        SBR_BEAM_D(32)
        SBR_BEAM_D(64)
        SBR_BEAM_D(128)
        SBR_BEAM_D(256)
        default: return -1; /* no such storage width: the caller fails the call */
    }
#undef SBR_BEAM_D
    return 2;
}

int launch_beam_backtrack(const BeamRows& r, const BeamRecord& rec, const BeamOut& o, hipStream_t s) {
    if (r.n <= 0) return 0;
    const size_t nb = (size_t)r.n * r.w;
    hipLaunchKernelGGL(beam_backtrack_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, s, r.n, r.w, r.steps, r.lengths, r.beams, rec.parent,
                       rec.item, rec.score, rec.lp, rec.cum, rec.shift, rec.mass, o.items, o.scores, o.lp, o.cum, o.shift, o.mass);
    return 1;
}

void launch_session_reset(const SessionView& sv, const uint32_t* slot, int n, int d, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(session_reset_kernel, dim3(blocks_for((size_t)n * (d / 4))), dim3(256), 0, s, slot, n, d, sv.H, sv.C, sv.len);
}

void launch_session_set_state(const SessionView& sv, const uint32_t* slot, int n, int d, int dl, const float* h_in, const float* c_in,
                              const unsigned long long* len_in, hipStream_t s) {
    if (n > 0)
        hipLaunchKernelGGL(session_set_state_kernel, dim3(blocks_for((size_t)n * d)), dim3(256), 0, s, slot, n, d, dl, h_in, c_in, len_in, sv.H,
                           sv.C, sv.len);
}

void launch_session_get_state(const SessionView& sv, const uint32_t* slot, int n, int d, int dl, float* h_out, float* c_out,
                              unsigned long long* len_out, hipStream_t s) {
    if (n > 0)
        hipLaunchKernelGGL(session_get_state_kernel, dim3(blocks_for((size_t)n * dl)), dim3(256), 0, s, slot, n, d, dl, sv.H, sv.C, sv.len, h_out,
                           c_out, len_out);
}

void launch_session_seen_append(const SeenView& sn, const uint32_t* slot, const unsigned long long* start, const uint32_t* count,
                                const uint32_t* ids, int n, hipStream_t s) {
    if (n > 0 && sn.w)
        hipLaunchKernelGGL(session_seen_append_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, slot, start, count, ids, n, sn.w, sn.ring, sn.cnt);
}

void launch_session_seen_clear(const SeenView& sn, const uint32_t* slot, int n, hipStream_t s) {
    if (n > 0 && sn.w) hipLaunchKernelGGL(session_seen_clear_kernel, dim3(blocks_for((size_t)n)), dim3(256), 0, s, slot, n, sn.cnt);
}

int launch_session_seen_lists(const SeenView& sn, const uint32_t* slot, int n, const uint64_t* eptr, const uint32_t* caller, uint32_t* out,
                              hipStream_t s) {
    if (n <= 0 || !sn.w) return 0;
    uint32_t p = 1;
    while (p < sn.w) p <<= 1;
    if (p <= 64)
        hipLaunchKernelGGL((session_seen_lists_kernel<64>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, slot, n, sn.w, p, sn.ring, sn.cnt, eptr,
                           caller, out);
    else
        hipLaunchKernelGGL((session_seen_lists_kernel<256>), dim3((unsigned)n), dim3(256), 0, s, slot, n, sn.w, p, sn.ring, sn.cnt, eptr, caller, out);
    return 1;
}

void launch_session_seen_get(const SeenView& sn, const uint32_t* slot, int n, uint32_t* out_n, uint32_t* out_items, hipStream_t s) {
    if (n > 0 && sn.w)
        hipLaunchKernelGGL(session_seen_get_kernel, dim3(blocks_for((size_t)n * sn.w)), dim3(256), 0, s, slot, n, sn.w, sn.ring, sn.cnt, out_n, out_items);
}

void launch_session_seen_set(const SeenView& sn, const uint32_t* slot, int n, const uint64_t* ptr, const uint32_t* ids, hipStream_t s) {
    if (n > 0 && sn.w)
        hipLaunchKernelGGL(session_seen_set_kernel, dim3(blocks_for((size_t)n * sn.w)), dim3(256), 0, s, slot, n, sn.w, ptr, ids, sn.ring, sn.cnt);
}

void launch_session_seen_counts(const SeenView& sn, const uint32_t* slot, int n, unsigned long long* out, hipStream_t s) {
    if (n > 0 && sn.w) hipLaunchKernelGGL(session_seen_count_kernel, dim3(blocks_for((size_t)n)), dim3(256), 0, s, slot, n, sn.cnt, out);
}

int launch_session_replay_feed(const SeenView& sn, const uint32_t* slot, const uint32_t* count, int n, int tm, const int* off,
                               const unsigned long long* start, uint32_t* items, hipStream_t s) {
    if (n <= 0 || tm <= 0 || !sn.w) return 0;
    if (off)
        hipLaunchKernelGGL(session_replay_feed_steps_kernel, dim3((unsigned)((n + 63) / 64), (unsigned)((tm + 63) / 64)), dim3(256), 0, s, slot, count,
                           n, tm, off, sn.w, sn.ring, sn.cnt, items);
    else
        hipLaunchKernelGGL(session_replay_feed_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, slot, start, count, n, sn.w, sn.ring,
                           sn.cnt, items);
    return 1;
}

namespace {
/* waves enough to fill the chip a few times over, no more than one per candidate */
inline unsigned audience_seen_grid(uint32_t num_cand) {
    const unsigned want = (num_cand + 3) / 4;
    return want < 2048u ? (want ? want : 1u) : 2048u;
}
}  // namespace

void launch_audience_seen_count(const SeenView& sn, const uint32_t* cand_slot, uint32_t num_cand, const uint32_t* qs_item,
                                const uint32_t* qs_idx, uint32_t nq, unsigned long long* total, hipStream_t s) {
    if (num_cand == 0 || nq == 0 || !sn.w || nq > audience_seen_max_queries) return;
    hipLaunchKernelGGL((audience_seen_match_kernel<false>), dim3(audience_seen_grid(num_cand)), dim3(256), 0, s, cand_slot, num_cand, sn.w, sn.ring,
                       sn.cnt, qs_item, qs_idx, nq, (uint64_t*)nullptr, 0ull, total);
}

void launch_audience_seen_fill(const SeenView& sn, const uint32_t* cand_slot, uint32_t num_cand, const uint32_t* qs_item,
                               const uint32_t* qs_idx, uint32_t nq, uint64_t* keys, unsigned long long cap, unsigned long long* cursor,
                               hipStream_t s) {
    if (num_cand == 0 || nq == 0 || !sn.w || cap == 0 || nq > audience_seen_max_queries) return;
    hipLaunchKernelGGL((audience_seen_match_kernel<true>), dim3(audience_seen_grid(num_cand)), dim3(256), 0, s, cand_slot, num_cand, sn.w, sn.ring,
                       sn.cnt, qs_item, qs_idx, nq, keys, cap, cursor);
}

void launch_audience_seen_csr(const uint64_t* keys, uint32_t n, uint32_t nq, uint64_t* eptr, uint32_t* excl, hipStream_t s) {
    const size_t threads = (size_t)n > (size_t)nq + 1 ? (size_t)n : (size_t)nq + 1;
    hipLaunchKernelGGL(audience_seen_csr_kernel, dim3(blocks_for(threads)), dim3(256), 0, s, keys, n, nq, eptr, excl);
}

}  // namespace sbr
