/* sbr_recommend.hip — exact top-k of the whole catalogue per user (sbr_recommend / sbr_recommend_reps).
 *
 *   topk_gemm_kernel  : S[u][i] = b[i] + sum_k h[u][k] E[i][k] on v_mfma_f32_32x32x2_f32 (the main loop of rank_gemm_kernel:
 *                       k ascending from 0, so every score has the bits of sbr_predict) with a top-k epilogue: per user and
 *                       item range, a running sorted list of the k best (score desc, id asc) in global scratch and its k-th
 *                       entry as the threshold in LDS.  A score that beats the threshold is staged in LDS; a full staging
 *                       buffer is sorted and merged into the list (which raises the threshold).
 *   topk_merge_kernel : one workgroup per user merges the item ranges' lists into the final k, padded with
 *                       (0xFFFFFFFF, -inf).
 * The U x I score matrix never leaves the registers.  Nothing can overflow (a staging buffer that fills is merged and the
 * candidates that did not fit are offered again), and the result is the first k of a total order, so it is deterministic. */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sbr_device.h"
#include "sbr_kernels.h"

namespace sbr {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TK_STAGE = 32;                 /* staged candidates per user between merges */
constexpr uint32_t TK_NONE = 0xFFFFFFFFu;    /* padding id; its score is -inf */

/* (score desc, id asc); -0.0 == +0.0 */
__device__ __forceinline__ bool tk_better(float as, uint32_t ai, float bs, uint32_t bi) { return as > bs || (as == bs && ai < bi); }

}  // namespace

template <int D>
__global__ __launch_bounds__(256, D <= 128 ? 2 : 1) void topk_gemm_kernel(ModelView m, const float* reps, const int* rep_row, uint32_t num_users,
                                                                         const uint64_t* excl_ptr, const uint32_t* excl_items,
                                                                         uint32_t items_per_group, uint32_t k, uint2* lists, uint32_t* lens,
                                                                         uint32_t* nonfinite_flag) {
    constexpr int LDE = D + 1;
    constexpr int KS = D / 2;
    __shared__ float Es[2][32 * LDE];
    __shared__ float Bs[2][32];
    // per-user state by accumulator slot p = wave * 32 + hh * 16 + q: user row (q & 3) + 8 (q >> 2) + 4 hh of the wave
    __shared__ float thS[128];
    __shared__ uint32_t thI[128];
    __shared__ uint32_t cnt[128];
    __shared__ uint32_t len[128];
    __shared__ uint2 st[128][TK_STAGE];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int hh = lane >> 5;
    const uint32_t G = gridDim.y;
    const uint32_t u0 = blockIdx.x * 128 + wave * 32;
    float a[KS];
    {
        const uint32_t u = u0 + l31;
        const float* h = reps + (size_t)rep_row[u < num_users ? u : num_users - 1] * D;
#pragma unroll
        for (int s = 0; s < KS; ++s) a[s] = u < num_users ? h[2 * s + hh] : 0.0f;
    }
    if (tid < 128) {
        thS[tid] = -INFINITY;
        thI[tid] = TK_NONE;
        cnt[tid] = 0;
        len[tid] = 0;
    }
    uint32_t umask = 0; /* accumulator registers q whose user exists */
#pragma unroll
    for (int q = 0; q < 16; ++q)
        if (u0 + (q & 3) + 8 * (q >> 2) + 4 * hh < num_users) umask |= 1u << q;
    bool bad = false;
    const uint32_t i_begin = blockIdx.y * items_per_group;
    uint32_t i_end = i_begin + items_per_group;
    if (i_end > m.num_items) i_end = m.num_items;
    const int ntiles = i_begin < i_end ? (int)((i_end - i_begin + 31) / 32) : 0;
    constexpr int NV = 32 * (D / 4);
    constexpr int ITER = (NV + 255) / 256;
    float4 ev[ITER];
    float bv = 0.0f;
    auto fetch = [&](int tile) {
        const uint32_t ib = i_begin + (uint32_t)tile * 32;
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int idx = tid + it * 256;
            const int r = idx / (D / 4);
            const int c4 = (idx % (D / 4)) * 4;
            ev[it] = (idx < NV && ib + r < i_end) ? ld4(m.E + (size_t)(ib + r) * D + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (tid < 32) bv = ib + tid < i_end ? m.b[ib + tid] : 0.0f;
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int idx = tid + it * 256;
            if (idx < NV) {
                const int r = idx / (D / 4);
                const int c4 = (idx % (D / 4)) * 4;
                float* dst = &Es[buf][r * LDE + c4];
                dst[0] = ev[it].x; dst[1] = ev[it].y; dst[2] = ev[it].z; dst[3] = ev[it].w;
            }
        }
        if (tid < 32) Bs[buf][tid] = bv;
    };
    // Merges the staged candidates of every user with at least `min_count` of them into the user's list.  Half a wave per user
    // (at most 32 staged), users p = wave + 4 j; a user's list is only ever touched by the same wave.
    auto merge_staged = [&](uint32_t min_count) {
        const int h32 = lane >> 5, ln = lane & 31;
        for (int j = 0; j < 16; ++j) {
            const int p = wave + 4 * (2 * j + h32);
            const uint32_t c = cnt[p];
            if (c < min_count || c == 0) continue;
            const int n = c < (uint32_t)TK_STAGE ? (int)c : TK_STAGE;
            const int qq = p & 15;
            const uint32_t ul = (uint32_t)((p >> 5) * 32 + (qq & 3) + 8 * (qq >> 2) + 4 * ((p >> 4) & 1));
            const uint32_t ug = blockIdx.x * 128 + ul;
            float s = -INFINITY;
            uint32_t id = TK_NONE;
            if (ln < n) {
                const uint2 e = st[p][ln];
                s = __uint_as_float(e.x);
                id = e.y;
                if (excl_ptr) { /* sorted, de-duplicated exclusion list of the user */
                    uint64_t lo = excl_ptr[ug], hi = excl_ptr[ug + 1];
                    while (lo < hi) {
                        const uint64_t mid = (lo + hi) >> 1;
                        if (excl_items[mid] < id) lo = mid + 1; else hi = mid;
                    }
                    if (lo < excl_ptr[ug + 1] && excl_items[lo] == id) { s = -INFINITY; id = TK_NONE; }
                }
            }
            // bitonic sort of the 32 lanes, best first
#pragma unroll
            for (int kk = 2; kk <= 32; kk <<= 1)
#pragma unroll
                for (int jj = kk >> 1; jj > 0; jj >>= 1) {
                    const float os = __shfl_xor(s, jj, 64);
                    const uint32_t oi = (uint32_t)__shfl_xor((int)id, jj, 64);
                    const bool keep_better = ((ln & jj) == 0) == ((ln & kk) == 0);
                    if (keep_better ? tk_better(os, oi, s, id) : tk_better(s, id, os, oi)) { s = os; id = oi; }
                }
            const uint64_t real = __ballot(id != TK_NONE);
            const int ne = __popcll(h32 ? (real >> 32) : (real & 0xFFFFFFFFull));
            if (ne == 0) {
                if (ln == 0) cnt[p] = 0;
                continue;
            }
            st[p][ln] = make_uint2(__float_as_uint(s), id);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const uint32_t L0 = len[p];
            uint2* L = lists + ((size_t)ug * G + blockIdx.y) * k;
            // new position of staged entry ln: ln + #{list entries better than it}
            uint32_t pos = 0;
            if (ln < ne) {
                uint32_t lo = 0, hi = L0;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    const uint2 e = L[mid];
                    if (tk_better(__uint_as_float(e.x), e.y, s, id)) lo = mid + 1; else hi = mid;
                }
                pos = (uint32_t)ln + lo;
            }
            const uint32_t first = (uint32_t)__shfl((int)pos, h32 * 32, 64); /* list entries before it stay where they are */
            // list entries [first, L0) move back by the number of staged entries better than them: chunks of 32 from the back, every
            // chunk read before it is written (a chunk's entries only move to higher positions than its own)
            if (L0 > first) {
                for (uint32_t cb = first + ((L0 - 1 - first) / 32) * 32;; cb -= 32) {
                    const uint32_t i = cb + (uint32_t)ln;
                    if (i < L0) {
                        const uint2 e = L[i];
                        const float es = __uint_as_float(e.x);
                        int lo = 0, hi = ne;
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            const uint2 sv = st[p][mid];
                            if (tk_better(__uint_as_float(sv.x), sv.y, es, e.y)) lo = mid + 1; else hi = mid;
                        }
                        const uint32_t np = i + (uint32_t)lo;
                        if (np < k) {
                            L[np] = e;
                            if (np == k - 1) { thS[p] = es; thI[p] = e.y; }
                        }
                    }
                    if (cb == first) break;
                }
            }
            if (ln < ne && pos < k) {
                L[pos] = make_uint2(__float_as_uint(s), id);
                if (pos == k - 1) { thS[p] = s; thI[p] = id; }
            }
            if (ln == 0) {
                len[p] = L0 + (uint32_t)ne < k ? L0 + (uint32_t)ne : k;
                cnt[p] = 0;
            }
        }
    };
    if (ntiles > 0) {
        fetch(0);
        stage(0);
    }
    __syncthreads();
    const int pbase = wave * 32 + hh * 16;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < ntiles) fetch(tile + 1);
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
        const float* eb = &Es[buf][l31 * LDE + hh];
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], eb[2 * s], acc, 0, 0, 0);
        const float bias = Bs[buf][l31];
        const uint32_t id = i_begin + (uint32_t)tile * 32 + (uint32_t)l31;
        uint32_t pend = id < i_end ? umask : 0u;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float sc = bias + acc[q];
            if (((pend >> q) & 1u) && !(sc - sc == 0.0f)) { bad = true; pend &= ~(1u << q); }
        }
        // offers the pending scores: below the threshold they are dropped, above it they take a staging slot if one is left
        auto offer = [&]() {
            if (!pend) return;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 t4 = ld4(&thS[pbase + 4 * q4]);
                const uint4 i4 = *reinterpret_cast<const uint4*>(&thI[pbase + 4 * q4]);
                const float ts[4] = {t4.x, t4.y, t4.z, t4.w};
                const uint32_t ti[4] = {i4.x, i4.y, i4.z, i4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int q = 4 * q4 + j;
                    const float sc = bias + acc[q];
                    if (((pend >> q) & 1u) && !tk_better(sc, id, ts[j], ti[j])) pend &= ~(1u << q);
                }
            }
            if (!pend) return;
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if ((pend >> q) & 1u) {
                    const float sc = bias + acc[q];
                    const uint32_t slot = atomicAdd(&cnt[pbase + q], 1u);
                    if (slot < (uint32_t)TK_STAGE) {
                        st[pbase + q][slot] = make_uint2(__float_as_uint(sc), id);
                        pend &= ~(1u << q);
                    }
                }
        };
        offer();
        if (tile + 1 < ntiles) stage(buf ^ 1);
        // a user whose staging filled is merged, then what did not fit is offered again (it fits: at most 32 per user and tile)
        while (__syncthreads_or(pend != 0u)) {
            merge_staged((uint32_t)TK_STAGE);
            __syncthreads();
            offer();
        }
    }
    merge_staged(1u);
    __syncthreads();
    if (tid < 128) {
        const int qq = tid & 15;
        const uint32_t u = blockIdx.x * 128 + (tid >> 5) * 32 + (qq & 3) + 8 * (qq >> 2) + 4 * ((tid >> 4) & 1);
        if (u < num_users) lens[(size_t)u * G + blockIdx.y] = len[tid];
    }
    if (__any(bad) && lane == 0) atomicOr(nonfinite_flag, 1u);
}

/* The G sorted lists of one user -> its k best, by a bitonic sort of all their entries in LDS (n = power of two >= G k, at most
 * TK_MERGE_MAX entries; empty slots hold the padding pair, which sorts last). */
__global__ __launch_bounds__(512) void topk_merge_kernel(const uint2* lists, const uint32_t* lens, uint32_t G, uint32_t k, uint32_t n,
                                                         uint32_t* out_items, float* out_scores) {
    __shared__ uint2 sm[TK_MERGE_MAX];
    const uint32_t u = blockIdx.x;
    const uint2* L = lists + (size_t)u * G * k;
    for (uint32_t e = threadIdx.x; e < n; e += blockDim.x) {
        const uint32_t g = e / k, j = e - g * k;
        sm[e] = (g < G && j < lens[(size_t)u * G + g]) ? L[e] : make_uint2(__float_as_uint(-INFINITY), TK_NONE);
    }
    __syncthreads();
    for (uint32_t kk = 2; kk <= n; kk <<= 1)
        for (uint32_t jj = kk >> 1; jj > 0; jj >>= 1) {
            for (uint32_t i = threadIdx.x; i < n / 2; i += blockDim.x) {
                const uint32_t lo = 2 * jj * (i / jj) + (i % jj), hi = lo + jj;
                const uint2 x = sm[lo], y = sm[hi];
                const bool yb = tk_better(__uint_as_float(y.x), y.y, __uint_as_float(x.x), x.y);
                const bool xb = tk_better(__uint_as_float(x.x), x.y, __uint_as_float(y.x), y.y);
                if ((lo & kk) == 0 ? yb : xb) { sm[lo] = y; sm[hi] = x; }
            }
            __syncthreads();
        }
    for (uint32_t j = threadIdx.x; j < k; j += blockDim.x) {
        const uint2 e = j < n ? sm[j] : make_uint2(__float_as_uint(-INFINITY), TK_NONE);
        out_items[(size_t)u * k + j] = e.y;
        if (out_scores) out_scores[(size_t)u * k + j] = __uint_as_float(e.x);
    }
}

uint32_t recommend_groups(uint32_t num_users, uint32_t num_items, uint32_t k, uint32_t* items_per_group) {
    const uint32_t utiles = (num_users + 127) / 128;
    // Two rounds of the chip's resident slots (two workgroups per CU at d <= 128), not launch_rank's six: a range's first k items
    // are all candidates and the rest about k ln(range / k), so fewer, longer ranges merge less (8 192 users x 1e6 items, d = 128,
    // k = 100: 113 ms of kernels at 4 608 workgroups); at most TK_MERGE_MAX / k lists per user for the merge
    constexpr uint32_t target_wgs = 256u * 2u * 2u;
    uint32_t groups = (target_wgs + utiles - 1) / utiles;
    const uint32_t max_groups = (num_items + 31) / 32;
    if (groups > max_groups) groups = max_groups;
    if (groups > TK_MERGE_MAX / k) groups = TK_MERGE_MAX / k;
    if (groups < 1) groups = 1;
    uint32_t per = (num_items + groups - 1) / groups;
    per = ((per + 31) / 32) * 32;
    groups = (num_items + per - 1) / per;
    *items_per_group = per;
    return groups;
}

void launch_recommend(const ModelView& m, const float* reps, const int* rep_row, uint32_t num_users, const uint64_t* excl_ptr,
                      const uint32_t* excl_items, uint32_t k, uint2* lists, uint32_t* lens, uint32_t* out_items, float* out_scores,
                      uint32_t* nonfinite_flag, hipStream_t s) {
    if (num_users == 0) return;
    uint32_t per = 0;
    const uint32_t groups = recommend_groups(num_users, m.num_items, k, &per);
    const uint32_t utiles = (num_users + 127) / 128;
    uint32_t n = 1;
    while (n < groups * k) n <<= 1;
#define TK_GEMM(DD)                                                                                                                        \
    hipLaunchKernelGGL((topk_gemm_kernel<DD>), dim3(utiles, groups), dim3(256), 0, s, m, reps, rep_row, num_users, excl_ptr, excl_items, per, \
                       k, lists, lens, nonfinite_flag)
    switch (m.d) {
        case 16: TK_GEMM(16); break;
        case 32: TK_GEMM(32); break;
        case 64: TK_GEMM(64); break;
        case 128: TK_GEMM(128); break;
        case 256: TK_GEMM(256); break;
        default: return;
    }
#undef TK_GEMM
    hipLaunchKernelGGL(topk_merge_kernel, dim3(num_users), dim3(512), 0, s, lists, lens, groups, k, n, out_items, out_scores);
}

}  // namespace sbr
