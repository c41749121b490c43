/* sbr_catalogue.hip — the prediction side: scores of items for a user state, and scans of the whole catalogue for a batch of
 * user states (mrr_score's ranks, rank_targets' ranks of many targets per user, recommend's top k).
 *
 *   predict_kernel         : b[i] + chain_dot(h, E[i]), k ascending from 0 (sbr_predict)
 *   rank_test_score_kernel : ts[u] = MIN if the test item is in the history, else bias + chain dot
 *   rank_gemm_kernel       : counts S[u][i] >= ts[u] (mrr_score, evaluation.rs:27-43)
 *   rank_history_kernel    : corrects the count for the (unique) history items, which the reference masks to f32::MIN
 *                            (evaluation.rs:30-32)
 *   rank_prefix_kernel     : sequence_ranks' correction of the same count for a scan row (sequence, step t) whose mask is the
 *                            sequence's own first t + 1 input items, read from the forward pass's packed rows
 *   rank_targets_*_kernel : rank_targets' exact ranks of many targets per user from one scan: prepare (thresholds, sorted per
 *                            scan-user), gemm (each score counted into the bucket between two thresholds, in LDS), finish (prefix
 *                            sums and the mask correction)
 *   topk_gemm_kernel       : per user and item range, a running sorted list of the k best (score desc, id asc) in global scratch
 *                            and its k-th entry as the threshold in LDS.  A score that beats the threshold is staged in LDS; a
 *                            full staging buffer is sorted and merged into the list (which raises the threshold).  With the
 *                            TagFilter policy an item's 32-bit tag word is tested against the user's two mask words before its
 *                            score is offered.
 *   topk_merge_kernel      : one workgroup per user merges the item ranges' lists into the final k, padded with
 *                            (0xFFFFFFFF, -inf).
 *   item_rnorm_kernel      : similar_items' r[i] = 1 / sqrt(chain_dot(E[i], E[i])) (0 for a zero row) of the whole catalogue
 *   similar_query_kernel   : similar_items' scan rows H[j] = E[q_j] * r[q_j]; the scan is topk_gemm_kernel with the ScaleMul
 *                            score policy, s(q, i) = chain_dot(H[j], E[i]) * r[i], r in the bias's place
 *   diverse_select_kernel  : recommend_diverse's greedy maximal-marginal-relevance picks from topk_merge_kernel's rows at k = pool:
 *                            one workgroup per user, the pool's rows in LDS
 *   capped_select_kernel   : recommend_capped's rule over topk_merge_kernel's rows at k = pool — an entry is kept while fewer than cap
 *                            earlier entries share its item group — and the compaction of the first k kept: one workgroup per user
 *   subset_gather_kernel   : recommend_among's sub-table E'[j] = E[S[j]], b'[j] = b[S[j]] of a sorted, unique item set S; the scan is
 *                            topk_gemm_kernel + topk_merge_kernel on a ModelView of E', b', |S|, and
 *   subset_ids_kernel      : maps the merged lists' positions in S back to catalogue ids
 *   rank_eligible_*_kernel (sbr_rank_eligible.h, included below) : rank_targets under a tag filter, through an item set or over a
 *                           session store's seen lists: the same three steps with the restriction as a mask list that is never built
 *   subset_positions_kernel, subset_words_kernel : an item set's launches (sbr_item_set_*: the sub-table is resident, gathered once):
 *                            the exclusion CSR in catalogue ids -> positions in S, in place, one wave per segment; the set's tag or
 *                            group words gathered per launch.  The sampled scan over a set is topk_gemm_kernel's GumbelMapped
 *                            policy, which hashes the noise from the rows' catalogue ids
 *   (audience)             : the reverse scan, "which rows for this item": topk_gemm_kernel with the QueryBias score policy — the
 *                            A operand is the query items' rows of E (reps = E, rep_row = the item ids), the scanned table a set of
 *                            state rows, and the bias the query's, b[q], held in LDS by slot
 *   candidate_score_kernel : score_candidates' b[i] + chain_dot(rep_u, E[i]) of a flat list of (user, item) pairs, 64 per wave
 *   partition_*_kernel     : log_partition's exact fixed-point mass of softmax(score / T) per row: shift (the row's largest scaled
 *                            score, from the top-k scan at k = 1), gemm (the catalogue scan with an epilogue that sums integer
 *                            weights), finish (the exclusion lists' items subtracted exactly)
 *   sequence_shift_kernel, partition_prefix_kernel : sequence_partition's shift and mass of a scan row (sequence, step t) whose
 *                            mask is the sequence's own first t + 1 input items: the shift from a small top-k pool, the prefix
 *                            items' weights subtracted as finish does
 *   rep_rows_kernel       : user_representations' rows rep_row[i] of H, embedding_dim floats each, in user order
 *
 * The three GEMM kernels share one catalogue scan, S[u][i] = b[i] + sum_k h[u][k] E[i][k] on v_mfma_f32_32x32x2_f32: a workgroup
 * owns 128 users (4 waves x 32, their states held in registers as MFMA A fragments) and a contiguous range of items, whose
 * 32-item tiles of E and b stream through an LDS double buffer; k ascends from 0, so every score has the bits of sbr_predict.  The
 * U x I score matrix never leaves the registers.  The top-k epilogue cannot overflow (a staging buffer that fills is merged and
 * the candidates that did not fit are offered again), and its result is the first k of a total order, so it is deterministic. */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <cstdlib>

#include "sbr_device.h"
#include "sbr_kernels.h"

namespace sbr {

namespace {

/* ---- the catalogue scan shared by rank_gemm_kernel, rank_targets_gemm_kernel and topk_gemm_kernel ---- */

/* The user of accumulator register q of a lane in wave half hh, for a wave whose 32 users start at u0 (the C layout of
 * v_mfma_f32_32x32x2_f32: row (q & 3) + 8 (q >> 2) + 4 hh; the lane's item is lane & 31). */
template <class T>
__device__ __forceinline__ T acc_user(T u0, int q, int hh) { return u0 + (q & 3) + 8 * (q >> 2) + 4 * hh; }

/* Per-user LDS state of a workgroup is indexed by slot p = wave * 32 + hh * 16 + q, the order its accumulator registers read it
 * (16-byte broadcasts); the user of slot p among the workgroup's 128. */
__device__ __forceinline__ int slot_user(int p) { return acc_user((p >> 5) * 32, p & 15, (p >> 4) & 1); }

/* A fragments of the wave's users u0 + (lane & 31), held for the whole item range: a[s] = h[u][2 s + lane / 32]; zero past the
 * last user. */
template <int D>
__device__ __forceinline__ void load_user_fragments(float (&a)[D / 2], const float* reps, const int* rep_row, uint32_t num_users,
                                                    uint32_t u0) {
    const int lane = threadIdx.x & 63;
    const uint32_t u = u0 + (lane & 31);
    const int hh = lane >> 5;
    const float* h = reps + (size_t)rep_row[u < num_users ? u : num_users - 1] * D;
#pragma unroll
    for (int s = 0; s < D / 2; ++s) a[s] = u < num_users ? h[2 * s + hh] : 0.0f;
}

/* The 32-item tiles of E and b in the workgroup's item range [i_begin, i_end) (range blockIdx.y): fetch() loads one into
 * registers, zeros past i_end; stage() writes them to one half of the LDS double buffer (E rows LDE floats apart).  Thread map:
 * idx = tid + 256 it -> item row idx / (D / 4), float4 column idx % (D / 4).  fetch_tags() / stage_tags() bring the tile's 32 item
 * tag words in beside the bias for the scan that filters by them (topk_gemm_kernel's TagFilter): the lane group behind the bias's,
 * zero past i_end. */
template <int D>
struct ItemTiles {
    static constexpr int LDE = D + 1;
    static constexpr int NV = 32 * (D / 4);
    static constexpr int ITER = (NV + 255) / 256;
    uint32_t i_begin, i_end;
    int ntiles;
    float4 ev[ITER];
    float bv = 0.0f;

    __device__ __forceinline__ ItemTiles(const ModelView& m, uint32_t items_per_group) {
        i_begin = blockIdx.y * items_per_group;
        i_end = i_begin + items_per_group;
        if (i_end > m.num_items) i_end = m.num_items;
        ntiles = i_begin < i_end ? (int)((i_end - i_begin + 31) / 32) : 0;
    }
    __device__ __forceinline__ void fetch(const ModelView& m, int tile) {
        const int tid = threadIdx.x;
        const uint32_t ib = i_begin + (uint32_t)tile * 32;
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int idx = tid + it * 256;
            const int r = idx / (D / 4);
            const int c4 = (idx % (D / 4)) * 4;
            ev[it] = (idx < NV && ib + r < i_end) ? ld4(m.E + (size_t)(ib + r) * D + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (tid < 32) bv = ib + tid < i_end ? m.b[ib + tid] : 0.0f;
    }
    __device__ __forceinline__ void stage(float* Es, float* Bs) {
        const int tid = threadIdx.x;
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int idx = tid + it * 256;
            if (idx < NV) {
                const int r = idx / (D / 4);
                const int c4 = (idx % (D / 4)) * 4;
                float* dst = &Es[r * LDE + c4];
                dst[0] = ev[it].x; dst[1] = ev[it].y; dst[2] = ev[it].z; dst[3] = ev[it].w;
            }
        }
        if (tid < 32) Bs[tid] = bv;
    }
    uint32_t tv = 0;
    __device__ __forceinline__ void fetch_tags(const uint32_t* tags, int tile) {
        const int tid = threadIdx.x;
        const uint32_t i = i_begin + (uint32_t)tile * 32 + (uint32_t)(tid - 32);
        if (tid >= 32 && tid < 64) tv = i < i_end ? tags[i] : 0u;
    }
    __device__ __forceinline__ void stage_tags(uint32_t* Ts) {
        const int tid = threadIdx.x;
        if (tid >= 32 && tid < 64) Ts[tid - 32] = tv;
    }
    /* fetch_ids() / stage_ids(): the catalogue ids a sub-table's 32 rows stand for (topk_gemm_kernel's GumbelMapped), the lane group
     * behind the tag words'; zero past i_end */
    uint32_t iv = 0;
    __device__ __forceinline__ void fetch_ids(const uint32_t* ids, int tile) {
        const int tid = threadIdx.x;
        const uint32_t i = i_begin + (uint32_t)tile * 32 + (uint32_t)(tid - 64);
        if (tid >= 64 && tid < 96) iv = i < i_end ? ids[i] : 0u;
    }
    __device__ __forceinline__ void stage_ids(uint32_t* Is) {
        const int tid = threadIdx.x;
        if (tid >= 64 && tid < 96) Is[tid - 64] = iv;
    }
};

/* One staged tile's dots: acc[q] = sum_k h[u][k] E[i][k] for user acc_user(u0, q, hh) and item lane & 31, a chain of
 * v_mfma_f32_32x32x2_f32 with k ascending from 0 (the numerics contract: bias + acc[q] has the bits of sbr_predict). */
template <int D>
__device__ __forceinline__ f32x16 tile_dots(const float (&a)[D / 2], const float* Es) {
    const int lane = threadIdx.x & 63;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    const float* eb = &Es[(lane & 31) * ItemTiles<D>::LDE + (lane >> 5)];
#pragma unroll
    for (int s = 0; s < D / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], eb[2 * s], acc, 0, 0, 0);
    return acc;
}

/* The wanted number of item ranges of a scan: by_default unless SBR_CATALOGUE_GROUPS=n (n >= 1) is set, a TEST HOOK read per call
 * (the tests force one long range or a few, whatever the split heuristics of the day prefer: tests/test_catalogue_gpu.py).  The
 * hard limits of split_items apply after it. */
uint32_t wanted_groups(uint32_t by_default) {
    const char* e = std::getenv("SBR_CATALOGUE_GROUPS");
    if (e && *e) {
        const long long n = std::atoll(e);
        if (n >= 1) return n < (long long)UINT32_MAX ? (uint32_t)n : UINT32_MAX;
    }
    return by_default;
}

/* Item ranges of a scan: `wanted` of them, but whole 32-item tiles per range, at most max_groups ranges of at most max_per items.
 * Returns the number of ranges; *items_per_group their length. */
uint32_t split_items(uint32_t num_items, uint32_t wanted, uint32_t max_groups, uint32_t max_per, uint32_t* items_per_group) {
    uint32_t groups = wanted;
    if (groups > (num_items + 31) / 32) groups = (num_items + 31) / 32;
    if (groups > max_groups) groups = max_groups;
    if (groups < 1) groups = 1;
    uint32_t per = (num_items + groups - 1) / groups;
    per = ((per + 31) / 32) * 32;
    if (per > max_per) per = max_per;
    *items_per_group = per;
    return (num_items + per - 1) / per;
}

constexpr int TK_STAGE = 32;                 /* staged candidates per user between merges */
constexpr uint32_t TK_NONE = 0xFFFFFFFFu;    /* padding id; its score is -inf */

/* (score desc, id asc).  A score of -0.0 is rare but possible (a -0.0 bias plus a chain that ends at -0.0: negative products
 * that underflow); it compares equal to +0.0, so the id orders the two, and its bits are reported as computed. */
__device__ __forceinline__ bool tk_better(float as, uint32_t ai, float bs, uint32_t bi) { return as > bs || (as == bs && ai < bi); }

}  // namespace

// ------------------------------------------------------------------------------------------------
// bias + chain-order dot (≙ an f32 MFMA accumulation over k)
// ------------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ float chain_dot(const float* __restrict__ h, const float* __restrict__ e) {
    float acc = 0.0f;
#pragma unroll
    for (int k4 = 0; k4 < D; k4 += 4) {
        const float4 v = ld4(e + k4);
        acc = sbr_fma(h[k4 + 0], v.x, acc);
        acc = sbr_fma(h[k4 + 1], v.y, acc);
        acc = sbr_fma(h[k4 + 2], v.z, acc);
        acc = sbr_fma(h[k4 + 3], v.w, acc);
    }
    return acc;
}

template <int D>
__global__ void predict_kernel(ModelView m, const float* user, const uint32_t* items, uint64_t n, float* out) {
    __shared__ float hs[D];
    for (int k = threadIdx.x; k < D; k += blockDim.x) hs[k] = user[k];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t it = items[i];
    out[i] = m.b[it] + chain_dot<D>(hs, m.E + (size_t)it * D);
}

// ------------------------------------------------------------------------------------------------
// mrr_score's ranks: the catalogue scan with a rank-count epilogue
// ------------------------------------------------------------------------------------------------
template <int D>
__global__ void rank_test_score_kernel(ModelView m, const float* reps, const int* rep_row, uint32_t num_users,
                                       const uint32_t* test_item, const uint32_t* test_in_hist, float* ts, uint32_t* ranks) {
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= num_users) return;
    const uint32_t ti = test_item[u];
    ts[u] = test_in_hist[u] ? SBR_F32_MIN : m.b[ti] + chain_dot<D>(reps + (size_t)rep_row[u] * D, m.E + (size_t)ti * D);
    ranks[u] = 0;
}

template <int D>
__global__ __launch_bounds__(256, D <= 128 ? 4 : 2) void rank_gemm_kernel(ModelView m, const float* reps, const int* rep_row, uint32_t num_users,
                                                                         const float* ts, uint32_t items_per_group, uint32_t* ranks,
                                                                         uint32_t* nonfinite_flag) {
    __shared__ float Es[2][32 * ItemTiles<D>::LDE];
    __shared__ float Bs[2][32];
    __shared__ float Ts[128]; /* thresholds by slot (slot_user) */
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int hh = lane >> 5;
    const uint32_t u0 = blockIdx.x * 128 + wave * 32;
    float a[D / 2];
    load_user_fragments<D>(a, reps, rep_row, num_users, u0);
    if (tid < 128) {
        const uint32_t u = blockIdx.x * 128 + (uint32_t)slot_user(tid);
        Ts[tid] = u < num_users ? ts[u] : 0.0f;
    }
    // per-lane counters of "score >= threshold", two 16-bit counters per register (a lane adds at most one per tile and
    // register: the launcher keeps an item range below 65 536 tiles)
    uint32_t cnt2[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) cnt2[q] = 0;
    bool bad = false;
    ItemTiles<D> tiles(m, items_per_group);
    const int ntiles = tiles.ntiles;
    if (ntiles > 0) {
        tiles.fetch(m, 0);
        tiles.stage(Es[0], Bs[0]);
    }
    __syncthreads();
    const int pbase = wave * 32 + hh * 16;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < ntiles) tiles.fetch(m, tile + 1);
        const f32x16 acc = tile_dots<D>(a, Es[buf]);
        const float bias = Bs[buf][l31];
        const bool item_ok = tiles.i_begin + (uint32_t)tile * 32 + l31 < tiles.i_end;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const float4 t4 = ld4(&Ts[pbase + 4 * q4]);
            const float tq[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = 4 * q4 + j;
                const float sc = bias + acc[q];
                if (item_ok) {
                    if (!(sc - sc == 0.0f)) bad = true;
                    if (sc >= tq[j]) cnt2[q >> 1] += (q & 1) ? 0x10000u : 1u;
                }
            }
        }
        if (tile + 1 < ntiles) tiles.stage(Es[buf ^ 1], Bs[buf ^ 1]);
        __syncthreads();
    }
    // per-user totals: sum over the 32 item lanes of each half-wave
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        int c = (int)((cnt2[q >> 1] >> ((q & 1) * 16)) & 0xFFFFu);
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
        const uint32_t u = acc_user(u0, q, hh);
        if (l31 == 0 && u < num_users && c) atomicAdd(&ranks[u], (uint32_t)c);
    }
    if (__any(bad) && lane == 0) atomicOr(nonfinite_flag, 1u);
}

template <int D>
__global__ __launch_bounds__(64) void rank_history_kernel(ModelView m, const float* reps, const int* rep_row, const float* ts,
                                                          const uint64_t* hist_ptr, const uint32_t* hist_items, uint32_t* ranks) {
    const int u = blockIdx.x;
    const float* h = reps + (size_t)rep_row[u] * D;
    const float t = ts[u];
    int cnt = 0;
    for (uint64_t e = hist_ptr[u] + threadIdx.x; e < hist_ptr[u + 1]; e += 64) {
        const uint32_t i = hist_items[e];
        const float s = m.b[i] + chain_dot<D>(h, m.E + (size_t)i * D);
        if (s >= t) --cnt;               /* it was counted by the GEMM pass ...          */
        if (SBR_F32_MIN >= t) ++cnt;     /* ... but the masked value only counts against MIN */
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (threadIdx.x == 0 && cnt) atomicAdd(&ranks[u], (uint32_t)cnt); /* two's complement: adds a negative delta */
}

/* sequence_ranks' mask correction.  A scan row is (sequence b, step t) of the forward pass's packed layout: its state is the one
 * after the input items x_0 .. x_t, its mask the distinct items among them, its target x_{t + 1}.  One wave per scan row, lane l the
 * inputs j = l, l + 64, ... <= t: where x_j is a first occurrence (first_occ, by packed row as in_idx: the flag does not depend on t,
 * so the host makes it once per sequence and a repeated item is masked once) the item is scored with rank_history_kernel's statement
 * and corrected by its two lines.  The items come from the packed in_idx rows off[j] + b that the forward pass uploaded: nothing of
 * size sum(t) exists.  The row's count belongs to this wave alone and the scan's atomics have finished in stream order, so it is added
 * with a plain read and write.
 *
 * The item rows of a sequence are read again by each of its steps' waves.  They are not staged in LDS: a sequence's steps are
 * neighbouring waves of neighbouring workgroups, the rows of one sequence are at most T x d floats (128 KB at T = 128, d = 256, 32 KB
 * at T = 64, d = 128) and stay in L2 between them, and the whole pass is about T / 2 dots per scan row against the scan's num_items —
 * 32 against 1e6 at T = 64.  A workgroup per sequence with the rows in LDS would need the t tiling above 64 KB and a launch shaped by
 * sequences where `last` keeps a few rows of each; neither pays for itself at that share. */
template <int D>
__global__ __launch_bounds__(256) void rank_prefix_kernel(ModelView m, const float* reps, const int* rep_row, const float* ts,
                                                           const uint2* unit_bt, uint32_t num_units, const int* off,
                                                           const uint32_t* in_idx, const uint32_t* first_occ, uint32_t* ranks) {
    const uint32_t unit = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= num_units) return; /* the whole wave */
    const uint32_t lane = threadIdx.x & 63;
    const uint2 bt = unit_bt[unit]; /* (b, t) */
    const float* h = reps + (size_t)rep_row[unit] * D;
    const float t = ts[unit];
    int cnt = 0;
    for (uint32_t j = lane; j <= bt.y; j += 64) {
        const uint32_t r = (uint32_t)off[j] + bt.x;
        if (!first_occ[r]) continue;
        const uint32_t i = in_idx[r];
        const float s = m.b[i] + chain_dot<D>(h, m.E + (size_t)i * D);
        if (s >= t) --cnt;               /* it was counted by the GEMM pass ...          */
        if (SBR_F32_MIN >= t) ++cnt;     /* ... but the masked value only counts against MIN */
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0 && cnt) ranks[unit] += (uint32_t)cnt; /* two's complement: adds a negative delta */
}

// ------------------------------------------------------------------------------------------------
// rank_targets: the catalogue scan with a multi-threshold rank epilogue
// ------------------------------------------------------------------------------------------------
/* A scan-user is one user state with at most TM targets (the host splits a user with more into several scan-users that share a
 * representation row); scan-user s owns the targets [sptr[s], sptr[s + 1]) of the launch's flat target list.
 *
 * One thread per (scan-user, slot j < TM): the threshold of target j, ts = m(u, t) — MIN if the target is in the user's mask list,
 * else bias + chain dot — then the scan-user's thresholds in descending order (position = number of thresholds that come before:
 * greater, or equal with a lower slot) into th[s][0..n), padded with -inf up to TM; tmin[s] = the lowest and tmin2[s] the one before
 * it (+inf where there is one threshold); the buckets and the total zeroed. */
template <int D, int TM>
__global__ __launch_bounds__(256) void rank_targets_prepare_kernel(ModelView m, const float* reps, const int* rep_row, const uint32_t* su_user,
                                                                   const uint32_t* sptr, uint32_t num_su, const uint32_t* tgt_items,
                                                                   const uint64_t* mask_ptr, const uint32_t* mask_items, float* ts, uint32_t* pos,
                                                                   float* th, float* tmin, float* tmin2, uint32_t* buckets,
                                                                   uint32_t* totals) {
    __shared__ float tl[256];
    const int tid = threadIdx.x;
    const int j = tid % TM;
    const uint32_t s = blockIdx.x * (256 / TM) + tid / TM;
    uint32_t e = 0, n = 0;
    float t = -INFINITY;
    if (s < num_su) {
        e = sptr[s] + j;
        n = sptr[s + 1] - sptr[s];
    }
    const bool real = (uint32_t)j < n;
    if (real) {
        const uint32_t ti = tgt_items[e];
        bool masked = false;
        if (mask_ptr) { /* sorted, de-duplicated mask list of the user */
            const uint32_t u = su_user[s];
            uint64_t lo = mask_ptr[u], hi = mask_ptr[u + 1];
            while (lo < hi) {
                const uint64_t mid = (lo + hi) >> 1;
                if (mask_items[mid] < ti) lo = mid + 1; else hi = mid;
            }
            masked = lo < mask_ptr[u + 1] && mask_items[lo] == ti;
        }
        t = masked ? SBR_F32_MIN : m.b[ti] + chain_dot<D>(reps + (size_t)rep_row[s] * D, m.E + (size_t)ti * D);
    }
    tl[tid] = t;
    __syncthreads();
    if (s >= num_su) return;
    uint32_t p = (uint32_t)j; /* the padding keeps its slot (>= n) */
    if (real) {
        p = 0;
        const float* mine = &tl[tid - j];
        for (uint32_t o = 0; o < n; ++o) {
            const float x = mine[o];
            p += (x > t || (x == t && o < (uint32_t)j)) ? 1u : 0u;
        }
        ts[e] = t;
        pos[e] = p;
        if (p == n - 1) tmin[s] = t;
        if (p + 2 == n) tmin2[s] = t;
    }
    if (j == 0) {
        if (n == 1) tmin2[s] = INFINITY;
        totals[s] = 0;
    }
    th[(size_t)s * TM + p] = t;
    buckets[(size_t)s * TM + j] = 0;
}

/* The scan.  Per workgroup and slot (slot_user) the TM descending thresholds and TM buckets live in LDS.  A score sc of a real item
 * that reaches the slot's lowest threshold (the one compare rank_gemm_kernel pays too) is counted in the lane's registers as there:
 * the total is the rank of the lowest target.  A score that also reaches the second lowest threshold is searched: j = #{thresholds
 * > sc}, which is below n - 1 for n thresholds because the last two are not above sc, and bucket j counts it with an LDS atomic; rank
 * of the target at sorted position r < n - 1 = sum of buckets 0..r.  So one target per user costs no search and no atomic, and a
 * trained model, whose scores mostly lie below all but the lowest targets, few.  The search is branch-free over the -inf padded
 * array (log2 TM dependent LDS reads), and the 16 users of a lane take each step together so the reads of a step are in flight at
 * once.  Within a half-wave the 32 lanes read one slot's TM consecutive words: distinct banks or a broadcast.  Buckets are 32 bits
 * wide; the lane counters 16, two per register: the launcher keeps an item range below 65 536 tiles. */
template <int D, int TM>
__global__ __launch_bounds__(256, D <= 128 ? 3 : 2) void rank_targets_gemm_kernel(ModelView m, const float* reps, const int* rep_row, uint32_t num_su,
                                                                                 const float* th, const float* tmin, const float* tmin2,
                                                                                 uint32_t items_per_group, uint32_t* buckets, uint32_t* totals,
                                                                                 uint32_t* nonfinite_flag) {
    __shared__ float Es[2][32 * ItemTiles<D>::LDE];
    __shared__ float Bs[2][32];
    __shared__ float Tmin[128];      /* by slot (slot_user) */
    __shared__ float Tmin2[128];
    __shared__ float Th[128 * TM];
    __shared__ uint32_t Hist[128 * TM];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int hh = lane >> 5;
    const uint32_t u0 = blockIdx.x * 128 + wave * 32;
    float a[D / 2];
    load_user_fragments<D>(a, reps, rep_row, num_su, u0);
    if (tid < 128) {
        const uint32_t u = blockIdx.x * 128 + (uint32_t)slot_user(tid);
        Tmin[tid] = u < num_su ? tmin[u] : INFINITY; /* no scan-user: nothing passes */
        Tmin2[tid] = u < num_su ? tmin2[u] : INFINITY;
    }
    uint32_t cnt2[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) cnt2[q] = 0;
    for (int idx = tid; idx < 128 * TM; idx += 256) {
        const uint32_t u = blockIdx.x * 128 + (uint32_t)slot_user(idx / TM);
        Th[idx] = u < num_su ? th[(size_t)u * TM + idx % TM] : -INFINITY;
        Hist[idx] = 0;
    }
    bool bad = false;
    ItemTiles<D> tiles(m, items_per_group);
    const int ntiles = tiles.ntiles;
    if (ntiles > 0) {
        tiles.fetch(m, 0);
        tiles.stage(Es[0], Bs[0]);
    }
    __syncthreads();
    const int pbase = wave * 32 + hh * 16;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < ntiles) tiles.fetch(m, tile + 1);
        const f32x16 acc = tile_dots<D>(a, Es[buf]);
        const float bias = Bs[buf][l31];
        const bool item_ok = tiles.i_begin + (uint32_t)tile * 32 + l31 < tiles.i_end;
        uint32_t pass = 0; /* accumulator registers q whose score reaches the slot's second lowest threshold */
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const float4 t4 = ld4(&Tmin[pbase + 4 * q4]);
            const float4 s4 = ld4(&Tmin2[pbase + 4 * q4]);
            const float tq[4] = {t4.x, t4.y, t4.z, t4.w};
            const float sq[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = 4 * q4 + j;
                const float sc = bias + acc[q];
                if (item_ok) {
                    if (!(sc - sc == 0.0f)) bad = true;
                    if (sc >= tq[j]) cnt2[q >> 1] += (q & 1) ? 0x10000u : 1u;
                    if (sc >= sq[j]) pass |= 1u << q;
                }
            }
        }
        if (__any(pass != 0u)) {
            int at[16]; /* #{thresholds > score} so far */
#pragma unroll
            for (int q = 0; q < 16; ++q) at[q] = 0;
#pragma unroll
            for (int step = TM / 2; step >= 1; step >>= 1)
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    if (Th[(pbase + q) * TM + at[q] + step - 1] > bias + acc[q]) at[q] += step;
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if ((pass >> q) & 1u) atomicAdd(&Hist[(pbase + q) * TM + at[q]], 1u);
        }
        if (tile + 1 < ntiles) tiles.stage(Es[buf ^ 1], Bs[buf ^ 1]);
        __syncthreads();
    }
    // per-slot totals: sum over the 32 item lanes of each half-wave
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        int c = (int)((cnt2[q >> 1] >> ((q & 1) * 16)) & 0xFFFFu);
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
        const uint32_t u = acc_user(u0, q, hh);
        if (l31 == 0 && u < num_su && c) atomicAdd(&totals[u], (uint32_t)c);
    }
    // the workgroup's buckets join the other item ranges'
    for (int idx = tid; idx < 128 * TM; idx += 256) {
        const uint32_t u = blockIdx.x * 128 + (uint32_t)slot_user(idx / TM);
        const uint32_t c = Hist[idx];
        if (u < num_su && c) atomicAdd(&buckets[(size_t)u * TM + idx % TM], c);
    }
    if (__any(bad) && lane == 0) atomicOr(nonfinite_flag, 1u);
}

/* One wave per scan-user: the mask correction of every target (rank_history_kernel's, with each masked item scored once for all
 * the scan-user's targets: its real score leaves the count, its masked value counts only against thresholds <= MIN), then
 * rank = buckets 0..position (the total at the last position) + correction. */
template <int D, int TM>
__global__ __launch_bounds__(64) void rank_targets_finish_kernel(ModelView m, const float* reps, const int* rep_row, const uint32_t* su_user,
                                                                 const uint32_t* sptr, const float* ts, const uint32_t* pos,
                                                                 const uint32_t* buckets, const uint32_t* totals, const uint64_t* mask_ptr,
                                                                 const uint32_t* mask_items, uint32_t* ranks) {
    __shared__ float tl[TM];
    __shared__ int delta[TM];
    const uint32_t s = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t e0 = sptr[s];
    const int n = (int)(sptr[s + 1] - e0);
    if (lane < TM) tl[lane] = lane < n ? ts[e0 + lane] : INFINITY;
    __syncthreads();
    int cnt[TM];
#pragma unroll
    for (int r = 0; r < TM; ++r) cnt[r] = 0;
    if (mask_ptr) {
        const uint32_t u = su_user[s];
        const float* h = reps + (size_t)rep_row[s] * D;
        for (uint64_t e = mask_ptr[u] + lane; e < mask_ptr[u + 1]; e += 64) {
            const uint32_t i = mask_items[e];
            const float sc = m.b[i] + chain_dot<D>(h, m.E + (size_t)i * D);
#pragma unroll
            for (int r = 0; r < TM; ++r) {
                const float t = tl[r];
                cnt[r] += (SBR_F32_MIN >= t ? 1 : 0) - (sc >= t ? 1 : 0);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < TM; ++r) {
        int c = cnt[r];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
        if (lane == r) delta[r] = c;
    }
    __syncthreads();
    if (lane < n) {
        const uint32_t p = pos[e0 + lane];
        uint32_t rank = 0;
        if (p + 1 == (uint32_t)n) rank = totals[s];
        else
            for (uint32_t j = 0; j <= p; ++j) rank += buckets[(size_t)s * TM + j];
        ranks[e0 + lane] = rank + (uint32_t)delta[lane]; /* two's complement: adds a negative delta */
    }
}

// ------------------------------------------------------------------------------------------------
// recommend's top k: the catalogue scan with a top-k epilogue, then a merge of the item ranges
// ------------------------------------------------------------------------------------------------
/* What the scan's per-item value (the Bs tile, ModelView::b) does to a dot: recommend adds the item bias, similar_items multiplies
 * by the item's reciprocal norm (launch_similar_items passes a ModelView whose b is r).  The policy is a constant and TK_SCORE the
 * one statement of the score, a macro on purpose: through a function of the policy — a forceinline static member, a plain one, a
 * lambda in the kernel — the BiasAdd instantiations compiled to 12 more VGPRs at every d <= 128 (101 -> 113 at d = 16, 178 -> 190
 * at d = 128); this form leaves their instruction streams what they were (profiles/similar_items_8192x1M_d128.md). */
struct BiasAdd {
    static constexpr bool scale = false, query = false, gumbel = false, mapped = false;
    struct Args {};
};
struct ScaleMul {
    static constexpr bool scale = true, query = false, gumbel = false, mapped = false;
    struct Args {};
};
/* audience's policy: the bias belongs to the scan's "user" — a query item q whose row E[q] is the A operand — not to the scanned
 * row (a session's state): score = b[q] + chain_dot(E[q], h_s), the bits of predict for (h_s, q) because every product of the chain
 * commutes.  The workgroup's 128 queries' biases sit in LDS by slot (qbS, as thS) and are added to the tile's accumulators once,
 * ahead of the epilogue, which then reads acc[q] as the score; the scanned row's Bs value takes no part.  Args is empty for the
 * other two policies, at the end of the argument block behind Filter::Args, and every statement of this one sits under
 * `if constexpr`: their instantiations keep their instruction streams (profiles/audience_asm_stats.md). */
struct QueryBias {
    static constexpr bool scale = false, query = true, gumbel = false, mapped = false;
    struct Args {
        const float* qb; /* [the A table's rows]: the bias of query item rep_row[u] */
    };
};
/* recommend_sampled's policy: what the epilogue orders is not the score s = b[i] + dot but the key fl(fl(s * inv_t) + g(u, i)), g the
 * counter-keyed Gumbel noise of sbr_numerics.h under the row's key K[u] — the k best keys are k draws without replacement from
 * softmax(s / T).  The rows' k0 / k1 sit in LDS by slot (gk0S / gk1S, as qbS) and acc[q] holds the key from the first stage on.  The
 * noise costs about as much vector ALU as a tile's MFMA chain takes, so it is evaluated only where it can matter; a pending score
 * passes three stages, each of which may drop it once the row's list is full (the threshold is -inf before):
 *   1. t = fl(s * inv_t) for every score; dropped unless fl(t + G_MAX) beats the row's threshold, G_MAX the largest g there is;
 *   2. the 23 noise bits r are hashed; dropped unless fl(t + G[r >> 13]) beats the threshold, G[j] the largest g of the j-th of
 *      1 024 equal ranges of r (gubS, computed by the workgroup: g never decreases in r, so it is g at the range's last r).  A
 *      wave pays for stage 3 whenever one of its 64 lanes survives, so the table is fine-grained: with 64 ranges a score survived
 *      with probability 1 / 64 at least and most waves went on (profiles/sampled_8192x1M_d128.md);
 *   3. the two logarithms, key = fl(t + g).
 * f32 addition is monotone and tk_better is monotone in the score at a fixed id, so a bound that does not beat the threshold means
 * the key does not either: the stages change no result (tests/test_sampled_gpu.py holds every bit to the numpy statement).
 * The non-finite test is on t: t is non-finite whenever s is (inv_t is finite and not zero), and a finite t cannot give a non-finite
 * key (|g| < 17 is below half an ulp of any t that close to overflow), so "a non-finite score or key of a scanned pair fails the
 * call" is decided before any stage drops anything.  The tag filter runs between stages 1 and 2: a disallowed item is never hashed.
 * Every statement of the policy sits under `if constexpr` and its Args are at the end of the argument block: the other
 * instantiations keep their instruction streams (profiles/sampled_asm_stats.md). */
struct GumbelBias {
    static constexpr bool scale = false, query = false, gumbel = true, mapped = false;
    struct Args {
        float inv_t;
        const uint64_t* keys; /* [num_users]: the row key K of scan row u (sample_keys_kernel) */
    };
};
/* GumbelBias over an item set's sub-table: the noise of (row, item) is a function of the item's CATALOGUE id, and the scanned row j
 * stands for item ids[j].  A tile's 32 id words come in beside its biases as the tag words do (Is, a double buffer: 256 more bytes of
 * LDS) and stages 2 and 3 hash the lane's id word where GumbelBias hashes `id`.  Thresholds, tie-breaks and staged entries stay
 * positions: ids ascends, so the order of positions is the order of ids and no result differs from the scan of the whole catalogue
 * with every other item excluded.  A policy of its own, every statement under `if constexpr`: the other instantiations keep their
 * instruction streams (profiles/item_set_asm_stats.md). */
struct GumbelMapped {
    static constexpr bool scale = false, query = false, gumbel = true, mapped = true;
    struct Args {
        float inv_t;
        const uint64_t* keys;
        const uint32_t* ids; /* [m.num_items]: the catalogue id of scanned row j, ascending */
    };
};
#define TK_SCORE(q) ((Score::query || Score::gumbel) ? acc[q] : Score::scale ? acc[q] * bias : bias + acc[q])

/* Whether the scan filters items by tag, the third constant policy.  TagFilter: item i is offered to user u only if
 * (tags[i] & none_of[u]) == 0 && (any_of[u] == 0 || (tags[i] & any_of[u]) != 0) — tags [num_items] the model's item tags, any_of /
 * none_of [num_users] the launch's masks.  A tile's 32 tag words come in beside its biases (Ts, a double buffer as Bs) and the
 * workgroup's 128 users' masks sit in LDS by slot for the whole range (with a third word per user, 1 where any_of is 0, so that
 * the any_of test is one AND-OR and one compare), read as thS / thI are: 1 792 more bytes of LDS.  The test
 * clears bits of `pend` behind the non-finite test, which therefore still sees every scanned score, and before the first offer(),
 * so an item that is not allowed never takes a staging slot; nothing else of the epilogue knows of the filter.  The result is the
 * first k of the same total order over the allowed items that are not excluded: what exclusion lists holding every other item give.
 * NoFilter's arguments are an empty struct at the end of the argument block and every statement of the filter sits under
 * `if constexpr`: those instantiations keep their instruction streams (profiles/filtered_asm_stats.md). */
struct NoFilter {
    static constexpr bool on = false;
    struct Args {};
};
struct TagFilter {
    static constexpr bool on = true;
    struct Args {
        const uint32_t *tags, *any_of, *none_of;
    };
};

template <int D, class Score, class Filter>
__global__ __launch_bounds__(256, D <= 128 ? 2 : 1) void topk_gemm_kernel(ModelView m, const float* reps, const int* rep_row, uint32_t num_users,
                                                                         const uint64_t* excl_ptr, const uint32_t* excl_items,
                                                                         uint32_t items_per_group, uint32_t k, uint2* lists, uint32_t* lens,
                                                                         uint32_t* nonfinite_flag, typename Filter::Args fa,
                                                                         typename Score::Args sa) {
    __shared__ float Es[2][32 * ItemTiles<D>::LDE];
    __shared__ float Bs[2][32];
    __shared__ __align__(16) float qbS[Score::query ? 128 : 4]; /* QueryBias only: the queries' biases by slot (slot_user) */
    // GumbelBias only: the rows' keys by slot (slot_user), and the largest noise of each of 1 024 equal ranges of the noise bits
    __shared__ uint32_t gk0S[Score::gumbel ? 128 : 1];
    __shared__ uint32_t gk1S[Score::gumbel ? 128 : 1];
    __shared__ float gubS[Score::gumbel ? 1024 : 1];
    // TagFilter only: the tiles' tag words, and the users' masks by slot (slot_user), read 16 bytes at a time
    __shared__ uint32_t Ts[2][Filter::on ? 32 : 1];
    __shared__ __align__(16) uint32_t anyS[Filter::on ? 128 : 4];
    __shared__ __align__(16) uint32_t anyZ[Filter::on ? 128 : 4]; /* 1 where the user's any_of is 0 (every tag passes it), else 0 */
    __shared__ __align__(16) uint32_t noneS[Filter::on ? 128 : 4];
    // per-user state by slot (slot_user)
    __shared__ float thS[128];
    __shared__ uint32_t thI[128];
    __shared__ uint32_t cnt[128];
    __shared__ uint32_t len[128];
    __shared__ uint2 st[128][TK_STAGE];
    // GumbelMapped only: the tiles' catalogue id words
    __shared__ uint32_t Is[2][Score::mapped ? 32 : 1];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int hh = lane >> 5;
    const uint32_t G = gridDim.y;
    const uint32_t u0 = blockIdx.x * 128 + wave * 32;
    float a[D / 2];
    load_user_fragments<D>(a, reps, rep_row, num_users, u0);
    if (tid < 128) {
        thS[tid] = -INFINITY;
        thI[tid] = TK_NONE;
        cnt[tid] = 0;
        len[tid] = 0;
        if constexpr (Filter::on) {
            const uint32_t u = blockIdx.x * 128 + (uint32_t)slot_user(tid);
            const uint32_t any = u < num_users ? fa.any_of[u] : 0u;
            anyS[tid] = any;
            anyZ[tid] = any == 0u ? 1u : 0u;
            noneS[tid] = u < num_users ? fa.none_of[u] : 0u;
        }
        if constexpr (Score::query) {
            const uint32_t u = blockIdx.x * 128 + (uint32_t)slot_user(tid);
            qbS[tid] = u < num_users ? sa.qb[rep_row[u]] : 0.0f;
        }
        if constexpr (Score::gumbel) {
            const uint32_t u = blockIdx.x * 128 + (uint32_t)slot_user(tid);
            const uint64_t K = u < num_users ? sa.keys[u] : 0ull;
            gk0S[tid] = (uint32_t)K;
            gk1S[tid] = (uint32_t)(K >> 32);
        }
    }
    if constexpr (Score::gumbel) {
#pragma unroll
        for (int j = tid; j < 1024; j += 256) gubS[j] = sbr_gumbel_of_bits((((uint32_t)j + 1u) << 13) - 1u);
    }
    uint32_t umask = 0; /* accumulator registers q whose user exists */
#pragma unroll
    for (int q = 0; q < 16; ++q)
        if (acc_user(u0, q, hh) < num_users) umask |= 1u << q;
    bool bad = false;
    ItemTiles<D> tiles(m, items_per_group);
    const int ntiles = tiles.ntiles;
    // Merges the staged candidates of every user with at least `min_count` of them into the user's list.  Half a wave per user
    // (at most 32 staged), users p = wave + 4 j; a user's list is only ever touched by the same wave.
    auto merge_staged = [&](uint32_t min_count) {
        const int h32 = lane >> 5, ln = lane & 31;
        for (int j = 0; j < 16; ++j) {
            const int p = wave + 4 * (2 * j + h32);
            const uint32_t c = cnt[p];
            if (c < min_count || c == 0) continue;
            const int n = c < (uint32_t)TK_STAGE ? (int)c : TK_STAGE;
            const int qq = p & 15; /* slot_user(p) written out: through the helper this kernel compiled up to 3 % slower (d = 128) */
            const uint32_t ug = blockIdx.x * 128 + (uint32_t)((p >> 5) * 32 + (qq & 3) + 8 * (qq >> 2) + 4 * ((p >> 4) & 1));
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
        tiles.fetch(m, 0);
        tiles.stage(Es[0], Bs[0]);
        if constexpr (Filter::on) {
            tiles.fetch_tags(fa.tags, 0);
            tiles.stage_tags(Ts[0]);
        }
        if constexpr (Score::mapped) {
            tiles.fetch_ids(sa.ids, 0);
            tiles.stage_ids(Is[0]);
        }
    }
    __syncthreads();
    const int pbase = wave * 32 + hh * 16;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < ntiles) {
            tiles.fetch(m, tile + 1);
            if constexpr (Filter::on) tiles.fetch_tags(fa.tags, tile + 1);
            if constexpr (Score::mapped) tiles.fetch_ids(sa.ids, tile + 1);
        }
        f32x16 acc = tile_dots<D>(a, Es[buf]);
        const float bias = Bs[buf][l31];
        if constexpr (Score::query) { /* the score is b[q] + dot, one rounding, as predict's; acc[q] holds it from here on */
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 b4 = ld4(&qbS[pbase + 4 * q4]);
                acc[4 * q4 + 0] = b4.x + acc[4 * q4 + 0];
                acc[4 * q4 + 1] = b4.y + acc[4 * q4 + 1];
                acc[4 * q4 + 2] = b4.z + acc[4 * q4 + 2];
                acc[4 * q4 + 3] = b4.w + acc[4 * q4 + 3];
            }
        }
        const uint32_t id = tiles.i_begin + (uint32_t)tile * 32 + (uint32_t)l31;
        uint32_t pend = id < tiles.i_end ? umask : 0u;
        if constexpr (Score::gumbel) { /* stage 1: acc[q] = t, the non-finite test, and the bound that needs no hash */
            const float gmax = gubS[1023];
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 t4 = ld4(&thS[pbase + 4 * q4]);
                const uint4 i4 = *reinterpret_cast<const uint4*>(&thI[pbase + 4 * q4]);
                const float ts[4] = {t4.x, t4.y, t4.z, t4.w};
                const uint32_t ti[4] = {i4.x, i4.y, i4.z, i4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int q = 4 * q4 + j;
                    const float t = __fmul_rn(bias + acc[q], sa.inv_t);
                    acc[q] = t;
                    const bool nf = !(t - t == 0.0f);
                    if (((pend >> q) & 1u) && nf) bad = true;
                    if (nf || !tk_better(__fadd_rn(t, gmax), id, ts[j], ti[j])) pend &= ~(1u << q);
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float sc = TK_SCORE(q);
                if (((pend >> q) & 1u) && !(sc - sc == 0.0f)) { bad = true; pend &= ~(1u << q); }
            }
        }
        if constexpr (Filter::on) { /* the lane's item against its 16 users' masks: what is not allowed is not offered */
            const uint32_t tag = Ts[buf][l31];
            uint32_t drop = 0;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const uint4 a4 = *reinterpret_cast<const uint4*>(&anyS[pbase + 4 * q4]);
                const uint4 z4 = *reinterpret_cast<const uint4*>(&anyZ[pbase + 4 * q4]);
                const uint4 n4 = *reinterpret_cast<const uint4*>(&noneS[pbase + 4 * q4]);
                const uint32_t any[4] = {a4.x, a4.y, a4.z, a4.w};
                const uint32_t anyz[4] = {z4.x, z4.y, z4.z, z4.w};
                const uint32_t none[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    /* two ANDs (one with the OR folded in) and two compares per user; `|`, not `||`: with the short-circuit form
                     * the compiler put every user's any_of test behind a branch on its none_of test (two exec-mask regions per
                     * user and tile) */
                    const uint32_t hit = (tag & none[j]) != 0u ? 1u : 0u;
                    const uint32_t miss = ((tag & any[j]) | anyz[j]) == 0u ? 1u : 0u;
                    drop |= (hit | miss) << (4 * q4 + j);
                }
            }
            pend &= ~drop;
        }
        if constexpr (Score::gumbel) { /* stages 2 and 3, for what is still pending: the hash, the range's bound, the noise */
            uint32_t nid = id; /* what the noise is a function of: the item's catalogue id */
            if constexpr (Score::mapped) nid = Is[buf][l31];
            if (pend) {
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    if ((pend >> q) & 1u) {
                        const uint32_t r = sbr_gumbel_bits(gk0S[pbase + q], gk1S[pbase + q], nid);
                        const float t = acc[q];
                        if (!tk_better(__fadd_rn(t, gubS[r >> 13]), id, thS[pbase + q], thI[pbase + q])) pend &= ~(1u << q);
                        else acc[q] = __fadd_rn(t, sbr_gumbel_of_bits(r));
                    }
            }
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
                    const float sc = TK_SCORE(q);
                    if (((pend >> q) & 1u) && !tk_better(sc, id, ts[j], ti[j])) pend &= ~(1u << q);
                }
            }
            if (!pend) return;
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if ((pend >> q) & 1u) {
                    const float sc = TK_SCORE(q);
                    const uint32_t slot = atomicAdd(&cnt[pbase + q], 1u);
                    if (slot < (uint32_t)TK_STAGE) {
                        st[pbase + q][slot] = make_uint2(__float_as_uint(sc), id);
                        pend &= ~(1u << q);
                    }
                }
        };
        offer();
        if (tile + 1 < ntiles) {
            tiles.stage(Es[buf ^ 1], Bs[buf ^ 1]);
            if constexpr (Filter::on) tiles.stage_tags(Ts[buf ^ 1]);
            if constexpr (Score::mapped) tiles.stage_ids(Is[buf ^ 1]);
        }
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
        const uint32_t u = blockIdx.x * 128 + (uint32_t)slot_user(tid);
        if (u < num_users) lens[(size_t)u * G + blockIdx.y] = len[tid];
    }
    if (__any(bad) && lane == 0) atomicOr(nonfinite_flag, 1u);
}
/* TK_SCORE stays defined up to above_gemm_kernel, the other kernel that states a score by policy */

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

// ------------------------------------------------------------------------------------------------
// similar_items: reciprocal norms of the catalogue and the scaled query rows; the scan is topk_gemm_kernel<D, ScaleMul>
// ------------------------------------------------------------------------------------------------
/* r[i] = n2 > 0 ? 1 / sqrt(n2) : 0 with n2 = chain_dot(E[i], E[i]), and the non-finite flag for a non-finite n2; without `cosine`
 * r is all 1.0f and nothing is checked (x * 1.0f is exact: the dot-product metric is the same scan).  The chain over a row is
 * sequential, so one thread owns a row; a workgroup's 256 rows come through LDS CH columns at a time, rows CH + 1 floats apart
 * (ItemTiles' stride: a wave reads one column of 64 rows from distinct banks), so the global loads are whole 128-byte pieces of
 * rows next to each other, not 64 lanes at a stride of 4 D bytes. */
template <int D>
__global__ __launch_bounds__(256) void item_rnorm_kernel(ModelView m, int cosine, float* r, uint32_t* nonfinite_flag) {
    constexpr int CH = D < 32 ? D : 32;
    constexpr int LD = CH + 1;
    constexpr int ITER = CH / 4; /* float4 loads per thread and column block: 256 rows x CH / 4 quads over 256 threads */
    __shared__ float Xs[256 * LD];
    const int tid = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * 256;
    const uint64_t row = row0 + (uint64_t)tid;
    if (!cosine) {
        if (row < m.num_items) r[row] = 1.0f;
        return;
    }
    float n2 = 0.0f;
    for (int c0 = 0; c0 < D; c0 += CH) {
        float4 ev[ITER];
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int idx = tid + it * 256;
            const int rr = idx / (CH / 4);
            const int c4 = (idx % (CH / 4)) * 4;
            ev[it] = row0 + rr < m.num_items ? ld4(m.E + (size_t)(row0 + rr) * D + c0 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int idx = tid + it * 256;
            float* dst = &Xs[(idx / (CH / 4)) * LD + (idx % (CH / 4)) * 4];
            dst[0] = ev[it].x; dst[1] = ev[it].y; dst[2] = ev[it].z; dst[3] = ev[it].w;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const float x = Xs[tid * LD + k];
            n2 = sbr_fma(x, x, n2);
        }
        __syncthreads();
    }
    bool bad = false;
    if (row < m.num_items) {
        bad = !(n2 - n2 == 0.0f);
        r[row] = n2 > 0.0f ? 1.0f / __builtin_sqrtf(n2) : 0.0f;
    }
    if (__any(bad) && (tid & 63) == 0) atomicOr(nonfinite_flag, 1u);
}

/* The scan rows of the launch's queries at storage width: H[j][c] = E[q_j][c] * r[q_j], each product rounded to f32 (the padding
 * columns stay zero because E's are). */
template <int D>
__global__ __launch_bounds__(256) void similar_query_kernel(ModelView m, const float* r, const uint32_t* query, uint32_t num_queries, float* H) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t j = idx / (D / 4);
    const int c4 = (int)(idx % (D / 4)) * 4;
    if (j >= num_queries) return;
    const uint32_t q = query[j];
    const float s = r[q];
    const float4 v = ld4(m.E + (size_t)q * D + c4);
    st4(H + (size_t)j * D + c4, make_float4(v.x * s, v.y * s, v.z * s, v.w * s));
}

// ------------------------------------------------------------------------------------------------
// recommend_diverse: greedy maximal-marginal-relevance selection of k_out items from the pool of a user's best `pool`
// ------------------------------------------------------------------------------------------------
/* One workgroup per user.  Its pool is row u of topk_merge_kernel's output at k = pool: n real entries, best first, then padding.
 * Dynamic LDS, sized by the launch's pool (not the largest one, so small pools keep several workgroups on a CU):
 *     qh [D]            the last pick's row scaled by its r (similar_items' qhat)
 *     X  [pool][D + 1]  the pool's rows, gathered by id once: whole 16-byte pieces, streaming (every row is read once per user);
 *                       rows D + 1 floats apart (ItemTiles' stride), so lanes that own different rows read different banks
 *     id, s, mx, r, pk [pool]   ids, pool scores, the running maximum similarity to the picks, reciprocal norms, picked flags
 *     red [8]           the waves' (value, position) of a round's arg-max
 * r is item_rnorm_kernel's formula over the pool's rows only (a non-finite row outside every pool does not matter here), all 1.0f
 * for the dot metric.  Thread tid owns the pool positions tid, tid + 256, ...: in each round it runs similar_items' score of the
 * last pick a against its unpicked rows, sim = chain_dot(E[a] * r[a], E[c_j]) * r[c_j] with k ascending from +0.0, folds it into
 * mx, and offers v = lam * s - mu * mx — two products and a difference, each rounded to f32 — to the arg-max (value descending,
 * position ascending: a total order, v is never NaN while s and mx are finite and lam, mu lie in [0, 1]).  Pick 0 is position 0; the
 * similarities of the last pick are not computed.  A non-finite squared norm (cosine) or sim raises the flag. */
template <int D>
__global__ __launch_bounds__(256) void diverse_select_kernel(ModelView m, const uint32_t* pool_items, const float* pool_scores, uint32_t pool,
                                                             uint32_t k_out, float lam, int cosine, uint32_t* out_items, float* out_scores,
                                                             uint32_t* nonfinite_flag) {
    constexpr int LD = D + 1;
    constexpr int QPR = D / 4; /* 16-byte pieces per row */
    extern __shared__ float dv_lds[];
    float* qh = dv_lds;
    float* X = qh + D;
    uint32_t* ids = reinterpret_cast<uint32_t*>(X + (size_t)pool * LD);
    float* sc = reinterpret_cast<float*>(ids + pool);
    float* mx = sc + pool;
    float* rn = mx + pool;
    uint32_t* pk = reinterpret_cast<uint32_t*>(rn + pool);
    uint32_t* red = pk + pool;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const size_t u = blockIdx.x;
    if (tid == 0) red[0] = 0;
    __syncthreads();
    uint32_t mine = 0; /* real entries among this thread's positions; the real entries are a prefix of the row */
    for (uint32_t j = tid; j < pool; j += 256) {
        const uint32_t id = pool_items[u * pool + j];
        ids[j] = id;
        sc[j] = pool_scores[u * pool + j];
        pk[j] = 0;
        mine += id != TK_NONE ? 1u : 0u;
    }
    if (mine) atomicAdd(&red[0], mine);
    __syncthreads();
    const uint32_t np = red[0]; /* the pool's size n; red is written again only behind the gather's barrier */
    /* the gather: piece idx = row idx / QPR, quad idx % QPR; four loads in flight per thread */
    const uint32_t pieces = np * QPR;
    for (uint32_t base = 0; base < pieces; base += 4 * 256) {
        float4 ev[4];
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const uint32_t idx = base + it * 256 + tid;
            const uint32_t id = idx < pieces ? ids[idx / QPR] : TK_NONE;
            ev[it] = id < m.num_items ? ld4s(m.E + (size_t)id * D + (idx % QPR) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const uint32_t idx = base + it * 256 + tid;
            if (idx < pieces) {
                float* dst = &X[(size_t)(idx / QPR) * LD + (idx % QPR) * 4];
                dst[0] = ev[it].x; dst[1] = ev[it].y; dst[2] = ev[it].z; dst[3] = ev[it].w;
            }
        }
    }
    __syncthreads();
    bool bad = false;
    for (uint32_t j = tid; j < np; j += 256) {
        float r = 1.0f;
        if (cosine) {
            const float* x = &X[(size_t)j * LD];
            float n2 = 0.0f;
#pragma unroll 8
            for (int k = 0; k < D; ++k) n2 = sbr_fma(x[k], x[k], n2);
            bad |= !(n2 - n2 == 0.0f);
            r = n2 > 0.0f ? 1.0f / __builtin_sqrtf(n2) : 0.0f;
        }
        rn[j] = r;
    }
    const uint32_t picks = k_out < np ? k_out : np;
    const float mu = 1.0f - lam;
    uint32_t a = 0; /* the last pick's position */
    for (uint32_t t = 0; t < picks; ++t) {
        if (t > 0) {
            __syncthreads(); /* rn (first round), pk and the last round's reads of qh and red */
            if (tid < D) qh[tid] = X[(size_t)a * LD + tid] * rn[a];
            __syncthreads();
            float bv = -INFINITY;
            uint32_t bp = TK_NONE;
            for (uint32_t j = tid; j < np; j += 256) {
                if (pk[j]) continue;
                const float* x = &X[(size_t)j * LD];
                float acc = 0.0f;
#pragma unroll 8
                for (int k4 = 0; k4 < D; k4 += 4) {
                    const float4 q = ld4(&qh[k4]);
                    acc = sbr_fma(q.x, x[k4 + 0], acc);
                    acc = sbr_fma(q.y, x[k4 + 1], acc);
                    acc = sbr_fma(q.z, x[k4 + 2], acc);
                    acc = sbr_fma(q.w, x[k4 + 3], acc);
                }
                const float sim = acc * rn[j];
                bad |= !(sim - sim == 0.0f);
                const float mj = t == 1 ? sim : fmaxf(mx[j], sim);
                mx[j] = mj;
                float v = __fsub_rn(__fmul_rn(lam, sc[j]), __fmul_rn(mu, mj));
                if (!(v == v)) v = -INFINITY; /* only behind a non-finite sim, which fails the call: the order stays total */
                if (v > bv || bp == TK_NONE) { bv = v; bp = j; } /* j ascends: an equal value keeps the lower position */
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float ov = __shfl_xor(bv, off, 64);
                const uint32_t op = (uint32_t)__shfl_xor((int)bp, off, 64);
                if (tk_better(ov, op, bv, bp)) { bv = ov; bp = op; }
            }
            if (lane == 0) {
                red[2 * wave] = __float_as_uint(bv);
                red[2 * wave + 1] = bp;
            }
            __syncthreads();
            bv = __uint_as_float(red[0]);
            bp = red[1];
#pragma unroll
            for (int w = 1; w < 4; ++w)
                if (tk_better(__uint_as_float(red[2 * w]), red[2 * w + 1], bv, bp)) { bv = __uint_as_float(red[2 * w]); bp = red[2 * w + 1]; }
            a = bp; /* every thread holds the same winner; it exists: t < picks <= np leaves an unpicked position */
        }
        if (tid == 0) {
            pk[a] = 1;
            out_items[u * k_out + t] = ids[a];
            if (out_scores) out_scores[u * k_out + t] = sc[a];
        }
    }
    for (uint32_t t = picks + tid; t < k_out; t += 256) {
        out_items[u * k_out + t] = TK_NONE;
        if (out_scores) out_scores[u * k_out + t] = -INFINITY;
    }
    if (__any(bad) && lane == 0) atomicOr(nonfinite_flag, 1u);
}

// ------------------------------------------------------------------------------------------------
// recommend_capped: at most `cap` items of one item group among the first k_out kept entries of a user's best `pool`
// ------------------------------------------------------------------------------------------------
/* One workgroup per user.  Its pool is row u of topk_merge_kernel's output at k = pool <= CAP_MAX_POOL: n real entries, best first,
 * then padding.  Static LDS: ids [pool] and grp [pool], the group words gathered from item_groups by id (8 KB at the largest pool).
 * An entry is kept iff its group is CAP_NO_GROUP or fewer than `cap` earlier entries of the row share its group — its ordinal within
 * its group, which depends on no other decision.  Thread tid owns the positions tid, tid + 256, ...: for position j it counts the
 * earlier positions of j's group (every lane of a wave reads the same grp[i]: an LDS broadcast) and stops at cap; the keep flags of
 * its at most CAP_MAX_POOL / 256 positions stay in a register.  The compaction runs in position order, one pass per 256 positions:
 * a ballot and a popcount within the wave, the waves' sums through LDS, a running base across the passes; the first k_out kept
 * entries leave with their pool scores, then the padding, and complete[u] = kept >= k_out || n < pool (the pool held every eligible
 * item).  No global atomics; nothing depends on the dispatch order. */
constexpr uint32_t CAP_NO_GROUP = 0xFFFFFFFFu;
constexpr uint32_t CAP_MAX_POOL = 1024u;
__global__ __launch_bounds__(256) void capped_select_kernel(const uint32_t* item_groups, uint32_t num_items, const uint32_t* pool_items,
                                                            const float* pool_scores, uint32_t pool, uint32_t k_out, uint32_t cap,
                                                            uint32_t* out_items, float* out_scores, uint8_t* out_complete) {
    __shared__ uint32_t ids[CAP_MAX_POOL];
    __shared__ uint32_t grp[CAP_MAX_POOL];
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t real;
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = tid >> 6;
    const size_t u = blockIdx.x;
    if (tid == 0) real = 0;
    __syncthreads();
    uint32_t mine = 0; /* real entries among this thread's positions; the real entries are a prefix of the row */
    for (uint32_t j = tid; j < pool; j += 256) {
        const uint32_t id = pool_items[u * pool + j];
        ids[j] = id;
        grp[j] = id < num_items ? item_groups[id] : CAP_NO_GROUP;
        mine += id != TK_NONE ? 1u : 0u;
    }
    if (mine) atomicAdd(&real, mine);
    __syncthreads();
    const uint32_t np = real; /* the pool's size n */
    uint32_t keep = 0;        /* bit p: position p * 256 + tid is kept */
    for (uint32_t p = 0, j = tid; j < np; ++p, j += 256) {
        const uint32_t g = grp[j];
        uint32_t c = 0;
        if (g != CAP_NO_GROUP)
            for (uint32_t i = 0; i < j && c < cap; ++i) c += grp[i] == g ? 1u : 0u;
        keep |= (c < cap ? 1u : 0u) << p;
    }
    uint32_t base = 0; /* kept entries ahead of the pass: the same in every thread */
    for (uint32_t p = 0; p * 256 < pool; ++p) {
        const uint32_t j = p * 256 + tid;
        const bool kp = (keep >> p) & 1u;
        const uint64_t b = __ballot(kp);
        if (lane == 0) wsum[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t pos = base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        for (uint32_t w = 0; w < wave; ++w) pos += wsum[w];
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (kp && pos < k_out) {
            out_items[u * k_out + pos] = ids[j];
            if (out_scores) out_scores[u * k_out + pos] = pool_scores[u * pool + j];
        }
        __syncthreads(); /* the next pass writes wsum again */
    }
    for (uint32_t t = base + tid; t < k_out; t += 256) {
        out_items[u * k_out + t] = TK_NONE;
        if (out_scores) out_scores[u * k_out + t] = -INFINITY;
    }
    if (tid == 0) out_complete[u] = base >= k_out || np < pool ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// recommend_among: the sub-table of an item set S and the way back from positions in S to catalogue ids
// ------------------------------------------------------------------------------------------------
/* E'[j] = E[S[j]] at storage width and b'[j] = b[S[j]]: one thread per 16-byte quad, so a row's D / 4 threads are neighbours and
 * both the read and the write are whole 4 D-byte runs.  The rows are read once and the copy is what the scan then reads 64 times
 * over: the reads stream, the writes stay plain. */
template <int D>
__global__ __launch_bounds__(256) void subset_gather_kernel(ModelView m, const uint32_t* subset, uint32_t num_subset, float* Es, float* bs) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t j = idx / (D / 4);
    const int c4 = (int)(idx % (D / 4)) * 4;
    if (j >= num_subset) return;
    const uint32_t i = subset[j];
    st4(Es + (size_t)j * D + c4, ld4s(m.E + (size_t)i * D + c4));
    if (c4 == 0) bs[j] = m.b[i];
}

/* items[e] = S[items[e]] for the n entries of the merged rows; the padding id stays what it is.  S is sorted and unique, so the
 * order of positions the scan ranked ties by is the order of ids. */
__global__ __launch_bounds__(256) void subset_ids_kernel(const uint32_t* subset, uint32_t* items, uint64_t n) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const uint32_t p = items[e];
    if (p != TK_NONE) items[e] = subset[p];
}

/* dst[j] = src[S[j]]: an item set's tag or group words, gathered per launch (the words are serving metadata the set does not cache) */
__global__ __launch_bounds__(256) void subset_words_kernel(const uint32_t* subset, uint32_t num_subset, const uint32_t* src, uint32_t* dst) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < num_subset) dst[j] = src[subset[j]];
}

/* An exclusion CSR in catalogue ids -> the same segments in positions of the item set S (sorted, unique), in place.  A segment is
 * what the scans take (the comment above session_seen_lists_kernel): non-decreasing, ids may repeat, a 0xFFFFFFFF tail.  One wave per
 * segment walks it 64 entries at a time: each lane takes the lower bound of its entry in S, the members are kept by a ballot and
 * written to base + popcount(the ballot's bits below the lane), and base advances by the ballot's popcount; when the walk ends
 * 0xFFFFFFFF fills the rest of the segment.  In place is safe: base never passes the block being read, so a block's writes land
 * below the next block's reads, and every lane's entry of the block is loaded before the ballot — which every store follows — is
 * known.  The result is non-decreasing in positions, repeats preserved, entries outside S gone; the segment pointers do not change. */
__global__ __launch_bounds__(256) void subset_positions_kernel(const uint32_t* subset, uint32_t num_subset, const uint64_t* eptr, uint32_t n,
                                                               uint32_t* excl) {
    const uint32_t seg = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (seg >= n) return; /* the whole wave */
    const uint64_t e0 = eptr[seg], e1 = eptr[seg + 1];
    uint64_t base = e0;
    for (uint64_t b0 = e0; b0 < e1; b0 += 64) {
        const uint64_t e = b0 + lane;
        const uint32_t id = e < e1 ? excl[e] : TK_NONE;
        uint32_t lo = 0, hi = num_subset;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (subset[mid] < id) lo = mid + 1; else hi = mid;
        }
        const bool member = id != TK_NONE && lo < num_subset && subset[lo] == id;
        const uint64_t kept = __ballot(member);
        if (member) excl[base + (uint64_t)__popcll(kept & ((1ull << lane) - 1ull))] = lo;
        base += (uint64_t)__popcll(kept);
    }
    for (uint64_t e = base + lane; e < e1; e += 64) excl[e] = TK_NONE;
}

// ------------------------------------------------------------------------------------------------
// score_candidates: b[i] + chain_dot(rep_u, E[i]) of a flat list of (user, item) pairs
// ------------------------------------------------------------------------------------------------
/* A wave owns 64 consecutive pairs, lane l the pair p0 + l: its item row comes through the wave's own LDS block CH columns at a time
 * (item_rnorm_kernel's layout: rows CH + 1 floats apart, a lane reads its row's column from its own bank), so the global loads are
 * CH / 4 neighbouring lanes per 4 CH-byte piece of a row, not 64 lanes at a stride of 4 D bytes; every piece of a row is read once
 * by the launch, so the loads stream (score_kernel's policy for its one-touch rows).  The lane then runs predict's chain — k
 * ascending from +0.0, one sbr_fma per column — against its user's representation row rep[pair_row[p]], which neighbouring pairs of
 * one user share (a broadcast, and cache-resident), and adds the bias.  No workgroup barrier: the four waves of a workgroup
 * share nothing.  Lanes past the last pair gather row 0 and store nothing. */
template <int D>
__global__ __launch_bounds__(256) void candidate_score_kernel(ModelView m, const float* reps, const uint32_t* pair_row, const uint32_t* pair_item,
                                                              uint64_t num_pairs, float* out, uint32_t* nonfinite_flag) {
    constexpr int CH = D < 32 ? D : 32;
    constexpr int LD = CH + 1;
    constexpr int ITER = CH / 4; /* float4 loads per lane and column block: 64 rows x CH / 4 quads over 64 lanes */
    __shared__ float Xs[4][64 * LD];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float* X = Xs[wave];
    const uint64_t p = ((uint64_t)blockIdx.x * 4 + wave) * 64 + lane;
    const bool real = p < num_pairs;
    const uint32_t item = real ? pair_item[p] : 0u;
    const float* h = reps + (size_t)(real ? pair_row[p] : 0u) * D;
    float acc = 0.0f;
    float4 ev[ITER];
    auto fetch = [&](int c0) { /* the wave's 64 rows' columns [c0, c0 + CH): quad idx % (CH / 4) of row idx / (CH / 4) */
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int idx = lane + it * 64;
            const uint32_t ri = (uint32_t)__shfl((int)item, idx / (CH / 4), 64);
            ev[it] = ld4s(m.E + (size_t)ri * D + c0 + (idx % (CH / 4)) * 4);
        }
    };
    fetch(0);
    /* not unrolled: unrolled, the compiler hoists every block's loads to the top — 264 VGPRs at d = 128, spills at d = 256 */
#pragma unroll 1
    for (int c0 = 0; c0 < D; c0 += CH) {
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int idx = lane + it * 64;
            float* dst = &X[(idx / (CH / 4)) * LD + (idx % (CH / 4)) * 4];
            dst[0] = ev[it].x; dst[1] = ev[it].y; dst[2] = ev[it].z; dst[3] = ev[it].w;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (c0 + CH < D) fetch(c0 + CH); /* the next block is in flight under this block's chain */
#pragma unroll
        for (int k4 = 0; k4 < CH; k4 += 4) {
            const float4 hv = ld4(h + c0 + k4);
            acc = sbr_fma(hv.x, X[lane * LD + k4 + 0], acc);
            acc = sbr_fma(hv.y, X[lane * LD + k4 + 1], acc);
            acc = sbr_fma(hv.z, X[lane * LD + k4 + 2], acc);
            acc = sbr_fma(hv.w, X[lane * LD + k4 + 3], acc);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    bool bad = false;
    if (real) {
        const float sc = m.b[item] + acc;
        bad = !(sc - sc == 0.0f);
        out[p] = sc;
    }
    if (__any(bad) && lane == 0) atomicOr(nonfinite_flag, 1u);
}

// ------------------------------------------------------------------------------------------------
// recommend_sampled: the rows' noise keys ahead of the scan (topk_gemm_kernel<D, GumbelBias>), the plain scores behind the merge
// ------------------------------------------------------------------------------------------------
/* K[u] of the launch's scan rows from the call's seed and the rows' streams (sbr_numerics.h): a function of (seed, stream) alone,
 * so neither the host's chunks nor the item ranges can change a row's noise. */
__global__ __launch_bounds__(256) void sample_keys_kernel(uint64_t seed, const uint64_t* streams, uint32_t n, uint64_t* keys) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u < n) keys[u] = sbr_sample_row_key(seed, streams[u]);
}

/* The merged rows as candidate_score_kernel's pairs: entry j of row u -> (rep_row[u], items[u][j]).  A padding entry stands in with
 * the row's first item, or item 0 in a row of padding — a pair the scan has scored, so the flag says nothing new — and
 * sample_pad_kernel gives it its -inf afterwards. */
__global__ __launch_bounds__(256) void sample_pairs_kernel(const int* rep_row, const uint32_t* items, uint32_t n, uint32_t k, uint32_t* pair_row,
                                                           uint32_t* pair_item) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (uint64_t)n * k) return;
    const uint64_t u = p / k;
    uint32_t i = items[p];
    if (i == TK_NONE) i = items[u * k];
    pair_row[p] = (uint32_t)rep_row[u];
    pair_item[p] = i == TK_NONE ? 0u : i;
}

__global__ __launch_bounds__(256) void sample_pad_kernel(const uint32_t* items, uint64_t n, float* scores) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n && items[p] == TK_NONE) scores[p] = -INFINITY;
}

// ------------------------------------------------------------------------------------------------
// log_partition: the exact fixed-point mass of softmax(score / T) per row — the k = 1 scan (topk_gemm_kernel<D, BiasAdd>) for the
// shift, a second catalogue scan with a summing epilogue, and the exclusion lists' correction
// ------------------------------------------------------------------------------------------------
/* shift[u] = fl(best score * inv_t) of the k = 1 scan's merged rows — the largest t of the row, because a product with a positive
 * inv_t is monotone — or -inf for a row of padding (nothing allowed); a zero shift is +0.0 whatever the sign of the best score's
 * zero.  mass[u] = 0 ahead of the scan's atomics. */
__global__ __launch_bounds__(256) void partition_shift_kernel(const uint32_t* best_item, const float* best_score, uint32_t n, float inv_t,
                                                              float* shift, unsigned long long* mass) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u >= n) return;
    shift[u] = best_item[u] == TK_NONE ? -INFINITY : __fadd_rn(__fmul_rn(best_score[u], inv_t), 0.0f);
    mass[u] = 0ull;
}

/* partition_shift_kernel's statement on column 0 of a k-row scan's output [n][k] (launch_topk_partition) */
__global__ __launch_bounds__(256) void partition_shift_strided_kernel(const uint32_t* items, const float* scores, uint32_t n, uint32_t k,
                                                                      float inv_t, float* shift, unsigned long long* mass) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u >= n) return;
    const size_t e = (size_t)u * k;
    shift[u] = items[e] == TK_NONE ? -INFINITY : __fadd_rn(__fmul_rn(scores[e], inv_t), 0.0f);
    mass[u] = 0ull;
}

/* The sum scan, rank_gemm_kernel's shape: every score of the workgroup's 128 users x its item range becomes t = fl(s * inv_t),
 * d = fl(t - shift[u]) and the integer weight w (sbr_softmax_weight), added into 16 64-bit per-lane accumulators; at the end of the
 * range the 32 item lanes of a half-wave are summed and one 64-bit atomic per user joins the other ranges'.  Integer addition is
 * associative: lanes, ranges and the host's chunks cannot change a bit of the sum.  The rows' shifts sit in LDS by slot (slot_user);
 * a row that does not exist, or that may see nothing, has shift -inf, so d = +inf and w = 0.  The exclusion lists are NOT searched
 * here: an excluded item that passes the tag test and has d <= 0 is added, and partition_finish_kernel subtracts exactly that.
 * With TagFilter the lane's item is tested against its 16 users' masks as in topk_gemm_kernel.  The non-finite test is on t and sees
 * every scanned pair of an existing row, allowed or not.  The skip of the polynomial is per tile and per wave, not per register:
 * a tile none of whose 64 x 16 scores weighs anything for the wave (every d below -64: a trained model at a small T) costs no
 * exp32; once one lane has one live score, all 16 registers of every lane run it, the dead ones on d = 0 and masked out of the add. */
template <int D, class Filter>
__global__ __launch_bounds__(256, D <= 128 ? 2 : 1) void partition_gemm_kernel(ModelView m, const float* reps, const int* rep_row, uint32_t num_users,
                                                                              const float* shift, float inv_t, uint32_t frac_bits,
                                                                              uint32_t items_per_group, unsigned long long* mass,
                                                                              uint32_t* nonfinite_flag, typename Filter::Args fa) {
    __shared__ float Es[2][32 * ItemTiles<D>::LDE];
    __shared__ float Bs[2][32];
    __shared__ __align__(16) float shS[128]; /* shifts by slot (slot_user) */
    __shared__ uint32_t Ts[2][Filter::on ? 32 : 1];
    __shared__ __align__(16) uint32_t anyS[Filter::on ? 128 : 4];
    __shared__ __align__(16) uint32_t anyZ[Filter::on ? 128 : 4]; /* 1 where the user's any_of is 0 (every tag passes it), else 0 */
    __shared__ __align__(16) uint32_t noneS[Filter::on ? 128 : 4];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int hh = lane >> 5;
    const uint32_t u0 = blockIdx.x * 128 + wave * 32;
    float a[D / 2];
    load_user_fragments<D>(a, reps, rep_row, num_users, u0);
    if (tid < 128) {
        const uint32_t u = blockIdx.x * 128 + (uint32_t)slot_user(tid);
        shS[tid] = u < num_users ? shift[u] : -INFINITY;
        if constexpr (Filter::on) {
            const uint32_t any = u < num_users ? fa.any_of[u] : 0u;
            anyS[tid] = any;
            anyZ[tid] = any == 0u ? 1u : 0u;
            noneS[tid] = u < num_users ? fa.none_of[u] : 0u;
        }
    }
    uint32_t umask = 0; /* accumulator registers q whose user exists */
#pragma unroll
    for (int q = 0; q < 16; ++q)
        if (acc_user(u0, q, hh) < num_users) umask |= 1u << q;
    uint64_t sum[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) sum[q] = 0ull;
    bool bad = false;
    ItemTiles<D> tiles(m, items_per_group);
    const int ntiles = tiles.ntiles;
    if (ntiles > 0) {
        tiles.fetch(m, 0);
        tiles.stage(Es[0], Bs[0]);
        if constexpr (Filter::on) {
            tiles.fetch_tags(fa.tags, 0);
            tiles.stage_tags(Ts[0]);
        }
    }
    __syncthreads();
    const int pbase = wave * 32 + hh * 16;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < ntiles) {
            tiles.fetch(m, tile + 1);
            if constexpr (Filter::on) tiles.fetch_tags(fa.tags, tile + 1);
        }
        const f32x16 acc = tile_dots<D>(a, Es[buf]);
        const float bias = Bs[buf][l31];
        const bool item_ok = tiles.i_begin + (uint32_t)tile * 32 + (uint32_t)l31 < tiles.i_end;
        uint32_t live = item_ok ? umask : 0u; /* accumulator registers q whose score may weigh something */
        float dq[16];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const float4 s4 = ld4(&shS[pbase + 4 * q4]);
            const float sh[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = 4 * q4 + j;
                const float t = __fmul_rn(bias + acc[q], inv_t);
                if (((live >> q) & 1u) && !(t - t == 0.0f)) bad = true;
                const float d = __fsub_rn(t, sh[j]);
                dq[q] = d;
                if (!(d <= 0.0f && d >= SBR_SOFTMAX_D_MIN)) live &= ~(1u << q);
            }
        }
        if constexpr (Filter::on) { /* the lane's item against its 16 users' masks, as topk_gemm_kernel's */
            const uint32_t tag = Ts[buf][l31];
            uint32_t drop = 0;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const uint4 a4 = *reinterpret_cast<const uint4*>(&anyS[pbase + 4 * q4]);
                const uint4 z4 = *reinterpret_cast<const uint4*>(&anyZ[pbase + 4 * q4]);
                const uint4 n4 = *reinterpret_cast<const uint4*>(&noneS[pbase + 4 * q4]);
                const uint32_t any[4] = {a4.x, a4.y, a4.z, a4.w};
                const uint32_t anyz[4] = {z4.x, z4.y, z4.z, z4.w};
                const uint32_t none[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t hit = (tag & none[j]) != 0u ? 1u : 0u;
                    const uint32_t miss = ((tag & any[j]) | anyz[j]) == 0u ? 1u : 0u;
                    drop |= (hit | miss) << (4 * q4 + j);
                }
            }
            live &= ~drop;
        }
        if (__any(live != 0u)) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const uint64_t w = sbr_fix(sbr_exp32(((live >> q) & 1u) ? dq[q] : 0.0f), frac_bits);
                sum[q] += ((live >> q) & 1u) ? w : 0ull;
            }
        }
        if (tile + 1 < ntiles) {
            tiles.stage(Es[buf ^ 1], Bs[buf ^ 1]);
            if constexpr (Filter::on) tiles.stage_tags(Ts[buf ^ 1]);
        }
        __syncthreads();
    }
    // per-user totals: sum over the 32 item lanes of each half-wave, the two halves of the 64-bit sum apart (the carry is added back)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        uint64_t c = sum[q];
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)c, off, 64);
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(c >> 32), off, 64);
            c += ((uint64_t)hi << 32) | lo;
        }
        const uint32_t u = acc_user(u0, q, hh);
        if (l31 == 0 && u < num_users && c) atomicAdd(&mass[u], (unsigned long long)c);
    }
    if (__any(bad) && lane == 0) atomicOr(nonfinite_flag, 1u);
}

/* One wave per row, as rank_history_kernel: every distinct entry of the row's ascending exclusion list (repeats and the 0xFFFFFFFF
 * padding of a session's list skipped) is scored again with the scan's functions, and its weight leaves the mass if the scan added
 * it — the item passes the row's tag test and d <= 0 (sbr_softmax_weight is zero otherwise: an excluded item that outscores every
 * allowed one was never added).  Integer subtraction of what was added: exact. */
template <int D>
__global__ __launch_bounds__(64) void partition_finish_kernel(ModelView m, const float* reps, const int* rep_row, const float* shift, float inv_t,
                                                              uint32_t frac_bits, const uint64_t* excl_ptr, const uint32_t* excl_items,
                                                              const uint32_t* tags, const uint32_t* any_of, const uint32_t* none_of,
                                                              unsigned long long* mass) {
    const int u = blockIdx.x;
    const float* h = reps + (size_t)rep_row[u] * D;
    const float sh = shift[u];
    const uint32_t any = tags ? any_of[u] : 0u, none = tags ? none_of[u] : 0u;
    const uint64_t e0 = excl_ptr[u], e1 = excl_ptr[u + 1];
    uint64_t sub = 0;
    for (uint64_t e = e0 + threadIdx.x; e < e1; e += 64) {
        const uint32_t i = excl_items[e];
        if (i >= m.num_items || (e > e0 && excl_items[e - 1] == i)) continue;
        if (tags) {
            const uint32_t tag = tags[i];
            if ((tag & none) != 0u || (any != 0u && (tag & any) == 0u)) continue;
        }
        const float s = m.b[i] + chain_dot<D>(h, m.E + (size_t)i * D);
        sub += sbr_softmax_weight(__fmul_rn(s, inv_t), sh, frac_bits);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)sub, off, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(sub >> 32), off, 64);
        sub += ((uint64_t)hi << 32) | lo;
    }
    if (threadIdx.x == 0 && sub) atomicAdd(&mass[u], (unsigned long long)(0ull - sub)); /* two's complement: subtracts */
}

/* sequence_partition's masked shift.  A scan row is (sequence b, step t) of the forward pass's packed layout, as in
 * rank_prefix_kernel: it may see every item that is not one of its inputs x_0 .. x_t.  The top-k scan ran over the row WITHOUT an
 * exclusion list and left its k best (score desc; padding 0xFFFFFFFF / -inf behind them) in pool_items / pool_scores [n][k]; the
 * first entry that is no prefix item is the row's best eligible item, and shift = fl(its score * inv_t) + 0.0f is
 * partition_shift_kernel's statement.  Padding before such an entry: the pool held the whole catalogue and all of it is in the
 * prefix, nothing is eligible, shift = -inf.  All k entries prefix items: the row is flagged in `unresolved` and the host has the
 * k = 1 scan decide it with the row's exclusion list (launch_sequence_shift_rows); its shift is -inf until then.
 * One wave per row.  The pool is walked 64 entries at a time, lane l holding entry e0 + l; the prefix items are loaded lane by lane
 * from the packed in_idx rows off[j] + b, 64 at a time, and each is broadcast to the wave and compared with the lane's entry.  The
 * lowest lane that holds padding or an eligible entry decides.  mass[row] = 0 ahead of the sum scan's atomics. */
__global__ __launch_bounds__(256) void sequence_shift_kernel(const uint32_t* pool_items, const float* pool_scores, uint32_t k,
                                                              const uint2* unit_bt, uint32_t num_units, const int* off,
                                                              const uint32_t* in_idx, float inv_t, float* shift, unsigned long long* mass,
                                                              uint8_t* unresolved) {
    const uint32_t unit = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= num_units) return; /* the whole wave */
    const uint32_t lane = threadIdx.x & 63;
    const uint2 bt = unit_bt[unit]; /* (b, t) */
    const uint32_t np = bt.y + 1;   /* prefix items */
    float sh = -INFINITY;
    uint32_t open = 1; /* no entry has decided the row yet */
    for (uint32_t e0 = 0; e0 < k && open; e0 += 64) {
        const uint32_t e = e0 + lane;
        const uint32_t item = e < k ? pool_items[(size_t)unit * k + e] : TK_NONE;
        bool hit = false;
        for (uint32_t j0 = 0; j0 < np; j0 += 64) {
            const uint32_t j = j0 + lane;
            const uint32_t x = j < np ? in_idx[(uint32_t)off[j] + bt.x] : TK_NONE;
            const uint32_t nj = np - j0 < 64u ? np - j0 : 64u;
            for (uint32_t jj = 0; jj < nj; ++jj) hit |= (uint32_t)__shfl((int)x, (int)jj, 64) == item;
        }
        const bool pad = item == TK_NONE; /* also the lanes past k: reached only when no entry before them decided */
        const unsigned long long decides = __ballot(pad || !hit);
        if (decides) {
            const int f = __ffsll((long long)decides) - 1;
            const uint32_t fe = e0 + (uint32_t)f;
            const uint32_t fitem = (uint32_t)__shfl((int)item, f, 64);
            if (fe < k) {
                open = 0;
                if (fitem != TK_NONE) sh = __fadd_rn(__fmul_rn(pool_scores[(size_t)unit * k + fe], inv_t), 0.0f);
            }
        }
    }
    if (lane == 0) {
        shift[unit] = sh;
        mass[unit] = 0ull;
        unresolved[unit] = open ? 1 : 0;
    }
}

/* the shifts of the rows the pool left unresolved, out of the k = 1 scan over them alone: row i of that scan is row rows[i] of the
 * call's launch; partition_shift_kernel's statement */
__global__ __launch_bounds__(256) void sequence_shift_rows_kernel(const uint32_t* best_item, const float* best_score, uint32_t n, float inv_t,
                                                                   const uint32_t* rows, float* shift) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    shift[rows[i]] = best_item[i] == TK_NONE ? -INFINITY : __fadd_rn(__fmul_rn(best_score[i], inv_t), 0.0f);
}

/* sequence_partition's prefix correction, in the shape of rank_prefix_kernel (one wave per scan row (b, t), lane l the inputs
 * j = l, l + 64, ... <= t, first occurrences only, item rows through L2 for the reason given there): the sum scan added every item
 * with d <= 0, the row's own prefix items among them, and this is partition_finish_kernel's subtraction of exactly those weights —
 * sbr_softmax_weight is zero where d > 0, so a prefix item that outscores the shift was never added.  The row's mass belongs to this
 * wave and the scan's atomics have finished in stream order: a plain read and write.  unit_bt NULL: nothing is masked and nothing
 * subtracted.  Lane 63, the one with the fewest inputs, scores the row's target with predict's statement. */
template <int D>
__global__ __launch_bounds__(256) void partition_prefix_kernel(ModelView m, const float* reps, const int* rep_row, const float* shift,
                                                                float inv_t, uint32_t frac_bits, const uint2* unit_bt, uint32_t num_units,
                                                                const int* off, const uint32_t* in_idx, const uint32_t* first_occ,
                                                                const uint32_t* target, unsigned long long* mass, float* scores) {
    const uint32_t unit = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= num_units) return; /* the whole wave */
    const uint32_t lane = threadIdx.x & 63;
    const float* h = reps + (size_t)rep_row[unit] * D;
    if (lane == 63) {
        const uint32_t i = target[unit];
        scores[unit] = m.b[i] + chain_dot<D>(h, m.E + (size_t)i * D);
    }
    if (!unit_bt) return;
    const uint2 bt = unit_bt[unit]; /* (b, t) */
    const float sh = shift[unit];
    uint64_t sub = 0;
    for (uint32_t j = lane; j <= bt.y; j += 64) {
        const uint32_t r = (uint32_t)off[j] + bt.x;
        if (!first_occ[r]) continue;
        const uint32_t i = in_idx[r];
        const float s = m.b[i] + chain_dot<D>(h, m.E + (size_t)i * D);
        sub += sbr_softmax_weight(__fmul_rn(s, inv_t), sh, frac_bits);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)sub, o, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(sub >> 32), o, 64);
        sub += ((uint64_t)hi << 32) | lo;
    }
    if (lane == 0 && sub) mass[unit] -= (unsigned long long)sub;
}

// ------------------------------------------------------------------------------------------------
// recommend_above / audience_above: every scanned column at or over a per-row score — the catalogue scan with an epilogue that
// counts, then (a second launch) writes
// ------------------------------------------------------------------------------------------------
/* partition_gemm_kernel's shape: 128 rows per workgroup, grid (row tiles, item ranges).  The rows' thresholds sit in LDS by slot
 * (slot_user; +inf for a row that does not exist: nothing passes), their exclusion segments' bounds beside them.  `passes` is the one
 * statement of what a tile contributes, used by both modes — the fill is only correct if it passes exactly what the count passed:
 *   1. the non-finite test on every scanned score of an existing row (it fails the call, as in topk_gemm_kernel);
 *   2. score >= threshold, the f32 compare (-0.0 >= +0.0 holds; the host refuses a NaN threshold);
 *   3. the tag test (TagFilter, as topk_gemm_kernel's);
 *   4. only for survivors, the binary search of the row's non-decreasing exclusion segment, as merge_staged does it.
 * Fill = false: 16 per-lane counters; at the range's end the 32 item lanes of a half-wave are summed and ONE value is stored to
 *   counts[row * G + range], a slot only this workgroup owns — no atomics, nothing to zero.
 * Fill = true: accumulator register q has a cursor that belongs to its half-wave alone and starts at offsets[row * G + range] (less
 *   the launch's base, offsets[0]: a launch writes fewer than 2^32 entries).  Per tile, for each q with a survivor, the half-wave's
 *   32 ballot bits place a passing lane at cursor + popcount(bits below it) and advance the cursor by their popcount.  Tiles ascend
 *   within a range and a row's ranges own consecutive slots, so a row's entries ascend by column whatever order the workgroups run
 *   in.  The cursors live in LDS by slot, each read by its half-wave's 32 lanes and then advanced by its lane 0: held in 16 registers
 *   per lane through the unrolled writes they took the d = 128 kernel to 256 VGPRs and 84 bytes of scratch, in LDS it needs 170 and
 *   none.  Every write is checked against the slot's end (offsets[row * G + range + 1], and the buffer's size): a pass beyond it is
 *   dropped and raises *overrun_flag — a disagreement between the two launches becomes an error, never a store out of bounds.
 * KEEP IN STEP: select_gemm_kernel below restates this kernel's prologue and stages 1, 3 and 4 of `passes` (the staging, the tag
 *   test, the exclusion search); recommend_top is only exact if the select and this count / fill pass the same columns, so a
 *   change to one of those stages here is made there as well (tests/test_top_gpu.py holds the two against each other). */
template <int D, class Score, class Filter, bool Fill>
__global__ __launch_bounds__(256, D <= 128 ? 2 : 1) void above_gemm_kernel(ModelView m, const float* reps, const int* rep_row, uint32_t num_users,
                                                                          const float* thresholds, const uint64_t* excl_ptr,
                                                                          const uint32_t* excl_items, uint32_t items_per_group, uint32_t* counts,
                                                                          const uint64_t* offsets, uint32_t* out_ids, float* out_scores,
                                                                          uint32_t out_cap, uint32_t* overrun_flag, uint32_t* nonfinite_flag,
                                                                          typename Filter::Args fa, typename Score::Args sa) {
    __shared__ float Es[2][32 * ItemTiles<D>::LDE];
    __shared__ float Bs[2][32];
    __shared__ __align__(16) float qbS[Score::query ? 128 : 4]; /* QueryBias only: the queries' biases by slot (slot_user) */
    __shared__ uint32_t Ts[2][Filter::on ? 32 : 1];
    __shared__ __align__(16) uint32_t anyS[Filter::on ? 128 : 4];
    __shared__ __align__(16) uint32_t anyZ[Filter::on ? 128 : 4]; /* 1 where the user's any_of is 0 (every tag passes it), else 0 */
    __shared__ __align__(16) uint32_t noneS[Filter::on ? 128 : 4];
    // per-row state by slot (slot_user)
    __shared__ __align__(16) float thS[128];
    __shared__ uint64_t exLo[128]; /* the row's exclusion segment [exLo, exHi) of excl_items; empty without lists */
    __shared__ uint64_t exHi[128];
    __shared__ __align__(16) uint32_t endS[Fill ? 128 : 4]; /* Fill: the end of the row's slot for this range, relative to the launch's base ... */
    __shared__ __align__(16) uint32_t curS[Fill ? 128 : 4]; /* ... and its cursor, which only the slot's own half-wave reads and advances */
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int hh = lane >> 5;
    const uint32_t G = gridDim.y;
    const uint32_t u0 = blockIdx.x * 128 + wave * 32;
    float a[D / 2];
    load_user_fragments<D>(a, reps, rep_row, num_users, u0);
    if (tid < 128) {
        const uint32_t u = blockIdx.x * 128 + (uint32_t)slot_user(tid);
        const bool real = u < num_users;
        thS[tid] = real ? thresholds[u] : INFINITY;
        exLo[tid] = real && excl_ptr ? excl_ptr[u] : 0ull;
        exHi[tid] = real && excl_ptr ? excl_ptr[u + 1] : 0ull;
        if constexpr (Fill) {
            uint64_t e = real ? offsets[(size_t)u * G + blockIdx.y + 1] - offsets[0] : 0ull;
            if (e > (uint64_t)out_cap) e = out_cap;
            endS[tid] = (uint32_t)e;
            const uint64_t c = real ? offsets[(size_t)u * G + blockIdx.y] - offsets[0] : 0ull;
            curS[tid] = c < 0xFFFFFFFFull ? (uint32_t)c : 0xFFFFFFFFu;
        }
        if constexpr (Filter::on) {
            const uint32_t any = real ? fa.any_of[u] : 0u;
            anyS[tid] = any;
            anyZ[tid] = any == 0u ? 1u : 0u;
            noneS[tid] = real ? fa.none_of[u] : 0u;
        }
        if constexpr (Score::query) qbS[tid] = real ? sa.qb[rep_row[u]] : 0.0f;
    }
    uint32_t umask = 0; /* accumulator registers q whose user exists */
#pragma unroll
    for (int q = 0; q < 16; ++q)
        if (acc_user(u0, q, hh) < num_users) umask |= 1u << q;
    uint32_t cnt[Fill ? 1 : 16]; /* Fill = false: the lane's counts */
#pragma unroll
    for (int q = 0; q < (Fill ? 1 : 16); ++q) cnt[q] = 0u;
    bool bad = false, over = false;
    ItemTiles<D> tiles(m, items_per_group);
    const int ntiles = tiles.ntiles;
    if (ntiles > 0) {
        tiles.fetch(m, 0);
        tiles.stage(Es[0], Bs[0]);
        if constexpr (Filter::on) {
            tiles.fetch_tags(fa.tags, 0);
            tiles.stage_tags(Ts[0]);
        }
    }
    __syncthreads();
    const int pbase = wave * 32 + hh * 16;
    /* the accumulator registers q of this lane's column `id` that pass their rows: THE pass predicate of both modes */
    auto passes = [&](const f32x16& acc, float bias, uint32_t id, int buf) -> uint32_t {
        uint32_t pend = id < tiles.i_end ? umask : 0u;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const float4 t4 = ld4(&thS[pbase + 4 * q4]);
            const float tq[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = 4 * q4 + j;
                const float sc = TK_SCORE(q);
                if (((pend >> q) & 1u) && !(sc - sc == 0.0f)) bad = true;
                if (!(sc >= tq[j])) pend &= ~(1u << q); /* a non-finite score passes nothing it should not: the call fails */
            }
        }
        if constexpr (Filter::on) { /* the lane's item against its 16 users' masks, as topk_gemm_kernel's */
            const uint32_t tag = Ts[buf][l31];
            uint32_t drop = 0;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const uint4 a4 = *reinterpret_cast<const uint4*>(&anyS[pbase + 4 * q4]);
                const uint4 z4 = *reinterpret_cast<const uint4*>(&anyZ[pbase + 4 * q4]);
                const uint4 n4 = *reinterpret_cast<const uint4*>(&noneS[pbase + 4 * q4]);
                const uint32_t any[4] = {a4.x, a4.y, a4.z, a4.w};
                const uint32_t anyz[4] = {z4.x, z4.y, z4.z, z4.w};
                const uint32_t none[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t hit = (tag & none[j]) != 0u ? 1u : 0u;
                    const uint32_t miss = ((tag & any[j]) | anyz[j]) == 0u ? 1u : 0u;
                    drop |= (hit | miss) << (4 * q4 + j);
                }
            }
            pend &= ~drop;
        }
        if (excl_ptr) { /* the survivors against their rows' lists: few where the threshold is selective */
            for (uint32_t rem = pend; rem; rem &= rem - 1u) {
                const int q = __ffs((int)rem) - 1;
                uint64_t lo = exLo[pbase + q];
                const uint64_t e1 = exHi[pbase + q];
                uint64_t hi = e1;
                while (lo < hi) {
                    const uint64_t mid = (lo + hi) >> 1;
                    if (excl_items[mid] < id) lo = mid + 1; else hi = mid;
                }
                if (lo < e1 && excl_items[lo] == id) pend &= ~(1u << q);
            }
        }
        return pend;
    };
    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < ntiles) {
            tiles.fetch(m, tile + 1);
            if constexpr (Filter::on) tiles.fetch_tags(fa.tags, tile + 1);
        }
        f32x16 acc = tile_dots<D>(a, Es[buf]);
        const float bias = Bs[buf][l31];
        if constexpr (Score::query) { /* the score is b[q] + dot, one rounding, as predict's; acc[q] holds it from here on */
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 b4 = ld4(&qbS[pbase + 4 * q4]);
                acc[4 * q4 + 0] = b4.x + acc[4 * q4 + 0];
                acc[4 * q4 + 1] = b4.y + acc[4 * q4 + 1];
                acc[4 * q4 + 2] = b4.z + acc[4 * q4 + 2];
                acc[4 * q4 + 3] = b4.w + acc[4 * q4 + 3];
            }
        }
        const uint32_t id = tiles.i_begin + (uint32_t)tile * 32 + (uint32_t)l31;
        const uint32_t pend = passes(acc, bias, id, buf);
        if constexpr (!Fill) {
#pragma unroll
            for (int q = 0; q < 16; ++q) cnt[q] += (pend >> q) & 1u;
        } else {
            if (__any(pend != 0u)) {
                /* four rows at a time: their cursors and ends in two 16-byte reads, the writes, the cursors back in one 16-byte
                 * write by the half-wave's lane 0.  One wave's LDS accesses complete in program order, so every lane has its
                 * cursors before lane 0 advances them; the fence below orders the tile's updates ahead of the next tile's reads. */
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    if (__ballot(((pend >> (4 * q4)) & 0xFu) != 0u) == 0ull) continue; /* wave-uniform */
                    const uint4 c4 = *reinterpret_cast<const uint4*>(&curS[pbase + 4 * q4]);
                    const uint4 e4 = *reinterpret_cast<const uint4*>(&endS[pbase + 4 * q4]);
                    uint32_t c[4] = {c4.x, c4.y, c4.z, c4.w};
                    const uint32_t e[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int q = 4 * q4 + j;
                        const bool p = ((pend >> q) & 1u) != 0u;
                        const uint64_t b = __ballot(p);
                        const uint32_t bits = hh ? (uint32_t)(b >> 32) : (uint32_t)b;
                        if (p) {
                            const uint64_t pos = (uint64_t)c[j] + (uint32_t)__popc(bits & ((1u << l31) - 1u));
                            if (pos < (uint64_t)e[j]) {
                                out_ids[pos] = id;
                                if (out_scores) out_scores[pos] = TK_SCORE(q);
                            } else
                                over = true;
                        }
                        const uint32_t adv = (uint32_t)__popc(bits);
                        c[j] = c[j] > 0xFFFFFFFFu - adv ? 0xFFFFFFFFu : c[j] + adv;
                    }
                    if (l31 == 0) *reinterpret_cast<uint4*>(&curS[pbase + 4 * q4]) = make_uint4(c[0], c[1], c[2], c[3]);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
        if (tile + 1 < ntiles) {
            tiles.stage(Es[buf ^ 1], Bs[buf ^ 1]);
            if constexpr (Filter::on) tiles.stage_tags(Ts[buf ^ 1]);
        }
        __syncthreads();
    }
    if constexpr (!Fill) {
        // per-row counts of the range: sum over the 32 item lanes of each half-wave, one plain store per (row, range)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            int c = (int)cnt[q];
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
            const uint32_t u = acc_user(u0, q, hh);
            if (l31 == 0 && u < num_users) counts[(size_t)u * G + blockIdx.y] = (uint32_t)c;
        }
    } else {
        if (__any(over) && lane == 0) atomicOr(overrun_flag, 1u);
    }
    if (__any(bad) && lane == 0) atomicOr(nonfinite_flag, 1u);
}

// ------------------------------------------------------------------------------------------------
// recommend_top / audience_top: the n-th largest eligible score of a row — a radix select over scores that are never written, one
// catalogue scan per 4-bit digit of the key, top digit first; above_gemm_kernel then runs at the cut and top_trim_kernel keeps n
// ------------------------------------------------------------------------------------------------
/* the monotone u32 of a score's f32 bits: a < b as floats <=> key(a) < key(b); -0.0 and +0.0 share +0.0's key */
__device__ __forceinline__ uint32_t select_key(float sc) {
    const uint32_t b = sc == 0.0f ? 0u : __float_as_uint(sc);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float select_unkey(uint32_t key) { return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key); }

/* One round of the select, in above_gemm_kernel's shape (128 rows per workgroup, grid (row tiles, item ranges)) and with its pass
 * predicate, the threshold compare replaced by the row's active interval: the keys whose decided bits (mask[u]) equal prefix[u].
 * A row that is decided (n = 0, or fewer eligible columns than n) has mask = 0 and prefix = 1, which no key meets.  Order as above:
 *   1. the non-finite test on every scanned score of an existing row;
 *   2. (key & mask) == prefix — everything in round 0, what shares the decided digits after it;
 *   3. the tag test;
 *   4. only for survivors, the binary search of the row's exclusion segment.
 * KEEP IN STEP: the prologue and stages 1, 3 and 4 are above_gemm_kernel's, restated here as a separate template so that its
 * instantiations keep their code; the count and fill that follow the select must pass exactly the columns it binned, so a change
 * to one of those stages is made in both kernels.
 * A survivor is binned by its digit (key >> shift) & 15 into hist[slot][16] in LDS.  Slot p = wave * 32 + hh * 16 + q belongs to
 * one half-wave alone, so the bins need no atomics: per q the half-waves agree on a digit (the first pending lane's), ballot the
 * lanes that hold it, and their lane 0 adds the popcount with a plain read and write: one turn per distinct digit among the
 * pending lanes.  A model's scores share their sign and most of their exponent, so rounds 0 to 2 bin nearly every score (2 to
 * 2.7 count scans each at 8 192 x 1e6, d = 128) and survivors are rare only from round 4 on, where the block is skipped under
 * __any and a round costs a count scan.  4 bits: 16 x 128 x 4 B = 8 KB beside the tiles keeps two workgroups per CU at
 * d <= 128; 8 bits would need 128 KB.  At the range's end the non-zero bins are added to
 * hist_out[u * 16 + digit] with integer device atomics: the sums do not depend on the order of arrival. */
template <int D, class Score, class Filter>
__global__ __launch_bounds__(256, D <= 128 ? 2 : 1) void select_gemm_kernel(ModelView m, const float* reps, const int* rep_row, uint32_t num_users,
                                                                           const uint32_t* prefix, const uint32_t* mask, int shift,
                                                                           const uint64_t* excl_ptr, const uint32_t* excl_items,
                                                                           uint32_t items_per_group, uint32_t* hist_out, uint32_t* nonfinite_flag,
                                                                           typename Filter::Args fa, typename Score::Args sa) {
    __shared__ float Es[2][32 * ItemTiles<D>::LDE];
    __shared__ float Bs[2][32];
    __shared__ __align__(16) float qbS[Score::query ? 128 : 4];
    __shared__ uint32_t Ts[2][Filter::on ? 32 : 1];
    __shared__ __align__(16) uint32_t anyS[Filter::on ? 128 : 4];
    __shared__ __align__(16) uint32_t anyZ[Filter::on ? 128 : 4];
    __shared__ __align__(16) uint32_t noneS[Filter::on ? 128 : 4];
    // per-row state by slot (slot_user)
    __shared__ __align__(16) uint32_t prefS[128];
    __shared__ __align__(16) uint32_t maskS[128];
    __shared__ uint64_t exLo[128];
    __shared__ uint64_t exHi[128];
    __shared__ uint32_t hist[128 * 16];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int hh = lane >> 5;
    const uint32_t u0 = blockIdx.x * 128 + wave * 32;
    float a[D / 2];
    load_user_fragments<D>(a, reps, rep_row, num_users, u0);
    if (tid < 128) {
        const uint32_t u = blockIdx.x * 128 + (uint32_t)slot_user(tid);
        const bool real = u < num_users;
        prefS[tid] = real ? prefix[u] : 1u;
        maskS[tid] = real ? mask[u] : 0u;
        exLo[tid] = real && excl_ptr ? excl_ptr[u] : 0ull;
        exHi[tid] = real && excl_ptr ? excl_ptr[u + 1] : 0ull;
        if constexpr (Filter::on) {
            const uint32_t any = real ? fa.any_of[u] : 0u;
            anyS[tid] = any;
            anyZ[tid] = any == 0u ? 1u : 0u;
            noneS[tid] = real ? fa.none_of[u] : 0u;
        }
        if constexpr (Score::query) qbS[tid] = real ? sa.qb[rep_row[u]] : 0.0f;
    }
    for (int i = tid; i < 128 * 16; i += 256) hist[i] = 0u;
    uint32_t umask = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q)
        if (acc_user(u0, q, hh) < num_users) umask |= 1u << q;
    bool bad = false;
    ItemTiles<D> tiles(m, items_per_group);
    const int ntiles = tiles.ntiles;
    if (ntiles > 0) {
        tiles.fetch(m, 0);
        tiles.stage(Es[0], Bs[0]);
        if constexpr (Filter::on) {
            tiles.fetch_tags(fa.tags, 0);
            tiles.stage_tags(Ts[0]);
        }
    }
    __syncthreads();
    const int pbase = wave * 32 + hh * 16;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < ntiles) {
            tiles.fetch(m, tile + 1);
            if constexpr (Filter::on) tiles.fetch_tags(fa.tags, tile + 1);
        }
        f32x16 acc = tile_dots<D>(a, Es[buf]);
        const float bias = Bs[buf][l31];
        if constexpr (Score::query) {
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 b4 = ld4(&qbS[pbase + 4 * q4]);
                acc[4 * q4 + 0] = b4.x + acc[4 * q4 + 0];
                acc[4 * q4 + 1] = b4.y + acc[4 * q4 + 1];
                acc[4 * q4 + 2] = b4.z + acc[4 * q4 + 2];
                acc[4 * q4 + 3] = b4.w + acc[4 * q4 + 3];
            }
        }
        const uint32_t id = tiles.i_begin + (uint32_t)tile * 32 + (uint32_t)l31;
        uint32_t pend = id < tiles.i_end ? umask : 0u;
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const uint4 p4 = *reinterpret_cast<const uint4*>(&prefS[pbase + 4 * q4]);
            const uint4 m4 = *reinterpret_cast<const uint4*>(&maskS[pbase + 4 * q4]);
            const uint32_t pq[4] = {p4.x, p4.y, p4.z, p4.w};
            const uint32_t mq[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = 4 * q4 + j;
                const float sc = TK_SCORE(q);
                if (((pend >> q) & 1u) && !(sc - sc == 0.0f)) bad = true;
                if ((select_key(sc) & mq[j]) != pq[j]) pend &= ~(1u << q);
            }
        }
        if constexpr (Filter::on) {
            const uint32_t tag = Ts[buf][l31];
            uint32_t drop = 0;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const uint4 a4 = *reinterpret_cast<const uint4*>(&anyS[pbase + 4 * q4]);
                const uint4 z4 = *reinterpret_cast<const uint4*>(&anyZ[pbase + 4 * q4]);
                const uint4 n4 = *reinterpret_cast<const uint4*>(&noneS[pbase + 4 * q4]);
                const uint32_t any[4] = {a4.x, a4.y, a4.z, a4.w};
                const uint32_t anyz[4] = {z4.x, z4.y, z4.z, z4.w};
                const uint32_t none[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t hit = (tag & none[j]) != 0u ? 1u : 0u;
                    const uint32_t miss = ((tag & any[j]) | anyz[j]) == 0u ? 1u : 0u;
                    drop |= (hit | miss) << (4 * q4 + j);
                }
            }
            pend &= ~drop;
        }
        if (excl_ptr) {
            for (uint32_t rem = pend; rem; rem &= rem - 1u) {
                const int q = __ffs((int)rem) - 1;
                uint64_t lo = exLo[pbase + q];
                const uint64_t e1 = exHi[pbase + q];
                uint64_t hi = e1;
                while (lo < hi) {
                    const uint64_t mid = (lo + hi) >> 1;
                    if (excl_items[mid] < id) lo = mid + 1; else hi = mid;
                }
                if (lo < e1 && excl_items[lo] == id) pend &= ~(1u << q);
            }
        }
        if (__any(pend != 0u)) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const bool p = ((pend >> q) & 1u) != 0u;
                const uint32_t digit = (select_key(TK_SCORE(q)) >> shift) & 15u;
                uint64_t rem = __ballot(p);
                while (rem) { /* wave-uniform: one turn per distinct digit among the pending lanes */
                    const uint32_t dg = (uint32_t)__shfl((int)digit, (int)__ffsll((unsigned long long)rem) - 1, 64);
                    const uint64_t same = __ballot(p && digit == dg);
                    const uint32_t mine = hh ? (uint32_t)(same >> 32) : (uint32_t)same;
                    if (l31 == 0 && mine) hist[(pbase + q) * 16 + (int)dg] += (uint32_t)__popc(mine);
                    rem &= ~same;
                }
            }
        }
        if (tile + 1 < ntiles) {
            tiles.stage(Es[buf ^ 1], Bs[buf ^ 1]);
            if constexpr (Filter::on) tiles.stage_tags(Ts[buf ^ 1]);
        }
        __syncthreads();
    }
    for (int i = tid; i < 128 * 16; i += 256) {
        const uint32_t u = blockIdx.x * 128 + (uint32_t)slot_user(i >> 4);
        const uint32_t c = hist[i];
        if (c && u < num_users) atomicAdd(&hist_out[(size_t)u * 16 + (i & 15)], c);
    }
    if (__any(bad) && lane == 0) atomicOr(nonfinite_flag, 1u);
}
#undef TK_SCORE

/* Between the select's rounds, one thread per row.  round < 0 starts the search: wanted = n (0: decided, cut +inf), nothing
 * decided, the histogram cleared.  round r has binned digit 28 - 4 r: the thread sums the row's 16 bins, in round 0 decides a row
 * with fewer eligible columns than wanted (cut -inf, everything eligible), else walks the bins from the top until the running
 * count reaches what is still wanted, fixes that digit and keeps the count above it in gt.  After round 7 the key is whole: cut is
 * its f32 (a zero is +0.0), gt = #{score > cut}, final = min(n, eligible) and keep_eq = n - gt, what top_trim_kernel keeps of the
 * scores equal to the cut.  The bins are cleared for the next round. */
__global__ __launch_bounds__(256) void select_step_kernel(uint32_t num_rows, int round, const uint64_t* n, uint64_t* wanted, uint32_t* prefix,
                                                          uint32_t* mask, uint32_t* hist, float* cuts, uint32_t* gt, uint32_t* final_counts,
                                                          uint32_t* keep_eq) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= num_rows) return;
    uint32_t* h = hist + (size_t)r * 16;
    if (round < 0) {
        const uint64_t w = n[r];
        wanted[r] = w;
        prefix[r] = w ? 0u : 1u;
        mask[r] = 0u;
        gt[r] = 0u;
        final_counts[r] = 0u;
        keep_eq[r] = 0u;
        cuts[r] = w ? -INFINITY : INFINITY;
        for (int b = 0; b < 16; ++b) h[b] = 0u;
        return;
    }
    if (mask[r] == 0u && prefix[r] == 1u) return; /* decided */
    const int shift = 28 - 4 * round;
    uint32_t c[16];
    uint64_t total = 0;
    for (int b = 0; b < 16; ++b) {
        c[b] = h[b];
        h[b] = 0u;
        total += c[b];
    }
    const uint64_t w = wanted[r];
    if (total < w) { /* only in round 0: later rounds hold at least `wanted` in the interval */
        cuts[r] = -INFINITY;
        gt[r] = (uint32_t)total;
        final_counts[r] = (uint32_t)total;
        keep_eq[r] = 0u;
        mask[r] = 0u;
        prefix[r] = 1u;
        return;
    }
    uint64_t run = 0;
    int b = 0;
    bool found = false;
#pragma unroll
    for (int i = 15; i >= 1; --i) { /* unrolled: c stays in registers; bin 0 takes what the others did not */
        if (!found && run + c[i] >= w) {
            found = true;
            b = i;
        }
        if (!found) run += c[i];
    }
    const uint32_t pre = prefix[r] | ((uint32_t)b << shift);
    const uint32_t g = gt[r] + (uint32_t)run;
    wanted[r] = w - run;
    gt[r] = g;
    if (shift > 0) {
        prefix[r] = pre;
        mask[r] |= 15u << shift;
        return;
    }
    cuts[r] = select_unkey(pre);
    final_counts[r] = g + (uint32_t)(w - run);
    keep_eq[r] = (uint32_t)(w - run);
    mask[r] = 0u;
    prefix[r] = 1u;
}

/* Row r of a fill at the cuts, ascending column at in_ids / in_scores [offsets[r G] - offsets[0], + ge[r]), to its final place
 * out_ids / out_scores [out_off[r], out_off[r + 1]): every entry over the cut and the first keep_eq[r] that equal it (the f32
 * compare: both zeros), column order kept.  One workgroup per row, 256 entries at a time; an entry's place is the count of kept
 * entries before it, which is #{over the cut before it} + min(#{equal before it}, keep_eq).  Reads and writes are bounds-checked:
 * one outside its buffer or its row's final range is dropped and raises *overrun_flag. */
__global__ __launch_bounds__(256) void top_trim_kernel(const uint32_t* in_ids, const float* in_scores, uint32_t in_cap, const uint64_t* offsets,
                                                       uint32_t G, const uint32_t* ge, const float* cuts, const uint32_t* keep_eq,
                                                       const uint64_t* out_off, uint32_t* out_ids, float* out_scores, uint32_t out_cap,
                                                       uint32_t* overrun_flag) {
    __shared__ uint32_t wg[4], we[4];
    const uint32_t r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t start = offsets[(size_t)r * G] - offsets[0];
    const uint32_t len = ge[r];
    const float cut = cuts[r];
    const uint32_t keep = keep_eq[r];
    const uint64_t o0 = out_off[r], o1 = out_off[r + 1];
    uint32_t gt_before = 0, eq_before = 0; /* of the row's entries ahead of this round's 256 */
    bool over = false;
    for (uint32_t base = 0; base < len; base += 256) {
        const uint64_t at = start + base + (uint32_t)tid;
        const bool have = base + (uint32_t)tid < len && at < (uint64_t)in_cap;
        if (base + (uint32_t)tid < len && !have) over = true;
        const uint32_t id = have ? in_ids[at] : 0u;
        const float sc = have ? in_scores[at] : 0.0f;
        const bool is_gt = have && sc > cut, is_eq = have && sc == cut;
        const uint64_t bg = __ballot(is_gt), be = __ballot(is_eq);
        if (lane == 0) {
            wg[wave] = (uint32_t)__popcll(bg);
            we[wave] = (uint32_t)__popcll(be);
        }
        __syncthreads();
        const uint64_t below = (1ull << lane) - 1ull;
        uint32_t g = gt_before + (uint32_t)__popcll(bg & below), e = eq_before + (uint32_t)__popcll(be & below);
        for (int w = 0; w < 4; ++w) {
            if (w < wave) {
                g += wg[w];
                e += we[w];
            }
            gt_before += wg[w];
            eq_before += we[w];
        }
        if (is_gt || (is_eq && e < keep)) {
            const uint64_t pos = o0 + g + (e < keep ? e : keep);
            if (pos < o1 && pos < (uint64_t)out_cap) {
                out_ids[pos] = id;
                if (out_scores) out_scores[pos] = sc;
            } else
                over = true;
        }
        __syncthreads();
    }
    if (__any(over) && lane == 0) atomicOr(overrun_flag, 1u);
}

/* The exclusive scan of counts [n G] in (row, range) order into offsets [n G + 1], and the rows' totals; one workgroup: each
 * thread sums a contiguous piece, the 1 024 sums are scanned in LDS, and the piece is walked again.  n G is at most a few hundred
 * thousand (8 192 rows x above_groups' ranges), a few microseconds next to the scan. */
__global__ __launch_bounds__(1024) void above_offsets_kernel(const uint32_t* counts, uint32_t n, uint32_t G, uint64_t* offsets, uint32_t* totals) {
    __shared__ uint64_t part[1024];
    const uint32_t tid = threadIdx.x;
    const uint64_t N = (uint64_t)n * G;
    const uint64_t per = (N + 1023) / 1024;
    const uint64_t i0 = (uint64_t)tid * per < N ? (uint64_t)tid * per : N;
    const uint64_t i1 = i0 + per < N ? i0 + per : N;
    uint64_t sum = 0;
    for (uint64_t i = i0; i < i1; ++i) sum += counts[i];
    part[tid] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        const uint64_t v = tid >= off ? part[tid - off] : 0ull;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint64_t run = part[tid] - sum;
    for (uint64_t i = i0; i < i1; ++i) {
        offsets[i] = run;
        run += counts[i];
    }
    if (tid == 1023) offsets[N] = part[1023];
    for (uint32_t r = tid; r < n; r += 1024) {
        uint32_t t = 0;
        for (uint32_t g = 0; g < G; ++g) t += counts[(size_t)r * G + g];
        totals[r] = t;
    }
}

// ------------------------------------------------------------------------------------------------
// user_representations: the users' final states out of the forward pass's packed rows
// ------------------------------------------------------------------------------------------------
/* out[i][c] = H[rep_row[i]][c] for c < dl (embedding_dim; H's rows are d floats): the rows in user order and at the caller's width,
 * so one copy brings the launch's representations to the host. */
__global__ __launch_bounds__(256) void rep_rows_kernel(const float* H, const int* rep_row, uint32_t num_users, int d, int dl, float* out) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t i = idx / (uint64_t)dl;
    if (i >= num_users) return;
    out[idx] = H[(size_t)rep_row[i] * d + (idx - i * (uint64_t)dl)];
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
void launch_predict(const ModelView& m, const float* user, const uint32_t* items, uint64_t n, float* out, hipStream_t s) {
    if (n == 0) return;
    DISPATCH_D(m.d, { hipLaunchKernelGGL((predict_kernel<DD>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, m, user, items, n, out); });
}

int launch_rank(const ModelView& m, const float* reps, const int* rep_row, uint32_t num_users, const uint32_t* test_item,
                const uint32_t* test_in_hist, const uint64_t* hist_ptr, const uint32_t* hist_items, float* ts_scratch,
                uint32_t* ranks, uint32_t* nonfinite_flag, hipStream_t s) {
    if (num_users == 0) return 0;
    // 32 users per wave (128 per workgroup, four waves per SIMD).  (A 64-users-per-wave form — half the barriers and LDS fills per
    // flop at half the waves — measured 5 % slower at 8 192 users x 1e6 items, d = 128: 100 against 105 TFLOP/s; removed.)
    const uint32_t utiles = (num_users + 127) / 128;
    // item ranges: MANY more workgroups than the chip holds at once (a launch of 1 024 workgroups on 768 resident slots ran one
    // full round and a third of a second one); the kernel's per-lane counters are 16 bits wide: fewer than 65 536 tiles per range
    uint32_t per = 0;
    const uint32_t groups = split_items(m.num_items, wanted_groups((768u * 6u + utiles - 1) / utiles), UINT32_MAX, 65535u * 32u, &per);
    DISPATCH_D(m.d, {
        hipLaunchKernelGGL((rank_test_score_kernel<DD>), dim3((num_users + 255) / 256), dim3(256), 0, s, m, reps, rep_row, num_users, test_item, test_in_hist, ts_scratch, ranks);
        hipLaunchKernelGGL((rank_gemm_kernel<DD>), dim3(utiles, groups), dim3(256), 0, s, m, reps, rep_row, num_users, ts_scratch, per, ranks, nonfinite_flag);
        hipLaunchKernelGGL((rank_history_kernel<DD>), dim3(num_users), dim3(64), 0, s, m, reps, rep_row, ts_scratch, hist_ptr, hist_items, ranks);
    });
    return 1; /* the ledger's count of mrr_score's scan (sbr_kernels.h) */
}

int launch_sequence_ranks(const ModelView& m, const float* reps, const int* rep_row, uint32_t num_units, const uint32_t* test_item,
                          const uint32_t* test_in_prefix, const uint2* unit_bt, const int* off, const uint32_t* in_idx,
                          const uint32_t* first_occ, float* ts_scratch, uint32_t* ranks, uint32_t* nonfinite_flag, hipStream_t s) {
    if (num_units == 0) return 0;
    // the scan is launch_rank's: the same user tiles and item ranges
    const uint32_t utiles = (num_units + 127) / 128;
    uint32_t per = 0;
    const uint32_t groups = split_items(m.num_items, wanted_groups((768u * 6u + utiles - 1) / utiles), UINT32_MAX, 65535u * 32u, &per);
    DISPATCH_D(m.d, {
        hipLaunchKernelGGL((rank_test_score_kernel<DD>), dim3((num_units + 255) / 256), dim3(256), 0, s, m, reps, rep_row, num_units, test_item, test_in_prefix, ts_scratch, ranks);
        hipLaunchKernelGGL((rank_gemm_kernel<DD>), dim3(utiles, groups), dim3(256), 0, s, m, reps, rep_row, num_units, ts_scratch, per, ranks, nonfinite_flag);
        if (unit_bt)
            hipLaunchKernelGGL((rank_prefix_kernel<DD>), dim3((num_units + 3) / 4), dim3(256), 0, s, m, reps, rep_row, ts_scratch, unit_bt, num_units, off, in_idx, first_occ, ranks);
    });
    return 1; /* one scan, as launch_rank */
}

uint32_t rank_targets_tmax(int d) {
    // the thresholds and buckets of 128 slots (2 x 128 x TM words of LDS) beside the item tiles: three workgroups per CU at d <= 128
    // (50 KB each), two at d = 256 (75 KB; with 16 thresholds a workgroup would take 83 KB and a CU hold one)
    return d <= 128 ? 16u : 8u;
}

int launch_rank_targets(const ModelView& m, const float* reps, const int* rep_row, const uint32_t* su_user, const uint32_t* sptr,
                        uint32_t num_su, const uint32_t* tgt_items, const uint64_t* mask_ptr, const uint32_t* mask_items, float* ts,
                        uint32_t* pos, float* th, float* tmin, float* tmin2, uint32_t* buckets, uint32_t* totals, uint32_t* ranks,
                        uint32_t* nonfinite_flag, hipStream_t s) {
    if (num_su == 0) return 0;
    const uint32_t utiles = (num_su + 127) / 128;
    // item ranges as launch_rank's, and its limit: the kernel's per-lane counters are 16 bits wide, fewer than 65 536 tiles per range
    uint32_t per = 0;
    const uint32_t groups = split_items(m.num_items, wanted_groups((768u * 6u + utiles - 1) / utiles), UINT32_MAX, 65535u * 32u, &per);
    DISPATCH_D(m.d, {
        constexpr int TM = DD <= 128 ? 16 : 8; /* = rank_targets_tmax(DD) */
        hipLaunchKernelGGL((rank_targets_prepare_kernel<DD, TM>), dim3((num_su + 256 / TM - 1) / (256 / TM)), dim3(256), 0, s, m, reps, rep_row,
                           su_user, sptr, num_su, tgt_items, mask_ptr, mask_items, ts, pos, th, tmin, tmin2, buckets, totals);
        hipLaunchKernelGGL((rank_targets_gemm_kernel<DD, TM>), dim3(utiles, groups), dim3(256), 0, s, m, reps, rep_row, num_su, th, tmin, tmin2,
                           per, buckets, totals, nonfinite_flag);
        hipLaunchKernelGGL((rank_targets_finish_kernel<DD, TM>), dim3(num_su), dim3(64), 0, s, m, reps, rep_row, su_user, sptr, ts, pos,
                           buckets, totals, mask_ptr, mask_items, ranks);
    });
    return 3;
}

#include "sbr_rank_eligible.h"

uint32_t recommend_groups(uint32_t num_users, uint32_t num_items, uint32_t k, uint32_t* items_per_group) {
    // Two rounds of the chip's resident slots (two workgroups per CU at d <= 128), not launch_rank's six: a range's first k items
    // are all candidates and the rest about k ln(range / k), so fewer, longer ranges merge less (8 192 users x 1e6 items, d = 128,
    // k = 100: 113 ms of kernels at 4 608 workgroups); at most TK_MERGE_MAX / k lists per user for the merge
    const uint32_t utiles = (num_users + 127) / 128;
    return split_items(num_items, wanted_groups((256u * 2u * 2u + utiles - 1) / utiles), TK_MERGE_MAX / k, UINT32_MAX, items_per_group);
}

namespace {

template <int D, class Score, class Filter>
void topk_gemm_launch(dim3 grid, const ModelView& cat, const float* reps, const TopkScan& sc, uint32_t items_per_group, typename Filter::Args fa,
                      typename Score::Args sa, hipStream_t s) {
    hipLaunchKernelGGL((topk_gemm_kernel<D, Score, Filter>), grid, dim3(256), 0, s, cat, reps, sc.rep_row, sc.n, sc.excl_ptr, sc.excl_items,
                       items_per_group, sc.k, sc.lists, sc.lens, sc.nonfinite_flag, fa, sa);
}

/* The top-k scan of every launcher below, two launches: topk_gemm_kernel<cat.d, Score, .> over the catalogue `cat` (its E, b,
 * num_items: the model's, or a launcher's rewrite of them) with the A rows reps[sc.rep_row[u]], split into recommend_groups' item
 * ranges, then topk_merge_kernel.  The only place that decides the split, the grid, the merge size and the Filter instantiation:
 * TagFilter where sc.f is set — never under QueryBias (audience has no filter), so that pair, five large kernels, does not exist. */
template <class Score>
int topk_scan(const ModelView& cat, const float* reps, const TopkScan& sc, typename Score::Args sa, hipStream_t s) {
    uint32_t per = 0;
    const uint32_t groups = recommend_groups(sc.n, cat.num_items, sc.k, &per);
    const dim3 grid((sc.n + 127) / 128, groups);
    uint32_t n = 1;
    while (n < groups * sc.k) n <<= 1;
    const bool filtered = !Score::query && sc.f.tags;
    DISPATCH_D(cat.d, {
        if constexpr (!Score::query)
            if (filtered) topk_gemm_launch<DD, Score, TagFilter>(grid, cat, reps, sc, per, TagFilter::Args{sc.f.tags, sc.f.any_of, sc.f.none_of}, sa, s);
        if (!filtered) topk_gemm_launch<DD, Score, NoFilter>(grid, cat, reps, sc, per, NoFilter::Args{}, sa, s);
    });
    hipLaunchKernelGGL(topk_merge_kernel, dim3(sc.n), dim3(512), 0, s, sc.lists, sc.lens, groups, sc.k, n, sc.out_items, sc.out_scores);
    return 2;
}

/* out_items' positions in a sub-table or a candidate list -> the ids they stand for; one launch */
int launch_subset_ids(const uint32_t* ids, const TopkScan& sc, hipStream_t s) {
    const uint64_t n = (uint64_t)sc.n * sc.k;
    hipLaunchKernelGGL(subset_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ids, sc.out_items, n);
    return 1;
}

}  // namespace

int launch_recommend(const ModelView& m, const float* reps, const TopkScan& sc, hipStream_t s) {
    if (sc.n == 0) return 0;
    return topk_scan<BiasAdd>(m, reps, sc, BiasAdd::Args{}, s);
}

int launch_recommend_sampled(const ModelView& m, const float* reps, const TopkScan& sc, const SampleScan& sp, hipStream_t s) {
    if (sc.n == 0) return 0;
    const uint64_t np = (uint64_t)sc.n * sc.k;
    const unsigned pair_blocks = (unsigned)((np + 255) / 256);
    hipLaunchKernelGGL(sample_keys_kernel, dim3((sc.n + 255) / 256), dim3(256), 0, s, sp.seed, sp.streams, sc.n, sc.g.keys);
    int n = 1 + (sp.ids ? topk_scan<GumbelMapped>(m, reps, sc, GumbelMapped::Args{sc.g.inv_t, sc.g.keys, sp.ids}, s)
                        : topk_scan<GumbelBias>(m, reps, sc, GumbelBias::Args{sc.g.inv_t, sc.g.keys}, s));
    hipLaunchKernelGGL(sample_pairs_kernel, dim3(pair_blocks), dim3(256), 0, s, sc.rep_row, sc.out_items, sc.n, sc.k, sp.pair_row, sp.pair_item);
    n += 1 + launch_candidate_scores(m, reps, sp.pair_row, sp.pair_item, np, sp.plain, sc.nonfinite_flag, s);
    hipLaunchKernelGGL(sample_pad_kernel, dim3(pair_blocks), dim3(256), 0, s, sc.out_items, np, sp.plain);
    /* the plain scores were taken on the sub-table by position; only now do the rows' positions become ids */
    return n + 1 + (sp.ids ? launch_subset_ids(sp.ids, sc, s) : 0);
}

namespace {

/* log_partition's sum scan over sc's rows at pt's shifts, then — with exclusion lists — the finish: the only place that decides the
 * sum scan's item ranges and its Filter instantiation */
int partition_sum(const ModelView& m, const float* reps, const TopkScan& sc, const PartitionScan& pt, hipStream_t s) {
    // item ranges as launch_recommend's at k = 1: two rounds of the chip's resident slots (two workgroups per CU at d <= 128)
    const uint32_t utiles = (sc.n + 127) / 128;
    uint32_t per = 0;
    const uint32_t groups = split_items(m.num_items, wanted_groups((256u * 2u * 2u + utiles - 1) / utiles), UINT32_MAX, UINT32_MAX, &per);
    const uint32_t fb = sbr_softmax_fbits(pt.num_items ? pt.num_items : m.num_items);
    const dim3 grid(utiles, groups);
    DISPATCH_D(m.d, {
        if (sc.f.tags)
            hipLaunchKernelGGL((partition_gemm_kernel<DD, TagFilter>), grid, dim3(256), 0, s, m, reps, sc.rep_row, sc.n, pt.shift, pt.inv_t, fb, per,
                               pt.mass, sc.nonfinite_flag, TagFilter::Args{sc.f.tags, sc.f.any_of, sc.f.none_of});
        else
            hipLaunchKernelGGL((partition_gemm_kernel<DD, NoFilter>), grid, dim3(256), 0, s, m, reps, sc.rep_row, sc.n, pt.shift, pt.inv_t, fb, per,
                               pt.mass, sc.nonfinite_flag, NoFilter::Args{});
        if (sc.excl_ptr)
            hipLaunchKernelGGL((partition_finish_kernel<DD>), dim3(sc.n), dim3(64), 0, s, m, reps, sc.rep_row, pt.shift, pt.inv_t, fb, sc.excl_ptr,
                               sc.excl_items, sc.f.tags, sc.f.any_of, sc.f.none_of, pt.mass);
    });
    return 1 + (sc.excl_ptr ? 1 : 0);
}

}  // namespace

int launch_log_partition(const ModelView& m, const float* reps, const TopkScan& sc, const PartitionScan& pt, hipStream_t s) {
    if (sc.n == 0) return 0;
    int n = topk_scan<BiasAdd>(m, reps, sc, BiasAdd::Args{}, s); /* sc.k == 1: the rows' best allowed items and their scores */
    hipLaunchKernelGGL(partition_shift_kernel, dim3((sc.n + 255) / 256), dim3(256), 0, s, sc.out_items, sc.out_scores, sc.n, pt.inv_t, pt.shift,
                       pt.mass);
    return n + 1 + partition_sum(m, reps, sc, pt, s);
}

int launch_topk_partition(const ModelView& m, const float* reps, const TopkScan& sc, const PartitionScan& pt, hipStream_t s) {
    if (sc.n == 0) return 0;
    int n = topk_scan<BiasAdd>(m, reps, sc, BiasAdd::Args{}, s); /* column 0: the rows' best allowed items, launch_log_partition's pre-scan */
    hipLaunchKernelGGL(partition_shift_strided_kernel, dim3((sc.n + 255) / 256), dim3(256), 0, s, sc.out_items, sc.out_scores, sc.n, sc.k, pt.inv_t,
                       pt.shift, pt.mass);
    return n + 1 + partition_sum(m, reps, sc, pt, s);
}

uint32_t sequence_shift_pool() {
    const char* e = std::getenv("SBR_SEQ_SHIFT_K");
    if (e && *e) {
        const long long k = std::atoll(e);
        if (k >= 1 && k <= 1024) return (uint32_t)k;
    }
    return 16; /* a row is unresolved only if its 16 best items of the whole catalogue are all in its own prefix */
}

int launch_sequence_shift(const ModelView& m, const float* reps, const TopkScan& sc, const SequencePartitionScan& sp, hipStream_t s) {
    if (sc.n == 0) return 0;
    int n = topk_scan<BiasAdd>(m, reps, sc, BiasAdd::Args{}, s); /* no exclusion list: the rows' sc.k best of the whole catalogue */
    if (sp.unit_bt)
        hipLaunchKernelGGL(sequence_shift_kernel, dim3((sc.n + 3) / 4), dim3(256), 0, s, sc.out_items, sc.out_scores, sc.k, sp.unit_bt, sc.n, sp.off,
                           sp.in_idx, sp.pt.inv_t, sp.pt.shift, sp.pt.mass, sp.unresolved);
    else /* sc.k == 1 and nothing masked: log_partition's own shift */
        hipLaunchKernelGGL(partition_shift_kernel, dim3((sc.n + 255) / 256), dim3(256), 0, s, sc.out_items, sc.out_scores, sc.n, sp.pt.inv_t,
                           sp.pt.shift, sp.pt.mass);
    return n + 1;
}

int launch_sequence_shift_rows(const ModelView& m, const float* reps, const TopkScan& sc, float inv_t, const uint32_t* rows, float* shift,
                               hipStream_t s) {
    if (sc.n == 0) return 0;
    int n = topk_scan<BiasAdd>(m, reps, sc, BiasAdd::Args{}, s); /* sc.k == 1, with the rows' exclusion lists */
    hipLaunchKernelGGL(sequence_shift_rows_kernel, dim3((sc.n + 255) / 256), dim3(256), 0, s, sc.out_items, sc.out_scores, sc.n, inv_t, rows, shift);
    return n + 1;
}

int launch_sequence_partition(const ModelView& m, const float* reps, const TopkScan& sc, const SequencePartitionScan& sp, hipStream_t s) {
    if (sc.n == 0) return 0;
    int n = partition_sum(m, reps, sc, sp.pt, s); /* sc has neither lists nor tags: every item with d <= 0 is added */
    const uint32_t fb = sbr_softmax_fbits(m.num_items);
    DISPATCH_D(m.d, {
        hipLaunchKernelGGL((partition_prefix_kernel<DD>), dim3((sc.n + 3) / 4), dim3(256), 0, s, m, reps, sc.rep_row, sp.pt.shift, sp.pt.inv_t, fb,
                           sp.unit_bt, sc.n, sp.off, sp.in_idx, sp.first_occ, sp.target, sp.pt.mass, sp.scores);
    });
    return n + 1;
}

uint32_t above_groups(uint32_t num_rows, uint32_t num_items, uint32_t* items_per_group) {
    // item ranges as launch_log_partition's sum scan: two rounds of the chip's resident slots; no limit from a merge, there is none
    const uint32_t utiles = (num_rows + 127) / 128;
    return split_items(num_items, wanted_groups((256u * 2u * 2u + utiles - 1) / (utiles ? utiles : 1u)), UINT32_MAX, UINT32_MAX, items_per_group);
}

namespace {

/* above_gemm_kernel over rows [r0, r0 + nr) of sc: the only place that decides its policies — QueryBias where qb is set (never with
 * a filter), TagFilter where sc.f.tags is */
template <bool Fill>
void above_scan(const ModelView& cat, const float* reps, const float* qb, const AboveScan& sc, uint32_t r0, uint32_t nr, uint32_t* out_ids,
                float* out_scores, uint32_t out_cap, hipStream_t s) {
    const dim3 grid((nr + 127) / 128, sc.groups);
    const size_t g0 = (size_t)r0 * sc.groups;
    const uint64_t* eptr = sc.excl_ptr ? sc.excl_ptr + r0 : nullptr;
    DISPATCH_D(cat.d, {
        if (qb)
            hipLaunchKernelGGL((above_gemm_kernel<DD, QueryBias, NoFilter, Fill>), grid, dim3(256), 0, s, cat, reps, sc.rep_row + r0, nr,
                               sc.thresholds + r0, eptr, sc.excl_items, sc.per, sc.counts + g0, sc.offsets + g0, out_ids, out_scores, out_cap,
                               sc.overrun_flag, sc.nonfinite_flag, NoFilter::Args{}, QueryBias::Args{qb});
        else if (sc.f.tags)
            hipLaunchKernelGGL((above_gemm_kernel<DD, BiasAdd, TagFilter, Fill>), grid, dim3(256), 0, s, cat, reps, sc.rep_row + r0, nr,
                               sc.thresholds + r0, eptr, sc.excl_items, sc.per, sc.counts + g0, sc.offsets + g0, out_ids, out_scores, out_cap,
                               sc.overrun_flag, sc.nonfinite_flag, TagFilter::Args{sc.f.tags, sc.f.any_of + r0, sc.f.none_of + r0},
                               BiasAdd::Args{});
        else
            hipLaunchKernelGGL((above_gemm_kernel<DD, BiasAdd, NoFilter, Fill>), grid, dim3(256), 0, s, cat, reps, sc.rep_row + r0, nr,
                               sc.thresholds + r0, eptr, sc.excl_items, sc.per, sc.counts + g0, sc.offsets + g0, out_ids, out_scores, out_cap,
                               sc.overrun_flag, sc.nonfinite_flag, NoFilter::Args{}, BiasAdd::Args{});
    });
}

}  // namespace

int launch_above_count(const ModelView& cat, const float* reps, const float* qb, const AboveScan& sc, hipStream_t s) {
    if (sc.n == 0 || cat.num_items == 0) return 0;
    above_scan<false>(cat, reps, qb, sc, 0, sc.n, nullptr, nullptr, 0, s);
    hipLaunchKernelGGL(above_offsets_kernel, dim3(1), dim3(1024), 0, s, sc.counts, sc.n, sc.groups, sc.offsets, sc.totals);
    return 2;
}

int launch_above_fill(const ModelView& cat, const float* reps, const float* qb, const AboveScan& sc, uint32_t r0, uint32_t nr, uint32_t* out_ids,
                      float* out_scores, uint32_t out_cap, hipStream_t s) {
    if (nr == 0 || cat.num_items == 0 || out_cap == 0) return 0;
    above_scan<true>(cat, reps, qb, sc, r0, nr, out_ids, out_scores, out_cap, s);
    return 1;
}

int launch_top_select(const ModelView& cat, const float* reps, const float* qb, const AboveScan& sc, const TopSelect& ts, hipStream_t s) {
    if (sc.n == 0) return 0;
    const dim3 rows((sc.n + 255) / 256);
    auto step = [&](int round) {
        hipLaunchKernelGGL(select_step_kernel, rows, dim3(256), 0, s, sc.n, round, ts.n, ts.wanted, ts.prefix, ts.mask, ts.hist, ts.cuts, ts.gt,
                           ts.final_counts, ts.keep_eq);
    };
    step(-1);
    const dim3 grid((sc.n + 127) / 128, sc.groups);
    for (int round = 0; round < 8; ++round) {
        const int shift = 28 - 4 * round;
        if (cat.num_items) { /* an empty catalogue: every bin stays zero and round 0 decides every row */
            DISPATCH_D(cat.d, {
                if (qb)
                    hipLaunchKernelGGL((select_gemm_kernel<DD, QueryBias, NoFilter>), grid, dim3(256), 0, s, cat, reps, sc.rep_row, sc.n, ts.prefix,
                                       ts.mask, shift, sc.excl_ptr, sc.excl_items, sc.per, ts.hist, sc.nonfinite_flag, NoFilter::Args{},
                                       QueryBias::Args{qb});
                else if (sc.f.tags)
                    hipLaunchKernelGGL((select_gemm_kernel<DD, BiasAdd, TagFilter>), grid, dim3(256), 0, s, cat, reps, sc.rep_row, sc.n, ts.prefix,
                                       ts.mask, shift, sc.excl_ptr, sc.excl_items, sc.per, ts.hist, sc.nonfinite_flag,
                                       TagFilter::Args{sc.f.tags, sc.f.any_of, sc.f.none_of}, BiasAdd::Args{});
                else
                    hipLaunchKernelGGL((select_gemm_kernel<DD, BiasAdd, NoFilter>), grid, dim3(256), 0, s, cat, reps, sc.rep_row, sc.n, ts.prefix,
                                       ts.mask, shift, sc.excl_ptr, sc.excl_items, sc.per, ts.hist, sc.nonfinite_flag, NoFilter::Args{},
                                       BiasAdd::Args{});
            });
        }
        step(round);
    }
    return cat.num_items ? 17 : 9;
}

int launch_top_trim(const AboveScan& sc, const TopSelect& ts, uint32_t r0, uint32_t nr, const uint32_t* in_ids, const float* in_scores,
                    uint32_t in_cap, uint32_t* out_ids, float* out_scores, uint32_t out_cap, hipStream_t s) {
    if (nr == 0) return 0;
    hipLaunchKernelGGL(above_offsets_kernel, dim3(1), dim3(1024), 0, s, ts.final_counts + r0, nr, 1u, ts.out_off, ts.out_tot);
    hipLaunchKernelGGL(top_trim_kernel, dim3(nr), dim3(256), 0, s, in_ids, in_scores, in_cap, sc.offsets + (size_t)r0 * sc.groups, sc.groups,
                       sc.totals + r0, ts.cuts + r0, ts.keep_eq + r0, ts.out_off, out_ids, out_scores, out_cap, sc.overrun_flag);
    return 2;
}

int launch_subset_words(const uint32_t* subset, uint32_t num_subset, const uint32_t* src, uint32_t* dst, hipStream_t s) {
    if (num_subset == 0) return 0;
    hipLaunchKernelGGL(subset_words_kernel, dim3((num_subset + 255) / 256), dim3(256), 0, s, subset, num_subset, src, dst);
    return 1;
}

int launch_subset_positions(const uint32_t* subset, uint32_t num_subset, const uint64_t* eptr, uint32_t n, uint32_t* excl, hipStream_t s) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(subset_positions_kernel, dim3((n + 3) / 4), dim3(256), 0, s, subset, num_subset, eptr, n, excl);
    return 1;
}

int launch_subset_gather(const ModelView& m, const uint32_t* subset, uint32_t num_subset, float* Esub, float* bsub, hipStream_t s) {
    if (num_subset == 0) return 0;
    DISPATCH_D(m.d, {
        hipLaunchKernelGGL((subset_gather_kernel<DD>), dim3((unsigned)(((uint64_t)num_subset * (DD / 4) + 255) / 256)), dim3(256), 0, s, m, subset,
                           num_subset, Esub, bsub);
    });
    return 1;
}

int launch_above_ids(const uint32_t* row_ids, uint32_t* ids, uint64_t n, hipStream_t s) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(subset_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, row_ids, ids, n);
    return 1;
}

uint32_t diverse_max_pool(int d) {
    // the pool's rows at most 32 768 floats (128 KiB); the padding column, ids, scores, maxima, norms and flags of such a pool fit
    // in what is left of the CU's 160 KiB: 256 rows at d = 128, 128 at d = 256, 1 024 (recommend's largest k) up to d = 32
    const uint32_t p = 32768u / (uint32_t)d;
    return p < 1024u ? p : 1024u;
}

int launch_diverse_select(const ModelView& m, const uint32_t* pool_items, const float* pool_scores, uint32_t num_users, uint32_t pool,
                          uint32_t k_out, float trade_off, bool cosine, uint32_t* out_items, float* out_scores, uint32_t* nonfinite_flag,
                          hipStream_t s) {
    if (num_users == 0) return 0;
    /* qh + X + (id, s, mx, r, pk) + red: diverse_select_kernel's layout */
    const size_t lds = ((size_t)m.d + (size_t)pool * (m.d + 1) + 5 * (size_t)pool + 8) * 4;
    int dev = 0;
    (void)hipGetDevice(&dev);
    dev = dev >= 0 && dev < 64 ? dev : 0;
    DISPATCH_D(m.d, {
        static std::atomic<size_t> granted[64]; /* dynamic LDS beyond 64 KB is granted per kernel and device, once */
        if (lds > granted[dev]) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(diverse_select_kernel<DD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            granted[dev] = lds;
        }
        hipLaunchKernelGGL((diverse_select_kernel<DD>), dim3(num_users), dim3(256), lds, s, m, pool_items, pool_scores, pool, k_out, trade_off,
                           cosine ? 1 : 0, out_items, out_scores, nonfinite_flag);
    });
    return 1;
}

int launch_capped_select(const uint32_t* item_groups, uint32_t num_items, const uint32_t* pool_items, const float* pool_scores,
                         uint32_t num_users, uint32_t pool, uint32_t k_out, uint32_t cap, uint32_t* out_items, float* out_scores,
                         uint8_t* out_complete, hipStream_t s) {
    if (num_users == 0 || pool > CAP_MAX_POOL) return 0;
    hipLaunchKernelGGL(capped_select_kernel, dim3(num_users), dim3(256), 0, s, item_groups, num_items, pool_items, pool_scores, pool, k_out, cap,
                       out_items, out_scores, out_complete);
    return 1;
}

int launch_similar_items(const ModelView& m, const uint32_t* query, bool cosine, float* rnorm, float* H, const TopkScan& sc, hipStream_t s) {
    if (sc.n == 0) return 0;
    DISPATCH_D(m.d, {
        hipLaunchKernelGGL((item_rnorm_kernel<DD>), dim3((unsigned)(((uint64_t)m.num_items + 255) / 256)), dim3(256), 0, s, m, cosine ? 1 : 0, rnorm,
                           sc.nonfinite_flag);
        hipLaunchKernelGGL((similar_query_kernel<DD>), dim3((unsigned)(((uint64_t)sc.n * (DD / 4) + 255) / 256)), dim3(256), 0, s, m, rnorm,
                           query, sc.n, H);
    });
    ModelView mr = m; /* the scan's per-item value: r in the bias's place, so ItemTiles brings it in as it brings the bias */
    mr.b = rnorm;
    return 2 + topk_scan<ScaleMul>(mr, H, sc, ScaleMul::Args{}, s);
}

int launch_recommend_among(const ModelView& m, const uint32_t* subset, uint32_t num_subset, float* Esub, float* bsub, const float* reps,
                           const TopkScan& sc, hipStream_t s) {
    if (sc.n == 0 || num_subset == 0) return 0;
    DISPATCH_D(m.d, {
        hipLaunchKernelGGL((subset_gather_kernel<DD>), dim3((unsigned)(((uint64_t)num_subset * (DD / 4) + 255) / 256)), dim3(256), 0, s, m, subset,
                           num_subset, Esub, bsub);
    });
    ModelView ms = m; /* the scan's catalogue: the sub-table, whose item j is S[j] */
    ms.E = Esub;
    ms.b = bsub;
    ms.num_items = num_subset;
    return 1 + launch_recommend(ms, reps, sc, s) + launch_subset_ids(subset, sc, s);
}

void launch_audience_gather(const ModelView& m, const float* rows_table, const uint32_t* rows, uint32_t num_rows, float* T, float* bT,
                            hipStream_t s) {
    if (num_rows == 0) return;
    ModelView mh = m; /* the gather's source: the state rows where the item table stands; its per-row value is read and unused, so
                         any readable memory of the table's length does (the rows themselves), and bT is zeroed behind it */
    mh.E = const_cast<float*>(rows_table);
    mh.b = const_cast<float*>(rows_table);
    DISPATCH_D(m.d, {
        hipLaunchKernelGGL((subset_gather_kernel<DD>), dim3((unsigned)(((uint64_t)num_rows * (DD / 4) + 255) / 256)), dim3(256), 0, s, mh, rows,
                           num_rows, T, bT);
    });
    (void)hipMemsetAsync(bT, 0, (size_t)num_rows * 4, s);
}

int launch_audience(const ModelView& m, const float* T, const float* bT, uint32_t num_rows, const uint32_t* row_ids, const TopkScan& sc,
                    hipStream_t s) {
    if (sc.n == 0 || num_rows == 0) return 0;
    ModelView mt = m; /* the scan's catalogue: the candidate rows, whose "item" j is row j of T */
    mt.E = const_cast<float*>(T);
    mt.b = const_cast<float*>(bT);
    mt.num_items = num_rows;
    const int launches = topk_scan<QueryBias>(mt, m.E, sc, QueryBias::Args{m.b}, s);
    return launches + (row_ids ? launch_subset_ids(row_ids, sc, s) : 0);
}

int launch_candidate_scores(const ModelView& m, const float* reps, const uint32_t* pair_row, const uint32_t* pair_item, uint64_t num_pairs,
                            float* out, uint32_t* nonfinite_flag, hipStream_t s) {
    if (num_pairs == 0) return 0;
    DISPATCH_D(m.d, {
        hipLaunchKernelGGL((candidate_score_kernel<DD>), dim3((unsigned)((num_pairs + 255) / 256)), dim3(256), 0, s, m, reps, pair_row, pair_item,
                           num_pairs, out, nonfinite_flag);
    });
    return 1;
}

int launch_rep_rows(const float* H, const int* rep_row, uint32_t num_users, int d, int dl, float* out, hipStream_t s) {
    if (num_users == 0) return 0;
    hipLaunchKernelGGL(rep_rows_kernel, dim3((unsigned)(((uint64_t)num_users * dl + 255) / 256)), dim3(256), 0, s, H, rep_row, num_users, d, dl, out);
    return 1;
}

}  // namespace sbr
