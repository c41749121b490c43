// sbr_rank_eligible.h — rank_targets under a restriction: a tag filter, an item set, a session store's seen items (included from
// sbr_catalogue.hip behind launch_rank_targets, inside namespace sbr: ItemTiles, tile_dots, chain_dot, slot_user, split_items and
// rank_targets_gemm_kernel are in scope).
//
// The contract (ELIGIBLE RANKS in include/sbr_hip.h): with M = unique(list) ∪ {items the masks forbid} ∪ (catalogue \ S) the ranks
// are those of rank_targets with the mask list M — m(i) = f32::MIN on M, else the score; rank(t) = #{i : m(i) >= m(t)}.  For a
// target with m(t) > MIN that is the number of scanned items (positions of `cat`: the catalogue, or the set's resident sub-table)
// that the masks allow, that are not in the list and that score >= m(t); for every other target it is the catalogue's num_items,
// because every finite score is >= MIN.  Nothing counts how many items the restriction removes.
//
//   rank_eligible_prepare_kernel : rank_targets_prepare_kernel, with the target's position in the set by a binary search of the set's
//                                  ascending ids, its score from the scanned table, and MIN for a target outside the set, forbidden by
//                                  the masks or in the list
//   rank_eligible_gemm_kernel    : rank_targets_gemm_kernel with topk_gemm_kernel's tag test ahead of both compares (the scan without a
//                                  filter — a set or a seen list alone — is rank_targets_gemm_kernel itself, over `cat`)
//   rank_eligible_finish_kernel  : rank_targets_finish_kernel, subtracting a list entry only where the scan counted it (a real
//                                  position, the first of its repeats, its tag word allowed) and answering num_items for a threshold
//                                  <= MIN
//
// Lists are what the top-k scans take: per user a non-decreasing segment of positions of `cat`, repeats and a 0xFFFFFFFF tail
// allowed (an uploaded CSR, session_seen_lists_kernel's merge, subset_positions_kernel's output).  Counts are integers joined by
// integer atomics: no result depends on dispatch order, the item-range split or the host's chunks.

/* whether user masks (any_of, none_of) allow an item with tag word `tag`: TagFilter's rule */
__device__ __forceinline__ bool rank_tag_allowed(uint32_t tag, uint32_t any_of, uint32_t none_of) {
    return (tag & none_of) == 0u && (any_of == 0u || (tag & any_of) != 0u);
}

/* One thread per (scan-user, slot j < TM), as rank_targets_prepare_kernel: threshold, descending order, tmin / tmin2, zeroed counts. */
template <int D, int TM>
__global__ __launch_bounds__(256) void rank_eligible_prepare_kernel(ModelView cat, const float* reps, RankEligible re) {
    __shared__ float tl[256];
    const int tid = threadIdx.x;
    const int j = tid % TM;
    const uint32_t s = blockIdx.x * (256 / TM) + tid / TM;
    uint32_t e = 0, n = 0;
    float t = -INFINITY;
    if (s < re.num_su) {
        e = re.sptr[s] + j;
        n = re.sptr[s + 1] - re.sptr[s];
    }
    const bool real = (uint32_t)j < n;
    if (real) {
        const uint32_t u = re.su_user[s];
        uint32_t ti = re.tgt_items[e]; /* a catalogue id; from here on a position of cat */
        bool masked = false;
        if (re.set_ids) {
            uint32_t lo = 0, hi = cat.num_items;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (re.set_ids[mid] < ti) lo = mid + 1; else hi = mid;
            }
            masked = !(lo < cat.num_items && re.set_ids[lo] == ti);
            ti = lo;
        }
        if (!masked && re.f.tags) masked = !rank_tag_allowed(re.f.tags[ti], re.f.any_of[u], re.f.none_of[u]);
        if (!masked && re.list_ptr) { /* the lower bound of the position in the user's non-decreasing segment */
            uint64_t lo = re.list_ptr[u], hi = re.list_ptr[u + 1];
            while (lo < hi) {
                const uint64_t mid = (lo + hi) >> 1;
                if (re.list_items[mid] < ti) lo = mid + 1; else hi = mid;
            }
            masked = lo < re.list_ptr[u + 1] && re.list_items[lo] == ti;
        }
        t = masked ? SBR_F32_MIN : cat.b[ti] + chain_dot<D>(reps + (size_t)re.rep_row[s] * D, cat.E + (size_t)ti * D);
    }
    tl[tid] = t;
    __syncthreads();
    if (s >= re.num_su) return;
    uint32_t p = (uint32_t)j; /* the padding keeps its slot (>= n) */
    if (real) {
        p = 0;
        const float* mine = &tl[tid - j];
        for (uint32_t o = 0; o < n; ++o) {
            const float x = mine[o];
            p += (x > t || (x == t && o < (uint32_t)j)) ? 1u : 0u;
        }
        re.ts[e] = t;
        re.pos[e] = p;
        if (p == n - 1) re.tmin[s] = t;
        if (p + 2 == n) re.tmin2[s] = t;
    }
    if (j == 0) {
        if (n == 1) re.tmin2[s] = INFINITY;
        re.totals[s] = 0;
    }
    re.th[(size_t)s * TM + p] = t;
    re.buckets[(size_t)s * TM + j] = 0;
}

/* rank_targets_gemm_kernel with the tag filter: the tile's 32 tag words come in beside its biases (Ts) and the 128 scan-users' mask
 * words sit in LDS by slot (anyS / anyZ / noneS, as topk_gemm_kernel<.., TagFilter>'s: 1 792 more bytes, 52 480 at d <= 128 — three
 * workgroups per CU still).  The non-finite test sees every scanned score; an item the masks do not allow is then neither counted
 * against the lowest threshold nor searched. */
template <int D, int TM>
__global__ __launch_bounds__(256, D <= 128 ? 3 : 2) void rank_eligible_gemm_kernel(ModelView cat, const float* reps, RankEligible re,
                                                                                  uint32_t items_per_group) {
    __shared__ float Es[2][32 * ItemTiles<D>::LDE];
    __shared__ float Bs[2][32];
    __shared__ uint32_t Ts[2][32];
    __shared__ float Tmin[128];      /* by slot (slot_user) */
    __shared__ float Tmin2[128];
    __shared__ __align__(16) uint32_t anyS[128];
    __shared__ __align__(16) uint32_t anyZ[128]; /* 1 where the user's any_of is 0 (every tag passes it), else 0 */
    __shared__ __align__(16) uint32_t noneS[128];
    __shared__ float Th[128 * TM];
    __shared__ uint32_t Hist[128 * TM];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int l31 = lane & 31;
    const int hh = lane >> 5;
    const uint32_t num_su = re.num_su;
    const uint32_t u0 = blockIdx.x * 128 + wave * 32;
    float a[D / 2];
    load_user_fragments<D>(a, reps, re.rep_row, num_su, u0);
    if (tid < 128) {
        const uint32_t u = blockIdx.x * 128 + (uint32_t)slot_user(tid);
        const bool is = u < num_su;
        Tmin[tid] = is ? re.tmin[u] : INFINITY; /* no scan-user: nothing passes */
        Tmin2[tid] = is ? re.tmin2[u] : INFINITY;
        const uint32_t lu = is ? re.su_user[u] : 0u;
        const uint32_t any = is ? re.f.any_of[lu] : 0u;
        anyS[tid] = any;
        anyZ[tid] = any == 0u ? 1u : 0u;
        noneS[tid] = is ? re.f.none_of[lu] : 0u;
    }
    uint32_t cnt2[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) cnt2[q] = 0;
    for (int idx = tid; idx < 128 * TM; idx += 256) {
        const uint32_t u = blockIdx.x * 128 + (uint32_t)slot_user(idx / TM);
        Th[idx] = u < num_su ? re.th[(size_t)u * TM + idx % TM] : -INFINITY;
        Hist[idx] = 0;
    }
    bool bad = false;
    ItemTiles<D> tiles(cat, items_per_group);
    const int ntiles = tiles.ntiles;
    if (ntiles > 0) {
        tiles.fetch(cat, 0);
        tiles.stage(Es[0], Bs[0]);
        tiles.fetch_tags(re.f.tags, 0);
        tiles.stage_tags(Ts[0]);
    }
    __syncthreads();
    const int pbase = wave * 32 + hh * 16;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < ntiles) {
            tiles.fetch(cat, tile + 1);
            tiles.fetch_tags(re.f.tags, tile + 1);
        }
        const f32x16 acc = tile_dots<D>(a, Es[buf]);
        const float bias = Bs[buf][l31];
        const uint32_t tag = Ts[buf][l31];
        const bool item_ok = tiles.i_begin + (uint32_t)tile * 32 + l31 < tiles.i_end;
        uint32_t pass = 0; /* accumulator registers q whose score reaches the slot's second lowest threshold */
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const float4 t4 = ld4(&Tmin[pbase + 4 * q4]);
            const float4 s4 = ld4(&Tmin2[pbase + 4 * q4]);
            const uint4 a4 = *reinterpret_cast<const uint4*>(&anyS[pbase + 4 * q4]);
            const uint4 z4 = *reinterpret_cast<const uint4*>(&anyZ[pbase + 4 * q4]);
            const uint4 n4 = *reinterpret_cast<const uint4*>(&noneS[pbase + 4 * q4]);
            const float tq[4] = {t4.x, t4.y, t4.z, t4.w};
            const float sq[4] = {s4.x, s4.y, s4.z, s4.w};
            const uint32_t any[4] = {a4.x, a4.y, a4.z, a4.w};
            const uint32_t anyz[4] = {z4.x, z4.y, z4.z, z4.w};
            const uint32_t none[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = 4 * q4 + j;
                const float sc = bias + acc[q];
                if (item_ok) {
                    if (!(sc - sc == 0.0f)) bad = true;
                    /* `|`, not `||`: one exec-mask region per user, as topk_gemm_kernel's test */
                    const uint32_t hit = (tag & none[j]) != 0u ? 1u : 0u;
                    const uint32_t miss = ((tag & any[j]) | anyz[j]) == 0u ? 1u : 0u;
                    if ((hit | miss) == 0u) {
                        if (sc >= tq[j]) cnt2[q >> 1] += (q & 1) ? 0x10000u : 1u;
                        if (sc >= sq[j]) pass |= 1u << q;
                    }
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
        if (tile + 1 < ntiles) {
            tiles.stage(Es[buf ^ 1], Bs[buf ^ 1]);
            tiles.stage_tags(Ts[buf ^ 1]);
        }
        __syncthreads();
    }
    // per-slot totals: sum over the 32 item lanes of each half-wave
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        int c = (int)((cnt2[q >> 1] >> ((q & 1) * 16)) & 0xFFFFu);
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
        const uint32_t u = acc_user(u0, q, hh);
        if (l31 == 0 && u < num_su && c) atomicAdd(&re.totals[u], (uint32_t)c);
    }
    // the workgroup's buckets join the other item ranges'
    for (int idx = tid; idx < 128 * TM; idx += 256) {
        const uint32_t u = blockIdx.x * 128 + (uint32_t)slot_user(idx / TM);
        const uint32_t c = Hist[idx];
        if (u < num_su && c) atomicAdd(&re.buckets[(size_t)u * TM + idx % TM], c);
    }
    if (__any(bad) && lane == 0) atomicOr(re.nonfinite_flag, 1u);
}

/* One wave per scan-user.  The scan counted every allowed position that scores >= the threshold; a list entry leaves that count if
 * the scan saw it — a real position (not the 0xFFFFFFFF tail), counted once however often it repeats, its tag word allowed.  Its
 * masked value MIN counts against no threshold above MIN, and a target whose threshold is <= MIN has every item of the CATALOGUE
 * at or above it: re.num_items, the same through a set. */
template <int D, int TM>
__global__ __launch_bounds__(64) void rank_eligible_finish_kernel(ModelView cat, const float* reps, RankEligible re) {
    __shared__ float tl[TM];
    __shared__ int delta[TM];
    const uint32_t s = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t e0 = re.sptr[s];
    const int n = (int)(re.sptr[s + 1] - e0);
    if (lane < TM) tl[lane] = lane < n ? re.ts[e0 + lane] : INFINITY;
    __syncthreads();
    int cnt[TM];
#pragma unroll
    for (int r = 0; r < TM; ++r) cnt[r] = 0;
    if (re.list_ptr) {
        const uint32_t u = re.su_user[s];
        const float* h = reps + (size_t)re.rep_row[s] * D;
        const uint64_t l0 = re.list_ptr[u], l1 = re.list_ptr[u + 1];
        for (uint64_t e = l0 + lane; e < l1; e += 64) {
            const uint32_t i = re.list_items[e];
            if (i >= cat.num_items || (e > l0 && re.list_items[e - 1] == i)) continue;
            if (re.f.tags && !rank_tag_allowed(re.f.tags[i], re.f.any_of[u], re.f.none_of[u])) continue;
            const float sc = cat.b[i] + chain_dot<D>(h, cat.E + (size_t)i * D);
#pragma unroll
            for (int r = 0; r < TM; ++r) cnt[r] -= sc >= tl[r] ? 1 : 0;
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
        const uint32_t p = re.pos[e0 + lane];
        uint32_t rank = 0;
        if (p + 1 == (uint32_t)n) rank = re.totals[s];
        else
            for (uint32_t j = 0; j <= p; ++j) rank += re.buckets[(size_t)s * TM + j];
        rank += (uint32_t)delta[lane]; /* two's complement: adds a negative delta */
        re.ranks[e0 + lane] = tl[lane] <= SBR_F32_MIN ? re.num_items : rank;
    }
}

int launch_rank_eligible(const ModelView& cat, const float* reps, const RankEligible& re, hipStream_t s) {
    if (re.num_su == 0 || cat.num_items == 0) return 0;
    const uint32_t utiles = (re.num_su + 127) / 128;
    // item ranges as launch_rank_targets', and its limit: 16-bit lane counters, fewer than 65 536 tiles per range
    uint32_t per = 0;
    const uint32_t groups = split_items(cat.num_items, wanted_groups((768u * 6u + utiles - 1) / utiles), UINT32_MAX, 65535u * 32u, &per);
    DISPATCH_D(cat.d, {
        constexpr int TM = DD <= 128 ? 16 : 8; /* = rank_targets_tmax(DD) */
        hipLaunchKernelGGL((rank_eligible_prepare_kernel<DD, TM>), dim3((re.num_su + 256 / TM - 1) / (256 / TM)), dim3(256), 0, s, cat, reps, re);
        if (re.f.tags)
            hipLaunchKernelGGL((rank_eligible_gemm_kernel<DD, TM>), dim3(utiles, groups), dim3(256), 0, s, cat, reps, re, per);
        else
            hipLaunchKernelGGL((rank_targets_gemm_kernel<DD, TM>), dim3(utiles, groups), dim3(256), 0, s, cat, reps, re.rep_row, re.num_su, re.th,
                               re.tmin, re.tmin2, per, re.buckets, re.totals, re.nonfinite_flag);
        hipLaunchKernelGGL((rank_eligible_finish_kernel<DD, TM>), dim3(re.num_su), dim3(64), 0, s, cat, reps, re);
    });
    return 3;
}
