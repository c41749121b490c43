/* sbr_device.h — device-side helpers shared by the kernel translation units (sbr_kernels.hip, sbr_steps.hip, sbr_catalogue.hip):
 * 16-byte loads and stores, the group all-reduce that realises the contract's dot order, the optimiser element update, the
 * sparse item-table update's one statement (LaneGroup, entry_source, RowSum, RowUpdate), the packed-f32 forms of the rational
 * tanh, and the SmallTail of a one-sequence step (header + loss accumulators + lagged loss figure + key ordering); and the
 * launchers' dispatches on d (DISPATCH_D) and on the owner kernels' device count (DISPATCH_NQ).
 * Everything here is __device__ __forceinline__: no symbol leaves a translation unit. */
#ifndef SBR_DEVICE_H
#define SBR_DEVICE_H

#include <hip/hip_runtime.h>

#include "../../include/sbr_hip.h"
#include "sbr_kernels.h"
#include "sbr_numerics.h"

namespace sbr {

typedef float f32x16 __attribute__((ext_vector_type(16))); /* the accumulators of v_mfma_f32_32x32x2_f32 */

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// the streaming (non-temporal, `nt`) forms, for rows a kernel touches once (which kernels use them: sbr_kernels.hip, sbr_catalogue.hip)
typedef float v4f_nt __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4s(const float* p) {
    const v4f_nt v = __builtin_nontemporal_load(reinterpret_cast<const v4f_nt*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st4s(float* p, float4 v) {
    v4f_nt t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
    __builtin_nontemporal_store(t, reinterpret_cast<v4f_nt*>(p));
}

// All-reduce over the L lanes of a group in the contract's tree order: p += p[lane ^ off] for off = L/2 ... 1
// (the dot order of sbr_numerics.h).  Every step is a cross-lane move inside the VALU — v_permlane32_swap /
// v_permlane16_swap (gfx950) for off = 32 / 16, DPP row rotate / shifts / quad permutes below — instead of a
// ds_bpermute round trip through the LDS crossbar per step (five dependent ones per dot product made the
// score kernel issue-bound).  Float addition is commutative, so "mine + theirs" has the same bits in both lanes.
typedef unsigned v2u __attribute__((ext_vector_type(2)));
template <int CTRL>
__device__ __forceinline__ float dpp_read(float p) {  // every lane has an in-row source for the controls used here
    return __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(p), CTRL, 0xF, 0xF, true));
}
template <int L>
__device__ __forceinline__ float group_allreduce(float p) {
    if constexpr (L >= 64) {
        const v2u r = __builtin_amdgcn_permlane32_swap(__float_as_uint(p), __float_as_uint(p), false, false);
        p = __uint_as_float(r.x) + __uint_as_float(r.y);
    }
    if constexpr (L >= 32) {
        const v2u r = __builtin_amdgcn_permlane16_swap(__float_as_uint(p), __float_as_uint(p), false, false);
        p = __uint_as_float(r.x) + __uint_as_float(r.y);
    }
    if constexpr (L >= 16) p = p + dpp_read<0x128>(p);  // row_ror:8 = lane ^ 8 inside a row of 16
    if constexpr (L >= 8) {  // lane ^ 4: banks 0, 2 of a row read 4 lanes up, banks 1, 3 read 4 lanes down
        unsigned t = __builtin_amdgcn_update_dpp(0u, __float_as_uint(p), 0x104, 0xF, 0x5, false);  // row_shl:4
        t = __builtin_amdgcn_update_dpp(t, __float_as_uint(p), 0x114, 0xF, 0xA, false);            // row_shr:4
        p = p + __uint_as_float(t);
    }
    if constexpr (L >= 4) p = p + dpp_read<0x4E>(p);  // quad_perm [2,3,0,1] = lane ^ 2
    if constexpr (L >= 2) p = p + dpp_read<0xB1>(p);  // quad_perm [1,0,3,2] = lane ^ 1
    return p;
}
// optimiser element update: Adagrad (acc = sum of squares) or Adam (acc = second moment, mom = first)
__device__ __forceinline__ void opt_update(const ModelView& m, float* w, float* acc, float* mom, float g) {
    if (m.optimizer == SBR_OPT_ADAM) sbr_adam(w, mom, acc, g, m.lr, m.l2, m.c1, m.c2);
    else sbr_adagrad(w, acc, g, m.lr, m.l2);
}

// ---- the sparse item-table update ("sparse row gradients"): THE statement of a row's gradient sum and of its one
// optimiser update.  Every kernel that reduces entries, combines chunk or device partials, or updates a table row does it through
// these types; the kernels differ only in how they get keys and rows in flight. ----

// The D/4-lane group of a wave that owns one unit (row, segment, chunk) at a time in the grid-stride kernels: lane `lg` of the
// group holds elements 4 lg .. 4 lg + 3 of the row.  A wave-uniform loop runs `for (i0 = wave_first; i0 < n; i0 += stride)` with
// the group's unit at i0 + grp; a per-group loop starts at first().
template <int D>
struct LaneGroup {
    static constexpr int L = D / 4, GPW = 64 / L;  // lanes per group, groups per wave
    int lg, grp;
    uint64_t wave_first, stride;
    // By default the whole grid's waves.  (Default ARGUMENTS, not a second constructor: they are evaluated in the kernel's own
    // body, where the compiler reads blockDim.x as the launch's uniform workgroup size; inside a helper function it reads the
    // possibly-partial last workgroup's size instead — a vector-memory load and a wait at the top of every kernel.)
    __device__ __forceinline__ LaneGroup(uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6,
                                         uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6)
        : lg((int)(threadIdx.x & 63) % L), grp((int)(threadIdx.x & 63) / L), wave_first(wave * GPW), stride(nwaves * GPW) {}
    __device__ __forceinline__ uint64_t first() const { return wave_first + grp; }
};

// An entry of the sparse update, decoded from its key's low word (3 x packed row + kind): kind 0 = the row's input (gradient row
// dX[r], scale 1, no bias term), 1 = its target (-coef[r] * H[r]), 2 = its negative (+coef[r] * H[r]); the last two carry the bias
// term, whose gradient is the scale itself.
struct EntrySource {
    uint32_t r, kind;
    __device__ __forceinline__ const float* rows(const float* dX, const float* H) const { return kind == 0 ? dX : H; }
    __device__ __forceinline__ float scale(float c) const { return kind == 0 ? 1.0f : (kind == 1 ? -c : c); }  // c = coef[r]
    __device__ __forceinline__ float scale_at(const float* coef) const { return kind == 0 ? 1.0f : scale(coef[r]); }  // no load for an input
    __device__ __forceinline__ bool carries_bias() const { return kind != 0; }
};
__device__ __forceinline__ EntrySource entry_source(uint32_t key_lo) { return EntrySource{key_lo / 3, key_lo % 3}; }

// A row's ordered gradient sum (4 elements per lane of the row's group, and the bias term).  Entries are added in key order,
// partials (chunks of SBR_SEG_CHUNK entries; devices) in their order; the FIRST term of either kind initialises the sum — it is
// not added to zero, so a first term of -0.0 stays -0.0 — and the bias term exists only where some entry carried one.
// The two "seen" flags (a term has arrived; a bias term has arrived) are kept as two booleans (RowSum: the sums over entries and
// chunks — scalar-register masks) or as the flag word of the exchange chunks and gradient lists, bit 0 = row touched, bit 1 =
// bias present (RowSumW: the owner kernels' sums over devices, whose inputs are such words).  The storage is the only
// difference; it is a template argument because either kind of kernel lost registers with the other's (seg_chunk_kernel, at
// its 80-register budget, spills with the word; owner_update_kernel<., 16> drops to one wave per SIMD with the booleans).
struct SeenBools {
    bool empty, hb;
    __device__ __forceinline__ SeenBools(bool any_, bool has_b_) : empty(!any_), hb(has_b_) {}
    __device__ __forceinline__ bool any() const { return !empty; }
    __device__ __forceinline__ bool has_b() const { return hb; }
};
struct SeenWord {
    uint32_t w;
    __device__ __forceinline__ SeenWord(bool any_, bool has_b_) : w((any_ ? 1u : 0u) | (has_b_ ? 2u : 0u)) {}
    __device__ __forceinline__ bool any() const { return (w & 1u) != 0; }
    __device__ __forceinline__ bool has_b() const { return (w & 2u) != 0; }
};
template <class Seen>
struct RowSumT {
    float4 g;
    float gb;
    Seen seen;
    __device__ __forceinline__ RowSumT() : g(make_float4(0.f, 0.f, 0.f, 0.f)), gb(0.0f), seen(false, false) {}
    __device__ __forceinline__ RowSumT(float4 g_, float gb_, bool any_, bool has_b_) : g(g_), gb(gb_), seen(any_, has_b_) {}
    __device__ __forceinline__ RowSumT(float4 g_, float gb_, uint32_t fl) : RowSumT(g_, gb_, (fl & 1u) != 0, (fl & 2u) != 0) {}
    __device__ __forceinline__ bool any() const { return seen.any(); }
    __device__ __forceinline__ bool has_b() const { return seen.has_b(); }
    __device__ __forceinline__ uint32_t flags() const { return (any() ? 1u : 0u) | (has_b() ? 2u : 0u); }
    __device__ __forceinline__ void add_entry(float4 v, float scale, bool carries_bias) { *this = with_entry(*this, v, scale, carries_bias); }
    template <class S2>
    __device__ __forceinline__ void add_partial(const RowSumT<S2>& o) { *this = with_partial(*this, o.g, o.gb, o.any(), o.has_b()); }

private:
    // (Both operations are stated on local copies that replace *this, with the first flag as "empty": with the members updated in
    // place, or with that flag's sense inverted, seg_chunk_kernel spilled two registers.)
    static __device__ __forceinline__ RowSumT with_entry(const RowSumT& s, float4 v, float scale, bool carries_bias) {
        float4 g = s.g;
        float gb = s.gb;
        bool empty = !s.any(), has_b = s.has_b();
        if (empty) {  // product, then add: no fused multiply-add
            g = make_float4(scale * v.x, scale * v.y, scale * v.z, scale * v.w);
            empty = false;
        } else {
            g.x = g.x + scale * v.x; g.y = g.y + scale * v.y;
            g.z = g.z + scale * v.z; g.w = g.w + scale * v.w;
        }
        if (carries_bias) {
            gb = has_b ? gb + scale : scale;
            has_b = true;
        }
        return RowSumT(g, gb, !empty, has_b);
    }
    static __device__ __forceinline__ RowSumT with_partial(const RowSumT& s, float4 v, float vb, bool o_any, bool o_has_b) {
        float4 g = s.g;
        float gb = s.gb;
        bool empty = !s.any(), has_b = s.has_b();
        if (o_any) {
            if (empty) g = v;
            else { g.x = g.x + v.x; g.y = g.y + v.y; g.z = g.z + v.z; g.w = g.w + v.w; }
            empty = false;
        }
        if (o_has_b) {
            gb = has_b ? gb + vb : vb;
            has_b = true;
        }
        return RowSumT(g, gb, !empty, has_b);
    }
};
typedef RowSumT<SeenBools> RowSum;
typedef RowSumT<SeenWord> RowSumW;

// how a row's parameter / optimiser-state quads travel: plain here; a kernel beside whose traffic they should not stay cached
// passes its own policy (sbr_kernels.hip: UpdAccess)
struct PlainAccess {
    static __device__ __forceinline__ float4 ld(const float* p) { return ld4(p); }
    static __device__ __forceinline__ void st(float* p, float4 v) { st4(p, v); }
};

// One optimiser update of an item-table row: the group's quads of E / Eacc / (Adam: Em) and, on the group's lane 0, the bias
// trio b / bacc / (bm).  load / apply / store are separate so that every kernel issues the loads where its schedule wants them
// (a value that is not loaded stays 0 and must not be stored).  ADAGRAD_ONLY: the caller's shape checks admit Adagrad only —
// no Adam code is generated.
template <int D, bool ADAGRAD_ONLY = false>
struct RowUpdate {
    float4 w, a, mo;
    float bv, ba, bmo;
    __device__ __forceinline__ RowUpdate() : w(make_float4(0.f, 0.f, 0.f, 0.f)), a(w), mo(w), bv(0.0f), ba(0.0f), bmo(0.0f) {}
    static __device__ __forceinline__ bool adam(const ModelView& m) { return !ADAGRAD_ONLY && m.optimizer == SBR_OPT_ADAM; }
    static __device__ __forceinline__ void element(const ModelView& m, float* wv, float* acc, float* mom, float g) {
        if constexpr (ADAGRAD_ONLY) sbr_adagrad(wv, acc, g, m.lr, m.l2);
        else opt_update(m, wv, acc, mom, g);
    }
    template <class Access = PlainAccess>
    __device__ __forceinline__ void load(const ModelView& m, uint64_t row, int lg) {
        w = Access::ld(m.E + row * D + 4 * lg);
        a = Access::ld(m.Eacc + row * D + 4 * lg);
        if (adam(m)) mo = ld4(m.Em + row * D + 4 * lg);
    }
    __device__ __forceinline__ void load_bias(const ModelView& m, uint64_t row) {
        bv = m.b[row]; ba = m.bacc[row];
        if (adam(m)) bmo = m.bm[row];
    }
    template <class Sum>
    __device__ __forceinline__ void apply(const ModelView& m, const Sum& s) {
        element(m, &w.x, &a.x, &mo.x, s.g.x);
        element(m, &w.y, &a.y, &mo.y, s.g.y);
        element(m, &w.z, &a.z, &mo.z, s.g.z);
        element(m, &w.w, &a.w, &mo.w, s.g.w);
    }
    template <class Sum>
    __device__ __forceinline__ void apply_bias(const ModelView& m, const Sum& s) { element(m, &bv, &ba, &bmo, s.gb); }
    template <class Access = PlainAccess>
    __device__ __forceinline__ void store(const ModelView& m, uint64_t row, int lg) const {
        Access::st(m.E + row * D + 4 * lg, w);
        Access::st(m.Eacc + row * D + 4 * lg, a);
        if (adam(m)) st4(m.Em + row * D + 4 * lg, mo);
    }
    __device__ __forceinline__ void store_bias(const ModelView& m, uint64_t row) const {
        m.b[row] = bv;
        m.bacc[row] = ba;
        if (adam(m)) m.bm[row] = bmo;
    }
    // the bias trio's whole read-modify-write on the group's lane 0, for the kernels that do not request it ahead
    template <class Sum>
    __device__ __forceinline__ void update_bias(const ModelView& m, uint64_t row, int lg, const Sum& s) {
        if (lg != 0 || !s.has_b()) return;
        load_bias(m, row);
        apply_bias(m, s);
        store_bias(m, row);
    }
};

// A kernel-argument pointer passed through an empty asm: the compiler can no longer hoist "pointer + per-lane
// offset" out of the time loop as a 64-bit VGPR pair that lives across it (those pairs were being spilled to
// scratch, and a scratch reload is a vector-memory operation that waits for EVERYTHING outstanding).
template <class T>
__device__ __forceinline__ T* launder(T* p) {
    typedef T __attribute__((address_space(1))) * global_ptr;  // keep the address space: a generic pointer would
    global_ptr g = (global_ptr)p;                              // turn every access into a flat_ operation
    asm volatile("" : "+s"(g));
    return (T*)g;
}

__device__ __forceinline__ float dot4(float4 x, float4 y) {
    float p = x.x * y.x;
    p = sbr_fma(x.y, y.y, p);
    p = sbr_fma(x.z, y.z, p);
    p = sbr_fma(x.w, y.w, p);
    return p;
}

typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f pk_fma(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ v2f pk_splat(float x) { return (v2f){x, x}; }
__device__ __forceinline__ void tanh_pq_x2(v2f x, v2f* p, v2f* q) {
    // sbr_tanh_pq's clamp (two comparison + select pairs; a NaN stays NaN) as one v_med3_f32 — which alone would turn a NaN
    // into -C — and one unordered comparison + select that puts the NaN back: the same bits for every input, fewer vector
    // instructions (which f32 MFMAs do not hide)
    const float cx = __builtin_amdgcn_fmed3f(x.x, -SBR_TANH_CLAMP, SBR_TANH_CLAMP), cy = __builtin_amdgcn_fmed3f(x.y, -SBR_TANH_CLAMP, SBR_TANH_CLAMP);
    x.x = x.x != x.x ? x.x : cx;
    x.y = x.y != x.y ? x.y : cy;
    const v2f x2 = x * x;
    v2f n = pk_splat(-2.76076847742355e-16f);
    n = pk_fma(n, x2, pk_splat(2.00018790482477e-13f));
    n = pk_fma(n, x2, pk_splat(-8.60467152213735e-11f));
    n = pk_fma(n, x2, pk_splat(5.12229709037114e-08f));
    n = pk_fma(n, x2, pk_splat(1.48572235717979e-05f));
    n = pk_fma(n, x2, pk_splat(6.37261928875436e-04f));
    n = pk_fma(n, x2, pk_splat(4.89352455891786e-03f));
    *p = n * x;
    v2f dq = pk_splat(1.19825839466702e-06f);
    dq = pk_fma(dq, x2, pk_splat(1.18534705686654e-04f));
    dq = pk_fma(dq, x2, pk_splat(2.26843463243900e-03f));
    dq = pk_fma(dq, x2, pk_splat(4.89352518554385e-03f));
    *q = dq;
}

// workgroup-scope release / acquire around a barrier: the phases of a one-workgroup step run hand their results to each other
// through this CU's vector cache / L2 and through LDS
__device__ __forceinline__ void phase_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---- the tail of a ONE-sequence step (SmallTail, sbr_kernels.h): one workgroup of 256 threads, after its score pass ----
// header + accumulators (block_header_kernel), the lagged loss figure of the one sequence (lagged_chain with B = 1: the node of
// its length is read, then takes the sequence's t-ascending loss sum), and the step's 3 R keys in (row, entry) order with the
// list of segment heads.  The keys are distinct (the entry number is their low word), so ranking every key among all of them
// IS the stable order by row that small_sort_kernel produces: integer work, identical output.
template <int NT>
__device__ __forceinline__ void small_tail(const MbView& mb, const BlockView& blk, const WorkView& w, const SmallTail& t, double lsum,
                                           unsigned int tsum) {
    constexpr int NMAX = 3 * SBR_SMALL_TAIL_MAX_ROWS, NW = NT / 64;
    __shared__ uint64_t ka[NMAX], kb[NMAX];
    __shared__ uint32_t s_cnt[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = mb.R;
    const uint32_t n = 3u * (uint32_t)R;
    /* the rows this workgroup's lanes have just written (ids, negatives, losses) are read by other lanes from here on */
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (wave == 0) {
        const int ns = mb.steps[0];
        /* the lagged loss figure (sbr_report.hip): the node of this length is read, then nodes 0 .. ns-1 take the sequence's
         * running sums — lane l holds the sum after term base + l */
        const float x = t.lag_state[1 + 2 * (ns - 1)];
        float sum = 0.0f;
        for (int base = 0; base < ns; base += 64) {
            const int tt = base + lane;
            const float v = tt < ns ? w.loss[mb.off[tt]] : 0.0f;
            const int cnt = ns - base < 64 ? ns - base : 64;
            float mine = 0.0f;
            for (int l = 0; l < cnt; ++l) {
                sum = sum + __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), l));
                mine = lane == l ? sum : mine;
            }
            if (tt < ns) t.lag_state[1 + 2 * tt] = mine;
        }
        if (lane == 0) {
            t.header[0] = (uint32_t)R;
            t.header[1] = tsum;
            t.header[2] = t.header[3] = 0;
            *reinterpret_cast<double*>(t.header + 4) = lsum;
            *reinterpret_cast<unsigned long long*>(t.header + 6) = (unsigned long long)R;
            if (t.loss_acc) {
                t.loss_acc[0] += lsum;
                t.loss_acc[1] += lsum;
                t.ex_acc[0] += (unsigned long long)R;
                t.ex_acc[1] += tsum;
                t.ex_acc[2] += (unsigned long long)R;
            }
            t.lag_state[0] = t.lag_state[0] + x;
        }
    }
    for (uint32_t e = tid; e < n; e += NT) {
        const uint32_t r = e / 3u, kind = e - 3u * r;
        const uint32_t* a = kind == 0 ? blk.in_idx : (kind == 1 ? blk.out_idx : blk.neg);
        ka[e] = ((uint64_t)a[r] << 32) | e;
    }
    __syncthreads();
    for (uint32_t e = tid; e < n; e += NT) {
        const uint64_t k = ka[e];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; ++j) rank += ka[j] < k ? 1u : 0u;
        kb[rank] = k;
    }
    __syncthreads();
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t base_heads = 0;
    for (uint32_t p0 = 0; p0 < n; p0 += NT) {  // workgroup-uniform trip count
        const uint32_t p = p0 + tid;
        const bool valid = p < n;
        const bool head = valid && (p == 0 || (uint32_t)(kb[p] >> 32) != (uint32_t)(kb[p - 1] >> 32));
        if (valid) t.keys_sorted[p] = kb[p];
        const uint64_t mm = __ballot(head);
        if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(mm);
        __syncthreads();
        uint32_t off = base_heads, total = 0;
#pragma unroll
        for (int w2 = 0; w2 < NW; ++w2) {
            if (w2 < wave) off += s_cnt[w2];
            total += s_cnt[w2];
        }
        if (head) t.head_pos[off + (uint32_t)__popcll(mm & lt)] = p;
        base_heads += total;
        __syncthreads();
    }
    if (tid == 0) {
        *t.nheads = base_heads;
        t.head_pos[base_heads] = n;
    }
}

}  // namespace sbr

/* host side: runs the statement list with constexpr int DD = d for the storage widths the kernels are built for */
#define DISPATCH_D(d, ...)                                         \
    switch (d) {                                                   \
        case 16: { constexpr int DD = 16; __VA_ARGS__; } break;    \
        case 32: { constexpr int DD = 32; __VA_ARGS__; } break;    \
        case 64: { constexpr int DD = 64; __VA_ARGS__; } break;    \
        case 128: { constexpr int DD = 128; __VA_ARGS__; } break;  \
        case 256: { constexpr int DD = 256; __VA_ARGS__; } break;  \
        default: break;                                            \
    }
/* host side: the owner kernels' instantiation for ndev devices (their requests are unrolled for NQ = 4 / 8 / 16): runs the
 * statement list with constexpr int NQ */
#define DISPATCH_NQ(ndev, ...)                                           \
    do {                                                                 \
        if ((ndev) <= 4) { constexpr int NQ = 4; __VA_ARGS__; }          \
        else if ((ndev) <= 8) { constexpr int NQ = 8; __VA_ARGS__; }     \
        else { constexpr int NQ = 16; __VA_ARGS__; }                     \
    } while (0)
#endif
