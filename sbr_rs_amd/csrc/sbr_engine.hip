// sbr_engine.hip — host side of libsbr_hip.so: the C-ABI of include/sbr_hip.h.
//
// Owns device memory (parameters resident in HBM for the life of the model), restates the
// reference's training driver (fit_sequence_model, /root/reference/src/models/sequence_model.rs:
// 70-178) as host-side index work (chunking, shuffles, partitioning, packing) and drives the
// gfx950 kernels of sbr_kernels.hip and its neighbours: a training step over the model's main stream and the fit plan's side streams
// (side, sorter, copier, exchange), joined by events; the prediction side (sbr_catalogue.hip, sbr_sessions.hip) on the
// main stream alone.  There is no CPU compute fallback: without a HIP device every entry point returns SBR_ERR_NO_DEVICE.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/sbr_hip.h"
#include "sbr_kernels.h"
#include "sbr_numerics.h"
#include "sbr_replay_plan.h"

namespace {

#define HIPCHK(expr)                                                                  \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) {                                                       \
            std::fprintf(stderr, "[sbr_hip] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return _e == hipErrorOutOfMemory ? SBR_ERR_OUT_OF_MEMORY                  \
                   : (_e == hipErrorNoDevice || _e == hipErrorInvalidDevice) ? SBR_ERR_NO_DEVICE : SBR_ERR_HIP; \
        }                                                                             \
    } while (0)

#define SBRCHK(expr)                     \
    do {                                 \
        sbr_status _s = (expr);          \
        if (_s != SBR_OK) return _s;     \
    } while (0)

/* The poisoned-scratch test hook: SBR_TEST_POISON=<byte 1..255>, read each time memory is handed out.  Every
 * block of ScratchCache::get (device and pinned host, hit or fresh) and the part of the serving arena a carve uses are filled
 * with that byte first, so a kernel that relies on zeros, or on what the last call left, loses bit-parity with the oracle
 * (tests/test_poisoned_scratch_gpu.py).  0 = off (unset, 0 or malformed): one getenv, nothing else. */
int test_poison_byte() {
    const char* e = std::getenv("SBR_TEST_POISON");
    if (!e || !*e) return 0;
    char* after = nullptr;
    const unsigned long v = std::strtoul(e, &after, 0);
    return (*after == 0 && v >= 1 && v <= 255) ? (int)v : 0;
}

/* The guarded-scratch test hook: SBR_TEST_GUARD=<KiB>, read each time memory is handed out.  Every block of
 * ScratchCache::get and every take of the serving arena gets a band of G = KiB x 1024 bytes of kGuardByte behind it — from the first
 * byte past the REQUESTED size, through the alignment padding and the unused part of a cache hit — and one in front (of a block;
 * of the first take of a carve).  The bands are compared with kGuardByte when a block is given back, at the head of the next carve
 * and on sbr_test_guard_report: a store past its buffer is a count and a record, never an abort
 * (tests/test_guarded_scratch_gpu.py).  0 = off (unset, 0 or malformed): one getenv, nothing else. */
constexpr int kGuardByte = 0xA5; /* none of the poison patterns 0xFF / 0x7F / 0x80, and no zero */
size_t test_guard_bytes() {
    const char* e = std::getenv("SBR_TEST_GUARD");
    if (!e || !*e) return 0;
    char* after = nullptr;
    const unsigned long v = std::strtoul(e, &after, 10);
    return (*after == 0 && v >= 1 && v <= (1ul << 20)) ? (size_t)v << 10 : 0;
}

/* What the guard checks found since sbr_test_guard_report last read them (process-wide), and the staging buffer of a check. */
struct GuardState {
    std::mutex mu;
    sbr_guard_report r = {};
    uint64_t allocs = 0; /* guarded blocks handed out since the last report: the ordinal of the next one */
    std::vector<uint8_t> staging;
};
GuardState& guard_state() {
    static GuardState* g = new GuardState;
    return *g;
}

/* One band [band, band + n) — pinned host memory, or device memory whose streams are drained — against kGuardByte.  offset0: the
 * position of the band's first byte as the report states it (+1: the first byte past the request; -n: n bytes before its start).
 * A changed band is counted once: it is filled again. */
void guard_check_band(uint8_t* band, size_t n, bool host, uint64_t where, uint64_t ordinal, uint64_t requested, int64_t offset0) {
    if (!n) return;
    GuardState& gs = guard_state();
    std::lock_guard<std::mutex> g(gs.mu);
    const uint8_t* src = band;
    if (!host) {
        if (gs.staging.size() < n) gs.staging.resize(n);
        if (hipMemcpy(gs.staging.data(), band, n, hipMemcpyDeviceToHost) != hipSuccess) return;
        src = gs.staging.data();
    }
    gs.r.bytes += n;
    uint64_t word;
    std::memset(&word, kGuardByte, 8);
    size_t first = n, changed = 0, i = 0;
    while (i < n) {
        uint64_t w;
        if (i + 8 <= n && (std::memcpy(&w, src + i, 8), w == word)) { i += 8; continue; }
        const size_t end = std::min(n, i + 8);
        for (; i < end; ++i)
            if (src[i] != (uint8_t)kGuardByte) { if (first == n) first = i; ++changed; }
    }
    if (!changed) return;
    gs.r.violations += 1;
    if (gs.r.where == SBR_GUARD_NONE) {
        gs.r.where = where; gs.r.ordinal = ordinal; gs.r.requested = requested;
        gs.r.offset = offset0 + (int64_t)first; gs.r.changed = changed;
    }
    if (host) std::memset(band, kGuardByte, n);
    else if (hipMemset(band, kGuardByte, n) == hipSuccess) (void)hipDeviceSynchronize();
}

/* Scratch of a fit call recycled across calls.  The reference's own bench re-fits one model in a loop (benches/benchmark.rs:40-42:
 * 10 000 interactions, three epochs per call): ~40 hipMalloc + 10 hipHostMalloc at sbr_fit_begin and as many frees at the end
 * cost 4-18 ms per call there — more than the call's kernels.  Blocks up to 64 MiB go back to this process-wide cache (768 MiB at
 * most, per kind) instead of the driver and are handed out again to requests of at most twice... the same size class; anything
 * larger takes the driver's path as before.  A block is cached only after the streams that used it were synchronised
 * (sbr_fit_plan_destroy, sbr_model_destroy), and nothing relies on fresh memory being zero.  sbr_release_cached_memory() empties it.
 * Under SBR_TEST_GUARD a block is allocated with `guard` bytes in front of p and behind p + bytes, is handed out only to requests
 * made under the same guard size, and is `live` whatever its size, so that put finds its bands. */
struct ScratchCache {
    static constexpr size_t kMaxBlock = 64ull << 20, kMaxTotal = 768ull << 20;
    struct Blk { void* p; size_t bytes; int device; bool host; size_t guard = 0, req = 0; uint64_t ordinal = 0; };
    std::mutex mu;
    std::vector<Blk> idle;
    std::unordered_map<void*, Blk> live;
    size_t cached[2] = {0, 0}; /* device, pinned host */
    static bool enabled() { return true; }
    hipError_t get(void** out, size_t bytes, bool host) {
        const size_t guard = test_guard_bytes();
        size_t stored = 0;
        const hipError_t e = get_block(out, bytes, host, &stored, guard);
        if (e != hipSuccess) return e;
        const int poison = test_poison_byte();
        if (!poison && !guard) return hipSuccess;
        uint8_t* p = static_cast<uint8_t*>(*out);
        if (host) {
            if (poison) std::memset(p, poison, stored);
            if (guard) { std::memset(p - guard, kGuardByte, guard); std::memset(p + bytes, kGuardByte, stored - bytes + guard); }
        } else { /* the model's streams are non-blocking: a null-stream memset is ordered against nothing without the sync */
            hipError_t pe = poison ? hipMemset(p, poison, stored) : hipSuccess;
            if (guard && pe == hipSuccess) pe = hipMemset(p - guard, kGuardByte, guard);
            if (guard && pe == hipSuccess) pe = hipMemset(p + bytes, kGuardByte, stored - bytes + guard);
            if (pe == hipSuccess) pe = hipDeviceSynchronize();
            if (pe != hipSuccess) { put(*out, host); *out = nullptr; return pe; }
        }
        return hipSuccess;
    }
    /* *stored = the size of the block handed out: a cache hit may be up to twice the request */
    hipError_t get_block(void** out, size_t bytes, bool host, size_t* stored, size_t guard) {
        *out = nullptr;
        const size_t req = bytes;
        bytes = (bytes + 255) & ~(size_t)255;
        int device = 0;
        if (!host) (void)hipGetDevice(&device);
        if (enabled() && bytes <= kMaxBlock) {
            std::lock_guard<std::mutex> g(mu);
            size_t best = idle.size();
            for (size_t i = 0; i < idle.size(); ++i) {
                const Blk& b = idle[i];
                if (b.host != host || (!host && b.device != device) || b.bytes < bytes || b.bytes > 2 * bytes + 4096 || b.guard != guard) continue;
                if (best == idle.size() || b.bytes < idle[best].bytes) best = i;
            }
            if (best != idle.size()) {
                Blk b = idle[best];
                idle[best] = idle.back();
                idle.pop_back();
                cached[host] -= b.bytes;
                if (guard) { b.req = req; b.ordinal = next_ordinal(); }
                live[b.p] = b;
                *out = b.p;
                *stored = b.bytes;
                return hipSuccess;
            }
        }
        const size_t total = bytes + 2 * guard;
        bool retried = false;
        hipError_t e = host ? hipHostMalloc(out, total, hipHostMallocDefault) : hipMalloc(out, total);
        if (e != hipSuccess) {
            bool have_cached;
            {
                std::lock_guard<std::mutex> g(mu);
                have_cached = cached[0] + cached[1] != 0;
            }
            if (e != hipErrorOutOfMemory || !have_cached) return e;
            trim(); /* give the cache back and try once more */
            retried = true;
            e = host ? hipHostMalloc(out, total, hipHostMallocDefault) : hipMalloc(out, total);
            if (e != hipSuccess) return e;
        }
        *stored = bytes;
        *out = static_cast<uint8_t*>(*out) + guard;
        if (enabled() && ((bytes <= kMaxBlock && !retried) || guard)) {
            std::lock_guard<std::mutex> g(mu);
            Blk b{*out, bytes, device, host};
            if (guard) { b.guard = guard; b.req = req; b.ordinal = next_ordinal(); }
            live[*out] = b;
        }
        return hipSuccess;
    }
    static uint64_t next_ordinal() {
        GuardState& gs = guard_state();
        std::lock_guard<std::mutex> g(gs.mu);
        return gs.allocs++;
    }
    /* both bands of a live guarded block; the streams that used it are drained */
    static void check(const Blk& b) {
        uint8_t* p = static_cast<uint8_t*>(b.p);
        const uint64_t where = b.host ? SBR_GUARD_PINNED_BLOCK : SBR_GUARD_DEVICE_BLOCK;
        {
            GuardState& gs = guard_state();
            std::lock_guard<std::mutex> g(gs.mu);
            gs.r.blocks += 1;
        }
        guard_check_band(p - b.guard, b.guard, b.host, where, b.ordinal, b.req, -(int64_t)b.guard);
        guard_check_band(p + b.req, b.bytes - b.req + b.guard, b.host, where, b.ordinal, b.req, 1);
    }
    static void release(const Blk& b) {
        void* raw = static_cast<uint8_t*>(b.p) - b.guard;
        if (b.host) (void)hipHostFree(raw); else (void)hipFree(raw);
    }
    void put(void* p, bool host) {
        if (!p) return;
        Blk b{p, 0, 0, host};
        {
            std::lock_guard<std::mutex> g(mu);
            auto it = live.find(p);
            if (it != live.end()) {
                b = it->second;
                live.erase(it);
            }
        }
        if (b.guard) check(b);
        if (b.bytes && b.bytes <= kMaxBlock && b.host == host) {
            std::lock_guard<std::mutex> g(mu);
            if (cached[host] + b.bytes <= kMaxTotal) {
                idle.push_back(b);
                cached[host] += b.bytes;
                return;
            }
        }
        b.host = host;
        release(b);
    }
    void check_live() {
        std::vector<Blk> blocks;
        {
            std::lock_guard<std::mutex> g(mu);
            for (const auto& kv : live) if (kv.second.guard) blocks.push_back(kv.second);
        }
        for (const Blk& b : blocks) check(b);
    }
    void trim() {
        std::vector<Blk> drop;
        {
            std::lock_guard<std::mutex> g(mu);
            drop.swap(idle);
            cached[0] = cached[1] = 0;
        }
        for (const Blk& b : drop) release(b);
    }
};
ScratchCache& scratch_cache() {
    static ScratchCache* c = new ScratchCache; /* never destroyed: the HIP runtime may be gone before static destructors run */
    return *c;
}

template <typename T>
sbr_status dmalloc(T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    HIPCHK(scratch_cache().get(reinterpret_cast<void**>(p), count * sizeof(T), false));
    return SBR_OK;
}
inline void dfree(void* p) { scratch_cache().put(p, false); }
template <typename T>
hipError_t hmalloc(T** p, size_t bytes) { return scratch_cache().get(reinterpret_cast<void**>(p), bytes, true); }
inline void hfree(void* p) { scratch_cache().put(p, true); }

int dim_ok(uint32_t d) { return d == 16 || d == 32 || d == 64 || d == 128 || d == 256; }

/* rows a replica's item-table arrays are allocated for: num_devices x S, S = ceil(num_items / num_devices) (one device: num_items) */
uint64_t table_rows_allocated(const sbr_hparams* hp) {
    const uint64_t n = hp->num_devices ? hp->num_devices : 1, I = hp->num_items;
    return n > 1 ? n * ((I + n - 1) / n) : I;
}

/* Storage width of an embedding_dim: the kernels exist for 16 / 32 / 64 / 128 / 256 columns; any other
 * embedding_dim <= 256 (the reference's builder takes any usize, lstm.rs:86-89) is stored in the next width up
 * with the extra columns — of the embeddings, of every weight row and column, of alpha — ZERO.  That is a fixed
 * point of the training step: a zero input/hidden unit with zero weights has z = 0, c = 0, h = 0 in the forward
 * pass, receives a zero gradient from the loss (its embedding columns are zero) and from the recurrence (its
 * weights are zero), so Adagrad/Adam leave it at zero — the padded model IS the embedding_dim-wide model, with
 * +0 terms in its sums.  0 = unsupported. */
int storage_dim(uint32_t e) {
    for (uint32_t p = 16; p <= 256; p *= 2)
        if (e >= 1 && e <= p) return (int)p;
    return 0;
}

/* ≙ wyrm nn::lstm::Parameters::new as recalled: four [(hidden+input) x hidden]
 * xavier_normal matrices (std 1/sqrt(rows)) drawn one after the other — forget, update gate, update
 * value, output gate — rows = hidden part first; a coupled layer draws all four and ignores the update
 * gate's.  Engine layout: W[2d][ng*d], rows [x ; h], column blocks i,f,g,o (coupled: f,g,o). */
void draw_lstm_weights(sbr_xorshift* rng, int dl, int d, int ng, std::vector<float>* w) { /* dl = embedding_dim, d = storage width */
    const double std_w = 1.0 / std::sqrt((double)(2 * dl));
    const int nz = ng * d;
    w->assign((size_t)2 * d * nz, 0.0f);
    for (int gate = 0; gate < 4; ++gate) {
        const int block = ng == 4 ? (gate == 0 ? 1 : gate == 1 ? 0 : gate) : (gate == 0 ? 0 : gate == 1 ? -1 : gate - 1);
        for (int row = 0; row < 2 * dl; ++row) {
            const int k = row < dl ? d + row : row - dl;
            for (int u = 0; u < dl; ++u) {
                const float v = sbr_rand_normal_f32(rng, 0.0, std_w);
                if (block >= 0) (*w)[(size_t)k * nz + block * d + u] = v;
            }
        }
    }
}

#ifndef SBR_PACK_THREADS
#define SBR_PACK_THREADS 8 /* host threads that fill a large minibatch's packed index arrays (build_epoch) */
#endif
struct TimingPair { hipEvent_t a, b; int family; uint64_t launches; };

}  // namespace

/* hipMemImportFromShareableHandle takes the POSIX file descriptor in its `void* osHandle` argument, and
 * the two HIP runtimes this library meets disagree on how: the runtime PyTorch bundles (ROCm 7.0) reads an
 * int THROUGH the pointer, the system runtime (ROCm 7.2) takes the descriptor VALUE cast to a pointer.
 * Passing a pointer is safe on both (7.2 rejects it with hipErrorInvalidValue), passing the value crashes
 * 7.0 — so: pointer first, value only after a clean rejection. */
static hipError_t import_shareable_fd(hipMemGenericAllocationHandle_t* handle, int fd) {
    int fd_copy = fd;
    hipError_t e = hipMemImportFromShareableHandle(handle, &fd_copy, hipMemHandleTypePosixFileDescriptor);
    if (e == hipSuccess) return e;
    (void)hipGetLastError();
    return hipMemImportFromShareableHandle(handle, reinterpret_cast<void*>(static_cast<uintptr_t>(fd)), hipMemHandleTypePosixFileDescriptor);
}

/* A device buffer made of one HIP virtual-memory allocation, so that it can be handed to another process
 * as a file descriptor (hipMemExportToShareableHandle) and mapped there. */
struct VmmBuf {
    void* ptr = nullptr;
    size_t bytes = 0;
    hipMemGenericAllocationHandle_t h{};
    bool have = false;

    static size_t granularity(int device) {
        hipMemAllocationProp prop = {};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = device;
        prop.requestedHandleTypes = hipMemHandleTypePosixFileDescriptor;
        size_t g = 0;
        if (hipMemGetAllocationGranularity(&g, &prop, hipMemAllocationGranularityRecommended) != hipSuccess) return 0;
        return g;
    }
    sbr_status map_access(int device) {
        if (hipMemAddressReserve(&ptr, bytes, 0, nullptr, 0) != hipSuccess) { ptr = nullptr; return SBR_ERR_OUT_OF_MEMORY; }
        if (hipMemMap(ptr, bytes, 0, h, 0) != hipSuccess) return SBR_ERR_HIP;
        hipMemAccessDesc acc = {};
        acc.location.type = hipMemLocationTypeDevice;
        acc.location.id = device;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        if (hipMemSetAccess(ptr, bytes, &acc, 1) != hipSuccess) return SBR_ERR_UNSUPPORTED;
        return SBR_OK;
    }
    sbr_status alloc(size_t want, int device) {
        const size_t g = granularity(device);
        if (!g) return SBR_ERR_UNSUPPORTED;
        bytes = (want + g - 1) / g * g;
        hipMemAllocationProp prop = {};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = device;
        prop.requestedHandleTypes = hipMemHandleTypePosixFileDescriptor;
        if (hipMemCreate(&h, bytes, &prop, 0) != hipSuccess) return SBR_ERR_OUT_OF_MEMORY;
        have = true;
        return map_access(device);
    }
    sbr_status export_fd(int* fd) const {
        if (!have) return SBR_ERR_INVALID_ARGUMENT;
        if (hipMemExportToShareableHandle(fd, h, hipMemHandleTypePosixFileDescriptor, 0) != hipSuccess) return SBR_ERR_HIP;
        return SBR_OK;
    }
    sbr_status import_fd(int fd, size_t nbytes, int device) {
        if (import_shareable_fd(&h, fd) != hipSuccess) return SBR_ERR_HIP;
        have = true;
        bytes = nbytes;
        return map_access(device);
    }
    void release() {
        if (ptr) { (void)hipMemUnmap(ptr, bytes); (void)hipMemAddressFree(ptr, bytes); ptr = nullptr; }
        if (have) { (void)hipMemRelease(h); have = false; }
    }
};

/* The item table of a partitioned model: ONE virtual address range per array (hipMemAddressReserve)
 * whose physical pages live on the owners' devices (hipMemCreate per run of pages, hipMemMap), readable
 * and writable from every device (hipMemSetAccess; remote pages travel over xGMI).  All replicas therefore
 * use the same table layout and the same global row ids — the kernels of the hot path are unchanged — while
 * each row is stored once and updated only by its owner.  Two deployments: a single-process group creates
 * every part itself (local_rank < 0); under one process per GPU each process creates the parts homed on its
 * rank and maps the others from file descriptors its peers exported. */
struct SharedTable {
    struct Part { hipMemGenericAllocationHandle_t h{}; size_t off = 0, bytes = 0; int home = 0; bool have = false, mapped = false; };
    void* base = nullptr;
    size_t total = 0;
    std::vector<Part> parts;
    float *E = nullptr, *Eacc = nullptr, *Em = nullptr, *b = nullptr, *bacc = nullptr, *bm = nullptr;
    int local_rank = -1;
    uint64_t slice = 0;
    /* single-process group: owner q's last update of its rows, as the group plan's partitioned step recorded it on q's stream
     * (the plan's event; null before the first step and after the plan is gone).  The rows of the table are written on their
     * OWNERS' streams, so whoever reads the table on another replica's stream joins these first (join_table_owners). */
    std::vector<hipEvent_t> owner_updated;

    ~SharedTable() {
        for (auto& pt : parts) {
            if (pt.mapped) (void)hipMemUnmap(reinterpret_cast<char*>(base) + pt.off, pt.bytes);
            if (pt.have) (void)hipMemRelease(pt.h);
        }
        if (base) (void)hipMemAddressFree(base, total);
    }

    /* layout: identical on every rank.  A page goes to the rank that owns its first row (rows [r*S, (r+1)*S)
     * belong to rank r); runs of pages with the same home are one part. */
    sbr_status plan(uint64_t num_items, uint64_t d, bool adam, int nranks, uint64_t S, int device) {
        slice = S;
        const size_t gran = VmmBuf::granularity(device);
        if (!gran) return SBR_ERR_UNSUPPORTED;
        struct Arr { float** ptr; uint64_t row_bytes; bool on; };
        Arr arrs[6] = {{&E, d * 4, true}, {&Eacc, d * 4, true}, {&Em, d * 4, adam}, {&b, 4, true}, {&bacc, 4, true}, {&bm, 4, adam}};
        size_t off[6], bytes[6];
        total = 0;
        for (int a = 0; a < 6; ++a) {
            off[a] = total;
            bytes[a] = arrs[a].on ? ((size_t)(num_items * arrs[a].row_bytes) + gran - 1) / gran * gran : 0;
            total += bytes[a];
        }
        if (hipMemAddressReserve(&base, total, gran, nullptr, 0) != hipSuccess) { base = nullptr; return SBR_ERR_OUT_OF_MEMORY; }
        for (int a = 0; a < 6; ++a) {
            if (!arrs[a].on) continue;
            *arrs[a].ptr = reinterpret_cast<float*>(reinterpret_cast<char*>(base) + off[a]);
            const size_t npages = bytes[a] / gran;
            auto home = [&](size_t page) {
                const uint64_t row = (uint64_t)(page * gran) / arrs[a].row_bytes;
                uint64_t owner = row / S;
                if (owner >= (uint64_t)nranks) owner = (uint64_t)nranks - 1;
                return (int)owner;
            };
            size_t run_begin = 0;
            while (run_begin < npages) {
                const int hm = home(run_begin);
                size_t run_end = run_begin + 1;
                while (run_end < npages && home(run_end) == hm) ++run_end;
                Part pt;
                pt.off = off[a] + run_begin * gran;
                pt.bytes = (run_end - run_begin) * gran;
                pt.home = hm;
                parts.push_back(pt);
                run_begin = run_end;
            }
        }
        return SBR_OK;
    }

    /* physical allocation + mapping of the parts this process is responsible for */
    sbr_status create_parts(const std::vector<int>& device_of_rank) {
        for (auto& pt : parts) {
            if (local_rank >= 0 && pt.home != local_rank) continue;
            hipMemAllocationProp prop = {};
            prop.type = hipMemAllocationTypePinned;
            prop.location.type = hipMemLocationTypeDevice;
            prop.location.id = device_of_rank[pt.home];
            prop.requestedHandleTypes = hipMemHandleTypePosixFileDescriptor;
            if (hipMemCreate(&pt.h, pt.bytes, &prop, 0) != hipSuccess) return SBR_ERR_OUT_OF_MEMORY;
            pt.have = true;
            if (hipMemMap(reinterpret_cast<char*>(base) + pt.off, pt.bytes, 0, pt.h, 0) != hipSuccess) return SBR_ERR_HIP;
            pt.mapped = true;
        }
        return SBR_OK;
    }

    sbr_status import_part(uint32_t i, int fd) {
        if (i >= parts.size() || parts[i].mapped) return SBR_ERR_INVALID_ARGUMENT;
        Part& pt = parts[i];
        if (import_shareable_fd(&pt.h, fd) != hipSuccess) return SBR_ERR_HIP;
        pt.have = true;
        if (hipMemMap(reinterpret_cast<char*>(base) + pt.off, pt.bytes, 0, pt.h, 0) != hipSuccess) return SBR_ERR_HIP;
        pt.mapped = true;
        return SBR_OK;
    }

    sbr_status set_access(const std::vector<int>& devices) {
        for (const auto& pt : parts)
            if (!pt.mapped) return SBR_ERR_INVALID_ARGUMENT; /* a peer's part has not been imported yet */
        std::vector<int> uniq(devices);
        std::sort(uniq.begin(), uniq.end());
        uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
        std::vector<hipMemAccessDesc> acc(uniq.size());
        for (size_t i = 0; i < uniq.size(); ++i) {
            acc[i].location.type = hipMemLocationTypeDevice;
            acc[i].location.id = uniq[i];
            acc[i].flags = hipMemAccessFlagsProtReadWrite;
        }
        if (hipMemSetAccess(base, total, acc.data(), acc.size()) != hipSuccess) return SBR_ERR_UNSUPPORTED;
        return SBR_OK;
    }

    /* single-process group: devices[r] = HIP device of replica r */
    sbr_status create(uint64_t num_items, uint64_t d, bool adam, const std::vector<int>& devices, uint64_t S) {
        SBRCHK(plan(num_items, d, adam, (int)devices.size(), S, devices[0]));
        SBRCHK(create_parts(devices));
        return set_access(devices);
    }
};

/* Scratch of the prediction side (user_representation, mrr_score, recommend*, rank_targets*), kept for the life of the model: one
 * device allocation that only grows, carved per launch — a call used to make and free ~25 device allocations (a quarter of
 * mrr_score's wall time at 8 192 users x 1e6 items went to the allocator and its implicit synchronisations).  What a launch needs
 * is not computed beside its takes but found by running them: measure(), the takes (which then only count), reserve(used), the
 * same takes again (carve_arena). */
struct DeviceArena {
    uint8_t* base = nullptr;
    size_t cap = 0, used = 0;
    bool measuring = false;
    bool overrun = false; /* a take since the last reserve went past cap (and got null): the call fails */
    /* SBR_TEST_GUARD: `guard` bytes in front of the first take and behind every take's padded end, counted by the measuring pass
     * like the takes themselves; `takes` = the current carve's, for the checks (carve_arena, check_arena_guards) */
    struct Take { size_t at, req, band_end; };
    size_t guard = 0, front = 0;
    std::vector<Take> takes;
    void measure(size_t guard_bytes = 0) { guard = guard_bytes; used = guard; measuring = true; }
    sbr_status reserve(size_t need) {
        used = front = guard;
        takes.clear();
        measuring = overrun = false;
        if (need <= cap) return SBR_OK;
        if (base) (void)hipFree(base);
        base = nullptr; cap = 0;
        const size_t want = need + need / 8 + 4096;
        if (hipMalloc(reinterpret_cast<void**>(&base), want) != hipSuccess) { base = nullptr; return SBR_ERR_OUT_OF_MEMORY; }
        cap = want;
        return SBR_OK;
    }
    static size_t padded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    template <typename T>
    T* take(size_t count) {
        const size_t at = used, bytes = (count ? count : 1) * sizeof(T);
        used += padded(bytes) + guard;
        if (measuring) return nullptr;
        if (used > cap) { overrun = true; return nullptr; }
        if (guard) takes.push_back(Take{at, bytes, used});
        return reinterpret_cast<T*>(base + at);
    }
    void release() { if (base) (void)hipFree(base); base = nullptr; cap = used = front = 0; takes.clear(); }
};

/* SBR_TEST_GUARD: the bands of the arena's current carve against the guard byte; the model's stream is drained.  A carve made
 * with the hook off has no takes on record: nothing happens. */
static void check_arena_guards(DeviceArena& ar) {
    if (ar.takes.empty()) return;
    {
        GuardState& gs = guard_state();
        std::lock_guard<std::mutex> g(gs.mu);
        gs.r.takes += ar.takes.size();
    }
    guard_check_band(ar.base, ar.front, false, SBR_GUARD_ARENA_TAKE, 0, ar.takes[0].req, -(int64_t)ar.front);
    for (size_t i = 0; i < ar.takes.size(); ++i) {
        const DeviceArena::Take& t = ar.takes[i];
        guard_check_band(ar.base + t.at + t.req, t.band_end - (t.at + t.req), false, SBR_GUARD_ARENA_TAKE, i, t.req, 1);
    }
}

struct sbr_model {
    sbr_hparams hp;
    std::shared_ptr<SharedTable> shared; /* partitioned group: the table arrays belong to this object */
    int d = 0, ng = 0; /* d = storage width (storage_dim of hp.embedding_dim) */
    int dl = 0;        /* embedding_dim as the caller sees it */
    int device = 0;
    sbr::ModelView mv;
    sbr_xorshift rng;
    sbr_xorshift rng_after_table; /* RNG state right after the item-table initialisation */
    std::vector<float> pending_E;  /* process-per-GPU partitioned table: this rank's rows until sbr_partition_finalize */
    bool partition_finalized = true;
    uint64_t global_epoch = 0;
    uint64_t opt_steps = 0; /* optimiser steps taken (Adam bias correction) */
    uint64_t param_gen = 0; /* parameter generation: bumped by whatever can write parameters (a fit plan opening or closing,
                             * sbr_model_set_param); a session store serves only the generation it was last bound to */
    uint32_t open_plans = 0; /* fit plans open on this model: their steps write parameters, so no session store call (reset_all
                              * included) is served until they are destroyed */
    float last_lagged_loss = 0.0f; /* what the reference's fit would have returned for the last sbr_model_fit / sbr_group_fit */
    bool opt_state_partial = false; /* owner-applied steps (sbr_fit_step_owner_update) have run since the item table's optimiser state was last
                                     * complete on this replica: only the rows this rank owns are current (sbr_model_table_slice /
                                     * sbr_model_optimizer_state_gathered; the library's own drivers gather when a fit ends) */
    bool reference_order = false; /* sbr_model_set_reference_order: negatives from the worker's sequential stream (one sequence per step) */
    int step_fusion = 2; /* one-sequence steps at d <= 32 (sbr_model_set_step_fusion): 0 separate launches, 1 fused launches
                          * (SmallTail + small_back: four per step), 2 runs of steps in one launch where the shape allows */
    uint32_t* item_tags = nullptr; /* sbr_model_set_item_tags: one tag word per item on this model's device, null until set.  Serving
                                    * metadata (guarded by mu), not a parameter: no generation bump, not saved, freed with the model */
    uint32_t* item_groups = nullptr; /* sbr_model_set_item_groups: one group word per item, stored and freed as item_tags */
    DeviceArena eval_arena;        /* prediction-side scratch (guarded by mu) */
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t side = nullptr;          /* second stream: dense-gradient GEMM runs beside the sparse update */
    hipStream_t sorter = nullptr;        /* third stream: key sort of the sparse update, underneath the backward pass */
    hipStream_t copier = nullptr;        /* uploads of the packed epochs; created at the first fit, kept (creating and destroying a
                                          * stream costs 1.5 + 1.3 ms — as much as a whole small fit call's kernels) */
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_scored = nullptr, ev_sorted = nullptr;
    std::mutex mu;
    bool timing = false;
    uint32_t timing_mask = 0xffffffffu; /* kernel families whose launches are bracketed by events while `timing` is on */
    bool overlap = true; /* false: the side-stream work is queued on the main stream (standalone kernel timing) */
    std::vector<TimingPair> pending;
    double ms[SBR_K_FAMILIES] = {0};
    uint64_t launches[SBR_K_FAMILIES] = {0};
    std::atomic<uint64_t> test_delays[5] = {}; /* SBR_TEST_STREAM_DELAY: delay kernels queued per role since sbr_test_delays_queued last read them */
};

namespace {

struct ScopedTimer {
    sbr_model* m;
    TimingPair tp;
    bool on;
    hipStream_t st;
    ScopedTimer(sbr_model* model, int family, uint64_t launches, hipStream_t stream = nullptr)
        : m(model), on(model->timing && ((model->timing_mask >> family) & 1u)), st(stream ? stream : model->stream) {
        if (!on) return;
        tp.family = family;
        tp.launches = launches;
        hipEventCreate(&tp.a);
        hipEventCreate(&tp.b);
        hipEventRecord(tp.a, st);
    }
    ~ScopedTimer() {
        if (!on) return;
        hipEventRecord(tp.b, st);
        m->pending.push_back(tp);
    }
    /* the bracket is closed here and a new one of the same family (no further launch counted) opened behind whatever the
     * caller queues in between: a delay of the stream-delay test hook is never inside a bracket */
    void pause() {
        if (!on) return;
        hipEventRecord(tp.b, st);
        m->pending.push_back(tp);
    }
    void resume() {
        if (!on) return;
        tp.launches = 0;
        hipEventCreate(&tp.a);
        hipEventCreate(&tp.b);
        hipEventRecord(tp.a, st);
    }
};

/* ---- the stream-delay test hook ---------------------------------------------------------------------------
 * SBR_TEST_STREAM_DELAY="<role>[@<device>]=<microseconds>[,...]", read per call; roles: main, side, sorter, copier, xs;
 * @<device> = the model's device_rank, without it every model.  A stream named there is made LATE: a delay kernel (one wave, no
 * memory traffic, bounded) is queued right behind every cross-stream wait the engine issues on it — stream_wait() below is the
 * only place the engine calls hipStreamWaitEvent — and at the head of the first work a call queues on it where no wait precedes
 * that work (stream_head()).  A consumer that really waits for the late stream's event sees no difference; one that does not reads
 * stale data and loses bit-parity with the oracle (tests/test_stream_joins_gpu.py).  Unset: no launch, nothing inside a kernel. */
enum { ROLE_MAIN = 0, ROLE_SIDE = 1, ROLE_SORTER = 2, ROLE_COPIER = 3, ROLE_XS = 4, ROLE_COUNT = 5 };
constexpr uint32_t test_delay_max_us = 5000;

int stream_role(const sbr_model* m, hipStream_t s) {
    if (s == m->stream) return ROLE_MAIN;
    if (s == m->side) return ROLE_SIDE;
    if (s == m->sorter) return ROLE_SORTER;
    if (s == m->copier) return ROLE_COPIER;
    return ROLE_XS; /* the group plan's exchange stream is the only other stream the engine waits on */
}

/* microseconds by which `role` of this model is to be late (0: not named, or the variable is unset or malformed) */
uint32_t test_delay_us(const sbr_model* m, int role) {
    const char* e = std::getenv("SBR_TEST_STREAM_DELAY");
    if (!e || !*e) return 0;
    static const char* const names[ROLE_COUNT] = {"main", "side", "sorter", "copier", "xs"};
    const size_t nl = std::strlen(names[role]);
    uint32_t us = 0;
    while (*e) {
        const char* end = std::strchr(e, ',');
        const size_t len = end ? (size_t)(end - e) : std::strlen(e);
        if (len > nl && std::strncmp(e, names[role], nl) == 0 && (e[nl] == '=' || e[nl] == '@')) {
            const char* q = e + nl;
            bool mine = true;
            if (*q == '@') {
                char* after = nullptr;
                const unsigned long dev = std::strtoul(q + 1, &after, 10);
                mine = after != q + 1 && dev == (unsigned long)m->hp.device_rank;
                q = after;
            }
            if (mine && q && *q == '=') {
                char* after = nullptr;
                const unsigned long v = std::strtoul(q + 1, &after, 10);
                if (after != q + 1 && after <= e + len) us = (uint32_t)std::min<unsigned long>(v, test_delay_max_us);
            }
        }
        e += len + (end ? 1 : 0);
    }
    return us;
}

int wall_clock_khz() { /* the rate of the kernels' wall_clock64() (100 MHz on CDNA) */
    int v = 0, dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeWallClockRate, dev) != hipSuccess || v <= 0) v = 100000;
    return v;
}

sbr_status queue_test_delay(sbr_model* m, hipStream_t s, int role, uint32_t us, ScopedTimer* open) {
    static const int khz = wall_clock_khz();
    const bool bracketed = open && open->on && open->st == s;
    if (bracketed) open->pause();
    sbr::launch_stream_delay((unsigned long long)us * (unsigned long long)khz / 1000ull, s);
    m->test_delays[role].fetch_add(1, std::memory_order_relaxed);
    if (bracketed) open->resume();
    HIPCHK(hipGetLastError());
    return SBR_OK;
}

/* every cross-stream join of the engine: stream `s` of model m waits for `e` (`open`: the timing bracket the caller holds, if any) */
sbr_status stream_wait(sbr_model* m, hipStream_t s, hipEvent_t e, ScopedTimer* open = nullptr) {
    HIPCHK(hipStreamWaitEvent(s, e, 0));
    const int role = stream_role(m, s);
    const uint32_t us = test_delay_us(m, role);
    return us ? queue_test_delay(m, s, role, us, open) : SBR_OK;
}

/* the head of the first work a call queues on `s` where no wait precedes it */
sbr_status stream_head(sbr_model* m, hipStream_t s) {
    const int role = stream_role(m, s);
    const uint32_t us = test_delay_us(m, role);
    return us ? queue_test_delay(m, s, role, us, nullptr) : SBR_OK;
}

/* A partitioned table is updated by its owners on THEIR streams (sbr_group_plan::partitioned_step): a reader of the table on this
 * model's stream — prediction, evaluation, sbr_model_get_param — waits for the other owners' last updates first.  (The next
 * training step does the same through the plan's wait_applied.) */
sbr_status join_table_owners(sbr_model* m) {
    if (!m->shared) return SBR_OK;
    const std::vector<hipEvent_t>& ev = m->shared->owner_updated;
    for (size_t q = 0; q < ev.size(); ++q)
        if (ev[q] && q != (size_t)m->hp.device_rank) SBRCHK(stream_wait(m, m->stream, ev[q]));
    return SBR_OK;
}

/* entry of a call that reads the model's parameters on its stream */
sbr_status enter_reader(sbr_model* m) {
    HIPCHK(hipSetDevice(m->device));
    return join_table_owners(m);
}

uint64_t dense_count(const sbr_model* m) {
    return m->ng ? (uint64_t)(2 * m->d + 1) * m->ng * m->d : (uint64_t)m->d;
}

/* exchange block geometry (identical to the oracle's) */
uint64_t block_bytes_for(const sbr_model* m, uint64_t rmax) {
    const uint64_t words = 8 + 4 * rmax + 2 * rmax * (uint64_t)m->d + dense_count(m);
    return ((words * 4 + 15) / 16) * 16;
}
uint64_t dense_offset_bytes(const sbr_model* m, uint64_t rmax) { return (8 + 4 * rmax + 2 * rmax * (uint64_t)m->d) * 4; }

sbr::BlockView block_view(const sbr_model* m, void* block, uint64_t rmax) {
    sbr::BlockView v;
    uint32_t* w = reinterpret_cast<uint32_t*>(block);
    v.header = w;
    v.in_idx = w + 8;
    v.out_idx = v.in_idx + rmax;
    v.neg = v.out_idx + rmax;
    v.coef = reinterpret_cast<float*>(v.neg + rmax);
    v.H = reinterpret_cast<float*>(w + 8 + 4 * rmax);
    v.dX = v.H + rmax * (uint64_t)m->d;
    v.dense = v.dX + rmax * (uint64_t)m->d;
    return v;
}

/* host-side packed description of a set of sequences (training minibatch or evaluation batch) */
struct Packed {
    int R = 0, B = 0, Tm = 0;
    std::vector<int> off, steps, prev_row, order; /* order[b] = index of the b-th sequence in the input */
    std::vector<uint32_t> in_idx, out_idx, ctr;
};

/* Sequences are given as (pointer to first item, number of steps, has_target).  Training:
 * steps = len - 1, in_t = item[t], out_t = item[t+1] (sequence_model.rs:115-122).  Evaluation:
 * steps = len, no targets (sequence_model.rs:192-194).  Ordered by steps descending (stable). */
void pack_sequences(const std::vector<const uint32_t*>& first, const std::vector<int>& nsteps, bool with_targets,
                    const std::vector<uint64_t>* ctr_base, int maxT, Packed* out) {
    const int nb = (int)first.size();
    out->B = nb;
    out->order.resize(nb);
    std::vector<int> cnt(maxT + 2, 0), pos(maxT + 2, 0);
    for (int i = 0; i < nb; ++i) cnt[nsteps[i]]++;
    int acc = 0;
    for (int l = maxT; l >= 0; --l) { pos[l] = acc; acc += cnt[l]; }
    for (int i = 0; i < nb; ++i) out->order[pos[nsteps[i]]++] = i;
    const int Tm = nb ? nsteps[out->order[0]] : 0;
    out->Tm = Tm;
    out->off.assign(Tm + 1, 0);
    out->steps.resize(nb);
    for (int b = 0; b < nb; ++b) out->steps[b] = nsteps[out->order[b]];
    {
        int alive = nb;
        for (int t = 0; t < Tm; ++t) {
            while (alive > 0 && out->steps[alive - 1] <= t) --alive;
            out->off[t + 1] = out->off[t] + alive;
        }
    }
    const int R = out->off[Tm];
    out->R = R;
    out->in_idx.assign(R, 0);
    out->out_idx.assign(R, 0);
    out->ctr.assign(R, 0);
    out->prev_row.assign(R, -1);
    for (int b = 0; b < nb; ++b) {
        const int src = out->order[b];
        const uint32_t* it = first[src];
        for (int t = 0; t < out->steps[b]; ++t) {
            const int r = out->off[t] + b;
            out->in_idx[r] = it[t];
            if (with_targets) out->out_idx[r] = it[t + 1];
            if (ctr_base) out->ctr[r] = (uint32_t)((*ctr_base)[src] + (uint64_t)t);
            out->prev_row[r] = t ? out->off[t - 1] + b : -1;
        }
    }
}

struct DevicePacked { /* device image of one or more Packed, concatenated */
    int* off = nullptr;
    int* steps = nullptr;
    int* prev_row = nullptr;
    uint32_t *in_idx = nullptr, *out_idx = nullptr, *ctr = nullptr;
    void release() {
        dfree(off); dfree(steps); dfree(prev_row); dfree(in_idx); dfree(out_idx); dfree(ctr);
        off = steps = prev_row = nullptr;
        in_idx = out_idx = ctr = nullptr;
    }
};

struct WorkBuffers {
    sbr::WorkView v{};
    void release() {
        dfree(v.C); dfree(v.G); dfree(v.dH); dfree(v.dZ); dfree(v.X); dfree(v.zeros); dfree(v.dHrec); dfree(v.dCrec); dfree(v.dab);
        dfree(v.partials); dfree(v.loss); dfree(v.tries); dfree(v.part_loss); dfree(v.part_tries);
        v = sbr::WorkView{};
    }
};

sbr_status alloc_work(const sbr_model* m, uint64_t rmax, uint64_t bmax, bool training, WorkBuffers* wb) {
    const uint64_t d = (uint64_t)m->d;
    sbr::WorkView& v = wb->v;
    v.fold_max_tiles = SBR_FOLD_MAX_TILES_DEFAULT;
    if (m->ng) {
        SBRCHK(dmalloc(&v.C, rmax * d));
        SBRCHK(dmalloc(&v.G, rmax * d * 4));
        SBRCHK(dmalloc(&v.X, rmax * d));
    }
    if (training) {
        SBRCHK(dmalloc(&v.dH, rmax * d));
        SBRCHK(dmalloc(&v.loss, rmax));
        SBRCHK(dmalloc(&v.tries, rmax));
        SBRCHK(dmalloc(&v.part_loss, 2048));
        SBRCHK(dmalloc(&v.part_tries, 2048));
        if (m->ng) {
            const uint64_t rchunk = (rmax + SBR_DW_CHUNK_ROWS - 1) / SBR_DW_CHUNK_ROWS * SBR_DW_CHUNK_ROWS;
            SBRCHK(dmalloc(&v.dZ, rchunk * d * (uint64_t)m->ng)); /* the dense-gradient GEMM reads dZ to the end of the last chunk */
            v.wide_addresses = std::getenv("SBR_DW_WIDE_ADDRESSES") ? 1 : 0; /* read when the plan's buffers are made */
            SBRCHK(dmalloc(&v.zeros, 256));
            HIPCHK(hipMemset(v.zeros, 0, 256 * sizeof(float)));
            SBRCHK(dmalloc(&v.dHrec, bmax * d));
            SBRCHK(dmalloc(&v.dCrec, bmax * d));
            const uint64_t nch = (rmax + SBR_DW_CHUNK_ROWS - 1) / SBR_DW_CHUNK_ROWS;
            SBRCHK(dmalloc(&v.partials, nch * dense_count(m)));
        } else {
            SBRCHK(dmalloc(&v.dab, bmax * d));
            SBRCHK(dmalloc(&v.partials, ((bmax + 255) / 256) * d));
        }
    }
    return SBR_OK;
}

/* ---- a training step's stream schedule: what the local half of ONE step queues on which stream.  Decided once, by step_schedule(),
 * before anything is queued; the step's consumers read the form of the block from the copy left in the plan (StepLeft). ---- */
enum SortAt {
    SORT_IN_SCORE,    /* the score launch orders the keys itself (StepSchedule::small_tail): no ordering launch */
    SORT_AT_START,    /* single-negative losses: the negatives are a hash of the row counter, the ordering needs only the index arrays */
    SORT_AFTER_SCORE, /* WARP (the negatives come out of the score kernel), everything on the main stream: between score and BPTT */
    SORT_AFTER_BPTT,  /* WARP with the side streams: behind the score kernel's event on the sorter, but queued by the host BEHIND
                       * BPTT — the ordering's up to nine short launches would otherwise sit in the host's queue ahead of the backward
                       * pass (50 us at a few hundred sequences per step, as long as the pass itself).  There it takes whatever slots
                       * BPTT's retiring workgroups free and is finished by the time the update needs the keys.  (Measured and dropped:
                       * the main stream before or right after BPTT for large steps — its 0.1-0.3 ms are then on the critical path;
                       * profiles/r04_tail_experiments.md (c).) */
};
struct StepSchedule {
    /* The side streams engage.  A small step (its sparse update is the single-launch form: <= 4 096 keys, 1 365 rows) is a chain of
     * launches of a few microseconds each; the event hand-offs between three streams then cost more than the overlap buys
     * (MovieLens-100K at one sequence per step: 1.67 s with the side streams, 1.57 s on one), so everything goes on the main stream. */
    bool overlap = false;
    /* the dense-gradient GEMM (MFMA-bound, reads dZ / X / H only): with overlap the side stream, so that the HBM-bound sparse
     * update that follows on the main stream overlaps it (ev_fork -> ev_join) */
    hipStream_t dense_on = nullptr;
    /* the key ordering: with overlap the sorter stream, underneath the backward pass (ev_scored -> ev_sorted); queued at sort_at */
    hipStream_t sort_on = nullptr;
    SortAt sort_at = SORT_IN_SCORE;
    /* WARP step with the ordering on the sorter: the per-sequence loss sums and the block header (row count, loss sum; the
     * single-device accumulators) are queued on THAT stream, behind the score kernel's event and ahead of the ordering — between
     * score and BPTT they were two launches and their gaps (~35 us of a 2.5 ms step) on the critical path for nobody's benefit.
     * Their consumers (update / scatter / dense / fit_end) all join the ordering's stream first. */
    bool side_header = false;
    /* EWMA + single-negative loss (BASELINE configs[4]): scan, scores and backward scan of a sequence in ONE pass (ewma_seq_kernel;
     * same bits as scan | score | backward scan, which EWMA + WARP and the reference-order mode still take: their negatives depend
     * on the scores / on a sequential stream) */
    bool ewma_fused = false;
    /* the figure the reference's fit returns (sbr_report.hip): a small step folds the lagged chain into the header launch; otherwise
     * the per-sequence sums come from a parallel kernel and the sequential chain runs as one wave on the ordering's stream, queued
     * at the end of the local half, off the critical path (ev_seqsum -> ev_lagged) */
    bool fuse_lag = false;
    /* under sbr_fit_step, small LSTM step: the dense gradient is left to the optimiser half's single launch (sbr::launch_small_back) */
    bool dw_deferred = false;
    /* Single device: the hot rows (segments of more than SBR_SEG_CHUNK entries: a skewed catalogue) are listed and their chunk units
     * counted behind the ordering on ITS stream, still underneath BPTT — registering them during the short-segment pass put their
     * three launches behind it on the update's critical path (Zipf(1) items at 8 192 sequences per step: 0.13 of 2.66 ms).  Only
     * under sbr_fit_step: the list's only consumer is sbr_fit_step_apply; a caller that drives ONE device through the exchange halves
     * (scatter / reduce_own register long segments themselves, on the main stream) must not find the list kernels beside them. */
    bool hot_prelist = false;
    bool header_accumulates = false; /* single device: the header kernel adds the step to loss_acc / ex_acc itself (one launch fewer) */
    /* ONE subsequence per step at d <= 32 (the reference's own schedule): header, lagged loss figure and the ordering of the step's
     * keys run at the end of the score launch (sbr::SmallTail) — three launches of ~5 us fewer in a step of ~40-100 us */
    bool small_tail() const { return sort_at == SORT_IN_SCORE; }
};
/* What the main stream may have to join before it reads or overwrites something a step left on another stream (join_main):
 *   need       event      recorded on   guards
 *   KEYS       ev_sorted  sorter        keys_sorted and the segment heads
 *   HEADER     ev_sorted  sorter        the block header and the loss accumulators of a step with a side header
 *   DENSE      ev_join    side          blk.dense (or its chunk partials)
 *   LAG_STATE  ev_lagged  sorter        lag_state / lag_seqsum (the lagged chain)
 *   TABLE      ev_hot     sorter        the hot rows of the item table (sbr_fit_step_apply's pass beside the short segments)
 * The rule, for every event alike: recording it makes it OWED; join_main() waits for what is owed among the caller's needs and
 * clears it; nothing else does.  A debt so outlives the step that made it: where a step whose ordering ran on the main stream
 * follows one whose ordering ran on the sorter and nobody has joined that one, the next reader of the keys still waits for
 * ev_sorted, on one device or several.  An event the main stream has joined is not waited for again. */
enum : unsigned { KEYS = 1, HEADER = 2, DENSE = 4, LAG_STATE = 8, TABLE = 16 };
struct StepLeft { /* what a step's local half leaves in the plan for its consumers */
    StepSchedule form;              /* of the last local half; cleared by the step's last consumer (step_consumed) */
    int dense_unreduced_chunks = 0; /* > 0: blk.dense is still that many chunk partials in wb.v.partials (one device: reduced by its consumer) */
    unsigned owed = 0;              /* the needs above whose event the main stream has not joined */
};
}  // namespace

struct sbr_fit_plan {
    sbr_model* m = nullptr;
    int ndev = 1, rank = 0, T = 0;
    uint64_t nseq_total = 0, part_len = 0;
    std::vector<uint64_t> seq_start; /* [ndev * part_len], offsets into items */
    std::vector<uint32_t> seq_len;
    std::vector<sbr_xorshift> part_rng;
    std::vector<uint64_t> fit_seed;
    std::vector<uint32_t> items; /* host copy of the CSR item ids */
    uint64_t rmax = 0, bmax = 0;
    /* epoch data is double-buffered: the GPU consumes ep[cur] while a host thread may already
     * shuffle, pack and upload the next epoch into ep[cur ^ 1] (sbr_fit_epoch_prefetch) */
    struct Mb { int R, B, Tm; uint64_t row_base, off_base, seq_base; };
    struct Epoch {
        uint64_t epoch_key_epoch = 0;
        uint64_t num_mb = 0;
        std::vector<Mb> mbs;
        std::vector<int> off_host;         /* concatenated off tables of this rank */
        std::vector<uint32_t> rows_of_dev; /* [num_mb][ndev] */
        DevicePacked dp;
        sbr::StepDesc* d_desc = nullptr;   /* one sequence per step (batch_sequences = 1): the steps of the epoch for the one-launch form */
        uint64_t desc_cap = 0;
        std::vector<sbr::StepDesc> desc_host;
        uint64_t rows_cap = 0, off_cap = 0, seq_cap = 0;
        /* pinned host staging of the packed index arrays (written directly by the packer, one DMA each) */
        uint32_t *h_in = nullptr, *h_out = nullptr, *h_ctr = nullptr;
        int *h_prev = nullptr, *h_steps = nullptr;
        uint64_t h_rows_cap = 0, h_seq_cap = 0;
        hipEvent_t free_event = nullptr;   /* recorded on the compute stream when the GPU is done with dp */
        bool free_recorded = false;
    } ep[2];
    int cur = 0;
    std::thread worker;
    bool pending = false;
    sbr_status pending_status = SBR_OK;
    hipStream_t copy_stream = nullptr;
    /* work */
    WorkBuffers wb;
    uint8_t* block = nullptr;
    uint64_t block_bytes = 0;
    uint64_t *keys = nullptr, *keys_sorted = nullptr;
    void* sort_temp = nullptr;
    size_t sort_temp_bytes = 0;
    int key_bits = 64;
    double* loss_acc = nullptr;
    unsigned long long* ex_acc = nullptr;
    uint32_t* ref_rng = nullptr;   /* reference order: the worker's xorshift128 state on the device (advanced by the score launch) */
    bool ref_rng_live = false;     /* ... and it has been advanced since the host last held it */
    unsigned long long* phase_clocks = nullptr; /* [6] epoch_steps_kernel's per-phase s_memtime ticks + steps (sbr_fit_debug_phase_clocks) */
    sbr::SegScratch seg{}; /* long-segment path of the sparse reduction (hot rows) */
    StepLeft left; /* the last step's form and what the main stream has not joined of it (join_main) */
    hipEvent_t ev_hot = nullptr;
    /* the loss figure the reference's fit returns (sbr_report.hip): [accumulator | loss-node value per sequence length], the
     * per-sequence sums of the current step, and the events that order the one-wave chain kernel (sorter stream) against the
     * main stream */
    float *lag_state = nullptr, *lag_seqsum = nullptr;
    hipEvent_t ev_seqsum = nullptr, ev_lagged = nullptr;
    /* partitioned item table: this device's gradient list (addressed by sorted-key position), the owner
     * bounds, and the owner-side merge buffers */
    float *glist = nullptr, *gblist = nullptr;
    uint32_t *gfl = nullptr, *bounds_dev = nullptr;
    /* one process per GPU: the list (and the sorted keys) live in exportable allocations, the peers' lists
     * are mapped from the file descriptors they exported: [0] keys_sorted [1] glist [2] gblist [3] gfl */
    /* peer transport of the replicated exchange: [0] this rank's send buffer (ndev chunks), [1] its reduced
     * own chunk — exportable; the peers' pair is mapped here and read in place by the kernels */
    VmmBuf xchg_own[2];
    std::vector<std::array<VmmBuf, 2>> xchg_peer;
    bool exportable_lists = false;
    VmmBuf own_x[4];
    std::vector<std::array<VmmBuf, 4>> peer_x;
    uint64_t *mkeys = nullptr, *mkeys_sorted = nullptr;
    void* msort_temp = nullptr;
    size_t msort_temp_bytes = 0;
    uint64_t mcap = 0;
    sbr::MergePlan* mplan = nullptr;  /* where this owner's row range lies in every device's sorted keys: on the DEVICE (merge_plan_kernel) */
    uint32_t* all_bounds_dev = nullptr; /* one process per GPU: the ranks' owner bounds, gathered on the device by the host's collective */
    /* last step (debug) */
    int last_R = 0;
    const void* last_block = nullptr;
};

namespace {

sbr::MbView mb_view(const sbr_fit_plan* p, uint64_t i) {
    const sbr_fit_plan::Epoch& e = p->ep[p->cur];
    const sbr_fit_plan::Mb& mb = e.mbs[i];
    sbr::MbView v;
    v.R = mb.R; v.B = mb.B; v.Tm = mb.Tm;
    v.off = e.dp.off + mb.off_base;
    v.steps = e.dp.steps + mb.seq_base;
    v.prev_row = e.dp.prev_row + mb.row_base;
    v.in_idx = e.dp.in_idx + mb.row_base;
    v.out_idx = e.dp.out_idx + mb.row_base;
    v.ctr = e.dp.ctr + mb.row_base;
    return v;
}

void shuffle_pairs(uint64_t* start, uint32_t* len, uint64_t n, sbr_xorshift* r) {
    for (uint64_t i = n; i >= 2;) { /* rand 0.5 Rng::shuffle: Fisher-Yates from the end over gen_range(0, i + 1) */
        i -= 1;
        const uint64_t j = sbr_rand_gen_range(r, i + 1);
        std::swap(start[i], start[j]);
        std::swap(len[i], len[j]);
    }
}

/* one optimiser step begins: advance the step count and refresh Adam's bias corrections */
void begin_optimizer_step(sbr_model* m) {
    m->opt_steps += 1;
    if (m->hp.optimizer == SBR_OPT_ADAM) sbr_adam_corrections(m->opt_steps, &m->mv.c1, &m->mv.c2);
}

sbr_status ensure_device(const sbr_model* m) {
    HIPCHK(hipSetDevice(m->device));
    return SBR_OK;
}

}  // namespace

extern "C" {

uint32_t sbr_abi_version(void) { return SBR_ABI_VERSION; }

void sbr_release_cached_memory(void) { scratch_cache().trim(); }

const char* sbr_status_string(sbr_status s) {
    switch (s) {
        case SBR_OK: return "ok";
        case SBR_ERR_NO_INTERACTIONS: return "No interactions were supplied.";
        case SBR_ERR_INVALID_PREDICTION: return "Invalid prediction value: non-finite or not a number.";
        case SBR_ERR_INVALID_ARGUMENT: return "invalid argument";
        case SBR_ERR_UNSUPPORTED: return "unsupported configuration";
        case SBR_ERR_NO_DEVICE: return "no HIP device (the engine has no CPU fallback)";
        case SBR_ERR_HIP: return "HIP runtime error";
        case SBR_ERR_OUT_OF_MEMORY: return "out of device memory";
    }
    return "unknown";
}

sbr_status sbr_device_info(char* device_name, uint64_t name_bytes, uint32_t* out_cus, uint64_t* out_hbm_bytes) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return SBR_ERR_NO_DEVICE;
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, dev));
    if (device_name && name_bytes) {
        std::snprintf(device_name, (size_t)name_bytes, "%s", prop.gcnArchName);
    }
    if (out_cus) *out_cus = (uint32_t)prop.multiProcessorCount;
    if (out_hbm_bytes) *out_hbm_bytes = (uint64_t)prop.totalGlobalMem;
    return SBR_OK;
}

/* shared != null: the table arrays are the group's SharedTable; only the replica with write_table
 * initialises them, the others take the RNG state that follows the table initialisation */
enum TableInit { TABLE_WRITE_ALL = 0, TABLE_WRITE_NONE = 1, TABLE_OWN_ROWS_DEFERRED = 2 };
static sbr_status model_create_impl(const sbr_hparams* hp, std::shared_ptr<SharedTable> shared, int table_init,
                                    const sbr_xorshift* rng_after_table, sbr_model** out) {
    if (!hp || !out) return SBR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!storage_dim(hp->embedding_dim) || hp->num_items == 0 || hp->max_sequence_length < 3 || hp->num_devices == 0 ||
        hp->num_devices > 16 || hp->device_rank >= hp->num_devices || hp->batch_sequences == 0 ||
        hp->model < 0 || hp->model > 2 || hp->loss < 0 || hp->loss > 2)
        return SBR_ERR_INVALID_ARGUMENT;
    if (hp->optimizer != SBR_OPT_ADAGRAD && hp->optimizer != SBR_OPT_ADAM) return SBR_ERR_INVALID_ARGUMENT;
    int ndevices = 0;
    if (hipGetDeviceCount(&ndevices) != hipSuccess || ndevices == 0) return SBR_ERR_NO_DEVICE;
    sbr_model* m = new (std::nothrow) sbr_model();
    if (!m) return SBR_ERR_OUT_OF_MEMORY;
    m->hp = *hp;
    m->dl = (int)hp->embedding_dim;
    m->d = storage_dim(hp->embedding_dim);
    m->ng = hp->model == SBR_MODEL_LSTM_NORMAL ? 4 : hp->model == SBR_MODEL_LSTM_COUPLED ? 3 : 0;
    if (hipGetDevice(&m->device) != hipSuccess) { delete m; return SBR_ERR_NO_DEVICE; }
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) { delete m; return SBR_ERR_HIP; }
    m->own_stream = true;
    /* the side stream carries the MFMA-bound dense-gradient GEMM beside the HBM-bound sparse update:
     * lowest priority, so the update's workgroups are placed first whenever a slot frees up */
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    /* the key sort gets its own stream: on the GEMM's stream its tail — the passes that did not fit underneath the
     * backward pass, whose workgroups fill every CU, so that the sort's kernels only run in slots that retiring
     * workgroups free — delayed the GEMM, which does not need the sorted keys, by 0.36 ms per step.  Priority: normal
     * (13.42-13.50 ms per step; high 13.62-13.74: the sort then wins every freed slot and the backward pass loses more
     * than the update gains; low 13.58-13.63). */
    (void)prio_greatest;
    if (hipStreamCreateWithPriority(&m->sorter, hipStreamNonBlocking, 0) != hipSuccess) { delete m; return SBR_ERR_HIP; }
    if (hipStreamCreateWithPriority(&m->side, hipStreamNonBlocking, prio_least) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_scored, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_sorted, hipEventDisableTiming) != hipSuccess) { delete m; return SBR_ERR_HIP; }
    sbr::ModelView& v = m->mv;
    std::memset(&v, 0, sizeof(v));
    v.d = m->d; v.ng = m->ng; v.coupled = m->ng == 3;
    v.num_items = hp->num_items; v.loss = hp->loss; v.lr = hp->learning_rate; v.l2 = hp->l2_penalty;
    v.optimizer = hp->optimizer; v.c1 = 1.0f; v.c2 = 1.0f;
    const bool adam = hp->optimizer == SBR_OPT_ADAM;
    const uint64_t I = hp->num_items, d = (uint64_t)m->d;
    /* a replica of a multi-device model stores num_devices x ceil(I / num_devices) rows: the owners' slices are then equally long, so
     * the all-gather of the updated parameter slices (sbr_fit_step_owner_update) can write every replica's table IN PLACE */
    const uint64_t Ia = table_rows_allocated(hp);
    sbr_status st = SBR_OK;
    auto fail = [&](sbr_status s) { sbr_model_destroy(m); return s; };
    m->shared = shared;
    if (shared) {
        v.E = shared->E; v.Eacc = shared->Eacc; v.b = shared->b; v.bacc = shared->bacc;
        v.Em = shared->Em; v.bm = shared->bm;
    } else {
        if ((st = dmalloc(&v.E, Ia * d)) != SBR_OK) return fail(st);
        if ((st = dmalloc(&v.Eacc, Ia * d)) != SBR_OK) return fail(st);
        if ((st = dmalloc(&v.b, Ia)) != SBR_OK) return fail(st);
        if ((st = dmalloc(&v.bacc, Ia)) != SBR_OK) return fail(st);
        if (adam) {
            if ((st = dmalloc(&v.Em, Ia * d)) != SBR_OK) return fail(st);
            if ((st = dmalloc(&v.bm, Ia)) != SBR_OK) return fail(st);
        }
        if (Ia > I) { /* the padding rows: never addressed by a row id, but they travel with the last owner's slice */
            hipMemsetAsync(v.E + I * d, 0, (Ia - I) * d * 4, m->stream);
            hipMemsetAsync(v.Eacc + I * d, 0, (Ia - I) * d * 4, m->stream);
            hipMemsetAsync(v.b + I, 0, (Ia - I) * 4, m->stream);
            hipMemsetAsync(v.bacc + I, 0, (Ia - I) * 4, m->stream);
            if (adam) {
                hipMemsetAsync(v.Em + I * d, 0, (Ia - I) * d * 4, m->stream);
                hipMemsetAsync(v.bm + I, 0, (Ia - I) * 4, m->stream);
            }
        }
    }
    /* ≙ build_params (lstm.rs:174-194): embeddings first, then the recurrent weights, same RNG */
    sbr_xs_seed(&m->rng, hp->seed);
    if (!shared || table_init == TABLE_WRITE_ALL) {
        if (adam) {
            hipMemsetAsync(v.Em, 0, I * d * 4, m->stream);
            hipMemsetAsync(v.bm, 0, I * 4, m->stream);
        }
        hipMemsetAsync(v.Eacc, 0, I * d * 4, m->stream);
        hipMemsetAsync(v.b, 0, I * 4, m->stream);
        hipMemsetAsync(v.bacc, 0, I * 4, m->stream);
        std::vector<float> host(I * d, 0.0f);
        const uint64_t dl = (uint64_t)m->dl;
        const double std_e = 1.0 / (double)dl; /* embedding_init, lstm.rs:22-25: row-major, embedding_dim values per row */
        for (uint64_t row = 0; row < I; ++row)
            for (uint64_t c = 0; c < dl; ++c) host[row * d + c] = sbr_rand_normal_f32(&m->rng, 0.0, std_e);
        if (hipMemcpy(v.E, host.data(), host.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(SBR_ERR_HIP);
    } else if (table_init == TABLE_OWN_ROWS_DEFERRED) {
        /* every rank walks the whole initialisation stream (the RNG has no skip-ahead through the normal
         * sampler's rejections) and keeps the rows it owns; they are written once the peers' parts are mapped */
        const uint64_t S = shared->slice, r0 = std::min<uint64_t>(I, (uint64_t)hp->device_rank * S), r1 = std::min<uint64_t>(I, r0 + S);
        m->pending_E.assign((size_t)((r1 - r0) * d), 0.0f);
        const uint64_t dl = (uint64_t)m->dl;
        const double std_e = 1.0 / (double)dl;
        for (uint64_t i = 0; i < I * dl; ++i) {
            const float val = sbr_rand_normal_f32(&m->rng, 0.0, std_e);
            const uint64_t row = i / dl;
            if (row >= r0 && row < r1) m->pending_E[(size_t)((row - r0) * d + i % dl)] = val;
        }
        m->partition_finalized = false;
    } else {
        m->rng = *rng_after_table;
    }
    m->rng_after_table = m->rng;
    if (m->ng) {
        const uint64_t nw = 2 * d * (uint64_t)m->ng * d, nb = (uint64_t)m->ng * d;
        if ((st = dmalloc(&v.W, nw)) != SBR_OK) return fail(st);
        if ((st = dmalloc(&v.Wacc, nw)) != SBR_OK) return fail(st);
        if ((st = dmalloc(&v.Wp, nw)) != SBR_OK) return fail(st);
        if ((st = dmalloc(&v.WTp, nw)) != SBR_OK) return fail(st);
        if ((st = dmalloc(&v.bW, nb)) != SBR_OK) return fail(st);
        if ((st = dmalloc(&v.bWacc, nb)) != SBR_OK) return fail(st);
        if (adam) {
            if ((st = dmalloc(&v.Wm, nw)) != SBR_OK) return fail(st);
            if ((st = dmalloc(&v.bWm, nb)) != SBR_OK) return fail(st);
            hipMemsetAsync(v.Wm, 0, nw * 4, m->stream);
            hipMemsetAsync(v.bWm, 0, nb * 4, m->stream);
        }
        hipMemsetAsync(v.Wacc, 0, nw * 4, m->stream);
        hipMemsetAsync(v.bW, 0, nb * 4, m->stream);
        hipMemsetAsync(v.bWacc, 0, nb * 4, m->stream);
        std::vector<float> host;
        draw_lstm_weights(&m->rng, m->dl, m->d, m->ng, &host);
        if (hipMemcpy(v.W, host.data(), nw * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(SBR_ERR_HIP);
        sbr::launch_repack_lstm(v, m->stream);
    } else {
        if ((st = dmalloc(&v.alpha, d)) != SBR_OK) return fail(st);
        if ((st = dmalloc(&v.alpha_acc, d)) != SBR_OK) return fail(st);
        if (adam) {
            if ((st = dmalloc(&v.alpha_m, d)) != SBR_OK) return fail(st);
            hipMemsetAsync(v.alpha_m, 0, d * 4, m->stream);
        }
        hipMemsetAsync(v.alpha, 0, d * 4, m->stream);
        hipMemsetAsync(v.alpha_acc, 0, d * 4, m->stream);
        /* the reference also draws the two unused d x d dense_init matrices fc1, fc2 from this RNG
         * (ewma.rs:179-188): drawn and dropped, so the driver's shuffles start where the reference's do */
        const uint64_t dl = (uint64_t)m->dl;
        const double std_fc = std::sqrt(2.0 / (double)(dl + dl));
        for (uint64_t i = 0; i < 2 * dl * dl; ++i) (void)sbr_rand_normal_f32(&m->rng, 0.0, std_fc);
    }
    if (hipStreamSynchronize(m->stream) != hipSuccess) return fail(SBR_ERR_HIP);
    *out = m;
    return SBR_OK;
}

sbr_status sbr_model_create(const sbr_hparams* hp, sbr_model** out) {
    return model_create_impl(hp, nullptr, TABLE_WRITE_ALL, nullptr, out);
}

void sbr_model_destroy(sbr_model* m) {
    if (!m) return;
    hipSetDevice(m->device);
    hipStreamSynchronize(m->stream); /* every stream that may still touch the arrays: they go back to the scratch cache, not the driver */
    if (m->side) hipStreamSynchronize(m->side);
    if (m->sorter) hipStreamSynchronize(m->sorter);
    sbr::ModelView& v = m->mv;
    if (!m->shared) { dfree(v.E); dfree(v.Eacc); dfree(v.b); dfree(v.bacc); dfree(v.Em); dfree(v.bm); }
    dfree(v.W); dfree(v.Wacc); dfree(v.bW); dfree(v.bWacc); dfree(v.Wp); dfree(v.WTp);
    dfree(v.alpha); dfree(v.alpha_acc);
    dfree(v.Wm); dfree(v.bWm); dfree(v.alpha_m);
    dfree(m->item_tags);
    dfree(m->item_groups);
    for (auto& tp : m->pending) { hipEventDestroy(tp.a); hipEventDestroy(tp.b); }
    check_arena_guards(m->eval_arena);
    m->eval_arena.release();
    if (m->own_stream && m->stream) hipStreamDestroy(m->stream);
    if (m->side) { hipStreamSynchronize(m->side); hipStreamDestroy(m->side); }
    if (m->sorter) { hipStreamSynchronize(m->sorter); hipStreamDestroy(m->sorter); }
    if (m->copier) { hipStreamSynchronize(m->copier); hipStreamDestroy(m->copier); }
    if (m->ev_fork) hipEventDestroy(m->ev_fork);
    if (m->ev_join) hipEventDestroy(m->ev_join);
    if (m->ev_scored) hipEventDestroy(m->ev_scored);
    if (m->ev_sorted) hipEventDestroy(m->ev_sorted);
    delete m;
}

sbr_status sbr_model_set_stream(sbr_model* m, void* hip_stream) {
    if (!m) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (m->own_stream && m->stream) hipStreamDestroy(m->stream);
    m->stream = reinterpret_cast<hipStream_t>(hip_stream);
    m->own_stream = false;
    return SBR_OK;
}

sbr_status sbr_model_synchronize(sbr_model* m) {
    if (!m) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    return SBR_OK;
}

/* Parameter arrays as the caller sees them: shapes in embedding_dim (dl) — E [I][dl], W [2 dl][ng dl] (rows [x ; h],
 * column blocks per gate), bW [ng dl], alpha [dl].  Storage is in the padded width d (storage_dim): `stored` is the
 * device array's element count, `shape` says how logical elements map into it. */
enum ParamShape { SHAPE_FLAT = 0, SHAPE_ROWS = 1, SHAPE_LSTM_W = 2, SHAPE_LSTM_B = 3 };
static float* param_ptr(sbr_model* m, int32_t which, uint64_t* count, uint64_t* stored = nullptr, int* shape = nullptr) {
    const uint64_t I = m->hp.num_items, d = (uint64_t)m->d, dl = (uint64_t)m->dl, ng = (uint64_t)m->ng;
    sbr::ModelView& v = m->mv;
    float* p = nullptr;
    uint64_t n = 0, ns = 0;
    int sh = SHAPE_FLAT;
    switch (which) {
        case SBR_PARAM_ITEM_EMBEDDING: p = v.E; n = I * dl; ns = I * d; sh = SHAPE_ROWS; break;
        case SBR_PARAM_ITEM_EMBEDDING_ACC: p = v.Eacc; n = I * dl; ns = I * d; sh = SHAPE_ROWS; break;
        case SBR_PARAM_ITEM_BIAS: p = v.b; n = ns = I; break;
        case SBR_PARAM_ITEM_BIAS_ACC: p = v.bacc; n = ns = I; break;
        case SBR_PARAM_LSTM_W: p = v.W; n = 2 * dl * ng * dl; ns = 2 * d * ng * d; sh = SHAPE_LSTM_W; break;
        case SBR_PARAM_LSTM_W_ACC: p = v.Wacc; n = 2 * dl * ng * dl; ns = 2 * d * ng * d; sh = SHAPE_LSTM_W; break;
        case SBR_PARAM_LSTM_B: p = v.bW; n = ng * dl; ns = ng * d; sh = SHAPE_LSTM_B; break;
        case SBR_PARAM_LSTM_B_ACC: p = v.bWacc; n = ng * dl; ns = ng * d; sh = SHAPE_LSTM_B; break;
        case SBR_PARAM_EWMA_ALPHA: p = v.alpha; n = ng ? 0 : dl; ns = ng ? 0 : d; break;
        case SBR_PARAM_EWMA_ALPHA_ACC: p = v.alpha_acc; n = ng ? 0 : dl; ns = ng ? 0 : d; break;
        case SBR_PARAM_ITEM_EMBEDDING_M: p = v.Em; n = v.Em ? I * dl : 0; ns = v.Em ? I * d : 0; sh = SHAPE_ROWS; break;
        case SBR_PARAM_ITEM_BIAS_M: p = v.bm; n = ns = v.bm ? I : 0; break;
        case SBR_PARAM_LSTM_W_M: p = v.Wm; n = v.Wm ? 2 * dl * ng * dl : 0; ns = v.Wm ? 2 * d * ng * d : 0; sh = SHAPE_LSTM_W; break;
        case SBR_PARAM_LSTM_B_M: p = v.bWm; n = v.bWm ? ng * dl : 0; ns = v.bWm ? ng * d : 0; sh = SHAPE_LSTM_B; break;
        case SBR_PARAM_EWMA_ALPHA_M: p = v.alpha_m; n = v.alpha_m ? dl : 0; ns = v.alpha_m ? d : 0; break;
    }
    *count = n;
    if (stored) *stored = ns;
    if (shape) *shape = sh;
    return p;
}

static bool is_table_optimizer_state(int32_t which) {
    return which == SBR_PARAM_ITEM_EMBEDDING_ACC || which == SBR_PARAM_ITEM_BIAS_ACC || which == SBR_PARAM_ITEM_EMBEDDING_M || which == SBR_PARAM_ITEM_BIAS_M;
}

/* copy between the caller's logical array and the stored (padded) array, host side; to_stored fills the padding with 0 */
static void param_repack(const sbr_model* m, int shape, const float* src, float* dst, bool to_stored) {
    const uint64_t I = m->hp.num_items, d = (uint64_t)m->d, dl = (uint64_t)m->dl, ng = (uint64_t)m->ng;
    auto move = [&](uint64_t logical, uint64_t stored, uint64_t n) {
        if (to_stored) std::memcpy(dst + stored, src + logical, n * 4);
        else std::memcpy(dst + logical, src + stored, n * 4);
    };
    switch (shape) {
        case SHAPE_ROWS:
            for (uint64_t r = 0; r < I; ++r) move(r * dl, r * d, dl);
            break;
        case SHAPE_LSTM_W:
            for (uint64_t kl = 0; kl < 2 * dl; ++kl) {
                const uint64_t k = kl < dl ? kl : d + (kl - dl);
                for (uint64_t g = 0; g < ng; ++g) move(kl * ng * dl + g * dl, k * ng * d + g * d, dl);
            }
            break;
        case SHAPE_LSTM_B:
            for (uint64_t g = 0; g < ng; ++g) move(g * dl, g * d, dl);
            break;
        default:
            move(0, 0, dl);  /* alpha */
            break;
    }
}

sbr_status sbr_model_param_count(const sbr_model* m, int32_t which, uint64_t* out_count) {
    if (!m || !out_count) return SBR_ERR_INVALID_ARGUMENT;
    param_ptr(const_cast<sbr_model*>(m), which, out_count);
    return SBR_OK;
}

sbr_status sbr_model_get_param(sbr_model* m, int32_t which, float* host_out, uint64_t count) {
    if (!m || !host_out) return SBR_ERR_INVALID_ARGUMENT;
    uint64_t n = 0, stored = 0;
    int shape = SHAPE_FLAT;
    float* p = param_ptr(m, which, &n, &stored, &shape);
    if (!p || n != count) return SBR_ERR_INVALID_ARGUMENT;
    if (m->opt_state_partial && is_table_optimizer_state(which)) return SBR_ERR_INVALID_ARGUMENT; /* gather the owners' slices first */
    SBRCHK(enter_reader(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (stored == n) {
        HIPCHK(hipMemcpy(host_out, p, n * 4, hipMemcpyDeviceToHost));
    } else {
        std::vector<float> tmp(stored);
        HIPCHK(hipMemcpy(tmp.data(), p, stored * 4, hipMemcpyDeviceToHost));
        param_repack(m, shape, tmp.data(), host_out, false);
    }
    return SBR_OK;
}

/* selected rows of an item-table block (embeddings and their optimiser state: [n][embedding_dim]; biases: [n]) */
sbr_status sbr_model_get_param_rows(sbr_model* m, int32_t which, const uint32_t* rows, uint64_t n, float* host_out) {
    if (!m || !host_out || (n && !rows)) return SBR_ERR_INVALID_ARGUMENT;
    uint64_t count = 0, stored = 0;
    int shape = SHAPE_FLAT;
    float* p = param_ptr(m, which, &count, &stored, &shape);
    const uint64_t I = m->hp.num_items;
    const bool table = shape == SHAPE_ROWS, bias = shape == SHAPE_FLAT && stored == I && (which == SBR_PARAM_ITEM_BIAS || which == SBR_PARAM_ITEM_BIAS_ACC || which == SBR_PARAM_ITEM_BIAS_M);
    if (!p || !count || (!table && !bias)) return SBR_ERR_INVALID_ARGUMENT;
    if (m->opt_state_partial && is_table_optimizer_state(which)) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(enter_reader(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    const uint64_t w = table ? (uint64_t)m->dl : 1, ws = table ? (uint64_t)m->d : 1;
    for (uint64_t i = 0; i < n; ++i) {
        if (rows[i] >= I) return SBR_ERR_INVALID_ARGUMENT;
        HIPCHK(hipMemcpy(host_out + i * w, p + (uint64_t)rows[i] * ws, w * 4, hipMemcpyDeviceToHost));
    }
    return SBR_OK;
}

sbr_status sbr_model_set_param(sbr_model* m, int32_t which, const float* host_in, uint64_t count) {
    if (!m || !host_in) return SBR_ERR_INVALID_ARGUMENT;
    uint64_t n = 0, stored = 0;
    int shape = SHAPE_FLAT;
    float* p = param_ptr(m, which, &n, &stored, &shape);
    if (!p || n != count) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->param_gen += 1;
    if (stored == n) {
        HIPCHK(hipMemcpy(p, host_in, n * 4, hipMemcpyHostToDevice));
    } else {
        std::vector<float> tmp(stored, 0.0f);
        param_repack(m, shape, host_in, tmp.data(), true);
        HIPCHK(hipMemcpy(p, tmp.data(), stored * 4, hipMemcpyHostToDevice));
    }
    if (which == SBR_PARAM_LSTM_W) {
        sbr::launch_repack_lstm(m->mv, m->stream);
        HIPCHK(hipStreamSynchronize(m->stream));
    }
    return SBR_OK;
}

sbr_status sbr_model_get_epoch(const sbr_model* m, uint64_t* out_global_epoch) {
    if (!m || !out_global_epoch) return SBR_ERR_INVALID_ARGUMENT;
    *out_global_epoch = m->global_epoch;
    return SBR_OK;
}

sbr_status sbr_model_get_counters(const sbr_model* m, uint64_t* out_global_epoch, uint64_t* out_optimizer_steps) {
    if (!m) return SBR_ERR_INVALID_ARGUMENT;
    if (out_global_epoch) *out_global_epoch = m->global_epoch;
    if (out_optimizer_steps) *out_optimizer_steps = m->opt_steps;
    return SBR_OK;
}

sbr_status sbr_model_set_counters(sbr_model* m, uint64_t global_epoch, uint64_t optimizer_steps) {
    if (!m) return SBR_ERR_INVALID_ARGUMENT;
    m->global_epoch = global_epoch;
    m->opt_steps = optimizer_steps;
    return SBR_OK;
}

sbr_status sbr_model_get_rng(const sbr_model* m, uint8_t out_state[16]) {
    if (!m || !out_state) return SBR_ERR_INVALID_ARGUMENT;
    const uint32_t w[4] = {m->rng.x, m->rng.y, m->rng.z, m->rng.w};
    for (int i = 0; i < 4; ++i)
        for (int b = 0; b < 4; ++b) out_state[4 * i + b] = (uint8_t)(w[i] >> (8 * b));
    return SBR_OK;
}

sbr_status sbr_model_set_rng(sbr_model* m, const uint8_t state[16]) {
    if (!m || !state) return SBR_ERR_INVALID_ARGUMENT;
    sbr_xs_seed(&m->rng, state);
    return SBR_OK;
}

sbr_status sbr_model_set_overlap(sbr_model* m, int32_t enable) {
    if (!m) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipStreamSynchronize(m->side));
    HIPCHK(hipStreamSynchronize(m->sorter));
    m->overlap = enable != 0;
    return SBR_OK;
}

sbr_status sbr_model_timing_enable(sbr_model* m, int32_t enable) {
    if (!m) return SBR_ERR_INVALID_ARGUMENT;
    m->timing = enable != 0;
    return SBR_OK;
}

sbr_status sbr_model_timing_select(sbr_model* m, uint32_t family_mask) {
    if (!m) return SBR_ERR_INVALID_ARGUMENT;
    m->timing_mask = family_mask;
    return SBR_OK;
}

sbr_status sbr_model_timing_read(sbr_model* m, double* out_ms, uint64_t* out_launches) {
    if (!m) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    for (auto& tp : m->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, tp.a, tp.b) == hipSuccess) {
            m->ms[tp.family] += (double)ms;
            m->launches[tp.family] += tp.launches;
        }
        hipEventDestroy(tp.a);
        hipEventDestroy(tp.b);
    }
    m->pending.clear();
    for (int f = 0; f < SBR_K_FAMILIES; ++f) {
        if (out_ms) out_ms[f] = m->ms[f];
        if (out_launches) out_launches[f] = m->launches[f];
        m->ms[f] = 0.0;
        m->launches[f] = 0;
    }
    return SBR_OK;
}

/* ---------------------------------------------------------------------------------------------
 * fit
 * ------------------------------------------------------------------------------------------- */
sbr_status sbr_fit_begin(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users,
                         sbr_fit_plan** out) {
    if (!m || !user_ptr || !out) return SBR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    SBRCHK(ensure_device(m));
    const uint64_t T = m->hp.max_sequence_length;
    for (uint64_t u = 0; u < num_users; ++u)
        if (user_ptr[u + 1] < user_ptr[u]) return SBR_ERR_INVALID_ARGUMENT; /* pointers must be non-decreasing */
    const uint64_t nnz = user_ptr[num_users];
    if (nnz && !item_ids) return SBR_ERR_INVALID_ARGUMENT;
    for (uint64_t i = 0; i < nnz; ++i)
        if (item_ids[i] >= m->hp.num_items) return SBR_ERR_INVALID_ARGUMENT;
    /* subsequences = chunks (first chunk short, data.rs:406-431) with len > 2 (sequence_model.rs:76-83) */
    std::vector<uint64_t> start;
    std::vector<uint32_t> len;
    for (uint64_t u = 0; u < num_users; ++u) {
        const uint64_t n = user_ptr[u + 1] - user_ptr[u];
        uint64_t idx = 0;
        while (idx < n) {
            const uint64_t mod = (n - idx) % T, cs = mod == 0 ? T : mod;
            if (cs > 2) { start.push_back(user_ptr[u] + idx); len.push_back((uint32_t)cs); }
            idx += cs;
        }
    }
    const uint64_t nseq = start.size();
    if (nseq == 0) return SBR_ERR_NO_INTERACTIONS; /* :86-88 */
    shuffle_pairs(start.data(), len.data(), nseq, &m->rng); /* :84, model RNG */
    const int ndev = (int)m->hp.num_devices;
    const uint64_t part = nseq / ndev; /* :91; the zip at :94-98 drops the remainder */
    if (part == 0) return SBR_ERR_INVALID_ARGUMENT; /* the reference panics here (chunks_mut(0)) */
    sbr_fit_plan* p = new (std::nothrow) sbr_fit_plan();
    if (!p) return SBR_ERR_OUT_OF_MEMORY;
    m->param_gen += 1; /* every fit opens its plans here: session states of the old parameters go stale */
    p->m = m; p->ndev = ndev; p->rank = (int)m->hp.device_rank; p->T = (int)T;
    p->nseq_total = nseq; p->part_len = part;
    start.resize((size_t)ndev * part);
    len.resize((size_t)ndev * part);
    p->seq_start.swap(start);
    p->seq_len.swap(len);
    p->part_rng.resize(ndev);
    p->fit_seed.resize(ndev);
    for (int q = 0; q < ndev; ++q) { /* :97 — XorShiftRng::from_seed(parameters.rng().gen()) */
        uint8_t seed[16];
        sbr_rand_gen_seed16(&m->rng, seed);
        sbr_xs_seed(&p->part_rng[q], seed);
        /* (reference order: the worker's stream is not touched here — its first use is the first epoch's shuffle, :109) */
        p->fit_seed[q] = m->reference_order ? 0 : sbr_xs_u64(&p->part_rng[q]);
    }
    p->items.assign(item_ids, item_ids + nnz);
    p->bmax = m->hp.batch_sequences;
    p->rmax = p->bmax * (T - 1);
    if (3 * p->rmax >= (1ull << 32) || part * T >= (1ull << 32)) { delete p; return SBR_ERR_INVALID_ARGUMENT; }
    m->open_plans += 1; /* until sbr_fit_plan_destroy, which every later exit goes through */
    sbr_status st = alloc_work(m, p->rmax, p->bmax, true, &p->wb);
    if (st == SBR_OK) { p->block_bytes = block_bytes_for(m, p->rmax); st = dmalloc(&p->block, p->block_bytes); }
    const uint64_t max_entries = 3 * p->rmax; /* only a device's own entries are ever sorted */
    int item_bits = 1;
    while ((1ull << item_bits) < (uint64_t)m->hp.num_items) ++item_bits;
    p->key_bits = 32 + item_bits;
    if (st == SBR_OK) st = dmalloc(&p->keys, max_entries);
    p->exportable_lists = m->shared && m->shared->local_rank >= 0;
    if (st == SBR_OK) {
        if (p->exportable_lists) {
            st = p->own_x[0].alloc(max_entries * sizeof(uint64_t), m->device);
            p->keys_sorted = reinterpret_cast<uint64_t*>(p->own_x[0].ptr);
        } else {
            st = dmalloc(&p->keys_sorted, max_entries);
        }
    }
    if (st == SBR_OK) {
        p->sort_temp_bytes = sbr::sparse_sort_temp_bytes(max_entries, p->key_bits);
        uint8_t* tmp = nullptr;
        st = dmalloc(&tmp, p->sort_temp_bytes);
        p->sort_temp = tmp;
    }
    {   /* a long segment has more than SBR_SEG_CHUNK entries: at most max_entries / chunk of them, and
         * their chunks number at most max_entries / chunk + (number of long segments) */
        const uint64_t cap = max_entries / SBR_SEG_ROUTE + 2, units = cap + max_entries / SBR_SEG_CHUNK + 2; /* routed segments; their chunks */
        p->seg.cap = (uint32_t)cap;
        if (st == SBR_OK) st = dmalloc(&p->seg.counters, 4);
        if (st == SBR_OK) st = dmalloc(&p->seg.long_start, cap);
        if (st == SBR_OK) st = dmalloc(&p->seg.long_end, cap);
        if (st == SBR_OK) st = dmalloc(&p->seg.unit_base, cap + 1);
        if (st == SBR_OK) st = dmalloc(&p->seg.P, units * (uint64_t)m->d);
        if (st == SBR_OK) st = dmalloc(&p->seg.Pb, units);
        if (st == SBR_OK) st = dmalloc(&p->seg.Pf, units);
        if (st == SBR_OK) st = dmalloc(&p->seg.head_pos, max_entries + 1);
        if (st == SBR_OK) st = dmalloc(&p->seg.nheads, 1);
    }
    if (st == SBR_OK && !m->copier && hipStreamCreateWithFlags(&m->copier, hipStreamNonBlocking) != hipSuccess) st = SBR_ERR_HIP;
    p->copy_stream = m->copier;
    for (int i = 0; i < 2 && st == SBR_OK; ++i)
        if (hipEventCreateWithFlags(&p->ep[i].free_event, hipEventDisableTiming) != hipSuccess) st = SBR_ERR_HIP;
    if (st == SBR_OK) st = dmalloc(&p->lag_state, 1 + 2 * T); /* accumulator + (node, staged value) per step: sbr_report.hip */
    if (st == SBR_OK) st = dmalloc(&p->lag_seqsum, p->bmax);
    if (st == SBR_OK && (hipEventCreateWithFlags(&p->ev_seqsum, hipEventDisableTiming) != hipSuccess ||
                         hipEventCreateWithFlags(&p->ev_lagged, hipEventDisableTiming) != hipSuccess ||
                         hipEventCreateWithFlags(&p->ev_hot, hipEventDisableTiming) != hipSuccess)) st = SBR_ERR_HIP;
    if (st == SBR_OK) st = dmalloc(&p->loss_acc, 17);  /* [0] all devices, [1 + q] device q */
    if (st == SBR_OK && m->reference_order) st = dmalloc(&p->ref_rng, 4);
    if (st == SBR_OK) st = dmalloc(&p->phase_clocks, 6);
    if (st == SBR_OK) hipMemsetAsync(p->phase_clocks, 0, 6 * sizeof(unsigned long long), m->stream);
    if (st == SBR_OK) st = dmalloc(&p->ex_acc, 18);    /* [0] examples, [1] negatives scored, [2 + q] examples of device q */
    if (st != SBR_OK) { sbr_fit_plan_destroy(p); return st; }
    hipMemsetAsync(p->lag_state, 0, (1 + 2 * T) * sizeof(float), m->stream); /* the reference builds its loss nodes per fit call */
    hipMemsetAsync(p->loss_acc, 0, 17 * sizeof(double), m->stream);
    hipMemsetAsync(p->ex_acc, 0, 18 * sizeof(unsigned long long), m->stream);
    hipMemsetAsync(p->block, 0, p->block_bytes, m->stream);
    *out = p;
    return SBR_OK;
}

void sbr_fit_plan_destroy(sbr_fit_plan* p) {
    if (!p) return;
    hipSetDevice(p->m->device);
    p->m->param_gen += 1;
    p->m->open_plans -= 1;
    if (p->pending) { p->worker.join(); p->pending = false; }
    hipStreamSynchronize(p->m->side);
    hipStreamSynchronize(p->m->sorter);
    hipStreamSynchronize(p->m->stream);
    for (int i = 0; i < 2; ++i) {
        p->ep[i].dp.release();
        dfree(p->ep[i].d_desc);
        if (p->ep[i].free_event) hipEventDestroy(p->ep[i].free_event);
        hfree(p->ep[i].h_in); hfree(p->ep[i].h_out); hfree(p->ep[i].h_ctr);
        hfree(p->ep[i].h_prev); hfree(p->ep[i].h_steps);
    }
    if (p->copy_stream) hipStreamSynchronize(p->copy_stream); /* the model's: stays */
    p->wb.release();
    for (auto& px : p->xchg_peer) for (auto& b : px) b.release();
    for (auto& b : p->xchg_own) b.release();
    if (p->exportable_lists) { /* the sorted keys and the list are virtual-memory allocations, not hipMalloc'ed */
        for (auto& px : p->peer_x) for (auto& b : px) b.release();
        for (auto& b : p->own_x) b.release();
        p->keys_sorted = nullptr; p->glist = p->gblist = nullptr; p->gfl = nullptr;
    }
    dfree(p->block); dfree(p->keys); dfree(p->keys_sorted); dfree(p->sort_temp);
    dfree(p->loss_acc); dfree(p->ex_acc); dfree(p->phase_clocks); dfree(p->ref_rng);
    dfree(p->lag_state); dfree(p->lag_seqsum);
    if (p->ev_seqsum) hipEventDestroy(p->ev_seqsum);
    if (p->ev_lagged) hipEventDestroy(p->ev_lagged);
    if (p->ev_hot) hipEventDestroy(p->ev_hot);
    dfree(p->seg.counters); dfree(p->seg.long_start); dfree(p->seg.long_end); dfree(p->seg.unit_base);
    dfree(p->seg.P); dfree(p->seg.Pb); dfree(p->seg.Pf);
    dfree(p->seg.head_pos); dfree(p->seg.nheads);
    dfree(p->glist); dfree(p->gblist); dfree(p->gfl); dfree(p->bounds_dev);
    dfree(p->mkeys); dfree(p->mkeys_sorted); dfree(p->msort_temp); dfree(p->mplan); dfree(p->all_bounds_dev);
    delete p;
}

/* Host side of one epoch: ≙ thread_rng.shuffle(partition) (sequence_model.rs:109) for every
 * partition (so that each device also knows the row counts its peers contribute to a step), then
 * packing of this rank's minibatches and upload of the packed index arrays on the copy stream. */
static sbr_status build_epoch(sbr_fit_plan* p, sbr_fit_plan::Epoch& e) {
    sbr_model* m = p->m;
    HIPCHK(hipSetDevice(m->device));
    if (p->ref_rng && p->ref_rng_live) { /* reference order: the stream the steps drew from shuffles the next epoch (:109) */
        HIPCHK(hipStreamSynchronize(m->stream));
        uint32_t st4w[4];
        HIPCHK(hipMemcpy(st4w, p->ref_rng, sizeof(st4w), hipMemcpyDeviceToHost));
        sbr_xorshift& r = p->part_rng[p->rank];
        r.x = st4w[0]; r.y = st4w[1]; r.z = st4w[2]; r.w = st4w[3];
        p->ref_rng_live = false;
    }
    for (int q = 0; q < p->ndev; ++q)
        shuffle_pairs(p->seq_start.data() + (size_t)q * p->part_len, p->seq_len.data() + (size_t)q * p->part_len,
                      p->part_len, &p->part_rng[q]);
    if (p->ref_rng) {
        const sbr_xorshift& r = p->part_rng[p->rank];
        const uint32_t st4w[4] = {r.x, r.y, r.z, r.w};
        HIPCHK(hipMemcpy(p->ref_rng, st4w, sizeof(st4w), hipMemcpyHostToDevice));
    }
    e.epoch_key_epoch = m->global_epoch;
    m->global_epoch += 1;
    const uint64_t B = p->bmax;
    const uint64_t nmb = (p->part_len + B - 1) / B;
    e.num_mb = nmb;
    e.rows_of_dev.assign(nmb * p->ndev, 0);
    for (int q = 0; q < p->ndev; ++q) {
        const uint32_t* ln = p->seq_len.data() + (size_t)q * p->part_len;
        for (uint64_t mb = 0; mb < nmb; ++mb) {
            const uint64_t p0 = mb * B, p1 = std::min(p0 + B, p->part_len);
            uint32_t r = 0;
            for (uint64_t i = p0; i < p1; ++i) r += ln[i] - 1;
            e.rows_of_dev[mb * p->ndev + q] = r;
        }
    }
    const uint64_t* st = p->seq_start.data() + (size_t)p->rank * p->part_len;
    const uint32_t* ln = p->seq_len.data() + (size_t)p->rank * p->part_len;
    e.mbs.resize(nmb);
    e.off_host.clear();
    uint64_t total_rows = 0;
    for (uint64_t i = 0; i < p->part_len; ++i) total_rows += ln[i] - 1;
    if (total_rows > e.h_rows_cap || p->part_len > e.h_seq_cap) {
        hfree(e.h_in); hfree(e.h_out); hfree(e.h_ctr); hfree(e.h_prev); hfree(e.h_steps);
        e.h_in = e.h_out = e.h_ctr = nullptr; e.h_prev = e.h_steps = nullptr;
        e.h_rows_cap = e.h_seq_cap = 0;
        const size_t rb = (size_t)(total_rows ? total_rows : 1) * 4, sb = (size_t)(p->part_len ? p->part_len : 1) * 4;
        if (hmalloc(&e.h_in, rb) != hipSuccess || hmalloc(&e.h_out, rb) != hipSuccess || hmalloc(&e.h_ctr, rb) != hipSuccess ||
            hmalloc(&e.h_prev, rb) != hipSuccess || hmalloc(&e.h_steps, sb) != hipSuccess)
            return SBR_ERR_OUT_OF_MEMORY;
        e.h_rows_cap = total_rows; e.h_seq_cap = p->part_len;
    }
    /* The staging buffers are read by the DMA of two epochs ago at the latest, which was waited for below
     * before that epoch's build returned: they are free.  Packing (time-major, sequences by length
     * descending, stable): counting sort of the minibatch, then the rows are written in row order — step t
     * outer, sequence inner — so every output array is filled sequentially; the t range is cut into pieces
     * of about equal row count for a few worker threads. */
    uint64_t row_base = 0, seq_base = 0;
    const int T = p->T;
    std::vector<int> cnt(T + 2), pos(T + 2), order;
    for (uint64_t mb = 0; mb < nmb; ++mb) {
        const uint64_t p0 = mb * B, p1 = std::min(p0 + B, p->part_len);
        const int nb = (int)(p1 - p0);
        std::fill(cnt.begin(), cnt.end(), 0);
        for (int i = 0; i < nb; ++i) cnt[ln[p0 + i] - 1]++;
        int acc = 0;
        for (int l = T; l >= 0; --l) { pos[l] = acc; acc += cnt[l]; }
        order.resize(nb);
        for (int i = 0; i < nb; ++i) order[pos[ln[p0 + i] - 1]++] = i;
        int* steps = e.h_steps + seq_base;
        for (int b = 0; b < nb; ++b) steps[b] = (int)ln[p0 + order[b]] - 1;
        const int Tm = nb ? steps[0] : 0;
        const size_t off_base = e.off_host.size();
        e.off_host.resize(off_base + Tm + 1);
        int* off = e.off_host.data() + off_base;
        off[0] = 0;
        {
            int alive = nb;
            for (int t = 0; t < Tm; ++t) {
                while (alive > 0 && steps[alive - 1] <= t) --alive;
                off[t + 1] = off[t] + alive;
            }
        }
        const int R = off[Tm];
        uint32_t *in_idx = e.h_in + row_base, *out_idx = e.h_out + row_base, *ctr = e.h_ctr + row_base;
        int* prev_row = e.h_prev + row_base;
        auto fill = [&](int t0, int t1) {
            for (int t = t0; t < t1; ++t) {
                const int alive = off[t + 1] - off[t];
                const int r0 = off[t], rp = t ? off[t - 1] : 0;
                for (int b = 0; b < alive; ++b) {
                    const uint64_t src = p0 + (uint64_t)order[b];
                    const uint32_t* it = p->items.data() + st[src];
                    in_idx[r0 + b] = it[t];
                    out_idx[r0 + b] = it[t + 1];
                    ctr[r0 + b] = (uint32_t)(src * (uint64_t)T + (uint64_t)t);
                    prev_row[r0 + b] = t ? rp + b : -1;
                }
            }
        };
        static const int pack_threads = [] {  /* at most half of the host's cores */
            const unsigned hc = std::thread::hardware_concurrency();
            const int half = hc >= 2 ? (int)(hc / 2) : 1;
            return half < SBR_PACK_THREADS ? half : SBR_PACK_THREADS;
        }();
        const int nthreads = R > (1 << 18) ? pack_threads : 1;
        if (nthreads == 1) fill(0, Tm);
        else {
            std::vector<std::thread> workers;
            int t0 = 0;
            for (int k = 0; k < nthreads; ++k) {
                int t1 = t0;
                const long long target = (long long)R * (k + 1) / nthreads;
                while (t1 < Tm && off[t1] < target) ++t1;
                if (k == nthreads - 1) t1 = Tm;
                if (t1 > t0) workers.emplace_back(fill, t0, t1);
                t0 = t1;
            }
            for (auto& w : workers) w.join();
        }
        sbr_fit_plan::Mb& d = e.mbs[mb];
        d.R = R; d.B = nb; d.Tm = Tm;
        d.row_base = row_base; d.seq_base = seq_base; d.off_base = off_base;
        row_base += (uint64_t)R;
        seq_base += (uint64_t)nb;
    }
    /* the GPU may still be reading this buffer's previous contents (two epochs ago) */
    if (e.free_recorded) {
        HIPCHK(hipEventSynchronize(e.free_event));
        e.free_recorded = false;
    }
    if (row_base > e.rows_cap || e.off_host.size() > e.off_cap || seq_base > e.seq_cap) {
        e.dp.release();
        SBRCHK(dmalloc(&e.dp.in_idx, row_base));
        SBRCHK(dmalloc(&e.dp.out_idx, row_base));
        SBRCHK(dmalloc(&e.dp.ctr, row_base));
        SBRCHK(dmalloc(&e.dp.prev_row, row_base));
        SBRCHK(dmalloc(&e.dp.off, e.off_host.size()));
        SBRCHK(dmalloc(&e.dp.steps, seq_base));
        e.rows_cap = row_base; e.off_cap = e.off_host.size(); e.seq_cap = seq_base;
    }
    hipStream_t cs = p->copy_stream;
    SBRCHK(stream_head(m, cs));
    e.desc_host.clear();
    if (B == 1 && p->ndev == 1) {
        e.desc_host.resize(nmb);
        for (uint64_t mb = 0; mb < nmb; ++mb) {
            const sbr_fit_plan::Mb& d = e.mbs[mb];
            e.desc_host[mb] = sbr::StepDesc{(uint32_t)d.R, (uint32_t)d.row_base, (uint32_t)d.off_base, (uint32_t)d.seq_base};
        }
        if (nmb > e.desc_cap) {
            dfree(e.d_desc);
            e.d_desc = nullptr; e.desc_cap = 0;
            SBRCHK(dmalloc(&e.d_desc, nmb));
            e.desc_cap = nmb;
        }
        HIPCHK(hipMemcpyAsync(e.d_desc, e.desc_host.data(), nmb * sizeof(sbr::StepDesc), hipMemcpyHostToDevice, cs));
    }
    HIPCHK(hipMemcpyAsync(e.dp.in_idx, e.h_in, row_base * 4, hipMemcpyHostToDevice, cs));
    HIPCHK(hipMemcpyAsync(e.dp.out_idx, e.h_out, row_base * 4, hipMemcpyHostToDevice, cs));
    HIPCHK(hipMemcpyAsync(e.dp.ctr, e.h_ctr, row_base * 4, hipMemcpyHostToDevice, cs));
    HIPCHK(hipMemcpyAsync(e.dp.prev_row, e.h_prev, row_base * 4, hipMemcpyHostToDevice, cs));
    HIPCHK(hipMemcpyAsync(e.dp.off, e.off_host.data(), e.off_host.size() * 4, hipMemcpyHostToDevice, cs));
    HIPCHK(hipMemcpyAsync(e.dp.steps, e.h_steps, seq_base * 4, hipMemcpyHostToDevice, cs));
    HIPCHK(hipStreamSynchronize(cs));
    return SBR_OK;
}

sbr_status sbr_fit_epoch_prepare(sbr_fit_plan* p, uint64_t* out_num_minibatches) {
    if (!p) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    SBRCHK(ensure_device(m));
    if (p->pending) { /* the next epoch was prefetched: hand the current buffers back and switch */
        p->worker.join();
        p->pending = false;
        SBRCHK(p->pending_status);
        sbr_fit_plan::Epoch& old = p->ep[p->cur];
        HIPCHK(hipEventRecord(old.free_event, m->stream));
        old.free_recorded = true;
        p->cur ^= 1;
    } else {
        sbr_fit_plan::Epoch& e = p->ep[p->cur];
        HIPCHK(hipEventRecord(e.free_event, m->stream));
        e.free_recorded = true;
        SBRCHK(build_epoch(p, e));
    }
    if (out_num_minibatches) *out_num_minibatches = p->ep[p->cur].num_mb;
    return SBR_OK;
}

sbr_status sbr_fit_epoch_prefetch(sbr_fit_plan* p) {
    if (!p || p->pending) return SBR_ERR_INVALID_ARGUMENT;
    if (p->ref_rng) return SBR_OK; /* reference order: the next epoch's shuffle continues the stream this epoch's steps draw from */
    p->pending = true;
    p->pending_status = SBR_OK;
    p->worker = std::thread([p]() { p->pending_status = build_epoch(p, p->ep[p->cur ^ 1]); });
    return SBR_OK;
}

sbr_status sbr_fit_minibatch_rows(const sbr_fit_plan* p, uint64_t minibatch, uint64_t* out_rows) {
    if (!p || !out_rows || minibatch >= p->ep[p->cur].num_mb) return SBR_ERR_INVALID_ARGUMENT;
    *out_rows = (uint64_t)p->ep[p->cur].mbs[minibatch].R;
    return SBR_OK;
}

/* The main stream joins what earlier steps left on other streams, as far as the caller is about to read or overwrite it (`needs`: the
 * table above StepLeft) and it is still owed: the only place a step function makes the main stream wait (`open`: as stream_wait) */
static sbr_status join_main(sbr_fit_plan* p, unsigned needs, ScopedTimer* open = nullptr) {
    sbr_model* m = p->m;
    const struct { unsigned needs; hipEvent_t ev; } joins[] = {
        {LAG_STATE, p->ev_lagged}, {KEYS | HEADER, m->ev_sorted}, {DENSE, m->ev_join}, {TABLE, p->ev_hot}};
    for (const auto& j : joins) {
        if (!(needs & p->left.owed & j.needs)) continue;
        SBRCHK(stream_wait(m, m->stream, j.ev, open));
        p->left.owed &= ~j.needs;
    }
    return SBR_OK;
}

/* blk.dense complete on the main stream: joins the GEMM and, if its chunk partials are still unreduced, reduces them */
static sbr_status ensure_dense_reduced(sbr_fit_plan* p) {
    SBRCHK(join_main(p, DENSE));
    if (p->left.dense_unreduced_chunks > 0) {
        sbr::launch_dense_reduce(p->m->mv, p->wb.v, p->left.dense_unreduced_chunks, block_view(p->m, p->block, p->rmax), p->m->stream);
        p->left.dense_unreduced_chunks = 0;
    }
    return SBR_OK;
}

/* the step's last consumer has run (or the block has been overwritten): its form says nothing any more; what is owed stays owed */
static void step_consumed(sbr_fit_plan* p) {
    p->left = StepLeft{StepSchedule{}, 0, p->left.owed};
}

/* no side effects, no HIP calls; fuse_back: called under sbr_fit_step, where nobody looks at the block between the two halves */
static StepSchedule step_schedule(const sbr_fit_plan* p, const sbr_fit_plan::Mb& mb, bool fuse_back) {
    const sbr_model* m = p->m;
    const bool one = p->ndev == 1, warp = m->hp.loss == SBR_LOSS_WARP;
    constexpr int small_rows = 1365;
    StepSchedule s;
    s.overlap = m->overlap && mb.R > small_rows;
    s.dense_on = s.overlap ? m->side : m->stream;
    s.sort_on = s.overlap ? m->sorter : m->stream;
    const bool small_tail = (m->step_fusion >= 1 || m->reference_order) && !s.overlap && (one || m->reference_order) &&
                            sbr::small_tail_shape_ok(m->mv, (int)mb.B, (int)mb.R, m->reference_order);
    s.sort_at = small_tail ? SORT_IN_SCORE : !warp ? SORT_AT_START : s.overlap ? SORT_AFTER_BPTT : SORT_AFTER_SCORE;
    s.side_header = s.overlap && warp;
    s.ewma_fused = !m->ng && !warp && mb.R > 0 && !m->reference_order;
    s.fuse_lag = !s.overlap && mb.B <= SBR_HEADER_LAG_MAX_B;
    s.dw_deferred = m->step_fusion >= 1 && fuse_back && !s.overlap && one && sbr::small_back_shape_ok(m->mv, (int)mb.R) && (m->ng || mb.B <= 256);
    s.hot_prelist = one && s.overlap && fuse_back && 3ull * (uint64_t)mb.R > 4096;
    s.header_accumulates = one;
    return s;
}

static sbr_status step_local(sbr_fit_plan* p, uint64_t minibatch, bool fuse_back) {
    if (minibatch >= p->ep[p->cur].num_mb) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    SBRCHK(ensure_device(m));
    const sbr_fit_plan::Epoch& ep = p->ep[p->cur];
    const sbr_fit_plan::Mb& mb = ep.mbs[minibatch];
    const sbr::MbView mv = mb_view(p, minibatch);
    const sbr::BlockView bv = block_view(m, p->block, p->rmax);
    const int* off_host = ep.off_host.data() + mb.off_base;
    SBRCHK(stream_head(m, m->stream));
    const StepSchedule s = step_schedule(p, mb, fuse_back);
    StepLeft& left = p->left = StepLeft{s, 0, p->left.owed};
    const uint64_t epoch_key = sbr_epoch_key(p->fit_seed[p->rank], ep.epoch_key_epoch);
    double* const loss_acc = s.header_accumulates ? p->loss_acc : nullptr;
    unsigned long long* const ex_acc = s.header_accumulates ? p->ex_acc : nullptr;
    const sbr::SmallTail tail{bv.header, loss_acc, ex_acc, p->lag_state, p->keys_sorted, p->seg.head_pos, p->seg.nheads};
    auto queue_sort = [&]() -> sbr_status {
        hipStream_t on = s.sort_on;
        if (s.overlap) {
            /* everything before: the previous step's readers of the keys, this step's score (a step with a side header has
             * recorded the event itself, before it queued the backward pass) */
            if (s.sort_at == SORT_AT_START) HIPCHK(hipEventRecord(m->ev_scored, m->stream));
            SBRCHK(stream_wait(m, on, m->ev_scored));
        }
        if (s.side_header) { /* the step's loss bookkeeping rides on the ordering's stream: nothing on the main stream waits for it */
            sbr::launch_seq_loss(mv, p->wb.v.loss, p->lag_seqsum, p->lag_state, mb.B, on);
            sbr::launch_block_header(m->mv, bv, p->wb.v, mv, mb.R, loss_acc, ex_acc, nullptr, on);
        }
        {
            ScopedTimer t(m, SBR_K_SPARSE_SORT, 1, on);
            sbr::launch_own_sort(bv, (uint32_t)mb.R, p->keys, p->keys_sorted, p->sort_temp, p->sort_temp_bytes, p->key_bits, p->seg, on,
                                 s.sort_at == SORT_AT_START ? &mv : nullptr, epoch_key, m->hp.num_items);
        }
        if (s.overlap) { /* on the main stream the update is ordered behind the sort anyway: no event */
            HIPCHK(hipEventRecord(m->ev_sorted, on));
            left.owed |= KEYS | HEADER;
            if (s.hot_prelist) sbr::launch_seg_prelist(p->seg, on);
        }
        return SBR_OK;
    };
    if (s.sort_at == SORT_AT_START) SBRCHK(queue_sort());
    if (s.small_tail()) SBRCHK(join_main(p, LAG_STATE)); /* an earlier step's chain on the sorter still owns lag_state */
    if (s.ewma_fused) {
        ScopedTimer t(m, SBR_K_SCORE, 1);
        sbr::launch_ewma_sequences(m->mv, mv, bv, p->wb.v, epoch_key, mb.R, m->stream, s.small_tail() ? &tail : nullptr);
    } else {
        {
            ScopedTimer t(m, SBR_K_RECURRENT_FWD, m->ng && m->d > 128 ? (uint64_t)mb.Tm : 1); /* d <= 128: one sequence-resident launch */
            sbr::launch_recurrent_forward(m->mv, mv, bv.H, p->wb.v, mb.Tm, off_host, m->stream);
        }
        ScopedTimer t(m, SBR_K_SCORE, 1);
        if (m->reference_order) {
            if (!p->ref_rng || !s.small_tail() || !sbr::launch_score_reference_order(m->mv, mv, bv, p->wb.v, p->ref_rng, mb.R, m->stream, tail))
                return SBR_ERR_UNSUPPORTED;
            p->ref_rng_live = true;
        } else {
            sbr::launch_score(m->mv, mv, bv, p->wb.v, epoch_key, mb.R, m->stream, s.small_tail() ? &tail : nullptr);
        }
    }
    if (s.side_header) {
        HIPCHK(hipEventRecord(m->ev_scored, m->stream)); /* right behind the score kernel */
    } else if (!s.small_tail()) { /* (small tail: header and lagged figure are done by the score launch) */
        SBRCHK(join_main(p, LAG_STATE)); /* the previous step's chain may still be running on the sorter: it owns lag_state / lag_seqsum */
        if (!s.fuse_lag) {
            sbr::launch_seq_loss(mv, p->wb.v.loss, p->lag_seqsum, p->lag_state, mb.B, m->stream);
            if (s.overlap) HIPCHK(hipEventRecord(p->ev_seqsum, m->stream));
        }
        sbr::launch_block_header(m->mv, bv, p->wb.v, mv, mb.R, loss_acc, ex_acc, s.fuse_lag ? p->lag_state : nullptr, m->stream);
    }
    if (s.sort_at == SORT_AFTER_SCORE) SBRCHK(queue_sort());
    if (!s.ewma_fused) {
        ScopedTimer t(m, SBR_K_RECURRENT_BWD, m->ng && m->d > 128 ? 2 * (uint64_t)mb.Tm : 1);
        sbr::launch_recurrent_backward(m->mv, mv, bv, p->wb.v, mb.Tm, mb.R, mb.B, off_host, m->stream);
    }
    if (s.sort_at == SORT_AFTER_BPTT) SBRCHK(queue_sort());
    if (s.overlap) { /* the side stream starts behind BPTT; joined by whoever reads blk.dense first (join_main DENSE) */
        HIPCHK(hipEventRecord(m->ev_fork, m->stream));
        SBRCHK(stream_wait(m, s.dense_on, m->ev_fork));
    }
    if (!s.dw_deferred) {
        /* one device: the ordered reduction of the chunk partials is left to the consumer — the optimiser step folds it into
         * the dense update's launch (sbr_fit_step_apply); the exchange halves and the debug fetch reduce on demand */
        ScopedTimer t(m, SBR_K_DENSE_GRAD, 1, s.dense_on);
        left.dense_unreduced_chunks = sbr::launch_dense_gradient(m->mv, mv, bv, p->wb.v, mb.R, mb.B, s.dense_on, /*defer_reduce=*/p->ndev == 1);
    }
    if (s.overlap) {
        HIPCHK(hipEventRecord(m->ev_join, s.dense_on));
        left.owed |= DENSE;
    }
    if (!s.fuse_lag) {
        if (s.overlap && !s.side_header) SBRCHK(stream_wait(m, s.sort_on, p->ev_seqsum)); /* (side_header: same stream as seq_loss) */
        sbr::launch_lagged_chain(mv, p->lag_seqsum, mb.B, p->lag_state, s.sort_on);
        if (s.overlap) {
            HIPCHK(hipEventRecord(p->ev_lagged, s.sort_on));
            left.owed |= LAG_STATE;
        }
    }
    p->last_R = mb.R;
    p->last_block = p->block;
    HIPCHK(hipGetLastError());
    return SBR_OK;
}

sbr_status sbr_fit_step_local(sbr_fit_plan* p, uint64_t minibatch) { return p ? step_local(p, minibatch, false) : SBR_ERR_INVALID_ARGUMENT; }

/* single device: optimiser step straight from the local block */
sbr_status sbr_fit_step_apply(sbr_fit_plan* p, uint64_t minibatch) {
    if (!p || minibatch >= p->ep[p->cur].num_mb || p->ndev != 1) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    SBRCHK(ensure_device(m));
    const uint8_t* all = p->block;
    SBRCHK(stream_head(m, m->stream));
    begin_optimizer_step(m);
    const StepSchedule s = p->left.form;
    const sbr::BlockView bv = block_view(m, p->block, p->rmax);
    const uint32_t R = p->ep[p->cur].rows_of_dev[minibatch];
    if (!s.header_accumulates) sbr::launch_accumulate_loss(all, p->block_bytes, 1, p->loss_acc, p->ex_acc, m->stream);
    if (s.dw_deferred) { /* small LSTM step: dense gradient + dense update + sparse update in one launch */
        ScopedTimer t(m, SBR_K_SPARSE_UPDATE, 1);
        SBRCHK(join_main(p, KEYS, &t));
        sbr::launch_small_back(m->mv, mb_view(p, minibatch), bv, p->wb.v, R, p->keys_sorted, p->seg, m->stream);
    } else {
        {
            ScopedTimer t(m, SBR_K_SPARSE_UPDATE, 1);
            SBRCHK(join_main(p, KEYS, &t));
            sbr::SegScratch sc = p->seg;
            sc.prelisted = s.hot_prelist ? 1u : 0u;
            sbr::launch_seg_apply(m->mv, bv, R, p->keys_sorted, sc, m->stream);
            if (s.hot_prelist) { /* the listed hot rows: chunk partials + ordered finish on the ordering's stream (behind the list, and
                                  * behind BPTT: ev_fork), beside the short segments' pass — disjoint table rows */
                SBRCHK(stream_wait(m, m->sorter, m->ev_fork, &t));
                sbr::launch_seg_hot_apply(m->mv, bv, p->keys_sorted, sc, m->sorter);
                HIPCHK(hipEventRecord(p->ev_hot, m->sorter));
                p->left.owed |= TABLE;
                SBRCHK(join_main(p, TABLE, &t));
            }
        }
        SBRCHK(join_main(p, DENSE));
        ScopedTimer t(m, SBR_K_DENSE_UPDATE, 1);
        if (p->left.dense_unreduced_chunks > 0) /* ordered reduction of the chunk partials + dense update in ONE launch */
            sbr::launch_dense_reduce_apply(m->mv, p->wb.v, p->left.dense_unreduced_chunks, bv, m->stream);
        else sbr::launch_dense_apply(m->mv, all, p->block_bytes, dense_offset_bytes(m, p->rmax), 1, m->stream);
    }
    step_consumed(p);
    HIPCHK(hipGetLastError());
    return SBR_OK;
}

sbr_status sbr_fit_step(sbr_fit_plan* p, uint64_t minibatch) {
    if (!p || p->ndev != 1) return SBR_ERR_INVALID_ARGUMENT; /* multi-device: the owner-reduce halves below, driven by the host */
    SBRCHK(step_local(p, minibatch, /*fuse_back=*/true));
    return sbr_fit_step_apply(p, minibatch);
}

/* `count` consecutive optimiser steps starting at `first`.  One sequence per step at d <= 32 (the reference's own schedule,
 * sequence_model.rs:111-169) with EWMA, a single-negative loss and Adagrad: runs of up to SBR_EPOCH_STEPS_PER_LAUNCH steps are ONE
 * launch each (sbr::launch_epoch_steps) — same bits as `count` calls of sbr_fit_step, which is what every other shape gets. */
#ifndef SBR_EPOCH_STEPS_PER_LAUNCH
#define SBR_EPOCH_STEPS_PER_LAUNCH 8192 /* a launch stays well under a second (a one-sequence step is 5-100 us) */
#endif
sbr_status sbr_fit_steps(sbr_fit_plan* p, uint64_t first, uint64_t count) {
    if (!p || p->ndev != 1) return SBR_ERR_INVALID_ARGUMENT;
    sbr_fit_plan::Epoch& ep = p->ep[p->cur];
    if (first > ep.num_mb || count > ep.num_mb - first) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    const bool runs_ok = m->step_fusion >= 2 && !m->timing && !m->reference_order && p->bmax == 1 && ep.d_desc && ep.desc_host.size() == ep.num_mb;
    const bool ewma_runs = runs_ok && sbr::epoch_steps_shape_ok(m->mv, p->T - 1);
    const bool lstm_runs = runs_ok && !ewma_runs && sbr::lstm_steps_shape_ok(m->mv, p->T - 1);
    if (!ewma_runs && !lstm_runs) {
        for (uint64_t mb = first; mb < first + count; ++mb) SBRCHK(sbr_fit_step(p, mb));
        return SBR_OK;
    }
    if (!count) return SBR_OK;
    SBRCHK(ensure_device(m));
    const sbr::BlockView bv = block_view(m, p->block, p->rmax);
    const sbr::EpochView ev{ep.dp.off, ep.dp.steps, ep.dp.prev_row, ep.dp.in_idx, ep.dp.out_idx, ep.dp.ctr, ep.d_desc};
    const sbr::SmallTail tail{bv.header, p->loss_acc, p->ex_acc, p->lag_state, p->keys_sorted, p->seg.head_pos, p->seg.nheads};
    const uint64_t epoch_key = sbr_epoch_key(p->fit_seed[p->rank], ep.epoch_key_epoch);
    const uint32_t row_cap = ewma_runs ? (uint32_t)(p->T - 1) : (uint32_t)sbr::lstm_steps_max_rows();
    /* maximal runs of consecutive steps the one-launch form takes (the LSTM form: steps of at most row_cap rows); a longer step goes
     * through the separate launches and the next run starts behind it */
    uint64_t b = first;
    const uint64_t end = first + count;
    while (b < end) {
        if (ep.desc_host[b].rows > row_cap) {
            SBRCHK(sbr_fit_step(p, b));
            ++b;
            continue;
        }
        uint64_t e = b;
        uint32_t run_max = 0;
        while (e < end && e - b < SBR_EPOCH_STEPS_PER_LAUNCH && ep.desc_host[e].rows <= row_cap) {
            run_max = std::max(run_max, ep.desc_host[e].rows);
            ++e;
        }
        SBRCHK(join_main(p, KEYS | HEADER | DENSE | LAG_STATE)); /* the run writes them all (a larger step before may still own them) */
        SBRCHK(stream_head(m, m->stream));
        if (ewma_runs) sbr::launch_epoch_steps(m->mv, ev, bv, p->wb.v, epoch_key, tail, (int)b, (int)e, p->T - 1, p->phase_clocks, m->stream);
        else sbr::launch_lstm_steps(m->mv, ev, bv, p->wb.v, epoch_key, tail, (int)b, (int)e, p->T - 1, (int)run_max, p->phase_clocks, m->stream);
        m->opt_steps += e - b; /* Adagrad: no per-step host-side corrections */
        step_consumed(p);
        p->last_R = ep.mbs[e - 1].R;
        p->last_block = p->block;
        b = e;
    }
    HIPCHK(hipGetLastError());
    return SBR_OK;
}

sbr_status sbr_fit_debug_phase_clocks(sbr_fit_plan* p, uint64_t out[6]) {
    if (!p || !out) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(p->m));
    HIPCHK(hipStreamSynchronize(p->m->stream));
    HIPCHK(hipMemcpy(out, p->phase_clocks, 6 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return SBR_OK;
}

/* Reference order across devices (sequence_model.rs:163-166; wyrm's SynchronizedOptimizer as recalled): the workers rendezvous, then
 * every worker's gradient goes in as its OWN optimiser step, one after the other in worker order — n Adagrad applications per step
 * (G += g_q^2 each) where the contract adds the devices' gradients and applies one.  device_blocks: the n devices' local blocks of
 * this step, gathered (block q at q * block bytes); every replica applies the same sequence and stays bit-identical. */
sbr_status sbr_fit_step_apply_blocks_in_order(sbr_fit_plan* p, uint64_t minibatch, const void* device_blocks) {
    if (!p || !device_blocks || minibatch >= p->ep[p->cur].num_mb || !p->m->reference_order) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    SBRCHK(ensure_device(m));
    const uint8_t* all = reinterpret_cast<const uint8_t*>(device_blocks);
    SBRCHK(join_main(p, DENSE));
    sbr::launch_accumulate_loss(all, p->block_bytes, p->ndev, p->loss_acc, p->ex_acc, m->stream);
    for (int q = 0; q < p->ndev; ++q) {
        const uint32_t R = p->ep[p->cur].rows_of_dev[minibatch * p->ndev + q];
        uint8_t* base = const_cast<uint8_t*>(all) + (size_t)q * p->block_bytes;
        const sbr::BlockView bv = block_view(m, base, p->rmax);
        begin_optimizer_step(m);
        sbr::launch_own_sort(bv, R, p->keys, p->keys_sorted, p->sort_temp, p->sort_temp_bytes, p->key_bits, p->seg, m->stream, nullptr, 0, 0);
        sbr::SegScratch sc = p->seg;
        sc.prelisted = 0u;
        sbr::launch_seg_apply(m->mv, bv, R, p->keys_sorted, sc, m->stream);
        sbr::launch_dense_apply(m->mv, base, p->block_bytes, dense_offset_bytes(m, p->rmax), 1, m->stream);
    }
    step_consumed(p);
    HIPCHK(hipGetLastError());
    return SBR_OK;
}

sbr_status sbr_fit_block_bytes(const sbr_fit_plan* p, uint64_t* out_bytes) {
    if (!p || !out_bytes) return SBR_ERR_INVALID_ARGUMENT;
    *out_bytes = p->block_bytes;
    return SBR_OK;
}

sbr_status sbr_model_set_reference_order(sbr_model* m, int32_t on) {
    if (!m) return SBR_ERR_INVALID_ARGUMENT;
    if (on && (m->hp.batch_sequences != 1 || !sbr::reference_order_shape_ok(m->d, (int)m->hp.max_sequence_length - 1) ||
               (m->hp.num_devices != 1 && (m->hp.parallelism != SBR_PAR_SYNCHRONOUS || m->shared))))
        return SBR_ERR_UNSUPPORTED; /* one sequence per step whose h rows + candidate window fit one workgroup's LDS (255 rows at d <= 64, 220 at
                                     * d = 128, 80 at d = 256); several workers: Synchronous, replicated */
    m->reference_order = on != 0;
    return SBR_OK;
}

sbr_status sbr_model_set_step_fusion(sbr_model* m, int32_t level) {
    if (!m || level < 0 || level > 2) return SBR_ERR_INVALID_ARGUMENT;
    m->step_fusion = level;
    return SBR_OK;
}

/* ---- multi-device owner-reduce protocol ------------------------------------------ */
static uint64_t slice_rows(const sbr_fit_plan* p) { return ((uint64_t)p->m->hp.num_items + p->ndev - 1) / p->ndev; }

sbr_status sbr_fit_chunk_bytes(const sbr_fit_plan* p, uint64_t* out_bytes) {
    if (!p || !out_bytes) return SBR_ERR_INVALID_ARGUMENT;
    *out_bytes = slice_rows(p) * ((uint64_t)p->m->d + 2) * 4;
    return SBR_OK;
}

sbr_status sbr_fit_dense_bytes(const sbr_fit_plan* p, uint64_t* out_bytes) {
    if (!p || !out_bytes) return SBR_ERR_INVALID_ARGUMENT;
    *out_bytes = (8 + dense_count(p->m)) * 4;
    return SBR_OK;
}

sbr_status sbr_fit_step_scatter(sbr_fit_plan* p, uint64_t minibatch, void* device_send) {
    if (!p || !device_send || minibatch >= p->ep[p->cur].num_mb) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    /* reference order with several workers is n optimiser applications per step in worker order plus an exchange of the workers'
     * generator states per epoch: only the single-process group driver sequences that (sbr_fit_step_apply_blocks_in_order).  The
     * summed-gradient exchange would silently give neither order. */
    if (m->reference_order && p->ndev > 1) return SBR_ERR_UNSUPPORTED;
    SBRCHK(ensure_device(m));
    const sbr::BlockView bv = block_view(m, p->block, p->rmax);
    const uint32_t R = p->ep[p->cur].rows_of_dev[minibatch * p->ndev + p->rank];
    {
        ScopedTimer t(m, SBR_K_SPARSE_UPDATE, 1);
        SBRCHK(join_main(p, KEYS, &t));
        sbr::launch_seg_scatter(m->mv, bv, R, p->ndev, slice_rows(p), device_send, p->keys_sorted, p->seg, m->stream);
    }
    HIPCHK(hipGetLastError());
    return SBR_OK;
}

/* small dense block = [8-word header | dense grads]; joins the side stream's dense-gradient GEMM, so
 * calling it late (after the chunk all-to-all has been queued) lets that GEMM overlap the transfer */
sbr_status sbr_fit_step_dense(sbr_fit_plan* p, void* device_dense_out) {
    if (!p || !device_dense_out) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    SBRCHK(ensure_device(m));
    const sbr::BlockView bv = block_view(m, p->block, p->rmax);
    SBRCHK(ensure_dense_reduced(p));
    SBRCHK(join_main(p, HEADER)); /* (side_header: written on the sorter; not left to the caller having run sbr_fit_step_scatter first) */
    HIPCHK(hipMemcpyAsync(device_dense_out, bv.header, 32, hipMemcpyDeviceToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(reinterpret_cast<uint8_t*>(device_dense_out) + 32, bv.dense, dense_count(m) * 4,
                          hipMemcpyDeviceToDevice, m->stream));
    HIPCHK(hipGetLastError());
    return SBR_OK;
}

static sbr::ChunkPtrs contiguous_chunks(const sbr_fit_plan* p, const void* base) {
    sbr::ChunkPtrs c;
    const uint64_t chunk = slice_rows(p) * ((uint64_t)p->m->d + 2) * 4;
    for (int q = 0; q < 16; ++q) c.p[q] = q < p->ndev ? reinterpret_cast<const uint8_t*>(base) + (size_t)q * chunk : nullptr;
    return c;
}

sbr_status sbr_fit_step_owner_reduce(sbr_fit_plan* p, const void* device_recv, void* device_own_chunk) {
    if (!p || !device_recv || !device_own_chunk) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    SBRCHK(ensure_device(m));
    {
        ScopedTimer t(m, SBR_K_SPARSE_UPDATE, 1);
        sbr::launch_owner_reduce(m->mv, contiguous_chunks(p, device_recv), p->ndev, slice_rows(p), device_own_chunk, m->stream);
    }
    HIPCHK(hipGetLastError());
    return SBR_OK;
}

sbr_status sbr_fit_step_owner_reduce_on(sbr_fit_plan* p, const void* device_recv, void* device_own_chunk, void* hip_stream) {
    if (!p || !device_recv || !device_own_chunk) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    SBRCHK(ensure_device(m));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    {
        ScopedTimer t(m, SBR_K_SPARSE_UPDATE, 1, st);
        sbr::launch_owner_reduce(m->mv, contiguous_chunks(p, device_recv), p->ndev, slice_rows(p), device_own_chunk, st);
    }
    HIPCHK(hipGetLastError());
    return SBR_OK;
}

/* the part of an exchanged step that every device applies identically: step counter, loss header,
 * dense parameters (device-order sum of the gathered dense blocks) */
static sbr_status apply_dense_blocks(sbr_fit_plan* p, const void* device_dense_all, bool begins_step = true) {
    sbr_model* m = p->m;
    const uint64_t db = (8 + dense_count(m)) * 4;
    const uint8_t* dall = reinterpret_cast<const uint8_t*>(device_dense_all);
    if (begins_step) begin_optimizer_step(m);
    /* one device driven through the exchange halves (bench.py --force-exchange): step_local's header launch has already added
     * this step to the plan's loss accumulators.  (The form stays: under the staleness-one pipeline it is the NEXT step's already.) */
    if (!p->left.form.header_accumulates) sbr::launch_accumulate_loss(dall, db, p->ndev, p->loss_acc, p->ex_acc, m->stream);
    {
        ScopedTimer t(m, SBR_K_DENSE_UPDATE, 1);
        sbr::launch_dense_apply(m->mv, dall, db, 32, p->ndev, m->stream);
    }
    return SBR_OK;
}

sbr_status sbr_fit_step_apply_table(sbr_fit_plan* p, const void* device_table, const void* device_dense_all) {
    if (!p || !device_table || !device_dense_all) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    if (m->shared) return SBR_ERR_INVALID_ARGUMENT; /* a partitioned table is updated by its owners (sbr_group_fit) */
    if (m->opt_state_partial) return SBR_ERR_INVALID_ARGUMENT; /* this replica holds its own rows' optimiser state only: gather it first */
    SBRCHK(ensure_device(m));
    SBRCHK(apply_dense_blocks(p, device_dense_all));
    {
        ScopedTimer t(m, SBR_K_SPARSE_UPDATE, 1);
        sbr::launch_table_apply(m->mv, contiguous_chunks(p, device_table), slice_rows(p), m->stream);
    }
    HIPCHK(hipGetLastError());
    return SBR_OK;
}

/* sbr_fit_step_apply_table in two halves, so that the item-table half does not have to wait for the dense-gradient
 * GEMM: rows first (it opens the optimiser step), dense second, once each per step. */
sbr_status sbr_fit_step_apply_rows(sbr_fit_plan* p, const void* device_table) {
    if (!p || !device_table) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    if (m->shared || m->opt_state_partial) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(m));
    begin_optimizer_step(m);
    {
        ScopedTimer t(m, SBR_K_SPARSE_UPDATE, 1);
        sbr::launch_table_apply(m->mv, contiguous_chunks(p, device_table), slice_rows(p), m->stream);
    }
    HIPCHK(hipGetLastError());
    return SBR_OK;
}

sbr_status sbr_fit_step_apply_dense(sbr_fit_plan* p, const void* device_dense_all) {
    if (!p || !device_dense_all) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    if (m->shared) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(m));
    SBRCHK(apply_dense_blocks(p, device_dense_all, /*begins_step=*/false));
    HIPCHK(hipGetLastError());
    return SBR_OK;
}

/* ---- owner-APPLIED update of the replicated exchange (Parallelism::Synchronous) ------------------------------------------
 * ≙ the one shared parameter + optimiser state of lstm.rs:259-260 / ewma.rs:267-269 under the synchronised step of
 * sequence_model.rs:163-169.  After the all-to-all the owner of a slice adds the devices' contributions in device order AND applies
 * the one optimiser update of every touched row of its slice, in place in its own replica; what the devices then all-gather is the
 * updated PARAMETER slices (E rows and biases), written straight into every replica's table (sbr_model_table_slice: the arrays are
 * allocated for num_devices equal slices).  Same sums in the same order, same update arithmetic, same bytes on the links as the
 * gradient all-gather of sbr_fit_step_owner_reduce + sbr_fit_step_apply_rows — same bits — but no replica walks the whole table
 * any more and the optimiser state of a row is maintained by its owner alone. */
sbr_status sbr_fit_step_owner_update(sbr_fit_plan* p, const void* device_recv) {
    if (!p || !device_recv) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    if (m->shared) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(m));
    begin_optimizer_step(m);
    const uint64_t S = slice_rows(p), I = m->hp.num_items;
    const uint64_t row0 = std::min<uint64_t>(I, (uint64_t)p->rank * S), nrows = std::min<uint64_t>(I, row0 + S) - row0;
    {
        ScopedTimer t(m, SBR_K_SPARSE_UPDATE, 1);
        sbr::launch_owner_update(m->mv, contiguous_chunks(p, device_recv), p->ndev, S, row0, nrows, m->stream);
    }
    if (p->ndev > 1) m->opt_state_partial = true;
    HIPCHK(hipGetLastError());
    return SBR_OK;
}

/* the owner update reading chunk `rank` of every peer's send buffer in place (peer transport) is sbr_fit_step_owner_reduce_peers'
 * sibling; not built: the peers' parameter slices would have to be exportable allocations as well */

sbr_status sbr_model_table_slice(sbr_model* m, int32_t which, void** out_base, uint64_t* out_slice_bytes) {
    if (!m || !out_base || !out_slice_bytes || m->shared) return SBR_ERR_INVALID_ARGUMENT;
    const uint64_t n = m->hp.num_devices, S = ((uint64_t)m->hp.num_items + n - 1) / n, d = (uint64_t)m->d;
    const sbr::ModelView& v = m->mv;
    float* base = nullptr;
    uint64_t row_bytes = 0;
    switch (which) {
        case SBR_PARAM_ITEM_EMBEDDING: base = v.E; row_bytes = d * 4; break;
        case SBR_PARAM_ITEM_EMBEDDING_ACC: base = v.Eacc; row_bytes = d * 4; break;
        case SBR_PARAM_ITEM_EMBEDDING_M: base = v.Em; row_bytes = d * 4; break;
        case SBR_PARAM_ITEM_BIAS: base = v.b; row_bytes = 4; break;
        case SBR_PARAM_ITEM_BIAS_ACC: base = v.bacc; row_bytes = 4; break;
        case SBR_PARAM_ITEM_BIAS_M: base = v.bm; row_bytes = 4; break;
        default: return SBR_ERR_INVALID_ARGUMENT;
    }
    *out_base = base; /* null: the block does not exist (Adam moments under Adagrad) */
    *out_slice_bytes = base ? S * row_bytes : 0;
    return SBR_OK;
}

sbr_status sbr_model_optimizer_state_gathered(sbr_model* m) {
    if (!m) return SBR_ERR_INVALID_ARGUMENT;
    m->opt_state_partial = false;
    return SBR_OK;
}

sbr_status sbr_model_optimizer_state_is_partial(const sbr_model* m, int32_t* out) {
    if (!m || !out) return SBR_ERR_INVALID_ARGUMENT;
    *out = m->opt_state_partial ? 1 : 0;
    return SBR_OK;
}

/* ---- partitioned item table (sbr_group_create flag SBR_GROUP_PARTITION_ITEM_TABLE) ------------------ */
static sbr_status partition_buffers(sbr_fit_plan* p) {
    if (p->glist) return SBR_OK;
    const uint64_t cap = 3 * p->rmax;
    if (cap >= (1ull << 28)) return SBR_ERR_UNSUPPORTED; /* list positions are 28-bit in the merge keys */
    if (p->exportable_lists) {
        const int dev = p->m->device;
        SBRCHK(p->own_x[1].alloc(cap * (uint64_t)p->m->d * 4, dev));
        SBRCHK(p->own_x[2].alloc(cap * 4, dev));
        SBRCHK(p->own_x[3].alloc(cap * 4, dev));
        p->glist = reinterpret_cast<float*>(p->own_x[1].ptr);
        p->gblist = reinterpret_cast<float*>(p->own_x[2].ptr);
        p->gfl = reinterpret_cast<uint32_t*>(p->own_x[3].ptr);
    } else {
        SBRCHK(dmalloc(&p->glist, cap * (uint64_t)p->m->d));
        SBRCHK(dmalloc(&p->gblist, cap));
        SBRCHK(dmalloc(&p->gfl, cap));
    }
    SBRCHK(dmalloc(&p->bounds_dev, 17));
    return SBR_OK;
}

/* The owner's merge buffers.  Since round 6 the number of merge keys of a step — the key positions of all devices inside this
 * owner's row range — is known on the device only (the host no longer reads the owner bounds back: that read drained every queue
 * every step), so the buffers hold the worst case, every entry of every device: ndev x 3 x rmax keys (2 x 8 B each + the radix
 * counters: 0.2 GB per owner at configs[4]'s 8 x 8 192 sequences of <= 63 steps).  Allocated at the first partitioned step. */
static sbr_status merge_capacity(sbr_fit_plan* p) {
    if (p->mcap) return SBR_OK;
    const uint64_t cap = (uint64_t)p->ndev * 3ull * p->rmax;
    if (cap >= (1ull << 32)) return SBR_ERR_UNSUPPORTED;
    SBRCHK(dmalloc(&p->mkeys, cap));
    SBRCHK(dmalloc(&p->mkeys_sorted, cap));
    p->msort_temp_bytes = sbr::sparse_sort_temp_bytes(cap, 64);
    uint8_t* tmp = nullptr;
    SBRCHK(dmalloc(&tmp, p->msort_temp_bytes));
    p->msort_temp = tmp;
    SBRCHK(dmalloc(&p->mplan, 1));
    p->mcap = cap;
    return SBR_OK;
}

/* this device's own entries reduced per row into its list + the owner bounds (after sbr_fit_step_local) */
static sbr_status partition_reduce_own(sbr_fit_plan* p, uint64_t minibatch) {
    sbr_model* m = p->m;
    SBRCHK(ensure_device(m));
    SBRCHK(partition_buffers(p));
    const sbr::BlockView bv = block_view(m, p->block, p->rmax);
    const uint32_t R = p->ep[p->cur].rows_of_dev[minibatch * p->ndev + p->rank];
    SBRCHK(join_main(p, KEYS));
    {
        ScopedTimer t(m, SBR_K_SPARSE_UPDATE, 1);
        sbr::launch_seg_list(m->mv, bv, R, p->ndev, slice_rows(p), p->keys_sorted, p->glist, p->gblist, p->gfl, p->bounds_dev, p->seg,
                             m->stream);
    }
    HIPCHK(hipGetLastError());
    return SBR_OK;
}

/* owner side: merge the peers' lists over this device's row range (device order) and update its rows; the range's position in the
 * peers' lists comes from their owner bounds ON THE DEVICE (pb: peer-readable arrays, or one gathered array) */
static sbr_status partition_owner_apply(sbr_fit_plan* p, const sbr::PeerLists& pl, const sbr::PeerBounds& pb) {
    sbr_model* m = p->m;
    SBRCHK(ensure_device(m));
    SBRCHK(merge_capacity(p));
    {
        ScopedTimer t(m, SBR_K_SPARSE_UPDATE, 1);
        sbr::launch_owner_list_apply(m->mv, pl, pb, p->ndev, p->rank, p->mplan, (uint32_t)p->mcap, p->mkeys, p->mkeys_sorted, p->msort_temp,
                                     p->msort_temp_bytes, m->stream);
    }
    HIPCHK(hipGetLastError());
    return SBR_OK;
}

sbr_status sbr_fit_end(sbr_fit_plan* p, float* out_loss, uint64_t* out_examples) {
    if (!p) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    SBRCHK(ensure_device(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipStreamSynchronize(m->sorter)); /* a step's header launch may ride on the ordering's stream */
    double loss[17];
    unsigned long long ex[18];
    HIPCHK(hipMemcpy(loss, p->loss_acc, sizeof(loss), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ex, p->ex_acc, sizeof(ex), hipMemcpyDeviceToHost));
    /* ≙ the sum over the partitions' workers of loss_value / (1.0 + examples) (sequence_model.rs:173-177); the
     * true loss sums, not the stale node values the reference reads */
    double total = 0.0;
    for (int q = 0; q < p->ndev; ++q) total += loss[1 + q] / (1.0 + (double)ex[2 + q]);
    if (out_loss) *out_loss = (float)total;
    if (out_examples) *out_examples = (uint64_t)ex[0];
    return SBR_OK;
}

/* ≙ the value `fit` returns in the reference: sum over the workers of (stale loss-node values) / (1 + examples)
 * (sequence_model.rs:157 before :160, :173-177).  This device's term; single device: the whole figure. */
sbr_status sbr_fit_end_lagged(sbr_fit_plan* p, float* out_term) {
    if (!p || !out_term) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    SBRCHK(ensure_device(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipStreamSynchronize(m->sorter));
    float lagged = 0.0f;
    unsigned long long ex[18];
    HIPCHK(hipMemcpy(&lagged, p->lag_state, sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ex, p->ex_acc, sizeof(ex), hipMemcpyDeviceToHost));
    *out_term = lagged / (1.0f + (float)ex[2 + p->rank]);
    return SBR_OK;
}

sbr_status sbr_model_last_fit_lagged_loss(const sbr_model* m, float* out_loss) {
    if (!m || !out_loss) return SBR_ERR_INVALID_ARGUMENT;
    *out_loss = m->last_lagged_loss;
    return SBR_OK;
}

sbr_status sbr_fit_counters(sbr_fit_plan* p, uint64_t* out_examples, uint64_t* out_negatives_scored) {
    if (!p) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(p->m));
    HIPCHK(hipStreamSynchronize(p->m->stream));
    HIPCHK(hipStreamSynchronize(p->m->sorter));
    unsigned long long v[2] = {0, 0};
    HIPCHK(hipMemcpy(v, p->ex_acc, sizeof(v), hipMemcpyDeviceToHost));
    if (out_examples) *out_examples = v[0];
    if (out_negatives_scored) *out_negatives_scored = v[1];
    return SBR_OK;
}

sbr_status sbr_fit_sparse_stats(sbr_fit_plan* p, uint64_t* out_entries, uint64_t* out_unique_rows) {
    if (!p) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(p->m));
    HIPCHK(hipStreamSynchronize(p->m->side));
    HIPCHK(hipStreamSynchronize(p->m->sorter));
    HIPCHK(hipStreamSynchronize(p->m->stream));
    uint32_t nheads = 0;
    HIPCHK(hipMemcpy(&nheads, p->seg.nheads, sizeof(nheads), hipMemcpyDeviceToHost));
    if (out_entries) *out_entries = 3ull * (uint64_t)p->last_R;
    if (out_unique_rows) *out_unique_rows = nheads;
    return SBR_OK;
}

sbr_status sbr_model_fit(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users,
                         float* out_loss) {
    if (!m) return SBR_ERR_INVALID_ARGUMENT;
    if (m->hp.num_devices != 1) return SBR_ERR_INVALID_ARGUMENT; /* multi-device fits are driven by the host (distributed.py) */
    sbr_fit_plan* p = nullptr;
    SBRCHK(sbr_fit_begin(m, user_ptr, item_ids, num_users, &p));
    sbr_status st = SBR_OK;
    for (uint32_t e = 0; e < m->hp.num_epochs && st == SBR_OK; ++e) {
        uint64_t nmb = 0;
        st = sbr_fit_epoch_prepare(p, &nmb);
        if (st == SBR_OK && e + 1 < m->hp.num_epochs) st = sbr_fit_epoch_prefetch(p); /* host packs epoch e+1 while the GPU runs e */
        if (st == SBR_OK) st = sbr_fit_steps(p, 0, nmb);
    }
    if (st == SBR_OK) st = sbr_fit_end(p, out_loss, nullptr);
    if (st == SBR_OK) st = sbr_fit_end_lagged(p, &m->last_lagged_loss);
    sbr_fit_plan_destroy(p);
    return st;
}

/* ---- the rendezvous of a step through RCCL INSIDE the library (one process per GPU; xGMI within a node) --------------------
 * ≙ the synchronised optimiser step of sequence_model.rs:92, 163-166 across processes.  A C / Rust host that runs one process per
 * GPU needs no collective library of its own: rank 0 makes an id (sbr_comm_unique_id), the host hands its 128 bytes to the other
 * ranks through whatever channel it has (a file, a socket, MPI), every rank calls sbr_comm_create on its device, and a step is
 * sbr_fit_step_local + sbr_fit_step_exchange.  librccl is opened at run time (dlopen): the engine has no link-time dependency on
 * it and hosts that bring their own transport (torch.distributed, MPI) never load it. */
namespace {
struct RcclId128 { char b[128]; }; /* ncclUniqueId: 128 opaque bytes, passed BY VALUE to ncclCommInitRank */
struct RcclApi {
    typedef RcclId128 Id128;
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, RcclId128, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    bool ok = false;
};
RcclApi* rccl_api() {
    static RcclApi* api = [] {
        RcclApi* a = new RcclApi;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            a->lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (a->lib) break;
        }
        if (!a->lib) return a;
        auto sym = [&](const char* n) { return dlsym(a->lib, n); };
        a->GetUniqueId = reinterpret_cast<decltype(a->GetUniqueId)>(sym("ncclGetUniqueId"));
        a->CommInitRank = reinterpret_cast<decltype(a->CommInitRank)>(sym("ncclCommInitRank"));
        a->CommDestroy = reinterpret_cast<decltype(a->CommDestroy)>(sym("ncclCommDestroy"));
        a->GroupStart = reinterpret_cast<decltype(a->GroupStart)>(sym("ncclGroupStart"));
        a->GroupEnd = reinterpret_cast<decltype(a->GroupEnd)>(sym("ncclGroupEnd"));
        a->Send = reinterpret_cast<decltype(a->Send)>(sym("ncclSend"));
        a->Recv = reinterpret_cast<decltype(a->Recv)>(sym("ncclRecv"));
        a->AllGather = reinterpret_cast<decltype(a->AllGather)>(sym("ncclAllGather"));
        a->ok = a->GetUniqueId && a->CommInitRank && a->CommDestroy && a->GroupStart && a->GroupEnd && a->Send && a->Recv && a->AllGather;
        return a;
    }();
    return api;
}
constexpr int kNcclUint8 = 1; /* ncclUint8 (rccl.h: ncclInt8 = 0, ncclUint8 = 1) */
}  // namespace

struct sbr_comm {
    void* comm = nullptr;
    uint32_t world = 0, rank = 0;
    int device = 0;
    uint8_t *send = nullptr, *recv = nullptr, *dense = nullptr, *dense_all = nullptr;
    uint64_t chunk = 0, db = 0; /* sizes the buffers were made for */
};

sbr_status sbr_comm_unique_id(uint8_t out_id[128]) {
    if (!out_id) return SBR_ERR_INVALID_ARGUMENT;
    RcclApi& a = *rccl_api();
    if (!a.ok) return SBR_ERR_UNSUPPORTED; /* no librccl on this host */
    return a.GetUniqueId(out_id) == 0 ? SBR_OK : SBR_ERR_HIP;
}

sbr_status sbr_comm_create(const uint8_t id[128], uint32_t world, uint32_t rank, sbr_comm** out) {
    if (!id || !out || world == 0 || world > 16 || rank >= world) return SBR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    RcclApi& a = *rccl_api();
    if (!a.ok) return SBR_ERR_UNSUPPORTED;
    sbr_comm* c = new (std::nothrow) sbr_comm;
    if (!c) return SBR_ERR_OUT_OF_MEMORY;
    c->world = world; c->rank = rank;
    (void)hipGetDevice(&c->device);
    RcclApi::Id128 uid;
    std::memcpy(uid.b, id, 128);
    if (a.CommInitRank(&c->comm, (int)world, uid, (int)rank) != 0) { delete c; return SBR_ERR_HIP; }
    *out = c;
    return SBR_OK;
}

void sbr_comm_destroy(sbr_comm* c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    if (c->comm) rccl_api()->CommDestroy(c->comm);
    dfree(c->send); dfree(c->recv); dfree(c->dense); dfree(c->dense_all);
    delete c;
}

/* the exchange and the update of one optimiser step (after sbr_fit_step_local): scatter -> all-to-all -> owner update (device-order
 * sum + the one optimiser update of the owner's rows, in place) -> all-gather of the updated parameter slices straight into this
 * replica's table; the dense block joins the dense-gradient GEMM late -> all-gather -> dense update.  Everything is queued on the
 * model's stream; the call does not block the host. */
static sbr_status comm_buffers(sbr_fit_plan* p, sbr_comm* c, uint64_t chunk, uint64_t db) {
    if (c->chunk == chunk && c->db == db && c->send) return SBR_OK;
    sbr_model* m = p->m;
    const uint32_t n = c->world;
    HIPCHK(hipStreamSynchronize(m->stream));
    dfree(c->send); dfree(c->recv); dfree(c->dense); dfree(c->dense_all);
    c->send = c->recv = c->dense = c->dense_all = nullptr;
    c->chunk = c->db = 0;
    /* all or nothing, BEFORE any collective of the step is queued: a rank that failed half-way through would leave its peers
     * waiting inside theirs */
    sbr_status st = dmalloc(&c->send, n * chunk);
    if (st == SBR_OK) st = dmalloc(&c->recv, n * chunk);
    if (st == SBR_OK) st = dmalloc(&c->dense, db);
    if (st == SBR_OK) st = dmalloc(&c->dense_all, n * db);
    if (st != SBR_OK) {
        dfree(c->send); dfree(c->recv); dfree(c->dense); dfree(c->dense_all);
        c->send = c->recv = c->dense = c->dense_all = nullptr;
        return st;
    }
    c->chunk = chunk; c->db = db;
    return SBR_OK;
}

/* in-place all-gather of one item-table block's owner slices (slice r of every replica <- rank r) */
static sbr_status comm_gather_block(sbr_model* m, sbr_comm* c, int32_t which) {
    RcclApi& a = *rccl_api();
    void* base = nullptr;
    uint64_t sb = 0;
    SBRCHK(sbr_model_table_slice(m, which, &base, &sb));
    if (!base) return SBR_OK;
    if (a.AllGather(reinterpret_cast<uint8_t*>(base) + (size_t)c->rank * sb, base, sb, kNcclUint8, c->comm, m->stream) != 0) return SBR_ERR_HIP;
    return SBR_OK;
}

sbr_status sbr_fit_step_exchange(sbr_fit_plan* p, uint64_t minibatch, sbr_comm* c) {
    if (!p || !c || (int)c->world != p->ndev || (int)c->rank != p->rank || minibatch >= p->ep[p->cur].num_mb || p->m->shared)
        return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    if (c->device != m->device) return SBR_ERR_INVALID_ARGUMENT; /* the communicator belongs to the device that was current at sbr_comm_create */
    SBRCHK(ensure_device(m));
    RcclApi& a = *rccl_api();
    uint64_t chunk = 0, db = 0;
    SBRCHK(sbr_fit_chunk_bytes(p, &chunk));
    SBRCHK(sbr_fit_dense_bytes(p, &db));
    const uint32_t n = c->world;
    SBRCHK(comm_buffers(p, c, chunk, db));
    hipStream_t st = m->stream;
    SBRCHK(sbr_fit_step_scatter(p, minibatch, c->send));
    if (a.GroupStart() != 0) return SBR_ERR_HIP; /* all-to-all: chunk q of this rank -> rank q */
    int bad = 0; /* the group is closed whatever happens inside it: an open group would swallow every later collective of this thread */
    for (uint32_t q = 0; q < n; ++q) {
        bad |= a.Send(c->send + (size_t)q * chunk, chunk, kNcclUint8, (int)q, c->comm, st);
        bad |= a.Recv(c->recv + (size_t)q * chunk, chunk, kNcclUint8, (int)q, c->comm, st);
    }
    bad |= a.GroupEnd();
    if (bad) return SBR_ERR_HIP;
    SBRCHK(sbr_fit_step_owner_update(p, c->recv));
    SBRCHK(comm_gather_block(m, c, SBR_PARAM_ITEM_EMBEDDING));
    SBRCHK(comm_gather_block(m, c, SBR_PARAM_ITEM_BIAS));
    SBRCHK(sbr_fit_step_dense(p, c->dense));
    if (a.AllGather(c->dense, c->dense_all, db, kNcclUint8, c->comm, st) != 0) return SBR_ERR_HIP;
    SBRCHK(sbr_fit_step_apply_dense(p, c->dense_all));
    return SBR_OK;
}

/* every replica's copy of the item table's optimiser state made complete again from the owners' slices (a fit through
 * sbr_fit_step_exchange leaves a row's state on its owner only) */
sbr_status sbr_comm_gather_optimizer_state(sbr_model* m, sbr_comm* c) {
    if (!m || !c || m->hp.num_devices != c->world || m->hp.device_rank != c->rank || c->device != m->device) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(m));
    for (int32_t which : {SBR_PARAM_ITEM_EMBEDDING_ACC, SBR_PARAM_ITEM_BIAS_ACC, SBR_PARAM_ITEM_EMBEDDING_M, SBR_PARAM_ITEM_BIAS_M})
        SBRCHK(comm_gather_block(m, c, which));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->opt_state_partial = false;
    return SBR_OK;
}

/* the whole fit of THIS rank through the library's own transport: ≙ fit with num_threads(world) across processes */
sbr_status sbr_model_fit_comm(sbr_model* m, sbr_comm* c, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, float* out_loss) {
    if (!m || !c || m->hp.num_devices != c->world || m->hp.device_rank != c->rank) return SBR_ERR_INVALID_ARGUMENT;
    if (m->reference_order && c->world > 1) return SBR_ERR_UNSUPPORTED; /* several workers in reference order: sbr_group_fit only */
    sbr_fit_plan* p = nullptr;
    SBRCHK(sbr_fit_begin(m, user_ptr, item_ids, num_users, &p));
    sbr_status st = SBR_OK;
    for (uint32_t e = 0; e < m->hp.num_epochs && st == SBR_OK; ++e) {
        uint64_t nmb = 0;
        st = sbr_fit_epoch_prepare(p, &nmb);
        if (st == SBR_OK && e + 1 < m->hp.num_epochs) st = sbr_fit_epoch_prefetch(p);
        for (uint64_t mb = 0; mb < nmb && st == SBR_OK; ++mb) {
            st = sbr_fit_step_local(p, mb);
            if (st == SBR_OK) st = sbr_fit_step_exchange(p, mb, c);
        }
    }
    if (st == SBR_OK) st = sbr_comm_gather_optimizer_state(m, c);
    if (st == SBR_OK) st = sbr_fit_end(p, out_loss, nullptr);
    if (st == SBR_OK) st = sbr_fit_end_lagged(p, &m->last_lagged_loss); /* this rank's term; hosts add the ranks' terms in rank order */
    sbr_fit_plan_destroy(p);
    return st;
}

/* ---- peer transport of the replicated owner-reduce exchange (one process per GPU) ----------------------
 * Instead of moving the chunks with collectives, every rank exports its send buffer and its reduced own
 * chunk once (file descriptors, like the partitioned table); the owner-reduce kernel then reads chunk q of
 * every peer's send buffer IN PLACE and the table update reads every owner's reduced chunk in place — the
 * bytes cross xGMI exactly once, inside the kernels that consume them, and no bulk collective is involved.
 * The host supplies the ordering: [scatter] barrier [owner reduce] barrier + all-gather of the small dense
 * blocks [apply]; the next step's scatter is safe because every rank passed the following barrier. */
sbr_status sbr_fit_exchange_export(sbr_fit_plan* p, int32_t out_fds[2], uint64_t out_bytes[2]) {
    if (!p || !out_fds || !out_bytes || p->ndev < 1 || p->m->shared) return SBR_ERR_INVALID_ARGUMENT;
    /* the peer transport runs the synchronous step whatever hp.parallelism says (the staleness-one pipeline belongs to the
     * collective transport): Asynchronous here IS Synchronous — deterministic, and a valid outcome of Hogwild */
    SBRCHK(ensure_device(p->m));
    const uint64_t chunk = slice_rows(p) * ((uint64_t)p->m->d + 2) * 4;
    if (!p->xchg_own[0].ptr) {
        SBRCHK(p->xchg_own[0].alloc((size_t)p->ndev * chunk, p->m->device));
        SBRCHK(p->xchg_own[1].alloc((size_t)chunk, p->m->device));
    }
    for (int i = 0; i < 2; ++i) {
        int fd = -1;
        SBRCHK(p->xchg_own[i].export_fd(&fd));
        out_fds[i] = fd;
        out_bytes[i] = p->xchg_own[i].bytes;
    }
    return SBR_OK;
}

sbr_status sbr_fit_exchange_import(sbr_fit_plan* p, uint32_t peer_rank, const int32_t fds[2], const uint64_t bytes[2]) {
    if (!p || !fds || !bytes || (int)peer_rank >= p->ndev || (int)peer_rank == p->rank) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(p->m));
    if (p->xchg_peer.empty()) p->xchg_peer.resize(p->ndev);
    for (int i = 0; i < 2; ++i) SBRCHK(p->xchg_peer[peer_rank][i].import_fd(fds[i], bytes[i], p->m->device));
    return SBR_OK;
}

static sbr_status peer_chunks(const sbr_fit_plan* p, int which, sbr::ChunkPtrs* out) {
    const uint64_t chunk = slice_rows(p) * ((uint64_t)p->m->d + 2) * 4;
    for (int r = 0; r < 16; ++r) out->p[r] = nullptr;
    for (int r = 0; r < p->ndev; ++r) {
        const VmmBuf* b = r == p->rank ? &p->xchg_own[which] : (p->xchg_peer.empty() ? nullptr : &p->xchg_peer[r][which]);
        if (!b || !b->ptr) return SBR_ERR_INVALID_ARGUMENT; /* exchange buffers of rank r not mapped */
        /* which 0: chunk `rank` of r's send buffer (what r contributes to my rows); which 1: r's reduced own chunk */
        out->p[r] = reinterpret_cast<const uint8_t*>(b->ptr) + (which == 0 ? (size_t)p->rank * chunk : 0);
    }
    return SBR_OK;
}

sbr_status sbr_fit_step_scatter_shared(sbr_fit_plan* p, uint64_t minibatch) {
    if (!p || !p->xchg_own[0].ptr) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(sbr_fit_step_scatter(p, minibatch, p->xchg_own[0].ptr));
    HIPCHK(hipStreamSynchronize(p->m->stream));
    return SBR_OK;
}

sbr_status sbr_fit_step_owner_reduce_peers(sbr_fit_plan* p) {
    if (!p || !p->xchg_own[1].ptr) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    SBRCHK(ensure_device(m));
    sbr::ChunkPtrs src;
    SBRCHK(peer_chunks(p, 0, &src));
    {
        ScopedTimer t(m, SBR_K_SPARSE_UPDATE, 1);
        sbr::launch_owner_reduce(m->mv, src, p->ndev, slice_rows(p), p->xchg_own[1].ptr, m->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(m->stream));
    return SBR_OK;
}

sbr_status sbr_fit_step_apply_table_peers(sbr_fit_plan* p, const void* device_dense_all) {
    if (!p || !device_dense_all || !p->xchg_own[1].ptr) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    SBRCHK(ensure_device(m));
    sbr::ChunkPtrs src;
    SBRCHK(peer_chunks(p, 1, &src));
    SBRCHK(apply_dense_blocks(p, device_dense_all));
    {
        ScopedTimer t(m, SBR_K_SPARSE_UPDATE, 1);
        sbr::launch_table_apply(m->mv, src, slice_rows(p), m->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(m->stream));
    return SBR_OK;
}

/* ---- one process per GPU over a partitioned table: the step halves the host sequences -----------------
 *   sbr_fit_step_local; sbr_fit_step_reduce_own (list + dense block; returns the owner bounds on the host,
 *   stream drained: this process has finished READING the table)  -> host: all-gather of the bounds and of
 *   the dense blocks (a rendezvous: every process has finished reading)  -> sbr_fit_step_owner_apply (merge
 *   of the peers' lists over this rank's rows, in-place update, stream drained)  -> host: barrier. */
sbr_status sbr_fit_lists_export(sbr_fit_plan* p, int32_t out_fds[4], uint64_t out_bytes[4]) {
    if (!p || !out_fds || !out_bytes || !p->exportable_lists) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(p->m));
    SBRCHK(partition_buffers(p));
    for (int i = 0; i < 4; ++i) {
        int fd = -1;
        SBRCHK(p->own_x[i].export_fd(&fd));
        out_fds[i] = fd;
        out_bytes[i] = p->own_x[i].bytes;
    }
    return SBR_OK;
}

sbr_status sbr_fit_lists_import(sbr_fit_plan* p, uint32_t peer_rank, const int32_t fds[4], const uint64_t bytes[4]) {
    if (!p || !fds || !bytes || !p->exportable_lists || (int)peer_rank >= p->ndev || (int)peer_rank == p->rank)
        return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(p->m));
    if (p->peer_x.empty()) p->peer_x.resize(p->ndev);
    for (int i = 0; i < 4; ++i) SBRCHK(p->peer_x[peer_rank][i].import_fd(fds[i], bytes[i], p->m->device));
    return SBR_OK;
}

sbr_status sbr_fit_step_reduce_own(sbr_fit_plan* p, uint64_t minibatch, uint32_t* host_bounds, void* device_dense_out) {
    if (!p || !host_bounds || !device_dense_out || !p->m->shared || minibatch >= p->ep[p->cur].num_mb) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(partition_reduce_own(p, minibatch));
    SBRCHK(sbr_fit_step_dense(p, device_dense_out));
    HIPCHK(hipStreamSynchronize(p->m->stream));
    HIPCHK(hipMemcpy(host_bounds, p->bounds_dev, (p->ndev + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SBR_OK;
}

/* the same half WITHOUT the host in the loop: nothing is drained, the owner bounds stay on the device (*out_device_bounds:
 * num_devices + 1 u32 of this rank, for the host's DEVICE all-gather) */
sbr_status sbr_fit_step_reduce_own_queued(sbr_fit_plan* p, uint64_t minibatch, void** out_device_bounds, void* device_dense_out) {
    if (!p || !out_device_bounds || !device_dense_out || !p->m->shared || minibatch >= p->ep[p->cur].num_mb) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(partition_reduce_own(p, minibatch));
    SBRCHK(sbr_fit_step_dense(p, device_dense_out));
    *out_device_bounds = p->bounds_dev;
    return SBR_OK;
}

static sbr_status owner_apply_lists(sbr_fit_plan* p, sbr::PeerLists* pl) {
    const int n = p->ndev, q = p->rank;
    std::memset(pl, 0, sizeof(*pl));
    for (int r = 0; r < n; ++r) {
        if (r == q) {
            pl->keys[r] = p->keys_sorted; pl->G[r] = p->glist; pl->gb[r] = p->gblist; pl->fl[r] = p->gfl;
        } else {
            if (p->peer_x.empty() || !p->peer_x[r][0].ptr) return SBR_ERR_INVALID_ARGUMENT; /* lists of rank r not imported */
            pl->keys[r] = reinterpret_cast<const uint64_t*>(p->peer_x[r][0].ptr);
            pl->G[r] = reinterpret_cast<const float*>(p->peer_x[r][1].ptr);
            pl->gb[r] = reinterpret_cast<const float*>(p->peer_x[r][2].ptr);
            pl->fl[r] = reinterpret_cast<const uint32_t*>(p->peer_x[r][3].ptr);
        }
    }
    return SBR_OK;
}

/* device_all_bounds: the ranks' owner bounds gathered ON THE DEVICE, rank r's num_devices + 1 words at r * (num_devices + 1);
 * queued, nothing drained */
sbr_status sbr_fit_step_owner_apply_queued(sbr_fit_plan* p, const void* device_all_bounds, const void* device_dense_all) {
    if (!p || !device_all_bounds || !device_dense_all || !p->exportable_lists) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    SBRCHK(ensure_device(m));
    sbr::PeerLists pl;
    SBRCHK(owner_apply_lists(p, &pl));
    sbr::PeerBounds pb;
    for (int r = 0; r < 16; ++r)
        pb.b[r] = r < p->ndev ? reinterpret_cast<const uint32_t*>(device_all_bounds) + (size_t)r * (p->ndev + 1) : nullptr;
    SBRCHK(apply_dense_blocks(p, device_dense_all));
    return partition_owner_apply(p, pl, pb);
}

sbr_status sbr_fit_step_owner_apply(sbr_fit_plan* p, const uint32_t* all_bounds, const void* device_dense_all) {
    if (!p || !all_bounds || !device_dense_all || !p->exportable_lists) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    SBRCHK(ensure_device(m));
    const size_t words = (size_t)p->ndev * (p->ndev + 1);
    if (!p->all_bounds_dev) SBRCHK(dmalloc(&p->all_bounds_dev, 17 * 16));
    HIPCHK(hipMemcpyAsync(p->all_bounds_dev, all_bounds, words * sizeof(uint32_t), hipMemcpyHostToDevice, m->stream));
    SBRCHK(sbr_fit_step_owner_apply_queued(p, p->all_bounds_dev, device_dense_all));
    HIPCHK(hipStreamSynchronize(m->stream));
    return SBR_OK;
}

/* ---- single-process multi-device fit (≙ fit with num_threads(n) on one host, sequence_model.rs:90-102, 163-169) --------
 * n replicas, each on its own HIP device and stream; the owner-reduce exchange of sbr_fit_step_scatter / _owner_reduce /
 * _apply_table is carried by peer copies (xGMI when the devices are peers) ordered with events:
 *   scattered[r]  send_r of this step is complete
 *   reduced[p]    own_p and dense_p of this step are complete
 *   applied[q]    q has finished reading its peers' buffers and has applied the step
 * A step is a short list of PHASES; inside a phase device r's work depends on nothing another device queues in the same phase,
 * so the phases either run as loops of one host thread or — sbr_group_plan_set_host_threads — on one host thread per device
 * (the reference runs one rayon worker per partition, sequence_model.rs:100-102): a device's ~20 launches per step are then
 * queued beside the other devices' instead of behind them.  An event is recorded in the phase BEFORE the one that waits for
 * it, and phases are separated by a host barrier, so hipStreamWaitEvent never sees an event that has not been recorded yet. */
namespace {

inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    __asm__ __volatile__("yield");
#else
    std::this_thread::yield();
#endif
}

/* n - 1 helper threads (the caller is worker 0).  run(f) = f(r) on every worker, then a barrier.  The helpers spin for the next
 * phase for a short while (a step's phases follow each other within microseconds) and then sleep on a condition variable. */
struct PhaseWorkers {
    std::vector<std::thread> threads;
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<uint64_t> generation{0};
    std::atomic<uint32_t> pending{0};
    std::atomic<bool> quit{false};
    const std::function<sbr_status(uint32_t)>* job = nullptr;
    std::vector<sbr_status> status;

    explicit PhaseWorkers(uint32_t n) : status(n, SBR_OK) {
        for (uint32_t r = 1; r < n; ++r) threads.emplace_back([this, r] { loop(r); });
    }
    ~PhaseWorkers() {
        {
            std::lock_guard<std::mutex> g(mu);
            quit.store(true, std::memory_order_release);
            generation.fetch_add(1, std::memory_order_release);
        }
        cv.notify_all();
        for (auto& t : threads) t.join();
    }
    void loop(uint32_t r) {
        uint64_t seen = 0;
        for (;;) {
            int spins = 0;
            while (generation.load(std::memory_order_acquire) == seen) {
                if (++spins < 20000) { cpu_relax(); continue; }
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [&] { return generation.load(std::memory_order_acquire) != seen; });
            }
            seen = generation.load(std::memory_order_acquire);
            if (quit.load(std::memory_order_acquire)) return;
            status[r] = (*job)(r);
            pending.fetch_sub(1, std::memory_order_acq_rel);
        }
    }
    sbr_status run(const std::function<sbr_status(uint32_t)>& f) {
        const uint32_t n = (uint32_t)status.size();
        job = &f;
        pending.store(n - 1, std::memory_order_release);
        {
            std::lock_guard<std::mutex> g(mu); /* a helper between its last spin and its wait must not miss the new generation */
            generation.fetch_add(1, std::memory_order_release);
        }
        cv.notify_all();
        status[0] = f(0);
        while (pending.load(std::memory_order_acquire) != 0) cpu_relax();
        for (uint32_t r = 0; r < n; ++r)
            if (status[r] != SBR_OK) return status[r];
        return SBR_OK;
    }
};

}  // namespace

struct sbr_group_plan {
    struct Dev {
        sbr_fit_plan* plan = nullptr;
        uint8_t *send = nullptr, *dense = nullptr, *recv = nullptr, *own = nullptr, *table = nullptr, *dense_all = nullptr;
        hipEvent_t scattered = nullptr, reduced = nullptr, applied = nullptr, gathered = nullptr;
        hipStream_t xs = nullptr; /* exchange stream (Asynchronous) */
    };
    std::vector<sbr_model*> models;
    std::vector<Dev> dev;
    uint32_t n = 0;
    uint64_t chunk = 0, db = 0, block_bytes = 0;
    bool partitioned = false, async = false, reforder = false;
    bool owner_applied = true;       /* Synchronous, replicated: the owners apply the update and the parameter slices travel (sbr_group_plan_set_exchange) */
    bool first = true;               /* no step has been applied yet: nothing to wait for */
    uint64_t nmb = 0;                /* minibatches of the prepared epoch */
    uint32_t epochs_prepared = 0;
    int64_t local_done = -1;         /* minibatch whose local half sbr_group_step_local has queued (parity access), or -1 */
    int64_t async_local_done = -1;   /* Asynchronous: minibatch whose local half the pipeline has queued ahead */
    std::unique_ptr<PhaseWorkers> workers;
    double enqueue_ms = 0.0;         /* host time spent inside sbr_group_step (queueing; a partitioned step includes its rendezvous) */
    uint64_t steps = 0;

    sbr_status phase(const std::function<sbr_status(uint32_t)>& f) {
        if (workers) return workers->run(f);
        for (uint32_t r = 0; r < n; ++r) SBRCHK(f(r));
        return SBR_OK;
    }
    sbr_status wait_applied(uint32_t r, hipStream_t s) { /* peers must be done with the previous step's buffers / table rows */
        if (first) return SBR_OK;
        for (uint32_t q = 0; q < n; ++q)
            if (q != r) SBRCHK(stream_wait(models[r], s, dev[q].applied));
        return SBR_OK;
    }
    /* local half of minibatch mb on device r (a partitioned table must not still be written by the previous step's owners) */
    sbr_status local(uint32_t r, uint64_t mb) {
        SBRCHK(ensure_device(models[r]));
        /* (reference order: the peers copy this plan's block on their own streams) */
        if (partitioned || reforder) SBRCHK(wait_applied(r, models[r]->stream));
        return sbr_fit_step_local(dev[r].plan, mb);
    }
    /* reference order (sbr_model_set_reference_order on every replica): the devices' blocks are gathered and applied as n optimiser
     * steps in device order on every replica (sbr_fit_step_apply_blocks_in_order) */
    sbr_status reforder_step(uint64_t mb) {
        const bool have_local = local_done == (int64_t)mb;
        SBRCHK(phase([&](uint32_t r) -> sbr_status {
            SBRCHK(ensure_device(models[r]));
            SBRCHK(wait_applied(r, models[r]->stream)); /* the peers have copied the previous step's block out of this plan */
            if (!have_local) SBRCHK(sbr_fit_step_local(dev[r].plan, mb));
            SBRCHK(ensure_dense_reduced(dev[r].plan));
            HIPCHK(hipEventRecord(dev[r].scattered, models[r]->stream));
            return SBR_OK;
        }));
        SBRCHK(phase([&](uint32_t q) -> sbr_status {
            SBRCHK(ensure_device(models[q]));
            for (uint32_t r = 0; r < n; ++r) {
                if (r != q) SBRCHK(stream_wait(models[q], models[q]->stream, dev[r].scattered));
                HIPCHK(hipMemcpyAsync(dev[q].recv + (size_t)r * block_bytes, dev[r].plan->block, block_bytes, hipMemcpyDefault, models[q]->stream));
            }
            SBRCHK(sbr_fit_step_apply_blocks_in_order(dev[q].plan, mb, dev[q].recv));
            HIPCHK(hipEventRecord(dev[q].applied, models[q]->stream));
            return SBR_OK;
        }));
        first = false;
        return SBR_OK;
    }
    sbr_status single_step(uint64_t mb) {
        if (local_done == (int64_t)mb) return sbr_fit_step_apply(dev[0].plan, mb);
        return sbr_fit_step(dev[0].plan, mb);
    }
    /* Parallelism::Synchronous: compute, exchange, apply — every device sees every update before its next minibatch.
     * owner_applied (default): the owner of a slice adds the devices' contributions AND updates its rows in place; the updated
     * parameter slices are all-gathered straight into every replica's table (peer copies) — no replica walks the whole table, a row's
     * optimiser state lives on its owner (gathered to all replicas when the fit ends).  Otherwise (sbr_group_plan_set_exchange 1;
     * what the staleness-one pipeline runs as well): the gradient chunks are all-gathered and every replica applies every update. */
    sbr_status sync_step(uint64_t mb) {
        const bool have_local = local_done == (int64_t)mb;
        SBRCHK(phase([&](uint32_t r) -> sbr_status {
            if (!have_local) SBRCHK(local(r, mb));
            SBRCHK(ensure_device(models[r]));
            SBRCHK(wait_applied(r, models[r]->stream));
            SBRCHK(sbr_fit_step_scatter(dev[r].plan, mb, dev[r].send));
            HIPCHK(hipEventRecord(dev[r].scattered, models[r]->stream));
            return SBR_OK;
        }));
        SBRCHK(phase([&](uint32_t p) -> sbr_status { /* all-to-all: chunk p of every device -> device p */
            SBRCHK(ensure_device(models[p]));
            for (uint32_t r = 0; r < n; ++r) {
                if (r != p) SBRCHK(stream_wait(models[p], models[p]->stream, dev[r].scattered));
                HIPCHK(hipMemcpyAsync(dev[p].recv + r * chunk, dev[r].send + p * chunk, chunk, hipMemcpyDefault, models[p]->stream));
            }
            if (owner_applied) SBRCHK(sbr_fit_step_owner_update(dev[p].plan, dev[p].recv));
            else SBRCHK(sbr_fit_step_owner_reduce(dev[p].plan, dev[p].recv, dev[p].own));
            SBRCHK(sbr_fit_step_dense(dev[p].plan, dev[p].dense));
            HIPCHK(hipEventRecord(dev[p].reduced, models[p]->stream));
            return SBR_OK;
        }));
        SBRCHK(phase([&](uint32_t q) -> sbr_status { /* all-gather of the owners' slices / chunks and of the dense blocks */
            SBRCHK(ensure_device(models[q]));
            for (uint32_t p = 0; p < n; ++p) {
                if (p != q) SBRCHK(stream_wait(models[q], models[q]->stream, dev[p].reduced));
                if (owner_applied) {
                    if (p != q) {
                        SBRCHK(copy_slice(q, p, SBR_PARAM_ITEM_EMBEDDING));
                        SBRCHK(copy_slice(q, p, SBR_PARAM_ITEM_BIAS));
                    }
                } else {
                    HIPCHK(hipMemcpyAsync(dev[q].table + p * chunk, dev[p].own, chunk, hipMemcpyDefault, models[q]->stream));
                }
                HIPCHK(hipMemcpyAsync(dev[q].dense_all + p * db, dev[p].dense, db, hipMemcpyDefault, models[q]->stream));
            }
            if (owner_applied) SBRCHK(sbr_fit_step_apply_dense(dev[q].plan, dev[q].dense_all));
            else SBRCHK(sbr_fit_step_apply_table(dev[q].plan, dev[q].table, dev[q].dense_all));
            HIPCHK(hipEventRecord(dev[q].applied, models[q]->stream));
            return SBR_OK;
        }));
        first = false;
        return SBR_OK;
    }
    /* the owner's reduced chunk and the gathered chunks of the gradient all-gather (the pipeline; sbr_group_plan_set_exchange 1) */
    sbr_status gradient_gather_buffers(uint32_t r) {
        Dev& v = dev[r];
        if (v.own) return SBR_OK;
        SBRCHK(ensure_device(models[r]));
        SBRCHK(dmalloc(&v.own, chunk));
        SBRCHK(dmalloc(&v.table, n * chunk));
        return SBR_OK;
    }
    /* replica q's copy of owner p's slice of one item-table block <- replica p's (queued on q's stream) */
    sbr_status copy_slice(uint32_t q, uint32_t p, int32_t which) {
        void *src = nullptr, *dst = nullptr;
        uint64_t sb = 0, sb2 = 0;
        SBRCHK(sbr_model_table_slice(models[p], which, &src, &sb));
        SBRCHK(sbr_model_table_slice(models[q], which, &dst, &sb2));
        if (!src || !dst || sb != sb2) return src || dst ? SBR_ERR_INVALID_ARGUMENT : SBR_OK;
        HIPCHK(hipMemcpyAsync(reinterpret_cast<uint8_t*>(dst) + (size_t)p * sb, reinterpret_cast<const uint8_t*>(src) + (size_t)p * sb, sb,
                              hipMemcpyDefault, models[q]->stream));
        return SBR_OK;
    }
    /* owner-applied steps leave a row's optimiser state on its owner only: every replica's copy made complete again (fit end) */
    sbr_status gather_optimizer_state() {
        bool any = false;
        for (uint32_t r = 0; r < n; ++r) any = any || models[r]->opt_state_partial;
        if (!any || partitioned) return SBR_OK;
        drain(); /* every owner's last update has landed */
        for (uint32_t q = 0; q < n; ++q) {
            SBRCHK(ensure_device(models[q]));
            for (uint32_t p = 0; p < n; ++p) {
                if (p == q) continue;
                for (int32_t which : {SBR_PARAM_ITEM_EMBEDDING_ACC, SBR_PARAM_ITEM_BIAS_ACC, SBR_PARAM_ITEM_EMBEDDING_M, SBR_PARAM_ITEM_BIAS_M})
                    SBRCHK(copy_slice(q, p, which));
            }
        }
        drain();
        for (uint32_t r = 0; r < n; ++r) models[r]->opt_state_partial = false;
        return SBR_OK;
    }
    /* Partitioned item table: every row is stored once (on its owner) and read by everybody through the shared mapping.  A step:
     * all devices compute on the current table; each reduces its own entries into a list and binary-searches its owner bounds;
     * every owner then waits — on its stream, through the devices' events — until nobody is READING the table any more, builds
     * its merge plan from the peers' bounds on the device, merges the peers' lists over its rows in device order and updates them in
     * place.  Bitwise the replicated Synchronous exchange.  Nothing of a step waits for the host. */
    sbr_status partitioned_step(uint64_t mb) {
        const bool have_local = local_done == (int64_t)mb;
        SBRCHK(phase([&](uint32_t r) -> sbr_status {
            if (!have_local) SBRCHK(local(r, mb));
            SBRCHK(ensure_device(models[r]));
            SBRCHK(partition_reduce_own(dev[r].plan, mb));
            SBRCHK(sbr_fit_step_dense(dev[r].plan, dev[r].dense));
            /* `scattered`: device r has finished READING the table, its list, owner bounds and dense block are complete — what the
             * owners wait for, on their own streams; the host reads nothing back and drains nothing (until round 5: a stream
             * synchronise + a blocking copy of the bounds per device and step, 0.96 of the step's time on the host) */
            HIPCHK(hipEventRecord(dev[r].scattered, models[r]->stream));
            return SBR_OK;
        }));
        SBRCHK(phase([&](uint32_t q) -> sbr_status {
            SBRCHK(ensure_device(models[q]));
            sbr::PeerLists pl;
            sbr::PeerBounds pb;
            std::memset(&pl, 0, sizeof(pl));
            for (uint32_t r = 0; r < 16; ++r) pb.b[r] = nullptr;
            for (uint32_t r = 0; r < n; ++r) {
                const sbr_fit_plan* pr = dev[r].plan;
                pl.keys[r] = pr->keys_sorted; pl.G[r] = pr->glist; pl.gb[r] = pr->gblist; pl.fl[r] = pr->gfl;
                pb.b[r] = pr->bounds_dev; /* read in place by merge_plan_kernel (peer-readable like the lists) */
                if (r != q) SBRCHK(stream_wait(models[q], models[q]->stream, dev[r].scattered));
            }
            for (uint32_t r = 0; r < n; ++r)
                HIPCHK(hipMemcpyAsync(dev[q].dense_all + r * db, dev[r].dense, db, hipMemcpyDefault, models[q]->stream));
            SBRCHK(apply_dense_blocks(dev[q].plan, dev[q].dense_all));
            SBRCHK(partition_owner_apply(dev[q].plan, pl, pb));
            HIPCHK(hipEventRecord(dev[q].applied, models[q]->stream));
            models[q]->shared->owner_updated[q] = dev[q].applied; /* readers of the table on the other replicas' streams join it */
            return SBR_OK;
        }));
        first = false;
        return SBR_OK;
    }
    /* Parallelism::Asynchronous (mod.rs:36-38), the deterministic analogue of Hogwild: staleness is fixed at one step.  Device
     * r computes minibatch mb + 1 on its compute stream while the exchange of step mb (peer copies + owner reduce) runs on its
     * exchange stream; update mb is applied after that computation has read the parameters. */
    sbr_status async_step(uint64_t mb) {
        if (async_local_done < (int64_t)mb) {
            SBRCHK(phase([&](uint32_t r) -> sbr_status { return local(r, mb); }));
            async_local_done = (int64_t)mb;
        }
        const bool ahead = mb + 1 < nmb;
        SBRCHK(phase([&](uint32_t r) -> sbr_status {
            SBRCHK(ensure_device(models[r]));
            SBRCHK(wait_applied(r, models[r]->stream));
            SBRCHK(sbr_fit_step_scatter(dev[r].plan, mb, dev[r].send));
            SBRCHK(sbr_fit_step_dense(dev[r].plan, dev[r].dense));
            HIPCHK(hipEventRecord(dev[r].scattered, models[r]->stream));
            if (ahead) SBRCHK(sbr_fit_step_local(dev[r].plan, mb + 1));
            return SBR_OK;
        }));
        if (ahead) async_local_done = (int64_t)mb + 1;
        SBRCHK(phase([&](uint32_t p) -> sbr_status {
            SBRCHK(ensure_device(models[p]));
            for (uint32_t r = 0; r < n; ++r) {
                SBRCHK(stream_wait(models[p], dev[p].xs, dev[r].scattered));
                HIPCHK(hipMemcpyAsync(dev[p].recv + r * chunk, dev[r].send + p * chunk, chunk, hipMemcpyDefault, dev[p].xs));
            }
            SBRCHK(sbr_fit_step_owner_reduce_on(dev[p].plan, dev[p].recv, dev[p].own, dev[p].xs)); /* belongs to the exchange stream */
            HIPCHK(hipEventRecord(dev[p].reduced, dev[p].xs));
            return SBR_OK;
        }));
        SBRCHK(phase([&](uint32_t q) -> sbr_status {
            SBRCHK(ensure_device(models[q]));
            for (uint32_t p = 0; p < n; ++p) {
                if (p != q) SBRCHK(stream_wait(models[q], dev[q].xs, dev[p].reduced));
                HIPCHK(hipMemcpyAsync(dev[q].table + p * chunk, dev[p].own, chunk, hipMemcpyDefault, dev[q].xs));
                HIPCHK(hipMemcpyAsync(dev[q].dense_all + p * db, dev[p].dense, db, hipMemcpyDefault, dev[q].xs));
            }
            HIPCHK(hipEventRecord(dev[q].gathered, dev[q].xs));
            SBRCHK(stream_wait(models[q], models[q]->stream, dev[q].gathered));
            SBRCHK(sbr_fit_step_apply_table(dev[q].plan, dev[q].table, dev[q].dense_all));
            HIPCHK(hipEventRecord(dev[q].applied, models[q]->stream));
            return SBR_OK;
        }));
        first = false;
        return SBR_OK;
    }
    sbr_status begin(sbr_model* const* ms, uint32_t count, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users) {
        n = count;
        models.assign(ms, ms + count);
        dev.resize(n);
        partitioned = models[0]->shared != nullptr;
        if (partitioned) models[0]->shared->owner_updated.assign(n, nullptr);
        /* a partitioned table is updated in place by its owners after a rendezvous, so there is no staleness-one pipeline for
         * it: Parallelism::Asynchronous runs the synchronous step there (same everywhere a partitioned table is driven) */
        async = models[0]->hp.parallelism == SBR_PAR_ASYNCHRONOUS && !partitioned;
        reforder = models[0]->reference_order;
        for (uint32_t r = 0; r < n; ++r)
            if (models[r]->reference_order != reforder) return SBR_ERR_INVALID_ARGUMENT;
        for (uint32_t r = 0; r < n; ++r) SBRCHK(sbr_fit_begin(models[r], user_ptr, item_ids, num_users, &dev[r].plan));
        block_bytes = dev[0].plan->block_bytes;
        SBRCHK(sbr_fit_chunk_bytes(dev[0].plan, &chunk));
        SBRCHK(sbr_fit_dense_bytes(dev[0].plan, &db));
        for (uint32_t r = 0; r < n; ++r) {
            Dev& v = dev[r];
            SBRCHK(ensure_device(models[r]));
            for (uint32_t q = 0; q < n; ++q)
                if (models[q]->device != models[r]->device) {
                    int can = 0;
                    if (hipDeviceCanAccessPeer(&can, models[r]->device, models[q]->device) == hipSuccess && can)
                        (void)hipDeviceEnablePeerAccess(models[q]->device, 0); /* already-enabled is fine */
                }
            (void)hipGetLastError();
            if (n == 1) continue; /* single_step: no exchange buffers */
            if (reforder) { /* the devices' whole blocks travel (one sequence each: tens of KB) */
                SBRCHK(dmalloc(&v.recv, n * block_bytes));
                HIPCHK(hipEventCreateWithFlags(&v.scattered, hipEventDisableTiming));
                HIPCHK(hipEventCreateWithFlags(&v.applied, hipEventDisableTiming));
                continue;
            }
            SBRCHK(dmalloc(&v.dense, db)); SBRCHK(dmalloc(&v.dense_all, n * db));
            if (!partitioned) { /* the replicated exchange moves table-sized chunks; the partitioned one needs none */
                SBRCHK(dmalloc(&v.send, n * chunk)); SBRCHK(dmalloc(&v.recv, n * chunk));
                if (async) SBRCHK(gradient_gather_buffers(r)); /* (Synchronous: the parameter slices are gathered in place) */
            }
            HIPCHK(hipEventCreateWithFlags(&v.scattered, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&v.reduced, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&v.applied, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&v.gathered, hipEventDisableTiming));
            if (async) HIPCHK(hipStreamCreateWithFlags(&v.xs, hipStreamNonBlocking));
        }
        return SBR_OK;
    }
    sbr_status epoch_prepare(uint64_t* out_nmb, bool prefetch_next) {
        uint64_t k0 = 0;
        if (reforder && n > 1) { /* every replica shuffles EVERY worker's partition (it needs the workers' step sizes): each worker's
                                  * stream, advanced on its own device during the epoch, goes to all of them first */
            for (uint32_t r = 0; r < n; ++r) {
                sbr_fit_plan* pr = dev[r].plan;
                if (!pr->ref_rng || !pr->ref_rng_live) continue;
                SBRCHK(ensure_device(models[r]));
                HIPCHK(hipStreamSynchronize(models[r]->stream));
                uint32_t st4w[4];
                HIPCHK(hipMemcpy(st4w, pr->ref_rng, sizeof(st4w), hipMemcpyDeviceToHost));
                for (uint32_t q = 0; q < n; ++q) {
                    sbr_xorshift& x = dev[q].plan->part_rng[r];
                    x.x = st4w[0]; x.y = st4w[1]; x.z = st4w[2]; x.w = st4w[3];
                }
                pr->ref_rng_live = false;
            }
        }
        for (uint32_t r = 0; r < n; ++r) {
            uint64_t k = 0;
            SBRCHK(sbr_fit_epoch_prepare(dev[r].plan, &k));
            if (r && k != k0) return SBR_ERR_INVALID_ARGUMENT;
            k0 = k;
            if (prefetch_next) SBRCHK(sbr_fit_epoch_prefetch(dev[r].plan));
        }
        nmb = k0;
        local_done = async_local_done = -1;
        ++epochs_prepared;
        if (out_nmb) *out_nmb = k0;
        return SBR_OK;
    }
    sbr_status step(uint64_t mb) {
        if (mb >= nmb) return SBR_ERR_INVALID_ARGUMENT;
        const auto t0 = std::chrono::steady_clock::now();
        /* a group of one has nobody to exchange with: the single-device step (its table may still be a mapped range) */
        const sbr_status st = n == 1 ? single_step(mb) : reforder ? reforder_step(mb) : partitioned ? partitioned_step(mb) : async ? async_step(mb) : sync_step(mb);
        local_done = -1;
        enqueue_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        ++steps;
        return st;
    }
    /* every stream of the group drained (also on an error path: a peer copy still in flight must not find its buffers recycled) */
    void drain() {
        for (uint32_t r = 0; r < n; ++r) {
            hipSetDevice(models[r]->device);
            hipStreamSynchronize(models[r]->stream);
            if (models[r]->side) hipStreamSynchronize(models[r]->side);
            if (models[r]->sorter) hipStreamSynchronize(models[r]->sorter);
            if (dev[r].xs) hipStreamSynchronize(dev[r].xs);
        }
    }
    ~sbr_group_plan() {
        workers.reset();
        (void)gather_optimizer_state(); /* (an abandoned plan as well: the models outlive it) */
        drain();
        if (partitioned && n && models[0]->shared) models[0]->shared->owner_updated.clear(); /* the events below go; everything has landed */
        for (uint32_t r = 0; r < n; ++r) {
            Dev& v = dev[r];
            hipSetDevice(models[r]->device);
            dfree(v.send); dfree(v.dense); dfree(v.recv); dfree(v.own); dfree(v.table); dfree(v.dense_all);
            if (v.scattered) hipEventDestroy(v.scattered);
            if (v.reduced) hipEventDestroy(v.reduced);
            if (v.applied) hipEventDestroy(v.applied);
            if (v.gathered) hipEventDestroy(v.gathered);
            if (v.xs) hipStreamDestroy(v.xs);
            if (v.plan) sbr_fit_plan_destroy(v.plan);
        }
    }
};

sbr_status sbr_group_fit_begin(sbr_model* const* models, uint32_t n, const uint64_t* user_ptr, const uint32_t* item_ids,
                               uint64_t num_users, sbr_group_plan** out) {
    if (!models || !out || n == 0 || n > 16) return SBR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    for (uint32_t r = 0; r < n; ++r) {
        const sbr_model* m = models[r];
        if (!m || m->hp.num_devices != n || m->hp.device_rank != r || m->hp.num_epochs != models[0]->hp.num_epochs ||
            m->shared != models[0]->shared)
            return SBR_ERR_INVALID_ARGUMENT;
    }
    sbr_group_plan* g = new (std::nothrow) sbr_group_plan;
    if (!g) return SBR_ERR_OUT_OF_MEMORY;
    const sbr_status st = g->begin(models, n, user_ptr, item_ids, num_users);
    if (st != SBR_OK) { delete g; return st; }
    /* default: one host thread per device from four devices on (measured: profiles/r05_group_driver.jsonl) */
    if (n >= 4) g->workers.reset(new PhaseWorkers(n));
    *out = g;
    return SBR_OK;
}

sbr_status sbr_group_plan_set_host_threads(sbr_group_plan* g, int32_t enable) {
    if (!g) return SBR_ERR_INVALID_ARGUMENT;
    if (enable && !g->workers && g->n > 1) g->workers.reset(new PhaseWorkers(g->n));
    if (!enable) g->workers.reset();
    return SBR_OK;
}

sbr_status sbr_group_plan_set_exchange(sbr_group_plan* g, int32_t gradient_all_gather) {
    if (!g) return SBR_ERR_INVALID_ARGUMENT;
    for (uint32_t r = 0; r < g->n; ++r)
        if (g->models[r]->opt_state_partial && gradient_all_gather) return SBR_ERR_INVALID_ARGUMENT; /* owner-applied steps have run: finish the fit first */
    if (gradient_all_gather && g->n > 1 && !g->partitioned && !g->reforder)
        for (uint32_t r = 0; r < g->n; ++r) SBRCHK(g->gradient_gather_buffers(r));
    g->owner_applied = !gradient_all_gather;
    return SBR_OK;
}

sbr_status sbr_group_gather_optimizer_state(sbr_group_plan* g) {
    if (!g) return SBR_ERR_INVALID_ARGUMENT;
    return g->gather_optimizer_state();
}

sbr_status sbr_group_epoch_prepare(sbr_group_plan* g, uint64_t* out_num_minibatches, int32_t prefetch_next) {
    if (!g) return SBR_ERR_INVALID_ARGUMENT;
    return g->epoch_prepare(out_num_minibatches, prefetch_next != 0);
}

sbr_status sbr_group_step(sbr_group_plan* g, uint64_t minibatch) {
    if (!g) return SBR_ERR_INVALID_ARGUMENT;
    return g->step(minibatch);
}

sbr_status sbr_group_step_local(sbr_group_plan* g, uint64_t minibatch) {
    if (!g || minibatch >= g->nmb || g->async) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(g->phase([&](uint32_t r) -> sbr_status { return g->local(r, minibatch); }));
    g->local_done = (int64_t)minibatch;
    return SBR_OK;
}

sbr_status sbr_group_member_plan(sbr_group_plan* g, uint32_t replica, sbr_fit_plan** out) {
    if (!g || !out || replica >= g->n) return SBR_ERR_INVALID_ARGUMENT;
    *out = g->dev[replica].plan;
    return SBR_OK;
}

sbr_status sbr_group_synchronize(sbr_group_plan* g) {
    if (!g) return SBR_ERR_INVALID_ARGUMENT;
    g->drain();
    return hipGetLastError() == hipSuccess ? SBR_OK : SBR_ERR_HIP;
}

sbr_status sbr_group_plan_stats(const sbr_group_plan* g, double* out_host_enqueue_ms, uint64_t* out_steps, int32_t* out_host_threads) {
    if (!g) return SBR_ERR_INVALID_ARGUMENT;
    if (out_host_enqueue_ms) *out_host_enqueue_ms = g->enqueue_ms;
    if (out_steps) *out_steps = g->steps;
    if (out_host_threads) *out_host_threads = g->workers ? (int32_t)g->n : 1;
    return SBR_OK;
}

sbr_status sbr_group_fit_end(sbr_group_plan* g, float* out_loss) {
    if (!g) return SBR_ERR_INVALID_ARGUMENT;
    auto finish = [&]() -> sbr_status {
        const uint32_t n = g->n;
        SBRCHK(g->gather_optimizer_state());
        for (uint32_t r = 1; r < n; ++r) SBRCHK(sbr_fit_end(g->dev[r].plan, nullptr, nullptr));
        float lagged = 0.0f; /* the workers' terms added in worker order, f32 (sequence_model.rs:173-177) */
        for (uint32_t r = 0; r < n; ++r) {
            float term = 0.0f;
            SBRCHK(sbr_fit_end_lagged(g->dev[r].plan, &term));
            lagged = lagged + term;
        }
        for (uint32_t r = 0; r < n; ++r) g->models[r]->last_lagged_loss = lagged;
        return sbr_fit_end(g->dev[0].plan, out_loss, nullptr);
    };
    const sbr_status st = finish();
    delete g;
    return st;
}

void sbr_group_plan_destroy(sbr_group_plan* g) { delete g; }

sbr_status sbr_group_fit(sbr_model* const* models, uint32_t n, const uint64_t* user_ptr, const uint32_t* item_ids,
                         uint64_t num_users, float* out_loss) {
    if (!models || n == 0) return SBR_ERR_INVALID_ARGUMENT;
    if (n == 1) {
        if (!models[0] || models[0]->hp.num_devices != 1 || models[0]->hp.device_rank != 0) return SBR_ERR_INVALID_ARGUMENT;
        return sbr_model_fit(models[0], user_ptr, item_ids, num_users, out_loss);
    }
    sbr_group_plan* g = nullptr;
    SBRCHK(sbr_group_fit_begin(models, n, user_ptr, item_ids, num_users, &g));
    const uint32_t epochs = models[0]->hp.num_epochs;
    sbr_status st = SBR_OK;
    for (uint32_t e = 0; e < epochs && st == SBR_OK; ++e) {
        uint64_t nmb = 0;
        st = sbr_group_epoch_prepare(g, &nmb, e + 1 < epochs);
        for (uint64_t mb = 0; mb < nmb && st == SBR_OK; ++mb) st = sbr_group_step(g, mb);
    }
    if (st != SBR_OK) { sbr_group_plan_destroy(g); return st; }
    return sbr_group_fit_end(g, out_loss);
}


/* n replicas of one model (num_devices = n, device_rank = r, replica r on HIP device r mod device count).
 * SBR_GROUP_PARTITION_ITEM_TABLE: instead of n full copies, the item table (embeddings, biases and their
 * optimiser state) exists once, rows [r*S, (r+1)*S), S = ceil(num_items / n), on replica r's device, mapped
 * into every replica's address space. */
sbr_status sbr_group_create(const sbr_hparams* hp, uint32_t n, uint32_t flags, sbr_model** out_models) {
    if (!hp || !out_models || n == 0 || n > 16) return SBR_ERR_INVALID_ARGUMENT;
    if (!storage_dim(hp->embedding_dim) || hp->num_items == 0) return SBR_ERR_INVALID_ARGUMENT;
    int ndevices = 0;
    if (hipGetDeviceCount(&ndevices) != hipSuccess || ndevices == 0) return SBR_ERR_NO_DEVICE;
    for (uint32_t r = 0; r < n; ++r) out_models[r] = nullptr;
    std::vector<int> devices(n);
    for (uint32_t r = 0; r < n; ++r) devices[r] = (int)(r % (uint32_t)ndevices);
    std::shared_ptr<SharedTable> shared;
    sbr_status st = SBR_OK;
    if (flags & SBR_GROUP_PARTITION_ITEM_TABLE) {
        shared = std::make_shared<SharedTable>();
        const uint64_t S = ((uint64_t)hp->num_items + n - 1) / n;
        st = shared->create(hp->num_items, (uint32_t)storage_dim(hp->embedding_dim), hp->optimizer == SBR_OPT_ADAM, devices, S);
    }
    for (uint32_t r = 0; r < n && st == SBR_OK; ++r) {
        sbr_hparams h = *hp;
        h.num_devices = n;
        h.device_rank = r;
        if (hipSetDevice(devices[r]) != hipSuccess) { st = SBR_ERR_HIP; break; }
        st = model_create_impl(&h, shared, r == 0 ? TABLE_WRITE_ALL : TABLE_WRITE_NONE, r ? &out_models[0]->rng_after_table : nullptr,
                               &out_models[r]);
    }
    (void)hipSetDevice(devices[0]);
    if (st != SBR_OK)
        for (uint32_t r = 0; r < n; ++r) { sbr_model_destroy(out_models[r]); out_models[r] = nullptr; }
    return st;
}

sbr_status sbr_model_is_partitioned(const sbr_model* m, int32_t* out) {
    if (!m || !out) return SBR_ERR_INVALID_ARGUMENT;
    *out = m->shared ? 1 : 0;
    return SBR_OK;
}

/* ---- partitioned item table under ONE PROCESS PER GPU --------------------------------------------------
 * Every process calls sbr_model_create_partitioned with the same hyper-parameters (num_devices = world,
 * device_rank = its rank) on its own device: the layout of the shared virtual range is planned identically
 * everywhere, the parts homed on this rank are allocated and mapped.  The host then moves file descriptors:
 * sbr_partition_export_part for own parts -> the peers' sbr_partition_import_part (Unix-socket SCM_RIGHTS;
 * sbr_rs_amd/partitioned.py), and sbr_partition_finalize writes this rank's rows. */
sbr_status sbr_model_create_partitioned(const sbr_hparams* hp, sbr_model** out) {
    if (!hp || !out) return SBR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!storage_dim(hp->embedding_dim) || hp->num_items == 0 || hp->num_devices == 0 || hp->num_devices > 16 ||
        hp->device_rank >= hp->num_devices)
        return SBR_ERR_INVALID_ARGUMENT;
    /* a partitioned table is updated in place by its owners after a rendezvous: Parallelism::Asynchronous runs the
     * synchronous step (no staleness-one pipeline), here as in sbr_group_fit */
    int ndevices = 0, device = 0;
    if (hipGetDeviceCount(&ndevices) != hipSuccess || ndevices == 0) return SBR_ERR_NO_DEVICE;
    HIPCHK(hipGetDevice(&device));
    auto shared = std::make_shared<SharedTable>();
    shared->local_rank = (int)hp->device_rank;
    const uint64_t S = ((uint64_t)hp->num_items + hp->num_devices - 1) / hp->num_devices;
    SBRCHK(shared->plan(hp->num_items, (uint32_t)storage_dim(hp->embedding_dim), hp->optimizer == SBR_OPT_ADAM, (int)hp->num_devices, S, device));
    std::vector<int> device_of_rank(hp->num_devices, device); /* only this rank's entry is used */
    SBRCHK(shared->create_parts(device_of_rank));
    return model_create_impl(hp, shared, TABLE_OWN_ROWS_DEFERRED, nullptr, out);
}

sbr_status sbr_partition_num_parts(const sbr_model* m, uint32_t* out) {
    if (!m || !m->shared || !out) return SBR_ERR_INVALID_ARGUMENT;
    *out = (uint32_t)m->shared->parts.size();
    return SBR_OK;
}

sbr_status sbr_partition_part_info(const sbr_model* m, uint32_t part, uint32_t* out_home_rank, uint64_t* out_bytes) {
    if (!m || !m->shared || part >= m->shared->parts.size()) return SBR_ERR_INVALID_ARGUMENT;
    if (out_home_rank) *out_home_rank = (uint32_t)m->shared->parts[part].home;
    if (out_bytes) *out_bytes = m->shared->parts[part].bytes;
    return SBR_OK;
}

sbr_status sbr_partition_export_part(sbr_model* m, uint32_t part, int32_t* out_fd) {
    if (!m || !m->shared || !out_fd || part >= m->shared->parts.size()) return SBR_ERR_INVALID_ARGUMENT;
    SharedTable::Part& pt = m->shared->parts[part];
    if (!pt.have || pt.home != m->shared->local_rank) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(m));
    int fd = -1;
    HIPCHK(hipMemExportToShareableHandle(&fd, pt.h, hipMemHandleTypePosixFileDescriptor, 0));
    *out_fd = fd;
    return SBR_OK;
}

sbr_status sbr_partition_import_part(sbr_model* m, uint32_t part, int32_t fd) {
    if (!m || !m->shared || m->shared->local_rank < 0) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(m));
    return m->shared->import_part(part, fd);
}

sbr_status sbr_partition_finalize(sbr_model* m) {
    if (!m || !m->shared || m->shared->local_rank < 0) return SBR_ERR_INVALID_ARGUMENT;
    if (m->partition_finalized) return SBR_OK;
    SBRCHK(ensure_device(m));
    SBRCHK(m->shared->set_access(std::vector<int>{m->device}));
    const sbr::ModelView& v = m->mv;
    const uint64_t I = m->hp.num_items, d = (uint64_t)m->d, S = m->shared->slice;
    const uint64_t r0 = std::min<uint64_t>(I, (uint64_t)m->hp.device_rank * S), r1 = std::min<uint64_t>(I, r0 + S), nr = r1 - r0;
    if (nr) {
        HIPCHK(hipMemcpy(v.E + r0 * d, m->pending_E.data(), nr * d * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(v.Eacc + r0 * d, 0, nr * d * 4));
        HIPCHK(hipMemset(v.b + r0, 0, nr * 4));
        HIPCHK(hipMemset(v.bacc + r0, 0, nr * 4));
        if (m->hp.optimizer == SBR_OPT_ADAM) {
            HIPCHK(hipMemset(v.Em + r0 * d, 0, nr * d * 4));
            HIPCHK(hipMemset(v.bm + r0, 0, nr * 4));
        }
    }
    HIPCHK(hipDeviceSynchronize());
    std::vector<float>().swap(m->pending_E);
    m->partition_finalized = true;
    return SBR_OK;
}

sbr_status sbr_device_count(int32_t* out_count) {
    if (!out_count) return SBR_ERR_INVALID_ARGUMENT;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) return SBR_ERR_NO_DEVICE;
    *out_count = nd;
    return SBR_OK;
}

sbr_status sbr_fit_debug_fetch(sbr_fit_plan* p, int32_t which, void* host_out, uint64_t bytes) {
    if (!p || !host_out || !p->last_block) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = p->m;
    SBRCHK(ensure_device(m));
    if (which == SBR_DBG_DENSE_GRAD) SBRCHK(ensure_dense_reduced(p));
    else SBRCHK(join_main(p, DENSE));
    HIPCHK(hipStreamSynchronize(m->stream));
    const sbr::BlockView bv = block_view(m, const_cast<void*>(p->last_block), p->rmax);
    const uint64_t R = (uint64_t)p->last_R, d = (uint64_t)m->d;
    const void* src = nullptr;
    uint64_t n = 0;
    switch (which) {
        case SBR_DBG_HIDDEN: src = bv.H; n = R * d * 4; break;
        case SBR_DBG_NEGATIVES: src = bv.neg; n = R * 4; break;
        case SBR_DBG_COEF: src = bv.coef; n = R * 4; break;
        case SBR_DBG_LOSS: src = p->wb.v.loss; n = R * 4; break;
        case SBR_DBG_DHIDDEN:
            /* only defined before the optimiser step of the same minibatch has been applied */
            sbr::launch_materialize_dh(m->mv, bv, p->last_R, p->wb.v.dH, m->stream);
            HIPCHK(hipStreamSynchronize(m->stream));
            src = p->wb.v.dH; n = R * d * 4; break;
        case SBR_DBG_DINPUT: src = bv.dX; n = R * d * 4; break;
        case SBR_DBG_DENSE_GRAD: src = bv.dense; n = dense_count(m) * 4; break;
        case SBR_DBG_IN_IDX: src = bv.in_idx; n = R * 4; break;
        case SBR_DBG_OUT_IDX: src = bv.out_idx; n = R * 4; break;
        case SBR_DBG_TRIES: src = p->wb.v.tries; n = R * 4; break;
        case SBR_DBG_DZ: if (!m->ng) return SBR_ERR_INVALID_ARGUMENT; src = p->wb.v.dZ; n = R * (uint64_t)m->ng * d * 4; break;
        default: return SBR_ERR_INVALID_ARGUMENT;
    }
    if (bytes < n) return SBR_ERR_INVALID_ARGUMENT;
    if (n) HIPCHK(hipMemcpy(host_out, src, n, hipMemcpyDeviceToHost));
    return SBR_OK;
}

/* ---------------------------------------------------------------------------------------------
 * prediction side
 * ------------------------------------------------------------------------------------------- */
namespace {

using Carve = std::function<void(DeviceArena&)>; /* a run of takes */

/* Reserves the model's eval arena for one launch and carves it: `carve` — the one place that says which buffers the launch has —
 * runs once measuring, the arena is reserved to what that took, and it runs again for real. */
sbr_status carve_arena(sbr_model* m, const Carve& carve) {
    DeviceArena& ar = m->eval_arena;
    const size_t guard = test_guard_bytes();
    ar.measure(guard);
    carve(ar);
    HIPCHK(hipStreamSynchronize(m->stream)); /* nothing of an earlier call may still read the arena */
    const size_t need = ar.used;
    check_arena_guards(ar); /* SBR_TEST_GUARD: what the last carve's kernels left of its bands (the measuring pass keeps its takes) */
    SBRCHK(ar.reserve(need));
    if (const int poison = test_poison_byte()) { /* what this carve uses, not cap: an earlier call may have grown it to gigabytes */
        HIPCHK(hipMemsetAsync(ar.base, poison, need, m->stream));
        if (!guard) HIPCHK(hipStreamSynchronize(m->stream)); /* a caller may fill its buffers with blocking copies, which no stream orders */
    }
    carve(ar);
    if (guard && !ar.overrun) { /* behind the poison fill on the same stream: poison in the payload, the guard byte in the bands */
        HIPCHK(hipMemsetAsync(ar.base, kGuardByte, ar.front, m->stream));
        for (const DeviceArena::Take& t : ar.takes) HIPCHK(hipMemsetAsync(ar.base + t.at + t.req, kGuardByte, t.band_end - (t.at + t.req), m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
    }
    if (ar.overrun) ar.takes.clear(); /* no bands were filled */
    return ar.overrun ? SBR_ERR_OUT_OF_MEMORY : SBR_OK;
}

/* device buffers of the recurrent forward over the packed sequences `pk` */
struct ForwardBufs {
    DevicePacked dp;
    float* H = nullptr;
    WorkBuffers wb;
    void carve(DeviceArena& ar, const sbr_model* m, const Packed& pk) {
        const size_t R = (size_t)pk.R, d = (size_t)m->d;
        dp.in_idx = ar.take<uint32_t>(R); /* no out_idx / ctr: only the score kernels of a training step read them */
        dp.prev_row = ar.take<int>(R); dp.off = ar.take<int>(pk.off.size()); dp.steps = ar.take<int>((size_t)pk.B);
        H = ar.take<float>(R * d);
        if (m->ng) {
            wb.v.C = ar.take<float>(R * d);
            wb.v.G = ar.take<float>(R * d * 4);
            wb.v.X = ar.take<float>(R * d);
        }
    }
};

/* The packed layout of a forward pass, for a caller that reads more than the final states: history i is sequence b with
 * pk.order[b] = i, its state after step t is row pk.off[t] + b of H and its t-th input item in_idx[pk.off[t] + b]; d_off / d_in_idx
 * are the device copies of pk.off / pk.in_idx in the eval arena, valid as long as H. */
struct PackedLayout {
    Packed pk;
    const int* d_off = nullptr;
    const uint32_t* d_in_idx = nullptr;
};

/* Runs the recurrent forward for a batch of histories; the hidden states are left in *H_out — memory of the model's eval arena,
 * valid until the next carve_arena — and rep_row[i] = packed row of the final state of history i.  `carve_epilogue`: what the
 * caller uses from the arena afterwards (the scan kernels' arrays), carved behind the forward pass's in the same allocation.
 * `layout` non-null: the packed layout is handed back (sequence_ranks scans every step's state, not the last one's alone). */
sbr_status forward_histories(sbr_model* m, const std::vector<const uint32_t*>& first, const std::vector<int>& nsteps,
                             const Carve& carve_epilogue, float** H_out, std::vector<int>* rep_row, PackedLayout* layout = nullptr) {
    Packed pk;
    pack_sequences(first, nsteps, false, nullptr, (int)m->hp.max_sequence_length, &pk);
    ForwardBufs fb;
    fb.wb.v.fold_max_tiles = SBR_FOLD_MAX_TILES_DEFAULT;
    SBRCHK(carve_arena(m, [&](DeviceArena& ar) { fb.carve(ar, m, pk); carve_epilogue(ar); }));
    const DevicePacked& dp = fb.dp;
    HIPCHK(hipMemcpyAsync(dp.in_idx, pk.in_idx.data(), (size_t)pk.R * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(dp.prev_row, pk.prev_row.data(), (size_t)pk.R * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(dp.off, pk.off.data(), pk.off.size() * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(dp.steps, pk.steps.data(), (size_t)pk.B * 4, hipMemcpyHostToDevice, m->stream));
    sbr::MbView mv;
    mv.R = pk.R; mv.B = pk.B; mv.Tm = pk.Tm;
    mv.off = dp.off; mv.steps = dp.steps; mv.prev_row = dp.prev_row;
    mv.in_idx = dp.in_idx; mv.out_idx = dp.out_idx; mv.ctr = dp.ctr;
    {
        ScopedTimer t(m, SBR_K_RECURRENT_FWD, m->ng && m->d > 128 ? (uint64_t)pk.Tm : 1);
        sbr::launch_recurrent_forward(m->mv, mv, fb.H, fb.wb.v, pk.Tm, pk.off.data(), m->stream);
    }
    /* the host vectors of `pk` are read by the asynchronous copies above: drain them before pk goes out of scope */
    HIPCHK(hipStreamSynchronize(m->stream));
    rep_row->assign(first.size(), 0);
    for (int b = 0; b < pk.B; ++b) (*rep_row)[pk.order[b]] = pk.off[pk.steps[b] - 1] + b;
    *H_out = fb.H;
    if (layout) {
        layout->d_off = dp.off;
        layout->d_in_idx = dp.in_idx;
        layout->pk = std::move(pk);
    }
    return SBR_OK;
}

/* The state of a history of n items: its last T items (sequence_model.rs:188); an empty history is one step of item 0
 * (lstm.rs:262-264). */
void state_window(const uint32_t* items, uint64_t n, uint64_t T, const uint32_t** first, int* nsteps) {
    static const uint32_t zero = 0;
    const uint64_t keep = std::min(n, T);
    *first = n ? items + (n - keep) : &zero;
    *nsteps = n ? (int)keep : 1;
}

/* A batch of users, user i's history items[i][0, len[i]): the state windows and, with lists, each history sorted and
 * de-duplicated in one CSR buffer (list_ptr [nu + 1], list_items; both empty without lists). */
struct UserBatch {
    std::vector<const uint32_t*> first;
    std::vector<int> nsteps;
    std::vector<uint64_t> list_ptr;
    std::vector<uint32_t> list_items;
};

void prepare_users(const std::vector<const uint32_t*>& items, const std::vector<uint64_t>& len, uint64_t T, bool lists, UserBatch* out) {
    const size_t nu = items.size();
    UserBatch& b = *out;
    b.first.resize(nu);
    b.nsteps.resize(nu);
    std::vector<uint64_t> raw_ptr(nu + 1, 0);
    std::vector<uint32_t> uniq_count(nu, 0);
    if (lists) {
        for (size_t i = 0; i < nu; ++i) raw_ptr[i + 1] = raw_ptr[i] + len[i];
        b.list_items.resize(raw_ptr[nu]);
        b.list_ptr.assign(nu + 1, 0);
    }
    /* sorted + de-duplicated in place inside one buffer (a vector per user was a third of mrr_score's host time at 8 192 users),
     * a few host threads over user ranges */
    auto prepare = [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) {
            state_window(items[i], len[i], T, &b.first[i], &b.nsteps[i]);
            if (!lists || len[i] == 0) continue;
            uint32_t* h = b.list_items.data() + raw_ptr[i];
            std::memcpy(h, items[i], len[i] * 4);
            std::sort(h, h + len[i]);
            uniq_count[i] = (uint32_t)(std::unique(h, h + len[i]) - h);
        }
    };
    const size_t nthreads = nu >= 2048 ? 8 : 1;
    if (nthreads == 1) prepare(0, nu);
    else {
        std::vector<std::thread> workers;
        for (size_t t = 0; t < nthreads; ++t) workers.emplace_back(prepare, nu * t / nthreads, nu * (t + 1) / nthreads);
        for (auto& w : workers) w.join();
    }
    if (lists) {
        for (size_t i = 0; i < nu; ++i) { /* close the gaps the de-duplication left */
            if (b.list_ptr[i] != raw_ptr[i]) std::memmove(b.list_items.data() + b.list_ptr[i], b.list_items.data() + raw_ptr[i], (size_t)uniq_count[i] * 4);
            b.list_ptr[i + 1] = b.list_ptr[i] + uniq_count[i];
        }
        b.list_items.resize(b.list_ptr[nu]);
    }
}

/* A CSR argument of a call (histories, exclusion lists, target lists): ptr[0 .. n] non-decreasing and every id of
 * ids[from, ptr[n]) below num_items, from = 0 (from_zero) or ptr[0]; ids may be null only where that range is empty. */
sbr_status check_csr(const sbr_model* m, const uint64_t* ptr, uint64_t n, const uint32_t* ids, bool from_zero) {
    for (uint64_t u = 0; u < n; ++u)
        if (ptr[u + 1] < ptr[u]) return SBR_ERR_INVALID_ARGUMENT;
    const uint64_t from = from_zero ? 0 : ptr[0];
    if (ptr[n] > from && !ids) return SBR_ERR_INVALID_ARGUMENT;
    for (uint64_t i = from; i < ptr[n]; ++i)
        if (ids[i] >= m->hp.num_items) return SBR_ERR_INVALID_ARGUMENT;
    return SBR_OK;
}

/* Where a call's user representations come from: the histories ptr / items (the recurrent forward runs), the rows `reps`
 * ([users, embedding_dim]) of the caller, rows the device makes from the item table, user u's from item item_rows[u]
 * (similar_items), or rows that already lie on the device at the storage width, user u's row dev_row[u] of dev_rows (a session
 * store: read in place); in the last three cases ptr / items are the exclusion lists (ptr null: none).  With `seen` (a session
 * store's seen-item memory; only with device rows, and only recommend_scan reads it) the device unites user u's list with what
 * slot seen_slots[u] remembers. */
struct RepSource {
    const uint64_t* ptr = nullptr;
    const uint32_t* items = nullptr;
    const float* reps = nullptr;  /* null: from histories or item rows */
    uint64_t held_out = 0;  /* histories: this many items at the end of each are not part of it (mrr_score: the test item) */
    bool lists = true;      /* whether the sorted, de-duplicated lists of ptr / items are wanted (with reps or item rows: always) */
    const uint32_t* item_rows = nullptr; /* non-null: the rows come from these item ids, on the device */
    const float* dev_rows = nullptr;     /* non-null: device rows [.][storage width], read in place ... */
    const int* dev_row = nullptr;        /* ... user u's is row dev_row[u] */
    const sbr::SeenView* seen = nullptr; /* non-null: lists come from a store's memory as well ... */
    const uint32_t* seen_slots = nullptr; /* ... user u's (the CALL's index) from this slot */
    bool from_histories() const { return !reps && !item_rows && !dev_rows; }
    /* the makers (member functions: the file's helpers stand inside extern "C", where a free function may not return a struct) */
    static RepSource of_histories(const uint64_t* ptr, const uint32_t* items, uint64_t held_out, bool lists) {
        RepSource s;
        s.ptr = ptr; s.items = items; s.held_out = held_out; s.lists = lists;
        return s;
    }
    static RepSource of_rows(const float* reps, const uint64_t* excl_ptr = nullptr, const uint32_t* excl_items = nullptr) {
        RepSource s;
        s.ptr = excl_ptr; s.items = excl_items; s.reps = reps;
        return s;
    }
    static RepSource of_item_rows(const uint32_t* item_rows, const uint64_t* excl_ptr, const uint32_t* excl_items) {
        RepSource s;
        s.ptr = excl_ptr; s.items = excl_items; s.item_rows = item_rows;
        return s;
    }
    /* a session store's rows, read in place: `rows` = session_rep_rows of the call's slots (the caller keeps it alive over the
     * scan), excl_ptr / excl_items the caller's exclusion lists (null: none); seen_slots non-null (a store with memory): the call's
     * slots, whose memories the scan unites with those lists */
    static RepSource of_sessions(const sbr_sessions* st, const std::vector<int>& rows, const uint64_t* excl_ptr, const uint32_t* excl_items,
                                 const uint32_t* seen_slots);
};

/* The representations of a chunk's users: user i's is row rep_row[i] of H (eval arena, valid until the next carve_arena; with
 * item rows H is not filled yet: the launch does that from d_item_rows);
 * b.list_ptr / b.list_items are the users' sorted, de-duplicated lists (both empty: none). */
struct UserReps {
    float* H = nullptr;
    std::vector<int> rep_row;
    UserBatch b;
    std::vector<float> gathered; /* caller's rows of users that are not consecutive, read by an asynchronous copy */
    std::vector<uint32_t> item_rows;  /* item rows: the users' item ids, read by an asynchronous copy into ... */
    uint32_t* d_item_rows = nullptr;  /* ... the arena; the launch fills H from them */
    PackedLayout* layout = nullptr;   /* non-null (the caller's, histories only): forward_histories' packed layout is left here */
};

/* Fills *out for `users` of `s`; `carve_epilogue` as forward_histories' (it may read out->b, which is complete by then).  The
 * uploads are asynchronous: *out lives until the stream is synchronised. */
sbr_status user_reps(sbr_model* m, const RepSource& s, const std::vector<uint64_t>& users, const Carve& carve_epilogue, UserReps* out) {
    const size_t nu = users.size(), d = (size_t)m->d, dl = (size_t)m->dl;
    const uint64_t T = m->hp.max_sequence_length;
    if (s.ptr) {
        std::vector<const uint32_t*> list(nu);
        std::vector<uint64_t> n(nu);
        for (size_t i = 0; i < nu; ++i) {
            list[i] = s.items ? s.items + s.ptr[users[i]] : nullptr;
            n[i] = s.ptr[users[i] + 1] - s.ptr[users[i]] - s.held_out;
        }
        /* with reps or item rows: the caller's lists, sorted and de-duplicated (their state windows go unused) */
        prepare_users(list, n, T, s.lists, &out->b);
    }
    if (s.from_histories()) return forward_histories(m, out->b.first, out->b.nsteps, carve_epilogue, &out->H, &out->rep_row, out->layout);
    if (s.dev_rows) { /* nothing is made or moved: the scan reads the caller's device rows through rep_row */
        SBRCHK(carve_arena(m, carve_epilogue));
        out->H = const_cast<float*>(s.dev_rows);
        out->rep_row.resize(nu);
        for (size_t i = 0; i < nu; ++i) out->rep_row[i] = s.dev_row[users[i]];
        return SBR_OK;
    }
    SBRCHK(carve_arena(m, [&](DeviceArena& ar) {
        out->H = ar.take<float>(nu * d);
        if (s.item_rows) out->d_item_rows = ar.take<uint32_t>(nu);
        carve_epilogue(ar);
    }));
    out->rep_row.resize(nu);
    for (size_t i = 0; i < nu; ++i) out->rep_row[i] = (int)i;
    if (s.item_rows) {
        out->item_rows.resize(nu);
        for (size_t i = 0; i < nu; ++i) out->item_rows[i] = s.item_rows[users[i]];
        HIPCHK(hipMemcpyAsync(out->d_item_rows, out->item_rows.data(), nu * 4, hipMemcpyHostToDevice, m->stream));
        return SBR_OK;
    }
    const float* rows = s.reps + users[0] * dl;
    if (users[nu - 1] - users[0] + 1 != nu) {
        out->gathered.resize(nu * dl);
        for (size_t i = 0; i < nu; ++i) std::memcpy(out->gathered.data() + i * dl, s.reps + users[i] * dl, dl * 4);
        rows = out->gathered.data();
    }
    /* padded to the storage width: the columns past embedding_dim are zero, as in the model's own states */
    HIPCHK(hipMemsetAsync(out->H, 0, nu * d * 4, m->stream));
    HIPCHK(hipMemcpy2DAsync(out->H, d * 4, rows, dl * 4, dl * 4, nu, hipMemcpyHostToDevice, m->stream));
    return SBR_OK;
}

/* Scan units per launch (a unit: a user, or a scan-user of rank_targets): the scan GEMM streams the item table once per 128 units
 * whatever the launch size, but every launch has its ramp and tail — mrr_score at 8 192 users x 1e6 items, d = 128: 104 / 108 /
 * 109 / 112 TFLOP/s at 1 024 / 2 048 / 4 096 / 8 192 users per launch */
constexpr size_t eval_units_cap = 8192;
/* the forward pass's scratch is (users x history steps) rows of 6d floats: bound a launch by rows as well */
constexpr size_t eval_rows_cap = (size_t)1 << 22;

/* One launch's share [c0, c1) of a call's scan units: its distinct users, ascending, and each unit's index into them */
struct Chunk {
    size_t c0 = 0, c1 = 0;
    std::vector<uint64_t> users;
    std::vector<uint32_t> lu;
};

/* Moves *ch to the chunk after it (a fresh Chunk: to the first); false when the units are used up.  unit_user[i] = user of unit
 * i, units of one user adjacent.  A chunk ends at unit_cap units and, where the forward pass runs, before the user whose rows take
 * it past eval_rows_cap unless it is the chunk's first; a user cut by a chunk's end is forwarded again in the next one. */
bool next_chunk(const std::vector<uint64_t>& unit_user, size_t unit_cap, const RepSource& s, uint64_t T, Chunk* ch) {
    const size_t c0 = ch->c1;
    if (c0 >= unit_user.size()) return false;
    ch->users.clear();
    ch->lu.clear();
    size_t c1 = c0, rows = 0;
    for (; c1 < unit_user.size() && c1 - c0 < unit_cap; ++c1) {
        const uint64_t u = unit_user[c1];
        if (c1 == c0 || u != unit_user[c1 - 1]) {
            if (s.from_histories()) {
                rows += (size_t)std::max<uint64_t>(1, std::min<uint64_t>(s.ptr[u + 1] - s.ptr[u] - s.held_out, T));
                if (rows > eval_rows_cap && c1 > c0) break;
            }
            ch->users.push_back(u);
        }
        ch->lu.push_back((uint32_t)(ch->users.size() - 1));
    }
    ch->c0 = c0;
    ch->c1 = c1;
    return true;
}

struct CopyOut { void* host; const void* device; size_t bytes; }; /* host null: not wanted */

/* a host CSR to its device arrays, by asynchronous copies: ptr, then the items unless there are none */
sbr_status upload_csr(sbr_model* m, uint64_t* d_ptr, const std::vector<uint64_t>& ptr, uint32_t* d_items, const std::vector<uint32_t>& items) {
    HIPCHK(hipMemcpyAsync(d_ptr, ptr.data(), ptr.size() * 8, hipMemcpyHostToDevice, m->stream));
    if (!items.empty()) HIPCHK(hipMemcpyAsync(d_items, items.data(), items.size() * 4, hipMemcpyHostToDevice, m->stream));
    return SBR_OK;
}

/* The tail of every catalogue scan: `launch` (timed as SBR_K_RANK; it returns the launches its launchers report, the ledger's
 * count) with the non-finite-score flag cleared before it, then — the stream drained, so the caller's host vectors have been read
 * by their asynchronous copies — the flag and, if it is clear, the results. */
sbr_status scan_launch(sbr_model* m, uint32_t* d_flag, const std::function<int()>& launch, std::initializer_list<CopyOut> outs) {
    HIPCHK(hipMemsetAsync(d_flag, 0, 4, m->stream));
    {
        ScopedTimer t(m, SBR_K_RANK, 0);
        t.tp.launches = (uint64_t)launch();
    }
    uint32_t flag = 0;
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipMemcpy(&flag, d_flag, 4, hipMemcpyDeviceToHost));
    if (flag) return SBR_ERR_INVALID_PREDICTION; /* predict fails the call on a non-finite score */
    for (const CopyOut& o : outs)
        if (o.host) HIPCHK(hipMemcpy(o.host, o.device, o.bytes, hipMemcpyDeviceToHost));
    return SBR_OK;
}

}  // namespace

sbr_status sbr_user_representation(sbr_model* m, const uint32_t* item_ids, uint64_t n, float* out_dim) {
    if (!m || !out_dim || (n && !item_ids)) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    const uint32_t* first = nullptr;
    int nsteps = 0;
    state_window(item_ids, n, m->hp.max_sequence_length, &first, &nsteps);
    for (int t = 0; t < nsteps; ++t)
        if (first[t] >= m->hp.num_items) return SBR_ERR_INVALID_ARGUMENT;
    const uint64_t ptr[2] = {0, n};
    UserReps ur;
    SBRCHK(user_reps(m, RepSource::of_histories(ptr, item_ids, 0, false), std::vector<uint64_t>(1, 0), [](DeviceArena&) {}, &ur));
    hipError_t e = hipMemcpy(out_dim, ur.H + (size_t)ur.rep_row[0] * m->d, (size_t)m->dl * 4, hipMemcpyDeviceToHost);
    return e == hipSuccess ? SBR_OK : SBR_ERR_HIP;
}

sbr_status sbr_predict(sbr_model* m, const float* user_dim, const uint32_t* item_ids, uint64_t n, float* out) {
    if (!m || !user_dim || (n && (!item_ids || !out))) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    for (uint64_t i = 0; i < n; ++i)
        if (item_ids[i] >= m->hp.num_items) return SBR_ERR_INVALID_ARGUMENT;
    if (n == 0) return SBR_OK;
    float *d_user = nullptr, *d_out = nullptr;
    uint32_t* d_items = nullptr;
    sbr_status st = SBR_OK;
    if ((st = dmalloc(&d_user, m->d)) == SBR_OK && (st = dmalloc(&d_items, n)) == SBR_OK && (st = dmalloc(&d_out, n)) == SBR_OK) {
        hipMemset(d_user, 0, (size_t)m->d * 4);
        hipMemcpy(d_user, user_dim, (size_t)m->dl * 4, hipMemcpyHostToDevice);
        hipMemcpy(d_items, item_ids, n * 4, hipMemcpyHostToDevice);
        sbr::launch_predict(m->mv, d_user, d_items, n, d_out, m->stream);
        if (hipStreamSynchronize(m->stream) != hipSuccess || hipMemcpy(out, d_out, n * 4, hipMemcpyDeviceToHost) != hipSuccess)
            st = SBR_ERR_HIP;
    }
    dfree(d_user); dfree(d_items); dfree(d_out);
    if (st != SBR_OK) return st;
    for (uint64_t i = 0; i < n; ++i)
        if (!std::isfinite(out[i])) return SBR_ERR_INVALID_PREDICTION; /* sequence_model.rs:225-229 */
    return SBR_OK;
}

namespace {

/* device buffers of launch_rank over nu users with nhist mask entries */
struct MrrBufs {
    int* rep;
    uint32_t *test, *tih, *hist, *ranks, *flag;
    float* ts;
    uint64_t* hptr;
    void carve(DeviceArena& ar, size_t nu, size_t nhist) {
        rep = ar.take<int>(nu);
        test = ar.take<uint32_t>(nu); tih = ar.take<uint32_t>(nu); hist = ar.take<uint32_t>(nhist);
        ranks = ar.take<uint32_t>(nu); flag = ar.take<uint32_t>(1);
        ts = ar.take<float>(nu);
        hptr = ar.take<uint64_t>(nu + 1);
    }
};

}  // namespace

sbr_status sbr_mrr_score(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users,
                         float* out_mrr, uint32_t* out_ranks, uint64_t* out_num_ranked) {
    if (!m || !user_ptr || !out_mrr) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    SBRCHK(check_csr(m, user_ptr, num_users, item_ids, true));
    std::vector<uint64_t> users; /* users with >= 2 interactions (evaluation.rs:20) */
    for (uint64_t u = 0; u < num_users; ++u)
        if (user_ptr[u + 1] - user_ptr[u] >= 2) users.push_back(u);
    if (out_num_ranked) *out_num_ranked = users.size();
    std::vector<uint32_t> ranks(users.size(), 0);
    /* train_items = all but last (evaluation.rs:24); ALL history items of a user are masked (evaluation.rs:30-32) */
    const RepSource s = RepSource::of_histories(user_ptr, item_ids, 1, true);
    for (Chunk ch; next_chunk(users, eval_units_cap, s, m->hp.max_sequence_length, &ch);) {
        const size_t nu = ch.users.size();
        UserReps ur;
        MrrBufs mb;
        SBRCHK(user_reps(m, s, ch.users, [&](DeviceArena& ar) { mb.carve(ar, nu, ur.b.list_items.size()); }, &ur));
        const std::vector<uint64_t>& hist_ptr = ur.b.list_ptr;
        const std::vector<uint32_t>& hist_items = ur.b.list_items;
        std::vector<uint32_t> test_item(nu), test_in_hist(nu);
        for (size_t i = 0; i < nu; ++i) {
            test_item[i] = item_ids[user_ptr[ch.users[i] + 1] - 1];
            test_in_hist[i] = std::binary_search(hist_items.data() + hist_ptr[i], hist_items.data() + hist_ptr[i + 1], test_item[i]) ? 1u : 0u;
        }
        HIPCHK(hipMemcpyAsync(mb.rep, ur.rep_row.data(), nu * 4, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(mb.test, test_item.data(), nu * 4, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(mb.tih, test_in_hist.data(), nu * 4, hipMemcpyHostToDevice, m->stream));
        SBRCHK(upload_csr(m, mb.hptr, hist_ptr, mb.hist, hist_items));
        SBRCHK(scan_launch(m, mb.flag, [&] {
            return sbr::launch_rank(m->mv, ur.H, mb.rep, (uint32_t)nu, mb.test, mb.tih, mb.hptr, mb.hist, mb.ts, mb.ranks, mb.flag, m->stream);
        }, {{ranks.data() + ch.c0, mb.ranks, nu * 4}}));
    }
    float sum = 0.0f; /* evaluation.rs:47 — sequential f32 sum in user order */
    for (size_t i = 0; i < ranks.size(); ++i) sum += 1.0f / (float)ranks[i];
    *out_mrr = sum / (float)ranks.size();
    if (out_ranks) std::memcpy(out_ranks, ranks.data(), ranks.size() * 4);
    return SBR_OK;
}

namespace {

/* device buffers of launch_sequence_ranks over ns scan rows of sequences with nrows packed rows */
struct SequenceRanksBufs {
    int* rep;
    uint32_t *test, *tip, *first, *ranks, *flag;
    uint2* bt;
    float* ts;
    void carve(DeviceArena& ar, size_t ns, size_t nrows) {
        rep = ar.take<int>(ns);
        test = ar.take<uint32_t>(ns); tip = ar.take<uint32_t>(ns);
        bt = ar.take<uint2>(ns);
        first = ar.take<uint32_t>(nrows);
        ranks = ar.take<uint32_t>(ns); flag = ar.take<uint32_t>(1);
        ts = ar.take<float>(ns);
    }
};

/* first[j] = 1 where w[j] does not occur in w[0 .. j): a stable sort of the positions by item, O(W log W) */
void first_occurrences(const uint32_t* w, size_t W, std::vector<uint32_t>* idx, uint32_t* first) {
    idx->resize(W);
    for (size_t j = 0; j < W; ++j) (*idx)[j] = (uint32_t)j;
    std::sort(idx->begin(), idx->end(), [&](uint32_t a, uint32_t b) { return w[a] != w[b] ? w[a] < w[b] : a < b; });
    for (size_t k = 0; k < W; ++k) first[(*idx)[k]] = k == 0 || w[(*idx)[k]] != w[(*idx)[k - 1]] ? 1u : 0u;
}

/* The windows and scan units the sequence_* calls share (the contract: sbr_sequence_ranks in include/sbr_hip.h): the window of a
 * user with n items is its last W = min(n, T + 1); its positions are 1 .. W - 1, of which the last `kept` are scanned. */
struct SequenceUnits {
    const uint64_t* user_ptr;
    uint64_t num_users, T;
    uint32_t last_positions;
    uint64_t total = 0;               /* kept positions of the call */
    std::vector<uint64_t> unit_user;  /* scan units: (user, position), a user's adjacent and ascending — the order of the output rows */
    std::vector<uint32_t> unit_pos;
    SequenceUnits(const sbr_model* m, const uint64_t* ptr, uint64_t nu, uint32_t last)
        : user_ptr(ptr), num_users(nu), T(m->hp.max_sequence_length), last_positions(last) {
        for (uint64_t u = 0; u < num_users; ++u) {
            uint64_t W, kept;
            window(u, &W, &kept);
            total += kept;
        }
    }
    void window(uint64_t u, uint64_t* W, uint64_t* kept) const {
        const uint64_t n = user_ptr[u + 1] - user_ptr[u];
        *W = std::min(n, T + 1);
        *kept = n < 2 ? 0 : *W - 1;
        if (last_positions) *kept = std::min<uint64_t>(*kept, last_positions);
    }
    void list_units() {
        unit_user.reserve(total);
        unit_pos.reserve(total);
        for (uint64_t u = 0; u < num_users; ++u) {
            uint64_t W, kept;
            window(u, &W, &kept);
            for (uint64_t p = W - kept; p < W; ++p) {
                unit_user.push_back(u);
                unit_pos.push_back((uint32_t)p);
            }
        }
    }
    void fill_out_ptr(uint64_t* out_ptr) const {
        out_ptr[0] = 0;
        for (uint64_t u = 0; u < num_users; ++u) {
            uint64_t W, kept;
            window(u, &W, &kept);
            out_ptr[u + 1] = out_ptr[u] + kept;
        }
    }
};

/* One chunk's scan rows over the forward pass's packed layout: per sequence, once, the first-occurrence flags of its window — those
 * of the W - 1 inputs by packed row (first_rows, the device's), and position p's own flag says whether its target occurs in its
 * prefix (in_prefix, set only while `mask`); per scan row its state's packed row, (sequence, step) and target. */
struct SequenceRows {
    std::vector<int> seq_of, rep;
    std::vector<uint64_t> wptr;
    std::vector<uint32_t> wfirst, first_rows, test, in_prefix;
    std::vector<uint2> bt;
    void build(const Chunk& ch, const UserReps& ur, const Packed& pk, const std::vector<uint32_t>& unit_pos, bool mask) {
        const size_t ns = ch.c1 - ch.c0, nlu = ch.users.size();
        seq_of.assign(nlu, 0);
        for (int b = 0; b < pk.B; ++b) seq_of[pk.order[b]] = b;
        wptr.assign(nlu + 1, 0);
        for (size_t i = 0; i < nlu; ++i) wptr[i + 1] = wptr[i] + (uint64_t)ur.b.nsteps[i] + 1;
        wfirst.assign(wptr[nlu], 0);
        first_rows.assign((size_t)pk.R, 0);
        std::vector<uint32_t> order;
        for (size_t i = 0; i < nlu; ++i) {
            const size_t W = (size_t)ur.b.nsteps[i] + 1;
            first_occurrences(ur.b.first[i], W, &order, wfirst.data() + wptr[i]);
            for (size_t j = 0; j + 1 < W; ++j) first_rows[(size_t)pk.off[j] + seq_of[i]] = wfirst[wptr[i] + j];
        }
        rep.resize(ns); test.resize(ns); in_prefix.resize(ns); bt.resize(ns);
        for (size_t i = 0; i < ns; ++i) {
            const uint32_t lu = ch.lu[i], p = unit_pos[ch.c0 + i];
            const int b = seq_of[lu];
            rep[i] = pk.off[p - 1] + b;
            bt[i] = make_uint2((uint32_t)b, p - 1);
            test[i] = ur.b.first[lu][p];
            in_prefix[i] = mask && !wfirst[wptr[lu] + p] ? 1u : 0u;
        }
    }
};

}  // namespace

sbr_status sbr_sequence_ranks(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, uint32_t flags,
                              uint32_t last_positions, uint64_t* out_ptr, uint32_t* out_ranks) {
    if (!m || !user_ptr || !out_ptr || (flags & ~SBR_RANK_INCLUDE_HISTORY)) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    if (m->open_plans) return SBR_ERR_INVALID_ARGUMENT; /* the plan's steps write the parameters this call reads row after row */
    SBRCHK(check_csr(m, user_ptr, num_users, item_ids, false));
    const uint64_t T = m->hp.max_sequence_length;
    const bool mask = !(flags & SBR_RANK_INCLUDE_HISTORY);
    SequenceUnits su(m, user_ptr, num_users, last_positions);
    const uint64_t total = su.total;
    if (out_ranks) {
        su.list_units();
        std::vector<uint32_t> ranks(total, 0);
        /* the forward pass runs over the window's first W - 1 items: all but the last item, of which the last T (as mrr_score) */
        const RepSource s = RepSource::of_histories(user_ptr, item_ids, 1, false);
        for (Chunk ch; next_chunk(su.unit_user, eval_units_cap, s, T, &ch);) {
            const size_t ns = ch.c1 - ch.c0;
            PackedLayout lay;
            UserReps ur;
            ur.layout = &lay;
            SequenceRanksBufs sb;
            SBRCHK(user_reps(m, s, ch.users, [&](DeviceArena& ar) {
                size_t nrows = 0;
                for (int n : ur.b.nsteps) nrows += (size_t)n;
                sb.carve(ar, ns, nrows);
            }, &ur));
            SequenceRows sr;
            sr.build(ch, ur, lay.pk, su.unit_pos, mask);
            HIPCHK(hipMemcpyAsync(sb.rep, sr.rep.data(), ns * 4, hipMemcpyHostToDevice, m->stream));
            HIPCHK(hipMemcpyAsync(sb.test, sr.test.data(), ns * 4, hipMemcpyHostToDevice, m->stream));
            HIPCHK(hipMemcpyAsync(sb.tip, sr.in_prefix.data(), ns * 4, hipMemcpyHostToDevice, m->stream));
            if (mask) {
                HIPCHK(hipMemcpyAsync(sb.bt, sr.bt.data(), ns * 8, hipMemcpyHostToDevice, m->stream));
                HIPCHK(hipMemcpyAsync(sb.first, sr.first_rows.data(), sr.first_rows.size() * 4, hipMemcpyHostToDevice, m->stream));
            }
            SBRCHK(scan_launch(m, sb.flag, [&] {
                return sbr::launch_sequence_ranks(m->mv, ur.H, sb.rep, (uint32_t)ns, sb.test, sb.tip, mask ? sb.bt : nullptr, lay.d_off, lay.d_in_idx,
                                                  sb.first, sb.ts, sb.ranks, sb.flag, m->stream);
            }, {{ranks.data() + ch.c0, sb.ranks, ns * 4}}));
        }
        if (total) std::memcpy(out_ranks, ranks.data(), total * 4);
    }
    su.fill_out_ptr(out_ptr);
    return SBR_OK;
}

/* ---------------------------------------------------------------------------------------------
 * exact top-k recommendation (sbr_catalogue.hip)
 * ------------------------------------------------------------------------------------------- */
namespace {

/* users per top-k launch: eval_units_cap, and few enough that the per-(user, item range) lists stay within 256 MB.  With
 * ranges * k <= TK_MERGE_MAX the lists of 8 192 users are at most 512 MB, so the loop halves at most once: 8 192 users while
 * ranges * k <= 4 096 (every k <= 256: at most 16 ranges are wanted for 64 user tiles), 4 096 users above that (possible from
 * k = 257 on; k = 1 024 from 5 ranges on) or where SBR_CATALOGUE_GROUPS forces more ranges. */
size_t recommend_users_cap(uint32_t num_items, uint32_t k) {
    size_t cap = eval_units_cap;
    for (;;) {
        uint32_t per = 0;
        const uint32_t g = sbr::recommend_groups((uint32_t)cap, num_items, k, &per);
        if (cap <= 128 || cap * g * k * 8 <= ((size_t)256 << 20)) return cap;
        cap /= 2;
    }
}

/* device buffers of launch_recommend over nu users with nexcl exclusion entries and a catalogue of num_items (the model's, or the
 * size of recommend_among's item set: the scan splits what it scans) */
struct TopkBufs {
    int* rep;
    uint64_t* eptr;
    uint32_t *excl, *lens, *items, *flag;
    uint32_t *any_of = nullptr, *none_of = nullptr; /* the tag filter's masks, one pair per user (with_masks) */
    uint2* lists;
    float* scores;
    void carve(DeviceArena& ar, uint32_t num_items, size_t nu, size_t nexcl, uint32_t k, bool with_masks) {
        uint32_t per = 0;
        const size_t g = sbr::recommend_groups((uint32_t)nu, num_items, k, &per);
        rep = ar.take<int>(nu);
        if (with_masks) {
            any_of = ar.take<uint32_t>(nu);
            none_of = ar.take<uint32_t>(nu);
        }
        eptr = ar.take<uint64_t>(nu + 1);
        excl = ar.take<uint32_t>(nexcl + 1);
        lists = ar.take<uint2>(nu * g * k);
        lens = ar.take<uint32_t>(nu * g);
        items = ar.take<uint32_t>(nu * k);
        scores = ar.take<float>(nu * k);
        flag = ar.take<uint32_t>(1);
    }
    /* the launch's descriptor over these buffers: nu users at k, with the exclusion CSR in eptr / excl or without one, scores
     * wanted or not, tags = the model's item tags where the masks filter (with_masks), else null */
    sbr::TopkScan scan(size_t nu, uint32_t k, bool exclusions, bool want_scores, const uint32_t* tags = nullptr) const {
        sbr::TopkScan sc{};
        sc.rep_row = rep; sc.n = (uint32_t)nu; sc.k = k;
        sc.excl_ptr = exclusions ? eptr : nullptr; sc.excl_items = excl;
        sc.lists = lists; sc.lens = lens; sc.out_items = items; sc.out_scores = want_scores ? scores : nullptr;
        sc.nonfinite_flag = flag;
        sc.f = sbr::TagMasks{tags, any_of, none_of};
        return sc;
    }
};

/* device buffers of recommend_among's sub-table of ns items, made anew by every launch (the arena does not outlive a carve) */
struct SubsetBufs {
    uint32_t* ids;
    float *E, *b;
    void carve(DeviceArena& ar, size_t ns, size_t d) {
        ids = ar.take<uint32_t>(ns);
        E = ar.take<float>(ns * d);
        b = ar.take<float>(ns);
    }
};

/* The users' sorted, de-duplicated lists as positions in the sorted, unique item set `subset`; entries outside it are dropped (they
 * are not scanned).  Both sides ascend, so the positions do too. */
void lists_to_subset_positions(const std::vector<uint32_t>& subset, std::vector<uint64_t>* list_ptr, std::vector<uint32_t>* list_items) {
    size_t w = 0;
    for (size_t u = 0; u + 1 < list_ptr->size(); ++u) {
        const uint64_t e0 = (*list_ptr)[u], e1 = (*list_ptr)[u + 1];
        (*list_ptr)[u] = w; /* w <= e0: entry u + 1 is still the old bound when user u + 1 reads it */
        auto at = subset.begin();
        for (uint64_t e = e0; e < e1; ++e) {
            at = std::lower_bound(at, subset.end(), (*list_items)[e]);
            if (at == subset.end()) break;
            if (*at == (*list_items)[e]) (*list_items)[w++] = (uint32_t)(at - subset.begin());
        }
    }
    if (!list_ptr->empty()) list_ptr->back() = w;
    list_items->resize(w);
}

/* recommend_diverse's selection behind a scan: k_out of the scan's k (the pool) per user, by greedy maximal marginal relevance */
struct Diverse {
    uint32_t k_out;
    float trade_off;
    uint32_t metric;
};

/* recommend_capped's rule behind a scan: the first k_out entries of the scan's k (the pool) per user of which no item group holds
 * more than cap; out_complete (host, one byte per user of the call) nullable */
struct Capped {
    uint32_t k_out, cap;
    uint8_t* out_complete;
};

/* the tag filter of a *_filtered call: the caller's masks, one pair per user of the call (a null array: all zeros) */
struct TagFilterArg {
    const uint32_t *any_of, *none_of;
};

/* recommend_sampled's noise on a scan (not with item rows, a subset or a selection): inv_t = 1.0f / temperature, checked by
 * sample_args; streams: one per user of the call, or null — then user u's is fallback[u] (a session call's slots), or u itself
 * where that is null too; out_keys (host, num_users x k) nullable */
struct Sample {
    float inv_t;
    uint64_t seed;
    const uint64_t* streams;
    const uint32_t* fallback;
    float* out_keys;
};

/* the noise of a *_sampled call out of its arguments: false for a temperature that is not finite and positive, or whose
 * reciprocal is not finite and non-zero in f32 */
bool sample_args(const sbr_sample_args* a, float* out_keys, Sample* out) {
    if (!a || !(a->temperature > 0.0f) || !std::isfinite(a->temperature)) return false;
    const float inv_t = 1.0f / a->temperature;
    if (!std::isfinite(inv_t) || inv_t == 0.0f) return false;
    *out = Sample{inv_t, a->seed, a->streams, nullptr, out_keys};
    return true;
}

/* the nullable mask pair of a *_sampled call: both null is no filter */
const TagFilterArg* sample_filter(const uint32_t* any_of, const uint32_t* none_of, TagFilterArg* hold) {
    if (!any_of && !none_of) return nullptr;
    *hold = TagFilterArg{any_of, none_of};
    return hold;
}

/* device buffers of launch_recommend_sampled beside TopkBufs over nu users */
struct SampleBufs {
    uint64_t *keys, *streams;
    uint32_t *pair_row, *pair_item;
    float* plain;
    void carve(DeviceArena& ar, size_t nu, uint32_t k) {
        keys = ar.take<uint64_t>(nu);
        streams = ar.take<uint64_t>(nu);
        pair_row = ar.take<uint32_t>(nu * k);
        pair_item = ar.take<uint32_t>(nu * k);
        plain = ar.take<float>(nu * k);
    }
};

/* log_partition on a scan at k = 1 (not with item rows, a subset, a selection or noise): inv_t = 1.0f / temperature, checked by
 * partition_args; out_shift / out_mass: host, one per user of the call — the call has no item or score rows */
struct Partition {
    float inv_t;
    float* out_shift;
    uint64_t* out_mass;
    uint32_t* out_frac_bits; /* scan_call writes the model's F here after success */
};

/* the arguments the *_log_partition calls share: false for a temperature sample_args refuses or an output that is missing */
bool partition_args(float temperature, uint64_t n, float* out_shift, uint64_t* out_mass, uint32_t* out_frac_bits, Partition* out) {
    const sbr_sample_args a{temperature, 0, nullptr};
    Sample sm;
    if (!sample_args(&a, nullptr, &sm) || !out_frac_bits || (n && (!out_shift || !out_mass))) return false;
    *out = Partition{sm.inv_t, out_shift, out_mass, out_frac_bits};
    return true;
}

}  // namespace
}  // extern "C"

/* An item set (ITEM SETS in include/sbr_hip.h): the sorted, unique ids S and a persistent device copy of their rows, E'[j] = E[S[j]]
 * and b'[j] = b[S[j]] at storage width, gathered by subset_gather_kernel at creation and by every refresh — plain device memory, not
 * the arena, so no launch gathers it again.  Bound to the model's parameter generation as a session store is.  Tags and groups are
 * not cached: they have no generation, and every launch gathers the set's words into the arena. */
struct sbr_item_set {
    sbr_model* m = nullptr;
    uint64_t gen = 0;           /* the model's param_gen the rows were gathered under */
    std::vector<uint32_t> ids;  /* S */
    uint32_t* d_ids = nullptr;  /* all three null for an empty set */
    float *E = nullptr, *b = nullptr;
};

namespace {

/* device blocks of one call or chunk outside the eval arena (which does not outlive a carve); given back once the stream is idle */
struct DeviceBlocks {
    hipStream_t stream;
    std::vector<void*> blocks;
    explicit DeviceBlocks(hipStream_t s) : stream(s) {}
    DeviceBlocks(const DeviceBlocks&) = delete;
    DeviceBlocks& operator=(const DeviceBlocks&) = delete;
    template <typename T>
    sbr_status take(T** p, size_t count) {
        SBRCHK(dmalloc(p, count ? count : 1));
        blocks.push_back(*p);
        return SBR_OK;
    }
    ~DeviceBlocks() {
        if (blocks.empty()) return;
        (void)hipStreamSynchronize(stream);
        for (void* b : blocks) dfree(b);
    }
};

}  // namespace

extern "C" {
namespace {

/* The threshold form of a scan (recommend_above / audience_above; not with item rows, a subset, a selection, noise or a partition):
 * every scanned column whose score is >= thresholds[row], as CSR.  out_counts [rows of the call] always; the pairs go to out_ids /
 * out_scores (host, `capacity` entries; out_ids null: counts only, out_scores alone may be null) in row order while the running
 * total fits the capacity — once it does not, the remaining chunks are counted only.  total: the pairs counted so far.
 * The budget form (recommend_top / audience_top) is the same descriptor with n in place of thresholds: the first min(n[row],
 * eligible) columns of each row in the total order, out_counts that number and out_cuts [rows] the rows' cuts; the capacity is
 * held against the sum of those counts, whatever the scores tied at the cuts take on the device. */
struct Above {
    const float* thresholds;
    uint64_t* out_counts;
    uint64_t capacity;
    uint32_t* out_ids;
    float* out_scores;
    uint64_t total;
    uint64_t* out_total;         /* scan_call writes `total` here after success (the audience calls do that themselves) */
    const uint64_t* n = nullptr; /* the budget form: thresholds is null */
    float* out_cuts = nullptr;
};

/* the output arguments the *_above calls share: false for a missing array, scores without ids, or a NaN threshold */
bool above_args(const float* thresholds, uint64_t n, uint64_t* out_counts, uint64_t* out_total, uint64_t capacity, uint32_t* out_ids,
                float* out_scores, Above* out) {
    if (!out_total || (n && (!thresholds || !out_counts)) || (out_scores && !out_ids)) return false;
    for (uint64_t i = 0; i < n; ++i)
        if (std::isnan(thresholds[i])) return false;
    *out = Above{thresholds, out_counts, capacity, out_ids, out_scores, 0, out_total};
    return true;
}

/* the same for the *_top calls: n (any value) where the thresholds stand, and the cuts */
bool top_args(const uint64_t* n, uint64_t rows, float* out_cuts, uint64_t* out_counts, uint64_t* out_total, uint64_t capacity, uint32_t* out_ids,
              float* out_scores, Above* out) {
    if (!out_total || (rows && (!n || !out_counts || !out_cuts)) || (out_scores && !out_ids)) return false;
    *out = Above{nullptr, out_counts, capacity, out_ids, out_scores, 0, out_total, n, out_cuts};
    return true;
}

/* a fill launch's share of the device output: 256 MB of (id, score) entries, the bound the top-k lists are kept to.
 * SBR_ABOVE_FILL_BYTES=n (n >= 1) is a TEST HOOK read per call that replaces it (small tests run several fill ranges). */
size_t above_fill_entries() {
    size_t bytes = (size_t)256 << 20;
    if (const char* e = std::getenv("SBR_ABOVE_FILL_BYTES")) {
        const long long n = std::atoll(e);
        if (n >= 1) bytes = (size_t)n;
    }
    const size_t entries = bytes / 8;
    return entries < 1 ? 1 : entries > 0xFFFFFFFFull ? 0xFFFFFFFFull : entries; /* a fill launch addresses its entries with 32 bits */
}

/* device buffers of launch_above_count / launch_above_fill over nu rows beside the scan's own (rep_row, the exclusion CSR, masks) */
struct AboveBufs {
    float* th;
    uint32_t *counts, *totals, *over;
    uint64_t* offsets;
    uint32_t groups = 0, per = 0;
    sbr::TopSelect ts{}; /* top: the select's per-row search state; its cuts are th */
    void carve(DeviceArena& ar, uint32_t num_items, size_t nu, bool top) {
        groups = sbr::above_groups((uint32_t)nu, num_items, &per);
        th = ar.take<float>(nu);
        counts = ar.take<uint32_t>(nu * groups);
        offsets = ar.take<uint64_t>(nu * groups + 1);
        totals = ar.take<uint32_t>(nu);
        over = ar.take<uint32_t>(1);
        if (!top) return;
        ts.cuts = th;
        ts.n = ts.wanted = ar.take<uint64_t>(nu); /* the step kernel's start reads n[r] and writes wanted[r]: one array serves */
        ts.out_off = ar.take<uint64_t>(nu + 1);
        ts.prefix = ar.take<uint32_t>(nu); ts.mask = ar.take<uint32_t>(nu);
        ts.hist = ar.take<uint32_t>(nu * 16);
        ts.gt = ar.take<uint32_t>(nu); ts.final_counts = ar.take<uint32_t>(nu); ts.keep_eq = ar.take<uint32_t>(nu);
        ts.out_tot = ar.take<uint32_t>(nu);
    }
};

/* One chunk of a threshold scan: rows [row0, row0 + as.n) of the call.  The count scan (behind `prelaunch`, which builds what the
 * scan reads and returns its launches), the rows' totals read back — as.n x 4 bytes — and, while the call's running total fits the
 * capacity, the fill over consecutive row ranges of the chunk whose entries fit above_fill_entries() (at least one row each), every
 * range copied to the host at its running offset.  cat / A / qb: launch_above_count's; row_ids non-null (audience with named ids):
 * what the written positions stand for.  as.thresholds is uploaded here.
 * The budget form (ab->n; ts: the chunk's select state): the select runs first, behind `prelaunch`, and leaves the cuts in
 * as.thresholds; the cuts and the final counts are read back (as.n x 8 bytes) and are all a call without pair outputs runs.  With
 * pairs the count scan follows at the cuts — its totals hold every score tied at a cut and size the fill — and every fill range is
 * trimmed on the device to its rows' final counts before it is copied out. */
sbr_status above_chunk(sbr_model* m, const sbr::ModelView& cat, const float* A, const float* qb, const sbr::AboveScan& as, const sbr::TopSelect& ts,
                       const uint32_t* row_ids, uint64_t row0, Above* ab, const std::function<int()>& prelaunch) {
    const size_t nu = as.n;
    const bool top = ab->n != nullptr;
    std::vector<uint32_t> totals(nu, 0), finals;
    if (top) {
        finals.assign(nu, 0);
        HIPCHK(hipMemcpyAsync(ts.wanted, ab->n + row0, nu * 8, hipMemcpyHostToDevice, m->stream));
        SBRCHK(scan_launch(m, as.nonfinite_flag, [&] { return prelaunch() + sbr::launch_top_select(cat, A, qb, as, ts, m->stream); },
                           {{finals.data(), ts.final_counts, nu * 4}, {ab->out_cuts + row0, ts.cuts, nu * 4}}));
    } else {
        HIPCHK(hipMemcpyAsync(const_cast<float*>(as.thresholds), ab->thresholds + row0, nu * 4, hipMemcpyHostToDevice, m->stream));
        SBRCHK(scan_launch(m, as.nonfinite_flag, [&] { return prelaunch() + sbr::launch_above_count(cat, A, qb, as, m->stream); },
                           {{totals.data(), as.totals, nu * 4}}));
    }
    const std::vector<uint32_t>& leaving = top ? finals : totals; /* the entries of each row that reach the caller */
    uint64_t chunk_total = 0;
    for (size_t i = 0; i < nu; ++i) {
        ab->out_counts[row0 + i] = leaving[i];
        chunk_total += leaving[i];
    }
    uint64_t at = ab->total; /* the chunk's first entry in the caller's arrays */
    ab->total += chunk_total;
    if (!ab->out_ids || ab->total > ab->capacity || chunk_total == 0) return SBR_OK;
    if (top) /* what the fill writes: the rows' scores at or over their cuts */
        SBRCHK(scan_launch(m, as.nonfinite_flag, [&] { return sbr::launch_above_count(cat, A, qb, as, m->stream); },
                           {{totals.data(), as.totals, nu * 4}}));
    const size_t budget = above_fill_entries();
    size_t largest = 0; /* entries of the largest range: one device block serves them all */
    for (size_t r0 = 0; r0 < nu;) {
        size_t r1 = r0 + 1, n = totals[r0];
        while (r1 < nu && n + totals[r1] <= budget) n += totals[r1++];
        largest = std::max(largest, n);
        r0 = r1;
    }
    DeviceBlocks out(m->stream);
    uint32_t *d_ids = nullptr, *t_ids = nullptr;   /* t_*: the trimmed entries of a range, at most as many as the fill wrote */
    float *d_scores = nullptr, *t_scores = nullptr;
    SBRCHK(out.take(&d_ids, largest));
    if (ab->out_scores || top) SBRCHK(out.take(&d_scores, largest)); /* the trim compares the scores */
    if (top) {
        SBRCHK(out.take(&t_ids, largest));
        if (ab->out_scores) SBRCHK(out.take(&t_scores, largest));
    }
    HIPCHK(hipMemsetAsync(as.overrun_flag, 0, 4, m->stream));
    for (size_t r0 = 0; r0 < nu;) {
        size_t r1 = r0 + 1, n = totals[r0];
        while (r1 < nu && n + totals[r1] <= budget) n += totals[r1++];
        if (n) {
            uint32_t over = 0;
            size_t keep = n; /* the entries that leave */
            if (top) {
                keep = 0;
                for (size_t i = r0; i < r1; ++i) keep += finals[i];
            }
            uint32_t* ids = top ? t_ids : d_ids;
            float* scores = top ? t_scores : d_scores;
            SBRCHK(scan_launch(m, as.nonfinite_flag, [&] {
                int l = sbr::launch_above_fill(cat, A, qb, as, (uint32_t)r0, (uint32_t)(r1 - r0), d_ids, d_scores, (uint32_t)n, m->stream);
                if (top)
                    l += sbr::launch_top_trim(as, ts, (uint32_t)r0, (uint32_t)(r1 - r0), d_ids, d_scores, (uint32_t)n, t_ids, t_scores, (uint32_t)keep,
                                              m->stream);
                return l + (row_ids ? sbr::launch_above_ids(row_ids, ids, keep, m->stream) : 0);
            }, {{&over, as.overrun_flag, 4}, {ab->out_ids + at, ids, keep * 4}, {ab->out_scores ? ab->out_scores + at : nullptr, scores, keep * 4}}));
            if (over) return SBR_ERR_HIP; /* the fill passed what the count did not: nothing was written out of bounds */
            at += keep;
        }
        r0 = r1;
    }
    return SBR_OK;
}

/* The ranks form of a scan (rank_targets under a filter, through a set or on a store; k == 1, not with item rows, a subset, a
 * selection, noise, a partition or a threshold): no top-k scan runs — the rows' targets [target_ptr[u], target_ptr[u + 1]) of
 * target_items (catalogue ids) are ranked among what the row may see, into out_ranks in target order (ELIGIBLE RANKS in sbr_hip.h). */
struct Ranks {
    const uint64_t* target_ptr;
    const uint32_t* target_items;
    uint32_t* out_ranks;
};

/* device buffers of launch_rank_eligible over ns scan-users with nt targets, beside the scan's own (the exclusion CSR, masks, flag) */
struct RanksBufs {
    int* rep;
    uint32_t *lu, *sptr, *tgt, *pos, *ranks, *buckets, *totals;
    float *ts, *th, *tmin, *tmin2;
    void carve(DeviceArena& ar, size_t ns, size_t nt, uint32_t tmax) {
        rep = ar.take<int>(ns);
        lu = ar.take<uint32_t>(ns);
        sptr = ar.take<uint32_t>(ns + 1);
        tgt = ar.take<uint32_t>(nt + 1);
        ts = ar.take<float>(nt + 1);
        pos = ar.take<uint32_t>(nt + 1);
        ranks = ar.take<uint32_t>(nt + 1);
        th = ar.take<float>(ns * tmax);
        buckets = ar.take<uint32_t>(ns * tmax);
        tmin = ar.take<float>(ns);
        tmin2 = ar.take<float>(ns);
        totals = ar.take<uint32_t>(ns);
    }
};

/* which variant of the top-k scan a call asks for; the default is plain recommend */
struct ScanVariant {
    const Ranks* rk = nullptr;
    bool cosine = false;                            /* item rows: rank by cosine, not by the plain dot product */
    const std::vector<uint32_t>* subset = nullptr;  /* recommend_among's item set */
    const Diverse* dv = nullptr;
    const TagFilterArg* flt = nullptr; /* through scan_call, null: the rows' own masks, a filter unless both are null */
    Sample* sm = nullptr;             /* the caller's own: scan_call sets a store's fallback streams in it */
    const Partition* pt = nullptr;
    Above* ab = nullptr;
    const Capped* cp = nullptr;
    const sbr_item_set* set = nullptr; /* the scan runs over the set's resident sub-table; not with item rows or a subset */
};

/* What the scans of (m, set) read and are carved for: the catalogue (set null), or the set's resident sub-table, whose item j is
 * S[j].  An empty set has no table: no scan runs (`none`), and buffers are carved as for one item. */
struct SetView {
    sbr::ModelView cat;
    uint32_t ns = 0;      /* the set's items; 0 without a set */
    uint32_t scanned;     /* the items the scan's buffers are carved for */
    bool none = false;    /* an empty set: nothing to scan */
    SetView(const sbr_model* m, const sbr_item_set* set) : cat(m->mv), scanned((uint32_t)m->hp.num_items) {
        if (!set) return;
        ns = (uint32_t)set->ids.size();
        scanned = std::max(ns, 1u);
        none = ns == 0;
        if (none) return;
        cat.E = set->E;
        cat.b = set->b;
        cat.num_items = ns;
    }
};

/* The tag masks of a chunk's nu rows, each `rep` times over (beam search: once per beam), to d_any / d_none: row i's are the call's
 * row users[i], or c0 + i where users is null.  *host holds the words (any_of, then none_of) until the stream is drained. */
sbr_status upload_masks(sbr_model* m, const TagFilterArg& flt, const uint64_t* users, size_t c0, size_t nu, size_t rep, uint32_t* d_any,
                        uint32_t* d_none, std::vector<uint32_t>* host) {
    const size_t nb = nu * rep;
    host->assign(2 * nb, 0u);
    for (size_t i = 0; i < nb; ++i) {
        const uint64_t u = users ? users[i / rep] : c0 + i / rep;
        if (flt.any_of) (*host)[i] = flt.any_of[u];
        if (flt.none_of) (*host)[nb + i] = flt.none_of[u];
    }
    HIPCHK(hipMemcpyAsync(d_any, host->data(), nb * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(d_none, host->data() + nb, nb * 4, hipMemcpyHostToDevice, m->stream));
    return SBR_OK;
}

/* a chunk cap's TEST HOOK: NAME=n (n >= 1) in the environment, read per call, stands in for `cap` */
size_t chunk_override(const char* name, size_t cap) {
    const char* e = std::getenv(name);
    const long long v = e ? std::atoll(e) : 0;
    return v >= 1 ? (size_t)v : cap;
}

/* top-k of every user of `s`, in chunks; results to out_items / out_scores (host, num_users x k; scores optional).  With item rows
 * (similar_items: the users are the queries) the launch makes the rows itself and ranks by cosine (v.cosine), or by the plain dot
 * product.
 * With v.subset (recommend_among: sorted, unique, not empty) only its items are scanned, as a sub-table every launch gathers.
 * With v.dv (recommend_diverse; not with item rows or a subset) the scan's rows are the users' pools: the same launch selects
 * dv->k_out of each, and the results are num_users x dv->k_out.
 * With v.flt (not with a subset) the scan offers user u only the items its masks allow against the model's item tags, which must be
 * set; the masks go with the call's user u through the chunks, whatever row of H holds its representation.
 * With s.seen (a session store's memory; not with a subset) the exclusion CSR is made on the device: user i of a chunk has the
 * segment [i w + c_i, (i + 1) w + c_(i + 1)), c = the chunk's caller-list pointers — known to the host without any device-side
 * count — which session_seen_lists_kernel fills, ahead of the scan, with the merge of the slot's memory and the caller's list.
 * With v.sm (recommend_sampled; not with item rows, a subset or v.dv) the scan orders by the noisy keys: out_scores receives the
 * plain scores of the drawn items and v.sm->out_keys the keys; the streams go with the call's user u through the chunks.
 * With v.pt (log_partition; k == 1, not with item rows, a subset, v.dv or v.sm) the scan finds the rows' shifts and a second scan
 * sums the softmax weights: out_items / out_scores are unused (null) and the results are v.pt->out_shift / out_mass.
 * With v.ab (recommend_above; k == 1, not with item rows, a subset, v.dv, v.sm or v.pt) no top-k scan runs: every chunk is
 * above_chunk's count and fill over the same representations, exclusion CSR and masks; out_items / out_scores are unused (null).
 * With v.cp (recommend_capped; the model's item groups set; not with item rows, a subset, v.dv, v.sm, v.pt or v.ab) the scan's rows
 * are the users' pools: the same launch keeps v.cp->k_out of each under the group cap, the results are num_users x v.cp->k_out and
 * v.cp->out_complete the rows' flags.
 * With v.rk (the ranks form; k == 1, not with item rows, a subset, v.dv, v.sm, v.pt, v.ab or v.cp) no top-k scan runs: the chunks
 * are runs of scan-users — a row's targets, at most rank_targets_tmax at a time — over the same representations, exclusion CSR,
 * masks and set, ranked by launch_rank_eligible; out_items / out_scores are unused (null).
 * With v.set (an item set, current; not with item rows or v.subset) every form above scans the set's resident sub-table where it
 * scans the catalogue: the exclusion CSR — uploaded, or made by session_seen_lists_kernel — is turned into positions of the set on
 * the device (subset_positions_kernel), the tag and group words of the set are gathered into the arena per launch, the noise is
 * hashed from the catalogue ids, F is the model's, and what leaves is catalogue ids.  An empty set answers on the host as a row that
 * may see nothing. */
sbr_status recommend_scan(sbr_model* m, const RepSource& s, uint64_t num_users, uint32_t k, uint32_t* out_items, float* out_scores,
                          const ScanVariant& v = ScanVariant()) {
    const Diverse* dv = v.dv;
    if (v.flt && (!m->item_tags || v.subset)) return SBR_ERR_INVALID_ARGUMENT;
    if (s.seen && v.subset) return SBR_ERR_INVALID_ARGUMENT;
    const Sample* sm = v.sm;
    if (sm && (s.item_rows || v.subset || dv)) return SBR_ERR_INVALID_ARGUMENT;
    const Partition* pt = v.pt;
    if (pt && (s.item_rows || v.subset || dv || sm || k != 1)) return SBR_ERR_INVALID_ARGUMENT;
    Above* ab = v.ab;
    if (ab && (s.item_rows || v.subset || dv || sm || pt || k != 1)) return SBR_ERR_INVALID_ARGUMENT;
    const Capped* cp = v.cp;
    if (cp && (!m->item_groups || s.item_rows || v.subset || dv || sm || pt || ab)) return SBR_ERR_INVALID_ARGUMENT;
    const Ranks* rk = v.rk;
    if (rk && (s.item_rows || v.subset || dv || sm || pt || ab || cp || k != 1)) return SBR_ERR_INVALID_ARGUMENT;
    const sbr_item_set* set = v.set;
    if (set && (s.item_rows || v.subset)) return SBR_ERR_INVALID_ARGUMENT;
    /* rk: the targets validated, and each row's cut into scan-users as rank_targets_scan cuts them — runs of at most tmax, in row
     * and target order, sharing the row's representation, list and masks */
    const uint32_t tmax = sbr::rank_targets_tmax(m->d);
    std::vector<uint64_t> su_user, su_begin; /* the row of scan-user i; its first target, an index into target_items */
    if (rk) {
        if (!rk->target_ptr) return SBR_ERR_INVALID_ARGUMENT;
        SBRCHK(check_csr(m, rk->target_ptr, num_users, rk->target_items, false));
        if (rk->target_ptr[num_users] - rk->target_ptr[0] && !rk->out_ranks) return SBR_ERR_INVALID_ARGUMENT;
        for (uint64_t u = 0; u < num_users; ++u)
            for (uint64_t e = rk->target_ptr[u]; e < rk->target_ptr[u + 1]; e += tmax) {
                su_user.push_back(u);
                su_begin.push_back(e);
            }
    }
    if (set && set->ids.empty()) { /* nothing to scan: every row is one that may see nothing */
        if (rk) { /* every target lies outside the set */
            const uint64_t nt = rk->target_ptr[num_users] - rk->target_ptr[0];
            if (nt) std::fill(rk->out_ranks, rk->out_ranks + nt, (uint32_t)m->hp.num_items);
            return SBR_OK;
        }
        const size_t ko = dv ? dv->k_out : cp ? cp->k_out : k;
        if (out_items) std::fill(out_items, out_items + num_users * ko, 0xFFFFFFFFu);
        if (out_scores) std::fill(out_scores, out_scores + num_users * ko, -INFINITY);
        if (sm && sm->out_keys) std::fill(sm->out_keys, sm->out_keys + num_users * ko, -INFINITY);
        if (cp && cp->out_complete) std::fill(cp->out_complete, cp->out_complete + num_users, (uint8_t)1); /* the pool held every eligible item */
        for (uint64_t u = 0; u < num_users; ++u) {
            if (pt) { pt->out_shift[u] = -INFINITY; pt->out_mass[u] = 0; }
            if (ab) {
                ab->out_counts[u] = 0;
                if (ab->n) ab->out_cuts[u] = ab->n[u] ? -INFINITY : INFINITY;
            }
        }
        return SBR_OK;
    }
    const size_t seen_w = s.seen ? s.seen->w : 0;
    std::vector<uint64_t> users(num_users);
    for (uint64_t u = 0; u < num_users; ++u) users[u] = u;
    const SetView sv(m, set);
    const sbr::ModelView& cat = sv.cat; /* what the launches scan */
    const uint32_t scanned_items = v.subset ? (uint32_t)v.subset->size() : sv.scanned;
    const size_t cap = recommend_users_cap(scanned_items, k);
    for (Chunk ch; next_chunk(rk ? su_user : users, rk ? eval_units_cap : cap, s, m->hp.max_sequence_length, &ch);) {
        const size_t nu = ch.users.size(); /* rk: the chunk's distinct rows; its units are the scan-users [ch.c0, ch.c1) */
        UserReps ur; /* its lists: what is excluded (list_ptr empty: nothing) */
        TopkBufs tb;
        RanksBufs rb{};
        const size_t rk_ns = rk ? ch.c1 - ch.c0 : 0;
        const uint64_t rk_t0 = rk ? su_begin[ch.c0] : 0; /* the chunk's targets are contiguous in target_items: [rk_t0, rk_t0 + rk_nt) */
        const size_t rk_nt = rk ? (size_t)(std::min(su_begin[ch.c1 - 1] + tmax, rk->target_ptr[su_user[ch.c1 - 1] + 1]) - rk_t0) : 0;
        SubsetBufs sb;
        SampleBufs smb{};
        float* rnorm = nullptr; /* item rows: the catalogue's reciprocal norms, once per chunk (the arena does not outlive a carve) */
        uint32_t* dv_items = nullptr; /* dv: the selection's rows, nu x dv->k_out */
        float* dv_scores = nullptr;
        uint8_t* cp_complete = nullptr; /* cp: the rows' flags; the kept rows are dv_items / dv_scores, nu x cp->k_out */
        uint32_t *seen_slot = nullptr, *seen_caller = nullptr; /* s.seen: the chunk's slots and caller lists, the build kernel's inputs */
        float* pt_shift = nullptr; /* pt: the rows' shifts and masses */
        unsigned long long* pt_mass = nullptr;
        AboveBufs abufs{};
        uint32_t *set_tags = nullptr, *set_groups = nullptr; /* set: its tag / group words, gathered by this launch */
        SBRCHK(user_reps(m, s, ch.users, [&](DeviceArena& ar) {
            tb.carve(ar, scanned_items, nu, nu * seen_w + ur.b.list_items.size(), k, v.flt != nullptr);
            if (set && v.flt) set_tags = ar.take<uint32_t>(scanned_items);
            if (set && cp) set_groups = ar.take<uint32_t>(scanned_items);
            if (s.seen) {
                seen_slot = ar.take<uint32_t>(nu);
                seen_caller = ar.take<uint32_t>(ur.b.list_items.size() + 1);
            }
            if (s.item_rows) rnorm = ar.take<float>(m->hp.num_items);
            if (v.subset) sb.carve(ar, v.subset->size(), (size_t)m->d);
            if (sm) smb.carve(ar, nu, k);
            if (ab) abufs.carve(ar, scanned_items, nu, ab->n != nullptr);
            if (rk) rb.carve(ar, rk_ns, rk_nt, tmax);
            if (pt) {
                pt_mass = ar.take<unsigned long long>(nu);
                pt_shift = ar.take<float>(nu);
            }
            if (dv) {
                dv_items = ar.take<uint32_t>(nu * dv->k_out);
                dv_scores = ar.take<float>(nu * dv->k_out);
            }
            if (cp) {
                dv_items = ar.take<uint32_t>(nu * cp->k_out);
                dv_scores = ar.take<float>(nu * cp->k_out);
                cp_complete = ar.take<uint8_t>(nu);
            }
        }, &ur));
        const bool excl = !ur.b.list_ptr.empty() || s.seen;
        std::vector<uint64_t> seen_eptr; /* s.seen: the segments' bounds and the chunk's slots, read by asynchronous copies */
        std::vector<uint32_t> seen_slots;
        if (v.subset) {
            if (excl) lists_to_subset_positions(*v.subset, &ur.b.list_ptr, &ur.b.list_items);
            HIPCHK(hipMemcpyAsync(sb.ids, v.subset->data(), v.subset->size() * 4, hipMemcpyHostToDevice, m->stream));
        }
        HIPCHK(hipMemcpyAsync(tb.rep, ur.rep_row.data(), nu * 4, hipMemcpyHostToDevice, m->stream));
        if (s.seen) {
            seen_eptr.resize(nu + 1);
            seen_slots.resize(nu);
            for (size_t i = 0; i <= nu; ++i) seen_eptr[i] = i * seen_w + (ur.b.list_ptr.empty() ? 0 : ur.b.list_ptr[i]);
            for (size_t i = 0; i < nu; ++i) seen_slots[i] = s.seen_slots[ch.users[i]]; /* the call's index, not the chunk's */
            HIPCHK(hipMemcpyAsync(seen_slot, seen_slots.data(), nu * 4, hipMemcpyHostToDevice, m->stream));
            SBRCHK(upload_csr(m, tb.eptr, seen_eptr, seen_caller, ur.b.list_items));
        } else if (excl)
            SBRCHK(upload_csr(m, tb.eptr, ur.b.list_ptr, tb.excl, ur.b.list_items));
        std::vector<uint32_t> masks; /* the chunk's users' any_of, then their none_of */
        if (v.flt) SBRCHK(upload_masks(m, *v.flt, ch.users.data(), 0, nu, 1, tb.any_of, tb.none_of, &masks));
        std::vector<uint64_t> streams; /* the chunk's users' streams */
        if (sm) {
            streams.resize(nu);
            for (size_t i = 0; i < nu; ++i) {
                const uint64_t u = ch.users[i]; /* the call's index, not the chunk's */
                streams[i] = sm->streams ? sm->streams[u] : sm->fallback ? (uint64_t)sm->fallback[u] : u;
            }
            HIPCHK(hipMemcpyAsync(smb.streams, streams.data(), nu * 8, hipMemcpyHostToDevice, m->stream));
        }
        const uint32_t* tags = !v.flt ? nullptr : set ? set_tags : m->item_tags;
        /* what every form runs ahead of its scan: the seen lists, and for a set the lists as positions and its words */
        auto prelaunch = [&]() -> int {
            int n = s.seen ? sbr::launch_session_seen_lists(*s.seen, seen_slot, (int)nu, tb.eptr, seen_caller, tb.excl, m->stream) : 0;
            if (!set) return n;
            if (excl) n += sbr::launch_subset_positions(set->d_ids, scanned_items, tb.eptr, (uint32_t)nu, tb.excl, m->stream);
            if (v.flt) n += sbr::launch_subset_words(set->d_ids, scanned_items, m->item_tags, set_tags, m->stream);
            if (cp) n += sbr::launch_subset_words(set->d_ids, scanned_items, m->item_groups, set_groups, m->stream);
            return n;
        };
        if (rk) {
            std::vector<int> srep(rk_ns);
            std::vector<uint32_t> sptr(rk_ns + 1);
            for (size_t i = 0; i < rk_ns; ++i) {
                srep[i] = ur.rep_row[ch.lu[i]];
                sptr[i] = (uint32_t)(su_begin[ch.c0 + i] - rk_t0);
            }
            sptr[rk_ns] = (uint32_t)rk_nt;
            HIPCHK(hipMemcpyAsync(rb.rep, srep.data(), rk_ns * 4, hipMemcpyHostToDevice, m->stream));
            HIPCHK(hipMemcpyAsync(rb.lu, ch.lu.data(), rk_ns * 4, hipMemcpyHostToDevice, m->stream));
            HIPCHK(hipMemcpyAsync(rb.sptr, sptr.data(), (rk_ns + 1) * 4, hipMemcpyHostToDevice, m->stream));
            HIPCHK(hipMemcpyAsync(rb.tgt, rk->target_items + rk_t0, rk_nt * 4, hipMemcpyHostToDevice, m->stream));
            SBRCHK(scan_launch(m, tb.flag, [&] {
                /* without masks, a set or a store's memory the lists are the host's sorted, de-duplicated ones: the plain call's launch */
                if (!tags && !set && !s.seen)
                    return sbr::launch_rank_targets(m->mv, ur.H, rb.rep, rb.lu, rb.sptr, (uint32_t)rk_ns, rb.tgt, excl ? tb.eptr : nullptr, tb.excl,
                                                    rb.ts, rb.pos, rb.th, rb.tmin, rb.tmin2, rb.buckets, rb.totals, rb.ranks, tb.flag, m->stream);
                sbr::RankEligible re{};
                re.rep_row = rb.rep; re.su_user = rb.lu; re.sptr = rb.sptr; re.num_su = (uint32_t)rk_ns; re.tgt_items = rb.tgt;
                re.list_ptr = excl ? tb.eptr : nullptr; re.list_items = tb.excl;
                re.f = sbr::TagMasks{tags, tb.any_of, tb.none_of};
                re.set_ids = set ? set->d_ids : nullptr;
                re.num_items = (uint32_t)m->hp.num_items;
                re.ts = rb.ts; re.pos = rb.pos; re.th = rb.th; re.tmin = rb.tmin; re.tmin2 = rb.tmin2;
                re.buckets = rb.buckets; re.totals = rb.totals; re.ranks = rb.ranks; re.nonfinite_flag = tb.flag;
                return prelaunch() + sbr::launch_rank_eligible(cat, ur.H, re, m->stream);
            }, {{rk->out_ranks + (rk_t0 - rk->target_ptr[0]), rb.ranks, rk_nt * 4}}));
            continue;
        }
        if (ab) { /* the chunk's rows are the call's [ch.c0, ch.c1): every user is one unit */
            sbr::AboveScan as{};
            as.rep_row = tb.rep; as.n = (uint32_t)nu; as.thresholds = abufs.th;
            as.excl_ptr = excl ? tb.eptr : nullptr; as.excl_items = tb.excl;
            as.f = sbr::TagMasks{tags, tb.any_of, tb.none_of};
            as.groups = abufs.groups; as.per = abufs.per;
            as.counts = abufs.counts; as.offsets = abufs.offsets; as.totals = abufs.totals;
            as.nonfinite_flag = tb.flag; as.overrun_flag = abufs.over;
            SBRCHK(above_chunk(m, cat, ur.H, nullptr, as, abufs.ts, set ? set->d_ids : nullptr, ch.c0, ab, prelaunch));
            continue;
        }
        const size_t ko = dv ? dv->k_out : cp ? cp->k_out : k; /* the width of the rows that leave */
        /* the selection reads the pool's scores whether or not the caller wants any; a sampled scan's are its keys */
        sbr::TopkScan sc = tb.scan(nu, k, excl, out_scores || dv || sm || pt, tags);
        if (sm) sc.g = sbr::SampleNoise{sm->inv_t, smb.keys};
        SBRCHK(scan_launch(m, tb.flag, [&] {
            int n = prelaunch();
            /* a set's mass is held to the model's F, and its noise to the catalogue ids, which also leave in the positions' place */
            if (pt)
                n += sbr::launch_log_partition(cat, ur.H, sc, sbr::PartitionScan{pt->inv_t, pt_shift, pt_mass, set ? (uint32_t)m->hp.num_items : 0u},
                                               m->stream);
            else if (sm)
                n += sbr::launch_recommend_sampled(cat, ur.H, sc, sbr::SampleScan{sm->seed, smb.streams, smb.pair_row, smb.pair_item, smb.plain,
                                                                                  set ? set->d_ids : nullptr}, m->stream);
            else if (set) n += sbr::launch_recommend(cat, ur.H, sc, m->stream);
            else if (v.subset) n += sbr::launch_recommend_among(m->mv, sb.ids, scanned_items, sb.E, sb.b, ur.H, sc, m->stream);
            else if (s.item_rows) n += sbr::launch_similar_items(m->mv, ur.d_item_rows, v.cosine, rnorm, ur.H, sc, m->stream);
            else n += sbr::launch_recommend(m->mv, ur.H, sc, m->stream);
            if (dv)
                n += sbr::launch_diverse_select(cat, tb.items, tb.scores, (uint32_t)nu, k, dv->k_out, dv->trade_off, dv->metric == SBR_SIMILAR_COSINE,
                                                dv_items, out_scores ? dv_scores : nullptr, tb.flag, m->stream);
            if (cp)
                n += sbr::launch_capped_select(set ? set_groups : m->item_groups, scanned_items, tb.items, sc.out_scores, (uint32_t)nu, k,
                                               cp->k_out, cp->cap, dv_items, out_scores ? dv_scores : nullptr, cp_complete, m->stream);
            /* the selections ran on positions against the sub-table and the gathered words; the rows that leave become ids */
            if (set && !pt && !sm) n += sbr::launch_above_ids(set->d_ids, dv || cp ? dv_items : tb.items, nu * ko, m->stream);
            return n;
        }, {{out_items ? out_items + ch.c0 * ko : nullptr, dv || cp ? dv_items : tb.items, nu * ko * 4},
            {cp && cp->out_complete ? cp->out_complete + ch.c0 : nullptr, cp_complete, nu},
            {pt ? pt->out_shift + ch.c0 : nullptr, pt_shift, nu * 4},
            {pt ? pt->out_mass + ch.c0 : nullptr, pt_mass, nu * 8},
            {out_scores ? out_scores + ch.c0 * ko : nullptr, dv || cp ? dv_scores : sm ? smb.plain : tb.scores, nu * ko * 4},
            {sm && sm->out_keys ? sm->out_keys + ch.c0 * ko : nullptr, tb.scores, nu * ko * 4}}));
    }
    return SBR_OK;
}

/* the exclusion-list arguments of the *_reps calls: both or neither, or lists that are all empty and no items */
bool excl_args_ok(const uint64_t* excl_ptr, const uint32_t* excl_items, uint64_t num_users) {
    return (excl_ptr == nullptr) == (excl_items == nullptr) || (excl_ptr && excl_ptr[num_users] == excl_ptr[0]);
}

/* the arguments the recommend_diverse calls share */
bool diverse_args_ok(const sbr_model* m, uint32_t k, uint32_t pool, float trade_off, uint32_t metric) {
    return k >= 1 && pool >= k && pool <= sbr::diverse_max_pool(m->d) && trade_off >= 0.0f && trade_off <= 1.0f /* false for a NaN */ &&
           metric <= SBR_SIMILAR_DOT;
}

/* k of a call of the recommend family, which scans at k: the plain call's own k, or with dv (recommend_diverse) the pool, of
 * which the selection keeps dv->k_out, the caller's k */
bool scan_k_ok(const sbr_model* m, uint32_t k, const Diverse* dv, const Capped* cp = nullptr) {
    /* recommend_capped: k is the pool; that the model holds groups is recommend_scan's check, under the model's lock */
    if (cp && (dv || cp->cap < 1 || cp->k_out < 1 || cp->k_out > k)) return false;
    return dv ? diverse_args_ok(m, dv->k_out, k, dv->trade_off, dv->metric) : k >= 1 && k <= SBR_RECOMMEND_MAX_K;
}

/* the arguments the *_capped calls share: the rule and the scan's k (the pool; 0: the default min(1 024, max(64, 4 k))) out of
 * sbr_cap_args, or false without them; the rest is scan_k_ok's */
bool capped_args(const sbr_cap_args* a, uint32_t k, uint8_t* out_complete, Capped* out, uint32_t* pool) {
    if (!a) return false;
    const uint64_t dflt = std::min<uint64_t>(1024, std::max<uint64_t>(64, 4ull * k));
    *pool = a->pool ? a->pool : (uint32_t)dflt;
    *out = Capped{k, a->cap, out_complete};
    return true;
}

/* The rows of a call of the scan families, from the one source `kind` states: histories (flags: SBR_RECOMMEND_INCLUDE_HISTORY only;
 * the lists are the histories themselves), the caller's representations, or a session store's slots (flags: the same flag, and only
 * on a store with memory), the last two with optional exclusion lists; and the rows' optional tag masks, which make a filter unless
 * both are null (a *_filtered call states its filter in the variant instead).  sbr_scan_rows' fields and the kind. */
struct ScanRows {
    enum Kind { Histories, Reps, Store } kind = Histories;
    const uint64_t* user_ptr = nullptr;
    const uint32_t* item_ids = nullptr;
    uint32_t flags = 0;
    const float* reps = nullptr;
    sbr_sessions* store = nullptr;
    const uint32_t* slots = nullptr;
    const uint64_t* excl_ptr = nullptr;
    const uint32_t* excl_items = nullptr;
    const uint32_t *any_of = nullptr, *none_of = nullptr;
    static ScanRows of_histories(const uint64_t* user_ptr, const uint32_t* item_ids, uint32_t flags, const uint32_t* any_of = nullptr,
                                 const uint32_t* none_of = nullptr) {
        ScanRows r;
        r.kind = Histories; r.user_ptr = user_ptr; r.item_ids = item_ids; r.flags = flags; r.any_of = any_of; r.none_of = none_of;
        return r;
    }
    static ScanRows of_reps(const float* reps, const uint64_t* excl_ptr, const uint32_t* excl_items, const uint32_t* any_of = nullptr,
                            const uint32_t* none_of = nullptr) {
        ScanRows r;
        r.kind = Reps; r.reps = reps; r.excl_ptr = excl_ptr; r.excl_items = excl_items; r.any_of = any_of; r.none_of = none_of;
        return r;
    }
    static ScanRows of_store(sbr_sessions* store, const uint32_t* slots, const uint64_t* excl_ptr, const uint32_t* excl_items, uint32_t flags,
                             const uint32_t* any_of = nullptr, const uint32_t* none_of = nullptr) {
        ScanRows r;
        r.kind = Store; r.store = store; r.slots = slots; r.excl_ptr = excl_ptr; r.excl_items = excl_items; r.flags = flags;
        r.any_of = any_of; r.none_of = none_of;
        return r;
    }
};

/* The one entry of the scan families (defined beside the session store, whose rows it reads): the 34 public entry points of the top-k families, and the two of the ranks form, parse their
 * family's arguments, name their rows and their variant, and call this. */
sbr_status scan_call(sbr_model* m, const sbr_item_set* set, const ScanRows& r, uint64_t n, uint32_t k, uint32_t* out_items, float* out_scores,
                     ScanVariant v);
sbr_status enter_item_set(const sbr_item_set* set);

}  // namespace

sbr_status sbr_recommend(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, uint32_t k, uint32_t flags,
                         uint32_t* out_items, float* out_scores) {
    return scan_call(m, nullptr, ScanRows::of_histories(user_ptr, item_ids, flags), num_users, k, out_items, out_scores, ScanVariant());
}

sbr_status sbr_recommend_reps(sbr_model* m, const float* reps, uint64_t num_users, uint32_t k, const uint64_t* excl_ptr,
                              const uint32_t* excl_items, uint32_t* out_items, float* out_scores) {
    return scan_call(m, nullptr, ScanRows::of_reps(reps, excl_ptr, excl_items), num_users, k, out_items, out_scores, ScanVariant());
}

/* ---------------------------------------------------------------------------------------------
 * the threshold form: every item at or over a per-row score, as CSR (sbr_catalogue.hip, above_gemm_kernel)
 * ------------------------------------------------------------------------------------------- */
sbr_status sbr_recommend_above(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, const float* thresholds,
                               uint32_t flags, const uint32_t* any_of, const uint32_t* none_of, uint64_t* out_counts, uint64_t* out_total,
                               uint64_t capacity, uint32_t* out_ids, float* out_scores) {
    Above ab;
    if (!above_args(thresholds, num_users, out_counts, out_total, capacity, out_ids, out_scores, &ab)) return SBR_ERR_INVALID_ARGUMENT;
    ScanVariant v;
    v.ab = &ab;
    return scan_call(m, nullptr, ScanRows::of_histories(user_ptr, item_ids, flags, any_of, none_of), num_users, 1, nullptr, nullptr, v);
}

sbr_status sbr_recommend_above_reps(sbr_model* m, const float* reps, uint64_t num_users, const float* thresholds, const uint64_t* excl_ptr,
                                    const uint32_t* excl_items, const uint32_t* any_of, const uint32_t* none_of, uint64_t* out_counts,
                                    uint64_t* out_total, uint64_t capacity, uint32_t* out_ids, float* out_scores) {
    Above ab;
    if (!above_args(thresholds, num_users, out_counts, out_total, capacity, out_ids, out_scores, &ab)) return SBR_ERR_INVALID_ARGUMENT;
    ScanVariant v;
    v.ab = &ab;
    return scan_call(m, nullptr, ScanRows::of_reps(reps, excl_ptr, excl_items, any_of, none_of), num_users, 1, nullptr, nullptr, v);
}

/* the budget form: the exact best n[row] of every row and its cut (sbr_catalogue.hip, select_gemm_kernel; TOP in sbr_hip.h) */
sbr_status sbr_recommend_top(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, const uint64_t* n, uint32_t flags,
                             const uint32_t* any_of, const uint32_t* none_of, float* out_cuts, uint64_t* out_counts, uint64_t* out_total,
                             uint64_t capacity, uint32_t* out_ids, float* out_scores) {
    Above ab;
    if (!top_args(n, num_users, out_cuts, out_counts, out_total, capacity, out_ids, out_scores, &ab)) return SBR_ERR_INVALID_ARGUMENT;
    ScanVariant v;
    v.ab = &ab;
    return scan_call(m, nullptr, ScanRows::of_histories(user_ptr, item_ids, flags, any_of, none_of), num_users, 1, nullptr, nullptr, v);
}

sbr_status sbr_recommend_top_reps(sbr_model* m, const float* reps, uint64_t num_users, const uint64_t* n, const uint64_t* excl_ptr,
                                  const uint32_t* excl_items, const uint32_t* any_of, const uint32_t* none_of, float* out_cuts,
                                  uint64_t* out_counts, uint64_t* out_total, uint64_t capacity, uint32_t* out_ids, float* out_scores) {
    Above ab;
    if (!top_args(n, num_users, out_cuts, out_counts, out_total, capacity, out_ids, out_scores, &ab)) return SBR_ERR_INVALID_ARGUMENT;
    ScanVariant v;
    v.ab = &ab;
    return scan_call(m, nullptr, ScanRows::of_reps(reps, excl_ptr, excl_items, any_of, none_of), num_users, 1, nullptr, nullptr, v);
}

/* ---------------------------------------------------------------------------------------------
 * item tags and the filtered scans (sbr_catalogue.hip, topk_gemm_kernel's TagFilter)
 * ------------------------------------------------------------------------------------------- */
sbr_status sbr_model_set_item_tags(sbr_model* m, const uint32_t* tags) {
    if (!m) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(ensure_device(m));
    HIPCHK(hipStreamSynchronize(m->stream)); /* no scan of this model is reading the old words */
    if (!tags) {
        dfree(m->item_tags);
        m->item_tags = nullptr;
        return SBR_OK;
    }
    if (!m->item_tags) SBRCHK(dmalloc(&m->item_tags, (size_t)m->hp.num_items));
    HIPCHK(hipMemcpy(m->item_tags, tags, (size_t)m->hp.num_items * 4, hipMemcpyHostToDevice));
    return SBR_OK;
}

sbr_status sbr_model_get_item_tags(sbr_model* m, uint32_t* out) {
    if (!m || !out) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->item_tags) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipMemcpy(out, m->item_tags, (size_t)m->hp.num_items * 4, hipMemcpyDeviceToHost));
    return SBR_OK;
}

sbr_status sbr_recommend_filtered(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, uint32_t k,
                                  uint32_t flags, const uint32_t* any_of, const uint32_t* none_of, uint32_t* out_items, float* out_scores) {
    const TagFilterArg flt{any_of, none_of};
    ScanVariant v;
    v.flt = &flt;
    return scan_call(m, nullptr, ScanRows::of_histories(user_ptr, item_ids, flags), num_users, k, out_items, out_scores, v);
}

sbr_status sbr_recommend_filtered_reps(sbr_model* m, const float* reps, uint64_t num_users, uint32_t k, const uint64_t* excl_ptr,
                                       const uint32_t* excl_items, const uint32_t* any_of, const uint32_t* none_of, uint32_t* out_items,
                                       float* out_scores) {
    const TagFilterArg flt{any_of, none_of};
    ScanVariant v;
    v.flt = &flt;
    return scan_call(m, nullptr, ScanRows::of_reps(reps, excl_ptr, excl_items), num_users, k, out_items, out_scores, v);
}

/* ---------------------------------------------------------------------------------------------
 * sampling without replacement from softmax(score / T) (sbr_catalogue.hip, topk_gemm_kernel's GumbelBias)
 * ------------------------------------------------------------------------------------------- */
sbr_status sbr_recommend_sampled(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, uint32_t k, uint32_t flags,
                                 const struct sbr_sample_args* sample, const uint32_t* any_of, const uint32_t* none_of, uint32_t* out_items,
                                 float* out_scores, float* out_keys) {
    Sample sm;
    if (!sample_args(sample, out_keys, &sm)) return SBR_ERR_INVALID_ARGUMENT;
    ScanVariant v;
    v.sm = &sm;
    return scan_call(m, nullptr, ScanRows::of_histories(user_ptr, item_ids, flags, any_of, none_of), num_users, k, out_items, out_scores, v);
}

sbr_status sbr_recommend_sampled_reps(sbr_model* m, const float* reps, uint64_t num_users, uint32_t k, const uint64_t* excl_ptr,
                                      const uint32_t* excl_items, const struct sbr_sample_args* sample, const uint32_t* any_of,
                                      const uint32_t* none_of, uint32_t* out_items, float* out_scores, float* out_keys) {
    Sample sm;
    if (!sample_args(sample, out_keys, &sm)) return SBR_ERR_INVALID_ARGUMENT;
    ScanVariant v;
    v.sm = &sm;
    return scan_call(m, nullptr, ScanRows::of_reps(reps, excl_ptr, excl_items, any_of, none_of), num_users, k, out_items, out_scores, v);
}

/* ---------------------------------------------------------------------------------------------
 * the exact mass of softmax(score / T): the k = 1 scan, the sum scan and the lists' correction (sbr_catalogue.hip)
 * ------------------------------------------------------------------------------------------- */
uint32_t sbr_softmax_frac_bits(uint32_t num_items) { return sbr_softmax_fbits(num_items); }

sbr_status sbr_softmax_weights(const float* scores, uint64_t n, float temperature, float shift, uint32_t frac_bits, uint64_t* out_w) {
    Partition pt;
    uint32_t fb = 0;
    if (!partition_args(temperature, 0, nullptr, nullptr, &fb, &pt) || frac_bits > 40u || (n && (!scores || !out_w))) return SBR_ERR_INVALID_ARGUMENT;
    for (uint64_t i = 0; i < n; ++i) out_w[i] = sbr_softmax_weight(scores[i] * pt.inv_t, shift, frac_bits);
    return SBR_OK;
}

sbr_status sbr_softmax_weights_rows(const float* scores, uint64_t rows, uint64_t m, float temperature, const float* shifts, uint32_t frac_bits,
                                    uint64_t* out_w) {
    if (rows && m && !shifts) return SBR_ERR_INVALID_ARGUMENT;
    if (rows == 0 || m == 0) return sbr_softmax_weights(nullptr, 0, temperature, 0.0f, frac_bits, nullptr); /* the argument checks alone */
    for (uint64_t r = 0; r < rows; ++r) {
        const sbr_status st = sbr_softmax_weights(scores ? scores + r * m : nullptr, m, temperature, shifts[r], frac_bits, out_w ? out_w + r * m : nullptr);
        if (st != SBR_OK) return st;
    }
    return SBR_OK;
}

sbr_status sbr_log_partition(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, uint32_t flags,
                             float temperature, const uint32_t* any_of, const uint32_t* none_of, float* out_shift, uint64_t* out_mass,
                             uint32_t* out_frac_bits) {
    Partition pt;
    if (!partition_args(temperature, num_users, out_shift, out_mass, out_frac_bits, &pt)) return SBR_ERR_INVALID_ARGUMENT;
    ScanVariant v;
    v.pt = &pt;
    return scan_call(m, nullptr, ScanRows::of_histories(user_ptr, item_ids, flags, any_of, none_of), num_users, 1, nullptr, nullptr, v);
}

sbr_status sbr_log_partition_reps(sbr_model* m, const float* reps, uint64_t num_users, const uint64_t* excl_ptr, const uint32_t* excl_items,
                                  float temperature, const uint32_t* any_of, const uint32_t* none_of, float* out_shift, uint64_t* out_mass,
                                  uint32_t* out_frac_bits) {
    Partition pt;
    if (!partition_args(temperature, num_users, out_shift, out_mass, out_frac_bits, &pt)) return SBR_ERR_INVALID_ARGUMENT;
    ScanVariant v;
    v.pt = &pt;
    return scan_call(m, nullptr, ScanRows::of_reps(reps, excl_ptr, excl_items, any_of, none_of), num_users, 1, nullptr, nullptr, v);
}

namespace {

/* device buffers of the sequence_partition launchers beside TopkBufs, over ns scan rows of sequences with nrows packed rows */
struct SequencePartitionBufs {
    unsigned long long* mass;
    uint2* bt;
    uint32_t *target, *first;
    float *shift, *scores;
    uint8_t* unresolved;
    void carve(DeviceArena& ar, size_t ns, size_t nrows) {
        mass = ar.take<unsigned long long>(ns);
        bt = ar.take<uint2>(ns);
        target = ar.take<uint32_t>(ns);
        first = ar.take<uint32_t>(nrows);
        shift = ar.take<float>(ns);
        scores = ar.take<float>(ns);
        unresolved = ar.take<uint8_t>(ns);
    }
};

/* The shifts of a chunk's rows whose pool held prefix items only (`rows`, ascending, not empty): their sorted distinct prefixes as
 * the exclusion CSR of a k = 1 scan over those rows alone, in device blocks of their own — the arena is the chunk's.  Nothing of
 * this size exists for a chunk without such rows. */
sbr_status sequence_unresolved_shifts(sbr_model* m, const float* H, const Chunk& ch, const UserReps& ur, const SequenceRows& sr,
                                      const std::vector<uint32_t>& unit_pos, const std::vector<uint32_t>& rows, float inv_t, float* d_shift,
                                      uint32_t* d_flag) {
    const size_t n = rows.size();
    std::vector<int> rep(n);
    std::vector<uint64_t> eptr(n + 1, 0);
    std::vector<uint32_t> excl;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t r = rows[i], p = unit_pos[ch.c0 + r];
        const uint32_t* w = ur.b.first[ch.lu[r]];
        rep[i] = sr.rep[r];
        const size_t e0 = excl.size();
        excl.insert(excl.end(), w, w + p);
        std::sort(excl.begin() + e0, excl.end());
        excl.erase(std::unique(excl.begin() + e0, excl.end()), excl.end());
        eptr[i + 1] = excl.size();
    }
    uint32_t per = 0;
    const size_t g = sbr::recommend_groups((uint32_t)n, (uint32_t)m->hp.num_items, 1, &per);
    DeviceBlocks blocks(m->stream);
    int* d_rep = nullptr;
    uint64_t* d_eptr = nullptr;
    uint32_t *d_rows = nullptr, *d_excl = nullptr, *d_lens = nullptr, *d_items = nullptr;
    uint2* d_lists = nullptr;
    float* d_scores = nullptr;
    SBRCHK(blocks.take(&d_rep, n));
    SBRCHK(blocks.take(&d_rows, n));
    SBRCHK(blocks.take(&d_eptr, n + 1));
    SBRCHK(blocks.take(&d_excl, excl.size() + 1));
    SBRCHK(blocks.take(&d_lists, n * g));
    SBRCHK(blocks.take(&d_lens, n * g));
    SBRCHK(blocks.take(&d_items, n));
    SBRCHK(blocks.take(&d_scores, n));
    HIPCHK(hipMemcpyAsync(d_rep, rep.data(), n * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(d_rows, rows.data(), n * 4, hipMemcpyHostToDevice, m->stream));
    SBRCHK(upload_csr(m, d_eptr, eptr, d_excl, excl));
    sbr::TopkScan sc{};
    sc.rep_row = d_rep; sc.n = (uint32_t)n; sc.k = 1;
    sc.excl_ptr = d_eptr; sc.excl_items = d_excl;
    sc.lists = d_lists; sc.lens = d_lens; sc.out_items = d_items; sc.out_scores = d_scores;
    sc.nonfinite_flag = d_flag;
    return scan_launch(m, d_flag, [&] { return sbr::launch_sequence_shift_rows(m->mv, H, sc, inv_t, d_rows, d_shift, m->stream); }, {});
}

}  // namespace

sbr_status sbr_sequence_partition(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, float temperature,
                                  uint32_t flags, uint32_t last_positions, uint64_t* out_ptr, float* out_shift, uint64_t* out_mass,
                                  float* out_scores, uint8_t* out_masked) {
    if (!m || !user_ptr || !out_ptr || (flags & ~SBR_RANK_INCLUDE_HISTORY)) return SBR_ERR_INVALID_ARGUMENT;
    const bool sizing = !out_shift && !out_mass && !out_scores && !out_masked;
    if (!sizing && (!out_shift || !out_mass || !out_scores || !out_masked)) return SBR_ERR_INVALID_ARGUMENT;
    const sbr_sample_args sa{temperature, 0, nullptr};
    Sample sm;
    if (!sample_args(&sa, nullptr, &sm)) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    if (m->open_plans) return SBR_ERR_INVALID_ARGUMENT; /* as sbr_sequence_ranks */
    SBRCHK(check_csr(m, user_ptr, num_users, item_ids, false));
    const uint64_t T = m->hp.max_sequence_length;
    const bool mask = !(flags & SBR_RANK_INCLUDE_HISTORY);
    SequenceUnits su(m, user_ptr, num_users, last_positions);
    const uint64_t total = su.total;
    if (!sizing) {
        su.list_units();
        std::vector<float> shift(total), scores(total);
        std::vector<uint64_t> mass(total);
        std::vector<uint8_t> masked(total), unresolved;
        /* the shift scan's k: a pool to look past the row's own prefix items in, or the arg-max alone where nothing is masked */
        const uint32_t k0 = mask ? sbr::sequence_shift_pool() : 1u;
        const size_t cap = std::min(eval_units_cap, recommend_users_cap((uint32_t)m->hp.num_items, k0));
        const RepSource s = RepSource::of_histories(user_ptr, item_ids, 1, false);
        for (Chunk ch; next_chunk(su.unit_user, cap, s, T, &ch);) {
            const size_t ns = ch.c1 - ch.c0;
            PackedLayout lay;
            UserReps ur;
            ur.layout = &lay;
            TopkBufs tb;
            SequencePartitionBufs pb;
            SBRCHK(user_reps(m, s, ch.users, [&](DeviceArena& ar) {
                size_t nrows = 0;
                for (int n : ur.b.nsteps) nrows += (size_t)n;
                tb.carve(ar, (uint32_t)m->hp.num_items, ns, 0, k0, false);
                pb.carve(ar, ns, nrows);
            }, &ur));
            SequenceRows sr;
            sr.build(ch, ur, lay.pk, su.unit_pos, mask);
            HIPCHK(hipMemcpyAsync(tb.rep, sr.rep.data(), ns * 4, hipMemcpyHostToDevice, m->stream));
            HIPCHK(hipMemcpyAsync(pb.target, sr.test.data(), ns * 4, hipMemcpyHostToDevice, m->stream));
            if (mask) {
                HIPCHK(hipMemcpyAsync(pb.bt, sr.bt.data(), ns * 8, hipMemcpyHostToDevice, m->stream));
                HIPCHK(hipMemcpyAsync(pb.first, sr.first_rows.data(), sr.first_rows.size() * 4, hipMemcpyHostToDevice, m->stream));
            }
            const sbr::TopkScan sc = tb.scan(ns, k0, false, true);
            const sbr::SequencePartitionScan sp{sbr::PartitionScan{sm.inv_t, pb.shift, pb.mass}, mask ? pb.bt : nullptr, lay.d_off, lay.d_in_idx,
                                                pb.first, pb.target, pb.scores, pb.unresolved};
            if (mask) { /* one byte per row comes back: which rows the pool did not resolve */
                unresolved.resize(ns);
                SBRCHK(scan_launch(m, tb.flag, [&] { return sbr::launch_sequence_shift(m->mv, ur.H, sc, sp, m->stream); },
                                   {{unresolved.data(), pb.unresolved, ns}}));
                std::vector<uint32_t> rows;
                for (size_t i = 0; i < ns; ++i)
                    if (unresolved[i]) rows.push_back((uint32_t)i);
                if (!rows.empty()) SBRCHK(sequence_unresolved_shifts(m, ur.H, ch, ur, sr, su.unit_pos, rows, sm.inv_t, pb.shift, tb.flag));
            }
            SBRCHK(scan_launch(m, tb.flag, [&] {
                const int n = mask ? 0 : sbr::launch_sequence_shift(m->mv, ur.H, sc, sp, m->stream); /* nothing masked: no host step between */
                return n + sbr::launch_sequence_partition(m->mv, ur.H, sc, sp, m->stream);
            }, {{shift.data() + ch.c0, pb.shift, ns * 4}, {mass.data() + ch.c0, pb.mass, ns * 8}, {scores.data() + ch.c0, pb.scores, ns * 4}}));
            for (size_t i = 0; i < ns; ++i) masked[ch.c0 + i] = (uint8_t)sr.in_prefix[i];
        }
        if (total) {
            std::memcpy(out_shift, shift.data(), total * 4);
            std::memcpy(out_mass, mass.data(), total * 8);
            std::memcpy(out_scores, scores.data(), total * 4);
            std::memcpy(out_masked, masked.data(), total);
        }
    }
    su.fill_out_ptr(out_ptr);
    return SBR_OK;
}

/* ---------------------------------------------------------------------------------------------
 * diversified top-k: recommend's scan at k = pool, then the selection (sbr_catalogue.hip)
 * ------------------------------------------------------------------------------------------- */
sbr_status sbr_recommend_diverse_max_pool(const sbr_model* m, uint32_t* out) {
    if (!m || !out) return SBR_ERR_INVALID_ARGUMENT;
    *out = sbr::diverse_max_pool(m->d);
    return SBR_OK;
}

sbr_status sbr_recommend_diverse(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, uint32_t k, uint32_t pool,
                                 float trade_off, uint32_t metric, uint32_t flags, uint32_t* out_items, float* out_scores) {
    const Diverse dv{k, trade_off, metric};
    ScanVariant v;
    v.dv = &dv;
    return scan_call(m, nullptr, ScanRows::of_histories(user_ptr, item_ids, flags), num_users, pool, out_items, out_scores, v);
}

sbr_status sbr_recommend_diverse_filtered(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, uint32_t k,
                                          uint32_t pool, float trade_off, uint32_t metric, uint32_t flags, const uint32_t* any_of,
                                          const uint32_t* none_of, uint32_t* out_items, float* out_scores) {
    const TagFilterArg flt{any_of, none_of};
    const Diverse dv{k, trade_off, metric};
    ScanVariant v;
    v.dv = &dv;
    v.flt = &flt;
    return scan_call(m, nullptr, ScanRows::of_histories(user_ptr, item_ids, flags), num_users, pool, out_items, out_scores, v);
}

sbr_status sbr_recommend_diverse_reps(sbr_model* m, const float* reps, uint64_t num_users, uint32_t k, uint32_t pool, float trade_off,
                                      uint32_t metric, const uint64_t* excl_ptr, const uint32_t* excl_items, uint32_t* out_items,
                                      float* out_scores) {
    const Diverse dv{k, trade_off, metric};
    ScanVariant v;
    v.dv = &dv;
    return scan_call(m, nullptr, ScanRows::of_reps(reps, excl_ptr, excl_items), num_users, pool, out_items, out_scores, v);
}

sbr_status sbr_recommend_diverse_filtered_reps(sbr_model* m, const float* reps, uint64_t num_users, uint32_t k, uint32_t pool, float trade_off,
                                               uint32_t metric, const uint64_t* excl_ptr, const uint32_t* excl_items, const uint32_t* any_of,
                                               const uint32_t* none_of, uint32_t* out_items, float* out_scores) {
    const TagFilterArg flt{any_of, none_of};
    const Diverse dv{k, trade_off, metric};
    ScanVariant v;
    v.dv = &dv;
    v.flt = &flt;
    return scan_call(m, nullptr, ScanRows::of_reps(reps, excl_ptr, excl_items), num_users, pool, out_items, out_scores, v);
}

/* ---------------------------------------------------------------------------------------------
 * item groups and the capped top-k: recommend's scan at k = pool, then the rule (sbr_catalogue.hip, capped_select_kernel)
 * ------------------------------------------------------------------------------------------- */
sbr_status sbr_model_set_item_groups(sbr_model* m, const uint32_t* groups) {
    if (!m) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(ensure_device(m));
    HIPCHK(hipStreamSynchronize(m->stream)); /* no scan of this model is reading the old words */
    if (!groups) {
        dfree(m->item_groups);
        m->item_groups = nullptr;
        return SBR_OK;
    }
    if (!m->item_groups) SBRCHK(dmalloc(&m->item_groups, (size_t)m->hp.num_items));
    HIPCHK(hipMemcpy(m->item_groups, groups, (size_t)m->hp.num_items * 4, hipMemcpyHostToDevice));
    return SBR_OK;
}

sbr_status sbr_model_get_item_groups(sbr_model* m, uint32_t* out) {
    if (!m || !out) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    if (!m->item_groups) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(ensure_device(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipMemcpy(out, m->item_groups, (size_t)m->hp.num_items * 4, hipMemcpyDeviceToHost));
    return SBR_OK;
}

sbr_status sbr_recommend_capped(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, uint32_t k, uint32_t flags,
                                const struct sbr_cap_args* cap, const uint32_t* any_of, const uint32_t* none_of, uint32_t* out_items,
                                float* out_scores, uint8_t* out_complete) {
    Capped cp;
    uint32_t pool = 0;
    if (!capped_args(cap, k, out_complete, &cp, &pool)) return SBR_ERR_INVALID_ARGUMENT;
    ScanVariant v;
    v.cp = &cp;
    return scan_call(m, nullptr, ScanRows::of_histories(user_ptr, item_ids, flags, any_of, none_of), num_users, pool, out_items, out_scores, v);
}

sbr_status sbr_recommend_capped_reps(sbr_model* m, const float* reps, uint64_t num_users, uint32_t k, const uint64_t* excl_ptr,
                                     const uint32_t* excl_items, const struct sbr_cap_args* cap, const uint32_t* any_of,
                                     const uint32_t* none_of, uint32_t* out_items, float* out_scores, uint8_t* out_complete) {
    Capped cp;
    uint32_t pool = 0;
    if (!capped_args(cap, k, out_complete, &cp, &pool)) return SBR_ERR_INVALID_ARGUMENT;
    ScanVariant v;
    v.cp = &cp;
    return scan_call(m, nullptr, ScanRows::of_reps(reps, excl_ptr, excl_items, any_of, none_of), num_users, pool, out_items, out_scores, v);
}

/* ---------------------------------------------------------------------------------------------
 * exact top-k neighbours of catalogue items (sbr_catalogue.hip)
 * ------------------------------------------------------------------------------------------- */
namespace {

sbr_status similar_items_call(sbr_model* m, const uint32_t* query_items, uint64_t num_queries, uint32_t k, uint32_t metric, uint32_t flags,
                              const uint64_t* excl_ptr, const uint32_t* excl_items, uint32_t* out_items, float* out_scores,
                              const TagFilterArg* flt) {
    if (!m || (num_queries && (!query_items || !out_items))) return SBR_ERR_INVALID_ARGUMENT;
    if (k < 1 || k > SBR_RECOMMEND_MAX_K || metric > SBR_SIMILAR_DOT || (flags & ~SBR_SIMILAR_INCLUDE_SELF)) return SBR_ERR_INVALID_ARGUMENT;
    if (!excl_args_ok(excl_ptr, excl_items, num_queries)) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    for (uint64_t j = 0; j < num_queries; ++j)
        if (query_items[j] >= m->hp.num_items) return SBR_ERR_INVALID_ARGUMENT;
    if (excl_ptr) SBRCHK(check_csr(m, excl_ptr, num_queries, excl_items, false));
    /* what a query's row may not hold: the caller's list and, unless it is wanted, the query itself */
    const bool self = (flags & SBR_SIMILAR_INCLUDE_SELF) != 0;
    std::vector<uint64_t> eptr;
    std::vector<uint32_t> eitems;
    if (!self) {
        eptr.assign(num_queries + 1, 0);
        eitems.reserve((size_t)num_queries + (excl_ptr ? (size_t)(excl_ptr[num_queries] - excl_ptr[0]) : 0));
        for (uint64_t j = 0; j < num_queries; ++j) {
            if (excl_ptr && excl_ptr[j + 1] > excl_ptr[j]) eitems.insert(eitems.end(), excl_items + excl_ptr[j], excl_items + excl_ptr[j + 1]);
            eitems.push_back(query_items[j]);
            eptr[j + 1] = eitems.size();
        }
    }
    ScanVariant v;
    v.flt = flt;
    v.cosine = metric == SBR_SIMILAR_COSINE;
    return recommend_scan(m, RepSource::of_item_rows(query_items, self ? excl_ptr : eptr.data(), self ? excl_items : eitems.data()), num_queries, k,
                          out_items, out_scores, v);
}

}  // namespace

sbr_status sbr_similar_items(sbr_model* m, const uint32_t* query_items, uint64_t num_queries, uint32_t k, uint32_t metric, uint32_t flags,
                             const uint64_t* excl_ptr, const uint32_t* excl_items, uint32_t* out_items, float* out_scores) {
    return similar_items_call(m, query_items, num_queries, k, metric, flags, excl_ptr, excl_items, out_items, out_scores, nullptr);
}

sbr_status sbr_similar_items_filtered(sbr_model* m, const uint32_t* query_items, uint64_t num_queries, uint32_t k, uint32_t metric,
                                      uint32_t flags, const uint64_t* excl_ptr, const uint32_t* excl_items, const uint32_t* any_of,
                                      const uint32_t* none_of, uint32_t* out_items, float* out_scores) {
    const TagFilterArg flt{any_of, none_of};
    return similar_items_call(m, query_items, num_queries, k, metric, flags, excl_ptr, excl_items, out_items, out_scores, &flt);
}

/* ---------------------------------------------------------------------------------------------
 * recommend within an item subset, batched candidate scoring, batched representations (sbr_catalogue.hip)
 * ------------------------------------------------------------------------------------------- */
namespace {

/* recommend_scan over the item set subset_items[0, num_subset) — validated, sorted and de-duplicated here; an empty set is rows of
 * padding without a scan */
sbr_status recommend_among_scan(sbr_model* m, const RepSource& s, uint64_t num_users, uint32_t k, const uint32_t* subset_items,
                                uint64_t num_subset, uint32_t* out_items, float* out_scores) {
    if (num_subset && !subset_items) return SBR_ERR_INVALID_ARGUMENT;
    for (uint64_t j = 0; j < num_subset; ++j)
        if (subset_items[j] >= m->hp.num_items) return SBR_ERR_INVALID_ARGUMENT;
    std::vector<uint32_t> subset(subset_items, subset_items + num_subset);
    std::sort(subset.begin(), subset.end());
    subset.erase(std::unique(subset.begin(), subset.end()), subset.end());
    if (subset.empty()) {
        std::fill(out_items, out_items + num_users * k, 0xFFFFFFFFu);
        if (out_scores) std::fill(out_scores, out_scores + num_users * k, -INFINITY);
        return SBR_OK;
    }
    ScanVariant v;
    v.subset = &subset;
    return recommend_scan(m, s, num_users, k, out_items, out_scores, v);
}

/* device buffers of launch_candidate_scores over np pairs */
struct CandidateBufs {
    uint32_t *row, *item, *flag;
    float* scores;
    void carve(DeviceArena& ar, size_t np) {
        row = ar.take<uint32_t>(np);
        item = ar.take<uint32_t>(np);
        scores = ar.take<float>(np);
        flag = ar.take<uint32_t>(1);
    }
};

/* Scores of every user's candidates, users from `s`.  The users that have candidates go through next_chunk; a chunk's pairs are
 * contiguous in cand_items (the users between them have none) and are scored in launches of at most candidate_pairs_cap pairs
 * against the chunk's one forward pass, a launch ending wherever in a user's list the cap falls. */
sbr_status score_candidates_scan(sbr_model* m, const RepSource& s, uint64_t num_users, const uint64_t* cand_ptr, const uint32_t* cand_items,
                                 float* out_scores) {
    if (!cand_ptr) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(check_csr(m, cand_ptr, num_users, cand_items, false));
    if (cand_ptr[num_users] == cand_ptr[0]) return SBR_OK;
    if (!out_scores) return SBR_ERR_INVALID_ARGUMENT;
    std::vector<uint64_t> users;
    for (uint64_t u = 0; u < num_users; ++u)
        if (cand_ptr[u + 1] > cand_ptr[u]) users.push_back(u);
    for (Chunk ch; next_chunk(users, eval_units_cap, s, m->hp.max_sequence_length, &ch);) {
        const size_t nu = ch.users.size();
        const uint64_t p0 = cand_ptr[ch.users[0]], p1 = cand_ptr[ch.users[nu - 1] + 1];
        const size_t cap = (size_t)std::min<uint64_t>(p1 - p0, sbr::candidate_pairs_cap);
        UserReps ur;
        CandidateBufs cb;
        SBRCHK(user_reps(m, s, ch.users, [&](DeviceArena& ar) { cb.carve(ar, cap); }, &ur));
        std::vector<uint32_t> row(cap);
        size_t i = 0; /* the chunk's user of the pair in hand */
        for (uint64_t q = p0; q < p1; q += cap) {
            const size_t n = (size_t)std::min<uint64_t>(cap, p1 - q);
            for (size_t j = 0; j < n; ++j) {
                while (cand_ptr[ch.users[i] + 1] <= q + j) ++i;
                row[j] = (uint32_t)ur.rep_row[i];
            }
            HIPCHK(hipMemcpyAsync(cb.row, row.data(), n * 4, hipMemcpyHostToDevice, m->stream));
            HIPCHK(hipMemcpyAsync(cb.item, cand_items + q, n * 4, hipMemcpyHostToDevice, m->stream));
            SBRCHK(scan_launch(m, cb.flag, [&] {
                return sbr::launch_candidate_scores(m->mv, ur.H, cb.row, cb.item, n, cb.scores, cb.flag, m->stream);
            }, {{out_scores + (q - cand_ptr[0]), cb.scores, n * 4}}));
        }
    }
    return SBR_OK;
}

}  // namespace

sbr_status sbr_user_representations(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, float* out_reps) {
    if (!m || !user_ptr || (num_users && !out_reps)) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    SBRCHK(check_csr(m, user_ptr, num_users, item_ids, false));
    std::vector<uint64_t> users(num_users);
    for (uint64_t u = 0; u < num_users; ++u) users[u] = u;
    const RepSource s = RepSource::of_histories(user_ptr, item_ids, 0, false);
    const size_t dl = (size_t)m->dl;
    for (Chunk ch; next_chunk(users, eval_units_cap, s, m->hp.max_sequence_length, &ch);) {
        const size_t nu = ch.users.size();
        UserReps ur;
        int* rep = nullptr;
        float* rows = nullptr;
        uint32_t* flag = nullptr; /* scan_launch's; nothing here raises it */
        SBRCHK(user_reps(m, s, ch.users, [&](DeviceArena& ar) {
            rep = ar.take<int>(nu);
            rows = ar.take<float>(nu * dl);
            flag = ar.take<uint32_t>(1);
        }, &ur));
        HIPCHK(hipMemcpyAsync(rep, ur.rep_row.data(), nu * 4, hipMemcpyHostToDevice, m->stream));
        SBRCHK(scan_launch(m, flag, [&] { return sbr::launch_rep_rows(ur.H, rep, (uint32_t)nu, m->d, m->dl, rows, m->stream); },
                           {{out_reps + ch.c0 * dl, rows, nu * dl * 4}}));
    }
    return SBR_OK;
}

sbr_status sbr_score_candidates(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users,
                                const uint64_t* cand_ptr, const uint32_t* cand_items, float* out_scores) {
    if (!m || !user_ptr) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    SBRCHK(check_csr(m, user_ptr, num_users, item_ids, false));
    return score_candidates_scan(m, RepSource::of_histories(user_ptr, item_ids, 0, false), num_users, cand_ptr, cand_items, out_scores);
}

sbr_status sbr_score_candidates_reps(sbr_model* m, const float* reps, uint64_t num_users, const uint64_t* cand_ptr, const uint32_t* cand_items,
                                     float* out_scores) {
    if (!m || (num_users && !reps)) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    return score_candidates_scan(m, RepSource::of_rows(reps), num_users, cand_ptr, cand_items, out_scores);
}

sbr_status sbr_recommend_among(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, uint32_t k, uint32_t flags,
                               const uint32_t* subset_items, uint64_t num_subset, uint32_t* out_items, float* out_scores) {
    if (!m || !user_ptr || (num_users && !out_items)) return SBR_ERR_INVALID_ARGUMENT;
    if (k < 1 || k > SBR_RECOMMEND_MAX_K || (flags & ~SBR_RECOMMEND_INCLUDE_HISTORY)) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    SBRCHK(check_csr(m, user_ptr, num_users, item_ids, false));
    return recommend_among_scan(m, RepSource::of_histories(user_ptr, item_ids, 0, !(flags & SBR_RECOMMEND_INCLUDE_HISTORY)), num_users, k, subset_items,
                                num_subset, out_items, out_scores);
}

sbr_status sbr_recommend_among_reps(sbr_model* m, const float* reps, uint64_t num_users, uint32_t k, const uint64_t* excl_ptr,
                                    const uint32_t* excl_items, const uint32_t* subset_items, uint64_t num_subset, uint32_t* out_items,
                                    float* out_scores) {
    if (!m || (num_users && (!reps || !out_items))) return SBR_ERR_INVALID_ARGUMENT;
    if (k < 1 || k > SBR_RECOMMEND_MAX_K) return SBR_ERR_INVALID_ARGUMENT;
    if (!excl_args_ok(excl_ptr, excl_items, num_users)) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    if (excl_ptr) SBRCHK(check_csr(m, excl_ptr, num_users, excl_items, false));
    return recommend_among_scan(m, RepSource::of_rows(reps, excl_ptr, excl_items), num_users, k, subset_items, num_subset, out_items, out_scores);
}

/* ---------------------------------------------------------------------------------------------
 * exact ranks of many targets per user from one catalogue scan (sbr_catalogue.hip)
 * ------------------------------------------------------------------------------------------- */
namespace {

/* device buffers of launch_rank_targets over ns scan-users of nlu users with nt targets and nmask mask entries */
struct RankTargetsBufs {
    int* rep;
    uint32_t *lu, *sptr, *tgt, *pos, *ranks, *mask, *buckets, *totals, *flag;
    float *ts, *th, *tmin, *tmin2;
    uint64_t* mptr;
    void carve(DeviceArena& ar, size_t ns, size_t nlu, size_t nt, size_t nmask, uint32_t tmax) {
        rep = ar.take<int>(ns);
        lu = ar.take<uint32_t>(ns);
        sptr = ar.take<uint32_t>(ns + 1);
        tgt = ar.take<uint32_t>(nt + 1);
        ts = ar.take<float>(nt + 1);
        pos = ar.take<uint32_t>(nt + 1);
        ranks = ar.take<uint32_t>(nt + 1);
        mptr = ar.take<uint64_t>(nlu + 1);
        mask = ar.take<uint32_t>(nmask + 1);
        th = ar.take<float>(ns * tmax);
        buckets = ar.take<uint32_t>(ns * tmax);
        tmin = ar.take<float>(ns);
        tmin2 = ar.take<float>(ns);
        totals = ar.take<uint32_t>(ns);
        flag = ar.take<uint32_t>(1);
    }
};

/* Ranks of every user's targets, users from `s`: validates the targets, cuts each user's into scan-users — runs of at most tmax,
 * in user and target order (a user without targets has none) — and scans them in chunks.  The targets of a chunk are contiguous in
 * target_items, and so are their ranks in out_ranks. */
sbr_status rank_targets_scan(sbr_model* m, const RepSource& s, uint64_t num_users, const uint64_t* target_ptr, const uint32_t* target_items,
                             uint32_t* out_ranks) {
    if (!target_ptr) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(check_csr(m, target_ptr, num_users, target_items, false));
    if (target_ptr[num_users] - target_ptr[0] && !out_ranks) return SBR_ERR_INVALID_ARGUMENT;
    const uint32_t tmax = sbr::rank_targets_tmax(m->d);
    std::vector<uint64_t> su_user, su_begin; /* the user of scan-user i; its first target, an index into target_items */
    for (uint64_t u = 0; u < num_users; ++u)
        for (uint64_t e = target_ptr[u]; e < target_ptr[u + 1]; e += tmax) {
            su_user.push_back(u);
            su_begin.push_back(e);
        }
    for (Chunk ch; next_chunk(su_user, eval_units_cap, s, m->hp.max_sequence_length, &ch);) {
        const size_t ns = ch.c1 - ch.c0, nlu = ch.users.size();
        const uint64_t t0 = su_begin[ch.c0];
        const size_t nt = (size_t)(std::min(su_begin[ch.c1 - 1] + tmax, target_ptr[su_user[ch.c1 - 1] + 1]) - t0);
        UserReps ur; /* its lists: the masks (list_ptr empty: no mask) */
        RankTargetsBufs rb;
        SBRCHK(user_reps(m, s, ch.users, [&](DeviceArena& ar) { rb.carve(ar, ns, nlu, nt, ur.b.list_items.size(), tmax); }, &ur));
        std::vector<int> srep(ns);
        std::vector<uint32_t> sptr(ns + 1);
        for (size_t i = 0; i < ns; ++i) {
            srep[i] = ur.rep_row[ch.lu[i]];
            sptr[i] = (uint32_t)(su_begin[ch.c0 + i] - t0);
        }
        sptr[ns] = (uint32_t)nt;
        const bool mask = !ur.b.list_ptr.empty();
        HIPCHK(hipMemcpyAsync(rb.rep, srep.data(), ns * 4, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(rb.lu, ch.lu.data(), ns * 4, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(rb.sptr, sptr.data(), (ns + 1) * 4, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(rb.tgt, target_items + t0, nt * 4, hipMemcpyHostToDevice, m->stream));
        if (mask) SBRCHK(upload_csr(m, rb.mptr, ur.b.list_ptr, rb.mask, ur.b.list_items));
        SBRCHK(scan_launch(m, rb.flag, [&] {
            return sbr::launch_rank_targets(m->mv, ur.H, rb.rep, rb.lu, rb.sptr, (uint32_t)ns, rb.tgt, mask ? rb.mptr : nullptr, rb.mask, rb.ts, rb.pos,
                                     rb.th, rb.tmin, rb.tmin2, rb.buckets, rb.totals, rb.ranks, rb.flag, m->stream);
        }, {{out_ranks + (t0 - target_ptr[0]), rb.ranks, nt * 4}}));
    }
    return SBR_OK;
}

}  // namespace

sbr_status sbr_rank_targets(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users,
                            const uint64_t* target_ptr, const uint32_t* target_items, uint32_t flags, uint32_t* out_ranks) {
    if (!m || !user_ptr || (flags & ~SBR_RANK_INCLUDE_HISTORY)) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    SBRCHK(check_csr(m, user_ptr, num_users, item_ids, false));
    /* the WHOLE history is masked (evaluation.rs:30-32) */
    return rank_targets_scan(m, RepSource::of_histories(user_ptr, item_ids, 0, !(flags & SBR_RANK_INCLUDE_HISTORY)), num_users, target_ptr,
                             target_items, out_ranks);
}

sbr_status sbr_rank_targets_reps(sbr_model* m, const float* reps, uint64_t num_users, const uint64_t* excl_ptr, const uint32_t* excl_items,
                                 const uint64_t* target_ptr, const uint32_t* target_items, uint32_t* out_ranks) {
    if (!m || (num_users && !reps)) return SBR_ERR_INVALID_ARGUMENT;
    if (!excl_args_ok(excl_ptr, excl_items, num_users)) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    if (excl_ptr) SBRCHK(check_csr(m, excl_ptr, num_users, excl_items, false));
    return rank_targets_scan(m, RepSource::of_rows(reps, excl_ptr, excl_items), num_users, target_ptr, target_items, out_ranks);
}

/* ---------------------------------------------------------------------------------------------
 * session store: device-resident recurrent states advanced one event at a time (sbr_sessions.hip)
 * ------------------------------------------------------------------------------------------- */
}  // extern "C"

struct sbr_sessions {
    sbr_model* m = nullptr;
    uint64_t capacity = 0;
    uint64_t gen = 0;       /* the model's param_gen the states were computed under (creation / the last reset_all) */
    sbr::SessionView v{nullptr, nullptr, nullptr}; /* rows [capacity + 1]: the last one is the empty-history row */
    std::vector<uint64_t> host_len; /* the host's copy of len, kept by every successful call: which slots read the empty-history row */
    sbr::SeenView seen{nullptr, nullptr, 0}; /* seen-item memory: ring [capacity][w], cnt [capacity]; w == 0: none (and no launch of its kernels) */
};

namespace {

constexpr uint64_t sessions_max_capacity = 0x7FFFFFFEull; /* the scans index rows with an int; one more row follows the slots */

/* a call's slots: each below capacity, none twice */
sbr_status check_slots(const sbr_sessions* st, const uint32_t* slots, uint64_t n) {
    if (n && !slots) return SBR_ERR_INVALID_ARGUMENT;
    for (uint64_t i = 0; i < n; ++i)
        if (slots[i] >= st->capacity) return SBR_ERR_INVALID_ARGUMENT;
    std::vector<uint32_t> sorted(slots, slots + n);
    std::sort(sorted.begin(), sorted.end());
    return std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end() ? SBR_OK : SBR_ERR_INVALID_ARGUMENT;
}

/* entry of every store call but reset_all / capacity / destroy (the caller holds the model's mutex): the model's reader entry, and
 * no call mixes states of two parameter sets — not while a fit plan is open either, whose steps change parameters under the store */
sbr_status enter_sessions(sbr_sessions* st) {
    SBRCHK(enter_reader(st->m));
    return st->gen == st->m->param_gen && st->m->open_plans == 0 ? SBR_OK : SBR_ERR_INVALID_ARGUMENT;
}

/* Appends items[ptr[i] .. ptr[i + 1]) to slot slots[i] (already validated; slot == capacity with advance = 0: the empty-history
 * row).  Sessions without items take no part; the others are ordered by item count descending, as the packers order sequences. */
sbr_status sessions_append(sbr_sessions* st, const uint32_t* slots, uint64_t n, const uint64_t* ptr, const uint32_t* ids, int advance) {
    sbr_model* m = st->m;
    const uint64_t total = ptr[n] - ptr[0];
    if (total == 0) return SBR_OK;
    if (total >= (1ull << 31)) return SBR_ERR_INVALID_ARGUMENT; /* packed rows are addressed with an int */
    std::vector<uint32_t> order;
    for (uint64_t i = 0; i < n; ++i)
        if (ptr[i + 1] > ptr[i]) order.push_back((uint32_t)i);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return ptr[a + 1] - ptr[a] > ptr[b + 1] - ptr[b]; });
    const size_t ns = order.size(), d = (size_t)m->d;
    const int tm = (int)(ptr[order[0] + 1] - ptr[order[0]]);
    std::vector<uint32_t> slot(ns), count(ns), packed;
    std::vector<unsigned long long> start(ns);
    std::vector<int> off;
    for (size_t b = 0; b < ns; ++b) {
        slot[b] = slots[order[b]];
        count[b] = (uint32_t)(ptr[order[b] + 1] - ptr[order[b]]);
        start[b] = ptr[order[b]] - ptr[0];
    }
    const bool lstm = m->ng != 0;
    if (lstm) { /* time-major: step t covers the sessions with more than t items, a prefix */
        off.assign((size_t)tm + 1, 0);
        packed.resize(total);
        size_t alive = ns;
        for (int t = 0; t < tm; ++t) {
            while (alive > 0 && count[alive - 1] <= (uint32_t)t) --alive;
            for (size_t b = 0; b < alive; ++b) packed[(size_t)off[t] + b] = ids[ptr[order[b]] + (uint64_t)t];
            off[t + 1] = off[t] + (int)alive;
        }
    }
    sbr::SessionAppend a{};
    uint32_t *d_slot = nullptr, *d_count = nullptr, *d_items = nullptr, *d_raw = nullptr;
    unsigned long long* d_start = nullptr;
    const bool remember = advance && st->seen.w; /* the ring writes read the call's ids session-major: EWMA's own arrays, a second copy for the LSTM */
    SBRCHK(carve_arena(m, [&](DeviceArena& ar) {
        d_slot = ar.take<uint32_t>(ns);
        d_count = ar.take<uint32_t>(ns);
        d_items = ar.take<uint32_t>(total);
        if (lstm) { a.Hs = ar.take<float>(2 * ns * d); a.Cs = ar.take<float>(2 * ns * d); }
        else d_start = ar.take<unsigned long long>(ns);
        if (lstm && remember) { d_raw = ar.take<uint32_t>(total); d_start = ar.take<unsigned long long>(ns); }
    }));
    HIPCHK(hipMemcpyAsync(d_slot, slot.data(), ns * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(d_count, count.data(), ns * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(d_items, lstm ? packed.data() : ids + ptr[0], total * 4, hipMemcpyHostToDevice, m->stream));
    if (!lstm || remember) HIPCHK(hipMemcpyAsync(d_start, start.data(), ns * 8, hipMemcpyHostToDevice, m->stream));
    if (lstm && remember) HIPCHK(hipMemcpyAsync(d_raw, ids + ptr[0], total * 4, hipMemcpyHostToDevice, m->stream));
    a.n = (int)ns; a.tm = tm;
    a.slot = d_slot; a.count = d_count; a.items = d_items; a.start = d_start;
    a.off_host = off.data();
    a.advance = advance;
    {
        ScopedTimer t(m, SBR_K_RECURRENT_FWD, (lstm ? (uint64_t)tm + 1 : 1) + (remember ? 1 : 0));
        if (sbr::launch_session_append(m->mv, st->v, a, m->stream) < 0) return SBR_ERR_UNSUPPORTED;
        if (remember) sbr::launch_session_seen_append(st->seen, d_slot, d_start, d_count, lstm ? d_raw : d_items, (int)ns, m->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(m->stream)); /* the host vectors are read by the asynchronous copies above */
    if (advance)
        for (size_t b = 0; b < ns; ++b) st->host_len[slot[b]] += count[b];
    return SBR_OK;
}

/* the store's device arrays back to the scratch cache (the caller has drained the stream: nothing may still read them) */
void sessions_free(sbr_sessions* st) {
    dfree(st->v.H); dfree(st->v.C); dfree(st->v.len); dfree(st->seen.ring); dfree(st->seen.cnt);
}

/* every slot empty, the empty-history row made from the model's current parameters, the store bound to them */
sbr_status sessions_rebind(sbr_sessions* st) {
    sbr_model* m = st->m;
    const size_t rows = (size_t)st->capacity + 1, d = (size_t)m->d;
    HIPCHK(hipMemsetAsync(st->v.H, 0, rows * d * 4, m->stream));
    if (st->v.C) HIPCHK(hipMemsetAsync(st->v.C, 0, rows * d * 4, m->stream));
    HIPCHK(hipMemsetAsync(st->v.len, 0, rows * 8, m->stream));
    if (st->seen.w) HIPCHK(hipMemsetAsync(st->seen.cnt, 0, (size_t)st->capacity * 8, m->stream)); /* every memory empty; the ring needs no clearing */
    std::fill(st->host_len.begin(), st->host_len.end(), 0);
    const uint32_t row = (uint32_t)st->capacity, item0 = 0; /* one step of item 0 from zero (lstm.rs:262-264); not a length */
    const uint64_t ptr[2] = {0, 1};
    SBRCHK(sessions_append(st, &row, 1, ptr, &item0, 0));
    st->gen = m->param_gen;
    return SBR_OK;
}

/* the row each slot's representation is read from: its own, or the empty-history row */
std::vector<int> session_rep_rows(const sbr_sessions* st, const uint32_t* slots, uint64_t n) {
    std::vector<int> rows(n);
    for (uint64_t i = 0; i < n; ++i) rows[i] = st->host_len[slots[i]] ? (int)slots[i] : (int)st->capacity;
    return rows;
}

/* h_out / c_out [n][embedding_dim] and len_out [n] (each optional) of rows `rows` of the store */
sbr_status sessions_gather(sbr_sessions* st, const uint32_t* rows, uint64_t n, float* h_out, float* c_out, uint64_t* len_out) {
    sbr_model* m = st->m;
    if (n == 0) return SBR_OK;
    const size_t dl = (size_t)m->dl;
    uint32_t* d_rows = nullptr;
    float *d_h = nullptr, *d_c = nullptr;
    unsigned long long* d_len = nullptr;
    SBRCHK(carve_arena(m, [&](DeviceArena& ar) {
        d_rows = ar.take<uint32_t>(n);
        if (h_out) d_h = ar.take<float>(n * dl);
        if (c_out) d_c = ar.take<float>(n * dl);
        if (len_out) d_len = ar.take<unsigned long long>(n);
    }));
    HIPCHK(hipMemcpyAsync(d_rows, rows, n * 4, hipMemcpyHostToDevice, m->stream));
    sbr::launch_session_get_state(st->v, d_rows, (int)n, m->d, m->dl, d_h, d_c, d_len, m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(m->stream));
    if (h_out) HIPCHK(hipMemcpy(h_out, d_h, n * dl * 4, hipMemcpyDeviceToHost));
    if (c_out) HIPCHK(hipMemcpy(c_out, d_c, n * dl * 4, hipMemcpyDeviceToHost));
    if (len_out) HIPCHK(hipMemcpy(len_out, d_len, n * 8, hipMemcpyDeviceToHost));
    return SBR_OK;
}

/* Sessions per replay chunk.  A chunk's scratch in the eval arena is its slot and count words, its item feed (at most w words per
 * session) and, for the LSTM, the two parities of scratch h and c rows the steps write: the chunk is as large as keeps that within
 * 256 MB — the bound the top-k scans keep their per-user lists to (recommend_users_cap) — and its feed addressable with an int.
 * SBR_SESSIONS_REPLAY_CHUNK=n (n >= 1) is a TEST HOOK read per call that replaces the first bound; the second still applies. */
size_t replay_chunk_cap(const sbr_model* m, uint32_t w) {
    constexpr size_t budget = (size_t)256 << 20;
    const size_t per = 8 + (size_t)w * 4 + (m->ng ? (size_t)m->d * 16 : 8);
    const size_t cap = chunk_override("SBR_SESSIONS_REPLAY_CHUNK", std::max<size_t>(budget / per, 1));
    return std::min<size_t>(cap, (size_t)0x7FFFFFFF / w);
}

/* One replay chunk (sbr_replay_plan.h): the feed written from the rings, then an append call's launches over it — the step
 * kernels' arithmetic is the contract — with no ring write.  The chunk's rows of H, C, len are zero when this runs. */
sbr_status sessions_replay_chunk(sbr_sessions* st, const sbr::ReplayPlan& plan, const sbr::ReplayChunk& ch) {
    sbr_model* m = st->m;
    const size_t ns = ch.n, d = (size_t)m->d;
    const bool lstm = m->ng != 0;
    sbr::SessionAppend a{};
    uint32_t *d_slot = nullptr, *d_count = nullptr, *d_items = nullptr;
    unsigned long long* d_start = nullptr;
    int* d_off = nullptr;
    SBRCHK(carve_arena(m, [&](DeviceArena& ar) {
        d_slot = ar.take<uint32_t>(ns);
        d_count = ar.take<uint32_t>(ns);
        d_items = ar.take<uint32_t>(ch.total);
        if (lstm) { a.Hs = ar.take<float>(2 * ns * d); a.Cs = ar.take<float>(2 * ns * d); d_off = ar.take<int>(ch.off.size()); }
        else d_start = ar.take<unsigned long long>(ns);
    }));
    HIPCHK(hipMemcpyAsync(d_slot, plan.slot.data() + ch.first, ns * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(d_count, plan.count.data() + ch.first, ns * 4, hipMemcpyHostToDevice, m->stream));
    if (lstm) HIPCHK(hipMemcpyAsync(d_off, ch.off.data(), ch.off.size() * 4, hipMemcpyHostToDevice, m->stream));
    else HIPCHK(hipMemcpyAsync(d_start, ch.start.data(), ns * 8, hipMemcpyHostToDevice, m->stream));
    a.n = (int)ns; a.tm = ch.tm;
    a.slot = d_slot; a.count = d_count; a.items = d_items; a.start = d_start;
    a.off_host = ch.off.data();
    a.advance = 1;
    { /* the feed is bracketed as the ordering family, which no other prediction-side call uses: timing_read splits a replay into feed and steps */
        ScopedTimer t(m, SBR_K_SPARSE_SORT, 1);
        sbr::launch_session_replay_feed(st->seen, d_slot, d_count, (int)ns, ch.tm, d_off, d_start, d_items, m->stream);
    }
    {
        ScopedTimer t(m, SBR_K_RECURRENT_FWD, lstm ? (uint64_t)ch.tm + 1 : 1);
        if (sbr::launch_session_append(m->mv, st->v, a, m->stream) < 0) return SBR_ERR_UNSUPPORTED;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(m->stream)); /* the plan's vectors are read by the asynchronous copies above */
    for (size_t b = 0; b < ns; ++b) st->host_len[plan.slot[ch.first + b]] = plan.count[ch.first + b];
    return SBR_OK;
}

}  // namespace

extern "C" {

sbr_status sbr_sessions_create(sbr_model* m, uint64_t capacity, sbr_sessions** out) { return sbr_sessions_create_seen(m, capacity, 0, out); }

sbr_status sbr_sessions_create_seen(sbr_model* m, uint64_t capacity, uint32_t seen_capacity, sbr_sessions** out) {
    if (!m || !out || capacity == 0 || capacity > sessions_max_capacity || seen_capacity > SBR_SESSIONS_MAX_SEEN) return SBR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    sbr_sessions* st = new (std::nothrow) sbr_sessions();
    if (!st) return SBR_ERR_OUT_OF_MEMORY;
    st->m = m;
    st->capacity = capacity;
    const size_t rows = (size_t)capacity + 1, d = (size_t)m->d;
    sbr_status s = dmalloc(&st->v.H, rows * d);
    if (s == SBR_OK && m->ng) s = dmalloc(&st->v.C, rows * d);
    if (s == SBR_OK) s = dmalloc(&st->v.len, rows);
    if (s == SBR_OK && seen_capacity) s = dmalloc(&st->seen.ring, (size_t)capacity * seen_capacity);
    if (s == SBR_OK && seen_capacity) s = dmalloc(&st->seen.cnt, (size_t)capacity);
    if (s == SBR_OK) {
        st->seen.w = seen_capacity;
        st->host_len.assign(capacity, 0);
        s = sessions_rebind(st);
    }
    if (s != SBR_OK) {
        hipStreamSynchronize(m->stream);
        sessions_free(st);
        delete st;
        return s;
    }
    *out = st;
    return SBR_OK;
}

void sbr_sessions_destroy(sbr_sessions* st) {
    if (!st) return;
    {
        std::lock_guard<std::mutex> lock(st->m->mu);
        hipSetDevice(st->m->device);
        hipStreamSynchronize(st->m->stream); /* the rows go back to the scratch cache: nothing may still read them */
        sessions_free(st);
    }
    delete st;
}

sbr_status sbr_sessions_capacity(const sbr_sessions* st, uint64_t* out) {
    if (!st || !out) return SBR_ERR_INVALID_ARGUMENT;
    *out = st->capacity;
    return SBR_OK;
}

sbr_status sbr_sessions_seen_capacity(const sbr_sessions* st, uint32_t* out) {
    if (!st || !out) return SBR_ERR_INVALID_ARGUMENT;
    *out = st->seen.w;
    return SBR_OK;
}

sbr_status sbr_sessions_reset_all(sbr_sessions* st) {
    if (!st) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(st->m->mu);
    SBRCHK(enter_reader(st->m));
    if (st->m->open_plans) return SBR_ERR_INVALID_ARGUMENT; /* states bound now would go stale with the plan's next step */
    return sessions_rebind(st);
}

sbr_status sbr_sessions_reset(sbr_sessions* st, const uint32_t* slots, uint64_t n) {
    if (!st) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = st->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_sessions(st));
    SBRCHK(check_slots(st, slots, n));
    if (n == 0) return SBR_OK;
    uint32_t* d_slot = nullptr;
    SBRCHK(carve_arena(m, [&](DeviceArena& ar) { d_slot = ar.take<uint32_t>(n); }));
    HIPCHK(hipMemcpyAsync(d_slot, slots, n * 4, hipMemcpyHostToDevice, m->stream));
    sbr::launch_session_reset(st->v, d_slot, (int)n, m->d, m->stream);
    sbr::launch_session_seen_clear(st->seen, d_slot, (int)n, m->stream); /* nothing without memory */
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(m->stream));
    for (uint64_t i = 0; i < n; ++i) st->host_len[slots[i]] = 0;
    return SBR_OK;
}

sbr_status sbr_sessions_append(sbr_sessions* st, const uint32_t* slots, uint64_t n, const uint64_t* item_ptr, const uint32_t* item_ids) {
    if (!st || !item_ptr) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(st->m->mu);
    SBRCHK(enter_sessions(st));
    SBRCHK(check_slots(st, slots, n));
    SBRCHK(check_csr(st->m, item_ptr, n, item_ids, false));
    return sessions_append(st, slots, n, item_ptr, item_ids, 1);
}

sbr_status sbr_sessions_lengths(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint64_t* out_lengths) {
    if (!st || (n && !out_lengths)) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(st->m->mu);
    SBRCHK(enter_sessions(st));
    SBRCHK(check_slots(st, slots, n));
    for (uint64_t i = 0; i < n; ++i) out_lengths[i] = st->host_len[slots[i]]; /* the host's copy is exact; get_state reads the device's */
    return SBR_OK;
}

sbr_status sbr_sessions_representations(sbr_sessions* st, const uint32_t* slots, uint64_t n, float* out_reps) {
    if (!st || (n && !out_reps)) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(st->m->mu);
    SBRCHK(enter_sessions(st));
    SBRCHK(check_slots(st, slots, n));
    const std::vector<int> rows = session_rep_rows(st, slots, n);
    return sessions_gather(st, reinterpret_cast<const uint32_t*>(rows.data()), n, out_reps, nullptr, nullptr);
}

sbr_status sbr_sessions_get_state(sbr_sessions* st, const uint32_t* slots, uint64_t n, float* out_h, float* out_c, uint64_t* out_len) {
    if (!st || (n && (!out_h || !out_len))) return SBR_ERR_INVALID_ARGUMENT;
    if (n && (out_c != nullptr) != (st->m->ng != 0)) return SBR_ERR_INVALID_ARGUMENT; /* c: the LSTM's, NULL for EWMA */
    std::lock_guard<std::mutex> lock(st->m->mu);
    SBRCHK(enter_sessions(st));
    SBRCHK(check_slots(st, slots, n));
    return sessions_gather(st, slots, n, out_h, out_c, out_len);
}

sbr_status sbr_sessions_set_state(sbr_sessions* st, const uint32_t* slots, uint64_t n, const float* h, const float* c, const uint64_t* len) {
    if (!st || (n && (!h || !len))) return SBR_ERR_INVALID_ARGUMENT;
    if (n && (c != nullptr) != (st->m->ng != 0)) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = st->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_sessions(st));
    SBRCHK(check_slots(st, slots, n));
    if (n == 0) return SBR_OK;
    const size_t dl = (size_t)m->dl;
    uint32_t* d_slot = nullptr;
    float *d_h = nullptr, *d_c = nullptr;
    unsigned long long* d_len = nullptr;
    SBRCHK(carve_arena(m, [&](DeviceArena& ar) {
        d_slot = ar.take<uint32_t>(n);
        d_h = ar.take<float>(n * dl);
        if (c) d_c = ar.take<float>(n * dl);
        d_len = ar.take<unsigned long long>(n);
    }));
    HIPCHK(hipMemcpyAsync(d_slot, slots, n * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(d_h, h, n * dl * 4, hipMemcpyHostToDevice, m->stream));
    if (c) HIPCHK(hipMemcpyAsync(d_c, c, n * dl * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(d_len, len, n * 8, hipMemcpyHostToDevice, m->stream));
    sbr::launch_session_set_state(st->v, d_slot, (int)n, m->d, m->dl, d_h, d_c, d_len, m->stream);
    sbr::launch_session_seen_clear(st->seen, d_slot, (int)n, m->stream); /* the restored state's items are unknown: set_seen follows */
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(m->stream));
    for (uint64_t i = 0; i < n; ++i) st->host_len[slots[i]] = len[i];
    return SBR_OK;
}

/* slot slots[i]'s remembered items, oldest first: out_items[out_ptr[i] .. out_ptr[i + 1]) */
sbr_status sbr_sessions_get_seen(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint64_t* out_ptr, uint32_t* out_items) {
    if (!st || !out_ptr || (n && !out_items) || !st->seen.w) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = st->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_sessions(st));
    SBRCHK(check_slots(st, slots, n));
    out_ptr[0] = 0;
    if (n == 0) return SBR_OK;
    const size_t w = st->seen.w;
    uint32_t *d_slot = nullptr, *d_n = nullptr, *d_items = nullptr;
    SBRCHK(carve_arena(m, [&](DeviceArena& ar) {
        d_slot = ar.take<uint32_t>(n);
        d_n = ar.take<uint32_t>(n);
        d_items = ar.take<uint32_t>(n * w);
    }));
    HIPCHK(hipMemcpyAsync(d_slot, slots, n * 4, hipMemcpyHostToDevice, m->stream));
    sbr::launch_session_seen_get(st->seen, d_slot, (int)n, d_n, d_items, m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(m->stream));
    std::vector<uint32_t> count(n), padded(n * w);
    HIPCHK(hipMemcpy(count.data(), d_n, n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(padded.data(), d_items, n * w * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n; ++i) { /* the device's rows of w, closed up */
        std::memcpy(out_items + out_ptr[i], padded.data() + i * w, (size_t)count[i] * 4);
        out_ptr[i + 1] = out_ptr[i] + count[i];
    }
    return SBR_OK;
}

sbr_status sbr_sessions_set_seen(sbr_sessions* st, const uint32_t* slots, uint64_t n, const uint64_t* ptr, const uint32_t* items) {
    if (!st || !ptr || !st->seen.w) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = st->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_sessions(st));
    SBRCHK(check_slots(st, slots, n));
    SBRCHK(check_csr(m, ptr, n, items, false));
    if (n == 0) return SBR_OK;
    const size_t total = (size_t)(ptr[n] - ptr[0]);
    uint32_t *d_slot = nullptr, *d_ids = nullptr;
    uint64_t* d_ptr = nullptr;
    SBRCHK(carve_arena(m, [&](DeviceArena& ar) {
        d_slot = ar.take<uint32_t>(n);
        d_ptr = ar.take<uint64_t>(n + 1);
        d_ids = ar.take<uint32_t>(total + 1);
    }));
    HIPCHK(hipMemcpyAsync(d_slot, slots, n * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(d_ptr, ptr, (n + 1) * 8, hipMemcpyHostToDevice, m->stream));
    if (total) HIPCHK(hipMemcpyAsync(d_ids, items + ptr[0], total * 4, hipMemcpyHostToDevice, m->stream));
    sbr::launch_session_seen_set(st->seen, d_slot, (int)n, d_ptr, d_ids, m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(m->stream));
    return SBR_OK;
}

/* States recomputed from the seen-item memories under the model's current parameters (REPLAY, include/sbr_hip.h).  Of the memory
 * the host reads cnt alone; the rings feed the step kernels on the device. */
sbr_status sbr_sessions_replay(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint64_t* out_replayed) {
    if (!st || !st->seen.w) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = st->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    if (m->open_plans) return SBR_ERR_INVALID_ARGUMENT; /* states bound now would go stale with the plan's next step */
    const bool whole = slots == nullptr;
    std::vector<uint32_t> named; /* the subset form's slots, each once */
    if (!whole) {
        if (st->gen != m->param_gen) return SBR_ERR_INVALID_ARGUMENT; /* the slots not named would keep states of other parameters */
        for (uint64_t i = 0; i < n; ++i)
            if (slots[i] >= st->capacity) return SBR_ERR_INVALID_ARGUMENT;
        named.assign(slots, slots + n);
        std::sort(named.begin(), named.end());
        named.erase(std::unique(named.begin(), named.end()), named.end());
    }
    const size_t ns = whole ? (size_t)st->capacity : named.size();
    if (out_replayed) *out_replayed = 0;
    if (ns == 0) return SBR_OK;
    std::vector<unsigned long long> cnt(ns);
    uint32_t* d_slot = nullptr;
    HIPCHK(hipStreamSynchronize(m->stream));
    if (whole) {
        HIPCHK(hipMemcpy(cnt.data(), st->seen.cnt, ns * 8, hipMemcpyDeviceToHost));
    } else {
        unsigned long long* d_cnt = nullptr;
        SBRCHK(carve_arena(m, [&](DeviceArena& ar) { d_slot = ar.take<uint32_t>(ns); d_cnt = ar.take<unsigned long long>(ns); }));
        HIPCHK(hipMemcpyAsync(d_slot, named.data(), ns * 4, hipMemcpyHostToDevice, m->stream));
        sbr::launch_session_seen_counts(st->seen, d_slot, (int)ns, d_cnt, m->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(m->stream));
        HIPCHK(hipMemcpy(cnt.data(), d_cnt, ns * 8, hipMemcpyDeviceToHost));
    }
    sbr::ReplayPlan plan;
    sbr::plan_replay(whole ? nullptr : named.data(), cnt.data(), ns, st->seen.w, replay_chunk_cap(m, st->seen.w), &plan);
    if (whole) { /* sessions_rebind without its cnt = 0: every state and length zero, the empty-history row of the current parameters */
        const size_t rows = (size_t)st->capacity + 1, d = (size_t)m->d;
        HIPCHK(hipMemsetAsync(st->v.H, 0, rows * d * 4, m->stream));
        if (st->v.C) HIPCHK(hipMemsetAsync(st->v.C, 0, rows * d * 4, m->stream));
        HIPCHK(hipMemsetAsync(st->v.len, 0, rows * 8, m->stream));
        std::fill(st->host_len.begin(), st->host_len.end(), 0);
        const uint32_t row = (uint32_t)st->capacity, item0 = 0;
        const uint64_t ptr[2] = {0, 1};
        SBRCHK(sessions_append(st, &row, 1, ptr, &item0, 0));
    } else { /* d_slot is still the arena's: nothing has carved it since */
        sbr::launch_session_reset(st->v, d_slot, (int)ns, m->d, m->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(m->stream));
        for (uint32_t s : named) st->host_len[s] = 0;
    }
    for (const sbr::ReplayChunk& ch : plan.chunks) SBRCHK(sessions_replay_chunk(st, plan, ch));
    if (whole) st->gen = m->param_gen;
    if (out_replayed) *out_replayed = plan.slot.size();
    return SBR_OK;
}

namespace {

RepSource RepSource::of_sessions(const sbr_sessions* st, const std::vector<int>& rows, const uint64_t* excl_ptr, const uint32_t* excl_items,
                                 const uint32_t* seen_slots) {
    RepSource s;
    s.ptr = excl_ptr; s.items = excl_items; s.dev_rows = st->v.H; s.dev_row = rows.data();
    if (seen_slots) { s.seen = &st->seen; s.seen_slots = seen_slots; }
    return s;
}

/* What a scan call has entered once it may read its rows: the model's mutex, held until the call ends, and of a store's slots the
 * rows of the store they read (session_rep_rows), which outlive the scan. */
struct ScanEntry {
    std::lock_guard<std::mutex> lock;
    std::vector<int> rows;
    explicit ScanEntry(sbr_model* m) : lock(m->mu) {}
    /* the set's entry (null: the catalogue), then the store's or the reader's, then the slots, then the lists: the order of refusal
     * of every scan; `st` is r's store (null: another source) */
    sbr_status enter(sbr_model* m, const sbr_item_set* set, sbr_sessions* st, const ScanRows& r, uint64_t n) {
        if (set) SBRCHK(enter_item_set(set));
        if (st) SBRCHK(enter_sessions(st));
        else if (!set) SBRCHK(enter_reader(m)); /* a set's entry is the reader's already */
        if (st) SBRCHK(check_slots(st, r.slots, n));
        if (r.kind == ScanRows::Histories) SBRCHK(check_csr(m, r.user_ptr, n, r.item_ids, false));
        else if (r.excl_ptr) SBRCHK(check_csr(m, r.excl_ptr, n, r.excl_items, false));
        if (st) rows = session_rep_rows(st, r.slots, n);
        return SBR_OK;
    }
};

sbr_model* model_of(const sbr_sessions* st) { return st ? st->m : nullptr; } /* a null store is scan_call's to refuse */

/* a store with memory takes sbr_recommend's flag, which ignores the memory for the call; one without refuses every flag */
bool store_flags_ok(const sbr_sessions* st, uint32_t flags) {
    return st->seen.w ? (flags & ~SBR_RECOMMEND_INCLUDE_HISTORY) == 0 : flags == 0;
}

/* Every call of the scan families, on the model (set null) or through an item set of it.  First what needs no device, so that a
 * machine without one still answers SBR_ERR_INVALID_ARGUMENT and writes nothing; then ScanEntry's sequence under the model's
 * mutex; then recommend_scan, whose own checks (tags or groups not set, ...) come last.  After success, and only then, the
 * threshold and budget forms' *out_total and log_partition's *out_frac_bits — the model's F, with or without a set. */
sbr_status scan_call(sbr_model* m, const sbr_item_set* set, const ScanRows& r, uint64_t n, uint32_t k, uint32_t* out_items, float* out_scores,
                     ScanVariant v) {
    if (!m || (n && !out_items && !v.pt && !v.ab && !v.rk) || !scan_k_ok(m, k, v.dv, v.cp)) return SBR_ERR_INVALID_ARGUMENT;
    sbr_sessions* st = nullptr;
    switch (r.kind) {
    case ScanRows::Histories:
        if (!r.user_ptr || (r.flags & ~SBR_RECOMMEND_INCLUDE_HISTORY)) return SBR_ERR_INVALID_ARGUMENT;
        break;
    case ScanRows::Reps:
        if (n && !r.reps) return SBR_ERR_INVALID_ARGUMENT;
        break;
    case ScanRows::Store:
        st = r.store;
        if (!st || st->m != m || !store_flags_ok(st, r.flags)) return SBR_ERR_INVALID_ARGUMENT;
        break;
    }
    if (r.kind != ScanRows::Histories && !excl_args_ok(r.excl_ptr, r.excl_items, n)) return SBR_ERR_INVALID_ARGUMENT;
    ScanEntry e(m);
    SBRCHK(e.enter(m, set, st, r, n));
    const bool include = (r.flags & SBR_RECOMMEND_INCLUDE_HISTORY) != 0;
    RepSource s;
    if (r.kind == ScanRows::Histories) s = RepSource::of_histories(r.user_ptr, r.item_ids, 0, !include); /* the WHOLE history is masked (evaluation.rs:30-32) */
    else if (r.kind == ScanRows::Reps) s = RepSource::of_rows(r.reps, r.excl_ptr, r.excl_items);
    else s = RepSource::of_sessions(st, e.rows, r.excl_ptr, r.excl_items, st->seen.w && !include ? r.slots : nullptr);
    if (st && v.sm) v.sm->fallback = r.slots; /* a session's default stream is its slot id */
    TagFilterArg hold;
    if (!v.flt) v.flt = sample_filter(r.any_of, r.none_of, &hold);
    v.set = set;
    SBRCHK(recommend_scan(m, s, n, k, out_items, out_scores, v));
    if (v.ab) *v.ab->out_total = v.ab->total;
    if (v.pt) *v.pt->out_frac_bits = sbr_softmax_fbits((uint32_t)m->hp.num_items);
    return SBR_OK;
}

}  // namespace

sbr_status sbr_sessions_recommend(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint32_t k, const uint64_t* excl_ptr,
                                  const uint32_t* excl_items, uint32_t flags, uint32_t* out_items, float* out_scores) {
    return scan_call(model_of(st), nullptr, ScanRows::of_store(st, slots, excl_ptr, excl_items, flags), n, k, out_items, out_scores,
                     ScanVariant());
}

sbr_status sbr_sessions_recommend_filtered(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint32_t k, const uint64_t* excl_ptr,
                                           const uint32_t* excl_items, uint32_t flags, const uint32_t* any_of, const uint32_t* none_of,
                                           uint32_t* out_items, float* out_scores) {
    const TagFilterArg flt{any_of, none_of};
    ScanVariant v;
    v.flt = &flt;
    return scan_call(model_of(st), nullptr, ScanRows::of_store(st, slots, excl_ptr, excl_items, flags), n, k, out_items, out_scores, v);
}

sbr_status sbr_sessions_recommend_sampled(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint32_t k, const uint64_t* excl_ptr,
                                          const uint32_t* excl_items, uint32_t flags, const struct sbr_sample_args* sample,
                                          const uint32_t* any_of, const uint32_t* none_of, uint32_t* out_items, float* out_scores,
                                          float* out_keys) {
    Sample sm;
    if (!sample_args(sample, out_keys, &sm)) return SBR_ERR_INVALID_ARGUMENT;
    ScanVariant v;
    v.sm = &sm;
    return scan_call(model_of(st), nullptr, ScanRows::of_store(st, slots, excl_ptr, excl_items, flags, any_of, none_of), n, k, out_items, out_scores, v);
}

sbr_status sbr_sessions_log_partition(sbr_sessions* st, const uint32_t* slots, uint64_t n, const uint64_t* excl_ptr, const uint32_t* excl_items,
                                      uint32_t flags, float temperature, const uint32_t* any_of, const uint32_t* none_of, float* out_shift,
                                      uint64_t* out_mass, uint32_t* out_frac_bits) {
    Partition pt;
    if (!partition_args(temperature, n, out_shift, out_mass, out_frac_bits, &pt)) return SBR_ERR_INVALID_ARGUMENT;
    ScanVariant v;
    v.pt = &pt;
    return scan_call(model_of(st), nullptr, ScanRows::of_store(st, slots, excl_ptr, excl_items, flags, any_of, none_of), n, 1, nullptr, nullptr, v);
}

sbr_status sbr_sessions_recommend_above(sbr_sessions* st, const uint32_t* slots, uint64_t n, const float* thresholds, const uint64_t* excl_ptr,
                                        const uint32_t* excl_items, uint32_t flags, const uint32_t* any_of, const uint32_t* none_of,
                                        uint64_t* out_counts, uint64_t* out_total, uint64_t capacity, uint32_t* out_ids, float* out_scores) {
    Above ab;
    if (!above_args(thresholds, n, out_counts, out_total, capacity, out_ids, out_scores, &ab)) return SBR_ERR_INVALID_ARGUMENT;
    ScanVariant v;
    v.ab = &ab;
    return scan_call(model_of(st), nullptr, ScanRows::of_store(st, slots, excl_ptr, excl_items, flags, any_of, none_of), n, 1, nullptr, nullptr, v);
}

sbr_status sbr_sessions_recommend_top(sbr_sessions* st, const uint32_t* slots, uint64_t n, const uint64_t* top_n, const uint64_t* excl_ptr,
                                      const uint32_t* excl_items, uint32_t flags, const uint32_t* any_of, const uint32_t* none_of, float* out_cuts,
                                      uint64_t* out_counts, uint64_t* out_total, uint64_t capacity, uint32_t* out_ids, float* out_scores) {
    Above ab;
    if (!top_args(top_n, n, out_cuts, out_counts, out_total, capacity, out_ids, out_scores, &ab)) return SBR_ERR_INVALID_ARGUMENT;
    ScanVariant v;
    v.ab = &ab;
    return scan_call(model_of(st), nullptr, ScanRows::of_store(st, slots, excl_ptr, excl_items, flags, any_of, none_of), n, 1, nullptr, nullptr, v);
}

sbr_status sbr_sessions_recommend_capped(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint32_t k, const uint64_t* excl_ptr,
                                         const uint32_t* excl_items, uint32_t flags, const struct sbr_cap_args* cap, const uint32_t* any_of,
                                         const uint32_t* none_of, uint32_t* out_items, float* out_scores, uint8_t* out_complete) {
    Capped cp;
    uint32_t pool = 0;
    if (!capped_args(cap, k, out_complete, &cp, &pool)) return SBR_ERR_INVALID_ARGUMENT;
    ScanVariant v;
    v.cp = &cp;
    return scan_call(model_of(st), nullptr, ScanRows::of_store(st, slots, excl_ptr, excl_items, flags, any_of, none_of), n, pool, out_items, out_scores, v);
}

sbr_status sbr_sessions_recommend_diverse(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint32_t k, uint32_t pool, float trade_off,
                                          uint32_t metric, const uint64_t* excl_ptr, const uint32_t* excl_items, uint32_t* out_items,
                                          float* out_scores) {
    const Diverse dv{k, trade_off, metric};
    ScanVariant v;
    v.dv = &dv;
    return scan_call(model_of(st), nullptr, ScanRows::of_store(st, slots, excl_ptr, excl_items, 0), n, pool, out_items, out_scores, v);
}

sbr_status sbr_sessions_recommend_diverse_filtered(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint32_t k, uint32_t pool,
                                                   float trade_off, uint32_t metric, const uint64_t* excl_ptr, const uint32_t* excl_items,
                                                   const uint32_t* any_of, const uint32_t* none_of, uint32_t* out_items, float* out_scores) {
    const TagFilterArg flt{any_of, none_of};
    const Diverse dv{k, trade_off, metric};
    ScanVariant v;
    v.dv = &dv;
    v.flt = &flt;
    return scan_call(model_of(st), nullptr, ScanRows::of_store(st, slots, excl_ptr, excl_items, 0), n, pool, out_items, out_scores, v);
}

/* ---------------------------------------------------------------------------------------------
 * rollout: a session's next items, picked and fed back on the device (ROLLOUT in include/sbr_hip.h)
 * ------------------------------------------------------------------------------------------- */
namespace {

/* What a rollout and a beam-search call share: the store's rows (slots, their optional lists, rep0 = session_rep_rows), the set
 * (null: the catalogue), and what steps_call makes of the args' steps, flags and masks. */
struct StepsCall {
    const sbr_item_set* set;
    const uint32_t* slots;
    const uint64_t* excl_ptr;
    const uint32_t* excl_items;
    const std::vector<int>* rep0;
    uint32_t steps, w;       /* w: the beam width; a rollout's 1 */
    bool allow_repeats, seen;
    const TagFilterArg* flt; /* null: no filter */
    float inv_t;             /* the partition's */
};

/* The half of a chunk the two share — rows [c0, c0 + nu) of the call, `nrows` of them on the device (a rollout's nu, a beam
 * search's nu W): the caller's lists, the tight exclusion CSR `src` (the seen lists merged with the caller's, as positions of the
 * set) that the steps' own segments are spread from, the slots, the identity rows of the scratch states, the set's tag words, and
 * the tail.  What differs — the scan's buffers, the rows' records and the per-step loop — stays with the two chunk functions. */
struct StepsChunk {
    sbr_sessions* st;
    sbr_model* m;
    const StepsCall& sc;
    const SetView sv;
    const size_t c0, nu, nrows, seen_w;
    const uint32_t slack;  /* room per row for the picks to come, which the steps exclude unless repeats are allowed */
    UserBatch ub;          /* the caller's lists of the chunk's rows, sorted and de-duplicated */
    size_t ncaller = 0, nsrc = 0;
    bool excl = false;     /* without lists, memory or slack nothing is ever excluded */
    uint64_t* src_ptr = nullptr;
    uint32_t *src = nullptr, *seen_caller = nullptr, *d_slot = nullptr, *d_ident = nullptr, *set_tags = nullptr;
    unsigned long long* d_start = nullptr;
    /* read by asynchronous copies: they live until finish() has drained the stream */
    std::vector<uint64_t> h_src_ptr;
    std::vector<uint32_t> h_ident, masks, masks_rows;
    std::vector<unsigned long long> h_start;

    StepsChunk(sbr_sessions* st_, const StepsCall& sc_, size_t c0_, size_t nu_, size_t nrows_)
        : st(st_), m(st_->m), sc(sc_), sv(st_->m, sc_.set), c0(c0_), nu(nu_), nrows(nrows_), seen_w(sc_.seen ? st_->seen.w : 0),
          slack(sc_.allow_repeats ? 0u : sc_.steps) {
        if (sc.excl_ptr) {
            std::vector<const uint32_t*> list(nu);
            std::vector<uint64_t> n(nu);
            for (size_t i = 0; i < nu; ++i) {
                list[i] = sc.excl_items ? sc.excl_items + sc.excl_ptr[c0 + i] : nullptr;
                n[i] = sc.excl_ptr[c0 + i + 1] - sc.excl_ptr[c0 + i];
            }
            prepare_users(list, n, m->hp.max_sequence_length, true, &ub);
        }
        ncaller = ub.list_items.size();
        nsrc = nu * seen_w + ncaller;
        excl = sc.excl_ptr || seen_w || slack;
    }
    const uint32_t* tags() const { return !sc.flt ? nullptr : sc.set ? set_tags : m->item_tags; }
    void carve(DeviceArena& ar) {
        if (sc.set && sc.flt) set_tags = ar.take<uint32_t>(sv.scanned);
        src_ptr = ar.take<uint64_t>(nu + 1);
        src = ar.take<uint32_t>(nsrc + 1);
        if (seen_w) seen_caller = ar.take<uint32_t>(ncaller + 1);
        d_slot = ar.take<uint32_t>(nu);
        d_ident = ar.take<uint32_t>(nrows);
        d_start = ar.take<unsigned long long>(nrows);
    }
    /* the uploads: the rows' representations' rows to d_rep, the slots, the identities and the tight CSR */
    sbr_status upload(int* d_rep) {
        h_src_ptr.resize(nu + 1);
        h_ident.resize(nrows);
        h_start.resize(nrows);
        for (size_t i = 0; i <= nu; ++i) h_src_ptr[i] = i * seen_w + (ub.list_ptr.empty() ? 0 : ub.list_ptr[i]);
        for (size_t i = 0; i < nrows; ++i) { h_ident[i] = (uint32_t)i; h_start[i] = i; }
        HIPCHK(hipMemcpyAsync(d_rep, sc.rep0->data() + c0, nu * 4, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(d_slot, sc.slots + c0, nu * 4, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(d_ident, h_ident.data(), nrows * 4, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(d_start, h_start.data(), nrows * 8, hipMemcpyHostToDevice, m->stream));
        if (excl) SBRCHK(upload_csr(m, src_ptr, h_src_ptr, seen_w ? seen_caller : src, ub.list_items));
        return SBR_OK;
    }
    /* what runs ahead of the steps' own segments: the seen lists, and for a set the lists as positions and its tag words */
    int prelaunch() {
        int n = seen_w ? sbr::launch_session_seen_lists(st->seen, d_slot, (int)nu, src_ptr, seen_caller, src, m->stream) : 0;
        if (sc.set && !sv.none && nsrc) n += sbr::launch_subset_positions(sc.set->d_ids, sv.ns, src_ptr, (uint32_t)nu, src, m->stream);
        if (set_tags && !sv.none) n += sbr::launch_subset_words(sc.set->d_ids, sv.ns, m->item_tags, set_tags, m->stream);
        return n;
    }
    /* the tail, as scan_launch's: the stream drained, the flag — a non-finite score at any step fails the whole call — and the results */
    sbr_status finish(const uint32_t* d_flag, std::initializer_list<CopyOut> outs) {
        HIPCHK(hipGetLastError());
        uint32_t flag = 0;
        HIPCHK(hipStreamSynchronize(m->stream));
        HIPCHK(hipMemcpy(&flag, d_flag, 4, hipMemcpyDeviceToHost));
        if (flag) return SBR_ERR_INVALID_PREDICTION;
        for (const CopyOut& o : outs)
            if (o.host) HIPCHK(hipMemcpy(o.host, o.device, o.bytes, hipMemcpyDeviceToHost));
        return SBR_OK;
    }
};

/* what a rollout call asks for beside StepsCall; the outputs are host arrays over the call's rows, null: not wanted */
struct RolloutCall : StepsCall {
    const Sample* sm;        /* null: greedy; inv_t = sm->inv_t in sample mode */
    uint32_t* out_items;
    float *out_scores, *out_keys;
    uint32_t* out_lengths;
    float* out_shift;        /* non-null: the partition per step, with out_mass */
    uint64_t* out_mass;
    float *out_h, *out_c;
};

/* Sessions per rollout chunk: the scan's bound (recommend_users_cap at k = 1), and few enough that a row's share of the arena — its
 * exclusion segment with the slack, twice (the tight lists it is spread from), its columns of the outputs and its scratch state —
 * keeps the chunk within 256 MB.  SBR_ROLLOUT_CHUNK=n (n >= 1) is a TEST HOOK read per call that replaces both, after
 * SBR_SESSIONS_REPLAY_CHUNK. */
size_t rollout_chunk_cap(const sbr_model* m, uint32_t w, uint32_t /* beam width */, uint32_t steps) {
    constexpr size_t budget = (size_t)256 << 20;
    const size_t per = ((size_t)w + steps) * 8 + (size_t)steps * 24 + (size_t)m->d * 16 + 64;
    return chunk_override("SBR_ROLLOUT_CHUNK", std::min(recommend_users_cap((uint32_t)m->hp.num_items, 1), std::max<size_t>(budget / per, 1)));
}

/* One chunk, rows [c0, c0 + nu) of the call: the scratch state and the exclusion CSR with slack, then per step the unchanged k = 1
 * scan (and the partition on the same descriptor), rollout_advance_kernel and one cell step — all queued without a synchronisation —
 * and at the end one flag check and the copies out, as scan_launch does.
 * With `set` (current; null: the catalogue) the scans run over its sub-table as recommend_scan's do: the tight exclusion CSR becomes
 * positions of the set before it is spread, the set's tag words are gathered once per chunk, F is the model's and the noise is
 * hashed from the catalogue ids; the advance turns the picks into ids.  An empty set runs no scan: every pick is padding. */
sbr_status sessions_rollout_chunk(sbr_sessions* st, const StepsCall& call, size_t c0, size_t nu) {
    const RolloutCall& rc = static_cast<const RolloutCall&>(call);
    sbr_model* m = st->m;
    StepsChunk f(st, rc, c0, nu, nu);
    const sbr_item_set* set = rc.set;
    const sbr::ModelView& cat = f.sv.cat; /* what the scans read */
    const bool none = f.sv.none, excl = f.excl;
    const uint32_t slack = f.slack;
    const size_t d = (size_t)m->d, dl = (size_t)m->dl, S = rc.steps;
    const bool lstm = m->ng != 0, sample = rc.sm != nullptr, part = rc.out_shift != nullptr;
    const bool final_state = rc.out_h != nullptr;
    TopkBufs tb;
    SampleBufs smb{};
    sbr::RolloutRows rr{};
    sbr::RolloutOut ro{};
    uint32_t* pt_items = nullptr;
    float *pt_scores = nullptr, *pt_shift = nullptr, *fin_h = nullptr, *fin_c = nullptr;
    unsigned long long* pt_mass = nullptr;
    SBRCHK(carve_arena(m, [&](DeviceArena& ar) {
        tb.carve(ar, f.sv.scanned, nu, f.nsrc + nu * slack, 1, rc.flt != nullptr);
        f.carve(ar);
        rr.Hs = ar.take<float>((lstm ? 2 : 1) * nu * d);
        if (lstm) rr.Cs = ar.take<float>(2 * nu * d);
        rr.len = ar.take<unsigned long long>(nu);
        rr.feed = ar.take<uint32_t>(nu);
        rr.count = ar.take<uint32_t>(nu);
        rr.ended = ar.take<uint32_t>(nu);
        rr.lengths = ar.take<uint32_t>(nu);
        if (sample) smb.carve(ar, nu, 1);
        if (part) {
            pt_mass = ar.take<unsigned long long>(nu);
            pt_shift = ar.take<float>(nu);
            ro.mass = ar.take<unsigned long long>(nu * S);
            ro.shift = ar.take<float>(nu * S);
            if (sample) { pt_items = ar.take<uint32_t>(nu); pt_scores = ar.take<float>(nu); }
        }
        ro.items = ar.take<uint32_t>(nu * S);
        ro.scores = ar.take<float>(nu * S);
        if (sample) ro.keys = ar.take<float>(nu * S);
        if (final_state) {
            fin_h = ar.take<float>(nu * dl);
            if (lstm) fin_c = ar.take<float>(nu * dl);
        }
    }));
    /* the host vectors below are read by asynchronous copies: they live until the stream is drained at the end */
    SBRCHK(f.upload(tb.rep));
    std::vector<uint64_t> h_eptr(nu + 1), streams;
    if (excl) { /* each row's tight list and its slack */
        for (size_t i = 0; i <= nu; ++i) h_eptr[i] = f.h_src_ptr[i] + i * slack;
        HIPCHK(hipMemcpyAsync(tb.eptr, h_eptr.data(), (nu + 1) * 8, hipMemcpyHostToDevice, m->stream));
    }
    if (rc.flt) SBRCHK(upload_masks(m, *rc.flt, nullptr, c0, nu, 1, tb.any_of, tb.none_of, &f.masks));
    if (sample) {
        streams.resize(nu);
        for (size_t i = 0; i < nu; ++i) streams[i] = rc.sm->streams ? rc.sm->streams[c0 + i] : (uint64_t)rc.slots[c0 + i];
        HIPCHK(hipMemcpyAsync(smb.streams, streams.data(), nu * 8, hipMemcpyHostToDevice, m->stream));
    }
    rr.n = (int)nu; rr.steps = rc.steps;
    rr.slot = f.d_slot; rr.ident = f.d_ident; rr.start = f.d_start;
    /* the step's scan: the pick's descriptor, and with the partition in sample mode a second one whose k = 1 scan is the plain one */
    sbr::TopkScan sc = tb.scan(nu, 1, excl, true, f.tags());
    sbr::TopkScan sc_pt = sc;
    if (sample) {
        sc.g = sbr::SampleNoise{rc.sm->inv_t, smb.keys};
        sc_pt.out_items = pt_items;
        sc_pt.out_scores = pt_scores;
    }
    /* a set's picks leave as ids: the plain scan's are positions, the sampled launch's already ids */
    const sbr::RolloutPick pick{tb.items, sample ? smb.plain : tb.scores, sample ? tb.scores : nullptr, pt_shift, pt_mass,
                                none ? nullptr : set ? set->d_ids : nullptr, f.sv.ns, sample};
    const size_t parity_stride = nu * d;
    HIPCHK(hipMemsetAsync(tb.flag, 0, 4, m->stream));
    if (none) HIPCHK(hipMemsetAsync(tb.items, 0xFF, nu * 4, m->stream)); /* nothing to scan: every step's pick is padding */
    {
        ScopedTimer t(m, SBR_K_RANK, 0);
        int n = sbr::launch_rollout_begin(m->mv, st->v, rr, m->stream) + f.prelaunch();
        if (excl) n += sbr::launch_rollout_segments(f.src_ptr, f.src, (int)nu, slack, tb.excl, m->stream);
        t.tp.launches = (uint64_t)n;
    }
    for (uint32_t j = 0; j < rc.steps; ++j) {
        /* step 0 scans the store's rows in place (an empty slot: the empty-history row); later steps the scratch the step before wrote */
        const float* reps = j == 0 ? st->v.H : lstm ? rr.Hs + (size_t)((j - 1) & 1u) * parity_stride : rr.Hs;
        sc.rep_row = sc_pt.rep_row = j == 0 ? tb.rep : reinterpret_cast<const int*>(f.d_ident);
        {
            ScopedTimer t(m, SBR_K_RANK, 0);
            int n = 0;
            if (!none) { /* a set's mass is held to the model's F, and its noise to the catalogue ids */
                const uint32_t f_items = set ? (uint32_t)m->hp.num_items : 0u;
                if (sample)
                    n += sbr::launch_recommend_sampled(cat, reps, sc, sbr::SampleScan{rc.sm->seed + (uint64_t)j, smb.streams, smb.pair_row,
                                                                                     smb.pair_item, smb.plain, set ? set->d_ids : nullptr}, m->stream);
                if (part) n += sbr::launch_log_partition(cat, reps, sc_pt, sbr::PartitionScan{rc.inv_t, pt_shift, pt_mass, f_items}, m->stream);
                else if (!sample) n += sbr::launch_recommend(cat, reps, sc, m->stream);
            }
            n += sbr::launch_rollout_advance(rr, j, pick, slack ? tb.eptr : nullptr, tb.excl, ro, m->stream);
            t.tp.launches = (uint64_t)n;
        }
        if (j + 1 == rc.steps && !final_state) break; /* nobody reads the state after the last pick */
        ScopedTimer t(m, SBR_K_RECURRENT_FWD, lstm ? 2 : 1);
        if (sbr::launch_rollout_step(m->mv, st->v, rr, j, m->stream) < 0) return SBR_ERR_UNSUPPORTED;
    }
    if (final_state) { /* the first embedding_dim columns of the rows after the last step */
        const sbr::SessionView fin{lstm ? rr.Hs + (size_t)((rc.steps - 1) & 1u) * parity_stride : rr.Hs,
                                   lstm ? rr.Cs + (size_t)((rc.steps - 1) & 1u) * parity_stride : nullptr, nullptr};
        sbr::launch_session_get_state(fin, f.d_ident, (int)nu, m->d, m->dl, fin_h, fin_c, nullptr, m->stream);
    }
    return f.finish(tb.flag, {{rc.out_items + c0 * S, ro.items, nu * S * 4},
                              {rc.out_scores ? rc.out_scores + c0 * S : nullptr, ro.scores, nu * S * 4},
                              {rc.out_keys ? rc.out_keys + c0 * S : nullptr, ro.keys, nu * S * 4},
                              {rc.out_lengths ? rc.out_lengths + c0 : nullptr, rr.lengths, nu * 4},
                              {part ? rc.out_shift + c0 * S : nullptr, ro.shift, nu * S * 4},
                              {part ? rc.out_mass + c0 * S : nullptr, ro.mass, nu * S * 8},
                              {rc.out_h ? rc.out_h + c0 * dl : nullptr, fin_h, nu * dl * 4},
                              {rc.out_c ? rc.out_c + c0 * dl : nullptr, fin_c, nu * dl * 4}});
}

/* The entry rollout_call and beam_call share, behind their own argument checks (st and its call's set, slots and lists are the
 * caller's, checked non-null where they must be): the steps and the flag bits, include_seen without memory, the lists' pairing;
 * ScanEntry's sequence under the model's mutex; the filter, which needs the model's tags; then `chunk` over the rows, `cap` of them
 * at a time, and *out_frac_bits (null: not wanted) — the model's F, with or without a set. */
sbr_status steps_call(sbr_sessions* st, StepsCall* sc, uint64_t n, uint32_t steps, uint32_t flags, uint32_t known, const uint32_t* any_of,
                      const uint32_t* none_of, size_t (*cap)(const sbr_model*, uint32_t seen_w, uint32_t w, uint32_t steps),
                      sbr_status (*chunk)(sbr_sessions*, const StepsCall&, size_t c0, size_t nu), uint32_t* out_frac_bits) {
    if (steps < 1 || steps > SBR_ROLLOUT_MAX_STEPS || (flags & ~known)) return SBR_ERR_INVALID_ARGUMENT;
    if ((flags & SBR_ROLLOUT_INCLUDE_SEEN) && !st->seen.w) return SBR_ERR_INVALID_ARGUMENT; /* nothing to include */
    if (!excl_args_ok(sc->excl_ptr, sc->excl_items, n)) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = st->m;
    ScanEntry e(m);
    SBRCHK(e.enter(m, sc->set, st, ScanRows::of_store(st, sc->slots, sc->excl_ptr, sc->excl_items, 0), n));
    TagFilterArg hold;
    sc->flt = sample_filter(any_of, none_of, &hold);
    if (sc->flt && !m->item_tags) return SBR_ERR_INVALID_ARGUMENT;
    sc->rep0 = &e.rows;
    sc->steps = steps;
    sc->allow_repeats = (flags & SBR_ROLLOUT_ALLOW_REPEATS) != 0;
    sc->seen = st->seen.w && !(flags & SBR_ROLLOUT_INCLUDE_SEEN);
    const size_t per = cap(m, sc->seen ? st->seen.w : 0, sc->w, steps);
    for (size_t c0 = 0; c0 < n; c0 += per) SBRCHK(chunk(st, *sc, c0, std::min<size_t>(per, n - c0)));
    if (out_frac_bits) *out_frac_bits = sbr_softmax_fbits((uint32_t)m->hp.num_items);
    return SBR_OK;
}

/* sbr_sessions_rollout, or (set non-null: the caller checked that it is the store's model's) sbr_item_set_rollout */
sbr_status rollout_call(sbr_sessions* st, const sbr_item_set* set, const uint32_t* slots, uint64_t n, const struct sbr_rollout_args* args,
                        const uint64_t* excl_ptr, const uint32_t* excl_items, const uint32_t* any_of, const uint32_t* none_of,
                        uint32_t* out_items, float* out_scores, float* out_keys, uint32_t* out_lengths, float* out_shift,
                        uint64_t* out_mass, uint32_t* out_frac_bits, float* out_h, float* out_c) {
    if (!st || !args || (n && !out_items)) return SBR_ERR_INVALID_ARGUMENT;
    const bool sample = (args->flags & SBR_ROLLOUT_SAMPLE) != 0;
    Sample sm;
    if (!sample_args(&args->sample, out_keys, &sm)) return SBR_ERR_INVALID_ARGUMENT;
    if (!sample && out_keys) return SBR_ERR_INVALID_ARGUMENT; /* a greedy pick has no key */
    if ((out_shift != nullptr) != (out_mass != nullptr) || (out_shift && !out_frac_bits)) return SBR_ERR_INVALID_ARGUMENT;
    if (out_c && (!out_h || !st->m->ng)) return SBR_ERR_INVALID_ARGUMENT; /* c: the LSTM's, with h */
    if (out_h && st->m->ng && !out_c) return SBR_ERR_INVALID_ARGUMENT;
    RolloutCall rc{};
    rc.set = set; rc.slots = slots; rc.excl_ptr = excl_ptr; rc.excl_items = excl_items;
    rc.w = 1;
    rc.sm = sample ? &sm : nullptr;
    rc.inv_t = sm.inv_t;
    rc.out_items = out_items; rc.out_scores = out_scores; rc.out_keys = out_keys; rc.out_lengths = out_lengths;
    rc.out_shift = out_shift; rc.out_mass = out_mass; rc.out_h = out_h; rc.out_c = out_c;
    return steps_call(st, &rc, n, args->steps, args->flags, SBR_ROLLOUT_SAMPLE | SBR_ROLLOUT_ALLOW_REPEATS | SBR_ROLLOUT_INCLUDE_SEEN, any_of,
                      none_of, rollout_chunk_cap, sessions_rollout_chunk, out_frac_bits);
}

}  // namespace

sbr_status sbr_sessions_rollout(sbr_sessions* st, const uint32_t* slots, uint64_t n, const struct sbr_rollout_args* args,
                                const uint64_t* excl_ptr, const uint32_t* excl_items, const uint32_t* any_of, const uint32_t* none_of,
                                uint32_t* out_items, float* out_scores, float* out_keys, uint32_t* out_lengths, float* out_shift,
                                uint64_t* out_mass, uint32_t* out_frac_bits, float* out_h, float* out_c) {
    return rollout_call(st, nullptr, slots, n, args, excl_ptr, excl_items, any_of, none_of, out_items, out_scores, out_keys, out_lengths,
                        out_shift, out_mass, out_frac_bits, out_h, out_c);
}

/* ---------------------------------------------------------------------------------------------
 * beam search: the W most likely next-n continuations of a session, on the device (BEAM SEARCH in include/sbr_hip.h)
 * ------------------------------------------------------------------------------------------- */
namespace {

/* what a beam-search call asks for beside StepsCall; the outputs are host arrays over the call's rows, null: not wanted */
struct BeamCall : StepsCall {
    uint32_t* out_items;
    float *out_scores, *out_lp, *out_cum;
    uint32_t *out_lengths, *out_beams;
    float* out_shift; /* non-null: the partition per (beam, step), with out_mass */
    uint64_t* out_mass;
};

/* Sessions per beam chunk: the scan's bound on its rows (recommend_users_cap at k = W) over the chunk's n W beam rows, and few enough
 * that a row's share of the arena — per beam two state parities (h and c), two exclusion segments with one entry of slack per step,
 * the per-step record (32 B) and the outputs (24 B) per step, the scan's bookkeeping; and the row's tight list — keeps the chunk within
 * 256 MB.  SBR_BEAM_CHUNK=n (n >= 1) is a TEST HOOK read per call that replaces both. */
size_t sessions_beam_chunk(const sbr_model* m, uint32_t seen_w, uint32_t w, uint32_t steps) {
    constexpr size_t budget = (size_t)256 << 20;
    const size_t per = (size_t)w * (((size_t)seen_w + steps) * 8 + (size_t)steps * 56 + (size_t)m->d * 16 + 128) + (size_t)seen_w * 8 + 64;
    return chunk_override("SBR_BEAM_CHUNK", std::max<size_t>(std::min(recommend_users_cap((uint32_t)m->hp.num_items, w) / w, budget / per), 1));
}

/* One chunk, rows [c0, c0 + nu) of the call, nb = nu W beam rows: the tight exclusion lists and the segment CSR, then per step the
 * unchanged top-k scan at k = W with its partition (launch_topk_partition: n rows at step 0, nb after), beam_select_kernel, the
 * children's segments and one cell step — all queued without a synchronisation — and at the end the backtrack, one flag check and
 * the copies out.
 * With `set` (current; null: the catalogue) the scans run over its sub-table as recommend_scan's do: the tight lists become positions
 * of the set before any segment is made from them, the set's tag words are gathered once per chunk, F is the model's; the selection
 * feeds and records ids and merges positions.  An empty set runs no scan: every row ends at step 0. */
sbr_status sessions_beam_chunk_run(sbr_sessions* st, const StepsCall& call, size_t c0, size_t nu) {
    const BeamCall& bc = static_cast<const BeamCall&>(call);
    sbr_model* m = st->m;
    const size_t d = (size_t)m->d, S = bc.steps, W = bc.w, nb = nu * W;
    StepsChunk f(st, bc, c0, nu, nb);
    const sbr_item_set* set = bc.set;
    const uint32_t num_items = (uint32_t)m->hp.num_items, scanned = f.sv.scanned, slack = f.slack;
    const sbr::ModelView& cat = f.sv.cat; /* what the scans read */
    const bool none = f.sv.none, excl = f.excl;
    const bool lstm = m->ng != 0, part_out = bc.out_shift != nullptr;
    const size_t nseg = W * f.nsrc + nb * slack;
    uint32_t per = 0;
    const size_t nlist = std::max(nu * sbr::recommend_groups((uint32_t)nu, scanned, bc.w, &per),
                                  nb * sbr::recommend_groups((uint32_t)nb, scanned, bc.w, &per));
    int* d_rep = nullptr;
    uint2* lists = nullptr;
    uint32_t *lens = nullptr, *scan_items = nullptr, *flag = nullptr;
    uint32_t *any0 = nullptr, *none0 = nullptr, *anyb = nullptr, *noneb = nullptr;
    uint32_t* seg[2] = {nullptr, nullptr};
    uint64_t* seg_ptr = nullptr;
    unsigned long long* mass = nullptr;
    float *scan_scores = nullptr, *shift = nullptr;
    sbr::BeamRows br{};
    sbr::BeamRecord rec{};
    sbr::BeamOut bo{};
    SBRCHK(carve_arena(m, [&](DeviceArena& ar) {
        d_rep = ar.take<int>(nu);
        f.carve(ar);
        lists = ar.take<uint2>(nlist * W);
        lens = ar.take<uint32_t>(nlist);
        scan_items = ar.take<uint32_t>(nb * W);
        scan_scores = ar.take<float>(nb * W);
        flag = ar.take<uint32_t>(1);
        if (bc.flt) {
            any0 = ar.take<uint32_t>(nu);
            none0 = ar.take<uint32_t>(nu);
            anyb = ar.take<uint32_t>(nb);
            noneb = ar.take<uint32_t>(nb);
        }
        seg_ptr = ar.take<uint64_t>(nb + 1);
        seg[0] = ar.take<uint32_t>(nseg + 1);
        if (slack) seg[1] = ar.take<uint32_t>(nseg + 1);
        shift = ar.take<float>(nb);
        mass = ar.take<unsigned long long>(nb);
        br.row_ended = ar.take<uint32_t>(nu);
        br.lengths = ar.take<uint32_t>(nu);
        br.beams = ar.take<uint32_t>(nu);
        br.alive = ar.take<uint32_t>(nb);
        br.ended = ar.take<uint32_t>(nb);
        br.in_row = ar.take<uint32_t>(nb);
        br.src_row = ar.take<uint32_t>(nb);
        br.feed = ar.take<uint32_t>(nb);
        br.count = ar.take<uint32_t>(nb);
        br.pick = ar.take<uint32_t>(nb);
        br.cum = ar.take<float>(nb);
        br.Hs = ar.take<float>(2 * nb * d);
        if (lstm) br.Cs = ar.take<float>(2 * nb * d);
        else br.len = ar.take<unsigned long long>(2 * nb);
        rec.parent = ar.take<uint32_t>(S * nb);
        rec.item = ar.take<uint32_t>(S * nb);
        rec.score = ar.take<float>(S * nb);
        rec.lp = ar.take<float>(S * nb);
        rec.cum = ar.take<float>(S * nb);
        if (part_out) {
            rec.shift = ar.take<float>(S * nb);
            rec.mass = ar.take<unsigned long long>(S * nb);
            bo.shift = ar.take<float>(nb * S);
            bo.mass = ar.take<unsigned long long>(nb * S);
        }
        bo.items = ar.take<uint32_t>(nb * S);
        bo.scores = ar.take<float>(nb * S);
        bo.lp = ar.take<float>(nb * S);
        bo.cum = ar.take<float>(nb);
    }));
    /* the host vectors below are read by asynchronous copies: they live until the stream is drained at the end */
    SBRCHK(f.upload(d_rep));
    uint64_t* const src_ptr = f.src_ptr;
    uint32_t* const src = f.src;
    std::vector<uint64_t> h_seg_ptr(nb + 1, 0);
    if (excl) { /* every beam row's segment: its row's tight list and the slack */
        for (size_t b = 0; b < nb; ++b) h_seg_ptr[b + 1] = h_seg_ptr[b] + (f.h_src_ptr[b / W + 1] - f.h_src_ptr[b / W]) + slack;
        HIPCHK(hipMemcpyAsync(seg_ptr, h_seg_ptr.data(), (nb + 1) * 8, hipMemcpyHostToDevice, m->stream));
    }
    if (bc.flt) { /* step 0 scans the rows, the later steps their beams */
        SBRCHK(upload_masks(m, *bc.flt, nullptr, c0, nu, 1, any0, none0, &f.masks));
        SBRCHK(upload_masks(m, *bc.flt, nullptr, c0, nu, W, anyb, noneb, &f.masks_rows));
    }
    br.n = (int)nu; br.w = bc.w; br.steps = bc.steps;
    br.slot = f.d_slot; br.ident = f.d_ident; br.start = f.d_start;
    const uint32_t fb = sbr_softmax_fbits(num_items);
    const sbr::BeamScan bs{scan_items, scan_scores, shift, mass, bc.inv_t, fb, none ? nullptr : set ? set->d_ids : nullptr};
    const size_t parity_stride = nb * d;
    HIPCHK(hipMemsetAsync(flag, 0, 4, m->stream));
    if (none) HIPCHK(hipMemsetAsync(scan_items, 0xFF, nb * W * 4, m->stream)); /* nothing to scan: no parent has an offer */
    {
        ScopedTimer t(m, SBR_K_RANK, 0);
        int n = sbr::launch_beam_begin(br, m->stream) + f.prelaunch();
        if (excl && !slack) n += sbr::launch_beam_segments((int)nb, bc.w, src_ptr, src, nullptr, nullptr, seg_ptr, seg[0], m->stream);
        t.tp.launches = (uint64_t)n;
    }
    for (uint32_t j = 0; j < bc.steps; ++j) {
        /* step 0 scans the store's rows in place, one per row (an empty slot: the empty-history row); later steps the beam rows the
         * step before wrote, with their own segments */
        sbr::TopkScan sc{};
        sc.rep_row = j == 0 ? d_rep : reinterpret_cast<const int*>(f.d_ident);
        sc.n = (uint32_t)(j == 0 ? nu : nb);
        sc.k = bc.w;
        sc.excl_ptr = !excl ? nullptr : j == 0 ? src_ptr : seg_ptr;
        sc.excl_items = j == 0 ? src : seg[slack ? (j - 1) & 1u : 0];
        sc.lists = lists; sc.lens = lens; sc.out_items = scan_items; sc.out_scores = scan_scores;
        sc.nonfinite_flag = flag;
        sc.f = sbr::TagMasks{f.tags(), j == 0 ? any0 : anyb, j == 0 ? none0 : noneb};
        const float* reps = j == 0 ? st->v.H : br.Hs + (size_t)((j - 1) & 1u) * parity_stride;
        {
            ScopedTimer t(m, SBR_K_RANK, 0);
            /* a set's mass is held to the model's F */
            int n = none ? 0 : sbr::launch_topk_partition(cat, reps, sc, sbr::PartitionScan{bc.inv_t, shift, mass, set ? num_items : 0u}, m->stream);
            n += sbr::launch_beam_select(br, j, bs, rec, m->stream); /* the kernel indexes the record by step */
            if (j + 1 < bc.steps && slack)
                n += sbr::launch_beam_segments((int)nb, bc.w, j == 0 ? src_ptr : seg_ptr, j == 0 ? src : seg[(j - 1) & 1u], br.src_row, br.pick,
                                               seg_ptr, seg[j & 1u], m->stream);
            t.tp.launches = (uint64_t)n;
        }
        if (j + 1 == bc.steps) break; /* nobody reads the state after the last selection */
        ScopedTimer t(m, SBR_K_RECURRENT_FWD, lstm ? 2 : 1);
        if (sbr::launch_beam_step(m->mv, st->v, br, j, m->stream) < 0) return SBR_ERR_UNSUPPORTED;
    }
    {
        ScopedTimer t(m, SBR_K_RANK, 0);
        t.tp.launches = (uint64_t)sbr::launch_beam_backtrack(br, rec, bo, m->stream);
    }
    return f.finish(flag, {{bc.out_items + c0 * W * S, bo.items, nb * S * 4},
                           {bc.out_scores ? bc.out_scores + c0 * W * S : nullptr, bo.scores, nb * S * 4},
                           {bc.out_lp ? bc.out_lp + c0 * W * S : nullptr, bo.lp, nb * S * 4},
                           {bc.out_cum ? bc.out_cum + c0 * W : nullptr, bo.cum, nb * 4},
                           {bc.out_lengths ? bc.out_lengths + c0 : nullptr, br.lengths, nu * 4},
                           {bc.out_beams ? bc.out_beams + c0 : nullptr, br.beams, nu * 4},
                           {part_out ? bc.out_shift + c0 * W * S : nullptr, bo.shift, nb * S * 4},
                           {part_out ? bc.out_mass + c0 * W * S : nullptr, bo.mass, nb * S * 8}});
}

/* sbr_sessions_beam_search, or (set non-null: the caller checked that it is the store's model's) sbr_item_set_beam_search */
sbr_status beam_call(sbr_sessions* st, const sbr_item_set* set, const uint32_t* slots, uint64_t n, const struct sbr_beam_args* args,
                     const uint64_t* excl_ptr, const uint32_t* excl_items, const uint32_t* any_of, const uint32_t* none_of,
                     uint32_t* out_items, float* out_scores, float* out_step_lp, float* out_cum, uint32_t* out_lengths,
                     uint32_t* out_beams, float* out_shift, uint64_t* out_mass, uint32_t* out_frac_bits) {
    if (!st || !args || (n && !out_items)) return SBR_ERR_INVALID_ARGUMENT;
    if (args->width < 1 || args->width > SBR_BEAM_MAX_WIDTH) return SBR_ERR_INVALID_ARGUMENT;
    sbr_sample_args sa{};
    sa.temperature = args->temperature;
    Sample sm;
    if (!sample_args(&sa, nullptr, &sm)) return SBR_ERR_INVALID_ARGUMENT;
    if ((out_shift != nullptr) != (out_mass != nullptr) || (out_shift != nullptr) != (out_frac_bits != nullptr)) return SBR_ERR_INVALID_ARGUMENT;
    BeamCall bc{};
    bc.set = set; bc.slots = slots; bc.excl_ptr = excl_ptr; bc.excl_items = excl_items;
    bc.w = args->width;
    bc.inv_t = sm.inv_t;
    bc.out_items = out_items; bc.out_scores = out_scores; bc.out_lp = out_step_lp; bc.out_cum = out_cum;
    bc.out_lengths = out_lengths; bc.out_beams = out_beams; bc.out_shift = out_shift; bc.out_mass = out_mass;
    return steps_call(st, &bc, n, args->steps, args->flags, SBR_ROLLOUT_ALLOW_REPEATS | SBR_ROLLOUT_INCLUDE_SEEN, any_of, none_of,
                      sessions_beam_chunk, sessions_beam_chunk_run, out_frac_bits);
}

}  // namespace

sbr_status sbr_sessions_beam_search(sbr_sessions* st, const uint32_t* slots, uint64_t n, const struct sbr_beam_args* args,
                                    const uint64_t* excl_ptr, const uint32_t* excl_items, const uint32_t* any_of, const uint32_t* none_of,
                                    uint32_t* out_items, float* out_scores, float* out_step_lp, float* out_cum, uint32_t* out_lengths,
                                    uint32_t* out_beams, float* out_shift, uint64_t* out_mass, uint32_t* out_frac_bits) {
    return beam_call(st, nullptr, slots, n, args, excl_ptr, excl_items, any_of, none_of, out_items, out_scores, out_step_lp, out_cum, out_lengths,
                     out_beams, out_shift, out_mass, out_frac_bits);
}

/* ---------------------------------------------------------------------------------------------
 * item sets: every catalogue call restricted to a resident sub-table (ITEM SETS in include/sbr_hip.h)
 * ------------------------------------------------------------------------------------------- */
namespace {

/* S's rows into the set's device copy, and the set bound to the parameters they were read from (the caller holds the model's mutex) */
sbr_status item_set_gather(sbr_item_set* set) {
    sbr_model* m = set->m;
    if (!set->ids.empty()) {
        sbr::launch_subset_gather(m->mv, set->d_ids, (uint32_t)set->ids.size(), set->E, set->b, m->stream);
        HIPCHK(hipGetLastError());
    }
    set->gen = m->param_gen;
    return SBR_OK;
}

void item_set_free(sbr_item_set* set) {
    dfree(set->d_ids); dfree(set->E); dfree(set->b);
}

/* entry of every scan through a set: enter_sessions' rule, for the rows the set holds */
sbr_status enter_item_set(const sbr_item_set* set) {
    SBRCHK(enter_reader(set->m));
    return set->gen == set->m->param_gen && set->m->open_plans == 0 ? SBR_OK : SBR_ERR_INVALID_ARGUMENT;
}

/* A set call's descriptor as scan_call's rows: false unless it names exactly one source of rows and none of the fields that source
 * forbids — histories no lists, representations no flags, item_ids or slots, a store no item_ids. */
bool descriptor_rows(const sbr_scan_rows* r, ScanRows* out) {
    if (!r || (r->user_ptr != nullptr) + (r->reps != nullptr) + (r->store != nullptr) != 1) return false;
    if (r->user_ptr) {
        if (r->excl_ptr || r->excl_items) return false;
        *out = ScanRows::of_histories(r->user_ptr, r->item_ids, r->flags, r->any_of, r->none_of);
    } else if (r->reps) {
        if (r->flags || r->item_ids || r->slots) return false;
        *out = ScanRows::of_reps(r->reps, r->excl_ptr, r->excl_items, r->any_of, r->none_of);
    } else {
        if (r->item_ids) return false;
        *out = ScanRows::of_store(r->store, r->slots, r->excl_ptr, r->excl_items, r->flags, r->any_of, r->none_of);
    }
    return true;
}

bool item_set_rows(const sbr_item_set* set, const sbr_scan_rows* r, ScanRows* out) { return set && descriptor_rows(r, out); }

}  // namespace

sbr_status sbr_item_set_create(sbr_model* m, const uint32_t* item_ids, uint64_t n, sbr_item_set** out) {
    if (!m || !out || (n && !item_ids)) return SBR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    for (uint64_t j = 0; j < n; ++j)
        if (item_ids[j] >= m->hp.num_items) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    if (m->open_plans) return SBR_ERR_INVALID_ARGUMENT; /* rows gathered now would go stale with the plan's next step */
    sbr_item_set* set = new (std::nothrow) sbr_item_set();
    if (!set) return SBR_ERR_OUT_OF_MEMORY;
    set->m = m;
    set->ids.assign(item_ids, item_ids + n);
    std::sort(set->ids.begin(), set->ids.end());
    set->ids.erase(std::unique(set->ids.begin(), set->ids.end()), set->ids.end());
    const size_t ns = set->ids.size();
    sbr_status s = SBR_OK;
    if (ns) {
        s = dmalloc(&set->d_ids, ns);
        if (s == SBR_OK) s = dmalloc(&set->E, ns * (size_t)m->d);
        if (s == SBR_OK) s = dmalloc(&set->b, ns);
        if (s == SBR_OK && hipMemcpy(set->d_ids, set->ids.data(), ns * 4, hipMemcpyHostToDevice) != hipSuccess) s = SBR_ERR_HIP;
    }
    if (s == SBR_OK) s = item_set_gather(set);
    if (s != SBR_OK) {
        hipStreamSynchronize(m->stream);
        item_set_free(set);
        delete set;
        return s;
    }
    *out = set;
    return SBR_OK;
}

void sbr_item_set_destroy(sbr_item_set* set) {
    if (!set) return;
    {
        std::lock_guard<std::mutex> lock(set->m->mu);
        hipSetDevice(set->m->device);
        hipStreamSynchronize(set->m->stream); /* the rows go back to the scratch cache: nothing may still read them */
        item_set_free(set);
    }
    delete set;
}

sbr_status sbr_item_set_size(const sbr_item_set* set, uint64_t* out) {
    if (!set || !out) return SBR_ERR_INVALID_ARGUMENT;
    *out = set->ids.size();
    return SBR_OK;
}

sbr_status sbr_item_set_items(const sbr_item_set* set, uint32_t* out) {
    if (!set || (!out && !set->ids.empty())) return SBR_ERR_INVALID_ARGUMENT;
    if (!set->ids.empty()) std::memcpy(out, set->ids.data(), set->ids.size() * 4);
    return SBR_OK;
}

sbr_status sbr_item_set_refresh(sbr_item_set* set) {
    if (!set) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(set->m->mu);
    SBRCHK(enter_reader(set->m));
    if (set->m->open_plans) return SBR_ERR_INVALID_ARGUMENT;
    return item_set_gather(set);
}

sbr_status sbr_item_set_recommend(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, uint32_t k, uint32_t* out_items,
                                  float* out_scores) {
    ScanRows r;
    if (!item_set_rows(set, rows, &r)) return SBR_ERR_INVALID_ARGUMENT;
    return scan_call(set->m, set, r, num_rows, k, out_items, out_scores, ScanVariant());
}

sbr_status sbr_item_set_recommend_diverse(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, uint32_t k, uint32_t pool,
                                          float trade_off, uint32_t metric, uint32_t* out_items, float* out_scores) {
    const Diverse dv{k, trade_off, metric};
    ScanRows r;
    ScanVariant v;
    if (!item_set_rows(set, rows, &r)) return SBR_ERR_INVALID_ARGUMENT;
    v.dv = &dv;
    return scan_call(set->m, set, r, num_rows, pool, out_items, out_scores, v);
}

sbr_status sbr_item_set_recommend_sampled(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, uint32_t k,
                                          const struct sbr_sample_args* sample, uint32_t* out_items, float* out_scores, float* out_keys) {
    Sample sm;
    ScanRows r;
    ScanVariant v;
    if (!sample_args(sample, out_keys, &sm) || !item_set_rows(set, rows, &r)) return SBR_ERR_INVALID_ARGUMENT;
    v.sm = &sm;
    return scan_call(set->m, set, r, num_rows, k, out_items, out_scores, v);
}

sbr_status sbr_item_set_log_partition(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, float temperature, float* out_shift,
                                      uint64_t* out_mass, uint32_t* out_frac_bits) {
    Partition pt;
    ScanRows r;
    ScanVariant v;
    if (!partition_args(temperature, num_rows, out_shift, out_mass, out_frac_bits, &pt) || !item_set_rows(set, rows, &r))
        return SBR_ERR_INVALID_ARGUMENT;
    v.pt = &pt;
    return scan_call(set->m, set, r, num_rows, 1, nullptr, nullptr, v);
}

sbr_status sbr_item_set_recommend_above(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, const float* thresholds,
                                        uint64_t* out_counts, uint64_t* out_total, uint64_t capacity, uint32_t* out_ids, float* out_scores) {
    Above ab;
    ScanRows r;
    ScanVariant v;
    if (!above_args(thresholds, num_rows, out_counts, out_total, capacity, out_ids, out_scores, &ab) || !item_set_rows(set, rows, &r))
        return SBR_ERR_INVALID_ARGUMENT;
    v.ab = &ab;
    return scan_call(set->m, set, r, num_rows, 1, nullptr, nullptr, v);
}

sbr_status sbr_item_set_recommend_top(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, const uint64_t* n, float* out_cuts,
                                      uint64_t* out_counts, uint64_t* out_total, uint64_t capacity, uint32_t* out_ids, float* out_scores) {
    Above ab;
    ScanRows r;
    ScanVariant v;
    if (!top_args(n, num_rows, out_cuts, out_counts, out_total, capacity, out_ids, out_scores, &ab) || !item_set_rows(set, rows, &r))
        return SBR_ERR_INVALID_ARGUMENT;
    v.ab = &ab;
    return scan_call(set->m, set, r, num_rows, 1, nullptr, nullptr, v);
}

sbr_status sbr_item_set_recommend_capped(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, uint32_t k,
                                         const struct sbr_cap_args* cap, uint32_t* out_items, float* out_scores, uint8_t* out_complete) {
    Capped cp;
    ScanRows r;
    ScanVariant v;
    uint32_t pool = 0;
    if (!capped_args(cap, k, out_complete, &cp, &pool) || !item_set_rows(set, rows, &r)) return SBR_ERR_INVALID_ARGUMENT;
    v.cp = &cp;
    return scan_call(set->m, set, r, num_rows, pool, out_items, out_scores, v);
}

/* ---------------------------------------------------------------------------------------------
 * ELIGIBLE RANKS: rank_targets under tag masks, through an item set, on a session store (sbr_rank_eligible.h)
 * ------------------------------------------------------------------------------------------- */
namespace {

/* the ranks form of scan_call over a descriptor's rows, on the model (set null) or through a set of it */
sbr_status rank_targets_rows(sbr_model* m, const sbr_item_set* set, const sbr_scan_rows* rows, uint64_t num_rows, const uint64_t* target_ptr,
                             const uint32_t* target_items, uint32_t* out_ranks) {
    ScanRows r;
    if (!m || !target_ptr || !descriptor_rows(rows, &r)) return SBR_ERR_INVALID_ARGUMENT;
    const Ranks rk{target_ptr, target_items, out_ranks};
    ScanVariant v;
    v.rk = &rk;
    return scan_call(m, set, r, num_rows, 1, nullptr, nullptr, v);
}

}  // namespace

sbr_status sbr_rank_targets_rows(sbr_model* m, const struct sbr_scan_rows* rows, uint64_t num_rows, const uint64_t* target_ptr,
                                 const uint32_t* target_items, uint32_t* out_ranks) {
    return rank_targets_rows(m, nullptr, rows, num_rows, target_ptr, target_items, out_ranks);
}

sbr_status sbr_item_set_rank_targets(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, const uint64_t* target_ptr,
                                     const uint32_t* target_items, uint32_t* out_ranks) {
    if (!set) return SBR_ERR_INVALID_ARGUMENT;
    return rank_targets_rows(set->m, set, rows, num_rows, target_ptr, target_items, out_ranks);
}

namespace {

/* the store descriptor of an item set's rollout or beam search: a store of the set's model, no other source, flags 0 (include_seen is
 * the args' flag); the rest is the plain call's to check */
bool set_store_rows(const sbr_item_set* set, const sbr_scan_rows* r) {
    return set && r && r->store && !r->user_ptr && !r->item_ids && !r->reps && r->flags == 0 && r->store->m == set->m;
}

}  // namespace

sbr_status sbr_item_set_rollout(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, const struct sbr_rollout_args* args,
                                uint32_t* out_items, float* out_scores, float* out_keys, uint32_t* out_lengths, float* out_shift,
                                uint64_t* out_mass, uint32_t* out_frac_bits, float* out_h, float* out_c) {
    if (!set_store_rows(set, rows)) return SBR_ERR_INVALID_ARGUMENT;
    return rollout_call(rows->store, set, rows->slots, num_rows, args, rows->excl_ptr, rows->excl_items, rows->any_of, rows->none_of, out_items,
                        out_scores, out_keys, out_lengths, out_shift, out_mass, out_frac_bits, out_h, out_c);
}

sbr_status sbr_item_set_beam_search(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, const struct sbr_beam_args* args,
                                    uint32_t* out_items, float* out_scores, float* out_step_lp, float* out_cum, uint32_t* out_lengths,
                                    uint32_t* out_beams, float* out_shift, uint64_t* out_mass, uint32_t* out_frac_bits) {
    if (!set_store_rows(set, rows)) return SBR_ERR_INVALID_ARGUMENT;
    return beam_call(rows->store, set, rows->slots, num_rows, args, rows->excl_ptr, rows->excl_items, rows->any_of, rows->none_of, out_items,
                     out_scores, out_step_lp, out_cum, out_lengths, out_beams, out_shift, out_mass, out_frac_bits);
}

sbr_status sbr_sessions_score_candidates(sbr_sessions* st, const uint32_t* slots, uint64_t n, const uint64_t* cand_ptr,
                                         const uint32_t* cand_items, float* out_scores) {
    if (!st) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = st->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_sessions(st));
    SBRCHK(check_slots(st, slots, n));
    const std::vector<int> rows = session_rep_rows(st, slots, n);
    return score_candidates_scan(m, RepSource::of_sessions(st, rows, nullptr, nullptr, nullptr), n, cand_ptr, cand_items, out_scores);
}

/* ---------------------------------------------------------------------------------------------
 * audience: the reverse scan — for each query item the k best candidate rows (sbr_catalogue.hip, the QueryBias policy)
 * ------------------------------------------------------------------------------------------- */
}  // extern "C"

namespace {

/* Where an audience call's candidate rows come from: the caller's host rows [num_rows][embedding_dim], or device rows at the storage
 * width (a session store's), candidate j's being row dev_row[j].  ids (ascending; null: the positions themselves) are what the
 * positions stand for in the results; with `seen` they are slots whose memories exclude. */
struct AudienceSource {
    const float* reps = nullptr;
    const float* dev_rows = nullptr;
    const uint32_t* dev_row = nullptr;
    const uint32_t* ids = nullptr;
    const sbr::SeenView* seen = nullptr;
};

int bits_for(uint64_t n) { /* bits that hold every value below n */
    int b = 1;
    while (b < 32 && (1ull << b) < n) ++b;
    return b;
}

/* The k best of the num_rows candidate rows for each of num_queries query items, in chunks of queries; the candidate table is made
 * once per call, outside the arena: one gather (or upload) however many chunks follow.  excl_ptr / excl_pos: per query the sorted,
 * de-duplicated candidate POSITIONS the caller excludes (excl_ptr empty: none).  With src.seen the chunk's exclusion CSR is built on
 * the device — a count pass over the candidates' rings, one u64 read back to size the key arrays, a fill pass behind the caller's
 * (query, position) keys, the key ordering, and the segment bounds — and never visits the host.
 * With ab (audience_above; k == 1, out_rows / out_scores unused) every chunk is above_chunk's count and fill over the same table and
 * exclusion CSR, the queries the rows and the candidates the columns. */
sbr_status audience_scan(sbr_model* m, const AudienceSource& src, uint64_t num_rows, const uint32_t* items, uint64_t num_queries, uint32_t k,
                         const std::vector<uint64_t>& excl_ptr, const std::vector<uint32_t>& excl_pos, uint32_t* out_rows, float* out_scores,
                         Above* ab = nullptr) {
    if (num_queries == 0) return SBR_OK;
    if (ab && num_rows == 0) { /* nobody to pass: empty rows */
        for (uint64_t j = 0; j < num_queries; ++j) {
            ab->out_counts[j] = 0;
            if (ab->n) ab->out_cuts[j] = ab->n[j] ? -INFINITY : INFINITY;
        }
        return SBR_OK;
    }
    if (num_rows == 0) { /* nobody to rank: rows of padding */
        for (uint64_t e = 0; e < num_queries * k; ++e) {
            out_rows[e] = 0xFFFFFFFFu;
            if (out_scores) out_scores[e] = -INFINITY;
        }
        return SBR_OK;
    }
    /* the scan indexes its A rows (item ids) with an int and its scanned rows with a u32 below the padding id */
    if (m->hp.num_items > 0x7FFFFFFFull || num_rows > 0x7FFFFFFFull) return SBR_ERR_UNSUPPORTED;
    const size_t S = (size_t)num_rows, d = (size_t)m->d, dl = (size_t)m->dl;
    DeviceBlocks call(m->stream);
    float *T = nullptr, *bT = nullptr;
    uint32_t *d_ids = nullptr, *d_rowidx = nullptr;
    SBRCHK(call.take(&T, S * d));
    SBRCHK(call.take(&bT, S));
    if (src.ids) {
        SBRCHK(call.take(&d_ids, S));
        HIPCHK(hipMemcpyAsync(d_ids, src.ids, S * 4, hipMemcpyHostToDevice, m->stream));
    }
    if (src.dev_rows) {
        SBRCHK(call.take(&d_rowidx, S));
        HIPCHK(hipMemcpyAsync(d_rowidx, src.dev_row, S * 4, hipMemcpyHostToDevice, m->stream));
        sbr::launch_audience_gather(m->mv, src.dev_rows, d_rowidx, (uint32_t)S, T, bT, m->stream);
    } else { /* padded to the storage width: the columns past embedding_dim are zero, as in the model's own states */
        HIPCHK(hipMemsetAsync(T, 0, S * d * 4, m->stream));
        HIPCHK(hipMemcpy2DAsync(T, d * 4, src.reps, dl * 4, dl * 4, S, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemsetAsync(bT, 0, S * 4, m->stream));
    }
    HIPCHK(hipGetLastError());
    const bool caller_lists = !excl_ptr.empty();
    size_t cap = recommend_users_cap((uint32_t)S, k);
    if (src.seen && cap > sbr::audience_seen_max_queries) cap = sbr::audience_seen_max_queries;
    for (uint64_t q0 = 0; q0 < num_queries; q0 += cap) {
        const size_t n = (size_t)std::min<uint64_t>(cap, num_queries - q0);
        const uint64_t c0 = caller_lists ? excl_ptr[q0] : 0, c1 = caller_lists ? excl_ptr[q0 + n] : 0;
        const size_t nc = (size_t)(c1 - c0);
        TopkBufs tb;
        uint32_t *qs_item = nullptr, *qs_idx = nullptr;
        unsigned long long* counters = nullptr; /* [0] the count pass's total, [1] the fill pass's cursor */
        AboveBufs abufs{};
        SBRCHK(carve_arena(m, [&](DeviceArena& ar) {
            tb.carve(ar, (uint32_t)S, n, src.seen ? 0 : nc, k, false);
            if (ab) abufs.carve(ar, (uint32_t)S, n, ab->n != nullptr);
            if (src.seen) {
                qs_item = ar.take<uint32_t>(n);
                qs_idx = ar.take<uint32_t>(n);
                counters = ar.take<unsigned long long>(2);
            }
        }));
        HIPCHK(hipMemcpyAsync(tb.rep, items + q0, n * 4, hipMemcpyHostToDevice, m->stream)); /* the scan's rep_row: item ids */
        std::vector<uint64_t> eptr;      /* host vectors the asynchronous copies read: they outlive `chunk`, which drains the stream */
        std::vector<uint32_t> order, sorted_items;
        std::vector<uint64_t> caller_keys;
        DeviceBlocks chunk(m->stream);
        bool lists = false;              /* whether tb.eptr holds an exclusion CSR, its entries at d_excl */
        const uint32_t* d_excl = tb.excl;
        if (!src.seen) {
            if (caller_lists) {
                eptr.resize(n + 1);
                for (size_t j = 0; j <= n; ++j) eptr[j] = excl_ptr[q0 + j] - c0;
                HIPCHK(hipMemcpyAsync(tb.eptr, eptr.data(), (n + 1) * 8, hipMemcpyHostToDevice, m->stream));
                if (nc) HIPCHK(hipMemcpyAsync(tb.excl, excl_pos.data() + c0, nc * 4, hipMemcpyHostToDevice, m->stream));
                lists = true;
            }
        } else {
            order.resize(n);
            for (size_t j = 0; j < n; ++j) order[j] = (uint32_t)j;
            std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return items[q0 + a] < items[q0 + b]; });
            sorted_items.resize(n);
            for (size_t j = 0; j < n; ++j) sorted_items[j] = items[q0 + order[j]];
            HIPCHK(hipMemcpyAsync(qs_item, sorted_items.data(), n * 4, hipMemcpyHostToDevice, m->stream));
            HIPCHK(hipMemcpyAsync(qs_idx, order.data(), n * 4, hipMemcpyHostToDevice, m->stream));
            HIPCHK(hipMemsetAsync(counters, 0, 16, m->stream));
            sbr::launch_audience_seen_count(*src.seen, d_ids, (uint32_t)S, qs_item, qs_idx, (uint32_t)n, counters, m->stream);
            HIPCHK(hipGetLastError());
            unsigned long long total = 0;
            HIPCHK(hipStreamSynchronize(m->stream));
            HIPCHK(hipMemcpy(&total, counters, 8, hipMemcpyDeviceToHost));
            const unsigned long long nkeys = total + nc;
            if (nkeys >= (1ull << 31)) return SBR_ERR_OUT_OF_MEMORY; /* the key ordering counts with 32 bits */
            lists = true;
            if (nkeys == 0) {
                HIPCHK(hipMemsetAsync(tb.eptr, 0, (n + 1) * 8, m->stream));
            } else {
                uint64_t *keys = nullptr, *ka = nullptr, *kb = nullptr;
                uint8_t* temp = nullptr;
                uint32_t* excl = nullptr;
                SBRCHK(chunk.take(&keys, (size_t)nkeys));
                SBRCHK(chunk.take(&ka, (size_t)nkeys));
                SBRCHK(chunk.take(&kb, (size_t)nkeys));
                SBRCHK(chunk.take(&temp, sbr::pair_sort_temp_bytes((size_t)nkeys)));
                SBRCHK(chunk.take(&excl, (size_t)nkeys));
                if (nc) {
                    caller_keys.resize(nc);
                    for (size_t j = 0; j < n; ++j)
                        for (uint64_t e = excl_ptr[q0 + j]; e < excl_ptr[q0 + j + 1]; ++e) caller_keys[e - c0] = ((uint64_t)j << 32) | excl_pos[e];
                    HIPCHK(hipMemcpyAsync(keys, caller_keys.data(), nc * 8, hipMemcpyHostToDevice, m->stream));
                }
                sbr::launch_audience_seen_fill(*src.seen, d_ids, (uint32_t)S, qs_item, qs_idx, (uint32_t)n, keys + nc, total, counters + 1, m->stream);
                sbr::launch_pair_sort(keys, (uint32_t)nkeys, bits_for(n), bits_for(S), ka, kb, temp, m->stream);
                sbr::launch_audience_seen_csr(keys, (uint32_t)nkeys, (uint32_t)n, tb.eptr, excl, m->stream);
                HIPCHK(hipGetLastError());
                d_excl = excl;
            }
        }
        if (ab) {
            sbr::AboveScan as{};
            as.rep_row = tb.rep; as.n = (uint32_t)n; as.thresholds = abufs.th;
            as.excl_ptr = lists ? tb.eptr : nullptr; as.excl_items = d_excl;
            as.f = sbr::TagMasks{nullptr, nullptr, nullptr};
            as.groups = abufs.groups; as.per = abufs.per;
            as.counts = abufs.counts; as.offsets = abufs.offsets; as.totals = abufs.totals;
            as.nonfinite_flag = tb.flag; as.overrun_flag = abufs.over;
            sbr::ModelView mt = m->mv; /* the scan's catalogue: the candidate rows, as launch_audience's */
            mt.E = T; mt.b = bT; mt.num_items = (uint32_t)S;
            SBRCHK(above_chunk(m, mt, m->mv.E, m->mv.b, as, abufs.ts, d_ids, q0, ab, [] { return 0; }));
            continue;
        }
        sbr::TopkScan sc = tb.scan(n, k, lists, out_scores != nullptr);
        sc.excl_items = d_excl;
        SBRCHK(scan_launch(m, tb.flag, [&] { return sbr::launch_audience(m->mv, T, bT, (uint32_t)S, d_ids, sc, m->stream); }, {{out_rows + q0 * k, tb.items, n * k * 4}, {out_scores ? out_scores + q0 * k : nullptr, tb.scores, n * k * 4}}));
    }
    return SBR_OK;
}

/* A caller's per-query lists of row ids (each below `bound`) as sorted, de-duplicated POSITIONS in the ascending candidate ids
 * `cand` (null: the ids are the positions); ids that are no candidates are dropped.  ptr null: no lists (both outputs empty). */
sbr_status audience_exclusions(const uint64_t* ptr, const uint32_t* ids, uint64_t num_queries, uint64_t bound, const std::vector<uint32_t>* cand,
                               std::vector<uint64_t>* out_ptr, std::vector<uint32_t>* out_pos) {
    out_ptr->clear();
    out_pos->clear();
    if (!ptr) return SBR_OK;
    for (uint64_t j = 0; j < num_queries; ++j)
        if (ptr[j + 1] < ptr[j]) return SBR_ERR_INVALID_ARGUMENT;
    if (ptr[num_queries] > ptr[0] && !ids) return SBR_ERR_INVALID_ARGUMENT;
    out_ptr->assign(num_queries + 1, 0);
    for (uint64_t j = 0; j < num_queries; ++j) {
        const size_t from = out_pos->size();
        for (uint64_t e = ptr[j]; e < ptr[j + 1]; ++e) {
            if (ids[e] >= bound) return SBR_ERR_INVALID_ARGUMENT;
            if (!cand) out_pos->push_back(ids[e]);
            else {
                const auto at = std::lower_bound(cand->begin(), cand->end(), ids[e]);
                if (at != cand->end() && *at == ids[e]) out_pos->push_back((uint32_t)(at - cand->begin()));
            }
        }
        std::sort(out_pos->begin() + from, out_pos->end());
        out_pos->erase(std::unique(out_pos->begin() + from, out_pos->end()), out_pos->end());
        (*out_ptr)[j + 1] = out_pos->size();
    }
    return SBR_OK;
}

bool audience_args_ok(const void* handle, const uint32_t* items, uint64_t num_queries, uint32_t k, const uint64_t* excl_ptr, const uint32_t* excl_ids,
                      const uint32_t* out_rows, const Above* ab = nullptr) {
    if (!handle || (num_queries && (!items || (!out_rows && !ab)))) return false;
    if (k < 1 || k > SBR_RECOMMEND_MAX_K) return false;
    return excl_args_ok(excl_ptr, excl_ids, num_queries);
}

/* sbr_audience_reps, and with ab (k == 1, no output rows) sbr_audience_above_reps */
sbr_status audience_reps_call(sbr_model* m, const float* reps, uint64_t num_rows, const uint32_t* items, uint64_t num_queries, uint32_t k,
                              const uint64_t* excl_ptr, const uint32_t* excl_rows, uint32_t* out_rows, float* out_scores, Above* ab) {
    if (!audience_args_ok(m, items, num_queries, k, excl_ptr, excl_rows, out_rows, ab) || (num_rows && !reps)) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    for (uint64_t j = 0; j < num_queries; ++j)
        if (items[j] >= m->hp.num_items) return SBR_ERR_INVALID_ARGUMENT;
    std::vector<uint64_t> eptr;
    std::vector<uint32_t> epos;
    SBRCHK(audience_exclusions(excl_ptr, excl_rows, num_queries, num_rows, nullptr, &eptr, &epos));
    AudienceSource src;
    src.reps = reps;
    return audience_scan(m, src, num_rows, items, num_queries, k, eptr, epos, out_rows, out_scores, ab);
}

/* sbr_audience, and with ab sbr_audience_above */
sbr_status audience_call(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, const uint32_t* items,
                         uint64_t num_queries, uint32_t k, uint32_t flags, uint32_t* out_users, float* out_scores, Above* ab) {
    if (!audience_args_ok(m, items, num_queries, k, nullptr, nullptr, out_users, ab) || !user_ptr) return SBR_ERR_INVALID_ARGUMENT;
    if (flags & ~SBR_RECOMMEND_INCLUDE_HISTORY) return SBR_ERR_INVALID_ARGUMENT;
    for (uint64_t j = 0; j < num_queries; ++j)
        if (items[j] >= m->hp.num_items) return SBR_ERR_INVALID_ARGUMENT;
    std::vector<float> reps((size_t)num_users * (size_t)m->dl + 1);
    SBRCHK(sbr_user_representations(m, user_ptr, item_ids, num_users, reps.data())); /* validates the histories */
    if (flags & SBR_RECOMMEND_INCLUDE_HISTORY)
        return audience_reps_call(m, reps.data(), num_users, items, num_queries, k, nullptr, nullptr, out_users, out_scores, ab);
    /* per query, the users whose WHOLE history holds the item (recommend's mask, evaluation.rs:30-32), ascending */
    std::vector<uint32_t> uniq(items, items + num_queries);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    std::vector<std::vector<uint32_t>> holders(uniq.size());
    for (uint64_t u = 0; u < num_users; ++u)
        for (uint64_t e = user_ptr[u]; e < user_ptr[u + 1]; ++e) {
            const auto at = std::lower_bound(uniq.begin(), uniq.end(), item_ids[e]);
            if (at == uniq.end() || *at != item_ids[e]) continue;
            std::vector<uint32_t>& h = holders[(size_t)(at - uniq.begin())];
            if (h.empty() || h.back() != (uint32_t)u) h.push_back((uint32_t)u);
        }
    std::vector<uint64_t> eptr(num_queries + 1, 0);
    std::vector<uint32_t> eusers;
    for (uint64_t j = 0; j < num_queries; ++j) {
        const std::vector<uint32_t>& h = holders[(size_t)(std::lower_bound(uniq.begin(), uniq.end(), items[j]) - uniq.begin())];
        eusers.insert(eusers.end(), h.begin(), h.end());
        eptr[j + 1] = eusers.size();
    }
    const uint32_t none = 0;
    return audience_reps_call(m, reps.data(), num_users, items, num_queries, k, eptr.data(), eusers.empty() ? &none : eusers.data(), out_users,
                              out_scores, ab);
}

/* sbr_sessions_audience, and with ab sbr_sessions_audience_above */
sbr_status sessions_audience_call(sbr_sessions* st, const uint32_t* items, uint64_t num_queries, uint32_t k, const uint32_t* slots,
                                  uint64_t num_slots, const uint64_t* excl_ptr, const uint32_t* excl_slots, uint32_t flags, uint32_t* out_slots,
                                  float* out_scores, Above* ab) {
    if (!audience_args_ok(st, items, num_queries, k, excl_ptr, excl_slots, out_slots, ab)) return SBR_ERR_INVALID_ARGUMENT;
    /* a store with memory takes sbr_recommend's flag; one without keeps refusing every flag */
    if (st->seen.w ? (flags & ~SBR_RECOMMEND_INCLUDE_HISTORY) != 0 : flags != 0) return SBR_ERR_INVALID_ARGUMENT;
    sbr_model* m = st->m;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_sessions(st));
    for (uint64_t j = 0; j < num_queries; ++j)
        if (items[j] >= m->hp.num_items) return SBR_ERR_INVALID_ARGUMENT;
    std::vector<uint32_t> cand; /* ascending slot ids: a tie goes to the lower position, which is then the lower slot */
    if (slots) {
        SBRCHK(check_slots(st, slots, num_slots));
        cand.assign(slots, slots + num_slots);
        std::sort(cand.begin(), cand.end());
    } else {
        if (num_slots) return SBR_ERR_INVALID_ARGUMENT;
        for (uint64_t sl = 0; sl < st->capacity; ++sl)
            if (st->host_len[sl]) cand.push_back((uint32_t)sl);
    }
    std::vector<uint64_t> eptr;
    std::vector<uint32_t> epos;
    SBRCHK(audience_exclusions(excl_ptr, excl_slots, num_queries, st->capacity, &cand, &eptr, &epos));
    std::vector<uint32_t> rows(cand.size());
    for (size_t j = 0; j < cand.size(); ++j) rows[j] = st->host_len[cand[j]] ? cand[j] : (uint32_t)st->capacity;
    AudienceSource src;
    src.dev_rows = st->v.H;
    src.dev_row = rows.data();
    src.ids = cand.data();
    if (st->seen.w && !(flags & SBR_RECOMMEND_INCLUDE_HISTORY)) src.seen = &st->seen;
    return audience_scan(m, src, cand.size(), items, num_queries, k, eptr, epos, out_slots, out_scores, ab);
}

}  // namespace

extern "C" {

sbr_status sbr_audience_reps(sbr_model* m, const float* reps, uint64_t num_rows, const uint32_t* items, uint64_t num_queries, uint32_t k,
                             const uint64_t* excl_ptr, const uint32_t* excl_rows, uint32_t* out_rows, float* out_scores) {
    return audience_reps_call(m, reps, num_rows, items, num_queries, k, excl_ptr, excl_rows, out_rows, out_scores, nullptr);
}

sbr_status sbr_audience(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, const uint32_t* items,
                        uint64_t num_queries, uint32_t k, uint32_t flags, uint32_t* out_users, float* out_scores) {
    return audience_call(m, user_ptr, item_ids, num_users, items, num_queries, k, flags, out_users, out_scores, nullptr);
}

sbr_status sbr_sessions_audience(sbr_sessions* st, const uint32_t* items, uint64_t num_queries, uint32_t k, const uint32_t* slots,
                                 uint64_t num_slots, const uint64_t* excl_ptr, const uint32_t* excl_slots, uint32_t flags, uint32_t* out_slots,
                                 float* out_scores) {
    return sessions_audience_call(st, items, num_queries, k, slots, num_slots, excl_ptr, excl_slots, flags, out_slots, out_scores, nullptr);
}

/* the threshold forms: every candidate row at or over a per-query score, as CSR (above_gemm_kernel with the QueryBias policy) */
sbr_status sbr_audience_above_reps(sbr_model* m, const float* reps, uint64_t num_rows, const uint32_t* items, uint64_t num_queries,
                                   const float* thresholds, const uint64_t* excl_ptr, const uint32_t* excl_rows, uint64_t* out_counts,
                                   uint64_t* out_total, uint64_t capacity, uint32_t* out_ids, float* out_scores) {
    Above ab;
    if (!above_args(thresholds, num_queries, out_counts, out_total, capacity, out_ids, out_scores, &ab)) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(audience_reps_call(m, reps, num_rows, items, num_queries, 1, excl_ptr, excl_rows, nullptr, nullptr, &ab));
    *out_total = ab.total;
    return SBR_OK;
}

sbr_status sbr_audience_above(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, const uint32_t* items,
                              uint64_t num_queries, const float* thresholds, uint32_t flags, uint64_t* out_counts, uint64_t* out_total,
                              uint64_t capacity, uint32_t* out_ids, float* out_scores) {
    Above ab;
    if (!above_args(thresholds, num_queries, out_counts, out_total, capacity, out_ids, out_scores, &ab)) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(audience_call(m, user_ptr, item_ids, num_users, items, num_queries, 1, flags, nullptr, nullptr, &ab));
    *out_total = ab.total;
    return SBR_OK;
}

sbr_status sbr_sessions_audience_above(sbr_sessions* st, const uint32_t* items, uint64_t num_queries, const float* thresholds,
                                       const uint32_t* slots, uint64_t num_slots, const uint64_t* excl_ptr, const uint32_t* excl_slots,
                                       uint32_t flags, uint64_t* out_counts, uint64_t* out_total, uint64_t capacity, uint32_t* out_ids,
                                       float* out_scores) {
    Above ab;
    if (!above_args(thresholds, num_queries, out_counts, out_total, capacity, out_ids, out_scores, &ab)) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(sessions_audience_call(st, items, num_queries, 1, slots, num_slots, excl_ptr, excl_slots, flags, nullptr, nullptr, &ab));
    *out_total = ab.total;
    return SBR_OK;
}

/* the budget forms: the exact best n[query] candidate rows of every query and its cut */
sbr_status sbr_audience_top_reps(sbr_model* m, const float* reps, uint64_t num_rows, const uint32_t* items, uint64_t num_queries, const uint64_t* n,
                                 const uint64_t* excl_ptr, const uint32_t* excl_rows, float* out_cuts, uint64_t* out_counts, uint64_t* out_total,
                                 uint64_t capacity, uint32_t* out_ids, float* out_scores) {
    Above ab;
    if (!top_args(n, num_queries, out_cuts, out_counts, out_total, capacity, out_ids, out_scores, &ab)) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(audience_reps_call(m, reps, num_rows, items, num_queries, 1, excl_ptr, excl_rows, nullptr, nullptr, &ab));
    *out_total = ab.total;
    return SBR_OK;
}

sbr_status sbr_audience_top(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, const uint32_t* items,
                            uint64_t num_queries, const uint64_t* n, uint32_t flags, float* out_cuts, uint64_t* out_counts, uint64_t* out_total,
                            uint64_t capacity, uint32_t* out_ids, float* out_scores) {
    Above ab;
    if (!top_args(n, num_queries, out_cuts, out_counts, out_total, capacity, out_ids, out_scores, &ab)) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(audience_call(m, user_ptr, item_ids, num_users, items, num_queries, 1, flags, nullptr, nullptr, &ab));
    *out_total = ab.total;
    return SBR_OK;
}

sbr_status sbr_sessions_audience_top(sbr_sessions* st, const uint32_t* items, uint64_t num_queries, const uint64_t* n, const uint32_t* slots,
                                     uint64_t num_slots, const uint64_t* excl_ptr, const uint32_t* excl_slots, uint32_t flags, float* out_cuts,
                                     uint64_t* out_counts, uint64_t* out_total, uint64_t capacity, uint32_t* out_ids, float* out_scores) {
    Above ab;
    if (!top_args(n, num_queries, out_cuts, out_counts, out_total, capacity, out_ids, out_scores, &ab)) return SBR_ERR_INVALID_ARGUMENT;
    SBRCHK(sessions_audience_call(st, items, num_queries, 1, slots, num_slots, excl_ptr, excl_slots, flags, nullptr, nullptr, &ab));
    *out_total = ab.total;
    return SBR_OK;
}

/* ---------------------------------------------------------------------------------------------
 * numerics self-tests (tests/test_numerics_gpu.py): run the contract's primitives on the device
 * ------------------------------------------------------------------------------------------- */
sbr_status sbr_selftest_math(const float* x, uint64_t n, float* out_cell_h, float* out_sig, float* out_tanh) {
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) return SBR_ERR_NO_DEVICE;
    float *dx, *de, *ds, *dt;
    SBRCHK(dmalloc(&dx, n)); SBRCHK(dmalloc(&de, n)); SBRCHK(dmalloc(&ds, n)); SBRCHK(dmalloc(&dt, n));
    HIPCHK(hipMemcpy(dx, x, n * 4, hipMemcpyHostToDevice));
    sbr::launch_selftest_math(dx, de, ds, dt, n, nullptr);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out_cell_h, de, n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_sig, ds, n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_tanh, dt, n * 4, hipMemcpyDeviceToHost));
    dfree(dx); dfree(de); dfree(ds); dfree(dt);
    return SBR_OK;
}

sbr_status sbr_selftest_dot_tree(const float* x, const float* y, uint32_t d, uint64_t nrows, float* out) {
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) return SBR_ERR_NO_DEVICE;
    if (!dim_ok(d) || nrows == 0) return SBR_ERR_INVALID_ARGUMENT;
    float *dx, *dy, *dout;
    SBRCHK(dmalloc(&dx, nrows * d)); SBRCHK(dmalloc(&dy, nrows * d)); SBRCHK(dmalloc(&dout, nrows));
    HIPCHK(hipMemcpy(dx, x, nrows * d * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dy, y, nrows * d * 4, hipMemcpyHostToDevice));
    sbr::launch_selftest_dot_tree(dx, dy, (int)d, nrows, dout, nullptr);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, dout, nrows * 4, hipMemcpyDeviceToHost));
    dfree(dx); dfree(dy); dfree(dout);
    return SBR_OK;
}

/* out[16][16] = c0 + a[16][k] b[k][16] on v_mfma_f32_16x16x4_f32; out32[32][32] = a32[32][k] b32[k][32]
 * on v_mfma_f32_32x32x2_f32 (k multiple of 4) */
sbr_status sbr_selftest_mfma(const float* a, const float* b, const float* c0, uint32_t k, float* out,
                             const float* a32, const float* b32, float* out32) {
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) return SBR_ERR_NO_DEVICE;
    if (k == 0 || k % 4) return SBR_ERR_INVALID_ARGUMENT;
    float *da, *db, *dc, *dout, *da32, *db32, *dout32;
    SBRCHK(dmalloc(&da, 16 * k)); SBRCHK(dmalloc(&db, 16 * k)); SBRCHK(dmalloc(&dc, 256)); SBRCHK(dmalloc(&dout, 256));
    SBRCHK(dmalloc(&da32, 32 * k)); SBRCHK(dmalloc(&db32, 32 * k)); SBRCHK(dmalloc(&dout32, 1024));
    HIPCHK(hipMemcpy(da, a, 16 * k * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(db, b, 16 * k * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dc, c0, 256 * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(da32, a32, 32 * k * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(db32, b32, 32 * k * 4, hipMemcpyHostToDevice));
    sbr::launch_selftest_mfma_chain(da, db, dc, (int)k, dout, nullptr);
    sbr::launch_selftest_mfma32_chain(da32, db32, (int)k, dout32, nullptr);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, dout, 256 * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out32, dout32, 1024 * 4, hipMemcpyDeviceToHost));
    dfree(da); dfree(db); dfree(dc); dfree(dout); dfree(da32); dfree(db32); dfree(dout32);
    return SBR_OK;
}

/* keys (rows[e] << 32 | e), e = 0..n-1, in (row, e) order on the engine's own key ordering (sbr_sort.hip), and the
 * positions at which a new row starts */
sbr_status sbr_selftest_sort(const uint32_t* rows, uint64_t n, uint32_t row_bits, uint64_t* out_keys, uint32_t* out_head_pos,
                             uint32_t* out_nheads) {
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) return SBR_ERR_NO_DEVICE;
    if (!rows || !out_keys || !out_head_pos || !out_nheads || n == 0 || n >= (1ull << 32) || row_bits == 0 || row_bits > 32)
        return SBR_ERR_INVALID_ARGUMENT;
    uint32_t *drows, *dheads, *dn;
    uint64_t *dtmp, *dout;
    uint8_t* temp;
    SBRCHK(dmalloc(&drows, n)); SBRCHK(dmalloc(&dheads, n + 1)); SBRCHK(dmalloc(&dn, 1));
    SBRCHK(dmalloc(&dtmp, n)); SBRCHK(dmalloc(&dout, n));
    SBRCHK(dmalloc(&temp, sbr::sparse_sort_temp_bytes(n, 32 + (int)row_bits)));
    HIPCHK(hipMemcpy(drows, rows, n * 4, hipMemcpyHostToDevice));
    sbr::launch_selftest_sort(drows, (uint32_t)n, (int)row_bits, dtmp, dout, temp, dheads, dn, nullptr);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out_keys, dout, n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_nheads, dn, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_head_pos, dheads, ((uint64_t)*out_nheads + 1) * 4, hipMemcpyDeviceToHost));
    dfree(drows); dfree(dheads); dfree(dn); dfree(dtmp); dfree(dout); dfree(temp);
    return SBR_OK;
}

/* the stream-delay test hook's counter: delay kernels queued per role (main, side, sorter, copier, xs) on this model's streams
 * since the last read */
sbr_status sbr_test_delays_queued(sbr_model* m, uint64_t out[5]) {
    if (!m || !out) return SBR_ERR_INVALID_ARGUMENT;
    for (int r = 0; r < ROLE_COUNT; ++r) out[r] = m->test_delays[r].exchange(0, std::memory_order_relaxed);
    return SBR_OK;
}

/* What the stream-delay method can see (tests/test_stream_joins_gpu.py): a float that is 1.0; stream A: delay, store of 2.0, event;
 * stream B: waits for the event (with_join) or not, then copies the float.  *out = 2.0 with the join; without it B's copy runs
 * while A is still held back and reads 1.0.  Only a plain float is ever read early. */
sbr_status sbr_selftest_stream_delay(uint32_t delay_us, int32_t with_join, float* out) {
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) return SBR_ERR_NO_DEVICE;
    if (!out) return SBR_ERR_INVALID_ARGUMENT;
    const unsigned long long ticks = (unsigned long long)std::min(delay_us, test_delay_max_us) * (unsigned long long)wall_clock_khz() / 1000ull;
    float* cell = nullptr; /* [0] the float, [1] B's copy of it */
    SBRCHK(dmalloc(&cell, 2));
    const float init[2] = {1.0f, 0.0f};
    hipStream_t a = nullptr, b = nullptr;
    hipEvent_t stored = nullptr;
    sbr_status st = SBR_OK;
    if (hipMemcpy(cell, init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipStreamCreateWithFlags(&a, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&b, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&stored, hipEventDisableTiming) != hipSuccess)
        st = SBR_ERR_HIP;
    if (st == SBR_OK) {
        sbr::launch_stream_delay(ticks, a);
        sbr::launch_selftest_store(cell, 2.0f, a);
        if (hipEventRecord(stored, a) != hipSuccess) st = SBR_ERR_HIP;
        if (st == SBR_OK && with_join && hipStreamWaitEvent(b, stored, 0) != hipSuccess) st = SBR_ERR_HIP;
        if (st == SBR_OK && hipMemcpyAsync(cell + 1, cell, sizeof(float), hipMemcpyDeviceToDevice, b) != hipSuccess) st = SBR_ERR_HIP;
    }
    if (b && hipStreamSynchronize(b) != hipSuccess) st = SBR_ERR_HIP;
    if (a && hipStreamSynchronize(a) != hipSuccess) st = SBR_ERR_HIP;
    if (st == SBR_OK && hipMemcpy(out, cell + 1, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) st = SBR_ERR_HIP;
    if (stored) hipEventDestroy(stored);
    if (a) hipStreamDestroy(a);
    if (b) hipStreamDestroy(b);
    dfree(cell);
    return st;
}

/* What the poisoned-scratch hook can see (tests/test_poisoned_scratch_gpu.py): a block of the scratch cache (kind 0 device, 1
 * pinned host) as it is handed out, copied to out_host[0, bytes); the block is then zeroed and given back, and the same size is
 * taken again — the cache hit — and copied to out_host[bytes, 2 bytes).  With SBR_TEST_POISON set every byte of both is the pattern. */
sbr_status sbr_selftest_scratch(uint32_t kind, uint64_t bytes, void* out_host) {
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) return SBR_ERR_NO_DEVICE;
    if (kind > 1 || bytes == 0 || !out_host) return SBR_ERR_INVALID_ARGUMENT;
    const bool host = kind == 1;
    for (int round = 0; round < 2; ++round) {
        uint8_t* p = nullptr;
        HIPCHK(scratch_cache().get(reinterpret_cast<void**>(&p), bytes, host));
        uint8_t* dst = static_cast<uint8_t*>(out_host) + (size_t)round * bytes;
        sbr_status st = SBR_OK;
        if (host) {
            std::memcpy(dst, p, bytes);
            std::memset(p, 0, bytes);
        } else if (hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost) != hipSuccess || hipMemset(p, 0, bytes) != hipSuccess ||
                   hipDeviceSynchronize() != hipSuccess) {
            st = SBR_ERR_HIP;
        }
        scratch_cache().put(p, host);
        SBRCHK(st);
    }
    return SBR_OK;
}

/* The same for the serving arena: carve `bytes`, copy out, zero, carve the same size again (no growth), copy out. */
sbr_status sbr_selftest_arena(sbr_model* m, uint64_t bytes, void* out_host) {
    if (!m || bytes == 0 || !out_host) return SBR_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(m->mu);
    SBRCHK(enter_reader(m));
    for (int round = 0; round < 2; ++round) {
        uint8_t* p = nullptr;
        SBRCHK(carve_arena(m, [&](DeviceArena& ar) { p = ar.take<uint8_t>(bytes); }));
        HIPCHK(hipMemcpyAsync(static_cast<uint8_t*>(out_host) + (size_t)round * bytes, p, bytes, hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemsetAsync(p, 0, bytes, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
    }
    return SBR_OK;
}

/* read-and-reset of the guard counters; `put_back` non-null: those become the counters (sbr_selftest_guard hands back what it set aside) */
static sbr_guard_report guard_counters_exchange(uint64_t* allocs, const sbr_guard_report* put_back) {
    GuardState& gs = guard_state();
    std::lock_guard<std::mutex> g(gs.mu);
    const sbr_guard_report r = gs.r;
    const uint64_t a = gs.allocs;
    gs.r = put_back ? *put_back : sbr_guard_report{};
    gs.allocs = put_back && allocs ? *allocs : 0;
    if (allocs) *allocs = a;
    return r;
}

sbr_status sbr_test_guard_report(sbr_model* m, sbr_guard_report* out) {
    int nd = 0, current = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) return SBR_ERR_NO_DEVICE;
    if (!out) return SBR_ERR_INVALID_ARGUMENT;
    HIPCHK(hipGetDevice(&current));
    for (int dev = 0; dev < nd; ++dev) { /* a live block may belong to any device's streams */
        HIPCHK(hipSetDevice(dev));
        HIPCHK(hipDeviceSynchronize());
    }
    HIPCHK(hipSetDevice(current));
    if (m) {
        std::lock_guard<std::mutex> lock(m->mu);
        SBRCHK(ensure_device(m));
        check_arena_guards(m->eval_arena);
        HIPCHK(hipSetDevice(current));
    }
    scratch_cache().check_live();
    *out = guard_counters_exchange(nullptr, nullptr);
    return SBR_OK;
}

/* What the guard can see: one byte, set by the library itself inside its own allocation, on the first and on the re-used one. */
sbr_status sbr_selftest_guard(sbr_model* m, uint32_t where, int32_t side, sbr_guard_report out[2]) {
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) return SBR_ERR_NO_DEVICE;
    if (where < SBR_GUARD_DEVICE_BLOCK || where > SBR_GUARD_BIG_BLOCK || side == 0 || !out || (where == SBR_GUARD_ARENA_TAKE && !m))
        return SBR_ERR_INVALID_ARGUMENT;
    const size_t bytes = 4096 + 100 + (where == SBR_GUARD_BIG_BLOCK ? ScratchCache::kMaxBlock : 0);
    const uint8_t other = (uint8_t)~kGuardByte;
    std::unique_lock<std::mutex> lock;
    if (where == SBR_GUARD_ARENA_TAKE) { /* what the last call's kernels left of the current carve's bands is a real finding: it is kept */
        lock = std::unique_lock<std::mutex>(m->mu);
        SBRCHK(enter_reader(m));
        HIPCHK(hipStreamSynchronize(m->stream));
        check_arena_guards(m->eval_arena);
    }
    uint64_t kept_allocs = 0;
    const sbr_guard_report kept = guard_counters_exchange(&kept_allocs, nullptr);
    sbr_status st = SBR_OK;
    if (where == SBR_GUARD_ARENA_TAKE) {
        for (int round = 0; round < 2 && st == SBR_OK; ++round) {
            uint8_t* p[3] = {nullptr, nullptr, nullptr};
            st = carve_arena(m, [&](DeviceArena& ar) { for (auto& q : p) q = ar.take<uint8_t>(bytes); });
            (void)guard_counters_exchange(nullptr, nullptr); /* the head of the second carve checked the first one's bands */
            if (st != SBR_OK) break;
            if (test_guard_bytes() && hipMemsetAsync(side > 0 ? p[1] + bytes : p[0] - 1, other, 1, m->stream) != hipSuccess) st = SBR_ERR_HIP;
            if (hipStreamSynchronize(m->stream) != hipSuccess) st = SBR_ERR_HIP;
            check_arena_guards(m->eval_arena);
            out[round] = guard_counters_exchange(nullptr, nullptr);
        }
    } else {
        const bool host = where == SBR_GUARD_PINNED_BLOCK;
        for (int round = 0; round < 2 && st == SBR_OK; ++round) {
            uint8_t* p = nullptr;
            if (scratch_cache().get(reinterpret_cast<void**>(&p), bytes, host) != hipSuccess) { st = SBR_ERR_OUT_OF_MEMORY; break; }
            if (test_guard_bytes()) {
                uint8_t* at = side > 0 ? p + bytes : p - 1;
                if (host) *at = other;
                else if (hipMemset(at, other, 1) != hipSuccess || hipDeviceSynchronize() != hipSuccess) st = SBR_ERR_HIP;
            }
            scratch_cache().put(p, host); /* checks the bands before the block is cached (or, past 64 MiB, freed) */
            out[round] = guard_counters_exchange(nullptr, nullptr);
        }
    }
    uint64_t a = kept_allocs;
    (void)guard_counters_exchange(&a, &kept);
    return st;
}

sbr_status sbr_set_device(int32_t ordinal) {
    HIPCHK(hipSetDevice(ordinal));
    return SBR_OK;
}

}  // extern "C"
