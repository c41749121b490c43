/* sbr_kernels.h — launch interface between the host engine (sbr_engine.hip) and the gfx950
 * kernels (sbr_kernels.hip and its neighbours; the prediction side is sbr_catalogue.hip).  Internal to libsbr_hip.so; the public
 * ABI is include/sbr_hip.h. */
#ifndef SBR_KERNELS_H
#define SBR_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sbr {

/* One device-local packed minibatch.  Rows are time-major: row(t, b) = off[t] + b, sequences b in
 * length-descending order, so the rows of step t are a prefix of the sequences of step t-1. */
struct MbView {
    int R;                   /* packed rows = sum over sequences of steps                     */
    int B;                   /* sequences                                                     */
    int Tm;                  /* max steps                                                     */
    const int* off;          /* device [Tm+1]                                                 */
    const int* steps;        /* device [B]   steps of sequence b                              */
    const int* prev_row;     /* device [R]   packed row of (t-1, b) or -1                      */
    const uint32_t* in_idx;  /* device [R]                                                    */
    const uint32_t* out_idx; /* device [R]   = in_idx of the same sequence's next step (both packers write item[t] / item[t + 1] of one
                              *               slice): the EWMA scans hand a step's target row on as the next step's input               */
    const uint32_t* ctr;     /* device [R]   p * max_sequence_length + t                       */
};

/* Views into one exchange block (layout: oracle/sbr_oracle.c "exchange block"). */
struct BlockView {
    uint32_t* header; /* [0]=R, [4..5]=f64 loss_sum, [6..7]=u64 examples */
    uint32_t* in_idx;
    uint32_t* out_idx;
    uint32_t* neg;
    float* coef;
    float* H;
    float* dX;
    float* dense;
};

struct ModelView {
    int d, ng;          /* ng = 4 / 3 / 0 */
    int coupled;
    uint32_t num_items;
    int loss;           /* sbr_loss */
    float lr, l2;
    float *E, *Eacc, *b, *bacc;
    float *W, *Wacc, *bW, *bWacc, *Wp, *WTp;
    float *alpha, *alpha_acc;
    /* Adam */
    int optimizer;      /* sbr_optimizer */
    float c1, c2;       /* 1 - beta^t of the current step */
    float *Em, *bm, *Wm, *bWm, *alpha_m;
};

/* Up to this many tiles the length-sorted tile list of the sequence-resident recurrent kernels is folded (alternate groups of
 * 256 reversed): with about as many tiles as resident slots (512) every CU then gets long + short.  ms per step on one box,
 * folded / not: 375 tiles 2.29 / 2.55, 512 tiles 2.65 / 2.97 (BPTT alone 0.72 / 0.91 — it had no fold before), 625 tiles 3.16 /
 * 3.33, 750 and 1 024 tiles equal; with several rounds of tiles the dispatcher's own order — longest first, next tile to the
 * first free slot — is the better schedule: 1 563 tiles 13.65 / 13.53. */
#define SBR_FOLD_MAX_TILES_DEFAULT 1024
struct WorkView { /* per-plan scratch, sized for Rmax rows / Bmax sequences */
    float *C, *G, *dH, *dZ;
    float* X;               /* [Rmax][d] copy of the gathered input rows (forward) for the dense-gradient GEMM */
    float *dHrec, *dCrec;   /* [Bmax][d] */
    float* dab;             /* EWMA per-sequence dalpha partials [Bmax][d] */
    float* partials;        /* dense-gradient chunk partials */
    float* loss;            /* [Rmax] */
    uint32_t* tries;        /* [Rmax] */
    double* part_loss;      /* per-workgroup partials of the score kernel [2048] */
    unsigned int* part_tries;
    float* zeros;           /* 256 zeros (h_{-1} of the dense-gradient GEMM, 64-bit address path) */
    int fold_max_tiles;     /* the recurrent kernels fold their length-sorted tile list up to this many tiles */
    int wide_addresses;     /* 1: the dense-gradient GEMM takes its 64-bit per-lane address path even where the buffer path would do (tests) */
    int stream_activations; /* set per launch by launch_recurrent_forward: 1 = gates / cell states / input copy are stored nt (the step's h rows fit
                             * the Infinity Cache and the score kernel, next on the stream, finds them there: SBR_STREAM_MAX_H_BYTES) */
};

/* one chunk pointer per device: slices of one gathered buffer (collective transport), or the peers' own
 * buffers read in place through peer mappings (peer transport) */
struct ChunkPtrs {
    const void* p[16];
};

/* Which segments of the ordered keys take the chunked path (seg_chunk_kernel: one lane group per <= SBR_SEG_CHUNK-entry chunk, the
 * chunks spread evenly over the chip; seg_finish_kernel adds a segment's chunk partials in order) instead of being reduced by the
 * lane group that meets them in seg_short_kernel: every segment of more than SBR_SEG_ROUTE entries.  The CONTRACT's chunk stays
 * SBR_SEG_CHUNK = 256 (a segment of 33..256 entries is ONE chunk: the same in-order sum either way, same bits); the routing
 * threshold only decides who walks it.  Under a skewed catalogue the grid-stride short-segment pass otherwise waits for the few lane
 * groups that meet several 100-entry segments one after the other (Zipf(1) items at 8 192 sequences per step: 0.81 ms against 0.28
 * for uniform items). */
#ifndef SBR_SEG_ROUTE
#define SBR_SEG_ROUTE 32
#endif
/* scratch of the long-segment path of the sparse reduction */
struct SegScratch {
    uint32_t* counters;   /* [0] long segments, [1] chunk units */
    uint32_t* long_start; /* first / one-past-last key position of every long segment */
    uint32_t* long_end;
    uint32_t* unit_base;  /* exclusive prefix of the long segments' chunk counts */
    float* P;             /* chunk partials [units][D] */
    float* Pb;
    uint32_t* Pf;         /* 1 = the chunk has a bias contribution */
    uint32_t cap;         /* capacity of the long-segment arrays */
    /* segment heads of the sorted keys (positions whose row differs from the previous key's), ascending, plus
     * the sentinel head_pos[*nheads] = number of keys; produced right after the sort, on its stream */
    uint32_t* head_pos;
    uint32_t* nheads;
    uint32_t prelisted;   /* 1: the long segments were listed and their chunk units counted right after the ordering (launch_seg_prelist):
                           * the short-segment pass skips them, their chunks are reduced beside it on another stream */
};
/* single device, large step: the hot rows' part of the sparse update off the update's critical path.  launch_seg_prelist (the
 * ordering's stream, underneath BPTT) lists the segments of more than SBR_SEG_CHUNK entries and counts their chunk units;
 * launch_seg_apply then runs the short segments only, and launch_seg_hot_apply reduces and applies the listed ones on another stream
 * (disjoint table rows). */
void launch_seg_prelist(const SegScratch& sc, hipStream_t s);

/* where the owner's row range lies in every device's sorted keys — DEVICE-resident, written by merge_plan_kernel from the devices'
 * owner bounds (round 6: the host no longer reads the bounds back, so a partitioned step is queued without a host rendezvous) */
struct MergePlan {
    uint32_t lo[16];   /* first position of the owner's row range in device r's sorted keys */
    uint32_t base[17]; /* exclusive prefix sum of the range lengths; base[16] = their total */
};
/* the devices' gradient lists as the owner of a row range sees them (device pointers, peer-readable) */
struct PeerLists {
    const uint64_t* keys[16];
    const float* G[16];
    const float* gb[16];
    const uint32_t* fl[16];
    const MergePlan* plan; /* on the owner's device */
};
/* device r's owner bounds [ndev + 1] (owner_bounds_kernel), peer-readable or gathered */
struct PeerBounds {
    const uint32_t* b[16];
};

/* recurrent forward over all steps of the minibatch (LSTM d <= 128: one sequence-resident launch; d = 256: one launch per step) */
void launch_recurrent_forward(const ModelView& m, const MbView& mb, float* H, const WorkView& w, int tm_host,
                              const int* off_host, hipStream_t s);
/* sbr_wave.hip: the wave-per-sequence form of the recurrent pass for small minibatches at d <= 32 (false: not taken, the
 * caller launches the tile kernels; same outputs bit for bit) */
bool launch_wave_forward(const ModelView& m, const MbView& mb, float* H, const WorkView& w, int tm_host, hipStream_t s);
bool launch_wave_backward(const ModelView& m, const MbView& mb, const BlockView& blk, const WorkView& w, int tm_host, int b_host,
                          hipStream_t s);
/* dense-gradient chunk partials of a small step at d <= 32: one wave per 32 x 32 output block (w.partials as the tile kernels') */
bool launch_wave_dense_gradient(const ModelView& m, const MbView& mb, const BlockView& blk, const WorkView& w, int rows_host,
                                hipStream_t s);
/* gather + negative sampling + loss + dloss/dh; also copies in/out idx into the block */
/* A step of ONE subsequence (the reference's own schedule, sequence_model.rs:111-169) at d <= 32: what follows the score pass —
 * block header + loss accumulators, the lagged loss figure, the (row, entry) ordering of the step's 3 R keys and its segment
 * heads — runs at the end of the score launch itself (one workgroup) instead of in three more launches of ~5 us each. */
#define SBR_SMALL_TAIL_MAX_ROWS 255
struct SmallTail {
    uint32_t* header;
    double* loss_acc;            /* may be null (several devices: the header travels) */
    unsigned long long* ex_acc;
    float* lag_state;            /* [accumulator | (loss node k, its staged next value) per step k] (sbr_report.hip) */
    uint64_t* keys_sorted;
    uint32_t* head_pos;
    uint32_t* nheads;
};
bool small_tail_shape_ok(const ModelView& m, int sequences_host, int rows_host, bool wide = false); /* wide: every kernel width (the reference-order step) */
bool reference_order_shape_ok(int d, int max_rows); /* sbr_steps.hip: the sequential-stream scorer's LDS */
/* Reference order (one sequence per step, one device): negatives from the worker's sequential xorshift stream (rng_state: 4 words on
 * the device, advanced by exactly the draws consumed), then the SmallTail.  Returns false where the one-sequence form does not exist. */
bool launch_score_reference_order(const ModelView& m, const MbView& mb, const BlockView& blk, const WorkView& w, uint32_t* rng_state,
                                  int rows_host, hipStream_t s, const SmallTail& tail);
/* The optimiser half of a small single-device LSTM step at d <= 32 (one dense-gradient chunk, single-launch sparse update) in ONE
 * launch: dense gradient (per-element row chains) + dense update + sparse update, instead of three. */
bool small_back_shape_ok(const ModelView& m, int rows_host);
/* A RUN of consecutive one-sequence optimiser steps (the reference's own schedule, sequence_model.rs:111-169) at d <= 32 in ONE
 * launch: one workgroup walks the steps with each step's working set in LDS — one gather of the step's 3 n rows and of the touched
 * rows' optimiser state, then scan, scores, backward scan, dalpha, key ordering, per-row reduction and the Adagrad updates out of
 * LDS (ewma_steps_kernel, sbr_steps.hip).  EWMA with a single-negative loss, Adagrad, at most SBR_EWMA_STEPS_MAX_ROWS rows per
 * step.  desc[i] = the i-th step of the epoch's packed arrays (one sequence each). */
struct StepDesc { uint32_t rows, row_base, off_base, seq_base; };
struct EpochView {
    const int* off;
    const int* steps;
    const int* prev_row;
    const uint32_t *in_idx, *out_idx, *ctr;
    const StepDesc* desc;
};
#define SBR_EPOCH_STEPS_MAX_LDS (150 * 1024)  /* dynamic LDS of the run's workgroup */
/* The same for the LSTM (Normal, d = 32, single-negative loss, Adagrad: the reference's Criterion shape): lstm_steps_kernel walks a
 * run of steps of at most lstm_steps_max_rows() rows each; lag_rows = max_sequence_length - 1 (the loss nodes of sbr_report.hip). */
bool lstm_steps_shape_ok(const ModelView& m, int lag_rows_host);
int lstm_steps_max_rows();
void launch_lstm_steps(const ModelView& m, const EpochView& ev, const BlockView& blk, const WorkView& w, uint64_t epoch_key,
                       const SmallTail& tail, int step_begin, int step_end, int lag_rows_host, int run_max_rows_host,
                       unsigned long long* phase_clocks, hipStream_t s);
bool epoch_steps_shape_ok(const ModelView& m, int max_rows_host);
void launch_epoch_steps(const ModelView& m, const EpochView& ev, const BlockView& blk, const WorkView& w, uint64_t epoch_key,
                        const SmallTail& tail, int step_begin, int step_end, int max_rows_host,
                        unsigned long long* phase_clocks /* [6] or null */, hipStream_t s);
void launch_seg_hot_apply(const ModelView& m, const BlockView& blk, const uint64_t* keys_sorted, const SegScratch& sc, hipStream_t s);
void launch_small_back(const ModelView& m, const MbView& mb, const BlockView& blk, const WorkView& w, uint32_t rows_host,
                       const uint64_t* keys_sorted, const SegScratch& sc, hipStream_t s);
void launch_score(const ModelView& m, const MbView& mb, const BlockView& blk, const WorkView& w, uint64_t epoch_key,
                  int rows_host, hipStream_t s, const SmallTail* tail = nullptr);
/* EWMA with a single-negative loss (hinge / BPR): forward scan, scoring and backward scan of a sequence in ONE pass (replaces
 * launch_recurrent_forward + launch_score + launch_recurrent_backward's scan; same outputs bit for bit; the dalpha reduction stays
 * launch_dense_gradient's) */
void launch_ewma_sequences(const ModelView& m, const MbView& mb, const BlockView& blk, const WorkView& w, uint64_t epoch_key,
                           int rows_host, hipStream_t s, const SmallTail* tail = nullptr);
/* debug only: dloss/dh of every packed row (the training path never materialises it) */
void launch_materialize_dh(const ModelView& m, const BlockView& blk, int rows_host, float* dH, hipStream_t s);
/* header of the exchange block (rows, loss sum, examples); loss_acc / ex_acc non-null (single device): the plan's accumulators
 * take the header in the same launch; lag_state non-null (small step, <= SBR_HEADER_LAG_MAX_B sequences): the lagged loss figure
 * (below) in the same launch too */
#define SBR_HEADER_LAG_MAX_B 1024
void launch_block_header(const ModelView& m, const BlockView& blk, const WorkView& w, const MbView& mb, int rows_host, double* loss_acc,
                         unsigned long long* ex_acc, float* lag_state, hipStream_t s);
void launch_block_header_parts(uint32_t* header, int rows_host, const double* part_loss, const unsigned int* part_tries, int nparts,
                               double* loss_acc, unsigned long long* ex_acc, const MbView& mb, const float* loss, float* lag_state,
                               hipStream_t s);
/* sbr_report.hip — the loss figure the reference's `fit` returns (sequence_model.rs:157 reads the loss node BEFORE :160 runs its
 * forward pass: a subsequence of s steps contributes the running sum L_{s-1} of the worker's most recent earlier subsequence with at
 * least s steps).  seq_loss: the sequences' running sums, t ascending (px[b] = what sequence b + 1 reads; the nodes' next values);
 * lagged_chain: the strictly sequential f32 accumulation over the minibatch's sequences on one wave.
 * lag_state = [accumulator | (node k, its staged next value) per step k]. */
void launch_seq_loss(const MbView& mb, const float* loss, float* px, float* lag_state, int b_host, hipStream_t s);
void launch_lagged_chain(const MbView& mb, const float* px, int b_host, float* lag_state, hipStream_t s);
/* BPTT (dX, dZ) and, separately, the dense gradient into blk.dense (may run on a second stream:
 * it reads only dZ, X, H) */
void launch_recurrent_backward(const ModelView& m, const MbView& mb, const BlockView& blk, const WorkView& w,
                               int tm_host, int rows_host, int b_host, const int* off_host, hipStream_t s);
/* returns the number of chunk partials left unreduced in w.partials (defer_reduce and more than one chunk), else 0 with blk.dense complete */
int launch_dense_gradient(const ModelView& m, const MbView& mb, const BlockView& blk, const WorkView& w, int rows_host,
                          int b_host, hipStream_t s, bool defer_reduce = false);
void launch_dense_reduce(const ModelView& m, const WorkView& w, int nchunks, const BlockView& blk, hipStream_t s);
void launch_dense_reduce_apply(const ModelView& m, const WorkView& w, int nchunks, const BlockView& blk, hipStream_t s);
/* dense: sum over device blocks in device order + Adagrad (+ repack of the LSTM weights) */
void launch_dense_apply(const ModelView& m, const uint8_t* all_blocks, uint64_t block_bytes, uint64_t dense_off,
                        int ndev, hipStream_t s);
void launch_repack_lstm(const ModelView& m, hipStream_t s);
/* sparse: keys of the device's own entries in (row, entry) order + the list of segment heads (sbr_sort.hip: a
 * stable LSD radix sort over the row bits, key_bits = 32 + bits of a row id; needs only indices and negatives) ->
 * per-row reduction in the contract's chunked order -> one of three consumers: optimiser update (single device),
 * the owners' dense send chunks (replicated multi-device), the position-addressed list + owner bounds
 * (partitioned table).  `keys` is a scratch array of the same size as `keys_sorted`. */
size_t sparse_sort_temp_bytes(size_t max_entries, int key_bits);
/* early_mb != null (single-negative losses): keys from the minibatch's index arrays and the negative-draw hash, i.e.
 * without waiting for the score kernel */
void launch_own_sort(const BlockView& blk, uint32_t rows_host, uint64_t* keys, uint64_t* keys_sorted, void* sort_temp,
                     size_t sort_temp_bytes, int key_bits, const SegScratch& sc, hipStream_t s, const MbView* early_mb = nullptr,
                     uint64_t epoch_key = 0, uint32_t num_items = 0);
void launch_seg_apply(const ModelView& m, const BlockView& blk, uint32_t rows_host, const uint64_t* keys_sorted,
                      const SegScratch& sc, hipStream_t s);
void launch_seg_scatter(const ModelView& m, const BlockView& blk, uint32_t rows_host, int ndev, uint64_t slice_rows,
                        void* send, const uint64_t* keys_sorted, const SegScratch& sc, hipStream_t s);
void launch_seg_list(const ModelView& m, const BlockView& blk, uint32_t rows_host, int ndev, uint64_t slice_rows,
                     const uint64_t* keys_sorted, float* G, float* gbl, uint32_t* fl, uint32_t* bounds, const SegScratch& sc,
                     hipStream_t s);
void launch_owner_reduce(const ModelView& m, const ChunkPtrs& recv, int ndev, uint64_t slice_rows, void* own, hipStream_t s);
void launch_table_apply(const ModelView& m, const ChunkPtrs& table, uint64_t slice_rows, hipStream_t s);
/* owner-applied update: device-order sum of the devices' contributions to the owner's rows [row0, row0 + nrows) and ONE optimiser
 * update of each touched row, in place (owner_reduce + table_apply for the owner's slice in one pass; the parameter slices travel) */
void launch_owner_update(const ModelView& m, const ChunkPtrs& recv, int ndev, uint64_t slice_rows, uint64_t row0, uint64_t nrows, hipStream_t s);
/* partitioned item table: the owner merges the peers' lists (read through peer mappings) in device order
 * and updates its rows */
void launch_owner_list_apply(const ModelView& m, const PeerLists& pl, const PeerBounds& pb, int ndev, int owner, MergePlan* plan,
                             uint32_t capacity, uint64_t* mkeys, uint64_t* mkeys_sorted, void* sort_temp, size_t sort_temp_bytes, hipStream_t s);
/* accumulate loss/examples headers of all blocks into the plan accumulators */
/* owner side of the partitioned table: (row, device, position) keys of the peers' list heads in that order
 * (generated in (device, position) order, so again a stable sort on the row bits) */
void launch_merge_sort(const PeerLists& pl, int ndev, uint32_t total, uint64_t* mkeys, uint64_t* mkeys_sorted, void* sort_temp,
                       size_t sort_temp_bytes, hipStream_t s);
void launch_accumulate_loss(const uint8_t* all_blocks, uint64_t block_bytes, int ndev, double* loss_acc,
                            unsigned long long* ex_acc, hipStream_t s);
/* prediction side (sbr_catalogue.hip).  A launcher of a catalogue scan (the host's scan_launch brackets it as SBR_K_RANK) returns the
 * launches the timing ledger counts for it: the kernels it queued, 0 where it had nothing to do — and launch_rank 1, its scan, as
 * mrr_score has always been counted (its two per-user passes beside the GEMM are not). */
void launch_predict(const ModelView& m, const float* user, const uint32_t* items, uint64_t n, float* out, hipStream_t s);
int launch_rank(const ModelView& m, const float* reps, const int* rep_row, uint32_t num_users, const uint32_t* test_item,
                const uint32_t* test_in_hist, const uint64_t* hist_ptr, const uint32_t* hist_items, float* ts_scratch,
                uint32_t* ranks, uint32_t* nonfinite_flag, hipStream_t s);
/* sequence_ranks' launch: launch_rank's threshold and scan kernels over num_units scan rows, unit i = (sequence b, step t) =
 * unit_bt[i] of the forward pass's packed layout with rep_row[i] = off[t] + b, then rank_prefix_kernel's mask correction over the
 * first occurrences (first_occ, by packed row) among the sequence's inputs in_idx[off[j] + b], j <= t.  test_in_prefix[i]: the
 * target occurs among them.  unit_bt NULL: nothing is masked (off, in_idx, first_occ unread). */
int launch_sequence_ranks(const ModelView& m, const float* reps, const int* rep_row, uint32_t num_units, const uint32_t* test_item,
                          const uint32_t* test_in_prefix, const uint2* unit_bt, const int* off, const uint32_t* in_idx,
                          const uint32_t* first_occ, float* ts_scratch, uint32_t* ranks, uint32_t* nonfinite_flag, hipStream_t s);
/* exact ranks of many targets per user state from one scan (sbr_catalogue.hip).  A scan-user is a representation row rep_row[s]
 * with the targets tgt_items[sptr[s] .. sptr[s + 1]), at most rank_targets_tmax(d) of them and at least one; su_user[s] indexes
 * mask_ptr / mask_items, the sorted de-duplicated lists of items masked to f32::MIN (NULL: none).  ranks [sptr[num_su]] in target
 * order.  Scratch: ts, pos [targets]; th, buckets [num_su][tmax]; tmin, tmin2, totals [num_su]. */
uint32_t rank_targets_tmax(int d);
int launch_rank_targets(const ModelView& m, const float* reps, const int* rep_row, const uint32_t* su_user, const uint32_t* sptr,
                        uint32_t num_su, const uint32_t* tgt_items, const uint64_t* mask_ptr, const uint32_t* mask_items, float* ts,
                        uint32_t* pos, float* th, float* tmin, float* tmin2, uint32_t* buckets, uint32_t* totals, uint32_t* ranks,
                        uint32_t* nonfinite_flag, hipStream_t s);
/* exact top-k of the catalogue per user (sbr_catalogue.hip): topk_gemm_kernel keeps per (user, item range) a sorted list of the
 * k best (score desc, id asc) in `lists` [n][groups][k] with its length in `lens` [n][groups]; topk_merge_kernel merges a user's
 * lists in LDS into out_items / out_scores [n][k] (padding: 0xFFFFFFFF / -inf).  excl_ptr / excl_items: sorted, de-duplicated
 * per-user exclusion lists (excl_ptr NULL: none).  groups * k <= TK_MERGE_MAX.
 * f (f.tags NULL: none): the scan's tag filter (topk_gemm_kernel's TagFilter policy) — device arrays tags [num_items], any_of /
 * none_of [n], none of them NULL; item i is eligible for user u only if (tags[i] & none_of[u]) == 0 && (any_of[u] == 0 ||
 * (tags[i] & any_of[u]) != 0). */
constexpr uint32_t TK_MERGE_MAX = 8192;
struct TagMasks {
    const uint32_t *tags, *any_of, *none_of;
};
/* rank_targets under a restriction (sbr_rank_eligible.h; the contract: ELIGIBLE RANKS in include/sbr_hip.h).  The scan-users are
 * launch_rank_targets'; `cat` is what is scanned — the catalogue, or an item set's sub-table with set_ids its ascending catalogue
 * ids (NULL: the catalogue) — and tgt_items stay catalogue ids.  su_user[s] indexes list_ptr / list_items — per user a
 * non-decreasing segment of positions of cat, repeats and a 0xFFFFFFFF tail allowed (list_ptr NULL: none) — and f.any_of /
 * f.none_of; f.tags [cat.num_items] are the scanned rows' tag words (NULL: no filter, and the scan is rank_targets_gemm_kernel).
 * num_items: the catalogue's, the rank of a target that is masked.  Scratch as launch_rank_targets'. */
struct RankEligible {
    const int* rep_row;
    const uint32_t *su_user, *sptr;
    uint32_t num_su;
    const uint32_t* tgt_items;
    const uint64_t* list_ptr;
    const uint32_t* list_items;
    TagMasks f;
    const uint32_t* set_ids;
    uint32_t num_items;
    float* ts;
    uint32_t* pos;
    float *th, *tmin, *tmin2;
    uint32_t *buckets, *totals, *ranks, *nonfinite_flag;
};
int launch_rank_eligible(const ModelView& cat, const float* reps, const RankEligible& re, hipStream_t s);
/* the noise of a sampled scan (topk_gemm_kernel's GumbelBias policy; keys NULL: not one): inv_t = float(1 / temperature), finite and
 * not zero, and keys [n], the rows' noise keys, which launch_recommend_sampled fills ahead of the scan */
struct SampleNoise {
    float inv_t;
    uint64_t* keys;
};
/* what every top-k scan launch is given beside its catalogue and its A-operand table: device arrays, over the launch's n scan
 * rows ("users": users, query items) */
struct TopkScan {
    const int* rep_row;         /* [n] scan row u's row of the A-operand table */
    uint32_t n;
    const uint64_t* excl_ptr;   /* [n + 1], NULL: no exclusion lists */
    const uint32_t* excl_items;
    uint32_t k;
    uint2* lists;               /* lists / lens: sized by recommend_groups(n, the scanned catalogue's items, k) */
    uint32_t *lens, *out_items;
    float* out_scores;          /* NULL: not wanted */
    uint32_t* nonfinite_flag;
    TagMasks f;
    SampleNoise g;
};
uint32_t recommend_groups(uint32_t num_users, uint32_t num_items, uint32_t k, uint32_t* items_per_group);
int launch_recommend(const ModelView& m, const float* reps, const TopkScan& sc, hipStream_t s);
/* k draws without replacement from softmax(score / T) per scan row (sbr_catalogue.hip; the contract: SAMPLING in include/sbr_hip.h):
 * launch_recommend with the GumbelBias policy — sc.out_scores (not NULL) receives the rows' KEYS, descending — between a prologue
 * that writes sc.g.keys[u] from (seed, streams[u]) and an epilogue that scores the merged rows' (row, item) pairs with
 * launch_candidate_scores into plain [n][k] (padding: -inf).  streams [n], pair_row / pair_item [n k]: device arrays.  Six launches:
 * keys, scan, merge, pairs, scores, padding. */
struct SampleScan {
    uint64_t seed;
    const uint64_t* streams;
    uint32_t *pair_row, *pair_item;
    float* plain;
    const uint32_t* ids = nullptr; /* an item set's scan (m: its sub-table): [m.num_items] ascending, the catalogue id of scanned row
                                      j — the noise is hashed from it (GumbelMapped) and the rows leave as ids; null: m's own rows */
};
int launch_recommend_sampled(const ModelView& m, const float* reps, const TopkScan& sc, const SampleScan& sp, hipStream_t s);
/* the exact fixed-point mass of softmax(score / T) per scan row (sbr_catalogue.hip; the contract: PARTITION in include/sbr_hip.h):
 * launch_recommend at sc.k == 1 (sc.out_scores not NULL) finds each row's best allowed item, partition_shift_kernel writes
 * shift[u] = fl(its score * inv_t) (-inf: nothing allowed) and zeroes mass[u], partition_gemm_kernel adds the weights
 * sbr_softmax_weight(t, shift[u], sbr_softmax_fbits(m.num_items)) of every item that passes sc.f's tag test, and — with
 * exclusion lists — partition_finish_kernel subtracts those of the lists' distinct items.  shift / mass [n]: device arrays.
 * Four or five launches: scan, merge, shift, sum scan, finish. */
struct PartitionScan {
    float inv_t;
    float* shift;
    unsigned long long* mass;
    uint32_t num_items = 0; /* what F is taken from: an item set's scan names its MODEL's items here, so that the mass is the plain
                               call's integer; 0: the scanned catalogue's */
};
int launch_log_partition(const ModelView& m, const float* reps, const TopkScan& sc, const PartitionScan& pt, hipStream_t s);
/* beam search's scan (the contract: BEAM SEARCH in include/sbr_hip.h): launch_recommend at any sc.k (sc.out_scores not NULL), then
 * launch_log_partition's shift, sum scan and finish on the same descriptor — the shift taken from column 0 of the k-row scan, whose
 * first entry IS launch_log_partition's k = 1 pre-scan, so that scan is not run again.  Four or five launches: scan, merge, shift,
 * sum scan, finish. */
int launch_topk_partition(const ModelView& m, const float* reps, const TopkScan& sc, const PartitionScan& pt, hipStream_t s);
/* sequence_partition (sbr_catalogue.hip; the contract: SEQUENCE PARTITION in include/sbr_hip.h): launch_log_partition's shift and
 * mass for scan rows that are (sequence b, step t) = unit_bt[i] of the forward pass's packed layout, as launch_sequence_ranks'
 * (rep_row[i] = off[t] + b; the row's mask: the first occurrences, first_occ by packed row, among in_idx[off[j] + b], j <= t),
 * without a list of size sum(t).  Three launchers, in stream order, sc without exclusion lists or tags in the first and the last:
 * launch_sequence_shift: the top-k scan at sc.k (the pool; sc.out_scores not NULL), then sequence_shift_kernel: pt.shift from the
 *   first pool entry outside the row's prefix, -inf where padding comes first, unresolved[i] = 1 where all sc.k entries are prefix
 *   items; pt.mass zeroed.  unit_bt NULL (nothing masked; sc.k == 1): partition_shift_kernel instead, unresolved untouched.
 * launch_sequence_shift_rows: for the unresolved rows alone, sc over them at k = 1 WITH their sorted distinct prefix lists as its
 *   exclusion CSR; shift[rows[i]] = scan row i's shift.
 * launch_sequence_partition: partition_gemm_kernel over all rows at pt.shift (it adds prefix items too), then
 *   partition_prefix_kernel: the prefix items' weights leave pt.mass (unit_bt NULL: none do) and scores[i] = the plain score of
 *   target[i]. */
struct SequencePartitionScan {
    PartitionScan pt;          /* shift, mass [sc.n] */
    const uint2* unit_bt;      /* [sc.n], NULL: nothing is masked (off, in_idx, first_occ, unresolved unread) */
    const int* off;
    const uint32_t *in_idx, *first_occ;
    const uint32_t* target;    /* [sc.n] */
    float* scores;             /* [sc.n] */
    uint8_t* unresolved;       /* [sc.n] */
};
/* the pool of launch_sequence_shift's scan where rows are masked: 16 unless SBR_SEQ_SHIFT_K=k (1 .. 1 024) is set, a TEST HOOK read
 * per call like SBR_CATALOGUE_GROUPS (the tests force small pools so that rows stay unresolved); no result depends on it */
uint32_t sequence_shift_pool();
int launch_sequence_shift(const ModelView& m, const float* reps, const TopkScan& sc, const SequencePartitionScan& sp, hipStream_t s);
int launch_sequence_shift_rows(const ModelView& m, const float* reps, const TopkScan& sc, float inv_t, const uint32_t* rows, float* shift,
                               hipStream_t s);
int launch_sequence_partition(const ModelView& m, const float* reps, const TopkScan& sc, const SequencePartitionScan& sp, hipStream_t s);
/* every scanned column at or over a per-row score (sbr_catalogue.hip; the contract: ABOVE in include/sbr_hip.h): the catalogue scan
 * with a count-then-write epilogue, above_gemm_kernel.  A column j passes row u if its score is finite and >= thresholds[u] (the f32
 * compare), f's tag test allows it and it is not in the row's exclusion segment (non-decreasing; repeats and a 0xFFFFFFFF tail as
 * the top-k scan takes them).  The item ranges are above_groups' — `groups` of `per` items — the same for both launchers.
 * launch_above_count: counts[u * groups + g] = row u's passes in range g (plain stores, nothing zeroed), then above_offsets_kernel:
 *   offsets[0 .. n groups] their exclusive scan in (row, range) order and totals[u] the rows' sums.  Two launches.
 * launch_above_fill: rows [r0, r0 + nr) write their passes, ascending column, to out_ids / out_scores (NULL: not wanted) at
 *   offsets[u * groups + g] - offsets[r0 * groups], fewer than 2^32 entries per launch, out_cap the buffers' entries; a pass
 *   beyond its slot's end or out_cap is not written and sets *overrun_flag.  One launch.
 * qb NULL: score = b[j] + chain_dot(reps[rep_row[u]], E[j]) of the catalogue `cat` (BiasAdd; f.tags may filter).  qb non-null
 * (audience): score = qb[rep_row[u]] + chain_dot(reps[rep_row[u]], cat.E[j]), cat.b fetched and unused (QueryBias; no filter). */
struct AboveScan {
    const int* rep_row;        /* [n] */
    uint32_t n;
    const float* thresholds;   /* [n]; no NaN */
    const uint64_t* excl_ptr;  /* [n + 1], NULL: no exclusion lists */
    const uint32_t* excl_items;
    TagMasks f;
    uint32_t groups, per;      /* above_groups(n, cat.num_items, &per) */
    uint32_t* counts;          /* [n groups] */
    uint64_t* offsets;         /* [n groups + 1] */
    uint32_t* totals;          /* [n] */
    uint32_t *nonfinite_flag, *overrun_flag;
};
uint32_t above_groups(uint32_t num_rows, uint32_t num_items, uint32_t* items_per_group);
int launch_above_count(const ModelView& cat, const float* reps, const float* qb, const AboveScan& sc, hipStream_t s);
int launch_above_fill(const ModelView& cat, const float* reps, const float* qb, const AboveScan& sc, uint32_t r0, uint32_t nr, uint32_t* out_ids,
                      float* out_scores, uint32_t out_cap, hipStream_t s);
/* the exact best n of a row (sbr_catalogue.hip; the contract: TOP in include/sbr_hip.h): a radix select on the monotone u32 of
 * the scores, 4 bits a round, finds every row's cut — its n-th largest eligible score — without writing a score; the count and
 * fill above then run at thresholds = cuts and the trim keeps exactly n of each row.  Eligible: what launch_above_count would pass
 * at threshold -inf.  All arrays are the caller's device memory, nothing needs zeroing.
 * launch_top_select: 8 rounds of select_gemm_kernel (one catalogue scan each, the ranges of sc.groups / sc.per; integer device
 *   atomics into hist) with select_step_kernel between them, no host round trip: 17 launches.  Leaves cuts[u] (+inf for n = 0, -inf
 *   where fewer than n are eligible, else the n-th score; a zero is +0.0), gt[u] = #{score > cut}, final_counts[u] =
 *   min(n, eligible) and keep_eq[u] = n - gt.  sc.counts / offsets / totals are not touched.
 * launch_top_trim: after launch_above_fill(sc with thresholds = cuts, r0, nr) wrote in_ids / in_scores (both wanted): out_off
 *   [nr + 1] = the exclusive scan of final_counts[r0 ..], and row u's entries over its cut with the first keep_eq[u] that equal it
 *   go, ascending column, to out_ids / out_scores (NULL: not wanted) at out_off[u - r0].  Bounds-checked against in_cap / out_cap
 *   and the row's range; a violation is dropped and sets *sc.overrun_flag.  Two launches. */
struct TopSelect {
    const uint64_t* n;       /* [sc.n] */
    uint64_t* wanted;        /* [sc.n] */
    uint32_t *prefix, *mask; /* [sc.n] */
    uint32_t* hist;          /* [sc.n x 16] */
    float* cuts;             /* [sc.n]: sc.thresholds of the count and fill that follow */
    uint32_t *gt, *final_counts, *keep_eq; /* [sc.n] */
    uint64_t* out_off;       /* [sc.n + 1] */
    uint32_t* out_tot;       /* [sc.n]: scratch of the scan */
};
int launch_top_select(const ModelView& cat, const float* reps, const float* qb, const AboveScan& sc, const TopSelect& ts, hipStream_t s);
int launch_top_trim(const AboveScan& sc, const TopSelect& ts, uint32_t r0, uint32_t nr, const uint32_t* in_ids, const float* in_scores,
                    uint32_t in_cap, uint32_t* out_ids, float* out_scores, uint32_t out_cap, hipStream_t s);
/* An item set S (sorted, unique ids, device) beside launch_recommend_among's sub-table, which launch_subset_gather makes once:
 * launch_subset_words: dst[j] = src[S[j]], the set's tag or group words, per launch.
 * launch_subset_positions: the exclusion CSR eptr / excl of n segments (non-decreasing catalogue ids, repeats and a 0xFFFFFFFF tail
 *   allowed — an uploaded CSR or launch_session_seen_lists' output) becomes, in place, the same segments in positions of S: entries
 *   outside S dropped, repeats kept, the tail refilled; eptr is unchanged.  One launch each (0 where there is nothing to do). */
int launch_subset_words(const uint32_t* subset, uint32_t num_subset, const uint32_t* src, uint32_t* dst, hipStream_t s);
int launch_subset_positions(const uint32_t* subset, uint32_t num_subset, const uint64_t* eptr, uint32_t n, uint32_t* excl, hipStream_t s);
int launch_subset_gather(const ModelView& m, const uint32_t* subset, uint32_t num_subset, float* Esub, float* bsub, hipStream_t s);
/* ids[e] = row_ids[ids[e]] for the n entries a fill wrote (audience: positions in the candidate table -> the ids they stand for) */
int launch_above_ids(const uint32_t* row_ids, uint32_t* ids, uint64_t n, hipStream_t s);
/* greedy maximal-marginal-relevance selection (sbr_catalogue.hip, diverse_select_kernel; the contract: sbr_recommend_diverse in
 * include/sbr_hip.h): pool_items / pool_scores [num_users][pool] are launch_recommend's outputs at k = pool; out_items / out_scores
 * [num_users][k_out] the picks in pick order with their pool scores, padded as the pool's rows.  1 <= k_out <= pool <=
 * diverse_max_pool(d): a user's pool lives in one workgroup's LDS.  Raises the flag for a non-finite squared norm of a pool row
 * (cosine) or a non-finite similarity the selection uses. */
uint32_t diverse_max_pool(int d);
int launch_diverse_select(const ModelView& m, const uint32_t* pool_items, const float* pool_scores, uint32_t num_users, uint32_t pool,
                          uint32_t k_out, float trade_off, bool cosine, uint32_t* out_items, float* out_scores, uint32_t* nonfinite_flag,
                          hipStream_t s);
/* the group cap behind a scan (sbr_catalogue.hip, capped_select_kernel; the contract: CAPPED in include/sbr_hip.h): pool_items /
 * pool_scores [num_users][pool] are launch_recommend's outputs at k = pool (pool_scores and out_scores both null: no scores);
 * item_groups [num_items] the model's group words.  out_items / out_scores [num_users][k_out]: the first k_out entries of each pool
 * row that the rule keeps, padded as the pool's rows; out_complete [num_users] the rows' flags.  1 <= k_out <= pool <= 1 024, cap >= 1. */
int launch_capped_select(const uint32_t* item_groups, uint32_t num_items, const uint32_t* pool_items, const float* pool_scores,
                         uint32_t num_users, uint32_t pool, uint32_t k_out, uint32_t cap, uint32_t* out_items, float* out_scores,
                         uint8_t* out_complete, hipStream_t s);
/* exact top-k neighbours of catalogue items (sbr_catalogue.hip): item_rnorm_kernel writes rnorm [num_items] (1 / |E[i]|, 0 for a zero
 * row; all 1.0f unless `cosine`) and raises the flag for a non-finite squared norm, similar_query_kernel writes the scan rows
 * H [sc.n][d] = E[query[j]] * rnorm[query[j]], and launch_recommend's two kernels rank s(j, i) = chain_dot(H[j], E[i]) *
 * rnorm[i] (no bias) with sc as there: rep_row, the exclusion lists, the tag filter (masks per query), lists / lens and the outputs
 * (the same recommend_groups split). */
int launch_similar_items(const ModelView& m, const uint32_t* query, bool cosine, float* rnorm, float* H, const TopkScan& sc, hipStream_t s);
/* launch_recommend restricted to the item set subset[0 .. num_subset), sorted and unique (sbr_catalogue.hip): subset_gather_kernel
 * copies the set's rows and biases into Esub [num_subset][d] / bsub [num_subset], launch_recommend's two kernels scan that sub-table
 * — sc.lists / lens sized by recommend_groups(sc.n, num_subset, sc.k), sc.excl_items POSITIONS in the subset, no tag filter — and
 * subset_ids_kernel turns out_items' positions into catalogue ids.  Only pairs (user, item of the subset) are scored. */
int launch_recommend_among(const ModelView& m, const uint32_t* subset, uint32_t num_subset, float* Esub, float* bsub, const float* reps,
                           const TopkScan& sc, hipStream_t s);
/* audience, the reverse scan (sbr_catalogue.hip): for each of the sc.n query items q = sc.rep_row[j] the k best rows of the candidate
 * table T [num_rows][d] by s(q, r) = b[q] + chain_dot(E[q], T[r]) — predict's bits for (state T[r], item q) — score descending, ties
 * to the lower row, padded as launch_recommend's rows.  topk_gemm_kernel with the QueryBias policy: reps = E, rep_row = the query
 * items' ids, the scanned ModelView's E = T and its b = bT [num_rows] (fetched, never used: any finite memory;
 * launch_audience_gather zeroes it).  sc.excl_ptr / excl_items: per QUERY a non-decreasing list of row positions (NULL: none);
 * sc.lists / lens sized by recommend_groups(sc.n, num_rows, sc.k); no tag filter.  row_ids non-null (ascending): the positions in
 * sc.out_items become row_ids[position].
 * launch_audience_gather: T[j] = rows_table[rows[j]] (rows of d floats), bT = 0. */
void launch_audience_gather(const ModelView& m, const float* rows_table, const uint32_t* rows, uint32_t num_rows, float* T, float* bT,
                            hipStream_t s);
int launch_audience(const ModelView& m, const float* T, const float* bT, uint32_t num_rows, const uint32_t* row_ids, const TopkScan& sc,
                    hipStream_t s);
/* out[p] = b[i] + chain_dot(reps[pair_row[p]], E[i]), i = pair_item[p], for the num_pairs pairs of a launch, with the bits of
 * launch_predict; raises the flag for a non-finite score.  A launch takes at most candidate_pairs_cap pairs: the host cuts a call's
 * flat candidate list there (12 bytes of device buffers per pair), wherever in a user's list that falls. */
constexpr size_t candidate_pairs_cap = (size_t)1 << 22;
int launch_candidate_scores(const ModelView& m, const float* reps, const uint32_t* pair_row, const uint32_t* pair_item, uint64_t num_pairs,
                            float* out, uint32_t* nonfinite_flag, hipStream_t s);
/* out [num_users][dl] = the first dl columns of rows rep_row[i] of H [.][d] (user_representations) */
int launch_rep_rows(const float* H, const int* rep_row, uint32_t num_users, int d, int dl, float* out, hipStream_t s);
/* session store (sbr_sessions.hip): H [capacity + 1][d] (LSTM h / EWMA s), C likewise (LSTM; null for EWMA), len [capacity + 1];
 * row `capacity` is the empty-history row (one step of item 0 from zero), len[capacity] stays 0 */
struct SessionView {
    float *H, *C;
    unsigned long long* len;
};
/* One append call's n sessions, ordered by item count descending (device arrays unless named host).  LSTM: items time-major, the
 * item of (step t, session b) at items[off_host[t] + b], step t covering sessions [0, off_host[t + 1] - off_host[t]); Hs / Cs: scratch
 * [2][n][d] the steps write alternately.  EWMA: items = the call's id array, session b's at [start[b], start[b] + count[b]).  tm = the
 * largest count (0: nothing is launched).  advance = 0: len is left alone (the empty-history row). */
struct SessionAppend {
    int n, tm;
    const uint32_t *slot, *count, *items;
    const unsigned long long* start;
    const int* off_host;
    float *Hs, *Cs;
    int advance;
};
/* launches queued (LSTM: tm steps + the commit, which alone writes the store; EWMA: one, in place); -1: no kernel for m.d */
int launch_session_append(const ModelView& m, const SessionView& sv, const SessionAppend& a, hipStream_t s);
void launch_session_reset(const SessionView& sv, const uint32_t* slot, int n, int d, hipStream_t s);
/* rows slot[i] <- h_in / c_in [n][dl] (zero where len_in[i] == 0 and past dl), len <- len_in; and the reverse (null outputs skipped) */
void launch_session_set_state(const SessionView& sv, const uint32_t* slot, int n, int d, int dl, const float* h_in, const float* c_in,
                              const unsigned long long* len_in, hipStream_t s);
void launch_session_get_state(const SessionView& sv, const uint32_t* slot, int n, int d, int dl, float* h_out, float* c_out,
                              unsigned long long* len_out, hipStream_t s);
/* seen-item memory of a session store (sbr_sessions.hip): ring [capacity][w], the last w items appended to each slot since its
 * reset — the q-th of them (q from 0) at entry q % w — and cnt [capacity], how many were remembered since then (the valid
 * entries: min(cnt, w), which are entries [0, cnt) while cnt < w and every entry afterwards).  w == 0: a store without memory. */
struct SeenView {
    uint32_t* ring;
    unsigned long long* cnt;
    uint32_t w;
};
/* One append call's ring writes: session b's items ids[start[b] .. start[b] + count[b]) (the call's id array, session-major) to
 * slot slot[b], its last w where count[b] > w, and cnt[slot[b]] += count[b].  One launch. */
void launch_session_seen_append(const SeenView& sn, const uint32_t* slot, const unsigned long long* start, const uint32_t* count,
                                const uint32_t* ids, int n, hipStream_t s);
/* cnt[slot[i]] = 0 (reset, set_state) */
void launch_session_seen_clear(const SeenView& sn, const uint32_t* slot, int n, hipStream_t s);
/* The exclusion CSR a scan of n users reads: segment i = [eptr[i], eptr[i + 1]) of out, eptr[i] = i * w + (entries of the
 * caller's lists before user i) — the ascending merge of slot[i]'s remembered ids (repeats kept) and the caller's sorted,
 * de-duplicated ids caller[eptr[i] - i * w .. eptr[i + 1] - (i + 1) * w), then 0xFFFFFFFF to the segment's end.  One launch (the
 * return value, as the scan launchers'; 0 without sessions or memory). */
int launch_session_seen_lists(const SeenView& sn, const uint32_t* slot, int n, const uint64_t* eptr, const uint32_t* caller, uint32_t* out,
                              hipStream_t s);
/* out_n[i] = slot[i]'s remembered items, out_items[i * w ..] = those, oldest first; and the reverse: slot[i]'s memory = the last
 * w of ids[ptr[i] - ptr[0] .. ptr[i + 1] - ptr[0]) */
void launch_session_seen_get(const SeenView& sn, const uint32_t* slot, int n, uint32_t* out_n, uint32_t* out_items, hipStream_t s);
void launch_session_seen_set(const SeenView& sn, const uint32_t* slot, int n, const uint64_t* ptr, const uint32_t* ids, hipStream_t s);
/* out[i] = cnt[slot[i]] */
void launch_session_seen_counts(const SeenView& sn, const uint32_t* slot, int n, unsigned long long* out, hipStream_t s);
/* The item feed of a replay chunk (sbr_sessions_replay; the plan: sbr_replay_plan.h), written from the rings without a visit to the
 * host: session b = slot slot[b] with count[b] = min(cnt, w) >= 1 items, counts descending, tm = count[0].  off != null (LSTM): the
 * time-major SessionAppend::items, the item of (step t, session b) at items[off[t] + b], off [tm + 1] on the device; off == null
 * (EWMA): session-major, session b's at items[start[b] .. start[b] + count[b]).  The ring and cnt are read only.  One launch (the
 * return value; 0 where nothing is to do). */
int launch_session_replay_feed(const SeenView& sn, const uint32_t* slot, const uint32_t* count, int n, int tm, const int* off,
                               const unsigned long long* start, uint32_t* items, hipStream_t s);
/* A rollout chunk (sbr_sessions.hip; the contract: ROLLOUT in include/sbr_hip.h): n sessions advanced `steps` times by their own
 * picks on scratch memory, the store read only.  Device arrays: slot [n] the sessions' store rows; ident [n] = 0 .. n - 1 and (EWMA)
 * start [n] = 0 .. n - 1, the step kernels' indices into the scratch; Hs / Cs the scratch state — LSTM: [2][n][d] each, written
 * alternately, step j into parity j & 1; EWMA: Hs [n][d] stepped in place with len [n], Cs null; feed / count [n] the next cell step's
 * item and whether the row takes it; ended / lengths [n].
 * launch_rollout_begin: ended = 0, lengths = steps, and for EWMA the scratch rows and lengths copied from the store.
 * launch_rollout_segments: row i's tight non-decreasing segment src[src_ptr[i], src_ptr[i + 1]) to out at src_ptr[i] + i slack, then
 *   `slack` entries of 0xFFFFFFFF.
 * launch_rollout_advance: step j's picks p (stride 1, the scan's outputs; keys / shift / mass null where o's are) into column j of
 *   o [n][steps], the rows' ends, the feed, and — ins_ptr non-null — each live pick into its row's segment [ins_ptr[i],
 *   ins_ptr[i + 1]) of excl, which must end in 0xFFFFFFFF.  With p.ids (an item set's scan) the segments hold positions of the set
 *   and the outputs and the feed catalogue ids (RolloutPick).
 * launch_rollout_step: one cell step of every row by its feed item (LSTM: from the store through `slot` at j == 0; an ended row keeps
 *   its state).  Each returns the launches it queued; launch_rollout_step -1 where there is no kernel for m.d. */
struct RolloutRows {
    int n;
    uint32_t steps;
    const uint32_t *slot, *ident;
    const unsigned long long* start;
    float *Hs, *Cs;
    unsigned long long* len;
    uint32_t *feed, *count, *ended, *lengths;
};
struct RolloutPick {
    const uint32_t* items;
    const float *scores, *keys, *shift;
    const unsigned long long* mass;
    const uint32_t* ids = nullptr; /* an item set's scan: its num_ids ascending catalogue ids; the segments hold positions, the outputs
                                      and the feed ids.  items are positions, or (is_id: the sampled launch maps them) already ids */
    uint32_t num_ids = 0;
    bool is_id = false;
};
struct RolloutOut {
    uint32_t* items;
    float *scores, *keys, *shift;
    unsigned long long* mass;
};
int launch_rollout_begin(const ModelView& m, const SessionView& sv, const RolloutRows& r, hipStream_t s);
int launch_rollout_segments(const uint64_t* src_ptr, const uint32_t* src, int n, uint32_t slack, uint32_t* out, hipStream_t s);
int launch_rollout_advance(const RolloutRows& r, uint32_t j, const RolloutPick& p, const uint64_t* ins_ptr, uint32_t* excl, const RolloutOut& o,
                           hipStream_t s);
int launch_rollout_step(const ModelView& m, const SessionView& sv, const RolloutRows& r, uint32_t j, hipStream_t s);
/* A beam-search chunk (sbr_sessions.hip; the contract: BEAM SEARCH in include/sbr_hip.h): n rows of w beams each, beam b of row i
 * the scan row i w + b, advanced `steps` times on scratch memory, the store read only.  Device arrays: slot [n] the rows' store rows;
 * row_ended / lengths / beams [n]; per beam row [n w]: alive, cum (the beam's path so far), ended (its row has ended: the LSTM
 * carry), in_row (the state row its cell step reads: the store's through the slot at step 0, else the other parity's), src_row (the
 * exclusion segment its own is copied from), feed / count / pick (its cell step's item, whether it takes it, the item merged into
 * its segment); ident / start = 0 .. n w - 1 (the EWMA step's indices); Hs / Cs [2][n w][d] (Cs null: EWMA), len [2][n w] (EWMA).
 * BeamScan: the step's k = w scan over its rows (n at step 0, n w after) — items / scores [rows][w] — and its partition shift / mass
 * [rows] at inv_t with F = fbits.  BeamRecord [steps][n w]: parent, item, score, lp, cum, and (shift null: not wanted) shift, mass.
 * BeamOut: items / scores / lp / shift / mass [n][w][steps], cum [n][w].
 * launch_beam_begin: no row ended, lengths = steps, beams = 0.
 * launch_beam_select: step j's selection (beam_select_kernel), one workgroup per row.
 * launch_beam_segments: nc children's segments [dst_ptr[c], dst_ptr[c + 1]) of dst = segment src_row[c] (null: c / w) of the
 *   src CSR with pick[c] merged in (null: none), padded with 0xFFFFFFFF.
 * launch_beam_step: one cell step of every beam row into parity j & 1 (-1 where there is no kernel for m.d).
 * launch_beam_backtrack: the record walked back into o.  Each returns the launches it queued. */
struct BeamRows {
    int n;
    uint32_t w, steps;
    const uint32_t* slot;
    uint32_t *row_ended, *lengths, *beams;
    uint32_t *alive, *ended, *in_row, *src_row, *feed, *count, *pick;
    float* cum;
    const uint32_t* ident;
    const unsigned long long* start;
    float *Hs, *Cs;
    unsigned long long* len;
};
struct BeamScan {
    const uint32_t* items;
    const float* scores;
    const float* shift;
    const unsigned long long* mass;
    float inv_t;
    uint32_t fbits;
    const uint32_t* ids = nullptr; /* an item set's scan: items are positions of its ascending ids; feed and the record take ids[item] */
};
struct BeamRecord {
    uint32_t *parent, *item;
    float *score, *lp, *cum, *shift;
    unsigned long long* mass;
};
struct BeamOut {
    uint32_t* items;
    float *scores, *lp, *cum, *shift;
    unsigned long long* mass;
};
int launch_beam_begin(const BeamRows& r, hipStream_t s);
int launch_beam_select(const BeamRows& r, uint32_t j, const BeamScan& sc, const BeamRecord& rec, hipStream_t s);
int launch_beam_segments(int nc, uint32_t w, const uint64_t* src_ptr, const uint32_t* src, const uint32_t* src_row, const uint32_t* pick,
                         const uint64_t* dst_ptr, uint32_t* dst, hipStream_t s);
int launch_beam_step(const ModelView& m, const SessionView& sv, const BeamRows& r, uint32_t j, hipStream_t s);
int launch_beam_backtrack(const BeamRows& r, const BeamRecord& rec, const BeamOut& o, hipStream_t s);
/* The inverted seen lists of an audience scan (sbr_sessions.hip): which candidates' memories hold which query item.  The chunk's
 * queries come sorted by item: qs_item [nq] ascending (repeats kept), qs_idx [nq] the query each stands for; candidate position p
 * is slot cand_slot[p].  A key is (query << 32 | position), one per (query, position) whose slot's min(cnt, w) valid ring entries hold
 * the query's item — a repeat in a ring counts once.  launch_audience_seen_count adds the number of keys to *total (zeroed by the
 * caller); launch_audience_seen_fill writes them, in no particular order, to keys[0 .. cap) through the cursor *cursor (zeroed by
 * the caller; a key past cap is dropped, which cannot happen with cap = the count).  nq <= audience_seen_max_queries. */
constexpr uint32_t audience_seen_max_queries = 8192;
void launch_audience_seen_count(const SeenView& sn, const uint32_t* cand_slot, uint32_t num_cand, const uint32_t* qs_item,
                                const uint32_t* qs_idx, uint32_t nq, unsigned long long* total, hipStream_t s);
void launch_audience_seen_fill(const SeenView& sn, const uint32_t* cand_slot, uint32_t num_cand, const uint32_t* qs_item,
                               const uint32_t* qs_idx, uint32_t nq, uint64_t* keys, unsigned long long cap, unsigned long long* cursor,
                               hipStream_t s);
/* sbr_sort.hip: n keys (hi << 32 | lo), generated in any order, into ascending order in place (hi < 2^hi_bits, lo < 2^lo_bits; a, b:
 * scratch of n keys each; temp: pair_sort_temp_bytes(n)) */
size_t pair_sort_temp_bytes(size_t n);
void launch_pair_sort(uint64_t* keys, uint32_t n, int hi_bits, int lo_bits, uint64_t* a, uint64_t* b, void* temp, hipStream_t s);
/* the exclusion CSR of an audience chunk out of its n sorted keys: eptr[j] = the first key of query j or above (j = 0 .. nq, so
 * eptr[nq] = n) and excl[e] = key e's position */
void launch_audience_seen_csr(const uint64_t* keys, uint32_t n, uint32_t nq, uint64_t* eptr, uint32_t* excl, hipStream_t s);
/* device self-tests of the numerics contract (tests/test_numerics_gpu.py) */
void launch_selftest_math(const float* x, float* out_cell_h, float* out_sig, float* out_tanh, uint64_t n, hipStream_t s);
void launch_selftest_dot_tree(const float* x, const float* y, int d, uint64_t nrows, float* out, hipStream_t s);
void launch_selftest_mfma_chain(const float* a, const float* b, const float* c0, int k, float* out, hipStream_t s);
void launch_selftest_mfma32_chain(const float* a, const float* b, int k, float* out, hipStream_t s);
/* the key ordering alone: keys (rows[e] << 32 | e) of n entries in (row, e) order + segment heads */
void launch_selftest_sort(const uint32_t* rows, uint32_t n, int row_bits, uint64_t* tmp, uint64_t* out, void* temp, uint32_t* head_pos,
                          uint32_t* nheads, hipStream_t s);
/* test hook (SBR_TEST_STREAM_DELAY): one wave, no memory traffic, that ends once the constant-rate clock has advanced by `ticks`
 * (or after a fixed number of polls, whichever comes first); *dst = v by one lane (sbr_selftest_stream_delay) */
void launch_stream_delay(unsigned long long ticks, hipStream_t s);
void launch_selftest_store(float* dst, float v, hipStream_t s);

}  // namespace sbr
#endif
