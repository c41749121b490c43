/* sbr_hip.h — C-ABI of libsbr_hip.so, the MI355X (gfx950) engine behind sbr's
 * sequence-recommender hot path.
 *
 * The reference crate (maciejkula/sbr-rs, mounted at /root/reference) has no FFI: its seam is the
 * private trait pair SequenceModelParameters / SequenceModel (src/models/sequence_model.rs:14-45)
 * under the public surface  Hyperparameters::build / fit, OnlineRankingModel, mrr_score and
 * data::CompressedInteractions.  Each entry point below cites the reference interface it
 * replaces; INTEGRATION.md shows the `extern "C"` block a maintainer of the Rust crate would add.
 *
 * Conventions: opaque handles; every call returns an sbr_status (no exceptions cross the ABI);
 * the caller owns all host buffers; the library owns device memory until *_destroy; item ids are
 * u32, CSR user pointers are u64 (reference: usize, src/lib.rs:77-81).  All float data is f32.
 * Calls on one model are not thread-safe except the const ones (user_representation / predict /
 * mrr_score), which serialise internally.
 */
#ifndef SBR_HIP_H
#define SBR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: the two reference error enums (src/lib.rs:84-97) + ABI-level errors ------ */
typedef enum sbr_status {
    SBR_OK = 0,
    SBR_ERR_NO_INTERACTIONS = 1,    /* FittingError::NoInteractions      (lib.rs:93-97)  */
    SBR_ERR_INVALID_PREDICTION = 2, /* PredictionError::InvalidPredictionValue (lib.rs:84-89) */
    SBR_ERR_INVALID_ARGUMENT = 3,
    SBR_ERR_UNSUPPORTED = 4,
    SBR_ERR_NO_DEVICE = 5, /* no gfx950 device / HIP runtime failure: the engine never falls back to CPU */
    SBR_ERR_HIP = 6,
    SBR_ERR_OUT_OF_MEMORY = 7
} sbr_status;

/* ---- enums (src/models/mod.rs:15-41, src/models/lstm.rs:28-35) ------------------------------- */
typedef enum sbr_model_kind { SBR_MODEL_LSTM_NORMAL = 0, SBR_MODEL_LSTM_COUPLED = 1, SBR_MODEL_EWMA = 2 } sbr_model_kind;
typedef enum sbr_loss { SBR_LOSS_BPR = 0, SBR_LOSS_HINGE = 1, SBR_LOSS_WARP = 2 } sbr_loss;
typedef enum sbr_optimizer { SBR_OPT_ADAGRAD = 0, SBR_OPT_ADAM = 1 } sbr_optimizer;
/* Asynchronous with num_devices > 1 = staleness-one pipeline: minibatch k+1 is computed on parameters
 * that lack update k (the deterministic analogue of Hogwild); with one device both are
 * the same step.  sbr_group_fit honours it; a host driving the step halves itself orders them
 * [scatter k, dense k] -> {exchange k || step_local k+1} -> apply_table k. */
typedef enum sbr_parallelism { SBR_PAR_ASYNCHRONOUS = 0, SBR_PAR_SYNCHRONOUS = 1 } sbr_parallelism;

/* ---- hyper-parameters: lstm::Hyperparameters (lstm.rs:39-52) / ewma::Hyperparameters
 * (ewma.rs:45-57).  num_devices plays the role of num_threads (one partition of the shuffled
 * subsequences per device, sequence_model.rs:91-98); batch_sequences is the GPU minibatch:
 * that many subsequences are evaluated against one parameter snapshot and their gradients are
 * summed into one optimiser step (batch_sequences = 1 is the reference's per-sequence SGD). */
typedef struct sbr_hparams {
    uint32_t num_items;
    uint32_t max_sequence_length;
    uint32_t embedding_dim; /* 1 .. 256; widths other than 16 / 32 / 64 / 128 / 256 are stored zero-padded to the next one */
    float learning_rate;
    float l2_penalty;
    int32_t model;       /* sbr_model_kind */
    int32_t loss;        /* sbr_loss */
    int32_t optimizer;   /* sbr_optimizer */
    int32_t parallelism; /* sbr_parallelism */
    uint8_t seed[16];    /* XorShiftRng::from_seed (lstm.rs:129-132) */
    uint32_t num_epochs;
    uint32_t num_devices;      /* world size; this process drives exactly one device */
    uint32_t device_rank;      /* 0 <= rank < num_devices */
    uint32_t batch_sequences;  /* subsequences per optimiser step and device */
} sbr_hparams;

typedef struct sbr_model sbr_model;
typedef struct sbr_fit_plan sbr_fit_plan;

/* Parameter blocks for get/set (golden-vector tests, checkpoint/resume: the serde derives at
 * lstm.rs:204,386 / ewma.rs:208,401).  "*_ACC" are the Adagrad accumulators, which live next to
 * the value in wyrm's HogwildParameter and persist across fit calls. */
typedef enum sbr_param {
    SBR_PARAM_ITEM_EMBEDDING = 0,     /* [num_items][dim]                         */
    SBR_PARAM_ITEM_EMBEDDING_ACC = 1,
    SBR_PARAM_ITEM_BIAS = 2,          /* [num_items]                              */
    SBR_PARAM_ITEM_BIAS_ACC = 3,
    SBR_PARAM_LSTM_W = 4,             /* [2*dim][gates*dim], rows = [x ; h], column blocks i,f,g,o (coupled: f,g,o) */
    SBR_PARAM_LSTM_W_ACC = 5,
    SBR_PARAM_LSTM_B = 6,             /* [gates*dim]                              */
    SBR_PARAM_LSTM_B_ACC = 7,
    SBR_PARAM_EWMA_ALPHA = 8,         /* [dim]                                    */
    SBR_PARAM_EWMA_ALPHA_ACC = 9,
    /* Adam first moments (the "*_ACC" blocks hold the second moments under Adam); empty under Adagrad */
    SBR_PARAM_ITEM_EMBEDDING_M = 10,
    SBR_PARAM_ITEM_BIAS_M = 11,
    SBR_PARAM_LSTM_W_M = 12,
    SBR_PARAM_LSTM_B_M = 13,
    SBR_PARAM_EWMA_ALPHA_M = 14
} sbr_param;

/* Per-minibatch intermediates that tests fetch to compare against the oracle. */
typedef enum sbr_debug_buffer {
    SBR_DBG_HIDDEN = 0,     /* f32 [R][dim]   h_t (LSTM) / s_t (EWMA), packed time-major rows */
    SBR_DBG_NEGATIVES = 1,  /* u32 [R]        sampled negative item ids                         */
    SBR_DBG_COEF = 2,       /* f32 [R]        dloss/dneg                                        */
    SBR_DBG_LOSS = 3,       /* f32 [R]        loss terms                                        */
    SBR_DBG_DHIDDEN = 4,    /* f32 [R][dim]   dloss/dh from the scoring step                    */
    SBR_DBG_DINPUT = 5,     /* f32 [R][dim]   gradient w.r.t. the gathered input embedding      */
    SBR_DBG_DENSE_GRAD = 6, /* f32 dense grad block: LSTM [2*dim+1][gates*dim] (last row = bias) / EWMA [dim] */
    SBR_DBG_IN_IDX = 7,     /* u32 [R] */
    SBR_DBG_OUT_IDX = 8,    /* u32 [R] */
    SBR_DBG_TRIES = 9,      /* u32 [R] number of negatives scored (k of BASELINE.md §4) */
    SBR_DBG_DZ = 10         /* f32 [R][gates*dim] gradient w.r.t. the gate pre-activations (LSTM; column blocks as SBR_PARAM_LSTM_W) */
} sbr_debug_buffer;

/* ≙ Hyperparameters::build (lstm.rs:197-201, ewma.rs:201-205): allocates device parameters and
 * initialises them from hp->seed (embedding_init lstm.rs:22-25; biases, alpha zero). */
sbr_status sbr_model_create(const sbr_hparams* hp, sbr_model** out);
void sbr_model_destroy(sbr_model* m);

/* ≙ ImplicitLSTMModel::fit / ImplicitEWMAModel::fit (lstm.rs:395-397, ewma.rs:408-410) →
 * fit_sequence_model (sequence_model.rs:70-178).  CSR = CompressedInteractions
 * (data.rs:227-234): user_ptr[num_users+1], item_ids[user_ptr[num_users]], time-sorted per user.
 * Re-callable: every call trains num_epochs more epochs, optimiser state persists.
 * Returns SBR_ERR_NO_INTERACTIONS when no subsequence of length > 2 exists (:86-88). */
sbr_status sbr_model_fit(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids,
                         uint64_t num_users, float* out_loss);

/* The same fit, staged, so a caller (bench.py, the multi-GPU driver) can keep inputs resident in
 * HBM and time / interleave individual optimiser steps:
 *   begin          = chunking + shuffle + partition      (sequence_model.rs:76-98)
 *   epoch_prepare  = per-epoch reshuffle (:109) + packing + upload; returns #minibatches
 *   step           = one minibatch: forward, negative sampling, loss, BPTT, optimiser (:111-169)
 *   step_local/step_apply = the two halves of step (compute, optimiser); multi-device: see below
 *   end            = ≙ the fold at :173-177; returns loss_sum / (1 + examples)            */
sbr_status sbr_fit_begin(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids,
                         uint64_t num_users, sbr_fit_plan** out);
sbr_status sbr_fit_epoch_prepare(sbr_fit_plan* p, uint64_t* out_num_minibatches);
/* Optional: start shuffling/packing/uploading the NEXT epoch on a host thread while the device works
 * on the current one; the following sbr_fit_epoch_prepare consumes it.  Call only if another epoch
 * follows (the shuffle advances the partition RNGs and the epoch counter). */
sbr_status sbr_fit_epoch_prefetch(sbr_fit_plan* p);
sbr_status sbr_fit_step(sbr_fit_plan* p, uint64_t minibatch);
/* `count` consecutive optimiser steps from `first` (= that many sbr_fit_step calls; sbr_model_fit runs every epoch as ONE such
 * call).  At the reference's own schedule — one subsequence per optimiser step, sequence_model.rs:111-169 (batch_sequences = 1) — with
 * a single-negative loss (hinge, BPR) and Adagrad, a run of steps is ONE kernel launch — EWMA at embedding_dim <= 32 and
 * max_sequence_length <= 129; the LSTM (Normal) at embedding_dim 32 for steps of at most 48 rows (longer steps inside an epoch take
 * the separate launches, the run resumes behind them): one workgroup walks the steps with each step's working set in LDS (one gather
 * per step; nobody else touches the parameters at one sequence per step).  Same bits as the separate launches.  Single device. */
sbr_status sbr_fit_steps(sbr_fit_plan* p, uint64_t first, uint64_t count);
/* How one-sequence steps at embedding_dim <= 32 are launched: 0 = one launch per kernel family (eight per step), 1 = fused
 * launches (LSTM four per step: forward, scoring + header + key ordering, BPTT, gradient + updates; EWMA two), 2 (default) =
 * additionally runs of steps in one launch through sbr_fit_steps / sbr_model_fit where the shape allows.  No result bit depends
 * on it (tests run all three). */
sbr_status sbr_model_set_step_fusion(sbr_model* m, int32_t level);
/* REFERENCE ORDER of the negatives (one subsequence per step; every embedding_dim; steps whose h rows and 64-draw candidate window fit
 * one workgroup's LDS: max_sequence_length <= 256 at embedding_dim <= 64, <= 221 at <= 128, <= 81 at <= 256): the
 * negatives of a step are drawn from the worker's own sequential generator exactly as sequence_model.rs:58-65 / :137 draw them —
 * `Uniform::new(0, num_items).sample(thread_rng)` (rand 0.5 as recalled), one draw per try, the same generator that shuffles the
 * worker's partition every epoch (:109) — instead of the engine's counter-keyed draws (which exist so that draws can be evaluated in
 * parallel).  Everything else of a worker's step is unchanged.  Checked bit for bit against the oracle's reference-order mode; SBR_ERR_UNSUPPORTED outside
 * the shapes above.  Set before sbr_model_fit / sbr_fit_begin. */
sbr_status sbr_model_set_reference_order(sbr_model* m, int32_t on);
/* ... with several workers (Parallelism::Synchronous, replicated table): every worker's gradient is applied as its OWN optimiser
 * step, one after the other in worker order (sequence_model.rs:163-166; n Adagrad applications per step where the contract sums
 * the devices' gradients and applies one).  sbr_group_fit / sbr_group_step do this when the replicas are in reference order; hosts
 * that drive one process per GPU gather the devices' local blocks (sbr_fit_block_bytes each, block q at q * bytes; after
 * sbr_fit_step_local) and call sbr_fit_step_apply_blocks_in_order on every rank. */
sbr_status sbr_fit_block_bytes(const sbr_fit_plan* p, uint64_t* out_bytes);
sbr_status sbr_fit_step_apply_blocks_in_order(sbr_fit_plan* p, uint64_t minibatch, const void* device_blocks);
/* Profiling aid of the one-launch step runs: shader-clock ticks of the run's workgroup summed per phase since sbr_fit_begin —
 * [0] ids, key ordering, gather, [1] scan + scores, [2] backward scan, [3] reduction + updates, [4] closing barrier — and [5] the steps. */
sbr_status sbr_fit_debug_phase_clocks(sbr_fit_plan* p, uint64_t out[6]);
sbr_status sbr_fit_minibatch_rows(const sbr_fit_plan* p, uint64_t minibatch, uint64_t* out_rows);
sbr_status sbr_fit_end(sbr_fit_plan* p, float* out_loss, uint64_t* out_examples);
/* The number the reference's `fit` returns.  sequence_model.rs:157 adds `loss.value()` of the loss node BEFORE :160 runs its
 * forward pass; the loss nodes are shared running sums (lstm.rs:322-328), so a subsequence of s steps contributes the running sum
 * L_{s-1} of the worker's most recent earlier subsequence with AT LEAST s steps (0 if none since this fit began), accumulated in f32; `fit` returns the sum over the workers of accumulator / (1 + examples) (:173-177).
 * sbr_fit_end / sbr_model_fit report the true mean instead; this is the lagged figure for a caller that must return what the
 * crate returns.  sbr_fit_end_lagged: THIS device's term (single device: the whole figure; multi-device hosts add the terms in
 * device order in f32).  sbr_model_last_fit_lagged_loss: the whole figure of the last completed sbr_model_fit / sbr_group_fit. */
sbr_status sbr_fit_end_lagged(sbr_fit_plan* p, float* out_term);
sbr_status sbr_model_last_fit_lagged_loss(const sbr_model* m, float* out_loss);
/* Running totals of the plan, all devices: loss terms processed and negatives scored by the WARP
 * search (the k of BASELINE.md §4's bytes-per-interaction formula). */
sbr_status sbr_fit_counters(sbr_fit_plan* p, uint64_t* out_examples, uint64_t* out_negatives_scored);
/* The last step's sparse update on this device: gradient entries (3 per loss term: input, target and
 * negative row) and the distinct item-table rows they touch (each is read-modified-written once,
 * sequence_model.rs:163-169) — what the real HBM traffic of the update is priced from. */
sbr_status sbr_fit_sparse_stats(sbr_fit_plan* p, uint64_t* out_entries, uint64_t* out_unique_rows);
void sbr_fit_plan_destroy(sbr_fit_plan* p);

/* The two halves of a single-device step (sbr_fit_step = local + apply).  With one device sbr_fit_step_local COMMITS the
 * minibatch's loss terms and example count to the plan's totals (sbr_fit_end / sbr_fit_counters) — the header launch that
 * closes the scoring pass adds them — whether or not sbr_fit_step_apply follows; the exchange halves below do not count them a
 * second time. */
sbr_status sbr_fit_step_local(sbr_fit_plan* p, uint64_t minibatch);
sbr_status sbr_fit_step_apply(sbr_fit_plan* p, uint64_t minibatch);

/* Multi-device step (user-sharded data parallelism, one process per GPU; ≙ the rendezvous of
 * Parallelism::Synchronous, sequence_model.rs:163-166).  Table rows are owned in contiguous slices
 * of ceil(num_items / num_devices) rows.  Per step, after sbr_fit_step_local:
 *   scatter      : own entries reduced per row into num_devices dense chunks (send buffer, one chunk
 *                  per owner; chunk = [G: S*dim f32][gb: S f32][flags: S u32])
 *                                                                     -> host: all-to-all of the chunks
 *   dense        : the small dense block [8-word header | dense grads]; call it after the all-to-all
 *                  has been queued: it waits for the dense-gradient GEMM, which then overlaps the transfer
 *   owner_reduce : the devices' contributions for the owned slice, added in device order -> one chunk
 *                                                                     -> host: all-gather of the chunks
 *                                                                        and of the dense blocks
 *   apply_table  : every device applies the identical update (replicas stay bit-identical).
 * All pointers are device pointers supplied by the host (torch tensors in sbr_rs_amd/distributed.py). */
sbr_status sbr_fit_chunk_bytes(const sbr_fit_plan* p, uint64_t* out_bytes);
sbr_status sbr_fit_dense_bytes(const sbr_fit_plan* p, uint64_t* out_bytes);
sbr_status sbr_fit_step_scatter(sbr_fit_plan* p, uint64_t minibatch, void* device_send);
sbr_status sbr_fit_step_dense(sbr_fit_plan* p, void* device_dense_out);
sbr_status sbr_fit_step_owner_reduce(sbr_fit_plan* p, const void* device_recv, void* device_own_chunk);
/* The same kernel launched on `hip_stream` instead of the model's stream, without synchronising either: the
 * caller orders the two streams itself (events / wait_stream).  What the staleness-one pipeline
 * (Parallelism::Asynchronous) uses to keep the exchange of step k on a side stream underneath the computation
 * of step k+1. */
sbr_status sbr_fit_step_owner_reduce_on(sbr_fit_plan* p, const void* device_recv, void* device_own_chunk, void* hip_stream);
sbr_status sbr_fit_step_apply_table(sbr_fit_plan* p, const void* device_table, const void* device_dense_all);
/* sbr_fit_step_apply_table in two halves: the item-table rows (needs only the gathered chunks, so it can be enqueued
 * while the dense-gradient GEMM is still running on the engine's side stream), then the dense parameters (after
 * sbr_fit_step_dense has joined that GEMM and the dense blocks have been gathered).  Rows first — it opens the
 * optimiser step —, dense second, once each per step; same bits as the one-call form. */
sbr_status sbr_fit_step_apply_rows(sbr_fit_plan* p, const void* device_table);
sbr_status sbr_fit_step_apply_dense(sbr_fit_plan* p, const void* device_dense_all);

/* OWNER-APPLIED update — the Synchronous step of a replicated table since round 6 (≙ the ONE shared parameter and optimiser state
 * behind every worker, lstm.rs:259-260 / ewma.rs:267-269, under the synchronised step of sequence_model.rs:163-169).  Per step, after
 * sbr_fit_step_local:
 *   scatter (as above)                                                   -> host: all-to-all of the chunks
 *   owner_update : the devices' contributions to the owned slice added in device order AND the one optimiser update of every touched
 *                  row of that slice, in place in this replica (opens the optimiser step)
 *                                                                        -> host: all-gather, IN PLACE, of the updated PARAMETER slices:
 *                                                                           sbr_model_table_slice(ITEM_EMBEDDING) and (ITEM_BIAS)
 *   dense + all-gather of the dense blocks + apply_dense (as above)
 * Same sums in the same order and the same update arithmetic as owner_reduce + apply_rows — bit-identical results — and the same
 * bytes on the links, but no replica walks the whole table (sbr_fit_step_apply_rows visits every row's flag on every device) and a
 * row's optimiser state is maintained by its owner alone.  Consequence: while such a fit runs, a replica's copy of the item table's
 * optimiser state (SBR_PARAM_ITEM_*_ACC / _M) is current for its OWN rows only; sbr_model_get_param on those blocks and the
 * gradient-all-gather halves (apply_table / apply_rows) return SBR_ERR_INVALID_ARGUMENT until the host has all-gathered those blocks
 * too (same in-place slices) and called sbr_model_optimizer_state_gathered — the library's own drivers (sbr_group_fit_end,
 * sbr_model_fit_comm) and sbr_rs_amd/distributed.py do that when a fit ends.  The staleness-one pipeline (Asynchronous) keeps the
 * gradient all-gather: its update lands one step late on every replica.
 *   sbr_model_table_slice: device pointer of an item-table block of THIS replica (allocated for num_devices slices of
 *   ceil(num_items / num_devices) rows each, so that slices are equally long) and the bytes of one slice: rank r's slice is
 *   [base + r * slice_bytes, + slice_bytes).  which: SBR_PARAM_ITEM_EMBEDDING / _ACC / _M, SBR_PARAM_ITEM_BIAS / _ACC / _M; base = NULL
 *   for a block the model does not have (Adam moments under Adagrad). */
sbr_status sbr_fit_step_owner_update(sbr_fit_plan* p, const void* device_recv);
sbr_status sbr_model_table_slice(sbr_model* m, int32_t which, void** out_base, uint64_t* out_slice_bytes);
sbr_status sbr_model_optimizer_state_gathered(sbr_model* m);
sbr_status sbr_model_optimizer_state_is_partial(const sbr_model* m, int32_t* out);

/* The same multi-device fit driven from ONE process (≙ fit with num_threads(n) on one host,
 * sequence_model.rs:90-102): models[r] was created with num_devices = n, device_rank = r, the same
 * seed, on the device that was current at its creation (sbr_set_device).  The exchange runs as
 * peer copies between the devices' streams, ordered with events; results are bit-identical to the
 * one-process-per-GPU driver.  n = 1 is sbr_model_fit. */
sbr_status sbr_group_fit(sbr_model* const* models, uint32_t n, const uint64_t* user_ptr, const uint32_t* item_ids,
                         uint64_t num_users, float* out_loss);
sbr_status sbr_device_count(int32_t* out_count);

/* sbr_group_fit taken apart, for a host that wants the group's steps one at a time (a progress bar, early stopping, the bench's
 * `--driver group`, the parity tests): begin -> per epoch [epoch_prepare -> step(0) .. step(n_minibatches - 1)] -> fit_end.
 * sbr_group_fit IS this sequence over hp.num_epochs epochs.  (≙ the loop of sequence_model.rs:100-171 with num_threads(n).)
 *   sbr_group_epoch_prepare   every replica's sbr_fit_epoch_prepare (prefetch_next != 0: the next epoch is packed in the background)
 *   sbr_group_step            one optimiser step of the whole group (Synchronous / partitioned / the staleness-one pipeline);
 *                             returns when it is QUEUED on the devices' streams (a partitioned step too since round 6: its owners
 *                             wait for the devices' events on their streams and read the owner bounds on the device)
 *                             A partitioned table's rows are updated on their OWNERS' streams: a prediction-side call or
 *                             sbr_model_get_param on any replica between steps waits, on that replica's stream, for the other
 *                             owners' last updates first, so it may follow sbr_group_step without a sbr_group_synchronize.
 *   sbr_group_step_local      parity access: only the local halves of `minibatch` (forward, scoring, BPTT on every replica); the
 *                             next sbr_group_step(minibatch) then runs the exchange and the update alone.  Not for Asynchronous.
 *   sbr_group_member_plan     replica r's plan, borrowed (sbr_fit_debug_fetch, sbr_fit_minibatch_rows, sbr_fit_counters)
 *   sbr_group_plan_set_host_threads   one host thread per device queues that device's launches (the reference runs one rayon
 *                             worker per partition, sequence_model.rs:100-102); default: from four devices on.  Same bits.
 *   sbr_group_plan_stats      host time spent inside sbr_group_step so far, the number of steps, the host threads in use
 *   sbr_group_fit_end         the loss of sbr_group_fit; destroys the plan.  sbr_group_plan_destroy: abandon a plan. */
typedef struct sbr_group_plan sbr_group_plan;
sbr_status sbr_group_fit_begin(sbr_model* const* models, uint32_t n, const uint64_t* user_ptr, const uint32_t* item_ids,
                               uint64_t num_users, sbr_group_plan** out);
sbr_status sbr_group_epoch_prepare(sbr_group_plan* g, uint64_t* out_num_minibatches, int32_t prefetch_next);
sbr_status sbr_group_step(sbr_group_plan* g, uint64_t minibatch);
sbr_status sbr_group_step_local(sbr_group_plan* g, uint64_t minibatch);
sbr_status sbr_group_member_plan(sbr_group_plan* g, uint32_t replica, sbr_fit_plan** out);
sbr_status sbr_group_synchronize(sbr_group_plan* g);
sbr_status sbr_group_plan_set_host_threads(sbr_group_plan* g, int32_t enable);
sbr_status sbr_group_plan_stats(const sbr_group_plan* g, double* out_host_enqueue_ms, uint64_t* out_steps, int32_t* out_host_threads);
/* The Synchronous step of a replicated group is the owner-applied update (sbr_fit_step_owner_update: parameter slices travel, in
 * place); gradient_all_gather != 0 selects the gradient all-gather + whole-table update of rounds 1-5 instead (A/B measurements and
 * the parity tests of those halves; the pipeline always runs it).  Same bits.  sbr_group_gather_optimizer_state: every replica's
 * copy of the item table's optimiser state made complete from the owners' slices — sbr_group_fit_end does it; a host that reads
 * SBR_PARAM_ITEM_*_ACC between steps calls it first. */
sbr_status sbr_group_plan_set_exchange(sbr_group_plan* g, int32_t gradient_all_gather);
sbr_status sbr_group_gather_optimizer_state(sbr_group_plan* g);
sbr_status sbr_group_fit_end(sbr_group_plan* g, float* out_loss);
void sbr_group_plan_destroy(sbr_group_plan* g);

/* Builds the n replicas of a single-process group in one call (replica r on HIP device r mod device
 * count; destroy each with sbr_model_destroy).  flags = 0: n full parameter replicas, exactly what n
 * sbr_model_create calls give.  SBR_GROUP_PARTITION_ITEM_TABLE (BASELINE configs[4]): the
 * item table (embeddings, biases and their optimiser state) exists ONCE — rows [r*S, (r+1)*S),
 * S = ceil(num_items / n), live on replica r's device and are mapped into every replica's address space
 * (HIP virtual memory management; remote rows are read over xGMI by the unchanged gather kernels).  In
 * sbr_group_fit each row is then updated by its owner only, from the devices' gradient lists merged in
 * device order: bitwise the same result as the replicated Synchronous exchange, with per-step traffic
 * proportional to the batch instead of to the table.  Prediction / mrr_score / get_param work on any
 * replica.  Parallelism::Asynchronous over a partitioned table runs the synchronous step (the owners update in
 * place after a rendezvous; there is no staleness-one pipeline to run) — in sbr_group_fit, under one process per GPU
 * and with the peer transport alike, so that a hyper-parameter draw never decides whether a configuration can run. */
#define SBR_GROUP_PARTITION_ITEM_TABLE 1u
sbr_status sbr_group_create(const sbr_hparams* hp, uint32_t n, uint32_t flags, sbr_model** out_models);
sbr_status sbr_model_is_partitioned(const sbr_model* m, int32_t* out);

/* The partitioned item table under ONE PROCESS PER GPU (the launcher model of bench.py --gpus N).  Every
 * process creates its model with the same hyper-parameters (num_devices = world, device_rank = its rank) on
 * its own device; the shared virtual range is planned identically everywhere and the parts (runs of pages)
 * homed on this rank are allocated.  The host then passes file descriptors between the processes
 * (SCM_RIGHTS over a Unix socket; sbr_rs_amd/partitioned.py): every part is exported by its home rank and
 * imported by all the others; sbr_partition_finalize then writes this rank's rows (the seeded initial
 * embeddings, zeroed optimiser state).  The fit is sequenced by the host:
 *   sbr_fit_lists_export / _import   once per plan: the ranks' gradient lists become readable by their peers
 *   per step: sbr_fit_step_local -> sbr_fit_step_reduce_own (returns this rank's owner bounds; stream
 *   drained) -> all-gather of the bounds and of the dense blocks -> sbr_fit_step_owner_apply (stream
 *   drained) -> barrier;  or, nothing drained, the *_queued forms below.
 * Same bits as sbr_group_fit over a partitioned group and as the replicated Synchronous exchange. */
/* Peer transport of the REPLICATED exchange (one process per GPU): every rank exports its send buffer and
 * its reduced own chunk once; the owner-reduce and table-update kernels then read the peers' buffers in
 * place through peer mappings (xGMI), so no bulk collective is involved.  Host sequencing per step:
 *   sbr_fit_step_local -> sbr_fit_step_scatter_shared -> barrier -> sbr_fit_step_owner_reduce_peers ->
 *   sbr_fit_step_dense + all-gather of the dense blocks (a barrier as well) -> sbr_fit_step_apply_table_peers
 *   -> barrier.  Every call returns with the stream drained.  Same bits as the collective transport. */
sbr_status sbr_fit_exchange_export(sbr_fit_plan* p, int32_t out_fds[2], uint64_t out_bytes[2]);
sbr_status sbr_fit_exchange_import(sbr_fit_plan* p, uint32_t peer_rank, const int32_t fds[2], const uint64_t bytes[2]);
sbr_status sbr_fit_step_scatter_shared(sbr_fit_plan* p, uint64_t minibatch);
sbr_status sbr_fit_step_owner_reduce_peers(sbr_fit_plan* p);
sbr_status sbr_fit_step_apply_table_peers(sbr_fit_plan* p, const void* device_dense_all);

sbr_status sbr_model_create_partitioned(const sbr_hparams* hp, sbr_model** out);
sbr_status sbr_partition_num_parts(const sbr_model* m, uint32_t* out);
sbr_status sbr_partition_part_info(const sbr_model* m, uint32_t part, uint32_t* out_home_rank, uint64_t* out_bytes);
sbr_status sbr_partition_export_part(sbr_model* m, uint32_t part, int32_t* out_fd);
sbr_status sbr_partition_import_part(sbr_model* m, uint32_t part, int32_t fd);
sbr_status sbr_partition_finalize(sbr_model* m);
sbr_status sbr_fit_lists_export(sbr_fit_plan* p, int32_t out_fds[4], uint64_t out_bytes[4]);
sbr_status sbr_fit_lists_import(sbr_fit_plan* p, uint32_t peer_rank, const int32_t fds[4], const uint64_t bytes[4]);
sbr_status sbr_fit_step_reduce_own(sbr_fit_plan* p, uint64_t minibatch, uint32_t* host_bounds, void* device_dense_out);
sbr_status sbr_fit_step_owner_apply(sbr_fit_plan* p, const uint32_t* all_bounds, const void* device_dense_all);
/* The same two halves WITHOUT the host in the loop (round 6), for hosts whose collectives run on the device (RCCL): nothing is
 * drained and nothing is read back.  reduce_own_queued leaves this rank's owner bounds (num_devices + 1 u32) on the device and
 * returns their address; the host all-gathers the ranks' bounds and dense blocks with DEVICE collectives on the model's stream (a
 * collective completes on a rank only after every rank's contribution: every rank has finished reading the table); the owner
 * builds its merge plan from the gathered bounds on the device (rank r's bounds at r * (num_devices + 1) words) and updates its
 * rows; a last small device collective keeps the next step's reads behind every owner's writes.  Same bits. */
sbr_status sbr_fit_step_reduce_own_queued(sbr_fit_plan* p, uint64_t minibatch, void** out_device_bounds, void* device_dense_out);
sbr_status sbr_fit_step_owner_apply_queued(sbr_fit_plan* p, const void* device_all_bounds, const void* device_dense_all);

/* The rendezvous of a step through RCCL INSIDE the library — for hosts that run one process per GPU and have no collective library
 * of their own (≙ the synchronised optimiser step of sequence_model.rs:92, 163-166 across processes; xGMI within a node).  librccl
 * is opened at run time; hosts that bring their own transport (torch.distributed, MPI: the sbr_fit_step_scatter / _owner_reduce /
 * _apply_* halves above) never load it.
 *   sbr_comm_unique_id    rank 0 makes the 128-byte id; the host hands it to the other ranks (a file, a socket, an environment
 *                         variable: any channel)
 *   sbr_comm_create       every rank, on its own device (sbr_set_device first), with the same id
 *   sbr_fit_step_exchange after sbr_fit_step_local: scatter -> all-to-all -> owner update (in place) -> all-gather of the updated
 *                         parameter slices into every replica's table, dense block -> all-gather -> dense update, all queued on
 *                         the model's stream; same bits as every other transport
 *   sbr_model_fit_comm    the whole fit of this rank (sbr_model_fit for num_devices = world across processes); the loss is the
 *                         all-rank figure, sbr_model_last_fit_lagged_loss holds THIS rank's term of the reference's figure
 * Replicated table, Parallelism::Synchronous order of work.  SBR_ERR_UNSUPPORTED: no librccl on this host. */
typedef struct sbr_comm sbr_comm;
sbr_status sbr_comm_unique_id(uint8_t out_id[128]);
sbr_status sbr_comm_create(const uint8_t id[128], uint32_t world, uint32_t rank, sbr_comm** out);
void sbr_comm_destroy(sbr_comm* c);
sbr_status sbr_fit_step_exchange(sbr_fit_plan* p, uint64_t minibatch, sbr_comm* c);
/* after the last sbr_fit_step_exchange of a fit driven step by step: the owners' optimiser-state slices all-gathered in place
 * (sbr_model_fit_comm does it itself) */
sbr_status sbr_comm_gather_optimizer_state(sbr_model* m, sbr_comm* c);
sbr_status sbr_model_fit_comm(sbr_model* m, sbr_comm* c, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users,
                              float* out_loss);

/* Device pointer / stream plumbing for the host side (torch only supplies memory + streams). */
sbr_status sbr_model_set_stream(sbr_model* m, void* hip_stream);
sbr_status sbr_model_synchronize(sbr_model* m);

/* Debug / parity access to the last minibatch processed by sbr_fit_step*. */
sbr_status sbr_fit_debug_fetch(sbr_fit_plan* p, int32_t which, void* host_out, uint64_t bytes);

/* ≙ OnlineRankingModel::user_representation (lib.rs:105-108; impl sequence_model.rs:182-211):
 * keeps the last max_sequence_length items; empty history = step 0 with item 0. */
sbr_status sbr_user_representation(sbr_model* m, const uint32_t* item_ids, uint64_t n, float* out_dim);
/* ≙ OnlineRankingModel::predict (lib.rs:111-115; impl sequence_model.rs:213-232):
 * out[i] = bias[item_ids[i]] + <user, E[item_ids[i]]>; SBR_ERR_INVALID_PREDICTION if any is non-finite. */
sbr_status sbr_predict(sbr_model* m, const float* user_dim, const uint32_t* item_ids, uint64_t n, float* out);
/* ≙ evaluation::mrr_score (evaluation.rs:12-48).  out_ranks (optional) receives one u32 rank per
 * test user with >= 2 interactions, in user order; out_num_ranked their count. */
sbr_status sbr_mrr_score(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids,
                         uint64_t num_users, float* out_mrr, uint32_t* out_ranks, uint64_t* out_num_ranked);

/* Exact top-k of the whole catalogue per user (no counterpart in the reference crate: user_representation + predict over every
 * item + a sort, on the device).  score(u, i) = bias[i] + <rep_u, E[i]> with the bits of sbr_predict; rows sorted by score
 * descending, ties to the lower item id (-0.0 == +0.0).  out_items / out_scores (optional): [num_users][k].  A row with fewer than
 * k eligible items is padded with item 0xFFFFFFFF and score -inf.  1 <= k <= SBR_RECOMMEND_MAX_K.  SBR_ERR_INVALID_PREDICTION if
 * any score of a scored user is non-finite.  Deterministic.
 * sbr_recommend: user u's history is item_ids[user_ptr[u] .. user_ptr[u + 1]) (the layout of sbr_mrr_score); its representation is
 * that of sbr_user_representation (last max_sequence_length items; empty = item 0), every user gets a row, and every item of the
 * whole history is excluded unless flags has SBR_RECOMMEND_INCLUDE_HISTORY.
 * sbr_recommend_reps: from representations (embedding_dim floats each, as sbr_user_representation returns them); excl_ptr /
 * excl_items: optional per-user exclusion lists (CSR; both NULL = none). */
#define SBR_RECOMMEND_MAX_K 1024u
#define SBR_RECOMMEND_INCLUDE_HISTORY 1u
sbr_status sbr_recommend(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users,
                         uint32_t k, uint32_t flags, uint32_t* out_items, float* out_scores);
sbr_status sbr_recommend_reps(sbr_model* m, const float* reps, uint64_t num_users, uint32_t k,
                              const uint64_t* excl_ptr, const uint32_t* excl_items, uint32_t* out_items, float* out_scores);

/* Diversified top-k: a greedy maximal-marginal-relevance (MMR) selection of k items from the pool of a user's best `pool` items (no
 * counterpart in the reference crate: recommend(k = pool) to the host, the pool's rows after it, and a loop per user).  With
 * chain_dot, n2[i] and r[i] exactly as in sbr_similar_items below (SBR_SIMILAR_DOT: r == 1.0f), per user:
 *   POOL       c_0 .. c_{n-1} with scores s_0 .. s_{n-1}: the non-padding entries of the row sbr_recommend / sbr_recommend_reps /
 *              sbr_sessions_recommend returns with k = pool — the same masking, order and score bits — so n <= pool.
 *   SIMILARITY of a picked item a to a pool item j: sim(a, j) = chain_dot(E[a] * r[a], E[c_j]) * r[c_j], which is
 *              sbr_similar_items' s(q = a, i = c_j) with the picked item as the query.  Bit-wise it is not symmetric: the
 *              definition fixes the direction.
 *   SELECTION  lam = trade_off, mu = 1.0f - lam (one f32 subtraction).  Pick 0 is pool position 0.  After pick t (position a_t)
 *              every unpicked j has m_j = sim(a_t, j) at t = 0 and m_j = max(m_j, sim(a_t, j)) after that, and pick t + 1 is the
 *              unpicked j that maximises v_j = (lam * s_j) - (mu * m_j): both products and the subtraction each rounded to f32, no
 *              fused multiply-add; ties to the lower pool position; -0.0 == +0.0 in the max and in the comparison.  It stops after
 *              min(k, n) picks; the similarities of the last pick are not needed and take no part in the error rule below.
 *   OUTPUT     row u of out_items / out_scores (optional), [num_users][k]: the picked items in pick order with their pool scores s
 *              (sbr_predict's bits), padded with (0xFFFFFFFF, -inf) from n on.
 * So trade_off == 1.0f gives sbr_recommend(k)'s row bit for bit, pool == k a permutation of it, and with trade_off == 0 the scores
 * only break ties.  metric: SBR_SIMILAR_COSINE or SBR_SIMILAR_DOT; flags: SBR_RECOMMEND_INCLUDE_HISTORY only; histories,
 * representations and exclusion lists as the plain calls take them.
 * A user's pool lives in one workgroup's LDS: pool <= sbr_recommend_diverse_max_pool = min(1024, 32768 / storage width), i.e. 1 024
 * up to embedding_dim 32, 512 up to 64, 256 up to 128, 128 up to 256.  There is no path for a larger pool.
 * SBR_ERR_INVALID_ARGUMENT: k < 1, pool < k, pool > sbr_recommend_diverse_max_pool, trade_off outside [0, 1] or NaN, an unknown
 * metric or flag, and wherever the plain call gives it.  SBR_ERR_INVALID_PREDICTION: wherever the pool's scan gives it, and when a
 * value the selection uses is non-finite — n2 of a pool item (COSINE), or sim of a picked item against a not yet picked pool item;
 * a non-finite row outside every pool, with finite scores, does not fail the call.  num_users == 0: nothing is done, SBR_OK.
 * Deterministic; reads parameters only; runs on every model sbr_recommend runs on.  The session form (declared with the session
 * store below) is refused while the store is stale, as sbr_sessions_recommend is. */
#define SBR_DIVERSE_MAX_POOL 1024u
sbr_status sbr_recommend_diverse_max_pool(const sbr_model* m, uint32_t* out);
sbr_status sbr_recommend_diverse(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users,
                                 uint32_t k, uint32_t pool, float trade_off, uint32_t metric, uint32_t flags,
                                 uint32_t* out_items, float* out_scores);
sbr_status sbr_recommend_diverse_reps(sbr_model* m, const float* reps, uint64_t num_users, uint32_t k, uint32_t pool,
                                      float trade_off, uint32_t metric, const uint64_t* excl_ptr, const uint32_t* excl_items,
                                      uint32_t* out_items, float* out_scores);

/* Exact top-k neighbours of catalogue items: "which items are like this one" (no counterpart in the reference crate: the whole
 * item table to the host, normalised and sorted there).  With E the item-embedding table — one table, shared by the input side and
 * the scoring side — and chain_dot(x, y) the k-ascending fused-multiply-add chain from +0.0 that sbr_predict uses:
 *     n2[i] = chain_dot(E[i], E[i])
 *     r[i]  = n2[i] > 0 ? 1.0f / sqrtf(n2[i]) : 0.0f                      (IEEE division and square root)
 *     SBR_SIMILAR_COSINE:  qhat = E[q] * r[q]  (elementwise, each product rounded to f32)
 *                          s(q, i) = chain_dot(qhat, E[i]) * r[i]
 *     SBR_SIMILAR_DOT:     s(q, i) = chain_dot(E[q], E[i])                (the same with r == 1.0f; x * 1.0f is exact)
 * The item bias takes no part.  A zero row has similarity 0 with everything.  Values are not clamped: a duplicate row can score
 * 1.0000006.  Row j of out_items / out_scores (optional), [num_queries][k], holds the k best items for query_items[j]: score
 * descending, ties to the lower item id (-0.0 == +0.0); a row with fewer than k eligible items is padded with item 0xFFFFFFFF and
 * score -inf.  1 <= k <= SBR_RECOMMEND_MAX_K.  The query item is excluded from its own row unless flags has
 * SBR_SIMILAR_INCLUDE_SELF; excl_ptr / excl_items: optional per-query exclusion lists (CSR, as sbr_recommend_reps': both NULL =
 * none; the library sorts and de-duplicates them).  Queries may repeat and come in any order; every query gets a row.
 * SBR_ERR_INVALID_PREDICTION if any n2[i] of the catalogue is non-finite (COSINE) or any score of a scanned pair is;
 * SBR_ERR_INVALID_ARGUMENT for a query or excluded id >= num_items, k out of range, an unknown metric or flag, or exclusion
 * arguments of which only one is NULL while a list is non-empty.  num_queries == 0: nothing is done, SBR_OK.  Deterministic; reads
 * parameters only; runs on every model sbr_recommend runs on. */
#define SBR_SIMILAR_COSINE 0u
#define SBR_SIMILAR_DOT 1u
#define SBR_SIMILAR_INCLUDE_SELF 1u
sbr_status sbr_similar_items(sbr_model* m, const uint32_t* query_items, uint64_t num_queries, uint32_t k,
                             uint32_t metric, uint32_t flags, const uint64_t* excl_ptr, const uint32_t* excl_items,
                             uint32_t* out_items, float* out_scores);

/* ITEM TAGS and per-user tag filters of the top-k scans: "only what this user may see" — territory, age rating, subscription tier,
 * in stock, not this category (no counterpart in the reference crate: a larger k and a filter on the host, which is not exact).
 * A model may hold item tags, tags[num_items], one 32-bit word per item, on its device; it has none until they are set.
 *   sbr_model_set_item_tags   copies tags[0 .. num_items) to the device; tags == NULL clears them (the model has none again)
 *   sbr_model_get_item_tags   out[0 .. num_items) = the words last set; SBR_ERR_INVALID_ARGUMENT while the model has none
 * Tags are serving metadata, not parameters: sbr_model_fit and the other fits, sbr_model_set_param and a load through it do not
 * touch them, setting them does not bump the parameter generation (a session store stays usable), and they are NOT PERSISTED — the
 * parameter blocks a save writes do not hold them, so whoever restores a model sets its tags again.  They are freed with the model
 * and live on the model's own device, so they work on a replica of a group and on a partitioned model wherever sbr_recommend runs.
 *
 * A *_filtered call is the plain call of the same name plus any_of[n] and none_of[n], one mask pair per user (query, slot) of the
 * call in the call's order; either may be NULL, which means all zeros.  Item i is ALLOWED for user u iff
 *     (tags[i] & none_of[u]) == 0 && (any_of[u] == 0 || (tags[i] & any_of[u]) != 0)
 * and the result is BIT FOR BIT that of the plain call with user u's exclusion list extended by every item that is not allowed for
 * u: items, score bits, order, padding with (0xFFFFFFFF, -inf), and the status.  So the non-finite rule is the plain call's — it
 * covers every scanned score, of an allowed item or not, as it covers excluded items; with all masks zero the result is the plain
 * call's; a user with no allowed item gets a row of padding.  For the diverse forms the pool is the filtered row at k = pool, as the
 * POOL clause above defines it; for sbr_similar_items_filtered the masks are per query ("similar items of the same category"), and
 * the query's own exclusion and SBR_SIMILAR_INCLUDE_SELF are the plain call's.  With histories the masks belong to the call's user
 * u, not to its history: two users with one history may carry different masks.
 * Nothing is materialised per user: the scan tests an item's tag word against the user's two mask words before the score is
 * offered to the user's list, 4 bytes read beside each item row.
 * SBR_ERR_INVALID_ARGUMENT: a filtered call on a model without tags (even with both masks NULL), and wherever the plain call gives
 * it.  NOT BUILT: a filter together with sbr_recommend_among's subset (the tags would have to be gathered with the sub-table; there
 * is no such entry point) and persistence of the tags.  sbr_rank_targets under a filter: sbr_rank_targets_rows, ELIGIBLE RANKS below. */
sbr_status sbr_model_set_item_tags(sbr_model* m, const uint32_t* tags);
sbr_status sbr_model_get_item_tags(sbr_model* m, uint32_t* out);
sbr_status sbr_recommend_filtered(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users,
                                  uint32_t k, uint32_t flags, const uint32_t* any_of, const uint32_t* none_of,
                                  uint32_t* out_items, float* out_scores);
sbr_status sbr_recommend_filtered_reps(sbr_model* m, const float* reps, uint64_t num_users, uint32_t k,
                                       const uint64_t* excl_ptr, const uint32_t* excl_items,
                                       const uint32_t* any_of, const uint32_t* none_of, uint32_t* out_items, float* out_scores);
sbr_status sbr_recommend_diverse_filtered(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users,
                                          uint32_t k, uint32_t pool, float trade_off, uint32_t metric, uint32_t flags,
                                          const uint32_t* any_of, const uint32_t* none_of, uint32_t* out_items, float* out_scores);
sbr_status sbr_recommend_diverse_filtered_reps(sbr_model* m, const float* reps, uint64_t num_users, uint32_t k, uint32_t pool,
                                               float trade_off, uint32_t metric, const uint64_t* excl_ptr, const uint32_t* excl_items,
                                               const uint32_t* any_of, const uint32_t* none_of, uint32_t* out_items, float* out_scores);
sbr_status sbr_similar_items_filtered(sbr_model* m, const uint32_t* query_items, uint64_t num_queries, uint32_t k,
                                      uint32_t metric, uint32_t flags, const uint64_t* excl_ptr, const uint32_t* excl_items,
                                      const uint32_t* any_of, const uint32_t* none_of, uint32_t* out_items, float* out_scores);

/* Recommend within an item subset, batched candidate scoring, batched representations (no counterparts in the reference crate:
 * loops over user_representation and predict, and a host-side filter).  Throughout, score(u, i) = bias[i] + chain_dot(rep_u, E[i])
 * has the bits of sbr_predict, and a history's representation is sbr_user_representation's (last max_sequence_length items; an
 * empty history = item 0).  All five calls are deterministic, read parameters only, run on every model sbr_recommend runs on and
 * refuse where it refuses.
 *
 * sbr_user_representations: out_reps [num_users][embedding_dim]; row u has the bits of sbr_user_representation of history
 * item_ids[user_ptr[u] .. user_ptr[u + 1]), and every user gets a row.  Ids are validated as sbr_recommend validates them.
 * num_users == 0: nothing is done, SBR_OK.
 *
 * sbr_score_candidates / _reps: the batched sbr_predict.  User u's candidates are cand_items[cand_ptr[u] .. cand_ptr[u + 1]): any
 * number, none included, in any order, duplicates allowed; out_scores[e - cand_ptr[0]] = score(u, cand_items[e]), in the caller's
 * order, nothing masked.  SBR_ERR_INVALID_PREDICTION if any computed score is non-finite (out_scores is then unspecified);
 * SBR_ERR_INVALID_ARGUMENT for decreasing pointers, ids >= num_items, cand_items NULL while a list is non-empty.  No pairs: nothing is
 * done, SBR_OK.  _reps: from representations (embedding_dim floats each).
 *
 * sbr_recommend_among / _reps: sbr_recommend / sbr_recommend_reps with every item outside S = subset_items[0 .. num_subset)
 * ineligible — the same order (score descending, ties to the lower item id, -0.0 == +0.0), padding (0xFFFFFFFF, -inf), range of k,
 * history / exclusion rules and flags; out_items holds catalogue ids, not positions in S.  S may be unsorted and hold duplicates
 * (the library sorts and de-duplicates it); num_subset == 0 gives rows of padding; with S the whole catalogue the result is bit-equal
 * to sbr_recommend's.  Only pairs (scanned user, item of S) are scored: a non-finite score outside S does not fail the call, one
 * inside S does (SBR_ERR_INVALID_PREDICTION).  SBR_ERR_INVALID_ARGUMENT for an id >= num_items in S, and wherever sbr_recommend /
 * sbr_recommend_reps give it.  Each launch copies S's rows and biases into scratch, |S| * (4 * storage width + 4) bytes;
 * SBR_ERR_OUT_OF_MEMORY if the device cannot hold that. */
sbr_status sbr_user_representations(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids,
                                    uint64_t num_users, float* out_reps);
sbr_status sbr_score_candidates(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users,
                                const uint64_t* cand_ptr, const uint32_t* cand_items, float* out_scores);
sbr_status sbr_score_candidates_reps(sbr_model* m, const float* reps, uint64_t num_users,
                                     const uint64_t* cand_ptr, const uint32_t* cand_items, float* out_scores);
sbr_status sbr_recommend_among(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users,
                               uint32_t k, uint32_t flags, const uint32_t* subset_items, uint64_t num_subset,
                               uint32_t* out_items, float* out_scores);
sbr_status sbr_recommend_among_reps(sbr_model* m, const float* reps, uint64_t num_users, uint32_t k,
                                    const uint64_t* excl_ptr, const uint32_t* excl_items,
                                    const uint32_t* subset_items, uint64_t num_subset,
                                    uint32_t* out_items, float* out_scores);

/* Exact ranks of many held-out items per user from ONE scan of the catalogue (no counterpart in the reference crate beyond the one
 * item of evaluation.rs:12-48, whose rule this applies to each target on its own).  With score(u, i) as above and the masked score
 * m(u, i) = f32::MIN if i is in the user's mask list, else score(u, i):
 *     rank(u, t) = #{ i in [0, num_items) : m(u, i) >= m(u, t) }
 * so the target counts itself (rank >= 1), ties count against it, other targets are ordinary items, a masked target has rank
 * num_items, and duplicate targets get equal ranks.  User u's targets are target_items[target_ptr[u] .. target_ptr[u + 1]) (any
 * number, none included); out_ranks[e - target_ptr[0]] is the rank of target_items[e].  Precision / recall / hit rate / NDCG at any k
 * and the mean rank follow from the ranks on the host.  SBR_ERR_INVALID_PREDICTION if any score of a scanned user is non-finite;
 * SBR_ERR_INVALID_ARGUMENT for decreasing pointers, ids >= num_items, unknown flags.  Deterministic (integer counts).
 * sbr_rank_targets: histories as sbr_recommend's (representation of the last max_sequence_length items, empty = item 0); the mask
 * is the WHOLE history unless flags has SBR_RANK_INCLUDE_HISTORY.  With one target per user (the last item) and the rest as history
 * the result is sbr_mrr_score's rank.
 * sbr_rank_targets_reps: from representations; excl_ptr / excl_items: optional per-user mask lists (CSR; both NULL = none). */
#define SBR_RANK_INCLUDE_HISTORY 1u
sbr_status sbr_rank_targets(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users,
                            const uint64_t* target_ptr, const uint32_t* target_items, uint32_t flags, uint32_t* out_ranks);
sbr_status sbr_rank_targets_reps(sbr_model* m, const float* reps, uint64_t num_users,
                                 const uint64_t* excl_ptr, const uint32_t* excl_items,
                                 const uint64_t* target_ptr, const uint32_t* target_items, uint32_t* out_ranks);

/* Exact next-item rank at EVERY position of a sequence from one forward pass per sequence: the teacher-forced evaluation of a
 * sequence recommender (no counterpart in the reference crate, whose mrr_score ranks the last item alone, evaluation.rs:12-48).
 *
 * WINDOW.  User u's items are x_0 .. x_{n-1} = item_ids[user_ptr[u] .. user_ptr[u + 1]).  With W = min(n, max_sequence_length + 1)
 * the window is the last W of them, w_0 .. w_{W-1}.  Items before the window are neither in any state nor in any mask: a sliding
 * window would need a forward pass per position, and callers split longer sequences themselves.
 * POSITIONS.  p = 1 .. W - 1: the history is w_0 .. w_{p-1} and the target w_p.  rep_p has the bits of
 * sbr_user_representation(w_0 .. w_{p-1}); a history of at most max_sequence_length items is never truncated.
 * RANK.  rank_p = #{ i in [0, num_items) : m(i) >= m(w_p) } with m(i) = f32::MIN if i is among the distinct items of
 * w_0 .. w_{p-1}, else b[i] + chain dot(rep_p, E[i]) with sbr_predict's bits; with SBR_RANK_INCLUDE_HISTORY in flags nothing is
 * masked.  So the target counts itself, ties count against it, a target that occurs in its own prefix has rank num_items, and a
 * prefix item that repeats is masked once.  rank_p equals sbr_rank_targets(history = w[0 .. p), targets = { w_p }), and for
 * n <= max_sequence_length + 1 the last entry of a row equals sbr_mrr_score's rank of that user.
 * OUTPUT.  CSR: out_ptr u64 [num_users + 1] from 0, out_ranks u32 [out_ptr[num_users]]; row u holds its positions ascending; a user
 * with n < 2 has an empty row.  last_positions (0 = all) keeps only the last min(last_positions, W - 1) positions of each window —
 * the scan costs one catalogue row per position, and this is the caller's cost control; the kept ranks are the numbers of the full
 * call.  out_ranks NULL: out_ptr alone is filled (sizing), with no device work.
 * ERRORS.  SBR_ERR_INVALID_PREDICTION if any score of a scanned row is non-finite; SBR_ERR_INVALID_ARGUMENT for decreasing
 * pointers, ids >= num_items, unknown flags, or while a fit plan is open on the model; the outputs are then untouched.
 * Both model families, every embedding_dim from 1 to 256.  Deterministic (integer counts). */
sbr_status sbr_sequence_ranks(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, uint32_t flags,
                              uint32_t last_positions, uint64_t* out_ptr, uint32_t* out_ranks);

/* SEQUENCE PARTITION — what the policy softmax(score / temperature) over the items a user may see (SAMPLING, PARTITION) needs to
 * price the item that actually came next at EVERY position of a sequence, from one forward pass per sequence.  WINDOW, POSITIONS,
 * `last_positions`, the CSR rows and their chunking are sbr_sequence_ranks'.  For every kept position p, with the prefix
 * w_0 .. w_{p-1} and the target w_p:
 *   out_shift, out_mass   bit for bit and integer for integer what sbr_log_partition returns for the explicit history w[0 .. p) at
 *                         this temperature: the largest fl(score * inv_t) over the eligible items (a zero is +0.0; -inf and mass 0
 *                         if nothing is eligible) and the sum of sbr_softmax_weight over them at sbr_softmax_frac_bits(num_items).
 *                         Eligible: every item not among the distinct items of the prefix, or with SBR_RANK_INCLUDE_HISTORY in
 *                         flags every item.
 *   out_scores            the target's plain score, sbr_predict's bits.
 *   out_masked            1 iff the prefix is masked and w_p occurs in it: the policy never shows that item, its log-probability
 *                         is -inf (the case in which sbr_sequence_ranks returns num_items); else 0.
 * log p(w_p) = log(w / mass) with w = sbr_softmax_weights(score, temperature, shift, frac_bits) is the caller's, on the host.
 * No result depends on the batch, the host's chunks or the scan's split.  All four outputs NULL: out_ptr alone is filled (sizing),
 * with no device work; otherwise all four are required, [out_ptr[num_users]] each.
 * ERRORS.  SBR_ERR_INVALID_ARGUMENT for a temperature that is not finite and > 0 (as sbr_log_partition), decreasing pointers,
 * ids >= num_items, unknown flags, some but not all outputs, or while a fit plan is open on the model; SBR_ERR_INVALID_PREDICTION
 * if any score of a scanned row is non-finite; the outputs are then untouched.  Both model families, every embedding_dim from 1
 * to 256.  Deterministic (integer sums). */
sbr_status sbr_sequence_partition(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, float temperature,
                                  uint32_t flags, uint32_t last_positions, uint64_t* out_ptr, float* out_shift, uint64_t* out_mass,
                                  float* out_scores, uint8_t* out_masked);

/* SESSIONS — device-resident user states advanced one event at a time (no counterpart in the reference crate, whose
 * user_representation walks the whole history on every call, sequence_model.rs:182-211).  A store belongs to one model and has
 * `capacity` slots; a slot holds len, the number of items appended since its last reset, and the recurrent state after those items:
 * h, c for the LSTM, s for EWMA (storage width; the columns past embedding_dim are zero, as in the model's own states).
 *
 * Appending item x to a slot is one step of the forward pass from the stored state: LSTM z = b + [E[x] ; h] W as a k-ascending fma
 * chain seeded with the bias, then the cell, from h = c = 0 when len == 0; EWMA s = E[x] for the first item
 * (ewma.rs:306) and s = fma(a, s, (1 - a) * E[x]), a = sigmoid(alpha), afterwards.  The representation of a slot is its h (s) when
 * len >= 1, and sbr_user_representation of the empty history — one step of item 0 from the zero state, lstm.rs:262-264 — when
 * len == 0; that step is not stored: the first real append still starts from zero.
 *
 * EXACT: a slot whose appended items are x_1 .. x_n, n <= max_sequence_length, however they were split across calls, has a
 * representation with the BITS of sbr_user_representation(x_1 .. x_n), at every embedding_dim and for all three model kinds.
 * BEYOND max_sequence_length a session does NOT truncate to the last max_sequence_length items as sbr_user_representation does
 * (state_window): it holds the recurrence over everything appended, i.e. the bits of user_representation of a model with the same
 * parameters and max_sequence_length >= n.  This is the one place sessions depart from the windowed call; a caller who wants the
 * window resets the slot and appends the window.
 *
 * STALENESS: the model has a parameter generation, bumped by whatever can write parameters — a fit plan opening by any route
 * (sbr_fit_begin, sbr_group_fit_begin, sbr_model_fit, sbr_model_fit_comm, sbr_group_fit) or closing, and sbr_model_set_param.  A store
 * remembers the generation of its creation, last sbr_sessions_reset_all or last whole-store sbr_sessions_replay (REPLAY below);
 * while the model's differs, every store call except those two, capacity and destroy returns SBR_ERR_INVALID_ARGUMENT: no call
 * mixes states of two parameter sets.  While a fit plan
 * is open on the model (from sbr_fit_begin to sbr_fit_plan_destroy; sbr_model_fit and the group fits open and destroy theirs
 * inside the call) its steps rewrite parameters, so every store call but capacity and destroy — sbr_sessions_reset_all included —
 * returns SBR_ERR_INVALID_ARGUMENT until the plan is destroyed.
 *
 * Every call validates before it launches anything, and an error leaves every slot as it was.  SBR_ERR_INVALID_ARGUMENT: a slot
 * >= capacity, the same slot twice in one call, decreasing pointers, an item id >= num_items, k outside sbr_recommend's range, flags
 * other than 0.  Slots need not be sorted or contiguous; a slot listed with no items is left alone; slots a call does not name keep
 * their bits.  A store works wherever sbr_user_representations works on its model, takes the model's mutex and runs on the model's
 * stream; it is destroyed before its model.
 *
 *   sbr_sessions_create          capacity slots, all empty (1 <= capacity < 2^31 - 1); SBR_ERR_OUT_OF_MEMORY if the device cannot hold them
 *   sbr_sessions_reset           the named slots: len = 0, zero state
 *   sbr_sessions_reset_all       every slot, and the store re-bound to the model's current parameters
 *   sbr_sessions_append          items item_ids[item_ptr[i] .. item_ptr[i + 1]) to slot slots[i], in order
 *   sbr_sessions_lengths         out_lengths[i] = len of slots[i]
 *   sbr_sessions_representations out_reps [n][embedding_dim], rows laid out as sbr_user_representations'
 *   sbr_sessions_get_state / _set_state   checkpoint / restore: h, c [n][embedding_dim] (c NULL for EWMA, required for the LSTM), len
 *                                [n]; a restored len of 0 is the empty slot (zero state, whatever h holds)
 *   sbr_sessions_recommend / _score_candidates   sbr_recommend_reps / sbr_score_candidates_reps on sbr_sessions_representations of
 *                                the same slots — results, padding, errors, non-finite handling, bit for bit — with the scan reading
 *                                the store's rows in place.  A store without seen-item memory keeps no item history: exclusions
 *                                are the caller's lists.
 * The other scans are reached through sbr_sessions_representations and the *_reps calls.
 *
 * SEEN-ITEM MEMORY: sbr_sessions_create_seen makes a store whose slots also remember the last seen_capacity items appended to them
 * since their last reset (1 <= seen_capacity <= SBR_SESSIONS_MAX_SEEN; capacity * seen_capacity * 4 more bytes on the device;
 * seen_capacity = 0 is sbr_sessions_create), in append order, repeats kept: a ring of u32 ids and a u64 count per slot, written on
 * the device by the call that appends (of more than seen_capacity items to one slot in one call, the last seen_capacity).
 * sbr_sessions_reset, _reset_all and _set_state empty the memory of the slots they touch (a restored state's items are unknown);
 * the empty-history row has none.  On such a store sbr_sessions_recommend, _recommend_filtered, _recommend_diverse and
 * _recommend_diverse_filtered exclude each slot's remembered items as sbr_recommend excludes the history — the result is, bit
 * for bit, the *_reps call on sbr_sessions_representations with user i's list = sbr_sessions_get_seen of slot i united with the
 * caller's list — and the two calls with `flags` accept SBR_RECOMMEND_INCLUDE_HISTORY, which ignores the memory for that call; on
 * a store without memory flags other than 0 stay SBR_ERR_INVALID_ARGUMENT.  sbr_sessions_score_candidates masks nothing.
 *   sbr_sessions_seen_capacity   *out = seen_capacity (0: no memory)
 *   sbr_sessions_get_seen        slot slots[i]'s remembered items, oldest first, at out_items[out_ptr[i] .. out_ptr[i + 1]);
 *                                out_ptr [n + 1] from 0, out_items holds n * seen_capacity ids
 *   sbr_sessions_set_seen        slot slots[i]'s memory = the last seen_capacity of items[ptr[i] .. ptr[i + 1]) (ids validated as
 *                                every CSR argument's); get_state + get_seen, then set_state + set_seen in that order, restore a
 *                                slot exactly
 * get_seen / set_seen on a store without memory: SBR_ERR_INVALID_ARGUMENT.
 *
 * REPLAY: sbr_sessions_replay recomputes slots' states from their seen-item memories under the model's CURRENT parameters, on the
 * device: a store survives a parameter change (a retrain, sbr_model_set_param, a load) with what it still knows of its sessions.
 * Let items_s be slot s's remembered items, oldest first — what sbr_sessions_get_seen returns, the min(cnt, seen_capacity) valid ring
 * entries.
 *   slots == NULL   every slot of the store (n ignored).  Allowed on a STALE store — besides sbr_sessions_reset_all it is the one
 *                   call such a store accepts — and afterwards the store is bound to the model's current parameters, its
 *                   empty-history row rebuilt as sbr_sessions_reset_all builds it.
 *   slots != NULL   the n named slots only, each < capacity; a slot named more than once counts once.  The store must be current,
 *                   as for every other call; every slot not named keeps every bit of its state, its length and its memory.
 * Every replayed slot then holds, bit for bit, the state a freshly reset slot holds after sbr_sessions_append of items_s: h (c),
 * and len = |items_s|.  A slot whose memory is empty becomes an empty slot (len 0, reading the empty-history row) even if
 * sbr_sessions_set_state had given it a state.  A slot whose memory has WRAPPED (more than seen_capacity items remembered since
 * its reset) gets the recurrence over its last seen_capacity items only and len = seen_capacity: what the store still knows,
 * not what it was told.  The memory itself — ring and count — is not written: sbr_sessions_get_seen returns the same lists before
 * and after.  *out_replayed (optional) = the number of slots, of those the call covers, that had a non-empty memory.
 * SBR_ERR_INVALID_ARGUMENT, with the store left as it was: a store without seen-item memory (there is nothing to replay from), a fit
 * plan open on the model, a slot >= capacity, slots != NULL on a stale store.  The rings never visit the host: it reads the slots'
 * counts (8 bytes per slot) to order them, the items are fed to the step kernels of sbr_sessions_append from the rings in chunks of
 * sessions sized to the model's scratch arena. */
#define SBR_SESSIONS_MAX_SEEN 1024u
typedef struct sbr_sessions sbr_sessions;
sbr_status sbr_sessions_create(sbr_model* m, uint64_t capacity, sbr_sessions** out);
sbr_status sbr_sessions_create_seen(sbr_model* m, uint64_t capacity, uint32_t seen_capacity, sbr_sessions** out);
sbr_status sbr_sessions_seen_capacity(const sbr_sessions* st, uint32_t* out);
sbr_status sbr_sessions_get_seen(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint64_t* out_ptr, uint32_t* out_items);
sbr_status sbr_sessions_set_seen(sbr_sessions* st, const uint32_t* slots, uint64_t n, const uint64_t* ptr, const uint32_t* items);
sbr_status sbr_sessions_replay(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint64_t* out_replayed);
void sbr_sessions_destroy(sbr_sessions* st);
sbr_status sbr_sessions_capacity(const sbr_sessions* st, uint64_t* out);
sbr_status sbr_sessions_reset(sbr_sessions* st, const uint32_t* slots, uint64_t n);
sbr_status sbr_sessions_reset_all(sbr_sessions* st);
sbr_status sbr_sessions_append(sbr_sessions* st, const uint32_t* slots, uint64_t n, const uint64_t* item_ptr, const uint32_t* item_ids);
sbr_status sbr_sessions_lengths(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint64_t* out_lengths);
sbr_status sbr_sessions_representations(sbr_sessions* st, const uint32_t* slots, uint64_t n, float* out_reps);
sbr_status sbr_sessions_get_state(sbr_sessions* st, const uint32_t* slots, uint64_t n, float* out_h, float* out_c, uint64_t* out_len);
sbr_status sbr_sessions_set_state(sbr_sessions* st, const uint32_t* slots, uint64_t n, const float* h, const float* c, const uint64_t* len);
sbr_status sbr_sessions_recommend(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint32_t k, const uint64_t* excl_ptr,
                                  const uint32_t* excl_items, uint32_t flags, uint32_t* out_items, float* out_scores);
sbr_status sbr_sessions_score_candidates(sbr_sessions* st, const uint32_t* slots, uint64_t n, const uint64_t* cand_ptr,
                                         const uint32_t* cand_items, float* out_scores);
/* sbr_recommend_diverse_reps on sbr_sessions_representations of the same slots, the scan reading the store's rows in place */
sbr_status sbr_sessions_recommend_diverse(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint32_t k, uint32_t pool,
                                          float trade_off, uint32_t metric, const uint64_t* excl_ptr, const uint32_t* excl_items,
                                          uint32_t* out_items, float* out_scores);
/* sbr_recommend_filtered_reps / sbr_recommend_diverse_filtered_reps on sbr_sessions_representations of the same slots: any_of /
 * none_of [n], slot slots[i]'s pair at i (ITEM TAGS above); setting the model's tags does not make a store stale */
sbr_status sbr_sessions_recommend_filtered(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint32_t k, const uint64_t* excl_ptr,
                                           const uint32_t* excl_items, uint32_t flags, const uint32_t* any_of, const uint32_t* none_of,
                                           uint32_t* out_items, float* out_scores);
sbr_status sbr_sessions_recommend_diverse_filtered(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint32_t k, uint32_t pool,
                                                   float trade_off, uint32_t metric, const uint64_t* excl_ptr, const uint32_t* excl_items,
                                                   const uint32_t* any_of, const uint32_t* none_of, uint32_t* out_items, float* out_scores);

/* SAMPLING — k draws without replacement from softmax(score / T) over the items a user may see: exploration, slates that differ
 * between visits, randomised logging that (seed, stream) gives back (no counterpart in the reference crate: predict over the
 * catalogue and a host loop).  By the Gumbel-top-k identity the draw is the plain scan over
 *     key(u, i) = fl(fl(score(u, i) * inv_t) + g(seed, streams[u], i)),   inv_t = 1.0f / temperature (one f32 division),
 * the product and the sum rounded separately, g standard Gumbel noise: the k items with the largest keys, in key order, are k
 * sequential draws without replacement.  Row u of out_items / out_scores / out_keys [n][k] (the last two optional):
 *   ORDER        keys descending, ties to the lower item id, short rows padded with (0xFFFFFFFF, -inf, -inf).
 *   ELIGIBILITY  the plain call's: history (flags: SBR_RECOMMEND_INCLUDE_HISTORY only), exclusion lists, a session's seen-item
 *                memory, and the tag masks any_of / none_of of ITEM TAGS — both NULL: no filter and no tags needed; either one
 *                non-NULL: the *_filtered call's rules.  An ineligible item draws no slot and changes no other item's noise.
 *   out_scores   the plain scores of the drawn items, sbr_predict's bits, in the row's (key) order — not sorted; padding -inf.
 *   NOISE        of (row, item) depends on (seed, streams[row], item) and on nothing else: not on k, the batch, the row's place in
 *                it, or how the call is cut up.  The same (seed, stream) with the same arguments returns the same row bit for bit;
 *                vary seed per request for a fresh draw.  streams: one u64 per row, NULL = the row's index in the call
 *                (sbr_sessions_recommend_sampled: the slot id).  With sbr_mix64 the 64-bit finaliser of the engine's counters,
 *                    K  = mix64(seed ^ mix64(stream * 0x9E3779B97F4A7C15 + 1));  k0 = low 32 bits, k1 = high 32 bits
 *                    x  = item ^ k0
 *                    x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16
 *                    x += k1
 *                    x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16
 *                    r  = x >> 9;  u = float(2 r + 1) * 2^-24;  g = -log32(-log32(u))
 *                log32 being the f32 logarithm of DESIGN.md section 6 (+, -, *, / and integer operations, each rounded once, no
 *                fused multiply-add): |g - exact| <= 5.7e-7 over all 2^23 values of r, g in [-2.8115408, 16.635532].
 * SBR_ERR_INVALID_ARGUMENT: sample NULL, a temperature that is not finite and > 0 or whose inv_t is not finite and non-zero, k
 * outside 1 .. SBR_RECOMMEND_MAX_K, masks on a model without tags, and wherever the plain call gives it.
 * SBR_ERR_INVALID_PREDICTION: a non-finite score of a scanned pair, as in the plain call, or a non-finite fl(score * inv_t) (then the
 * key is not finite; a finite product cannot give a non-finite key).  Deterministic; reads parameters only. */
typedef struct sbr_sample_args {
    float temperature;
    uint64_t seed;
    const uint64_t* streams; /* [n] or NULL */
} sbr_sample_args;
sbr_status sbr_recommend_sampled(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, uint32_t k,
                                 uint32_t flags, const struct sbr_sample_args* sample, const uint32_t* any_of, const uint32_t* none_of,
                                 uint32_t* out_items, float* out_scores, float* out_keys);
sbr_status sbr_recommend_sampled_reps(sbr_model* m, const float* reps, uint64_t num_users, uint32_t k, const uint64_t* excl_ptr,
                                      const uint32_t* excl_items, const struct sbr_sample_args* sample, const uint32_t* any_of,
                                      const uint32_t* none_of, uint32_t* out_items, float* out_scores, float* out_keys);
sbr_status sbr_sessions_recommend_sampled(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint32_t k, const uint64_t* excl_ptr,
                                          const uint32_t* excl_items, uint32_t flags, const struct sbr_sample_args* sample,
                                          const uint32_t* any_of, const uint32_t* none_of, uint32_t* out_items, float* out_scores,
                                          float* out_keys);

/* PARTITION — the exact mass of softmax(score / T) over the items a row may see, and with it the propensity of every draw the
 * *_sampled calls make: what off-policy evaluation, inverse-propensity weighting and counterfactual training need beside a logged
 * draw (no counterpart in the reference crate).  The sum is taken in FIXED POINT: integer addition is associative, so the result does
 * not depend on the batch, the host's chunks, the item ranges or the lanes' order, and a numpy restatement holds every bit
 * (tests/partition_expect.py).  One row's result is a function of its representation, the temperature, its exclusions and masks:
 *   s_i      b[i] + chain_dot(h, E[i]), sbr_predict's bits
 *   t_i      fl(s_i * inv_t), inv_t = 1.0f / temperature (one f32 division), as the *_sampled calls scale
 *   allowed  exactly the items the plain call would choose from: history (flags: SBR_RECOMMEND_INCLUDE_HISTORY only), exclusion
 *            lists, a session's seen-item memory, and the tag masks — both NULL: no filter and no tags needed
 *   shift    out_shift[u] = the largest t_i over the allowed items = fl(s_max * inv_t); -inf when nothing is allowed; a zero is +0.0
 *   d_i      fl(t_i - shift)
 *   w_i      0 where d_i > 0 or d_i < -64, else fix_F(exp32(d_i)) — exp32 the f32 exponential of DESIGN.md section 6 (integer
 *            operations and f32 +, -, * only, each rounded once; max relative error 2.54e-7 on [-64, 0], exp32(0) == 1 exactly),
 *            fix_F(x) = floor(x 2^F) by shifting x's 24-bit significand
 *   F        *out_frac_bits = sbr_softmax_frac_bits(num_items) = min(40, 63 - bit_length(num_items)): the sum cannot overflow
 *   mass     out_mass[u] = the sum of w_i over the allowed items; >= 2^F whenever something is allowed (the arg-max weighs exactly
 *            2^F), else 0
 * and on the host, in float64, log_z = shift + log(mass / 2^F) (-inf for an empty row).  The model's probability of item i is
 * w_i / mass, the softmax at resolution 2^-F: |mass / 2^F - sum exp(d_i)| <= num_items 2^-F + 2.54e-7 sum exp(d_i).
 * sbr_softmax_weights is the one host statement of the t / d / exp32 / fix_F chain: out_w[j] = w of scores[j] against `shift` —
 * log(out_w[j] / mass) is the log-probability of a draw with plain score scores[j]; a slate drawn without replacement has the
 * Plackett-Luce conditional probabilities w_j / (mass - the w of the draws before it), the remaining mass an exact integer;
 * sbr_softmax_weights_rows is the same over many rows, each against its own shift, in one call.  The helpers need no device and no
 * model.
 * SBR_ERR_INVALID_ARGUMENT: a temperature that is not finite and > 0 or whose inv_t is not finite and non-zero, a NULL output,
 * frac_bits > 40, masks on a model without tags, and wherever the plain call gives it.  SBR_ERR_INVALID_PREDICTION: a non-finite
 * s or t of a scanned pair, as in sbr_recommend / sbr_recommend_sampled; then no output is written.  Deterministic; reads
 * parameters only.  Not built: a single-pass form without the k = 1 scan, among= subsets, and partitions for similar_items,
 * audience and recommend_diverse. */
uint32_t sbr_softmax_frac_bits(uint32_t num_items);
sbr_status sbr_softmax_weights(const float* scores, uint64_t n, float temperature, float shift, uint32_t frac_bits, uint64_t* out_w);
/* sbr_softmax_weights of `rows` rows of m scores each, row r against shifts[r]: scores / out_w [rows][m] */
sbr_status sbr_softmax_weights_rows(const float* scores, uint64_t rows, uint64_t m, float temperature, const float* shifts,
                                    uint32_t frac_bits, uint64_t* out_w);
sbr_status sbr_log_partition(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, uint32_t flags,
                             float temperature, const uint32_t* any_of, const uint32_t* none_of, float* out_shift, uint64_t* out_mass,
                             uint32_t* out_frac_bits);
sbr_status sbr_log_partition_reps(sbr_model* m, const float* reps, uint64_t num_users, const uint64_t* excl_ptr, const uint32_t* excl_items,
                                  float temperature, const uint32_t* any_of, const uint32_t* none_of, float* out_shift, uint64_t* out_mass,
                                  uint32_t* out_frac_bits);
sbr_status sbr_sessions_log_partition(sbr_sessions* st, const uint32_t* slots, uint64_t n, const uint64_t* excl_ptr,
                                      const uint32_t* excl_items, uint32_t flags, float temperature, const uint32_t* any_of,
                                      const uint32_t* none_of, float* out_shift, uint64_t* out_mass, uint32_t* out_frac_bits);

/* ROLLOUT — a session's next `steps` items, each chosen given the ones before it, picked and fed back on the device: queue
 * continuation, an "up next" rail, trajectories under the softmax policy (no counterpart in the reference crate: a host loop of
 * recommend(k = 1) + append + a rebuilt exclusion list per step).  A rollout is HYPOTHETICAL: it reads the store and writes none of
 * it — not a state, not a length, not the seen-item memory.  Stated against the calls above, for row i and step j = 0 .. steps - 1:
 *   ELIGIBILITY  X_0 = what sbr_sessions_recommend[_filtered](k = 1) may choose from at call time: excl_ptr / excl_items, the slot's
 *                seen-item memory (unless SBR_ROLLOUT_INCLUDE_SEEN; only a store with memory takes that flag), the masks any_of /
 *                none_of (both NULL: no filter).  X_j = X_0 without picks 0 .. j - 1; with SBR_ROLLOUT_ALLOW_REPEATS X_j = X_0.
 *   GREEDY       pick j = the first item of X_j in every call's order (score descending, ties to the lower id, -0.0 == +0.0), the
 *                scores taken against the state after picks 0 .. j - 1; out_scores has sbr_predict's bits.  Step 0 of an empty slot
 *                reads the empty-history row, as sbr_sessions_recommend does.
 *   SAMPLE       (SBR_ROLLOUT_SAMPLE) pick j = the one draw of sbr_sessions_recommend_sampled(k = 1) over X_j with sample's
 *                temperature and streams (NULL: the slot ids) and seed (sample->seed + j) mod 2^64 — the noise is a function of
 *                (seed, stream, item) alone, so one seed for all steps would give an item the same noise at every step.  out_keys
 *                (optional; must be NULL without the flag) receives the winning keys.  steps = 1 IS that call.
 *   STATE        after pick j the row's state is what sbr_sessions_append(slot, [pick]) would make of it: one cell step of the forward
 *                pass's arithmetic, the whole recurrence, no window; an empty slot starts from zero.  out_h / out_c (optional;
 *                [n][embedding_dim]; out_c with out_h and the LSTM only) receive the states after all steps, the bits of
 *                sbr_sessions_get_state after appending row i's out_lengths[i] picks — whose len is the slot's length + out_lengths[i].
 *   END          a row with X_j empty ends: entry j and every later one is (0xFFFFFFFF, -inf), -inf in out_keys, and
 *                out_lengths[i] = j (optional; steps for a row that never ends); its state stops changing.
 *   PARTITION    out_shift non-NULL (then out_mass and out_frac_bits too) asks for it, in either mode: out_shift / out_mass [n][steps]
 *                = sbr_sessions_log_partition's shift and mass for step j's state over X_j at sample->temperature, bit for bit;
 *                (-inf, 0) at padding.  The log-probability of pick j is log(sbr_softmax_weights(out_scores) / mass), on the host.
 * out_items / out_scores [n][steps] (scores optional).  1 <= steps <= SBR_ROLLOUT_MAX_STEPS.  The same arguments return the same rows
 * whatever the batch, the host's chunks or the scan's item ranges.  All steps of a chunk are queued without a host synchronisation;
 * the insert of a pick into its row's exclusion segment costs O(segment) per row and step.
 * SBR_ERR_INVALID_ARGUMENT, with nothing launched: args NULL, steps out of range, unknown flags, a temperature sbr_sample_args
 * refuses (checked in both modes), SBR_ROLLOUT_INCLUDE_SEEN on a store without memory, masks on a model without tags, a stale store,
 * an open fit plan, a slot out of range or named twice.  SBR_ERR_INVALID_PREDICTION: a non-finite score at any step fails the whole
 * call, as in sbr_recommend: what the outputs then hold is unspecified, and no binding returns it.  Within an item set:
 * sbr_item_set_rollout (ITEM SETS below).  Not built: k > 1 per step (see BEAM SEARCH below), a rollout that commits, caps or
 * thresholds inside a rollout, a per-step temperature, rollouts from *_reps rows. */
#define SBR_ROLLOUT_MAX_STEPS 1024u
#define SBR_ROLLOUT_SAMPLE 1u
#define SBR_ROLLOUT_ALLOW_REPEATS 2u
#define SBR_ROLLOUT_INCLUDE_SEEN 4u
typedef struct sbr_rollout_args {
    uint32_t steps;
    uint32_t flags;
    struct sbr_sample_args sample;
} sbr_rollout_args;
sbr_status sbr_sessions_rollout(sbr_sessions* st, const uint32_t* slots, uint64_t n, const struct sbr_rollout_args* args,
                                const uint64_t* excl_ptr, const uint32_t* excl_items, const uint32_t* any_of, const uint32_t* none_of,
                                uint32_t* out_items, float* out_scores, float* out_keys, uint32_t* out_lengths, float* out_shift,
                                uint64_t* out_mass, uint32_t* out_frac_bits, float* out_h, float* out_c);

/* BEAM SEARCH — the `width` most likely next-`steps` continuations of each session, searched on the device: "up next" rails,
 * playlist continuation, next-basket candidates (no counterpart in the reference crate: a host loop of temporary slots, set_state,
 * append, recommend(k = W) and log_partition per step).  Greedy and deterministic; HYPOTHETICAL like ROLLOUT: it writes nothing of
 * the store.  For row i (slot slots[i]), W = width (1 .. SBR_BEAM_MAX_WIDTH) and steps (1 .. SBR_ROLLOUT_MAX_STEPS):
 *   ELIGIBILITY  X_0 is ROLLOUT's (excl_ptr / excl_items, the seen-item memory unless SBR_ROLLOUT_INCLUDE_SEEN, the masks any_of /
 *                none_of).  A beam whose path so far is p_0 .. p_{j-1} may choose from X_j = X_0 without them, or X_0 under
 *                SBR_ROLLOUT_ALLOW_REPEATS.
 *   STATE        a beam's state is what sbr_sessions_append(slot, path) would make: the whole recurrence, no window.  Step 0 of an
 *                empty slot reads the empty-history row.
 *   STEP LOG-PROBABILITY  an f32 quantity of correctly rounded operations only, (shift, mass) = sbr_sessions_log_partition's for the
 *                beam's state over X_j at `temperature`, F its frac_bits:
 *                  inv_t = fl(1 / T); t = fl(score * inv_t); d = fl(t - shift)                        (d <= 0)
 *                  s = max(0, bit_length(mass) - 24); x = f32(mass >> s) 2^(s - F)                    (exact; x >= 1)
 *                  L = sbr_log32(x) (one per beam and step); lp = fl(d - L); cum_j = fl(cum_{j-1} + lp_j), cum_{-1} = 0
 *                lp is finite wherever the scores are and approximates log(w / mass) to about 1e-7 relative where w is not tiny.
 *                It is NOT Partition.log_prob, which is -inf where w == 0: for the exact f64 value ask for out_shift / out_mass
 *                and use sbr_softmax_weights on the host.
 *   SELECTION    at step j every live beam offers its first W items of X_j in every call's order (score descending, ties to the
 *                lower id, -0.0 == +0.0); the row keeps the W best of all offers by (cum descending, the parent's beam rank
 *                ascending, the offer's position in its parent's row ascending).  Step 0 has one parent, the slot.  A k = W scan per
 *                beam is exact: lp does not increase along a beam's score order, so every offer above a kept offer of the same
 *                parent is kept too.
 *   END          without repeats |X_j| = |X_0| - j for every beam of a row, so a row's beams end together: out_lengths[i] (optional)
 *                = the real steps (steps for a row that never ends); out_beams[i] (optional) = the live beams, fewer than W while the
 *                distinct paths are fewer.
 * Outputs, beams in selection order at the row's last real step: out_items u32 / out_scores f32 (optional; sbr_predict's bits of
 * each pick against its beam's state at that step) / out_step_lp f32 (optional) [n][W][steps], out_cum f32 [n][W] (optional);
 * out_shift f32 / out_mass u64 [n][W][steps] and out_frac_bits (optional, all three or none): the step's partition of the beam.
 * Padding (0xFFFFFFFF, -inf), -inf in out_step_lp / out_cum / out_shift, 0 in out_mass.  With W = 1 the items and scores are greedy
 * sbr_sessions_rollout's.  The same arguments return the same bits whatever the batch, the host's chunks or the scan's item ranges.
 * All steps of a chunk are queued without a host synchronisation.
 * SBR_ERR_INVALID_ARGUMENT, with nothing launched: args NULL, width or steps out of range, unknown flags (SBR_ROLLOUT_SAMPLE among
 * them), a temperature sbr_sample_args refuses, SBR_ROLLOUT_INCLUDE_SEEN on a store without memory, masks on a model without tags, a
 * stale store, an open fit plan, a slot out of range or named twice.  SBR_ERR_INVALID_PREDICTION: a non-finite score at any step
 * fails the whole call.  Within an item set: sbr_item_set_beam_search (ITEM SETS below).  Not built: stochastic beam search, caps,
 * beams that commit to the store. */
#define SBR_BEAM_MAX_WIDTH 32u
typedef struct sbr_beam_args {
    uint32_t steps;
    uint32_t width;
    uint32_t flags; /* SBR_ROLLOUT_ALLOW_REPEATS | SBR_ROLLOUT_INCLUDE_SEEN */
    float temperature;
} sbr_beam_args;
sbr_status sbr_sessions_beam_search(sbr_sessions* st, const uint32_t* slots, uint64_t n, const struct sbr_beam_args* args,
                                    const uint64_t* excl_ptr, const uint32_t* excl_items, const uint32_t* any_of, const uint32_t* none_of,
                                    uint32_t* out_items, float* out_scores, float* out_step_lp, float* out_cum, uint32_t* out_lengths,
                                    uint32_t* out_beams, float* out_shift, uint64_t* out_mass, uint32_t* out_frac_bits);

/* AUDIENCE— the reverse question, "which rows for this item": for each of num_queries query items q = items[j] (any order, repeats
 * allowed, each < num_items) the k candidate rows that score it highest, score(q, s) = b[q] + chain_dot(h_s, E[q]) with the bits of
 * sbr_predict / sbr_score_candidates for that (state, item) pair: the catalogue scan with the operands' roles exchanged (every
 * product of the chain commutes), the query's bias added in the epilogue.  Row j of out_rows / out_scores [num_queries][k]: score
 * descending, ties to the lower row id, short rows padded with (0xFFFFFFFF, -inf); out_scores may be NULL.  sbr_recommend's rules:
 * 1 <= k <= SBR_RECOMMEND_MAX_K, -0.0 == +0.0, a non-finite score of a scanned (query, candidate) pair is
 * SBR_ERR_INVALID_PREDICTION for the call — a non-finite row outside the candidates does not fail it.  num_queries == 0 is a no-op.
 *   sbr_audience_reps      candidates = the caller's rows reps [num_rows][embedding_dim]; results are row indices.  excl_ptr /
 *                          excl_rows: per QUERY a list of row indices (each < num_rows, any order) left out of its row; both NULL: none
 *   sbr_audience           candidates = sbr_user_representations of the histories; results are user indices.  Unless flags has
 *                          SBR_RECOMMEND_INCLUDE_HISTORY a user whose (whole) history holds the query item is left out of its row
 *   sbr_sessions_audience  candidates = the store's slots `slots` [num_slots] (each < capacity, none twice, any order; an empty slot
 *                          reads the empty-history row), or with slots == NULL (and num_slots == 0) every slot of length > 0;
 *                          results are slot ids.  excl_ptr / excl_slots: per query a list of slot ids (each < capacity; one that
 *                          is no candidate is ignored).  On a store with seen-item memory a candidate whose memory holds the query
 *                          item is left out as well — the lists are inverted on the device, the ring never visits the host — unless
 *                          flags has SBR_RECOMMEND_INCLUDE_HISTORY; on a store without memory flags other than 0 are
 *                          SBR_ERR_INVALID_ARGUMENT.  A stale store refuses the call as it refuses every other.
 * Not offered: tag filters per slot, k above SBR_RECOMMEND_MAX_K, a threshold form, item subsets. */
sbr_status sbr_audience_reps(sbr_model* m, const float* reps, uint64_t num_rows, const uint32_t* items, uint64_t num_queries, uint32_t k,
                             const uint64_t* excl_ptr, const uint32_t* excl_rows, uint32_t* out_rows, float* out_scores);
sbr_status sbr_audience(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, const uint32_t* items,
                        uint64_t num_queries, uint32_t k, uint32_t flags, uint32_t* out_users, float* out_scores);
sbr_status sbr_sessions_audience(sbr_sessions* st, const uint32_t* items, uint64_t num_queries, uint32_t k, const uint32_t* slots,
                                 uint64_t num_slots, const uint64_t* excl_ptr, const uint32_t* excl_slots, uint32_t flags, uint32_t* out_slots,
                                 float* out_scores);

/* ABOVE — the threshold form of the scans: for each row r and a per-row f32 threshold t = thresholds[r], EVERY scanned column whose
 * score satisfies score >= t — a set, not a list of k, so neither SBR_RECOMMEND_MAX_K nor any other k applies.  A row is a user,
 * a representation or a slot and a column an item (sbr_recommend_above*), or a row is a query item and a column a candidate row, user
 * or slot (sbr_audience_above*).  Each call takes the arguments of its top-k sibling with k replaced by thresholds [rows]:
 *   columns   exactly those the sibling would choose from: not in the row's exclusion list (any order, repeats allowed), allowed by
 *             the row's tag masks (the recommend forms; any_of / none_of both NULL: no filter and no tags needed), and on a store
 *             with memory not in the seen ring unless flags has SBR_RECOMMEND_INCLUDE_HISTORY
 *   scores    the bits of sbr_predict / sbr_score_candidates for the pair
 *   compare   the f32 compare, the rank rule of sbr_mrr_score and sbr_rank_targets: -0.0 and +0.0 are equal, ties at the threshold
 *             are all included; t = -inf returns every allowed column, t = +inf none
 * The result is CSR.  out_counts [rows] (required) receives each row's number of pairs and *out_total (required) their sum.  Row
 * r's pairs are entries [sum of out_counts before r, + out_counts[r]) of out_ids / out_scores, in ASCENDING id order (the set's
 * natural order, which the kernel produces by construction; include/sbr.hpp and the Python layer sort a row by score on the host).
 * out_ids and out_scores both NULL: counts only — one scan, the cheap way to choose a threshold or size a buffer; with empty
 * masks and no exclusions out_counts[r] is sbr_rank_targets' rank of an item that scores exactly t.  out_scores alone may be NULL.
 * Pairs are written only if *out_total <= capacity (entries of out_ids / out_scores).  Otherwise the call still returns SBR_OK with
 * the counts and the total — that is how a caller sizes a second call — and writes no pair; for a call of at most 8 192 rows the two
 * arrays are then untouched (a longer call runs in chunks of 8 192 rows and may have written the chunks that still fitted).
 * rows == 0, or nothing to scan, is SBR_OK with zero counts.
 * SBR_ERR_INVALID_ARGUMENT, before any launch: a NaN threshold, a NULL out_counts / out_total / thresholds, out_scores without
 * out_ids, and wherever the sibling gives it.  SBR_ERR_INVALID_PREDICTION: a non-finite score of any scanned pair of an existing
 * row, as in sbr_recommend.  Deterministic; reads parameters only.
 * Not offered: a device-side sort by score, among= subsets, thresholds on sbr_similar_items or on sampled keys, a tag filter in the
 * audience orientation. */
sbr_status sbr_recommend_above(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, const float* thresholds,
                               uint32_t flags, const uint32_t* any_of, const uint32_t* none_of, uint64_t* out_counts, uint64_t* out_total,
                               uint64_t capacity, uint32_t* out_ids, float* out_scores);
sbr_status sbr_recommend_above_reps(sbr_model* m, const float* reps, uint64_t num_users, const float* thresholds, const uint64_t* excl_ptr,
                                    const uint32_t* excl_items, const uint32_t* any_of, const uint32_t* none_of, uint64_t* out_counts,
                                    uint64_t* out_total, uint64_t capacity, uint32_t* out_ids, float* out_scores);
sbr_status sbr_sessions_recommend_above(sbr_sessions* st, const uint32_t* slots, uint64_t n, const float* thresholds, const uint64_t* excl_ptr,
                                        const uint32_t* excl_items, uint32_t flags, const uint32_t* any_of, const uint32_t* none_of,
                                        uint64_t* out_counts, uint64_t* out_total, uint64_t capacity, uint32_t* out_ids, float* out_scores);
sbr_status sbr_audience_above_reps(sbr_model* m, const float* reps, uint64_t num_rows, const uint32_t* items, uint64_t num_queries,
                                   const float* thresholds, const uint64_t* excl_ptr, const uint32_t* excl_rows, uint64_t* out_counts,
                                   uint64_t* out_total, uint64_t capacity, uint32_t* out_ids, float* out_scores);
sbr_status sbr_audience_above(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, const uint32_t* items,
                              uint64_t num_queries, const float* thresholds, uint32_t flags, uint64_t* out_counts, uint64_t* out_total,
                              uint64_t capacity, uint32_t* out_ids, float* out_scores);
sbr_status sbr_sessions_audience_above(sbr_sessions* st, const uint32_t* items, uint64_t num_queries, const float* thresholds,
                                       const uint32_t* slots, uint64_t num_slots, const uint64_t* excl_ptr, const uint32_t* excl_slots,
                                       uint32_t flags, uint64_t* out_counts, uint64_t* out_total, uint64_t capacity, uint32_t* out_ids,
                                       float* out_scores);

/* TOP — the budget form of the scans: for each row r and a per-row budget n = n[r] (any value >= 0; SBR_RECOMMEND_MAX_K does not
 * apply), the exact best n of the row.  Rows, columns and scores are ABOVE's: the eligible columns of row r are those
 * sbr_*_above(thresholds[r] = -inf) returns, m_r of them.  The total order is every other call's: score descending, ties to the
 * lower id, -0.0 == +0.0.  top(r, n) is the first min(n, m_r) eligible columns in that order, and the row's cut c_r (out_cuts [rows],
 * required) is
 *   the score of the last column returned   when m_r >= n >= 1 (a zero cut is written as +0.0, whichever zero that column holds);
 *   -inf                                    when m_r < n: everything eligible, sbr_*_above(-inf)'s row;
 *   +inf                                    when n == 0: an empty row.
 * So for n <= SBR_RECOMMEND_MAX_K the row is the top-k sibling's row at k = n without its padding; for any n it is the first n
 * entries, by (score descending, id ascending), of sbr_*_above(thresholds[r] = c_r)'s row; that call's count is >= n and the number
 * of eligible scores > c_r is < n; of a tie group that straddles the cut exactly the lowest ids are kept.
 * The result is CSR as ABOVE's: out_counts [rows] (required) = min(n[r], m_r), *out_total their sum, row r's pairs in ASCENDING id
 * order (the hosts layers sort a row by score).  out_ids and out_scores both NULL: the select only — cuts and counts, no pair; the
 * cheap form.  Pairs are written only if *out_total <= capacity; otherwise SBR_OK with counts, cuts and the total, and no pair (a
 * call of more than 8 192 rows may have written the chunks that still fitted).  The capacity is held against the pairs returned;
 * on the device a row's fill first holds every score tied at its cut, which under mass ties is more than n (in ranges of 256 MB of
 * entries, one row at least).  That intermediate, G = sum over rows of #{eligible score >= c_r}, is not refused at any size: the
 * device memory it takes is bounded by the ranges, the time is not.  A call with pairs runs 1 + ceil(8 G / 256 MB) + (rows that
 * alone exceed a range) catalogue scans behind the select's 8, so where ties are few (G close to *out_total) that is the ABOVE
 * call's cost, and in the worst case — every score of every row equal — G = rows x columns whatever n is: 8 192 rows x 1e6 columns
 * at n = 1 write 8.2e9 pairs in about 245 rescans to return 8 192.  A caller that cannot rule out mass ties asks for the cuts alone
 * first (NULL pair outputs) and sizes G with the ABOVE call's count form at those cuts.
 * Cost: 8 catalogue scans per chunk of 8 192 rows for the cuts (a radix select on the scores' bits, 4 bits a scan, no host round
 * trip between them), then with pairs ABOVE's count and fill at the cuts and a trim.
 * SBR_ERR_INVALID_ARGUMENT, before any launch: a NULL n / out_cuts / out_counts / out_total, out_scores without out_ids, and
 * wherever the sibling gives it.  SBR_ERR_INVALID_PREDICTION: a non-finite score of any scanned pair of an existing row — also of
 * a row with n == 0.  Deterministic (integer counts only); reads parameters only.
 * Not offered: a device-side sort by score, a fill that stops inside a tie group, among= subsets, a tag filter in the audience
 * orientation. */
sbr_status sbr_recommend_top(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, const uint64_t* n,
                             uint32_t flags, const uint32_t* any_of, const uint32_t* none_of, float* out_cuts, uint64_t* out_counts,
                             uint64_t* out_total, uint64_t capacity, uint32_t* out_ids, float* out_scores);
sbr_status sbr_recommend_top_reps(sbr_model* m, const float* reps, uint64_t num_users, const uint64_t* n, const uint64_t* excl_ptr,
                                  const uint32_t* excl_items, const uint32_t* any_of, const uint32_t* none_of, float* out_cuts,
                                  uint64_t* out_counts, uint64_t* out_total, uint64_t capacity, uint32_t* out_ids, float* out_scores);
sbr_status sbr_sessions_recommend_top(sbr_sessions* st, const uint32_t* slots, uint64_t n, const uint64_t* top_n, const uint64_t* excl_ptr,
                                      const uint32_t* excl_items, uint32_t flags, const uint32_t* any_of, const uint32_t* none_of,
                                      float* out_cuts, uint64_t* out_counts, uint64_t* out_total, uint64_t capacity, uint32_t* out_ids,
                                      float* out_scores);
sbr_status sbr_audience_top_reps(sbr_model* m, const float* reps, uint64_t num_rows, const uint32_t* items, uint64_t num_queries,
                                 const uint64_t* n, const uint64_t* excl_ptr, const uint32_t* excl_rows, float* out_cuts, uint64_t* out_counts,
                                 uint64_t* out_total, uint64_t capacity, uint32_t* out_ids, float* out_scores);
sbr_status sbr_audience_top(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, const uint32_t* items,
                            uint64_t num_queries, const uint64_t* n, uint32_t flags, float* out_cuts, uint64_t* out_counts, uint64_t* out_total,
                            uint64_t capacity, uint32_t* out_ids, float* out_scores);
sbr_status sbr_sessions_audience_top(sbr_sessions* st, const uint32_t* items, uint64_t num_queries, const uint64_t* n, const uint32_t* slots,
                                     uint64_t num_slots, const uint64_t* excl_ptr, const uint32_t* excl_slots, uint32_t flags, float* out_cuts,
                                     uint64_t* out_counts, uint64_t* out_total, uint64_t capacity, uint32_t* out_ids, float* out_scores);

/* CAPPED — exact top-k with at most `cap` items of one ITEM GROUP: "at most one per series", "two per seller", "three of a category"
 * (no counterpart in the reference crate; a larger k and a filter on the host is not exact, because no k is known to be enough).
 * ITEM GROUPS: a model may hold groups[num_items], one u32 per item, on its device.  SBR_NO_GROUP = "belongs to no group, never
 * capped".  Serving metadata exactly as the item tags: fit, sbr_model_set_param and a load leave them alone, setting them bumps no
 * parameter generation (a session store stays current), they are not saved and are freed with the model.
 * sbr_model_set_item_groups(m, NULL) clears them; sbr_model_get_item_groups gives SBR_ERR_INVALID_ARGUMENT while there are none.
 * THE RULE R(L, cap, k): L = a row's eligible items in the total order (score descending, ties to the lower id, -0.0 == +0.0).  Walk
 * L; keep an entry iff its group is SBR_NO_GROUP or fewer than cap entries of its group were kept before it; stop after k kept.  The
 * kept entries of a group are its first cap, so an entry is kept iff its ordinal within its group, among the entries before it in
 * L, is below cap — whatever k, the other groups and every earlier decision are.
 * THE CALL is the plain call at k = pool followed by R on that row.  Eligibility is the top-k sibling's in everything: history
 * (flags: SBR_RECOMMEND_INCLUDE_HISTORY) or exclusion lists, a session's seen-item memory, and the masks any_of / none_of of ITEM
 * TAGS — both NULL: no filter and no tags needed; either one non-NULL: the *_filtered call's rules.  Row u of out_items / out_scores
 * [n][k] (scores optional): the kept items with their pool scores — sbr_predict's bits — padded with (0xFFFFFFFF, -inf).
 * out_complete [n] (optional), one byte per row, is 1 iff k entries were kept or the pool row itself had padding (the pool held
 * every eligible item).  Either way the row is the exact R over the whole catalogue: an item outside the pool scores no better than
 * every pool entry, and the first k kept never reach it.  Otherwise 0: the row holds fewer than k entries, a prefix of the exact
 * answer, and a larger pool — or sbr_recommend_top at a growing n with the rule on the host, which the Python and C++ layers do —
 * finishes it.
 * ARGUMENTS: cap >= 1; 1 <= k <= pool <= SBR_RECOMMEND_MAX_K; pool == 0: the default min(1 024, max(64, 4 k)).
 * SBR_ERR_INVALID_ARGUMENT, with nothing written, for anything else, a NULL sbr_cap_args, a model without groups, masks on a model
 * without tags, and wherever the plain call gives it.  SBR_ERR_INVALID_PREDICTION: the scan's rule, a non-finite score of a scanned
 * pair.  IDENTITIES: with every item in a group of its own, or every item SBR_NO_GROUP, or cap >= k, the row is the plain call's at
 * k bit for bit and every row is complete; cap = 1 is "collapse by group".  Cost: the plain scan at k = pool and one workgroup per
 * row over the pool's ids.  Deterministic; reads parameters only.
 * Not offered: caps on similar_items, audience, the sampled or diverse calls, a cap per user or per group, among= subsets, saved
 * groups, a cap inside the scan that needs no pool. */
#define SBR_NO_GROUP 0xFFFFFFFFu
typedef struct sbr_cap_args {
    uint32_t cap;
    uint32_t pool; /* 0: the default */
} sbr_cap_args;
sbr_status sbr_model_set_item_groups(sbr_model* m, const uint32_t* groups);
sbr_status sbr_model_get_item_groups(sbr_model* m, uint32_t* out);
sbr_status sbr_recommend_capped(sbr_model* m, const uint64_t* user_ptr, const uint32_t* item_ids, uint64_t num_users, uint32_t k, uint32_t flags,
                                const struct sbr_cap_args* cap, const uint32_t* any_of, const uint32_t* none_of, uint32_t* out_items,
                                float* out_scores, uint8_t* out_complete);
sbr_status sbr_recommend_capped_reps(sbr_model* m, const float* reps, uint64_t num_users, uint32_t k, const uint64_t* excl_ptr,
                                     const uint32_t* excl_items, const struct sbr_cap_args* cap, const uint32_t* any_of,
                                     const uint32_t* none_of, uint32_t* out_items, float* out_scores, uint8_t* out_complete);
sbr_status sbr_sessions_recommend_capped(sbr_sessions* st, const uint32_t* slots, uint64_t n, uint32_t k, const uint64_t* excl_ptr,
                                         const uint32_t* excl_items, uint32_t flags, const struct sbr_cap_args* cap, const uint32_t* any_of,
                                         const uint32_t* none_of, uint32_t* out_items, float* out_scores, uint8_t* out_complete);

/* ≙ the serde derives (lstm.rs:204,386; ewma.rs:208,401): element counts and raw access. */
sbr_status sbr_model_param_count(const sbr_model* m, int32_t which, uint64_t* out_count);
sbr_status sbr_model_get_param(sbr_model* m, int32_t which, float* host_out, uint64_t count);
sbr_status sbr_model_set_param(sbr_model* m, int32_t which, const float* host_in, uint64_t count);
/* Selected rows of an item-table block — SBR_PARAM_ITEM_EMBEDDING / _ACC / _M: host_out [n][embedding_dim]; SBR_PARAM_ITEM_BIAS /
 * _ACC / _M: host_out [n] — without moving the whole table (1e7 items x 256 is 10 GB per block). */
sbr_status sbr_model_get_param_rows(sbr_model* m, int32_t which, const uint32_t* rows, uint64_t n, float* host_out);
sbr_status sbr_model_get_epoch(const sbr_model* m, uint64_t* out_global_epoch);
/* Optimiser steps taken so far (Adam's bias-correction counter) and the epoch counter that keys the
 * negative draws: together with the parameter blocks this is the complete resumable state. */
sbr_status sbr_model_get_counters(const sbr_model* m, uint64_t* out_global_epoch, uint64_t* out_optimizer_steps);
/* State of the model RNG (the Hyperparameters' rng, which the reference serialises with the model,
 * lstm.rs:38-51): 16 bytes that re-create it through XorShiftRng::from_seed.  A restored model continues
 * the shuffle / partition-seed stream of the saved one. */
sbr_status sbr_model_get_rng(const sbr_model* m, uint8_t out_state[16]);
sbr_status sbr_model_set_rng(sbr_model* m, const uint8_t state[16]);
sbr_status sbr_model_set_counters(sbr_model* m, uint64_t global_epoch, uint64_t optimizer_steps);

/* Library / device identification ("gfx950", CU count, HBM bytes); device_name may be NULL. */
sbr_status sbr_device_info(char* device_name, uint64_t name_bytes, uint32_t* out_cus, uint64_t* out_hbm_bytes);
const char* sbr_status_string(sbr_status s);
/* ITEM SETS — every catalogue call above restricted to a set of items S (in stock, one category, this week's releases) that is kept
 * on the device.  An item set is a handle owned by a model: the sorted, de-duplicated ids S and a persistent device copy of their
 * rows, E'[j] = E[S[j]] and b'[j] = b[S[j]] at storage width (|S| * (storage width + 1) * 4 bytes of plain device memory), gathered
 * once at creation, so that a call's cost follows |S| and not the catalogue.
 * The contract is sbr_recommend_among's, for every family: a call through a set returns, bit for bit, what the same call on the
 * model returns with every item outside S added to each row's exclusion list — ids (catalogue ids, never positions), score bits,
 * keys, order, padding, the non-finite rule, shift and mass as integers (out_frac_bits is the MODEL's F), counts, cuts, CSR
 * contents and complete flags.  The noise of a sampled call is a function of (seed, stream, catalogue id), as on the model.  Inputs
 * stay catalogue ids — histories, exclusion lists, a session's seen items — and entries outside S are ignored.  Rows outside S are
 * never read: a non-finite row outside S fails no call, one inside S does.
 * Lifecycle: the set is bound to the model's parameters as a session store is.  After sbr_model_fit, sbr_model_set_param or a load
 * every scan through it returns SBR_ERR_INVALID_ARGUMENT until sbr_item_set_refresh gathers the rows again; while a fit plan is
 * open on the model every call but size / items / destroy does.  Item tags and item groups are not cached: every launch gathers the
 * set's words, so sbr_model_set_item_tags / sbr_model_set_item_groups take effect at once.  An empty set is legal: every call answers
 * as the plain call does for a row that may see nothing.  sbr_item_set_create takes ids in any order, duplicates allowed; an id >=
 * num_items is an argument error.  A set follows the session stores' rule of destruction: it holds a pointer to its model and works
 * on the model's stream; it is destroyed before its model.
 * One descriptor names a call's rows — exactly one of three sources (zero or two: an argument error):
 *   histories        user_ptr / item_ids as sbr_recommend's, flags 0 or SBR_RECOMMEND_INCLUDE_HISTORY; excl_* must be NULL;
 *   representations  reps [num_rows][embedding_dim] as the *_reps calls', flags 0, with the optional lists excl_ptr / excl_items;
 *   a store          store / slots as the sbr_sessions_* scans', the store current and of the set's model, flags as theirs
 *                    (SBR_RECOMMEND_INCLUDE_HISTORY: do not exclude the seen items), with the optional lists.
 * any_of / none_of (both NULL: no filter) are the tag masks of the filtered forms, one pair per row.  The seven scan calls take the
 * descriptor and then the argument tail of their *_reps siblings without the lists and masks, which the descriptor carries; the
 * rollout and beam-search calls take a store descriptor and the argument tail of their sbr_sessions_* siblings. */
typedef struct sbr_item_set sbr_item_set;
typedef struct sbr_scan_rows {     /* exactly one of the three sources */
    const uint64_t* user_ptr; const uint32_t* item_ids; uint32_t flags;   /* histories; SBR_RECOMMEND_INCLUDE_HISTORY */
    const float* reps;                                                    /* representations */
    sbr_sessions* store; const uint32_t* slots;                           /* a current store of the set's model; flags' INCLUDE_HISTORY = include_seen */
    const uint64_t* excl_ptr; const uint32_t* excl_items;                 /* caller's lists (reps, store); nullable */
    const uint32_t *any_of, *none_of;                                     /* nullable */
} sbr_scan_rows;
sbr_status sbr_item_set_create(sbr_model* m, const uint32_t* item_ids, uint64_t n, sbr_item_set** out);
void sbr_item_set_destroy(sbr_item_set* set);
sbr_status sbr_item_set_size(const sbr_item_set* set, uint64_t* out);
sbr_status sbr_item_set_items(const sbr_item_set* set, uint32_t* out); /* out [size]: the sorted unique ids */
sbr_status sbr_item_set_refresh(sbr_item_set* set);
sbr_status sbr_item_set_recommend(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, uint32_t k, uint32_t* out_items,
                                  float* out_scores);
sbr_status sbr_item_set_recommend_diverse(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, uint32_t k, uint32_t pool,
                                          float trade_off, uint32_t metric, uint32_t* out_items, float* out_scores);
sbr_status sbr_item_set_recommend_sampled(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, uint32_t k,
                                          const struct sbr_sample_args* sample, uint32_t* out_items, float* out_scores, float* out_keys);
sbr_status sbr_item_set_log_partition(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, float temperature, float* out_shift,
                                      uint64_t* out_mass, uint32_t* out_frac_bits);
sbr_status sbr_item_set_recommend_above(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, const float* thresholds,
                                        uint64_t* out_counts, uint64_t* out_total, uint64_t capacity, uint32_t* out_ids, float* out_scores);
sbr_status sbr_item_set_recommend_top(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, const uint64_t* n, float* out_cuts,
                                      uint64_t* out_counts, uint64_t* out_total, uint64_t capacity, uint32_t* out_ids, float* out_scores);
sbr_status sbr_item_set_recommend_capped(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, uint32_t k,
                                         const struct sbr_cap_args* cap, uint32_t* out_items, float* out_scores, uint8_t* out_complete);
/* ROLLOUT and BEAM SEARCH within a set: sbr_sessions_rollout / sbr_sessions_beam_search of rows->store and rows->slots with every
 * item outside S appended to each row's exclusion list, bit for bit — items (catalogue ids), scores, keys (the same draw per
 * (seed + j, stream, catalogue id)), lengths, padding, out_h / out_c, out_step_lp / out_cum / out_beams, shift and mass, and
 * out_frac_bits the MODEL's F.  A set of the whole catalogue is the plain call; an empty set ends every row at step 0 (out_h / out_c
 * the slots' current states, beams 0).  Only the store source: user_ptr or reps is SBR_ERR_INVALID_ARGUMENT, and so is rows->flags
 * != 0 — include_seen is said once, as SBR_ROLLOUT_INCLUDE_SEEN in args->flags.  excl_ptr / excl_items and any_of / none_of are the
 * plain call's, entries outside S ignored.  Every other argument rule is the plain call's, with the set's lifecycle above.  Per step
 * the unchanged scans run over the set's sub-table and the picks fed back are catalogue ids. */
sbr_status sbr_item_set_rollout(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, const struct sbr_rollout_args* args,
                                uint32_t* out_items, float* out_scores, float* out_keys, uint32_t* out_lengths, float* out_shift,
                                uint64_t* out_mass, uint32_t* out_frac_bits, float* out_h, float* out_c);
sbr_status sbr_item_set_beam_search(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, const struct sbr_beam_args* args,
                                    uint32_t* out_items, float* out_scores, float* out_step_lp, float* out_cum, uint32_t* out_lengths,
                                    uint32_t* out_beams, float* out_shift, uint64_t* out_mass, uint32_t* out_frac_bits);
/* ELIGIBLE RANKS — sbr_rank_targets among what a row may be shown: under tag masks, through an item set, on a session store.
 * For a row with list L (its history unless SBR_RECOMMEND_INCLUDE_HISTORY, or the caller's excl list, united with the slot's seen
 * items on a store with memory unless that flag is given), masks (any_of, none_of) and an optional set S, let
 *   M = unique(L) ∪ { i : tags[i] is not allowed by the masks } ∪ (catalogue \ S).
 * The ranks are, integer for integer, what sbr_rank_targets_reps returns for the row's representation with the mask list M:
 * m(i) = f32::MIN on M, else sbr_predict's score; rank(t) = #{ i in the catalogue : m(i) >= m(t) }.  So a target in M has rank
 * num_items — the CATALOGUE's, also through a set — ties count against the target, duplicate targets get equal ranks, all-zero
 * masks without a set is the plain call, and a set of every item is the model's call.  Targets are catalogue ids; an id >= num_items
 * is SBR_ERR_INVALID_ARGUMENT.  The descriptor's sources, lists, masks and flags are those of the item-set scans above; masks need
 * sbr_model_set_item_tags; a stale set or store and an open fit plan refuse the call; the flag on a store without memory is an
 * error.  A non-finite score of a scanned pair fails the call (SBR_ERR_INVALID_PREDICTION) whether the masks allow the item or not;
 * rows outside S are never read.  An empty set answers on the host: every rank is num_items.  out_ranks [target_ptr[num_rows] -
 * target_ptr[0]] in target order; a row's targets are scanned rank_targets' way, up to 16 (8 at storage width 256) per scan row. */
sbr_status sbr_rank_targets_rows(sbr_model* m, const struct sbr_scan_rows* rows, uint64_t num_rows, const uint64_t* target_ptr,
                                 const uint32_t* target_items, uint32_t* out_ranks);
sbr_status sbr_item_set_rank_targets(sbr_item_set* set, const struct sbr_scan_rows* rows, uint64_t num_rows, const uint64_t* target_ptr,
                                     const uint32_t* target_items, uint32_t* out_ranks);

#define SBR_ABI_VERSION 13u /* what sbr_abi_version returns from a library built from this header */
uint32_t sbr_abi_version(void);

/* Scratch of a fit call (device and pinned-host blocks up to 64 MiB, at most 768 MiB of each kind per process) is kept for the
 * next call instead of going back to the driver: the reference's own bench re-fits one model in a loop
 * (benches/benchmark.rs:40-42) and ~50 allocations per call cost more than its kernels.  This returns everything that is idle
 * to the driver (a long-lived host process that is done fitting). */
void sbr_release_cached_memory(void);

/* Kernel timing hook for bench.py: wall time (ms, HIP events on the engine stream) and launch
 * count accumulated per kernel family since the last reset.  Families: see sbr_kernel_family. */
typedef enum sbr_kernel_family {
    SBR_K_RECURRENT_FWD = 0,
    SBR_K_SCORE = 1,       /* gather + negative sampling + loss: the HBM-roofline kernel */
    SBR_K_RECURRENT_BWD = 2,
    SBR_K_DENSE_GRAD = 3,
    SBR_K_DENSE_UPDATE = 4,
    SBR_K_SPARSE_UPDATE = 5,
    SBR_K_RANK = 6,
    SBR_K_SPARSE_SORT = 7, /* key ordering of the sparse update: radix passes + segment heads (sbr_sort.hip) */
    SBR_K_FAMILIES = 8
} sbr_kernel_family;
sbr_status sbr_model_timing_enable(sbr_model* m, int32_t enable);
/* Which families' launches are bracketed by events while timing is enabled (bit f = sbr_kernel_family f; default: all).  Every
 * bracketed launch costs two event records on its stream — a few microseconds each, which a 2.5 ms step of ~20 launches feels —
 * so a throughput measurement that needs one kernel's duration selects that family alone. */
sbr_status sbr_model_timing_select(sbr_model* m, uint32_t family_mask);
/* enable = 0 queues the side-stream work (key sort, dense-gradient GEMM) on the main stream, so that every
 * kernel family is timed running alone; results are identical.  Default: overlap on. */
sbr_status sbr_model_set_overlap(sbr_model* m, int32_t enable);
sbr_status sbr_model_timing_read(sbr_model* m, double* out_ms /*[SBR_K_FAMILIES]*/, uint64_t* out_launches /*[SBR_K_FAMILIES]*/);


/* Selects the HIP device this process drives (before sbr_model_create); default = current device. */
sbr_status sbr_set_device(int32_t ordinal);

/* Numerics-contract self-tests: run sbr_numerics.h primitives on the device so tests can compare
 * them bit for bit with the CPU oracle (no reference counterpart: wyrm's fast-math kernels are
 * replaced by the engine's own). */
sbr_status sbr_selftest_math(const float* x, uint64_t n, float* out_cell_h, float* out_sig, float* out_tanh);
sbr_status sbr_selftest_dot_tree(const float* x, const float* y, uint32_t d, uint64_t nrows, float* out);
sbr_status sbr_selftest_mfma(const float* a, const float* b, const float* c0, uint32_t k, float* out,
                             const float* a32, const float* b32, float* out32);
/* The sparse update's key ordering alone (sbr_sort.hip; ≙ the per-row visiting order of Optimizer::step over the sparse
 * gradients, sequence_model.rs:163-169): out_keys[n] = (rows[e] << 32 | e) in (row, e) order, row ids below 2^row_bits;
 * out_head_pos[*out_nheads + 1] = positions where a new row starts, then n. */
sbr_status sbr_selftest_sort(const uint32_t* rows, uint64_t n, uint32_t row_bits, uint64_t* out_keys, uint32_t* out_head_pos,
                             uint32_t* out_nheads);

/* Stream-delay test hook (tests/test_stream_joins_gpu.py).  A training step is spread over three or four streams
 * per model (main, side, sorter, copier) and one exchange stream per member of a group plan (xs), tied together by events.  The
 * environment variable
 *     SBR_TEST_STREAM_DELAY="<role>[@<device>]=<microseconds>[,...]"     roles: main side sorter copier xs
 * read per call, makes the named streams LATE: a delay kernel (one wave, no memory traffic; it sleeps until a constant-rate
 * clock has advanced by the requested time, at most 5 000 us, under a fixed cap of polls — a bounded wait) is queued right
 * behind every cross-stream wait the engine issues on such a stream, and at the head of the first work a call queues on it where
 * no wait precedes that work.  @<device> restricts an entry to the model whose device_rank it names.  A consumer that waits for
 * the late stream's event computes the same bits; one that does not reads stale data.  Unset: nothing changes.
 * sbr_test_delays_queued: the delay kernels queued on this model's streams per role, in the order above, since the last read.
 * sbr_selftest_stream_delay: the method's own check — a device float that is 1.0; one stream is delayed, stores 2.0 and records
 * an event; a second stream waits for that event (with_join != 0) or not and copies the float: *out = 2.0 with the join, 1.0
 * without it. */
sbr_status sbr_test_delays_queued(sbr_model* m, uint64_t out[5]);
sbr_status sbr_selftest_stream_delay(uint32_t delay_us, int32_t with_join, float* out);

/* Poisoned-scratch test hook (tests/test_poisoned_scratch_gpu.py).  The engine's scratch comes from three places: a
 * process-wide cache of device blocks and of pinned host blocks, which hands blocks of finished calls out again with their old
 * content, and each model's serving arena, which every serving call carves anew out of what the previous call left there.  The
 * environment variable
 *     SBR_TEST_POISON=<byte>     1..255; unset or 0: off
 * read each time memory is handed out, fills every block the cache hands out (the whole block as stored, hit or fresh) and the
 * part of the arena a carve uses with that byte first.  Code that writes what it reads computes the same bits; code that relies
 * on zeros or on leftovers does not.  The pages of a partitioned table are parameters, not scratch, and are left alone.
 * sbr_selftest_scratch: the method's own check — a block of the cache (kind 0 device, 1 pinned host) as handed out, copied to
 * out_host[0, bytes); the block is zeroed and given back; the same size taken again, the cache hit, copied to
 * out_host[bytes, 2 bytes).  sbr_selftest_arena: the same with two carves of `bytes` of m's serving arena.  With the hook set
 * every byte of both copies is the pattern. */
sbr_status sbr_selftest_scratch(uint32_t kind, uint64_t bytes, void* out_host);
sbr_status sbr_selftest_arena(sbr_model* m, uint64_t bytes, void* out_host);

/* Guarded-scratch test hook (tests/test_guarded_scratch_gpu.py): where the kernels WRITE.  The cache's blocks and
 * the arena's takes lie back to back, rounded to 256 bytes, a cache hit up to twice the request: a store past the end of its
 * buffer faults nowhere.  The environment variable
 *     SBR_TEST_GUARD=<KiB>     1..1048576; unset, 0 or malformed: off
 * read each time memory is handed out, puts a band of KiB x 1024 guard bytes (0xA5) in front of every block of the cache
 * (device and pinned host; hit, fresh, or past the cache's 64 MiB) and behind it — from the first byte past the REQUESTED size,
 * through the rounding and the unused part of a cache hit — and likewise behind every take of a carve of the serving arena and in
 * front of its first take.  With SBR_TEST_POISON as well, the poison byte fills the payload and the guard byte the bands.  The
 * bands are compared with the guard byte when a block is given back, at the head of the model's next carve and when the model
 * releases its arena; a changed band is a count and a record below (and is filled again), never an abort.  Reads past a buffer,
 * a stride that jumps a whole band, stores into another live buffer's payload, the pages of a partitioned table and exportable
 * lists, and the caller's own output arrays are not seen.
 * sbr_test_guard_report: synchronises the device, checks every live block of the cache and (m non-null) the current carve of m's
 * arena, adds what the checks above found since the last report, and resets the counters.
 * sbr_selftest_guard: the method's own check — a device block (where = SBR_GUARD_DEVICE_BLOCK), a pinned block, three arena takes
 * of m, or a device block past the cache's 64 MiB (SBR_GUARD_BIG_BLOCK; reported as a device block), each of 4 196 bytes (the big
 * block: 64 MiB more); the library sets ONE byte with hipMemset / memset — side > 0: the first byte past the request (of the
 * middle take), side < 0: the last byte before the block (before the first take) — and out[0] is the report of that alone;
 * out[1] the same on the re-used allocation: the cache hit, the second carve.  Pending findings of other checks are kept for the
 * next sbr_test_guard_report.  Hook off: nothing is written and both reports are zero.  m is needed for the arena only. */
enum {
    SBR_GUARD_NONE = 0,
    SBR_GUARD_DEVICE_BLOCK = 1,
    SBR_GUARD_PINNED_BLOCK = 2,
    SBR_GUARD_ARENA_TAKE = 3,
    SBR_GUARD_BIG_BLOCK = 4
};
typedef struct sbr_guard_report {
    uint64_t blocks;     /* cache blocks checked */
    uint64_t takes;      /* arena takes checked */
    uint64_t bytes;      /* guard bytes compared */
    uint64_t violations; /* bands with at least one changed byte */
    /* the first violated band: */
    uint64_t where;      /* SBR_GUARD_* */
    uint64_t ordinal;    /* of the take within its carve; of the block among the guarded blocks handed out since the last report */
    uint64_t requested;  /* bytes the owner asked for */
    int64_t offset;      /* of the first changed byte: +1 = the first byte past the request, -1 = the last byte before its start */
    uint64_t changed;    /* changed bytes in that band */
} sbr_guard_report;
sbr_status sbr_test_guard_report(sbr_model* m, sbr_guard_report* out);
sbr_status sbr_selftest_guard(sbr_model* m, uint32_t where, int32_t side, sbr_guard_report out[2]);

#ifdef __cplusplus
}
#endif
#endif /* SBR_HIP_H */
