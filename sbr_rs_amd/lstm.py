"""LSTM-based sequence model — host-side mirror of ``sbr::models::lstm``
(/root/reference/src/models/lstm.rs): same builder, same method names, same error behaviour,
calling the gfx950 engine through the C-ABI instead of wyrm."""
from __future__ import annotations

import os

import numpy as np

from ._abi import ModelKind, make_hparams
from .data import CompressedInteractions
from .engine import Model
from .models import ImplicitUser, Loss, LSTMVariant, Optimizer, Parallelism
from .rng import XorShiftRng


class _HyperparametersBase:
    """Builder shared by lstm::Hyperparameters (lstm.rs:39-202) and ewma::Hyperparameters
    (ewma.rs:45-206).  Defaults follow ``new`` (lstm.rs:56-71 / ewma.rs:61-75)."""

    def __init__(self, num_items: int, max_sequence_length: int):
        self._num_items = int(num_items)
        self._max_sequence_length = int(max_sequence_length)
        self._item_embedding_dim = 16
        self._learning_rate = 0.01
        self._l2_penalty = 0.0
        self._loss = Loss.BPR
        self._optimizer = Optimizer.Adam
        self._parallelism = Parallelism.Synchronous
        self._rng = XorShiftRng.from_seed(os.urandom(16))  # rand::thread_rng().gen()
        self._num_threads = 1  # devices; the reference default is rayon::current_num_threads()
        self._num_epochs = 10
        self._batch_sequences = 32  # GPU minibatch (no reference counterpart; 1 = per-sequence SGD)

    def learning_rate(self, learning_rate: float):
        self._learning_rate = float(learning_rate)
        return self

    def l2_penalty(self, l2_penalty: float):
        self._l2_penalty = float(l2_penalty)
        return self

    def embedding_dim(self, embedding_dim: int):
        self._item_embedding_dim = int(embedding_dim)
        return self

    def num_epochs(self, num_epochs: int):
        self._num_epochs = int(num_epochs)
        return self

    def loss(self, loss: Loss):
        self._loss = Loss(loss)
        return self

    def num_threads(self, num_threads: int):
        """Number of parallel workers = devices (lstm.rs:110-113)."""
        self._num_threads = int(num_threads)
        return self

    def parallelism(self, parallelism: Parallelism):
        self._parallelism = Parallelism(parallelism)
        return self

    def rng(self, rng: XorShiftRng):
        self._rng = rng
        return self

    def from_seed(self, seed):
        self._rng = XorShiftRng.from_seed(seed)
        return self

    def optimizer(self, optimizer: Optimizer):
        self._optimizer = Optimizer(optimizer)
        return self

    def batch_sequences(self, batch_sequences: int):
        """Subsequences per optimiser step (engine extension)."""
        self._batch_sequences = int(batch_sequences)
        return self

    def partition_item_table(self, flag: bool = True):
        """With ``num_threads(n) > 1`` in one process: store the item table once, row range r on replica
        r's device, instead of n full copies (engine extension; results are identical)."""
        self._partition = bool(flag)
        return self

    def _build_engine(self, model_kind: int, device_rank: int):
        """Model handle(s) for build(): one handle, or the whole single-process group when the item
        table is partitioned (the replicas must then be created together)."""
        hp = self._hparams(model_kind, device_rank)
        if getattr(self, "_partition", False):
            import torch.distributed as dist

            if dist.is_available() and dist.is_initialized() and dist.get_world_size() == self._num_threads > 1:
                # one process per GPU: this process owns the rows of its rank, the peers' rows are mapped
                from .partitioned import create_partitioned_model

                return create_partitioned_model(self._hparams(model_kind, dist.get_rank())), None
            from .engine import group_create

            group = group_create(hp, self._num_threads, partition_item_table=True)
            return group[0], group
        return Model(hp), None

    def _hparams(self, model_kind: int, device_rank: int = 0):
        return make_hparams(self._num_items, self._max_sequence_length, self._item_embedding_dim, self._learning_rate,
                            self._l2_penalty, model_kind, int(self._loss), int(self._optimizer), int(self._parallelism),
                            self._rng.state_seed(), self._num_epochs, self._num_threads, device_rank,
                            self._batch_sequences)

    @classmethod
    def _random_common(cls, num_items: int, rng: XorShiftRng):
        """``Hyperparameters::random`` (lstm.rs:141-172): same ranges; the draws come from this
        engine's RNG, so the sampled points differ from the Rust crate's."""
        def uni(lo, hi):
            return lo + (hi - lo) * rng.unit()

        h = cls(num_items, 2 ** (4 + rng.below(4)))
        h._item_embedding_dim = 2 ** (4 + rng.below(4))
        h._learning_rate = float(np.float32(10.0) ** np.float32(uni(-3.0, 0.5)))
        h._l2_penalty = float(np.float32(10.0) ** np.float32(uni(-7.0, -3.0)))
        h._loss = Loss.BPR if uni(0.0, 1.0) < 0.5 else Loss.Hinge
        h._optimizer = Optimizer.Adam if uni(0.0, 1.0) < 0.5 else Optimizer.Adagrad
        return h, uni


class Hyperparameters(_HyperparametersBase):
    """Hyperparameters for the ImplicitLSTMModel (lstm.rs:39-202)."""

    def __init__(self, num_items: int, max_sequence_length: int):
        super().__init__(num_items, max_sequence_length)
        self._lstm_type = LSTMVariant.Coupled

    @classmethod
    def new(cls, num_items: int, max_sequence_length: int) -> "Hyperparameters":
        return cls(num_items, max_sequence_length)

    def lstm_variant(self, variant: LSTMVariant):
        self._lstm_type = LSTMVariant(variant)
        return self

    @classmethod
    def random(cls, num_items: int, rng: XorShiftRng) -> "Hyperparameters":
        h, uni = cls._random_common(num_items, rng)
        h._lstm_type = LSTMVariant.Normal if uni(0.0, 1.0) < 0.5 else LSTMVariant.Coupled
        h._parallelism = Parallelism.Asynchronous if uni(0.0, 1.0) < 0.5 else Parallelism.Synchronous
        h._num_epochs = 2 ** (3 + rng.below(4))
        return h

    def build(self, device_rank: int = 0) -> "ImplicitLSTMModel":
        """Build a model out of the chosen hyperparameters (lstm.rs:197-201): parameters are
        initialised from the builder's RNG on the device."""
        kind = ModelKind.LSTM_NORMAL if self._lstm_type == LSTMVariant.Normal else ModelKind.LSTM_COUPLED
        return ImplicitLSTMModel(*self._build_engine(int(kind), device_rank))


class _ImplicitSequenceModel:
    """fit / OnlineRankingModel surface shared by both models (lstm.rs:391-416, ewma.rs:404-429)."""

    def __init__(self, engine_model: Model, group=None):
        self.params = engine_model
        self._peers = group[1:] if group else None

    def fit(self, interactions: CompressedInteractions) -> float:
        """Fit the model; returns the loss value.  Raises FittingError.NoInteractions
        (lstm.rs:395-397 → sequence_model.rs:86-88)."""
        world = int(self.params.hp.num_devices)
        if world == 1:
            return self.params.fit(interactions.user_pointers, interactions.item_ids)
        try:  # torch is needed only for the one-process-per-GPU driver
            import torch.distributed as dist

            launched = dist.is_available() and dist.is_initialized()
        except ImportError:
            launched = False
        if launched and getattr(self, "_peers", None) is None:
            # one process per GPU (torchrun): this process drives replica hp.device_rank
            if self.params.is_partitioned():
                from .partitioned import fit_partitioned

                return fit_partitioned(self.params, interactions)
            from .distributed import fit_distributed

            return fit_distributed(self.params, interactions)
        # one process, num_threads replicas (≙ the reference's rayon workers): sbr_group_fit
        from .engine import group_fit

        return group_fit(self._replicas(), interactions.user_pointers, interactions.item_ids)

    def set_reference_order(self, on: bool = True):
        """The crate's own ORDER of work at one subsequence per step (``batch_sequences(1)``, embedding_dim <= 32): negatives from the
        worker's sequential XorShiftRng stream (sequence_model.rs:58-65, :137) and, with ``num_threads(n)``, one optimiser application
        per worker in worker order (:163-166).  Call before ``fit``."""
        for m in self._replicas():
            m.set_reference_order(on)
        return self

    def last_fit_lagged_loss(self) -> float:
        """The number the reference's ``fit`` would have returned for the last single-process ``fit`` (one device or
        ``num_threads`` replicas): sequence_model.rs:157 reads the loss node before :160 runs its forward pass, so every
        subsequence of s steps contributes the running loss sum L_{s-1} of the worker's most recent earlier subsequence with at
        least s steps (the loss nodes are shared running sums, lstm.rs:322-328).  ``fit`` returns the
        true mean loss."""
        return self.params.last_fit_lagged_loss()

    def _replicas(self):
        """Replica r of a single-process multi-device model lives on HIP device r mod device_count;
        the peers are created at the first fit, from the same seed as the primary."""
        if getattr(self, "_peers", None) is None:
            import copy

            from .engine import device_count, set_device

            if int(self.params.hp.device_rank) != 0 or self.params.counters() != (0, 0):
                raise RuntimeError("single-process multi-device fit needs the untrained rank-0 model")
            ndev = device_count()
            peers = []
            for r in range(1, int(self.params.hp.num_devices)):
                hp = copy.copy(self.params.hp)
                hp.device_rank = r
                set_device(r % ndev)
                peers.append(Model(hp))
            set_device(0)
            self._peers = peers
        return [self.params] + self._peers

    def user_representation(self, item_ids) -> ImplicitUser:
        return ImplicitUser(self.params.user_representation(np.asarray(item_ids, dtype=np.uint32)))

    def predict(self, user: ImplicitUser, item_ids) -> np.ndarray:
        return self.params.predict(user.user_embedding, np.asarray(item_ids, dtype=np.uint32))

    @staticmethod
    def _csr(interactions_or_histories):
        """A CompressedInteractions or a list of item-id sequences -> (pointers u64, item ids u32)"""
        if isinstance(interactions_or_histories, CompressedInteractions):
            return interactions_or_histories.user_pointers, interactions_or_histories.item_ids
        seqs = [np.asarray(h, dtype=np.uint32).ravel() for h in interactions_or_histories]
        up = np.zeros(len(seqs) + 1, dtype=np.uint64)
        up[1:] = np.cumsum([s.size for s in seqs])
        return up, (np.concatenate(seqs) if seqs else np.zeros(0, dtype=np.uint32))

    def set_item_tags(self, tags):
        """One 32-bit tag word per item for the ``any_of=`` / ``none_of=`` filters of ``recommend``, ``recommend_diverse``,
        ``similar_items`` and the session calls, kept on the device; ``None`` clears them.  Tags are serving metadata: ``fit``
        leaves them alone and ``save`` does not write them — set them again after ``load``."""
        self.params.set_item_tags(tags)
        return self

    def item_tags(self) -> np.ndarray:
        """The tag words last set (u32 [num_items]); raises while the model has none."""
        return self.params.item_tags()

    def recommend(self, interactions_or_histories, k: int, exclude_history: bool = True, among=None, any_of=None, none_of=None):
        """The k best items of the whole catalogue for each user's history, on the device: (items [U, k] u32, scores
        [U, k] f32), score descending, ties to the lower item id.  ``interactions_or_histories`` is a
        CompressedInteractions or a list of item-id sequences.  Every item of a history is excluded unless
        ``exclude_history`` is False; a row with fewer than k eligible items is padded with (0xFFFFFFFF, -inf).
        ``among``: None, or the item ids the answer is restricted to (in stock, one category, ...; any order, duplicates
        allowed) — the exact top k of that set, found by scanning its rows only.
        ``any_of`` / ``none_of``: the per-user tag filter against ``set_item_tags`` — a u32 mask per user, or one for all: item
        i is eligible for user u iff ``tags[i] & none_of[u] == 0 and (any_of[u] == 0 or tags[i] & any_of[u] != 0)`` (territory,
        rating, tier, in stock, "not this category"), tested inside the scan.  Not together with ``among``: ``item_set(among)`` takes
        both, and keeps the set on the device between calls."""
        up, it = self._csr(interactions_or_histories)
        if among is None:
            return self.params.recommend(up, it, k, include_history=not exclude_history, any_of=any_of, none_of=none_of)
        if any_of is not None or none_of is not None:
            raise ValueError("a tag filter together with among= is not supported: filter the item set instead, or use item_set()")
        return self.params.recommend_among(up, it, k, among, include_history=not exclude_history)

    def recommend_sampled(self, interactions_or_histories, k: int, temperature: float = 1.0, seed: int = 0, streams=None,
                          exclude_history: bool = True, any_of=None, none_of=None, log_prob: bool = False):
        """``recommend`` with a dice: k draws without replacement from softmax(score / ``temperature``) over the items each user
        may see, inside the catalogue scan — (items [U, k] u32, scores [U, k] f32: the plain scores of the drawn items in draw
        order, keys [U, k] f32 descending).  Exploration, slates that differ between visits, and reproducible randomised logging:
        the noise of a row is a function of (``seed``, ``streams[row]``, item) alone — ``streams`` one integer per row (a user or
        request id), default the row's index — so the same (seed, stream) gives the same row bit for bit.  Eligibility
        (``exclude_history``, ``any_of`` / ``none_of``) is ``recommend``'s.  A small temperature approaches ``recommend``.
        ``log_prob=True`` appends log_prob [U, k] f64, each draw's propensity given the draws before it (``log_partition``)."""
        up, it = self._csr(interactions_or_histories)
        return self.params.recommend_sampled(up, it, k, temperature=temperature, seed=seed, streams=streams,
                                             include_history=not exclude_history, any_of=any_of, none_of=none_of, log_prob=log_prob)

    def recommend_sampled_reps(self, reps, k: int, temperature: float = 1.0, seed: int = 0, streams=None, exclude=None, any_of=None,
                               none_of=None, log_prob: bool = False):
        """``recommend_sampled`` from representations [U, embedding_dim] (``user_representations``); ``exclude``: None or one
        sequence of item ids per user."""
        return self.params.recommend_sampled_reps(reps, k, temperature=temperature, seed=seed, streams=streams, exclude=exclude,
                                                  any_of=any_of, none_of=none_of, log_prob=log_prob)

    def log_partition(self, interactions_or_histories, temperature: float = 1.0, exclude_history: bool = True, any_of=None,
                      none_of=None):
        """The softmax normaliser of ``recommend_sampled``'s distribution, exactly: per user the mass of softmax(score /
        ``temperature``) over the items ``recommend`` would choose from, summed on the device as integers in fixed point, so the
        result does not depend on the batch or on how the scan is cut up (``engine.Partition``: ``shift``, ``mass``, ``frac_bits``,
        ``log_z``, ``log_prob(scores)`` and ``slate_log_prob(scores)`` — the propensities that off-policy evaluation needs)."""
        up, it = self._csr(interactions_or_histories)
        return self.params.log_partition(up, it, temperature, include_history=not exclude_history, any_of=any_of, none_of=none_of)

    def log_partition_reps(self, reps, temperature: float = 1.0, exclude=None, any_of=None, none_of=None):
        """``log_partition`` from representations [U, embedding_dim]; ``exclude``: None or one sequence of item ids per user."""
        return self.params.log_partition_reps(reps, temperature, exclude=exclude, any_of=any_of, none_of=none_of)

    def audience(self, interactions_or_histories, items, k: int, exclude_history: bool = True):
        """The reverse of ``recommend``: for each query item of ``items`` the k users whose histories score it highest, on the
        device — (users [Q, k] u32, scores [Q, k] f32), ``predict``'s bits, score descending, ties to the lower user, short rows
        padded with (0xFFFFFFFF, -inf).  Runs ``user_representations``, then ``params.audience_reps``; with ``exclude_history`` a
        user whose history holds the query item is left out of that item's row.  For live sessions: ``sessions(...).audience``."""
        up, it = self._csr(interactions_or_histories)
        return self.params.audience(up, it, items, k, include_history=not exclude_history)

    def recommend_above(self, interactions_or_histories, threshold, exclude_history: bool = True, any_of=None, none_of=None,
                        max_results=None, order: str = "score"):
        """``recommend`` without a k: for each user's history EVERY eligible item whose score is >= ``threshold`` (a scalar or one
        per user), on the device — an ``engine.Above`` (``ptr``, ``ids``, ``scores``, ``counts``, ``row(i)``, ``pairs()``), each row
        by score descending with ties to the lower id (``order="id"``: ascending id).  The set may hold far more than
        ``recommend``'s 1 024 per row.  With ``log_partition``, ``threshold = temperature * (np.log(p) + part.log_z)`` reads
        "every item this user would be shown with probability at least p".  ``max_results`` (default 2^24 pairs) bounds the
        result; a larger one raises a ValueError that states the total (``count_above`` says how many to expect)."""
        up, it = self._csr(interactions_or_histories)
        return self.params.recommend_above(up, it, threshold, include_history=not exclude_history, any_of=any_of, none_of=none_of,
                                           max_results=max_results, order=order)

    def count_above(self, interactions_or_histories, threshold, exclude_history: bool = True, any_of=None, none_of=None):
        """``recommend_above(...).counts`` without writing any pair: one scan, the cheap way to choose a threshold."""
        up, it = self._csr(interactions_or_histories)
        return self.params.count_above(up, it, threshold, include_history=not exclude_history, any_of=any_of, none_of=none_of)

    def recommend_above_reps(self, reps, threshold, exclude=None, any_of=None, none_of=None, max_results=None, order: str = "score"):
        """``recommend_above`` from representations [U, embedding_dim]; ``exclude``: None or one sequence of item ids per user."""
        return self.params.recommend_above_reps(reps, threshold, exclude=exclude, any_of=any_of, none_of=none_of, max_results=max_results,
                                                order=order)

    def count_above_reps(self, reps, threshold, exclude=None, any_of=None, none_of=None):
        """``recommend_above_reps(...).counts`` without writing any pair."""
        return self.params.count_above_reps(reps, threshold, exclude=exclude, any_of=any_of, none_of=none_of)

    def audience_above(self, interactions_or_histories, items, threshold, exclude_history: bool = True, max_results=None,
                       order: str = "score"):
        """``audience`` without a k: for each query item EVERY user whose history scores it >= ``threshold`` (a scalar or one per
        query) — an ``engine.Above`` over the queries, user indices.  For live sessions: ``sessions(...).audience_above``."""
        up, it = self._csr(interactions_or_histories)
        return self.params.audience_above(up, it, items, threshold, include_history=not exclude_history, max_results=max_results,
                                          order=order)

    def count_audience_above(self, interactions_or_histories, items, threshold, exclude_history: bool = True):
        """``audience_above(...).counts`` without writing any pair."""
        up, it = self._csr(interactions_or_histories)
        return self.params.count_audience_above(up, it, items, threshold, include_history=not exclude_history)

    def audience_above_reps(self, reps, items, threshold, exclude=None, max_results=None, order: str = "score"):
        """``audience_above`` over representation rows [S, embedding_dim]; ``exclude``: None or one sequence of row indices per
        query."""
        return self.params.audience_above_reps(reps, items, threshold, exclude=exclude, max_results=max_results, order=order)

    def count_audience_above_reps(self, reps, items, threshold, exclude=None):
        """``audience_above_reps(...).counts`` without writing any pair."""
        return self.params.count_audience_above_reps(reps, items, threshold, exclude=exclude)

    def set_item_groups(self, groups):
        """One u32 group word per item — a series, a seller, a category; ``engine.NO_GROUP`` (0xFFFFFFFF) for an item that is
        never capped — for ``recommend_capped`` and the session call, kept on the device; ``None`` clears them.  Serving metadata
        as the tags: ``fit`` leaves them alone and ``save`` does not write them — set them again after ``load``."""
        self.params.set_item_groups(groups)
        return self

    def item_groups(self) -> np.ndarray:
        """The group words last set (u32 [num_items]); raises while the model has none."""
        return self.params.item_groups()

    def recommend_capped(self, interactions_or_histories, k: int, cap: int = 1, pool=None, exclude_history: bool = True, any_of=None,
                         none_of=None, exact: bool = True):
        """``recommend`` under the hard slate rule "at most ``cap`` items of one group" (``set_item_groups``): (items [U, k] u32,
        scores [U, k] f32, complete [U] bool) — each row is ``recommend``'s order walked from the top, an entry kept while fewer
        than cap kept entries share its group, k kept in all; exact over the whole catalogue, not a filter of some larger k.  The
        device applies the rule to each row's best ``pool`` (default min(1 024, max(64, 4 k))); with ``exact=True`` the rows that
        pool did not settle are finished through ``recommend_top``, and complete is all True.  ``exact=False``: the device's
        rows as they are, a short row with complete False being a prefix of the exact answer.  Eligibility is ``recommend``'s."""
        up, it = self._csr(interactions_or_histories)
        return self.params.recommend_capped(up, it, k, cap=cap, pool=pool, include_history=not exclude_history, any_of=any_of,
                                            none_of=none_of, exact=exact)

    def recommend_capped_reps(self, reps, k: int, cap: int = 1, pool=None, exclude=None, any_of=None, none_of=None, exact: bool = True):
        """``recommend_capped`` from representations [U, embedding_dim]; ``exclude``: None or one sequence of item ids per user."""
        return self.params.recommend_capped_reps(reps, k, cap=cap, pool=pool, exclude=exclude, any_of=any_of, none_of=none_of, exact=exact)

    def recommend_top(self, interactions_or_histories, n, exclude_history: bool = True, any_of=None, none_of=None, max_results=None,
                      order: str = "score"):
        """``recommend`` with a budget in place of k: each user's exact best ``n`` eligible items (a scalar or one per user, any
        size — no cap of 1 024), on the device — an ``engine.Above`` whose ``cuts`` holds each row's n-th score (-inf where the row
        is everything eligible, +inf for n = 0).  Same order as every call: for n <= 1 024 a row is ``recommend(k=n)``'s without
        padding."""
        up, it = self._csr(interactions_or_histories)
        return self.params.recommend_top(up, it, n, include_history=not exclude_history, any_of=any_of, none_of=none_of,
                                         max_results=max_results, order=order)

    def nth_score(self, interactions_or_histories, n, exclude_history: bool = True, any_of=None, none_of=None):
        """``(cuts, counts)`` of ``recommend_top(...)`` without writing any pair: the select alone."""
        up, it = self._csr(interactions_or_histories)
        return self.params.nth_score(up, it, n, include_history=not exclude_history, any_of=any_of, none_of=none_of)

    def recommend_top_reps(self, reps, n, exclude=None, any_of=None, none_of=None, max_results=None, order: str = "score"):
        """``recommend_top`` from representations [U, embedding_dim]; ``exclude``: None or one sequence of item ids per user."""
        return self.params.recommend_top_reps(reps, n, exclude=exclude, any_of=any_of, none_of=none_of, max_results=max_results, order=order)

    def nth_score_reps(self, reps, n, exclude=None, any_of=None, none_of=None):
        """``(cuts, counts)`` of ``recommend_top_reps(...)`` without writing any pair."""
        return self.params.nth_score_reps(reps, n, exclude=exclude, any_of=any_of, none_of=none_of)

    def audience_top(self, interactions_or_histories, items, n, exclude_history: bool = True, max_results=None, order: str = "score"):
        """``audience`` with a budget in place of k: for each query item the exact best ``n`` users (a scalar or one per query, any
        size) — an ``engine.Above`` over the queries with ``cuts``, user indices.  For live sessions: ``sessions(...).audience_top``."""
        up, it = self._csr(interactions_or_histories)
        return self.params.audience_top(up, it, items, n, include_history=not exclude_history, max_results=max_results, order=order)

    def nth_audience_score(self, interactions_or_histories, items, n, exclude_history: bool = True):
        """``(cuts, counts)`` of ``audience_top(...)`` without writing any pair."""
        up, it = self._csr(interactions_or_histories)
        return self.params.nth_audience_score(up, it, items, n, include_history=not exclude_history)

    def audience_top_reps(self, reps, items, n, exclude=None, max_results=None, order: str = "score"):
        """``audience_top`` over representation rows [S, embedding_dim]; ``exclude``: None or one sequence of row indices per query."""
        return self.params.audience_top_reps(reps, items, n, exclude=exclude, max_results=max_results, order=order)

    def nth_audience_score_reps(self, reps, items, n, exclude=None):
        """``(cuts, counts)`` of ``audience_top_reps(...)`` without writing any pair."""
        return self.params.nth_audience_score_reps(reps, items, n, exclude=exclude)

    def user_representations(self, histories) -> np.ndarray:
        """``user_representation`` of many histories in one device pass: [U, embedding_dim] f32, row u for history u."""
        return self.params.user_representations(*self._csr(histories))

    def score_candidates(self, histories, candidates):
        """``predict`` for many users in one device pass: ``candidates[u]`` are the item ids to score for history u (any
        order, duplicates allowed, may be empty).  One f32 array per user, in candidate order; nothing is masked."""
        up, it = self._csr(histories)
        cp, ci = self._csr(candidates)
        return self.params.score_candidates(up, it, cp, ci)

    def rerank(self, histories, candidates, k=None):
        """Each user's candidates ordered by the model: a list of (items u32, scores f32) per user, score descending, ties to
        the lower item id, duplicates removed, cut to the first ``k`` if given.  The scores come from ``score_candidates`` on
        the device; the per-user sort (``np.lexsort``) is host work."""
        cands = [np.asarray(c, dtype=np.uint32).ravel() for c in candidates]
        out = []
        for c, s in zip(cands, self.score_candidates(histories, cands)):
            ids, first = np.unique(c, return_index=True)
            sc = s[first]
            order = np.lexsort((ids, -sc))[:k]
            out.append((ids[order], sc[order]))
        return out

    def similar_items(self, query_items, k: int, metric: str = "cosine", include_self: bool = False, exclude=None, any_of=None,
                      none_of=None):
        """The k items most like each query item, on the device: (items [Q, k] u32, scores [Q, k] f32), by the cosine of the
        item embeddings (``metric="dot"``: their dot product), score descending, ties to the lower item id.  The query is left
        out of its own row unless ``include_self``; ``exclude``: None or one sequence of item ids per query; a row with fewer
        than k eligible items is padded with (0xFFFFFFFF, -inf).  ``any_of`` / ``none_of``: ``recommend``'s tag filter with one
        mask pair per query."""
        return self.params.similar_items(query_items, k, metric=metric, include_self=include_self, exclude=exclude, any_of=any_of,
                                         none_of=none_of)

    def recommend_diverse(self, interactions_or_histories, k: int, pool=None, trade_off: float = 0.5, metric: str = "cosine",
                          exclude_history: bool = True, any_of=None, none_of=None):
        """``recommend`` without the near-duplicates, on the device: from each user's ``pool`` best items, k are picked greedily by
        maximal marginal relevance — ``trade_off`` * score - (1 - ``trade_off``) * (the largest similarity to an item already
        picked), similarity as ``similar_items`` measures it; the first pick is the best item.  (items [U, k] u32 in pick order,
        scores [U, k] f32, ``recommend``'s bits.)  ``pool=None``: min(4 k, the largest pool the device holds for this embedding
        width, ``params.diverse_max_pool()``); ``trade_off=1`` is ``recommend(k)``.  ``any_of`` / ``none_of``: ``recommend``'s tag
        filter; the pool then holds eligible items only."""
        up, it = self._csr(interactions_or_histories)
        if pool is None:
            pool = min(4 * int(k), self.params.diverse_max_pool())
        return self.params.recommend_diverse(up, it, k, pool, trade_off=trade_off, metric=metric, include_history=not exclude_history,
                                             any_of=any_of, none_of=none_of)

    def item_set(self, item_ids):
        """A long-lived item set (a category, a territory, what is in stock) kept on the device: ``item_ids`` in any order,
        duplicates allowed.  The returned ``ItemSetView`` offers ``recommend``, ``recommend_sampled``, ``log_partition``,
        ``recommend_above`` / ``count_above``, ``recommend_top`` / ``nth_score``, ``recommend_capped`` and ``recommend_diverse``
        (and their ``*_reps`` forms) under this model's names and keywords, each restricted to the set — bit for bit what the
        model's call returns with every other item excluded, at the cost of scanning the set's rows only — together with tag
        filters, and ``on(store)`` for a session store.  Call its ``refresh()`` after ``fit`` or ``load``."""
        return ItemSetView(self, self.params.item_set(item_ids))

    def sessions(self, capacity: int, remember: int = 0):
        """A session store of ``capacity`` slots on the device (``engine.Sessions``): each slot holds one user's recurrent state,
        ``append`` advances it by one cell step per item instead of re-running the whole history, and ``recommend`` /
        ``score_candidates`` read the states in place.  Exact: a slot's representation has the bits of ``user_representation``
        of what was appended to it, up to max_sequence_length items; beyond that a session does not truncate.  ``remember`` > 0:
        every slot also remembers the last ``remember`` items appended to it, on the device, and ``recommend`` /
        ``recommend_diverse`` of the store exclude them as ``recommend`` excludes the history."""
        return self.params.sessions(capacity, remember)

    def rollout(self, histories, steps: int, mode: str = "greedy", temperature: float = 1.0, seed: int = 0, streams=None,
                exclude_history: bool = True, any_of=None, none_of=None, allow_repeats: bool = False, log_prob: bool = False,
                final_state: bool = False):
        """Each history's next ``steps`` items, each chosen given the ones before it, picked and fed back on the device
        (``engine.Rollout``; ``engine.Sessions.rollout`` is the call, and its docstring the contract): defined as a temporary session
        store, ``append`` of each history's last max_sequence_length items and ``store.rollout`` — ``mode="greedy"`` the top-1 per
        step, ``mode="sample"`` one draw of ``recommend_sampled`` per step at seed + step."""
        return self.params.rollout(histories, steps, mode=mode, temperature=temperature, seed=seed, streams=streams,
                                   exclude_history=exclude_history, any_of=any_of, none_of=none_of, allow_repeats=allow_repeats,
                                   log_prob=log_prob, final_state=final_state)

    def beam_search(self, histories, steps: int, width: int = 4, temperature: float = 1.0, exclude_history: bool = True, any_of=None,
                    none_of=None, allow_repeats: bool = False, partitions: bool = False):
        """The ``width`` most likely next-``steps`` continuations of each history, searched on the device (``engine.Beams``;
        ``engine.Sessions.beam_search`` is the call, and its docstring the contract): defined as a temporary session store,
        ``append`` of each history's last max_sequence_length items and ``store.beam_search``."""
        return self.params.beam_search(histories, steps, width=width, temperature=temperature, exclude_history=exclude_history,
                                       any_of=any_of, none_of=none_of, allow_repeats=allow_repeats, partitions=partitions)

    def load_sessions(self, path, capacity=None, remember=None, replay: bool = False):
        """A session store restored from a file written by ``store.save(path)`` (``persistence.load_sessions``).  With
        ``replay=True`` only the remembered items are restored and every state is recomputed from them on the device under this
        model's parameters (``engine.Sessions.replay``): the route after a retrain."""
        return self.params.load_sessions(path, capacity=capacity, remember=remember, replay=replay)

    def rank_targets(self, histories, targets, mask_history: bool = True, any_of=None, none_of=None, item_set=None):
        """Exact catalogue ranks of each user's targets from one device scan (``evaluation.rank_targets``): one uint32 array
        per user, in target order."""
        from .evaluation import rank_targets

        return rank_targets(self, histories, targets, mask_history=mask_history, any_of=any_of, none_of=none_of, item_set=item_set)

    def sequence_ranks(self, test, mask_history: bool = True, last=None):
        """Exact next-item rank at every position of every test sequence from one forward pass per sequence
        (``evaluation.sequence_ranks``): one uint32 array per user, positions ascending."""
        from .evaluation import sequence_ranks

        return sequence_ranks(self, test, mask_history=mask_history, last=last)

    def sequence_log_probs(self, test, temperature: float = 1.0, mask_history: bool = True, last=None):
        """The exact log-probability of the next item under softmax(score / temperature) at every position of every test
        sequence (``evaluation.sequence_log_probs``): one float64 array per user, -inf where the policy masks the target."""
        from .evaluation import sequence_log_probs

        return sequence_log_probs(self, test, temperature=temperature, mask_history=mask_history, last=last)

    def calibrate_temperature(self, validation, bounds=(0.01, 100.0), evaluations: int = 24, mask_history: bool = True, last=1):
        """The maximum-likelihood temperature on held-out next items (``evaluation.calibrate_temperature``)."""
        from .evaluation import calibrate_temperature

        return calibrate_temperature(self, validation, bounds=bounds, evaluations=evaluations, mask_history=mask_history, last=last)


class ItemSetView:
    """``model.item_set(item_ids)``: an ``engine.ItemSet`` under the model wrappers' conventions — histories as a
    CompressedInteractions or a list of item-id sequences, ``exclude_history`` where the engine says ``include_history``.  The
    ``*_reps`` forms, ``size``, ``items``, ``refresh()``, ``close()`` and ``on(store)`` are the engine object's own."""

    def __init__(self, model: "_ImplicitSequenceModel", item_set):
        self.model, self.set = model, item_set

    def __getattr__(self, name):  # size, items, refresh, close, on and the *_reps methods
        return getattr(self.set, name)

    def __len__(self) -> int:
        return self.set.size

    def recommend(self, interactions_or_histories, k: int, exclude_history: bool = True, any_of=None, none_of=None):
        up, it = self.model._csr(interactions_or_histories)
        return self.set.recommend(up, it, k, include_history=not exclude_history, any_of=any_of, none_of=none_of)

    def recommend_sampled(self, interactions_or_histories, k: int, temperature: float = 1.0, seed: int = 0, streams=None,
                          exclude_history: bool = True, any_of=None, none_of=None, log_prob: bool = False):
        up, it = self.model._csr(interactions_or_histories)
        return self.set.recommend_sampled(up, it, k, temperature=temperature, seed=seed, streams=streams,
                                          include_history=not exclude_history, any_of=any_of, none_of=none_of, log_prob=log_prob)

    def log_partition(self, interactions_or_histories, temperature: float = 1.0, exclude_history: bool = True, any_of=None, none_of=None):
        up, it = self.model._csr(interactions_or_histories)
        return self.set.log_partition(up, it, temperature, include_history=not exclude_history, any_of=any_of, none_of=none_of)

    def recommend_above(self, interactions_or_histories, threshold, exclude_history: bool = True, any_of=None, none_of=None,
                        max_results=None, order: str = "score"):
        up, it = self.model._csr(interactions_or_histories)
        return self.set.recommend_above(up, it, threshold, include_history=not exclude_history, any_of=any_of, none_of=none_of,
                                        max_results=max_results, order=order)

    def rank_targets(self, histories, targets, mask_history: bool = True, any_of=None, none_of=None):
        """``model.rank_targets`` within the set (``evaluation.rank_targets(..., item_set=...)``): one uint32 array per user."""
        from .evaluation import rank_targets

        return rank_targets(self.model, histories, targets, mask_history=mask_history, any_of=any_of, none_of=none_of, item_set=self.set)

    def count_above(self, interactions_or_histories, threshold, exclude_history: bool = True, any_of=None, none_of=None):
        up, it = self.model._csr(interactions_or_histories)
        return self.set.count_above(up, it, threshold, include_history=not exclude_history, any_of=any_of, none_of=none_of)

    def recommend_top(self, interactions_or_histories, n, exclude_history: bool = True, any_of=None, none_of=None, max_results=None,
                      order: str = "score"):
        up, it = self.model._csr(interactions_or_histories)
        return self.set.recommend_top(up, it, n, include_history=not exclude_history, any_of=any_of, none_of=none_of,
                                      max_results=max_results, order=order)

    def nth_score(self, interactions_or_histories, n, exclude_history: bool = True, any_of=None, none_of=None):
        up, it = self.model._csr(interactions_or_histories)
        return self.set.nth_score(up, it, n, include_history=not exclude_history, any_of=any_of, none_of=none_of)

    def recommend_capped(self, interactions_or_histories, k: int, cap: int = 1, pool=None, exclude_history: bool = True, any_of=None,
                         none_of=None, exact: bool = True):
        up, it = self.model._csr(interactions_or_histories)
        return self.set.recommend_capped(up, it, k, cap=cap, pool=pool, include_history=not exclude_history, any_of=any_of,
                                         none_of=none_of, exact=exact)

    def recommend_diverse(self, interactions_or_histories, k: int, pool=None, trade_off: float = 0.5, metric: str = "cosine",
                          exclude_history: bool = True, any_of=None, none_of=None):
        up, it = self.model._csr(interactions_or_histories)
        if pool is None:
            pool = min(4 * int(k), self.model.params.diverse_max_pool())
        return self.set.recommend_diverse(up, it, k, pool, trade_off=trade_off, metric=metric, include_history=not exclude_history,
                                          any_of=any_of, none_of=none_of)

    def rollout(self, histories, steps: int, mode: str = "greedy", temperature: float = 1.0, seed: int = 0, streams=None,
                exclude_history: bool = True, any_of=None, none_of=None, allow_repeats: bool = False, log_prob: bool = False,
                final_state: bool = False):
        """The model's ``rollout`` within the set (``engine.ItemSet.rollout``)."""
        return self.set.rollout(histories, steps, mode=mode, temperature=temperature, seed=seed, streams=streams,
                                exclude_history=exclude_history, any_of=any_of, none_of=none_of, allow_repeats=allow_repeats,
                                log_prob=log_prob, final_state=final_state)

    def beam_search(self, histories, steps: int, width: int = 4, temperature: float = 1.0, exclude_history: bool = True, any_of=None,
                    none_of=None, allow_repeats: bool = False, partitions: bool = False):
        """The model's ``beam_search`` within the set (``engine.ItemSet.beam_search``)."""
        return self.set.beam_search(histories, steps, width=width, temperature=temperature, exclude_history=exclude_history,
                                    any_of=any_of, none_of=none_of, allow_repeats=allow_repeats, partitions=partitions)


class ImplicitLSTMModel(_ImplicitSequenceModel):
    """An LSTM-based sequence model for implicit feedback (lstm.rs:386-416)."""
