"""Evaluation — mirror of ``sbr::evaluation`` (/root/reference/src/evaluation.rs), plus what the reference lacks: exact ranks
of several held-out items per user from one scan of the catalogue (``rank_targets``) and the ranking metrics at k that follow
from them (``ranking_metrics``)."""
from __future__ import annotations

import numpy as np

from .data import CompressedInteractions


def mrr_score(model, test: CompressedInteractions) -> float:
    """MRR of the last item of each test sequence, all but the last item being the inputs
    (evaluation.rs:12-48).  Runs on the device through ``sbr_mrr_score``."""
    mrr, _ranks = model.params.mrr_score(test.user_pointers, test.item_ids)
    return mrr


def mrr_ranks(model, test: CompressedInteractions):
    """As :func:`mrr_score` but also returns the integer ranks (one per user with >= 2 items)."""
    return model.params.mrr_score(test.user_pointers, test.item_ids)


def _csr(seqs, dtype=np.uint32):
    seqs = [np.asarray(s, dtype=dtype).ravel() for s in seqs]
    ptr = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if seqs:
        ptr[1:] = np.cumsum([s.size for s in seqs])
    items = np.concatenate(seqs) if seqs else np.zeros(0, dtype=dtype)
    return ptr, np.ascontiguousarray(items, dtype=dtype)


def rank_targets(model, histories, targets, mask_history: bool = True, any_of=None, none_of=None, item_set=None):
    """Exact rank of every target of every user among the whole catalogue, on the device in one scan (``sbr_rank_targets``).

    ``histories`` and ``targets`` are one item-id sequence per user (a user may have no targets, or an empty history: the
    state of item 0, as ``recommend``).  rank(u, t) = #{items i : m(u, i) >= m(u, t)} with m = the score of ``predict``, or
    f32::MIN for every item of the WHOLE history while ``mask_history`` — the rule of evaluation.rs:30-41 applied to each
    target on its own: the target counts itself, ties count against it, a target inside the masked history has rank
    num_items, duplicate targets get equal ranks.  -> one uint32 array per user, in target order.

    ``any_of`` / ``none_of`` (``recommend``'s tag masks: a scalar or one per user) and ``item_set`` (an ``ItemSet`` of the model)
    state the serving policy the ranks are taken under: every item the masks forbid and every item outside the set is masked
    to f32::MIN as the history is, so a target the policy can never show has rank num_items (:func:`eligible_targets`)."""
    params = getattr(model, "params", model)
    if len(histories) != len(targets):
        raise ValueError("one target sequence per history")
    up, it = _csr(histories)
    tp, ti = _csr(targets)
    if item_set is not None:
        ranks = item_set.rank_targets(up, it, tp, ti, include_history=not mask_history, any_of=any_of, none_of=none_of)
    elif any_of is not None or none_of is not None:
        ranks = params.rank_targets(up, it, tp, ti, include_history=not mask_history, any_of=any_of, none_of=none_of)
    else:
        ranks = params.rank_targets(up, it, tp, ti, include_history=not mask_history)
    tp = tp.astype(np.int64)
    return [ranks[tp[u]: tp[u + 1]].copy() for u in range(len(targets))]


def ranking_metrics_from_ranks(ranks_per_user, ks=(10, 100)):
    """precision / recall / hit rate / NDCG at every k of ``ks``, MRR (1 / best rank) and mean rank from the catalogue ranks
    of each user's DISTINCT relevant items (r of them; ranks alone cannot tell a duplicate from a tie).  Pure numpy, float64.

        hits_k = #{t : rank_t <= k}    precision = hits_k / k    recall = hits_k / r    hit_rate = hits_k > 0
        ndcg = sum_{rank_t <= k} 1 / log2(1 + rank_t)  /  sum_{j = 1..min(r, k)} 1 / log2(1 + j)

    Users without ranks are left out of the means.  -> dict with ``ks``, ``num_users_ranked``, ``users`` (indices of the
    users that went in), the means ``precision`` / ``recall`` / ``hit_rate`` / ``ndcg`` ({k: float}), ``mrr``,
    ``mean_rank`` (NaN without a ranked user, as mrr_score's 0 / 0) and ``per_user`` with the same keys holding one value per
    ranked user."""
    ks = tuple(int(k) for k in ks)
    if any(k < 1 for k in ks):
        raise ValueError("every k must be >= 1")
    rows = [np.asarray(r, dtype=np.int64).ravel() for r in ranks_per_user]
    if any(r.size and r.min() < 1 for r in rows):
        raise ValueError("ranks start at 1")
    users = np.array([u for u, r in enumerate(rows) if r.size], dtype=np.int64)
    n = users.size
    kmax = max(ks) if ks else 0
    ideal = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(1.0 + np.arange(1, kmax + 1, dtype=np.float64)))])
    per = {name: {k: np.zeros(n, dtype=np.float64) for k in ks} for name in ("precision", "recall", "hit_rate", "ndcg")}
    per["mrr"] = np.zeros(n, dtype=np.float64)
    per["mean_rank"] = np.zeros(n, dtype=np.float64)
    for j, u in enumerate(users):
        r = np.sort(rows[u])
        # summed in rank order like `ideal`: term by term no larger than it (the j-th best target has rank >= j), so ndcg <= 1 exactly
        dcg = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(1.0 + r.astype(np.float64)))])
        per["mrr"][j] = 1.0 / float(r[0])
        per["mean_rank"][j] = float(np.mean(r.astype(np.float64)))
        for k in ks:
            hits = int(np.searchsorted(r, k, side="right"))
            per["precision"][k][j] = hits / k
            per["recall"][k][j] = hits / r.size
            per["hit_rate"][k][j] = 1.0 if hits else 0.0
            per["ndcg"][k][j] = dcg[hits] / ideal[min(r.size, k)]
    mean = (lambda a: float(np.mean(a))) if n else (lambda a: float("nan"))
    out = {"ks": ks, "num_users_ranked": int(n), "users": users, "per_user": per}
    for name in ("precision", "recall", "hit_rate", "ndcg"):
        out[name] = {k: mean(per[name][k]) for k in ks}
    out["mrr"] = mean(per["mrr"])
    out["mean_rank"] = mean(per["mean_rank"])
    return out


def holdout_split(test: CompressedInteractions, holdout: int = 1):
    """The evaluation split of :func:`ranking_metrics`: for every user with at least ``holdout + 1`` items the last
    ``holdout`` items are the targets — de-duplicated, first occurrence kept — and the rest the history (at ``holdout`` = 1
    the reference's ``>= 2``, evaluation.rs:20-25).  -> (users, histories, targets): the users' indices and one array each."""
    holdout = int(holdout)
    if holdout < 1:
        raise ValueError("holdout must be >= 1")
    ptr = np.asarray(test.user_pointers, dtype=np.int64)
    users, histories, targets = [], [], []
    for u in range(len(ptr) - 1):
        seq = test.item_ids[ptr[u]: ptr[u + 1]]
        if seq.size < holdout + 1:
            continue
        held = seq[seq.size - holdout:]
        _, first = np.unique(held, return_index=True)
        users.append(u)
        histories.append(seq[: seq.size - holdout])
        targets.append(held[np.sort(first)])
    return np.array(users, dtype=np.int64), histories, targets


def eligible_targets(model, histories, targets, mask_history: bool = True, any_of=None, none_of=None, item_set=None):
    """Whether the serving policy could show each target at all — the host statement of "not in M" for :func:`rank_targets`:
    the target is in the item set (if one is given), its tag word ``item_tags()[t]`` is allowed by the user's masks
    ((tag & none_of) == 0 and (any_of == 0 or (tag & any_of) != 0)), and while ``mask_history`` it is not in the user's history.
    Pure numpy over ``model.item_tags()`` and ``item_set.items``.  -> one bool array per user, in target order."""
    params = getattr(model, "params", model)
    if len(histories) != len(targets):
        raise ValueError("one target sequence per history")
    nu = len(targets)

    def per_user(mask):
        if mask is None:
            return np.zeros(nu, dtype=np.uint32)
        a = np.asarray(mask)
        if a.ndim == 0:
            return np.full(nu, int(a) & 0xFFFFFFFF, dtype=np.uint32)
        a = a.ravel().astype(np.uint32)
        if a.size != nu:
            raise ValueError("one mask per user")
        return a

    filtered = any_of is not None or none_of is not None
    anyv, nonev = per_user(any_of), per_user(none_of)
    tags = np.asarray(params.item_tags(), dtype=np.uint32) if filtered else None
    members = None if item_set is None else np.asarray(item_set.items, dtype=np.uint32)
    out = []
    for u in range(nu):
        t = np.asarray(targets[u], dtype=np.uint32).ravel()
        ok = np.ones(t.size, dtype=bool)
        if members is not None:
            ok &= np.isin(t, members)
        if filtered:
            w = tags[t]
            ok &= (w & nonev[u]) == 0
            if anyv[u]:
                ok &= (w & anyv[u]) != 0
        if mask_history:
            ok &= ~np.isin(t, np.asarray(histories[u], dtype=np.uint32).ravel())
        out.append(ok)
    return out


def apply_ineligible(ranks_per_user, eligible_per_user, ineligible: str = "miss"):
    """The ``ineligible`` rule of :func:`ranking_metrics` on rank rows: ``"miss"`` keeps every rank (a target the policy can
    never show stays at rank num_items: a miss at every k), ``"skip"`` drops the targets that are not eligible.
    -> (rank rows, number of targets dropped)."""
    if ineligible not in ("miss", "skip"):
        raise ValueError('ineligible: "miss" or "skip"')
    if len(ranks_per_user) != len(eligible_per_user):
        raise ValueError("one eligibility row per rank row")
    if ineligible == "miss":
        return [np.asarray(r) for r in ranks_per_user], 0
    rows, skipped = [], 0
    for r, e in zip(ranks_per_user, eligible_per_user):
        r, e = np.asarray(r), np.asarray(e, dtype=bool)
        if r.shape != e.shape:
            raise ValueError("one eligibility flag per rank")
        rows.append(r[e])
        skipped += int(r.size - int(e.sum()))
    return rows, skipped


def ranking_metrics(model, test: CompressedInteractions, ks=(10, 100), holdout: int = 1, mask_history: bool = True, any_of=None,
                    none_of=None, item_set=None, ineligible: str = "miss"):
    """precision@k, recall@k, hit-rate@k and NDCG@k at every k of ``ks``, MRR and mean rank over a hold-out of the last
    ``holdout`` items of each test sequence (:func:`holdout_split`), from exact catalogue ranks computed in one device scan
    whose cost does not depend on k (:func:`rank_targets`).  Users with fewer than ``holdout + 1`` items are skipped.
    -> the dict of :func:`ranking_metrics_from_ranks`; its ``users`` index the test set's users.

    ``any_of`` / ``none_of`` (a scalar, or one mask per user of the TEST SET) and ``item_set`` evaluate under a serving policy
    (:func:`rank_targets`).  ``ineligible`` says what a target the policy can never show (:func:`eligible_targets`) counts as:
    ``"miss"`` keeps it at rank num_items — the reference's rule for a target in its own history — and ``"skip"`` leaves it out of
    every mean (a user left without targets is not ranked); ``targets_skipped`` reports how many were left out."""
    if ineligible not in ("miss", "skip"):
        raise ValueError('ineligible: "miss" or "skip"')
    users, histories, targets = holdout_split(test, holdout)

    def of_users(mask):  # a per-user mask of the test set follows the users the split kept
        return mask if mask is None or np.ndim(mask) == 0 else np.asarray(mask).ravel()[users]

    any_u, none_u = of_users(any_of), of_users(none_of)
    policy = dict(mask_history=mask_history, any_of=any_u, none_of=none_u, item_set=item_set)
    ranks = rank_targets(model, histories, targets, **policy) if len(users) else []
    skipped = 0
    if ineligible == "skip" and len(users):
        ranks, skipped = apply_ineligible(ranks, eligible_targets(model, histories, targets, **policy), "skip")
    out = ranking_metrics_from_ranks(ranks, ks)
    out["targets_skipped"] = skipped
    out["users"] = users[out["users"]] if len(users) else users
    return out


def sequence_ranks(model, test: CompressedInteractions, mask_history: bool = True, last=None):
    """Exact next-item rank at EVERY position of every test sequence, from one forward pass per sequence and one scan row per
    position (``sbr_sequence_ranks``) — the teacher-forced evaluation of a sequence recommender.

    With T = max_sequence_length, W = min(n, T + 1) and w the last W items of a user, position p = 1 .. W - 1 ranks w[p]
    against the state after w[:p]; while ``mask_history`` the distinct items of w[:p] are masked to f32::MIN (a target that
    occurs in its own prefix has rank num_items).  Each rank is the number ``rank_targets([w[:p]], [[w[p]]])`` gives; items
    before the window are neither in a state nor in a mask.  ``last`` (None = all) keeps the last ``last`` positions of each
    window: the same numbers at a fraction of the scan.  -> one uint32 array per user, positions ascending (empty for n < 2)."""
    params = getattr(model, "params", model)
    ptr, ranks = params.sequence_ranks(test.user_pointers, test.item_ids, include_history=not mask_history, last=last)
    ptr = ptr.astype(np.int64)
    return [ranks[ptr[u]: ptr[u + 1]].copy() for u in range(len(ptr) - 1)]


def _position_metrics(ranks, ks):
    """mrr, mean_rank, hit_rate[k], ndcg[k] as means over the float64 ``ranks`` (one relevant item per rank); NaN when empty."""
    if ranks.size == 0:
        nan = float("nan")
        return {"mrr": nan, "mean_rank": nan, "hit_rate": {k: nan for k in ks}, "ndcg": {k: nan for k in ks}}
    gain = 1.0 / np.log2(1.0 + ranks)
    return {"mrr": float(np.mean(1.0 / ranks)), "mean_rank": float(np.mean(ranks)),
            "hit_rate": {k: float(np.mean(ranks <= k)) for k in ks},
            "ndcg": {k: float(np.mean(np.where(ranks <= k, gain, 0.0))) for k in ks}}


def sequence_metrics_from_ranks(ranks_per_user, ks=(10, 100), max_sequence_length=None):
    """The metrics of :func:`sequence_metrics` from the per-user rank rows of :func:`sequence_ranks`.  Pure numpy, float64.

    Every position has ONE relevant item, so with r its rank: reciprocal rank 1 / r, hit@k = [r <= k], ndcg@k = 1 / log2(1 + r)
    if r <= k else 0.  -> dict with ``ks``, ``num_positions``, ``num_users_ranked``; ``mrr`` / ``mean_rank`` / ``hit_rate``
    ({k: float}) / ``ndcg`` ({k: float}) as the mean over ALL positions; ``macro`` with the same keys as the mean of the per-user
    means (users without positions left out); ``by_history_length`` with ``count`` (int64) and ``mrr`` / ``mean_rank`` /
    ``hit_rate`` / ``ndcg`` as arrays indexed by the history length p (index 0 unused; up to ``max_sequence_length``, or the
    longest row when that is None), NaN where no position has that history length.  The history length of the j-th entry of a
    row of m entries is taken as p = j + 1 — exact for rows of a full call (``last`` = None) on sequences of at most
    max_sequence_length + 1 items; with ``last`` the caller passes rows whose first entries were cut and should not read
    ``by_history_length``.  Means are NaN when there is no position."""
    ks = tuple(int(k) for k in ks)
    if any(k < 1 for k in ks):
        raise ValueError("every k must be >= 1")
    rows = [np.asarray(r, dtype=np.float64).ravel() for r in ranks_per_user]
    if any(r.size and r.min() < 1 for r in rows):
        raise ValueError("ranks start at 1")
    ranked = [r for r in rows if r.size]
    allr = np.concatenate(ranked) if ranked else np.zeros(0, dtype=np.float64)
    out = {"ks": ks, "num_positions": int(allr.size), "num_users_ranked": len(ranked)}
    out.update(_position_metrics(allr, ks))
    per_user = [_position_metrics(r, ks) for r in ranked]
    mean = (lambda v: float(np.mean(np.asarray(v, dtype=np.float64)))) if ranked else (lambda v: float("nan"))
    out["macro"] = {"mrr": mean([m["mrr"] for m in per_user]), "mean_rank": mean([m["mean_rank"] for m in per_user]),
                    "hit_rate": {k: mean([m["hit_rate"][k] for m in per_user]) for k in ks},
                    "ndcg": {k: mean([m["ndcg"][k] for m in per_user]) for k in ks}}
    longest = max([r.size for r in rows], default=0)
    L = longest if max_sequence_length is None else int(max_sequence_length)
    if L < longest:
        raise ValueError("a row has more positions than max_sequence_length")
    by = {"count": np.zeros(L + 1, dtype=np.int64), "mrr": np.full(L + 1, np.nan), "mean_rank": np.full(L + 1, np.nan),
          "hit_rate": {k: np.full(L + 1, np.nan) for k in ks}, "ndcg": {k: np.full(L + 1, np.nan) for k in ks}}
    for p in range(1, L + 1):
        at = np.array([r[p - 1] for r in rows if r.size >= p], dtype=np.float64)
        by["count"][p] = at.size
        if at.size:
            pm = _position_metrics(at, ks)
            by["mrr"][p], by["mean_rank"][p] = pm["mrr"], pm["mean_rank"]
            for k in ks:
                by["hit_rate"][k][p], by["ndcg"][k][p] = pm["hit_rate"][k], pm["ndcg"][k]
    out["by_history_length"] = by
    return out


def sequence_metrics(model, test: CompressedInteractions, ks=(10, 100), mask_history: bool = True, last=None):
    """MRR, mean rank, hit-rate@k and NDCG@k of next-item prediction at every position of every test sequence
    (:func:`sequence_ranks`): micro (over positions), ``macro`` (mean of per-user means) and ``by_history_length`` — how good
    the model is after 1, 5 or 50 events.  With ``last`` the rows hold each window's last positions only and
    ``by_history_length`` is indexed from the first KEPT position (see :func:`sequence_metrics_from_ranks`).
    -> the dict of :func:`sequence_metrics_from_ranks`."""
    params = getattr(model, "params", model)
    ranks = sequence_ranks(model, test, mask_history=mask_history, last=last)
    hp = getattr(params, "hp", None)
    T = int(hp.max_sequence_length) if hp is not None and hasattr(hp, "max_sequence_length") else None
    return sequence_metrics_from_ranks(ranks, ks, max_sequence_length=T)


def _sequence_log_probs_flat(model, test, temperature, mask_history, last):
    """(ptr int64 [U + 1], log_prob f64 [positions], masked bool [positions]) of one ``sequence_partition`` call: log(w / mass)
    through ``Partition.log_prob`` — the one host statement of the weights — and -inf where the policy masks the target."""
    params = getattr(model, "params", model)
    ptr, part, scores, masked = params.sequence_partition(test.user_pointers, test.item_ids, temperature=temperature,
                                                          include_history=not mask_history, last=last)
    masked = masked.astype(bool)
    lp = part.log_prob(scores[:, None])[:, 0] if scores.size else np.zeros(0, dtype=np.float64)
    return ptr.astype(np.int64), np.where(masked, -np.inf, lp), masked


def sequence_log_probs(model, test: CompressedInteractions, temperature: float = 1.0, mask_history: bool = True, last=None):
    """The exact log-probability of the item that came next, at EVERY position of every test sequence, under the policy
    ``recommend_sampled`` draws from: softmax(score / temperature) over the items the user may see — every item, or while
    ``mask_history`` every item not among the distinct items of the prefix (``sbr_sequence_partition``: one forward pass per
    sequence, two catalogue scans per position, no list of prefixes).

    Windows, positions and ``last`` are :func:`sequence_ranks`'.  Each value is ``log_partition([w[:p]]).log_prob`` of the score
    of w[p]: log(w / mass) over exact integer weights.  A target that occurs in its own masked prefix is never shown by the policy
    and has -inf; so has a target more than 64 / temperature-scaled units below the row's best (its weight is 0).
    -> one float64 array per user, positions ascending (empty for n < 2)."""
    ptr, lp, _ = _sequence_log_probs_flat(model, test, temperature, mask_history, last)
    return [lp[ptr[u]: ptr[u + 1]].copy() for u in range(len(ptr) - 1)]


def sequence_log_likelihood_from_log_probs(log_probs_per_user, max_sequence_length=None):
    """The summary of :func:`sequence_log_likelihood` from the per-user rows of :func:`sequence_log_probs`.  Pure numpy, float64.

    Positions with log-prob -inf — the masked ones: the policy cannot show them, so no temperature could have predicted them —
    are LEFT OUT of every mean and counted in ``masked_positions``.  -> dict with ``positions`` (those in the means),
    ``masked_positions``, ``mean_log_prob`` and ``perplexity`` = exp(-mean) over all counted positions, ``macro`` with
    ``mean_log_prob`` / ``perplexity`` as the mean of the per-user means and ``users`` (users with a counted position), and
    ``by_history_length`` with ``count``, ``masked`` (int64) and ``mean_log_prob`` / ``perplexity`` indexed by the history length p
    (index 0 unused; up to ``max_sequence_length``, or the longest row when that is None; the j-th entry of a row counts as
    p = j + 1, as in :func:`sequence_metrics_from_ranks`).  Means are NaN where nothing is counted."""
    rows = [np.asarray(r, dtype=np.float64).ravel() for r in log_probs_per_user]
    if any(r.size and (np.isnan(r).any() or r.max() > 0.0) for r in rows):
        raise ValueError("log-probabilities are <= 0")
    nan = float("nan")
    kept = [r[~np.isneginf(r)] for r in rows]
    allp = np.concatenate(kept) if kept else np.zeros(0, dtype=np.float64)
    mean = float(np.mean(allp)) if allp.size else nan
    user_means = np.array([np.mean(k) for k in kept if k.size], dtype=np.float64)
    macro = float(np.mean(user_means)) if user_means.size else nan
    out = {"positions": int(allp.size), "masked_positions": int(sum(r.size for r in rows) - allp.size),
           "mean_log_prob": mean, "perplexity": float(np.exp(-mean)),
           "macro": {"mean_log_prob": macro, "perplexity": float(np.exp(-macro)), "users": int(user_means.size)}}
    longest = max([r.size for r in rows], default=0)
    L = longest if max_sequence_length is None else int(max_sequence_length)
    if L < longest:
        raise ValueError("a row has more positions than max_sequence_length")
    by = {"count": np.zeros(L + 1, dtype=np.int64), "masked": np.zeros(L + 1, dtype=np.int64),
          "mean_log_prob": np.full(L + 1, np.nan), "perplexity": np.full(L + 1, np.nan)}
    for p in range(1, L + 1):
        at = np.array([r[p - 1] for r in rows if r.size >= p], dtype=np.float64)
        live = at[~np.isneginf(at)]
        by["count"][p], by["masked"][p] = live.size, at.size - live.size
        if live.size:
            by["mean_log_prob"][p] = np.mean(live)
            by["perplexity"][p] = np.exp(-np.mean(live))
    out["by_history_length"] = by
    return out


def sequence_log_likelihood(model, test: CompressedInteractions, temperature: float = 1.0, mask_history: bool = True, last=None):
    """Mean log-likelihood and perplexity of next-item prediction under softmax(score / temperature) at every position of every
    test sequence (:func:`sequence_log_probs`) — the probabilistic counterpart of :func:`sequence_metrics`: micro, ``macro`` and
    ``by_history_length``.  Masked positions (log-prob -inf) are left out of every mean and counted in ``masked_positions``.
    With ``last`` the rows hold each window's last positions and ``by_history_length`` is indexed from the first KEPT position.
    -> the dict of :func:`sequence_log_likelihood_from_log_probs`."""
    params = getattr(model, "params", model)
    rows = sequence_log_probs(model, test, temperature=temperature, mask_history=mask_history, last=last)
    hp = getattr(params, "hp", None)
    T = int(hp.max_sequence_length) if hp is not None and hasattr(hp, "max_sequence_length") else None
    return sequence_log_likelihood_from_log_probs(rows, max_sequence_length=T)


def golden_section_max(f, lo: float, hi: float, evaluations: int = 24):
    """The maximiser of a unimodal (for one, concave) ``f`` on [lo, hi] by golden-section search with exactly ``evaluations``
    calls of f (>= 2): the bracket shrinks by 0.618 per call after the first two.  Where the two interior values tie — two -inf of
    an extended-valued concave function among them — the LOWER part of the bracket is kept.  -> (x, f(x)), the best point seen."""
    lo, hi, evaluations = float(lo), float(hi), int(evaluations)
    if not lo < hi or evaluations < 2:
        raise ValueError("golden_section_max needs lo < hi and at least two evaluations")
    r = (np.sqrt(5.0) - 1.0) / 2.0
    a, b = lo, hi
    c, d = b - r * (b - a), a + r * (b - a)
    fc, fd = f(c), f(d)
    for _ in range(evaluations - 2):
        if fc >= fd:
            b, d, fd = d, c, fc
            c = b - r * (b - a)
            fc = f(c)
        else:
            a, c, fc = c, d, fd
            d = a + r * (b - a)
            fd = f(d)
    return (c, fc) if fc >= fd else (d, fd)


def calibrate_temperature(model, validation: CompressedInteractions, bounds=(0.01, 100.0), evaluations: int = 24,
                          mask_history: bool = True, last=1):
    """The maximum-likelihood temperature of the policy softmax(score / T) on held-out next items: the T in ``bounds`` with the
    largest mean :func:`sequence_log_probs` over the positions of ``validation`` that the policy does not mask (``last`` = 1:
    each sequence's final item; None: every position).

    With beta = 1 / T the mean log-prob is a linear term minus a mean log-sum-exp, so it is concave in beta, and a golden-section
    search on beta (:func:`golden_section_max`) finds its maximum with ``evaluations`` calls of ``sequence_partition``.  A beta so
    large that some target's weight is 0 has mean -inf; the search then moves towards smaller beta.
    -> (temperature, mean_log_prob)."""
    lo_t, hi_t = float(bounds[0]), float(bounds[1])
    if not 0.0 < lo_t < hi_t or not np.isfinite(hi_t):
        raise ValueError("bounds: 0 < lowest temperature < highest, both finite")

    def mean_log_prob(beta):
        _, lp, masked = _sequence_log_probs_flat(model, validation, 1.0 / beta, mask_history, last)
        live = lp[~masked]
        if live.size == 0:
            raise ValueError("calibrate_temperature: no position of the validation set is priced by the policy")
        return float(np.mean(live))

    beta, best = golden_section_max(mean_log_prob, 1.0 / hi_t, 1.0 / lo_t, evaluations)
    return 1.0 / beta, best
