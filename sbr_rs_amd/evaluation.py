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


def rank_targets(model, histories, targets, mask_history: bool = True):
    """Exact rank of every target of every user among the whole catalogue, on the device in one scan (``sbr_rank_targets``).

    ``histories`` and ``targets`` are one item-id sequence per user (a user may have no targets, or an empty history: the
    state of item 0, as ``recommend``).  rank(u, t) = #{items i : m(u, i) >= m(u, t)} with m = the score of ``predict``, or
    f32::MIN for every item of the WHOLE history while ``mask_history`` — the rule of evaluation.rs:30-41 applied to each
    target on its own: the target counts itself, ties count against it, a target inside the masked history has rank
    num_items, duplicate targets get equal ranks.  -> one uint32 array per user, in target order."""
    params = getattr(model, "params", model)
    if len(histories) != len(targets):
        raise ValueError("one target sequence per history")
    up, it = _csr(histories)
    tp, ti = _csr(targets)
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


def ranking_metrics(model, test: CompressedInteractions, ks=(10, 100), holdout: int = 1, mask_history: bool = True):
    """precision@k, recall@k, hit-rate@k and NDCG@k at every k of ``ks``, MRR and mean rank over a hold-out of the last
    ``holdout`` items of each test sequence (:func:`holdout_split`), from exact catalogue ranks computed in one device scan
    whose cost does not depend on k (:func:`rank_targets`).  Users with fewer than ``holdout + 1`` items are skipped.
    -> the dict of :func:`ranking_metrics_from_ranks`; its ``users`` index the test set's users."""
    users, histories, targets = holdout_split(test, holdout)
    ranks = rank_targets(model, histories, targets, mask_history=mask_history) if len(users) else []
    out = ranking_metrics_from_ranks(ranks, ks)
    out["users"] = users[out["users"]] if len(users) else users
    return out
