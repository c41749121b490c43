"""The expectation of sbr_recommend_diverse, from the contract (include/sbr_hip.h) alone:

    pool       recommend's row at k = pool: recommend_expect.topk_expectation / oracle_recommend
    sim(a, j)  similar_expect.SimilarExpectation(E, metric).scores(c_a)[c_j]: the oracle's chain with numpy-f32 r, qhat and final
               multiply — similar_items' s(q = a, i = c_j), the picked item as the query
    selection  numpy float32, one operation per rounding: mu = 1 - lam; m = sim of the first pick, then max(m, sim); v = (lam * s) -
               (mu * m); np.argmax over the unpicked positions (the first maximum: ties to the lower position; -0.0 == +0.0)

It shares no code with the product."""
from __future__ import annotations

import numpy as np

from recommend_expect import NO_ITEM, oracle_recommend, topk_expectation
from similar_expect import SimilarExpectation


def clustered_case(d, seed, items=600, clusters=12, users=40):
    """The clustered table of the diversity test: item i in cluster i % clusters, E[i] = centroid + (0.1 / sqrt(d)) randn, zero bias;
    `users` representations centroid[a] + 0.7 centroid[b] + (0.3 / sqrt(d)) randn with b != a: a user likes two clusters, one of them
    more.  -> (E, bias, reps)"""
    rs = np.random.RandomState(seed)
    cent = rs.randn(clusters, d) / np.sqrt(d)
    E = (cent[np.arange(items) % clusters] + (0.1 / np.sqrt(d)) * rs.randn(items, d)).astype(np.float32)
    a = rs.randint(0, clusters, users)
    b = (a + 1 + rs.randint(0, clusters - 1, users)) % clusters
    reps = (cent[a] + 0.7 * cent[b] + (0.3 / np.sqrt(d)) * rs.randn(users, d)).astype(np.float32)
    return E, np.zeros(items, np.float32), reps


class DiverseExpectation:
    """The selection over one item table under one metric; similarities are kept per picked item."""

    def __init__(self, E, metric="cosine"):
        self.sim = SimilarExpectation(E, metric)

    def select(self, pool_items, pool_scores, k, trade_off):
        """One user: the pool's row (padded) -> (items [k] u32, scores [k] f32) in pick order, padded."""
        c = np.asarray(pool_items, dtype=np.uint32)
        s = np.asarray(pool_scores, dtype=np.float32)
        n = int(np.count_nonzero(c != NO_ITEM))
        assert np.all(c[:n] != NO_ITEM)  # the real entries are a prefix
        c, s = c[:n], s[:n]
        lam = np.float32(trade_off)
        mu = np.float32(1.0) - lam
        items = np.full(k, NO_ITEM, dtype=np.uint32)
        scores = np.full(k, -np.inf, dtype=np.float32)
        if n == 0:
            return items, scores
        picked = [0]
        free = np.ones(n, dtype=bool)
        free[0] = False
        m = None
        ls = (lam * s).astype(np.float32)
        for _ in range(1, min(k, n)):
            sim = self.sim.scores(c[picked[-1]])[c].astype(np.float32)
            m = sim if m is None else np.maximum(m, sim)
            v = (ls - (mu * m).astype(np.float32)).astype(np.float32)
            pos = np.flatnonzero(free)
            j = int(pos[np.argmax(v[pos])])
            picked.append(j)
            free[j] = False
        items[: len(picked)] = c[picked]
        scores[: len(picked)] = s[picked]
        return items, scores

    def rows(self, pool_rows, k, trade_off):
        """pool_rows: (items [U, pool], scores [U, pool]) -> (items [U, k], scores [U, k])"""
        out = [self.select(pi, ps, k, trade_off) for pi, ps in zip(*pool_rows)]
        return (np.array([r[0] for r in out], dtype=np.uint32).reshape(-1, k),
                np.array([r[1] for r in out], dtype=np.float32).reshape(-1, k))


def pool_from_histories(o, num_items, ptr, item_ids, pool, include_history=False):
    return oracle_recommend(o, num_items, ptr, item_ids, pool, include_history=include_history)


def pool_from_reps(o, num_items, reps, pool, exclude=None):
    all_items = np.arange(num_items, dtype=np.uint32)
    rows = [topk_expectation(o.predict(r, all_items), () if exclude is None else [int(x) for x in exclude[u]], pool)
            for u, r in enumerate(np.asarray(reps, dtype=np.float32))]
    return (np.array([r[0] for r in rows], dtype=np.uint32).reshape(-1, pool),
            np.array([r[1] for r in rows], dtype=np.float32).reshape(-1, pool))
