"""The expectation of sbr_similar_items, from the contract's formulas (include/sbr_hip.h) with the CPU oracle as the chain:

    n2[i]   = chain_dot(E[i], E[i])
    r[i]    = n2[i] > 0 ? 1 / sqrt(n2[i]) : 0
    cosine:   qhat = E[q] * r[q];  s(q, i) = chain_dot(qhat, E[i]) * r[i]
    dot:      s(q, i) = chain_dot(E[q], E[i])

The chain is orc_predict's on an OracleModel with the same item table and an ALL-ZERO bias: predict(x, [i]) = 0.0f + chain_dot(x,
E[i]).  0.0f + chain has the chain's bits except for a chain that ends at -0.0 (0.0f + -0.0f = +0.0f), and a chain from +0.0 ends at
-0.0 only when negative products underflow to -0.0; the tables of the tests that use this helper keep every product far from
underflow (an entry is zero or, with 0.3 * randn and 1e-3 * (i + 1), many orders above 1e-19), so this cannot occur.  r, qhat and the final multiply are numpy
float32 operations (IEEE, correctly rounded); the order and padding are recommend_expect.topk_expectation's."""
from __future__ import annotations

import numpy as np

from helpers import LOSS_HINGE, hparams
from oracle.oracle import OracleModel
from recommend_expect import topk_expectation
from sbr_rs_amd._abi import ModelKind, Param


class SimilarExpectation:
    """Scores of one item table under one metric; the score vector of a query item is computed once and kept."""

    def __init__(self, E, metric="cosine"):
        E = np.ascontiguousarray(E, dtype=np.float32)
        self.E = E
        self.num_items, d = E.shape
        self.o = OracleModel(hparams(self.num_items, 8, d, int(ModelKind.EWMA), LOSS_HINGE))
        self.o.set_param(Param.ITEM_EMBEDDING, E)
        self.o.set_param(Param.ITEM_BIAS, np.zeros(self.num_items, np.float32))
        self.all_items = np.arange(self.num_items, dtype=np.uint32)
        if metric == "cosine":
            n2 = np.array([self.o.predict(E[i], [i])[0] for i in range(self.num_items)], dtype=np.float32)
            self.n2 = n2
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.float32(1.0) / np.sqrt(n2, dtype=np.float32)
            self.r = np.where(n2 > 0, r, np.float32(0.0)).astype(np.float32)
        elif metric == "dot":
            self.r = np.ones(self.num_items, np.float32)
        else:
            raise ValueError(metric)
        self._scores = {}

    def scores(self, q):
        """s(q, i) for every item i: [num_items] f32"""
        q = int(q)
        if q not in self._scores:
            qhat = (self.E[q] * self.r[q]).astype(np.float32)
            self._scores[q] = (self.o.predict(qhat, self.all_items) * self.r).astype(np.float32)
        return self._scores[q]

    def rows(self, queries, k, include_self=False, exclude=None):
        """-> (items [Q, k] u32, scores [Q, k] f32)"""
        ri, rs = [], []
        for j, q in enumerate(queries):
            ex = [] if exclude is None else [int(x) for x in exclude[j]]
            if not include_self:
                ex.append(int(q))
            it, sc = topk_expectation(self.scores(q), ex, k)
            ri.append(it)
            rs.append(sc)
        return np.array(ri, dtype=np.uint32).reshape(-1, k), np.array(rs, dtype=np.float32).reshape(-1, k)
