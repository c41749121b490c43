"""A plain-numpy reference of the audience scan (sbr_audience_reps / sbr_sessions_audience, include/sbr_hip.h AUDIENCE): given the
scores of every (query, candidate) pair, the candidates' ids and the per-query exclusions, the rows the call must return.

The order is the header's: score descending, -0.0 equal to +0.0, a tie to the lower id; the scores are reported with the bits they
came with; rows shorter than k end in (0xFFFFFFFF, -inf).  Nothing here computes a score: the tests take them from
store.score_candidates, which runs on the vector ALU, not in the scan.  seen_excluded() is the rule for which slots a store with
seen-item memory leaves out of a query's row, on tests/seen_expect.SeenModel's ring contents."""
import numpy as np

NO_ROW = 0xFFFFFFFF


def expected_rows(score_bits, ids, k, exclude=None):
    """score_bits [Q, S] uint32 (f32 bits of score(query j, candidate s)), ids [S] the candidates' ids (distinct), exclude None or
    one collection of ids per query -> (rows [Q, k] uint32, score bits [Q, k] uint32)"""
    score_bits = np.ascontiguousarray(score_bits, dtype=np.uint32)
    ids = np.asarray(ids, dtype=np.uint32).ravel()
    nq = score_bits.shape[0]
    assert score_bits.shape == (nq, ids.size) and len(set(ids.tolist())) == ids.size
    if exclude is not None and len(exclude) != nq:
        raise ValueError("one exclusion collection per query")
    rows = np.full((nq, k), NO_ROW, dtype=np.uint32)
    out = np.full((nq, k), np.float32(-np.inf).view(np.uint32), dtype=np.uint32)
    for j in range(nq):
        sc = score_bits[j].view(np.float32)
        keep = np.ones(ids.size, dtype=bool)
        if exclude is not None:
            keep &= ~np.isin(ids, np.asarray(list(exclude[j]), dtype=np.uint32))
        at = np.flatnonzero(keep)
        # lexsort: last key first; -sc makes -0.0 and +0.0 the same key (0.0 == -0.0), so the id decides between them
        order = at[np.lexsort((ids[at], -sc[at].astype(np.float64)))][:k]
        rows[j, : order.size] = ids[order]
        out[j, : order.size] = score_bits[j, order]
    return rows, out


def brute_force_rows(score_bits, ids, k, exclude=None):
    """The same rows by the definition alone — a Python sort with an explicit comparison — for the reference's own test."""
    import functools

    score_bits = np.ascontiguousarray(score_bits, dtype=np.uint32)
    ids = [int(x) for x in np.asarray(ids).ravel()]
    rows, out = [], []
    for j in range(score_bits.shape[0]):
        banned = set() if exclude is None else {int(x) for x in exclude[j]}
        pairs = [(float(np.uint32(b).view(np.float32)), i, int(b)) for b, i in zip(score_bits[j].tolist(), ids) if i not in banned]

        def before(a, b):
            if a[0] > b[0]:
                return -1
            if a[0] < b[0]:
                return 1
            return -1 if a[1] < b[1] else (1 if a[1] > b[1] else 0)

        pairs.sort(key=functools.cmp_to_key(before))
        pairs = pairs[:k] + [(-np.inf, NO_ROW, int(np.float32(-np.inf).view(np.uint32)))] * max(0, k - len(pairs))
        rows.append([p[1] for p in pairs])
        out.append([p[2] for p in pairs])
    return np.array(rows, dtype=np.uint32).reshape(-1, k), np.array(out, dtype=np.uint32).reshape(-1, k)


def seen_excluded(seen_model, slots, items):
    """Per query item, the set of candidate slots whose memory (SeenModel: the last W items appended since the slot's reset) holds
    it — a repeat in a memory counts once, a slot outside `slots` never."""
    mem = {int(s): set(x.tolist()) for s, x in zip(slots, seen_model.seen(slots))}
    return [{s for s, have in mem.items() if int(q) in have} for q in np.asarray(items).ravel()]


def unite(a, b):
    """per-query union of two exclusion collections (either may be None)"""
    if a is None:
        return b
    if b is None:
        return a
    return [set(int(v) for v in x) | set(int(v) for v in y) for x, y in zip(a, b)]
