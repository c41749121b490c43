"""A plain-Python model of a session store's seen-item memory (sbr_sessions_create_seen): per slot, the list of the last W items
appended since the slot's last reset, in append order, repeats kept.  The rules are the header's (include/sbr_hip.h, SEEN-ITEM
MEMORY): append pushes and forgets the oldest beyond W; reset, reset of everything and set_state empty a slot's list; set_seen
replaces it with the last W items given.  Nothing here knows how the device stores it."""
import numpy as np


class SeenModel:
    def __init__(self, capacity: int, w: int):
        if w < 1:
            raise ValueError("a model of a store WITH memory: w >= 1")
        self.capacity, self.w = int(capacity), int(w)
        self.lists = [[] for _ in range(self.capacity)]

    def _check(self, slots):
        slots = [int(s) for s in slots]
        if any(s < 0 or s >= self.capacity for s in slots) or len(set(slots)) != len(slots):
            raise ValueError("slots: each below capacity, none twice")
        return slots

    def append(self, slots, items):
        slots = self._check(slots)
        if len(items) != len(slots):
            raise ValueError("one item sequence per slot")
        for s, seq in zip(slots, items):
            kept = self.lists[s] + [int(x) for x in seq]
            self.lists[s] = kept[max(0, len(kept) - self.w):]

    def reset(self, slots=None):
        for s in range(self.capacity) if slots is None else self._check(slots):
            self.lists[s] = []

    def set_state(self, slots):
        """a restored state's items are unknown: the memory is emptied"""
        self.reset(slots)

    def set_seen(self, slots, items):
        slots = self._check(slots)
        if len(items) != len(slots):
            raise ValueError("one item sequence per slot")
        for s, seq in zip(slots, items):
            seq = [int(x) for x in seq]
            self.lists[s] = seq[max(0, len(seq) - self.w):]

    def seen(self, slots):
        """one uint32 array per slot, oldest first"""
        return [np.array(self.lists[s], dtype=np.uint32) for s in self._check(slots)]

    def excluded(self, slots, exclude=None):
        """what a scan of `slots` excludes: each slot's memory united with the caller's list, as one array per slot"""
        mine = self.seen(slots)
        if exclude is None:
            return mine
        return [np.concatenate([a, np.asarray(e, dtype=np.uint32).ravel()]) for a, e in zip(mine, exclude)]
