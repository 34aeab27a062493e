"""Where a pool lives: the one place that knows how router positions (`r.cfmms[i]`), packed positions (the order of the
device pool store and of its trade arrays), batches and device segments map onto each other.  Plain numpy: no device, no
backend.  Built once from what `_segments_of` decides; everything below is looked up, not re-derived, per call."""
from __future__ import annotations

import numpy as np

from ._lib import ArgumentError
from .cfmms import KINDS, _sync_pool


class PoolLayout:
    """batches: homogeneous PoolBatches in packed order (an empty batch has no device segment); order[k]: router position
    of the k-th packed pool (None: packing kept the router order); host: router positions of the host-evaluated pools, which
    a backend numbers behind the packed ones."""

    def __init__(self, batches, order=None, host=()):
        self.batches = batches
        self.order = None if order is None else np.asarray(order, dtype=np.int64)
        self.host = np.asarray(list(host), dtype=np.int64)
        self.offsets = np.cumsum([0] + [len(b) for b in batches])           # first packed position of every batch
        self.m = int(self.offsets[-1])                                      # pools with a device kernel
        self.n_pools = self.m + self.host.size
        self.seg_of = {}                                                    # batch number -> device segment
        for b, batch in enumerate(batches):
            if len(batch):
                self.seg_of[b] = len(self.seg_of)
        self.coins = [int(batches[b].Ai.shape[1]) for b in self.seg_of]     # per segment
        # weighted / Curve pools: trades are per-pool vectors (the reference's ragged Vector{Vector}, src/router.jl:7-8)
        self.ragged = any(KINDS[b.kind].family is not None for b in batches)
        self.per_pool = self.ragged or self.host.size > 0
        # backend position -> router position, and its inverse
        self.place = np.concatenate([np.arange(self.m, dtype=np.int64) if order is None else self.order, self.host])
        self._where = np.empty(self.n_pools, dtype=np.int64)
        self._where[self.place] = np.arange(self.n_pools)
        sizes = np.repeat(np.array(self.coins, dtype=np.int64), [len(batches[b]) for b in self.seg_of]) if self.ragged else []
        self._cuts = np.cumsum(sizes)[:-1]                                  # where split() cuts the flat ragged trades

    def segments(self):
        """(segment, first packed position, batch) over the non-empty batches, segments numbered from 0"""
        return [(seg, int(self.offsets[b]), self.batches[b]) for b, seg in self.seg_of.items()]

    def locate(self, i):
        """router position -> ("device", batch number, row) or ("host", position among the host pools)"""
        i = int(i)
        if not 0 <= i < self.n_pools:
            raise ArgumentError(f"pool {i} out of range 0:{self.n_pools - 1}")
        k = int(self._where[i])
        if k >= self.m:
            return "host", k - self.m
        b = int(np.searchsorted(self.offsets, k, side="right") - 1)
        return "device", b, k - int(self.offsets[b])

    def zero_trades(self):
        """zerotrade per pool (src/router.jl:23-26), packed order: an [m, 2] array, or per-pool vectors if ragged"""
        if self.ragged:
            return [np.zeros(b.Ai.shape[1]) for b in self.batches for _ in range(len(b))]
        return np.zeros((self.m, 2))

    def split(self, flat):
        """the ragged flat trade layout of cfmm_get_trades (packed order) -> per-pool vectors"""
        return np.split(np.ravel(flat), self._cuts) if self.m else []

    def to_router(self, dev_rows, host_rows=()):
        """packed rows, then the host pools' rows -> one list in router order"""
        out, place = [None] * self.n_pools, self.place.tolist()
        for k in range(self.m):
            out[place[k]] = dev_rows[k]
        for j in range(self.host.size):
            out[place[self.m + j]] = host_rows[j]
        return out

    def Ai_router_order(self):
        """the token indices of a router of two-coin device pools, [m, 2] in router order"""
        Ai = np.concatenate([b.Ai for b in self.batches]) if self.batches else np.zeros((0, 2), dtype=np.int64)
        if self.order is None:
            return Ai
        Ar = np.empty_like(Ai)
        Ar[self.order] = Ai
        return Ar

    def sync_pools(self, cfmms, batch_no=None, rows=None):
        """Keep the per-pool objects of a router built from a pool list in step with the batches: all pools after
        update_reserves! (reserves and prices moved), or `rows` of one batch after update_pools_ (any state, ladders too)."""
        if not isinstance(cfmms, list):        # (built from batches: r.cfmms materialises pools on demand)
            return
        for b in range(len(self.batches)) if batch_no is None else (batch_no,):
            batch, first = self.batches[b], int(self.offsets[b])
            for row in range(len(batch)) if rows is None else rows:
                _sync_pool(cfmms[int(self.place[first + row])], batch, row, full=rows is not None)
