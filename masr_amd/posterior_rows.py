"""Row bookkeeping of a streaming pool's posterior history (``StreamPool(predictor, timestamps=True)``, serving.py): which rows of the
device-resident row pool [n_rows, V] belong to which session.  Pure python: it needs neither the library nor a GPU.

Rows are handed out one by one -- freed rows first (last freed, first reused), then fresh ones -- so a session's rows are neither
contiguous nor increasing in general; ``rows_of`` keeps them in frame order, which is what masr_ctc_align_rows reads as its
``frame_row`` table.  The pool grows by whole slabs of ``slab`` rows; a row keeps its number for as long as its session holds it
(``reset`` / ``close`` of the session give its rows back)."""
import numpy as np


class RowAllocator:
    def __init__(self, slab=4096):
        if slab <= 0:
            raise ValueError('RowAllocator: slab > 0 expected')
        self.slab = int(slab)
        self.capacity = 0             # rows the pool must hold: a multiple of ``slab``
        self.fresh = 0                # rows never handed out lie at fresh .. capacity
        self._free = []               # rows given back
        self._rows = {}               # owner -> list of its rows in frame order

    def take(self, owner, n):
        """``n`` more rows for ``owner`` (appended behind the rows it has, i.e. its next ``n`` frames) -> their numbers, int64 [n].
        ``capacity`` has grown by whole slabs when the call returns if the free and the fresh rows did not suffice."""
        n = int(n)
        if n < 0:
            raise ValueError('RowAllocator.take: n >= 0 expected')
        reuse = min(n, len(self._free))
        got = [self._free.pop() for _ in range(reuse)]
        rest = n - reuse
        if rest:
            need = self.fresh + rest
            if need > self.capacity:
                self.capacity = -(-need // self.slab) * self.slab
            got.extend(range(self.fresh, need))
            self.fresh = need
        self._rows.setdefault(owner, []).extend(got)
        return np.asarray(got, np.int64)

    def rows_of(self, owner):
        """the owner's rows in frame order (the list itself: not to be changed by the caller)"""
        return self._rows.get(owner, [])

    def release(self, owner):
        """give all rows of ``owner`` back -> how many"""
        rows = self._rows.pop(owner, [])
        self._free.extend(rows)
        return len(rows)

    @property
    def in_use(self):
        return self.fresh - len(self._free)
