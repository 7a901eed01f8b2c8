"""Rings of pinned host buffers: the one discipline behind every staging and read-back buffer of the offline path.

A ring has a fixed number of slots that take turns.  The slot count says how many copies may be in flight before a buffer is
written again: it is chosen by the owner for the number of passes it keeps in flight.  A ring made with ``events=True`` also
carries one event per slot: ``take`` waits for the event of the slot it hands out, and the caller records it
(``slot.record()``) on the stream of its copy once that copy is queued, so a buffer is never rewritten under a copy that still
reads it.  Buffers are allocated (zero-filled) on first use and again only when a request outgrows them.

A ring keeps separate slots per dtype (and per ``key``, for owners that share one ring between named uses)."""
import torch


class _Slot:
    __slots__ = ('buf', '_lane', '_k')

    def __init__(self, buf, lane, k):
        self.buf, self._lane, self._k = buf, lane, k

    def record(self, stream=None):
        """the slot's copy is queued: record its event on ``stream`` (default: the current one); rings with events only"""
        events = self._lane[1]
        ev = events[self._k] or torch.cuda.Event()
        if stream is None:
            ev.record()
        else:
            ev.record(stream)
        events[self._k] = ev


class PinnedRing:
    def __init__(self, slots, min_numel=0, headroom=False, events=False):
        """``min_numel``: the least a buffer is allocated with; ``headroom``: a buffer that has to grow is allocated a quarter
        larger than asked for (requests of slowly growing size then reallocate once, not every time)"""
        self.slots, self.min_numel, self.headroom, self.events = int(slots), int(min_numel), bool(headroom), bool(events)
        self._lanes = {}                 # (key, dtype) -> [buffers, events, turn]

    def take(self, numel, dtype=torch.int32, key=None):
        """the next slot in turn -> its first ``numel`` elements as ``slot.buf`` (waits for the slot's event, if it has one)"""
        lane = self._lanes.get((key, dtype))
        if lane is None:
            lane = self._lanes[(key, dtype)] = [[None] * self.slots, [None] * self.slots if self.events else None, 0]
        bufs, events, k = lane
        lane[2] = (k + 1) % self.slots
        if events is not None and events[k] is not None:
            events[k].synchronize()
        if bufs[k] is None or bufs[k].numel() < numel:
            want = numel + numel // 4 if self.headroom else numel
            bufs[k] = torch.zeros(max(want, self.min_numel), dtype=dtype, pin_memory=True)
        return _Slot(bufs[k][:numel], lane, k)
