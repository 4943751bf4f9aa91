"""The low-precision weight shadows of one ``functions.Runtime``: the bf16 copy ('n') and the transposed bf16 copy ('t') of a
parameter that the MFMA kernels read instead of the fp32 weight.  ``WeightShadows`` is the only code that knows how an entry is
stored; everything else (Runtime.weight / weight_t, the fused optimizers, engine.TrainStep) goes through its methods."""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import ops


class ShadowEntry(NamedTuple):
    version: int            # the parameter's ``_version`` the buffer was cast at
    ptr: int                # ... and its ``data_ptr()``: a parameter whose storage moved gets a new buffer
    buf: torch.Tensor


class WeightShadows:
    """Cache of shadow buffers keyed by ``(id(parameter), tag)``.

    An entry is owned by this object and is current while the parameter's version counter and data pointer are the ones it was
    cast at.  A new version at the same pointer is recast IN PLACE (``get``, ``refresh``, or an optimizer kernel that writes
    the buffer itself and then calls ``mark_current``): a captured graph keeps reading the same buffer.  A new pointer, or
    ``discard``, gives a fresh buffer.  After ``pin()`` - a captured graph has baked the buffer addresses in - a replaced
    buffer is never freed, only set aside (``retire``).  ``signature()`` names the set of buffers: whoever captured a graph
    compares it before a replay and captures again when it changed."""

    def __init__(self):
        self._entries = {}          # (id(param), tag) -> ShadowEntry
        self._retired = []          # buffers a captured graph may still read
        self._pinned = False
        self._plan = None           # the ops.WeightShadowPlan of the last refresh

    def __len__(self):
        return len(self._entries)

    @property
    def pinned(self):
        return self._pinned

    def get(self, w, tag, make):
        """The current shadow ``tag`` of ``w``.  ``make(out=None)`` casts ``w``, into ``out`` when given."""
        key = (id(w), tag)
        ent = self._entries.get(key)
        version, ptr = w._version, w.data_ptr()
        if ent is None or ent.version != version or ent.ptr != ptr:
            if ent is not None and ent.ptr == ptr:
                buf = make(out=ent.buf)     # refresh IN PLACE: a captured graph keeps reading the same shadow buffer
            else:
                if ent is not None:
                    self.retire(ent.buf)
                buf = make()
            ent = self._entries[key] = ShadowEntry(version, ptr, buf)
        return ent.buf

    def buffers(self):
        """{id(param): {'n': buffer, 't': buffer}} of every entry (a tag that was never asked for is absent)."""
        out = {}
        for (pid, tag), ent in self._entries.items():
            out.setdefault(pid, {})[tag] = ent.buf
        return out

    def signature(self):
        """Sorted (id(param), tag, buffer pointer) of every entry: what a captured graph baked in of this cache."""
        return tuple(sorted((pid, tag, ent.buf.data_ptr()) for (pid, tag), ent in self._entries.items()))

    def mark_current(self, params, only_buffers=None):
        """Somebody else wrote the shadows of ``params`` from their present values: set the entries' version to the parameters'
        current one.  ``only_buffers`` (a set of data pointers): only the entries whose buffer is one of them.  The pointer an
        entry was cast at stays, so a parameter whose storage moved still gets a fresh buffer on its next ``get``."""
        for p in params:
            for tag in ('n', 't'):
                ent = self._entries.get((id(p), tag))
                if ent is not None and (only_buffers is None or ent.buf.data_ptr() in only_buffers):
                    self._entries[(id(p), tag)] = ent._replace(version=p._version)

    def refresh(self, params):
        """Recast every cached shadow of ``params`` in place with ONE multi-tensor launch (after an optimizer step when replaying
        a graph: the captured kernels keep reading the same buffers)."""
        cached, by_id = self.buffers(), {id(p): p for p in params}
        params = [by_id[pid] for pid in cached if pid in by_id]
        entries = [(p.detach().reshape(p.shape[0], -1), cached[id(p)].get('n'), cached[id(p)].get('t')) for p in params]
        if not entries:
            return
        key = tuple((w.data_ptr(), 0 if n is None else n.data_ptr(), 0 if t is None else t.data_ptr()) for w, n, t in entries)
        if self._plan is None or self._plan.key != key:
            self._plan = ops.WeightShadowPlan(entries)
        self._plan.run()
        self.mark_current(params)

    def snapshot(self, params):
        """Copies of the cached shadows of ``params``, with whether each was current: what ``restore`` puts back."""
        by_id = {id(p): p for p in params}
        return {key: (ent.version == by_id[key[0]]._version and ent.ptr == by_id[key[0]].data_ptr(), ent.buf.clone())
                for key, ent in self._entries.items() if key[0] in by_id}

    def restore(self, saved, params):
        """The parameters were set back in place to what they held at ``snapshot``: so are the shadows, IN PLACE (a captured graph
        keeps reading the same buffers).  An entry ``saved`` has no copy of (created since) is recast from its parameter; one that was
        not current at the snapshot holds its old bits again and stays not current."""
        self.refresh(params)
        for key, (current, buf) in saved.items():
            ent = self._entries.get(key)
            if ent is not None and ent.buf.shape == buf.shape:
                ent.buf.copy_(buf)
                if not current:
                    self._entries[key] = ent._replace(version=-1)

    def pin(self):
        """A captured graph reads the buffers from now on: none is freed any more, only refreshed in place or retired."""
        self._pinned = True

    def retire(self, buf):
        """``buf`` (a tensor, or a tuple of them) leaves the cache: kept alive when pinned, dropped otherwise."""
        if self._pinned:
            self._retired.append(buf)

    def discard(self, w):
        """Drop the entries of ``w`` (retired when pinned): the next ``get`` casts into fresh buffers."""
        for key in [k for k in self._entries if k[0] == id(w)]:
            self.retire(self._entries.pop(key).buf)
