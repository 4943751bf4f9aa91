"""The bookkeeping of the weight-shadow cache (functions.WeightShadows) on CPU tensors: when an entry is served, recast in place or
re-created, what pin / retire / discard keep alive, what the signature sees and what mark_current touches.  No kernel runs."""
import gc
import types
import weakref

import pytest
import torch


class _Casts:
    """``make`` of one parameter: w -> bf16, into ``out`` when given; records every call's ``out``."""

    def __init__(self, w):
        self.w, self.calls = w, []

    def __call__(self, out=None):
        self.calls.append(out)
        new = self.w.detach().to(torch.bfloat16)
        return new if out is None else out.copy_(new)


@pytest.fixture
def cache(vited):
    return vited.functions.WeightShadows()


@pytest.fixture
def params():
    g = torch.Generator().manual_seed(0)
    return torch.nn.Parameter(torch.randn(4, 8, generator=g)), torch.nn.Parameter(torch.randn(8, generator=g))


def _bump(w):
    torch.autograd.graph.increment_version([w])


def test_same_version_serves_the_buffer_without_a_cast(cache, params):
    for w in params:
        make = _Casts(w)
        buf = cache.get(w, 'n', make)
        assert torch.equal(buf, w.detach().to(torch.bfloat16)) and make.calls == [None]
        assert cache.get(w, 'n', make) is buf and make.calls == [None]
    assert len(cache) == 2


def test_new_version_recasts_in_place_and_keeps_the_signature(cache, params):
    for w in params:
        make = _Casts(w)
        buf = cache.get(w, 'n', make)
        ptr, sig = buf.data_ptr(), cache.signature()
        with torch.no_grad():
            w.mul_(2.0)                         # a new value ...
        _bump(w)                                # ... and (again) a new version
        again = cache.get(w, 'n', make)
        assert len(make.calls) == 2 and make.calls[1] is buf, 'the recast must be handed the old buffer as out='
        assert again is buf and again.data_ptr() == ptr and torch.equal(again, w.detach().to(torch.bfloat16))
        assert cache.signature() == sig


@pytest.mark.parametrize('pinned', [False, True])
def test_moved_storage_gets_a_new_buffer_and_pin_keeps_the_old_one(cache, params, pinned):
    if pinned:
        cache.pin()
    for w in params:
        make = _Casts(w)
        buf = cache.get(w, 'n', make)
        ptr, sig, old = buf.data_ptr(), cache.signature(), weakref.ref(buf)
        w.data = w.data.clone()
        new = cache.get(w, 'n', make)
        assert make.calls == [None, None], 'a moved parameter is cast into a fresh buffer'
        assert new is not buf and new.data_ptr() != ptr
        assert cache.signature() != sig
        assert (id(w), 'n', new.data_ptr()) in cache.signature()
        del buf
        gc.collect()
        assert (old() is not None) == pinned, 'the old buffer is retired (kept) exactly when the cache is pinned'
        if pinned:
            assert old().data_ptr() == ptr


def test_signature_is_sorted_pid_tag_pointer(cache, params):
    w, b = params
    bufs = {(id(p), tag): cache.get(p, tag, _Casts(p)) for p in (w, b) for tag in ('t', 'n')}
    assert cache.signature() == tuple(sorted((pid, tag, buf.data_ptr()) for (pid, tag), buf in bufs.items()))
    assert cache.buffers() == {id(p): {'n': bufs[(id(p), 'n')], 't': bufs[(id(p), 't')]} for p in (w, b)}


def test_mark_current_touches_only_the_named_buffers(cache, params):
    w, b = params
    make_n, make_t, make_b = _Casts(w), _Casts(w), _Casts(b)
    n, t, other = cache.get(w, 'n', make_n), cache.get(w, 't', make_t), cache.get(b, 'n', make_b)
    _bump(w), _bump(b)
    cache.mark_current([w, b], only_buffers={n.data_ptr()})
    assert cache.get(w, 'n', make_n) is n and len(make_n.calls) == 1, 'marked current: no cast'
    assert cache.get(w, 't', make_t) is t and make_t.calls == [None, t], 'not in the set: left stale, recast in place'
    assert cache.get(b, 'n', make_b) is other and make_b.calls == [None, other]
    _bump(w), _bump(b)
    cache.mark_current([w])                     # without a set: every entry of the parameters given, and of no other
    assert cache.get(w, 'n', make_n) is n and cache.get(w, 't', make_t) is t
    assert len(make_n.calls) == 1 and len(make_t.calls) == 2
    cache.get(b, 'n', make_b)
    assert len(make_b.calls) == 3


@pytest.mark.parametrize('pinned', [False, True])
def test_discard_gives_fresh_buffers(cache, params, pinned):
    w, b = params
    if pinned:
        cache.pin()
    make, make_b = _Casts(w), _Casts(b)
    olds = [cache.get(w, 'n', make), cache.get(w, 't', make)]
    kept = cache.get(b, 'n', make_b)
    ptrs, refs = [o.data_ptr() for o in olds], [weakref.ref(o) for o in olds]
    cache.discard(w)
    assert len(cache) == 1 and id(w) not in cache.buffers()
    news = [cache.get(w, 'n', make), cache.get(w, 't', make)]
    assert make.calls == [None] * 4
    assert all(new.data_ptr() not in ptrs for new in news)
    assert cache.get(b, 'n', make_b) is kept and make_b.calls == [None], 'another parameter\'s entry stays'
    del olds
    gc.collect()
    assert all((r() is not None) == pinned for r in refs)


def test_retire_keeps_a_buffer_only_when_pinned(cache):
    for pinned in (False, True):
        bufs = (torch.zeros(3), torch.zeros(3))        # (a tuple of buffers: the folded kv weights go in as one)
        ref = weakref.ref(bufs[0])
        cache.retire(bufs)
        del bufs
        gc.collect()
        assert (ref() is not None) == pinned
        cache.pin()


def test_shadows_of(vited):
    shadows_of = vited.functions.shadows_of
    assert shadows_of(types.SimpleNamespace(_runtimes={})) == []
    assert shadows_of(object()) == []
    rt = types.SimpleNamespace(shadows=vited.functions.WeightShadows())
    assert shadows_of(types.SimpleNamespace(_runtimes={torch.bfloat16: rt})) == [rt.shadows]
