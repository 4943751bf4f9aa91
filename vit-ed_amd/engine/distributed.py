"""Process-group setup and the data-parallel gradient exchange: one flat fp32 gradient buffer, all-reduced by RCCL over xGMI in
one or two buckets, instead of DistributedDataParallel's 25 MB buckets (misc/utils.py:319-344, misc/engine.py:75)."""
from __future__ import annotations

import os

import torch
import torch.distributed as dist


def configure_ddp(backend: str | None = None):
    """env:// rendezvous like the reference, but device-aware: 'nccl' (= RCCL on ROCm) when a GPU is
    present, 'gloo' otherwise (the reference hard-codes nccl and cannot run BASELINE config 0 on CPU)."""
    rank = int(os.environ.get('RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29511')
    use_cuda = torch.cuda.is_available()
    if use_cuda:
        torch.cuda.set_device(local_rank)
    if not dist.is_initialized():
        kw = {}
        if use_cuda:
            kw['device_id'] = torch.device('cuda', local_rank)
        dist.init_process_group(backend=backend or ('nccl' if use_cuda else 'gloo'), init_method='env://',
                                world_size=world, rank=rank, **kw)
    dist.barrier()
    return local_rank, rank, world


def _avg_supported(group=None) -> bool:
    """ReduceOp.AVG exists on the nccl (= RCCL) backend only; gloo has SUM."""
    return dist.is_initialized() and dist.get_backend(group) == 'nccl'


class FlatGradients:
    """All parameter gradients as views of ONE contiguous fp32 buffer.

    ``p.grad`` is pre-set to a view, so autograd accumulates in place and the buffer is always the
    gradient; ``zero()`` replaces ``optimizer.zero_grad()``; ``all_reduce_mean()`` is the data-parallel
    exchange: one RCCL all-reduce of the whole buffer (133 MB fp32 at config A - SURVEY.md 2.3 C1 -
    instead of six 25 MB buckets), optionally bf16-compressed on the wire.

    ``early`` (an iterable of parameters) are laid out FIRST: ``buckets()`` then yields two contiguous
    ranges, [early | rest].  TrainStep passes the decoder-only parameters there - their gradients are
    final when the decoder's backward returns, so their all-reduce can run under the encoder's backward
    (the overlap c10d's DDP reducer gives the reference, misc/engine.py:75)."""

    def __init__(self, params, compress_bf16: bool = False, early=None):
        params = [p for p in params if p.requires_grad]
        if not params:
            raise ValueError('no trainable parameters')
        early_ids = {id(p) for p in (early or ())}
        first = [p for p in params if id(p) in early_ids]
        rest = [p for p in params if id(p) not in early_ids]
        self.params = first + rest
        dev = self.params[0].device
        # every view starts on a 64-byte boundary (config H's [1] head bias would otherwise leave everything behind it on an odd
        # word: the kernels that add into these views use 16-byte accesses); the padding words stay zero
        align = lambda n: (n + 15) // 16 * 16
        self.offsets, off = [], 0
        for i, p in enumerate(self.params):
            self.offsets.append(off)
            off += align(p.numel())
            if i + 1 == len(first):
                self.split = off                        # [0, split) = early bucket, [split, total) = the rest
        total = off
        if not first:
            self.split = 0
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.wire = torch.empty(total, dtype=torch.bfloat16, device=dev) if compress_bf16 else None
        self.views = []
        for p, o in zip(self.params, self.offsets):
            v = self.flat[o: o + p.numel()].view_as(p)
            p.grad = v
            self.views.append(v)
        self._pending = []

    def buckets(self):
        total = self.flat.numel()
        return [(0, self.split), (self.split, total)] if 0 < self.split < total else [(0, total)]

    def attach(self):
        """Make every ``p.grad`` the flat view again.  ``optimizer.zero_grad()`` (the reference's loop,
        misc/engine.py:231; set_to_none=True by default since torch 2.0) detaches them: a parameter whose grad
        is None gets its view back ZEROED, one that received a fresh tensor has it copied into the view."""
        detached = [(p, v) for p, v in zip(self.params, self.views) if p.grad is not v]
        if not detached:
            return 0
        if len(detached) == len(self.params) and all(p.grad is None for p, _ in detached):
            self.flat.zero_()                      # the common case: one fill instead of one per parameter
        else:
            for p, v in detached:
                if p.grad is None:
                    v.zero_()
                else:
                    v.copy_(p.grad)
        for p, v in detached:
            p.grad = v
        return len(detached)

    def zero(self):
        self.flat.zero_()
        for p, v in zip(self.params, self.views):
            if p.grad is not v:          # someone called zero_grad(set_to_none=True): re-attach
                p.grad = v

    # -- the exchange ------------------------------------------------------------------------
    def start_all_reduce(self, lo: int, hi: int, group=None):
        """Launch the mean all-reduce of flat[lo:hi] WITHOUT waiting for it (RCCL runs it on the process
        group's own stream behind everything already queued on the current stream).  ``finish_all_reduce``
        joins."""
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        # VITED_FORCE_COLLECTIVE=1: issue the collective on a one-rank group too (a one-GPU box can then exercise the RCCL calls and
        # their ordering against the graph replays; the mean over one rank is the identity)
        force = world == 1 and dist.is_initialized() and os.environ.get('VITED_FORCE_COLLECTIVE') == '1'
        if (world == 1 and not force) or hi <= lo:
            return
        seg = self.flat[lo:hi]
        if self.wire is not None:
            buf = self.wire[lo:hi]
            buf.copy_(seg)
        else:
            buf = seg
        avg = _avg_supported(group)
        work = dist.all_reduce(buf, op=dist.ReduceOp.AVG if avg else dist.ReduceOp.SUM, group=group, async_op=True)
        self._pending.append((work, seg, buf, None if avg else 1.0 / world))

    def finish_all_reduce(self):
        for work, seg, buf, scale in self._pending:
            work.wait()                       # the current stream now waits for the collective
            if buf is not seg:
                seg.copy_(buf)
            if scale is not None:
                seg.mul_(scale)
        self._pending = []

    def all_reduce_mean(self, group=None):
        self.start_all_reduce(0, self.flat.numel(), group)
        self.finish_all_reduce()

    def clip_(self, max_norm: float):
        """clip_grad_norm_ on the flat buffer: one norm kernel instead of 280 (misc/utils.py:215-217)."""
        norm = torch.linalg.vector_norm(self.flat)
        scale = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        self.flat.mul_(scale)
        return norm


def broadcast_parameters(model, src: int = 0, group=None):
    """DDP ctor semantics: every rank starts from rank 0's parameters - as ONE
    broadcast of a flattened copy (the reference's DDP ctor also coalesces) instead of one per tensor."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return
    params = [p.data for p in model.parameters()]
    by_dtype = {}
    for p in params:
        by_dtype.setdefault(p.dtype, []).append(p)
    for ps in by_dtype.values():
        flat = torch.cat([p.reshape(-1) for p in ps])
        dist.broadcast(flat, src=src, group=group)
        off = 0
        for p in ps:
            p.copy_(flat[off: off + p.numel()].view_as(p))
            off += p.numel()
