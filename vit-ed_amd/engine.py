"""The driven training step of the reference (misc/engine.py:183-257, misc/utils.py:206-232,319-344)
re-plumbed for MI355X: one process per GPU, RCCL all-reduce of a single flat fp32 gradient buffer
over xGMI instead of c10d's 25 MB DDP buckets, bf16 autocast instead of fp16 + GradScaler, and the
whole forward+backward replayable as one hipGraph.

Only what drives the hot path is here, with the evaluation paths
on the device (retrieval, geshaem, puzzle, and ``validate_classifier`` for main.py's validation); data
loading, logging and checkpoint rotation stay in the reference's ``Trainer``.
"""
from __future__ import annotations

import functools
import math
import os
from typing import NamedTuple

import torch
import torch.distributed as dist


# ---------------------------------------------------------------------------------------------
# process group (misc/utils.py:319-344)
# ---------------------------------------------------------------------------------------------
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


# ---------------------------------------------------------------------------------------------
# flat gradient buffer + all-reduce (replaces DistributedDataParallel, misc/engine.py:75)
# ---------------------------------------------------------------------------------------------
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


# ---------------------------------------------------------------------------------------------
# optimizer (misc/optimizer.py:10-46)
# ---------------------------------------------------------------------------------------------
def param_groups_no_decay_1d(model):
    decay, no_decay = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        (no_decay if (p.ndim == 1 or name.endswith('.bias')) else decay).append(p)
    return [{'params': decay}, {'params': no_decay, 'weight_decay': 0.}]


def build_optimizer(config, model, capturable: bool = False, fused_hip: bool | None = None, skip_nonfinite: bool = False):
    """misc/optimizer.py:10-46: AdamW / Nesterov SGD with the no-decay group for 1-D parameters and ``*.bias``.

    On a GPU model they are ``optim.FlatAdamW`` / ``optim.FlatSGD`` (the HIP multi-tensor kernels: clip + update + bf16
    weight-shadow refresh in one pass, hipGraph-replayable with a per-iteration learning rate); ``fused_hip=False`` gives
    ``torch.optim.AdamW(fused=True)`` / ``torch.optim.SGD`` instead, with ``capturable`` forwarded to AdamW (a torch optimizer
    captured into a hipGraph must be built with capturable=True, and TrainStep keeps its learning rate in a device tensor).
    ``skip_nonfinite=True`` (HIP optimizers only) leaves out an update whose gradient norm is inf or NaN, which is what
    ``GradScaler.step`` does in the reference's loop (misc/utils.py:206-226)."""
    name = config.TRAIN.OPTIMIZER.NAME.lower()
    groups = param_groups_no_decay_1d(model)
    on_gpu = all(p.is_cuda for g in groups for p in g['params'])
    hip = on_gpu and (fused_hip is None or fused_hip)
    if name not in ('adamw', 'sgd'):
        raise ValueError(f'unknown optimizer {name}')
    if skip_nonfinite and not hip:
        raise ValueError('skip_nonfinite=True needs the HIP optimizers (a GPU model and fused_hip in (None, True)): the torch '
                         'optimizers have no such check')
    if name == 'adamw':
        kw = dict(eps=config.TRAIN.OPTIMIZER.EPS, betas=tuple(config.TRAIN.OPTIMIZER.BETAS), lr=config.TRAIN.BASE_LR,
                  weight_decay=config.TRAIN.WEIGHT_DECAY)
        if hip:
            from .optim import FlatAdamW
            # the model's bf16 weight shadows are refreshed by the update kernel
            return FlatAdamW(groups, model=model, skip_nonfinite=skip_nonfinite, **kw)
        if on_gpu:
            return torch.optim.AdamW(groups, fused=True, capturable=capturable, **kw)
        return torch.optim.AdamW(groups, **kw)
    kw = dict(momentum=config.TRAIN.OPTIMIZER.MOMENTUM, nesterov=True, lr=config.TRAIN.BASE_LR, weight_decay=config.TRAIN.WEIGHT_DECAY)
    if hip:
        from .optim import FlatSGD
        return FlatSGD(groups, model=model, skip_nonfinite=skip_nonfinite, **kw)
    return torch.optim.SGD(groups, **kw)


class NativeScalerWithGradNormCount:
    """Call-compatible with misc/utils.py:206-232.  bf16 needs no loss scaling, so ``scale`` is 1;
    the call still does backward -> (all-reduce) -> clip -> step and returns the gradient norm.

    With ``flat`` (a FlatGradients) the gradients live in one buffer that is all-reduced and clipped as a
    whole.  The reference's loop calls ``optimizer.zero_grad()`` after every update (misc/engine.py:231),
    which DETACHES ``p.grad`` from the buffer (set_to_none), so the views are re-attached (and zeroed)
    before every backward - otherwise the exchange and the clip would act on a stale buffer while the
    optimizer consumed un-reduced gradients."""
    state_dict_key = 'amp_scaler'

    def __init__(self, flat: FlatGradients | None = None):
        self.flat = flat

    def __call__(self, loss, optimizer, clip_grad=None, parameters=None, create_graph=False, update_grad=True):
        if self.flat is not None:
            self.flat.attach()
        loss.backward(create_graph=create_graph)
        if not update_grad:
            return None
        if self.flat is not None:
            self.flat.attach()     # a backward that found grad=None would have allocated fresh tensors: fold them in
            self.flat.all_reduce_mean()
            norm = self.flat.clip_(clip_grad) if clip_grad is not None else torch.linalg.vector_norm(self.flat.flat)
        else:
            parameters = list(parameters)
            if clip_grad is not None:
                norm = torch.nn.utils.clip_grad_norm_(parameters, clip_grad)
            else:
                norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in parameters]))
        optimizer.step()
        return norm

    def state_dict(self):
        return {'scale': 1.0}

    def load_state_dict(self, state_dict):
        pass


# ---------------------------------------------------------------------------------------------
# the per-iteration body of train_one_epoch (misc/engine.py:202-231), hipGraph-replayable
# ---------------------------------------------------------------------------------------------
def _decoder_only_parameters(model):
    """Parameters whose gradient is complete once the decoder + head backward has run: everything except the
    encoder blocks and the tensors both image paths share (patch_embed.*, pos_embed get gradient from the
    encoder too, vision_transformer.py:379,391-392)."""
    out = []
    for name, p in model.named_parameters():
        if name.startswith(('cross_blocks.', 'norm.', 'head.')) or name == 'cls_token':
            out.append(p)
    return out


# Graph capture must not make OTHER threads' HIP calls illegal: RCCL's watchdog thread polls the events of finished collectives
# (hipEventQuery) whenever it likes, and under the default "global" capture mode such a query during a capture kills the process
# group ("operation not permitted when stream is capturing").  Only this thread's own calls are restricted.
_CAPTURE_MODE = 'thread_local'


class TrainMeters:
    """The meters of the reference's training loop (misc/engine.py:195-196, 221-222, 235, 256-257) in fp64 accumulators on the
    device, so that keeping them costs no host read per iteration:
      loss       ``loss_meter.update(loss * accumulation_steps, n)`` per micro-step (``loss`` is the divided loss TrainStep returns)
      grad_norm  ``norm_meter.update(grad_norm)`` per update
      nonfinite  how many of those norms were inf or NaN (each of them also makes ``grad_norm.avg`` non-finite, as it does in the
                 reference's log line)
    The arithmetic is AverageMeter's, operation for operation, in fp64.  Elementwise torch operations on ``device``: they run
    eagerly or inside a captured graph alike."""

    def __init__(self, device='cuda', accumulation_steps: int = 1):
        self.accum = max(int(accumulation_steps), 1)
        # loss: val, sum, count; grad_norm: val, sum, count; non-finite norms
        self.state = torch.zeros(7, dtype=torch.float64, device=torch.device(device))

    def reset(self):
        """Start an epoch."""
        self.state.zero_()

    @torch.no_grad()
    def update_loss(self, loss: torch.Tensor, n):
        """``n``: the number of target rows, a Python number or a device scalar (``MinedPairs.counts[3]``)."""
        v = loss.detach().to(torch.float64)
        if self.accum > 1:
            v = v * self.accum
        n = n.to(torch.float64) if torch.is_tensor(n) else float(n)
        self.state[0].copy_(v)
        self.state[1].add_(v * n)
        self.state[2].add_(n)

    @torch.no_grad()
    def update_norm(self, norm: torch.Tensor):
        v = norm.detach().to(torch.float64)
        self.state[3].copy_(v)
        self.state[4].add_(v)
        self.state[5].add_(1.0)
        self.state[6].add_((~torch.isfinite(v)).to(torch.float64))

    def values(self) -> dict:
        """{'loss': MeterValue(val, avg), 'grad_norm': MeterValue(val, avg), 'nonfinite': int} of this rank: one host copy."""
        h = self.state.tolist()
        return {'loss': MeterValue(h[0], h[1] / h[2] if h[2] else 0.0), 'grad_norm': MeterValue(h[3], h[4] / h[5] if h[5] else 0.0),
                'nonfinite': int(h[6])}

    def all_reduce(self, group=None) -> float:
        """``AverageMeter.all_reduce`` of the loss meter (misc/utils.py:293-303): an fp32 [sum, count] SUM all-reduce (the rounding
        to fp32 happens at world size 1 too, as it does there); returns the average ``train_one_epoch`` returns."""
        total = self.state[1:3].to(torch.float32)
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(total, op=dist.ReduceOp.SUM, group=group)
        s, count = total.tolist()
        if not count:
            raise ValueError('no training step was metered before all_reduce')
        return s / count


class TrainStep:
    """forward (autocast) -> BCE-with-logits / accumulation_steps -> backward -> flat all-reduce -> clip 5.0 ->
    optimizer step -> lr_scheduler.step_update -> zero   (misc/engine.py:202-231).

    * ``accumulation_steps`` > 1: gradients accumulate in the flat buffer over that many calls and the
      exchange / clip / update happen on the last one (the reference all-reduces on every micro-step because
      it never uses ``no_sync()``; the mean of sums is the same number).
    * The exchange is split in two buckets: the decoder-only gradients are all-reduced while the encoder's
      backward still runs (``overlap=True``; needs a model with the reference's 3-way forward), the rest
      after it.  The backward is driven in two stages for that: decoder + head first, then the encoder from
      the gradient of the features.
    * ``num_updates`` (the index handed to ``lr_scheduler.step_update``) counts iterations, whether or not an optimizer built
      with ``skip_nonfinite=True`` left an update out - the reference's index does the same; ``optimizer.num_updates`` counts
      the updates that were applied.
    * ``meters=True`` keeps the loop's loss and gradient-norm meters (``TrainMeters``) on the device, eagerly and in replay,
      without a host read; what ``step`` returns does not change.
    * ``use_graph=True`` replays hipGraphs (forward + decoder backward | encoder backward | update) captured
      after two eager warm-up steps, with the RCCL all-reduces issued between the replays, so the ~900
      launches of a step cost three graph launches on the host.  The learning rate lives in a device scalar,
      so ``lr_scheduler.step_update`` / ``set_lr`` take effect in the replayed update.
    * Stochastic depth (a model built with ``drop_path_rate`` > 0, in training mode): every step draws its scales inside the
      model's forward.  Under ``use_graph`` the draw is part of the captured graph and uses the device's default generator,
      which torch registers with the graph: every replay draws anew, and ``model.last_drop_path`` is a static buffer that holds
      the latest replay's scales.  A custom ``model.drop_path_generator`` raises at capture.  ``step.drop_path`` = a
      ``DropPathScales`` of static tensors forces the scales instead (tests, reproducing a step): a captured graph reads those
      tensors in place."""

    def __init__(self, model, optimizer, *, clip_grad=5.0, amp=True, criterion=None, use_graph=False,
                 compress_bf16=False, forward_fn=None, accumulation_steps=1, lr_scheduler=None, overlap=True, group=None,
                 start_update=0, meters=False):
        self.model, self.optimizer, self.clip_grad, self.amp = model, optimizer, clip_grad, amp
        self.criterion = criterion or torch.nn.BCEWithLogitsLoss()
        self.accum = max(int(accumulation_steps), 1)
        self.lr_scheduler, self.group = lr_scheduler, group
        self.split = bool(overlap) and forward_fn is None and hasattr(model, 'cross_blocks')
        self.flat = FlatGradients(model.parameters(), compress_bf16=compress_bf16,
                                  early=_decoder_only_parameters(model) if self.split else None)
        if hasattr(model, 'direct_param_grads') or hasattr(model, 'runtime'):
            model.direct_param_grads = True     # HIP model: weight-gradient kernels add straight into the flat buffer
        self.drop_path = None       # forced stochastic-depth scales (a DropPathScales); None: the model draws when it should
        self.forward_fn = forward_fn or (lambda m, x: m(x) if self.drop_path is None else m(x, drop_path=self.drop_path))
        self.use_graph = use_graph and torch.cuda.is_available()
        self.hip_opt = hasattr(optimizer, 'bind_flat')       # optim.FlatAdamW / FlatSGD: clip + update + shadow refresh in one kernel
        if self.hip_opt:
            optimizer.bind_flat(self.flat, model)
        elif self.use_graph:
            bad = [g for g in optimizer.param_groups if not g.get('capturable', False)]
            if bad:
                raise ValueError('TrainStep(use_graph=True) captures optimizer.step() into a hipGraph: build the torch optimizer with '
                                 'capturable=True (engine.build_optimizer(config, model, capturable=True)) or use optim.FlatAdamW / optim.FlatSGD')
        self._g1 = self._g2 = self._g_opt = None
        self._opt_signature = None
        self.recaptures = 0
        self._static_x = self._static_y = self._static_loss = self._static_norm = None
        self._eager_steps = 0
        self._micro = 0
        # updates done before this TrainStep existed: a resumed run passes epoch * num_steps // accumulation_steps so that the
        # per-iteration schedule continues where it stopped (misc/engine.py:228 counts from the start of training)
        self.num_updates = int(start_update)
        self.last_norm = None
        self._lr_tensors = None
        # a torch optimizer built with capturable=True reads its learning rate from a device scalar: keep it there in eager
        # mode too, so eager and replayed updates see the same (fp32) value
        self._tensor_lr = (not self.hip_opt) and all(g.get('capturable', False) for g in optimizer.param_groups) \
            and next(model.parameters()).is_cuda
        self.device_type = 'cuda' if next(model.parameters()).is_cuda else 'cpu'
        # meters=True: the loop's loss / grad-norm meters on the device (read them with ``meters.values()`` when a log line is due)
        self.meters = TrainMeters(next(model.parameters()).device, self.accum) if meters else None

    # -- learning rate -----------------------------------------------------------------------
    def set_lr(self, lr: float, group_index: int | None = None):
        """Per-iteration LR (misc/engine.py:228 ``lr_scheduler.step_update``): takes effect in eager and replayed updates."""
        for i, g in enumerate(self.optimizer.param_groups):
            if group_index is None or i == group_index:
                g['lr'] = float(lr) * g.get('lr_scale', 1.0)
        self._sync_lr()

    def _sync_lr(self):
        """Schedulers write Python floats into ``param_groups[i]['lr']``; a captured update reads a device scalar.
        Fold the floats into the per-group device tensors (torch optimizers: the tensors ARE ``group['lr']``)."""
        if self.hip_opt:
            self.optimizer.sync_hyperparameters()
            return
        if not self._tensor_lr:
            return
        if self._lr_tensors is None:
            dev = next(self.model.parameters()).device
            self._lr_tensors = [torch.tensor(float(g['lr']), dtype=torch.float32, device=dev) for g in self.optimizer.param_groups]
        for g, t in zip(self.optimizer.param_groups, self._lr_tensors):
            if g['lr'] is not t:
                t.fill_(float(g['lr']))
                g['lr'] = t

    # -- pieces ------------------------------------------------------------------------------
    def _loss(self, out, y):
        loss = self.criterion(out.float(), y)
        return loss / self.accum if self.accum > 1 else loss

    def _fwd_bwd(self, x, y):
        """One-stage form (any model / forward_fn)."""
        with torch.autocast(self.device_type, dtype=torch.bfloat16, enabled=self.amp):
            out = self.forward_fn(self.model, x)
            loss = self._loss(out, y)
        loss.backward()
        return loss.detach()

    def _fwd_dec_bwd(self, x, y):
        """Stage 1 of the split backward: encoder forward, decoder + head forward, loss, decoder backward.
        Returns (loss, features, d loss / d features)."""
        with torch.autocast(self.device_type, dtype=torch.bfloat16, enabled=self.amp):
            forced = {} if self.drop_path is None else dict(drop_path=self.drop_path)
            feats = self.model(x[:, 0], forward_first_part=True, **forced)
            leaf = feats.detach().requires_grad_(True)
            out = self.model(leaf, x[:, 1], **forced)
            loss = self._loss(out, y)
        loss.backward()
        return loss.detach(), feats, leaf.grad

    @staticmethod
    def _enc_bwd(feats, dfeats):
        feats.backward(dfeats)

    def _meter_loss(self, loss, y):
        if self.meters is not None:
            self.meters.update_loss(loss, y.counts[3] if hasattr(y, 'counts') else y.shape[0])    # MinedPairs: the real pairs

    def _update(self):
        if self.hip_opt:
            norm = self.optimizer.step_flat(self.clip_grad)      # clip + update + shadow refresh + zero: one pass
        else:
            norm = self.flat.clip_(self.clip_grad) if self.clip_grad is not None else torch.linalg.vector_norm(self.flat.flat)
            self.optimizer.step()
            self._refresh_shadows()       # the bf16 weight shadows follow the update (eval right after training sees them)
            self.flat.zero()
        return norm

    def _refresh_shadows(self):
        rts = getattr(self.model, '_runtimes', None)
        if rts:
            params = list(self.model.parameters())
            for rt in rts.values():
                rt.refresh_shadows(params)

    def _after_update(self):
        # misc/engine.py:228: lr_scheduler.step_update((epoch * num_steps + idx) // ACCUMULATION_STEPS) runs AFTER the update of
        # iteration idx with the count of updates done BEFORE it: 0, 1, 2, ...
        if self.lr_scheduler is not None:
            self.lr_scheduler.step_update(self.num_updates)
        self.num_updates += 1

    # -- public ------------------------------------------------------------------------------
    def step(self, x, y):
        """One call of the loop body.  Returns the (micro-batch) loss; ``last_norm`` holds the gradient norm of the
        last update."""
        last = (self._micro + 1) % self.accum == 0
        self._micro += 1
        if (self._g1 is not None and self.hip_opt and (self._micro - 1) % self.accum == 0
                and self.optimizer.shadow_signature() != self._opt_signature):
            # a bf16 weight shadow was re-created (or added) after capture: the captured forward / backward graphs read the old
            # buffers and the captured update refreshes the old set.  Drop every graph; this cycle runs eagerly, the next re-captures.
            torch.cuda.synchronize()
            self._g1 = self._g2 = self._g_opt = None
            self._eager_steps = 2 * self.accum - self.accum
            self.recaptures += 1
        if self.use_graph and self._g1 is None and self._eager_steps >= 2 * self.accum and (self._micro - 1) % self.accum == 0:
            self._capture(x, y)     # at the start of an accumulation cycle, after two eager updates: the flat buffer is zero
        if self._g1 is None:
            if self.use_graph:             # warm up allocator, workspaces and weight shadows eagerly
                self._eager_steps += 1
            return self._eager(x, y, last)
        self._static_x.copy_(x, non_blocking=True)
        self._static_y.copy_(y, non_blocking=True)
        buckets = self.flat.buckets()
        self._g1.replay()
        if self._g2 is not None:
            if last and len(buckets) == 2:
                self.flat.start_all_reduce(*buckets[0], group=self.group)   # runs under the encoder's backward
            self._g2.replay()
        if last:
            if self._g2 is not None and len(buckets) == 2:
                self.flat.start_all_reduce(*buckets[1], group=self.group)
            else:
                self.flat.start_all_reduce(0, self.flat.flat.numel(), group=self.group)
            self.flat.finish_all_reduce()
            self._sync_lr()
            self._g_opt.replay()
            self.last_norm = self._static_norm
            self._after_update()
        return self._static_loss

    def _eager(self, x, y, last):
        buckets = self.flat.buckets()
        if self.split and torch.is_tensor(x) and x.dim() == 5:
            loss, feats, dfeats = self._fwd_dec_bwd(x, y)
            if last and len(buckets) == 2:
                self.flat.start_all_reduce(*buckets[0], group=self.group)
            self._enc_bwd(feats, dfeats)
            if last:
                if len(buckets) == 2:
                    self.flat.start_all_reduce(*buckets[1], group=self.group)
                else:
                    self.flat.start_all_reduce(0, self.flat.flat.numel(), group=self.group)
        else:
            loss = self._fwd_bwd(x, y)
            if last:
                self.flat.start_all_reduce(0, self.flat.flat.numel(), group=self.group)
        self._meter_loss(loss, y)
        if last:
            self.flat.finish_all_reduce()
            self._sync_lr()
            self.last_norm = self._update()
            if self.meters is not None:
                self.meters.update_norm(self.last_norm)
            self._after_update()
        return loss

    def _capture(self, x, y):
        from . import ops
        if not torch.is_tensor(x):
            raise TypeError('TrainStep(use_graph=True) replays on a static input tensor: pass use_graph=False for structured batches')
        self._static_x, self._static_y = x.clone(), y.clone()
        self._sync_lr()
        torch.cuda.synchronize()
        ops.pin_workspace()               # captured kernels bake buffer addresses in: later growth must not free them
        for rt in getattr(self.model, '_runtimes', {}).values():
            rt.pinned = True
        split = self.split and torch.is_tensor(x) and x.dim() == 5
        self._g1 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._g1, capture_error_mode=_CAPTURE_MODE):
            if split:
                self._static_loss, self._feats, self._dfeats = self._fwd_dec_bwd(self._static_x, self._static_y)
            else:
                self._static_loss = self._fwd_bwd(self._static_x, self._static_y)
            self._meter_loss(self._static_loss, self._static_y)      # part of the replayed graph
        if split:
            self._g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._g2, pool=self._g1.pool(), capture_error_mode=_CAPTURE_MODE):
                self._enc_bwd(self._feats, self._dfeats)
        self._capture_update()

    def _capture_update(self):
        """(Re-)capture the update graph.  Its kernels bake in the optimizer's descriptor table, i.e. the set of weight-shadow
        buffers to refresh; ``step`` compares that set before every replay."""
        torch.cuda.synchronize()
        if self.hip_opt:
            self.optimizer._descriptors()          # build the table outside the capture
            self._opt_signature = self.optimizer.shadow_signature()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=self._g1.pool(), capture_error_mode=_CAPTURE_MODE):
            norm = self._update()
            if self.meters is not None:
                self.meters.update_norm(norm)
        if self._static_norm is None:
            self._static_norm = norm
        elif norm.data_ptr() != self._static_norm.data_ptr():
            self._static_norm = norm
        self._g_opt = g


# ---------------------------------------------------------------------------------------------
# input pipeline: host -> HBM one batch ahead (misc/engine.py:202-204)
# ---------------------------------------------------------------------------------------------
class DevicePrefetcher:
    """Wraps a loader of (samples, targets) CPU batches.  The reference copies every batch on the compute stream at the top of
    the iteration (``samples.cuda(non_blocking=True)``, misc/engine.py:203-204) as fp32.  Here the batch is staged in pinned host
    memory and copied on a side stream ``depth`` batches ahead of the step that consumes it, and uint8 images stay uint8 all the
    way into the patch-embedding kernel (``vited_patchify_u8`` applies ToTensor + Normalize), so a config-A batch of 1024 pairs
    is 25 MB on PCIe instead of 101 MB.  Yields device tensors; iteration order and contents equal the wrapped loader's."""

    def __init__(self, loader, device, depth: int = 2):
        self.loader, self.device, self.depth = loader, torch.device(device), max(int(depth), 1)
        self.stream = torch.cuda.Stream(device=self.device) if self.device.type == 'cuda' else None
        self._pinned = {}

    def __len__(self):
        return len(self.loader)

    def _stage(self, t, slot, name):
        """CPU tensor -> device tensor through a reusable pinned buffer (per ring slot), on the copy stream."""
        if not torch.is_tensor(t):
            return t
        if self.stream is None:
            return t.to(self.device)
        key = (slot, name, tuple(t.shape), t.dtype)
        ent = self._pinned.get(key)
        if ent is None:
            ent = self._pinned[key] = [torch.empty(t.shape, dtype=t.dtype).pin_memory(), None]
        buf, ev = ent
        if ev is not None:
            ev.synchronize()               # the previous H2D copy out of this pinned slot must have executed before it is rewritten
        buf.copy_(t)
        out = buf.to(self.device, non_blocking=True)
        ent[1] = torch.cuda.Event()
        ent[1].record(self.stream)
        return out

    def __iter__(self):
        import collections
        queue = collections.deque()
        slot = 0
        for batch in self.loader:
            samples, targets = batch
            if self.stream is not None:
                with torch.cuda.stream(self.stream):
                    item = (self._stage(samples, slot, 'x'), self._stage(targets, slot, 'y'))
                    ev = torch.cuda.Event()
                    ev.record(self.stream)
            else:
                item, ev = (self._stage(samples, slot, 'x'), self._stage(targets, slot, 'y')), None
            queue.append((item, ev))
            slot = (slot + 1) % (self.depth + 1)          # a pinned buffer is rewritten only after its batch was handed out
            if len(queue) > self.depth:
                yield self._hand_out(*queue.popleft())
        while queue:
            yield self._hand_out(*queue.popleft())

    def _hand_out(self, item, ev):
        if ev is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)                              # the consumer's stream waits for the copy, the host does not
            for t in item:
                if torch.is_tensor(t):
                    t.record_stream(cur)
        return item


# ---------------------------------------------------------------------------------------------
# patch-pair assembly on the device (data/datasets/div2k_patch.py:108-162)
# ---------------------------------------------------------------------------------------------
def div2k_pair_plan(u: torch.Tensor, img_size: int, erosion_ratio: float, with_negative: bool = True, train: bool = True):
    """The random choices of ``DIV2KPatch.__getitem__`` (div2k_patch.py:114-153) for a whole batch at once, from uniform numbers
    ``u`` [B, 4] in [0, 1) (columns: negative-pair draw, first swap, second swap, erosion):
      cells  int32 [B, 2]   grid cells (3 columns x 2 rows, row-major) of image 1 and image 2
      labels fp32  [B, 4]   the 4-bin target (all-zero for the 30 % negatives)
      erode  int32 [B]      eroded cell size e = ceil(S (1 - r)), r ~ U(erosion_ratio, 2 erosion_ratio) in training
    first = cell 0, second = 1 (right of it), third = 4 (below second), fourth = 3 (below first), spare = 2."""
    dev = u.device
    a, b = u[:, 1] > 0.5, u[:, 2] > 0.5
    neg = (u[:, 0] < 0.3) if with_negative else torch.zeros_like(a)
    second = torch.where(neg, torch.where(a, 4, 2), torch.where(a, 3, 1))      # negative: third / spare; positive: fourth / second
    first = torch.zeros_like(second)
    img1 = torch.where(b, second, first)
    img2 = torch.where(b, first, second)
    cells = torch.stack([img1, img2], dim=1).to(torch.int32)
    bin_ = a.long() + 2 * b.long()                                              # (a, b) -> label bin 0, 1, 2, 3
    labels = torch.nn.functional.one_hot(bin_, 4).float() * (~neg).float().unsqueeze(1)
    r = erosion_ratio * (1.0 + u[:, 3].double()) if train else torch.full_like(u[:, 3], erosion_ratio, dtype=torch.float64)
    erode = torch.ceil(img_size * (1.0 - r)).to(torch.int32).clamp_(1, img_size)
    return cells.contiguous(), labels.to(dev), erode.contiguous()


def assemble_pairs(regions_u8: torch.Tensor, cells: torch.Tensor, erode: torch.Tensor, img_size: int) -> torch.Tensor:
    """uint8 regions [B, C, 2 S, 3 S] on the device -> uint8 pairs [B, 2, C, S, S]: erosion crop + Pillow-exact bilinear resize of
    the two chosen cells in one kernel (``vited_crop_pairs_u8``).  Feed the result straight to the model: ToTensor + Normalize
    are folded into the patch-embedding kernel."""
    from . import ops
    return ops.crop_pairs_u8(regions_u8, cells, erode, img_size)


# ---------------------------------------------------------------------------------------------
# the stage in front of it on the device too: resident images, augmentation and crop (div2k_patch.py:84-111)
# ---------------------------------------------------------------------------------------------
class Div2kImageStore:
    """The decoded images of a DIV2K split, resident on ``device``: ``images`` (HWC uint8 arrays or tensors, 3 channels) packed
    back to back into one uint8 buffer (``data``), with their byte offsets and (H, W) sizes on the device (``offsets_dev`` int64
    [n], ``sizes_dev`` int32 [n, 2]) and on the host (``offsets``, ``sizes``).  DIV2K train is about 7 GB this way."""

    def __init__(self, images, device):
        self.device = torch.device(device)
        flat, sizes, offsets, off = [], [], [], 0
        for k, im in enumerate(images):
            t = torch.as_tensor(im)
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
                raise ValueError(f'image {k}: expected a uint8 [H, W, 3] array, got {t.dtype} {tuple(t.shape)}')
            flat.append(t.contiguous().reshape(-1))
            sizes.append([t.shape[0], t.shape[1]])
            offsets.append(off)
            off += t.numel()
        if not flat:
            raise ValueError('an image store needs at least one image')
        self.sizes = torch.tensor(sizes, dtype=torch.int32)
        self.offsets = torch.tensor(offsets, dtype=torch.int64)
        self.data = torch.empty(off, dtype=torch.uint8, device=self.device)
        for t, o in zip(flat, offsets):                    # image by image: no second host copy of the whole set
            self.data[o: o + t.numel()].copy_(t)
        self.sizes_dev, self.offsets_dev = self.sizes.to(self.device), self.offsets.to(self.device)

    def __len__(self):
        return self.sizes.shape[0]

    def require_window(self, img_size: int):
        """Every image must hold the (2 S) x (3 S) window the crop keeps (torchvision's crops raise or pad otherwise)."""
        small = ((self.sizes[:, 0] < 2 * img_size) | (self.sizes[:, 1] < 3 * img_size)).nonzero().flatten().tolist()
        if small:
            k = small[0]
            raise ValueError(f'{len(small)} image(s) are smaller than the {2 * img_size} x {3 * img_size} crop window, the first is '
                             f'image {k} with {int(self.sizes[k, 0])} x {int(self.sizes[k, 1])}')


def div2k_augment_plan(u: torch.Tensor, image: torch.Tensor, sizes: torch.Tensor, img_size: int, train: bool = True):
    """The random choices of ``DIV2KPatch.read_image`` and of the crop of ``__getitem__`` (div2k_patch.py:89-111) for a whole batch at
    once, from uniform numbers ``u`` [B, 13] in [0, 1) (columns: horizontal flip, vertical flip, warp, angle, scale, dx, dy, colour
    shift, its three channel shifts, crop top, crop left), the image indices ``image`` [B] and ``sizes`` int32 [n, 2] = (H, W):
      image int32 [B]      the indices
      flags int32 [B]      bit 0 / 1: RandomHorizontalFlip / RandomVerticalFlip (p = 0.5); bit 2: A.ShiftScaleRotate (p = 0.5);
                           bit 3: A.RGBShift (p = 0.5)
      minv  fp64  [B, 6]   inverse of  getRotationMatrix2D((W / 2 - 0.5, H / 2 - 0.5), angle ~ U(-20, 20), scale ~ U(0.85, 1.15))
                           + (dx W, dy H), dx, dy ~ U(-0.05, 0.05), inverted as cv2.warpAffine does; the identity with the warp off
      rgb   fp32  [B, 3]   channel shifts ~ U(-15, 15); 0 with the colour shift off
      crop  int32 [B, 2]   RandomCrop origin floor(u (H - 2 S + 1)), floor(u (W - 3 S + 1))
    ``train=False``: no augmentation and CenterCrop's origin int(round((H - 2 S) / 2)) (round half to even).  Elementwise torch
    operations on the device of ``u``: no host copy, no sync; every fp64 product and sum is an operation of its own."""
    u = u.double()
    n_rows = u.shape[0]
    image = image.to(device=u.device, dtype=torch.int64)
    hw = sizes.to(u.device)[image.clamp(0, sizes.shape[0] - 1)]
    H, W = hw[:, 0].double(), hw[:, 1].double()
    room_y, room_x = (H - 2 * img_size).clamp_(min=0), (W - 3 * img_size).clamp_(min=0)
    zero, one = torch.zeros_like(H), torch.ones_like(H)
    if not train:
        flags = torch.zeros(n_rows, dtype=torch.int32, device=u.device)
        minv = torch.stack([one, zero, zero, zero, one, zero], dim=1)
        rgb = torch.zeros(n_rows, 3, dtype=torch.float32, device=u.device)
        crop = torch.stack([torch.round(room_y / 2), torch.round(room_x / 2)], dim=1).to(torch.int32)
        return image.to(torch.int32), flags, minv.contiguous(), rgb, crop.contiguous()
    hflip, vflip, warp, colour = u[:, 0] < 0.5, u[:, 1] < 0.5, u[:, 2] < 0.5, u[:, 7] < 0.5
    flags = (hflip.int() + 2 * vflip.int() + 4 * warp.int() + 8 * colour.int()).to(torch.int32)
    angle = (u[:, 3] * 40.0 - 20.0) * (torch.pi / 180.0)
    scale = u[:, 4] * 0.3 + 0.85
    dx, dy = (u[:, 5] * 0.1 - 0.05) * W, (u[:, 6] * 0.1 - 0.05) * H
    cx, cy = W / 2 - 0.5, H / 2 - 0.5
    alpha, beta = torch.cos(angle) * scale, torch.sin(angle) * scale
    m0, m1, m2 = alpha, beta, (1 - alpha) * cx - beta * cy + dx            # cv2.getRotationMatrix2D, then the translation
    m3, m4, m5 = -beta, alpha, beta * cx + (1 - alpha) * cy + dy
    det = m0 * m4 - m1 * m3                                                 # cv2.warpAffine without WARP_INVERSE_MAP
    d = torch.where(det != 0, 1.0 / det, zero)
    i0, i1, i3, i4 = m4 * d, m1 * (-d), m3 * (-d), m0 * d
    i2, i5 = -(i0 * m2) - i1 * m5, -(i3 * m2) - i4 * m5
    minv = torch.stack([torch.where(warp, a, b) for a, b in zip((i0, i1, i2, i3, i4, i5), (one, zero, zero, zero, one, zero))], dim=1)
    rgb = ((u[:, 8:11] * 30.0 - 15.0) * colour.unsqueeze(1)).float()
    crop = torch.stack([torch.minimum(torch.floor(u[:, 11] * (room_y + 1)), room_y),
                        torch.minimum(torch.floor(u[:, 12] * (room_x + 1)), room_x)], dim=1).to(torch.int32)
    return image.to(torch.int32), flags, minv.contiguous(), rgb.contiguous(), crop.contiguous()


class Div2kDeviceLoader:
    """The DIV2K pair loader on the device: what ``build_loader`` + ``DIV2KPatch`` + ``DevicePrefetcher`` deliver, from a
    ``Div2kImageStore``, without a host copy or a sync per batch.  An epoch is a permutation (drawn on the device, the same on
    every rank) of the image indices repeated ``repeat`` times, of which rank r takes every ``world``-th from r on; the last
    incomplete batch is dropped.  Each batch: uniforms -> ``div2k_augment_plan`` -> ``ops.div2k_regions_u8`` -> ``div2k_pair_plan``
    -> ``assemble_pairs``; it yields (pairs uint8 [B, 2, 3, S, S], labels fp32 [B, 4]) for ``TrainStep.step``."""

    def __init__(self, store: Div2kImageStore, batch_size: int, img_size: int, erosion_ratio: float, with_negative: bool = True,
                 train: bool = True, repeat: int = 5, rank: int = 0, world: int = 1, seed: int = 0):
        store.require_window(img_size)
        if not 0 <= rank < world:
            raise ValueError(f'rank {rank} outside a world of {world}')
        self.store, self.batch_size, self.img_size, self.erosion_ratio = store, int(batch_size), int(img_size), float(erosion_ratio)
        self.with_negative, self.train, self.repeat, self.rank, self.world, self.seed = with_negative, train, int(repeat), rank, world, seed
        self.epoch = 0
        if len(self) < 1:
            raise ValueError(f'{len(store)} images x {repeat} over {world} rank(s) do not fill one batch of {batch_size}')

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.store) * self.repeat // self.world // self.batch_size

    def _generator(self, stream: int):
        g = torch.Generator(device=self.store.device)
        g.manual_seed((self.seed * 1000003 + self.epoch) * 4099 + stream)
        return g

    def epoch_order(self) -> torch.Tensor:
        """The epoch's permutation of the repeated image indices (int64 on the store's device), before sharding."""
        n = len(self.store)
        return torch.randperm(n * self.repeat, generator=self._generator(0), device=self.store.device) % n

    def rank_indices(self) -> torch.Tensor:
        """[len(self), batch_size]: the image index of every sample this rank sees in the epoch."""
        per_rank = len(self.store) * self.repeat // self.world
        mine = self.epoch_order()[self.rank::self.world][:per_rank]
        return mine[: len(self) * self.batch_size].view(len(self), self.batch_size)

    def plan(self, image: torch.Tensor, generator: torch.Generator):
        """One batch's draws: (the five tensors of ``div2k_augment_plan``, the three of ``div2k_pair_plan``)."""
        u = torch.rand(image.numel(), 17, generator=generator, device=self.store.device)
        return (div2k_augment_plan(u[:, :13], image, self.store.sizes_dev, self.img_size, self.train),
                div2k_pair_plan(u[:, 13:], self.img_size, self.erosion_ratio, self.with_negative, self.train))

    def __iter__(self):
        from . import ops
        g = self._generator(1 + self.rank)
        for image in self.rank_indices():
            (idx, flags, minv, rgb, crop), (cells, labels, erode) = self.plan(image, g)
            regions = ops.div2k_regions_u8(self.store.data, self.store.offsets_dev, self.store.sizes_dev, idx, flags, minv, rgb, crop,
                                           self.img_size)
            yield assemble_pairs(regions, cells, erode, self.img_size), labels


# ---------------------------------------------------------------------------------------------
# config H's input pipeline on the device: RandomAffine, ShiftScaleRotate, RandomCrop, ColorJitter, GaussianBlur (hisfrag.py:63-115;
# DESIGN.md section 17)
# ---------------------------------------------------------------------------------------------
HISFRAG_PLAN_COLUMNS = 21


class HisfragPlan(NamedTuple):
    """One batch's per-sample arguments of ``ops.hisfrag_windows_u8`` / ``hisfrag_jitter_u8`` / ``hisfrag_blur_u8``."""
    image: torch.Tensor      # int32 [B]     image index
    flags: torch.Tensor      # int32 [B]     bit 0 RandomAffine, bit 1 ShiftScaleRotate, bit 2 ColorJitter, bit 3 GaussianBlur
    afix: torch.Tensor       # int64 [B, 6]  Pillow's 16.16 coefficients a0..a5 of the RandomAffine matrix
    minv: torch.Tensor       # fp64  [B, 6]  inverse ShiftScaleRotate matrix
    origin: torch.Tensor     # int32 [B, 2]  (top, left) of the window in unpadded image coordinates
    order: torch.Tensor      # int32 [B, 4]  jitter operations in the order they run (0 brightness, 1 contrast, 2 saturation, 3 hue)
    factors: torch.Tensor    # fp32  [B, 3]  brightness, contrast, saturation factors
    hue: torch.Tensor        # int32 [B]     the uint8 added to H
    blur: torch.Tensor       # fp32  [B, 2]  (k_edge, k_mid) of the 3-tap Gaussian


def hisfrag_augment_plan(u: torch.Tensor, image: torch.Tensor, sizes: torch.Tensor, img_size: int, train: bool = True) -> HisfragPlan:
    """The random choices of ``HisfragTrainer.get_transforms`` (hisfrag.py:66-78) for a whole batch at once, from uniform numbers
    ``u`` [B, 21] in [0, 1), the image indices ``image`` [B] and ``sizes`` int32 [n, 2] = (H, W).  Columns of ``u``:
      0-2    RandomAffine(5, translate=(0.1, 0.1)): angle ~ U(-5, 5), tx = round(U(-0.1 W, 0.1 W)), ty likewise (half to even);
             the matrix is torchvision's _get_inverse_affine_matrix about (0.5 W, 0.5 H), its 16.16 form Pillow's FIX
      3-7    A.ShiftScaleRotate at p = 0.5: angle ~ U(-10, 10), scale ~ U(0.9, 1.1), dx, dy ~ U(-0.05, 0.05) of W, H; the forward
             matrix and its inversion as in ``div2k_augment_plan``
      8-9    RandomCrop(S, pad_if_needed=True): origin floor(u (Hp - S + 1)) - pad, pad = max(S - H, 0), Hp = H + 2 pad
      10-18  ColorJitter(0.3, 0.3, 0.3, 0.3) at p = 0.5: the order is the argsort of four uniforms, brightness / contrast /
             saturation ~ U(0.7, 1.3), hue ~ U(-0.3, 0.3) as the uint8 shift trunc(hue 255) mod 256
      19-20  GaussianBlur((3, 3), (1, 2)) at p = 0.5: sigma ~ U(1, 2), e = exp(-0.5 / sigma^2) rounded to fp32 once, then
             k_edge = e / (e + 1 + e), k_mid = 1 / (e + 1 + e) in fp32
    ``train=False``: everything off and CenterCrop's origin (round half to even; torchvision's centre padding for an image smaller
    than S).  Elementwise torch operations on the device of ``u``: no host copy, no sync; fp64 throughout, every product and sum
    an operation of its own."""
    u = u.double()
    n_rows, dev, S = u.shape[0], u.device, int(img_size)
    image = image.to(device=dev, dtype=torch.int64)
    hw = sizes.to(dev)[image.clamp(0, sizes.shape[0] - 1)]
    H, W = hw[:, 0].double(), hw[:, 1].double()
    zero, one = torch.zeros_like(H), torch.ones_like(H)
    ident = torch.stack([one, zero, zero, zero, one, zero], dim=1)
    ident_fix = torch.tensor([65536, 0, 32768, 0, 65536, 32768], dtype=torch.int64, device=dev).expand(n_rows, 6)
    natural = torch.arange(4, dtype=torch.int32, device=dev).expand(n_rows, 4)
    no_blur = torch.tensor([0.0, 1.0], dtype=torch.float32, device=dev).expand(n_rows, 2)
    if not train:
        centre = lambda n: torch.where(n >= S, torch.round((n - S) / 2), -torch.floor((S - n) / 2))
        return HisfragPlan(image.to(torch.int32), torch.zeros(n_rows, dtype=torch.int32, device=dev), ident_fix.contiguous(), ident.contiguous(),
                           torch.stack([centre(H), centre(W)], dim=1).to(torch.int32).contiguous(), natural.contiguous(),
                           torch.ones(n_rows, 3, dtype=torch.float32, device=dev), torch.zeros(n_rows, dtype=torch.int32, device=dev),
                           no_blur.contiguous())
    warp, jitter, blur_on = u[:, 3] < 0.5, u[:, 10] < 0.5, u[:, 19] < 0.5
    flags = (1 + 2 * warp.int() + 4 * jitter.int() + 8 * blur_on.int()).to(torch.int32)
    # RandomAffine
    rot = (u[:, 0] * 10.0 - 5.0) * (torch.pi / 180.0)
    tx, ty = torch.round((u[:, 1] * 2.0 - 1.0) * (0.1 * W)), torch.round((u[:, 2] * 2.0 - 1.0) * (0.1 * H))
    cx, cy = W * 0.5, H * 0.5
    cos, sin = torch.cos(rot), torch.sin(rot)
    M0, M1, M3, M4 = cos, sin, -sin, cos
    M2 = (M0 * (-cx - tx) + M1 * (-cy - ty)) + cx
    M5 = (M3 * (-cx - tx) + M4 * (-cy - ty)) + cy
    fix = lambda t: torch.floor(t * 65536.0 + 0.5).to(torch.int64)
    afix = torch.stack([fix(M0), fix(M1), fix(M2 + M0 * 0.5 + M1 * 0.5), fix(M3), fix(M4), fix(M5 + M3 * 0.5 + M4 * 0.5)], dim=1)
    # ShiftScaleRotate
    angle = (u[:, 4] * 20.0 - 10.0) * (torch.pi / 180.0)
    scale = u[:, 5] * 0.2 + 0.9
    dx, dy = (u[:, 6] * 0.1 - 0.05) * W, (u[:, 7] * 0.1 - 0.05) * H
    wx, wy = W / 2 - 0.5, H / 2 - 0.5
    alpha, beta = torch.cos(angle) * scale, torch.sin(angle) * scale
    m0, m1, m2 = alpha, beta, (1 - alpha) * wx - beta * wy + dx
    m3, m4, m5 = -beta, alpha, beta * wx + (1 - alpha) * wy + dy
    det = m0 * m4 - m1 * m3
    d = torch.where(det != 0, 1.0 / det, zero)
    i0, i1, i3, i4 = m4 * d, m1 * (-d), m3 * (-d), m0 * d
    i2, i5 = -(i0 * m2) - i1 * m5, -(i3 * m2) - i4 * m5
    minv = torch.where(warp.unsqueeze(1), torch.stack([i0, i1, i2, i3, i4, i5], dim=1), ident)
    # RandomCrop with pad_if_needed
    pad_y, pad_x = (S - H).clamp_(min=0), (S - W).clamp_(min=0)
    room_y, room_x = H + 2 * pad_y - S, W + 2 * pad_x - S
    origin = torch.stack([torch.minimum(torch.floor(u[:, 8] * (room_y + 1)), room_y) - pad_y,
                          torch.minimum(torch.floor(u[:, 9] * (room_x + 1)), room_x) - pad_x], dim=1).to(torch.int32)
    # ColorJitter
    order = torch.where(jitter.unsqueeze(1), torch.argsort(u[:, 11:15], dim=1, stable=True).to(torch.int32), natural)
    factors = torch.where(jitter.unsqueeze(1), u[:, 15:18] * 0.6 + 0.7, one.unsqueeze(1)).float()
    hue = torch.where(jitter, torch.trunc((u[:, 18] * 0.6 - 0.3) * 255.0).to(torch.int64) % 256, 0).to(torch.int32)
    # GaussianBlur
    inv_sigma = 1.0 / (u[:, 20] + 1.0)
    e = torch.exp(-0.5 * (inv_sigma * inv_sigma)).float()
    den = (e + 1.0) + e
    blur = torch.where(blur_on.unsqueeze(1), torch.stack([e / den, 1.0 / den], dim=1), no_blur)
    return HisfragPlan(image.to(torch.int32), flags, afix.contiguous(), minv.contiguous(), origin.contiguous(), order.contiguous(),
                       factors.contiguous(), hue.contiguous(), blur.contiguous())


def hisfrag_feed(store: 'Div2kImageStore', plan: HisfragPlan, img_size: int) -> torch.Tensor:
    """``plan`` -> uint8 [B, 3, S, S] on the store's device: geometry, colour jitter and blur, three entry points back to back."""
    from . import ops
    windows = ops.hisfrag_windows_u8(store.data, store.offsets_dev, store.sizes_dev, plan.image, plan.flags, plan.afix, plan.minv,
                                     plan.origin, img_size)
    jittered = ops.hisfrag_jitter_u8(windows, plan.flags, plan.order, plan.factors, plan.hue, out=windows)     # pointwise: in place
    return ops.hisfrag_blur_u8(jittered, plan.flags, plan.blur)


class HisfragDeviceLoader:
    """Config H's training loader on the device: what ``HisfragTrainer.get_dataloader`` (hisfrag.py:101-115) delivers, from a
    ``Div2kImageStore`` of the decoded fragments and their writer ids ``labels``, without a host copy or a sync per batch.
    Sampling is ``MPerClassSampler(labels, m)``'s scheme: passes over a device-drawn permutation of the writers, ``m`` members
    per writer (a random order without repetition where the writer has at least ``m``, cycling through a random order of its
    members where it has fewer), passes concatenated and cut into batches.  Every rank draws from its own generator stream (the
    reference's sampler is not distributed either).  Each batch: uniforms -> ``hisfrag_augment_plan`` -> ``hisfrag_feed``; it yields
    (images uint8 [B, 3, S, S], targets int64 [B]) for ``hisfrag_prepare_data``.  Images smaller than the window are padded."""

    def __init__(self, store: Div2kImageStore, labels, batch_size: int, img_size: int, m: int = 3, train: bool = True, repeat: int = 1,
                 rank: int = 0, world: int = 1, seed: int = 0):
        if not 0 <= rank < world:
            raise ValueError(f'rank {rank} outside a world of {world}')
        labels = torch.as_tensor(labels).reshape(-1).to(torch.int64).cpu()
        if labels.numel() != len(store):
            raise ValueError(f'{labels.numel()} labels for {len(store)} images')
        if m < 1 or batch_size % m:
            raise ValueError(f'batch size {batch_size} is no multiple of m = {m}')
        self.store, self.batch_size, self.img_size, self.m = store, int(batch_size), int(img_size), int(m)
        self.train, self.repeat, self.rank, self.world, self.seed = train, int(repeat), rank, world, seed
        self.epoch = 0
        writers, member_of = torch.unique(labels, return_inverse=True)
        counts = torch.bincount(member_of, minlength=writers.numel())
        table = torch.zeros(writers.numel(), int(counts.max()), dtype=torch.int64)      # the writers' members, padded with 0
        for w in range(writers.numel()):
            table[w, : int(counts[w])] = (member_of == w).nonzero().flatten()
        dev = store.device
        self.labels_dev, self.members_dev, self.counts_dev = labels.to(dev), table.to(dev), counts.to(dev)
        if len(self) < 1:
            raise ValueError(f'{len(store)} images x {repeat} over {world} rank(s) do not fill one batch of {batch_size}')

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.store) * self.repeat // self.world // self.batch_size

    def _generator(self, stream: int):
        g = torch.Generator(device=self.store.device)
        g.manual_seed((self.seed * 1000003 + self.epoch) * 4099 + stream)
        return g

    def rank_indices(self) -> torch.Tensor:
        """[len(self), batch_size]: the image index of every sample this rank sees in the epoch (int64 on the store's device)."""
        dev, m = self.store.device, self.m
        n_writers, width = self.members_dev.shape
        need = len(self) * self.batch_size
        passes = -(-need // (n_writers * m))
        g = self._generator(2 * self.rank)
        writer = torch.stack([torch.randperm(n_writers, generator=g, device=dev) for _ in range(passes)])            # [passes, writers]
        keys = torch.rand(passes, n_writers, width, generator=g, device=dev)
        count = self.counts_dev[writer]                                                                              # [passes, writers]
        keys = torch.where(torch.arange(width, device=dev) < count.unsqueeze(2), keys, 2.0)                          # padding sorts last
        shuffled = torch.argsort(keys, dim=2)                                                # the real members first, in a random order
        take = torch.arange(m, device=dev).expand(passes, n_writers, m) % count.unsqueeze(2)
        picked = self.members_dev[writer.unsqueeze(2), shuffled.gather(2, take)]                                     # [passes, writers, m]
        return picked.reshape(-1)[:need].view(len(self), self.batch_size)

    def plan(self, image: torch.Tensor, generator: torch.Generator) -> HisfragPlan:
        """One batch's draws."""
        u = torch.rand(image.numel(), HISFRAG_PLAN_COLUMNS, generator=generator, device=self.store.device)
        return hisfrag_augment_plan(u, image, self.store.sizes_dev, self.img_size, self.train)

    def __iter__(self):
        g = self._generator(2 * self.rank + 1)
        for image in self.rank_indices():
            yield hisfrag_feed(self.store, self.plan(image, g), self.img_size), self.labels_dev[image]


# ---------------------------------------------------------------------------------------------
# michigan.py's input pipeline on the device: RandomCrop, RandomResizedCrop, CoarseDropout, flips, ColorJitter, Pillow's GaussianBlur,
# RandomGrayscale (michigan.py:68-101)
# ---------------------------------------------------------------------------------------------
MICHIGAN_PLAN_COLUMNS = 104
MICHIGAN_MAX_HOLES = 16
_RRC_ATTEMPTS = 10


class MichiganPlan(NamedTuple):
    """One batch's per-sample arguments of ``ops.michigan_windows_u8`` / ``hisfrag_jitter_u8`` / ``michigan_blur_gray_u8``."""
    image: torch.Tensor      # int32 [B]         image index
    flags: torch.Tensor      # int32 [B]         bit 0 dropout, 1 horizontal flip, 2 ColorJitter, 3 GaussianBlur, 4 vertical flip, 5 grey
    origin: torch.Tensor     # int32 [B, 2]      (top, left) of the window in unpadded image coordinates
    box: torch.Tensor        # int32 [B, 4]      RandomResizedCrop's (i, j, h, w) in the window (what the tap tables were made from)
    x0: torch.Tensor         # int32 [B, S]      first horizontal tap per output column, in window coordinates
    kx: torch.Tensor         # int32 [B, S, 3]   its 22-bit fixed-point weights
    y0: torch.Tensor         # int32 [B, S]      first vertical tap per output row
    ky: torch.Tensor         # int32 [B, S, 3]
    holes: torch.Tensor      # int32 [B, 16, 4]  (x1, y1, x2, y2), half-open, before the flips
    n_holes: torch.Tensor    # int32 [B]
    order: torch.Tensor      # int32 [B, 4]      jitter operations in the order they run (0 brightness, 1 contrast, 2 saturation, 3 hue)
    factors: torch.Tensor    # fp32  [B, 3]      brightness, contrast, saturation factors
    hue: torch.Tensor        # int32 [B]         the uint8 added to H
    blur: torch.Tensor       # int32 [B, 2]      (ww, fw) of Pillow's box blur


def _bilinear_taps(in_size: torch.Tensor, out_size: int, first: torch.Tensor, index: torch.Tensor):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter where it scales up (support 1, three taps): per
    sample ``in_size`` fp64 [B] source pixels starting at ``first`` fp64 [B] are resized to ``out_size``; for the output indices
    ``index`` fp64 [n] -> (first tap int32 [B, n], weights int32 [B, n, 3])."""
    scale = in_size / torch.full_like(in_size, float(out_size))          # a tensor divisor: a true division on every device
    center = (index.unsqueeze(0) + 0.5) * scale.unsqueeze(1)
    xmin = torch.trunc(center - 1.0 + 0.5).clamp_(min=0)
    xmax = torch.minimum(torch.trunc(center + 1.0 + 0.5), in_size.unsqueeze(1)) - xmin
    w = []
    for t in range(3):
        wt = (1.0 - torch.abs((t + xmin) - center + 0.5)).clamp_(min=0)
        w.append(torch.where(t < xmax, wt, torch.zeros_like(wt)))
    ww = (w[0] + w[1]) + w[2]
    k = torch.stack([torch.trunc(0.5 + (wt / ww) * float(1 << 22)) for wt in w], dim=2)
    return (xmin + first.unsqueeze(1)).to(torch.int32).contiguous(), k.to(torch.int32).contiguous()


def _inclusive_draw(t: torch.Tensor, lo, hi):
    """random.randint(lo, hi) from uniforms ``t``: lo + floor(t (hi - lo + 1)), never above hi; lo / hi numbers or tensors like t."""
    span = torch.as_tensor(hi - lo, dtype=t.dtype, device=t.device)
    return torch.minimum(torch.floor(t * (span + 1)), span) + lo


def michigan_augment_plan(u: torch.Tensor, image: torch.Tensor, sizes: torch.Tensor, img_size: int, train: bool = True,
                          holes=(3, 16), hole_size=(16, 64), radius_max: float = 1.0) -> MichiganPlan:
    """The random choices of michigan.py's ``HisfragTrainer.get_transforms`` (michigan.py:71-85) for a whole batch at once, from
    uniform numbers ``u`` [B, 104] in [0, 1), the image indices ``image`` [B] and ``sizes`` int32 [n, 2] = (H, W).  Columns of ``u``:
      0-1      RandomCrop(S, pad_if_needed=True, fill 255): origin floor(u (Hp - S + 1)) - pad, pad = max(S - H, 0), Hp = H + 2 pad
      2-21     RandomResizedCrop(S, scale=(0.6, 1)) on the window: ten attempts of (area, ratio) uniforms, area = (0.6 + 0.4 u) S^2,
               ratio = exp(log(3/4) + u (log(4/3) - log(3/4))), w = round(sqrt(area ratio)), h = round(sqrt(area / ratio)) (half to
               even); the first attempt with 0 < w <= S and 0 < h <= S wins, otherwise the whole window
      22-23    its position: i = floor(u (S - h + 1)), j = floor(u (S - w + 1)); the tap tables are Pillow's bilinear coefficients for
               (h, w) -> (S, S), first taps offset by (i, j)
      24-25    CoarseDropout at p = 0.9; the number of holes, an inclusive integer draw lo + floor(u (hi - lo + 1)) in ``holes``
      26-89    per hole (height, width, y1, x1): height / width inclusive draws in ``hole_size`` clamped to S, y1 in [0, S - height],
               x1 in [0, S - width]
      90-91    horizontal, vertical flip at p = 0.5
      92-100   ColorJitter(0.2, 0.3, 0.3, 0.1) at p = 0.5: the order is the argsort of four uniforms, brightness ~ U(0.8, 1.2),
               contrast / saturation ~ U(0.7, 1.3), hue ~ U(-0.1, 0.1) as the uint8 shift trunc(hue 255) mod 256
      101-102  GaussianBlur at p = 0.5: r = fp32(0.1 + (radius_max - 0.1) u), then in fp32 s = r r / 3, a = (-(3 s)) / (6 (s - 1)),
               ww = trunc(2^24 / (a 2 + 1)), and fw = (2^24 - ww) // 2 (Pillow's box radius is 0 for every r <= 1)
      103      RandomGrayscale at p = 0.2
    ``train=False``: PadCenterCrop((S, S), fill 255) -> Resize(R = int(1.15 S)) -> CenterCrop(S): the origin is round((W - S) / 2) for
    W >= S and round(d / 2) - d for a deficit d = S - W (the reference pads both sides by d), the tables are those of S -> R at the
    output indices x + round((R - S) / 2), every flag is 0.  Elementwise torch operations on the device of ``u``: no host copy, no
    sync; fp64 except where stated, every product and sum an operation of its own."""
    S = int(img_size)
    lo_n, hi_n = (int(t) for t in holes)
    lo_s, hi_s = (int(t) for t in hole_size)
    if not 0 <= lo_n <= hi_n <= MICHIGAN_MAX_HOLES or not 1 <= lo_s <= hi_s:
        raise ValueError(f'holes {holes} must lie in 0..{MICHIGAN_MAX_HOLES} and hole_size {hole_size} be positive, both ascending')
    if not 0.1 <= radius_max <= 1.0:
        raise ValueError(f'radius_max {radius_max} outside [0.1, 1]: beyond 1 Pillow\'s box radius is no longer 0')
    u = u.double()
    n_rows, dev = u.shape[0], u.device
    image = image.to(device=dev, dtype=torch.int64)
    hw = sizes.to(dev)[image.clamp(0, sizes.shape[0] - 1)]
    H, W = hw[:, 0].double(), hw[:, 1].double()
    zero, one = torch.zeros_like(H), torch.ones_like(H)
    izero = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    natural = torch.arange(4, dtype=torch.int32, device=dev).expand(n_rows, 4)
    no_blur = torch.tensor([1 << 24, 0], dtype=torch.int32, device=dev).expand(n_rows, 2)
    no_holes = torch.zeros(n_rows, MICHIGAN_MAX_HOLES, 4, dtype=torch.int32, device=dev)
    index = torch.arange(S, dtype=torch.float64, device=dev)
    full = one * S
    if not train:
        centre = lambda n: torch.where(n >= S, torch.round((n - S) / 2), torch.round((S - n) / 2) - (S - n))
        R = int(S * 1.15)
        x0, kx = _bilinear_taps(full, R, zero, index + round((R - S) / 2))
        box = torch.stack([zero, zero, full, full], dim=1).to(torch.int32)
        return MichiganPlan(image.to(torch.int32), izero, torch.stack([centre(H), centre(W)], dim=1).to(torch.int32).contiguous(),
                            box.contiguous(), x0, kx, x0.clone(), kx.clone(), no_holes, izero.clone(), natural.contiguous(),
                            torch.ones(n_rows, 3, dtype=torch.float32, device=dev), izero.clone(), no_blur.contiguous())
    draw = _inclusive_draw
    # RandomCrop with pad_if_needed
    pad_y, pad_x = (S - H).clamp_(min=0), (S - W).clamp_(min=0)
    origin = torch.stack([draw(u[:, 0], 0.0, H + 2 * pad_y - S) - pad_y, draw(u[:, 1], 0.0, W + 2 * pad_x - S) - pad_x], dim=1).to(torch.int32)
    # RandomResizedCrop
    log_lo, log_hi = math.log(3.0 / 4.0), math.log(4.0 / 3.0)
    area = (u[:, 2:22:2] * 0.4 + 0.6) * float(S * S)
    ratio = torch.exp(u[:, 3:22:2] * (log_hi - log_lo) + log_lo)
    w_try, h_try = torch.round(torch.sqrt(area * ratio)), torch.round(torch.sqrt(area / ratio))
    valid = (w_try > 0) & (w_try <= S) & (h_try > 0) & (h_try <= S)
    first = (valid.int().cumsum(1) == 0).sum(1)                            # the attempts in front of the first valid one
    pick = first.clamp(max=_RRC_ATTEMPTS - 1).unsqueeze(1)
    found = first < _RRC_ATTEMPTS
    bw, bh = torch.where(found, w_try.gather(1, pick).squeeze(1), full), torch.where(found, h_try.gather(1, pick).squeeze(1), full)
    bi, bj = torch.where(found, draw(u[:, 22], 0.0, S - bh), zero), torch.where(found, draw(u[:, 23], 0.0, S - bw), zero)
    x0, kx = _bilinear_taps(bw, S, bj, index)
    y0, ky = _bilinear_taps(bh, S, bi, index)
    # CoarseDropout
    dropout = u[:, 24] < 0.9
    count = torch.where(dropout, draw(u[:, 25], float(lo_n), float(hi_n)), zero)
    hu = u[:, 26:90].reshape(n_rows, MICHIGAN_MAX_HOLES, 4)
    limit = lambda t: t.clamp(max=float(S))
    hh = limit(draw(hu[:, :, 0], float(lo_s), float(hi_s)))
    hwid = limit(draw(hu[:, :, 1], float(lo_s), float(hi_s)))
    y1, x1 = draw(hu[:, :, 2], 0.0, S - hh), draw(hu[:, :, 3], 0.0, S - hwid)
    used = torch.arange(MICHIGAN_MAX_HOLES, device=dev).unsqueeze(0) < count.unsqueeze(1)
    rects = torch.where(used.unsqueeze(2), torch.stack([x1, y1, x1 + hwid, y1 + hh], dim=2), zero.view(-1, 1, 1)).to(torch.int32)
    # flips, jitter, blur, grey
    hflip, vflip, jitter, blur_on, grey = u[:, 90] < 0.5, u[:, 91] < 0.5, u[:, 92] < 0.5, u[:, 101] < 0.5, u[:, 103] < 0.2
    flags = (dropout.int() + 2 * hflip.int() + 4 * jitter.int() + 8 * blur_on.int() + 16 * vflip.int() + 32 * grey.int()).to(torch.int32)
    order = torch.where(jitter.unsqueeze(1), torch.argsort(u[:, 93:97], dim=1, stable=True).to(torch.int32), natural)
    drawn = torch.stack([u[:, 97] * 0.4 + 0.8, u[:, 98] * 0.6 + 0.7, u[:, 99] * 0.6 + 0.7], dim=1)
    factors = torch.where(jitter.unsqueeze(1), drawn, one.unsqueeze(1)).float()
    hue = torch.where(jitter, torch.trunc((u[:, 100] * 0.2 - 0.1) * 255.0).to(torch.int64) % 256, 0).to(torch.int32)
    r = (u[:, 102] * (float(radius_max) - 0.1) + 0.1).float()              # Pillow takes the radius as a C float: fp32 from here on
    s2 = (r * r) / torch.full_like(r, 3.0)                                  # tensor divisors: true divisions on every device
    a = (-(s2 * 3.0)) / ((s2 - 1.0) * 6.0)
    ww = torch.trunc(16777216.0 / (a * 2.0 + 1.0)).to(torch.int64)
    fw = torch.div((1 << 24) - ww, 2, rounding_mode='floor')
    blur = torch.where(blur_on.unsqueeze(1), torch.stack([ww, fw], dim=1).to(torch.int32), no_blur)
    box = torch.stack([bi, bj, bh, bw], dim=1).to(torch.int32)
    return MichiganPlan(image.to(torch.int32), flags, origin.contiguous(), box.contiguous(), x0, kx, y0, ky, rects.contiguous(),
                        count.to(torch.int32), order.contiguous(), factors.contiguous(), hue.contiguous(), blur.contiguous())


def michigan_feed(store: 'Div2kImageStore', plan: MichiganPlan, img_size: int) -> torch.Tensor:
    """``plan`` -> uint8 [B, 3, S, S] on the store's device: geometry, colour jitter, blur and grey, three entry points back to back."""
    from . import ops
    windows = ops.michigan_windows_u8(store.data, store.offsets_dev, store.sizes_dev, plan.image, plan.flags, plan.origin, plan.x0,
                                      plan.kx, plan.y0, plan.ky, plan.holes, plan.n_holes, img_size)
    jittered = ops.hisfrag_jitter_u8(windows, plan.flags, plan.order, plan.factors, plan.hue, out=windows)     # pointwise: in place
    return ops.michigan_blur_gray_u8(jittered, plan.flags, plan.blur)


class MichiganDeviceLoader(HisfragDeviceLoader):
    """michigan.py's training loader on the device: ``HisfragDeviceLoader``'s sampler, epochs, ranks and generator streams, with
    michigan.py's transforms (michigan.py:68-101).  Each batch: uniforms -> ``michigan_augment_plan`` -> ``michigan_feed``; it yields
    (images uint8 [B, 3, S, S], targets int64 [B]) for ``hisfrag_prepare_data``.  Images smaller than the window are padded with
    255.  The reference runs 20 passes over the set per epoch (michigan.py:110-112): that is the caller's ``repeat``."""

    def plan(self, image: torch.Tensor, generator: torch.Generator) -> MichiganPlan:
        """One batch's draws."""
        u = torch.rand(image.numel(), MICHIGAN_PLAN_COLUMNS, generator=generator, device=self.store.device)
        return michigan_augment_plan(u, image, self.store.sizes_dev, self.img_size, self.train)

    def __iter__(self):
        g = self._generator(2 * self.rank + 1)
        for image in self.rank_indices():
            yield michigan_feed(self.store, self.plan(image, g), self.img_size), self.labels_dev[image]


# ---------------------------------------------------------------------------------------------
# pair mining for the two-stage HisFrag training step (hisfrag.py:117-159)
# ---------------------------------------------------------------------------------------------
def mine_pairs(targets: torch.Tensor, neg_per_pos: float = 2.0, generator=None, ordered_negatives: bool = False):
    """(groups int64 [P, 2], labels fp32 [P, 1]): every same-label pair (i, j), j > i, in row-major order, then a
    random subset of the different-label pairs of size min(#neg, int(neg_per_pos * #pos)) - what
    ``HisfragTrainer.prepare_data`` (hisfrag.py:117-145) builds with a Python loop over the batch and 2n
    ``nonzero`` host syncs.  Here: one ``triu_indices`` + two boolean selects on the device (the pair count is
    data-dependent, so one host sync per step remains).
    ``ordered_negatives``: the negative candidates are ALL ordered pairs (i, j), i != j, with different labels, row-major
    (michigan.py:142-148 scans the whole row, not its upper half); with ``neg_per_pos=1.0`` that is michigan's rule
    (michigan.py:150).  The positives are the upper-triangle pairs either way."""
    t = targets.reshape(-1)
    n = t.numel()
    i, j = torch.triu_indices(n, n, offset=1, device=t.device)
    same = t[i] == t[j]
    pos = torch.stack([i[same], j[same]], dim=1)
    if ordered_negatives:
        neg = torch.nonzero(t.view(-1, 1) != t.view(1, -1))            # row-major: i outer, j ascending
    else:
        neg = torch.stack([i[~same], j[~same]], dim=1)
    keep = min(neg.shape[0], int(neg_per_pos * pos.shape[0]))
    perm = torch.randperm(neg.shape[0], generator=generator, device=neg.device if generator is None else generator.device)[:keep]
    neg = neg[perm.to(neg.device)]
    groups = torch.cat([pos, neg], dim=0)
    labels = torch.cat([torch.ones(pos.shape[0], device=t.device), torch.zeros(neg.shape[0], device=t.device)]).view(-1, 1)
    return groups, labels


def hisfrag_prepare_data(model, samples: torch.Tensor, targets: torch.Tensor, amp: bool = True, generator=None):
    """The first half of the reference's two-stage step (hisfrag.py:117-155): mine pairs, run the encoder ONCE per
    image, gather.  Returns ((x, x1_feats), labels) for ``model(x1_feats, x)`` exactly like the reference's
    ``prepare_data`` -> ``train_step`` hand-off (hisfrag.py:153-159)."""
    groups, labels = mine_pairs(targets, generator=generator)
    with torch.autocast(samples.device.type, dtype=torch.bfloat16, enabled=amp):
        feats = model(samples, forward_first_part=True)
    return (samples[groups[:, 0]], feats[groups[:, 1]]), labels


def hisfrag_prepare_indexed(model, samples: torch.Tensor, targets: torch.Tensor, amp: bool = True, generator=None, neg_per_pos: float = 2.0,
                            ordered_negatives: bool = False):
    """``hisfrag_prepare_data`` without its two gathers: returns ((samples, feats, x2_index, x1_index), labels) with
    x2_index = groups[:, 0] (int64 [P]) and x1_index = ops.pair_segments(groups[:, 1], n) - what hisfrag.py:153-154 gathers - for
    ``model(feats, samples, x2_index=x2_index, x1_index=x1_index)``.  The decoder then embeds image 2 through the index, projects
    the cross-attention keys / values once per IMAGE and sums every image's key / value gradient over its pairs in a fixed order:
    the step is bitwise reproducible, which the gathered form (an atomic scatter-add in ``feats[index]``'s backward) is not.
    ``neg_per_pos`` / ``ordered_negatives``: ``mine_pairs``' rule (1.0 / True: michigan.py:150)."""
    from . import ops
    groups, labels = mine_pairs(targets, neg_per_pos=neg_per_pos, generator=generator, ordered_negatives=ordered_negatives)
    with torch.autocast(samples.device.type, dtype=torch.bfloat16, enabled=amp):
        feats = model(samples, forward_first_part=True)
    x2_index = groups[:, 0].contiguous()
    return (samples, feats, x2_index, ops.pair_segments(groups[:, 1], samples.shape[0])), labels


# ---------------------------------------------------------------------------------------------
# pair mining on the device: fixed shape, no host read, a rule that is restated on the CPU
# ---------------------------------------------------------------------------------------------
class MinedPairs(NamedTuple):
    """What ``mine_pairs_device`` returns: ``capacity`` rows - positives, kept negatives, padding."""
    groups: torch.Tensor      # int64 [capacity, 2]: (image 2, image 1) like ``mine_pairs``; a padding row is (0, 0)
    labels: torch.Tensor      # fp32 [capacity, 1]: 1 same writer, 0 different (and padding)
    weights: torch.Tensor     # fp32 [capacity, 1]: 1 for a pair, 0 for a padding row
    segments: 'ops.PairSegments'   #  of groups[:, 1] over the batch's images
    counts: torch.Tensor      # int32 [5]: positives, candidates, negatives emitted, pairs emitted, pairs dropped (capacity)


def _mine_pairs_restated(t, keys, neg_per_pos, ordered_negatives, capacity):
    """The rule of ``mine_pairs_device`` in plain torch (any device; used for CPU tensors)."""
    from . import ops
    n, dev = t.numel(), t.device
    same = t.view(-1, 1) == t.view(1, -1)
    upper = torch.ones(n, n, dtype=torch.bool, device=dev).triu(1)
    pos = torch.nonzero(same & upper)                                  # row-major = ascending cell
    is_cand = ~same if ordered_negatives else ~same & upper
    cand = torch.nonzero(is_cand)
    keep = max(min(cand.shape[0], int(neg_per_pos * pos.shape[0])), 0)
    by_key = torch.argsort(keys.view(n, n)[is_cand], stable=True)      # equal keys: the lower cell first
    pos_rows = min(pos.shape[0], capacity)
    neg_rows = min(keep, capacity - pos_rows)
    rows = pos_rows + neg_rows
    groups = torch.zeros(capacity, 2, dtype=torch.int64, device=dev)
    labels, weights = (torch.zeros(capacity, 1, dtype=torch.float32, device=dev) for _ in range(2))
    groups[:pos_rows] = pos[:pos_rows]
    groups[pos_rows:rows] = cand[by_key[:neg_rows]]
    labels[:pos_rows] = 1.0
    weights[:rows] = 1.0
    counts = torch.tensor([pos.shape[0], cand.shape[0], neg_rows, rows, pos.shape[0] + keep - rows], dtype=torch.int32, device=dev)
    return MinedPairs(groups, labels, weights, ops.pair_segments(groups[:, 1].contiguous(), n), counts)


def mine_pairs_device(targets: torch.Tensor, capacity: int, neg_per_pos: float = 2.0, generator=None, ordered_negatives: bool = False,
                      keys: torch.Tensor | None = None) -> MinedPairs:
    """``mine_pairs`` with a fixed-shape result and no host read: ``capacity`` rows whatever the batch holds.

    Positives: every (i, j), i < j, of one writer, row-major - ``mine_pairs``' set and order.  Negatives: of the different-writer
    cells (i < j; every i != j with ``ordered_negatives``, michigan.py:142-148) the min(#candidates, int(neg_per_pos * #positives))
    with the smallest key, ``keys`` fp32 [n * n] in [0, 1) holding one key per ordered cell i * n + j; in ascending (key, cell)
    order.  With i.i.d. uniform keys that subset has the distribution of ``randperm(#candidates)[:keep]``; two keys that are equal
    at fp32 resolution go to the lower cell.  Then padding rows (0, 0) with label 0 and weight 0.  Pairs beyond ``capacity`` are
    dropped, negatives from the end first, and ``counts[4]`` says how many.

    On a GPU tensor: ``keys`` are drawn with ``torch.rand`` on the device unless given (from ``generator``, or the device's default
    generator, which a graph capture registers), then one kernel (``ops.mine_pairs``; at most 128 images): capturable.  On a CPU
    tensor: the same rule in plain torch, without the 128-image limit - identical results for identical keys."""
    from . import ops
    t = targets.reshape(-1).to(torch.int64).contiguous()
    n, capacity = t.numel(), int(capacity)
    if n < 1 or capacity < 1:
        raise ValueError(f'mine_pairs_device: {n} images, capacity {capacity}: both must be at least 1')
    if keys is None:
        keys = torch.rand(n * n, generator=generator, device=t.device if generator is None else generator.device).to(t.device)
    if keys.dtype != torch.float32 or keys.numel() != n * n or keys.device != t.device:
        raise ValueError(f'mine_pairs_device: keys must be {n * n} float32 values on {t.device}, got {keys.dtype} {tuple(keys.shape)} '
                         f'on {keys.device}')
    neg_per_pos = float(neg_per_pos)
    if not 0.0 <= neg_per_pos < float('inf'):
        raise ValueError(f'mine_pairs_device: neg_per_pos must be a finite number >= 0, got {neg_per_pos}')
    keys = keys.reshape(-1).contiguous()
    if t.is_cuda:
        return MinedPairs(*ops.mine_pairs(t, keys, neg_per_pos, ordered_negatives, capacity))
    return _mine_pairs_restated(t, keys, neg_per_pos, bool(ordered_negatives), capacity)


@functools.lru_cache(maxsize=None)
def _reachable_positive_counts(n: int) -> int:
    """Bit p is set when some labeling of n images has p same-label pairs (i < j): the sums of s (s - 1) / 2 over the class
    sizes of a partition of n."""
    reach = [0] * (n + 1)
    reach[0] = 1
    for s in range(1, n + 1):
        for total in range(0, n - s + 1):          # ascending: a class size may repeat
            if reach[total]:
                reach[total + s] |= reach[total] << (s * (s - 1) // 2)
    return reach[n]


def mined_pair_capacity(n: int, m: int | None = None, neg_per_pos: float = 2.0, ordered_negatives: bool = False) -> int:
    """Rows ``mine_pairs_device`` needs for a batch of ``n`` images (host arithmetic only; at least 1).  With ``m``: the exact
    pair count of n / m distinct classes of m images each, the batch ``MPerClassSampler`` aims for - (24, 3) gives 72, and 48
    under michigan's rule (neg_per_pos 1, ordered).  Without: the largest count over ALL labelings of n images (every partition's
    positive count is tried), so that nothing is ever dropped."""
    n, cells = int(n), int(n) * (int(n) - 1) // 2
    if n < 1:
        raise ValueError(f'mined_pair_capacity: {n} images')

    def pairs(pos):
        cand = 2 * (cells - pos) if ordered_negatives else cells - pos
        return pos + max(min(cand, int(neg_per_pos * pos)), 0)

    if m is not None:
        m = int(m)
        if m < 1 or n % m:
            raise ValueError(f'mined_pair_capacity: {n} images are no multiple of m = {m}')
        return max(pairs(n // m * (m * (m - 1) // 2)), 1)
    reach, best, pos = _reachable_positive_counts(n), 1, 0
    while reach:
        if reach & 1:
            best = max(best, pairs(pos))
        reach >>= 1
        pos += 1
    return best


def mined_bce_with_logits(logits: torch.Tensor, mined: MinedPairs, reduction: str = 'mean') -> torch.Tensor:
    """BCE-with-logits over the valid rows of a ``MinedPairs``: 'mean' = sum(weights * bce) / max(counts[3], 1) (what
    ``BCEWithLogitsLoss()`` gives on the real pairs, hisfrag.py), 'sum' = the weighted sum (michigan.py's reduction).  ``logits``
    [capacity] or [capacity, C]; with C > 1 outputs every column takes the pair's label and the mean divides by C as well.  Plain
    torch on the logits' device, fp32, no host read; a padding row has weight 0 and contributes exact zeros to the loss and to
    every gradient.  Usable as ``TrainStep(criterion=mined_bce_with_logits)`` with ``y = mined``."""
    if reduction not in ('mean', 'sum'):
        raise ValueError(f"mined_bce_with_logits: reduction must be 'mean' or 'sum', got {reduction!r}")
    x = logits.float()
    x = x.unsqueeze(1) if x.dim() == 1 else x
    if x.dim() != 2 or x.shape[0] != mined.labels.shape[0]:
        raise ValueError(f'mined_bce_with_logits: logits {tuple(logits.shape)} for {mined.labels.shape[0]} mined rows')
    total = torch.nn.functional.binary_cross_entropy_with_logits(x, mined.labels.expand_as(x), weight=mined.weights.expand_as(x),
                                                                 reduction='sum')
    if reduction == 'sum':
        return total
    return total / (mined.counts[3].clamp(min=1).to(torch.float32) * x.shape[1])


def hisfrag_prepare_mined(model, samples: torch.Tensor, targets: torch.Tensor, capacity: int, amp: bool = True, generator=None,
                          neg_per_pos: float = 2.0, ordered_negatives: bool = False):
    """``hisfrag_prepare_indexed`` on ``mine_pairs_device``: returns ((samples, feats, x2_index, segments), mined) for
    ``model(feats, samples, x2_index=x2_index, x1_index=segments)`` and ``mined_bce_with_logits(logits, mined)``.  Every tensor
    has ``capacity`` rows, nothing is read back: the host runs ahead of the device, and the decoder's shapes never change."""
    mined = mine_pairs_device(targets, capacity, neg_per_pos=neg_per_pos, generator=generator, ordered_negatives=ordered_negatives)
    with torch.autocast(samples.device.type, dtype=torch.bfloat16, enabled=amp):
        feats = model(samples, forward_first_part=True)
    return (samples, feats, mined.groups[:, 0].contiguous(), mined.segments), mined


# ---------------------------------------------------------------------------------------------
# pairwise similarity-matrix inference (hisfrag.py:161-302, BASELINE config 5)
# ---------------------------------------------------------------------------------------------
def shard_rows_by_pair_count(n: int, world: int):
    """Contiguous row blocks of the upper triangle (i <= j) with ~equal PAIR counts per rank - the
    balancing rule of data/samplers.py:108-137 in closed form.  Returns world+1 row boundaries."""
    total = n * (n + 1) // 2
    bounds, acc, r = [0], 0, 1
    for i in range(n):
        acc += n - i
        while r < world and acc >= total * r / world:
            bounds.append(i + 1)
            r += 1
    while len(bounds) < world + 1:
        bounds.append(n)
    bounds[-1] = n
    return bounds


def _row_block_pairs(a0, a1, c0, c1, dev):
    """Pairs (i, j), i in [a0, a1), j in [c0, c1), j >= i, row-major - the order every rank and the assembler agree on."""
    ii = torch.arange(a0, a1, device=dev).view(-1, 1).expand(a1 - a0, c1 - c0)
    jj = torch.arange(c0, c1, device=dev).view(1, -1).expand(a1 - a0, c1 - c0)
    keep = jj >= ii
    return ii[keep], jj[keep]


class _ImageSource:
    """Images by index range for the streamed similarity run: a tensor [n, C, S, S] (host or device, uint8 or float) or a
    callable ``(lo, hi) -> tensor`` with ``n_images`` (the reference re-opens its dataset with ``lower_bound`` per row block,
    hisfrag.py:201-211).  Host blocks travel through ``DevicePrefetcher`` (pinned staging, side stream, uint8 stays uint8)."""

    def __init__(self, images, n_images, dev):
        self.images, self.dev = images, dev
        if torch.is_tensor(images):
            self.n = images.shape[0]
        else:
            if n_images is None:
                raise ValueError('pairwise_similarity: a callable image source needs n_images')
            self.n = int(n_images)

    def host_block(self, lo, hi):
        return self.images[lo:hi] if torch.is_tensor(self.images) else self.images(lo, hi)

    def block(self, lo, hi):
        t = self.host_block(lo, hi)
        return t if t.device == self.dev else t.to(self.dev, non_blocking=True)

    def column_blocks(self, start, step):
        """(c0, c1, images on the device) for c0 = start, start + step, ...; host blocks are copied one block ahead."""
        spans = [(c0, min(c0 + step, self.n)) for c0 in range(start, self.n, step)]
        if not spans:
            return
        probe = self.host_block(*spans[0])
        if probe.device == self.dev or self.dev.type != 'cuda':
            for i, (c0, c1) in enumerate(spans):
                yield c0, c1, (probe if i == 0 else self.host_block(c0, c1)).to(self.dev)
            return
        loader = ((probe if i == 0 else self.host_block(c0, c1), torch.tensor([c0, c1])) for i, (c0, c1) in enumerate(spans))
        for (imgs, _), (c0, c1) in zip(DevicePrefetcher(loader, self.dev, depth=1), spans):
            yield c0, c1, imgs


def _similarity_scores_streamed(model, src, r0, r1, *, block, col_block, pair_batch, amp, state_path, meta, after_row_block):
    """This rank's score vector (pairs of rows [r0, r1) in _row_block_pairs order, row block by row block, column block by
    column block) with O(block + col_block) images resident: per row block the encoder output and the cross-attention K / V of
    ``block`` images; per column block the image-2 token cache of ``col_block`` images.  Finished row blocks are saved to
    ``state_path`` (what hisfrag.py:181-195,243-246 does with ``*_result_rank{r}.pt``) and skipped on a restart."""
    n, dev = src.n, src.dev
    total = sum(n - i for i in range(r0, r1))
    scores = torch.empty(total, dtype=torch.float32, device=dev)
    done_rows, off = r0, 0
    if state_path is not None and os.path.exists(state_path):
        st = torch.load(state_path, map_location='cpu', weights_only=True)
        if st.get('meta') == meta and r0 <= int(st['done_rows']) <= r1:
            done_rows = int(st['done_rows'])
            off = int(st['scores'].numel())
            scores[:off] = st['scores'].to(dev)
    dtype_ctx = lambda: torch.autocast(dev.type, dtype=torch.bfloat16, enabled=amp)
    for a0 in range(r0, r1, block):
        a1 = min(a0 + block, r1)
        if a1 <= done_rows:
            continue                                                        # finished before the restart
        with dtype_ctx():
            feats = model(src.block(a0, a1), forward_first_part=True)       # encoder once per row block
            kvs = model.cache_context_kv(feats)                             # K / V of every decoder block, once per row block
        del feats
        for c0, c1, imgs2 in src.column_blocks(a0, col_block):
            with dtype_ctx():
                tokens2, q0 = model.cache_image2_tokens(imgs2)              # everything that depends on image 2 alone
            ii, jj = _row_block_pairs(a0, a1, c0, c1, dev)
            for p0 in range(0, ii.numel(), pair_batch):
                with dtype_ctx():
                    out = model.forward_pairs_cached(tokens2, jj[p0:p0 + pair_batch] - c0, kvs, ii[p0:p0 + pair_batch] - a0, q0)
                cnt = out.numel()
                scores[off: off + cnt] = out.float().reshape(-1)
                off += cnt
            del tokens2, q0, imgs2
        del kvs
        if state_path is not None:
            tmp = state_path + '.tmp'
            torch.save({'meta': meta, 'done_rows': a1, 'scores': scores[:off].cpu(), 'is_finished': a1 == r1}, tmp)
            os.replace(tmp, state_path)                                     # a kill between blocks never leaves a torn file
        if after_row_block is not None:
            after_row_block(a0, a1)
    assert off == total, (off, total)
    return scores


@torch.no_grad()
def pairwise_similarity(model, images, *, rank: int = 0, world: int = 1, block: int = 64, pair_batch: int = 512,
                        amp: bool = True, group=None, pair_cache: bool = True, col_block: int = 256, n_images=None,
                        state_path=None, after_row_block=None):
    """similarity[i, j] = similarity[j, i] = fp16(logit(model(features(image_i), image_j))) for i <= j.

    What hisfrag.py:161-302 computes, re-plumbed: the encoder runs ONCE per image of this rank's row
    block, the decoder runs on `pair_batch` pairs at a time, and the ranks exchange their score vectors with ONE
    all-gather (RCCL on GPU) instead of the reference's per-rank files + 120 s polling.  Every rank returns the full
    symmetric [n, n] fp16 matrix of raw logits (callers take 1 - similarity as the distance, hisfrag.py:294-296).

    With the HIP model (``supports_pair_cache``) the run STREAMS: ``images`` may be a host tensor (uint8 or float) or a
    callable ``(lo, hi) -> tensor`` (+ ``n_images``), only ``block`` row images and ``col_block`` column images are
    resident at a time, scores land in one pre-sized buffer, and with ``state_path`` finished row blocks are saved and a
    restarted run skips them (hisfrag.py:181-195,243-246).  Models without the cache (the CPU oracle in the tests) take the
    plain path on a resident image tensor."""
    cached = bool(getattr(model, 'supports_pair_cache', False)) and pair_cache
    was_training = model.training
    model.eval()
    if cached:
        dev = next(model.parameters()).device
        src = _ImageSource(images, n_images, dev)
        n = src.n
        bounds = shard_rows_by_pair_count(n, world)
        r0, r1 = bounds[rank], bounds[rank + 1]
        meta = {'n': n, 'r0': r0, 'r1': r1, 'block': block, 'col_block': col_block}
        mine = _similarity_scores_streamed(model, src, r0, r1, block=block, col_block=col_block, pair_batch=pair_batch, amp=amp,
                                           state_path=state_path, meta=meta, after_row_block=after_row_block)
        enumerate_pairs = lambda lo, hi: [(_row_block_pairs(a0, min(a0 + block, hi), c0, min(c0 + col_block, n), dev))
                                          for a0 in range(lo, hi, block) for c0 in range(a0, n, col_block)]
    else:
        n = images.shape[0]
        dev = images.device
        bounds = shard_rows_by_pair_count(n, world)
        r0, r1 = bounds[rank], bounds[rank + 1]
        dtype_ctx = torch.autocast(dev.type, dtype=torch.bfloat16, enabled=amp)
        by_index = bool(getattr(model, 'supports_x2_index', False))
        scores = []
        for a0 in range(r0, r1, block):
            a1 = min(a0 + block, r1)
            with dtype_ctx:
                feats = model(images[a0:a1], forward_first_part=True)          # encoder once per row block
            ii, jj = torch.triu_indices(a1 - a0, n - a0, offset=0, device=dev)  # pairs (a0+ii, a0+jj), jj >= ii
            for c0 in range(0, ii.numel(), pair_batch):
                i_sub, j_sub = ii[c0:c0 + pair_batch], (jj[c0:c0 + pair_batch] + a0)
                with dtype_ctx:
                    out = model(feats[i_sub], images, x2_index=j_sub) if by_index else model(feats[i_sub], images[j_sub])
                scores.append(out.float().reshape(-1))
        mine = torch.cat(scores) if scores else torch.zeros(0, device=dev)

        def enumerate_pairs(lo, hi):
            out = []
            for a0 in range(lo, hi, block):
                a1 = min(a0 + block, hi)
                ii, jj = torch.triu_indices(a1 - a0, n - a0, offset=0, device=dev)
                out.append((ii + a0, jj + a0))
            return out
    model.train(was_training)

    # exchange: pad to the largest shard, one all-gather, then every rank rebuilds the matrix
    counts = [sum(n - i for i in range(bounds[r], bounds[r + 1])) for r in range(world)]
    if world > 1:
        pad = torch.zeros(max(counts), dtype=torch.float32, device=dev)
        pad[:mine.numel()] = mine
        gathered = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(gathered, pad, group=group)
    else:
        gathered = [mine]
    sim = torch.zeros((n, n), dtype=torch.float16, device=dev)
    for r in range(world):
        off = 0
        for ii, jj in enumerate_pairs(bounds[r], bounds[r + 1]):      # the same enumeration order as the compute loop
            vals = gathered[r][off: off + ii.numel()].to(torch.float16)
            sim[ii, jj] = vals
            sim[jj, ii] = vals
            off += ii.numel()
        assert off == counts[r], (r, off, counts[r])
    return sim


# ---------------------------------------------------------------------------------------------
# retrieval metrics of the distance matrix (misc/wi19_evaluate.get_metrics, hisfrag.py:309,321)
# ---------------------------------------------------------------------------------------------
def _summed_rows(share, n, rows, nsums, device, group):
    """The float64 [nsums] sums ``share(r0, r1)`` returns for ``rows=(r0, r1)`` (default: all n rows), SUM all-reduced over
    ``group`` when one is given.  An empty share (more ranks than rows) contributes zeros but still joins the reduction."""
    r0, r1 = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= r0 <= r1 <= n:
        raise ValueError(f'rows ({r0}, {r1}) is not a range inside [0, {n}]')
    sums = share(r0, r1) if r1 > r0 else torch.zeros(nsums, dtype=torch.float64, device=device)
    if group is not None:
        dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
    return sums


def class_members(labels: torch.Tensor):
    """(class ids int32 [n] in [0, C), offsets int32 [C + 1], members int32 [n]): the columns of class c are
    members[offsets[c]:offsets[c + 1]], in ascending order.  Equal input labels get equal ids, so 'same class' is unchanged."""
    _, ids = torch.unique(labels, return_inverse=True)
    members = torch.argsort(ids, stable=True)
    counts = torch.bincount(ids)
    offsets = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=labels.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return ids.to(torch.int32), offsets.to(torch.int32), members.to(torch.int32)


def metrics_from_sums(sums):
    """(mAP, top-1, Pr@10, Pr@100) from the 7 sums of vited_retrieval_metrics (after any cross-rank SUM).  mAP is NaN when
    no row has a correct retrieval (numpy's mean of an empty array); Pr@k is NaN as soon as one row has none, as in the
    reference."""
    ap, valid, top1, pr10, pr100, _, rows = (float(v) for v in sums.tolist())
    nan = float('nan')
    return (ap / valid if valid else nan,) + ((top1 / rows, pr10 / rows, pr100 / rows) if rows else (nan, nan, nan))


def retrieval_metrics(distance: torch.Tensor, labels, *, rows=None, remove_self_column: bool = True,
                      from_similarity: bool = False, group=None):
    """(mAP, top-1, Pr@10, Pr@100) of ``wi19_evaluate.get_metrics(distance, labels, remove_self_column)`` on the GPU.

    ``distance``: [n, n] float16 / bfloat16 / float32 on the device (with ``from_similarity``: the similarity matrix S, ranked
    by dtype(1 - S)).  ``labels``: int class ids [n] (a device tensor, or anything torch.as_tensor takes).  ``rows=(r0, r1)``
    computes this rank's share of the rows (default: all); with ``group`` (a process group, e.g. ``dist.group.WORLD``) ONE
    all-reduce (SUM, so gloo works too) combines the shares and every rank returns the metrics of all rows.  Without a group
    the result covers ``rows`` only."""
    from . import ops                                       # ops.retrieval_metrics_rows refuses CPU tensors: no CPU fallback
    n = distance.shape[0]
    labels = torch.as_tensor(labels, device=distance.device)
    if labels.dim() != 1 or labels.numel() != n:
        raise ValueError(f'labels must be a vector of length {n}, got shape {tuple(labels.shape)}')
    if labels.is_floating_point() or labels.is_complex():
        raise TypeError(f'labels must be integer class ids, got {labels.dtype}')

    def share(r0, r1):
        ids, offsets, members = class_members(labels)
        return ops.retrieval_metrics_rows(distance, ids, offsets, members, (r0, r1), remove_self_column=remove_self_column,
                                          from_similarity=from_similarity)[1]
    return metrics_from_sums(_summed_rows(share, n, rows, 7, distance.device, group))


@torch.no_grad()
def hisfrag_retrieval_metrics(similarity: torch.Tensor, labels, *, rank: int = 0, world: int = 1, group=None,
                              remove_self_column: bool = True):
    """The evaluation step after ``pairwise_similarity``: every rank holds the [n, n] fp16 similarity, ranks the rows
    ``shard_rows_by_pair_count(n, world)`` gives it by fp16(1 - similarity), and one all-reduce gives every rank the metrics of
    all rows.  Replaces, on every rank (hisfrag.py:294-296,306-309):

        distance_matrix = 1 - similarity_matrix
        labels = utils.list_to_idx(img_names, lambda x: x.split('_')[0])
        m_ap, top1, pr_k10, pr_k100 = wi19_evaluate.get_metrics(distance_matrix.numpy(), np.asarray(labels))

    with ``hisfrag_retrieval_metrics(similarity, labels, rank=rank, world=world)`` (same ``labels``)."""
    n = similarity.shape[0]
    bounds = shard_rows_by_pair_count(n, world)
    if world > 1 and group is None:
        group = dist.group.WORLD
    return retrieval_metrics(similarity, labels, rows=(bounds[rank], bounds[rank + 1]), remove_self_column=remove_self_column,
                             from_similarity=True, group=group if world > 1 else None)


# ---------------------------------------------------------------------------------------------
# group mAP / Pr@k (misc/metric.calc_map_prak) and the geshaem evaluation (michigan.py:188-233)
# ---------------------------------------------------------------------------------------------
def _relation_csr(uniq, id_of, relation, row_ids, device):
    """(offsets int32 [L + 1], label ids int32): for every label id a whose label is in ``row_ids``, the ascending, duplicate-free
    ids of the labels of ``relation[label]`` that occur among the columns (others cannot match).  A missing key raises KeyError,
    as the reference's ``positive_pairs[labels[i]]`` does; labels of rows outside the range get an empty row."""
    offsets, flat = [0], []
    for a, label in enumerate(uniq):
        if a in row_ids:
            flat.extend(sorted({id_of[b] for b in relation[label] if b in id_of}))
        offsets.append(len(flat))
    return (torch.tensor(offsets, dtype=torch.int32, device=device), torch.tensor(flat, dtype=torch.int32, device=device))


def group_relations(labels, positive_pairs, negative_pairs=None, device='cuda', *, rows=None):
    """The device form of (labels, positive_pairs, negative_pairs) that ``ops.group_retrieval_metrics_rows`` takes:
    (label ids int32 [n], (offsets, members) of every label's columns, positive CSR, negative CSR or None), label ids numbered
    by first appearance.  Only the labels of ``rows`` (default: all) are looked up in the mappings."""
    labels = list(labels)
    r0, r1 = (0, len(labels)) if rows is None else (int(rows[0]), int(rows[1]))
    id_of = {}
    ids = [id_of.setdefault(label, len(id_of)) for label in labels]
    uniq = list(id_of)
    row_ids = set(ids[r0:r1])
    label_ids, col_off, col_mem = class_members(torch.tensor(ids, dtype=torch.int64, device=device))
    pos = _relation_csr(uniq, id_of, positive_pairs, row_ids, device)
    neg = None if negative_pairs is None else _relation_csr(uniq, id_of, negative_pairs, row_ids, device)
    return label_ids, (col_off, col_mem), pos, neg


def map_prak(distances: torch.Tensor, labels, positive_pairs, negative_pairs=None, prak=(1, 5), *, rows=None, group=None):
    """``(m_ap, (pr@k for k in prak))`` of ``misc/metric.calc_map_prak(distances, labels, positive_pairs, negative_pairs, prak)``
    on the GPU.

    ``distances``: [n, n] float16 / bfloat16 / float32 on the device.  ``labels``: n hashables (``dist_df.columns``); row i has
    the label ``labels[i]``.  ``positive_pairs`` / ``negative_pairs``: mappings from a label to an iterable of labels
    (``fragment_to_group``); "correct" and "eligible" are set membership.  A row label missing from a mapping raises KeyError.
    Each row is ordered by a STABLE argsort (ties to the lower column, NaN last; numpy's default sort may order ties otherwise),
    its first eligible element is skipped whatever it is, and rows without a correct retrieval are left out, as in the
    reference.  Where no row has one the reference divides by zero; here every result is then NaN.  ``prak``: up to 8 ints >= 1.
    ``rows=(r0, r1)`` computes this rank's share of the rows (default: all); with ``group`` ONE all-reduce (SUM, so gloo works
    too) combines the shares and every rank returns the metrics of all rows.  Without a group the result covers ``rows`` only."""
    from . import ops                                       # ops refuses CPU tensors: no CPU fallback
    n = distances.shape[0]
    labels = list(labels)
    if len(labels) != n:
        raise ValueError(f'labels must hold {n} labels, got {len(labels)}')
    prak = tuple(int(k) for k in prak)
    if not 1 <= len(prak) <= 8 or min(prak) < 1:
        raise ValueError(f'prak must be 1 to 8 cut-offs >= 1, got {prak}')

    def share(r0, r1):
        rel = group_relations(labels, positive_pairs, negative_pairs, distances.device, rows=(r0, r1))
        return ops.group_retrieval_metrics_rows(distances, *rel, prak, (r0, r1))[1]
    s = [float(v) for v in _summed_rows(share, n, rows, 2 + len(prak), distances.device, group).tolist()]
    if s[1] == 0:
        return float('nan'), tuple(float('nan') for _ in prak)
    return s[0] / s[1], tuple(v / s[1] for v in s[2:])


class PairScoreStats(NamedTuple):
    """What ``PairScoreAggregator.finish`` returns.  mean / min float32 [n, n] of the distances 1 - score of every cell (NaN where
    a cell has no value), count int32 [n, n], std_stats = (avg_std, std_std): the mean and the sample stdev of the per-cell
    sample stdevs over the cells with more than one value (NaN where there are too few), std float64 [n, n] those stdevs."""
    mean: torch.Tensor
    min: torch.Tensor
    count: torch.Tensor
    std_stats: tuple
    std: torch.Tensor


class PairScoreAggregator:
    """The distance maps of ``geshaem_test`` (michigan.py:188-209) on the device.  ``add(pairs, scores)`` takes a validation
    batch's fragment-id pairs [m, 2] (int32 / int64, on the host or the device) and its scores [m] (the model's
    ``output.view(-1)``, float32 / bfloat16 / float16, on the device: never copied to the host).  Every score adds 1 - score to
    cell (i, j) and to cell (j, i).  ``finish()`` reduces every record added so far (PairScoreStats); its result is bit-identical
    whatever the batching and order of the records (include/vited.h)."""

    def __init__(self, n_fragments: int, device):
        self.n = int(n_fragments)
        self.device = torch.device(device)
        self.counts = torch.zeros((self.n, self.n), dtype=torch.int32, device=self.device)
        self.bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.size = 0
        self._cells = torch.empty((0, 2), dtype=torch.int32, device=self.device)
        self._values = torch.empty(0, dtype=torch.float32, device=self.device)

    def _reserve(self, extra: int):
        need = self.size + extra
        if need <= self._values.numel():
            return
        cap = max(need, 2 * self._values.numel(), 1 << 16)
        cells = torch.empty((cap, 2), dtype=torch.int32, device=self.device)
        values = torch.empty(cap, dtype=torch.float32, device=self.device)
        cells[:self.size] = self._cells[:self.size]
        values[:self.size] = self._values[:self.size]
        self._cells, self._values = cells, values

    def add(self, pairs: torch.Tensor, scores: torch.Tensor):
        from . import ops
        scores = scores.reshape(-1)
        pairs = pairs.to(self.device, non_blocking=True)
        m = pairs.shape[0]
        if m == 0:
            return
        self._reserve(m)
        ops.pair_scores_add(pairs, scores, self.n, self.counts, self._cells[self.size:self.size + m],
                            self._values[self.size:self.size + m], self.bad)
        self.size += m

    def finish(self) -> PairScoreStats:
        from . import ops
        mean, minv, std, stats = ops.pair_scores_finish(self._cells[:self.size], self._values[:self.size], self.n, self.counts,
                                                       self.bad)
        bad = int(self.bad.item())
        if bad & 1:
            raise ValueError(f'a fragment id outside [0, {self.n}) was added (those records were ignored)')
        if bad:
            raise RuntimeError('vited_pair_scores_finish: counts and records disagree')
        avg_std, std_std = (float(v) for v in stats.tolist())
        return PairScoreStats(mean, minv, self.counts.clone(), (avg_std, std_std), std)


class GeshaemMetrics(NamedTuple):
    """``geshaem_pair_metrics``: ``mean`` / ``min`` = (m_ap, (pr@k, ...)) of calc_map_prak on the MEAN / MIN distance maps,
    ``avg_std`` / ``std_std`` as logged by the reference, ``n_categories`` = the number of scored fragments."""
    mean: tuple
    min: tuple
    avg_std: float
    std_std: float
    n_categories: int


@torch.no_grad()
def geshaem_pair_metrics(aggregator: PairScoreAggregator, fragments, fragment_to_group, prak=(1, 5, 10)) -> GeshaemMetrics:
    """The evaluation of ``geshaem_test`` after its loop (michigan.py:211-233): the fragments that were scored, in ascending
    fragment index (the order the reference's dicts and DataFrame get from its unshuffled loader), labelled
    ``fragments[index]`` (``dataset.fragments``), ranked by the MEAN and by the MIN distance map with ``fragment_to_group`` as
    the positive relation.  The reference's return value is ``1 - max(result.mean[0], result.min[0])``."""
    res = aggregator.finish()
    scored = torch.nonzero((res.count > 0).any(dim=1)).flatten()
    idx = scored.tolist()
    labels = [fragments[a] for a in idx]
    out = []
    for matrix in (res.mean, res.min):
        sub = matrix.index_select(0, scored).index_select(1, scored)
        out.append(map_prak(sub, labels, fragment_to_group, prak=prak))
    return GeshaemMetrics(out[0], out[1], res.std_stats[0], res.std_stats[1], len(idx))


# ---------------------------------------------------------------------------------------------
# puzzle evaluation (evaluation.py:100-133, solver_driver.py, paikin_tal_solver/): type-1 puzzles of one image, fixed size
# ---------------------------------------------------------------------------------------------
PUZZLE_SIDES = ('top', 'right', 'bottom', 'left')          # PuzzlePieceSide values 0..3; side s touches side (s + 2) % 4
_SIDE_STEP = ((-1, 0), (0, 1), (1, 0), (0, -1))
_DQ_UNSET = 2 ** 31 - 1                                     # the reference's fill of its distance arrays (the diagonal)


def _ordered_block_pairs(a0, a1, n, dev):
    """Pairs (i, j), i in [a0, a1), j in [0, n), j != i, row-major."""
    ii = torch.arange(a0, a1, device=dev).view(-1, 1).expand(a1 - a0, n)
    jj = torch.arange(0, n, device=dev).view(1, -1).expand(a1 - a0, n)
    keep = jj != ii
    return ii[keep], jj[keep]


@torch.no_grad()
def puzzle_distances(model, pieces, *, pair_batch: int = 1024, amp: bool = True, block: int = 128, return_logits: bool = False):
    """The reference's integer piece distances ``Dq`` int32 [4, n, n] on the device (evaluation.py:100-133 feeding
    inter_piece_distance.py:206-223): Dq[s, i, j] is the distance of side s of piece i (top 0, right 1, bottom 2, left 3) to the
    complementary side of piece j, from the model's logits of the ordered pair (i, j) (bin (s + 3) % 4), quantised as
    uint32(trunc(fp32(fp32(1 - sigmoid(logit)) * 1000))).  The diagonal holds 2^31 - 1 (never read).

    ``pieces``: the n pieces of one puzzle at model size, uint8 [n, 3, S, S] (normalised in the patch-embedding kernel) or
    normalised float, on the host or the device.  The encoder and the image-2 token cache run once per piece; the decoder runs on
    all n (n - 1) ordered pairs, ``pair_batch`` at a time, row block by row block of ``block`` pieces, and every batch's logits
    are quantised and scattered into Dq on the device.  ``return_logits`` also returns the fp32 logits [n, n, 4] (diagonal 0)."""
    from . import ops
    if not getattr(model, 'supports_pair_cache', False):
        raise TypeError('puzzle_distances needs the HIP model (VisionTransformerCustom): it runs on the pair caches')
    if getattr(model, 'num_classes', 4) != 4:
        raise ValueError(f'puzzle_distances needs the 4-bin puzzle head, the model has {model.num_classes} outputs')
    dev = next(model.parameters()).device
    src = _ImageSource(pieces, None, dev)
    n = src.n
    if n < 2:
        raise ValueError('a puzzle needs at least two pieces')
    dq = torch.full((4, n, n), _DQ_UNSET, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    logits = torch.zeros((n, n, 4), dtype=torch.float32, device=dev) if return_logits else None
    dtype_ctx = lambda: torch.autocast(dev.type, dtype=torch.bfloat16, enabled=amp)
    was_training = model.training
    model.eval()
    try:
        with dtype_ctx():
            tokens2, q0 = model.cache_image2_tokens(src.block(0, n))        # once per piece
        for a0 in range(0, n, block):
            a1 = min(a0 + block, n)
            with dtype_ctx():
                feats = model(src.block(a0, a1), forward_first_part=True)   # encoder once per piece
                kvs = model.cache_context_kv(feats)
            del feats
            ii, jj = _ordered_block_pairs(a0, a1, n, dev)
            for p0 in range(0, ii.numel(), pair_batch):
                i_sub, j_sub = ii[p0:p0 + pair_batch], jj[p0:p0 + pair_batch]
                with dtype_ctx():
                    out = model.forward_pairs_cached(tokens2, j_sub, kvs, i_sub - a0, q0)
                out = out.float().reshape(-1, 4).contiguous()
                ops.puzzle_distances_from_logits(out, i_sub.contiguous(), j_sub.contiguous(), dq, bad)
                if logits is not None:
                    logits[i_sub, j_sub] = out
            del kvs
    finally:
        model.train(was_training)
    if int(bad.item()):
        raise RuntimeError('puzzle_distances: a pair index fell outside the puzzle (internal error)')
    return (dq, logits) if return_logits else dq


class PuzzleCompatibility:
    """The Paikin-Tal compatibility state of one puzzle on the device (InterPieceDistance, type 1): built from Dq int32 [4, n, n]
    by ``vited_puzzle_compat_init``; ``recalc`` and ``best_slot`` are the solver's two pool-empty steps.  Tensors: min_d,
    second_d int64 [n, 4], candidate, best_buddy int32 [n, 4], compat, mutual float32 [4, n, n], start_count int32 [n],
    start_total float32 [n], start_order int32 [n]."""

    def __init__(self, dq: torch.Tensor):
        from . import ops
        self._ops = ops
        self.dq = dq.to(torch.int32).contiguous()
        self.n = self.dq.shape[1]
        self.state = ops.puzzle_compat_init(self.dq)
        dev = self.dq.device
        self._placed = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.changed = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self._word = torch.empty(1, dtype=torch.int64, device=dev)

    def __getattr__(self, name):
        state = self.__dict__.get('state')
        if state is not None and name in state:
            return state[name]
        raise AttributeError(name)

    def recalc(self, placed) -> torch.Tensor:
        """recalculate_remaining_piece_compatibilities for the boolean mask ``placed`` [n]; returns the changed flags (device)."""
        self._placed.copy_(torch.as_tensor(placed, dtype=torch.int32))
        self._ops.puzzle_compat_recalc(self.dq, self._placed, self.state, self.changed)
        return self.changed

    def best_slot(self, placed, slot_piece, slot_side):
        """(piece, slot index, value) of the first maximum of mutual[(slot_side[k] + 2) % 4, p, slot_piece[k]] over unplaced p
        ascending x slots k in list order."""
        dev = self.dq.device
        self._placed.copy_(torch.as_tensor(placed, dtype=torch.int32))
        sp = torch.as_tensor(slot_piece, dtype=torch.int32).to(dev)
        ss = torch.as_tensor(slot_side, dtype=torch.int32).to(dev)
        self._ops.puzzle_best_slot(self.mutual, self._placed, sp, ss, out=self._word)
        hit = self._ops.puzzle_unpack_slot(int(self._word.item()), sp.numel())
        if hit is None:
            raise RuntimeError('best_slot: no unplaced piece')
        p, k = hit
        return p, k, float(self.mutual[(int(slot_side[k]) + 2) % 4, p, int(slot_piece[k])])


class PuzzleSolution(NamedTuple):
    locations: 'object'         # int64 [n, 2]: (row, col) of every piece, the placed block's top-left corner at (0, 0)
    board_locations: 'object'   # int64 [n, 2]: where the solver put each piece on its n x n board (seed at (n // 2, n // 2))
    order: 'object'             # int64 [n]: placement order, the seed first
    recalcs: int                # times the best-buddy pool ran empty and the compatibilities were recalculated
    grid: 'object'              # int64 [rows, cols]: the piece at each cell, -1 for none


class _BuddyHeapEntry:
    """A best-buddy / open-slot pairing of the solver's heap (solver.py:32-64): heapq pops the largest mutual compatibility, ties
    falling out of the heap's own structure, so the push order and this one comparison must be the reference's."""
    __slots__ = ('compat', 'piece', 'piece_side', 'neighbor', 'neighbor_side', 'location')

    def __init__(self, compat, piece, piece_side, neighbor, neighbor_side, location):
        self.compat, self.piece, self.piece_side = compat, piece, piece_side
        self.neighbor, self.neighbor_side, self.location = neighbor, neighbor_side, location

    def __lt__(self, other):
        return self.compat > other.compat


def solve_puzzle(distances: torch.Tensor, grid_size) -> PuzzleSolution:
    """Paikin-Tal placement (PaikinTalSolver, solver.py) of one type-1 puzzle of ``grid_size`` = (rows, cols) pieces from the
    distances Dq int32 [4, n, n] of ``puzzle_distances``, making the reference's decisions in the reference's order: the seed from
    the start ordering at the board centre, best buddies pooled as pieces are placed, the best-buddy heap popped until it yields a
    placeable entry, and - whenever the pool is empty - a device recalculation of the compatibilities followed by a device scan
    of every unplaced piece against every open slot.  The host keeps a mirror of the mutual compatibility, refreshed by one copy
    per recalculation, for the heap's lookups."""
    import heapq

    import numpy as np
    rows, cols = int(grid_size[0]), int(grid_size[1])
    n = distances.shape[1]
    if rows * cols != n or tuple(distances.shape) != (4, n, n):
        raise ValueError(f'distances {tuple(distances.shape)} do not describe a {rows} x {cols} puzzle')
    comp = PuzzleCompatibility(distances)
    mutual = comp.mutual.cpu().numpy()
    best_buddy = comp.best_buddy.cpu().numpy()
    seed = int(comp.start_order[0].item())

    placed = np.zeros(n, dtype=bool)
    occupied = np.zeros((n, n), dtype=bool)                # the reference's board: n x n, indexed as numpy indexes it
    board_loc = np.full((n, 2), -1, dtype=np.int64)
    top_left, bottom_right = [n // 2, n // 2], [n // 2, n // 2]
    open_slots = []                                         # (location, piece, side of that piece facing the slot), list order
    pool = {}                                               # best buddies waiting, insertion ordered
    heap = []
    order = []
    recalcs = 0

    def fits(loc):
        for d, size in ((0, rows), (1, cols)):
            if loc[d] - top_left[d] + 1 > size or bottom_right[d] - loc[d] + 1 > size:
                return False
        return True

    def slot_open(loc):
        return not occupied[loc] and fits(loc)

    def put(piece, loc):
        board_loc[piece] = loc
        occupied[loc] = True
        placed[piece] = True
        order.append(piece)

    def add_best_buddies(piece):
        for s in range(4):
            bb = int(best_buddy[piece, s])
            if bb < 0 or placed[bb] or bb in pool:
                continue
            pool[bb] = None
            for loc, q, side in open_slots:
                heapq.heappush(heap, _BuddyHeapEntry(float(mutual[(side + 2) % 4, bb, q]), bb, (side + 2) % 4, q, side, loc))

    def open_slots_around(piece):
        r, c = board_loc[piece]
        for s, (dr, dc) in enumerate(_SIDE_STEP):
            loc = (int(r + dr), int(c + dc))
            if slot_open(loc):
                open_slots.append((loc, piece, s))
                for bb in list(pool):
                    heapq.heappush(heap, _BuddyHeapEntry(float(mutual[s, piece, bb]), bb, (s + 2) % 4, piece, s, loc))

    put(seed, (n // 2, n // 2))
    add_best_buddies(seed)
    open_slots_around(seed)
    while not placed.all():
        if pool:
            while True:
                e = heapq.heappop(heap)
                if not placed[e.piece] and slot_open(e.location):
                    break
            piece, loc, from_pool = e.piece, e.location, True
        else:
            recalcs += 1
            comp.recalc(placed)
            mutual = comp.mutual.cpu().numpy()
            valid = [k for k, (loc, _, _) in enumerate(open_slots) if slot_open(loc)]
            piece, k, _ = comp.best_slot(placed, [open_slots[v][1] for v in valid], [open_slots[v][2] for v in valid])
            loc, from_pool = open_slots[valid[k]][0], False
        for d in range(2):
            if top_left[d] > loc[d]:
                top_left[d] = loc[d]
            elif bottom_right[d] < loc[d]:
                bottom_right[d] = loc[d]
        put(piece, loc)
        open_slots = [slot for slot in open_slots if slot[0] != loc]
        if from_pool:
            del pool[piece]
        add_best_buddies(piece)
        open_slots_around(piece)

    locations = board_loc - board_loc.min(axis=0)
    shape = locations.max(axis=0) + 1
    grid = np.full((int(shape[0]), int(shape[1])), -1, dtype=np.int64)
    grid[locations[:, 0], locations[:, 1]] = np.arange(n)
    return PuzzleSolution(locations, board_loc, np.array(order, dtype=np.int64), recalcs, grid)


def puzzle_accuracy(solution: PuzzleSolution, true_locations) -> dict:
    """The accuracies PuzzleResultsCollection.collect_results reports for one solved puzzle (puzzle_importer.py:779-844, the rules
    of :985-1150 and :1386-1520), every piece from the one original puzzle and unrotated: ``Direct_Standard`` (pieces at their true
    cell / n), ``Direct_Modified`` (the same, best over the origins the reference's search from the top-left corner offers),
    ``neighbor`` (sides whose neighbour - or board edge - is the true one / 4n) and ``perfect``.  ``true_locations`` int [n, 2]:
    where piece i belongs in the original rows x cols grid."""
    import numpy as np
    true = np.asarray(true_locations, dtype=np.int64)
    loc = np.asarray(solution.locations, dtype=np.int64)
    n = true.shape[0]
    t_rows, t_cols = int(true[:, 0].max()) + 1, int(true[:, 1].max()) + 1
    orig_id = true[:, 0] * t_cols + true[:, 1]
    g_rows, g_cols = int(loc[:, 0].max()) + 1, int(loc[:, 1].max()) + 1
    placed_id = np.full((g_rows, g_cols), -1, dtype=np.int64)
    placed_id[loc[:, 0], loc[:, 1]] = orig_id

    def correct_at(origin):
        return int(np.all(loc == true + np.asarray(origin), axis=1).sum())

    standard = correct_at((0, 0))
    # the reference's breadth-first search for the candidate origins (puzzle_importer.py:1081-1138)
    frontier, explored, found = [(0, 0)], [], None
    while found is None or (frontier and frontier[0][0] + frontier[0][1] <= found):
        cur = frontier.pop(0)
        explored.append(cur)
        if found is None and placed_id[cur] != -1:
            found = cur[0] + cur[1]
        else:
            for nxt in ((cur[0] + 1, cur[1]), (cur[0], cur[1] + 1)):
                if nxt[0] < g_rows and nxt[1] < g_cols and nxt not in explored and nxt not in frontier:
                    frontier.append(nxt)
    modified = max(correct_at(origin) for origin in explored)

    neighbors = 0
    for p in range(n):
        for s, (dr, dc) in enumerate(_SIDE_STEP):
            tr, tc = true[p, 0] + dr, true[p, 1] + dc
            want = int(tr * t_cols + tc) if 0 <= tr < t_rows and 0 <= tc < t_cols else None
            r, c = loc[p, 0] + dr, loc[p, 1] + dc
            got = int(placed_id[r, c]) if 0 <= r < g_rows and 0 <= c < g_cols else -1
            neighbors += (None if got < 0 else got) == want
    return {'Direct_Standard': standard / n, 'Direct_Modified': modified / n, 'neighbor': neighbors / (4 * n), 'perfect': standard == n}


# ---------------------------------------------------------------------------------------------
# validation of the multi-output binary classifier (main.py:49-132, DefaultTrainer.validate)
# ---------------------------------------------------------------------------------------------
_METERS = ('loss', 'acc', 'f1', 'precision', 'recall')


class MeterValue(NamedTuple):
    """AverageMeter's ``val`` (the last batch's value) and ``avg`` (sum / count on this rank)."""
    val: float
    avg: float


class ValidationResult(NamedTuple):
    """The averages ``DefaultTrainer.validate`` logs after its all-reduce; ``loss`` is what it returns.  ``samples``: the
    all-reduced sample count (fp32, as the reference's meters hold it)."""
    loss: float
    acc: float
    f1: float
    precision: float
    recall: float
    samples: int


class ClassificationMeters:
    """The reference's five validation AverageMeters (loss, acc, f1, precision, recall) on the device.

    ``update(logits, targets)`` is one launch of vited_cls_metrics_update per batch (no host sync): it replaces main.py:73-93, the
    host copy of the batch and the 16 sklearn calls.  ``values()`` copies the meters to the host once, for the PRINT_FREQ log
    lines.  ``all_reduce(group)`` replaces the six ``AverageMeter.all_reduce`` calls (main.py:113-119) with ONE fp32 SUM
    all-reduce of every (sum, count), rounded to fp32 first as the reference rounds them (also at world size 1); the bad-target
    flag travels in the same reduction, so every rank raises together."""

    def __init__(self, num_classes: int = 4, device='cuda'):
        self.num_classes = int(num_classes)
        if not 1 <= self.num_classes <= 64:
            raise ValueError(f'num_classes must be in [1, 64], got {num_classes}')
        self.device = torch.device(device)
        self.meters = torch.zeros(2 * len(_METERS), dtype=torch.float64, device=self.device)   # (sum, count) per meter
        self.last = torch.zeros(len(_METERS), dtype=torch.float64, device=self.device)
        self.bad = torch.zeros(1, dtype=torch.int32, device=self.device)

    def reset(self):
        self.meters.zero_()
        self.last.zero_()
        self.bad.zero_()

    def update(self, logits: torch.Tensor, targets: torch.Tensor):
        from . import ops                                   # ops refuses CPU tensors: no CPU fallback
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f'logits must be [B, {self.num_classes}], got {tuple(logits.shape)}')
        ops.cls_metrics_update(logits, targets, self.meters, self.last, self.bad)

    def values(self) -> dict:
        """name -> MeterValue(val, avg) of each meter on this rank (one device-to-host copy)."""
        host = torch.cat([self.last, self.meters]).tolist()
        last, state = host[:len(_METERS)], host[len(_METERS):]
        return {name: MeterValue(last[k], state[2 * k] / state[2 * k + 1] if state[2 * k + 1] else 0.0)
                for k, name in enumerate(_METERS)}

    def all_reduce(self, group=None) -> ValidationResult:
        """The all-reduced averages.  Raises ValueError when a target other than 0 / 1 was seen on any rank, and when no sample
        was added on any rank.  Joins the reduction over ``group`` (None: the default group) when torch.distributed is
        initialised; otherwise the result is this process's."""
        state = torch.cat([self.meters.to(torch.float32), self.bad.to(torch.float32)])   # AverageMeter.all_reduce's fp32 tensor
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(state, op=dist.ReduceOp.SUM, group=group)
        host = state.tolist()
        if host[-1]:
            raise ValueError('validation targets must be 0 or 1: vited_cls_metrics_update saw another value')
        if not host[1]:
            raise ValueError('no validation sample was added before all_reduce')
        avg = [host[2 * k] / host[2 * k + 1] for k in range(len(_METERS))]
        return ValidationResult(*avg, samples=int(host[1]))


@torch.no_grad()
def validate_classifier(model, data_loader, *, amp: bool = True, group=None, print_freq: int | None = None,
                        log=None) -> ValidationResult:
    """``DefaultTrainer.validate`` (main.py:49-132) with its metrics on the device.

    ``model``: the classifier (a DDP wrapper too), run in eval mode under no_grad and bf16 autocast when ``amp``; its previous
    mode is restored.  ``data_loader`` yields (images, targets [B, C] of 0 / 1): batches already on the model's device are used
    as they are, host batches go through DevicePrefetcher.  ``log(idx, values)`` is called with ``ClassificationMeters.values()``
    on every batch with idx % print_freq == 0 (the only batches that wait for the device).  One all-reduce over ``group`` at the
    end; the result's ``loss`` is what the reference's validate() returns."""
    import itertools
    dev = next(model.parameters()).device
    batches = iter(data_loader)
    first = next(batches, None)
    if first is None:
        raise ValueError('the validation loader yielded no batch')
    batches = itertools.chain([first], batches)
    if not (torch.is_tensor(first[0]) and first[0].device == dev):
        batches = DevicePrefetcher(batches, dev)
    meters = None
    was_training = model.training
    model.eval()
    try:
        for idx, (images, target) in enumerate(batches):
            with torch.autocast(dev.type, dtype=torch.bfloat16, enabled=amp):
                output = model(images)
            if meters is None:
                meters = ClassificationMeters(output.shape[1], dev)
            meters.update(output, target)
            if log is not None and print_freq and idx % print_freq == 0:
                log(idx, meters.values())
    finally:
        model.train(was_training)
    return meters.all_reduce(group)


# ---------------------------------------------------------------------------------------------
# attention relevancy maps (scripts/visualise_attentions.py: Generator.generate_ours / generate_raw_attn / generate_attn_gradcam)
# ---------------------------------------------------------------------------------------------
def _handle_residual(r: torch.Tensor) -> torch.Tensor:
    """Eq. 8 + 9 of Chefer et al. (handle_residual of the script), batched: the part of a self-relevancy beyond the identity,
    rows normalised to sum 1, plus the identity.  A row that is still the identity gives 0 / 0 = NaN, which rule 10 turns into 0.
    (The script also asserts a non-negative diagonal; with the non-negative maps of rule 5 it cannot fail, and the check would
    make the device wait for the host.)"""
    eye = torch.eye(r.shape[-1], dtype=r.dtype, device=r.device)
    rest = r - eye
    return rest / rest.sum(dim=-1, keepdim=True) + eye


def relevancy_from_cams(enc_cams, dec_self_cams, dec_cross_cams, normalize_self_attention: bool = True, apply_self_in_rule_10: bool = True):
    """Relevancy propagation of ``Generator.generate_ours`` for a batch of pairs, from the head-averaged maps of rule 5
    (``get_attn_cam()`` of every attention): ``enc_cams`` depth x [B, N1, N1], ``dec_self_cams`` c_depth x [B, N2, N2],
    ``dec_cross_cams`` c_depth x [B, N2, N1].  Returns R_qi [B, N2, N1] in the maps' dtype: the relevancy of every image-1 token
    for every image-2 token (row 0: the cls token).  Order of the updates as in the script: R_ii += cam R_ii over the encoder
    blocks; then per decoder block rules 6 + 7 (both additions from the OLD R_qq and R_qi) and rule 10,
    R_qi += norm(R_qq)^T (cam norm(R_ii)) with NaN -> 0.  Plain batched torch: works on CPU tensors (fp64 in the tests) too."""
    enc_cams, dec_self_cams, dec_cross_cams = list(enc_cams), list(dec_self_cams), list(dec_cross_cams)
    if not dec_cross_cams or len(dec_self_cams) != len(dec_cross_cams):
        raise ValueError(f'relevancy_from_cams: need one self and one cross map per decoder block, got {len(dec_self_cams)} and '
                         f'{len(dec_cross_cams)}')
    ref = dec_cross_cams[0]
    if ref.dim() != 3:
        raise ValueError(f'relevancy_from_cams: maps are [B, Nq, Nk], got {tuple(ref.shape)}')
    b, n2, n1 = ref.shape
    for name, cams, shape in (('encoder', enc_cams, (b, n1, n1)), ('decoder self', dec_self_cams, (b, n2, n2)), ('decoder cross', dec_cross_cams, (b, n2, n1))):
        for cam in cams:
            if tuple(cam.shape) != shape or cam.dtype != ref.dtype or cam.device != ref.device:
                raise ValueError(f'relevancy_from_cams: a {name} map is {tuple(cam.shape)} {cam.dtype}, expected {shape} {ref.dtype}')
    kw = dict(dtype=ref.dtype, device=ref.device)
    r_ii = torch.eye(n1, **kw).expand(b, n1, n1).clone()
    r_qq = torch.eye(n2, **kw).expand(b, n2, n2).clone()
    r_qi = torch.zeros((b, n2, n1), **kw)
    for cam in enc_cams:
        r_ii = r_ii + torch.bmm(cam, r_ii)
    for cam_qq, cam_qi in zip(dec_self_cams, dec_cross_cams):
        add_qq, add_qi = torch.bmm(cam_qq, r_qq), torch.bmm(cam_qq, r_qi)
        r_qq, r_qi = r_qq + add_qq, r_qi + add_qi
        if apply_self_in_rule_10:
            nqq, nii = (_handle_residual(r_qq), _handle_residual(r_ii)) if normalize_self_attention else (r_qq, r_ii)
            add = torch.bmm(nqq.transpose(1, 2), torch.bmm(cam_qi, nii))
        else:
            add = cam_qi
        r_qi = r_qi + torch.where(torch.isnan(add), torch.zeros_like(add), add)
    return r_qi


_RELEVANCY_METHODS = ('relevance', 'raw', 'gradcam')


def _relevancy_of_store(net, method, include_cls, normalize_self_attention, apply_self_in_rule_10, propagate_dtype):
    store = net._attn_store
    if method == 'relevance':
        cams = lambda kind, n, which: [store[(kind, i, which)]['cam'].to(propagate_dtype) for i in range(n)]
        r_qi = relevancy_from_cams(cams('blocks', net.depth, 'attn'), cams('cross_blocks', net.c_depth, 'attn'),
                                   cams('cross_blocks', net.c_depth, 'cross_attn'), normalize_self_attention, apply_self_in_rule_10)
        return (r_qi if include_cls else r_qi[:, 1:, :]).to(torch.float32)
    # the last cross-attention, cls query (row 0), weighted over the heads: sum_h w[b, h] P_h[0, :]
    from . import ops
    q, k, v, do, lse = store[('cross_blocks', net.c_depth - 1, 'cross_attn')]['cam_operands']
    heads, hd = net.num_heads, net.embed_dim // net.num_heads
    weight = None                                   # 'raw': the head mean of the attention
    if method == 'gradcam':
        # mean_ij dP_h = (sum_i dO_i) . (sum_j v_j) / (Nq Nk): the per-head weight without forming dP; / H: the mean over the heads
        b, nq, nk = q.shape[0], q.shape[1], k.shape[1]
        weight = (do.float().sum(1).view(b, heads, hd) * v.float().sum(1).view(b, heads, hd)).sum(-1) / float(nq * nk * heads)
        weight = weight.contiguous()
    cam = ops.attention_cam(q[:, 0:1], k, None, None, lse[:, :, 0:1].contiguous(), heads, hd ** -0.5, mode='prob', head_weight=weight)
    cam = cam[:, 0, :]
    return cam.clamp_(min=0) if method == 'gradcam' else cam


def pair_relevancy(model, images, target=None, amp: bool = True, method: str = 'relevance', include_cls: bool = False, chunk: int | None = None,
                   normalize_self_attention: bool = True, apply_self_in_rule_10: bool = True, propagate_dtype=torch.float64):
    """Which patches made the model decide: the three generators of scripts/visualise_attentions.py for a BATCH of pairs.

    ``images`` [B, 2, 3, S, S] (float, or uint8 normalised in the patch-embedding kernel).  One forward, one backward from a one-hot
    of ``target`` (an int, or int64 [B]; None: every sample's own arg-max logit, taken on the device), with ``model.keep_cam``
    on: every attention's backward also writes its head-averaged map mean_h max(P o dP, 0) [B, Nq, Nk] from one fused kernel
    (ops.attention_cam) - no per-head N x N map exists at any time, which is what makes a batch fit.
    Returns (relevancy, logits [B, C]):
      'relevance'  Generator.generate_ours: R_qi [B, N2 - 1, N1] (all N2 rows with ``include_cls``), relevancy_from_cams;
      'raw'        generate_raw_attn: head mean of the last cross-attention, cls query, [B, N1];
      'gradcam'    generate_attn_gradcam: max(mean_h mean(dP_h) P_h, 0) of the same row, [B, N1].
    The maps are fp32; the propagation over them runs in ``propagate_dtype`` and the result is returned as fp32.  fp64 by default:
    handle_residual subtracts the identity from 1 + (sum of maps), which in fp32 loses whatever of a map lies below 6e-8.
    ``chunk`` bounds the pairs in flight.  The model's keep_cam / keep_attn switches are restored, its attention store is left
    empty and no parameter gradient is touched: under keep_cam the weight-gradient kernels are not launched, the backward returns
    no parameter gradient to autograd, and the direct accumulation into p.grad / FlatGradients.flat is off for that backward."""
    net = getattr(model, 'module', model)
    if method not in _RELEVANCY_METHODS:
        raise ValueError(f'pair_relevancy: method must be one of {_RELEVANCY_METHODS}, got {method!r}')
    if images.dim() != 5 or images.shape[1] != 2:
        raise ValueError(f'pair_relevancy: expected stacked pairs [B, 2, C, S, S], got {tuple(images.shape)}')
    if not hasattr(net, 'keep_cam'):
        raise TypeError('pair_relevancy needs the HIP VisionTransformerCustom (model.keep_cam)')
    if not any(p.requires_grad for p in net.parameters()):
        raise ValueError('pair_relevancy: the maps are recorded by the backward, which only runs for a model with trainable parameters')
    b = images.shape[0]
    chunk = b if chunk is None else int(chunk)
    if chunk <= 0:
        raise ValueError(f'pair_relevancy: chunk must be positive, got {chunk}')
    dev = images.device
    if target is not None:
        target = torch.as_tensor(target, device=dev).to(torch.int64).reshape(-1)
        if target.numel() not in (1, b):
            raise ValueError(f'pair_relevancy: target must be one class or one per pair, got {target.numel()} for {b} pairs')
        target = target.expand(b)
    saved = (net.keep_cam, net.keep_attn)
    rel, out = [], []
    try:
        net.keep_cam, net.keep_attn = True, False
        for lo in range(0, b, chunk):
            net._attn_store.clear()
            with torch.enable_grad():
                with torch.autocast(dev.type, dtype=torch.bfloat16, enabled=amp):
                    logits = net(images[lo:lo + chunk])
                index = target[lo:lo + chunk] if target is not None else logits.detach().argmax(dim=-1)
                one_hot = torch.zeros_like(logits).scatter_(1, index.unsqueeze(1), 1.0)
                logits.backward(one_hot)
            rel.append(_relevancy_of_store(net, method, include_cls, normalize_self_attention, apply_self_in_rule_10, propagate_dtype))
            out.append(logits.detach())
    finally:
        net.keep_cam, net.keep_attn = saved
        net._attn_store.clear()
    return (rel[0], out[0]) if len(rel) == 1 else (torch.cat(rel), torch.cat(out))
