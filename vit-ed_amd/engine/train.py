"""The training step (misc/engine.py:183-257, misc/utils.py:206-232, misc/optimizer.py:10-46): optimizer factory, the reference's
scaler call shape, ``TrainStep`` (eager or replayed as hipGraphs), its meters on the device, and ``TwoStageTrainStep``, the mined
two-stage step of hisfrag.py / michigan.py on the same machinery."""
from __future__ import annotations

import gc

import torch
import torch.distributed as dist

from .. import ops
from ..functions import shadows_of
from ..lr_scheduler import Scheduler, build_scheduler  # noqa: F401  (build_scheduler: misc/lr_scheduler.py, re-exported by engine)
from .distributed import FlatGradients
from .metrics import MeterValue
from .mining import mine_pairs_device, mined_bce_fused


def param_groups_no_decay_1d(model):
    decay, no_decay = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        (no_decay if (p.ndim == 1 or name.endswith('.bias')) else decay).append(p)
    return [{'params': decay}, {'params': no_decay, 'weight_decay': 0.}]


def build_optimizer(config, model, capturable: bool = False, fused_hip: bool | None = None, skip_nonfinite: bool = False,
                    ema_decay: float | None = None, ema_warmup: bool = False):
    """misc/optimizer.py:10-46: AdamW / Nesterov SGD with the no-decay group for 1-D parameters and ``*.bias``.

    On a GPU model they are ``optim.FlatAdamW`` / ``optim.FlatSGD`` (the HIP multi-tensor kernels: clip + update + bf16
    weight-shadow refresh in one pass, hipGraph-replayable with a per-iteration learning rate); ``fused_hip=False`` gives
    ``torch.optim.AdamW(fused=True)`` / ``torch.optim.SGD`` instead, with ``capturable`` forwarded to AdamW (a torch optimizer
    captured into a hipGraph must be built with capturable=True, and TrainStep keeps its learning rate in a device tensor).
    ``skip_nonfinite=True`` (HIP optimizers only) leaves out an update whose gradient norm is inf or NaN, which is what
    ``GradScaler.step`` does in the reference's loop (misc/utils.py:206-226).  ``ema_decay`` / ``ema_warmup`` (HIP optimizers only)
    keep timm's ``--model-ema`` average of the parameters inside the update launch (optim.py); None keeps none.

    ``'lamb'`` (or ``'fused_lamb'``, the spelling of the reference drivers' ``--optim`` help) is ``optim.FlatLAMB`` with EPS, BETAS,
    BASE_LR, WEIGHT_DECAY and the no-decay group as for AdamW.  It exists as a HIP optimizer only: on a CPU model, or with
    ``fused_hip=False``, the name is unknown.

    ``'lion'`` is ``optim.FlatLion`` with BASE_LR, BETAS, WEIGHT_DECAY and the no-decay group (EPS is unused), HIP only in the same
    way.  The config's values are passed as they are: Lion wants a rate 3-10x smaller and a decay 3-10x larger than AdamW's.

    ``'muon'`` is ``optim.FlatMuon``, HIP only in the same way, with three groups: the 2-D weights under ``blocks.*`` and
    ``cross_blocks.*`` as the Muon group (BASE_LR, WEIGHT_DECAY, Muon's own momentum of 0.95 - OPTIMIZER.MOMENTUM is SGD's key - and
    ``adjust_lr_fn='match_rms_adamw'``, so that the rates the configs hold for AdamW carry over); everything else that is decayed (the
    head, the patch projection, ``pos_embed``, ``cls_token``) as an aux AdamW group with BETAS and EPS; the no-decay group as the second
    aux group."""
    name = config.TRAIN.OPTIMIZER.NAME.lower()
    groups = param_groups_no_decay_1d(model)
    on_gpu = all(p.is_cuda for g in groups for p in g['params'])
    hip = on_gpu and (fused_hip is None or fused_hip)
    lamb, lion, muon = name in ('lamb', 'fused_lamb'), name == 'lion', name == 'muon'
    if name not in ('adamw', 'sgd') and not ((lamb or lion or muon) and hip):
        raise ValueError(f'unknown optimizer {name}' + (f' ({"LAMB" if lamb else "Lion" if lion else "Muon"} exists as a HIP optimizer only: a GPU model and '
                                                         f'fused_hip in (None, True))' if lamb or lion or muon else ''))
    if skip_nonfinite and not hip:
        raise ValueError('skip_nonfinite=True needs the HIP optimizers (a GPU model and fused_hip in (None, True)): the torch '
                         'optimizers have no such check')
    if ema_decay is not None and not hip:
        raise ValueError('ema_decay needs the HIP optimizers (a GPU model and fused_hip in (None, True)): the average is kept by their '
                         'update kernel')
    ema = dict(ema_decay=ema_decay, ema_warmup=ema_warmup)
    if muon:
        from ..optim import FlatMuon
        decay, no_decay = (set(map(id, g['params'])) for g in groups)
        in_blocks = {id(p) for n, p in model.named_parameters() if n.startswith(('blocks.', 'cross_blocks.'))}
        params = [p for g in groups for p in g['params']]
        pick = lambda keep: [p for p in params if keep(p)]
        muon_ids = {id(p) for p in params if id(p) in decay and id(p) in in_blocks and p.ndim == 2}
        return FlatMuon([{'params': pick(lambda p: id(p) in muon_ids), 'use_muon': True},
                         {'params': pick(lambda p: id(p) in decay and id(p) not in muon_ids)},
                         {'params': pick(lambda p: id(p) in no_decay), 'weight_decay': 0.}],
                        lr=config.TRAIN.BASE_LR, momentum=0.95, nesterov=True, weight_decay=config.TRAIN.WEIGHT_DECAY,
                        adjust_lr_fn='match_rms_adamw', betas=tuple(config.TRAIN.OPTIMIZER.BETAS), adam_eps=config.TRAIN.OPTIMIZER.EPS,
                        model=model, skip_nonfinite=skip_nonfinite, **ema)
    if lion:
        from ..optim import FlatLion
        return FlatLion(groups, lr=config.TRAIN.BASE_LR, betas=tuple(config.TRAIN.OPTIMIZER.BETAS), weight_decay=config.TRAIN.WEIGHT_DECAY,
                        model=model, skip_nonfinite=skip_nonfinite, **ema)
    if name == 'adamw' or lamb:
        kw = dict(eps=config.TRAIN.OPTIMIZER.EPS, betas=tuple(config.TRAIN.OPTIMIZER.BETAS), lr=config.TRAIN.BASE_LR,
                  weight_decay=config.TRAIN.WEIGHT_DECAY)
        if lamb:
            from ..optim import FlatLAMB
            return FlatLAMB(groups, model=model, skip_nonfinite=skip_nonfinite, **ema, **kw)
        if hip:
            from ..optim import FlatAdamW     # here, not at the top: optim imports this package (FlatGradients)
            # the model's bf16 weight shadows are refreshed by the update kernel
            return FlatAdamW(groups, model=model, skip_nonfinite=skip_nonfinite, **ema, **kw)
        if on_gpu:
            return torch.optim.AdamW(groups, fused=True, capturable=capturable, **kw)
        return torch.optim.AdamW(groups, **kw)
    kw = dict(momentum=config.TRAIN.OPTIMIZER.MOMENTUM, nesterov=True, lr=config.TRAIN.BASE_LR, weight_decay=config.TRAIN.WEIGHT_DECAY)
    if hip:
        from ..optim import FlatSGD
        return FlatSGD(groups, model=model, skip_nonfinite=skip_nonfinite, **ema, **kw)
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


def _decoder_only_parameters(model):
    """Parameters whose gradient is complete once the decoder + head backward has run: everything except the
    encoder blocks and the tensors both image paths share (patch_embed.*, pos_embed get gradient from the
    encoder too, vision_transformer.py:379,391-392)."""
    out = []
    for name, p in model.named_parameters():
        if name.startswith(('cross_blocks.', 'norm.', 'fc_norm.', 'head.')) or name == 'cls_token':
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
    * ``lr_scheduler``: one of ``lr_scheduler.py``'s classes (``engine.build_scheduler``) on ``optim.FlatAdamW`` / ``optim.FlatSGD`` is
      stepped on the device: a one-workgroup launch behind the update (part of the captured update graph) computes ``_get_lr(n)`` from a
      device counter that starts at ``start_update`` and writes it into the optimizer's device array, so no rate is uploaded per
      iteration; ``step_update(n)`` on the host then only keeps ``param_groups`` current for the log line and checkpoints.
      ``lr_scheduler.on_device = False``, any other scheduler object and the torch optimizers are stepped by the host.
    * An optimizer built with ``ema_decay`` averages the parameters inside its update launch, eagerly and in replay alike: the flat
      average is one more buffer the captured update graph bakes in (allocated once, when the optimizer is bound here), and a changed
      ``optimizer.ema_decay`` reaches a replayed update through ``sync_hyperparameters``.  ``with optimizer.swap_ema():`` evaluates on
      the averaged weights; ``step`` raises inside it.
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
      tensors in place.
    * Patch dropout (``patch_drop_rate`` > 0, training mode) works the same way: the keys and the ranking kernel that turns them into
      keep indices are part of the captured graph, ``model.last_patch_keep`` is a static buffer that holds the latest replay's
      indices, and ``step.patch_keep`` = a ``PatchKeep`` of static tensors forces them.  The shortened sequences have a fixed length
      (the rate is the model's), so the captured shapes never change.
    * Position dropout (``pos_drop_rate`` > 0, training mode) likewise: the draw of the two seeds is part of the captured graph, the
      dropout kernel reads them from device memory, so every replay masks anew, ``model.last_pos_drop`` is a static buffer that holds
      the latest replay's seeds, and ``step.pos_drop`` = a ``PosDropSeeds`` of static tensors forces them.  No mask is stored between
      the forward and the backward graph: the encoder's backward regenerates it from the seed."""

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
        self.patch_keep = None      # forced patch-dropout indices (a PatchKeep); None: the model draws when it should
        self.pos_drop = None        # forced position-dropout seeds (a PosDropSeeds); None: the model draws when it should
        self.forward_fn = forward_fn or (lambda m, x: m(x, **self._forced()))
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
        # a schedule of lr_scheduler.py on a HIP optimizer is stepped by a launch behind the update (its rates never pass through the
        # host); every other combination - a scheduler that only has step_update, on_device = False, a torch optimizer, a rule the
        # device table cannot state - is stepped by the host through param_groups, as before.  After bind_flat: the launch writes
        # into the hyper-parameter array that binding (re-)allocated.
        self.lr_on_device = (self.hip_opt and isinstance(lr_scheduler, Scheduler) and lr_scheduler.on_device is not False
                          and lr_scheduler.device_capable())
        if self.lr_on_device:
            lr_scheduler.attach(optimizer, self.num_updates)
        elif isinstance(lr_scheduler, Scheduler):
            lr_scheduler.detach()
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

    def _forced(self):
        """The keyword arguments that hand the forced scales / indices of this step to the model (none: it draws for itself)."""
        forced = {} if self.drop_path is None else dict(drop_path=self.drop_path)
        if self.patch_keep is not None:
            forced['patch_keep'] = self.patch_keep
        if self.pos_drop is not None:
            forced['pos_drop'] = self.pos_drop
        return forced

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
            forced = self._forced()
            feats = self.model(x[:, 0], forward_first_part=True, **forced)
            leaf = feats.detach().requires_grad_(True)
            out = self.model(leaf, x[:, 1], **forced)
            loss = self._loss(out, y)
        loss.backward()
        return loss.detach(), feats, leaf.grad

    @staticmethod
    def _enc_bwd(feats, dfeats):
        feats.backward(dfeats)

    def _two_stage(self, x):
        """Whether the backward of this batch is driven in two stages (``_fwd_dec_bwd`` + ``_enc_bwd``) or as one (``_fwd_bwd``)."""
        return self.split and torch.is_tensor(x) and x.dim() == 5

    def _meter_loss(self, loss, y):
        if self.meters is not None:
            self.meters.update_loss(loss, y.counts[3] if hasattr(y, 'counts') else y.shape[0])    # MinedPairs: the real pairs

    def _update(self):
        if self.hip_opt:
            norm = self.optimizer.step_flat(self.clip_grad)      # clip + update + shadow refresh + zero: one pass
            if self.lr_on_device:
                self.lr_scheduler.step_device()                  # the rate of the NEXT update, from the device counter
        else:
            norm = self.flat.clip_(self.clip_grad) if self.clip_grad is not None else torch.linalg.vector_norm(self.flat.flat)
            self.optimizer.step()
            self._refresh_shadows()       # the bf16 weight shadows follow the update (eval right after training sees them)
            self.flat.zero()
        return norm

    def _refresh_shadows(self):
        caches = shadows_of(self.model)
        if caches:
            params = list(self.model.parameters())
            for cache in caches:
                cache.refresh(params)

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
        if self.hip_opt and self.optimizer.ema_swapped:
            raise RuntimeError('TrainStep.step: not inside `with optimizer.swap_ema():` (the parameters hold the averaged weights)')
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
        if self._two_stage(x):
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
        if not torch.is_tensor(x):
            raise TypeError('TrainStep(use_graph=True) replays on a static input tensor: pass use_graph=False for structured batches')
        self._static_x, self._static_y = x.clone(), y.clone()
        self._sync_lr()
        # A dead TrainStep is a reference cycle (its default forward_fn closes over it), so the graphs it holds wait for the cyclic
        # collector - which may run whenever an allocation tips it, also in the autograd thread in the middle of this capture, where
        # destroying a hipGraph is not permitted and ends the process.  torch.cuda.graph no longer collects on entry: do it here.
        gc.collect()
        torch.cuda.synchronize()
        ops.pin_workspace()               # captured kernels bake buffer addresses in: later growth must not free them
        for cache in shadows_of(self.model):
            cache.pin()
        split = self._two_stage(x)
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


class TwoStageTrainStep(TrainStep):
    """The step ``hisfrag.py`` / ``michigan.py`` train with (hisfrag.py:117-159, michigan.py:120-160) as one object, eager or replayed:
    ``step(samples [n, C, S, S], targets integer [n])`` - what the loader yields - mines the pairs on the device
    (``mine_pairs_device``, ``capacity`` rows), runs the encoder once per image, the decoder on the pair indices
    (``model(feats, samples, x2_index=groups[:, 0], x1_index=segments)``), takes ``mined_bce_fused(..., scale=1 / accumulation_steps)``
    and runs the decoder's backward; then the encoder's backward from d feats, and from there on everything is ``TrainStep``: the two
    all-reduce buckets (the decoder-only one under the encoder's backward), the fused update, the device schedule, the meters
    (``counts[3]``, the real pairs, as ``n``).  ``michigan.py`` is ``neg_per_pos=1.0, ordered_negatives=True, reduction='sum'``.

    * ``use_graph=True`` captures, after two eager updates, mining + encoder forward + decoder forward + loss + decoder backward +
      loss meter | encoder backward | update, and replays them from static copies of ``samples`` and ``targets``; no host read
      anywhere, so the host runs ahead of the device.  The batch shape is fixed by the capture.
    * The keys of the negatives' random subset come from the device's default generator inside the captured region: every replay
      mines anew.  ``step.mine_keys`` = an fp32 [n * n] tensor forces them (tests, reproducing a step); a captured graph reads that
      tensor in place.  ``step.last_mined`` is the ``MinedPairs`` of the latest call (static buffers under replay).
    * Live ``drop_path_rate`` / ``patch_drop_rate`` / ``pos_drop_rate`` draw inside the step, per image in the encoder and per pair in
      the decoder.  Forcing them per stage is not offered: a non-None ``step.drop_path`` / ``patch_keep`` / ``pos_drop`` raises."""

    def __init__(self, model, optimizer, *, capacity, neg_per_pos=2.0, ordered_negatives=False, reduction='mean', clip_grad=5.0, amp=True,
                 use_graph=False, compress_bf16=False, accumulation_steps=1, lr_scheduler=None, overlap=True, group=None, start_update=0,
                 meters=False, forward_fn=None, criterion=None):
        if forward_fn is not None or criterion is not None:
            raise ValueError('TwoStageTrainStep: forward_fn and criterion are fixed here (the pair-indexed decoder call and '
                             'mined_bce_fused); use TrainStep for a forward or a loss of your own')
        if not getattr(model, 'supports_x1_index', False):
            raise ValueError('TwoStageTrainStep: model must take the pair-indexed decoder call model(feats, x2, x2_index=..., x1_index=...) '
                             '(supports_x1_index)')
        capacity = int(capacity)
        if not 1 <= capacity <= ops.MINE_MAX_CAPACITY:
            raise ValueError(f'TwoStageTrainStep: capacity must lie in [1, {ops.MINE_MAX_CAPACITY}] (the mining kernel\'s rows), got {capacity}')
        if reduction not in ('mean', 'sum'):
            raise ValueError(f"TwoStageTrainStep: reduction must be 'mean' or 'sum', got {reduction!r}")
        neg_per_pos = float(neg_per_pos)
        if not 0.0 <= neg_per_pos < float('inf'):
            raise ValueError(f'TwoStageTrainStep: neg_per_pos must be a finite number >= 0, got {neg_per_pos}')
        super().__init__(model, optimizer, clip_grad=clip_grad, amp=amp, use_graph=use_graph, compress_bf16=compress_bf16,
                         accumulation_steps=accumulation_steps, lr_scheduler=lr_scheduler, overlap=overlap, group=group,
                         start_update=start_update, meters=meters)
        self.capacity, self.neg_per_pos, self.ordered_negatives, self.reduction = capacity, neg_per_pos, bool(ordered_negatives), reduction
        self.mine_keys = None       # forced mining keys (fp32 [n * n]); None: drawn on the device in every call
        self.last_mined = None      # the MinedPairs of the latest call

    def _two_stage(self, x):
        return True

    def _check_batch(self, samples, targets):
        """Everything ``step`` refuses, before any launch."""
        for name in ('drop_path', 'patch_keep', 'pos_drop'):
            if getattr(self, name) is not None:
                raise ValueError(f'TwoStageTrainStep: step.{name} cannot be forced here (the two stages draw per image and per pair); '
                                 f'leave it None')
        if not torch.is_tensor(samples) or samples.dim() != 4:
            raise ValueError(f'TwoStageTrainStep: samples must be images [n, C, S, S], got '
                             f'{tuple(samples.shape) if torch.is_tensor(samples) else type(samples).__name__}')
        n = samples.shape[0]
        if not torch.is_tensor(targets) or targets.dtype.is_floating_point or targets.dtype == torch.bool or targets.numel() != n:
            raise ValueError(f'TwoStageTrainStep: targets must be {n} integer labels, one per image of samples, got '
                             f'{f"{targets.dtype} {tuple(targets.shape)}" if torch.is_tensor(targets) else type(targets).__name__}')
        if samples.is_cuda and n > ops.mine_pairs_max_images():
            raise ValueError(f'TwoStageTrainStep: samples holds {n} images, the mining kernel takes at most {ops.mine_pairs_max_images()}')
        k = self.mine_keys
        if k is not None and (not torch.is_tensor(k) or k.dtype != torch.float32 or k.numel() != n * n or k.device != targets.device
                              or not k.is_contiguous()):
            raise ValueError(f'TwoStageTrainStep: mine_keys must be {n * n} contiguous float32 values on {targets.device}, got '
                             f'{f"{k.dtype} {tuple(k.shape)} on {k.device}" if torch.is_tensor(k) else type(k).__name__}')

    def _fwd_dec_bwd(self, x, y):
        """Stage 1: mining, encoder forward per image, decoder + head forward per pair, fused loss, decoder backward.
        Returns (loss, features, d loss / d features)."""
        with torch.autocast(self.device_type, dtype=torch.bfloat16, enabled=self.amp):
            mined = mine_pairs_device(y, self.capacity, neg_per_pos=self.neg_per_pos, ordered_negatives=self.ordered_negatives,
                                      keys=self.mine_keys)
            feats = self.model(x, forward_first_part=True)
            leaf = feats.detach().requires_grad_(True)
            out = self.model(leaf, x, x2_index=mined.groups[:, 0], x1_index=mined.segments)
            loss = mined_bce_fused(out, mined, self.reduction, scale=1.0 / self.accum)
        loss.backward()
        self.last_mined = mined
        return loss.detach(), feats, leaf.grad

    def _meter_loss(self, loss, y):
        super()._meter_loss(loss, self.last_mined)        # n = counts[3], the real pairs

    def step(self, samples, targets):
        """One call of the loop body on what the loader yields.  Returns the (micro-batch) loss; ``last_norm`` holds the gradient norm
        of the last update, ``last_mined`` the pairs of this call."""
        self._check_batch(samples, targets)
        return super().step(samples, targets)
