"""The learning-rate range test of the reference's ``lr_finder.py`` (ignite's ``FastaiLRFinder``: an exponential sweep of the rate while
the ordinary training step runs, a smoothed loss, a stop on divergence, a suggestion at the steepest descent) with every per-iteration
decision on the device (csrc/lr_finder.hip): ``LRRangeTest`` owns the buffers and queues one launch per iteration
behind the step, ``find_lr`` is the loop, and the host neither reads a loss nor sets a rate while it runs."""
from __future__ import annotations

import math
from typing import NamedTuple

import torch
import torch.distributed as dist

from .. import ops
from ..functions import shadows_of
from .train import TrainStep

LR_FINDER_MAX_ITER = 1 << 16       # the capacity of a history: 65,536 rows of three doubles


class LRFinderResult(NamedTuple):
    lrs: torch.Tensor            # fp64 [iterations] on the CPU: the rate of group 0 in every recorded iteration
    losses: torch.Tensor         # fp64 [iterations]: the raw losses
    smoothed: torch.Tensor       # fp64 [iterations]: the smoothed losses
    suggestion: float | None     # the rate at the steepest descent of the smoothed loss; None with fewer than two rows
    state: int                   # ops.LRF_DONE, LRF_DIVERGED, LRF_NONFINITE - or LRF_RUNNING where the loader ran out first
    iterations: int              # rows recorded: the halting iteration is the last one


class LRRangeTest:
    """One range test on a bound fused optimizer (``optim.FlatAdamW`` / ``FlatSGD`` / ``FlatLAMB`` / ``FlatLion`` / ``FlatMuon``): iteration i of group g runs at
    ``start_g * (end_g / start_g) ** (i / num_iter)``.  A scalar ``start_lr`` / ``end_lr`` gives ``value * lr_scale`` of every group, as
    ``TrainStep.set_lr`` does; a sequence gives one value per group.

    Building it puts ``start_g`` into ``param_groups`` and (rounded to fp32) into the optimizer's device array - the rate of iteration
    0.  From then on ``record(loss)`` - one launch on the current stream, on the device loss of the iteration that just ran - writes
    the history row, the smoothed and the best loss, the halt state and the next iteration's rate into the array's rate words
    (``hyper_lr_words()``); once halted it writes 0.0 there, at which the optimizers leave finite parameters where they are, so the
    host may look as seldom as it likes.  ``param_groups`` are not touched between two ``state()`` calls, so ``sync_hyperparameters``
    sees nothing to upload; ``state()`` copies the words the kernel wrote into them and tells the optimizer (``mark_lr_on_device``).
    Re-binding the optimizer (a second ``TrainStep`` on it, ``load_state_dict``) allocates or re-uploads the array: not during a test."""

    def __init__(self, optimizer, num_iter, start_lr=1e-7, end_lr=1e-2, smooth_f=0.05, diverge_th=5.0):
        name = type(self).__name__
        if not (hasattr(optimizer, 'hyper_lr_words') and hasattr(optimizer, 'mark_lr_on_device')):
            raise NotImplementedError(f'{name}: the rates are written on the device into the hyper-parameter array of a fused optimizer - '
                                      f'optim.FlatMuon / optim.FlatLion / optim.FlatLAMB / optim.FlatAdamW / optim.FlatSGD; {type(optimizer).__name__} has none (engine.build_optimizer gives the HIP optimizers '
                                      f'for a GPU model)')
        if getattr(optimizer, '_hyper', None) is None:
            raise RuntimeError(f'{name}: the optimizer has no device hyper-parameter array yet (bind_flat first; engine.TrainStep does)')
        num_iter = int(num_iter)
        if not 1 <= num_iter <= LR_FINDER_MAX_ITER:
            raise ValueError(f'{name}: num_iter {num_iter} is outside [1, {LR_FINDER_MAX_ITER}], the capacity of the history')
        smooth_f, diverge_th = float(smooth_f), float(diverge_th)
        if not 0.0 <= smooth_f <= 1.0:
            raise ValueError(f'{name}: smooth_f {smooth_f} is outside [0, 1]')
        if not diverge_th > 1.0:
            raise ValueError(f'{name}: diverge_th {diverge_th} must be above 1')
        groups = optimizer.param_groups
        ends = []
        for which, value in (('start_lr', start_lr), ('end_lr', end_lr)):
            if isinstance(value, (list, tuple)):
                if len(value) != len(groups):
                    raise ValueError(f'{name}: {which} has {len(value)} values for {len(groups)} parameter groups')
                per_group = [float(v) for v in value]
            else:
                per_group = [float(value) * g.get('lr_scale', 1.0) for g in groups]
            if not all(v > 0.0 and math.isfinite(v) for v in per_group):
                raise ValueError(f'{name}: {which} must be positive and finite in every group, got {per_group}')
            ends.append(per_group)
        self.start, self.end = ends
        if not all(a < b for a, b in zip(self.start, self.end)):
            raise ValueError(f'{name}: start_lr must lie below end_lr in every group, got {self.start} and {self.end}')
        self.optimizer, self.num_iter, self.smooth_f, self.diverge_th = optimizer, num_iter, smooth_f, diverge_th
        dev = optimizer._hyper.device
        self.rows = 0              # rows recorded as of the last ``state()``
        self._first, self._stride = optimizer.hyper_lr_words()
        self._state = torch.zeros(ops.LRF_STATE_WORDS, dtype=torch.int64, device=dev)
        self._history = torch.zeros(num_iter, ops.LRF_HISTORY_COLS, dtype=torch.float64, device=dev)
        self._start = torch.tensor(self.start, dtype=torch.float64).to(dev)
        self._end = torch.tensor(self.end, dtype=torch.float64).to(dev)
        # iteration 0 runs at exactly start_g: through param_groups and one ordinary upload, after which the host holds what the device does
        for g, lr in zip(groups, self.start):
            g['lr'] = lr
        optimizer.sync_hyperparameters()

    def record(self, loss: torch.Tensor):
        """Queue the record of the iteration that just ran on its device loss (one fp32 element).  No host synchronisation."""
        loss = loss.detach()
        if loss.dtype != torch.float32:
            loss = loss.float()
        ops.lr_finder_step(loss, self._state, self._history, self._start, self._end, self.num_iter, self.smooth_f, self.diverge_th,
                           self.optimizer._hyper, self._first, self._stride)

    def state(self) -> int:
        """The halt state (``ops.LRF_RUNNING`` / ``LRF_DONE`` / ``LRF_DIVERGED`` / ``LRF_NONFINITE``): one host read - the two counters
        and the groups' rate words together, all exact in a double - which also brings ``param_groups`` up to the rates the kernel wrote."""
        words = self.optimizer._hyper[self._first::self._stride][:len(self.start)]
        h = torch.cat([self._state[:2].to(torch.float64), words.to(torch.float64)]).tolist()
        self.rows = int(h[0])
        for g, lr in zip(self.optimizer.param_groups, h[2:]):
            g['lr'] = lr
        self.optimizer.mark_lr_on_device()
        return int(h[1])

    def history(self) -> torch.Tensor:
        """fp64 [rows, 3] on the CPU: (rate of group 0, loss, smoothed loss) of every recorded iteration, the halting one last."""
        self.state()
        return self._history[:self.rows].cpu()

    def suggestion(self, skip_start: int = 0, skip_end: int = 0) -> float:
        """The rate at the steepest descent of the smoothed loss (``ops.lr_suggestion``); fewer than two rows raise ValueError."""
        h = self.history()
        return ops.lr_suggestion(h[:, 0].numpy(), h[:, 2].numpy(), skip_start, skip_end)


class _Snapshot:
    """What a sweep moves, copied before it and copied back IN PLACE after it: every buffer keeps its address, so graphs captured before
    or during the sweep stay valid, and nothing is re-bound (``bind_flat`` would allocate a fresh hyper-parameter array behind the
    captured update's back)."""

    def __init__(self, step):
        opt = step.optimizer
        self.step, self.params = step, [p for p in step.model.parameters()]
        self.values = [p.detach().clone() for p in self.params]
        self.bufs = {n: b.clone() for n, b in opt._bufs.items()}
        self.hyper = opt._hyper.clone()                   # the EMA counter hyper[5] with it
        self.ema = None if opt.ema is None else opt.ema.clone()
        self.workspace = opt._ws.clone()                  # scratch, but for FlatLAMB.trust_ratios, which reads its ratio table
        self.seen = None if opt._hyper_seen is None else list(opt._hyper_seen)
        self.rates = [g['lr'] for g in opt.param_groups]
        self.state_keys = {id(p): set(opt.state[p]) if p in opt.state else None for g in opt.param_groups for p in g['params']}
        self.installed = getattr(opt, '_state_installed', None)
        self.shadows = [(cache, cache.snapshot(self.params)) for cache in shadows_of(step.model)]
        self.num_updates = step.num_updates
        self.meters = None if step.meters is None else step.meters.state.clone()

    @torch.no_grad()
    def restore(self):
        step, opt = self.step, self.step.optimizer
        for p, v in zip(self.params, self.values):
            p.copy_(v)
        for n, b in self.bufs.items():
            opt._bufs[n].copy_(b)
        opt._hyper.copy_(self.hyper)
        if self.ema is not None:
            opt.ema.copy_(self.ema)
        opt._ws.copy_(self.workspace)
        opt._hyper_seen = self.seen
        for g, lr in zip(opt.param_groups, self.rates):
            g['lr'] = lr
        for g in opt.param_groups:                 # state entries the sweep's first update installed (FlatSGD) leave again
            for p in g['params']:
                keys = self.state_keys[id(p)]
                if keys is None:
                    opt.state.pop(p, None)
                else:
                    for k in [k for k in opt.state[p] if k not in keys]:
                        del opt.state[p][k]
        if self.installed is not None:
            opt._state_installed = self.installed
        before = {id(cache): saved for cache, saved in self.shadows}
        for cache in shadows_of(step.model):       # a cache the sweep created has no copies: its shadows are recast from the parameters
            cache.restore(before.get(id(cache), {}), self.params)
        step.num_updates = self.num_updates
        if self.meters is not None:
            step.meters.state.copy_(self.meters)


def find_lr(step, loader, num_iter=None, start_lr=1e-7, end_lr=1e-2, smooth_f=0.05, diverge_th=5.0, restore=True, poll_every=16,
            group=None) -> LRFinderResult:
    """``lr_finder.py``'s range test over ``step`` - an ``engine.TrainStep`` or ``TwoStageTrainStep`` on one of ``optim.py``'s fused
    optimizers, built without an ``lr_scheduler`` and with ``accumulation_steps == 1``, ``use_graph`` either way - and ``loader``,
    anything that yields ``(x, y)``; ``num_iter=None`` takes ``len(loader)``.  Per iteration: ``loss = step.step(x, y)``, then
    ``LRRangeTest.record(loss)``, and nothing else - the rate of the next iteration, the smoothed and the best loss, the stop and the
    history are the kernel's.  The halt state is read every ``poll_every`` iterations (0: only at the end) and the loop ends at the
    first poll that sees a halt; the iterations in between ran at a rate of 0 and recorded nothing.  With ``group``, or an initialised
    default group of more than one rank, the loss is all-reduced to its mean on the device before the record, so every rank takes
    the same decisions and sets the same rates.

    ``restore=True`` puts back, in place and bit for bit, the parameters, the optimizer's state with its step and skip counters, the
    parameter average (``ema_decay``) with its counter, the rate words and ``param_groups``, the weight shadows, ``step.num_updates`` and the step's meters; captured graphs stay valid.  Random
    draws the step made (mining keys, dropout) are not rewound.  ``restore=False`` leaves the swept state - the rate words at 0 after a
    halt - and after a halt on a non-finite loss (``LRF_NONFINITE``) the parameters are not meaningful: the update that followed the
    loss may have written non-finite values, which a rate of 0 does not undo.

    Plotting is the caller's: ``result.lrs`` against ``result.smoothed`` on a logarithmic axis is ``FastaiLRFinder.plot``."""
    if not isinstance(step, TrainStep):
        raise TypeError(f'find_lr: step must be an engine.TrainStep or TwoStageTrainStep, got {type(step).__name__}')
    if step.lr_scheduler is not None:
        raise ValueError('find_lr: the step was built with an lr_scheduler, which would set the rates the sweep sets: build it without one')
    if step.accum != 1:
        raise ValueError(f'find_lr: the step was built with accumulation_steps {step.accum}: the sweep sets a rate per call, build it with 1')
    if not step.hip_opt:
        raise NotImplementedError(f'find_lr: the rates are written on the device into the hyper-parameter array of a fused optimizer - '
                                  f'optim.FlatMuon / optim.FlatLion / optim.FlatLAMB / optim.FlatAdamW / optim.FlatSGD; {type(step.optimizer).__name__} has none')
    if num_iter is None:
        num_iter = len(loader)
    poll_every = int(poll_every)
    if poll_every < 0:
        raise ValueError(f'find_lr: poll_every {poll_every} must not be negative (0: read the state only at the end)')
    if int(num_iter) > LR_FINDER_MAX_ITER:
        raise ValueError(f'find_lr: num_iter {int(num_iter)} is above {LR_FINDER_MAX_ITER}, the capacity of the history')
    saved = _Snapshot(step) if restore else None
    test = LRRangeTest(step.optimizer, num_iter, start_lr, end_lr, smooth_f, diverge_th)
    world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
    mean = torch.zeros(1, dtype=torch.float32, device=step.optimizer._hyper.device) if world > 1 else None
    try:
        for it, (x, y) in zip(range(1, test.num_iter + 1), loader):
            loss = step.step(x, y)
            if mean is not None:
                mean.copy_(loss.detach().reshape(1))
                dist.all_reduce(mean, op=dist.ReduceOp.SUM, group=group)
                loss = mean.div_(world)
            test.record(loss)
            if poll_every and it % poll_every == 0 and test.state() != ops.LRF_RUNNING:
                break
        halt = test.state()
        history = test._history[:test.rows].cpu()
    finally:
        if saved is not None:
            saved.restore()
    lrs, losses, smoothed = history[:, 0].clone(), history[:, 1].clone(), history[:, 2].clone()
    suggestion = ops.lr_suggestion(lrs.numpy(), smoothed.numpy()) if test.rows >= 2 else None
    return LRFinderResult(lrs, losses, smoothed, suggestion, halt, test.rows)
