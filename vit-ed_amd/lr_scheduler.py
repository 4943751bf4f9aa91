"""``build_scheduler`` and the four per-iteration learning-rate schedules of the reference's loop (misc/lr_scheduler.py:16-62 over
``timm.scheduler``; stepped by misc/engine.py:228), written out here because timm is not a dependency of this package.  They work
with any ``torch.optim.Optimizer`` on the host; with ``optim.FlatAdamW`` / ``optim.FlatSGD`` under ``engine.TrainStep`` they are stepped
on the device by one small launch behind the update (``attach`` / ``step_device``; csrc/lr_schedule.hip).

The rule, restated (timm's ``Scheduler`` with ``t_in_epochs=False`` and no noise):

* ``base_values[g] = group.setdefault('initial_lr', group['lr'])``.  The constructor writes the base values into the groups, then,
  with ``warmup_t`` set, ``warmup_lr_init``; ``warmup_steps[g] = (base_values[g] - warmup_lr_init) / warmup_t`` (1 without warm-up).
* ``update_groups(v)`` writes ``v * group['lr_scale']`` into ``group['lr']`` where the group has an ``'lr_scale'``, else ``v``; a scalar
  goes to every group.
* ``step_update(num_updates)`` sets ``_get_lr(num_updates)``; ``step(epoch)`` does nothing.
* ``state_dict()`` is every instance attribute except the optimizer (and, of this module's own, the device binding and
  ``on_device``: they belong to the process, not to the schedule); ``load_state_dict(d)`` is
  ``self.__dict__.update(d)``, so a dict saved by timm's classes loads, unknown keys included.

``_get_lr(t)`` per group, in Python floats, in exactly this operation order (``base = base_values[g]``):

* all four, ``t < warmup_t``:   ``warmup_lr_init + t * warmup_steps[g]``
* cosine:      ``t -= warmup_t`` under ``warmup_prefix``; ``i = t // t_initial``; ``t_curr = t - t_initial * i``; for ``i < cycle_limit``
               ``lr_min + 0.5 * (base * cycle_decay ** i - lr_min) * (1 + math.cos(math.pi * t_curr / t_initial))``, else ``lr_min``
               (``cycle_decay`` is 1; ``cycle_mul != 1`` and ``k_decay != 1`` raise ``NotImplementedError``)
* linear:      ``t -= warmup_t``; ``total = t_initial - warmup_t``; ``base - (base - base * lr_min_rate) * (t / total)`` - no clamp
               behind ``t_initial``, as in the reference
* step:        ``base * decay_rate ** (t // decay_t)``, ``t`` shifted by ``warmup_t`` only under ``warmup_prefix``.  timm's default for
               this class's ``warmup_prefix`` has differed between releases and the reference does not pass it: it is a keyword here
               (``step_warmup_prefix=False`` of ``build_scheduler``).  The two choices agree when ``WARMUP_EPOCHS`` is 0.
* multistep:   ``base * gamma ** bisect.bisect_right(milestones, t)``; the constructor asserts ``warmup_t <= min(milestones)``

Out of scope: noise, ``cycle_mul`` / ``k_decay``, epoch-wise stepping (``t_in_epochs=True``), weight-decay schedules.
"""
from __future__ import annotations

import bisect
import copy
import math

import torch

KIND_COSINE, KIND_LINEAR, KIND_STEP, KIND_MULTISTEP = 0, 1, 2, 3


def build_scheduler(config, optimizer, n_iter_per_epoch, step_warmup_prefix: bool = False):
    """misc/lr_scheduler.py:16-62: the schedule ``config.TRAIN.LR_SCHEDULER.NAME`` names, counted in updates; ``None`` for a name that is
    none of cosine, linear, step, multistep (as the reference)."""
    train, sched, n = config.TRAIN, config.TRAIN.LR_SCHEDULER, n_iter_per_epoch
    updates = {key: int(epochs * n) for key, epochs in (('all', train.EPOCHS), ('warmup', train.WARMUP_EPOCHS), ('decay', sched.DECAY_EPOCHS))}
    warm = dict(warmup_lr_init=train.WARMUP_LR, warmup_t=updates['warmup'], t_in_epochs=False)
    if sched.NAME == 'cosine':
        t_initial = updates['all'] - updates['warmup'] if sched.WARMUP_PREFIX else updates['all']
        return CosineLRScheduler(optimizer, t_initial=t_initial, lr_min=train.MIN_LR, cycle_limit=1, warmup_prefix=sched.WARMUP_PREFIX, **warm)
    if sched.NAME == 'linear':
        return LinearLRScheduler(optimizer, t_initial=updates['all'], lr_min_rate=0.01, **warm)
    if sched.NAME == 'step':
        return StepLRScheduler(optimizer, decay_t=updates['decay'], decay_rate=sched.DECAY_RATE, warmup_prefix=step_warmup_prefix, **warm)
    if sched.NAME == 'multistep':
        return MultiStepLRScheduler(optimizer, milestones=[epoch * n for epoch in sched.MULTISTEPS], gamma=sched.GAMMA, **warm)
    return None


class _DeviceBinding:
    """What a device-stepped scheduler keeps on the GPU, allocated ONCE (a captured update graph bakes the addresses in; later changes
    are copied INTO the buffers): the rule table, the groups' base rates and scales, the update counter and a mirror of the rates."""

    def __init__(self, device, groups):
        from . import ops_lrsched as L
        self.device, self.groups = device, groups
        self.table = torch.zeros(L.LR_TABLE_WORDS, dtype=torch.float64, device=device)
        self.base = torch.zeros(groups, dtype=torch.float64, device=device)
        self.scale = torch.ones(groups, dtype=torch.float64, device=device)
        self.counter = torch.zeros(1, dtype=torch.int64, device=device)
        self.last_lr = torch.zeros(groups, dtype=torch.float32, device=device)


class Scheduler:
    """timm's ``Scheduler`` for ``param_group_field='lr'``, stepped per update, without noise."""
    kind = None
    on_device = None        # None: engine.TrainStep decides (the HIP optimizers: on the device); False: stepped by the host

    def __init__(self, optimizer, warmup_t=0, warmup_lr_init=0., t_in_epochs=False, initialize=True):
        if t_in_epochs:
            raise NotImplementedError(f'{type(self).__name__}: epoch-wise stepping (t_in_epochs=True) is not supported')
        self.optimizer = optimizer
        self.param_group_field = 'lr'
        self._initial_param_group_field = 'initial_lr'
        if initialize:
            for group in optimizer.param_groups:
                group.setdefault('initial_lr', group['lr'])
        self.base_values = [group['initial_lr'] for group in optimizer.param_groups]
        self.metric = None
        self.t_in_epochs = t_in_epochs
        self.noise_range_t = None
        self.noise_pct, self.noise_type, self.noise_std, self.noise_seed = 0.67, 'normal', 1.0, 42
        self.update_groups(self.base_values)
        self.warmup_t = warmup_t
        self.warmup_lr_init = warmup_lr_init
        if self.warmup_t:
            self.warmup_steps = [(base - warmup_lr_init) / self.warmup_t for base in self.base_values]
            self.update_groups(self.warmup_lr_init)
        else:
            self.warmup_steps = [1] * len(self.base_values)
        self._device = None

    # -- timm's surface ------------------------------------------------------------------------
    _NOT_STATE = ('optimizer', '_device', 'on_device')       # the binding to this process, not the schedule

    def state_dict(self):
        return {k: v for k, v in self.__dict__.items() if k not in self._NOT_STATE}

    def load_state_dict(self, state_dict):
        """``self.__dict__.update(state_dict)``.  Attached, the loaded rule is copied INTO the buffers a captured graph reads; one that
        the device table cannot state raises ``ValueError`` and leaves this scheduler as it was (``detach()`` first to load it)."""
        loaded = {k: v for k, v in state_dict.items() if k not in self._NOT_STATE}
        if self._device is not None:
            probe = copy.copy(self)
            probe.__dict__.update(loaded)
            probe._table_words()         # raises before anything of self changed
        self.__dict__.update(loaded)
        if self._device is not None:
            self._upload()

    def _get_lr(self, t):
        """The groups' rates at update t, before lr_scale: the warm-up ramp, behind it the class's own rule."""
        if t < self.warmup_t:
            return [self.warmup_lr_init + t * step for step in self.warmup_steps]
        return [self._rule(base, t) for base in self.base_values]

    def _rule(self, base, t):
        """The rate of a group whose base rate is ``base`` at update t >= warmup_t."""
        raise NotImplementedError

    def get_update_values(self, num_updates: int):
        return self._get_lr(num_updates)

    def get_epoch_values(self, epoch: int):
        return None

    def step(self, epoch: int, metric=None):
        """Per-epoch call of the reference's loop: a no-op, the schedule counts updates."""
        self.metric = metric

    def step_update(self, num_updates: int, metric=None):
        """``param_groups[g]['lr'] = _get_lr(num_updates)[g]`` (times ``lr_scale``).  Attached to a HIP optimizer this only keeps the host
        mirror (the log line, ``optimizer.state_dict()``): ``step_device`` already put the value into the device array, and the
        optimizer is told so that it does not upload it."""
        self.metric = metric
        self.update_groups(self.get_update_values(num_updates))
        if self._device is not None:
            self.optimizer.mark_lr_on_device()

    def update_groups(self, values):
        if not isinstance(values, (list, tuple)):
            values = [values] * len(self.optimizer.param_groups)
        for group, value in zip(self.optimizer.param_groups, values):
            group['lr'] = value * group['lr_scale'] if 'lr_scale' in group else value

    # -- the device-stepped form ---------------------------------------------------------------
    def _table(self):
        """The table words of this rule ({name of ops_lrsched.LR_*: value}); raises ValueError where the device form cannot state it."""
        raise NotImplementedError

    def device_capable(self) -> bool:
        """Whether csrc/lr_schedule.h states this schedule as it stands (up to 32 ascending milestones, positive periods, warm-up
        steps that are the base values' own)."""
        try:
            self._table_words()
            return True
        except ValueError:
            return False

    def _table_words(self):
        from . import ops_lrsched as L
        name = type(self).__name__
        warmup_t = self.warmup_t or 0
        if warmup_t != int(warmup_t) or warmup_t < 0:
            raise ValueError(f'{name}: warmup_t {warmup_t} is not a number of updates')
        want = [(base - self.warmup_lr_init) / warmup_t for base in self.base_values] if warmup_t else None
        if want is not None and list(self.warmup_steps) != want:
            raise ValueError(f'{name}: warmup_steps are not (base_values - warmup_lr_init) / warmup_t: the device form derives them')
        if self._device is not None and len(self.base_values) != self._device.groups:
            raise ValueError(f'{name}: {len(self.base_values)} base values for {self._device.groups} parameter groups')
        words = [0.0] * L.LR_TABLE_WORDS
        words[L.LR_KIND], words[L.LR_WARMUP_T], words[L.LR_WARMUP_LR_INIT] = float(self.kind), float(warmup_t), float(self.warmup_lr_init)
        for index, value in self._table().items():
            words[index] = float(value)
        return words

    def attached(self) -> bool:
        return self._device is not None

    def attach(self, optimizer, start_update: int = 0):
        """Step this schedule on the device from now on: ``optimizer`` (a bound ``optim.FlatAdamW`` / ``FlatSGD``, the one this scheduler
        was built on) receives the rates in its device hyper-parameter array; the counter starts at ``start_update``.  Call it again
        after the optimizer was re-bound, after ``base_values`` or an ``lr_scale`` changed, or to move the counter.

        With ``start_update`` > 0 (a resumed run, a second ``TrainStep``) and groups that hold exactly what ``step_update(start_update
        - 1)`` left in them, the first rate is derived again ON THE DEVICE by one launch at ``start_update - 1``: in the cos and pow
        branches the host's value can lie one fp32 ulp from the kernel's, and an uninterrupted run would have used the kernel's.
        Groups that hold anything else (a caller's ``set_lr``, an optimizer state from elsewhere) keep their rate for that update."""
        if optimizer is not self.optimizer:
            raise ValueError(f'{type(self).__name__}.attach: not the optimizer this scheduler was built on')
        hyper = getattr(optimizer, '_hyper', None)
        if hyper is None:
            raise RuntimeError(f'{type(self).__name__}.attach: the optimizer has no device hyper-parameter array yet (bind_flat first; '
                               f'engine.TrainStep does)')
        groups = len(optimizer.param_groups)
        if self._device is None or self._device.device != hyper.device or self._device.groups != groups:
            self._device = _DeviceBinding(hyper.device, groups)
        try:
            self._upload()
        except ValueError:
            self._device = None
            raise
        start_update = int(start_update)
        held = [group['lr'] for group in optimizer.param_groups]
        resumed = start_update > 0 and held == [v * g['lr_scale'] if 'lr_scale' in g else v
                                                for v, g in zip(self._get_lr(start_update - 1), optimizer.param_groups)]
        self._device.counter.copy_(torch.tensor([start_update - 1 if resumed else start_update], dtype=torch.int64))
        if resumed:
            optimizer.sync_hyperparameters()      # the groups' other words, and the host's rates as seen: nothing more to upload
            self.step_device()                    # the kernel's own rate of update start_update - 1; the counter arrives at start_update

    def detach(self):
        """Back to host stepping."""
        self._device = None

    def _upload(self):
        d = self._device
        words = self._table_words()
        d.table.copy_(torch.tensor(words, dtype=torch.float64))
        d.base.copy_(torch.tensor([float(v) for v in self.base_values], dtype=torch.float64))
        d.scale.copy_(torch.tensor([float(g['lr_scale']) if 'lr_scale' in g else 1.0 for g in self.optimizer.param_groups],
                                   dtype=torch.float64))

    def step_device(self):
        """Queue one schedule step on the current stream (``vited_lr_schedule_step``): the rates of ``_get_lr(counter)`` go into the
        optimizer's device array, the counter advances.  No host synchronisation; capturable into a hipGraph."""
        from . import ops_lrsched as L
        d = self._device
        if d is None:
            raise RuntimeError(f'{type(self).__name__}.step_device: attach(optimizer, start_update) first')
        first, stride = self.optimizer.hyper_lr_words()
        L.lr_schedule_step(d.table, d.base, d.scale, d.counter, self.optimizer._hyper, first, stride, d.last_lr)

    @property
    def device_update(self) -> int:
        """The device counter: the index the next ``step_device`` uses (one host read)."""
        return int(self._device.counter.item())

    @property
    def device_rates(self):
        """The rates the last ``step_device`` wrote, per group (one host read)."""
        return self._device.last_lr.tolist()


class CosineLRScheduler(Scheduler):
    kind = KIND_COSINE

    def __init__(self, optimizer, t_initial, lr_min=0., cycle_mul=1., cycle_decay=1., cycle_limit=1, warmup_t=0, warmup_lr_init=0,
                 warmup_prefix=False, t_in_epochs=False, k_decay=1.0, initialize=True):
        assert t_initial > 0
        assert lr_min >= 0
        if cycle_mul != 1 or k_decay != 1:
            raise NotImplementedError('CosineLRScheduler: cycle_mul != 1 and k_decay != 1 are not supported')
        self.t_initial, self.lr_min = t_initial, lr_min
        self.cycle_mul, self.cycle_decay, self.cycle_limit = cycle_mul, cycle_decay, cycle_limit
        self.warmup_prefix, self.k_decay = warmup_prefix, k_decay
        super().__init__(optimizer, warmup_t, warmup_lr_init, t_in_epochs, initialize)

    def _get_lr(self, t):
        if self.cycle_mul != 1 or self.k_decay != 1:
            raise NotImplementedError('CosineLRScheduler: cycle_mul != 1 and k_decay != 1 are not supported')
        return super()._get_lr(t)

    def _rule(self, base, t):
        if self.warmup_prefix:
            t -= self.warmup_t
        i = t // self.t_initial
        t_curr = t - self.t_initial * i
        if i < self.cycle_limit:
            return self.lr_min + 0.5 * (base * self.cycle_decay ** i - self.lr_min) * (1 + math.cos(math.pi * t_curr / self.t_initial))
        return self.lr_min

    def _table(self):
        from . import ops_lrsched as L
        if self.cycle_mul != 1 or self.k_decay != 1 or self.cycle_decay != 1:
            raise ValueError('CosineLRScheduler: the device form has no cycle_mul, cycle_decay or k_decay')
        if self.t_initial != int(self.t_initial) or self.t_initial <= 0 or self.cycle_limit != int(self.cycle_limit):
            raise ValueError(f'CosineLRScheduler: t_initial {self.t_initial} / cycle_limit {self.cycle_limit} are not whole update counts')
        return {L.LR_T_INITIAL: self.t_initial, L.LR_LR_MIN: self.lr_min, L.LR_CYCLE_LIMIT: self.cycle_limit,
                L.LR_WARMUP_PREFIX: 1.0 if self.warmup_prefix else 0.0}


class LinearLRScheduler(Scheduler):
    kind = KIND_LINEAR

    def __init__(self, optimizer, t_initial, lr_min_rate, warmup_t=0, warmup_lr_init=0., t_in_epochs=False, initialize=True):
        self.t_initial, self.lr_min_rate = t_initial, lr_min_rate
        super().__init__(optimizer, warmup_t, warmup_lr_init, t_in_epochs, initialize)

    def _rule(self, base, t):
        t -= self.warmup_t
        total = self.t_initial - self.warmup_t
        return base - (base - base * self.lr_min_rate) * (t / total)

    def _table(self):
        from . import ops_lrsched as L
        if self.t_initial != int(self.t_initial) or self.t_initial - (self.warmup_t or 0) == 0:
            raise ValueError(f'LinearLRScheduler: t_initial {self.t_initial} with warmup_t {self.warmup_t} leaves no whole, non-zero span')
        return {L.LR_T_INITIAL: self.t_initial, L.LR_LR_MIN_RATE: self.lr_min_rate}


class StepLRScheduler(Scheduler):
    kind = KIND_STEP

    def __init__(self, optimizer, decay_t, decay_rate=1., warmup_t=0, warmup_lr_init=0, warmup_prefix=False, t_in_epochs=False,
                 initialize=True):
        self.decay_t, self.decay_rate, self.warmup_prefix = decay_t, decay_rate, warmup_prefix
        super().__init__(optimizer, warmup_t, warmup_lr_init, t_in_epochs, initialize)

    def _rule(self, base, t):
        if self.warmup_prefix:
            t -= self.warmup_t
        return base * self.decay_rate ** (t // self.decay_t)

    def _table(self):
        from . import ops_lrsched as L
        if self.decay_t != int(self.decay_t) or self.decay_t <= 0:
            raise ValueError(f'StepLRScheduler: decay_t {self.decay_t} is not a positive number of updates')
        return {L.LR_DECAY_T: self.decay_t, L.LR_DECAY_RATE: self.decay_rate, L.LR_WARMUP_PREFIX: 1.0 if self.warmup_prefix else 0.0}


class MultiStepLRScheduler(Scheduler):
    kind = KIND_MULTISTEP

    def __init__(self, optimizer, milestones, gamma=0.1, warmup_t=0, warmup_lr_init=0, t_in_epochs=False, initialize=True):
        self.milestones, self.gamma = milestones, gamma
        super().__init__(optimizer, warmup_t, warmup_lr_init, t_in_epochs, initialize)
        assert self.warmup_t <= min(self.milestones)

    def _rule(self, base, t):
        return base * self.gamma ** bisect.bisect_right(self.milestones, t)

    def _table(self):
        from . import ops_lrsched as L
        stones = [float(m) for m in self.milestones]
        if len(stones) > L.LR_MAX_MILESTONES:
            raise ValueError(f'MultiStepLRScheduler: {len(stones)} milestones, the device table holds {L.LR_MAX_MILESTONES}')
        if stones != sorted(stones):
            raise ValueError('MultiStepLRScheduler: the device form bisects ascending milestones')
        words = {L.LR_GAMMA: self.gamma, L.LR_MILESTONES: len(stones)}
        words.update({L.LR_FIRST_MILESTONE + i: m for i, m in enumerate(stones)})
        return words
