"""``FlatAdamW`` and ``FlatSGD``: torch.optim.AdamW's and torch.optim.SGD's updates (misc/optimizer.py:22-27) as ONE HIP
multi-tensor pass over the flat gradient buffer - gradient-norm clip (misc/utils.py:215-217), the update, refresh of the
bf16 weight shadows the MFMA kernels read, and ``zero_grad`` (misc/engine.py:231) - ``vited_adamw_step`` /
``vited_sgd_step`` of include/vited.h.

They are ``torch.optim.Optimizer``s (param_groups / state_dict / lr schedulers work as usual); ``engine.TrainStep``
drives them through ``step_flat``.  There is no CPU path: parameters must live on the GPU.

``skip_nonfinite=True`` leaves out an update whose gradient norm is inf or NaN, as ``GradScaler.step`` does for the reference
(misc/utils.py:206-226): parameters, optimizer state and shadows keep their bits, the gradients are zeroed, the step count
stays and ``skipped_updates`` goes up.  The norm is that of the all-reduced flat buffer, so every data-parallel rank decides
alike.

``ema_decay=d`` keeps an exponential moving average of the parameters (timm's ``ModelEmaV2``, ``--model-ema``) inside the update
launch (``vited_adamw_step_ema`` / ``vited_sgd_step_ema``): one more flat fp32 buffer, ``optimizer.ema``, laid out like the gradient
buffer and equal to the parameters, bit for bit, until the first update.  ``ema_warmup=True`` uses ``min(d, (1 + n) / (10 + n))``
with ``n`` the EMA updates done so far; a skipped update leaves the average and ``n`` alone.  ``with optimizer.swap_ema():``
exchanges parameters and averages in place (``vited_ema_swap``, shadows included) for an evaluation on the averaged weights, and
exchanges them back on exit.  ``ema_state_dict`` / ``load_ema_state_dict`` carry the average under the model's ``state_dict`` keys,
``num_ema_updates`` is the one integer that goes with them; ``state_dict()`` stays torch's.

``FlatLAMB`` is LAMB (You et al. 2020, with timm's ``Lamb`` conventions) on the same base - ``vited_lamb_step``: five launches, because
every tensor's trust ratio needs two norms over the whole tensor before any element moves - with ``FlatAdamW``'s state and
``state_dict``; ``trust_ratios()`` reads the ratios of the latest applied update.

``FlatLion`` is Lion (Chen et al. 2023, with timm's ``Lion`` conventions) on the same base - ``vited_lion_step``: the three launches of
``FlatAdamW`` with one moment, ``p -= lr sign(b1 m + (1 - b1) g)`` after the decoupled decay, every product rounded on its own.

``FlatMuon`` is Muon (Jordan et al. 2024, with ``torch.optim.Muon``'s conventions) on the same base - ``vited_muon_step``: the momentum of
every 2-D tensor of a ``use_muon=True`` group is orthogonalised by Newton-Schulz steps on the matrix cores, all tensors sharing every
launch; every other group takes ``FlatAdamW``'s rule in the same update.
"""
from __future__ import annotations

import contextlib

import torch

from . import _lib, ops
from .functions import shadows_of

HYPER_HEADER, GROUP_WORDS, DESC_WORDS = 8, 8, 10
HYPER_STEP, HYPER_SKIP_FLAG, HYPER_SKIPPED = 0, 1, 2
HYPER_EMA_DECAY, HYPER_EMA_WARMUP, HYPER_EMA_COUNT = 3, 4, 5


def _checked_ema_decay(value, who):
    if value is None:
        return None
    value = float(value)
    if not 0.0 <= value < 1.0:
        raise ValueError(f'{who}: ema_decay must lie in [0, 1), got {value}')
    return value


class _FlatOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share: the binding to a ``FlatGradients``, one flat buffer per state tensor, the descriptor
    table, the device hyper-parameter array, the weight-shadow bookkeeping and the launch.  A subclass names its entry point
    (``_entry``), its state tensors (``_state_names``: descriptor words 2 and 3) and its 8 words per parameter group."""
    manages_weight_shadows = True      # functions._install_optimizer_step_hook: this optimizer publishes its updates itself
    _entry = None
    _state_names = ()
    _state_at_bind = True              # install state[p] views when bound (AdamW) or after the first update (SGD, as torch does)

    def __init__(self, params, defaults, model=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False):
        ema_decay = _checked_ema_decay(ema_decay, type(self).__name__)      # before anything is built
        super().__init__(params, defaults)
        self.flat = None
        self._model = model
        self.skip_nonfinite = bool(skip_nonfinite)
        self._ema_decay, self.ema_warmup = ema_decay, bool(ema_warmup)
        self._ema = None               # the flat fp32 average, laid out like the gradient buffer (allocated at the first bind)
        self._ema_seen = None          # the EMA words sync_hyperparameters uploaded last
        self._ema_loaded = None        # {id(p): tensor} of a load_ema_state_dict before bind_flat
        self._ema_loaded_count = None  # ... and its num_ema_updates
        self._swapped = False          # inside ``with swap_ema():``
        self._bufs = None              # {state name: flat fp32 buffer laid out like the gradient buffer}
        self._desc = self._desc_key = None
        self._hyper = self._hyper_seen = None
        self.hyper_uploads = 0         # copies sync_hyperparameters really made (a device-stepped lr schedule needs one)
        self._norm = self._ws = None

    # -- wiring --------------------------------------------------------------------------------
    def bind_flat(self, flat, model=None):
        """Use ``flat`` (engine.FlatGradients over the same parameters) as the gradient buffer; ``model`` (optional)
        supplies the bf16 weight shadows to refresh (its ``_runtimes``)."""
        name = type(self).__name__
        mine = {id(p) for g in self.param_groups for p in g['params'] if p.requires_grad}
        if {id(p) for p in flat.params} != mine:
            raise ValueError(f'{name}.bind_flat: the flat gradient buffer does not cover exactly the optimizer\'s trainable parameters')
        dev = flat.flat.device
        if dev.type != 'cuda':
            raise RuntimeError(f'{name} runs on the MI355X HIP kernel only (no CPU path); use torch.optim for CPU parameters')
        if self._swapped:
            raise RuntimeError(f'{name}.bind_flat: not inside `with swap_ema():` (parameters and averages are exchanged)')
        rebind = self.flat is flat and self._bufs is not None and all(b.numel() == flat.flat.numel() for b in self._bufs.values())
        # the averages of an earlier binding to another buffer go along, like the counters in the hyper header
        ema_before = None if rebind or self._ema is None else {id(p): self.ema_of(p).clone() for p in self.flat.params}
        self.flat = flat
        if model is not None:
            self._model = model
        if not rebind:
            # first binding to this buffer: the state buffers, the hyper-parameter array and the workspace are allocated ONCE - a
            # captured update graph bakes their addresses in, so a later load_state_dict copies INTO them (below) instead of
            # replacing them
            self._bufs = {n: torch.zeros_like(flat.flat) for n in self._state_names}
            hyper = torch.zeros(HYPER_HEADER + GROUP_WORDS * len(self.param_groups), dtype=torch.float32, device=dev)
            if self._hyper is not None:
                # bound before (a second TrainStep on the same optimizer): the counts of applied and skipped updates go along with
                # the state, on the device
                hyper[:HYPER_HEADER].copy_(self._hyper[:HYPER_HEADER])
            self._hyper = hyper
            self._norm = torch.zeros(1, dtype=torch.float32, device=dev)
            self._ws = self._new_workspace(flat, dev)
            self._desc = self._desc_key = None
            self._ema = None
        self._hyper[HYPER_SKIP_FLAG: HYPER_SKIP_FLAG + 1].fill_(1.0 if self.skip_nonfinite else 0.0)
        self._hyper_seen = self._ema_seen = None
        if self._ema_decay is not None:
            self._bind_ema(ema_before)
        for p, off in zip(flat.params, flat.offsets):
            st = self.state[p] if (self._state_at_bind or p in self.state) else {}
            for key, n in self._state_keys(p):
                old = st.get(key)
                if old is None and not self._state_at_bind:
                    continue                                 # no state yet (or a loaded None): the zero the buffer holds
                new = self._bufs[n][off: off + p.numel()].view_as(p)
                if old is not None and old.data_ptr() != new.data_ptr():
                    new.copy_(old)
                st[key] = new
        self._after_bind()

    def _after_bind(self):
        pass

    def _state_keys(self, p):
        """((key in ``state[p]``, name of the flat buffer it views), ...) of parameter ``p``: the same for every parameter, unless a
        subclass keeps different state on different tensors (``FlatMuon``)."""
        return tuple((n, n) for n in self._state_names)

    def _entry_extras(self):
        """What ``_entry`` takes behind the stream (``FlatMuon``: the tile tables, the steps and the coefficients)."""
        return ()

    def _new_workspace(self, flat, dev):
        """The workspace of ``_entry`` for ``flat``, allocated by ``bind_flat`` before the descriptor table exists."""
        return torch.empty(_lib.load().vited_adamw_workspace_bytes() // 4, dtype=torch.float32, device=dev)

    def _state_view(self, name, p):
        off = self.flat.offsets[next(i for i, q in enumerate(self.flat.params) if q is p)]
        return self._bufs[name][off: off + p.numel()].view_as(p)

    # -- the moving average of the parameters ----------------------------------------------------
    def _bind_ema(self, before=None):
        """The flat average exists from here on: allocated ONCE per binding (a captured update graph bakes its address in) and equal
        to the parameters bit for bit, unless an earlier binding (``before``) or a ``load_ema_state_dict`` says otherwise."""
        fresh = self._ema is None
        if fresh:
            self._ema = torch.zeros_like(self.flat.flat)
        with torch.no_grad():
            for p in self.flat.params:
                src = (self._ema_loaded or {}).get(id(p))
                if src is None and fresh:
                    src = p if before is None or id(p) not in before else before[id(p)]
                if src is not None:
                    self.ema_of(p).copy_(src)
        if self._ema_loaded_count is not None:
            self._hyper[HYPER_EMA_COUNT] = float(self._ema_loaded_count)
        elif fresh and before is None:
            self._hyper[HYPER_EMA_COUNT] = 0.0
        self._ema_loaded = self._ema_loaded_count = None

    @property
    def ema_decay(self):
        """The decay ``d`` of the average (None: no average is kept).  Assigning a number between two steps reaches the device through
        ``sync_hyperparameters``, so a replayed update follows it without a recapture; assigning one to an optimizer that kept no
        average starts one from the present parameters, and None drops it (either changes what a captured update graph bakes in:
        ``shadow_signature`` tells ``engine.TrainStep`` to capture again)."""
        return self._ema_decay

    @ema_decay.setter
    def ema_decay(self, value):
        value = _checked_ema_decay(value, type(self).__name__)
        if (value is None) != (self._ema_decay is None):
            if self._swapped or torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f'{type(self).__name__}: the average cannot be switched on or off inside `with swap_ema():` or during '
                                   f'graph capture')
            self._ema_decay = value
            if value is None:
                self._ema = self._ema_seen = None
            elif self.flat is not None:
                self._bind_ema()
            return
        self._ema_decay = value

    @property
    def ema(self):
        """The flat fp32 average (None before ``bind_flat`` or without ``ema_decay``); inside ``with swap_ema():`` it holds the raw
        parameters."""
        return self._ema

    def ema_of(self, p):
        """The average of parameter ``p``: a view of ``ema`` shaped like ``p``."""
        if self._ema is None:
            raise RuntimeError(f'{type(self).__name__}.ema_of: no average is kept (build the optimizer with ema_decay=... and bind it)')
        off = self.flat.offsets[next(i for i, q in enumerate(self.flat.params) if q is p)]
        return self._ema[off: off + p.numel()].view_as(p)

    @property
    def num_ema_updates(self) -> int:
        """EMA updates done, the ``n`` of the warmup (one host read once bound); a skipped update does not count."""
        if self._ema_loaded_count is not None:
            return int(self._ema_loaded_count)
        return int(self._hyper[HYPER_EMA_COUNT].item()) if self._hyper is not None and self._ema_decay is not None else 0

    @property
    def ema_swapped(self) -> bool:
        """Inside ``with swap_ema():``."""
        return self._swapped

    def _exchange_ema(self):
        desc = self._descriptors()
        ops.ema_swap(desc, self._tiles, self._ema, self.flat.flat)
        _FlatOptimizer._publish_update(self)         # p and the table's shadows were raw-written, exactly as by an update

    @contextlib.contextmanager
    def swap_ema(self):
        """Inside the block the parameters and their bf16 shadows hold the averaged weights, at unchanged addresses - the model, its
        pair caches and any captured forward graph evaluate on them as they are - and ``ema`` holds the raw parameters; on exit
        every bit is back.  One launch each way."""
        name = type(self).__name__
        if self._ema_decay is None:
            raise RuntimeError(f'{name}.swap_ema: no average is kept (build the optimizer with ema_decay=...)')
        if self._swapped:
            raise RuntimeError(f'{name}.swap_ema: already inside `with swap_ema():` (nested use would exchange the weights back)')
        if self._ema is None:
            raise RuntimeError(f'{name}.swap_ema: call bind_flat(FlatGradients) first (engine.TrainStep does)')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f'{name}.swap_ema: not during graph capture (the exchange back on exit would be captured with it)')
        self._exchange_ema()
        self._swapped = True
        try:
            yield self
        finally:
            self._swapped = False
            self._exchange_ema()

    def _trainable_ids(self):
        return {id(p) for g in self.param_groups for p in g['params'] if p.requires_grad}

    @torch.no_grad()
    def ema_state_dict(self, model):
        """{name: tensor} under ``model.state_dict()``'s keys: clones of the averages; a parameter that is not trainable and a buffer
        contribute their own value.  ``num_ema_updates`` is the one integer to save beside it."""
        mine, named = self._trainable_ids(), dict(model.named_parameters())
        out = {}
        for key, value in model.state_dict().items():
            p = named.get(key)
            if p is None or id(p) not in mine:
                out[key] = value.detach().clone()
            elif self._swapped:
                out[key] = p.detach().clone()            # inside the block the parameter holds the average
            elif self._ema is not None:
                out[key] = self.ema_of(p).clone()
            else:                                        # not bound yet: what was loaded, else e == p
                out[key] = (self._ema_loaded or {}).get(id(p), p).detach().clone()
        return out

    @torch.no_grad()
    def load_ema_state_dict(self, state_dict, model, num_ema_updates=None):
        """Load what ``ema_state_dict`` gave, before or after ``bind_flat``: once bound the values are copied INTO the existing flat
        buffer, so a captured update graph stays valid.  ``num_ema_updates`` (None: keep the counter) sets the ``n`` of the warmup."""
        name = type(self).__name__
        if self._ema_decay is None:
            raise RuntimeError(f'{name}.load_ema_state_dict: no average is kept (build the optimizer with ema_decay=...)')
        if self._swapped:
            raise RuntimeError(f'{name}.load_ema_state_dict: not inside `with swap_ema():`')
        mine = self._trainable_ids()
        loaded = {}
        for key, p in model.named_parameters():
            if id(p) not in mine:
                continue
            if key not in state_dict:
                raise KeyError(f'{name}.load_ema_state_dict: {key} is missing')
            value = state_dict[key]
            if value.shape != p.shape:
                raise ValueError(f'{name}.load_ema_state_dict: {key} has shape {tuple(value.shape)}, the parameter {tuple(p.shape)}')
            loaded[id(p)] = value.detach().to(device=p.device, dtype=torch.float32)
        if num_ema_updates is not None and int(num_ema_updates) < 0:
            raise ValueError(f'{name}.load_ema_state_dict: num_ema_updates must not be negative, got {num_ema_updates}')
        if self._ema is None:
            self._ema_loaded = {k: v.clone() for k, v in loaded.items()}
            self._ema_loaded_count = None if num_ema_updates is None else int(num_ema_updates)
            return
        for p in self.flat.params:
            self.ema_of(p).copy_(loaded[id(p)])
        if num_ema_updates is not None:
            self._hyper[HYPER_EMA_COUNT] = float(int(num_ema_updates))

    @property
    def num_updates(self) -> int:
        """Updates applied (one host read once bound); a skipped update does not count."""
        return int(self._hyper[HYPER_STEP].item()) if self._hyper is not None else 0

    @property
    def skipped_updates(self) -> int:
        """Updates left out because the gradient norm was not finite (one host read)."""
        return int(self._hyper[HYPER_SKIPPED].item()) if self._hyper is not None else 0

    def _group_words(self, group):
        raise NotImplementedError

    def sync_hyperparameters(self):
        """Fold ``param_groups`` (what schedulers write) into the device hyper-parameter array when they changed.  The header
        (step count, skip flag, skipped count) is owned by the kernel and ``bind_flat`` and never overwritten here."""
        vals = []
        for g in self.param_groups:
            vals += self._group_words(g)
        if vals != self._hyper_seen:
            # a fresh host tensor per change and an ordinary (host-synchronous) copy of ~16 floats: a reused pinned buffer
            # with a non-blocking copy could be rewritten with the NEXT iteration's rate before this copy executed (the host
            # runs ahead of the device under graph replay)
            self._hyper[HYPER_HEADER:].copy_(torch.tensor(vals, dtype=torch.float32))
            self._hyper_seen = vals
            self.hyper_uploads += 1
        if self._ema_decay is not None:
            words = [self._ema_decay, 1.0 if self.ema_warmup else 0.0]       # hyper[3..4]; hyper[5], the counter, is the kernel's
            if words != self._ema_seen:
                self._hyper[HYPER_EMA_DECAY: HYPER_EMA_WARMUP + 1].copy_(torch.tensor(words, dtype=torch.float32))
                self._ema_seen = words
                self.hyper_uploads += 1

    @staticmethod
    def hyper_lr_words():
        """(first word, stride) of the groups' learning rates in the device hyper-parameter array: where a device-stepped schedule
        (lr_scheduler.Scheduler.step_device) writes."""
        return HYPER_HEADER, GROUP_WORDS

    def mark_lr_on_device(self):
        """The rates now in ``param_groups`` are the ones a schedule step on the device already wrote into the hyper-parameter array
        (lr_scheduler.Scheduler.step_update says so): ``sync_hyperparameters`` does not upload them.  Any other change - a caller's
        ``set_lr``, another word of a group - still differs from what was seen and is uploaded."""
        if self._hyper_seen is not None:
            for gi, g in enumerate(self.param_groups):
                self._hyper_seen[gi * GROUP_WORDS] = float(g['lr'])

    def _descriptors(self):
        shadows = {}
        for cache in shadows_of(self._model):
            for pid, tags in cache.buffers().items():
                shadows.setdefault(pid, {}).update(tags)
        group_of = {id(p): gi for gi, g in enumerate(self.param_groups) for p in g['params']}
        state = [self._bufs[n].data_ptr() for n in self._state_names] + [None] * (2 - len(self._state_names))
        rows_, tile = [], 0
        for p, v, off in zip(self.flat.params, self.flat.views, self.flat.offsets):
            if not p.is_contiguous() or p.dtype != torch.float32:
                raise ValueError(f'{type(self).__name__}: parameters must be contiguous fp32')
            r = p.shape[0] if p.dim() >= 2 else 1
            c = p.numel() // r
            sh = shadows.get(id(p), {})
            n, t = sh.get('n'), sh.get('t')
            rows_.append([p.data_ptr(), v.data_ptr()] + [0 if s is None else s + 4 * off for s in state]
                         + [0 if n is None else n.data_ptr(), 0 if t is None else t.data_ptr(), r, c, tile, group_of[id(p)]])
            tile += ((r + 63) // 64) * ((c + 63) // 64)
        key = tuple(tuple(r[:6]) for r in rows_)
        if key != self._desc_key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f'{type(self).__name__}: the set of weight shadows changed during graph capture (run one eager step first)')
            self._desc = torch.tensor(rows_, dtype=torch.int64).to(self.flat.flat.device)
            self._desc_key, self._tiles = key, tile
        return self._desc

    # -- the update ----------------------------------------------------------------------------
    def step_flat(self, max_norm=None, zero_grad: bool = True):
        """clip(max_norm) + update + shadow refresh (+ zero the gradients).  Returns the pre-clip gradient norm (device scalar)."""
        if self.flat is None:
            raise RuntimeError(f'{type(self).__name__}.step_flat: call bind_flat(FlatGradients) first (engine.TrainStep does)')
        if self._swapped:
            raise RuntimeError(f'{type(self).__name__}.step_flat: not inside `with swap_ema():` (the update would act on the averaged '
                               f'weights and average the raw ones)')
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            self.sync_hyperparameters()
        desc = self._descriptors()
        # with an average the *_ema entry, which takes the flat average behind the workspace; without, the entry as it always was
        entry, ema = (self._entry, ()) if self._ema_decay is None else (self._entry + '_ema', (self._ema.data_ptr(), self._ema.numel()))
        _lib.call(entry, desc.data_ptr(), desc.shape[0], self._tiles, self.flat.flat.data_ptr(), self.flat.flat.numel(),
                  self._hyper.data_ptr(), float(max_norm) if max_norm else 0.0, int(zero_grad), self._norm.data_ptr(), self._ws.data_ptr(),
                  self._ws.numel() * 4, *ema, torch.cuda.current_stream().cuda_stream, *self._entry_extras())
        if not capturing:
            self._publish_update()
        return self._norm[0]

    def shadow_signature(self):
        """What a captured update graph baked in besides this optimizer's state buffers: the set of weight-shadow buffers and, where
        an average is kept, its buffer (which also tells the entry that was captured)."""
        shadows = tuple(sorted(item for cache in shadows_of(self._model) for item in cache.signature()))
        return shadows if self._ema is None else shadows + (('ema', self._ema.data_ptr()),)

    def _publish_update(self):
        """The kernel raw-wrote the fp32 parameters (and the shadows listed in its descriptor table).  Bump every
        parameter's version counter - anything that caches by version (a Runtime whose shadows the table did NOT cover, e.g.
        an optimizer built without ``model``) then recasts - and mark the shadows the kernel did refresh as current."""
        params = self.flat.params
        torch.autograd.graph.increment_version(params)
        refreshed = {ptr for row in (self._desc_key or ()) for ptr in row[4:6] if ptr}
        for cache in shadows_of(self._model):
            cache.mark_current(params, only_buffers=refreshed)

    @torch.no_grad()
    def step(self, closure=None):
        """``torch.optim.Optimizer.step`` for callers that own the loop (the reference's NativeScaler path): gradients are
        taken from ``p.grad`` (folded into a flat buffer on first use), no clipping, no zeroing."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.flat is None:
            from .engine import FlatGradients
            grads = {id(p): p.grad for g in self.param_groups for p in g['params']}
            flat = FlatGradients([p for g in self.param_groups for p in g['params']])
            for p, v in zip(flat.params, flat.views):
                if grads[id(p)] is not None:
                    v.copy_(grads[id(p)])
            self.bind_flat(flat, self._model)
        else:
            self.flat.attach()
        self.step_flat(None, zero_grad=False)
        return loss

    def zero_grad(self, set_to_none: bool = True):
        if self.flat is not None:
            self.flat.zero()        # keeps p.grad attached to the flat buffer
        else:
            super().zero_grad(set_to_none=set_to_none)


class _FlatAdamMoments(_FlatOptimizer):
    """What ``FlatAdamW`` and ``FlatLAMB`` share: the two moments, one step count, and torch.optim.AdamW's ``state_dict`` layout."""
    _state_names = ('exp_avg', 'exp_avg_sq')

    def __init__(self, params, defaults, model=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False):
        super().__init__(params, defaults, model, skip_nonfinite, ema_decay, ema_warmup)
        self._loaded_step = None       # step count of a state_dict loaded before bind_flat (the reference's resume order)

    exp_avg = property(lambda self: self._bufs['exp_avg'] if self._bufs else None)
    exp_avg_sq = property(lambda self: self._bufs['exp_avg_sq'] if self._bufs else None)

    def _after_bind(self):
        if self._loaded_step is not None:
            # torch.optim.AdamW keeps one step count per parameter; they advance together, so one counter serves (bias correction)
            self._hyper[HYPER_STEP] = float(self._loaded_step)
            self._loaded_step = None

    @property
    def num_updates(self) -> int:
        if self._hyper is not None:
            return int(self._hyper[HYPER_STEP].item())
        return int(self._loaded_step or 0)

    # -- checkpoint compatibility with torch.optim.AdamW (misc/utils.py:130-142 saves optimizer.state_dict()) ----
    def state_dict(self):
        sd = super().state_dict()
        n = self.num_updates                     # the kernel's counter once bound, else the step of a loaded checkpoint
        for st in sd['state'].values():
            st['step'] = torch.tensor(float(n))
        return sd

    def load_state_dict(self, state_dict):
        """Works in either order relative to ``bind_flat`` / ``TrainStep`` (the reference resumes as: build optimizer,
        ``load_checkpoint``, then build the loop - misc/utils.py:57-70): the loaded step count is kept until the flat buffers
        exist.  Once bound the loaded moments are copied INTO the existing flat buffers, so a captured update graph stays valid."""
        flat = self.flat
        super().load_state_dict(state_dict)
        steps = [float(st['step']) for st in self.state.values() if 'step' in st]
        self._loaded_step = max(steps) if steps else None
        if flat is not None:
            self.bind_flat(flat)                 # copies the loaded moments into the flat buffers and applies the step count


class FlatAdamW(_FlatAdamMoments):
    _entry = 'vited_adamw_step'

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, model=None, skip_nonfinite=False,
                 ema_decay=None, ema_warmup=False):
        """``model`` (the HIP ViT-ED whose parameters these are) lets the kernel refresh the model's bf16 weight shadows in the
        same pass; without it the parameters' version counters are bumped after every update instead, so the model recasts its
        shadows on the next forward (correct, one extra launch per weight)."""
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay), model, skip_nonfinite, ema_decay,
                         ema_warmup)

    def _group_words(self, g):
        return [float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']), float(g['weight_decay']), 0., 0., 0.]


LAMB_RATIO_AT = 1028               # the first word of ratio[count] in vited_lamb_step's workspace (include/vited.h)


class FlatLAMB(_FlatAdamMoments):
    """LAMB (You et al. 2020, Algorithm 2) with timm's ``Lamb`` conventions - bias correction, gradient averaging, the weight decay
    inside the update (L2 in ``u``, not AdamW's decoupled decay), the trust ratio only where it applies - in the fused update:
    ``vited_lamb_step`` / ``vited_lamb_step_ema``, the rule is csrc/optim_update.h's.  Per parameter tensor, with ``c`` the step's clip
    coefficient and ``t`` the updates applied::

        g' = g c;  m = m + (g' - m)(1 - b1);  v = b2 v + (1 - b2) g' g'
        u  = (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps) + wd p
        r  = 1 if wd == 0 and not always_adapt else (|p| / |u| if |p| > 0 and |u| > 0 else 1);   trust_clip: r = min(r, 1)
        p  = p - lr r u

    The gradient clip is the step's own (``step_flat(max_norm)``, ``TRAIN.CLIP_GRAD``): there is no second ``max_grad_norm``.  State
    and ``state_dict`` are ``FlatAdamW``'s (``exp_avg``, ``exp_avg_sq``, one step count), so a checkpoint of either loads into the other.
    Everything else - shadows, graph replay, device-stepped rates, skipped updates, the parameter average - is ``_FlatOptimizer``'s."""
    _entry = 'vited_lamb_step'

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, always_adapt=False, trust_clip=False,
                 model=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False):
        if not 0.0 <= lr:
            raise ValueError(f'Invalid learning rate: {lr}')
        if not 0.0 <= eps:
            raise ValueError(f'Invalid epsilon value: {eps}')
        betas = tuple(betas)
        if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f'Invalid beta parameters: {betas}')
        if not 0.0 <= weight_decay:
            raise ValueError(f'Invalid weight_decay value: {weight_decay}')
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, always_adapt=bool(always_adapt),
                        trust_clip=bool(trust_clip))
        super().__init__(params, defaults, model, skip_nonfinite, ema_decay, ema_warmup)

    def _group_words(self, g):
        return [float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']), float(g['weight_decay']),
                1.0 if g['always_adapt'] else 0.0, 1.0 if g['trust_clip'] else 0.0, 0.]

    def _new_workspace(self, flat, dev):
        # the tile count depends on the parameters' shapes alone (``_descriptors`` counts the same way), so the workspace - ratio[count]
        # and two sums per tile behind AdamW's words - can be sized, once per binding, before the table exists
        tiles = 0
        for p in flat.params:
            r = p.shape[0] if p.dim() >= 2 else 1
            tiles += ((r + 63) // 64) * ((p.numel() // r + 63) // 64)
        nbytes = _lib.load().vited_lamb_workspace_bytes(tiles, len(flat.params))
        if nbytes <= 0:
            raise ValueError(f'FlatLAMB: no workspace for {len(flat.params)} parameters in {tiles} tiles')
        return torch.zeros(nbytes // 4, dtype=torch.float32, device=dev)

    def load_state_dict(self, state_dict):
        """As ``FlatAdamW.load_state_dict``; groups saved by ``FlatAdamW`` (or torch.optim.AdamW) carry no ``always_adapt`` /
        ``trust_clip`` and take this optimizer's defaults."""
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            for key in ('always_adapt', 'trust_clip'):
                g.setdefault(key, self.defaults[key])

    def trust_ratios(self):
        """{parameter name, or its index in ``state_dict()`` where the optimizer has no ``model`` that names it: r} of the latest applied
        update of this binding (0.0 before the first): one host read of the ratio table."""
        if self.flat is None:
            raise RuntimeError('FlatLAMB.trust_ratios: call bind_flat(FlatGradients) first (engine.TrainStep does)')
        names = {id(p): n for n, p in self._model.named_parameters()} if hasattr(self._model, 'named_parameters') else {}
        index = {id(p): i for i, p in enumerate(p for g in self.param_groups for p in g['params'])}
        values = self._ws[LAMB_RATIO_AT: LAMB_RATIO_AT + len(self.flat.params)].tolist()
        return {names.get(id(p), index[id(p)]): r for p, r in zip(self.flat.params, values)}


class FlatLion(_FlatOptimizer):
    """Lion (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms") with timm's ``Lion`` conventions in the fused update:
    ``vited_lion_step`` / ``vited_lion_step_ema``, the rule is csrc/optim_update.h's.  Per element, with ``c`` the step's clip
    coefficient::

        g' = g c;  pe = p (1 - lr wd);  s = sign(b1 m + (1 - b1) g')
        p  = pe - lr s;  m = m + (g' - m)(1 - b2)

    One moment (4 B of state per parameter instead of AdamW's 8), no step count in the rule, no bias correction; every product is
    rounded on its own, so the kernel gives the bits of the rule written as separate fp32 operations.  The step has the same size for
    every element, so Lion wants a rate 3-10x smaller and a decay 3-10x larger than AdamW's.  ``state_dict()`` has timm Lion's layout
    (``exp_avg`` per parameter, no ``step``); ``load_state_dict`` also takes a ``FlatAdamW`` / ``FlatLAMB`` / ``torch.optim.AdamW``
    checkpoint, of which ``exp_avg`` is kept.  Everything else - shadows, graph replay, device-stepped rates, skipped updates, the
    parameter average - is ``_FlatOptimizer``'s."""
    _entry = 'vited_lion_step'
    _state_names = ('exp_avg',)

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0, model=None, skip_nonfinite=False, ema_decay=None,
                 ema_warmup=False):
        if not 0.0 <= lr:
            raise ValueError(f'Invalid learning rate: {lr}')
        betas = tuple(betas)
        if len(betas) != 2:
            raise ValueError(f'Invalid beta parameters: {betas}')
        for i, b in enumerate(betas):
            if not 0.0 <= b < 1.0:
                raise ValueError(f'Invalid beta parameter at index {i}: {b}')
        if not 0.0 <= weight_decay:
            raise ValueError(f'Invalid weight_decay value: {weight_decay}')
        # timm Lion's group keys, so that a state_dict moves between the two
        defaults = dict(lr=lr, betas=betas, weight_decay=weight_decay, foreach=None, maximize=False)
        super().__init__(params, defaults, model, skip_nonfinite, ema_decay, ema_warmup)
        for g in self.param_groups:
            self._check_group(g)

    exp_avg = property(lambda self: self._bufs['exp_avg'] if self._bufs else None)

    @staticmethod
    def _check_group(g):
        if g.get('maximize'):
            raise ValueError('FlatLion does not support maximize=True')

    def _group_words(self, g):
        self._check_group(g)
        return [float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), 0., float(g['weight_decay']), 0., 0., 0.]

    def load_state_dict(self, state_dict):
        """Accepts timm ``Lion``'s state and that of ``FlatAdamW`` / ``FlatLAMB`` / ``torch.optim.AdamW`` (``exp_avg`` is taken,
        ``exp_avg_sq`` and ``step`` are dropped), before or after ``bind_flat``; a parameter without a loaded ``exp_avg`` starts from
        zero.  Once bound the loaded moments are copied INTO the existing flat buffer, so a captured update graph stays valid."""
        flat = self.flat
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            for key in ('foreach', 'maximize'):
                g.setdefault(key, self.defaults[key])
            self._check_group(g)
        for st in self.state.values():
            for key in [k for k in st if k != 'exp_avg']:
                del st[key]
        if flat is not None:
            for st in self.state.values():       # a loaded moment may be a view of the flat buffer itself (our own state_dict)
                if st.get('exp_avg') is not None:
                    st['exp_avg'] = st['exp_avg'].clone()
            self._bufs['exp_avg'].zero_()
            self.bind_flat(flat)


MUON_GRANULE, MUON_MAX_SHORT_SIDE, MUON_TILE_WORDS = 64, 1024, 8


def muon_layout(shapes, is_muon, group_of=None):
    """The workspace layout and the host side of ``vited_muon_step``'s tables for parameters of ``shapes`` (in flat-buffer order), of
    which ``is_muon[i]`` says whether tensor ``i`` belongs to a Muon group and ``group_of[i]`` (default: 0 everywhere) names its group.  A Muon tensor ``[rows, cols]`` has ``m = min``, ``n = max``
    of the two, padded up to the GEMM granule of 64 as ``mp``, ``np``; its region of the bf16 scratch holds ``X0 [mp, np]``, ``X1``,
    ``XT0 [np, mp]``, ``XT1``, ``A [mp, mp]``, ``B [mp, mp]``.  Returns a dict:

    ``meta``        ``[rows, cols, ndim, is_muon, group]`` per tensor (the HOST table the entry checks)
    ``tensor_tab``  ``[base, mp, np, tall]`` per tensor, ``base`` in bf16 elements from the start of the scratch, -1 for an aux tensor
    ``tiles_sq``    ``[tensor, tile row, tile column, base, mp, np, tall, 0]`` per 64 x 64 tile of every Muon tensor's ``A``
    ``tiles_x``     the same row per 64 x 64 tile of every Muon tensor's ``X``
    ``total_tiles`` the update's 64 x 64 tiles over all tensors; ``float_words``: the fp32 words in front of the scratch;
    ``scratch_elems``: the bf16 elements of the scratch; ``nbytes``: what ``vited_muon_workspace_bytes`` returns."""
    meta, tensor_tab, tiles_sq, tiles_x, total, base = [], [], [], [], 0, 0
    group_of = [0] * len(is_muon) if group_of is None else list(group_of)
    for i, (shape, mu) in enumerate(zip(shapes, is_muon)):
        shape = tuple(int(d) for d in shape)
        rows = shape[0] if len(shape) >= 2 else 1
        numel = 1
        for d in shape:
            numel *= d
        cols = numel // rows
        meta.append([rows, cols, len(shape), 1 if mu else 0, int(group_of[i])])
        total += ((rows + 63) // 64) * ((cols + 63) // 64)
        if not mu:
            tensor_tab.append([-1, 0, 0, 0])
            continue
        if len(shape) != 2:
            raise ValueError(f'Muon takes 2-D tensors only: tensor {i} has the shape {shape}')
        m, n, tall = min(rows, cols), max(rows, cols), int(rows > cols)
        if m > MUON_MAX_SHORT_SIDE:
            raise ValueError(f'Muon: tensor {i} of shape {shape} has a short side above {MUON_MAX_SHORT_SIDE}, the limit of the scratch layout')
        mp, np_ = -(-m // MUON_GRANULE) * MUON_GRANULE, -(-n // MUON_GRANULE) * MUON_GRANULE
        tensor_tab.append([base, mp, np_, tall])
        tiles_sq += [[i, ti, tj, base, mp, np_, tall, 0] for ti in range(mp // 64) for tj in range(mp // 64)]
        tiles_x += [[i, ti, tj, base, mp, np_, tall, 0] for ti in range(mp // 64) for tj in range(np_ // 64)]
        base += 4 * mp * np_ + 2 * mp * mp
    words = -(-(1028 + len(meta) + total) // 64) * 64
    return dict(meta=meta, tensor_tab=tensor_tab, tiles_sq=tiles_sq, tiles_x=tiles_x, total_tiles=total, float_words=words,
                scratch_elems=base, nbytes=4 * words + 2 * base)


class FlatMuon(_FlatAdamMoments):
    """Muon (Jordan et al. 2024) with ``torch.optim.Muon``'s conventions in the fused update - ``vited_muon_step`` /
    ``vited_muon_step_ema``, the rule is csrc/muon_update.h's.  A param group with ``use_muon=True`` is a Muon group and takes 2-D tensors
    only; with ``c`` the step's clip coefficient and ``(a, b, cc) = ns_coefficients``, per tensor ``[rows, cols]``::

        g'  = g c;  buf = buf + (g' - buf)(1 - momentum);  u = g' + (buf - g') momentum if nesterov else buf
        X   = bf16(u / max(|u|_F, eps))                      transposed when rows > cols
        ns_steps times:  A = bf16(X X^T);  B = bf16(b A + cc A A);  X = bf16(a X + B X)
        p   = p (1 - lr wd) - lr adj X                       adj = sqrt(max(1, rows / cols)), or 0.2 sqrt(max(rows, cols)) with
                                                             adjust_lr_fn='match_rms_adamw'

    Every other group is an aux group and takes ``FlatAdamW``'s rule, bit for bit, with ``betas`` and ``adam_eps`` - all 1-D parameters,
    ``cls_token``, ``pos_embed``, the patch projection, the head: Jordan's ``MuonWithAuxAdam`` in one optimizer and one flat buffer.  The
    products of all Muon tensors share ``3 ns_steps`` launches.  ``ns_steps`` and ``ns_coefficients`` are fixed at construction (a
    captured update bakes the launch count in); every group value can change between updates without a recapture.

    ``state_dict()``: a Muon tensor carries ``momentum_buffer`` (``torch.optim.Muon``'s key), an aux tensor ``step``, ``exp_avg``,
    ``exp_avg_sq``.  ``load_state_dict`` also takes a ``FlatAdamW`` / ``FlatLAMB`` / ``FlatLion`` checkpoint over the same groups of
    parameters - on a Muon tensor its ``exp_avg``, the same kind of average of the gradients, becomes ``momentum_buffer`` - and a
    ``torch.optim.Muon`` state.  A checkpoint written under ``build_optimizer('adamw' | 'lamb' | 'lion')``, which has two groups where
    ``build_optimizer('muon')`` has three, is regrouped by the parameters' order in ``model`` (``_regrouped``), so a run may switch to
    Muon on resume.  Both flat state buffers span all parameters: ``exp_avg_sq`` is
    allocated over the Muon tensors too and never touched there (4 B per Muon parameter, 85 MB on config A's).  Everything else - shadows, graph replay, device-stepped rates, skipped updates, the parameter average -
    is ``_FlatOptimizer``'s."""
    _entry = 'vited_muon_step'
    _ADJUST = {None: 0.0, 'original': 0.0, 'match_rms_adamw': 1.0}

    def __init__(self, params, lr=1e-3, momentum=0.95, nesterov=True, weight_decay=0.1, ns_steps=5,
                 ns_coefficients=(3.4445, -4.7750, 2.0315), eps=1e-7, adjust_lr_fn=None, betas=(0.9, 0.999), adam_eps=1e-8, model=None,
                 skip_nonfinite=False, ema_decay=None, ema_warmup=False):
        if not 0.0 <= lr:
            raise ValueError(f'Invalid learning rate: {lr}')
        if not 0.0 <= momentum < 1.0:
            raise ValueError(f'Invalid momentum value: {momentum}')
        if not 0.0 <= weight_decay:
            raise ValueError(f'Invalid weight_decay value: {weight_decay}')
        if not 0.0 <= eps or not 0.0 <= adam_eps:
            raise ValueError(f'Invalid epsilon value: {eps if not 0.0 <= eps else adam_eps}')
        if isinstance(ns_steps, bool) or int(ns_steps) != ns_steps or not 1 <= ns_steps <= 16:
            raise ValueError(f'Invalid ns_steps: {ns_steps} (an integer in [1, 16])')
        ns_coefficients = tuple(float(v) for v in ns_coefficients)
        if len(ns_coefficients) != 3:
            raise ValueError(f'Invalid ns_coefficients: {ns_coefficients} (exactly 3 values)')
        if adjust_lr_fn not in self._ADJUST:
            raise ValueError(f'Invalid adjust_lr_fn: {adjust_lr_fn!r} (None, \'original\' or \'match_rms_adamw\')')
        betas = tuple(betas)
        if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f'Invalid beta parameters: {betas}')
        defaults = dict(lr=lr, momentum=momentum, nesterov=bool(nesterov), weight_decay=weight_decay, eps=eps, adjust_lr_fn=adjust_lr_fn,
                        betas=betas, adam_eps=adam_eps, use_muon=False)
        super().__init__(params, defaults, model, skip_nonfinite, ema_decay, ema_warmup)
        self._ns_steps, self._ns_coefficients = int(ns_steps), ns_coefficients
        self._mu = None                # the device tables and the host tables of the current binding
        self._muon_set = None          # ids of the Muon groups' parameters, gathered once per binding and per load
        names = {id(p): n for n, p in model.named_parameters()} if hasattr(model, 'named_parameters') else {}
        for gi, g in enumerate(self.param_groups):
            self._check_group(g)
            if g['use_muon']:
                for i, p in enumerate(g['params']):
                    if p.ndim != 2:
                        raise ValueError(f'FlatMuon: {names.get(id(p), f"parameter {i} of group {gi}")} has the shape {tuple(p.shape)}; a '
                                         f'Muon group (use_muon=True) takes 2-D tensors only - put it into an aux group')

    ns_steps = property(lambda self: self._ns_steps)
    ns_coefficients = property(lambda self: self._ns_coefficients)

    @classmethod
    def _check_group(cls, g):
        if g['adjust_lr_fn'] not in cls._ADJUST:
            raise ValueError(f'Invalid adjust_lr_fn: {g["adjust_lr_fn"]!r} (None, \'original\' or \'match_rms_adamw\')')
        if not 0.0 <= g['momentum'] < 1.0:
            raise ValueError(f'Invalid momentum value: {g["momentum"]}')

    def _group_words(self, g):
        self._check_group(g)
        if g['use_muon']:
            return [float(g['lr']), float(g['momentum']), 1.0 if g['nesterov'] else 0.0, float(g['eps']), float(g['weight_decay']),
                    self._ADJUST[g['adjust_lr_fn']], 1.0, 0.]
        return [float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['adam_eps']), float(g['weight_decay']), 0., 0., 0.]

    def _muon_ids(self):
        return {id(p) for g in self.param_groups if g['use_muon'] for p in g['params']}

    def _after_bind(self):
        super()._after_bind()
        self._muon_set = None          # the next binding gathers the ids again (add_param_group may have come between)

    def _state_keys(self, p):
        if self._muon_set is None:
            self._muon_set = self._muon_ids()
        if id(p) in self._muon_set:
            return (('momentum_buffer', 'exp_avg'),)
        return (('exp_avg', 'exp_avg'), ('exp_avg_sq', 'exp_avg_sq'))

    def _new_workspace(self, flat, dev):
        # the tables depend on the parameters' shapes and groups alone, so they are built, and uploaded, once per binding, with the
        # workspace they describe
        mine = self._muon_ids()
        group_of = {id(p): gi for gi, g in enumerate(self.param_groups) for p in g['params']}
        lay = muon_layout([p.shape for p in flat.params], [id(p) in mine for p in flat.params], [group_of[id(p)] for p in flat.params])
        meta = torch.tensor(lay['meta'], dtype=torch.int64)
        kinds = torch.tensor([1 if g['use_muon'] else 0 for g in self.param_groups], dtype=torch.int64)     # word 6 of _group_words
        rows, cols, kind = (meta[:, j].contiguous() for j in (0, 1, 3))         # alive across the call that reads them
        nbytes = _lib.load().vited_muon_workspace_bytes(len(lay['meta']), rows.data_ptr(), cols.data_ptr(), kind.data_ptr())
        if nbytes != lay['nbytes']:
            raise RuntimeError(f'FlatMuon: the library sizes the workspace at {nbytes} bytes, the layout at {lay["nbytes"]}')
        table = lambda rows, width: torch.tensor(rows, dtype=torch.int64).reshape(-1, width).to(dev)
        self._mu = dict(meta=meta, kinds=kinds, float_words=lay['float_words'], tensor_tab=table(lay['tensor_tab'], 4), tiles_sq=table(lay['tiles_sq'], MUON_TILE_WORDS),
                        tiles_x=table(lay['tiles_x'], MUON_TILE_WORDS))
        return torch.zeros(nbytes // 4, dtype=torch.float32, device=dev)

    def orthogonalized(self, p):
        """O of Muon tensor ``p`` as the latest applied update of this binding left it in the scratch: a bf16 copy shaped like ``p``
        (one device copy; what the apply pass read)."""
        if self.flat is None:
            raise RuntimeError('FlatMuon.orthogonalized: call bind_flat(FlatGradients) first (engine.TrainStep does)')
        i = next(k for k, q in enumerate(self.flat.params) if q is p)
        base, mp, np_, tall = self._mu['tensor_tab'][i].tolist()
        if base < 0:
            raise ValueError('FlatMuon.orthogonalized: not a tensor of a Muon group')
        rp, cp = (np_, mp) if tall else (mp, np_)
        at = base + ((2 if tall else 0) + (self._ns_steps & 1)) * mp * np_
        scratch = self._ws[self._mu['float_words']:].view(torch.bfloat16)
        return scratch[at: at + rp * cp].view(rp, cp)[: p.shape[0], : p.shape[1]].clone()

    def _entry_extras(self):
        mu = self._mu
        return (mu['tiles_sq'].data_ptr(), mu['tiles_sq'].shape[0], mu['tiles_x'].data_ptr(), mu['tiles_x'].shape[0],
                mu['tensor_tab'].data_ptr(), mu['meta'].data_ptr(), mu['kinds'].data_ptr(), mu['kinds'].numel(), self._ns_steps, *self._ns_coefficients)

    def state_dict(self):
        sd = torch.optim.Optimizer.state_dict(self)
        n = self.num_updates
        for st in sd['state'].values():
            if 'momentum_buffer' not in st:
                st['step'] = torch.tensor(float(n))
        return sd

    def _regrouped(self, state_dict):
        """``state_dict`` of an optimizer that held the same parameters in fewer groups, each of them a union of whole groups of this
        one with its parameters in the model's order (what ``engine.build_optimizer`` builds under every other name: the decayed group
        is the Muon group and the decayed aux group together), rewritten over this optimizer's groups.  Which groups were united is
        found from the group sizes and the shapes of the state tensors; none or several fits are a ``ValueError``."""
        import itertools
        name = type(self).__name__
        if not hasattr(self._model, 'named_parameters'):
            raise ValueError(f'{name}.load_state_dict: the checkpoint has {len(state_dict["param_groups"])} parameter groups, this optimizer '
                             f'{len(self.param_groups)}; regrouping it needs the order of the parameters (build the optimizer with model=...)')
        rank = {id(p): k for k, (_, p) in enumerate(self._model.named_parameters())}
        theirs, state = state_dict['param_groups'], state_dict['state']
        fits = []
        for assign in itertools.product(range(len(theirs)), repeat=len(self.param_groups)):
            index, ok = {}, True
            for j, g in enumerate(theirs):
                members = sorted((p for gi, mg in enumerate(self.param_groups) if assign[gi] == j for p in mg['params']), key=lambda p: rank.get(id(p), -1))
                if len(members) != len(g['params']) or any(id(p) not in rank for p in members):
                    ok = False
                    break
                for p, k in zip(members, g['params']):
                    shapes = [tuple(v.shape) for v in state.get(k, {}).values() if torch.is_tensor(v) and v.dim() > 0]
                    ok = ok and all(s == tuple(p.shape) for s in shapes)
                    index[id(p)] = k
            if ok:
                fits.append((assign, index))
        if len(fits) != 1:
            raise ValueError(f'{name}.load_state_dict: the checkpoint\'s {len(theirs)} groups of {[len(g["params"]) for g in theirs]} parameters '
                             f'can be spread over this optimizer\'s groups of {[len(g["params"]) for g in self.param_groups]} in {len(fits)} ways '
                             f'(exactly one is needed)')
        assign, index = fits[0]
        groups, new_state, at = [], {}, 0
        for gi, mg in enumerate(self.param_groups):
            ids = list(range(at, at + len(mg['params'])))
            at += len(ids)
            groups.append({**{k: v for k, v in theirs[assign[gi]].items() if k != 'params'}, 'params': ids})
            for p, k in zip(mg['params'], ids):
                if index[id(p)] in state:
                    new_state[k] = state[index[id(p)]]
        return {'state': new_state, 'param_groups': groups}

    def load_state_dict(self, state_dict):
        """Accepts this class's state, that of ``FlatAdamW`` / ``FlatLAMB`` / ``FlatLion`` / ``torch.optim.AdamW`` over the same groups of
        parameters (on a Muon tensor ``exp_avg`` becomes ``momentum_buffer``; ``exp_avg_sq`` and ``step`` are dropped there) and that of
        ``torch.optim.Muon``, before or after ``bind_flat``.  Groups of a foreign checkpoint give their rate and decay (and, where they
        have them, the momentum words on a Muon group and ``betas`` / ``eps`` on an aux group); which group is a Muon group is never
        loaded.  A checkpoint with FEWER groups than this optimizer - ``build_optimizer('adamw' | 'lamb' | 'lion')`` writes two, ``'muon'``
        has three - is regrouped first (``_regrouped``), which needs the ``model`` for the order of the parameters.  Once bound the
        loaded state is copied INTO the existing flat buffers, so a captured update graph stays valid."""
        flat = self.flat
        before = [{k: v for k, v in g.items() if k != 'params'} for g in self.param_groups]
        if len(state_dict['param_groups']) < len(self.param_groups):
            state_dict = self._regrouped(state_dict)
        torch.optim.Optimizer.load_state_dict(self, state_dict)
        for g, old in zip(self.param_groups, before):
            loaded = {k: v for k, v in g.items() if k != 'params'}
            if 'use_muon' not in loaded:                 # a foreign checkpoint
                keep = {'lr', 'weight_decay'} | ({'momentum', 'nesterov', 'eps', 'adjust_lr_fn'} if old['use_muon'] and 'momentum' in loaded
                                                  else set())
                take = {k: loaded[k] for k in keep if k in loaded}
                if not old['use_muon'] and 'betas' in loaded:
                    take['betas'] = tuple(loaded['betas'])
                    if 'eps' in loaded:
                        take['adam_eps'] = loaded['eps']
                for k in loaded:
                    del g[k]
                g.update({**old, **take})
            g['use_muon'] = old['use_muon']
            for k, v in old.items():
                g.setdefault(k, v)
            self._check_group(g)
        mine, steps = self._muon_ids(), []
        for p, st in list(self.state.items()):
            if 'step' in st:
                steps.append(float(st['step']))
            if id(p) in mine:
                buf = st.get('momentum_buffer', st.get('exp_avg'))
                self.state[p] = {} if buf is None else {'momentum_buffer': buf.clone()}
            else:
                self.state[p] = {k: st[k].clone() for k in ('exp_avg', 'exp_avg_sq') if st.get(k) is not None}
        self._loaded_step = max(steps) if steps else None
        if flat is not None:
            for b in self._bufs.values():
                b.zero_()
            self.bind_flat(flat)


class FlatSGD(_FlatOptimizer):
    """torch.optim.SGD with momentum / Nesterov momentum (misc/optimizer.py:22-24 builds ``nesterov=True``); dampening is not
    supported.  ``state[p]['momentum_buffer']`` is a view into one flat buffer; like torch's, the state is empty before the first
    update and stays empty for a group whose momentum is 0."""
    _entry = 'vited_sgd_step'
    _state_names = ('momentum_buffer',)
    _state_at_bind = False

    def __init__(self, params, lr=1e-3, momentum=0., dampening=0, weight_decay=0., nesterov=False, model=None, skip_nonfinite=False,
                 ema_decay=None, ema_warmup=False):
        if lr < 0.0:
            raise ValueError(f'Invalid learning rate: {lr}')
        if momentum < 0.0:
            raise ValueError(f'Invalid momentum value: {momentum}')
        if dampening != 0:
            raise ValueError('FlatSGD does not support dampening (torch.optim.SGD does)')
        if nesterov and momentum <= 0:
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        # torch.optim.SGD's group keys, so that a state_dict moves between the two in both directions
        defaults = dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=bool(nesterov), maximize=False,
                        foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults, model, skip_nonfinite, ema_decay, ema_warmup)
        for g in self.param_groups:
            self._check_group(g)
        self._state_installed = False

    @staticmethod
    def _check_group(g):
        if g['dampening'] != 0:
            raise ValueError('FlatSGD does not support dampening (torch.optim.SGD does)')
        if g['nesterov'] and g['momentum'] <= 0:
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        if g.get('maximize'):
            raise ValueError('FlatSGD does not support maximize=True')

    def _group_words(self, g):
        self._check_group(g)
        return [float(g['lr']), float(g['momentum']), 1.0 if g['nesterov'] else 0.0, 0., float(g['weight_decay']), 0., 0., 0.]

    def _install_state(self):
        """After the first update torch.optim.SGD holds a momentum buffer for every parameter of a group with momentum."""
        for g in self.param_groups:
            if g['momentum'] != 0:
                for p in g['params']:
                    if p.requires_grad and self.state[p].get('momentum_buffer') is None:
                        self.state[p]['momentum_buffer'] = self._state_view('momentum_buffer', p)
        self._state_installed = True

    def _after_bind(self):
        self._state_installed = False

    def _publish_update(self):
        super()._publish_update()
        if not self._state_installed:
            self._install_state()

    def state_dict(self):
        if self.flat is not None and not self._state_installed and self.num_updates > 0:
            self._install_state()                # every update so far was a graph replay
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Accepts a ``torch.optim.SGD`` state, before or after ``bind_flat``; a ``None`` or absent momentum buffer loads as zeros.
        Once bound the loaded buffers are copied INTO the existing flat buffer, so a captured update graph stays valid."""
        flat = self.flat
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            self._check_group(g)
        if flat is not None:
            for st in self.state.values():       # a loaded buffer may be a view of the flat buffer itself (our own state_dict)
                if st.get('momentum_buffer') is not None:
                    st['momentum_buffer'] = st['momentum_buffer'].clone()
            self._bufs['momentum_buffer'].zero_()
            self.bind_flat(flat)
