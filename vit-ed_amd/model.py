"""``VisionTransformerCustom`` on MI355X: the module contract of the reference
(models/vision_transformer.py:275-420) with every FLOP executed by the HIP kernels in ``csrc/``.

Drop-in surface kept:
  * ctor keyword names that ``models/build.py:19-32`` forwards;
  * ``forward(x)``, ``forward(x, forward_first_part=True)``, ``forward(feats, x2)`` and the
    ``forward_first_part / prepare_x2-less forward_second_part / forward_head``-level methods;
  * parameter names, shapes and ranks == the reference ``state_dict`` (checkpoints load unchanged;
    ``misc/optimizer.py:36-46`` puts ``ndim == 1`` / ``*.bias`` in the no-decay group; ``.head`` is
    re-initialised by ``misc/utils.py:110-119``);
  * raw fp32 logits out.
  * ``drop_path_rate``: stochastic depth on every residual branch in training mode, applied inside the residual epilogues of
    the kernels (``draw_drop_path`` / ``forward(..., drop_path=...)`` / ``last_drop_path``).
  * ``qk_norm``: ``q_norm`` / ``k_norm`` = LayerNorm(head_dim, eps=1e-6) on every head's queries and keys of every self- and
    cross-attention, with the reference's ``state_dict`` keys (``*.attn.q_norm.weight`` ...); a HIP kernel of its own between the
    projection and the attention kernels.  Off by default: no such module, key or launch exists then.

  * ``patch_drop_rate``: timm PatchDropout as the reference constructs it (prob, num_prefix_tokens=1, ordered=False) - in training mode
    a random subset of the patch tokens of each image is embedded and runs through the blocks; the others are never read
    (``draw_patch_keep`` / ``forward(..., patch_keep=...)`` / ``last_patch_keep``).  Off by default.

  * ``global_pool`` / ``fc_norm``: timm's head options.  ``global_pool='avg'`` feeds the head the mean of the patch tokens instead of the cls
    token, ``fc_norm`` (None: on exactly under 'avg', timm's rule) moves the head's LayerNorm behind the pooling - the model then has
    ``fc_norm.weight`` / ``fc_norm.bias`` and no ``norm.*``, as the reference's ``state_dict`` does.  Under 'avg' every row of the last
    decoder block reaches the loss, so that block runs on all rows, and the pooling and its backward are HIP kernels of their own
    (csrc/pool_head.hip).  Off by default: same modules, keys and launches as before.

  * ``pos_drop_rate``: timm's ``pos_drop = nn.Dropout(pos_drop_rate)`` at the end of ``_pos_embed`` and of the reference's
    ``_pos_embed_no_cls`` - in training mode every element of both token streams is zeroed with that probability and the others are
    scaled by 1 / (1 - p), directly behind the position embedding.  The mask comes from a counter-based generator inside a HIP kernel
    (csrc/token_dropout.hip) and is regenerated from a per-call seed in the backward: no mask is ever stored
    (``draw_pos_drop`` / ``forward(..., pos_drop=...)`` / ``last_pos_drop``).  No parameter, no key.  Off by default.

Precision follows the caller exactly like the reference follows ``torch.cuda.amp.autocast``
(misc/engine.py:208): inside an autocast region the bf16 MFMA kernels run, outside it the fp32
kernels run; ``model.compute_dtype = torch.bfloat16 | torch.float32`` pins it.

There is no PyTorch fallback: calling the model with CPU tensors or without the built
``libvited_hip.so`` raises.
"""
from __future__ import annotations

from collections import namedtuple

import torch
import torch.nn as nn

from . import functions as F_
from . import ops
from .functions import (DEC_BLOCK_KEYS, DEC_BLOCK_QK_KEYS, DEC_SHARED_FC_KEYS, DEC_SHARED_KEYS, ENC_BLOCK_KEYS, ENC_BLOCK_QK_KEYS,
                        ENC_SHARED_KEYS, Runtime)

LN_EPS = F_.LN_EPS

# Stochastic-depth scales of one forward: enc fp32 [depth, 2, B] for the (attn, mlp) branches of every encoder block, dec fp32
# [c_depth, 3, B] for the (self, cross, mlp) branches of every decoder block; each value 0 (the sample skips the branch) or
# 1 / keep.  Either field may be None for a call that runs only the other half.
DropPathScales = namedtuple('DropPathScales', 'enc dec')

# Patch-dropout keep indices of one forward (timm PatchDropout): int32 / int64 tables, per sample the token
# indices that argsort(randn)[:, :K] kept, counted behind the prefix slot, in keep order, distinct within a row.
#   x1 [B1, K1]: the image-1 path has no cls token, so the prefix slot falls on patch 0, which is always kept: the encoder runs on
#                patch 0 followed by the patches 1 + x1[b, :] - 1 + K1 tokens.
#   x2 [B2, K2]: the prefix is the cls token: the decoder runs on cls followed by the patches x2[b, :] - 1 + K2 tokens; one row per
#                pair of the call.
# Either field may be None for a call that does not run that half.
PatchKeep = namedtuple('PatchKeep', 'x1 x2')

# Position-dropout seeds of one forward (timm's pos_drop): each field an int64 tensor of ONE element on the
# model's device, from which the kernel regenerates the elementwise mask of that stream in the forward and in the backward
# (x1: the image-1 stream [B1, n1, D], x2: the image-2 stream [B2, 1 + n1, D], one sample per pair of the call).  Either field may
# be None for a call that does not run that half.
PosDropSeeds = namedtuple('PosDropSeeds', 'x1 x2')


def patch_keep_count(tokens: int, rate: float) -> int:
    """How many of ``tokens`` tokens behind the prefix timm's PatchDropout keeps: max(1, int(L * (1. - p))), in Python float
    arithmetic as timm writes it."""
    return max(1, int(tokens * (1. - rate)))


class _Holder(nn.Module):
    """Parameter container (its forward is never used: the Functions read the parameters)."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('sub-modules of the HIP ViT-ED are parameter holders; call the model itself')


class _Linear(_Holder):
    def __init__(self, in_f, out_f, bias=True):
        super().__init__()
        ref = nn.Linear(in_f, out_f, bias=bias)  # PyTorch default init (decoder side keeps it)
        self.in_features, self.out_features = in_f, out_f
        self.weight = ref.weight
        self.bias = ref.bias

    def extra_repr(self):
        return f'in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}'


class _Norm(_Holder):
    def __init__(self, d):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))
        self.bias = nn.Parameter(torch.zeros(d))
        self.eps = LN_EPS

    def extra_repr(self):
        return f'({self.weight.numel()},), eps={self.eps}'


class _SelfAttn(_Holder):
    def __init__(self, d, heads, qkv_bias, qk_norm=False):
        super().__init__()
        self.num_heads, self.head_dim, self.scale = heads, d // heads, (d // heads) ** -0.5
        self.qkv = _Linear(d, 3 * d, qkv_bias)
        self._add_qk_norm(qk_norm)
        self.proj = _Linear(d, d)
        self.keep_attn = False

    def _add_qk_norm(self, qk_norm):
        """q_norm / k_norm holders (vision_transformer.py:35-36, 153-154): weight 1, bias 0; absent without the option, where the
        reference has parameter-free Identity modules."""
        if qk_norm:
            self.q_norm = _Norm(self.head_dim)
            self.k_norm = _Norm(self.head_dim)

    _store, _key = None, None     # set by VisionTransformerCustom: the runtime's attention store and this module's key

    def _lookup(self, what):
        ent = (self._store() or {}).get(self._key) if self._store is not None else None
        if ent is None or what not in ent:
            raise RuntimeError('no attention map recorded: build the model with MODEL.PJS.KEEP_ATTN True (keep_attn=True) and '
                               'run a forward' + (' and a backward' if what in ('grad', 'cam') else '') + ' first'
                               + (' (get_attn_cam: set model.keep_cam = True instead)' if what == 'cam' else ''))
        return ent[what]

    def get_attn(self):
        """softmax(q k^T / sqrt(hd)) [B, h, Nq, Nk] of the last forward (vision_transformer.py:46-47,166-167)."""
        return self._lookup('attn')

    def get_attn_gradients(self):
        """d loss / d attn of the last backward (vision_transformer.py:49-50,169-170)."""
        return self._lookup('grad')

    def get_attn_cam(self):
        """mean_h max(attn o grad, 0) [B, Nq, Nk] of the last backward under ``model.keep_cam``: avg_heads(get_attn(),
        get_attn_gradients()) of scripts/visualise_attentions.py for every sample, from one fused kernel (ops.attention_cam)."""
        return self._lookup('cam')


class _CrossAttn(_SelfAttn):
    def __init__(self, d, heads, qkv_bias, qk_norm=False):
        _Holder.__init__(self)
        self.num_heads, self.head_dim, self.scale = heads, d // heads, (d // heads) ** -0.5
        self.q = _Linear(d, d, qkv_bias)
        self.kv = _Linear(d, 2 * d, qkv_bias)
        self._add_qk_norm(qk_norm)
        self.proj = _Linear(d, d)
        self.keep_attn = False


class _Mlp(_Holder):
    def __init__(self, d, hidden):
        super().__init__()
        self.fc1 = _Linear(d, hidden)
        self.fc2 = _Linear(hidden, d)


class Block(_Holder):
    """Encoder block parameters (vision_transformer.py:83-127)."""

    def __init__(self, d, heads, hidden, qkv_bias, qk_norm=False):
        super().__init__()
        self.norm1 = _Norm(d)
        self.attn = _SelfAttn(d, heads, qkv_bias, qk_norm)
        self.norm2 = _Norm(d)
        self.mlp = _Mlp(d, hidden)


class CrossBlock(_Holder):
    """Decoder block parameters (vision_transformer.py:213-272)."""

    def __init__(self, d, heads, hidden, qkv_bias, qk_norm=False):
        super().__init__()
        self.norm1 = _Norm(d)
        self.attn = _SelfAttn(d, heads, qkv_bias, qk_norm)
        self.norm_cross = _Norm(d)
        self.norm_context = _Norm(d)
        self.cross_attn = _CrossAttn(d, heads, qkv_bias, qk_norm)
        self.norm2 = _Norm(d)
        self.mlp = _Mlp(d, hidden)


class _PatchEmbed(_Holder):
    def __init__(self, img_size, patch, in_chans, d):
        super().__init__()
        self.img_size, self.patch_size = (img_size, img_size), (patch, patch)
        self.grid_size = (img_size // patch, img_size // patch)
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.proj = nn.Conv2d(in_chans, d, kernel_size=patch, stride=patch, bias=True)  # holder only


def _get(module, dotted):
    for part in dotted.split('.'):
        module = getattr(module, part)
    return module


class VisionTransformerCustom(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12, c_depth=12,
                 num_heads=12, mlp_ratio=4., qkv_bias=True, keep_attn=False, arch_version='v1', compute_dtype=None,
                 drop_path_rate=0., qk_norm=False, patch_drop_rate=0., global_pool='token', fc_norm=None, pos_drop_rate=0.,
                 **unsupported):
        super().__init__()
        if global_pool not in ('token', 'avg'):
            # timm also takes '' (no pooling: forward_head returns per-token logits), which nothing here computes
            raise NotImplementedError(f'global_pool={global_pool!r} is not on the HIP hot path: the head pools the cls token '
                                      "(global_pool='token') or averages the patch tokens (global_pool='avg')")
        drop_path_rate = float(drop_path_rate or 0.)
        if not 0. <= drop_path_rate < 1.:
            raise ValueError(f'drop_path_rate={drop_path_rate}: stochastic depth takes a rate in [0, 1)')
        patch_drop_rate = float(patch_drop_rate or 0.)
        if not 0. <= patch_drop_rate < 1.:
            raise ValueError(f'patch_drop_rate={patch_drop_rate}: patch dropout takes a rate in [0, 1)')
        pos_drop_rate = float(pos_drop_rate or 0.)
        if not 0. <= pos_drop_rate < 1.:
            raise ValueError(f'pos_drop_rate={pos_drop_rate}: position dropout takes a rate in [0, 1)')
        live = {k: v for k, v in unsupported.items() if v not in (None, False, 0, 0., '', 'token')}
        if live:
            raise NotImplementedError(f'options outside the shipped pjs configs are not on the HIP hot path: {sorted(live)}')
        if embed_dim % num_heads:
            raise AssertionError('dim should be divisible by num_heads')
        if img_size % patch_size:
            raise AssertionError('image size must be a multiple of the patch size')
        # limits of the HIP kernels (they would return VITED_ERR_UNSUPPORTED at the first launch): say so here
        if embed_dim % 4 or embed_dim > 1024:
            raise NotImplementedError(f'EMBED_DIM={embed_dim}: the LayerNorm kernels cover multiples of 4 up to 1024 '
                                      '(csrc/layernorm.hip, LN_MAX_VPL)')
        if embed_dim // num_heads not in (32, 64):
            raise NotImplementedError(f'head_dim={embed_dim // num_heads}: the attention kernels cover head_dim 32 and 64 '
                                      '(12 x 32 at configs/puzzle, 6 x 64 at configs/hisfrag)')
        self.img_size, self.patch_size, self.in_chans = img_size, patch_size, in_chans
        self.num_classes, self.embed_dim = num_classes, embed_dim
        self.num_features = embed_dim
        self.depth, self.c_depth, self.num_heads = depth, c_depth, num_heads
        self.keep_attn = bool(keep_attn)    # visualisation slow path: attention maps are ALSO materialised (PyTorch ops)
        self.keep_cam = False               # record head-averaged relevancy maps in the backward (fused kernel; engine.pair_relevancy):
                                            # such a backward leaves every parameter gradient untouched
        self.arch_version = arch_version.lower()
        self.qk_norm = bool(qk_norm)        # q_norm / k_norm = LayerNorm(head_dim) in every attention
        self.global_pool = global_pool      # what the head reads: the cls row ('token') or the mean of the rows behind it ('avg')
        self.use_fc_norm = (global_pool == 'avg') if fc_norm is None else bool(fc_norm)     # timm's rule
        self.compute_dtype = compute_dtype
        # stochastic depth (timm DropPath, scale_by_keep): the reference's two decay rules, fp32 linspace as it computes them
        # (vision_transformer.py:351 for the decoder, timm's VisionTransformer for the encoder); DropPath has no parameters
        self.drop_path_rate = drop_path_rate
        self._drop_probs = ([torch.linspace(0, drop_path_rate, depth)[i].item() for i in range(depth)],
                            [torch.linspace(0, drop_path_rate, c_depth)[i].item() for i in range(c_depth)])
        self.drop_path_generator = None     # torch.Generator of the draws in training mode (None: the device's default generator)
        self.last_drop_path = None          # DropPathScales of the latest forward (None: it ran without stochastic depth)
        self._keep_cache = {}
        # patch dropout (timm PatchDropout(prob, num_prefix_tokens=1, ordered=False)): no parameters either
        self.patch_drop_rate = patch_drop_rate
        self.patch_drop_generator = None    # torch.Generator of the keys in training mode (None: the device's default generator)
        self.last_patch_keep = None         # PatchKeep of the latest forward (None: it ran on every patch)
        # position dropout (timm's pos_drop = nn.Dropout(pos_drop_rate)): no parameters either
        self.pos_drop_rate = pos_drop_rate
        self.pos_drop_generator = None      # torch.Generator of the seeds in training mode (None: the device's default generator)
        self.last_pos_drop = None           # PosDropSeeds of the latest forward (None: it ran without position dropout)
        # uint8 inputs are normalised inside the patch-embedding kernel: ToTensor + Normalize(0.5, 0.5) of data/transforms.py:14-18
        self.input_mean, self.input_std = (0.5,) * in_chans, (0.5,) * in_chans
        hidden = int(embed_dim * mlp_ratio)
        self.patch_embed = _PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        n1 = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, n1 + 1, embed_dim))
        self.blocks = nn.Sequential(*[Block(embed_dim, num_heads, hidden, qkv_bias, self.qk_norm) for _ in range(depth)])
        if self.use_fc_norm:
            self.fc_norm = _Norm(embed_dim)     # behind the pooling; the reference's norm is then a parameter-free Identity
        else:
            self.norm = _Norm(embed_dim)
        self.head = _Linear(embed_dim, num_classes)
        self._init_like_timm()  # runs before the decoder exists, exactly as in the reference ctor (:344-347)
        self.cross_blocks = nn.ModuleList([CrossBlock(embed_dim, num_heads, hidden, qkv_bias, self.qk_norm) for _ in range(c_depth)])
        self._runtimes = {}
        import weakref
        me = weakref.ref(self)
        self._attn_store = {}
        store = lambda: (me()._attn_store if me() is not None else None)
        for i, blk in enumerate(self.blocks):
            blk.attn._store, blk.attn._key, blk.attn.keep_attn = store, ('blocks', i, 'attn'), self.keep_attn
        for i, blk in enumerate(self.cross_blocks):
            blk.attn._store, blk.attn._key, blk.attn.keep_attn = store, ('cross_blocks', i, 'attn'), self.keep_attn
            blk.cross_attn._store, blk.cross_attn._key, blk.cross_attn.keep_attn = store, ('cross_blocks', i, 'cross_attn'), self.keep_attn
        print(f'Using {arch_version} Arch!')

    def _init_like_timm(self):
        nn.init.trunc_normal_(self.pos_embed, std=.02, a=-2., b=2.)
        nn.init.normal_(self.cls_token, std=1e-6)
        for m in self.modules():
            if isinstance(m, _Linear):
                nn.init.trunc_normal_(m.weight, std=.02, a=-2., b=2.)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    # -- launch context ----------------------------------------------------------------------
    def _act_dtype(self):
        if self.compute_dtype is not None:
            return self.compute_dtype
        return torch.bfloat16 if torch.is_autocast_enabled() else torch.float32

    def runtime(self, act_dtype=None) -> Runtime:
        dt = act_dtype or self._act_dtype()
        rt = self._runtimes.get(dt)
        if rt is None:
            rt = Runtime(img_size=self.img_size, patch_size=self.patch_size, in_chans=self.in_chans,
                         num_classes=self.num_classes, embed_dim=self.embed_dim, depth=self.depth, c_depth=self.c_depth,
                         num_heads=self.num_heads, act_dtype=dt, qk_norm=self.qk_norm, global_pool=self.global_pool,
                         fc_norm=self.use_fc_norm)
            self._runtimes[dt] = rt
        # the model's settings are re-synchronised onto the Runtime on every call
        rt.direct_grads = bool(getattr(self, 'direct_param_grads', False))
        rt.input_mean, rt.input_std = self.input_mean, self.input_std
        rt.keep_attn, rt.attn_store = self.keep_attn, self._attn_store
        rt.keep_cam = bool(self.keep_cam)
        if rt.keep_cam and self.global_pool == 'avg':
            raise NotImplementedError("keep_cam / engine.pair_relevancy read the cls row's attention maps, which a model with global_pool='avg' "
                                      'does not classify from')
        if rt.keep_cam:
            rt.direct_grads = False         # nothing of that backward may reach a p.grad or the flat gradient buffer behind it
        return rt

    def _encoder_params(self):
        ps = [_get(self, k) for k in ENC_SHARED_KEYS]
        for blk in self.blocks:
            ps += [_get(blk, k) for k in (ENC_BLOCK_QK_KEYS if self.qk_norm else ENC_BLOCK_KEYS)]
        return ps

    def _decoder_params(self):
        ps = [_get(self, k) for k in (DEC_SHARED_FC_KEYS if self.use_fc_norm else DEC_SHARED_KEYS)]
        for blk in self.cross_blocks:
            ps += [_get(blk, k) for k in (DEC_BLOCK_QK_KEYS if self.qk_norm else DEC_BLOCK_KEYS)]
        return ps

    def _check_images(self, img):
        if img.dim() != 4 or img.shape[1] != self.in_chans or img.shape[2] != self.img_size or img.shape[3] != self.img_size:
            raise AssertionError(f'input {tuple(img.shape)} does not match the model '
                                 f'([B, {self.in_chans}, {self.img_size}, {self.img_size}])')
        if not img.is_cuda:
            raise RuntimeError('the HIP ViT-ED runs on MI355X only: got a CPU tensor (no CPU fallback exists)')

    # -- stochastic depth ---------------------------------------------------------------------
    @property
    def drop_path_probs(self):
        """(drop probability of every encoder block, of every decoder block): both branches of encoder block i drop with
        linspace(0, rate, depth)[i], the three branches of decoder block i with linspace(0, rate, c_depth)[i]."""
        return list(self._drop_probs[0]), list(self._drop_probs[1])

    def _keep(self, which, device):
        """(keep probability, fp32(1) / fp32(keep)) of every block of the encoder (0) / decoder (1) as fp32 [blocks, 1, 1].  Built
        on the host and uploaded once per device; ``_apply`` does that when the model moves, so a capture finds them in place."""
        key = (which, str(device))
        ent = self._keep_cache.get(key)
        if ent is None:
            if device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f'the keep probabilities are not on {device} yet and a graph capture cannot upload them: draw once '
                                   'eagerly on that device before capturing')
            keep = torch.tensor([1.0 - p for p in self._drop_probs[which]], dtype=torch.float32).view(-1, 1, 1)
            ent = self._keep_cache[key] = (keep.to(device), (torch.ones((), dtype=torch.float32) / keep).to(device))
        return ent

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._keep_cache.clear()
        device = self.pos_embed.device
        if self.drop_path_rate > 0. and device.type == 'cuda':
            self._keep(0, device), self._keep(1, device)
        return out

    def draw_drop_path(self, batch_enc, batch_dec, generator=None, device=None):
        """Draw the scales of one forward: DropPathScales(enc fp32 [depth, 2, batch_enc], dec fp32 [c_depth, 3, batch_dec]), every
        branch and sample independently 1 / keep with probability keep, else 0 (timm drop_path, scale_by_keep=True).  A batch of
        None leaves that field None.  One Bernoulli launch and one multiply per half, whatever the depth; plain torch, so it
        also runs on the CPU."""
        device = torch.device(device) if device is not None else self.pos_embed.device
        if generator is not None and device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('drop-path draws inside a graph capture use the device\'s default generator (torch registers it with '
                               'the graph, so every replay draws anew); a custom generator would freeze one mask into the graph')
        out = []
        for which, (batch, branches) in enumerate(((batch_enc, 2), (batch_dec, 3))):
            if batch is None or not self._drop_probs[which]:
                out.append(None)
                continue
            keep, inv_keep = self._keep(which, device)
            kept = torch.bernoulli(keep.expand(-1, branches, int(batch)), generator=generator)
            out.append(kept * inv_keep)
        return DropPathScales(*out)

    def _resolve_drop_path(self, drop_path, batch_enc, batch_dec, device):
        """What a forward passes on to the Functions: (enc, dec, (live enc, live dec)) or None.  Explicit scales hold in any mode and
        make every branch live; otherwise training mode with a live rate draws, and only the branches with p > 0 are live."""
        if drop_path is not None:
            enc, dec = drop_path
            live = ([[True, True]] * self.depth, [[True, True, True]] * self.c_depth)
            used = DropPathScales(enc if batch_enc is not None else None, dec if batch_dec is not None else None)
        elif self.training and self.drop_path_rate > 0. and not self.keep_cam:      # (a relevancy-map backward never drops)
            used = self.draw_drop_path(batch_enc, batch_dec, generator=self.drop_path_generator, device=device)
            live = ([[p > 0.] * 2 for p in self._drop_probs[0]], [[p > 0.] * 3 for p in self._drop_probs[1]])
        else:
            self.last_drop_path = None
            return None
        for name, t, b in (('enc', used.enc, batch_enc), ('dec', used.dec, batch_dec)):
            if b is not None and t is None and (self.depth if name == 'enc' else self.c_depth):
                raise ValueError(f'drop_path.{name} is missing for a call that runs that half of the model')
        # a two-stage step is two calls: each records its half and leaves the other call's half in place
        prev = self.last_drop_path or DropPathScales(None, None)
        self.last_drop_path = DropPathScales(used.enc if batch_enc is not None else prev.enc, used.dec if batch_dec is not None else prev.dec)
        return used.enc, used.dec, live

    # -- patch dropout ------------------------------------------------------------------------
    @property
    def patch_keep_counts(self):
        """(K1, K2): the columns of PatchKeep.x1 / .x2 at the model's rate - the image-1 path keeps K1 of its n1 - 1 patches behind
        patch 0, the image-2 path K2 of its n1 patches behind the cls token (the streams then hold 1 + K1 and 1 + K2 tokens)."""
        n1 = self.patch_embed.num_patches
        if n1 < 2:
            raise ValueError('patch dropout needs at least 2 patches per image: on the image-1 path patch 0 takes the prefix slot')
        return patch_keep_count(n1 - 1, self.patch_drop_rate), patch_keep_count(n1, self.patch_drop_rate)

    def draw_patch_keep(self, batch_x1, batch_x2, generator=None, device=None):
        """Draw the keep indices of one forward as timm does: PatchKeep(x1 [batch_x1, K1], x2 [batch_x2, K2]) with
        row = argsort(randn(L))[:K], independently per sample and per half; a batch of None leaves that field None.  On the GPU
        the keys are torch's randn and the K smallest of every row come from one ranking kernel (ops.keep_from_keys; int32, no host
        read: capturable); on the CPU plain torch.argsort(stable=True) (int64)."""
        device = torch.device(device) if device is not None else self.pos_embed.device
        if generator is not None and device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('patch-dropout draws inside a graph capture use the device\'s default generator (torch registers it with '
                               'the graph, so every replay draws anew); a custom generator would freeze one set of indices into the graph')
        n1 = self.patch_embed.num_patches
        out = []
        for batch, tokens, k in zip((batch_x1, batch_x2), (n1 - 1, n1), self.patch_keep_counts):
            if batch is None:
                out.append(None)
                continue
            keys = torch.randn(int(batch), tokens, generator=generator, device=device if generator is None else generator.device).to(device)
            out.append(ops.keep_from_keys(keys, k) if device.type == 'cuda' else torch.argsort(keys, dim=-1, stable=True)[:, :k])
        return PatchKeep(*out)

    def _resolve_patch_keep(self, patch_keep, batch_x1, batch_x2, device):
        """What a forward passes on to the Functions: (x1 table | None, x2 table | None) or None.  Explicit tables hold in any mode;
        otherwise training mode with a live rate draws - never under keep_attn / keep_cam, whose maps are over all patches."""
        if patch_keep is not None:
            used = PatchKeep(patch_keep[0] if batch_x1 is not None else None, patch_keep[1] if batch_x2 is not None else None)
        elif self.training and self.patch_drop_rate > 0. and not (self.keep_attn or self.keep_cam):
            used = self.draw_patch_keep(batch_x1, batch_x2, generator=self.patch_drop_generator, device=device)
        else:
            self.last_patch_keep = None
            return None
        n1 = self.patch_embed.num_patches
        for name, t, b, tokens in (('x1', used.x1, batch_x1, n1 - 1), ('x2', used.x2, batch_x2, n1)):
            if b is None:
                continue
            if t is None:
                raise ValueError(f'patch_keep.{name} is missing for a call that runs that half of the model')
            if (not torch.is_tensor(t) or t.dtype not in (torch.int32, torch.int64) or t.dim() != 2 or t.shape[0] != b
                    or not 1 <= t.shape[1] <= tokens or t.device != device):
                got = f'{t.dtype} {tuple(t.shape)} on {t.device}' if torch.is_tensor(t) else type(t).__name__
                raise ValueError(f'patch_keep.{name}: expected int32 / int64 [{b}, 1..{tokens}] on {device}, got {got}')
        # a two-stage step is two calls: each records its half and leaves the other call's half in place
        prev = self.last_patch_keep or PatchKeep(None, None)
        self.last_patch_keep = PatchKeep(used.x1 if batch_x1 is not None else prev.x1, used.x2 if batch_x2 is not None else prev.x2)
        return used.x1, used.x2

    # -- position dropout --------------------------------------------------------------------
    def draw_pos_drop(self, run_x1, run_x2, generator=None, device=None):
        """Draw the seeds of one forward: PosDropSeeds(x1, x2), each one int64 over the whole int64 range on ``device`` (the model's), or
        None for a half the call does not run (``run_x1`` / ``run_x2`` false or None).  One torch.randint per half: no host read, so it
        can be captured."""
        device = torch.device(device) if device is not None else self.pos_embed.device
        if generator is not None and device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('position-dropout draws inside a graph capture use the device\'s default generator (torch registers it with '
                               'the graph, so every replay draws anew); a custom generator would freeze one seed into the graph')
        lo, hi = -2 ** 63, 2 ** 63 - 1
        out = []
        for run in (run_x1, run_x2):
            if not run:
                out.append(None)
                continue
            out.append(torch.randint(lo, hi, (1,), dtype=torch.int64, generator=generator,
                                     device=device if generator is None else generator.device).to(device))
        return PosDropSeeds(*out)

    def _resolve_pos_drop(self, pos_drop, run_x1, run_x2, device):
        """What a forward passes on to the Functions: (x1 seed | None, x2 seed | None, rate) or None.  Explicit seeds hold in any mode;
        otherwise training mode with a live rate draws - never under keep_cam (a relevancy backward never drops).  A model whose rate
        is 0 never drops.  The tensors are handed over as they are and never written afterwards."""
        if self.pos_drop_rate > 0. and pos_drop is not None:
            used = PosDropSeeds(pos_drop[0] if run_x1 else None, pos_drop[1] if run_x2 else None)
        elif self.pos_drop_rate > 0. and self.training and not self.keep_cam:
            used = self.draw_pos_drop(run_x1, run_x2, generator=self.pos_drop_generator, device=device)
        else:
            self.last_pos_drop = None
            return None
        for name, t, run in (('x1', used.x1, run_x1), ('x2', used.x2, run_x2)):
            if not run:
                continue
            if t is None:
                raise ValueError(f'pos_drop.{name} is missing for a call that runs that half of the model')
            if not torch.is_tensor(t) or t.dtype != torch.int64 or t.numel() != 1 or t.device != device:
                got = f'{t.dtype} {tuple(t.shape)} on {t.device}' if torch.is_tensor(t) else type(t).__name__
                raise ValueError(f'pos_drop.{name}: expected one int64 on {device}, got {got}')
        # a two-stage step is two calls: each records its half and leaves the other call's half in place
        prev = self.last_pos_drop or PosDropSeeds(None, None)
        self.last_pos_drop = PosDropSeeds(used.x1 if run_x1 else prev.x1, used.x2 if run_x2 else prev.x2)
        return used.x1, used.x2, self.pos_drop_rate

    def _run_fn(self, fn, drop, keep, *args):
        """``args``: the Function's remaining arguments, the position-dropout seeds (``_resolve_pos_drop``) first."""
        return fn.apply(self.runtime(), drop, keep, *args)

    # -- the reference's forward surface -----------------------------------------------------
    def forward_first_part(self, x1, drop_path=None, patch_keep=None, pos_drop=None):
        """[B, N1, D] features; under patch dropout [B, 1 + K1, D] in keep order (patch 0 first), as the reference returns them."""
        self._check_images(x1)
        return self._encode(x1, self._resolve_drop_path(drop_path, x1.shape[0], None, x1.device),
                            self._resolve_patch_keep(patch_keep, x1.shape[0], None, x1.device),
                            self._resolve_pos_drop(pos_drop, True, False, x1.device))

    def _encode(self, x1, drop, keep=None, pdrop=None):
        """The encoder with what ``_resolve_drop_path``, ``_resolve_patch_keep`` and ``_resolve_pos_drop`` returned."""
        return self._run_fn(F_.EncoderFn, drop, keep, pdrop, x1, *self._encoder_params())

    supports_x2_index = True   # engine.pairwise_similarity gathers image-2 rows inside the patch-embed kernel

    def _check_x2(self, x2, x2_index, indexed_features=False):
        """The checked index and the number of pairs of a decoder call."""
        self._check_images(x2)
        if x2_index is None:
            return None, x2.shape[0]
        if not indexed_features and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError('x2_index (gather-in-kernel) without x1_index is an inference path: call it under torch.no_grad(), '
                                      'or train on the pair-indexed form model(feats, x2, x2_index=j, x1_index=i)')
        x2_index = x2_index.to(device=x2.device, dtype=torch.int64).contiguous()
        return x2_index, x2_index.numel()

    supports_x1_index = True   # the pair-indexed two-stage step: engine.hisfrag_prepare_indexed

    def _check_x1(self, x1_feats, x1_index, pairs):
        """The image-1 index of a decoder call as ``ops.PairSegments`` on the features' device (None stays None)."""
        if x1_index is None:
            return None
        if self.keep_attn or self.keep_cam:
            raise NotImplementedError('x1_index is a training / scoring path: the attention-map paths (keep_attn / keep_cam) take '
                                      'gathered features, model(feats[i], x2[j])')
        if x1_feats.dim() != 3:
            raise ValueError(f'x1_index goes with per-image features [images, N1, D], got {tuple(x1_feats.shape)}')
        if isinstance(x1_index, ops.PairSegments):
            seg = x1_index.to(x1_feats.device)
            if seg.items != x1_feats.shape[0]:
                raise ValueError(f'x1_index groups {seg.items} items, the features hold {x1_feats.shape[0]}')
        else:
            seg = ops.pair_segments(x1_index.to(device=x1_feats.device), x1_feats.shape[0])
        if seg.index.numel() != pairs:
            raise ValueError(f'x1_index names {seg.index.numel()} pairs, the image-2 side {pairs}')
        return seg

    def forward_second_part_head(self, x1_feats, x2, x2_index=None, drop_path=None, x1_index=None, patch_keep=None, pos_drop=None):
        """``x1_index`` (int64 [P] or ``ops.PairSegments``): ``x1_feats`` holds one item per IMAGE and pair p reads
        x1_feats[x1_index[p]] - == self(x1_feats[x1_index], x2[x2_index]) (hisfrag.py:153-159) without the two gathers and with
        norm_context + the kv projections once per image; under autograd and under no_grad.  Returns [P, C] logits."""
        x2_index, pairs = self._check_x2(x2, x2_index, indexed_features=x1_index is not None)
        x1_index = self._check_x1(x1_feats, x1_index, pairs)
        return self._decode_head(x1_feats, x2, x2_index, self._resolve_drop_path(drop_path, None, pairs, x2.device), x1_index,
                                 self._resolve_patch_keep(patch_keep, None, pairs, x2.device),
                                 self._resolve_pos_drop(pos_drop, False, True, x2.device))

    def _decode_head(self, x1_feats, x2, x2_index, drop, x1_index=None, keep=None, pdrop=None):
        """The decoder and head with what ``_resolve_drop_path``, ``_resolve_patch_keep`` and ``_resolve_pos_drop`` returned."""
        return self._run_fn(F_.DecoderFn, drop, keep, pdrop, x1_feats, x2, x2_index, x1_index, *self._decoder_params())

    # -- pair-cached inference (engine.pairwise_similarity) ---------------------------------
    supports_pair_cache = True

    @torch.no_grad()
    def cache_image2_tokens(self, images, turn=0):
        """Everything of the decoder that depends on image 2 alone, once per image: prepare_x2 (vision_transformer.py:390-395),
        the first CrossBlock's self-attention branch and its cross-attention queries.  Returns (tokens [n, N2, D] fp32, q0 | None).
        ``turn`` (an int 0..3, or an int tensor [n] with one per image): the cache of the images turned by that many clockwise quarter
        turns, ``torch.rot90(images, -turn, (2, 3))``, their patches gathered from the upright images (learned type-2 puzzles);
        ``turn=0`` makes the launches of the upright cache and no other."""
        self._check_images(images)
        upright = type(turn) is int and turn == 0
        return F_.image2_tokens(self.runtime(), images, self._decoder_params(), turn=None if upright else turn)

    @torch.no_grad()
    def cache_context_kv(self, feats):
        """Cross-attention keys / values of every decoder block for a block of image-1 features (:177-179), once per block."""
        return F_.context_kv(self.runtime(), feats, self._decoder_params())

    @torch.no_grad()
    def forward_pairs_cached(self, tokens2, j_idx, kvs, i_idx, q0=None):
        """== self(feats[i_idx], images[j_idx]) (hisfrag.py:226-229) from the caches."""
        dev = tokens2.device
        j_idx = j_idx.to(device=dev, dtype=torch.int64).contiguous()
        i_idx = i_idx.to(device=dev, dtype=torch.int64).contiguous()
        return F_.decoder_cached(self.runtime(), tokens2, j_idx, kvs, i_idx, self._decoder_params(), q0)

    def forward(self, x, x2=None, forward_first_part=False, x2_index=None, drop_path=None, x1_index=None, patch_keep=None, pos_drop=None):
        """``drop_path``: explicit DropPathScales for this call (any mode; tests, reproducing a step).  None: training mode with a
        live ``drop_path_rate`` draws them for the batch of the call - the images of ``forward_first_part``, the pairs of
        ``(feats, x2)``, the B pairs of a one-shot call for both halves - and ``eval()`` or rate 0 runs without.  The scales used
        are kept in ``last_drop_path``.
        ``patch_keep``: explicit PatchKeep indices for this call (any mode).  None: training mode with a live ``patch_drop_rate``
        draws them - one set per image of ``forward_first_part``, one per pair of ``(feats, x2)``, both for a one-shot call - and
        ``eval()``, rate 0, ``keep_attn`` and ``keep_cam`` run on every patch.  The indices used are kept in ``last_patch_keep``.
        ``pos_drop``: explicit PosDropSeeds for this call (any mode, on a model with a live ``pos_drop_rate``).  None: training mode
        draws one seed per stream of the call; ``eval()``, rate 0 and ``keep_cam`` never drop.  The seeds used are kept in
        ``last_pos_drop``; the pair caches (``cache_image2_tokens`` ...) never drop."""
        if forward_first_part:
            return self.forward_first_part(x, drop_path, patch_keep, pos_drop)
        if x2 is not None:
            return self.forward_second_part_head(x, x2, x2_index, drop_path, x1_index, patch_keep, pos_drop)
        if x1_index is not None:
            raise ValueError('x1_index belongs to the two-stage form model(feats, x2, x1_index=...)')
        if x.dim() != 5 or x.shape[1] != 2:
            raise AssertionError(f'expected stacked pairs [B, 2, C, S, S], got {tuple(x.shape)}')
        drop = self._resolve_drop_path(drop_path, x.shape[0], x.shape[0], x.device)
        keep = self._resolve_patch_keep(patch_keep, x.shape[0], x.shape[0], x.device)
        x1, x2 = x[:, 0], x[:, 1]                                           # strided views: the kernels take a batch stride
        self._check_images(x1)
        self._check_images(x2)
        pdrop = self._resolve_pos_drop(pos_drop, True, True, x.device)
        return self._decode_head(self._encode(x1, drop, keep, pdrop), x2, None, drop, keep=keep, pdrop=pdrop)

    def flops_parts(self):
        """Algorithmic forward FLOPs (2MNK per contraction) of (the encoder on ONE image incl. its
        patch embedding, the decoder + head on ONE pair incl. image 2's patch embedding)."""
        d, n1 = self.embed_dim, self.patch_embed.num_patches
        n2 = n1 + 1
        kp = self.in_chans * self.patch_size ** 2
        enc = self.depth * (24 * n1 * d * d + 4 * n1 * n1 * d)
        dec = self.c_depth * (28 * n2 * d * d + 4 * n1 * d * d + 4 * n2 * n2 * d + 4 * n2 * n1 * d)
        return 2 * n1 * kp * d + enc, 2 * n1 * kp * d + dec + 2 * d * self.num_classes

    def flops(self, batch=1):
        """Algorithmic forward FLOPs per pair (one-shot forward on a stacked pair)."""
        enc, dec = self.flops_parts()
        return batch * (enc + dec)
