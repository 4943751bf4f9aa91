"""Encoder / decoder autograd Functions of the ViT-ED hot path, composed from the HIP ops.

Two coarse Functions instead of ~230 per-op autograd nodes: the whole encoder
(models/vision_transformer.py:382-388 ``forward_first_part``) and the whole decoder + head
(:390-405 ``prepare_x2`` / ``cross_part`` / ``forward_second_part`` and timm ``forward_head``).
Inside each, forward and backward are explicit sequences of kernel launches with hand-managed
saved activations, which is what lets the residual adds, the low-precision copies of the residual
gradient and the accumulation of d(context) over the c_depth decoder blocks live in kernel
epilogues instead of separate elementwise passes.

Data types: the residual stream, LayerNorm statistics, parameters and parameter gradients are
fp32; activations that feed contractions are ``rt.act_dtype`` (bf16 on the MFMA path, fp32 on the
exact path).
"""
from __future__ import annotations

import contextlib
import os
from collections import namedtuple

import torch

from . import ops
from ._lib import (B_KN, B_NK, EPI_GELU_GRAD, EPI_MUL, EPI_RESIDUAL, EPI_STORE, EPI_STORE_F32)
from .shadows import WeightShadows

LN_EPS = 1e-6  # partial(nn.LayerNorm, eps=1e-6), vision_transformer.py:348


def _bundle(name, table):
    """(namedtuple of the short names, tuple of the state_dict keys) of one ``field=key`` table, the only statement of which field
    is which parameter and of their order: model.py and the checkpoint layout read the keys, the code below reads the fields."""
    fields, keys = zip(*(pair.split('=') for pair in table.split()))
    return namedtuple(name, fields), keys


_ATTN = 'g1=norm1.weight b1=norm1.bias wqkv=attn.qkv.weight bqkv=attn.qkv.bias wproj=attn.proj.weight bproj=attn.proj.bias '
_CROSS = ('gc=norm_cross.weight bc=norm_cross.bias gx=norm_context.weight bx=norm_context.bias wq=cross_attn.q.weight '
          'bq=cross_attn.q.bias wkv=cross_attn.kv.weight bkv=cross_attn.kv.bias wcp=cross_attn.proj.weight bcp=cross_attn.proj.bias ')
_MLP = 'g2=norm2.weight b2=norm2.bias w1=mlp.fc1.weight bb1=mlp.fc1.bias w2=mlp.fc2.weight bb2=mlp.fc2.bias'
_PATCH = 'pw=patch_embed.proj.weight pb=patch_embed.proj.bias pos=pos_embed '
# q/k-norm (qk_norm=True): LayerNorm(head_dim) of the self-attention's and of the cross-attention's queries and keys
_QKN = 'gqn=attn.q_norm.weight bqn=attn.q_norm.bias gkn=attn.k_norm.weight bkn=attn.k_norm.bias '
_CQKN = ('gcqn=cross_attn.q_norm.weight bcqn=cross_attn.q_norm.bias gckn=cross_attn.k_norm.weight '
         'bckn=cross_attn.k_norm.bias ')
EncBlock, ENC_BLOCK_KEYS = _bundle('EncBlock', _ATTN + _MLP)
DecBlock, DEC_BLOCK_KEYS = _bundle('DecBlock', _ATTN + _CROSS + _MLP)
EncBlockQK, ENC_BLOCK_QK_KEYS = _bundle('EncBlockQK', _ATTN + _QKN + _MLP)            # the blocks of a qk_norm=True model
DecBlockQK, DEC_BLOCK_QK_KEYS = _bundle('DecBlockQK', _ATTN + _QKN + _CROSS + _CQKN + _MLP)
EncShared, ENC_SHARED_KEYS = _bundle('EncShared', _PATCH)
DecShared, DEC_SHARED_KEYS = _bundle('DecShared', _PATCH + 'cls=cls_token gN=norm.weight bN=norm.bias wh=head.weight bh=head.bias')
# the decoder's shared bundle of a model whose head norm is fc_norm (behind the pooling) instead of norm: the same fields, other keys
DecSharedFc, DEC_SHARED_FC_KEYS = _bundle('DecSharedFc', _PATCH + 'cls=cls_token gN=fc_norm.weight bN=fc_norm.bias wh=head.weight bh=head.bias')


def split_params(params, shared_type, block_type):
    """Flat ``*params`` of a Function (model._encoder_params / _decoder_params) -> (shared bundle, [block bundle, ...])."""
    ns, nb = len(shared_type._fields), len(block_type._fields)
    if len(params) < ns or (len(params) - ns) % nb:
        raise ValueError(f'{len(params)} parameters are not {ns} shared + a whole number of {nb}-parameter blocks')
    return shared_type._make(params[:ns]), [block_type._make(params[i: i + nb]) for i in range(ns, len(params), nb)]


def flatten_params(shared, blocks):
    """Inverse of split_params: the flat tuple in key order (what a Function's backward returns for ``*params``)."""
    return (*shared, *(g for block in blocks for g in block))


_step_hook_installed = False


def _install_optimizer_step_hook():
    """The bf16 weight shadows are validated by the parameters' version counters.  ``torch.optim.*(fused=True)`` updates the
    parameters WITHOUT bumping them (measured: ``p._version`` is unchanged by a fused AdamW step, while the default / foreach
    implementations bump it), so a model trained by such an optimizer in the reference's own loop would keep running on its
    initial weights.  A global optimizer post-step hook bumps the versions of whatever any optimizer just stepped; optimizers
    that refresh the shadows themselves (optim.FlatAdamW) opt out with ``manages_weight_shadows``."""
    global _step_hook_installed
    if _step_hook_installed:
        return
    from torch.optim.optimizer import register_optimizer_step_post_hook

    def bump(optimizer, args, kwargs):
        if getattr(optimizer, 'manages_weight_shadows', False):
            return
        params = [p for g in optimizer.param_groups for p in g['params'] if torch.is_tensor(p)]
        if params:
            torch.autograd.graph.increment_version(params)

    register_optimizer_step_post_hook(bump)
    _step_hook_installed = True


class Runtime:
    """Per-model launch context: static shape, activation dtype and the low-precision weight shadows."""

    def __init__(self, *, img_size, patch_size, in_chans, num_classes, embed_dim, depth, c_depth, num_heads,
                 act_dtype=torch.bfloat16, qk_norm=False, global_pool='token', fc_norm=False):
        if global_pool not in ('token', 'avg'):
            raise NotImplementedError(f'global_pool={global_pool!r}: the head pools the cls token (\'token\') or averages the patch tokens (\'avg\')')
        # the head (timm forward_head): 'avg' pools the mean of the tokens behind the cls row (ops.token_pool_fwd /
        # _bwd) instead of the cls row; fc_norm: the head's LayerNorm sits behind the pooling (fc_norm.*) instead of in front of it (norm.*)
        self.pool_avg, self.fc_norm = global_pool == 'avg', bool(fc_norm)
        self.dec_shared = DecSharedFc if self.fc_norm else DecShared
        self.qk_norm = bool(qk_norm)   # q_norm / k_norm in every attention (ops.qk_norm_fwd / _bwd)
        self.enc_block, self.dec_block = (EncBlockQK, DecBlockQK) if self.qk_norm else (EncBlock, DecBlock)   # the blocks' bundles
        self.img_size, self.patch_size, self.in_chans = img_size, patch_size, in_chans
        self.num_classes, self.dim, self.depth, self.c_depth, self.heads = num_classes, embed_dim, depth, c_depth, num_heads
        self.n1 = (img_size // patch_size) ** 2
        self.n2 = self.n1 + 1
        self.head_dim = embed_dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.act_dtype = act_dtype
        self.direct_grads = False   # accumulate parameter gradients straight into existing p.grad (engine.FlatGradients)
        self.input_mean, self.input_std = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)   # Normalize() of data/transforms.py:14-18, for uint8 inputs
        self.keep_attn = False      # MODEL.PJS.KEEP_ATTN: also materialise the attention maps (visualisation slow path)
        self.keep_cam = False       # record the head-averaged relevancy map of every attention in the backward (ops.attention_cam): no
                                    # per-head map is formed, and the backward leaves every parameter gradient alone (see _cam_only)
        self.attn_store = {}        # (kind, block index, 'attn' | 'cross_attn') -> {'attn': ..., 'grad': ..., 'cam': [B, Nq, Nk]}
        # last decoder block on the cls rows only (exact; see _dec_self_fwd) - never under 'avg', where every token row reaches the loss
        self.cls_tail = os.environ.get('VITED_CLS_TAIL', '1') != '0' and not self.pool_avg
        self.fused_mlp = os.environ.get('VITED_FUSED_MLP', '1') != '0'   # vited_mlp_fwd on the no-grad paths
        self.fused_ln = os.environ.get('VITED_FUSED_LN', '1') != '0'     # LayerNorm inside the neighbouring Linear's kernel (gemm_row.hip)
        self.batch_dw = os.environ.get('VITED_BATCH_DW', '1') != '0'     # a block's weight gradients in one launch (vited_linear_bwd_weight_batched)
        self.group_dw = os.environ.get('VITED_GROUP_DW', '1') != '0'     # ... and several blocks' together while they fit one round of workgroups
        self.dw_queue = None        # inside a block's backward: [(dy, x, dW target, dbias target | None, accumulate)]
        self.ln_queue = None        # inside a Function's backward: deferred LayerNorm column sums (ops.layernorm_bwd_finish)
        self.fold_context = os.environ.get('VITED_FOLD_CONTEXT', '1') != '0'   # norm_context + kv of all decoder blocks as one GEMM
        # ... in ONE launch of ops.gemm_nt_wreg instead of one GEMM per block: the same bits, 426 -> 305 us for the eight of config A, but
        # 0.04 - 0.17 ms of the 23.4 ms step in four A / B sessions, inside the parent's run-to-run range in three of them: off by default
        # 
        self.kv_one_launch = os.environ.get('VITED_KV_ONE_LAUNCH', '0') != '0'
        self._fold_bufs = None      # (folded W [L 2D, D], its transpose, folded bias): refreshed in place every forward
        self._unit_ln = None        # (ones, zeros) for the affine-free LayerNorm of the features
        self.tap = None             # test/diagnostic: a dict that receives clones of per-block activations and gradients
        self.block_events = None    # measurement (bench.py): a list that receives (kind, block, 'fwd' | 'bwd', start event, end event)
        self.shadows = WeightShadows()   # the bf16 copies of the weights, and what a captured hipGraph needs kept alive
        if not self.exact:
            _install_optimizer_step_hook()

    @property
    def exact(self):
        return self.act_dtype == torch.float32

    def weight(self, w: torch.Tensor) -> torch.Tensor:
        """[N, K] operand of the forward GEMM in the activation dtype (cached per parameter version)."""
        w2 = w.detach().reshape(w.shape[0], -1)
        if self.exact:
            return w2
        return self.shadows.get(w, 'n', lambda out=None: ops.cast(w2, self.act_dtype, out=out))

    def weight_t(self, w: torch.Tensor):
        """Operand + layout of the input-gradient GEMM dX = dY . W: the transposed bf16 shadow (NT
        MFMA kernel) or, on the exact path, W itself read as [K, N]."""
        w2 = w.detach().reshape(w.shape[0], -1)
        if self.exact:
            return w2, B_KN
        return self.shadows.get(w, 't', lambda out=None: ops.cast_transpose(w2.contiguous(), self.act_dtype, out=out)), B_NK

    def refresh_shadows(self, params):
        self.shadows.refresh(params)


def shadows_of(model):
    """The WeightShadows of every Runtime of ``model`` (anything with a ``_runtimes`` dict; none without one)."""
    return [rt.shadows for rt in getattr(model, '_runtimes', {}).values()]


class _BlockSpan:
    """Brackets one block's launches with HIP events on the launch stream when ``rt.block_events`` is a list (bench.py's
    ``fused_block`` figure: time of the attention + MLP block's kernels); free otherwise."""

    def __init__(self, rt, kind, index, phase):
        self.sink, self.tag = rt.block_events, (kind, index, phase)

    def __enter__(self):
        if self.sink is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.sink is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.sink.append(self.tag + (self.e0, e1))
        return False


def _lp(rt: Runtime, t_f32: torch.Tensor) -> torch.Tensor:
    return t_f32 if rt.exact else ops.cast(t_f32, rt.act_dtype)


def _lp_scaled(rt: Runtime, t_f32: torch.Tensor, row_scale) -> torch.Tensor:
    """_lp with the copy scaled per row (on the exact path the copy then is a tensor of its own)."""
    return _lp(rt, t_f32) if row_scale is None else ops.scale_rows_cast(t_f32, row_scale, rt.act_dtype)


class _DropRows:
    """Stochastic-depth scales of one Function call as the kernels read them: one fp32 value per ROW.
    ``scales`` fp32 [blocks, branches, B] holds 0 or 1 / keep per sample; ``live[i][j]`` says whether branch j of block i drops at
    all - a branch that does not gets None everywhere and its launches are those of a model without stochastic depth.  The
    per-sample values are repeated over the ``n`` rows of a sample for every branch of the Function in ONE launch; a block
    that runs on the cls rows alone (``cls_block``: one row per sample) reads the per-sample vector itself."""

    def __init__(self, scales, live, n, cls_block=None):
        nblk, nbr, batch = scales.shape
        self.per_sample, self.live, self.cls_block = scales, live, cls_block
        self.per_row = scales.unsqueeze(-1).expand(nblk, nbr, batch, n).reshape(nblk, nbr, batch * n)

    def get(self, i, j):
        """Branch j of block i, one value per row of that block's stream; None where the branch does not drop (or i < 0)."""
        if i < 0 or not self.live[i][j]:
            return None
        return (self.per_sample if i == self.cls_block else self.per_row)[i, j]

    def block(self, i):
        return tuple(self.get(i, j) for j in range(self.per_sample.shape[1]))


def _take_drop_rows(dp, which, nblk, nbr, batch, n, device, cls_block=None):
    """The _DropRows of half ``which`` (0: encoder, 1: decoder) of this call from the Function's ``drop_path`` argument = (encoder scales
    fp32 [depth, 2, B] | None, decoder scales fp32 [c_depth, 3, B] | None, (live encoder branches, live decoder branches)) as
    model._resolve_drop_path returns it; None: no stochastic depth in this call."""
    if dp is None or dp[which] is None:
        return None
    scales, live = dp[which], dp[2][which]
    if not any(any(row) for row in live):
        return None
    if tuple(scales.shape) != (nblk, nbr, batch) or scales.dtype != torch.float32 or scales.device != device:
        raise ValueError(f'drop-path scales: expected fp32 {(nblk, nbr, batch)} on {device}, got {scales.dtype} {tuple(scales.shape)} on '
                         f'{scales.device}')
    return _DropRows(scales.contiguous(), live, n, cls_block)


# ---------------------------------------------------------------------------------------------
# shared pieces
# ---------------------------------------------------------------------------------------------
def _gtarget(rt, p):
    """p.grad when gradients may be accumulated straight into it (saves autograd's AccumulateGrad add and
    a temporary per parameter): only when the caller pre-attached dense fp32 .grad tensors."""
    if p is None or not rt.direct_grads:
        return None
    g = p.grad
    if g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape or g.device != p.device:
        return None
    return g


def _ln_bwd(rt, dy, x, gamma, beta, mean, rstd, **kw):
    """LayerNorm backward; returns (dx, dx_lp, dgamma | None, dbeta | None) - None when accumulated in place."""
    gg, gb = _gtarget(rt, gamma), _gtarget(rt, beta)
    if gg is not None and gb is not None:
        dx, dx_lp, _, _ = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dgamma=gg, dbeta=gb, **kw)
        return dx, dx_lp, None, None
    return ops.layernorm_bwd(dy, x, gamma, mean, rstd, **kw)


def _weight_grads(rt, dy, x_saved, w, b):
    """(dW | None, db | None) of y = x W^T + b; None when accumulated straight into w.grad / b.grad.  Inside a _DwBatch (one
    transformer block's backward) the product is only QUEUED: the block's weight gradients then go out as one launch.
    Under ``rt.keep_cam`` nothing is launched: that backward exists for the relevancy maps and hands no parameter gradient on."""
    if rt.keep_cam:
        return None, None
    gw = _gtarget(rt, w)
    gb = _gtarget(rt, b) if b is not None else None
    direct = gw is not None and (b is None or gb is not None)
    q = rt.dw_queue
    if q is not None and dy.dtype == torch.bfloat16 and dy.shape[0] >= 4096 and x_saved.shape[1] % 384 == 0:
        if direct:
            q.append((dy, x_saved, gw.view(gw.shape[0], -1), gb, True))
            return None, None
        dw = torch.empty((dy.shape[1], x_saved.shape[1]), dtype=torch.float32, device=dy.device)
        db = torch.empty(dy.shape[1], dtype=torch.float32, device=dy.device) if b is not None else None
        q.append((dy, x_saved, dw, db, False))
        return dw.view_as(w), db
    if direct:
        ops.linear_bwd_weight(dy, x_saved, want_bias=b is not None, dw_out=gw.view(gw.shape[0], -1), db_out=gb)
        return None, None
    dw, db = ops.linear_bwd_weight(dy, x_saved)
    return dw.view_as(w), (db if b is not None else None)


class _DwBatch:
    """``with _DwBatch(rt) as g:`` around a backward's LOOP over blocks, ``with g.block():`` around each block: the weight-gradient
    products issued inside are collected and launched together (vited_linear_bwd_weight_batched) - they only read tensors the
    block's backward already produced, and nothing inside a backward pass consumes a weight gradient.  The products of several
    blocks go out together (rt.group_dw), flushed when another block of the same size would no longer fit one round of 256
    workgroups (an encoder block of the embed-384 models is 36 output tiles of 128 x 384: seven blocks = 252 tiles = ONE row range
    per product - no split-M slabs to write and sum - where one block alone is cut into 7 row ranges)."""

    ROUND = 256

    def __init__(self, rt, kind=None):
        self.rt, self.blocks, self.kind = rt, rt.group_dw, kind

    def __enter__(self):
        self.outer = self.rt.dw_queue
        self.rt.dw_queue = [] if (self.rt.batch_dw and not self.rt.exact) else None
        self.mark = 0
        return self

    @contextlib.contextmanager
    def block(self):
        yield
        self._end_of_block()

    @staticmethod
    def _tiles(items):
        return sum(-(-dy.shape[1] // 128) * (x.shape[1] // 384) for dy, x, _dw, _db, _a in items)

    def _end_of_block(self):
        q = self.rt.dw_queue
        if q is None:
            return
        if not self.blocks:
            self.flush()
            return
        this, count = self._tiles(q[self.mark:]), len(q) - self.mark      # the block that just ended: the next one is taken to be alike
        self.mark = len(q)
        if self._tiles(q) + this > self.ROUND or len(q) + count > ops.MAX_BATCHED_WEIGHT_GRADS:
            self.flush()

    def flush(self):
        q = self.rt.dw_queue
        if not q:
            return
        self.rt.dw_queue, self.mark = [], 0
        with _BlockSpan(self.rt, self.kind, len(q), 'dw'):     # (bench.py: these launches belong to the blocks queued since the last flush)
            for acc in (True, False):
                _launch_weight_grads([(dy, x, dw, db) for dy, x, dw, db, a in q if a == acc], acc)

    def __exit__(self, exc_type, *exc):
        if exc_type is None:
            self.flush()
        self.rt.dw_queue = self.outer
        return False


def _launch_weight_grads(items, accumulate):
    """items: [(dy, x, dW target, dbias target | None)].  One batched launch per MAX_BATCHED_WEIGHT_GRADS products where the
    batched kernel covers them, otherwise one launch per product."""
    for i in range(0, len(items), ops.MAX_BATCHED_WEIGHT_GRADS):
        part = items[i: i + ops.MAX_BATCHED_WEIGHT_GRADS]
        if len(part) > 1 and ops.linear_bwd_weight_batched(part, accumulate):
            continue
        for dy, x, dw, db in part:
            if accumulate:
                ops.linear_bwd_weight(dy, x, want_bias=db is not None, dw_out=dw, db_out=db)
                continue
            got_w, got_b = ops.linear_bwd_weight(dy, x, want_bias=db is not None)
            dw.copy_(got_w)
            if db is not None:
                db.copy_(got_b)


def _linear_bwd(rt, dy, x_saved, w, b=None, aux=None):
    """(dx, dW, db) of y = x W^T + b given dy (activation dtype); with ``aux`` dx is multiplied by it elementwise."""
    wt, layout = rt.weight_t(w)
    if aux is not None:
        dx = ops.gemm(dy, wt, b_layout=layout, epilogue=EPI_MUL, aux=aux)
    else:
        dx = ops.gemm(dy, wt, b_layout=layout)
    dw, db = _weight_grads(rt, dy, x_saved, w, b)
    return dx, dw, db


def _row_kernel_ok(rt, m, n, k, dtype, *rowwise):
    """The row-complete Linear + LayerNorm kernels (gemm_row.hip) take this product: bf16, 384 output columns, dense rows."""
    return (rt.fused_ln and not rt.exact and ops.linear_layernorm_supported(m, n, k, dtype)
            and all(t is None or (t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 4 == 0) for t in rowwise))


def _res_linear(rt, a, w, bias, residual, ln=None, scale=None):
    """y = residual + a W^T + bias (fp32) and, with ``ln`` = (gamma, beta) of the LayerNorm that FOLLOWS on the residual stream
    (the next sub-block's norm: vision_transformer.py:124-127, 268-272), also (h, mean, rstd) = LayerNorm(y) - in ONE kernel when
    the row-complete kernel covers the shape, otherwise as vited_gemm(RESIDUAL) + vited_layernorm_fwd.
    ``scale`` (fp32, one value per row; stochastic depth): y = residual + scale[row] * (a W^T + bias), in the same kernels.
    Returns (y, (h, mean, rstd) | None)."""
    wsh = rt.weight(w)
    if ln is not None and _row_kernel_ok(rt, a.shape[0], wsh.shape[0], a.shape[1], a.dtype, a, residual):
        y, h, mean, rstd = ops.linear_residual_layernorm_fwd(a, wsh, bias, residual, ln[0], ln[1], LN_EPS, row_scale=scale)
        return y, (h, mean, rstd)
    y = ops.gemm(a, wsh, epilogue=EPI_RESIDUAL, bias=bias, residual=residual, row_scale=scale)
    return y, (ops.layernorm_fwd(y, ln[0], ln[1], LN_EPS, rt.act_dtype) if ln is not None else None)


def _linear_ln_bwd(rt, dy, h_saved, w, bias, x, gamma, beta, mean, rstd, dx_in=None, dx_out=None, want_lp=True, lp_scale=None):
    """Backward of  y = LayerNorm(x; gamma, beta) W^T + bias  given dy: the input-gradient GEMM and the LayerNorm backward in
    ONE kernel when the row-complete kernel covers the shape (d(LayerNorm output) then never exists in HBM).
    ``lp_scale`` (fp32, one value per row): the low-precision copy alone is scaled, dx_lp = T(lp_scale[row] * dx) - the stochastic-depth
    scale of the branch whose backward consumes it; on the exact path the copy then is an fp32 tensor of its own.
    Returns (dx fp32 = dx_in + ..., dx_lp | None (dx itself on the exact path), dgamma, dbeta, dW, dbias) - gradients are None when
    accumulated in place."""
    want_lp = want_lp and not rt.exact
    wt, layout = rt.weight_t(w)
    if layout == B_NK and _row_kernel_ok(rt, dy.shape[0], wt.shape[0], dy.shape[1], dy.dtype, dy, x, dx_in, dx_out):
        gg, gb = _gtarget(rt, gamma), _gtarget(rt, beta)
        direct = gg is not None and gb is not None
        dx, dx_lp, dg, db = ops.linear_layernorm_bwd(dy, wt, x, gamma, mean, rstd, dx_in=dx_in, dx_out=dx_out, want_lp=want_lp,
                                                     dgamma=gg if direct else None, dbeta=gb if direct else None, defer=rt.ln_queue,
                                                     lp_scale=lp_scale)
        if direct:
            dg = db = None
    else:
        dh = ops.gemm(dy, wt, b_layout=layout)
        dx, dx_lp, dg, db = _ln_bwd(rt, dh, x, gamma, beta, mean, rstd, dx_in=dx_in, dx_out=dx_out, want_lp=want_lp, lp_scale=lp_scale,
                                    lp_dtype=rt.act_dtype)
    dw, dbias = _weight_grads(rt, dy, h_saved, w, bias)
    return dx, (dx if rt.exact and lp_scale is None else dx_lp), dg, db, dw, dbias


@contextlib.contextmanager
def _ln_sums(rt):
    """``with _ln_sums(rt):`` around a Function's backward: the LayerNorm column sums that _linear_ln_bwd defers inside
    (d gamma, d beta of the row-complete kernel) go out together at the end, one launch per 16 LayerNorms."""
    rt.ln_queue = [] if not rt.exact else None
    try:
        yield
        ops.layernorm_bwd_finish(rt.ln_queue)           # (nothing to do for None or an empty list)
    finally:
        rt.ln_queue = None


def _keep_attention(rt, key, q, k):
    """KEEP_ATTN slow path (vision_transformer.py:67-75,188-195; consumer: scripts/visualise_attentions.py): materialise
    softmax(q k^T * scale) [B, h, Nq, Nk] with plain PyTorch ops, beside the fused kernels that never form it."""
    b, nq, d = q.shape
    qh = q.float().reshape(b, nq, rt.heads, rt.head_dim).transpose(1, 2)
    kh = k.float().reshape(b, k.shape[1], rt.heads, rt.head_dim).transpose(1, 2)
    rt.attn_store.setdefault(key, {})['attn'] = torch.softmax((qh * rt.scale) @ kh.transpose(-2, -1), dim=-1)


def _keep_attention_grad(rt, key, do, v):
    """What the reference's ``attn.register_hook(self.save_attn_gradients)`` records: d loss / d attn = dO V^T."""
    b, nq, d = do.shape
    doh = do.float().reshape(b, nq, rt.heads, rt.head_dim).transpose(1, 2)
    vh = v.float().reshape(b, v.shape[1], rt.heads, rt.head_dim).transpose(1, 2)
    rt.attn_store.setdefault(key, {})['grad'] = doh @ vh.transpose(-2, -1)


def _keep_attention_cam(rt, key, q, k, v, do, lse):
    """keep_cam: what the consumer of the two maps above reduces them to, mean_h max(attn o grad, 0) [B, Nq, Nk] (avg_heads of
    scripts/visualise_attentions.py), from the operands the attention backward is about to read - one kernel, no per-head map."""
    ent = rt.attn_store.setdefault(key, {})
    ent['cam'] = ops.attention_cam(q, k, v, do, lse, rt.heads, rt.scale, mode='grad')
    if key == ('cross_blocks', rt.c_depth - 1, 'cross_attn'):
        ent['cam_operands'] = (q, k, v, do, lse)   # the last cross-attention's operands: the 'raw' / 'gradcam' maps of engine.pair_relevancy


def _cam_only(rt, grads):
    """The parameter gradients a Function's backward returns: under ``rt.keep_cam`` none - autograd then adds nothing to any
    p.grad, and with direct gradients switched off for that backward (model.runtime) no kernel has added to one either."""
    return [None] * len(grads) if rt.keep_cam else grads


_QKN_FIELDS = ('gqn', 'bqn', 'gkn', 'bkn')
# what a self-attention's q/k-norm saves: the normalised q [batch, nq, D] and k [batch, n, D] as the attention read them (two views
# of one buffer; buffers of their own when cls_only) and the two norms' statistics
QkNormSaved = namedtuple('QkNormSaved', 'qn kn sq sk')


def _qk_norm_self(rt, qkv, P, batch, n, cls_only=False):
    """q_norm / k_norm of a self-attention on the packed projection qkv [batch n, 3D] (vision_transformer.py:60): the pre-norm q / k
    stay where the GEMM wrote them (the backward recomputes xhat from them), the normalised ones go to a buffer of their own that
    the attention kernels read.  ``cls_only``: the query is row 0 of every sample alone.
    Returns (q view [batch, nq, D], k view [batch, n, D], a QkNormSaved whose qn / kn are these two views)."""
    d = rt.dim
    if cls_only:
        qn = torch.empty((batch, d), dtype=qkv.dtype, device=qkv.device)
        kn = torch.empty((batch * n, d), dtype=qkv.dtype, device=qkv.device)
        _, _, sq, sk = ops.qk_norm_fwd(qkv.view(batch, n * 3 * d)[:, 0:d], qkv[:, d:2 * d], P.gqn, P.bqn, P.gkn, P.bkn, rt.heads, LN_EPS,
                                       out=(qn, kn))
        q3, k3 = qn.view(batch, 1, d), kn.view(batch, n, d)
    else:
        qk = torch.empty((batch * n, 2 * d), dtype=qkv.dtype, device=qkv.device)
        _, _, sq, sk = ops.qk_norm_fwd(qkv[:, 0:d], qkv[:, d:2 * d], P.gqn, P.bqn, P.gkn, P.bkn, rt.heads, LN_EPS,
                                       out=(qk[:, 0:d], qk[:, d:2 * d]))
        qk3 = qk.view(batch, n, 2 * d)
        q3, k3 = qk3[:, :, 0:d], qk3[:, :, d:2 * d]
    return q3, k3, QkNormSaved(q3, k3, sq, sk)


def _qk_norm_self_bwd(rt, dqkv, qkv, P, qkn, batch, n, cls_only=False):
    """Backward of _qk_norm_self, in place on the q and k columns of dqkv (they then are the gradient of the qkv projection's output).
    Returns the four norm-parameter gradients by field name - None when accumulated in place."""
    d = rt.dim
    rows = (lambda t: t.view(batch, n * 3 * d)[:, 0:d]) if cls_only else (lambda t: t[:, 0:d])
    targets = [_gtarget(rt, p) for p in (P.gqn, P.bqn, P.gkn, P.bkn)]
    direct = all(t is not None for t in targets)
    got = ops.qk_norm_bwd(rows(dqkv), rows(qkv), qkn.sq, P.gqn, dqkv[:, d:2 * d], qkv[:, d:2 * d], qkn.sk, P.gkn, rt.heads,
                          *(targets if direct else ()))
    return dict.fromkeys(_QKN_FIELDS) if direct else dict(zip(_QKN_FIELDS, got))


def _self_attn_fwd(rt, h, P, batch, n, key=None):
    """Returns (qkv, o, lse, qkn): ``qkn`` is what the q/k-norm saved (_qk_norm_self), None on a model without it."""
    d = rt.dim
    qkv = ops.gemm(h, rt.weight(P.wqkv), bias=P.bqkv)               # [M, 3D], columns [3][h][hd] (:58)
    qkv3 = qkv.view(batch, n, 3 * d)
    q3, k3, qkn = qkv3[:, :, 0:d], qkv3[:, :, d:2 * d], None
    if rt.qk_norm:
        q3, k3, qkn = _qk_norm_self(rt, qkv, P, batch, n)
    o, lse = ops.attention_fwd(q3, k3, qkv3[:, :, 2 * d:3 * d], rt.heads, rt.scale)
    if rt.keep_attn and key is not None:
        _keep_attention(rt, key, q3, k3)
    return qkv, o.view(batch * n, d), lse, qkn


def _self_attn_bwd(rt, do, qkv, o, lse, batch, n, key=None, P=None, qkn=None):
    """Returns (dqkv, the q/k-norm parameter gradients by field name: empty without the norm)."""
    d = rt.dim
    qkv3 = qkv.view(batch, n, 3 * d)
    q3, k3 = qkv3[:, :, 0:d], qkv3[:, :, d:2 * d]
    if qkn is not None:                                 # the attention saw the normalised q / k
        q3, k3 = qkn.qn, qkn.kn
    if rt.keep_attn and key is not None:
        _keep_attention_grad(rt, key, do.view(batch, n, d), qkv3[:, :, 2 * d:3 * d])
    if rt.keep_cam and key is not None:
        _keep_attention_cam(rt, key, q3, k3, qkv3[:, :, 2 * d:3 * d], do.view(batch, n, d), lse)
    dqkv = torch.empty_like(qkv)
    dqkv3 = dqkv.view(batch, n, 3 * d)
    ops.attention_bwd(q3, k3, qkv3[:, :, 2 * d:3 * d], o.view(batch, n, d),
                      do.view(batch, n, d), lse, rt.heads, rt.scale, dqkv3[:, :, 0:d], dqkv3[:, :, d:2 * d],
                      dqkv3[:, :, 2 * d:3 * d])
    return dqkv, (_qk_norm_self_bwd(rt, dqkv, qkv, P, qkn, batch, n) if qkn is not None else {})


FUSED_MLP_TILE = 128        # token rows per workgroup of vited_mlp_fwd (one workgroup per CU)
FUSED_MLP_CUS = 256


def _fused_mlp_rows(rt, x, w1, grad):
    """How many leading rows the fused MLP kernel (vited_mlp_fwd) takes: it runs one 128-row workgroup per CU, so a last
    round that fills less than a quarter of the chip is left to the unfused kernels (66,560 rows = 520 tiles = 2 rounds + 8
    tiles: the 8 tiles would cost a third round).  0 = do not use it.  Measured (profiles/mlp_probe.py, M = 65,536): it beats
    LayerNorm + fc1/GELU + fc2/residual when nothing is saved for backward (269 vs 344 us) and loses when the backward's
    operands must be written (376 us; in the training step: +0.9 ms), so it serves the no-grad paths (evaluation,
    similarity-matrix inference)."""
    if grad or rt.exact or not rt.fused_mlp or x.shape[1] != 384 or tuple(w1.shape) != (1536, 384) or x.stride(0) != 384:
        return 0
    tiles = x.shape[0] // FUSED_MLP_TILE
    rem = tiles % FUSED_MLP_CUS
    if tiles >= FUSED_MLP_CUS and rem < FUSED_MLP_CUS // 4:
        tiles -= rem
    elif x.shape[0] % FUSED_MLP_TILE:
        tiles += 1                      # ragged last tile: the kernel clamps rows
    return min(tiles * FUSED_MLP_TILE, x.shape[0])


def _hand_over_ln(rt, x, P, grad):
    """Whether the Linear kernels before and after this block's MLP (x: its input rows) also produce the LayerNorm that follows
    them: always when training; on the no-grad path only when the one-kernel MLP, which does its own LayerNorm, leaves the rows."""
    return grad or not _fused_mlp_rows(rt, x, P.w1, grad)


# what a stage's forward saves for its backward
MlpSaved = namedtuple('MlpSaved', 'mean rstd h gd u')                   # norm2's statistics and output, gelu'(z), gelu(z)
AttnSaved = namedtuple('AttnSaved', 'mean rstd h qkv o lse qkn')        # norm1's ...; qkn: what _qk_norm_self saved | None


def _mlp_fwd(rt, x, P, grad=True, ln=None, next_ln=None, scale=None):
    """x + fc2(gelu(fc1(LayerNorm(x)))) with the block's norm2 / mlp parameters (P: an EncBlock or a DecBlock).  ``ln`` = (h, mean,
    rstd) when the LayerNorm was already produced by the kernel that wrote x; ``next_ln`` = (gamma, beta) of the LayerNorm that
    follows on the output.  ``scale``: the branch's stochastic-depth scale per row; the one-kernel MLP does not know it and is
    then not chosen.  Returns (y, saved | None, next | None)."""
    g, b, w1, b1, w2, b2 = P.g2, P.b2, P.w1, P.bb1, P.w2, P.bb2
    rows = _fused_mlp_rows(rt, x, w1, grad) if ln is None and scale is None else 0
    if rows:
        y = torch.empty_like(x)
        ops.mlp_fwd(x[:rows], g, b, rt.weight(w1), b1, rt.weight(w2), b2, LN_EPS, save=False, out=(y[:rows], None, None, None, None, None))
        if rows < x.shape[0]:
            xt = x[rows:]
            ht, _, _ = ops.layernorm_fwd(xt, g, b, LN_EPS, rt.act_dtype)
            _, ut = ops.gemm(ht, rt.weight(w1), epilogue=EPI_GELU_GRAD, bias=b1)
            ops.gemm(ut, rt.weight(w2), epilogue=EPI_RESIDUAL, bias=b2, residual=xt, out=y[rows:])
        nxt = ops.layernorm_fwd(y, next_ln[0], next_ln[1], LN_EPS, rt.act_dtype) if next_ln is not None else None
        return y, None, nxt
    h, mean, rstd = ln if ln is not None else ops.layernorm_fwd(x, g, b, LN_EPS, rt.act_dtype)
    # fc1 saves gelu'(z) and gelu(z) (one exponential serves both): the backward of the activation is then one multiply
    gd, u = ops.gemm(h, rt.weight(w1), epilogue=EPI_GELU_GRAD, bias=b1)
    y, nxt = _res_linear(rt, u, w2, b2, x, next_ln, scale)
    return y, MlpSaved(mean, rstd, h, gd, u), nxt


def _mlp_bwd(rt, dy, dy_lp, x, P, saved, lp_scale=None):
    """Backward of _mlp_fwd.  Under stochastic depth ``dy_lp`` arrives scaled by this branch's scale (so everything inside the branch
    sees s dy, the residual path dy) and ``lp_scale`` is the scale of the branch whose backward runs next: the returned copy carries it.
    Returns (dx, its low-precision copy, the six parameter gradients by field name)."""
    s = saved
    dz, dw2, dbb2 = _linear_bwd(rt, dy_lp, s.u, P.w2, P.bb2, aux=s.gd)
    dx, dx_lp, dg2, db2, dw1, dbb1 = _linear_ln_bwd(rt, dz, s.h, P.w1, P.bb1, x, P.g2, P.b2, s.mean, s.rstd, dx_in=dy, lp_scale=lp_scale)
    return dx, dx_lp, dict(g2=dg2, b2=db2, w1=dw1, bb1=dbb1, w2=dw2, bb2=dbb2)


def _attn_branch_fwd(rt, x, P, batch, n, key=None, ln=None, next_ln=None, scale=None):
    """x + proj(attention(qkv(LayerNorm(x)))) with the block's norm1 / attn parameters; ``ln`` / ``next_ln`` as in _mlp_fwd.
    Returns (y, saved, next | None)."""
    h, mean, rstd = ln if ln is not None else ops.layernorm_fwd(x, P.g1, P.b1, LN_EPS, rt.act_dtype)
    qkv, o, lse, qkn = _self_attn_fwd(rt, h, P, batch, n, key)
    y, nxt = _res_linear(rt, o, P.wproj, P.bproj, x, next_ln, scale)
    return y, AttnSaved(mean, rstd, h, qkv, o, lse, qkn), nxt


def _attn_branch_bwd(rt, dy, dy_lp, x, P, saved, batch, n, key=None, lp_scale=None):
    """Backward of _attn_branch_fwd (``lp_scale`` as in _mlp_bwd).  Returns (dx, its low-precision copy, the six parameter gradients by
    field name)."""
    s = saved
    do, dwproj, dbproj = _linear_bwd(rt, dy_lp, s.o, P.wproj, P.bproj)
    dqkv, gn = _self_attn_bwd(rt, do, s.qkv, s.o, s.lse, batch, n, key, P, s.qkn)
    dx, dx_lp, dg1, db1, dwqkv, dbqkv = _linear_ln_bwd(rt, dqkv, s.h, P.wqkv, P.bqkv, x, P.g1, P.b1, s.mean, s.rstd, dx_in=dy, lp_scale=lp_scale)
    return dx, dx_lp, dict(g1=dg1, b1=db1, wqkv=dwqkv, bqkv=dbqkv, wproj=dwproj, bproj=dbproj, **gn)


def _take_patch_keep(patch_keep, which):
    """The keep table of this call's half (0: image 1, 1: image 2) from the Function's ``patch_keep`` argument = (image-1 table int32
    [B1, K1] | None, image-2 table [B2, K2] | None) as model._resolve_patch_keep returns it; None: no patch dropout in this call."""
    return patch_keep[which] if patch_keep is not None else None


def _take_pos_drop(pos_drop, which):
    """(seed int64 [1], rate) of this call's half (0: image 1, 1: image 2) from the Function's ``pos_drop`` argument = (image-1 seed | None,
    image-2 seed | None, rate) as model._resolve_pos_drop returns it; None: no position dropout in this call."""
    if pos_drop is None or pos_drop[which] is None:
        return None
    return pos_drop[which], pos_drop[2]


def _pos_drop(rt, x, batch, rows, with_cls, pos_drop, keep, in_place):
    """timm's pos_drop on a stream x fp32 [B*rows, D]: the elementwise mask of this call's seed, regenerated by the
    kernel wherever it is needed - on the tokens in the forward and, with the same arguments, on their gradient in the backward.
    Stream 0 is the image-1 path (n1 tokens), stream 1 the image-2 path (cls + n1 tokens); under patch dropout the rows carry the
    masks of their original tokens (``keep``: the table the stream was embedded through).  ``in_place`` only where nothing else reads x."""
    if pos_drop is None:
        return x
    seed, rate = pos_drop
    x3 = x.view(batch, rows, rt.dim)
    y = ops.token_dropout(x3, seed, rate, rt.n2 if with_cls else rt.n1, int(with_cls), keep=keep, lead=not with_cls,
                          out=x3 if in_place else None)
    return y.view(batch * rows, rt.dim)


def _patch_tokens_fwd(rt, img, S, with_cls, batch_index=None, keep=None, turn=None):
    """timm PatchEmbed + pos-embed (+ cls row, S: a DecShared) : returns x fp32 [B*rows, D] and the saved patch matrix.
    ``keep`` (int32 [B, K]; patch dropout): only the kept patches are extracted, embedded and given their
    position - rows = K + 1 either way: patch 0 leads without a cls row (the reference's prefix slot falls on it), the cls row with
    one.  Without it the launches are exactly those of a model that has no patch dropout.
    ``turn`` (an int 0..3 or an int tensor [B]; learned type-2 puzzles): the patches of every image turned by
    that many clockwise quarter turns, gathered from the upright image; None is the upright path, launch for launch."""
    if keep is not None:
        lead = not with_cls
        patches = ops.patchify_kept(img, rt.patch_size, rt.act_dtype, keep, lead, batch_index, mean=rt.input_mean, std=rt.input_std)
        tok = ops.gemm(patches, rt.weight(S.pw), epilogue=EPI_STORE_F32, bias=S.pb)
        x = ops.tokens_kept(tok, S.pos.view(rt.n2, rt.dim), S.cls.view(-1) if with_cls else None, keep, lead)
        batch, rows = x.shape[0], x.shape[1]
        return x.view(batch * rows, rt.dim), patches, batch, rows
    if turn is not None:
        patches = ops.patchify_turned(img, rt.patch_size, rt.act_dtype, turn, batch_index, mean=rt.input_mean, std=rt.input_std)
    else:
        patches = ops.patchify(img, rt.patch_size, rt.act_dtype, batch_index, mean=rt.input_mean, std=rt.input_std)
    batch = patches.shape[0] // rt.n1
    pos2 = S.pos.view(rt.n2, rt.dim)
    rows, first = (rt.n2, 1) if with_cls else (rt.n1, 0)        # under a cls row the patch tokens start at row 1 of every image
    x = ops.gemm(patches, rt.weight(S.pw), epilogue=EPI_RESIDUAL, bias=S.pb, residual=pos2[1 - first:], rows_per_batch=rt.n1,
                 out_rows_per_batch=rows, row_offset=first, residual_bcast=True, out_rows=batch * rows)
    if with_cls:
        ops.write_cls_row(x.view(batch, rt.n2, rt.dim), S.cls.view(-1), pos2)
    return x, patches, batch, rows


def _patch_tokens_bwd(rt, dx, patches, S, with_cls, batch, keep=None):
    """dx fp32 [B*rows, D] -> the gradients of pw, pb, pos (and cls) by field name.  ``keep``: the table the forward embedded through;
    d pos then sums every patch's row over the samples that kept it (ops.tokens_kept_bwd: fixed order, no atomics) and the
    weight gradient runs on the kept rows."""
    if keep is not None:
        rows = dx.shape[0] // batch
        dx3 = dx.view(batch, rows, rt.dim)
        dpos, dcls = ops.tokens_kept_bwd(dx3, ops.keep_inverse(keep, not with_cls, rt.n1), with_cls)
        grads = dict(pos=dpos.view_as(S.pos))
        if with_cls:
            grads['cls'] = dcls.view_as(S.cls)
            dtok = ops.slice_rows_cast(dx3, 1, rows - 1, rt.act_dtype)
        else:
            dtok = dx if rt.exact else ops.cast(dx, rt.act_dtype)
        grads['pw'], grads['pb'] = _weight_grads(rt, dtok, patches, S.pw, S.pb)
        return grads
    rows = rt.n2 if with_cls else rt.n1
    dx3 = dx.view(batch, rows, rt.dim)
    dpos_rows = ops.sum_rows(dx3.view(batch, rows * rt.dim)).view(rows, rt.dim)
    dpos = torch.zeros_like(S.pos)
    grads = dict(pos=dpos)
    if with_cls:
        dpos[0] = dpos_rows
        grads['cls'] = dpos_rows[0].clone().view_as(S.cls)
        dtok = ops.slice_rows_cast(dx3, 1, rt.n1, rt.act_dtype)
    else:
        dpos[0, 1:] = dpos_rows
        dtok = dx if rt.exact else ops.cast(dx, rt.act_dtype)
    grads['pw'], grads['pb'] = _weight_grads(rt, dtok, patches, S.pw, S.pb)
    return grads


def _norm1_of(blocks, i):
    """(gamma, beta) of block i's norm1, None past the last block: what the previous block's fc2 kernel is asked to produce."""
    return (blocks[i].g1, blocks[i].b1) if i < len(blocks) else None


# ---------------------------------------------------------------------------------------------
# encoder: forward_first_part (vision_transformer.py:382-388)
# ---------------------------------------------------------------------------------------------
# an encoder block's tape entry: the inputs of its two branches (x, xa) and what each saved (AttnSaved, MlpSaved)
EncTape = namedtuple('EncTape', 'x sa xa sm')


class EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rt: Runtime, drop_path, patch_keep, pos_drop, img, *params):
        """``drop_path`` / ``patch_keep`` / ``pos_drop``: this call's stochastic-depth scales, keep tables and position-dropout seeds as the
        model resolved them (_take_drop_rows, _take_patch_keep, _take_pos_drop), or None."""
        shared, blocks = split_params(params, EncShared, rt.enc_block)
        grad = any(ctx.needs_input_grad)  # False under no_grad: nothing is saved for inference
        keep = _take_patch_keep(patch_keep, 0)
        pdrop = _take_pos_drop(pos_drop, 0)
        x, patches, batch, n = _patch_tokens_fwd(rt, img, shared, with_cls=False, keep=keep)
        x = _pos_drop(rt, x, batch, n, False, pdrop, keep, in_place=True)      # the stream was just written and nothing else holds it
        if rt.tap is not None:
            rt.tap['enc.in'] = x.clone()        # the input of encoder block 0
        drop = _take_drop_rows(drop_path, 0, len(blocks), 2, batch, n, x.device)      # stochastic depth: per-row scales of (attn, mlp) per block
        tape = []
        ln1 = None          # (h, mean, rstd) of this block's norm1 when the previous block's fc2 kernel already produced it
        for i, P in enumerate(blocks):
            s_attn, s_mlp = drop.block(i) if drop is not None else (None, None)
            chain = _hand_over_ln(rt, x, P, grad or s_mlp is not None)
            with _BlockSpan(rt, 'enc', i, 'fwd'):
                xa, sa, ln2 = _attn_branch_fwd(rt, x, P, batch, n, key=('blocks', i, 'attn'), ln=ln1, next_ln=(P.g2, P.b2) if chain else None,
                                               scale=s_attn)
                xb, sm, ln1 = _mlp_fwd(rt, xa, P, grad, ln=ln2, next_ln=_norm1_of(blocks, i + 1) if chain else None, scale=s_mlp)
            if grad:
                tape.append(EncTape(x, sa, xa, sm))
            x = xb
            if rt.tap is not None:
                rt.tap[f'enc.x.{len(tape) - 1 if grad else 0}'] = x.clone()
        if grad:
            ctx.rt, ctx.tape, ctx.patches, ctx.batch, ctx.params = rt, tape, patches, batch, (shared, blocks)
            ctx.drop, ctx.n, ctx.keep, ctx.pos_drop = drop, n, keep, pdrop
        return x.view(batch, n, rt.dim)

    @staticmethod
    def backward(ctx, dout):
        rt, batch, n = ctx.rt, ctx.batch, ctx.n      # n: the call's token count (fewer than rt.n1 under patch dropout)
        shared, blocks = ctx.params
        dx = dout.contiguous().view(batch * n, rt.dim).float()
        if rt.tap is not None:
            rt.tap[f'enc.dx.{len(blocks)}'] = dx.clone()      # gradient w.r.t. the encoder's OUTPUT: what autograd hands over
        drop = ctx.drop
        scale_of = (lambda i, j: drop.get(i, j)) if drop is not None else (lambda i, j: None)
        dx_lp = _lp_scaled(rt, dx, scale_of(len(blocks) - 1, 1))      # the last block's MLP branch consumes it
        gblocks = [None] * len(blocks)
        with _ln_sums(rt), _DwBatch(rt, kind='enc') as dwg:      # the encoder's 2 x depth LayerNorm column sums
            for i in reversed(range(len(blocks))):
                t = ctx.tape[i]
                ctx.tape[i] = None
                with _BlockSpan(rt, 'enc', i, 'bwd'), dwg.block():
                    dx, dx_lp, gm = _mlp_bwd(rt, dx, dx_lp, t.xa, blocks[i], t.sm, lp_scale=scale_of(i, 0))
                    dx, dx_lp, ga = _attn_branch_bwd(rt, dx, dx_lp, t.x, blocks[i], t.sa, batch, n, key=('blocks', i, 'attn'),
                                                     lp_scale=scale_of(i - 1, 1))
                if rt.tap is not None:
                    rt.tap[f'enc.dx.{i}'] = dx.clone()      # gradient w.r.t. the INPUT of encoder block i
                gblocks[i] = rt.enc_block(**ga, **gm)
        # position dropout: the same mask on the stream's gradient, into a tensor of its own (dx may be the caller's gradient)
        dx = _pos_drop(rt, dx, batch, n, False, ctx.pos_drop, ctx.keep, in_place=False)
        gshared = EncShared(**_patch_tokens_bwd(rt, dx, ctx.patches, shared, with_cls=False, batch=batch, keep=ctx.keep))
        ctx.tape = ctx.patches = ctx.drop = ctx.keep = ctx.pos_drop = None
        return (None, None, None, None, None, *_cam_only(rt, flatten_params(gshared, gblocks)))


# ---------------------------------------------------------------------------------------------
# one CrossBlock (vision_transformer.py:268-272) in three stages: self-attention, cross-attention, MLP (_mlp_fwd / _mlp_bwd).
# DecoderFn (training and no_grad), decoder_cached and image2_tokens (pair-cached inference) are all built from them.
# ---------------------------------------------------------------------------------------------
def _dense_rows(t):
    """[rows, D] copy with row stride D (``.contiguous()`` keeps the strides of a one-row view, and the GEMM epilogue needs ldo)."""
    out = torch.empty(t.shape, dtype=t.dtype, device=t.device)
    out.copy_(t)
    return out


def _dec_self_fwd(rt, x, P, batch, n, cls_only, key=None, ln1=None, fuse_ln=True, scale=None):
    """Self stage: x -> (xa = x + attn(norm1(x)), saved, lnq).  ``cls_only`` (the LAST decoder block): only x[:, 0] of the
    block's output reaches the head (:400, :417 - the final norm and the head are row-wise), and within a CrossBlock the
    token rows only mix in the self-attention, as keys / values.  So after the block's qkv projection everything runs on the
    cls row alone: self-attention for query 0, proj, the whole cross-attention query side and the MLP - 1 row instead of
    N2 = 65 / 1025 per pair - with identical logits and gradients (the dropped rows' outputs are dead, their gradients exactly
    zero); xa is then [batch, D].  ``ln1`` = (h, mean, rstd) of norm1(x) when the previous block's fc2 kernel produced it.
    ``fuse_ln``: the proj kernel also produces lnq = (h, mean, rstd) of norm_cross(xa); else lnq is None (_cross_q computes it).
    ``scale``: the branch's stochastic-depth scale, one value per row of xa (per sample when cls_only)."""
    next_ln = (P.gc, P.bc) if fuse_ln else None
    if not cls_only:
        return _attn_branch_fwd(rt, x, P, batch, n, key=key, ln=ln1, next_ln=next_ln, scale=scale)
    d = rt.dim
    h1, m1, r1 = ln1 if ln1 is not None else ops.layernorm_fwd(x, P.g1, P.b1, LN_EPS, rt.act_dtype)
    qkv = ops.gemm(h1, rt.weight(P.wqkv), bias=P.bqkv)            # K and V of every row feed query 0
    qkv3 = qkv.view(batch, n, 3 * d)
    q0, k3, qkn = qkv3[:, 0:1, 0:d], qkv3[:, :, d:2 * d], None
    if rt.qk_norm:                                                  # the norm is per row: query 0's alone, every key's
        q0, k3, qkn = _qk_norm_self(rt, qkv, P, batch, n, cls_only=True)
    o0, lse0 = ops.attention_fwd(q0, k3, qkv3[:, :, 2 * d:3 * d], rt.heads, rt.scale)
    o0 = o0.view(batch, d)
    x0 = _dense_rows(x.view(batch, n, d)[:, 0, :])
    xa, lnq = _res_linear(rt, o0, P.wproj, P.bproj, x0, next_ln, scale)
    return xa, AttnSaved(m1, r1, h1, qkv, o0, lse0, qkn), lnq


def _dec_self_bwd(rt, dx, dx_lp, x, P, saved, batch, n, cls_only, key=None, lp_scale=None):
    """Backward of _dec_self_fwd.  dx / dx_lp: gradient w.r.t. xa (all rows, or the cls rows when cls_only); ``lp_scale`` as in _mlp_bwd
    (one value per row of x: all rows, also when cls_only).
    Returns (d x fp32 [batch n, D], its low-precision copy, the six parameter gradients by field name)."""
    if not cls_only:
        return _attn_branch_bwd(rt, dx, dx_lp, x, P, saved, batch, n, key=key, lp_scale=lp_scale)
    d = rt.dim
    s, qkv, qkn = saved, saved.qkv, saved.qkn        # (o and lse: of query 0 alone)
    do0, dwproj, dbproj = _linear_bwd(rt, dx_lp, s.o, P.wproj, P.bproj)
    qkv3 = qkv.view(batch, n, 3 * d)
    q0, k3 = qkv3[:, 0:1, 0:d], qkv3[:, :, d:2 * d]
    if qkn is not None:
        q0, k3 = qkn.qn, qkn.kn
    dqkv = torch.zeros_like(qkv)                 # d(q) of the rows that never queried is zero
    dqkv3 = dqkv.view(batch, n, 3 * d)
    ops.attention_bwd(q0, k3, qkv3[:, :, 2 * d:3 * d], s.o.view(batch, 1, d), do0.view(batch, 1, d),
                      s.lse, rt.heads, rt.scale, dqkv3[:, 0:1, 0:d], dqkv3[:, :, d:2 * d], dqkv3[:, :, 2 * d:3 * d])
    gn = _qk_norm_self_bwd(rt, dqkv, qkv, P, qkn, batch, n, cls_only=True) if qkn is not None else {}
    dres = torch.zeros((batch * n, d), dtype=torch.float32, device=dx.device)   # the residual path carries gradient on the cls rows only
    dres.view(batch, n, d)[:, 0, :].copy_(dx)
    dx, dx_lp, dg1, db1, dwqkv, dbqkv = _linear_ln_bwd(rt, dqkv, s.h, P.wqkv, P.bqkv, x, P.g1, P.b1, s.mean, s.rstd, dx_in=dres, lp_scale=lp_scale)
    return dx, dx_lp, dict(g1=dg1, b1=db1, wqkv=dwqkv, bqkv=dbqkv, wproj=dwproj, bproj=dbproj, **gn)


# a cross-attention's q/k-norm: a tensor beside the norm's statistics - ``qraw``: the PRE-norm queries, ``kn``: the NORMALISED keys
Normed = namedtuple('Normed', 't stats')
# what the cross stage saves: norm_cross's (mq, rq, hq), norm_context's (mc, rc, hc: None when the keys / values were computed ahead), q
# as the attention read it, kv (``folded``: this block's view of _context_kv_folded's all-blocks tensor), the attention's output and lse
CrossSaved = namedtuple('CrossSaved', 'mq rq hq mc rc hc q kv oc lse qraw kn folded')


def _cross_q(rt, xa, P, lnq=None):
    """q = Linear_q(norm_cross(xa)) of the cross-attention (:176); ``lnq`` = (h, mean, rstd) of norm_cross(xa) when the self
    stage's proj kernel produced it.  Returns (q in the activation dtype as the attention reads it, (h, mean, rstd), qraw): with the
    q/k-norm q is q_norm(Linear_q(...)) (:180) and ``qraw`` = Normed(the pre-norm q, its statistics) for the backward, else None."""
    hq, mq, rq = lnq if lnq is not None else ops.layernorm_fwd(xa, P.gc, P.bc, LN_EPS, rt.act_dtype)
    q = ops.gemm(hq, rt.weight(P.wq), bias=P.bq)
    if not rt.qk_norm:
        return q, (hq, mq, rq), None
    qn, _, sq, _ = ops.qk_norm_fwd(q, None, P.gcqn, P.bcqn, None, None, rt.heads, LN_EPS)
    return qn, (hq, mq, rq), Normed(q, sq)


def _k_norm_cross(rt, kv, P, in_place=False):
    """k_norm of a cross-attention on the K half of kv [Mc, 2D] (:180).  Returns Normed(normalised keys [Mc, D], their statistics);
    ``in_place`` (the inference caches: nothing is saved for a backward) writes them over the K half itself."""
    k = kv[:, 0:rt.dim]
    _, kn, _, sk = ops.qk_norm_fwd(None, k, None, None, P.gckn, P.bckn, rt.heads, LN_EPS, out=(None, k) if in_place else None)
    return Normed(kn, sk)


def _dec_cross_fwd(rt, xa, P, batch, lnq=None, q=None, kv3=None, ctxf=None, kv_index=None, key=None, fuse_ln=True, scale=None, items=None,
                   kn=None):
    """Cross stage (:174-200, :270): xa [batch Nq, D] -> (xb = xa + proj(attention(q, k, v)), saved, ln2) with q from the image-2
    tokens (_cross_q, unless the pair cache hands ``q`` over) and k / v from the image-1 features: ``kv3`` [., N1, 2 D] when they
    were computed ahead for all blocks (_context_kv_folded, context_kv; with ``kv_index`` pair p reads kv3[kv_index[p]]), else
    Linear_kv(norm_context(ctxf)) here - on ``items`` feature maps (default: one per pair).  ``fuse_ln``: the cross-proj kernel also
    produces ln2 = (h, mean, rstd) of norm2(xb).
    With the q/k-norm a ``q`` handed over is the normalised one, and keys computed ahead are either normalised in place inside ``kv3``
    (the inference cache) or come as ``kn`` = (normalised keys [items N1, D], their statistics) beside the pre-norm ones in kv3."""
    d, nq = rt.dim, xa.shape[0] // batch
    hq = mq = rq = hc = mc = rc = qraw = None
    if q is None:
        q, (hq, mq, rq), qraw = _cross_q(rt, xa, P, lnq)
    kv, ahead = kv3, kv3 is not None       # computed ahead: a view, nothing of norm_context is saved here
    if not ahead:
        hc, mc, rc = ops.layernorm_fwd(ctxf, P.gx, P.bx, LN_EPS, rt.act_dtype)
        kv = ops.gemm(hc, rt.weight(P.wkv), bias=P.bkv)              # [Mc, 2D], columns [2][h][hd] (:178)
        items = batch if items is None else items
        kv3 = kv.view(items, kv.shape[0] // items, 2 * d)      # the context's length is the call's: the features' token count
        if rt.qk_norm:
            kn = _k_norm_cross(rt, kv, P)
    k3 = kv3[:, :, 0:d] if kn is None else kn.t.view(kv3.shape[0], kv3.shape[1], d)
    oc, lse_c = ops.attention_fwd(q.view(batch, nq, d), k3, kv3[:, :, d:2 * d], rt.heads, rt.scale, kv_index=kv_index)
    if rt.keep_attn and key is not None:
        _keep_attention(rt, key, q.view(batch, nq, d), k3)
    oc = oc.view(batch * nq, d)
    xb, ln2 = _res_linear(rt, oc, P.wcp, P.bcp, xa, (P.g2, P.b2) if fuse_ln else None, scale)
    return xb, CrossSaved(mq, rq, hq, mc, rc, hc, q, kv, oc, lse_c, qraw, kn, folded=ahead), ln2


def _dec_cross_bwd(rt, dx, dx_lp, xa, P, saved, ctxf, dctx, batch, index, dkv3=None, lp_scale=None, seg=None):
    """Backward of _dec_cross_fwd.  Returns (d xa fp32, its low-precision copy, d context (accumulated in place), the ten parameter
    gradients by field name).  When the keys / values came from _context_kv_folded, d(kv) is written into ``dkv3`` (this block's
    view of the all-blocks tensor) and gx, bx, wkv, bkv stay None: _context_kv_folded_bwd fills them in after the last block.
    ``seg`` (ops.PairSegments): the keys / values are per IMAGE and pair p read item seg.index[p]; d(kv) is then per image too, each
    item the sum of its pairs' terms (ops.attention_bwd(segments=...)), and so is everything that follows it."""
    d, nq = rt.dim, xa.shape[0] // batch
    items = batch if seg is None else seg.items
    s, q, kv, oc, kn = saved, saved.q, saved.kv, saved.oc, saved.kn
    doc, dwcp, dbcp = _linear_bwd(rt, dx_lp, oc, P.wcp, P.bcp)
    dq = torch.empty_like(q)
    if s.folded:
        kv3, dkv = kv, dkv3                 # views of the all-blocks kv / d(kv) tensors
    else:
        dkv = torch.empty_like(kv)
        kv3, dkv3 = kv.view(items, kv.shape[0] // items, 2 * d), dkv.view(items, kv.shape[0] // items, 2 * d)
    k3 = kv3[:, :, 0:d] if kn is None else kn.t.view(items, kv3.shape[1], d)       # what the attention read: the normalised keys
    if rt.keep_attn:
        _keep_attention_grad(rt, ('cross_blocks', index, 'cross_attn'), doc.view(batch, nq, d), kv3[:, :, d:2 * d])
    if rt.keep_cam:
        _keep_attention_cam(rt, ('cross_blocks', index, 'cross_attn'), q.view(batch, nq, d), k3, kv3[:, :, d:2 * d],
                            doc.view(batch, nq, d), s.lse)
    ops.attention_bwd(q.view(batch, nq, d), k3, kv3[:, :, d:2 * d], oc.view(batch, nq, d),
                      doc.view(batch, nq, d), s.lse, rt.heads, rt.scale, dq.view(batch, nq, d), dkv3[:, :, 0:d],
                      dkv3[:, :, d:2 * d], segments=seg)
    if rt.tap is not None:
        i = index
        rt.tap[f'dec.doc.{i}'], rt.tap[f'dec.dq.{i}'], rt.tap[f'dec.dkv.{i}'] = doc.clone(), dq.clone(), dkv.clone()
        rt.tap[f'dec.q.{i}'], rt.tap[f'dec.kv.{i}'], rt.tap[f'dec.oc.{i}'] = q.clone(), kv.clone(), oc.clone()
    gn = {}
    if rt.qk_norm:
        # q_norm and k_norm backward in one launch, in place: dq and the K half of d(kv) become the projections' output gradients.  With
        # per-image keys (seg) d(kv) already is the sum over each image's pairs, so the norm's backward runs once per image
        fields = ('gcqn', 'bcqn', 'gckn', 'bckn')
        targets = [_gtarget(rt, getattr(P, f)) for f in fields]
        direct = all(t is not None for t in targets)
        got = ops.qk_norm_bwd(dq, s.qraw.t, s.qraw.stats, P.gcqn, dkv3.reshape(-1, 2 * d)[:, 0:d], kv3.reshape(-1, 2 * d)[:, 0:d], kn.stats, P.gckn,
                              rt.heads, *(targets if direct else ()))
        gn = dict.fromkeys(fields) if direct else dict(zip(fields, got))
    if rt.tap is not None:
        rt.tap[f'dec.dkvo.{index}'] = dkv.clone()     # gradient of the kv projection's OUTPUT (dec.dkv: before the k_norm backward)
    # q = Linear(norm_cross(x')), kv = Linear(norm_context(features)): input-gradient GEMM + LayerNorm backward fused
    dx, dx_lp, dgc, dbc, dwq, dbq = _linear_ln_bwd(rt, dq, s.hq, P.wq, P.bq, xa, P.gc, P.bc, s.mq, s.rq, dx_in=dx, lp_scale=lp_scale)
    dgx = dbx = dwkv = dbkv = None
    if not s.folded:
        # d(context) accumulates over the c_depth blocks in fp32, in place
        dctx, _, dgx, dbx, dwkv, dbkv = _linear_ln_bwd(rt, dkv, s.hc, P.wkv, P.bkv, ctxf, P.gx, P.bx, s.mc, s.rc, dx_in=dctx, dx_out=dctx, want_lp=False)
    return dx, dx_lp, dctx, dict(gc=dgc, bc=dbc, gx=dgx, bx=dbx, wq=dwq, bq=dbq, wkv=dwkv, bkv=dbkv, wcp=dwcp, bcp=dbcp, **gn)


# a decoder block's tape entry: the inputs of its three stages (x, xa, xb) and what each stage saved (AttnSaved, CrossSaved, MlpSaved)
DecTape = namedtuple('DecTape', 'x sa xa sc xb sm')


def _dec_block_fwd(rt, x, ctxf, P, batch, n, grad, cls_only, index=0, ln1=None, next_ln=None, kv3=None, scales=(None, None, None),
                   seg=None, kn=None):
    """One CrossBlock forward of DecoderFn: self + cross + MLP stage, every following LayerNorm asked of the Linear before it
    (``next_ln`` = (gamma, beta) of the NEXT block's norm1).  ``scales``: the stochastic-depth scales of the (self, cross, mlp) branches,
    each one value per row of its stage or None.  ``seg``: the context is per image, pair p attends over item seg.index[p].
    Returns (block output, tape entry | None, next block's ln1 | None)."""
    xa, sa, lnq = _dec_self_fwd(rt, x, P, batch, n, cls_only, key=('cross_blocks', index, 'attn'), ln1=ln1, scale=scales[0])
    xb, sc, ln2 = _dec_cross_fwd(rt, xa, P, batch, lnq=lnq, kv3=kv3, ctxf=ctxf, key=('cross_blocks', index, 'cross_attn'),
                                 fuse_ln=_hand_over_ln(rt, xa, P, grad or scales[2] is not None), scale=scales[1],
                                 kv_index=seg.index if seg is not None else None, items=seg.items if seg is not None else None, kn=kn)
    xc, sm, nxt = _mlp_fwd(rt, xb, P, grad, ln=ln2, next_ln=next_ln, scale=scales[2])
    return xc, (DecTape(x, sa, xa, sc, xb, sm) if grad else None), nxt


def _dec_block_bwd(rt, dx, dx_lp, ctxf, dctx, P, entry, batch, n, cls_only, index, dkv3=None, lp_scales=(None, None, None), seg=None):
    """Backward of _dec_block_fwd.  dx / dx_lp: gradient w.r.t. the block's output (all rows, or the cls rows when cls_only).
    ``lp_scales``: the stochastic-depth scales carried by the low-precision copies that leave the MLP, cross and self stage - those
    of this block's cross branch, of its self branch and of the PREVIOUS block's MLP branch.
    Returns (d input fp32, its low-precision copy, d context (accumulated in place), the parameter gradients as a DecBlock)."""
    t = entry
    dx, dx_lp, gm = _mlp_bwd(rt, dx, dx_lp, t.xb, P, t.sm, lp_scale=lp_scales[0])
    dx, dx_lp, dctx, gc = _dec_cross_bwd(rt, dx, dx_lp, t.xa, P, t.sc, ctxf, dctx, batch, index, dkv3, lp_scale=lp_scales[1], seg=seg)
    dx, dx_lp, ga = _dec_self_bwd(rt, dx, dx_lp, t.x, P, t.sa, batch, n, cls_only, key=('cross_blocks', index, 'attn'), lp_scale=lp_scales[2])
    return dx, dx_lp, dctx, rt.dec_block(**ga, **gc, **gm)


# ---------------------------------------------------------------------------------------------
# pair-cached decoder for similarity-matrix inference (hisfrag.py:213-231)
# ---------------------------------------------------------------------------------------------
# hisfrag.py:226-229 calls model(x1[idx1], x2[idx2]) per pair batch, so the reference (and DecoderFn) re-embeds image 2 and
# re-runs norm_context + the kv projection of every decoder block for EVERY pair.  Neither depends on the pair:
#   * prepare_x2 (vision_transformer.py:390-395) depends on image j only  -> image2_tokens(), once per image;
#   * cross-attention keys / values (:177-179) depend on image i's features only -> context_kv(), once per image-1 row block;
# the pair batch then gathers token rows by index j and the attention kernel reads K / V by index i (vited_attention_fwd_indexed).
# ``params`` is the decoder's flat parameter list (model._decoder_params) throughout.
@torch.no_grad()
def image2_tokens(rt: Runtime, img, params, turn=None):
    """Everything of the decoder that depends on image 2 ALONE, once per image:
      * x  = patch embedding + cls row + pos_embed (timm _pos_embed), the decoder's input stream;
      * x' = x + attn(norm1(x)) of the FIRST CrossBlock (its self-attention sees image 2 only: the features enter at the
             cross-attention that follows, vision_transformer.py:269-270) - unless that block is also the last one (cls-only);
      * q  = Linear_q(norm_cross(x')) of that block's cross-attention (:176), activation dtype.
    Returns (x' or x as [n, N2, D] fp32, q [n, N2, D] or None).  ``turn``: the images enter turned (``_patch_tokens_fwd``)."""
    shared, blocks = split_params(params, rt.dec_shared, rt.dec_block)
    x, _, batch, _ = _patch_tokens_fwd(rt, img, shared, with_cls=True, turn=turn)
    if not blocks or (rt.cls_tail and rt.c_depth == 1):
        return x.view(batch, rt.n2, rt.dim), None
    xa, _, lnq = _dec_self_fwd(rt, x, blocks[0], batch, rt.n2, cls_only=False)
    q, _, _ = _cross_q(rt, xa, blocks[0], lnq)          # (with the q/k-norm: the normalised queries)
    return xa.view(batch, rt.n2, rt.dim), q.view(batch, rt.n2, rt.dim)


@torch.no_grad()
def context_kv(rt: Runtime, feats, params):
    """Per decoder block: kv = Linear_kv(norm_context(features)) as [b1, N1, 2 D] in the activation dtype (columns [2][h][hd]); with the
    q/k-norm the K half is k_norm of it, which is what decoder_cached's attention reads."""
    _, blocks = split_params(params, rt.dec_shared, rt.dec_block)
    b1 = feats.shape[0]
    ctxf = feats.detach().contiguous().float().view(b1 * rt.n1, rt.dim)
    out = []
    for P in blocks:
        hc, _, _ = ops.layernorm_fwd(ctxf, P.gx, P.bx, LN_EPS, rt.act_dtype)
        kv = ops.gemm(hc, rt.weight(P.wkv), bias=P.bkv)
        if rt.qk_norm:
            _k_norm_cross(rt, kv, P, in_place=True)          # the cache holds the NORMALISED keys
        out.append(kv.view(b1, rt.n1, 2 * rt.dim))
    return out


@torch.no_grad()
def decoder_cached(rt: Runtime, tokens2, j_idx, kvs, i_idx, params, q0=None):
    """Logits [P, C] of the pairs (image-1 row i_idx[p] of the cached block, image j_idx[p]): forward_second_part + forward_head
    (vision_transformer.py:397-405,417) on cached image-2 tokens and cached cross-attention keys / values.  With ``q0`` the cache
    already holds block 0's self-attention branch and cross-attention queries (image2_tokens)."""
    shared, blocks = split_params(params, rt.dec_shared, rt.dec_block)
    d, n = rt.dim, rt.n2
    batch = j_idx.numel()
    x = tokens2.index_select(0, j_idx).view(batch * n, d)
    for l, (P, kv3) in enumerate(zip(blocks, kvs)):
        cls_only = rt.cls_tail and l == rt.c_depth - 1          # see _dec_self_fwd: the last block runs on the cls row alone
        lnq = q = None
        if l == 0 and q0 is not None:
            xa, q = x, q0.index_select(0, j_idx)                  # cached: x IS x + attn(norm1(x)) of block 0
        else:
            # fuse_ln: the historical form of this path, not a measured choice - its cls-rows-only proj leaves norm_cross to a
            # separate launch (DecoderFn fuses it), and below its cross-proj never produces norm2, its fc2 never the next norm1
            xa, _, lnq = _dec_self_fwd(rt, x, P, batch, n, cls_only, fuse_ln=not cls_only)
        xb, _, _ = _dec_cross_fwd(rt, xa, P, batch, lnq=lnq, q=q, kv3=kv3, kv_index=i_idx, fuse_ln=False)
        x, _, _ = _mlp_fwd(rt, xb, P, grad=False)
    return _head_fwd(rt, x, shared, batch, n, rt.cls_tail and rt.c_depth > 0, save=False)[0]


# ---------------------------------------------------------------------------------------------
# decoder + head: forward_second_part + forward_head (vision_transformer.py:390-405,417)
# ---------------------------------------------------------------------------------------------
def _kv_params(blocks):
    """(kv weights, kv biases, norm_context gammas, norm_context betas) of every decoder block: what the fold works on."""
    return [P.wkv for P in blocks], [P.bkv for P in blocks], [P.gx for P in blocks], [P.bx for P in blocks]


FoldSaved = namedtuple('FoldSaved', 'kv_all xhat mean rstd wt')      # what _context_kv_folded leaves for _context_kv_folded_bwd
# the head's norm: its input rows (the cls rows, or under 'avg' + fc_norm the pooled rows), its output in the activation dtype, its statistics
FinalSaved = namedtuple('FinalSaved', 'xcls y mean rstd')
# 'avg' without fc_norm, where norm and pooling are one kernel: the last block's output [B, n, D], the pooled rows in the activation dtype
# (the head GEMM's operand), the statistics of norm on every pooled row [B n]
PoolSaved = namedtuple('PoolSaved', 'x y mean rstd')


def _context_kv_folded(rt, ctxf, blocks):
    """Keys / values of EVERY decoder block from one LayerNorm and one GEMM (csrc/context_fold.hip): xhat = LayerNorm(features; 1, 0),
    kv_all = xhat W'^T + b' with W'_l = W_l o gamma_l, b'_l = b_l + W_l beta_l stacked over the blocks.
    Returns FoldSaved(kv_all [L, Mc, 2D], xhat, mean, rstd, wt = the folded weights' transpose [D, L 2D])."""
    dev = ctxf.device
    if rt._unit_ln is None or rt._unit_ln[0].device != dev:
        rt._unit_ln = (torch.ones(rt.dim, dtype=torch.float32, device=dev), torch.zeros(rt.dim, dtype=torch.float32, device=dev))
    ws, bs, gs, bes = _kv_params(blocks)
    bufs = rt._fold_bufs
    if bufs is not None and (bufs[0].shape[0] != len(blocks) * 2 * rt.dim or bufs[0].device != dev):
        rt.shadows.retire(bufs)             # a captured graph may still read them
        bufs = None
    rt._fold_bufs = bufs = ops.fold_context_weights([w.detach() for w in ws], [b.detach() if b is not None else None for b in bs],
                                                    [g.detach() for g in gs], [b.detach() for b in bes], out=bufs)
    xhat, mean, rstd = ops.layernorm_fwd(ctxf, rt._unit_ln[0], rt._unit_ln[1], LN_EPS, rt.act_dtype)
    # one [Mc, 2D] tensor per block (each block's attention then reads dense rows; ONE [Mc, L 2D] product would also push the stacked
    # weights - 4.7 MB at 8 blocks - out of an XCD's L2: measured 690 us for the single GEMM against 8 x 55 us)
    n2 = 2 * rt.dim
    kv_all = torch.empty((len(blocks), ctxf.shape[0], n2), dtype=rt.act_dtype, device=dev)
    wf, wft, bf = bufs
    # rt.kv_one_launch, 384-wide models: all 2 L key / value groups in one launch of the weights-in-registers kernel, which holds a
    # group's weights for the whole launch (nothing to fall out of L2) and addresses kv_all[l]'s dense rows itself; the same bits as the loop
    if (rt.kv_one_launch and rt.dim == ops.WREG_WIDTH and xhat.dtype == torch.bfloat16
            and ops.gemm_nt_wreg_supported(xhat.shape[0], 2 * len(blocks), 2, lda=xhat.stride(0), ldw=wf.stride(0))):
        ops.gemm_nt_wreg(xhat, wf, bf, kv_all, groups=2 * len(blocks))
        return FoldSaved(kv_all, xhat, mean, rstd, wt=wft)
    for l in range(len(blocks)):
        ops.gemm(xhat, wf[l * n2:(l + 1) * n2], bias=bf[l * n2:(l + 1) * n2], out=kv_all[l])
    return FoldSaved(kv_all, xhat, mean, rstd, wt=wft)


def _context_kv_folded_bwd(rt, dkv_all, ctxf, saved, blocks):
    """Backward of _context_kv_folded once every block has written its d(kv) slice: d(features) from ONE row-complete kernel
    (input-gradient GEMM with K = L 2D + the affine-free LayerNorm's backward), the folded weights' gradient from one
    weight-gradient GEMM, unfolded into dW_kv, db_kv, d(norm_context.weight / bias) of every block.
    Returns (d features fp32, per block the gradients of gx, bx, wkv, bkv by field name - None when accumulated straight into .grad)."""
    xhat, wt = saved.xhat, saved.wt
    ones = rt._unit_ln[0]
    nblk, mc, n2 = dkv_all.shape
    if _row_kernel_ok(rt, mc, wt.shape[0], nblk * n2, dkv_all.dtype, ctxf):
        dctx, _, _, _ = ops.linear_layernorm_bwd(dkv_all, wt, ctxf, ones, saved.mean, saved.rstd)      # contraction over all blocks' d(kv)
    else:
        dh = torch.zeros((mc, rt.dim), dtype=torch.float32, device=ctxf.device)
        for l in range(nblk):
            dh = ops.gemm(dkv_all[l], wt[:, l * n2:(l + 1) * n2], epilogue=EPI_RESIDUAL, residual=dh)
        dctx, _, _, _ = ops.layernorm_bwd(dh, ctxf, ones, saved.mean, saved.rstd)
    dwf = torch.empty((nblk * n2, rt.dim), dtype=torch.float32, device=ctxf.device)
    dbf = torch.empty(nblk * n2, dtype=torch.float32, device=ctxf.device)
    _launch_weight_grads([(dkv_all[l], xhat, dwf[l * n2:(l + 1) * n2], dbf[l * n2:(l + 1) * n2]) for l in range(nblk)], False)
    ws, bs, gs, bes = _kv_params(blocks)
    targets = [(_gtarget(rt, w), _gtarget(rt, b) if b is not None else None, _gtarget(rt, g), _gtarget(rt, be)) for w, b, g, be in zip(ws, bs, gs, bes)]
    direct = all(tw is not None and tg is not None and tbe is not None and (b is None or tb is not None) for (tw, tb, tg, tbe), b in zip(targets, bs))
    if not direct:
        targets = [(torch.empty_like(w), torch.empty_like(b) if b is not None else None, torch.empty_like(g), torch.empty_like(be))
                   for w, b, g, be in zip(ws, bs, gs, bes)]
    ops.unfold_context_grads(dwf, dbf, [w.detach() for w in ws], [g.detach() for g in gs], [b.detach() for b in bes],
                             [tw for tw, _, _, _ in targets], [tb for _, tb, _, _ in targets], [tg for _, _, tg, _ in targets],
                             [tbe for _, _, _, tbe in targets], accumulate=direct)
    return dctx, [dict.fromkeys(('gx', 'bx', 'wkv', 'bkv')) if direct else dict(gx=tg, bx=tbe, wkv=tw, bkv=tb) for tw, tb, tg, tbe in targets]


def _head_fwd(rt, x, S, batch, n, cls_rows, save=True):
    """norm, pooling and head on the last block's output x - fp32 [batch n, D], or [batch, D] when that block ran on the cls rows alone
    (``cls_rows``) - as cross_part's last line and timm's forward_head order them (vision_transformer.py:400,417):
      'token':           norm on the cls rows alone (LayerNorm is row-wise), head; with fc_norm the same arithmetic under the other keys;
      'avg' + fc_norm:   mean of the rows behind the cls row (ops.token_pool_fwd), fc_norm on [batch, D], head;
      'avg' alone:       norm on every row and the mean of the rows behind the cls row in ONE kernel - the normalised rows never exist.
    Returns (logits fp32 [batch, C], a FinalSaved or PoolSaved for _final_norm_bwd / _pool_bwd)."""
    d = rt.dim
    if rt.pool_avg and not rt.fc_norm:
        x3 = x.view(batch, n, d)
        pooled, mean, rstd = ops.token_pool_fwd(x3, 1, S.gN, S.bN, LN_EPS, save_stats=save)
        saved = PoolSaved(x3, _lp(rt, pooled), mean, rstd)
    else:
        if rt.pool_avg:
            rows, _, _ = ops.token_pool_fwd(x.view(batch, n, d), 1)
        else:
            rows = x if cls_rows else x.view(batch, n, d)[:, 0, :]
        saved = FinalSaved(rows, *ops.layernorm_fwd(rows, S.gN, S.bN, LN_EPS, rt.act_dtype))
    return ops.gemm(saved.y, rt.weight(S.wh), epilogue=EPI_STORE_F32, bias=S.bh), saved


def _pool_bwd(rt, dy, final, S, s_head, batch, n):
    """_final_norm_bwd under 'avg': (d x fp32 [batch n, D], its low-precision copy, d gN, d bN) given dy [B, D] at the head GEMM's operand.
    ops.token_pool_bwd writes every row of d x and of the copy itself, the zero cls rows included; the copy carries ``s_head``."""
    d = rt.dim
    lp_dtype = rt.act_dtype if (s_head is not None or not rt.exact) else None
    if rt.fc_norm:
        dpool, _, dgN, dbN = _ln_bwd(rt, dy, final.xcls, S.gN, S.bN, final.mean, final.rstd)
        dx, dx_lp, _, _ = ops.token_pool_bwd(dpool, n, 1, lp_dtype=lp_dtype, lp_scale=s_head)
    else:
        gg, gb = _gtarget(rt, S.gN), _gtarget(rt, S.bN)
        direct = gg is not None and gb is not None
        dx, dx_lp, dgN, dbN = ops.token_pool_bwd(dy if rt.exact else ops.cast(dy, torch.float32), n, 1, x=final.x, gamma=S.gN, mean=final.mean,
                                                 rstd=final.rstd, lp_dtype=lp_dtype, lp_scale=s_head, dgamma=gg if direct else None,
                                                 dbeta=gb if direct else None)
        if direct:
            dgN = dbN = None
    dx = dx.view(batch * n, d)
    return dx, (dx if dx_lp is None else dx_lp.view(batch * n, d)), dgN, dbN


def _final_norm_bwd(rt, dy, final, S, s_head, cls_tail, batch, n):
    """Backward of the final norm (on the cls rows) given dy [B, D].  Returns (d x fp32, its low-precision copy, d gN, d bN) over the rows
    of the last block's output: the cls rows when it ran on them alone (``cls_tail``), else all rows, zero but for the cls rows.
    ``s_head``: the per-sample stochastic-depth scale the low-precision copy carries (see the caller), or None."""
    if rt.pool_avg:
        return _pool_bwd(rt, dy, final, S, s_head, batch, n)
    d = rt.dim
    kw = dict(lp_scale=s_head, lp_dtype=rt.act_dtype) if s_head is not None else {}
    if cls_tail:
        if s_head is None:
            kw = dict(want_lp=not rt.exact)
        dx, dx_lp, dgN, dbN = _ln_bwd(rt, dy, final.xcls, S.gN, S.bN, final.mean, final.rstd, **kw)
    else:
        dx = torch.zeros((batch * n, d), dtype=torch.float32, device=dy.device)
        dx_lp = dx_lp0 = None
        if s_head is not None or not rt.exact:
            dx_lp = torch.zeros((batch * n, d), dtype=rt.act_dtype, device=dy.device)
            dx_lp0 = dx_lp.view(batch, n, d)[:, 0, :]
        _, _, dgN, dbN = _ln_bwd(rt, dy, final.xcls, S.gN, S.bN, final.mean, final.rstd, dx_out=dx.view(batch, n, d)[:, 0, :], dx_lp=dx_lp0, **kw)
    if rt.exact and s_head is None:
        dx_lp = dx
    return dx, dx_lp, dgN, dbN


class DecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rt: Runtime, drop_path, patch_keep, pos_drop, feats, img2, img2_index, img1_index, *params):
        """``drop_path`` / ``patch_keep`` / ``pos_drop``: as in EncoderFn.forward.
        ``img2_index`` (int64 [P] | None): pair p embeds img2[img2_index[p]] (gathered inside the patch-embedding kernel).
        ``img1_index`` (ops.PairSegments | None): ``feats`` holds one item per IMAGE and pair p attends over feats[index[p]]: norm_context
        and the kv projections run once per image, the cross-attention reads them through the index, and the backward sums every
        image's d(kv) over its pairs before the per-image kv / norm_context backward (hisfrag.py:117-159 without its two gathers)."""
        shared, blocks = split_params(params, rt.dec_shared, rt.dec_block)
        grad = any(ctx.needs_input_grad)
        keep = _take_patch_keep(patch_keep, 1)
        pdrop = _take_pos_drop(pos_drop, 1)
        x, patches, batch, n = _patch_tokens_fwd(rt, img2, shared, with_cls=True, batch_index=img2_index, keep=keep)
        x = _pos_drop(rt, x, batch, n, True, pdrop, keep, in_place=True)       # per pair of the call, also under an image-2 index
        if rt.tap is not None:
            rt.tap['dec.in'] = x.clone()        # the input of decoder block 0
        seg = img1_index
        b1 = batch if seg is None else seg.items
        if seg is not None:
            if rt.keep_attn or rt.keep_cam:
                raise NotImplementedError('the attention-map paths (keep_attn / keep_cam) take gathered features, not an image-1 index')
            if seg.index.numel() != batch:
                raise ValueError(f'{seg.index.numel()} image-1 indices for {batch} image-2 samples')
        nc = feats.shape[1] if feats.dim() == 3 else 0      # the context's tokens: rt.n1, or what the encoder kept under patch dropout
        if feats.dim() != 3 or feats.shape != (b1, nc, rt.dim) or not 1 <= nc <= rt.n1:
            raise ValueError(f'features {tuple(feats.shape)} do not match {b1} context items of 1 to {rt.n1} tokens')
        ctxf = feats.detach().contiguous().float().view(b1 * nc, rt.dim)
        tape = []
        d = rt.dim
        cls_tail = rt.cls_tail and rt.c_depth > 0 and not (rt.keep_attn or rt.keep_cam)    # the visualisation paths want every query row's map
        drop = _take_drop_rows(drop_path, 1, len(blocks), 3, batch, n, x.device, cls_block=rt.c_depth - 1 if cls_tail else None)
        ln1 = None
        fold = rt.fold_context and not rt.exact and rt.c_depth > 1 and rt.c_depth <= ops.MAX_FOLDED_BLOCKS and rt.dim % 32 == 0
        folded = kv_all = kn_all = None
        if fold:
            folded = _context_kv_folded(rt, ctxf, blocks)
            kv_all = folded.kv_all
            if rt.qk_norm:          # k_norm per block on its keys, once per context item (per image under an image-1 index)
                kn_all = [_k_norm_cross(rt, kv_all[l], P) for l, P in enumerate(blocks)]
        for i, P in enumerate(blocks):
            x, entry, ln1 = _dec_block_fwd(rt, x, ctxf, P, batch, n, grad, cls_tail and i == rt.c_depth - 1, index=i, ln1=ln1,
                                           next_ln=_norm1_of(blocks, i + 1), kv3=kv_all[i].view(b1, nc, 2 * d) if fold else None,
                                           scales=drop.block(i) if drop is not None else (None, None, None), seg=seg,
                                           kn=kn_all[i] if kn_all is not None else None)
            if grad:
                tape.append(entry)
            if rt.tap is not None:
                rt.tap[f'dec.x.{i}'] = x.clone()
        # final norm on the cls rows only (LayerNorm is row-wise; only x[:, 0] reaches the head, :400,:417); under 'avg' the pooled head
        logits, final = _head_fwd(rt, x, shared, batch, n, cls_tail, save=grad)
        if grad:
            ctx.rt, ctx.tape, ctx.patches, ctx.batch, ctx.params = rt, tape, patches, batch, (shared, blocks)
            ctx.ctxf, ctx.final, ctx.cls_tail = ctxf, final, cls_tail
            ctx.feats_needs_grad = feats.requires_grad
            ctx.fold = folded           # a FoldSaved; None when every block computes its own keys / values
            ctx.drop = drop
            ctx.seg, ctx.n, ctx.nc, ctx.keep, ctx.pos_drop = seg, n, nc, keep, pdrop
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        rt, batch, n, nc, d = ctx.rt, ctx.batch, ctx.n, ctx.nc, ctx.rt.dim      # n, nc: the call's image-2 and context token counts
        shared, blocks = ctx.params
        final = ctx.final
        # head: logits = y Wh^T + bh
        dl = _lp(rt, dlogits.contiguous().float())
        wh_act = rt.weight(shared.wh)
        dy = ops.gemm(dl, wh_act, b_layout=B_KN)                         # [B, D]
        dwh, dbh = _weight_grads(rt, dl, final.y, shared.wh, shared.bh)
        drop, last = ctx.drop, len(blocks) - 1
        seg = ctx.seg
        b1 = batch if seg is None else seg.items
        scale_of = (lambda i, j: drop.get(i, j)) if drop is not None else (lambda i, j: None)
        # the low-precision copy that leaves the final norm feeds the last block's MLP branch: it carries that branch's scale, per
        # sample (the final norm runs on the cls rows)
        s_head = drop.per_sample[last, 2] if drop is not None and drop.live[last][2] else None
        dx, dx_lp, dgN, dbN = _final_norm_bwd(rt, dy, final, shared, s_head, ctx.cls_tail, batch, n)
        if rt.tap is not None:
            rt.tap[f'dec.dx.{len(blocks)}'] = dx.clone()      # gradient w.r.t. the last block's OUTPUT (its cls rows under the cls tail)
        dctx = None
        gblocks = [None] * len(blocks)
        dkv_all = torch.empty_like(ctx.fold.kv_all) if ctx.fold else None
        with _ln_sums(rt):                              # the decoder's 4 x c_depth LayerNorm column sums
            with _DwBatch(rt, kind='dec') as dwg:
                for i in reversed(range(len(blocks))):
                    entry = ctx.tape[i]
                    ctx.tape[i] = None
                    with dwg.block():
                        dx, dx_lp, dctx, gblocks[i] = _dec_block_bwd(rt, dx, dx_lp, ctx.ctxf, dctx, blocks[i], entry, batch, n,
                                                                     ctx.cls_tail and i == rt.c_depth - 1, i,
                                                                     dkv3=dkv_all[i].view(b1, nc, 2 * d) if ctx.fold else None,
                                                                     lp_scales=(scale_of(i, 1), scale_of(i, 0), scale_of(i - 1, 2)), seg=seg)
                    if rt.tap is not None:
                        rt.tap[f'dec.dx.{i}'] = dx.clone()      # gradient w.r.t. the INPUT of decoder block i
                        if dctx is not None:
                            rt.tap[f'dec.dctx.{i}'] = dctx.clone()  # running d(features) after blocks c_depth-1 .. i
            if ctx.fold:
                dctx, kv_grads = _context_kv_folded_bwd(rt, dkv_all, ctx.ctxf, ctx.fold, blocks)
                gblocks = [g._replace(**kv) for g, kv in zip(gblocks, kv_grads)]
                ctx.fold = None
        if rt.tap is not None and dctx is not None:
            rt.tap['dec.dfeats'] = dctx.clone()     # total d(features), whichever way the keys / values were computed
        dx = _pos_drop(rt, dx, batch, n, True, ctx.pos_drop, ctx.keep, in_place=False)     # position dropout on the stream's gradient
        gshared = rt.dec_shared(**_patch_tokens_bwd(rt, dx, ctx.patches, shared, with_cls=True, batch=batch, keep=ctx.keep), gN=dgN, bN=dbN, wh=dwh, bh=dbh)
        dfeats = dctx.view(b1, nc, d) if ctx.feats_needs_grad and dctx is not None else None
        ctx.tape = ctx.patches = ctx.ctxf = ctx.final = ctx.drop = ctx.seg = ctx.keep = ctx.pos_drop = None
        return (None, None, None, None, dfeats, None, None, None, *_cam_only(rt, flatten_params(gshared, gblocks)))
