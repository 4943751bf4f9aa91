"""Functional wrappers of the pooled-head entry points (csrc/pool_head.hip), re-exported by ``ops``.

They are ``ops`` functions in every respect - each tensor goes through ``ops._check`` before its pointer reaches ``ops._lib.call``, the
launch goes to torch's current stream, nothing synchronises - kept in a module of their own; everything is looked up on ``ops`` at
call time, so whatever replaces the library or the device gate there (tests/test_ops_args.py does) holds here too."""
from __future__ import annotations

import torch

from . import ops as _o

POOL_MAX_DIM = 1024        # 128 * POOL_MAX_VPL: the LayerNorm kernels' range
_f32, _bf16 = torch.float32, torch.bfloat16


def _tokens(op, name, t, dtype, dev, shape=None, like=None):
    """(item stride, token stride) of a [items, tokens, dim] operand whose rows are dense and whose rows and items lie apart."""
    t = _o._check(op, name, t, dtype, (None, None, None) if shape is None else shape, dev, _o.DENSE_LAST, like=like)
    items, tokens, dim = t.shape
    i_s, t_s = t.stride(0), t.stride(1)
    if tokens == 1:
        t_s = dim
    if items == 1:
        i_s = (tokens - 1) * t_s + dim
    if t_s < dim or i_s < (tokens - 1) * t_s + dim or t_s % 4 or i_s % 4 or t.data_ptr() % (16 if t.dtype == _f32 else 8):
        raise ValueError(f'{op}: {name} is moved 16 bytes at a time and its rows and items must lie apart: got {list(t.shape)} stride '
                         f'{list(t.stride())} at offset {t.data_ptr() % 16} of a 16-byte line')
    return i_s, t_s


def _shape(op, x, first):
    items, tokens, dim = x.shape
    first = int(first)
    if not 0 <= first < tokens or items < 1:
        raise ValueError(f'{op}: {items} items of {tokens} tokens leave nothing to pool behind a prefix of {first}')
    if dim % 4 or not 0 < dim <= POOL_MAX_DIM:
        raise ValueError(f'{op}: dim {dim} is outside the kernels\' range (multiples of 4 up to {POOL_MAX_DIM})')
    return items, tokens, dim, first


def _workspace(op, items, tokens, first, dim, dev, workspace):
    """(pointer, bytes) of the scratch the entry needs: ``ops``' grow-only buffer, or the caller's fp32 tensor, checked for size."""
    need = _o._lib.load().vited_token_pool_workspace_bytes(items, tokens, first, dim)
    if workspace is None:
        return _o._scratch(need, dev, 16)
    _o._check(op, 'workspace', workspace, _f32, _o._Min((need + 3) // 4), dev)
    if workspace.data_ptr() % 16:
        raise ValueError(f'{op}: workspace must be 16-byte aligned')
    return workspace.data_ptr(), workspace.numel() * 4


def token_pool_fwd(x: torch.Tensor, first: int = 1, gamma=None, beta=None, eps: float = 1e-6, save_stats: bool = False, out=None,
                   workspace=None):
    """x fp32 [items, tokens, dim] (a dense last dim; any item / token stride that keeps rows and items apart) -> (pooled fp32 [items,
    dim], mean | None, rstd | None): pooled[b] = mean over t >= first of x[b, t], or with ``gamma`` / ``beta`` (fp32 [dim]) of
    LayerNorm(x[b, t]; gamma, beta, eps), whose rows are never written (``vited_token_pool_fwd``).  ``save_stats`` (with gamma): also
    the rows' statistics, fp32 [items * tokens], for ``token_pool_bwd``; the prefix rows' entries are left as allocated.  ``out``: a
    pre-made pooled (row-strided ok).  One summation order fixed by the shape: two runs give the same bits."""
    _o._need_gpu(x, gamma, beta, out, workspace)
    op, dev = 'token_pool_fwd', x.device
    x_is, x_ts = _tokens(op, 'x', x, _f32, dev)
    items, tokens, dim, first = _shape(op, x, first)
    if (gamma is None) != (beta is None):
        raise ValueError(f'{op}: gamma and beta go together')
    _o._check(op, 'gamma', gamma, _f32, (dim,), dev, optional=True, like='x')
    _o._check(op, 'beta', beta, _f32, (dim,), dev, optional=True, like='x')
    pooled = _o._out(op, 'out (pooled)', out, _f32, (items, dim), dev, _o.DENSE_LAST)
    if pooled.data_ptr() % 16 or (items > 1 and pooled.stride(0) % 4):
        raise ValueError(f'{op}: out (pooled) is written 16 bytes at a time: pointer and row stride must be aligned')
    mean = rstd = None
    if save_stats:
        if gamma is None:
            raise ValueError(f'{op}: save_stats goes with gamma / beta: the plain mean has no row statistics')
        mean = torch.empty(items * tokens, dtype=_f32, device=dev)
        rstd = torch.empty(items * tokens, dtype=_f32, device=dev)
    ws = _workspace(op, items, tokens, first, dim, dev, workspace)
    _o._lib.call('vited_token_pool_fwd', _o._ptr(x), x_is, x_ts, _o._ptr(gamma), _o._ptr(beta), float(eps), _o._ptr(pooled),
                 pooled.stride(0) if items > 1 else dim, _o._ptr(mean), _o._ptr(rstd), items, tokens, first, dim, *ws, _o._stream())
    return pooled, mean, rstd


def token_pool_bwd(g: torch.Tensor, tokens: int, first: int = 1, x=None, gamma=None, mean=None, rstd=None, dx=None, lp_dtype=None,
                   dx_lp=None, lp_scale=None, dgamma=None, dbeta=None, workspace=None):
    """Backward of ``token_pool_fwd`` given g fp32 [items, dim]: returns (dx fp32 [items, tokens, dim], dx_lp | None, dgamma | None,
    dbeta | None).  Every element of dx is written once (``vited_token_pool_bwd``): zero rows in front of ``first``, g[b] / (tokens -
    first) behind it, or with ``gamma`` the LayerNorm backward of that row gradient from ``x`` and the saved ``mean`` / ``rstd``.
    ``lp_dtype`` (bf16 / fp32) or a pre-made ``dx_lp``: the copy lp_dtype(lp_scale[b] * dx[b]) from the same pass; ``lp_scale`` fp32
    [items] optional.  ``dx`` / ``dx_lp`` may be pre-made strided destinations.  With gamma the column sums are returned, or ADDED onto
    ``dgamma`` / ``dbeta`` when those are given."""
    _o._need_gpu(g, x, gamma, mean, rstd, dx, dx_lp, lp_scale, dgamma, dbeta, workspace)
    op, dev = 'token_pool_bwd', g.device
    _o._check(op, 'g', g, _f32, (None, None), dev, _o.DENSE_LAST)
    items, dim = g.shape
    tokens = int(tokens)
    if g.data_ptr() % 16 or (items > 1 and g.stride(0) % 4):
        raise ValueError(f'{op}: g is read 16 bytes at a time: pointer and row stride must be aligned')
    shape = (items, tokens, dim)
    if dx is None:
        dx = torch.empty(shape, dtype=_f32, device=dev)
    dx_is, dx_ts = _tokens(op, 'dx', dx, _f32, dev, shape, like='g')
    items, tokens, dim, first = _shape(op, dx, first)
    lp_is = lp_ts = 0
    if dx_lp is None and lp_dtype is not None:
        dx_lp = torch.empty(shape, dtype=lp_dtype, device=dev)
    if dx_lp is not None:
        lp_is, lp_ts = _tokens(op, 'dx_lp', dx_lp, (_f32, _bf16) if lp_dtype is None else lp_dtype, dev, shape, like='g')
    if lp_scale is not None and dx_lp is None:
        raise ValueError(f'{op}: lp_scale scales the low-precision copy: give lp_dtype or dx_lp')
    _o._check(op, 'lp_scale', lp_scale, _f32, (items,), dev, optional=True, like='g')
    x_is = x_ts = accumulate = 0
    ws = (0, 0)
    if gamma is not None:
        _o._check(op, 'gamma', gamma, _f32, (dim,), dev, like='g')
        x_is, x_ts = _tokens(op, 'x', x, _f32, dev, shape, like='g')
        _o._check(op, 'mean', mean, _f32, items * tokens, dev, like='x')
        _o._check(op, 'rstd', rstd, _f32, items * tokens, dev, like='x')
        accumulate, dgamma, dbeta = _o._ln_grads(op, dev, dim, dgamma, dbeta)
        ws = _workspace(op, items, tokens, first, dim, dev, workspace)
    elif any(t is not None for t in (mean, rstd, dgamma, dbeta)):
        raise ValueError(f'{op}: mean, rstd, dgamma and dbeta go with gamma')
    else:
        x = None
    _o._lib.call('vited_token_pool_bwd', _o._ptr(g), g.stride(0) if items > 1 else dim, _o._ptr(x), x_is, x_ts, _o._ptr(gamma), _o._ptr(mean),
                 _o._ptr(rstd), _o._ptr(dx), dx_is, dx_ts, _o._ptr(dx_lp), _o._code(dx_lp.dtype) if dx_lp is not None else 0, lp_is, lp_ts,
                 _o._ptr(lp_scale), _o._ptr(dgamma), _o._ptr(dbeta), int(accumulate), items, tokens, first, dim, *ws, _o._stream())
    return dx, dx_lp, dgamma, dbeta
