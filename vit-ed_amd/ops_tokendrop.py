"""Functional wrapper of elementwise token dropout (csrc/token_dropout.hip), re-exported by ``ops``, and the
same mask rule restated in numpy integer arithmetic for CPU tensors and for the tests' oracle.

``token_dropout`` on CUDA tensors is an ``ops`` function in every respect - each tensor goes through ``ops._check`` before its pointer
reaches ``ops._lib.call``, the launch goes to torch's current stream, nothing synchronises - kept in a module of its own; everything
is looked up on ``ops`` at call time, so whatever replaces the library or the device gate there (tests/test_ops_args.py does) holds
here too.

The rule (csrc/token_dropout.h states it for the kernel): element e = (b T + t) D + d of a stream [batch, T, D], t the token's
original index, reads word e & 3 of Philox4x32-10 with the counter (lo32(e >> 2), hi32(e >> 2), stream, 0) and the key (lo32(seed),
hi32(seed)); it is kept iff word >= thr and then scaled by fp32(1 / (1 - p)), else set to 0."""
from __future__ import annotations

import numpy as np
import torch

from . import ops as _o

TOKEN_DROPOUT_MAX_DIM = 1024       # TD_MAX_DIM: the LayerNorm kernels' range
_f32, _bf16, _i32, _i64 = torch.float32, torch.bfloat16, torch.int32, torch.int64
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)


def dropout_threshold(p: float):
    """(thr, scale) of a drop probability p in [0, 1): an element is kept iff its 32-bit word >= thr = min(2^32 - 1, int(p 2^32)),
    and a kept one is multiplied by scale = fp32(1 / (1 - p)) - one division in double, rounded once."""
    p = float(p)
    if not 0. <= p < 1.:
        raise ValueError(f'dropout_threshold: p={p} is not a drop probability in [0, 1)')
    return min(2 ** 32 - 1, int(p * 4294967296.0)), float(np.float32(1.0 / (1.0 - p)))


def philox4x32(counter, key):
    """Philox4x32-10 of uint32 counters [..., 4] under the key (k0, k1): the uint32 outputs [..., 4], vectorised over the leading
    extents (uint64 arithmetic: a 32 x 32 bit product fits)."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) & _LO for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    m0, m1 = np.uint64(_M0), np.uint64(_M1)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def _seed_value(seed) -> int:
    """The seed as the uint64 the kernel reads: an int, or an int64 tensor of one element (any device: one host read)."""
    if torch.is_tensor(seed):
        if seed.dtype != _i64 or seed.numel() != 1:
            raise ValueError(f'token dropout: seed must be one int64, got {seed.dtype} {list(seed.shape)}')
        seed = int(seed.reshape(()).item())
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def _row_tokens(op, keep, lead, batch, tokens):
    """int64 [batch, rows]: the original token of every row - arange(tokens) without a table; with one the prefix token 0, then the
    kept patches' tokens (clamped as the kernels clamp them)."""
    if keep is None:
        return np.broadcast_to(np.arange(tokens, dtype=np.int64), (batch, tokens))
    k = np.asarray(keep.detach().cpu().numpy() if torch.is_tensor(keep) else keep).astype(np.int64)
    if k.ndim != 2 or k.shape[0] != batch or not 1 <= k.shape[1] < tokens:
        raise ValueError(f'{op}: keep {list(k.shape)} is not a table of 1 to {tokens - 1} kept tokens for each of {batch} samples')
    n = tokens if lead else tokens - 1                     # patches the indices range over (+ the leading patch 0 with lead)
    patch = np.clip(k + (1 if lead else 0), 0, n - 1)
    return np.concatenate([np.zeros((batch, 1), np.int64), patch if lead else patch + 1], axis=1)


def token_dropout_mask(seed, p, batch, tokens, dim, stream, keep=None, lead=False) -> torch.Tensor:
    """The bool keep mask [batch, rows, dim] of the rule (rows = tokens, or K + 1 under a keep table int [batch, K]), on the CPU."""
    op = 'token_dropout_mask'
    batch, tokens, dim, stream = int(batch), int(tokens), int(dim), int(stream)
    if batch < 1 or tokens < 1 or dim < 4 or dim % 4 or stream not in (0, 1):
        raise ValueError(f'{op}: batch {batch}, tokens {tokens}, dim {dim} (a multiple of 4), stream {stream} (0 or 1)')
    thr, _ = dropout_threshold(p)
    seed = _seed_value(seed)
    tok = _row_tokens(op, keep, lead, batch, tokens)                                        # [batch, rows]
    row = (np.arange(batch, dtype=np.int64)[:, None] * tokens + tok) * dim                  # element address of channel 0
    group = (row[:, :, None] >> 2) + np.arange(dim // 4, dtype=np.int64)                    # [batch, rows, dim / 4]: dim % 4 == 0
    g = group.astype(np.uint64)
    counter = np.stack([g & _LO, g >> np.uint64(32), np.full_like(g, stream), np.zeros_like(g)], axis=-1)
    words = philox4x32(counter, (seed & 0xFFFFFFFF, seed >> 32))
    return torch.from_numpy((words >= np.uint32(thr)).reshape(batch, tok.shape[1], dim))


def _strides(op, name, t):
    """(batch stride, row stride) of a [batch, rows, dim] operand as the entry wants them: those of a size-1 extent do not matter."""
    batch, rows, dim = t.shape
    bs, rs = t.stride(0), t.stride(1)
    if rows == 1:
        rs = dim
    if batch == 1:
        bs = (rows - 1) * rs + dim
    vec = 4 * t.element_size()
    if rs % 4 or bs % 4 or t.data_ptr() % vec:
        raise ValueError(f'{op}: {name} is moved {vec} bytes at a time: got stride {list(t.stride())} at offset {t.data_ptr() % vec} of '
                         f'a {vec}-byte line')
    return bs, rs


def token_dropout(x: torch.Tensor, seed, p: float, tokens: int, stream: int, keep=None, lead: bool = False, out=None) -> torch.Tensor:
    """x fp32 / bf16 [batch, rows, dim] (a dense last dim; any row / batch stride that keeps rows and samples apart) -> x with the
    rule's mask applied: kept elements times fp32(1 / (1 - p)), rounded once to x's dtype, dropped ones 0 (``vited_token_dropout``).
    ``seed``: one int64 on x's device, read by the kernel (an int also does for CPU tensors).  ``tokens``: the full token count T of
    the stream; ``keep`` int32 / int64 [batch, rows - 1] with ``lead`` as in ``tokens_kept``: the rows are the prefix token and the
    kept patches, each masked as its original token.  ``out``: a destination of x's shape and dtype, x itself for in place.
    On CPU tensors the same rule runs in numpy, bit for bit; it has no size limit."""
    op = 'token_dropout'
    thr, scale = dropout_threshold(p)
    tokens, stream = int(tokens), int(stream)
    if stream not in (0, 1):
        raise ValueError(f'{op}: stream {stream} is neither 0 (image 1) nor 1 (image 2)')
    if not torch.is_tensor(x) or not x.is_cuda:
        if not torch.is_tensor(x) or x.dim() != 3 or x.dtype not in (_f32, _bf16):
            raise ValueError(f'{op}: x must be a float32 / bfloat16 [batch, rows, dim] tensor')
        mask = token_dropout_mask(seed, p, x.shape[0], tokens, x.shape[2], stream, keep, lead)
        if mask.shape != x.shape:
            raise ValueError(f'{op}: x {list(x.shape)} does not hold the {mask.shape[1]} rows of {tokens} tokens' + (' under keep' if keep is not None else ''))
        y = torch.where(mask, (x.float() * torch.tensor(scale, dtype=_f32)).to(x.dtype), torch.zeros((), dtype=x.dtype))
        return y if out is None else out.copy_(y)
    _o._need_gpu(x, seed if torch.is_tensor(seed) else None, keep, out)
    dev = x.device
    _o._check(op, 'x', x, (_f32, _bf16), (_o._Min(1), _o._Min(1), _o._Min(4)), dev, _o.DENSE_LAST)
    batch, rows, dim = x.shape
    if dim % 4 or dim > TOKEN_DROPOUT_MAX_DIM:
        raise ValueError(f'{op}: dim {dim} is outside the kernel\'s range (multiples of 4 up to {TOKEN_DROPOUT_MAX_DIM})')
    _o._check(op, 'seed', seed, _i64, 1, dev, like='x')
    k = 0
    if keep is not None:
        _o._check(op, 'keep', keep, (_i32, _i64), (batch, rows - 1), dev, None, like='x')
        keep = keep.to(_i32).contiguous()
        k = keep.shape[1]
        if k < 1 or rows > tokens:
            raise ValueError(f'{op}: {rows} rows (a prefix and {k} kept tokens) do not fit a stream of {tokens} tokens')
    elif rows != tokens:
        raise ValueError(f'{op}: x has {rows} rows, the stream {tokens} tokens, and no keep table says which ones they are')
    out = x.new_empty(x.shape) if out is None else _o._check(op, 'out', out, x.dtype, tuple(x.shape), dev, _o.DENSE_LAST, like='x')
    x_bs, x_rs = _strides(op, 'x', x)
    o_bs, o_rs = _strides(op, 'out', out)
    _o._lib.call('vited_token_dropout', _o._ptr(x), x_bs, x_rs, _o._ptr(out), o_bs, o_rs, _o._code(x.dtype), batch, rows, dim, tokens, stream,
                 _o._ptr(keep), k, int(bool(lead)), _o._ptr(seed), thr, scale, _o._stream())
    return out
