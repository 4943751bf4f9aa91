"""Functional wrappers of the patch-dropout entry points (csrc/patch_keep.hip), re-exported by ``ops``.

They are ``ops`` functions in every respect - each tensor goes through ``ops._check`` before its pointer reaches ``ops._lib.call``, the
launch goes to torch's current stream, nothing synchronises - kept in a module of their own; everything is looked up on ``ops`` at
call time, so whatever replaces the library or the device gate there (tests/test_ops_args.py does) holds here too."""
from __future__ import annotations

import ctypes as C

import torch

from . import ops as _o

MAX_KEEP_KEYS = 4096       # PK_MAX_KEYS: keys per row the ranking kernel holds in LDS
_f32, _i32, _i64, _u8 = torch.float32, torch.int32, torch.int64, torch.uint8


def _keep_table(op, keep, dev, lead, n_patches, batch=None):
    """(keep int32 [B, K] as the kernels read it, K, lead) of a keep table given as int32 or int64: checked, never read."""
    _o._check(op, 'keep', keep, (_i32, _i64), (batch, None), dev, None)
    keep = keep.to(torch.int32).contiguous()
    k, lead = keep.shape[1], int(bool(lead))
    if k < 1 or k + lead > n_patches:
        raise ValueError(f'{op}: keep has {k} columns{" behind the leading patch" if lead else ""}, which do not fit {n_patches} patches')
    return keep, k, lead


def keep_from_keys(keys: torch.Tensor, k: int) -> torch.Tensor:
    """keys fp32 [B, L] -> int32 [B, k]: the indices of the k smallest keys of every row in ascending key order, equal keys by index:
    ``torch.argsort(keys, dim=-1, stable=True)[:, :k]`` without the sort (``vited_keep_from_keys``; L <= 4096)."""
    _o._need_gpu(keys)
    _o._check('keep_from_keys', 'keys', keys, _f32, (_o._Min(1), _o._Min(1)), keys.device)
    b, l = keys.shape
    k = int(k)
    if not 1 <= k <= l:
        raise ValueError(f'keep_from_keys: keys has {l} columns, of which {k} cannot be kept')
    if l > MAX_KEEP_KEYS:
        raise ValueError(f'keep_from_keys: keys has {l} columns, the kernel ranks at most {MAX_KEEP_KEYS}')
    keep = torch.empty((b, k), dtype=torch.int32, device=keys.device)
    _o._lib.call('vited_keep_from_keys', _o._ptr(keys), _o._ptr(keep), b, l, k, _o._stream())
    return keep


def patchify_kept(img: torch.Tensor, patch: int, dtype: torch.dtype, keep: torch.Tensor, lead: bool,
                  batch_index: torch.Tensor | None = None, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)) -> torch.Tensor:
    """``ops.patchify`` for the kept patches alone: [B * R, C*p*p] with R = K (+ 1 with ``lead``: patch 0, then the patches 1 + keep),
    row (b, r) bit-equal to ``patchify``'s row of that patch (``vited_patchify_kept`` / ``_u8``).  keep int32 / int64 [B, K], one row
    per OUTPUT sample (per pair under ``batch_index``)."""
    _o._need_gpu(img, batch_index, keep)
    op = 'patchify_kept'
    u8 = img.dtype == _u8
    if img.dtype in (torch.bfloat16, torch.float16):
        img = img.float()
    _o._check(op, 'img', img, (_u8, _f32), (None, None) + tuple(img.shape[2:3]) * 2, img.device, None)     # [B, C, S, S]
    if img.stride()[1:] != (img.shape[2] * img.shape[3], img.shape[3], 1):
        img = img.contiguous()
    b, c, s, _ = img.shape
    _o._check(op, 'batch_index', batch_index, _i64, None, img.device, optional=True)
    nb = b if batch_index is None else batch_index.numel()
    if patch < 1 or s % patch:
        raise ValueError(f'{op}: img is {s} x {s}, which {patch} x {patch} patches do not tile')
    g = s // patch
    keep, k, lead = _keep_table(op, keep, img.device, lead, g * g, nb)
    out = torch.empty((nb * (k + lead), c * patch * patch), dtype=dtype, device=img.device)
    if u8:
        mean, std = ([float(v) for v in list(t)[:c]] for t in (mean, std))
        _o._lib.call('vited_patchify_kept_u8', _o._ptr(img), img.stride(0), _o._ptr(batch_index), _o._ptr(keep), k, lead, _o._ptr(out),
                     _o._code(dtype), nb, c, s, patch, _o._host_array(C.c_float, mean, c), _o._host_array(C.c_float, std, c), _o._stream())
    else:
        _o._lib.call('vited_patchify_kept', _o._ptr(img), img.stride(0), _o._ptr(batch_index), _o._ptr(keep), k, lead, _o._ptr(out),
                     _o._code(dtype), nb, c, s, patch, _o._stream())
    return out


def tokens_kept(tok: torch.Tensor, pos: torch.Tensor, cls: torch.Tensor | None, keep: torch.Tensor, lead: bool) -> torch.Tensor:
    """tok fp32 [B * R, D] (patch-embedding product + bias of the kept rows), pos fp32 [1 + n, D] -> x fp32 [B, R (+ 1 with cls), D]:
    x[b, t] = tok[b, t] + pos[1 + patch(b, t)], behind the row cls + pos[0] when ``cls`` fp32 [D] is given (``vited_tokens_kept``)."""
    _o._need_gpu(tok, pos, cls, keep)
    op, dev = 'tokens_kept', tok.device
    _o._check(op, 'tok', tok, _f32, (None, None), dev)
    d = tok.shape[1]
    _o._check(op, 'pos', pos, _f32, (_o._Min(2), d), dev, like='tok')
    _o._check(op, 'cls', cls, _f32, (d,), dev, optional=True, like='tok')
    keep, k, lead = _keep_table(op, keep, dev, lead, pos.shape[0] - 1)
    b, r = keep.shape[0], k + lead
    _o._check(op, 'tok', tok, _f32, (b * r, d), dev, like='keep')
    if d % 4 or any(_o._ptr(t) % 16 for t in (tok, pos, cls)):
        raise ValueError(f'{op}: tok, pos and cls are read 16 bytes at a time: dim {d} must be a multiple of 4 and the pointers aligned')
    x = torch.empty((b, r + (cls is not None), d), dtype=torch.float32, device=dev)
    _o._lib.call('vited_tokens_kept', _o._ptr(tok), _o._ptr(pos), _o._ptr(cls), _o._ptr(keep), k, lead, _o._ptr(x), b, pos.shape[0] - 1, d,
                 _o._stream())
    return x


def keep_inverse(keep: torch.Tensor, lead: bool, n_patches: int) -> torch.Tensor:
    """int32 [B, n_patches]: the kept row of every patch, -1 where the sample dropped it (``vited_keep_inverse``)."""
    _o._need_gpu(keep)
    dev = keep.device if torch.is_tensor(keep) else None
    keep, k, lead = _keep_table('keep_inverse', keep, dev, lead, int(n_patches))
    inv = torch.empty((keep.shape[0], int(n_patches)), dtype=torch.int32, device=dev)
    _o._lib.call('vited_keep_inverse', _o._ptr(keep), k, lead, _o._ptr(inv), keep.shape[0], int(n_patches), _o._stream())
    return inv


def tokens_kept_bwd(dx: torch.Tensor, inv: torch.Tensor, with_cls: bool):
    """Backward of ``tokens_kept`` w.r.t. pos and cls: dx fp32 [B, rows, D], inv int32 [B, n] (``keep_inverse``) -> (dpos fp32 [1 + n, D],
    dcls fp32 [D] | None).  dpos[1 + p] sums dx over the samples that kept p in ascending sample order (exact zeros if nobody did);
    dpos[0] = dcls = the batch sum of row 0 with a cls row, zeros without.  No atomics: bitwise reproducible."""
    _o._need_gpu(dx, inv)
    op, dev = 'tokens_kept_bwd', dx.device
    _o._check(op, 'dx', dx, _f32, (None, None, None), dev)
    b, rows, d = dx.shape
    _o._check(op, 'inv', inv, _i32, (b, _o._Min(1)), dev, like='dx')
    n, first = inv.shape[1], int(bool(with_cls))
    if not first < rows <= n + first:
        raise ValueError(f'{op}: dx has {rows} rows per sample, which are not 1 to {n} kept patches{" behind a cls row" if first else ""}')
    if d % 4 or _o._ptr(dx) % 16:
        raise ValueError(f'{op}: dx is read 16 bytes at a time: dim {d} must be a multiple of 4 and the pointer aligned')
    dpos = torch.empty((n + 1, d), dtype=torch.float32, device=dev)
    dcls = torch.empty(d, dtype=torch.float32, device=dev) if first else None
    _o._lib.call('vited_tokens_kept_bwd', _o._ptr(dx), _o._ptr(inv), _o._ptr(dpos), _o._ptr(dcls), b, rows, first, n, d, _o._stream())
    return dpos, dcls
