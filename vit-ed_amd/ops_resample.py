"""Functional wrapper of the Pillow-exact resize on the device (csrc/resample_u8.hip), re-exported by ``ops``, and
the same rule restated in numpy for CPU tensors and for the tests' oracle.

``resample_u8`` on CUDA tensors is an ``ops`` function in every respect - each tensor goes through ``ops._check`` before its pointer
reaches ``ops._lib.call``, the launch goes to torch's current stream, nothing synchronises - kept in a module of its own; everything
is looked up on ``ops`` at call time, so whatever replaces the library or the device gate there (tests/test_ops_args.py does) holds
here too.

The rule is Pillow's ``Image.resize((Rw, Rh), Image.BILINEAR)`` for 8-bit images (ImagingResample: precompute_coeffs,
normalize_coeffs_8bpc, the horizontal pass into a uint8 intermediate, then the vertical pass), at any scale: the bilinear filter's
support grows with the scale where the image shrinks, which antialiases it."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

from . import ops as _o

RESAMPLE_MAX_OUT = 1024            # RS_MAX_OUT: PUZZLE_MAX_SIZE
RESAMPLE_MAX_RATIO = 8             # RS_MAX_RATIO: in_len / out_len
RESAMPLE_MAX_TAPS = 17             # RS_MAX_TAPS
_BITS = 22                         # PRECISION_BITS = 32 - 8 - 2
_u8, _i32, _i64 = torch.uint8, torch.int32, torch.int64


def resample_ksize(in_len: int, out_len: int) -> int:
    """Taps per output pixel: ceil(max(in_len / out_len, 1)) * 2 + 1."""
    return int(math.ceil(max(float(in_len) / float(out_len), 1.0))) * 2 + 1


def resample_taps(in_len: int, out_len: int):
    """Pillow's coefficients of one axis, ``in_len`` pixels resized to ``out_len`` with the bilinear filter: (first int32 [out_len],
    count int32 [out_len], weights int32 [out_len, ksize]) - output pixel o is clip8((2^21 + sum_j pixel[first[o] + j] weights[o, j])
    >> 22) over j < count[o]; the weights behind count are 0.  Double arithmetic, every product and sum rounded on its own."""
    in_len, out_len = int(in_len), int(out_len)
    if in_len < 1 or out_len < 1:
        raise ValueError(f'resample_taps: cannot resize {in_len} pixels to {out_len}')
    scale = np.float64(in_len) / np.float64(out_len)
    fs = max(scale, np.float64(1.0))
    support = np.float64(1.0) * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = np.float64(1.0) / fs
    center = (np.arange(out_len, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5), 0.0)
    xmax = np.minimum(np.trunc(center + support + 0.5), float(in_len)) - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    a = np.abs(((x + xmin[:, None]) - center[:, None] + 0.5) * ss)
    w = np.where((a < 1.0) & (x < xmax[:, None]), 1.0 - a, 0.0)
    ww = np.zeros(out_len, dtype=np.float64)
    for j in range(ksize):                                   # accumulated in order, as the C loop does
        ww = np.where(j < xmax, ww + w[:, j], ww)
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    k = np.where(w < 0.0, np.trunc(-0.5 + w * float(1 << _BITS)), np.trunc(0.5 + w * float(1 << _BITS)))
    return xmin.astype(np.int32), xmax.astype(np.int32), k.astype(np.int32)


def _pass(img: np.ndarray, taps, axis: int) -> np.ndarray:
    """One pass of the rule along ``axis`` (0 or 1) of uint8 [H, W, C]."""
    first, count, k = taps
    n = img.shape[axis]
    idx = np.minimum(first[:, None].astype(np.int64) + np.arange(k.shape[1]), n - 1)              # behind count the weight is 0
    src = np.moveaxis(img, axis, 0).astype(np.int64)                                               # [n, other, C]
    acc = np.zeros((first.shape[0],) + src.shape[1:], dtype=np.int64)
    for j in range(k.shape[1]):
        acc += src[idx[:, j]] * k[:, j].astype(np.int64)[:, None, None]
    out = np.clip((acc + (1 << (_BITS - 1))) >> _BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resample_image(img, Rh: int, Rw: int) -> np.ndarray:
    """``Image.fromarray(img).resize((Rw, Rh), Image.BILINEAR)`` of a uint8 [H, W, C] array in numpy integer arithmetic: the
    horizontal pass first, a uint8 intermediate, then the vertical pass."""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3:
        raise ValueError(f'resample_image: expected a uint8 [H, W, C] array, got {img.dtype} {img.shape}')
    return _pass(_pass(img, resample_taps(img.shape[1], Rw), 1), resample_taps(img.shape[0], Rh), 0)


def window_image(img: np.ndarray, top: int, left: int, h: int, w: int, fill: int) -> np.ndarray:
    """The window (top, left, h, w) of uint8 [H, W, C] in image coordinates; whatever lies outside the image is ``fill``."""
    H, W = img.shape[:2]
    out = np.full((h, w, img.shape[2]), fill, dtype=np.uint8)
    y0, y1, x0, x1 = max(top, 0), min(top + h, H), max(left, 0), min(left + w, W)
    if y0 < y1 and x0 < x1:
        out[y0 - top: y1 - top, x0 - left: x1 - left] = img[y0:y1, x0:x1]
    return out


class ResampleTables(NamedTuple):
    """The tap tables of one axis for every window length a caller resizes to ``out_len`` (``resample_tables``)."""
    table: torch.Tensor          # int32 [classes, out_len, 2 + ksize]: first tap, count, weights (zeros behind count)
    lengths: torch.Tensor        # int32 [classes], ascending: the window length of each class, on the table's device
    ksize: int
    max_len: int
    out_len: int


def resample_tables(in_lens, out_len: int, device) -> ResampleTables:
    """``resample_taps`` of every distinct length in ``in_lens`` -> ``out_len``, computed once in fp64 on the host and copied to
    ``device``.  A length the kernel cannot take (out_len above 1024, a ratio above 8) is refused here, by name."""
    out_len = int(out_len)
    lens = sorted({int(v) for v in in_lens})
    if not lens or lens[0] < 1 or out_len < 1:
        raise ValueError(f'resample_tables: window lengths {lens[:4]} -> {out_len}: every length must be positive')
    if out_len > RESAMPLE_MAX_OUT or lens[-1] > RESAMPLE_MAX_RATIO * out_len:
        raise ValueError(f'resample_tables: {lens[-1]} -> {out_len} pixels is outside the kernel\'s range (outputs up to {RESAMPLE_MAX_OUT}, '
                         f'shrinking up to {RESAMPLE_MAX_RATIO}x)')
    ks = resample_ksize(lens[-1], out_len)
    tab = np.zeros((len(lens), out_len, 2 + ks), dtype=np.int32)
    for c, n in enumerate(lens):
        first, count, k = resample_taps(n, out_len)
        tab[c, :, 0], tab[c, :, 1], tab[c, :, 2: 2 + k.shape[1]] = first, count, k
    return ResampleTables(torch.from_numpy(tab).to(device), torch.tensor(lens, dtype=_i32, device=device), ks, lens[-1], out_len)


def _classes(tables: ResampleTables, lengths: torch.Tensor) -> torch.Tensor:
    """int32 [n]: the class of each window length (a length the tables do not hold gets the next larger one's, clamped)."""
    return torch.searchsorted(tables.lengths, lengths.to(_i32).contiguous()).clamp_(max=tables.lengths.numel() - 1).to(_i32)


def _resample_cpu(op, store, img_off, img_hw, image, windows, fill, Rh, Rw, crop_top, crop_left, S, out):
    data, off, hw = store.numpy(), img_off.numpy(), img_hw.numpy()
    n = image.numel()
    res = np.empty((n, 3, S, S), dtype=np.uint8)
    for b, idx in enumerate(np.clip(image.numpy().astype(np.int64), 0, len(off) - 1)):
        H, W = int(hw[idx, 0]), int(hw[idx, 1])
        img = data[off[idx]: off[idx] + H * W * 3].reshape(H, W, 3)
        if windows is not None:
            top, left, h, w = (int(v) for v in windows[b])
            img = window_image(img, top, left, h, w, fill)
        r = resample_image(img, Rh, Rw)[crop_top: crop_top + S, crop_left: crop_left + S]
        res[b] = r.transpose(2, 0, 1)
    res = torch.from_numpy(res)
    return res if out is None else out.copy_(res)


def resample_u8(store: torch.Tensor, img_off: torch.Tensor, img_hw: torch.Tensor, image: torch.Tensor, windows, fill: int,
                xtables, ytables, Rh: int, Rw: int, crop_top: int, crop_left: int, img_size: int, out=None) -> torch.Tensor:
    """Resident images -> uint8 [n, 3, S, S] (``vited_resample_u8``): per sample the window ``windows`` int32 [n, 4] = (top, left, h, w)
    of image ``image`` int32 [n] (None: the whole image; outside the image a window reads ``fill``) is resized to Rh x Rw as Pillow's
    ``Image.resize(..., BILINEAR)`` does, and the S x S crop at (crop_top, crop_left) of that is the output.  store / img_off / img_hw
    as for ``div2k_regions_u8``.  ``xtables`` / ``ytables``: ``resample_tables`` of the window widths -> Rw and heights -> Rh; every
    window's length must be among theirs (the class of each sample is looked up on the device).  ``out``: a destination uint8
    [n, 3, S, S] with dense samples and any batch stride, ``pairs[:, 1]`` of a [B, 2, 3, S, S] tensor for one.
    On CPU tensors the same rule runs in numpy, bit for bit; it needs no tables and has no size limit."""
    op = 'resample_u8'
    S, Rh, Rw, crop_top, crop_left, fill = int(img_size), int(Rh), int(Rw), int(crop_top), int(crop_left), int(fill)
    if not 0 <= fill <= 255:
        raise ValueError(f'{op}: fill {fill} is not a uint8')
    if S < 1 or crop_top < 0 or crop_left < 0 or crop_top + S > Rh or crop_left + S > Rw:
        raise ValueError(f'{op}: the {S} x {S} crop at ({crop_top}, {crop_left}) leaves the resized image of {Rh} x {Rw}')
    if not torch.is_tensor(store) or not store.is_cuda:
        dev = torch.device('cpu')
        n = _o._store_args(op, store, img_off, img_hw)
        _o._check(op, 'image', image, (_i32, _i64), (None,), dev)
        _o._check(op, 'windows', windows, _i32, (image.numel(), 4), dev, optional=True)
        _o._check(op, 'out', out, _u8, (image.numel(), 3, S, S), dev, None, optional=True)
        return _resample_cpu(op, store, img_off, img_hw, image, windows, fill, Rh, Rw, crop_top, crop_left, S, out)
    _o._need_gpu(store, img_off, img_hw, image, windows, out)
    dev = store.device
    n_images, n = _o._store_args(op, store, img_off, img_hw), image.numel()
    _o._check(op, 'image', image, _i32, (n,), dev)
    _o._check(op, 'windows', windows, _i32, (n, 4), dev, optional=True)
    for name, t, R in (('xtables', xtables, Rw), ('ytables', ytables, Rh)):
        if not isinstance(t, ResampleTables) or t.out_len != R:
            raise ValueError(f'{op}: {name} must be the resample_tables of the window lengths -> {R}')
        _o._check(op, f'{name}.table', t.table, _i32, (t.lengths.numel(), R, 2 + t.ksize), dev)
        _o._check(op, f'{name}.lengths', t.lengths, _i32, (None,), dev)
    if windows is None:
        hw = img_hw[image.long().clamp_(0, n_images - 1)]
        heights, widths = hw[:, 0], hw[:, 1]
    else:
        heights, widths = windows[:, 2], windows[:, 3]
    xcls, ycls = _classes(xtables, widths), _classes(ytables, heights)
    out = _o._out(op, 'out', out, _u8, (n, 3, S, S), dev, _o.DENSE_ITEMS)
    out_bs = out.stride(0) if n > 1 else 3 * S * S
    if n > 1 and out_bs < 3 * S * S:
        raise ValueError(f'{op}: out has the batch stride {out_bs}: its samples of {3 * S * S} bytes would overlap')
    _o._lib.call('vited_resample_u8', _o._ptr(store), _o._ptr(img_off), _o._ptr(img_hw), n_images, _o._ptr(image), _o._ptr(windows), fill,
                 _o._ptr(xtables.table), _o._ptr(xcls), xtables.lengths.numel(), xtables.ksize, _o._ptr(ytables.table), _o._ptr(ycls),
                 ytables.lengths.numel(), ytables.ksize, ytables.max_len, xtables.max_len, Rh, Rw, crop_top, crop_left, S, _o._ptr(out),
                 out_bs, n, _o._stream())
    return out
