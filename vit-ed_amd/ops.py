"""Functional wrappers over the C ABI: one Python function per entry point of include/vited.h.

These allocate outputs (PyTorch owns every buffer), pass every tensor through ``_check`` (dtype, extent,
strides, device: ValueError BEFORE the launch) and raise on any non-zero status.  They are not autograd-aware; ``functions.py`` composes
them into the encoder / decoder autograd Functions.  Every op launches on torch's current HIP
stream, never synchronises and never allocates on the device side, so the whole forward+backward
is hipGraph-capturable.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import NamedTuple

import torch

from . import _lib
from ._lib import (B_KN, B_NK, BF16, EPI_GELU, EPI_GELU_GRAD, EPI_MUL, EPI_MUL_GELU_GRAD, EPI_RESIDUAL, EPI_STORE, EPI_STORE_F32, F16,
                   F32, I32, I64)

_DTYPE = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16, torch.int32: I32, torch.int64: I64}
_FLOATS = (torch.float32, torch.bfloat16, torch.float16)       # what the ranking and pair-score entries take
_ACT = (torch.float32, torch.bfloat16)                         # activations: what _code takes


def _code(dtype: torch.dtype) -> int:
    """dtype code of an activation (fp32 or bf16)."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f'vited ops support float32 and bfloat16 activations, got {dtype}')
    return _DTYPE[dtype]


def _need_gpu(*tensors, error=RuntimeError):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise error('vited ops run on the MI355X HIP kernels only: got a CPU tensor '
                        '(there is no CPU fallback; the fp32 CPU oracle lives in oracle/ for tests)')


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _host_array(ctype, values, length=None):
    """ctypes array of ``values`` (zero-filled up to ``length``) for an entry that reads a host array; a ``c_void_p`` array takes
    tensors, ``None`` being null."""
    values = list(values)
    if ctype is C.c_void_p:
        values = [_ptr(t) or None for t in values]
    return (ctype * (len(values) if length is None else length))(*values)


# ---- the one argument check: every tensor whose pointer reaches _lib.call goes through _check first ------------------------------
_f32, _bf16, _i32, _i64, _u8, _f64 = torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.uint8, torch.float64
CONTIGUOUS = 'contiguous'              # the stride assumptions an entry point can make of a buffer
DENSE_LAST = 'dense last dim'          # [..., rows, width]: unit column stride, any row / item stride that keeps them apart
DENSE_ITEMS = 'dense items'            # [B, ...]: every item contiguous, any batch stride
_ANY2, _ANY3 = (None, None), (None, None, None)      # any 2-D / 3-D extent: recognised by identity, no walk over the sizes


class _Min(int):
    """An extent of ``_check``: at least this many."""


def _check(op, name, t, dtype, shape, dev, strides=CONTIGUOUS, optional=False, like=None, ld=None):
    """Raise ValueError unless ``t`` is a tensor of ``dtype`` (one, a tuple of them, or None: any) on ``dev`` with the extent ``shape``
    and the stride assumption ``strides`` (None: the caller copies it dense itself); returns ``t``.  ``shape`` is a tuple of sizes
    (None: any, ``_Min(n)``: at least n), an element count for a buffer of any rank (an int or a ``_Min``), or None.  ``ld``: the row
    stride it must have.  None passes only where ``optional``.  ``like`` names the operand the expectation was taken from.  An
    activation (``_ACT``) of another dtype is a TypeError, as from ``_code``.  Host work only: metadata, never device memory."""
    if t is None and optional:
        return None
    try:
        ok = t.device == dev and (dtype is None or t.dtype == dtype or (type(dtype) is tuple and t.dtype in dtype))
    except AttributeError:                         # None, or not a tensor
        ok = False
    if ok:
        sizes = t.shape
        if isinstance(shape, tuple):
            if sizes != shape:                     # unequal: a wildcard, or a wrong extent
                ok = len(sizes) == len(shape)
                for s, e in zip(sizes, shape) if ok and shape is not _ANY2 and shape is not _ANY3 else ():
                    if e is not None and (s < e if type(e) is _Min else s != e):
                        ok = False
        elif shape is not None:
            ok = t.numel() >= shape if type(shape) is _Min else t.numel() == shape
    if ok:
        if strides is CONTIGUOUS:
            ok = t.is_contiguous()
        elif strides is DENSE_LAST:
            if ld is not None or not sizes or not t.is_contiguous():          # a contiguous tensor has dense, disjoint rows
                st, n = t.stride(), len(sizes)
                ok = n >= 1 and (sizes[-1] <= 1 or st[-1] == 1) and (
                    n < 2 or sizes[-2] <= 1 or (st[-2] >= sizes[-1] if ld is None else st[-2] == ld)) and (
                    n < 3 or sizes[-3] <= 1 or st[-3] >= sizes[-2] * st[-2])          # nor do the [rows, width] items overlap
        elif strides is DENSE_ITEMS:
            want = 1
            for size, stride in zip(reversed(sizes[1:]), reversed(t.stride()[1:])):
                ok = ok and (size <= 1 or stride == want)
                want *= size
    if ok:
        return t
    if isinstance(shape, tuple):
        want = ['*' if e is None else f'>={int(e)}' if type(e) is _Min else str(e) for e in shape]
        extent = f'vector of length {want[0]}' if len(want) == 1 else '[' + ', '.join(want) + ']'
    else:
        extent = 'tensor' if shape is None else f'buffer of {">=" if type(shape) is _Min else ""}{int(shape)} elements'
    dtypes = 'any dtype' if dtype is None else ' / '.join(str(d).replace('torch.', '') for d in (dtype if type(dtype) is tuple else (dtype,)))
    want = f'{strides or "strided"} {dtypes} {extent}{f" with row stride {ld}" if ld is not None else ""} on {dev}'
    got = f'{t.dtype} {list(t.shape)} stride {list(t.stride())} on {t.device}' if torch.is_tensor(t) else type(t).__name__
    error = TypeError if dtype is _ACT and torch.is_tensor(t) and t.dtype not in _ACT else ValueError
    raise error(f'{op}: {name} {f"does not match {like}: it " if like else ""}must be a {want}, got {got}')


def _out(op, name, t, dtype, shape, dev, strides=CONTIGUOUS):
    """The ``out=None`` pattern: a fresh ``dtype`` tensor of ``shape`` (a vector where it is an element count), or the given one checked."""
    return torch.empty(shape, dtype=dtype, device=dev) if t is None else _check(op, name, t, dtype, shape, dev, strides)


def _rows(op, name, t, dtype, dev, cols=None, rows=None, like=None):
    """Row stride of a [rows, cols] operand with a dense last dim, checked."""
    return _check(op, name, t, dtype, _ANY2 if cols is rows is None else (rows, cols), dev, DENSE_LAST, like=like).stride(0)


def _head_dim(op, name, d, heads):
    if heads <= 0 or d % heads:
        raise ValueError(f'{op}: {name} has {d} columns, which are not {heads} heads')
    return d // heads


def _head_operand(op, name, t, dtype, shape, dev, optional=False, like=None):
    """Strides in front of the dense last dim of a q / k / v-like operand [..., heads * head_dim] - a column slice of a packed
    projection: (row stride,) of [rows, D], (batch stride, token stride) of [B, N, D]; zeros for an absent optional one."""
    if t is None and optional:
        return (0,) * (len(shape) - 1)
    return _check(op, name, t, dtype, shape, dev, DENSE_LAST, like=like).stride()[:-1]


_ws_cache = {}
_ws_pinned = False
_ws_retired = []


def pin_workspace():
    """Called when a hipGraph has been captured: its kernels baked the workspace address in, so a later (eager) growth
    must not free that buffer - it is retired (kept alive) and a larger one serves the eager calls."""
    global _ws_pinned
    _ws_pinned = True


def workspace(nbytes: int, device) -> torch.Tensor:
    """Grow-only scratch buffer per device (fp32 elements).  Contents never outlive one op."""
    key = (device.type, device.index)
    buf = _ws_cache.get(key)
    n = (int(nbytes) + 3) // 4
    if buf is None or buf.numel() < n:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('vited workspace must be sized before graph capture: run one eager step first')
        if buf is not None and _ws_pinned:
            _ws_retired.append(buf)
        buf = torch.empty(max(n, 1 << 20), dtype=torch.float32, device=device)
        _ws_cache[key] = buf
    return buf


def _scratch(nbytes: int, device, align: int = 1):
    """(pointer, size in bytes) of ``workspace(nbytes, device)``; with ``align``, of one that many bytes larger, the pointer rounded up."""
    ws = workspace(nbytes + (align if align > 1 else 0), device)
    base = -(-ws.data_ptr() // align) * align
    return base, ws.numel() * 4 - (base - ws.data_ptr())


# ---------------------------------------------------------------------------------------------
def cast(src: torch.Tensor, dtype: torch.dtype, out: torch.Tensor | None = None) -> torch.Tensor:
    _need_gpu(src, out)
    src = _check('cast', 'src', src, _ACT, None, src.device, None).contiguous()
    out = torch.empty_like(src, dtype=dtype) if out is None else _check('cast', 'out', out, dtype, src.numel(), src.device)
    _lib.call('vited_cast', _ptr(src), _code(src.dtype), _ptr(out), _code(dtype), src.numel(), _stream())
    return out


def scale_rows_cast(src: torch.Tensor, row_scale: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """dst[r, :] = dtype(row_scale[r] * src[r, :]) for fp32 ``src`` [rows, dim] (``vited_scale_rows_cast``)."""
    _need_gpu(src, row_scale)
    ld = _rows('scale_rows_cast', 'src', src, _f32, src.device)
    rows, dim = src.shape
    _check('scale_rows_cast', 'row_scale', row_scale, _f32, (rows,), src.device)
    out = torch.empty((rows, dim), dtype=dtype, device=src.device)
    _lib.call('vited_scale_rows_cast', _ptr(src), ld, _ptr(row_scale), _ptr(out), _code(dtype), dim, rows, dim, _stream())
    return out


def cast_transpose(w: torch.Tensor, dtype: torch.dtype, out: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 [R, C] -> dtype [C, R] (transposed weight shadow)."""
    _need_gpu(w, out)
    _check('cast_transpose', 'w', w, _f32, _ANY2, w.device)
    out = _out('cast_transpose', 'out', out, dtype, (w.shape[1], w.shape[0]), w.device)
    _lib.call('vited_cast_transpose', _ptr(w), _ptr(out), _code(dtype), w.shape[0], w.shape[1], _stream())
    return out


class WeightShadowPlan:
    """Device descriptor table for ``vited_cast_weights``: built once per set of (weight, shadow, transposed
    shadow) buffers, then every refresh is one launch."""

    def __init__(self, entries):
        """entries: iterable of (w fp32 [rows, cols] contiguous, dst bf16 [rows, cols] | None, dst_t bf16 [cols, rows] | None)."""
        rows_, keep, tile = [], [], 0
        for i, (w, dst, dst_t) in enumerate(entries):
            _need_gpu(w, dst, dst_t)
            _check('WeightShadowPlan', f'entries[{i}] w', w, _f32, _ANY2, w.device)
            r, c = w.shape
            _check('WeightShadowPlan', f'entries[{i}] dst', dst, _bf16, (r, c), w.device, optional=True)
            _check('WeightShadowPlan', f'entries[{i}] dst_t', dst_t, _bf16, (c, r), w.device, optional=True)
            if any(_ptr(t) % 16 for t in (w, dst, dst_t)):
                raise ValueError(f'WeightShadowPlan: entries[{i}] w, dst and dst_t must be 16-byte aligned')
            if dst is None and dst_t is None:
                continue
            rows_.append([w.data_ptr(), _ptr(dst), _ptr(dst_t), r, c, tile])
            tile += ((r + 63) // 64) * ((c + 63) // 64)
            keep.append((w, dst, dst_t))
        self.count, self.total_tiles, self._keep = len(rows_), tile, keep
        self.key = tuple(tuple(r[:3]) for r in rows_)
        self.table = torch.tensor(rows_, dtype=torch.int64).to(keep[0][0].device) if rows_ else None

    def run(self):
        if self.count:
            _lib.call('vited_cast_weights', _ptr(self.table), self.count, self.total_tiles, _stream())


def patchify(img: torch.Tensor, patch: int, dtype: torch.dtype, batch_index: torch.Tensor | None = None,
             mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)) -> torch.Tensor:
    """img fp32 [B, C, S, S] (any batch stride, dense [C, S, S]) -> [B * (S/p)^2, C*p*p].  uint8 images are normalised on the
    fly: (pixel / 255 - mean[c]) / std[c] (``vited_patchify_u8``)."""
    _need_gpu(img, batch_index)
    u8 = img.dtype == torch.uint8
    if not u8 and img.dtype != torch.float32:
        img = img.float()
    if img.dim() == 4 and img.stride()[1:] != (img.shape[2] * img.shape[3], img.shape[3], 1):
        img = img.contiguous()
    _check('patchify', 'img', img, (_u8, _f32), (None, None) + tuple(img.shape[2:3]) * 2, img.device, DENSE_ITEMS)     # [B, C, S, S]
    b, c, s, _ = img.shape
    _check('patchify', 'batch_index', batch_index, _i64, None, img.device, optional=True)
    nb = b if batch_index is None else batch_index.numel()
    if patch < 1 or s % patch:
        raise ValueError(f'patchify: img is {s} x {s}, which {patch} x {patch} patches do not tile')
    g = s // patch
    out = torch.empty((nb * g * g, c * patch * patch), dtype=dtype, device=img.device)
    if u8:
        mean, std = ([float(v) for v in list(t)[:c]] for t in (mean, std))
        _lib.call('vited_patchify_u8', _ptr(img), img.stride(0), _ptr(batch_index), _ptr(out), _code(dtype), nb, c, s, patch,
                  _host_array(C.c_float, mean, c), _host_array(C.c_float, std, c), _stream())
    else:
        _lib.call('vited_patchify', _ptr(img), img.stride(0), _ptr(batch_index), _ptr(out), _code(dtype), nb, c, s, patch, _stream())
    return out


def crop_pairs_u8(regions: torch.Tensor, cells: torch.Tensor, erode: torch.Tensor, img_size: int) -> torch.Tensor:
    """regions uint8 [B, C, 2 S, 3 S] (any batch stride), cells int32 [B, 2], erode int32 [B] -> uint8 [B, 2, C, S, S]: the pair
    of eroded grid cells resized back to S x S (``vited_crop_pairs_u8``; div2k_patch.py:108-121,155-162)."""
    _need_gpu(regions, cells, erode)
    s, dev = int(img_size), regions.device
    if regions.dim() == 4 and regions.stride()[1:] != (6 * s * s, 3 * s, 1):
        regions = regions.contiguous()
    _check('crop_pairs_u8', 'regions', regions, _u8, (None, None, 2 * s, 3 * s), dev, DENSE_ITEMS)
    b, c = regions.shape[:2]
    _check('crop_pairs_u8', 'cells', cells, _i32, (b, 2), dev)
    _check('crop_pairs_u8', 'erode', erode, _i32, (b,), dev)
    out = torch.empty((b, 2, c, s, s), dtype=torch.uint8, device=regions.device)
    _lib.call('vited_crop_pairs_u8', _ptr(regions), regions.stride(0), _ptr(cells), _ptr(erode), _ptr(out), b, c, s, _stream())
    return out


def _store_args(op, store: torch.Tensor, img_off: torch.Tensor, img_hw: torch.Tensor) -> int:
    """The resident image store of the feed entry points (``engine.Div2kImageStore``); returns its image count."""
    _check(op, 'store', store, _u8, (None,), store.device)
    _check(op, 'img_off', img_off, _i64, (None,), store.device)
    _check(op, 'img_hw', img_hw, _i32, (img_off.numel(), 2), store.device)
    return img_off.numel()


def _batch_args(op, dev, b: int, **specs):
    """Per-sample plan columns: name=(tensor, dtype, shape of one sample)."""
    for name, (t, dtype, shape) in specs.items():
        _check(op, name, t, dtype, (b, *shape), dev)


def _crop_args(op, img: torch.Tensor, out: torch.Tensor | None, in_place: bool):
    """(B, S, out) of uint8 crops [B, 3, S, S] and an ``out`` like them (made here when None); it may be ``img`` only with ``in_place``."""
    _check(op, 'img', img, _u8, (None, 3) + tuple(img.shape[2:3]) * 2, img.device)
    out = _out(op, 'out', out, _u8, tuple(img.shape), img.device)
    if not in_place and out.data_ptr() == img.data_ptr():
        raise ValueError(f'{op}: out must not be img itself (the filter cannot run in place)')
    return img.shape[0], img.shape[2], out


def div2k_regions_u8(store: torch.Tensor, img_off: torch.Tensor, img_hw: torch.Tensor, image: torch.Tensor, flags: torch.Tensor,
                     minv: torch.Tensor, rgb: torch.Tensor, crop: torch.Tensor, img_size: int,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """Resident images -> uint8 regions [B, 3, 2 S, 3 S] (``vited_div2k_regions_u8``; div2k_patch.py:84-111): per sample the image
    index, the flag bits (1 hflip, 2 vflip, 4 warp, 8 colour shift), the inverse affine map fp64 [B, 6], the channel shifts
    fp32 [B, 3] and the crop origin int32 [B, 2] (top, left).  store uint8 [bytes] holds the HWC images at the byte offsets
    img_off int64 [n] with sizes img_hw int32 [n, 2] (H, W); the caller guarantees that every image lies inside the store and is
    at least 2 S x 3 S (``engine.Div2kImageStore`` does).  Indices and origins are clamped by the kernel."""
    _need_gpu(store, img_off, img_hw, image, flags, minv, rgb, crop, out)
    op, dev = 'div2k_regions_u8', store.device
    s, n, b = int(img_size), _store_args(op, store, img_off, img_hw), image.numel()
    _batch_args(op, dev, b, image=(image, _i32, ()), flags=(flags, _i32, ()), minv=(minv, _f64, (6,)), rgb=(rgb, _f32, (3,)),
                crop=(crop, _i32, (2,)))
    out = _out(op, 'out', out, _u8, (b, 3, 2 * s, 3 * s), dev)
    _lib.call('vited_div2k_regions_u8', _ptr(store), _ptr(img_off), _ptr(img_hw), n, _ptr(image), _ptr(flags), _ptr(minv), _ptr(rgb),
              _ptr(crop), _ptr(out), b, s, _stream())
    return out


def hisfrag_windows_u8(store: torch.Tensor, img_off: torch.Tensor, img_hw: torch.Tensor, image: torch.Tensor, flags: torch.Tensor,
                       afix: torch.Tensor, minv: torch.Tensor, origin: torch.Tensor, img_size: int,
                       out: torch.Tensor | None = None) -> torch.Tensor:
    """Resident images -> uint8 windows [B, 3, S, S] (``vited_hisfrag_windows_u8``; hisfrag.py:67-72): per sample the image index,
    the flag bits (1 RandomAffine, 2 ShiftScaleRotate; higher bits are ignored), Pillow's 16.16 affine coefficients int64 [B, 6],
    the inverse warp map fp64 [B, 6] and the window origin int32 [B, 2] (top, left) in unpadded image coordinates, negative in the
    pad.  store / img_off / img_hw as for ``div2k_regions_u8``.  Everything outside the image is 0; indices are clamped."""
    _need_gpu(store, img_off, img_hw, image, flags, afix, minv, origin, out)
    op, dev = 'hisfrag_windows_u8', store.device
    s, n, b = int(img_size), _store_args(op, store, img_off, img_hw), image.numel()
    _batch_args(op, dev, b, image=(image, _i32, ()), flags=(flags, _i32, ()), afix=(afix, _i64, (6,)), minv=(minv, _f64, (6,)),
                origin=(origin, _i32, (2,)))
    out = _out(op, 'out', out, _u8, (b, 3, s, s), dev)
    _lib.call('vited_hisfrag_windows_u8', _ptr(store), _ptr(img_off), _ptr(img_hw), n, _ptr(image), _ptr(flags), _ptr(afix), _ptr(minv),
              _ptr(origin), _ptr(out), b, s, _stream())
    return out


def hisfrag_jitter_u8(img: torch.Tensor, flags: torch.Tensor, order: torch.Tensor, factors: torch.Tensor, hue: torch.Tensor,
                      out: torch.Tensor | None = None) -> torch.Tensor:
    """ColorJitter on uint8 crops [B, 3, S, S] (``vited_hisfrag_jitter_u8``; hisfrag.py:73-75), Pillow's arithmetic bit for bit: per
    sample flag bit 4 (jitter on; a sample without it is copied), the four operations in the order they run int32 [B, 4]
    (0 brightness, 1 contrast, 2 saturation, 3 hue), the brightness / contrast / saturation factors fp32 [B, 3] and the uint8 hue
    shift int32 [B].  ``out`` may be ``img`` itself."""
    _need_gpu(img, flags, order, factors, hue, out)
    b, s, out = _crop_args('hisfrag_jitter_u8', img, out, in_place=True)
    _batch_args('hisfrag_jitter_u8', img.device, b, flags=(flags, _i32, ()), order=(order, _i32, (4,)), factors=(factors, _f32, (3,)),
                hue=(hue, _i32, ()))
    sums = torch.empty(b, dtype=torch.int64, device=img.device)             # the contrast means' L sums; the entry point zeroes them
    _lib.call('vited_hisfrag_jitter_u8', _ptr(img), _ptr(flags), _ptr(order), _ptr(factors), _ptr(hue), _ptr(sums), _ptr(out), b, s, _stream())
    return out


def hisfrag_blur_u8(img: torch.Tensor, flags: torch.Tensor, weights: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """GaussianBlur((3, 3)) on uint8 crops [B, 3, S, S] (``vited_hisfrag_blur_u8``; hisfrag.py:76-78): per sample flag bit 8 (blur on; a
    sample without it is copied) and the 1-D weights (k_edge, k_mid) fp32 [B, 2].  ``out`` must not overlap ``img``."""
    _need_gpu(img, flags, weights, out)
    b, s, out = _crop_args('hisfrag_blur_u8', img, out, in_place=False)
    _batch_args('hisfrag_blur_u8', img.device, b, flags=(flags, _i32, ()), weights=(weights, _f32, (2,)))
    _lib.call('vited_hisfrag_blur_u8', _ptr(img), _ptr(flags), _ptr(weights), _ptr(out), b, s, _stream())
    return out


def michigan_windows_u8(store: torch.Tensor, img_off: torch.Tensor, img_hw: torch.Tensor, image: torch.Tensor, flags: torch.Tensor,
                        origin: torch.Tensor, x0: torch.Tensor, kx: torch.Tensor, y0: torch.Tensor, ky: torch.Tensor, holes: torch.Tensor,
                        n_holes: torch.Tensor, img_size: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """Resident images -> uint8 crops [B, 3, S, S] (``vited_michigan_windows_u8``; michigan.py:72-79): per sample the image index, the
    flag bits (1 dropout, 2 horizontal flip, 16 vertical flip; the others are ignored), the window origin int32 [B, 2] (top, left)
    in unpadded image coordinates, Pillow's bilinear tap tables per axis (first tap int32 [B, S] in window coordinates, 22-bit
    weights int32 [B, S, 3]) and the dropout rectangles int32 [B, 16, 4] = (x1, y1, x2, y2), half-open, of which the first
    n_holes int32 [B] count.  store / img_off / img_hw as for ``div2k_regions_u8``.  Everything outside the image, and a tap outside
    the window, is 255; indices and the hole count are clamped."""
    _need_gpu(store, img_off, img_hw, image, flags, origin, x0, kx, y0, ky, holes, n_holes, out)
    op, dev = 'michigan_windows_u8', store.device
    s, n, b = int(img_size), _store_args(op, store, img_off, img_hw), image.numel()
    _batch_args(op, dev, b, image=(image, _i32, ()), flags=(flags, _i32, ()), origin=(origin, _i32, (2,)), x0=(x0, _i32, (s,)),
                kx=(kx, _i32, (s, 3)), y0=(y0, _i32, (s,)), ky=(ky, _i32, (s, 3)), holes=(holes, _i32, (16, 4)), n_holes=(n_holes, _i32, ()))
    out = _out(op, 'out', out, _u8, (b, 3, s, s), dev)
    _lib.call('vited_michigan_windows_u8', _ptr(store), _ptr(img_off), _ptr(img_hw), n, _ptr(image), _ptr(flags), _ptr(origin), _ptr(x0),
              _ptr(kx), _ptr(y0), _ptr(ky), _ptr(holes), _ptr(n_holes), _ptr(out), b, s, _stream())
    return out


def michigan_blur_gray_u8(img: torch.Tensor, flags: torch.Tensor, weights: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """ImageFilter.GaussianBlur(radius <= 1) and RandomGrayscale on uint8 crops [B, 3, S, S] (``vited_michigan_blur_gray_u8``;
    michigan.py:83-85): per sample flag bit 8 (blur), bit 32 (grey; a sample with neither is copied) and the box-blur weights
    (ww, fw) int32 [B, 2].  ``out`` must not overlap ``img``."""
    _need_gpu(img, flags, weights, out)
    b, s, out = _crop_args('michigan_blur_gray_u8', img, out, in_place=False)
    _batch_args('michigan_blur_gray_u8', img.device, b, flags=(flags, _i32, ()), weights=(weights, _i32, (2,)))
    _lib.call('vited_michigan_blur_gray_u8', _ptr(img), _ptr(flags), _ptr(weights), _ptr(out), b, s, _stream())
    return out


def slice_rows_cast(x: torch.Tensor, row_offset: int, rows: int, dtype: torch.dtype) -> torch.Tensor:
    """fp32 [B, R, D] -> dtype [B * rows, D] taking rows [row_offset, row_offset + rows) of every batch."""
    _need_gpu(x)
    _check('slice_rows_cast', 'x', x, _f32, _ANY3, x.device)
    b, r, d = x.shape
    if not 0 <= row_offset <= row_offset + rows <= r:
        raise ValueError(f'slice_rows_cast: x has {r} rows per batch, rows [{row_offset}, {row_offset + rows}) are not inside them')
    out = torch.empty((b * rows, d), dtype=dtype, device=x.device)
    _lib.call('vited_slice_rows_cast', _ptr(x), _ptr(out), _code(dtype), b, r, row_offset, rows, d, _stream())
    return out


def write_cls_row(x: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor):
    """x fp32 [B, R, D]: x[:, 0] = cls + pos[0]."""
    _need_gpu(x, cls, pos)
    _check('write_cls_row', 'x', x, _f32, _ANY3, x.device)
    b, r, d = x.shape
    _check('write_cls_row', 'cls', cls, _f32, _Min(d), x.device)
    _check('write_cls_row', 'pos', pos, _f32, _Min(d), x.device)
    _lib.call('vited_write_cls_row', _ptr(x), _ptr(cls), _ptr(pos), b, r, d, _stream())


def sum_rows(x: torch.Tensor) -> torch.Tensor:
    """[batch, width] (fp32 or bf16, dense rows) -> fp32 [width] column sums, deterministic."""
    _need_gpu(x)
    ld = _rows('sum_rows', 'x', x, _ACT, x.device)
    b, w = x.shape
    out = torch.empty(w, dtype=torch.float32, device=x.device)
    ws = _scratch(_lib.load().vited_sum_rows_workspace_bytes(b, w), x.device)
    _lib.call('vited_sum_rows', _ptr(x), _code(x.dtype), ld, _ptr(out), b, w, *ws, _stream())
    return out


# ---------------------------------------------------------------------------------------------
def _ln_grads(op, dev, dim, dgamma, dbeta):
    """(accumulate, dgamma, dbeta): the given fp32 [dim] pair to add onto, or a fresh pair."""
    if dgamma is None:
        return False, torch.empty(dim, dtype=torch.float32, device=dev), torch.empty(dim, dtype=torch.float32, device=dev)
    return True, _check(op, 'dgamma', dgamma, _f32, dim, dev), _check(op, 'dbeta', dbeta, _f32, dim, dev)


def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out_dtype: torch.dtype, out=None):
    """x fp32 [rows, dim] (row-strided ok) -> (y [rows, dim] out_dtype, mean, rstd).  ``out`` = (y, mean, rstd) pre-made
    (e.g. row slices of larger tensors)."""
    _need_gpu(x, gamma, beta)
    op, dev = 'layernorm_fwd', x.device
    ld = _rows(op, 'x', x, _f32, dev)
    rows, dim = x.shape
    _check(op, 'gamma', gamma, _f32, (dim,), dev)
    _check(op, 'beta', beta, _f32, (dim,), dev)
    y, mean, rstd = out if out is not None else (None, None, None)
    y = _out(op, 'out[0] (y)', y, out_dtype, (rows, dim), dev)
    mean = _out(op, 'out[1] (mean)', mean, _f32, rows, dev)
    rstd = _out(op, 'out[2] (rstd)', rstd, _f32, rows, dev)
    _lib.call('vited_layernorm_fwd', _ptr(x), ld, _ptr(gamma), _ptr(beta), _ptr(y), _code(out_dtype), dim, _ptr(mean), _ptr(rstd), rows,
              dim, float(eps), _stream())
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dx_in=None, dx_out=None, want_lp: bool = False, dx_lp=None, dgamma=None,
                  dbeta=None, lp_scale=None, lp_dtype=torch.bfloat16):
    """Returns (dx fp32, dx_lp bf16 | None, dgamma, dbeta).  When ``dgamma`` / ``dbeta`` are given (fp32,
    contiguous - e.g. views of the flat gradient buffer) the column sums are ADDED onto them.

    dx = (dx_in or 0) + LN'(dy).  ``dx_out`` / ``dx_lp`` may be given as pre-made (row-strided)
    destinations - e.g. the cls rows of a zero-filled token-gradient tensor.
    ``lp_scale`` (fp32 [rows]): dx_lp = lp_dtype(lp_scale[r] * dx[r]) (``vited_layernorm_bwd_scaled``; fp32 allowed then)."""
    _need_gpu(dy, x, gamma, mean, rstd, dx_in, dx_out, dx_lp, lp_scale, dgamma, dbeta)
    op, dev = 'layernorm_bwd', x.device
    x_ld = _rows(op, 'x', x, _f32, dev)
    rows, dim = x.shape
    dy_ld = _rows(op, 'dy', dy, _ACT, dev, dim, rows)
    for name, t, size in (('gamma', gamma, dim), ('mean', mean, rows), ('rstd', rstd, rows)):
        _check(op, name, t, _f32, size, dev)
    dx_out = _out(op, 'dx_out', dx_out, _f32, (rows, dim), dev, DENSE_LAST)
    if lp_scale is not None:
        _check(op, 'lp_scale', lp_scale, _f32, (rows,), dev)
        want_lp = True
    else:
        lp_dtype = torch.bfloat16
    if want_lp or dx_lp is not None:
        dx_lp = _out(op, 'dx_lp', dx_lp, lp_dtype, (rows, dim), dev, DENSE_LAST)
    _check(op, 'dx_in', dx_in, _f32, (rows, dim), dev, DENSE_LAST, optional=True)
    accumulate, dgamma, dbeta = _ln_grads(op, dev, dim, dgamma, dbeta)
    ws = _scratch(_lib.load().vited_layernorm_bwd_workspace_bytes(rows, dim), x.device)
    head = (_ptr(dy), _code(dy.dtype), dy_ld, _ptr(x), x_ld, _ptr(gamma), _ptr(mean), _ptr(rstd),
            _ptr(dx_in), dx_in.stride(0) if dx_in is not None else 0, _ptr(dx_out), dx_out.stride(0),
            _ptr(dx_lp), _code(lp_dtype), dx_lp.stride(0) if dx_lp is not None else 0)
    tail = (_ptr(dgamma), _ptr(dbeta), int(accumulate), rows, dim, *ws, _stream())
    if lp_scale is not None:
        _lib.call('vited_layernorm_bwd_scaled', *head, _ptr(lp_scale), *tail)
    else:
        _lib.call('vited_layernorm_bwd', *head, *tail)
    return dx_out, dx_lp, dgamma, dbeta


# ---------------------------------------------------------------------------------------------
def qk_norm_fwd(q, k, gq, bq, gk, bk, heads: int, eps: float, out=None):
    """q_norm / k_norm of the reference's attention (``qk_norm=True``): LayerNorm over the head_dim elements of every head of every
    row, for q and k in ONE launch (``vited_qk_norm_fwd``).  q, k: [rows, heads * head_dim] fp32 or bf16 with a dense last dim and
    any row stride - column slices of the packed projections - each with its own row count; either may be None (and its
    parameters with it).  gq, bq, gk, bk: fp32 [head_dim].  ``out`` = (q_out | None, k_out | None) pre-made (a slice of a larger
    buffer, or the input itself: in place).
    Returns (q_out, k_out, (q_mean, q_rstd), (k_mean, k_rstd)) - None for an absent operand; the statistics are fp32 [rows, heads]."""
    if q is None and k is None:
        raise ValueError('qk_norm_fwd: neither q nor k given')
    _need_gpu(q, k, gq, bq, gk, bk, *(out or ()))
    op, ref = 'qk_norm_fwd', q if q is not None else k
    dtype, dev = ref.dtype, ref.device
    outs, stats, args, width = [], [], [], None
    for name, t, g, b, o in (('q', q, gq, bq, out[0] if out else None), ('k', k, gk, bk, out[1] if out else None)):
        if t is None:
            outs.append(None)
            stats.append(None)
            args.append((0, 0, 0, 0, 0, 0, 0, 0, 0))
            continue
        ld, = _head_operand(op, name, t, _ACT if t is ref else dtype, (None, width), dev, like=None if t is ref else 'q')
        rows, width = t.shape
        hd = _head_dim(op, name, width, heads)
        _check(op, f'g{name}', g, _f32, hd, dev)
        _check(op, f'b{name}', b, _f32, hd, dev)
        o = _out(op, f'out[{len(outs)}]', o, dtype, (rows, width), dev, DENSE_LAST)
        mean = torch.empty((rows, heads), dtype=torch.float32, device=dev)
        rstd = torch.empty((rows, heads), dtype=torch.float32, device=dev)
        outs.append(o)
        stats.append((mean, rstd))
        args.append((_ptr(t), ld, rows, _ptr(g), _ptr(b), _ptr(o), o.stride(0), _ptr(mean), _ptr(rstd)))
    (qp, qld, qr, gqp, bqp, qop, qold, qm, qs), (kp, kld, kr, gkp, bkp, kop, kold, km, ks) = args
    _lib.call('vited_qk_norm_fwd', qp, qld, qr, kp, kld, kr, gqp, bqp, gkp, bkp, qop, qold, kop, kold, qm, qs, km, ks, _code(dtype), heads, hd,
              float(eps), _stream())
    return outs[0], outs[1], stats[0], stats[1]


def qk_norm_bwd(dq, q, q_stats, gq, dk, k, k_stats, gk, heads: int, dgq=None, dbq=None, dgk=None, dbk=None):
    """Backward of ``qk_norm_fwd`` (``vited_qk_norm_bwd``), one launch for both operands.  dq / dk hold the gradient of the NORMALISED
    q / k (where the attention backward wrote it) and are overwritten IN PLACE by the gradient of the pre-norm q / k; q, k are the
    saved pre-norm operands, q_stats / k_stats their (mean, rstd).  Either operand may be None.  The parameter gradients are
    deterministic sums over all rows and heads; given ``dgq`` ... ``dbk`` (fp32 [head_dim], contiguous - e.g. views of the flat
    gradient buffer; all of the present operands' or none) they are ADDED onto them.
    Returns (dgq, dbq, dgk, dbk), None for an absent operand."""
    if dq is None and dk is None:
        raise ValueError('qk_norm_bwd: neither dq nor dk given')
    _need_gpu(dq, q, gq, dk, k, gk, dgq, dbq, dgk, dbk)
    op, ref = 'qk_norm_bwd', dq if dq is not None else dk
    dtype, dev = ref.dtype, ref.device
    given = [t is not None for d, pair in ((dq, (dgq, dbq)), (dk, (dgk, dbk))) if d is not None for t in pair]
    accumulate = all(given)
    if any(given) and not accumulate:
        raise ValueError('qk_norm_bwd: give every gradient destination of the present operands, or none')
    args, grads, width, rows_of = [], [], None, []
    for name, d, x, st, g, dg, db in (('q', dq, q, q_stats, gq, dgq, dbq), ('k', dk, k, k_stats, gk, dgk, dbk)):
        if d is None:
            args.append((0,) * 10)
            grads += [None, None]
            rows_of.append(0)
            continue
        ld, = _head_operand(op, f'd{name}', d, _ACT if d is ref else dtype, (None, width), dev, like=None if d is ref else 'dq')
        rows, width = d.shape
        hd = _head_dim(op, f'd{name}', width, heads)
        x_ld, = _head_operand(op, name, x, dtype, (rows, width), dev, like=f'd{name}')
        mean, rstd = st
        _check(op, f'{name}_stats[0]', mean, _f32, (rows, heads), dev)
        _check(op, f'{name}_stats[1]', rstd, _f32, (rows, heads), dev)
        _check(op, f'g{name}', g, _f32, hd, dev)
        dg = _out(op, f'dg{name}', dg, _f32, hd, dev)
        db = _out(op, f'db{name}', db, _f32, hd, dev)
        grads += [dg, db]
        rows_of.append(rows)
        args.append((_ptr(d), ld, _ptr(x), x_ld, _ptr(mean), _ptr(rstd), _ptr(g), _ptr(dg), _ptr(db), rows))
    ws = _scratch(_lib.load().vited_qk_norm_bwd_workspace_bytes(rows_of[0], rows_of[1], heads, hd), dev)
    _lib.call('vited_qk_norm_bwd', *args[0], *args[1], _code(dtype), int(accumulate), heads, hd, *ws, _stream())
    return tuple(grads)


# ---------------------------------------------------------------------------------------------
def gemm(a: torch.Tensor, b: torch.Tensor, *, b_layout: int = B_NK, epilogue: int = EPI_STORE, bias=None, aux=None,
         residual=None, out=None, out2=None, rows_per_batch: int = 0, out_rows_per_batch: int = 0, row_offset: int = 0,
         residual_bcast: bool = False, out_rows: int | None = None, row_scale=None):
    """acc = a[M,K] . (b[N,K]^T | b[K,N]); see VITED_EPI_* in include/vited.h.  ``row_scale`` (fp32 [M], EPI_RESIDUAL with the
    identity row map only): out = residual + row_scale[m] * (acc + bias) (``vited_gemm_scaled``).

    Returns ``out`` (and ``out2`` for EPI_GELU)."""
    _need_gpu(a, b, bias, aux, residual, out, out2, row_scale)
    op, dev = 'gemm', a.device
    lda = _rows(op, 'a', a, _ACT, dev)
    m, k = a.shape
    ldb = _rows(op, 'b', b, a.dtype, dev, *((k, None) if b_layout == B_NK else (None, k)), like='a')
    n = b.shape[0] if b_layout == B_NK else b.shape[1]
    if row_scale is not None and (epilogue != EPI_RESIDUAL or rows_per_batch):
        raise ValueError('gemm: row_scale goes with EPI_RESIDUAL and the identity row map')
    # the rows written: m under the identity map, else up to the image of row m - 1 under the RESIDUAL remap of include/vited.h
    remap = epilogue == EPI_RESIDUAL and rows_per_batch > 0 and m > 0
    need = (m - 1) // rows_per_batch * out_rows_per_batch + (m - 1) % rows_per_batch + row_offset + 1 if remap else m
    out_dtype = torch.float32 if epilogue in (EPI_RESIDUAL, EPI_STORE_F32) else a.dtype
    if out is None and out_rows is None:
        out = torch.empty((m, n), dtype=out_dtype, device=dev)
        ldo = out.stride(0)
    else:
        out = torch.empty((out_rows, n), dtype=out_dtype, device=dev) if out is None else out
        ldo = _rows(op, 'out', out, out_dtype, dev, n, m if row_scale is not None else _Min(need))
    gelu = epilogue in (EPI_GELU, EPI_GELU_GRAD)
    out2 = (torch.empty_like(out) if out2 is None else out2) if gelu else None
    _check(op, 'out2', out2, out_dtype, tuple(out.shape), dev, DENSE_LAST, optional=not gelu, ld=ldo)
    _check(op, 'aux', aux, a.dtype, (m, n), dev, DENSE_LAST, optional=True, ld=ldo)
    if residual is not None:
        while residual.dim() > 2 and residual.shape[0] == 1:          # leading unit dims: the same rows
            residual = residual[0]
        res_rows = (min(m, rows_per_batch) + row_offset if residual_bcast else need) if remap else m
        _check(op, 'residual', residual, _f32, (_Min(res_rows), n), dev, DENSE_LAST, ld=ldo)
    _check(op, 'bias', bias, _f32, n, dev, optional=True)
    if row_scale is not None:
        _check(op, 'row_scale', row_scale, _f32, (m,), dev)
        _lib.call('vited_gemm_scaled', _ptr(a), lda, _ptr(b), ldb, b_layout, _code(a.dtype), m, n, k, _ptr(bias), _ptr(residual),
                  _ptr(row_scale), _ptr(out), ldo, _stream())
        return out
    _lib.call('vited_gemm', _ptr(a), lda, _ptr(b), ldb, b_layout, _code(a.dtype), m, n, k, epilogue, _ptr(bias), _ptr(aux), _ptr(residual),
              _ptr(out), _ptr(out2), ldo, rows_per_batch, out_rows_per_batch, row_offset, int(bool(residual_bcast)), _stream())
    return (out, out2) if gelu else out


def linear_bwd_weight(dy: torch.Tensor, x: torch.Tensor, want_bias: bool = True, dw_out=None, db_out=None):
    """dW[N,K] = dy[M,N]^T x[M,K] (fp32), dbias[N] = column sums of dy (fp32) or None.  With ``dw_out``
    (and ``db_out``) the results are ADDED onto those fp32 tensors (a parameter's .grad) instead."""
    _need_gpu(dy, x, dw_out, db_out)
    op, dev = 'linear_bwd_weight', x.device
    lddy = _rows(op, 'dy', dy, _ACT, dev)
    m, n = dy.shape
    ldx = _rows(op, 'x', x, dy.dtype, dev, None, m, like='dy')
    k = x.shape[1]
    accumulate = dw_out is not None
    if accumulate:
        dw = _check(op, 'dw_out', dw_out, _f32, n * k, dev)
        db = _check(op, 'db_out', db_out, _f32, n, dev, optional=True) if want_bias else None
    else:
        dw = torch.empty((n, k), dtype=torch.float32, device=dev)
        db = torch.empty(n, dtype=torch.float32, device=dev) if want_bias else None
    ws = _scratch(_lib.load().vited_linear_bwd_weight_workspace_bytes(m, n, k), x.device)
    _lib.call('vited_linear_bwd_weight', _ptr(dy), lddy, _ptr(x), ldx, _code(x.dtype), m, n, k, _ptr(dw), _ptr(db), int(accumulate), *ws,
              _stream())
    return dw, db


MAX_BATCHED_WEIGHT_GRADS = 40


def linear_bwd_weight_batched(items, accumulate: bool) -> bool:
    """items: list of (dy [M, N], x [M, K], dw fp32 [N, K] contiguous, db fp32 [N] | None).  dW_i (+)= dy_i^T x_i and db_i (+)= column
    sums of dy_i for every item in ONE launch of the wide weight-gradient kernel + one slab-sum launch
    (``vited_linear_bwd_weight_batched``).  Returns False (nothing launched) when the set is not covered - the caller then issues
    ``linear_bwd_weight`` per item."""
    n = len(items)
    if n < 1 or n > MAX_BATCHED_WEIGHT_GRADS:
        return False
    for i, (dy, x, dw, db) in enumerate(items):
        _need_gpu(dy, x, dw, db)
        if dy.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 or dy.shape[0] != x.shape[0]:
            return False
        op, dev = 'linear_bwd_weight_batched', items[0][0].device
        _rows(op, f'items[{i}][0] (dy)', dy, _bf16, dev)
        _rows(op, f'items[{i}][1] (x)', x, _bf16, dev)
        _check(op, f'items[{i}][2] (dw)', dw, _f32, dy.shape[1] * x.shape[1], dev)
        _check(op, f'items[{i}][3] (db)', db, _f32, dy.shape[1], dev, optional=True)
        if dw.data_ptr() % 16 or (db is not None and db.data_ptr() % 16) or dy.data_ptr() % 16 or x.data_ptr() % 16:
            return False                 # the batched kernels use 16-byte accesses throughout
    dys, xs, dws, dbs = zip(*items)
    M = _host_array(C.c_int64, [dy.shape[0] for dy in dys])
    N = _host_array(C.c_int64, [dy.shape[1] for dy in dys])
    K = _host_array(C.c_int64, [x.shape[1] for x in xs])
    lib = _lib.load()
    if not lib.vited_linear_bwd_weight_batched_supported(n, M, N, K, BF16):
        return False
    lddy, ldx = _host_array(C.c_int64, [dy.stride(0) for dy in dys]), _host_array(C.c_int64, [x.stride(0) for x in xs])
    ws = _scratch(lib.vited_linear_bwd_weight_batched_workspace_bytes(n, M, N, K), dys[0].device)
    _lib.call('vited_linear_bwd_weight_batched', n, _host_array(C.c_void_p, dys), lddy, _host_array(C.c_void_p, xs), ldx, M, N, K,
              _host_array(C.c_void_p, dws), _host_array(C.c_void_p, dbs), BF16, int(bool(accumulate)), *ws, _stream())
    return True


# ---------------------------------------------------------------------------------------------
def linear_layernorm_supported(m: int, n: int, k: int, dtype: torch.dtype) -> bool:
    """Whether the row-complete fused Linear + LayerNorm kernels (gemm_row.hip) cover the shape."""
    return dtype == torch.bfloat16 and bool(_lib.load().vited_linear_layernorm_supported(int(m), int(n), int(k)))


def linear_residual_layernorm_fwd(a, w, bias, residual, gamma=None, beta=None, eps: float = 1e-6, out=None, row_scale=None):
    """y = residual + a w^T + bias (fp32) and, with gamma / beta, h = LayerNorm(y) (bf16), mean, rstd - one kernel
    (``vited_linear_residual_layernorm_fwd``).  Returns (y, h | None, mean | None, rstd | None).
    ``row_scale`` (fp32 [M]): y = residual + row_scale[m] * (a w^T + bias) (``vited_linear_residual_layernorm_fwd_scaled``)."""
    _need_gpu(a, w, bias, residual, gamma, beta, out, row_scale)
    op, dev = 'linear_residual_layernorm_fwd', a.device
    lda = _rows(op, 'a', a, _bf16, dev)
    m, k = a.shape
    ldw = _rows(op, 'w', w, _bf16, dev, k)
    n = w.shape[0]
    ldr = _rows(op, 'residual', residual, _f32, dev, n, m)
    _check(op, 'bias', bias, _f32, n, dev, optional=True)
    y = _out(op, 'out', out, _f32, (m, n), dev, DENSE_LAST)
    h = mean = rstd = None
    if gamma is not None:
        _check(op, 'gamma', gamma, _f32, n, dev)
        _check(op, 'beta', beta, _f32, n, dev)
        h = torch.empty((m, n), dtype=torch.bfloat16, device=dev)
        mean = torch.empty(m, dtype=torch.float32, device=dev)
        rstd = torch.empty(m, dtype=torch.float32, device=dev)
    tail = (_ptr(y), y.stride(0), _ptr(gamma), _ptr(beta), float(eps), _ptr(h), n, _ptr(mean), _ptr(rstd), m, n, k, _stream())
    if row_scale is not None:
        _check(op, 'row_scale', row_scale, _f32, (m,), dev)
        _lib.call('vited_linear_residual_layernorm_fwd_scaled', _ptr(a), lda, _ptr(w), ldw, _ptr(bias), _ptr(residual), ldr, _ptr(row_scale),
                  *tail)
    else:
        _lib.call('vited_linear_residual_layernorm_fwd', _ptr(a), lda, _ptr(w), ldw, _ptr(bias), _ptr(residual), ldr, *tail)
    return y, h, mean, rstd


def linear_layernorm_bwd(dy, wt, x, gamma, mean, rstd, dx_in=None, dx_out=None, want_lp: bool = False, dgamma=None, dbeta=None,
                         defer=None, lp_scale=None):
    """dx = (dx_in or 0) + LN'(dy wt^T; x, mean, rstd, gamma) in one kernel (``vited_linear_layernorm_bwd``): the input
    gradient of ``y = LayerNorm(x) W^T`` without materialising d(LayerNorm output).  ``wt`` = the transposed weight shadow
    [N, K].  Returns (dx fp32, dx_lp bf16 | None, dgamma, dbeta); given ``dgamma`` / ``dbeta`` are ADDED onto.
    ``defer`` (a list): the column sums are NOT finished here - (partials, rows, dgamma, dbeta, accumulate) is appended and
    ``layernorm_bwd_finish(defer)`` later finishes many LayerNorms with one launch.
    ``lp_scale`` (fp32 [M]): dx_lp = bf16(lp_scale[m] * dx[m]) (``vited_linear_layernorm_bwd_scaled``)."""
    _need_gpu(dy, wt, x, gamma, mean, rstd, dx_in, dx_out, lp_scale, dgamma, dbeta)
    op, dev = 'linear_layernorm_bwd', x.device
    segments = 1
    if torch.is_tensor(dy) and dy.dim() == 3:
        # [L, M, seg_k]: the contraction dim arrives as L tensors (one per decoder block), wt is [N, L * seg_k]
        _check(op, 'dy', dy, _bf16, _ANY3, dev, DENSE_LAST)
        if dy.stride(0) % 8:
            raise ValueError(f'linear_layernorm_bwd: dy must have a segment stride that is a multiple of 8 elements, got {dy.stride(0)}')
        segments, m, seg_k = dy.shape
        lddy, seg_stride, k = dy.stride(1), dy.stride(0), segments * seg_k
    else:
        lddy = _rows(op, 'dy', dy, _bf16, dev)
        m, k = dy.shape
    ldwt = _rows(op, 'wt', wt, _bf16, dev, k)
    n = wt.shape[0]
    ldx = _rows(op, 'x', x, _f32, dev, n, m)
    for name, t, size in (('gamma', gamma, n), ('mean', mean, m), ('rstd', rstd, m)):
        _check(op, name, t, _f32, size, dev)
    lib = _lib.load()
    dx_out = _out(op, 'dx_out', dx_out, _f32, (m, n), dev, DENSE_LAST)
    _check(op, 'dx_in', dx_in, _f32, (m, n), dev, DENSE_LAST, optional=True)
    if lp_scale is not None:
        _check(op, 'lp_scale', lp_scale, _f32, (m,), dev)
        if segments != 1:
            raise ValueError('linear_layernorm_bwd: lp_scale does not go with a segmented dy')
        want_lp = True
    dx_lp = torch.empty((m, n), dtype=torch.bfloat16, device=dev) if want_lp else None
    accumulate, dgamma, dbeta = _ln_grads(op, dev, n, dgamma, dbeta)
    if defer is not None:
        rows = int(lib.vited_linear_layernorm_bwd_partial_rows_n(m, n))
        part = torch.empty(rows * 2 * n, dtype=torch.float32, device=x.device)     # lives until the flush
        defer.append((part, rows, dgamma, dbeta, accumulate))
        ws = (part.data_ptr(), part.numel() * 4)
    else:
        ws = _scratch(lib.vited_linear_layernorm_bwd_workspace_bytes(m, n), x.device)
    dx_args = (_ptr(x), ldx, _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dx_in), dx_in.stride(0) if dx_in is not None else 0, _ptr(dx_out),
               dx_out.stride(0), _ptr(dx_lp), n)
    sum_args = (0 if defer is not None else _ptr(dgamma), 0 if defer is not None else _ptr(dbeta), int(accumulate))
    tail = dx_args + sum_args
    if lp_scale is not None:          # the scaled prototype takes the scale right after the low-precision copy it applies to
        _lib.call('vited_linear_layernorm_bwd_scaled', _ptr(dy), lddy, _ptr(wt), ldwt, *dx_args, _ptr(lp_scale), *sum_args, m, n, k, *ws,
                  _stream())
    elif segments > 1:
        _lib.call('vited_linear_layernorm_bwd_segmented', _ptr(dy), lddy, seg_k, seg_stride, segments, _ptr(wt), ldwt, *tail, m, n, *ws,
                  _stream())
    else:
        _lib.call('vited_linear_layernorm_bwd', _ptr(dy), lddy, _ptr(wt), ldwt, *tail, m, n, k, *ws, _stream())
    return dx_out, dx_lp, dgamma, dbeta


def layernorm_bwd_finish(entries):
    """Finish the deferred column sums of ``linear_layernorm_bwd(..., defer=entries)``: one launch per 16 LayerNorms."""
    if not entries:
        return
    parts, rows, dgammas, dbetas, accumulate = zip(*entries)
    dim, dev = dgammas[0].numel(), dgammas[0].device
    _need_gpu(*parts, *dgammas, *dbetas)
    for i, (part, n_rows, dgamma, dbeta) in enumerate(zip(parts, rows, dgammas, dbetas)):
        for j, t, size in ((0, part, _Min(n_rows * 2 * dim)), (2, dgamma, dim), (3, dbeta, dim)):
            _check('layernorm_bwd_finish', f'entries[{i}][{j}]', t, _f32, size, dev)
    _lib.call('vited_layernorm_bwd_finish_batched', len(entries), _host_array(C.c_void_p, parts), _host_array(C.c_int, rows),
              _host_array(C.c_void_p, dgammas), _host_array(C.c_void_p, dbetas), _host_array(C.c_int, map(int, accumulate)),
              dim, _stream())
    entries.clear()


# ---------------------------------------------------------------------------------------------
MAX_FOLDED_BLOCKS = 16


def _block_lists(op, dev, n_blk, **lists):
    """Per-block fp32 buffers of the context fold: name=(list, shape or element count, whether an entry may be None)."""
    for name, (ts, shape, optional) in lists.items():
        if len(ts) != n_blk:
            raise ValueError(f'{op}: {name} has {len(ts)} entries for {n_blk} blocks')
        for i, t in enumerate(ts):
            _check(op, f'{name}[{i}]', t, _f32, shape, dev, optional=optional)


def fold_context_weights(ws, biases, gammas, betas, out=None):
    """Folded kv weights of several decoder blocks: W'_l = W_l o gamma_l (bf16, stacked [L N, K] and transposed [K, L N]) and
    b'_l = b_l + W_l beta_l (fp32 [L N]) - ``vited_fold_context_weights``.  ``out`` = (w, wt, b) buffers to refresh in place."""
    n_blk = len(ws)
    _need_gpu(*ws, *biases, *gammas, *betas, *(out or ()))
    op, dev = 'fold_context_weights', ws[0].device
    n, k = _check(op, 'ws[0]', ws[0], _f32, _ANY2, dev).shape
    _block_lists(op, dev, n_blk, ws=(ws, (n, k), False), biases=(biases, n, True), gammas=(gammas, k, False), betas=(betas, k, False))
    w_out, wt_out, b_out = out if out is not None else (None, None, None)
    out = (_out(op, 'out[0]', w_out, _bf16, (n_blk * n, k), dev), _out(op, 'out[1]', wt_out, _bf16, (k, n_blk * n), dev),
           _out(op, 'out[2]', b_out, _f32, n_blk * n, dev))
    _lib.call('vited_fold_context_weights', n_blk, *(_host_array(C.c_void_p, ts) for ts in (ws, biases, gammas, betas)), n, k,
              _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream())
    return out


def unfold_context_grads(dwf, dbf, ws, gammas, betas, dws, dbiases, dgammas, dbetas, accumulate: bool):
    """Gradients of the folded weights / bias -> dW_l, db_l, dgamma_l, dbeta_l (``vited_unfold_context_grads``)."""
    n_blk = len(ws)
    _need_gpu(dwf, dbf, *ws, *gammas, *betas, *dws, *dbiases, *dgammas, *dbetas)
    op, dev = 'unfold_context_grads', dwf.device
    n, k = _check(op, 'ws[0]', ws[0], _f32, _ANY2, dev).shape
    _check(op, 'dwf', dwf, _f32, (n_blk * n, k), dev)
    _check(op, 'dbf', dbf, _f32, n_blk * n, dev)
    _block_lists(op, dev, n_blk, ws=(ws, (n, k), False), gammas=(gammas, k, False), betas=(betas, k, False), dws=(dws, n * k, False),
                 dbiases=(dbiases, n, True), dgammas=(dgammas, k, False), dbetas=(dbetas, k, False))
    _lib.call('vited_unfold_context_grads', n_blk, _ptr(dwf), _ptr(dbf),
              *(_host_array(C.c_void_p, ts) for ts in (ws, gammas, betas, dws, dbiases, dgammas, dbetas)), n, k, int(bool(accumulate)),
              _stream())


# ---------------------------------------------------------------------------------------------
def mlp_fwd(x, gamma, beta, w1, b1, w2, b2, eps: float, save: bool = True, out=None):
    """y = x + fc2(gelu(fc1(LayerNorm(x)))) in one kernel (``vited_mlp_fwd``).  x fp32 [rows, 384]; w1 / w2 the bf16 weights.
    Returns (y, saved) with saved = (mean, rstd, h, gd, u) or None.  ``out`` = (y, mean, rstd, h, gd, u) pre-made outputs
    (row slices of larger tensors are fine for y; the others must be dense)."""
    _need_gpu(x, gamma, beta, w1, b1, w2, b2, *(out or ()))
    op, dev = 'mlp_fwd', x.device
    ldx = _rows(op, 'x', x, _f32, dev)
    rows, dim = x.shape
    hidden = _check(op, 'w1', w1, _bf16, (None, dim), dev).shape[0]
    _check(op, 'w2', w2, _bf16, (dim, hidden), dev)
    for name, t, size in (('gamma', gamma, dim), ('beta', beta, dim), ('b1', b1, hidden), ('b2', b2, dim)):
        _check(op, name, t, _f32, size, dev)
    y, mean, rstd, h, gd, u = out if out is not None else (None,) * 6
    y = _out(op, 'out[0] (y)', y, _f32, (rows, dim), dev, DENSE_LAST)
    if save:
        saved = ((mean, _f32, rows), (rstd, _f32, rows), (h, _bf16, (rows, dim)), (gd, _bf16, (rows, hidden)), (u, _bf16, (rows, hidden)))
        mean, rstd, h, gd, u = (_out(op, f'out[{i + 1}]', t, dtype, shape, dev) for i, (t, dtype, shape) in enumerate(saved))
    _lib.call('vited_mlp_fwd', _ptr(x), ldx, _ptr(gamma), _ptr(beta), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(y), y.stride(0),
              _ptr(h) if save else 0, _ptr(gd) if save else 0, _ptr(u) if save else 0, _ptr(mean) if save else 0, _ptr(rstd) if save else 0,
              rows, dim, hidden, float(eps), _stream())
    return y, ((mean, rstd, h, gd, u) if save else None)


def _block_params(op, dev, *params):
    """Parameters of a whole-block entry: (name, tensor, shape) of a bf16 weight, (name, tensor, length) of an fp32 bias or LayerNorm
    vector; only the biases of the q / k / v projections (qkv_bias=False) may be absent."""
    for name, t, shape in params:
        _check(op, name, t, _bf16 if type(shape) is tuple else _f32, shape, dev, optional=name in ('bqkv', 'bq', 'bkv'))


def block_fwd(x, heads: int, ln1_g, ln1_b, wqkv, bqkv, wproj, bproj, ln2_g, ln2_b, w1, b1, w2, b2, eps: float = 1e-6):
    """Encoder Block forward through ``vited_block_fwd``: x fp32 [B, N, D] -> y fp32 [B, N, D] (bf16 weights, inference form).
    The whole-block entry has no q/k-norm: a ``qk_norm=True`` model runs its blocks through functions.py (``qk_norm_fwd``)."""
    _need_gpu(x, ln1_g, ln1_b, wqkv, bqkv, wproj, bproj, ln2_g, ln2_b, w1, b1, w2, b2)
    op, dev = 'block_fwd', x.device
    b, n, d = _check(op, 'x', x, _f32, _ANY3, dev).shape
    _head_dim(op, 'x', d, heads)
    hidden = _check(op, 'w1', w1, _bf16, (None, d), dev).shape[0]
    _block_params(op, dev, ('wqkv', wqkv, (3 * d, d)), ('wproj', wproj, (d, d)), ('w2', w2, (d, hidden)), ('ln1_g', ln1_g, d), ('ln1_b', ln1_b, d),
                  ('bqkv', bqkv, 3 * d), ('bproj', bproj, d), ('ln2_g', ln2_g, d), ('ln2_b', ln2_b, d), ('b1', b1, hidden), ('b2', b2, d))
    y = torch.empty_like(x)
    ws = _scratch(_lib.load().vited_block_workspace_bytes(b, n, d, hidden, heads), dev, align=256)
    _lib.call('vited_block_fwd', _ptr(x), _ptr(y), b, n, d, heads, hidden, _ptr(ln1_g), _ptr(ln1_b), _ptr(wqkv), _ptr(bqkv), _ptr(wproj),
              _ptr(bproj), _ptr(ln2_g), _ptr(ln2_b), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), float(eps), *ws, _stream())
    return y


def cross_block_fwd(x, context, heads: int, ln1, wqkv, bqkv, wproj, bproj, lnq, lnc, wq, bq, wkv, bkv, wcproj, bcproj, ln2, w1, b1, w2, b2,
                    eps: float = 1e-6):
    """Decoder CrossBlock forward through ``vited_cross_block_fwd``: x fp32 [B, N2, D], context fp32 [B, N1, D] -> y fp32 [B, N2, D]
    (bf16 weights, inference form).  ln1 / lnq / lnc / ln2 = (gamma, beta) of norm1 / norm_cross / norm_context / norm2.
    The whole-block entry has no q/k-norm: a ``qk_norm=True`` model runs its blocks through functions.py (``qk_norm_fwd``)."""
    _need_gpu(x, context, *ln1, wqkv, bqkv, wproj, bproj, *lnq, *lnc, wq, bq, wkv, bkv, wcproj, bcproj, *ln2, w1, b1, w2, b2)
    op, dev = 'cross_block_fwd', x.device
    b, n, d = _check(op, 'x', x, _f32, _ANY3, dev).shape
    nc = _check(op, 'context', context, _f32, (b, None, d), dev).shape[1]
    _head_dim(op, 'x', d, heads)
    hidden = _check(op, 'w1', w1, _bf16, (None, d), dev).shape[0]
    _block_params(op, dev, ('wqkv', wqkv, (3 * d, d)), ('wproj', wproj, (d, d)), ('wq', wq, (d, d)), ('wkv', wkv, (2 * d, d)),
                  ('wcproj', wcproj, (d, d)), ('w2', w2, (d, hidden)), ('bqkv', bqkv, 3 * d), ('bproj', bproj, d), ('bq', bq, d), ('bkv', bkv, 2 * d),
                  ('bcproj', bcproj, d), ('b1', b1, hidden), ('b2', b2, d), ('ln1[0]', ln1[0], d), ('ln1[1]', ln1[1], d), ('lnq[0]', lnq[0], d),
                  ('lnq[1]', lnq[1], d), ('lnc[0]', lnc[0], d), ('lnc[1]', lnc[1], d), ('ln2[0]', ln2[0], d), ('ln2[1]', ln2[1], d))
    y = torch.empty_like(x)
    ws = _scratch(_lib.load().vited_cross_block_workspace_bytes(b, n, nc, d, hidden, heads), dev, align=256)
    _lib.call('vited_cross_block_fwd', _ptr(x), _ptr(context), _ptr(y), b, n, nc, d, heads, hidden, _ptr(ln1[0]), _ptr(ln1[1]), _ptr(wqkv),
              _ptr(bqkv), _ptr(wproj), _ptr(bproj), _ptr(lnq[0]), _ptr(lnq[1]), _ptr(lnc[0]), _ptr(lnc[1]), _ptr(wq), _ptr(bq), _ptr(wkv),
              _ptr(bkv), _ptr(wcproj), _ptr(bcproj), _ptr(ln2[0]), _ptr(ln2[1]), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), float(eps), *ws,
              _stream())
    return y


# ---------------------------------------------------------------------------------------------
def _qkv_operands(op, q, k, v, heads, items=None):
    """(B, Nq, Nk, D, head_dim) and the (pointer, batch stride, token stride) triples of q [B, Nq, D] and k / v [items or B, Nk, D]."""
    dev = q.device
    qs = _head_operand(op, 'q', q, _ACT, _ANY3, dev)
    b, nq, d = q.shape
    ks = _head_operand(op, 'k', k, q.dtype, (b if items is None else items, None, d), dev, like='q')
    vs = _head_operand(op, 'v', v, q.dtype, k.shape, dev, like='k')
    return (b, nq, k.shape[1], d, _head_dim(op, 'q', d, heads)), (_ptr(q), *qs, _ptr(k), *ks, _ptr(v), *vs)


def attention_fwd(q, k, v, heads: int, scale: float, kv_index=None):
    """q [B,Nq,D], k/v [B,Nk,D] (strided views of the packed qkv / kv projections are fine)
    -> (o [B,Nq,D] contiguous, lse fp32 [B,H,Nq]).  With ``kv_index`` (int64 [B]) batch item b attends over
    k[kv_index[b]] / v[kv_index[b]] and k / v may hold any number of items (inference only)."""
    _need_gpu(q, k, v, kv_index)
    (b, nq, nk, d, hd), qkv = _qkv_operands('attention_fwd', q, k, v, heads, items=None if kv_index is None else k.shape[0])
    _check('attention_fwd', 'kv_index', kv_index, _i64, b, q.device, optional=True)
    o = torch.empty((b, nq, d), dtype=q.dtype, device=q.device)
    lse = torch.empty((b, heads, nq), dtype=torch.float32, device=q.device)
    _lib.call('vited_attention_fwd_indexed', *qkv, _ptr(kv_index), _ptr(o), nq * d,
              d, _ptr(lse), _code(q.dtype), b, heads, nq, nk, hd, float(scale), _stream())
    return o, lse


class PairSegments(NamedTuple):
    """The pairs of a pair batch grouped by the key/value item they read (``pair_segments``)."""
    index: torch.Tensor      # int64 [P]: pair p reads item index[p]
    order: torch.Tensor      # int64 [P]: the stable argsort of index - pair numbers grouped by item, ascending inside a group
    offsets: torch.Tensor    # int64 [items + 1]: group g is order[offsets[g]:offsets[g + 1]]

    @property
    def items(self) -> int:
        return self.offsets.numel() - 1

    def to(self, device):
        return self if self.index.device == torch.device(device) else PairSegments(*(t.to(device) for t in self))


def pair_segments(index: torch.Tensor, items: int) -> PairSegments:
    """Group the pairs of ``index`` (integers [P], pair p reads item index[p] of ``items``) for ``attention_bwd(segments=...)``.
    Plain torch (stable argsort, counts, cumsum), on the index's device - CPU tensors too.  Raises ValueError for an index outside
    [0, items): that check reads one flag back (one synchronisation on a GPU tensor), so that no bad index ever reaches a kernel."""
    items = int(items)
    if index.dim() != 1 or index.dtype.is_floating_point or index.dtype == torch.bool:
        raise ValueError(f'pair_segments: expected a 1-D integer index, got {index.dtype} {tuple(index.shape)}')
    if items < 0 or (items == 0 and index.numel()):
        raise ValueError(f'pair_segments: {index.numel()} pairs over {items} items')
    index = index.to(torch.int64).contiguous()
    if index.numel() and bool(((index < 0) | (index >= items)).any()):
        raise ValueError(f'pair_segments: index outside [0, {items}): min {int(index.min())}, max {int(index.max())}')
    order = torch.argsort(index, stable=True)
    offsets = torch.zeros(items + 1, dtype=torch.int64, device=index.device)
    if items:
        offsets[1:] = torch.cumsum(torch.bincount(index, minlength=items), 0)
    return PairSegments(index, order, offsets)


MINE_MAX_CAPACITY = 24576      # vited_mine_pairs keeps one byte of LDS per output row (include/vited.h)


def mine_pairs_max_images() -> int:
    """The largest batch ``mine_pairs`` takes (128: its sort of the n * n cells lives in one workgroup's LDS)."""
    return int(_lib.load().vited_mine_pairs_max_images())


def _mine_pairs_args(targets, keys, neg_per_pos, capacity):
    """The argument checks of ``mine_pairs`` (before any launch, also without a GPU).  Returns (n, neg_per_pos, capacity)."""
    dev = targets.device if torch.is_tensor(targets) else None
    _check('mine_pairs', 'targets', targets, _i64, (_Min(1),), dev)
    n = targets.numel()
    _check('mine_pairs', 'keys', keys, _f32, (n * n,), dev)                 # one key per ordered cell
    neg_per_pos, capacity = float(neg_per_pos), int(capacity)
    if not 0.0 <= neg_per_pos < float('inf'):
        raise ValueError(f'mine_pairs: neg_per_pos must be a finite number >= 0, got {neg_per_pos}')
    if capacity < 1:
        raise ValueError(f'mine_pairs: capacity must be at least 1, got {capacity}')
    _need_gpu(targets, error=ValueError)        # engine.mine_pairs_device restates the rule for CPU tensors
    if n > mine_pairs_max_images():
        raise ValueError(f'mine_pairs: {n} images, the kernel takes at most {mine_pairs_max_images()}')
    if capacity > MINE_MAX_CAPACITY:
        raise ValueError(f'mine_pairs: capacity {capacity} above the {MINE_MAX_CAPACITY} rows the kernel supports')
    return n, neg_per_pos, capacity


def mine_pairs_out(targets, keys, neg_per_pos, ordered_negatives, groups, labels, weights, seg_index, seg_order, seg_offsets, counts):
    """``mine_pairs`` into the caller's buffers (every element of every one is written): groups int64 [capacity, 2], labels /
    weights fp32 [capacity, 1], seg_index / seg_order int64 [capacity], seg_offsets int64 [n + 1], counts int32 [5]."""
    n, neg_per_pos, capacity = _mine_pairs_args(targets, keys, neg_per_pos, groups.shape[0] if torch.is_tensor(groups) and groups.dim() else 0)
    for name, t, dtype, shape in (('groups', groups, _i64, (capacity, 2)), ('labels', labels, _f32, (capacity, 1)),
                                  ('weights', weights, _f32, (capacity, 1)), ('seg_index', seg_index, _i64, (capacity,)),
                                  ('seg_order', seg_order, _i64, (capacity,)), ('seg_offsets', seg_offsets, _i64, (n + 1,)),
                                  ('counts', counts, _i32, (5,))):
        _check('mine_pairs', name, t, dtype, shape, targets.device)
    _lib.call('vited_mine_pairs', _ptr(targets), n, _ptr(keys), neg_per_pos, int(bool(ordered_negatives)), capacity, _ptr(groups),
              _ptr(labels), _ptr(weights), _ptr(seg_index), _ptr(seg_order), _ptr(seg_offsets), _ptr(counts), _stream())


def mine_pairs(targets: torch.Tensor, keys: torch.Tensor, neg_per_pos: float, ordered_negatives: bool, capacity: int):
    """Pair mining of the two-stage training step in one launch, without a host read (include/vited.h states the rule).

    ``targets`` int64 [n] (n <= 128), ``keys`` fp32 [n * n] in [0, 1): one per ordered cell i * n + j.  Rows: every cell with i < j and
    equal targets in ascending cell order, then the min(#candidates, int(neg_per_pos * #positives)) different-target candidates
    (i < j, or i != j with ``ordered_negatives``) with the smallest (key, cell), then padding rows (0, 0) up to ``capacity``.
    Returns (groups int64 [capacity, 2], labels fp32 [capacity, 1], weights fp32 [capacity, 1] - 1 for a pair, 0 for padding -,
    ``PairSegments`` of groups[:, 1] over n items, counts int32 [5]: positives, candidates, negatives emitted, pairs emitted,
    pairs dropped for lack of capacity).  Raises ValueError for a bad argument before anything is launched."""
    n, neg_per_pos, capacity = _mine_pairs_args(targets, keys, neg_per_pos, capacity)
    dev = targets.device
    groups = torch.empty((capacity, 2), dtype=torch.int64, device=dev)
    labels = torch.empty((capacity, 1), dtype=torch.float32, device=dev)
    weights = torch.empty((capacity, 1), dtype=torch.float32, device=dev)
    seg_index, seg_order = (torch.empty(capacity, dtype=torch.int64, device=dev) for _ in range(2))
    seg_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    counts = torch.empty(5, dtype=torch.int32, device=dev)
    mine_pairs_out(targets, keys, neg_per_pos, ordered_negatives, groups, labels, weights, seg_index, seg_order, seg_offsets, counts)
    return groups, labels, weights, PairSegments(seg_index, seg_order, seg_offsets), counts


def attention_bwd(q, k, v, o, do, lse, heads: int, scale: float, dq, dk, dv, kv_index=None, segments=None):
    """Writes dq/dk/dv (pre-allocated, same strided conventions as q/k/v).
    With ``segments`` (a ``PairSegments``; or ``kv_index``, an integer [B] tensor it is then built from) batch item b read
    k[index[b]] / v[index[b]] in the forward: k / v / dk / dv hold ``segments.items`` items, dq stays per pair and
    dk[g] / dv[g] are the sums over the pairs of item g in ascending pair order - zeros for an item without pairs
    (``vited_attention_bwd_indexed``: per-pair terms in the workspace, then a segmented sum; no atomics)."""
    _need_gpu(q, k, v, o, do, lse, dq, dk, dv)
    op, dev = 'attention_bwd', q.device
    if segments is None and kv_index is not None:
        segments = pair_segments(kv_index, k.shape[0])
    if segments is not None and not isinstance(segments, PairSegments):
        raise TypeError(f'attention_bwd: segments must be a PairSegments (ops.pair_segments), got {type(segments).__name__}')
    items = None if segments is None else k.shape[0]
    (b, nq, nk, d, hd), qkv = _qkv_operands(op, q, k, v, heads, items)
    _check(op, 'o', o, q.dtype, q.shape, dev, like='q')
    _check(op, 'do', do, q.dtype, q.shape, dev, like='q')
    _check(op, 'lse', lse, _f32, (b, heads, nq), dev)
    grads = (_ptr(dq), *_head_operand(op, 'dq', dq, q.dtype, q.shape, dev, like='q'),
             _ptr(dk), *_head_operand(op, 'dk', dk, q.dtype, k.shape, dev, like='k'),
             _ptr(dv), *_head_operand(op, 'dv', dv, q.dtype, k.shape, dev, like='v'))
    delta = torch.empty((b, heads, nq), dtype=torch.float32, device=dev)
    tail = (_ptr(o), _ptr(do), nq * d, d, _ptr(lse), _ptr(delta), *grads, _code(q.dtype), b, heads, nq, nk, hd, float(scale))
    if segments is None:
        _lib.call('vited_attention_bwd', *qkv, *tail, _stream())
        return dq, dk, dv
    if kv_index is not None and kv_index is not segments.index and not torch.equal(kv_index.to(segments.index.device), segments.index):
        raise ValueError('attention_bwd: kv_index and segments.index differ')
    for name, t, size in (('index', segments.index, b), ('order', segments.order, b), ('offsets', segments.offsets, items + 1)):
        _check(op, f'segments.{name}', t, _i64, (size,), dev)
    nbytes = _lib.load().vited_attention_bwd_indexed_workspace_bytes(_code(q.dtype), b, heads, nk, hd)
    if nbytes < 0:
        raise ValueError(f'attention_bwd: empty operands (B {b}, heads {heads}, Nk {nk}, head_dim {hd})')
    _lib.call('vited_attention_bwd_indexed', *qkv, _ptr(segments.index), _ptr(segments.order), _ptr(segments.offsets), items, *tail,
              *_scratch(nbytes, dev, align=16), _stream())
    return dq, dk, dv


CAM_GRAD, CAM_PROB = 0, 1          # VITED_CAM_GRAD / VITED_CAM_PROB
_CAM_MODES = {'grad': CAM_GRAD, 'prob': CAM_PROB, CAM_GRAD: CAM_GRAD, CAM_PROB: CAM_PROB}


def attention_cam(q, k, v, do, lse, heads: int, scale: float, *, mode, head_weight=None, out=None):
    """Head-averaged relevancy map [B, Nq, Nk] fp32 of one attention, never forming a per-head map (vited_attention_cam):
    ``mode='grad'``: mean_h max(P_h o dP_h, 0) with P_h = softmax(scale q_h k_h^T) rebuilt from ``lse`` (what attention_fwd
    returned for these q / k) and dP_h = dO_h v_h^T - avg_heads(attn, grad) of scripts/visualise_attentions.py;
    ``mode='prob'``: sum_h head_weight[b, h] P_h (``head_weight`` fp32 [B, H]; None = 1/H, the head mean of the attention);
    ``v`` and ``do`` are not read and may be None.  q [B,Nq,D], k / v [B,Nk,D], do [B,Nq,D]: strided views of the packed
    projections are fine.  ``out``: fp32 [B, Nq, >= Nk] view with a dense last dim; only [:, :, :Nk] is written."""
    if mode not in _CAM_MODES:
        raise ValueError(f"attention_cam: mode must be 'grad' or 'prob', got {mode!r}")
    mode = _CAM_MODES[mode]
    if mode == CAM_GRAD and (v is None or do is None):
        raise ValueError("attention_cam: mode='grad' needs v and do")
    if mode == CAM_GRAD and head_weight is not None:
        raise ValueError("attention_cam: head_weight belongs to mode='prob'")
    if mode == CAM_PROB:
        v = do = None
    _need_gpu(q, k, v, do, lse, head_weight, out)
    op, dev = 'attention_cam', q.device
    qs = _head_operand(op, 'q', q, _ACT, _ANY3, dev)
    b, nq, d = q.shape
    hd = _head_dim(op, 'q', d, heads)
    ks = _head_operand(op, 'k', k, q.dtype, (b, None, d), dev, like='q')
    nk = k.shape[1]
    vs = _head_operand(op, 'v', v, q.dtype, (b, nk, d), dev, optional=True, like='q')
    dos = _head_operand(op, 'do', do, q.dtype, (b, nq, d), dev, optional=True, like='q')
    if b == 0 or nq == 0 or nk == 0:
        raise ValueError(f'attention_cam: empty operands (B {b}, Nq {nq}, Nk {nk})')
    _check(op, 'lse', lse, _f32, (b, heads, nq), dev)
    _check(op, 'head_weight', head_weight, _f32, (b, heads), dev, optional=True)
    if out is None:
        out = torch.empty((b, nq, nk), dtype=torch.float32, device=dev)
    _check(op, 'out', out, _f32, (b, nq, _Min(nk)), dev, DENSE_LAST)
    _lib.call('vited_attention_cam', _ptr(q), *qs, _ptr(k), *ks, _ptr(v), *vs, _ptr(do), *dos, _ptr(lse),
              _ptr(head_weight), _ptr(out), out.stride(0), out.stride(1), mode, _code(q.dtype), b, heads, nq, nk, hd,
              float(scale), _stream())
    return out[:, :, :nk] if out.shape[2] != nk else out


def last_paths():
    lib = _lib.load()
    return lib.vited_last_gemm_path(), lib.vited_last_attention_path()


def fp32_gemm_supported(m: int, n: int, k: int, b_layout: int = B_NK, epilogue: int = EPI_STORE) -> bool:
    """Whether ``gemm`` of that shape on GEMM path 1 (fp32, or bf16 outside the bf16 MFMA tiles) takes the matrix-core kernel
    (gemm_f32_mfma.hip) under ``'auto'``.  Host-only."""
    return bool(_lib.load().vited_gemm_f32_mfma_supported(int(m), int(n), int(k), int(b_layout), int(epilogue)))


def last_fp32_gemm_kernel() -> int:
    """Which kernel the last path-1 ``gemm`` / ``linear_bwd_weight`` of this thread ran: 0 none yet, 1 vector-ALU, 2 matrix-core."""
    return _lib.load().vited_last_fp32_gemm_kernel()


_FP32_GEMM_MODES = {'auto': 0, 'valu': 1}


@contextlib.contextmanager
def fp32_gemm_kernels(mode: str):
    """Within the block, path-1 GEMMs pick their kernel automatically (``'auto'``, the default of the process) or stay on the
    vector-ALU kernels (``'valu'``); the previous mode returns on exit.  Both give the same bits.  Process-wide."""
    if mode not in _FP32_GEMM_MODES:
        raise ValueError(f"fp32_gemm_kernels: mode is 'auto' or 'valu', not {mode!r}")
    select = _lib.load().vited_fp32_gemm_select          # returns the previous mode, not a status: only valid modes are passed
    previous = select(_FP32_GEMM_MODES[mode])
    try:
        yield
    finally:
        select(previous)


# ---------------------------------------------------------------------------------------------
# evaluation: retrieval metrics of a distance matrix (misc/wi19_evaluate.get_metrics)
# ---------------------------------------------------------------------------------------------
def _ranking_args(op, what, matrix, labels, rows):
    """(dtype code, ld, n, r0, r1) of the [n, n] matrix a ranking-metrics entry takes, after the checks both entries share."""
    if matrix.dtype not in _FLOATS:
        raise TypeError(f'{op}: matrix must be float32, bfloat16 or float16 for the {what} metrics, got {matrix.dtype}')
    if matrix.dim() != 2 or matrix.shape[0] != matrix.shape[1]:
        raise ValueError(f'{op}: matrix must be a square [n, n] matrix, got shape {tuple(matrix.shape)}')
    n = matrix.shape[0]
    ld = _rows(op, 'matrix', matrix, _FLOATS, matrix.device, n, n)
    _check(op, 'labels', labels, _i32, (n,), matrix.device)
    r0, r1 = int(rows[0]), int(rows[1])
    if not 0 <= r0 < r1 <= n:
        raise ValueError(f'{op}: rows ({r0}, {r1}) is not a non-empty range inside [0, {n})')
    return _DTYPE[matrix.dtype], ld, n, r0, r1


def retrieval_metrics_rows(matrix: torch.Tensor, labels: torch.Tensor, offsets: torch.Tensor, members: torch.Tensor,
                           rows: tuple[int, int], *, remove_self_column: bool = True, from_similarity: bool = False):
    """Row records (float64 [r1 - r0, 5]: AP sum, correct retrievals, top-1 hit, hits in the first 10, in the first 100) and
    their sums (float64 [7], see include/vited.h) for the rows [r0, r1) of the [n, n] matrix.  ``labels`` int32 [n] in
    [0, C) with the class CSR ``offsets`` int32 [C + 1] / ``members`` int32 [n] built from them (engine.class_members)."""
    _need_gpu(matrix, labels, offsets, members)
    dt, ld, n, r0, r1 = _ranking_args('retrieval_metrics_rows', 'retrieval', matrix, labels, rows)
    _check('retrieval_metrics_rows', 'members', members, _i32, (n,), matrix.device)
    _check('retrieval_metrics_rows', 'offsets', offsets, _i32, (None,), matrix.device)
    rows_out = torch.empty((r1 - r0, 5), dtype=torch.float64, device=matrix.device)
    sums = torch.empty(7, dtype=torch.float64, device=matrix.device)
    _lib.call('vited_retrieval_metrics', _ptr(matrix), dt, ld, n, r0, r1, _ptr(labels), _ptr(offsets), _ptr(members), offsets.numel() - 1,
              int(bool(remove_self_column)), int(bool(from_similarity)), _ptr(rows_out), _ptr(sums), _stream())
    return rows_out, sums


# ---------------------------------------------------------------------------------------------
# evaluation: group mAP / Pr@k (misc/metric.calc_map_prak) and pair-score aggregation (michigan.py:188-209)
# ---------------------------------------------------------------------------------------------
def group_retrieval_metrics_rows(matrix: torch.Tensor, labels: torch.Tensor, col_csr, pos_csr, neg_csr, ks, rows: tuple[int, int]):
    """Row records (float64 [r1 - r0, 3 + len(ks)]: AP, valid, correct retrievals, hits_k for every k) and their sums
    (float64 [2 + len(ks)], see include/vited.h) of calc_map_prak for the rows [r0, r1) of the [n, n] distance matrix.
    ``labels`` int32 [n] label ids in [0, L); ``col_csr`` = (offsets int32 [L + 1], members int32 [n]) the columns of every label;
    ``pos_csr`` / ``neg_csr`` = (offsets int32 [L + 1], label ids int32), every row ascending and without duplicates; ``neg_csr``
    may be None.  ``ks``: 1 to 8 ints >= 1."""
    _need_gpu(matrix, labels, *col_csr, *pos_csr, *(neg_csr or ()))
    op = 'group_retrieval_metrics_rows'
    dt, ld, n, r0, r1 = _ranking_args(op, 'group retrieval', matrix, labels, rows)
    num_labels = col_csr[0].numel() - 1
    for name, (off, vals) in (('col_csr', col_csr), ('pos_csr', pos_csr)) + ((('neg_csr', neg_csr),) if neg_csr is not None else ()):
        _check(op, f'{name}[0] (offsets)', off, _i32, (num_labels + 1,), matrix.device)
        _check(op, f'{name}[1] (members)', vals, _i32, (n if name == 'col_csr' else None,), matrix.device)
    ks = [int(k) for k in ks]
    if not 1 <= len(ks) <= 8 or min(ks) < 1:
        raise ValueError(f'ks must be 1 to 8 cut-offs >= 1, got {ks}')
    rows_out = torch.empty((r1 - r0, 3 + len(ks)), dtype=torch.float64, device=matrix.device)
    sums = torch.empty(2 + len(ks), dtype=torch.float64, device=matrix.device)
    neg_off, neg_lab = neg_csr if neg_csr is not None else (None, None)
    _lib.call('vited_group_retrieval_metrics', _ptr(matrix), dt, ld, n, r0, r1, _ptr(labels), num_labels, _ptr(col_csr[0]),
              _ptr(col_csr[1]), _ptr(pos_csr[0]), _ptr(pos_csr[1]), _ptr(neg_off), _ptr(neg_lab), _host_array(C.c_int, ks), len(ks),
              _ptr(rows_out), _ptr(sums), _stream())
    return rows_out, sums


def _pair_score_buffers(op, dev, n, m, counts, rec_cells, rec_values, bad):
    """The accumulator state both pair-score entries take: counts int32 [n, n], m records, the flag word."""
    for name, t, dtype, shape in (('counts', counts, _i32, (n, n)), ('rec_cells', rec_cells, _i32, (m, 2)), ('rec_values', rec_values, _f32, (m,)),
                                  ('bad', bad, _i32, (1,))):
        _check(op, name, t, dtype, shape, dev)


def pair_scores_add(pairs: torch.Tensor, scores: torch.Tensor, n: int, counts: torch.Tensor, rec_cells: torch.Tensor,
                    rec_values: torch.Tensor, bad: torch.Tensor):
    """Stores the records (pairs[r, 0], pairs[r, 1], 1 - scores[r]) into rec_cells int32 [m, 2] / rec_values float32 [m] and
    counts them into counts int32 [n, n] (both cells (i, j) and (j, i)).  Ids outside [0, n) set bit 0 of bad int32 [1]."""
    _need_gpu(pairs, scores, counts, rec_cells, rec_values, bad)
    op, dev = 'pair_scores_add', pairs.device
    if torch.is_tensor(pairs) and pairs.dim() == 2 and pairs.stride(1) != 1:
        pairs = pairs.contiguous()
    _check(op, 'pairs', pairs, (_i32, _i64), (None, 2), dev, DENSE_LAST)
    m = pairs.shape[0]
    scores = _check(op, 'scores', scores, _FLOATS, (m,), dev, None).contiguous()
    _pair_score_buffers(op, dev, n, m, counts, rec_cells, rec_values, bad)
    if m == 0:
        return
    _lib.call('vited_pair_scores_add', _ptr(pairs), _DTYPE[pairs.dtype], pairs.stride(0), _ptr(scores), _DTYPE[scores.dtype], m, n,
              _ptr(counts), _ptr(rec_cells), _ptr(rec_values), _ptr(bad), _stream())


def pair_scores_finish(rec_cells: torch.Tensor, rec_values: torch.Tensor, n: int, counts: torch.Tensor, bad: torch.Tensor):
    """(mean float32 [n, n], min float32 [n, n], stdev float64 [n, n], stats float64 [2] = (avg_std, std_std)) of every stored
    record; see include/vited.h."""
    _need_gpu(rec_cells, rec_values, counts, bad)
    m = rec_values.numel()
    _pair_score_buffers('pair_scores_finish', counts.device, n, m, counts, rec_cells, rec_values, bad)
    ws_bytes = _lib.load().vited_pair_scores_workspace_bytes(n, m)
    if ws_bytes < 0:
        raise ValueError(f'{n} fragments / {m} records is outside what vited_pair_scores_finish takes')
    dev = counts.device
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    mean = torch.empty((n, n), dtype=torch.float32, device=dev)
    minv = torch.empty((n, n), dtype=torch.float32, device=dev)
    stdev = torch.empty((n, n), dtype=torch.float64, device=dev)
    stats = torch.empty(2, dtype=torch.float64, device=dev)
    _lib.call('vited_pair_scores_finish', _ptr(rec_cells), _ptr(rec_values), m, n, _ptr(counts), _ptr(mean), _ptr(minv), _ptr(stdev),
              _ptr(stats), _ptr(bad), _ptr(ws), ws_bytes, _stream())
    return mean, minv, stdev, stats


# ---- puzzle solving: Paikin-Tal compatibility stage (include/vited.h) ------------------------------------------------------------
def puzzle_distances_from_logits(logits: torch.Tensor, pi: torch.Tensor, pj: torch.Tensor, dq: torch.Tensor, bad: torch.Tensor):
    """dq[s, pi[r], pj[r]] = uint32(trunc(fp32(fp32(1 - sigmoid(logits[r, (s + 3) % 4])) * 1000))) for s = 0..3 (top, right, bottom,
    left).  logits float32 [m, 4], pi / pj int64 [m], dq int32 [4, n, n]; a pair outside [0, n) or with i == j sets bad int32 [1]."""
    _need_gpu(logits, pi, pj, dq, bad)
    m, dev = pi.numel(), dq.device
    n = dq.shape[1]
    for name, t, dtype, shape in (('logits', logits, _f32, (m, 4)), ('pi', pi, _i64, (m,)), ('pj', pj, _i64, (m,)), ('dq', dq, _i32, (4, n, n)),
                                  ('bad', bad, _i32, (1,))):
        _check('puzzle_distances_from_logits', name, t, dtype, shape, dev)
    _lib.call('vited_puzzle_distances_from_logits', _ptr(logits), _ptr(pi), _ptr(pj), m, n, _ptr(dq), _ptr(bad), _stream())


def puzzle_compat_init(dq: torch.Tensor) -> dict:
    """InterPieceDistance.__init__ on the device: a dict of the state tensors (min_d, second_d, candidate, best_buddy, compat,
    mutual, start_count, start_total, start_order) of the distances dq int32 [4, n, n]."""
    _need_gpu(dq)
    n, dev = dq.shape[1], dq.device
    _check('puzzle_compat_init', 'dq', dq, _i32, (4, n, n), dev)
    st = {'min_d': torch.empty((n, 4), dtype=torch.int64, device=dev), 'second_d': torch.empty((n, 4), dtype=torch.int64, device=dev),
          'candidate': torch.empty((n, 4), dtype=torch.int32, device=dev), 'best_buddy': torch.empty((n, 4), dtype=torch.int32, device=dev),
          'compat': torch.empty((4, n, n), dtype=torch.float32, device=dev), 'mutual': torch.empty((4, n, n), dtype=torch.float32, device=dev),
          'start_count': torch.empty(n, dtype=torch.int32, device=dev), 'start_total': torch.empty(n, dtype=torch.float32, device=dev),
          'start_order': torch.empty(n, dtype=torch.int32, device=dev)}
    _lib.call('vited_puzzle_compat_init', _ptr(dq), n, *(_ptr(st[k]) for k in ('min_d', 'second_d', 'candidate', 'best_buddy', 'compat',
                                                                                   'mutual', 'start_count', 'start_total', 'start_order')),
              _stream())
    return st


def puzzle_compat_recalc(dq: torch.Tensor, placed: torch.Tensor, st: dict, changed: torch.Tensor):
    """recalculate_remaining_piece_compatibilities(placed) on the state ``st`` of puzzle_compat_init, in place; changed int32 [n]
    receives 1 for every piece whose min / second-best distances moved.  placed int32 [n] (0 / 1)."""
    _need_gpu(dq, placed, changed, *(st[key] for key in ('min_d', 'second_d', 'compat', 'mutual')))
    op, n, dev = 'puzzle_compat_recalc', dq.shape[1], dq.device
    for name, t, dtype, shape in (('dq', dq, _i32, (4, n, n)), ('placed', placed, _i32, (n,)), ('changed', changed, _i32, (n,)),
                                  ("st['min_d']", st['min_d'], _i64, (n, 4)), ("st['second_d']", st['second_d'], _i64, (n, 4)),
                                  ("st['compat']", st['compat'], _f32, (4, n, n)), ("st['mutual']", st['mutual'], _f32, (4, n, n))):
        _check(op, name, t, dtype, shape, dev)
    _lib.call('vited_puzzle_compat_recalc', _ptr(dq), n, _ptr(placed), _ptr(st['min_d']), _ptr(st['second_d']), _ptr(st['compat']),
              _ptr(st['mutual']), _ptr(changed), _stream())


def puzzle_best_slot(mutual: torch.Tensor, placed: torch.Tensor, slot_piece: torch.Tensor, slot_side: torch.Tensor,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """The packed int64 [1] word of the first maximum of mutual[(slot_side[k] + 2) % 4, p, slot_piece[k]] over unplaced p ascending
    x slot k (see include/vited.h; decode with puzzle_unpack_slot).  placed, slot_piece, slot_side int32."""
    _need_gpu(mutual, placed, slot_piece, slot_side, out)
    op, n, dev, k = 'puzzle_best_slot', mutual.shape[1], mutual.device, slot_piece.numel()
    for name, t, dtype, shape in (('mutual', mutual, _f32, (4, n, n)), ('placed', placed, _i32, (n,)), ('slot_piece', slot_piece, _i32, (k,)),
                                  ('slot_side', slot_side, _i32, (k,))):
        _check(op, name, t, dtype, shape, dev)
    out = _out(op, 'out', out, _i64, (1,), dev)
    _lib.call('vited_puzzle_best_slot', _ptr(mutual), n, _ptr(placed), _ptr(slot_piece), _ptr(slot_side), k, _ptr(out), _stream())
    return out


def puzzle_unpack_slot(word: int, slots: int):
    """(piece, slot index) of a vited_puzzle_best_slot word; None when no piece was unplaced."""
    word &= (1 << 64) - 1
    if word == 0:
        return None
    lin = 0xffffffff - (word & 0xffffffff)
    return lin // slots, lin % slots


# ---- validation metrics of a multi-output binary classifier (include/vited.h) ------------------------------------------------
def cls_metrics_update(logits: torch.Tensor, targets: torch.Tensor, meters: torch.Tensor, last: torch.Tensor, bad: torch.Tensor):
    """One validation batch (main.py:73-93): BCE-with-logits loss, accuracy and macro f1 / precision / recall of pred = logit > 0
    per column, averaged over the columns and added to the device meters as AverageMeter.update(val, n=B) does.

    ``logits`` / ``targets`` [B, C] (1 <= C <= 64) on one device, unit column stride; bf16 / fp16 logits and non-fp32 targets are
    cast to fp32.  ``meters`` fp64 [10]: (sum, count) of loss, acc, f1, precision, recall; ``last`` fp64 [5] receives the batch's
    values; a target other than 0 / 1 sets ``bad`` int32 [1].  One launch, no host sync."""
    _need_gpu(logits, targets, meters, last, bad)
    op, dev = 'cls_metrics_update', meters.device
    if logits.dtype not in _FLOATS:
        raise TypeError(f'cls_metrics_update: logits must be float32 / bfloat16 / float16, got {logits.dtype}')
    if targets.dtype == torch.bool or targets.is_complex():
        raise TypeError(f'cls_metrics_update: targets must be real numbers 0 / 1, got {targets.dtype}')
    logits = _check(op, 'logits', logits.float(), _f32, _ANY2, dev, DENSE_LAST)
    b, c = logits.shape
    if b < 1 or not 1 <= c <= 64:
        raise ValueError(f'cls_metrics_update: logits: need B >= 1 rows and 1 <= C <= 64 columns, got [{b}, {c}]')
    targets = _check(op, 'targets', targets.float(), _f32, (b, c), dev, DENSE_LAST, like='logits')
    for name, t, dtype, size in (('meters', meters, _f64, 10), ('last', last, _f64, 5), ('bad', bad, _i32, 1)):
        _check(op, name, t, dtype, (size,), dev)
    ld = lambda t: t.stride(0) if b > 1 else c
    _lib.call('vited_cls_metrics_update', _ptr(logits), ld(logits), _ptr(targets), ld(targets), b, c, _ptr(meters), _ptr(last), _ptr(bad),
              _stream())


# ---- patch dropout: the wrappers of csrc/patch_keep.hip live in ops_patchdrop.py, on this module's checker and call path ------------
from .ops_patchdrop import (MAX_KEEP_KEYS, keep_from_keys, keep_inverse, patchify_kept, tokens_kept,  # noqa: E402,F401
                            tokens_kept_bwd)

# ---- pooled head: the wrappers of csrc/pool_head.hip live in ops_poolhead.py, on this module's checker and call path ---------------
from .ops_poolhead import POOL_MAX_DIM, token_pool_bwd, token_pool_fwd  # noqa: E402,F401

# ---- elementwise token dropout: the wrapper of csrc/token_dropout.hip and the CPU statement of its mask rule live in ops_tokendrop.py --
from .ops_tokendrop import (TOKEN_DROPOUT_MAX_DIM, dropout_threshold, philox4x32, token_dropout,  # noqa: E402,F401
                            token_dropout_mask)

# ---- device-stepped learning-rate schedule: the wrapper of csrc/lr_schedule.hip and its table layout live in ops_lrsched.py -----------
from .ops_lrsched import LR_MAX_MILESTONES, LR_TABLE_WORDS, lr_schedule_step  # noqa: E402,F401

# ---- learning-rate range test: the wrapper of csrc/lr_finder.hip, its rule in numpy and the suggestion live in ops_lrfinder.py ----------
from .ops_lrfinder import (LRF_DIVERGED, LRF_DONE, LRF_HISTORY_COLS, LRF_NONFINITE, LRF_RUNNING, LRF_STATE_WORDS,  # noqa: E402,F401
                           lr_finder_rate, lr_finder_step, lr_suggestion)

# ---- fused mined-pair loss: the wrapper of csrc/mined_bce.hip lives in ops_minedloss.py ---------------------------------------------
from .ops_minedloss import MINED_BCE_MAX_CLASSES, mined_bce  # noqa: E402,F401

# ---- ranked retrieval lists and the wi19 curve counts: the wrappers of csrc/rank_lists.hip and of the curve record of
# csrc/rank_metrics.hip live in ops_ranklists.py -----------------------------------------------------------------------------------
from .ops_ranklists import TOPK_MAX_K, retrieval_curve_rows, retrieval_topk_rows  # noqa: E402,F401

# ---- classical puzzle baseline: the wrappers of csrc/puzzle_pixels.hip (cut, resize, border distances, board) live in ops_puzzlepixels.py
from .ops_puzzlepixels import (PUZZLE_MAX_ERODED, PUZZLE_MAX_PIECES, PUZZLE_MAX_SIZE, puzzle_assemble, puzzle_cut,  # noqa: E402,F401
                               puzzle_eroded_width, puzzle_pixel_distances, puzzle_resize_pieces)

# ---- type-2 puzzles (pieces of unknown rotation): the wrappers of the *2 entry points of csrc/puzzle_pixels.hip and
# csrc/puzzle_compat.hip live in ops_puzzle2.py ---------------------------------------------------------------------------------------
from .ops_puzzle2 import (puzzle_assemble2, puzzle_best_slot2, puzzle_compat2_init, puzzle_compat2_recalc,  # noqa: E402,F401
                          puzzle_pixel_distances2, puzzle_unpack_slot2)

# ---- learned type-2 puzzles (pieces turned under the pair model): the wrappers of csrc/puzzle_turn.hip and of the turned-pair scatter of
# csrc/puzzle_compat.hip live in ops_puzzlerot.py --------------------------------------------------------------------------------------
from .ops_puzzlerot import patchify_turned, puzzle_distances2_from_logits  # noqa: E402,F401

# ---- mixed-bag and unknown-dimension puzzles: the wrapper of the point lookups of M of csrc/puzzle_compat.hip lives in ops_puzzlemixed.py
from .ops_puzzlemixed import puzzle_mutual_gather  # noqa: E402,F401

# ---- parameter EMA: the wrapper of vited_ema_swap (csrc/optimizer.hip) lives in ops_ema.py ---------------------------------------------
from .ops_ema import ema_swap  # noqa: E402,F401

# matrix-core fp32 attention: predicate, per-thread record and kernel selection (csrc/attention_f32_mfma.hip); ops_f32attn.py
from .ops_f32attn import fp32_attention_kernels, fp32_attention_supported, last_fp32_attention_kernel  # noqa: E402,F401

# ---- 384-column NT products with the weights in registers: the wrapper of vited_gemm_nt_wreg (csrc/gemm_nt_wreg.hip); ops_wreg.py
from .ops_wreg import WREG_WIDTH, gemm_nt_wreg, gemm_nt_wreg_dispatch, gemm_nt_wreg_supported  # noqa: E402,F401

# ---- Pillow-exact resize at any scale: the wrapper of csrc/resample_u8.hip, its tap tables and the rule in numpy live in ops_resample.py
from .ops_resample import (RESAMPLE_MAX_OUT, RESAMPLE_MAX_RATIO, RESAMPLE_MAX_TAPS, ResampleTables, resample_image,  # noqa: E402,F401
                           resample_ksize, resample_tables, resample_taps, resample_u8, window_image)
