"""Functional wrappers over the C ABI: one Python function per entry point of include/vited.h.

These allocate outputs (PyTorch owns every buffer), validate shape/dtype/contiguity BEFORE the
launch and raise on any non-zero status.  They are not autograd-aware; ``functions.py`` composes
them into the encoder / decoder autograd Functions.  Every op launches on torch's current HIP
stream, never synchronises and never allocates on the device side, so the whole forward+backward
is hipGraph-capturable.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from . import _lib
from ._lib import (B_KN, B_NK, BF16, EPI_GELU, EPI_GELU_GRAD, EPI_MUL, EPI_MUL_GELU_GRAD, EPI_RESIDUAL, EPI_STORE, EPI_STORE_F32, F16,
                   F32, I32, I64)

_DTYPE = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16, torch.int32: I32, torch.int64: I64}
_FLOATS = (torch.float32, torch.bfloat16, torch.float16)       # what the ranking and pair-score entries take


def _code(dtype: torch.dtype) -> int:
    """dtype code of an activation (fp32 or bf16)."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f'vited ops support float32 and bfloat16 activations, got {dtype}')
    return _DTYPE[dtype]


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError('vited ops run on the MI355X HIP kernels only: got a CPU tensor '
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


def _rows2d(t: torch.Tensor):
    """(tensor, row stride) of a [rows, dim] view whose last dim is dense."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f'expected a 2-D tensor with a dense last dim, got shape {tuple(t.shape)} stride {t.stride()}')
    return t.stride(0)


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


def _scratch(nbytes: int, device):
    """(pointer, size in bytes) of ``workspace(nbytes, device)``."""
    ws = workspace(nbytes, device)
    return ws.data_ptr(), ws.numel() * 4


# ---------------------------------------------------------------------------------------------
def cast(src: torch.Tensor, dtype: torch.dtype, out: torch.Tensor | None = None) -> torch.Tensor:
    _need_gpu(src, out)
    src = src.contiguous()
    if out is None:
        out = torch.empty_like(src, dtype=dtype)
    assert out.dtype == dtype and out.numel() == src.numel() and out.is_contiguous()
    _lib.call('vited_cast', _ptr(src), _code(src.dtype), _ptr(out), _code(dtype), src.numel(), _stream())
    return out


def scale_rows_cast(src: torch.Tensor, row_scale: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """dst[r, :] = dtype(row_scale[r] * src[r, :]) for fp32 ``src`` [rows, dim] (``vited_scale_rows_cast``)."""
    _need_gpu(src, row_scale)
    rows, dim = src.shape
    _check_row_scale(row_scale, rows)
    assert src.dtype == torch.float32
    out = torch.empty((rows, dim), dtype=dtype, device=src.device)
    _lib.call('vited_scale_rows_cast', _ptr(src), _rows2d(src), _ptr(row_scale), _ptr(out), _code(dtype), dim, rows, dim, _stream())
    return out


def _check_row_scale(row_scale, rows):
    """A drop-path scale vector: fp32, one value per row, contiguous."""
    if row_scale.dtype != torch.float32 or row_scale.dim() != 1 or row_scale.numel() != rows or not row_scale.is_contiguous():
        raise ValueError(f'row scale: expected a contiguous fp32 vector of {rows} rows, got {row_scale.dtype} {tuple(row_scale.shape)}')


def cast_transpose(w: torch.Tensor, dtype: torch.dtype, out: torch.Tensor | None = None) -> torch.Tensor:
    """fp32 [R, C] -> dtype [C, R] (transposed weight shadow)."""
    _need_gpu(w, out)
    assert w.dtype == torch.float32 and w.dim() == 2 and w.is_contiguous()
    if out is None:
        out = torch.empty((w.shape[1], w.shape[0]), dtype=dtype, device=w.device)
    assert out.dtype == dtype and out.shape == (w.shape[1], w.shape[0]) and out.is_contiguous()
    _lib.call('vited_cast_transpose', _ptr(w), _ptr(out), _code(dtype), w.shape[0], w.shape[1], _stream())
    return out


class WeightShadowPlan:
    """Device descriptor table for ``vited_cast_weights``: built once per set of (weight, shadow, transposed
    shadow) buffers, then every refresh is one launch."""

    def __init__(self, entries):
        """entries: iterable of (w fp32 [rows, cols] contiguous, dst bf16 [rows, cols] | None, dst_t bf16 [cols, rows] | None)."""
        rows_, keep, tile = [], [], 0
        for w, dst, dst_t in entries:
            _need_gpu(w, dst, dst_t)
            assert w.dtype == torch.float32 and w.dim() == 2 and w.is_contiguous() and w.data_ptr() % 16 == 0
            r, c = w.shape
            for t, shape in ((dst, (r, c)), (dst_t, (c, r))):
                assert t is None or (t.dtype == torch.bfloat16 and tuple(t.shape) == shape and t.is_contiguous()
                                     and t.data_ptr() % 16 == 0)
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
    assert img.dim() == 4 and img.shape[2] == img.shape[3], 'expected [B, C, S, S]'
    b, c, s, _ = img.shape
    if img.stride()[1:] != (s * s, s, 1):
        img = img.contiguous()
    nb = b
    if batch_index is not None:
        assert batch_index.dtype == torch.int64 and batch_index.is_contiguous()
        nb = batch_index.numel()
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
    s = int(img_size)
    assert regions.dtype == torch.uint8 and regions.dim() == 4 and regions.shape[2] == 2 * s and regions.shape[3] == 3 * s
    b, c = regions.shape[:2]
    if regions.stride()[1:] != (6 * s * s, 3 * s, 1):
        regions = regions.contiguous()
    assert cells.dtype == torch.int32 and cells.shape == (b, 2) and cells.is_contiguous()
    assert erode.dtype == torch.int32 and erode.shape == (b,) and erode.is_contiguous()
    out = torch.empty((b, 2, c, s, s), dtype=torch.uint8, device=regions.device)
    _lib.call('vited_crop_pairs_u8', _ptr(regions), regions.stride(0), _ptr(cells), _ptr(erode), _ptr(out), b, c, s, _stream())
    return out


def _store_args(store: torch.Tensor, img_off: torch.Tensor, img_hw: torch.Tensor) -> int:
    """The resident image store of the feed entry points (``engine.Div2kImageStore``); returns its image count."""
    assert store.dtype == torch.uint8 and store.dim() == 1 and store.is_contiguous()
    assert img_off.dtype == torch.int64 and img_off.dim() == 1 and img_off.is_contiguous()
    assert img_hw.dtype == torch.int32 and img_hw.shape == (img_off.numel(), 2) and img_hw.is_contiguous()
    return img_off.numel()


def _batch_args(b: int, *specs):
    for t, dtype, shape in specs:
        assert t.dtype == dtype and tuple(t.shape) == (b, *shape) and t.is_contiguous(), (t.dtype, tuple(t.shape), dtype, (b, *shape))


def _crop_args(img: torch.Tensor, out: torch.Tensor | None, in_place: bool):
    """(B, S, out) of uint8 crops [B, 3, S, S] and an ``out`` like them (made here when None); it may be ``img`` only with ``in_place``."""
    assert img.dtype == torch.uint8 and img.dim() == 4 and img.shape[1] == 3 and img.shape[2] == img.shape[3] and img.is_contiguous()
    if out is None:
        out = torch.empty_like(img)
    assert out.dtype == torch.uint8 and out.shape == img.shape and out.is_contiguous() and (in_place or out.data_ptr() != img.data_ptr())
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
    s, n, b = int(img_size), _store_args(store, img_off, img_hw), image.numel()
    _batch_args(b, (image, torch.int32, ()), (flags, torch.int32, ()), (minv, torch.float64, (6,)), (rgb, torch.float32, (3,)),
                (crop, torch.int32, (2,)))
    if out is None:
        out = torch.empty((b, 3, 2 * s, 3 * s), dtype=torch.uint8, device=store.device)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (b, 3, 2 * s, 3 * s) and out.is_contiguous()
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
    s, n, b = int(img_size), _store_args(store, img_off, img_hw), image.numel()
    _batch_args(b, (image, torch.int32, ()), (flags, torch.int32, ()), (afix, torch.int64, (6,)), (minv, torch.float64, (6,)),
                (origin, torch.int32, (2,)))
    if out is None:
        out = torch.empty((b, 3, s, s), dtype=torch.uint8, device=store.device)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (b, 3, s, s) and out.is_contiguous()
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
    b, s, out = _crop_args(img, out, in_place=True)
    _batch_args(b, (flags, torch.int32, ()), (order, torch.int32, (4,)), (factors, torch.float32, (3,)), (hue, torch.int32, ()))
    sums = torch.empty(b, dtype=torch.int64, device=img.device)             # the contrast means' L sums; the entry point zeroes them
    _lib.call('vited_hisfrag_jitter_u8', _ptr(img), _ptr(flags), _ptr(order), _ptr(factors), _ptr(hue), _ptr(sums), _ptr(out), b, s, _stream())
    return out


def hisfrag_blur_u8(img: torch.Tensor, flags: torch.Tensor, weights: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """GaussianBlur((3, 3)) on uint8 crops [B, 3, S, S] (``vited_hisfrag_blur_u8``; hisfrag.py:76-78): per sample flag bit 8 (blur on; a
    sample without it is copied) and the 1-D weights (k_edge, k_mid) fp32 [B, 2].  ``out`` must not overlap ``img``."""
    _need_gpu(img, flags, weights, out)
    b, s, out = _crop_args(img, out, in_place=False)
    _batch_args(b, (flags, torch.int32, ()), (weights, torch.float32, (2,)))
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
    s, n, b = int(img_size), _store_args(store, img_off, img_hw), image.numel()
    i32 = torch.int32
    _batch_args(b, (image, i32, ()), (flags, i32, ()), (origin, i32, (2,)), (x0, i32, (s,)), (kx, i32, (s, 3)), (y0, i32, (s,)),
                (ky, i32, (s, 3)), (holes, i32, (16, 4)), (n_holes, i32, ()))
    if out is None:
        out = torch.empty((b, 3, s, s), dtype=torch.uint8, device=store.device)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (b, 3, s, s) and out.is_contiguous()
    _lib.call('vited_michigan_windows_u8', _ptr(store), _ptr(img_off), _ptr(img_hw), n, _ptr(image), _ptr(flags), _ptr(origin), _ptr(x0),
              _ptr(kx), _ptr(y0), _ptr(ky), _ptr(holes), _ptr(n_holes), _ptr(out), b, s, _stream())
    return out


def michigan_blur_gray_u8(img: torch.Tensor, flags: torch.Tensor, weights: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """ImageFilter.GaussianBlur(radius <= 1) and RandomGrayscale on uint8 crops [B, 3, S, S] (``vited_michigan_blur_gray_u8``;
    michigan.py:83-85): per sample flag bit 8 (blur), bit 32 (grey; a sample with neither is copied) and the box-blur weights
    (ww, fw) int32 [B, 2].  ``out`` must not overlap ``img``."""
    _need_gpu(img, flags, weights, out)
    b, s, out = _crop_args(img, out, in_place=False)
    _batch_args(b, (flags, torch.int32, ()), (weights, torch.int32, (2,)))
    _lib.call('vited_michigan_blur_gray_u8', _ptr(img), _ptr(flags), _ptr(weights), _ptr(out), b, s, _stream())
    return out


def slice_rows_cast(x: torch.Tensor, row_offset: int, rows: int, dtype: torch.dtype) -> torch.Tensor:
    """fp32 [B, R, D] -> dtype [B * rows, D] taking rows [row_offset, row_offset + rows) of every batch."""
    _need_gpu(x)
    assert x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()
    b, r, d = x.shape
    out = torch.empty((b * rows, d), dtype=dtype, device=x.device)
    _lib.call('vited_slice_rows_cast', _ptr(x), _ptr(out), _code(dtype), b, r, row_offset, rows, d, _stream())
    return out


def write_cls_row(x: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor):
    """x fp32 [B, R, D]: x[:, 0] = cls + pos[0]."""
    _need_gpu(x, cls, pos)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3
    b, r, d = x.shape
    _lib.call('vited_write_cls_row', _ptr(x), _ptr(cls), _ptr(pos), b, r, d, _stream())


def sum_rows(x: torch.Tensor) -> torch.Tensor:
    """[batch, width] (fp32 or bf16, dense rows) -> fp32 [width] column sums, deterministic."""
    _need_gpu(x)
    ld = _rows2d(x)
    b, w = x.shape
    out = torch.empty(w, dtype=torch.float32, device=x.device)
    ws = _scratch(_lib.load().vited_sum_rows_workspace_bytes(b, w), x.device)
    _lib.call('vited_sum_rows', _ptr(x), _code(x.dtype), ld, _ptr(out), b, w, *ws, _stream())
    return out


# ---------------------------------------------------------------------------------------------
def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out_dtype: torch.dtype, out=None):
    """x fp32 [rows, dim] (row-strided ok) -> (y [rows, dim] out_dtype, mean, rstd).  ``out`` = (y, mean, rstd) pre-made
    (e.g. row slices of larger tensors)."""
    _need_gpu(x, gamma, beta)
    assert x.dtype == torch.float32 and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    ld = _rows2d(x)
    rows, dim = x.shape
    if out is not None:
        y, mean, rstd = out
        assert y.shape == (rows, dim) and y.dtype == out_dtype and _rows2d(y) == dim and mean.numel() == rows and rstd.numel() == rows
    else:
        y = torch.empty((rows, dim), dtype=out_dtype, device=x.device)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
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
    _need_gpu(dy, x, gamma, mean, rstd, dx_in, dx_out, dx_lp, lp_scale)
    dy_ld, x_ld = _rows2d(dy), _rows2d(x)
    rows, dim = x.shape
    assert dy.shape == x.shape and x.dtype == torch.float32
    if dx_out is None:
        dx_out = torch.empty((rows, dim), dtype=torch.float32, device=x.device)
    if lp_scale is not None:
        _check_row_scale(lp_scale, rows)
        want_lp = True
    else:
        lp_dtype = torch.bfloat16
    if want_lp and dx_lp is None:
        dx_lp = torch.empty((rows, dim), dtype=lp_dtype, device=x.device)
    assert dx_lp is None or dx_lp.dtype == lp_dtype
    if dx_in is not None:
        assert dx_in.dtype == torch.float32 and dx_in.shape == x.shape
    accumulate = dgamma is not None
    if accumulate:
        assert dbeta is not None and dgamma.dtype == dbeta.dtype == torch.float32 and dgamma.is_contiguous() and dbeta.is_contiguous()
    else:
        dgamma = torch.empty(dim, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(dim, dtype=torch.float32, device=x.device)
    ws = _scratch(_lib.load().vited_layernorm_bwd_workspace_bytes(rows, dim), x.device)
    head = (_ptr(dy), _code(dy.dtype), dy_ld, _ptr(x), x_ld, _ptr(gamma), _ptr(mean), _ptr(rstd),
            _ptr(dx_in), _rows2d(dx_in) if dx_in is not None else 0, _ptr(dx_out), _rows2d(dx_out),
            _ptr(dx_lp), _code(lp_dtype), _rows2d(dx_lp) if dx_lp is not None else 0)
    tail = (_ptr(dgamma), _ptr(dbeta), int(accumulate), rows, dim, *ws, _stream())
    if lp_scale is not None:
        _lib.call('vited_layernorm_bwd_scaled', *head, _ptr(lp_scale), *tail)
    else:
        _lib.call('vited_layernorm_bwd', *head, *tail)
    return dx_out, dx_lp, dgamma, dbeta


# ---------------------------------------------------------------------------------------------
def _qkn_operand(name, t, heads, like=None):
    """(rows, row stride, head_dim) of a q / k operand of the q/k-norm: [rows, heads * head_dim], dense last dim, any row stride."""
    ld = _rows2d(t)
    if t.shape[1] % heads:
        raise ValueError(f'{name}: {t.shape[1]} columns are not {heads} heads')
    if like is not None and (t.shape != like.shape or t.dtype != like.dtype):
        raise ValueError(f'{name}: {t.dtype} {tuple(t.shape)} does not match {like.dtype} {tuple(like.shape)}')
    return t.shape[0], ld, t.shape[1] // heads


def _qkn_params(hd, *params):
    for p in params:
        assert p.dtype == torch.float32 and p.is_contiguous() and p.numel() == hd, 'q/k-norm parameters are fp32 [head_dim]'


def qk_norm_fwd(q, k, gq, bq, gk, bk, heads: int, eps: float, out=None):
    """q_norm / k_norm of the reference's attention (``qk_norm=True``): LayerNorm over the head_dim elements of every head of every
    row, for q and k in ONE launch (``vited_qk_norm_fwd``).  q, k: [rows, heads * head_dim] fp32 or bf16 with a dense last dim and
    any row stride - column slices of the packed projections - each with its own row count; either may be None (and its
    parameters with it).  gq, bq, gk, bk: fp32 [head_dim].  ``out`` = (q_out | None, k_out | None) pre-made (a slice of a larger
    buffer, or the input itself: in place).
    Returns (q_out, k_out, (q_mean, q_rstd), (k_mean, k_rstd)) - None for an absent operand; the statistics are fp32 [rows, heads]."""
    if q is None and k is None:
        raise ValueError('qk_norm_fwd: neither q nor k given')
    _need_gpu(q, k, gq, bq, gk, bk)
    ref = q if q is not None else k
    dtype, dev = ref.dtype, ref.device
    outs, stats, args, hd = [], [], [], None
    for name, t, g, b, o in (('q', q, gq, bq, out[0] if out else None), ('k', k, gk, bk, out[1] if out else None)):
        if t is None:
            outs.append(None)
            stats.append(None)
            args.append((0, 0, 0, 0, 0, 0, 0, 0, 0))
            continue
        rows, ld, hd_t = _qkn_operand(name, t, heads)
        assert t.dtype == dtype and (hd is None or hd == hd_t), 'q and k share the dtype and the head width'
        hd = hd_t
        _qkn_params(hd, g, b)
        if o is None:
            o = torch.empty((rows, heads * hd), dtype=dtype, device=dev)
        else:
            _need_gpu(o)
            _qkn_operand(name + '_out', o, heads, like=t)
        mean = torch.empty((rows, heads), dtype=torch.float32, device=dev)
        rstd = torch.empty((rows, heads), dtype=torch.float32, device=dev)
        outs.append(o)
        stats.append((mean, rstd))
        args.append((_ptr(t), ld, rows, _ptr(g), _ptr(b), _ptr(o), _rows2d(o), _ptr(mean), _ptr(rstd)))
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
    ref = dq if dq is not None else dk
    dtype, dev = ref.dtype, ref.device
    given = [t is not None for d, pair in ((dq, (dgq, dbq)), (dk, (dgk, dbk))) if d is not None for t in pair]
    accumulate = all(given)
    if any(given) and not accumulate:
        raise ValueError('qk_norm_bwd: give every gradient destination of the present operands, or none')
    args, grads, hd, rows_of = [], [], None, []
    for name, d, x, st, g, dg, db in (('q', dq, q, q_stats, gq, dgq, dbq), ('k', dk, k, k_stats, gk, dgk, dbk)):
        if d is None:
            args.append((0,) * 10)
            grads += [None, None]
            rows_of.append(0)
            continue
        rows, ld, hd_t = _qkn_operand('d' + name, d, heads)
        _qkn_operand(name, x, heads, like=d)
        assert d.dtype == dtype and (hd is None or hd == hd_t), 'q and k share the dtype and the head width'
        hd = hd_t
        mean, rstd = st
        assert mean.shape == rstd.shape == (rows, heads) and mean.dtype == rstd.dtype == torch.float32 and mean.is_contiguous() and rstd.is_contiguous()
        _qkn_params(hd, g)
        if accumulate:
            _qkn_params(hd, dg, db)
        else:
            dg = torch.empty(hd, dtype=torch.float32, device=dev)
            db = torch.empty(hd, dtype=torch.float32, device=dev)
        grads += [dg, db]
        rows_of.append(rows)
        args.append((_ptr(d), ld, _ptr(x), _rows2d(x), _ptr(mean), _ptr(rstd), _ptr(g), _ptr(dg), _ptr(db), rows))
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
    _need_gpu(a, b, bias, aux, residual, out)
    assert a.dtype == b.dtype, f'operand dtypes differ: {a.dtype} vs {b.dtype}'
    lda, ldb = _rows2d(a), _rows2d(b)
    m, k = a.shape
    n = b.shape[0] if b_layout == B_NK else b.shape[1]
    kb = b.shape[1] if b_layout == B_NK else b.shape[0]
    if kb != k:
        raise ValueError(f'contraction mismatch: A is [{m},{k}], B gives K={kb}')
    f32_out = epilogue in (EPI_RESIDUAL, EPI_STORE_F32)
    if out is None:
        rows = m if out_rows is None else out_rows
        out = torch.empty((rows, n), dtype=torch.float32 if f32_out else a.dtype, device=a.device)
    ldo = _rows2d(out)
    if epilogue in (EPI_GELU, EPI_GELU_GRAD):
        if out2 is None:
            out2 = torch.empty_like(out)
        assert out2.dtype == out.dtype and out2.shape == out.shape and _rows2d(out2) == ldo
    else:
        out2 = None
    if aux is not None:
        assert aux.dtype == a.dtype and _rows2d(aux) == ldo
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.stride(-1) == 1
        assert residual.stride(-2) == ldo if residual.dim() >= 2 else True
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == n
    if row_scale is not None:
        _need_gpu(row_scale)
        _check_row_scale(row_scale, m)
        if epilogue != EPI_RESIDUAL or rows_per_batch:
            raise ValueError('row_scale goes with EPI_RESIDUAL and the identity row map')
        assert out.shape[0] == m
        _lib.call('vited_gemm_scaled', _ptr(a), lda, _ptr(b), ldb, b_layout, _code(a.dtype), m, n, k, _ptr(bias), _ptr(residual),
                  _ptr(row_scale), _ptr(out), ldo, _stream())
        return out
    _lib.call('vited_gemm', _ptr(a), lda, _ptr(b), ldb, b_layout, _code(a.dtype), m, n, k, epilogue, _ptr(bias), _ptr(aux), _ptr(residual),
              _ptr(out), _ptr(out2), ldo, rows_per_batch, out_rows_per_batch, row_offset, int(bool(residual_bcast)), _stream())
    return (out, out2) if epilogue in (EPI_GELU, EPI_GELU_GRAD) else out


def linear_bwd_weight(dy: torch.Tensor, x: torch.Tensor, want_bias: bool = True, dw_out=None, db_out=None):
    """dW[N,K] = dy[M,N]^T x[M,K] (fp32), dbias[N] = column sums of dy (fp32) or None.  With ``dw_out``
    (and ``db_out``) the results are ADDED onto those fp32 tensors (a parameter's .grad) instead."""
    _need_gpu(dy, x)
    assert dy.dtype == x.dtype and dy.shape[0] == x.shape[0]
    lddy, ldx = _rows2d(dy), _rows2d(x)
    m, n = dy.shape
    k = x.shape[1]
    accumulate = dw_out is not None
    if accumulate:
        assert dw_out.dtype == torch.float32 and dw_out.is_contiguous() and dw_out.numel() == n * k
        dw, db = dw_out, (db_out if want_bias else None)
        assert db is None or (db.dtype == torch.float32 and db.is_contiguous() and db.numel() == n)
    else:
        dw = torch.empty((n, k), dtype=torch.float32, device=x.device)
        db = torch.empty(n, dtype=torch.float32, device=x.device) if want_bias else None
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
    for dy, x, dw, db in items:
        _need_gpu(dy, x, dw, db)
        if dy.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 or dy.shape[0] != x.shape[0]:
            return False
        assert dw.dtype == torch.float32 and dw.is_contiguous() and dw.numel() == dy.shape[1] * x.shape[1]
        assert db is None or (db.dtype == torch.float32 and db.is_contiguous() and db.numel() == dy.shape[1])
        if dw.data_ptr() % 16 or (db is not None and db.data_ptr() % 16) or dy.data_ptr() % 16 or x.data_ptr() % 16:
            return False                 # the batched kernels use 16-byte accesses throughout
    dys, xs, dws, dbs = zip(*items)
    M = _host_array(C.c_int64, [dy.shape[0] for dy in dys])
    N = _host_array(C.c_int64, [dy.shape[1] for dy in dys])
    K = _host_array(C.c_int64, [x.shape[1] for x in xs])
    lib = _lib.load()
    if not lib.vited_linear_bwd_weight_batched_supported(n, M, N, K, BF16):
        return False
    lddy, ldx = _host_array(C.c_int64, map(_rows2d, dys)), _host_array(C.c_int64, map(_rows2d, xs))
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
    assert a.dtype == w.dtype == torch.bfloat16 and residual.dtype == torch.float32
    lda, ldw, ldr = _rows2d(a), _rows2d(w), _rows2d(residual)
    m, k = a.shape
    n = w.shape[0]
    assert w.shape[1] == k and residual.shape == (m, n)
    y = out if out is not None else torch.empty((m, n), dtype=torch.float32, device=a.device)
    assert y.dtype == torch.float32 and y.shape == (m, n)
    h = mean = rstd = None
    if gamma is not None:
        h = torch.empty((m, n), dtype=torch.bfloat16, device=a.device)
        mean = torch.empty(m, dtype=torch.float32, device=a.device)
        rstd = torch.empty(m, dtype=torch.float32, device=a.device)
    tail = (_ptr(y), _rows2d(y), _ptr(gamma), _ptr(beta), float(eps), _ptr(h), n, _ptr(mean), _ptr(rstd), m, n, k, _stream())
    if row_scale is not None:
        _check_row_scale(row_scale, m)
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
    _need_gpu(dy, wt, x, gamma, mean, rstd, dx_in, dx_out, lp_scale)
    assert dy.dtype == wt.dtype == torch.bfloat16 and x.dtype == torch.float32
    segments = 1
    if dy.dim() == 3:
        # [L, M, seg_k]: the contraction dim arrives as L tensors (one per decoder block), wt is [N, L * seg_k]
        assert dy.stride(2) == 1 and dy.stride(0) % 8 == 0
        segments, m, seg_k = dy.shape
        lddy, seg_stride, k = dy.stride(1), dy.stride(0), segments * seg_k
    else:
        lddy = _rows2d(dy)
        m, k = dy.shape
    ldwt, ldx = _rows2d(wt), _rows2d(x)
    n = wt.shape[0]
    assert wt.shape[1] == k and x.shape == (m, n)
    lib = _lib.load()
    if dx_out is None:
        dx_out = torch.empty((m, n), dtype=torch.float32, device=x.device)
    if lp_scale is not None:
        _check_row_scale(lp_scale, m)
        assert segments == 1
        want_lp = True
    dx_lp = torch.empty((m, n), dtype=torch.bfloat16, device=x.device) if want_lp else None
    accumulate = dgamma is not None
    if accumulate:
        assert dbeta is not None and dgamma.dtype == dbeta.dtype == torch.float32 and dgamma.is_contiguous() and dbeta.is_contiguous()
    else:
        dgamma = torch.empty(n, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(n, dtype=torch.float32, device=x.device)
    if defer is not None:
        rows = int(lib.vited_linear_layernorm_bwd_partial_rows(m))
        part = torch.empty(rows * 2 * n, dtype=torch.float32, device=x.device)     # lives until the flush
        defer.append((part, rows, dgamma, dbeta, accumulate))
        ws = (part.data_ptr(), part.numel() * 4)
    else:
        ws = _scratch(lib.vited_linear_layernorm_bwd_workspace_bytes(m, n), x.device)
    dx_args = (_ptr(x), ldx, _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dx_in), _rows2d(dx_in) if dx_in is not None else 0, _ptr(dx_out),
               _rows2d(dx_out), _ptr(dx_lp), n)
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
    _lib.call('vited_layernorm_bwd_finish_batched', len(entries), _host_array(C.c_void_p, parts), _host_array(C.c_int, rows),
              _host_array(C.c_void_p, dgammas), _host_array(C.c_void_p, dbetas), _host_array(C.c_int, map(int, accumulate)),
              dgammas[0].numel(), _stream())
    entries.clear()


# ---------------------------------------------------------------------------------------------
MAX_FOLDED_BLOCKS = 16


def fold_context_weights(ws, biases, gammas, betas, out=None):
    """Folded kv weights of several decoder blocks: W'_l = W_l o gamma_l (bf16, stacked [L N, K] and transposed [K, L N]) and
    b'_l = b_l + W_l beta_l (fp32 [L N]) - ``vited_fold_context_weights``.  ``out`` = (w, wt, b) buffers to refresh in place."""
    n_blk = len(ws)
    _need_gpu(*ws, *gammas, *betas)
    n, k = ws[0].shape
    dev = ws[0].device
    if out is None:
        out = (torch.empty((n_blk * n, k), dtype=torch.bfloat16, device=dev), torch.empty((k, n_blk * n), dtype=torch.bfloat16, device=dev),
               torch.empty(n_blk * n, dtype=torch.float32, device=dev))
    for t in list(ws) + list(gammas) + list(betas):
        assert t.dtype == torch.float32 and t.is_contiguous()
    _lib.call('vited_fold_context_weights', n_blk, *(_host_array(C.c_void_p, ts) for ts in (ws, biases, gammas, betas)), n, k,
              _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream())
    return out


def unfold_context_grads(dwf, dbf, ws, gammas, betas, dws, dbiases, dgammas, dbetas, accumulate: bool):
    """Gradients of the folded weights / bias -> dW_l, db_l, dgamma_l, dbeta_l (``vited_unfold_context_grads``)."""
    n_blk = len(ws)
    n, k = ws[0].shape
    assert dwf.dtype == dbf.dtype == torch.float32 and dwf.is_contiguous() and dbf.is_contiguous()
    assert dwf.shape == (n_blk * n, k) and dbf.numel() == n_blk * n
    _lib.call('vited_unfold_context_grads', n_blk, _ptr(dwf), _ptr(dbf),
              *(_host_array(C.c_void_p, ts) for ts in (ws, gammas, betas, dws, dbiases, dgammas, dbetas)), n, k, int(bool(accumulate)),
              _stream())


# ---------------------------------------------------------------------------------------------
def mlp_fwd(x, gamma, beta, w1, b1, w2, b2, eps: float, save: bool = True, out=None):
    """y = x + fc2(gelu(fc1(LayerNorm(x)))) in one kernel (``vited_mlp_fwd``).  x fp32 [rows, 384]; w1 / w2 the bf16 weights.
    Returns (y, saved) with saved = (mean, rstd, h, gd, u) or None.  ``out`` = (y, mean, rstd, h, gd, u) pre-made outputs
    (row slices of larger tensors are fine for y; the others must be dense)."""
    _need_gpu(x, gamma, beta, w1, b1, w2, b2)
    assert x.dtype == torch.float32 and w1.dtype == w2.dtype == torch.bfloat16 and w1.is_contiguous() and w2.is_contiguous()
    ldx = _rows2d(x)
    rows, dim = x.shape
    hidden = w1.shape[0]
    assert w1.shape == (hidden, dim) and w2.shape == (dim, hidden)
    dev = x.device
    if out is not None:
        y, mean, rstd, h, gd, u = out
    else:
        y = torch.empty((rows, dim), dtype=torch.float32, device=dev)
        mean = rstd = h = gd = u = None
        if save:
            mean = torch.empty(rows, dtype=torch.float32, device=dev)
            rstd = torch.empty(rows, dtype=torch.float32, device=dev)
            h = torch.empty((rows, dim), dtype=torch.bfloat16, device=dev)
            gd = torch.empty((rows, hidden), dtype=torch.bfloat16, device=dev)
            u = torch.empty((rows, hidden), dtype=torch.bfloat16, device=dev)
    if save:
        assert h.is_contiguous() and gd.is_contiguous() and u.is_contiguous() and h.shape == (rows, dim) and gd.shape == u.shape == (rows, hidden)
    _lib.call('vited_mlp_fwd', _ptr(x), ldx, _ptr(gamma), _ptr(beta), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(y), _rows2d(y),
              _ptr(h) if save else 0, _ptr(gd) if save else 0, _ptr(u) if save else 0, _ptr(mean) if save else 0, _ptr(rstd) if save else 0,
              rows, dim, hidden, float(eps), _stream())
    return y, ((mean, rstd, h, gd, u) if save else None)


def block_fwd(x, heads: int, ln1_g, ln1_b, wqkv, bqkv, wproj, bproj, ln2_g, ln2_b, w1, b1, w2, b2, eps: float = 1e-6):
    """Encoder Block forward through ``vited_block_fwd``: x fp32 [B, N, D] -> y fp32 [B, N, D] (bf16 weights, inference form).
    The whole-block entry has no q/k-norm: a ``qk_norm=True`` model runs its blocks through functions.py (``qk_norm_fwd``)."""
    _need_gpu(x, wqkv, wproj, w1, w2)
    assert x.dtype == torch.float32 and x.dim() == 3 and x.is_contiguous()
    assert all(t.dtype == torch.bfloat16 and t.is_contiguous() for t in (wqkv, wproj, w1, w2))
    b, n, d = x.shape
    hidden = w1.shape[0]
    y = torch.empty_like(x)
    ws, nbytes = _scratch(_lib.load().vited_block_workspace_bytes(b, n, d, hidden, heads) + 256, x.device)
    base = (ws + 255) // 256 * 256
    _lib.call('vited_block_fwd', _ptr(x), _ptr(y), b, n, d, heads, hidden, _ptr(ln1_g), _ptr(ln1_b), _ptr(wqkv), _ptr(bqkv), _ptr(wproj),
              _ptr(bproj), _ptr(ln2_g), _ptr(ln2_b), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), float(eps), base, nbytes - (base - ws),
              _stream())
    return y


def cross_block_fwd(x, context, heads: int, ln1, wqkv, bqkv, wproj, bproj, lnq, lnc, wq, bq, wkv, bkv, wcproj, bcproj, ln2, w1, b1, w2, b2,
                    eps: float = 1e-6):
    """Decoder CrossBlock forward through ``vited_cross_block_fwd``: x fp32 [B, N2, D], context fp32 [B, N1, D] -> y fp32 [B, N2, D]
    (bf16 weights, inference form).  ln1 / lnq / lnc / ln2 = (gamma, beta) of norm1 / norm_cross / norm_context / norm2.
    The whole-block entry has no q/k-norm: a ``qk_norm=True`` model runs its blocks through functions.py (``qk_norm_fwd``)."""
    _need_gpu(x, context, wqkv, wproj, wq, wkv, wcproj, w1, w2)
    assert x.dtype == context.dtype == torch.float32 and x.dim() == context.dim() == 3 and x.is_contiguous() and context.is_contiguous()
    assert all(t.dtype == torch.bfloat16 and t.is_contiguous() for t in (wqkv, wproj, wq, wkv, wcproj, w1, w2))
    b, n, d = x.shape
    nc = context.shape[1]
    assert context.shape == (b, nc, d)
    hidden = w1.shape[0]
    y = torch.empty_like(x)
    ws, nbytes = _scratch(_lib.load().vited_cross_block_workspace_bytes(b, n, nc, d, hidden, heads) + 256, x.device)
    base = (ws + 255) // 256 * 256
    _lib.call('vited_cross_block_fwd', _ptr(x), _ptr(context), _ptr(y), b, n, nc, d, heads, hidden, _ptr(ln1[0]), _ptr(ln1[1]), _ptr(wqkv),
              _ptr(bqkv), _ptr(wproj), _ptr(bproj), _ptr(lnq[0]), _ptr(lnq[1]), _ptr(lnc[0]), _ptr(lnc[1]), _ptr(wq), _ptr(bq), _ptr(wkv),
              _ptr(bkv), _ptr(wcproj), _ptr(bcproj), _ptr(ln2[0]), _ptr(ln2[1]), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), float(eps), base,
              nbytes - (base - ws), _stream())
    return y


# ---------------------------------------------------------------------------------------------
def _head_view(t: torch.Tensor, heads: int, head_dim: int):
    """t is [B, N, heads*head_dim] (a last-dim slice of the packed projection): (ptr-holder, bs, ts)."""
    assert t.dim() == 3 and t.stride(2) == 1 and t.shape[2] == heads * head_dim
    return t.stride(0), t.stride(1)


def attention_fwd(q, k, v, heads: int, scale: float, kv_index=None):
    """q [B,Nq,D], k/v [B,Nk,D] (strided views of the packed qkv / kv projections are fine)
    -> (o [B,Nq,D] contiguous, lse fp32 [B,H,Nq]).  With ``kv_index`` (int64 [B]) batch item b attends over
    k[kv_index[b]] / v[kv_index[b]] and k / v may hold any number of items (inference only)."""
    _need_gpu(q, k, v, kv_index)
    b, nq, d = q.shape
    nk = k.shape[1]
    hd = d // heads
    assert q.dtype == k.dtype == v.dtype and k.shape == v.shape and k.shape[2] == d
    if kv_index is None:
        assert k.shape[0] == b
    else:
        assert kv_index.dtype == torch.int64 and kv_index.is_contiguous() and kv_index.numel() == b
    q_bs, q_ts = _head_view(q, heads, hd)
    k_bs, k_ts = _head_view(k, heads, hd)
    v_bs, v_ts = _head_view(v, heads, hd)
    o = torch.empty((b, nq, d), dtype=q.dtype, device=q.device)
    lse = torch.empty((b, heads, nq), dtype=torch.float32, device=q.device)
    _lib.call('vited_attention_fwd_indexed', _ptr(q), q_bs, q_ts, _ptr(k), k_bs, k_ts, _ptr(v), v_bs, v_ts, _ptr(kv_index), _ptr(o), nq * d,
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
    for name, t, dtype in (('targets', targets, torch.int64), ('keys', keys, torch.float32)):
        if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != 1:
            raise ValueError(f'mine_pairs: {name} must be a 1-D {dtype} tensor, got '
                             f'{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}')
        if not t.is_contiguous():
            raise ValueError(f'mine_pairs: {name} must be contiguous, got strides {t.stride()}')
    n = targets.numel()
    if n < 1:
        raise ValueError('mine_pairs: no images')
    if keys.numel() != n * n:
        raise ValueError(f'mine_pairs: {keys.numel()} keys for {n} images, expected one per ordered cell: {n * n}')
    if keys.device != targets.device:
        raise ValueError(f'mine_pairs: keys on {keys.device}, targets on {targets.device}')
    neg_per_pos, capacity = float(neg_per_pos), int(capacity)
    if not 0.0 <= neg_per_pos < float('inf'):
        raise ValueError(f'mine_pairs: neg_per_pos must be a finite number >= 0, got {neg_per_pos}')
    if capacity < 1:
        raise ValueError(f'mine_pairs: capacity must be at least 1, got {capacity}')
    if not targets.is_cuda:
        raise ValueError('mine_pairs: the kernel takes device tensors (engine.mine_pairs_device restates the rule for CPU tensors)')
    if n > mine_pairs_max_images():
        raise ValueError(f'mine_pairs: {n} images, the kernel takes at most {mine_pairs_max_images()}')
    if capacity > MINE_MAX_CAPACITY:
        raise ValueError(f'mine_pairs: capacity {capacity} above the {MINE_MAX_CAPACITY} rows the kernel supports')
    return n, neg_per_pos, capacity


def mine_pairs_out(targets, keys, neg_per_pos, ordered_negatives, groups, labels, weights, seg_index, seg_order, seg_offsets, counts):
    """``mine_pairs`` into the caller's buffers (every element of every one is written): groups int64 [capacity, 2], labels /
    weights fp32 [capacity, 1], seg_index / seg_order int64 [capacity], seg_offsets int64 [n + 1], counts int32 [5]."""
    n, neg_per_pos, capacity = _mine_pairs_args(targets, keys, neg_per_pos, groups.shape[0] if torch.is_tensor(groups) and groups.dim() else 0)
    for name, t, dtype, shape in (('groups', groups, torch.int64, (capacity, 2)), ('labels', labels, torch.float32, (capacity, 1)),
                                  ('weights', weights, torch.float32, (capacity, 1)), ('seg_index', seg_index, torch.int64, (capacity,)),
                                  ('seg_order', seg_order, torch.int64, (capacity,)), ('seg_offsets', seg_offsets, torch.int64, (n + 1,)),
                                  ('counts', counts, torch.int32, (5,))):
        if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != targets.device:
            raise ValueError(f'mine_pairs: {name} must be a contiguous {dtype} tensor of shape {shape} on {targets.device}')
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
    b, nq, d = q.shape
    nk = k.shape[1]
    hd = d // heads
    assert o.is_contiguous() and do.is_contiguous() and o.dtype == do.dtype == q.dtype
    if segments is None and kv_index is not None:
        segments = pair_segments(kv_index, k.shape[0])
    if segments is not None:
        return _attention_bwd_indexed(q, k, v, o, do, lse, heads, scale, dq, dk, dv, kv_index, segments)
    q_bs, q_ts = _head_view(q, heads, hd)
    k_bs, k_ts = _head_view(k, heads, hd)
    v_bs, v_ts = _head_view(v, heads, hd)
    dq_bs, dq_ts = _head_view(dq, heads, hd)
    dk_bs, dk_ts = _head_view(dk, heads, hd)
    dv_bs, dv_ts = _head_view(dv, heads, hd)
    delta = torch.empty((b, heads, nq), dtype=torch.float32, device=q.device)
    _lib.call('vited_attention_bwd',
              _ptr(q), q_bs, q_ts, _ptr(k), k_bs, k_ts, _ptr(v), v_bs, v_ts, _ptr(o), _ptr(do), nq * d, d, _ptr(lse), _ptr(delta),
              _ptr(dq), dq_bs, dq_ts, _ptr(dk), dk_bs, dk_ts, _ptr(dv), dv_bs, dv_ts, _code(q.dtype), b, heads, nq, nk, hd,
              float(scale), _stream())
    return dq, dk, dv


def _attention_bwd_indexed(q, k, v, o, do, lse, heads, scale, dq, dk, dv, kv_index, seg):
    if not isinstance(seg, PairSegments):
        raise TypeError(f'attention_bwd: segments must be a PairSegments (ops.pair_segments), got {type(seg).__name__}')
    b, nq, d = q.shape
    items, nk = k.shape[0], k.shape[1]
    hd = d // heads
    if kv_index is not None and kv_index is not seg.index and not torch.equal(kv_index.to(seg.index.device), seg.index):
        raise ValueError('attention_bwd: kv_index and segments.index differ')
    for name, t, size in (('index', seg.index, b), ('order', seg.order, b), ('offsets', seg.offsets, items + 1)):
        if t.dtype != torch.int64 or t.dim() != 1 or t.numel() != size or not t.is_contiguous() or t.device != q.device:
            raise ValueError(f'attention_bwd: segments.{name} must be a contiguous int64 [{size}] tensor on {q.device}, got {t.dtype} '
                             f'{tuple(t.shape)} on {t.device} ({b} pairs over {items} key/value items)')
    assert q.dtype == k.dtype == v.dtype == dq.dtype == dk.dtype == dv.dtype
    assert k.shape == v.shape == dk.shape == dv.shape and k.shape[2] == d and dq.shape == q.shape
    q_bs, q_ts = _head_view(q, heads, hd)
    k_bs, k_ts = _head_view(k, heads, hd)
    v_bs, v_ts = _head_view(v, heads, hd)
    dq_bs, dq_ts = _head_view(dq, heads, hd)
    dk_bs, dk_ts = _head_view(dk, heads, hd)
    dv_bs, dv_ts = _head_view(dv, heads, hd)
    delta = torch.empty((b, heads, nq), dtype=torch.float32, device=q.device)
    nbytes = _lib.load().vited_attention_bwd_indexed_workspace_bytes(_code(q.dtype), b, heads, nk, hd)
    if nbytes < 0:
        raise ValueError(f'attention_bwd: empty operands (B {b}, heads {heads}, Nk {nk}, head_dim {hd})')
    ws, ws_bytes = _scratch(nbytes + 16, q.device)
    base = (ws + 15) // 16 * 16
    _lib.call('vited_attention_bwd_indexed',
              _ptr(q), q_bs, q_ts, _ptr(k), k_bs, k_ts, _ptr(v), v_bs, v_ts, _ptr(seg.index), _ptr(seg.order), _ptr(seg.offsets), items,
              _ptr(o), _ptr(do), nq * d, d, _ptr(lse), _ptr(delta), _ptr(dq), dq_bs, dq_ts, _ptr(dk), dk_bs, dk_ts, _ptr(dv), dv_bs, dv_ts,
              _code(q.dtype), b, heads, nq, nk, hd, float(scale), base, ws_bytes - (base - ws), _stream())
    return dq, dk, dv


CAM_GRAD, CAM_PROB = 0, 1          # VITED_CAM_GRAD / VITED_CAM_PROB
_CAM_MODES = {'grad': CAM_GRAD, 'prob': CAM_PROB, CAM_GRAD: CAM_GRAD, CAM_PROB: CAM_PROB}


def _cam_operand(name, t, heads, like=None):
    if t.dim() != 3 or t.stride(2) != 1 or t.shape[2] % heads:
        raise ValueError(f'attention_cam: {name} must be [B, N, heads*head_dim] with a dense last dim, got shape {tuple(t.shape)} '
                         f'stride {t.stride()} for {heads} heads')
    if like is not None and (t.dtype != like.dtype or t.device != like.device or t.shape[0] != like.shape[0] or t.shape[2] != like.shape[2]):
        raise ValueError(f'attention_cam: {name} {tuple(t.shape)} {t.dtype} does not match q {tuple(like.shape)} {like.dtype}')
    return t.stride(0), t.stride(1)


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
    if heads <= 0:
        raise ValueError(f'attention_cam: heads must be positive, got {heads}')
    q_bs, q_ts = _cam_operand('q', q, heads)
    k_bs, k_ts = _cam_operand('k', k, heads, q)
    v_bs, v_ts = _cam_operand('v', v, heads, q) if v is not None else (0, 0)
    do_bs, do_ts = _cam_operand('do', do, heads, q) if do is not None else (0, 0)
    b, nq, d = q.shape
    nk = k.shape[1]
    if v is not None and v.shape[1] != nk:
        raise ValueError(f'attention_cam: v has {v.shape[1]} tokens, k has {nk}')
    if do is not None and do.shape[1] != nq:
        raise ValueError(f'attention_cam: do has {do.shape[1]} tokens, q has {nq}')
    if b == 0 or nq == 0 or nk == 0:
        raise ValueError(f'attention_cam: empty operands (B {b}, Nq {nq}, Nk {nk})')
    if lse.dtype != torch.float32 or tuple(lse.shape) != (b, heads, nq) or not lse.is_contiguous():
        raise ValueError(f'attention_cam: lse must be contiguous float32 [{b}, {heads}, {nq}], got {tuple(lse.shape)} {lse.dtype}')
    if head_weight is not None and (head_weight.dtype != torch.float32 or tuple(head_weight.shape) != (b, heads) or not head_weight.is_contiguous()):
        raise ValueError(f'attention_cam: head_weight must be contiguous float32 [{b}, {heads}], got {tuple(head_weight.shape)} {head_weight.dtype}')
    if out is None:
        out = torch.empty((b, nq, nk), dtype=torch.float32, device=q.device)
    elif (out.dtype != torch.float32 or out.dim() != 3 or out.shape[0] != b or out.shape[1] != nq or out.shape[2] < nk or out.stride(2) != 1
          or out.stride(1) < nk or out.device != q.device):
        raise ValueError(f'attention_cam: out must be float32 [{b}, {nq}, >= {nk}] with a dense last dim, got {tuple(out.shape)} '
                         f'stride {out.stride()} {out.dtype}')
    _lib.call('vited_attention_cam', _ptr(q), q_bs, q_ts, _ptr(k), k_bs, k_ts, _ptr(v), v_bs, v_ts, _ptr(do), do_bs, do_ts, _ptr(lse),
              _ptr(head_weight), _ptr(out), out.stride(0), out.stride(1), mode, _code(q.dtype), b, heads, nq, nk, d // heads,
              float(scale), _stream())
    return out[:, :, :nk] if out.shape[2] != nk else out


def last_paths():
    lib = _lib.load()
    return lib.vited_last_gemm_path(), lib.vited_last_attention_path()


# ---------------------------------------------------------------------------------------------
# evaluation: retrieval metrics of a distance matrix (misc/wi19_evaluate.get_metrics)
# ---------------------------------------------------------------------------------------------
def _int32_vector(name, t, device, size=None):
    if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or (size is not None and t.numel() != size):
        raise ValueError(f'{name} must be a contiguous int32 vector{f" of length {size}" if size else ""}, '
                         f'got {t.dtype} of shape {tuple(t.shape)}')
    if t.device != device:
        raise ValueError(f'{name} is on {t.device}, the matrix on {device}')


def _ranking_args(what, matrix, labels, rows):
    """(dtype code, ld, n, r0, r1) of the [n, n] matrix a ranking-metrics entry takes, after the checks both entries share."""
    if matrix.dtype not in _FLOATS:
        raise TypeError(f'{what} metrics take float32, bfloat16 or float16 matrices, got {matrix.dtype}')
    if matrix.dim() != 2 or matrix.shape[0] != matrix.shape[1]:
        raise ValueError(f'expected a square [n, n] matrix, got shape {tuple(matrix.shape)}')
    ld = _rows2d(matrix)
    n = matrix.shape[0]
    _int32_vector('labels', labels, matrix.device, n)
    r0, r1 = int(rows[0]), int(rows[1])
    if not 0 <= r0 < r1 <= n:
        raise ValueError(f'rows ({r0}, {r1}) is not a non-empty range inside [0, {n})')
    return _DTYPE[matrix.dtype], ld, n, r0, r1


def retrieval_metrics_rows(matrix: torch.Tensor, labels: torch.Tensor, offsets: torch.Tensor, members: torch.Tensor,
                           rows: tuple[int, int], *, remove_self_column: bool = True, from_similarity: bool = False):
    """Row records (float64 [r1 - r0, 5]: AP sum, correct retrievals, top-1 hit, hits in the first 10, in the first 100) and
    their sums (float64 [7], see include/vited.h) for the rows [r0, r1) of the [n, n] matrix.  ``labels`` int32 [n] in
    [0, C) with the class CSR ``offsets`` int32 [C + 1] / ``members`` int32 [n] built from them (engine.class_members)."""
    _need_gpu(matrix, labels, offsets, members)
    dt, ld, n, r0, r1 = _ranking_args('retrieval', matrix, labels, rows)
    _int32_vector('members', members, matrix.device, n)
    _int32_vector('offsets', offsets, matrix.device)
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
    dt, ld, n, r0, r1 = _ranking_args('group retrieval', matrix, labels, rows)
    num_labels = col_csr[0].numel() - 1
    for name, (off, vals) in (('col', col_csr), ('pos', pos_csr)) + ((('neg', neg_csr),) if neg_csr is not None else ()):
        _int32_vector(f'{name} offsets', off, matrix.device, num_labels + 1)
        _int32_vector(f'{name} members', vals, matrix.device)
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


def pair_scores_add(pairs: torch.Tensor, scores: torch.Tensor, n: int, counts: torch.Tensor, rec_cells: torch.Tensor,
                    rec_values: torch.Tensor, bad: torch.Tensor):
    """Stores the records (pairs[r, 0], pairs[r, 1], 1 - scores[r]) into rec_cells int32 [m, 2] / rec_values float32 [m] and
    counts them into counts int32 [n, n] (both cells (i, j) and (j, i)).  Ids outside [0, n) set bit 0 of bad int32 [1]."""
    _need_gpu(pairs, scores, counts, rec_cells, rec_values, bad)
    if pairs.dtype not in (torch.int32, torch.int64) or pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError(f'pairs must be int32 / int64 [m, 2], got {pairs.dtype} of shape {tuple(pairs.shape)}')
    if pairs.stride(1) != 1:
        pairs = pairs.contiguous()
    if scores.dtype not in _FLOATS or scores.dim() != 1 or scores.numel() != pairs.shape[0]:
        raise ValueError(f'scores must be a float32 / bfloat16 / float16 vector of {pairs.shape[0]}, '
                         f'got {scores.dtype} of shape {tuple(scores.shape)}')
    scores = scores.contiguous()
    m = pairs.shape[0]
    for name, t, dtype, shape in (('counts', counts, torch.int32, (n, n)), ('rec_cells', rec_cells, torch.int32, (m, 2)),
                                  ('rec_values', rec_values, torch.float32, (m,)), ('bad', bad, torch.int32, (1,))):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != pairs.device:
            raise ValueError(f'{name} must be contiguous {dtype} {shape} on {pairs.device}, got {t.dtype} {tuple(t.shape)} on {t.device}')
    if m == 0:
        return
    _lib.call('vited_pair_scores_add', _ptr(pairs), _DTYPE[pairs.dtype], pairs.stride(0), _ptr(scores), _DTYPE[scores.dtype], m, n,
              _ptr(counts), _ptr(rec_cells), _ptr(rec_values), _ptr(bad), _stream())


def pair_scores_finish(rec_cells: torch.Tensor, rec_values: torch.Tensor, n: int, counts: torch.Tensor, bad: torch.Tensor):
    """(mean float32 [n, n], min float32 [n, n], stdev float64 [n, n], stats float64 [2] = (avg_std, std_std)) of every stored
    record; see include/vited.h."""
    _need_gpu(rec_cells, rec_values, counts, bad)
    m = rec_values.numel()
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
def _puzzle_check(name, t, dtype, shape, dev):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != dev:
        raise ValueError(f'{name} must be contiguous {dtype} {tuple(shape)} on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}')


def puzzle_distances_from_logits(logits: torch.Tensor, pi: torch.Tensor, pj: torch.Tensor, dq: torch.Tensor, bad: torch.Tensor):
    """dq[s, pi[r], pj[r]] = uint32(trunc(fp32(fp32(1 - sigmoid(logits[r, (s + 3) % 4])) * 1000))) for s = 0..3 (top, right, bottom,
    left).  logits float32 [m, 4], pi / pj int64 [m], dq int32 [4, n, n]; a pair outside [0, n) or with i == j sets bad int32 [1]."""
    _need_gpu(logits, pi, pj, dq, bad)
    m, dev = pi.numel(), dq.device
    n = dq.shape[1]
    _puzzle_check('logits', logits, torch.float32, (m, 4), dev)
    _puzzle_check('pi', pi, torch.int64, (m,), dev)
    _puzzle_check('pj', pj, torch.int64, (m,), dev)
    _puzzle_check('dq', dq, torch.int32, (4, n, n), dev)
    _puzzle_check('bad', bad, torch.int32, (1,), dev)
    _lib.call('vited_puzzle_distances_from_logits', _ptr(logits), _ptr(pi), _ptr(pj), m, n, _ptr(dq), _ptr(bad), _stream())


def puzzle_compat_init(dq: torch.Tensor) -> dict:
    """InterPieceDistance.__init__ on the device: a dict of the state tensors (min_d, second_d, candidate, best_buddy, compat,
    mutual, start_count, start_total, start_order) of the distances dq int32 [4, n, n]."""
    _need_gpu(dq)
    n, dev = dq.shape[1], dq.device
    _puzzle_check('dq', dq, torch.int32, (4, n, n), dev)
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
    _need_gpu(dq, placed, changed)
    n, dev = dq.shape[1], dq.device
    _puzzle_check('dq', dq, torch.int32, (4, n, n), dev)
    _puzzle_check('placed', placed, torch.int32, (n,), dev)
    _puzzle_check('changed', changed, torch.int32, (n,), dev)
    _lib.call('vited_puzzle_compat_recalc', _ptr(dq), n, _ptr(placed), _ptr(st['min_d']), _ptr(st['second_d']), _ptr(st['compat']),
              _ptr(st['mutual']), _ptr(changed), _stream())


def puzzle_best_slot(mutual: torch.Tensor, placed: torch.Tensor, slot_piece: torch.Tensor, slot_side: torch.Tensor,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """The packed int64 [1] word of the first maximum of mutual[(slot_side[k] + 2) % 4, p, slot_piece[k]] over unplaced p ascending
    x slot k (see include/vited.h; decode with puzzle_unpack_slot).  placed, slot_piece, slot_side int32."""
    _need_gpu(mutual, placed, slot_piece, slot_side)
    n, dev, k = mutual.shape[1], mutual.device, slot_piece.numel()
    _puzzle_check('mutual', mutual, torch.float32, (4, n, n), dev)
    _puzzle_check('placed', placed, torch.int32, (n,), dev)
    _puzzle_check('slot_piece', slot_piece, torch.int32, (k,), dev)
    _puzzle_check('slot_side', slot_side, torch.int32, (k,), dev)
    out = torch.empty(1, dtype=torch.int64, device=dev) if out is None else out
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
    dev = meters.device
    if logits.dim() != 2 or tuple(targets.shape) != tuple(logits.shape):
        raise ValueError(f'logits and targets must be [B, C] of the same shape, got {tuple(logits.shape)} and {tuple(targets.shape)}')
    b, c = logits.shape
    if b < 1 or not 1 <= c <= 64:
        raise ValueError(f'need B >= 1 rows and 1 <= C <= 64 columns, got [{b}, {c}]')
    if logits.device != dev or targets.device != dev:
        raise ValueError(f'logits ({logits.device}) and targets ({targets.device}) must be on the meters\' device {dev}')
    if logits.dtype not in _FLOATS:
        raise TypeError(f'logits must be float32 / bfloat16 / float16, got {logits.dtype}')
    if targets.dtype == torch.bool or targets.is_complex():
        raise TypeError(f'targets must be real numbers 0 / 1, got {targets.dtype}')
    logits, targets = logits.float(), targets.float()
    for name, t in (('logits', logits), ('targets', targets)):
        if (c > 1 and t.stride(1) != 1) or (b > 1 and t.stride(0) < c):
            raise ValueError(f'{name} must have a unit column stride and a row stride >= {c}, got strides {t.stride()}')
    _puzzle_check('meters', meters, torch.float64, (10,), dev)
    _puzzle_check('last', last, torch.float64, (5,), dev)
    _puzzle_check('bad', bad, torch.int32, (1,), dev)
    ld = lambda t: t.stride(0) if b > 1 else c
    _lib.call('vited_cls_metrics_update', _ptr(logits), ld(logits), _ptr(targets), ld(targets), b, c, _ptr(meters), _ptr(last), _ptr(bad),
              _stream())
