"""Functional wrappers of the classical puzzle baseline's pixel entry points (csrc/puzzle_pixels.hip),
re-exported by ``ops``: the cut of an image into eroded pieces, the pieces at the model's size, the prediction-based border distances
and the solved board as an image.

They are ``ops`` functions in every respect - each tensor goes through ``ops._check`` before its pointer reaches ``ops._lib.call``, the
launch goes to torch's current stream, nothing synchronises - kept in a module of their own; everything is looked up on ``ops`` at
call time, so whatever replaces the library or the device gate there (tests/test_ops_args.py does) holds here too.  The piece order
and the piece locations are HOST data (a solver's decisions): they are validated here, so no index the device reads can leave its
array."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops as _o

PUZZLE_MAX_ERODED = 935722       # MAX_ERODED of csrc/puzzle_pixels.h: 765 * 3 * We stays inside int32
PUZZLE_MAX_PIECES = 46340        # MAX_PIECES: the solver's bound
PUZZLE_MAX_SIZE = 1024           # the resize kernel keeps one tap record per output column in LDS
_i32, _u8 = torch.int32, torch.uint8


def puzzle_eroded_width(piece_width: int, erosion: float = 0.) -> int:
    """Width of a piece cut from a cell of ``piece_width`` under ``erosion`` (puzzle_importer.py:224, centre_crop's clamp)."""
    return min(math.ceil(piece_width * (1 - erosion)), piece_width)


def _widths(op, piece_width, eroded):
    P, We = int(piece_width), int(eroded)
    if We < 2 or P < We:
        raise ValueError(f'{op}: needs 2 <= eroded width <= piece width, got eroded width {We} and piece width {P}')
    if We > PUZZLE_MAX_ERODED:
        raise ValueError(f'{op}: eroded width {We} is above {PUZZLE_MAX_ERODED}, where a distance can leave int32')
    return P, We


def _pieces(op, pieces):
    """(n, We) of pieces uint8 [n, We, We, 3], checked."""
    _o._check(op, 'pieces', pieces, _u8, (None, None, None, 3), getattr(pieces, 'device', None))
    n, We = pieces.shape[0], pieces.shape[1]
    if pieces.shape[2] != We or We < 2 or n < 1:
        raise ValueError(f'{op}: pieces must be [n, We, We, 3] with n >= 1 and We >= 2, got shape {tuple(pieces.shape)}')
    if n > PUZZLE_MAX_PIECES or We > PUZZLE_MAX_ERODED:
        raise ValueError(f'{op}: pieces {tuple(pieces.shape)} are above {PUZZLE_MAX_PIECES} pieces or {PUZZLE_MAX_ERODED} wide')
    return n, We


def _host_ints(op, name, values, shape):
    try:
        a = np.asarray(values.cpu() if isinstance(values, torch.Tensor) else values)
    except Exception:
        a = None
    if a is None or a.dtype.kind not in 'iu' or a.shape != shape:
        raise ValueError(f'{op}: {name} must be host integers of shape {list(shape)}, got {getattr(a, "dtype", type(values).__name__)} '
                         f'{list(getattr(a, "shape", ()))}')
    return a.astype(np.int64)


def puzzle_cut(image: torch.Tensor, piece_width: int, eroded_width: int | None = None, order=None, out: torch.Tensor | None = None):
    """Puzzle.make_pieces on the device (``vited_puzzle_cut``): image uint8 [H, W, 3] -> pieces uint8 [n, We, We, 3], n = (H // P) *
    (W // P) cells of the centred grid in row-major order, each centre-cropped to ``eroded_width`` (default: the piece width).  With
    ``order`` (host integers [n], a permutation) piece k is cell order[k]."""
    _o._need_gpu(image, out)
    op = 'puzzle_cut'
    P, We = _widths(op, piece_width, piece_width if eroded_width is None else eroded_width)
    dev = getattr(image, 'device', None)
    _o._check(op, 'image', image, _u8, (None, None, 3), dev)
    H, W = image.shape[0], image.shape[1]
    n = (H // P) * (W // P)
    if n < 1:
        raise ValueError(f'{op}: image {tuple(image.shape)} holds no cell of {P} x {P}')
    if n > PUZZLE_MAX_PIECES:
        raise ValueError(f'{op}: {n} pieces are above {PUZZLE_MAX_PIECES}')
    order_dev = None
    if order is not None:
        perm = _host_ints(op, 'order', order, (n,))
        if not np.array_equal(np.sort(perm), np.arange(n)):
            raise ValueError(f'{op}: order must be a permutation of 0 .. {n - 1}')
        order_dev = torch.from_numpy(perm.astype(np.int32)).to(dev)
    out = _o._out(op, 'out', out, _u8, (n, We, We, 3), dev)
    _o._lib.call('vited_puzzle_cut', _o._ptr(image), H, W, P, We, _o._ptr(order_dev), n, _o._ptr(out), _o._stream())
    return out


def puzzle_resize_pieces(pieces: torch.Tensor, size: int, out: torch.Tensor | None = None):
    """Pillow's ``resize((size, size), BILINEAR)`` of every piece, bit for bit, as planes (``vited_puzzle_resize_pieces``): pieces
    uint8 [n, We, We, 3] -> uint8 [n, 3, size, size], what ``engine.puzzle_distances`` takes.  We <= size <= 1024 (upscaling)."""
    _o._need_gpu(pieces, out)
    op = 'puzzle_resize_pieces'
    n, We = _pieces(op, pieces)
    S = int(size)
    if S < We or S > PUZZLE_MAX_SIZE:
        raise ValueError(f'{op}: size must be in [{We}, {PUZZLE_MAX_SIZE}] for pieces {We} wide (upscaling only), got {S}')
    out = _o._out(op, 'out', out, _u8, (n, 3, S, S), pieces.device)
    _o._lib.call('vited_puzzle_resize_pieces', _o._ptr(pieces), n, We, S, _o._ptr(out), _o._stream())
    return out


def puzzle_pixel_distances(pieces: torch.Tensor, out: torch.Tensor | None = None, puzzle_type: int = 1):
    """PuzzlePiece.calculate_asymmetric_distance over all ordered pairs and sides (``vited_puzzle_pixel_distances``): pieces uint8
    [n, We, We, 3], n >= 2 -> Dq int32 [4, n, n], Dq[s, i, j] = sum | 2 B_s(i) - B'_s(i) - B_(s+2)%4(j) |; the diagonal is 2^31 - 1.
    ``puzzle_type=2``: all 16 side pairings, Dq2 int32 [4, n, n, 4] of ``puzzle_pixel_distances2``."""
    if puzzle_type == 2:
        return _o.puzzle_pixel_distances2(pieces, out)
    if puzzle_type != 1:
        raise ValueError(f'puzzle_pixel_distances: puzzle_type must be 1 or 2, got {puzzle_type!r}')
    _o._need_gpu(pieces, out)
    op = 'puzzle_pixel_distances'
    n, We = _pieces(op, pieces)
    if n < 2:
        raise ValueError(f'{op}: pieces must hold at least two pieces, got {n}')
    out = _o._out(op, 'out', out, _i32, (4, n, n), pieces.device)
    ws = _o._scratch(_o._lib.load().vited_puzzle_pixel_distances_workspace_bytes(n, We), pieces.device, align=256)
    _o._lib.call('vited_puzzle_pixel_distances', _o._ptr(pieces), n, We, _o._ptr(out), *ws, _o._stream())
    return out


def _board_cells(op, n, We, P, loc, true, marker):
    """(cells int32 [R * C], R, C, the marker as one integer or -1) of ``vited_puzzle_assemble`` from validated host locations."""
    if loc.min() < 0:
        raise ValueError(f'{op}: locations must lie inside the board, got a negative cell')
    R, C = int(loc[:, 0].max()) + 1, int(loc[:, 1].max()) + 1
    if R * C != n:
        raise ValueError(f'{op}: locations span a board of {R} x {C} cells, which {n} pieces do not fill')
    flat = loc[:, 0] * C + loc[:, 1]
    if np.unique(flat).size != n:
        raise ValueError(f'{op}: locations must be distinct cells, two pieces collide')
    colour = -1
    if marker is not None:
        m = _host_ints(op, 'marker', marker, (3,))
        if m.min() < 0 or m.max() > 255:
            raise ValueError(f'{op}: marker must be three bytes, got {m.tolist()}')
        if (P - We) // 2 < 1:
            raise ValueError(f'{op}: marker needs a pixel of padding around the pieces, (piece width - eroded width) // 2 = {(P - We) // 2}')
        colour = int(m[0]) | int(m[1]) << 8 | int(m[2]) << 16
    framed = (loc != true).any(axis=1) if marker is not None else np.zeros(n, bool)
    cells = np.full(R * C, -1, np.int32)
    cells[flat] = 2 * np.arange(n) + framed
    return cells, R, C, colour


def puzzle_assemble(pieces: torch.Tensor, locations, true_locations, piece_width: int, marker=None, out: torch.Tensor | None = None):
    """Puzzle.reconstruct_from_pieces on the device (``vited_puzzle_assemble``): the board uint8 [R * P, C * P, 3] of pieces uint8
    [n, We, We, 3] placed at ``locations`` (host integers [n, 2], distinct cells (row, col) >= 0; R, C their extent, R * C = n), each
    at (r P + pad, c P + pad), pad = (P - We) // 2, black elsewhere.  With ``marker`` (three bytes) every piece whose location
    differs from its ``true_locations`` row gets a one-pixel frame of that colour, which needs pad >= 1."""
    _o._need_gpu(pieces, out)
    op = 'puzzle_assemble'
    n, We = _pieces(op, pieces)
    P, We = _widths(op, piece_width, We)
    loc = _host_ints(op, 'locations', locations, (n, 2))
    true = _host_ints(op, 'true_locations', true_locations, (n, 2))
    cells, R, C, colour = _board_cells(op, n, We, P, loc, true, marker)
    cells_dev = torch.from_numpy(cells).to(pieces.device)
    out = _o._out(op, 'out', out, _u8, (R * P, C * P, 3), pieces.device)
    _o._lib.call('vited_puzzle_assemble', _o._ptr(pieces), n, We, P, _o._ptr(cells_dev), R, C, colour, _o._ptr(out), _o._stream())
    return out
