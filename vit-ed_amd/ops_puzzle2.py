"""Functional wrappers of the type-2 puzzle entry points (pieces of unknown rotation: csrc/puzzle_pixels.hip, csrc/puzzle_compat.hip;
DESIGN.md section 32), re-exported by ``ops``: the border distances of all 16 side pairings, the compatibility state over (piece,
side) candidates with its recalculation and slot scan, and the board of rotated pieces.

They are ``ops`` functions in every respect, kept in a module of their own as ``ops_puzzlepixels`` is: each tensor goes through
``ops._check`` before its pointer reaches ``ops._lib.call``, the launch goes to torch's current stream, nothing synchronises, and
everything is looked up on ``ops`` at call time.  Distances, compat and mutual are [4, n, n, 4], indexed [si, i, j, sj]: side si of
piece i against side sj of piece j."""
from __future__ import annotations

import numpy as np
import torch

from . import ops as _o
from . import ops_puzzlepixels as _pp

_i32, _i64, _u8, _f32 = torch.int32, torch.int64, torch.uint8, torch.float32
_STATE = (('min_d', _i64, (4,)), ('second_d', _i64, (4,)), ('min_count', _i32, (4,)), ('candidate', _i32, (4, 2)),
          ('best_buddy', _i32, (4, 2)), ('compat', _f32, None), ('mutual', _f32, None), ('start_count', _i32, ()),
          ('start_total', _f32, ()), ('start_order', _i32, ()))


def _pieces_of(op, dq2):
    """n of distances [4, n, n, 4], refused in ``op``'s name when the extents are not those."""
    shape = tuple(getattr(dq2, 'shape', ()))
    if len(shape) != 4 or shape[0] != 4 or shape[3] != 4 or shape[1] != shape[2] or not 2 <= shape[1] <= _pp.PUZZLE_MAX_PIECES:
        raise ValueError(f'{op}: dq2 must be [4, n, n, 4] with 2 <= n <= {_pp.PUZZLE_MAX_PIECES}, got shape {list(shape)}')
    return shape[1]


def puzzle_pixel_distances2(pieces: torch.Tensor, out: torch.Tensor | None = None):
    """PuzzlePiece.calculate_asymmetric_distance over all ordered pairs and all 16 side pairings (``vited_puzzle_pixel_distances2``):
    pieces uint8 [n, We, We, 3], n >= 2 -> Dq2 int32 [4, n, n, 4], Dq2[si, i, j, sj] = sum | 2 B_si(i) - B'_si(i) - B_sj(j) | with
    j's border reversed where the reference reverses it; Dq2[si, i, i, sj] is 2^31 - 1.  Dq2[s, :, :, (s + 2) % 4] is
    ``puzzle_pixel_distances``' Dq[s]."""
    _o._need_gpu(pieces, out)
    op = 'puzzle_pixel_distances2'
    n, We = _pp._pieces(op, pieces)
    if n < 2:
        raise ValueError(f'{op}: pieces must hold at least two pieces, got {n}')
    out = _o._out(op, 'out', out, _i32, (4, n, n, 4), pieces.device)
    ws = _o._scratch(_o._lib.load().vited_puzzle_pixel_distances2_workspace_bytes(n, We), pieces.device, align=256)
    _o._lib.call('vited_puzzle_pixel_distances2', _o._ptr(pieces), n, We, _o._ptr(out), *ws, _o._stream())
    return out


def puzzle_compat2_init(dq2: torch.Tensor) -> dict:
    """InterPieceDistance.__init__ for type 2 on the device: a dict of the state tensors of the distances dq2 int32 [4, n, n, 4] -
    min_d, second_d int64 [n, 4], min_count int32 [n, 4], candidate, best_buddy int32 [n, 4, 2] ((piece, side) or (-1, -1)), compat,
    mutual float32 [4, n, n, 4], start_count int32 [n], start_total float32 [n], start_order int32 [n]."""
    _o._need_gpu(dq2)
    op = 'puzzle_compat2_init'
    n, dev = _pieces_of(op, dq2), dq2.device
    _o._check(op, 'dq2', dq2, _i32, (4, n, n, 4), dev)
    st = {name: torch.empty((4, n, n, 4) if tail is None else (n,) + tail, dtype=dtype, device=dev) for name, dtype, tail in _STATE}
    _o._lib.call('vited_puzzle_compat2_init', _o._ptr(dq2), n, *(_o._ptr(st[name]) for name, _, _ in _STATE), _o._stream())
    return st


def puzzle_compat2_recalc(dq2: torch.Tensor, placed: torch.Tensor, st: dict, changed: torch.Tensor):
    """recalculate_remaining_piece_compatibilities(placed) on the state ``st`` of puzzle_compat2_init, in place; changed int32 [n]
    receives 1 for every piece whose min / second-best distances moved.  placed int32 [n] (0 / 1)."""
    _o._need_gpu(dq2, placed, changed, *(st[key] for key in ('min_d', 'second_d', 'compat', 'mutual')))
    op = 'puzzle_compat2_recalc'
    n, dev = _pieces_of(op, dq2), dq2.device
    for name, t, dtype, shape in (('dq2', dq2, _i32, (4, n, n, 4)), ('placed', placed, _i32, (n,)), ('changed', changed, _i32, (n,)),
                                  ("st['min_d']", st['min_d'], _i64, (n, 4)), ("st['second_d']", st['second_d'], _i64, (n, 4)),
                                  ("st['compat']", st['compat'], _f32, (4, n, n, 4)), ("st['mutual']", st['mutual'], _f32, (4, n, n, 4))):
        _o._check(op, name, t, dtype, shape, dev)
    _o._lib.call('vited_puzzle_compat2_recalc', _o._ptr(dq2), n, _o._ptr(placed), _o._ptr(st['min_d']), _o._ptr(st['second_d']),
                 _o._ptr(st['compat']), _o._ptr(st['mutual']), _o._ptr(changed), _o._stream())


def puzzle_best_slot2(mutual: torch.Tensor, placed: torch.Tensor, slot_piece: torch.Tensor, slot_side: torch.Tensor,
                      out: torch.Tensor | None = None) -> torch.Tensor:
    """The packed int64 [1] word of the first maximum of mutual[side, p, slot_piece[k], slot_side[k]] over unplaced p ascending x slot
    k x side 0..3 (include/vited.h; decode with puzzle_unpack_slot2).  mutual float32 [4, n, n, 4]; placed, slot_piece, slot_side
    int32."""
    _o._need_gpu(mutual, placed, slot_piece, slot_side, out)
    op = 'puzzle_best_slot2'
    shape = tuple(getattr(mutual, 'shape', ()))
    if len(shape) != 4 or shape[1] < 2:
        raise ValueError(f'{op}: mutual must be [4, n, n, 4] with n >= 2, got shape {list(shape)}')
    n, dev, k = shape[1], mutual.device, getattr(slot_piece, 'numel', lambda: 0)()
    for name, t, dtype, extent in (('mutual', mutual, _f32, (4, n, n, 4)), ('placed', placed, _i32, (n,)), ('slot_piece', slot_piece, _i32, (k,)),
                                   ('slot_side', slot_side, _i32, (k,))):
        _o._check(op, name, t, dtype, extent, dev)
    if k < 1 or 4 * n * k > 0xffffffff:
        raise ValueError(f'{op}: slot_piece must list at least one slot and 4 * n * slots must stay below 2^32, got {k} slots')
    out = _o._out(op, 'out', out, _i64, (1,), dev)
    _o._lib.call('vited_puzzle_best_slot2', _o._ptr(mutual), n, _o._ptr(placed), _o._ptr(slot_piece), _o._ptr(slot_side), k, _o._ptr(out),
                 _o._stream())
    return out


def puzzle_unpack_slot2(word: int, slots: int):
    """(piece, slot index, side of the piece) of a vited_puzzle_best_slot2 word; None when no piece was unplaced."""
    hit = _o.puzzle_unpack_slot(word, 4 * slots)
    return None if hit is None else (hit[0], hit[1] // 4, hit[1] % 4)


def puzzle_assemble2(pieces: torch.Tensor, locations, rotations, true_locations, piece_width: int, marker=None,
                     out: torch.Tensor | None = None):
    """Puzzle.reconstruct_from_pieces for a type-2 solution (``vited_puzzle_assemble2``): ``puzzle_assemble`` with piece k entering as
    numpy.rot90(pieces[k], rotations[k]) (host integers [n], quarter turns 0..3).  As in the reference, the frame marks a piece away
    from its true location, whatever its rotation."""
    _o._need_gpu(pieces, out)
    op = 'puzzle_assemble2'
    n, We = _pp._pieces(op, pieces)
    P, We = _pp._widths(op, piece_width, We)
    loc = _pp._host_ints(op, 'locations', locations, (n, 2))
    rot = _pp._host_ints(op, 'rotations', rotations, (n,))
    true = _pp._host_ints(op, 'true_locations', true_locations, (n, 2))
    if rot.min() < 0 or rot.max() > 3:
        raise ValueError(f'{op}: rotations must be quarter turns 0..3, got {int(rot.min())} .. {int(rot.max())}')
    cells, R, C, colour = _pp._board_cells(op, n, We, P, loc, true, marker)
    turns = np.zeros(R * C, np.int32)
    turns[loc[:, 0] * C + loc[:, 1]] = rot
    dev = pieces.device
    cells_dev, turns_dev = torch.from_numpy(cells).to(dev), torch.from_numpy(turns).to(dev)
    out = _o._out(op, 'out', out, _u8, (R * P, C * P, 3), dev)
    _o._lib.call('vited_puzzle_assemble2', _o._ptr(pieces), n, We, P, _o._ptr(cells_dev), _o._ptr(turns_dev), R, C, colour, _o._ptr(out),
                 _o._stream())
    return out
