"""Type-2 puzzles (pieces of unknown rotation): the fixtures the reference's own solver wrote
(tools/make_puzzle_type2_golden.py -> tests/golden/rot_puzzle_*.npz, rot_pixel_puzzle_*.npz) and the rules restated in numpy - the border
distance of all 16 side pairings, the min / second / C / M rules over (piece, side) candidates, one recalculation, the slot scan and the
board of rotated pieces.  Shared by the CPU and the GPU tests; nothing here is changed by a test."""
import functools

import numpy as np

import puzzle_pixels_cases as pc

SYNTHETIC = ('rot_puzzle_4x4', 'rot_puzzle_clean_8x9', 'rot_puzzle_ties_7x8', 'rot_puzzle_noisy_9x11')
PIXEL = ('rot_pixel_puzzle_even_4x5', 'rot_pixel_puzzle_odd_5x4', 'rot_pixel_puzzle_poster_5x6')
DQ_UNSET = pc.DQ_UNSET
MAXSIZE = 2 ** 63 - 1
STEP = ((-1, 0), (0, 1), (1, 0), (0, -1))
fixture = pc.fixture


def dq2_of(g):
    """The fixture's distances as the int32 [4, n, n, 4] the kernels take: 2^31 - 1 at j == i."""
    d = g['Dq2'].astype(np.int32)
    n = d.shape[1]
    d[:, np.arange(n), np.arange(n), :] = DQ_UNSET
    return d


def locations(g):
    return g['final_loc'] - g['final_loc'].min(axis=0)


# ---- calculate_asymmetric_distance on all 16 pairings (puzzle_piece.py:535-609) ----------------------------------------------------------
def reversed_pairing(si, sj):
    return si == sj or (si, sj) in ((1, 0), (0, 1), (3, 2), (2, 3))


def distances2(pieces):
    border, second = pc.side_lines(pieces)                 # [4, n, We, 3], top / bottom in column order, left / right in row order
    pred = 2 * border - second
    n = pieces.shape[0]
    dq2 = np.empty((4, n, n, 4), np.int64)
    for si in range(4):
        for sj in range(4):
            face = border[sj][:, ::-1] if reversed_pairing(si, sj) else border[sj]
            dq2[si, :, :, sj] = np.abs(pred[si][:, None] - face[None]).sum(axis=(2, 3))
    dq2[:, np.arange(n), np.arange(n), :] = DQ_UNSET
    assert dq2.max() <= DQ_UNSET
    return dq2.astype(np.int32)


# ---- InterPieceDistance for type 2 -----------------------------------------------------------------------------------------------------------
def two_smallest(values):
    row = np.sort(np.concatenate([np.asarray(values, np.int64).ravel(), [MAXSIZE - 1, MAXSIZE]]))
    return row[0], row[1]


def compat_value(d, second):
    return np.float32(1.0 if d == 0 else (-MAXSIZE if second == 0 else 1 - 1.0 * d / second))


def init_state(dq2):
    """(min_d, second_d int64 [n, 4], min_count int64 [n, 4], candidate int64 [n, 4, 2], C, M float32 [4, n, n, 4]) of __init__."""
    D = dq2.astype(np.int64)
    n = D.shape[1]
    mn, sec, cnt = np.empty((n, 4), np.int64), np.empty((n, 4), np.int64), np.empty((n, 4), np.int64)
    cand = np.full((n, 4, 2), -1, np.int64)
    C = np.full((4, n, n, 4), np.inf, np.float32)
    for i in range(n):
        others = np.arange(n) != i
        for s in range(4):
            mn[i, s], sec[i, s] = two_smallest(D[s, i][others])
            hit = np.argwhere((D[s, i] == mn[i, s]) & others[:, None])
            cnt[i, s] = len(hit)
            if len(hit) == 1:
                cand[i, s] = hit[0]
            for j in np.flatnonzero(others):
                for sj in range(4):
                    C[s, i, j, sj] = compat_value(D[s, i, j, sj], sec[i, s])
    return mn, sec, cnt, cand, C, mutual_of(C)


def mutual_of(C):
    """M[si, i, j, sj] = (C[si, i, j, sj] + C[sj, j, i, si]) / 2 in fp32; inf + inf = inf keeps the j == i entries."""
    return ((C + C.transpose(3, 2, 1, 0)) / np.float32(2)).astype(np.float32)


def recalc_state(dq2, placed, mn0, sec0, C0, M0):
    """recalculate_remaining_piece_compatibilities(placed): (changed, min_d, second_d, C, M)."""
    D = dq2.astype(np.int64)
    n = D.shape[1]
    mn, sec, changed = mn0.copy(), sec0.copy(), np.zeros(n, bool)
    for i in np.flatnonzero(~placed):
        keep = ~placed & (np.arange(n) != i)
        for s in range(4):
            mn[i, s], sec[i, s] = two_smallest(D[s, i][keep])
        changed[i] = (mn[i] != mn0[i]).any() or (sec[i] != sec0[i]).any()
    C = C0.copy()
    for i in np.flatnonzero(changed):
        for s in range(4):
            for j in np.flatnonzero(~placed):
                if j != i:
                    for sj in range(4):
                        C[s, i, j, sj] = compat_value(D[s, i, j, sj], sec[i, s])
    M = M0.copy()
    pair = (changed[:, None] | changed[None, :]) & ~np.eye(n, dtype=bool)
    fresh = mutual_of(C)
    M[:, pair, :] = fresh[:, pair, :]
    return changed, mn, sec, C, M


def brute_force_slot(M, placed, slot_piece, slot_side):
    """_get_next_piece_from_pool: unplaced pieces ascending x slots in list order x the piece's side, strict >."""
    best = None
    for p in np.flatnonzero(~placed):
        for k, (q, sq) in enumerate(zip(slot_piece, slot_side)):
            for side in range(4):
                v = M[side, p, q, sq]
                if best is None or v > best[3]:
                    best = (int(p), k, side, v)
    return best


# ---- the board -----------------------------------------------------------------------------------------------------------------------------
def board2(pieces, loc, rotations, true_locations, P, marker=None):
    """insert_piece_into_image: the frame goes by the location alone, then the padded, framed piece is turned by numpy.rot90."""
    n, We = pieces.shape[:2]
    loc, true = np.asarray(loc), np.asarray(true_locations)
    R, C = loc[:, 0].max() + 1, loc[:, 1].max() + 1
    pad = pc.pad_of(P, We)
    out = np.zeros((R * P, C * P, 3), np.uint8)
    for k in range(n):
        tile = np.zeros((We + 2 * pad, We + 2 * pad, 3), np.uint8)
        if marker is not None and (loc[k] != true[k]).any():
            tile[pad - 1:pad + We + 1, pad - 1:pad + We + 1] = np.asarray(marker, np.uint8)
        tile[pad:pad + We, pad:pad + We] = pieces[k]
        tile = np.rot90(tile, int(rotations[k]))
        y, x = loc[k, 0] * P, loc[k, 1] * P
        out[y:y + tile.shape[0], x:x + tile.shape[1]] = tile
    return out


# ---- synthetic piece sets for the distance kernel: name -> (n, We) ------------------------------------------------------------------------------
SHAPES = {
    'two_pieces_two_lines': (2, 2),         # the smallest width with a second line, the smallest n
    'three_pieces_three_lines': (3, 3),
    'seventeen_odd': (17, 15),              # 3 We = 45, padded to 48
    'seventeen_even': (17, 16),             # 3 We = 48: no padding
    'wide_above_a_wave': (5, 67),           # 3 We = 201 values: four LDS stages, the last one short
    'off_tile': (pc.TILE + 3, 4),           # n = 35: two tiles each way, the second nearly empty
}


@functools.lru_cache(maxsize=None)
def shape_pieces(name):
    n, We = SHAPES[name]
    p = np.random.default_rng(100 + sorted(SHAPES).index(name)).integers(0, 256, size=(n, We, We, 3), dtype=np.uint8)
    p.setflags(write=False)
    return p
