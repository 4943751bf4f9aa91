"""The pixel rules of the classical puzzle baseline restated in numpy, the fixtures the reference's own code
wrote (tools/make_puzzle_pixels_golden.py -> tests/golden/pixel_puzzle_*.npz), and synthetic piece sets for the shapes at which the
distance kernel's tiling could go wrong.  Shared by the CPU and the GPU tests; nothing here is changed by a test."""
import functools
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURES = ('pixel_puzzle_clean_6x7', 'pixel_puzzle_odd_5x6', 'pixel_puzzle_half_6x5', 'pixel_puzzle_noisy_8x9',
            'pixel_puzzle_poster_7x8')
DQ_UNSET = 2 ** 31 - 1
REFERENCE_MARKER = (0, 0, 255)          # insert_piece_into_image's frame, BGR
TILE = 32                               # PD_TILE of csrc/puzzle_pixels.hip


@functools.lru_cache(maxsize=None)
def fixture(name):
    with np.load(os.path.join(GOLDEN, name + '.npz')) as z:
        g = {k: z[k] for k in z.files}
    for a in g.values():
        a.setflags(write=False)
    return g


def eroded_width(P, erosion):
    return min(math.ceil(P * (1 - erosion)), P)


def pad_of(P, We):
    return (P - We) // 2


def marker_for(P, We):
    """The reference frames misplaced pieces whenever it can: with pad < 1 its border width is negative (and its fixtures are solved
    perfectly, so nothing is framed)."""
    return REFERENCE_MARKER if pad_of(P, We) >= 1 else None


# ---- the three rules ---------------------------------------------------------------------------------------------------------------
def cut(image, P, We, order=None):
    H, W = image.shape[:2]
    rows, cols = H // P, W // P
    top, left = (H - rows * P) // 2, (W - cols * P) // 2
    o = int(round((P - We) / 2.0))
    cells = np.arange(rows * cols) if order is None else np.asarray(order)
    out = np.empty((rows * cols, We, We, 3), np.uint8)
    for k, cell in enumerate(cells):
        y, x = top + (cell // cols) * P + o, left + (cell % cols) * P + o
        out[k] = image[y:y + We, x:x + We]
    return out


def side_lines(pieces):
    """(border, next line) int64 [4, n, We, 3]: top / bottom in column order, left / right in row order."""
    p = pieces.astype(np.int64)
    border = np.stack([p[:, 0], p[:, :, -1], p[:, -1], p[:, :, 0]])
    second = np.stack([p[:, 1], p[:, :, -2], p[:, -2], p[:, :, 1]])
    return border, second


def distances(pieces):
    border, second = side_lines(pieces)
    n = pieces.shape[0]
    pred = 2 * border - second
    dq = np.empty((4, n, n), np.int64)
    for s in range(4):
        dq[s] = np.abs(pred[s][:, None] - border[(s + 2) % 4][None]).sum(axis=(2, 3))
        np.fill_diagonal(dq[s], DQ_UNSET)
    assert dq.max() <= DQ_UNSET
    return dq.astype(np.int32)


def board(pieces, locations, true_locations, P, marker=None):
    n, We = pieces.shape[:2]
    loc, true = np.asarray(locations), np.asarray(true_locations)
    R, C = loc[:, 0].max() + 1, loc[:, 1].max() + 1
    pad = pad_of(P, We)
    out = np.zeros((R * P, C * P, 3), np.uint8)
    for k in range(n):
        y, x = loc[k, 0] * P + pad, loc[k, 1] * P + pad
        if marker is not None and (loc[k] != true[k]).any():
            out[y - 1:y + We + 1, x - 1:x + We + 1] = np.asarray(marker, np.uint8)
        out[y:y + We, x:x + We] = pieces[k]
    return out


def pillow_resize(pieces, S):
    """uint8 [n, 3, S, S]: Image.resize((S, S), BILINEAR) of every piece - the expected value of the resize rule."""
    from PIL import Image
    return np.stack([np.asarray(Image.fromarray(p).resize((S, S), Image.BILINEAR)).transpose(2, 0, 1) for p in pieces])


# ---- synthetic piece sets: name -> (n, We, kind) -------------------------------------------------------------------------------------
SHAPES = {
    'two': (2, 5, 'random'),
    'below_tile': (TILE - 1, 4, 'random'),
    'at_tile': (TILE, 4, 'random'),
    'above_tile': (TILE + 1, 4, 'random'),
    'grid_7x11': (77, 6, 'random'),
    'two_lines': (9, 2, 'random'),                  # border and second line are the only two lines and swap roles
    'three_lines': (9, 3, 'random'),
    'odd_above_stage': (35, 23, 'random'),          # 3 We = 69 > 64 (PD_STAGE), padded to 72: a second, short LDS stage
    'extremes': (6, 7, 'extremes'),                 # all-0 against all-255 pieces, and both striped ones
}


@functools.lru_cache(maxsize=None)
def shape_pieces(name):
    n, We, kind = SHAPES[name]
    rng = np.random.default_rng(sorted(SHAPES).index(name))
    if kind == 'random':
        p = rng.integers(0, 256, size=(n, We, We, 3), dtype=np.uint8)
    else:
        p = np.zeros((n, We, We, 3), np.uint8)
        p[1] = 255
        p[2, ::2], p[3, 1::2] = 255, 255                 # rows alternate: predictions of -255 and 510 on top / bottom
        p[4, :, ::2], p[5, :, 1::2] = 255, 255           # columns alternate: the same on left / right
    p.setflags(write=False)
    return p
