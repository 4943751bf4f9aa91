"""Writes tests/golden/pixel_puzzle_*.npz: the reference's classical Paikin-Tal baseline (``solver_driver.py``) run on synthetic images.

    python tools/make_puzzle_pixels_golden.py --reference <checkout of glmanhtu/vit-ed> [--time-loop]

``paikin_tal_solver`` is imported from the checkout, not copied.  cv2 is not needed for what is recorded here - the cut, the border
distance, the solver and the reconstruction are numpy slicing and integer arithmetic - so a stand-in module is registered under that
name before the import: ``cvtColor`` is the identity (the colour conversion stays with the caller),
``imread`` returns the case's synthetic image and ``copyMakeBorder`` pads with a constant, honouring a 3-channel ``value``.

Per case the reference's own code runs: ``Puzzle(0, path, P, erosion=e)`` (make_pieces), a seeded permutation of ``pieces`` (the
driver's random.shuffle, made explicit), ``PuzzlePiece.calculate_asymmetric_distance`` over every ordered pair and side,
``PaikinTalSolver(...).run()``, ``Puzzle.reconstruct_from_pieces`` and ``PuzzleResultsCollection.collect_results``.

The files are named pixel_puzzle_*, not puzzle_*: that pattern is the solver fixtures' of tools/make_puzzle_golden.py, whose tests
take every file matching it.

Each file holds arrays only:
  image       uint8 [H, W, 3]       the synthetic image (a low-frequency field plus noise, or a posterised one)
  piece_width int64 [], erosion float64 []
  perm        int64 [n]             piece k of the solver is piece perm[k] of the row-major cut
  pieces      uint8 [n, We, We, 3]  the solver's pieces, in its order
  true_loc    int64 [n, 2], grid int64 [2]
  Dq          int32 [4, n, n]       calculate_asymmetric_distance(i, s, j, s^); the diagonal is 2^31 - 1
  final_loc   int64 [n, 2], order int64 [n], recalcs int64 []: as in puzzle_*.npz (tools/make_puzzle_golden.py)
  acc         float64 [3], perfect int64 []: Direct_Standard, Direct_Modified, neighbor of collect_results, and its perfect flag
  board       uint8 [R * P, C * P, 3] reconstruct_from_pieces' image, misplaced pieces framed in (0, 0, 255)
"""
import argparse
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DQ_UNSET = 2 ** 31 - 1

# name -> (rows, cols, extra height, extra width, piece width, erosion, seed, kind, noise std)
CASES = {
    'pixel_puzzle_clean_6x7': (6, 7, 3, 4, 28, 0.0, 11, 'smooth', 2.0),           # We 28 (even), remainders 3 and 4, solves perfectly
    'pixel_puzzle_odd_5x6': (5, 6, 1, 2, 16, 0.07, 12, 'smooth', 2.0),            # We 15: 3 We odd, crop offset round(0.5) = 0, pad 0
    'pixel_puzzle_half_6x5': (6, 5, 5, 0, 13, 0.25, 13, 'smooth', 2.0),           # We 10: crop offset round(1.5) = 2, pad 1
    'pixel_puzzle_noisy_8x9': (8, 9, 3, 5, 16, 0.15, 6, 'smooth', 16.0),          # We 14, pad 1: misplaced pieces, framed
    'pixel_puzzle_poster_7x8': (7, 8, 2, 7, 12, 0.2, 15, 'poster', 0.0),          # We 10, pad 1: ties, zeros, 0 against 255
}
IMAGE = {}


def _install_cv2_standin():
    cv2 = types.ModuleType('cv2')
    cv2.COLOR_BGR2LAB, cv2.COLOR_LAB2BGR, cv2.BORDER_CONSTANT = 44, 56, 0
    cv2.cvtColor = lambda img, code: np.array(img, copy=True)

    def copy_make_border(img, top, bottom, left, right, border_type, value=None):
        out = np.zeros((img.shape[0] + top + bottom, img.shape[1] + left + right, img.shape[2]), img.dtype)   # raises on a negative width
        if value is not None:
            out[...] = np.asarray(value, img.dtype)
        out[top:top + img.shape[0], left:left + img.shape[1]] = img
        return out

    cv2.copyMakeBorder = copy_make_border
    cv2.imread = lambda path: np.array(IMAGE['image'], copy=True)
    sys.modules['cv2'] = cv2


def smooth_image(rng, H, W, noise):
    """A random grid of colours one node every 9 pixels, interpolated bilinearly, plus Gaussian noise."""
    g = rng.integers(0, 256, size=(H // 9 + 2, W // 9 + 2, 3)).astype(np.float64)
    ys, xs = np.linspace(0, g.shape[0] - 1.001, H), np.linspace(0, g.shape[1] - 1.001, W)
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    out = (g[y0][:, x0] * (1 - fy) * (1 - fx) + g[y0][:, x0 + 1] * (1 - fy) * fx + g[y0 + 1][:, x0] * fy * (1 - fx)
           + g[y0 + 1][:, x0 + 1] * fy * fx)
    out += rng.normal(0, noise, out.shape)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def poster_image(rng, H, W, P):
    """Four grey levels per channel over a smooth field (flat regions: tied and zero distances), and two blocks of lines that
    alternate 0 and 255 across cell borders, along rows and along columns (the prediction's extremes, -255 and 510)."""
    levels = np.array([0, 85, 170, 255], np.uint8)
    img = levels[smooth_image(rng, H, W, 0.0) // 64]
    img[: 3 * P, : 2 * P] = np.where(np.arange(3 * P) % 2 == 0, 0, 255).astype(np.uint8)[:, None, None]
    img[-3 * P:, -3 * P:] = np.where(np.arange(3 * P) % 2 == 0, 255, 0).astype(np.uint8)[None, :, None]
    return img


def reference_distances(pieces):
    from paikin_tal_solver.puzzle_piece import PuzzlePiece, PuzzlePieceSide
    n = len(pieces)
    D = np.full((4, n, n), DQ_UNSET, np.int64)
    for i in range(n):
        for j in range(n):
            if i != j:
                for s in PuzzlePieceSide.get_all_sides():
                    D[s.value, i, j] = PuzzlePiece.calculate_asymmetric_distance(pieces[i], s, pieces[j], s.complementary_side)
    return D.astype(np.int32)


def run_case(rows, cols, dh, dw, P, erosion, seed, kind, noise):
    from paikin_tal_solver.inter_piece_distance import InterPieceDistance
    from paikin_tal_solver.puzzle_importer import Puzzle, PuzzleResultsCollection, PuzzleSolver, PuzzleType
    from paikin_tal_solver.puzzle_piece import PuzzlePiece
    from paikin_tal_solver.solver import PaikinTalSolver

    rng = np.random.default_rng(seed)
    H, W = rows * P + dh, cols * P + dw
    image = smooth_image(rng, H, W, noise) if kind == 'smooth' else poster_image(rng, H, W, P)
    IMAGE['image'] = image
    puzzle = Puzzle(0, __file__, P, starting_piece_id=0, erosion=erosion)
    assert puzzle.grid_size == (rows, cols)
    perm = rng.permutation(rows * cols)
    pieces = [puzzle.pieces[k] for k in perm]                     # solver_driver.py: random.shuffle(pieces)
    out = {'image': image, 'piece_width': np.int64(P), 'erosion': np.float64(erosion), 'perm': perm.astype(np.int64),
           'pieces': np.stack([p.lab_image for p in pieces]), 'true_loc': np.array([p._orig_loc for p in pieces], np.int64),
           'grid': np.array([rows, cols], np.int64)}
    out['Dq'] = reference_distances(pieces)

    order, recalcs = [], [0]
    mark, recalc = PaikinTalSolver._mark_piece_placed, InterPieceDistance.recalculate_remaining_piece_compatibilities

    def mark_spy(self, piece_id):
        order.append(piece_id)
        return mark(self, piece_id)

    def recalc_spy(self, *a, **k):
        recalcs[0] += 1
        return recalc(self, *a, **k)

    PaikinTalSolver._mark_piece_placed, InterPieceDistance.recalculate_remaining_piece_compatibilities = mark_spy, recalc_spy
    try:
        solver = PaikinTalSolver(1, pieces, PuzzlePiece.calculate_asymmetric_distance, PuzzleType.type1, 0, puzzle.grid_size)
        solver.run()
    finally:
        PaikinTalSolver._mark_piece_placed, InterPieceDistance.recalculate_remaining_piece_compatibilities = mark, recalc
    out['final_loc'] = np.array([p.location for p in pieces], np.int64)
    out['order'] = np.array(order, np.int64)
    out['recalcs'] = np.int64(recalcs[0])
    solved, _ = solver.get_solved_puzzles()
    new_puzzle = Puzzle.reconstruct_from_pieces(solved[0], P, solved[0][0].puzzle_id)
    results = PuzzleResultsCollection(PuzzleSolver.PaikinTal, PuzzleType.type1, [new_puzzle.pieces], ['synthetic.png'])
    results.calculate_accuracies([new_puzzle])
    result, perfect = results.collect_results()
    out['acc'] = np.array([result['Direct_Standard'][0], result['Direct_Modified'][0], result['neighbor'][0]], np.float64)
    out['perfect'] = np.int64(perfect[0])
    out['board'] = np.asarray(new_puzzle._img, np.uint8)
    return out


def prediction_extremes(pieces):
    """(min, max) of 2 B - B' over the four sides of every piece."""
    p = pieces.astype(np.int64)
    pred = [2 * p[:, 0] - p[:, 1], 2 * p[:, :, -1] - p[:, :, -2], 2 * p[:, -1] - p[:, -2], 2 * p[:, :, 0] - p[:, :, 1]]
    return min(int(v.min()) for v in pred), max(int(v.max()) for v in pred)


def time_reference_loop(n_rows=18, n_cols=24, P=28):
    """Seconds the reference's Python distance loop takes at n = 432 pieces of 28 x 28 on this CPU (context for DESIGN.md)."""
    from paikin_tal_solver.puzzle_importer import Puzzle
    IMAGE['image'] = smooth_image(np.random.default_rng(0), n_rows * P, n_cols * P, 2.0)
    pieces = Puzzle(0, __file__, P, starting_piece_id=0, erosion=0.0).pieces
    t0 = time.perf_counter()
    reference_distances(pieces)
    return len(pieces), time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of glmanhtu/vit-ed (holds paikin_tal_solver/)')
    ap.add_argument('--out', default=GOLDEN)
    ap.add_argument('--time-loop', action='store_true', help='also time the reference distance loop at 432 pieces (prints only)')
    args = ap.parse_args()
    _install_cv2_standin()
    sys.path.insert(0, os.path.abspath(args.reference))
    lo, hi = 0, 0
    for name, case in CASES.items():
        out = run_case(*case)
        path = os.path.join(args.out, name + '.npz')
        np.savez_compressed(path, **out)
        e = prediction_extremes(out['pieces'])
        lo, hi = min(lo, e[0]), max(hi, e[1])
        dq = out['Dq'][out['Dq'] != DQ_UNSET]
        print(f'{path}: {os.path.getsize(path)} bytes, We {out["pieces"].shape[1]}, recalcs {int(out["recalcs"])}, '
              f'acc {out["acc"].round(4).tolist()}, perfect {int(out["perfect"])}, Dq max {int(dq.max())} zeros {int((dq == 0).sum())} '
              f'distinct {np.unique(dq).size}/{dq.size}, prediction range {e}')
    assert (lo, hi) == (-255, 510), (lo, hi)
    if args.time_loop:
        n, seconds = time_reference_loop()
        print(f'reference distance loop, n = {n}: {seconds:.1f} s ({4 * n * (n - 1)} calls)')


if __name__ == '__main__':
    main()
