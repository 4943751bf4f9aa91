"""Writes tests/golden/rot_puzzle_*.npz and rot_pixel_puzzle_*.npz: the reference's Paikin-Tal solver (``paikin_tal_solver/``) run with
PuzzleType.type2 - any side of a piece may meet any side of another, the solver assigns each placed piece a rotation - on synthetic
distances and on synthetic images.

    python tools/make_puzzle_type2_golden.py --reference <checkout of glmanhtu/vit-ed> [--only NAME ...]

The solver package is imported from the checkout, not copied; cv2 is replaced by the stand-in of tools/make_puzzle_pixels_golden.py
(identity colour conversion, constant borders), whose image generators are reused as well.  Nothing is rotated physically, as in
paikin_tal_tester.py: the pieces are handed over upright and the accuracies count a piece as right only at rotation 0.

The files are named rot_*: puzzle_*.npz and pixel_puzzle_*.npz are the type-1 fixtures' patterns, whose tests take every match.

rot_puzzle_* (synthetic integer distances; low at (s, (s + 2) % 4) of true neighbours, drawn from the ranges of
tools/make_puzzle_golden.py elsewhere) hold arrays only:
  grid          int64 [2]             (rows, cols)
  Dq2           uint16 [4, n, n, 4]   Dq2[si, i, j, sj]: side si of piece i against side sj of piece j (65535 at j == i; nothing reads it)
  true_loc      int64 [n, 2]          where piece i belongs
  min_d / second_d int64 [n, 4]       InterPieceDistance's per-side minimum and second-best distance after __init__
  bb            int64 [n, 4, 2]       the best buddy (piece, side) of (piece, side), (-1, -1) for none
  start_order   int64 [n]             _start_piece_ordering (piece ids); start_count int64 / start_total float32 [n] its keys
  C / M         float32 [4, n, n, 4]  asymmetric / mutual compatibility after __init__ (smallest case only; inf at j == i)
  final_loc     int64 [n, 2]          each piece's board location (board of n x n, seed at the centre)
  rotations     int64 [n]             each piece's rotation in quarter turns (PuzzlePieceRotation.value // 90)
  order         int64 [n]             placement order (the seed first)
  recalcs       int64 []              times the solver recalculated the compatibilities (best-buddy pool empty)
  acc           float64 [3], perfect int64 [], wrong_rotation int64 []: Direct_Standard, Direct_Modified, neighbor of collect_results, its
                perfect flag, and numb_wrong_rotation of the standard direct accuracy
rot_pixel_puzzle_* (synthetic images through PuzzlePiece.calculate_asymmetric_distance) hold the same except C / M, with Dq2 int32
(2^31 - 1 at j == i), and beside them image uint8 [H, W, 3], piece_width int64 [], erosion float64 [], perm int64 [n] (piece k of the
solver is piece perm[k] of the row-major cut), pieces uint8 [n, We, We, 3] and board uint8 [R P, C P, 3], reconstruct_from_pieces'
image with misplaced pieces framed in (0, 0, 255) where the padding leaves room for the frame.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_puzzle_golden as synth                  # noqa: E402  DELTA, the tie levels and their weights
import make_puzzle_pixels_golden as pix             # noqa: E402  the cv2 stand-in and the image generators

GOLDEN = pix.GOLDEN
DQ_UNSET = 2 ** 31 - 1

# name -> (rows, cols, seed, kind)
SYNTHETIC = {
    'rot_puzzle_4x4': (4, 4, 21, 'clean'),
    'rot_puzzle_clean_8x9': (8, 9, 22, 'clean'),
    'rot_puzzle_ties_7x8': (7, 8, 23, 'ties'),
    'rot_puzzle_noisy_9x11': (9, 11, 24, 'noisy'),
}
FULL_COMPAT = ('rot_puzzle_4x4',)
# name -> (rows, cols, extra height, extra width, piece width, erosion, seed, kind, noise std)
PIXEL = {
    'rot_pixel_puzzle_even_4x5': (4, 5, 2, 3, 14, 0.15, 31, 'smooth', 2.0),          # We 12 (even), pad 1
    'rot_pixel_puzzle_odd_5x4': (5, 4, 1, 4, 13, 0.16, 32, 'smooth', 14.0),          # We 11 (odd), pad 1, noisy: misplaced and turned pieces
    'rot_pixel_puzzle_poster_5x6': (5, 6, 3, 2, 12, 0.2, 33, 'poster', 0.0),         # We 10, pad 1: zeros and ties
}
PIXEL_WIDTHS = {'rot_pixel_puzzle_even_4x5': 12, 'rot_pixel_puzzle_odd_5x4': 11, 'rot_pixel_puzzle_poster_5x6': 10}


def _distances(rng, true_loc, kind):
    """Dq2 uint16 [4, n, n, 4]: the generator of make_puzzle_golden.py on every pairing, low only where si of i truly meets sj of j."""
    n = true_loc.shape[0]
    where = {tuple(loc): k for k, loc in enumerate(true_loc)}
    if kind == 'ties':
        D = rng.choice(synth.TIE_LEVELS, size=(4, n, n, 4), p=synth.TIE_FAR)
    else:
        D = rng.integers(150, 1000, size=(4, n, n, 4))
    for i in range(n):
        for s, (dr, dc) in enumerate(synth.DELTA):
            j = where.get((true_loc[i, 0] + dr, true_loc[i, 1] + dc))
            if j is None:
                continue
            if kind == 'clean':
                D[s, i, j, (s + 2) % 4] = rng.integers(0, 100)
            elif kind == 'noisy':
                D[s, i, j, (s + 2) % 4] = rng.integers(0, 420)
            else:
                D[s, i, j, (s + 2) % 4] = rng.choice(synth.TIE_LEVELS, p=synth.TIE_NEAR)
    D[:, np.arange(n), np.arange(n), :] = 65535
    return D.astype(np.uint16)


def solve(pieces, distance_function, grid_size, piece_width, full_compat):
    """PaikinTalSolver(..., PuzzleType.type2, ...) with its distance state recorded between construction and run(), then the
    reconstruction and the accuracies of solver_driver.py.  Returns (the arrays, the reconstructed Puzzle)."""
    from paikin_tal_solver.inter_piece_distance import InterPieceDistance
    from paikin_tal_solver.puzzle_importer import Puzzle, PuzzleResultsCollection, PuzzleSolver, PuzzleType
    from paikin_tal_solver.solver import PaikinTalSolver

    n = len(pieces)
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
        solver = PaikinTalSolver(1, pieces, distance_function, PuzzleType.type2, 0, grid_size)
        ipd = solver._inter_piece_distance
        info = ipd._piece_distance_info
        out = {'min_d': np.array([[int(v) for v in info[i]._min_distance] for i in range(n)], np.int64),
               'second_d': np.array([[int(v) for v in info[i]._second_best_distance] for i in range(n)], np.int64)}
        bb = np.full((n, 4, 2), -1, np.int64)
        for i in range(n):
            for s in range(4):
                lst = info[i]._best_buddies[s]
                assert len(lst) <= 1
                if lst:
                    bb[i, s] = (lst[0][0], lst[0][1].value)
        out['bb'] = bb
        out['start_order'] = np.array([e[0] for e in ipd._start_piece_ordering], np.int64)
        out['start_count'] = np.array([e[1] for e in ipd._start_piece_ordering], np.int64)
        out['start_total'] = np.array([e[2] for e in ipd._start_piece_ordering], np.float32)
        if full_compat:
            out['C'] = np.stack([np.stack([info[i]._asymmetric_compatibilities[s] for i in range(n)]) for s in range(4)])
            out['M'] = np.stack([np.stack([info[i]._mutual_compatibilities[s] for i in range(n)]) for s in range(4)])
        solver.run()
    finally:
        PaikinTalSolver._mark_piece_placed, InterPieceDistance.recalculate_remaining_piece_compatibilities = mark, recalc
    out['final_loc'] = np.array([p.location for p in pieces], np.int64)
    out['rotations'] = np.array([p.rotation.value // 90 for p in pieces], np.int64)
    out['order'] = np.array(order, np.int64)
    out['recalcs'] = np.int64(recalcs[0])
    solved, _ = solver.get_solved_puzzles()
    new_puzzle = Puzzle.reconstruct_from_pieces(solved[0], piece_width, solved[0][0].puzzle_id)
    results = PuzzleResultsCollection(PuzzleSolver.PaikinTal, PuzzleType.type2, [new_puzzle.pieces], ['synthetic.png'])
    results.calculate_accuracies([new_puzzle])
    result, perfect = results.collect_results()
    out['acc'] = np.array([result['Direct_Standard'][0], result['Direct_Modified'][0], result['neighbor'][0]], np.float64)
    out['perfect'] = np.int64(perfect[0])
    out['wrong_rotation'] = np.int64(results.results[0].standard_direct_accuracy.numb_wrong_rotation)
    return out, new_puzzle


def run_synthetic(rows, cols, seed, kind, full_compat):
    from paikin_tal_solver.puzzle_piece import PuzzlePiece
    rng = np.random.default_rng(seed)
    n = rows * cols
    pieces = [PuzzlePiece(0, (r, c), np.zeros((2, 2, 3), np.uint8), piece_id=r * cols + c, puzzle_grid_size=(rows, cols))
              for r in range(rows) for c in range(cols)]
    pieces = [pieces[k] for k in rng.permutation(n)]
    true_loc = np.array([p._orig_loc for p in pieces], np.int64)
    D = _distances(rng, true_loc, kind)
    calls = [0]

    def distance_function(piece_i, side_i, piece_j, side_j):
        calls[0] += 1
        return int(D[side_i.value, piece_i.id_number, piece_j.id_number, side_j.value])

    out, _ = solve(pieces, distance_function, (rows, cols), 4, full_compat)
    assert calls[0] == 16 * n * (n - 1)
    out.update(grid=np.array([rows, cols], np.int64), Dq2=D, true_loc=true_loc)
    return out


def reference_distances(pieces):
    from paikin_tal_solver.puzzle_piece import PuzzlePiece, PuzzlePieceSide
    n = len(pieces)
    D = np.full((4, n, n, 4), DQ_UNSET, np.int64)
    for i in range(n):
        for j in range(n):
            if i != j:
                for si in PuzzlePieceSide.get_all_sides():
                    for sj in PuzzlePieceSide.get_all_sides():
                        D[si.value, i, j, sj.value] = PuzzlePiece.calculate_asymmetric_distance(pieces[i], si, pieces[j], sj)
    return D.astype(np.int32)


def run_pixel(rows, cols, dh, dw, P, erosion, seed, kind, noise):
    from paikin_tal_solver.puzzle_importer import Puzzle
    from paikin_tal_solver.puzzle_piece import PuzzlePiece
    rng = np.random.default_rng(seed)
    H, W = rows * P + dh, cols * P + dw
    image = pix.smooth_image(rng, H, W, noise) if kind == 'smooth' else pix.poster_image(rng, H, W, P)
    pix.IMAGE['image'] = image
    puzzle = Puzzle(0, __file__, P, starting_piece_id=0, erosion=erosion)
    assert puzzle.grid_size == (rows, cols)
    perm = rng.permutation(rows * cols)
    pieces = [puzzle.pieces[k] for k in perm]
    out = {'image': image, 'piece_width': np.int64(P), 'erosion': np.float64(erosion), 'perm': perm.astype(np.int64),
           'pieces': np.stack([p.lab_image for p in pieces]), 'true_loc': np.array([p._orig_loc for p in pieces], np.int64),
           'grid': np.array([rows, cols], np.int64)}
    out['Dq2'] = reference_distances(pieces)
    solved, new_puzzle = solve(pieces, PuzzlePiece.calculate_asymmetric_distance, puzzle.grid_size, P, False)
    out.update(solved)
    out['board'] = np.asarray(new_puzzle._img, np.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of glmanhtu/vit-ed (holds paikin_tal_solver/)')
    ap.add_argument('--out', default=GOLDEN)
    ap.add_argument('--only', nargs='*', help='case names to write (default: all)')
    args = ap.parse_args()
    pix._install_cv2_standin()
    sys.path.insert(0, os.path.abspath(args.reference))
    cap = os.path.getsize(os.path.join(GOLDEN, 'puzzle_noisy_14x18.npz'))
    for name, case in list(SYNTHETIC.items()) + list(PIXEL.items()):
        if args.only and name not in args.only:
            continue
        t0 = time.perf_counter()
        out = run_synthetic(*case, name in FULL_COMPAT) if name in SYNTHETIC else run_pixel(*case)
        path = os.path.join(args.out, name + '.npz')
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        off = out['Dq2'][out['Dq2'] < min(DQ_UNSET, 65535)] if name in SYNTHETIC else out['Dq2'][out['Dq2'] != DQ_UNSET]
        print(f'{path}: {size} bytes ({time.perf_counter() - t0:.1f} s), recalcs {int(out["recalcs"])}, acc {out["acc"].round(4).tolist()}, '
              f'perfect {int(out["perfect"])}, wrong rotation {int(out["wrong_rotation"])}, rotations '
              f'{np.bincount(out["rotations"], minlength=4).tolist()}, bb sides {int((out["bb"][:, :, 0] >= 0).sum())}/{4 * len(out["order"])}, '
              f'second==0 {int((out["second_d"] == 0).sum())}, Dq2==0 {int((off == 0).sum())}'
              + (f', We {out["pieces"].shape[1]}' if 'pieces' in out else ''))
        assert size < cap, f'{name}: {size} bytes, the cap is {cap}'
        assert name not in PIXEL_WIDTHS or out['pieces'].shape[1] == PIXEL_WIDTHS[name]


if __name__ == '__main__':
    main()
