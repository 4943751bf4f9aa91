"""Writes tests/golden/puzzle_*.npz: the reference's Paikin-Tal solver (``paikin_tal_solver/``) run on synthetic type-1 puzzles.

    python tools/make_puzzle_golden.py --reference <checkout of glmanhtu/vit-ed>

The solver package is imported from the checkout, not copied.  cv2 is not needed by anything recorded here (the solver and the
accuracy classes only read piece locations), so a minimal stand-in module is registered under that name before the import: pieces
get tiny synthetic arrays and the stand-in's colour conversion is the identity.  The distance function hands the solver a
synthetic integer distance ``Dq[s, i, j]`` (side s of piece i against the complementary side of piece j, indexed by the solver's
piece ids) drawn from a seeded generator: low for the true neighbour, high elsewhere, with per-case noise.

Each file holds arrays only:
  grid          int64 [2]        (rows, cols)
  Dq            uint16 [4, n, n] the distances (the diagonal is 65535; nothing reads it)
  true_loc      int64 [n, 2]     where piece i belongs
  min_d / second_d int64 [n, 4]  InterPieceDistance's per-side minimum and second-best distance after __init__
  bb            int64 [n, 4]     the best buddy of (piece, side), -1 for none
  start_order   int64 [n]        _start_piece_ordering (piece ids); start_count int64 / start_total float32 [n] its keys
  C / M         float32 [4, n, n] asymmetric / mutual compatibility after __init__ (smallest case only; diagonal inf)
  final_loc     int64 [n, 2]     each piece's board location as the solver placed it (board of n x n, seed at the centre)
  order         int64 [n]        placement order (the seed first)
  recalcs       int64 []         times the solver recalculated the compatibilities (best-buddy pool empty)
  acc           float64 [3], perfect int64 []: Direct_Standard, Direct_Modified, neighbor of collect_results, and its perfect flag
"""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

# name -> (rows, cols, seed, kind)
CASES = {
    'puzzle_4x4': (4, 4, 1, 'noisy'),
    'puzzle_clean_8x12': (8, 12, 2, 'clean'),
    'puzzle_noisy_14x18': (14, 18, 3, 'noisy'),
    'puzzle_ties_9x10': (9, 10, 4, 'ties'),
}
FULL_COMPAT = ('puzzle_4x4',)
DELTA = ((-1, 0), (0, 1), (1, 0), (0, -1))       # top, right, bottom, left
TIE_LEVELS = np.array([0, 3, 7, 12, 40, 200, 999])
TIE_FAR = np.array([0.012, 0.03, 0.1, 0.2, 0.3, 0.2, 0.158])      # level weights away from the true neighbour
TIE_NEAR = np.array([0.4, 0.2, 0.15, 0.1, 0.1, 0.05, 0.0])     # and at it


def _install_cv2_standin():
    cv2 = types.ModuleType('cv2')
    cv2.COLOR_BGR2LAB, cv2.COLOR_LAB2BGR, cv2.BORDER_CONSTANT = 44, 56, 0
    cv2.cvtColor = lambda img, code: np.array(img, copy=True)

    def copy_make_border(img, top, bottom, left, right, border_type, value=None):
        fill = 0 if value is None else value[0]
        return np.pad(img, ((top, bottom), (left, right), (0, 0)), constant_values=fill)

    cv2.copyMakeBorder = copy_make_border
    cv2.imread = lambda path: np.zeros((8, 8, 3), np.uint8)
    sys.modules['cv2'] = cv2


def _distances(rng, true_loc, kind):
    n = true_loc.shape[0]
    where = {tuple(loc): k for k, loc in enumerate(true_loc)}
    if kind == 'ties':
        D = rng.choice(TIE_LEVELS, size=(4, n, n), p=TIE_FAR)
    else:
        D = rng.integers(150, 1000, size=(4, n, n))
    for i in range(n):
        for s, (dr, dc) in enumerate(DELTA):
            j = where.get((true_loc[i, 0] + dr, true_loc[i, 1] + dc))
            if j is None:
                continue
            if kind == 'clean':
                D[s, i, j] = rng.integers(0, 100)
            elif kind == 'noisy':
                D[s, i, j] = rng.integers(0, 320)
            else:
                D[s, i, j] = rng.choice(TIE_LEVELS, p=TIE_NEAR)
    for s in range(4):
        np.fill_diagonal(D[s], 65535)
    return D.astype(np.uint16)


def run_case(rows, cols, seed, kind, full_compat):
    from paikin_tal_solver.inter_piece_distance import InterPieceDistance
    from paikin_tal_solver.puzzle_importer import Puzzle, PuzzleResultsCollection, PuzzleSolver, PuzzleType
    from paikin_tal_solver.puzzle_piece import PuzzlePiece
    from paikin_tal_solver.solver import PaikinTalSolver

    rng = np.random.default_rng(seed)
    n = rows * cols
    pieces = [PuzzlePiece(0, (r, c), np.zeros((2, 2, 3), np.uint8), piece_id=r * cols + c, puzzle_grid_size=(rows, cols))
              for r in range(rows) for c in range(cols)]
    pieces = [pieces[k] for k in rng.permutation(n)]
    true_loc = np.array([p._orig_loc for p in pieces], np.int64)
    D = _distances(rng, true_loc, kind)

    def distance_function(piece_i, side_i, piece_j, side_j):
        assert side_j == side_i.complementary_side
        return int(D[side_i.value, piece_i.id_number, piece_j.id_number])

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
        # what solver_driver.paikin_tal_driver does, with the distance state recorded between construction and run()
        solver = PaikinTalSolver(1, pieces, distance_function, PuzzleType.type1, 0, (rows, cols))
        ipd = solver._inter_piece_distance
        info = ipd._piece_distance_info
        out = {'grid': np.array([rows, cols], np.int64), 'Dq': D, 'true_loc': true_loc,
               'min_d': np.array([[int(v) for v in info[i]._min_distance] for i in range(n)], np.int64),
               'second_d': np.array([[int(v) for v in info[i]._second_best_distance] for i in range(n)], np.int64)}
        bb = np.full((n, 4), -1, np.int64)
        for i in range(n):
            for s in range(4):
                lst = info[i]._best_buddies[s]
                assert len(lst) <= 1
                if lst:
                    bb[i, s] = lst[0][0]
        out['bb'] = bb
        out['start_order'] = np.array([e[0] for e in ipd._start_piece_ordering], np.int64)
        out['start_count'] = np.array([e[1] for e in ipd._start_piece_ordering], np.int64)
        out['start_total'] = np.array([e[2] for e in ipd._start_piece_ordering], np.float32)
        if full_compat:
            out['C'] = np.stack([np.stack([info[i]._asymmetric_compatibilities[s, :, 0] for i in range(n)]) for s in range(4)])
            out['M'] = np.stack([np.stack([info[i]._mutual_compatibilities[s, :, 0] for i in range(n)]) for s in range(4)])
        solver.run()
    finally:
        PaikinTalSolver._mark_piece_placed, InterPieceDistance.recalculate_remaining_piece_compatibilities = mark, recalc
    out['final_loc'] = np.array([p.location for p in pieces], np.int64)
    out['order'] = np.array(order, np.int64)
    out['recalcs'] = np.int64(recalcs[0])
    solved, _ = solver.get_solved_puzzles()
    new_puzzle = Puzzle.reconstruct_from_pieces(solved[0], 4, solved[0][0].puzzle_id)
    results = PuzzleResultsCollection(PuzzleSolver.PaikinTal, PuzzleType.type1, [new_puzzle.pieces], ['synthetic.png'])
    results.calculate_accuracies([new_puzzle])
    result, perfect = results.collect_results()
    out['acc'] = np.array([result['Direct_Standard'][0], result['Direct_Modified'][0], result['neighbor'][0]], np.float64)
    out['perfect'] = np.int64(perfect[0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of glmanhtu/vit-ed (holds paikin_tal_solver/)')
    ap.add_argument('--out', default=GOLDEN)
    args = ap.parse_args()
    _install_cv2_standin()
    sys.path.insert(0, os.path.abspath(args.reference))
    for name, (rows, cols, seed, kind) in CASES.items():
        out = run_case(rows, cols, seed, kind, name in FULL_COMPAT)
        path = os.path.join(args.out, name + '.npz')
        np.savez_compressed(path, **out)
        print(f'{path}: {os.path.getsize(path)} bytes, recalcs {int(out["recalcs"])}, acc {out["acc"].round(4).tolist()}, '
              f'perfect {int(out["perfect"])}, bb sides {int((out["bb"] >= 0).sum())}/{4 * rows * cols}, '
              f'second==0 {int((out["second_d"] == 0).sum())}, Dq==0 {int((out["Dq"] == 0).sum())}')


if __name__ == '__main__':
    main()
