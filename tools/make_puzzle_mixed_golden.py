"""Writes tests/golden/mixed_puzzle.npz: the reference's Paikin-Tal solver (``paikin_tal_solver/``) run without puzzle dimensions - on
the pooled pieces of several synthetic puzzles, where it spawns boards, and on one puzzle of unknown size.

    python tools/make_puzzle_mixed_golden.py --reference <checkout of glmanhtu/vit-ed>

The solver package is imported from the checkout, not copied, with the cv2 stand-in of tools/make_puzzle_pixels_golden.py; the distance
generators of tools/make_puzzle_golden.py (and of tools/make_puzzle_type2_golden.py) are reused on a pool of ground-truth grids: low distances between true
neighbours of one puzzle, the far range everywhere else.  Piece ids are unique over the pool, as Puzzle(starting_piece_id=...) makes
them; the pool is shuffled.

The file is named mixed_*: puzzle_*.npz is the pattern of the type-1 fixtures, whose tests take every match.

The file holds arrays only, every name prefixed with its case (``a_`` .. ``e_``):
  grids         int64 [K, 2]          (rows, cols) of the K pooled puzzles
  numb_puzzles  int64 [], threshold float64 []: the solver's numb_puzzles and new_board_mutual_compatibility
  Dq            uint16 [4, n, n] (type 1) or Dq2 uint16 [4, n, n, 4] (type 2): the distances (65535 at j == i; nothing reads it)
  true_loc      int64 [n, 2], true_puzzle int64 [n]: where piece i belongs, and in which puzzle
  board         int64 [n]             the board the solver placed piece i on
  final_loc     int64 [n, 2]          its location on that board (n x n, seed at the centre)
  rotations     int64 [n]             type 2 only: quarter turns
  order         int64 [n]             placement order, seeds included
  spawns        int64 [B]             the index in ``order`` of every board's seed
  spawn_from_heap int64 [B - 1]       1: the weak piece that spawned the board came off the best-buddy heap, 0: out of the slot scan
  recalcs       int64 []              recalculations of the compatibilities
  top_left, bottom_right int64 [B, 2] PuzzleDimensions of every board
  acc           float64 [S, 3], perfect int64 [S]: Direct_Standard, Direct_Modified, neighbor and the perfect flag of collect_results for
                the S scored original puzzles; different_puzzle int64 [S] and wrong_puzzle_id int64 [S]: numb_different_puzzle of the
                standard direct accuracy and wrong_puzzle_id of the neighbour accuracy, the weights in the denominators
  wrong_rotation int64 [S]            type 2 only
  refused_by_dimensions int64 []      case d: placements that the fixed-dimension check of (rows, cols) would have refused
Case ``p_`` is the pixel path: image0, image1 uint8 [H, W, 3], piece_width int64 [], erosion float64 [], perm int64 [n] (piece k of the
solver is piece perm[k] of the images' row-major cuts pooled in image order), pieces uint8 [n, We, We, 3], the arrays above without
Dq, and board0, board1 uint8 [R P, C P, 3], reconstruct_from_pieces' image of every solved board.

The tool asserts what makes the cases meaningful and fails otherwise: every mixed case spawns exactly numb_puzzles boards; over all
cases a spawn happens on the heap branch and one on the empty-pool branch; in case b a piece lies on the board of another puzzle;
case d (the distances of puzzle_ties_9x10.npz) makes a placement the fixed-dimension check would refuse and ends somewhere else
than that golden."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_puzzle_golden as synth                  # noqa: E402  DELTA, the tie levels and their weights
import make_puzzle_pixels_golden as pix             # noqa: E402  the cv2 stand-in and the image generator

GOLDEN = synth.GOLDEN

# case -> (grids, numb_puzzles, seed, kind, the exclusive top of a true neighbour's distance for 'noisy', puzzle type)
CASES = {
    'a': (((3, 4), (3, 4)), 2, 41, 'noisy', 120, 1),
    'b': (((3, 4), (4, 4), (2, 5)), 3, 42, 'noisy', 230, 1),
    'c': (((6, 8), (6, 8)), 2, 43, 'noisy', 230, 1),
    'd': (((9, 10),), 1, 4, 'ties', 0, 1),           # seed and kind of puzzle_ties_9x10 in tools/make_puzzle_golden.py
    'e': (((3, 3), (3, 3)), 2, 43, 'noisy', 230, 2),
}
THRESHOLD = 0.5


def pooled_pieces(grids, rng):
    from paikin_tal_solver.puzzle_piece import PuzzlePiece
    pieces, first = [], 0
    for k, (rows, cols) in enumerate(grids):
        pieces += [PuzzlePiece(k, (r, c), np.zeros((2, 2, 3), np.uint8), piece_id=first + r * cols + c, puzzle_grid_size=(rows, cols))
                   for r in range(rows) for c in range(cols)]
        first += rows * cols
    return [pieces[k] for k in rng.permutation(len(pieces))]


def distances(rng, true_loc, true_puzzle, kind, near, type2):
    """The generators of make_puzzle_golden.py / make_puzzle_type2_golden.py over a pool: a true neighbour is one of the same puzzle."""
    n = true_loc.shape[0]
    where = {(int(k), int(r), int(c)): i for i, (k, (r, c)) in enumerate(zip(true_puzzle, true_loc))}
    shape = (4, n, n, 4) if type2 else (4, n, n)
    D = rng.choice(synth.TIE_LEVELS, size=shape, p=synth.TIE_FAR) if kind == 'ties' else rng.integers(150, 1000, size=shape)
    for i in range(n):
        for s, (dr, dc) in enumerate(synth.DELTA):
            j = where.get((int(true_puzzle[i]), int(true_loc[i, 0] + dr), int(true_loc[i, 1] + dc)))
            if j is None:
                continue
            value = rng.choice(synth.TIE_LEVELS, p=synth.TIE_NEAR) if kind == 'ties' else rng.integers(0, near)
            D[(s, i, j, (s + 2) % 4) if type2 else (s, i, j)] = value
    if type2:
        D[:, np.arange(n), np.arange(n), :] = 65535
    else:
        for s in range(4):
            np.fill_diagonal(D[s], 65535)
    return D.astype(np.uint16)


def run_case(grids, numb_puzzles, seed, kind, near, puzzle_type):
    rng = np.random.default_rng(seed)
    type2 = puzzle_type == 2
    pieces = pooled_pieces(grids, rng)
    true_loc = np.array([p._orig_loc for p in pieces], np.int64)
    true_puzzle = np.array([p._orig_puzzle_id for p in pieces], np.int64)
    D = distances(rng, true_loc, true_puzzle, kind, near, type2)

    def distance_function(piece_i, side_i, piece_j, side_j):
        if type2:
            return int(D[side_i.value, piece_i.id_number, piece_j.id_number, side_j.value])
        assert side_j == side_i.complementary_side
        return int(D[side_i.value, piece_i.id_number, piece_j.id_number])

    out, _ = solve(pieces, distance_function, numb_puzzles, type2, 4, len(grids))
    out.update({'grids': np.array(grids, np.int64), 'Dq2' if type2 else 'Dq': D})
    return out


def solve(pieces, distance_function, numb_puzzles, type2, piece_width, numb_images):
    """PaikinTalSolver(numb_puzzles, ..., THRESHOLD, None).run() with its placements, spawns and recalculations recorded, then the
    reconstruction of every board and the accuracies.  Returns (the arrays, the reconstructed Puzzles)."""
    from paikin_tal_solver.inter_piece_distance import InterPieceDistance
    from paikin_tal_solver.puzzle_importer import Puzzle, PuzzleResultsCollection, PuzzleSolver, PuzzleType
    from paikin_tal_solver.solver import PaikinTalSolver

    true_loc = np.array([p._orig_loc for p in pieces], np.int64)
    true_puzzle = np.array([p._orig_puzzle_id for p in pieces], np.int64)
    order, recalcs, spawns, from_heap, last_find = [], [0], [0], [], [None]
    mark, recalc = PaikinTalSolver._mark_piece_placed, InterPieceDistance.recalculate_remaining_piece_compatibilities
    find, spawn = PaikinTalSolver._find_next_piece, PaikinTalSolver._spawn_new_board

    def mark_spy(self, piece_id):
        order.append(piece_id)
        return mark(self, piece_id)

    def recalc_spy(self, *a, **k):
        recalcs[0] += 1
        return recalc(self, *a, **k)

    def find_spy(self):
        last_find[0] = len(self._best_buddies_pool) > 0
        return find(self)

    def spawn_spy(self):
        spawns.append(len(order))
        from_heap.append(int(last_find[0]))
        return spawn(self)

    PaikinTalSolver._mark_piece_placed, InterPieceDistance.recalculate_remaining_piece_compatibilities = mark_spy, recalc_spy
    PaikinTalSolver._find_next_piece, PaikinTalSolver._spawn_new_board = find_spy, spawn_spy
    try:
        solver = PaikinTalSolver(numb_puzzles, pieces, distance_function, PuzzleType.type2 if type2 else PuzzleType.type1, THRESHOLD, None)
        solver.run()
    finally:
        PaikinTalSolver._mark_piece_placed, InterPieceDistance.recalculate_remaining_piece_compatibilities = mark, recalc
        PaikinTalSolver._find_next_piece, PaikinTalSolver._spawn_new_board = find, spawn
    out = {'numb_puzzles': np.int64(numb_puzzles), 'threshold': np.float64(THRESHOLD), 'true_loc': true_loc, 'true_puzzle': true_puzzle,
           'board': np.array([p.puzzle_id for p in pieces], np.int64), 'final_loc': np.array([p.location for p in pieces], np.int64),
           'order': np.array(order, np.int64), 'spawns': np.array(spawns, np.int64), 'spawn_from_heap': np.array(from_heap, np.int64),
           'recalcs': np.int64(recalcs[0]),
           'top_left': np.array([d.top_left for d in solver._placed_puzzle_dimensions], np.int64),
           'bottom_right': np.array([d.bottom_right for d in solver._placed_puzzle_dimensions], np.int64)}
    if type2:
        out['rotations'] = np.array([p.rotation.value // 90 for p in pieces], np.int64)
    assert len(spawns) == numb_puzzles == solver._numb_puzzles, f'{len(spawns)} boards for {numb_puzzles} puzzles'

    solved, unassigned = solver.get_solved_puzzles()
    assert not unassigned
    new_puzzles = [Puzzle.reconstruct_from_pieces(solved[b], piece_width, b) for b in range(numb_puzzles)]
    results = PuzzleResultsCollection(PuzzleSolver.PaikinTal, PuzzleType.type2 if type2 else PuzzleType.type1,
                                      [p.pieces for p in new_puzzles], [f'synthetic_{k}.png' for k in range(numb_images)])
    results.calculate_accuracies(new_puzzles)
    result, perfect = results.collect_results()
    scored = len(result['neighbor'])
    out['acc'] = np.array([[result['Direct_Standard'][i], result['Direct_Modified'][i], result['neighbor'][i]] for i in range(scored)],
                          np.float64).reshape(scored, 3)
    out['perfect'] = np.array(perfect, np.int64)
    out['different_puzzle'] = np.array([r.standard_direct_accuracy.numb_different_puzzle for r in results.results[:scored]], np.int64)
    out['wrong_puzzle_id'] = np.array([r.modified_neighbor_accuracy.wrong_puzzle_id for r in results.results[:scored]], np.int64)
    if type2:
        out['wrong_rotation'] = np.array([r.standard_direct_accuracy.numb_wrong_rotation for r in results.results[:scored]], np.int64)
    return out, new_puzzles


# the pixel case: (rows, cols, extra height, extra width, seed) of every image; piece width, erosion, noise std, seed of the shuffle
PIXEL_IMAGES = ((3, 4, 2, 3, 51), (3, 4, 1, 0, 52))
PIXEL_P, PIXEL_EROSION, PIXEL_NOISE, PIXEL_SEED = 13, 0.16, 2.0, 53         # We 11, pad 1


def run_pixel():
    """Two synthetic images cut by Puzzle(k, ..., starting_piece_id=...), pooled, shuffled and solved as a mixed bag on
    PuzzlePiece.calculate_asymmetric_distance; the boards are reconstruct_from_pieces' images."""
    from paikin_tal_solver.puzzle_importer import Puzzle
    from paikin_tal_solver.puzzle_piece import PuzzlePiece
    out, pool, first = {}, [], 0
    for k, (rows, cols, dh, dw, seed) in enumerate(PIXEL_IMAGES):
        image = pix.smooth_image(np.random.default_rng(seed), rows * PIXEL_P + dh, cols * PIXEL_P + dw, PIXEL_NOISE)
        pix.IMAGE['image'] = image
        puzzle = Puzzle(k, __file__, PIXEL_P, starting_piece_id=first, erosion=PIXEL_EROSION)
        assert puzzle.grid_size == (rows, cols)
        pool += puzzle.pieces
        first += rows * cols
        out[f'image{k}'] = image
    perm = np.random.default_rng(PIXEL_SEED).permutation(len(pool))
    pieces = [pool[k] for k in perm]
    solved, new_puzzles = solve(pieces, PuzzlePiece.calculate_asymmetric_distance, len(PIXEL_IMAGES), False, PIXEL_P, len(PIXEL_IMAGES))
    out.update(solved)
    out.update(grids=np.array([c[:2] for c in PIXEL_IMAGES], np.int64), perm=perm.astype(np.int64), piece_width=np.int64(PIXEL_P),
               erosion=np.float64(PIXEL_EROSION), pieces=np.stack([p.lab_image for p in pieces]))
    for b, puzzle in enumerate(new_puzzles):
        out[f'board{b}'] = np.asarray(puzzle._img, np.uint8)
    return out


def refused_by_dimensions(out, rows, cols):
    """Placements of a one-board run that _check_board_dimensions would have refused for (rows, cols), replayed over the order."""
    top_left = bottom_right = None
    refused = 0
    for piece in out['order']:
        loc = out['final_loc'][piece]
        if top_left is None:
            top_left, bottom_right = list(loc), list(loc)
            continue
        refused += any(loc[d] - top_left[d] + 1 > size or bottom_right[d] - loc[d] + 1 > size for d, size in ((0, rows), (1, cols)))
        for d in range(2):
            if top_left[d] > loc[d]:
                top_left[d] = loc[d]
            elif bottom_right[d] < loc[d]:
                bottom_right[d] = loc[d]
    return refused


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of glmanhtu/vit-ed (holds paikin_tal_solver/)')
    ap.add_argument('--out', default=GOLDEN)
    args = ap.parse_args()
    pix._install_cv2_standin()
    sys.path.insert(0, os.path.abspath(args.reference))
    everything, branches = {}, []
    for name, case in CASES.items():
        out = run_case(*case)
        branches += out['spawn_from_heap'].tolist()
        if name == 'b':
            assert out['different_puzzle'].sum() > 0 and out['wrong_puzzle_id'].sum() > 0, 'case b: no piece on the board of another puzzle'
        if name == 'd':
            fixed = np.load(os.path.join(GOLDEN, 'puzzle_ties_9x10.npz'))
            assert np.array_equal(fixed['Dq'], out['Dq']) and np.array_equal(fixed['true_loc'], out['true_loc'])
            out['refused_by_dimensions'] = np.int64(refused_by_dimensions(out, 9, 10))
            assert out['refused_by_dimensions'] > 0, 'case d: every placement fits 9 x 10'
            assert not np.array_equal(fixed['final_loc'], out['final_loc']), 'case d: the fixed-dimension solution'
        print(f'{name}: n {len(out["order"])}, boards {len(out["spawns"])}, spawns at {out["spawns"].tolist()} from heap '
              f'{out["spawn_from_heap"].tolist()}, recalcs {int(out["recalcs"])}, acc {out["acc"].round(4).tolist()}, perfect '
              f'{out["perfect"].tolist()}, different puzzle {out["different_puzzle"].tolist()}, wrong puzzle id '
              f'{out["wrong_puzzle_id"].tolist()}, extents {(out["bottom_right"] - out["top_left"] + 1).tolist()}'
              + (f', refused by 9 x 10: {int(out["refused_by_dimensions"])}' if name == 'd' else ''))
        everything.update({f'{name}_{key}': value for key, value in out.items()})
    out = run_pixel()
    print(f'p: n {len(out["order"])}, spawns at {out["spawns"].tolist()} from heap {out["spawn_from_heap"].tolist()}, recalcs '
          f'{int(out["recalcs"])}, acc {out["acc"].round(4).tolist()}, different puzzle {out["different_puzzle"].tolist()}, boards '
          f'{[out[f"board{b}"].shape for b in range(len(out["spawns"]))]}')
    everything.update({f'p_{key}': value for key, value in out.items()})
    assert 1 in branches and 0 in branches, f'spawn branches {branches}: both the heap and the empty-pool branch must occur'
    assert int(everything['c_recalcs']) > 0, 'case c: no recalculation'
    path = os.path.join(args.out, 'mixed_puzzle.npz')
    np.savez_compressed(path, **everything)
    print(f'{path}: {os.path.getsize(path)} bytes')
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
