"""The fixture of the mixed-bag and unknown-dimension puzzles (tools/make_puzzle_mixed_golden.py -> tests/golden/mixed_puzzle.npz, the
reference's own solver run without dimensions), shared by the CPU and the GPU tests.  Nothing here is changed by a
test."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = ('a', 'b', 'c', 'd', 'e')       # two 3 x 4; 3 x 4 + 4 x 4 + 2 x 5; two 6 x 8; one 9 x 10 without dimensions; two 3 x 3 of type 2
MIXED = ('a', 'b', 'c', 'e')


@functools.lru_cache(maxsize=None)
def case(name):
    """The arrays of one case without their prefix, read-only."""
    with np.load(os.path.join(GOLDEN, 'mixed_puzzle.npz')) as z:
        g = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + '_')}
    for a in g.values():
        a.setflags(write=False)
    return g


def distances(name):
    """int32 [4, n, n] or [4, n, n, 4] with the engine's diagonal."""
    g = case(name)
    d = (g['Dq2'] if 'Dq2' in g else g['Dq']).astype(np.int32)
    n = d.shape[1]
    d[:, np.arange(n), np.arange(n)] = 2 ** 31 - 1
    return d


def relative_locations(g):
    """Every piece's location from the top-left corner of its own board: what reconstruct_from_pieces makes of the solver's."""
    loc = np.array(g['final_loc'])
    for b in np.unique(g['board']):
        on = g['board'] == b
        loc[on] -= loc[on].min(axis=0)
    return loc


def golden_solution(engine, name):
    """The reference's placements as the ``PuzzleBoards`` that ``solve_puzzle`` has to return."""
    g = case(name)
    loc = relative_locations(g)
    grids = []
    for b in range(len(g['spawns'])):
        on = np.flatnonzero(g['board'] == b)
        grid = np.full(tuple(loc[on].max(axis=0) + 1), -1, np.int64)
        grid[loc[on, 0], loc[on, 1]] = on
        grids.append(grid)
    return engine.PuzzleBoards(loc, np.array(g['final_loc']), np.array(g['order']), int(g['recalcs']), grids[0], g.get('rotations'),
                               boards=np.array(g['board']), top_left=np.array(g['top_left']), bottom_right=np.array(g['bottom_right']),
                               grids=grids, spawns=np.array(g['spawns']), spawn_from_heap=g['spawn_from_heap'].astype(bool))


def assert_solution(sol, name):
    """Board, location, rotation, placement order, spawn points and recalculation count of the reference."""
    g = case(name)
    np.testing.assert_array_equal(sol.boards, g['board'])
    np.testing.assert_array_equal(sol.board_locations, g['final_loc'])
    np.testing.assert_array_equal(sol.locations, relative_locations(g))
    np.testing.assert_array_equal(sol.order, g['order'])
    np.testing.assert_array_equal(sol.spawns, g['spawns'])
    np.testing.assert_array_equal(np.asarray(sol.spawn_from_heap, np.int64), g['spawn_from_heap'])
    np.testing.assert_array_equal(sol.top_left, g['top_left'])
    np.testing.assert_array_equal(sol.bottom_right, g['bottom_right'])
    assert sol.recalcs == int(g['recalcs']) and sol.numb_boards == len(g['spawns'])
    if 'rotations' in g:
        np.testing.assert_array_equal(sol.rotations, g['rotations'])
    else:
        assert sol.rotations is None


def assert_accuracy(acc, name):
    """The dict of ``puzzle_accuracy(..., true_puzzle=)`` against collect_results' numbers, exactly."""
    g = case(name)
    assert acc['Direct_Standard'] == g['acc'][:, 0].tolist() and acc['Direct_Modified'] == g['acc'][:, 1].tolist()
    assert acc['neighbor'] == g['acc'][:, 2].tolist() and [bool(v) for v in acc['perfect']] == [bool(v) for v in g['perfect']]
    if 'wrong_rotation' in g:
        assert acc['wrong_rotation'] == g['wrong_rotation'].tolist()
    else:
        assert 'wrong_rotation' not in acc
