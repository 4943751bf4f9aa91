"""The Paikin-Tal fixtures (tests/golden/puzzle_*.npz, written by tools/make_puzzle_golden.py from the reference's solver) are
self-consistent, and engine.puzzle_accuracy reproduces the reference's accuracies from the reference's own placements.  No GPU."""
import glob
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'puzzle_*.npz')))


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


def reference_solution(g):
    from vited_amd import engine
    board = g['final_loc']
    loc = board - board.min(axis=0)
    grid = np.full(tuple(loc.max(axis=0) + 1), -1, np.int64)
    grid[loc[:, 0], loc[:, 1]] = np.arange(loc.shape[0])
    return engine.PuzzleSolution(loc, board, g['order'], int(g['recalcs']), grid)


def test_the_cases_are_there():
    assert CASES == ['puzzle_4x4', 'puzzle_clean_8x12', 'puzzle_noisy_14x18', 'puzzle_ties_9x10']
    for name in CASES:
        assert os.path.getsize(os.path.join(GOLDEN, name + '.npz')) < 1 << 20


@pytest.mark.parametrize('name', CASES)
def test_fixture_is_consistent(name):
    g = load(name)
    rows, cols = (int(v) for v in g['grid'])
    n = rows * cols
    assert g['Dq'].shape == (4, n, n) and g['Dq'].dtype == np.uint16
    assert all((np.diagonal(g['Dq'][s]) == 65535).all() for s in range(4))
    # every true cell once, every piece placed once, on distinct board cells inside a rows x cols block
    assert sorted(map(tuple, g['true_loc'])) == [(r, c) for r in range(rows) for c in range(cols)]
    assert sorted(g['order'].tolist()) == list(range(n)) and sorted(g['start_order'].tolist()) == list(range(n))
    assert g['order'][0] == g['start_order'][0], 'the seed is the first start piece'
    assert len(set(map(tuple, g['final_loc']))) == n
    assert tuple(g['final_loc'].max(axis=0) - g['final_loc'].min(axis=0) + 1) == (rows, cols)
    assert tuple(g['final_loc'][g['order'][0]]) == (n // 2, n // 2), 'the seed sits at the board centre'
    # min / second-best are the two smallest of each side's row, with multiplicity
    D = g['Dq'].astype(np.int64)
    for s in range(4):
        for i in range(n):
            row = np.sort(np.delete(D[s, i], i))
            assert (g['min_d'][i, s], g['second_d'][i, s]) == (row[0], row[1])
    # best buddies name each other on complementary sides, and their side held the unique minimum
    bb = g['bb']
    for i, s in zip(*np.nonzero(bb >= 0)):
        j = bb[i, s]
        assert bb[j, (s + 2) % 4] == i
        assert D[s, i, j] == g['min_d'][i, s] and (np.delete(D[s, i], i) == g['min_d'][i, s]).sum() == 1
    # the start ordering is a stable descending sort of its keys
    keys = list(zip(g['start_count'].tolist(), g['start_total'].tolist()))
    assert keys == sorted(keys, reverse=True)
    for a in range(n - 1):
        if keys[a] == keys[a + 1]:
            assert g['start_order'][a] < g['start_order'][a + 1]
    if 'M' in g:
        C, M = g['C'], g['M']
        off = ~np.eye(n, dtype=bool)
        for s in range(4):
            want = ((C[s] + C[(s + 2) % 4].T) / np.float32(2)).astype(np.float32)
            assert np.array_equal(M[s][off].view(np.uint32), want[off].view(np.uint32))
            assert np.isinf(np.diagonal(C[s])).all() and np.isinf(np.diagonal(M[s])).all()


def test_the_cases_cover_the_branches():
    ties, clean, noisy = load('puzzle_ties_9x10'), load('puzzle_clean_8x12'), load('puzzle_noisy_14x18')
    assert (ties['Dq'] == 0).sum() > 0 and (ties['second_d'] == 0).sum() > 0, 'the d == 0 and second == 0 branches of C'
    assert int(clean['perfect']) == 1 and int(clean['recalcs']) == 0
    assert int(noisy['recalcs']) > 10 and noisy['acc'][0] < 1


@pytest.mark.parametrize('name', CASES)
def test_accuracy_of_the_reference_placement(name):
    from vited_amd import engine
    g = load(name)
    acc = engine.puzzle_accuracy(reference_solution(g), g['true_loc'])
    assert [acc['Direct_Standard'], acc['Direct_Modified'], acc['neighbor']] == g['acc'].tolist()
    assert acc['perfect'] == bool(g['perfect'])


def test_accuracy_of_shifted_and_partial_solutions():
    from vited_amd import engine
    rows, cols = 3, 4
    true = np.array([(r, c) for r in range(rows) for c in range(cols)])
    perfect = engine.PuzzleSolution(true, true, np.arange(12), 0, np.arange(12).reshape(rows, cols))
    assert engine.puzzle_accuracy(perfect, true) == {'Direct_Standard': 1.0, 'Direct_Modified': 1.0, 'neighbor': 1.0, 'perfect': True}
    # the columns rolled by one: no piece in its true cell, every vertical side still right, and of the horizontal ones those
    # whose seam did not wrap round (or whose board edge is still an edge)
    rolled = true.copy()
    rolled[:, 1] = (true[:, 1] + 1) % cols
    acc = engine.puzzle_accuracy(engine.PuzzleSolution(rolled, rolled, np.arange(12), 0, None), true)
    assert acc['Direct_Standard'] == 0.0 and not acc['perfect']
    assert acc['neighbor'] == pytest.approx((12 * 2 + 3 * 4) / 48)
