"""CPU: mixed-bag and unknown-dimension puzzles - the argument rules of engine.solve_puzzle, the accuracies of
several puzzles against the reference's numbers (tests/golden/mixed_puzzle.npz), the extents rule, the fixture's own conditions, the
C entry's refusals and the wrapper's argument checks with the library replaced by a recorder."""
import ctypes
import fnmatch
import inspect
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import puzzle_mixed_cases as mc

BAD, UNSUPPORTED = 1, 2


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def test_the_fixture_meets_the_conditions_that_make_it_meaningful():
    assert not fnmatch.fnmatch('mixed_puzzle.npz', 'puzzle_*.npz') and not fnmatch.fnmatch('mixed_puzzle.npz', 'pixel_puzzle_*.npz')
    branches = []
    for name in mc.MIXED:
        g = mc.case(name)
        assert len(g['spawns']) == int(g['numb_puzzles']) == len(g['grids']) and g['spawns'][0] == 0
        assert len(np.unique(g['board'])) == int(g['numb_puzzles'])
        assert int(g['grids'].prod(axis=1).sum()) == len(g['order'])
        branches += g['spawn_from_heap'].tolist()
    assert 0 in branches and 1 in branches                                          # the empty-pool branch and the heap branch
    assert [len(mc.case(c)['order']) for c in mc.CASES] == [24, 38, 96, 90, 18]
    b = mc.case('b')
    assert b['different_puzzle'].sum() > 0 and (b['wrong_puzzle_id'] == 4 * b['different_puzzle']).all()
    assert int(mc.case('c')['recalcs']) > 0
    d, fixed = mc.case('d'), np.load(mc.GOLDEN + '/puzzle_ties_9x10.npz')
    assert np.array_equal(d['Dq'], fixed['Dq']) and not np.array_equal(d['final_loc'], fixed['final_loc'])
    assert int(d['refused_by_dimensions']) > 0 and len(d['spawns']) == 1
    assert 'Dq2' in mc.case('e') and mc.case('e')['Dq2'].shape == (4, 18, 18, 4)


# ---- argument rules ------------------------------------------------------------------------------------------------------------------
def test_solve_puzzle_keywords_and_refusals(vited):
    engine = vited.engine
    sig = inspect.signature(engine.solve_puzzle).parameters
    assert sig['grid_size'].default is None and sig['numb_puzzles'].default == 1
    assert sig['new_board_mutual_compatibility'].default == 0.5 and sig['mutual_lookup'].default is None
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('numb_puzzles', 'new_board_mutual_compatibility', 'mutual_lookup'))
    dq = torch.from_numpy(mc.distances('a'))                                        # on the host: every refusal comes before the device
    with pytest.raises(ValueError, match='^When specifying puzzle dimensions, only a single puzzle is allowed.$'):
        engine.solve_puzzle(dq, (4, 6), numb_puzzles=2)
    with pytest.raises(ValueError, match='^At least a single puzzle is required.$'):
        engine.solve_puzzle(dq, None, numb_puzzles=0)
    with pytest.raises(ValueError, match="mutual_lookup must be 'gather' or 'mirror'"):
        engine.solve_puzzle(dq, None, mutual_lookup='host')
    with pytest.raises(ValueError, match="mutual_lookup='gather' belongs to grid_size=None"):
        engine.solve_puzzle(dq, (4, 6), mutual_lookup='gather')
    with pytest.raises(ValueError, match=r'neither \[4, n, n\] nor \[4, n, n, 4\]'):
        engine.solve_puzzle(dq[:, :, :5], None)
    check = engine.puzzle_mixed.check_solve_arguments
    assert check(None, 1, None) == 'gather' and check(None, 3, None) == 'gather' and check((4, 6), 1, None) == 'mirror'
    assert check(None, 2, 'mirror') == 'mirror'
    p = inspect.signature(engine.solve_pixel_puzzle).parameters
    assert p['grid_size'].default == 'cut' and p['numb_puzzles'].default is None and p['grid_size'].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(p)[:6] == ['image', 'piece_width', 'erosion', 'order', 'marker', 'puzzle_type']


def test_the_old_solution_still_constructs_and_the_new_one_is_one(vited):
    engine = vited.engine
    loc = np.array([[0, 0], [0, 1]])
    old = engine.PuzzleSolution(loc, loc, np.arange(2), 0, None)
    assert len(old) == 6 and old.rotations is None and engine.PuzzleSolution._fields[-1] == 'rotations'
    new = mc.golden_solution(engine, 'b')
    assert isinstance(new, engine.PuzzleSolution) and len(new) == 6 and new.rotations is None and new.numb_boards == 3
    assert new[:4] == (new.locations, new.board_locations, new.order, new.recalcs) and new.grid is new.grids[0]
    assert [g.shape for g in new.grids] == [(3, 4), (2, 3), (7, 6)] and mc.golden_solution(engine, 'e').rotations is not None
    assert engine.PuzzleCut(None, None, (3, 4), 13).true_puzzle is None


# ---- accuracies ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', mc.CASES)
def test_accuracy_of_several_puzzles_is_the_reference_s(vited, name):
    g = mc.case(name)
    acc = vited.engine.puzzle_accuracy(mc.golden_solution(vited.engine, name), g['true_loc'], true_puzzle=g['true_puzzle'])
    mc.assert_accuracy(acc, name)
    assert all(len(v) == len(g['acc']) for v in acc.values())


def test_accuracy_weights_and_the_zip_of_results_with_boards(vited):
    """Case b by hand: original puzzle i is scored on board i alone, and the pieces of other puzzles on that board weigh in - once in
    the direct accuracies, four times (once per side) in the neighbour accuracy."""
    g, engine = mc.case('b'), vited.engine
    sol = mc.golden_solution(engine, 'b')
    acc = engine.puzzle_accuracy(sol, g['true_loc'], true_puzzle=g['true_puzzle'])
    loc = mc.relative_locations(g)
    for k in range(3):
        on = g['board'] == k
        mine = on & (g['true_puzzle'] == k)
        different = int((on & (g['true_puzzle'] != k)).sum())
        assert different == int(g['different_puzzle'][k])
        pieces = int((g['true_puzzle'] == k).sum())
        correct = int((loc[mine] == g['true_loc'][mine]).all(axis=1).sum())
        assert acc['Direct_Standard'][k] == correct / (pieces + different)
        sides = acc['neighbor'][k] * 4 * (pieces + 4 * different)                   # the correct sides: a whole number under that weight
        assert abs(sides - round(sides)) < 1e-9 and int(g['wrong_puzzle_id'][k]) == 4 * different
    assert g['different_puzzle'].tolist() == [0, 5, 16]
    # puzzles handed over in another order are scored against other boards: the zip, not a best match
    swapped = np.where(g['true_puzzle'] == 0, 2, np.where(g['true_puzzle'] == 2, 0, 1))
    other = engine.puzzle_accuracy(sol, g['true_loc'], true_puzzle=swapped)
    assert other['Direct_Standard'] != acc['Direct_Standard']


def test_accuracy_without_true_puzzle_is_unchanged(vited):
    engine = vited.engine
    g = mc.case('d')
    sol = mc.golden_solution(engine, 'd')
    one = engine.puzzle_accuracy(sol, g['true_loc'])
    assert [one['Direct_Standard'], one['Direct_Modified'], one['neighbor']] == g['acc'][0].tolist() and one['perfect'] is False
    plain = engine.PuzzleSolution(sol.locations, sol.board_locations, sol.order, sol.recalcs, sol.grid)
    assert engine.puzzle_accuracy(plain, g['true_loc']) == one
    fixed = np.load(mc.GOLDEN + '/puzzle_4x4.npz')
    loc = fixed['final_loc'] - fixed['final_loc'].min(axis=0)
    old = engine.puzzle_accuracy(engine.PuzzleSolution(loc, fixed['final_loc'], fixed['order'], int(fixed['recalcs']), None), fixed['true_loc'])
    assert [old['Direct_Standard'], old['Direct_Modified'], old['neighbor']] == fixed['acc'].tolist()
    with pytest.raises(ValueError, match='scored with true_puzzle'):
        engine.puzzle_accuracy(mc.golden_solution(engine, 'a'), mc.case('a')['true_loc'])
    with pytest.raises(ValueError, match='true_puzzle must be'):
        engine.puzzle_accuracy(mc.golden_solution(engine, 'a'), mc.case('a')['true_loc'], true_puzzle=np.zeros(3, np.int64))


# ---- extents -------------------------------------------------------------------------------------------------------------------------
def test_extents_follow_the_reference_s_if_elif(vited):
    grow = vited.engine.puzzle_mixed.grow_extents
    top_left, bottom_right = [5, 5], [5, 5]
    grow(top_left, bottom_right, (5, 6))
    assert (top_left, bottom_right) == ([5, 5], [5, 6])
    grow(top_left, bottom_right, (4, 6))
    assert (top_left, bottom_right) == ([4, 5], [5, 6])
    grow(top_left, bottom_right, (6, 4))                                            # both dimensions move, each on its own branch
    assert (top_left, bottom_right) == ([4, 4], [6, 6])
    grow(top_left, bottom_right, (5, 5))                                            # inside: nothing moves
    assert (top_left, bottom_right) == ([4, 4], [6, 6])
    top_left, bottom_right = [3, 3], [2, 2]                                         # per dimension it is either corner, never both
    grow(top_left, bottom_right, (0, 9))
    assert (top_left, bottom_right) == ([0, 3], [2, 9])
    for name in mc.CASES:                                                           # the placements of the reference, replayed
        g = mc.case(name)
        corners = {}
        for piece in g['order']:
            loc, b = g['final_loc'][piece].tolist(), int(g['board'][piece])
            if b not in corners:
                corners[b] = (list(loc), list(loc))
            grow(*corners[b], loc)
        assert [corners[b][0] for b in sorted(corners)] == g['top_left'].tolist()
        assert [corners[b][1] for b in sorted(corners)] == g['bottom_right'].tolist()
        seeds = [next(k for k, piece in enumerate(g['order']) if g['board'][piece] == b) for b in sorted(corners)]
        assert seeds == g['spawns'].tolist()                                        # a board's seed is its first placed piece


# ---- the C entries and the wrapper ---------------------------------------------------------------------------------------------------
def test_gather_entries_refuse_bad_arguments_before_any_launch(vited):
    L = vited._lib
    lib = L.load()
    i, i64, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    a = 4096                                                                        # a non-null address that is never dereferenced
    for name in ('vited_puzzle_mutual_gather', 'vited_puzzle_mutual_gather2'):
        assert L.SIGNATURES[name] == (i, [p, i64, p, i64, p, p, p])
        fn = getattr(lib, name)
        assert fn(None, 6, a, 3, a, a, None) == BAD and fn(a, 6, None, 3, a, a, None) == BAD and fn(a, 6, a, 3, None, a, None) == BAD
        assert fn(a, 6, a, 3, a, None, None) == BAD and fn(a, 6, a, -1, a, a, None) == BAD
        assert fn(a, 1, a, 3, a, a, None) == BAD and fn(a, 46341, a, 3, a, a, None) == BAD
        assert fn(a, 6, a, 2 ** 31, a, a, None) == UNSUPPORTED
        assert fn(a, 6, a, 0, a, a, None) == 0                                      # nothing to look up: no launch


@pytest.fixture
def ops(vited, monkeypatch):
    calls = []
    monkeypatch.setattr(vited.ops, '_need_gpu', lambda *tensors, **kw: None)
    monkeypatch.setattr(vited.ops, '_stream', lambda: 0)
    monkeypatch.setattr(vited.ops, '_lib', SimpleNamespace(call=lambda name, *args: calls.append((name, args))))
    vited.ops.calls = calls
    yield vited.ops


def test_wrapper_picks_the_entry_by_rank_and_checks_every_tensor(ops):
    N, m = 6, 5
    f, i32 = (lambda *s: torch.zeros(*s)), (lambda *s: torch.zeros(*s, dtype=torch.int32))
    out = ops.puzzle_mutual_gather(f(4, N, N), i32(m, 3))
    assert out.shape == (m,) and out.dtype == torch.float32
    name, args = ops.calls.pop()
    assert name == 'vited_puzzle_mutual_gather' and args[1] == N and args[3] == m and not ops.calls
    given, bad = f(m), i32(1)
    assert ops.puzzle_mutual_gather(f(4, N, N, 4), i32(m, 4), out=given, bad=bad) is given
    name, args = ops.calls.pop()
    assert name == 'vited_puzzle_mutual_gather2' and args[4] == given.data_ptr() and args[5] == bad.data_ptr()
    words = f(m + 1)                                                                # the engine's layout: the flag word, then the values
    ops.puzzle_mutual_gather(f(4, N, N), i32(m, 3), out=words[1:], bad=words[:1].view(torch.int32))
    assert ops.calls.pop()[1][4] == words.data_ptr() + 4
    refused = [
        ('mutual', lambda: ops.puzzle_mutual_gather(f(4, N), i32(m, 3))),
        ('mutual', lambda: ops.puzzle_mutual_gather(f(4, N, N).double(), i32(m, 3))),
        ('mutual', lambda: ops.puzzle_mutual_gather(f(4, N, N + 1), i32(m, 3))),
        ('mutual', lambda: ops.puzzle_mutual_gather(f(4, N, N, 3), i32(m, 4))),
        ('lookups', lambda: ops.puzzle_mutual_gather(f(4, N, N), i32(m, 4))),       # a type-2 lookup into a type-1 tensor
        ('lookups', lambda: ops.puzzle_mutual_gather(f(4, N, N, 4), i32(m, 3))),
        ('lookups', lambda: ops.puzzle_mutual_gather(f(4, N, N), i32(m, 3).long())),
        ('lookups', lambda: ops.puzzle_mutual_gather(f(4, N, N), i32(m, 6)[:, ::2])),
        ('lookups', lambda: ops.puzzle_mutual_gather(f(4, N, N), i32(3 * m))),
        ('out', lambda: ops.puzzle_mutual_gather(f(4, N, N), i32(m, 3), out=f(m + 1))),
        ('out', lambda: ops.puzzle_mutual_gather(f(4, N, N), i32(m, 3), out=i32(m))),
        ('bad', lambda: ops.puzzle_mutual_gather(f(4, N, N), i32(m, 3), bad=i32(2))),
        ('bad', lambda: ops.puzzle_mutual_gather(f(4, N, N), i32(m, 3), bad=f(1))),
    ]
    for argument, call in refused:
        with pytest.raises(ValueError, match=rf'^puzzle_mutual_gather: {argument}\b'):
            call()
        assert not ops.calls, argument
