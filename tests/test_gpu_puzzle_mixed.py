"""Mixed-bag and unknown-dimension puzzles on the MI355X: the point lookups of the mutual compatibility against
torch's indexing bit for bit, engine.solve_puzzle without dimensions against the reference's own placements
(tests/golden/mixed_puzzle.npz) with both lookup modes, the fixed-size path left as it was, and the pixel driver on a list of images."""
import numpy as np
import pytest
import torch

import puzzle_mixed_cases as mc
import puzzle_pixels_cases as pc

pytestmark = pytest.mark.gpu

PATTERN = 0x5a5aa5a5                                    # the fill of an output nothing may touch
N = 9


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


@pytest.fixture(scope='module')
def planted(gpu):
    """puzzle type -> (PuzzleCompatibility of random distances, the cells planted with -0.0, inf and the fp32 image of -maxsize)."""
    from vited_amd import engine
    out = {}
    for puzzle_type, shape in ((1, (4, N, N)), (2, (4, N, N, 4))):
        rng = np.random.default_rng(60 + puzzle_type)
        dq = rng.integers(0, 1000, size=shape).astype(np.int32)
        dq[:, np.arange(N), np.arange(N)] = 2 ** 31 - 1
        comp = engine.PuzzleCompatibility(torch.from_numpy(dq).to(gpu))
        cells = [(0, 1, 2), (3, 8, 0), (2, 4, 7), (1, 0, 8)]
        cells = cells if puzzle_type == 1 else [c + (k,) for k, c in enumerate(cells)]
        for cell, value in zip(cells, (-0.0, float('inf'), float(-(2 ** 63 - 1)), float('-inf'))):
            comp.mutual[cell] = value
        torch.cuda.synchronize()
        assert _bits(comp.mutual[cells[0]].reshape(1))[0] == -2 ** 31                 # the sign bit alone: -0.0 went in as it is
        out[puzzle_type] = (comp, cells)
    return out


def _lookups(puzzle_type, m, cells, seed):
    rng = np.random.default_rng(seed)
    width = 3 if puzzle_type == 1 else 4
    look = np.stack([rng.integers(0, 4, m), rng.integers(0, N, m), rng.integers(0, N, m), rng.integers(0, 4, m)], axis=1)[:, :width]
    take = min(m, len(cells))
    look[:take] = np.array(cells)[rng.permutation(len(cells))[:take]]               # the planted cells first, the diagonal's inf by chance
    return look.astype(np.int32)


@pytest.mark.parametrize('m', (1, 7, 70))
@pytest.mark.parametrize('puzzle_type', (1, 2))
def test_mutual_gather_is_torch_indexing_bit_for_bit(gpu, planted, puzzle_type, m):
    from vited_amd import ops
    comp, cells = planted[puzzle_type]
    look = _lookups(puzzle_type, m, cells, 100 * puzzle_type + m)
    look_dev = torch.from_numpy(look).to(gpu)
    want = _bits(comp.mutual[tuple(torch.from_numpy(look.astype(np.int64)).to(gpu).unbind(1))])
    runs = []
    for _ in range(2):
        room = torch.full((m + 16,), PATTERN, dtype=torch.int32, device=gpu).view(torch.float32)
        bad = torch.zeros(1, dtype=torch.int32, device=gpu)
        out = ops.puzzle_mutual_gather(comp.mutual, look_dev, out=room[8:8 + m], bad=bad)
        torch.cuda.synchronize()
        assert out.data_ptr() == room.data_ptr() + 32 and int(bad.item()) == 0
        got = _bits(room)
        np.testing.assert_array_equal(got[8:8 + m], want)
        assert (got[:8] == PATTERN).all() and (got[8 + m:] == PATTERN).all()       # only the m slots changed
        runs.append(got)
    np.testing.assert_array_equal(runs[0], runs[1])
    if m >= 4:
        assert {-2 ** 31, 0x7f800000}.issubset(set(want[:4].tolist()))               # -0.0 and inf were among the lookups
    np.testing.assert_array_equal(comp.mutual_at(look).view(np.int32), want)       # the engine's path: pinned buffer, one read
    np.testing.assert_array_equal(comp.mutual_at(look.tolist()).view(np.int32), want)


@pytest.mark.parametrize('puzzle_type', (1, 2))
def test_mutual_gather_flags_an_index_outside_the_tensor_and_leaves_its_slot(gpu, planted, puzzle_type):
    from vited_amd import ops
    comp, cells = planted[puzzle_type]
    look = _lookups(puzzle_type, 7, cells, 7)
    outside = {1: (0, N, 0, 0), 2: (4, 0, 0, 0), 4: (0, 0, -1, 0), 5: (-1, 0, 0, 0)}
    if puzzle_type == 2:
        outside[6] = (0, 0, 0, 4)
    for row, values in outside.items():
        look[row] = values[:look.shape[1]]
    inside = [r for r in range(7) if r not in outside]
    want = _bits(comp.mutual[tuple(torch.from_numpy(look[inside].astype(np.int64)).to(gpu).unbind(1))])
    room = torch.full((7,), PATTERN, dtype=torch.int32, device=gpu).view(torch.float32)
    bad = torch.zeros(1, dtype=torch.int32, device=gpu)
    ops.puzzle_mutual_gather(comp.mutual, torch.from_numpy(look).to(gpu), out=room, bad=bad)
    torch.cuda.synchronize()
    got = _bits(room)
    assert int(bad.item()) == 1
    np.testing.assert_array_equal(got[inside], want)
    assert (got[sorted(outside)] == PATTERN).all()
    with pytest.raises(IndexError, match='mutual_at'):
        comp.mutual_at(look)
    np.testing.assert_array_equal(comp.mutual_at(look[inside]).view(np.int32), want)        # the flag does not stick
    assert comp.mutual_at(np.empty((0, look.shape[1]), np.int32)).shape == (0,)


@pytest.fixture
def gather_calls(monkeypatch):
    """The number of lookups of every ``ops.puzzle_mutual_gather`` call, the op itself still running."""
    from vited_amd import ops
    calls, real = [], ops.puzzle_mutual_gather

    def spy(mutual, lookups, *a, **k):
        calls.append(int(lookups.shape[0]))
        return real(mutual, lookups, *a, **k)

    monkeypatch.setattr(ops, 'puzzle_mutual_gather', spy)
    return calls


@pytest.mark.parametrize('name', mc.CASES)
def test_solve_puzzle_reproduces_the_reference_without_dimensions(gpu, gather_calls, name):
    from vited_amd import engine
    g = mc.case(name)
    dq = torch.from_numpy(mc.distances(name)).to(gpu)
    keywords = dict(numb_puzzles=int(g['numb_puzzles']), new_board_mutual_compatibility=float(g['threshold']))
    gathered = engine.solve_puzzle(dq, None, **keywords)                            # 'gather' is the default without dimensions
    assert isinstance(gathered, engine.PuzzleBoards) and gather_calls and min(gather_calls) >= 1
    mc.assert_solution(gathered, name)
    del gather_calls[:]
    mirrored = engine.solve_puzzle(dq, None, mutual_lookup='mirror', **keywords)
    assert not gather_calls
    mc.assert_solution(mirrored, name)
    for a, b in zip(gathered.grids, mirrored.grids):
        np.testing.assert_array_equal(a, b)
    mc.assert_accuracy(engine.puzzle_accuracy(gathered, g['true_loc'], true_puzzle=g['true_puzzle']), name)


def test_the_fixed_size_path_makes_no_lookup_and_returns_what_it_returned(gpu, gather_calls):
    from vited_amd import engine
    g = np.load(mc.GOLDEN + '/puzzle_4x4.npz')
    dq = torch.from_numpy(g['Dq'].astype(np.int32))
    for s in range(4):
        dq[s].fill_diagonal_(2 ** 31 - 1)
    sol = engine.solve_puzzle(dq.to(gpu), (4, 4))
    assert not gather_calls and type(sol) is engine.PuzzleSolution and len(sol) == 6 and sol.rotations is None
    np.testing.assert_array_equal(sol.order, g['order'])
    np.testing.assert_array_equal(sol.board_locations, g['final_loc'])
    assert sol.recalcs == int(g['recalcs']) and sol.grid.shape == (4, 4)
    with pytest.raises(ValueError, match='only a single puzzle is allowed'):
        engine.solve_puzzle(dq.to(gpu), (4, 4), numb_puzzles=2)


def test_solve_pixel_puzzle_on_a_list_of_images(gpu):
    """Two images of 3 x 4 pieces, pooled and shuffled as the reference's run was: its placements, its board images (frames around the
    misplaced pieces, black where a board has no piece) and its accuracies."""
    from vited_amd import engine
    g = mc.case('p')
    P, erosion = int(g['piece_width']), float(g['erosion'])
    images = [torch.from_numpy(np.array(g[f'image{k}'])).to(gpu) for k in range(2)]
    cut = engine.cut_puzzle(images, P, erosion, order=g['perm'])
    np.testing.assert_array_equal(cut.pieces.cpu().numpy(), g['pieces'])
    np.testing.assert_array_equal(cut.true_locations, g['true_loc'])
    np.testing.assert_array_equal(cut.true_puzzle, g['true_puzzle'])
    assert cut.grid_size == ((3, 4), (3, 4))
    sol, acc, boards = engine.solve_pixel_puzzle(images, P, erosion, order=g['perm'], marker=pc.REFERENCE_MARKER)
    mc.assert_solution(sol, 'p')
    assert acc == engine.puzzle_accuracy(sol, g['true_loc'], true_puzzle=g['true_puzzle'])
    mc.assert_accuracy(acc, 'p')
    assert len(boards) == 2 and any((grid < 0).any() for grid in sol.grids)         # a board with empty cells among them
    loc = mc.relative_locations(g)
    for b, board in enumerate(boards):
        on = g['board'] == b
        want = pc.board(g['pieces'][on], loc[on], g['true_loc'][on], P, marker=pc.REFERENCE_MARKER)
        np.testing.assert_array_equal(want, g[f'board{b}'])                         # numpy's assembly is the reference's image
        np.testing.assert_array_equal(board.cpu().numpy(), want)
    with pytest.raises(ValueError, match='only a single puzzle is allowed'):
        engine.solve_pixel_puzzle(images, P, erosion, grid_size=(4, 6))


def test_one_image_without_dimensions(gpu):
    from vited_amd import engine
    g = mc.case('p')
    P, erosion = int(g['piece_width']), float(g['erosion'])
    image = torch.from_numpy(np.array(g['image0'])).to(gpu)
    order = np.random.default_rng(3).permutation(12)
    sol, acc, boards = engine.solve_pixel_puzzle(image, P, erosion, order=order, grid_size=None)
    assert isinstance(sol, engine.PuzzleBoards) and sol.numb_boards == 1 and len(boards) == 1 and sol.spawns.tolist() == [0]
    cut = engine.cut_puzzle(image, P, erosion, order)
    again = engine.solve_puzzle(engine.puzzle_pixel_distances(cut.pieces), None, mutual_lookup='mirror')
    np.testing.assert_array_equal(sol.board_locations, again.board_locations)
    np.testing.assert_array_equal(sol.order, again.order)
    assert acc == engine.puzzle_accuracy(sol, cut.true_locations) and isinstance(acc['Direct_Standard'], float)
    rows, cols = sol.grid.shape
    assert boards[0].shape == (rows * P, cols * P, 3)
    np.testing.assert_array_equal(boards[0].cpu().numpy(), pc.board(cut.pieces.cpu().numpy(), sol.locations, cut.true_locations, P))
    fixed, fixed_acc, fixed_board = engine.solve_pixel_puzzle(image, P, erosion, order=order)       # the default is still the cut's grid
    assert type(fixed) is engine.PuzzleSolution and torch.is_tensor(fixed_board) and isinstance(fixed_acc['neighbor'], float)
