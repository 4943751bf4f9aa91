"""Type-2 puzzles (pieces of unknown rotation) on the MI355X: the 16-pairing border distances, the compatibility kernels over (piece, side)
candidates, the slot scan, engine.solve_puzzle / solve_pixel_puzzle and the board of rotated pieces, against the fixtures the reference's
own solver wrote (tests/golden/rot_puzzle_*.npz, rot_pixel_puzzle_*.npz) and the numpy rules of tests/puzzle_type2_cases.py.  Every quantity
is an integer or a bit-defined fp32: exact equality throughout."""
import numpy as np
import pytest
import torch

import puzzle_pixels_cases as pc
import puzzle_type2_cases as t2

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


def _dev(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)                # a copy: the fixtures are read-only


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


# ---- the distances -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', t2.PIXEL)
def test_distances_equal_the_reference_and_hold_the_type1_kernel_output(gpu, vited, name):
    ops, g = vited.ops, t2.fixture(name)
    n = g['pieces'].shape[0]
    pieces = _dev(g['pieces'], gpu)
    dq2 = torch.full((4, n, n, 4), -7, dtype=torch.int32, device=gpu)     # a sentinel no distance equals: an element left out shows
    assert ops.puzzle_pixel_distances(pieces, out=dq2, puzzle_type=2) is dq2
    np.testing.assert_array_equal(dq2.cpu().numpy(), g['Dq2'])
    dq = ops.puzzle_pixel_distances(pieces)
    for s in range(4):
        assert torch.equal(dq2[s, :, :, (s + 2) % 4], dq[s])
    assert torch.equal(vited.engine.puzzle_pixel_distances(pieces, puzzle_type=2), dq2)


@pytest.mark.parametrize('name', sorted(t2.SHAPES))
def test_distances_at_the_tiling_edges(gpu, vited, name):
    pieces = t2.shape_pieces(name)
    n = pieces.shape[0]
    dev = _dev(pieces, gpu)
    first = torch.full((4, n, n, 4), -7, dtype=torch.int32, device=gpu)
    vited.ops.puzzle_pixel_distances2(dev, out=first)
    second = vited.ops.puzzle_pixel_distances2(dev)
    got = first.cpu().numpy()
    np.testing.assert_array_equal(got, t2.distances2(pieces))
    assert (got[:, np.arange(n), np.arange(n), :] == 2 ** 31 - 1).all()
    assert torch.equal(first, second)
    dq = vited.ops.puzzle_pixel_distances(dev)
    for s in range(4):
        assert torch.equal(first[s, :, :, (s + 2) % 4], dq[s])


# ---- the compatibility stage -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', t2.SYNTHETIC + t2.PIXEL)
def test_compat_init_matches_the_reference(gpu, vited, name):
    g = t2.fixture(name)
    comp = vited.engine.PuzzleCompatibility(_dev(t2.dq2_of(g), gpu))
    assert comp.puzzle_type == 2
    np.testing.assert_array_equal(comp.min_d.cpu().numpy(), g['min_d'])
    np.testing.assert_array_equal(comp.second_d.cpu().numpy(), g['second_d'])
    np.testing.assert_array_equal(comp.best_buddy.cpu().numpy(), g['bb'])
    order = g['start_order']
    np.testing.assert_array_equal(comp.start_order.cpu().numpy(), order)
    np.testing.assert_array_equal(comp.start_count.cpu().numpy()[order], g['start_count'])
    np.testing.assert_array_equal(_bits(comp.start_total)[order], g['start_total'].view(np.uint32))
    if 'C' in g:
        np.testing.assert_array_equal(_bits(comp.compat), g['C'].view(np.uint32))
        np.testing.assert_array_equal(_bits(comp.mutual), g['M'].view(np.uint32))


@pytest.mark.parametrize('name', ['rot_puzzle_4x4', 'rot_pixel_puzzle_poster_5x6'])
def test_compat_init_matches_the_numpy_rules(gpu, vited, name):
    """The whole state, C and M included, on a tie-free case and on the posterised one (zeros, ties, second == 0)."""
    dq2 = t2.dq2_of(t2.fixture(name))
    mn, sec, cnt, cand, C, M = t2.init_state(dq2)
    comp = vited.engine.PuzzleCompatibility(_dev(dq2, gpu))
    np.testing.assert_array_equal(comp.min_d.cpu().numpy(), mn)
    np.testing.assert_array_equal(comp.second_d.cpu().numpy(), sec)
    np.testing.assert_array_equal(comp.min_count.cpu().numpy(), cnt)
    np.testing.assert_array_equal(comp.candidate.cpu().numpy(), cand)
    np.testing.assert_array_equal(_bits(comp.compat), C.view(np.uint32))
    np.testing.assert_array_equal(_bits(comp.mutual), M.view(np.uint32))
    if name == 'rot_pixel_puzzle_poster_5x6':
        assert (cnt > 1).any() and (sec == 0).any() and (C == np.float32(-t2.MAXSIZE)).any()


def test_recalc_follows_the_reference_rules(gpu, vited):
    """One recalculation with about half the pieces placed against the numpy statement of recalculate_remaining_piece_compatibilities."""
    dq2 = t2.dq2_of(t2.fixture('rot_puzzle_ties_7x8'))
    n = dq2.shape[1]
    comp = vited.engine.PuzzleCompatibility(_dev(dq2, gpu))
    C0, M0 = comp.compat.cpu().numpy().copy(), comp.mutual.cpu().numpy().copy()
    mn0, sec0 = comp.min_d.cpu().numpy().copy(), comp.second_d.cpu().numpy().copy()
    bb0, order0 = comp.best_buddy.cpu().numpy().copy(), comp.start_order.cpu().numpy().copy()
    placed = np.random.default_rng(5).random(n) < 0.5
    changed = comp.recalc(placed).cpu().numpy().astype(bool)
    want_changed, mn, sec, C, M = t2.recalc_state(dq2, placed, mn0, sec0, C0, M0)
    np.testing.assert_array_equal(changed, want_changed)
    assert want_changed.any() and (~want_changed & ~placed).any() and 0.3 < placed.mean() < 0.7
    np.testing.assert_array_equal(comp.min_d.cpu().numpy(), mn)
    np.testing.assert_array_equal(comp.second_d.cpu().numpy(), sec)
    np.testing.assert_array_equal(_bits(comp.compat), C.view(np.uint32))
    np.testing.assert_array_equal(_bits(comp.mutual), M.view(np.uint32))
    assert (C != C0).any() and (C[:, :, placed] == C0[:, :, placed]).all()           # stale C at placed j
    np.testing.assert_array_equal(comp.best_buddy.cpu().numpy(), bb0)                # best buddies and the start order untouched
    np.testing.assert_array_equal(comp.start_order.cpu().numpy(), order0)


@pytest.mark.parametrize('n,seed', [(16, 0), (16, 1), (17, 2), (17, 3), (72, 4), (72, 5)])
def test_best_slot_matches_a_brute_force_scan(gpu, vited, n, seed):
    rng = np.random.default_rng(seed)
    comp = vited.engine.PuzzleCompatibility(_dev(rng.integers(0, 1000, size=(4, n, n, 4)).astype(np.int32), gpu))
    M = rng.choice(np.float32([-2.0, -0.5, 0.0, 0.25, 0.5, 0.75]), size=(4, n, n, 4)).astype(np.float32)
    top = np.float32(0.9)
    placed = rng.random(n) < rng.uniform(0.2, 0.8)
    placed[1], placed[0], placed[n - 1] = True, False, False
    k = int(rng.integers(2, 40))
    slot_piece = rng.choice(np.flatnonzero(placed), size=k)
    slot_side = rng.integers(0, 4, size=k)
    # planted ties of the maximum across pieces, sides and slots: the first in scan order must win
    unplaced = np.flatnonzero(~placed)
    for p, kk, side in zip(rng.choice(unplaced, size=5), rng.integers(0, k, size=5), rng.integers(0, 4, size=5)):
        M[side, p, slot_piece[kk], slot_side[kk]] = top
    p = unplaced[-1]                                       # and two in one (piece, slot), on different sides
    M[1, p, slot_piece[k - 1], slot_side[k - 1]] = M[3, p, slot_piece[k - 1], slot_side[k - 1]] = top
    comp.state['mutual'].copy_(torch.from_numpy(M))
    got = comp.best_slot(placed, slot_piece, slot_side)
    want = t2.brute_force_slot(M, placed, slot_piece, slot_side)
    assert got[:3] == want[:3] and got[3] == float(want[3]) == float(top)


def test_best_slot_negative_zero_and_last_candidate(gpu, vited):
    n = 8
    comp = vited.engine.PuzzleCompatibility(torch.zeros((4, n, n, 4), dtype=torch.int32, device=gpu))
    M = np.full((4, n, n, 4), -1.0, np.float32)
    placed = np.array([1, 0, 0, 0, 0, 0, 0, 1], bool)
    M[2, 3, 0, 1] = -0.0                     # scanned after (piece 1, slot 1, side 0) holding +0.0: equal, so the earlier one wins
    M[0, 1, 7, 2] = 0.0
    comp.state['mutual'].copy_(torch.from_numpy(M))
    assert comp.best_slot(placed, [0, 7], [1, 2])[:3] == (1, 1, 0)
    M[:] = -1.0
    M[3, 6, 7, 2] = 0.5                      # the very last candidate of the scan
    comp.state['mutual'].copy_(torch.from_numpy(M))
    assert comp.best_slot(placed, [0, 7], [1, 2]) == (6, 1, 3, 0.5)


# ---- the solver ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', t2.SYNTHETIC)
def test_solve_puzzle_reproduces_the_reference(gpu, vited, name):
    engine, g = vited.engine, t2.fixture(name)
    sol = engine.solve_puzzle(_dev(t2.dq2_of(g), gpu), tuple(int(v) for v in g['grid']))
    np.testing.assert_array_equal(sol.order, g['order'])
    np.testing.assert_array_equal(sol.board_locations, g['final_loc'])
    np.testing.assert_array_equal(sol.rotations, g['rotations'])
    assert sol.recalcs == int(g['recalcs']) and sol.rotations.dtype == np.int64
    acc = engine.puzzle_accuracy(sol, g['true_loc'])
    assert [acc['Direct_Standard'], acc['Direct_Modified'], acc['neighbor']] == g['acc'].tolist()
    assert acc['perfect'] == bool(g['perfect']) and acc['wrong_rotation'] == int(g['wrong_rotation'])


@pytest.mark.parametrize('name', t2.PIXEL)
def test_solve_pixel_puzzle_reproduces_the_reference_run(gpu, vited, name):
    engine, g = vited.engine, t2.fixture(name)
    P = int(g['piece_width'])
    run = lambda: engine.solve_pixel_puzzle(np.array(g['image']), P, float(g['erosion']), order=g['perm'], marker=pc.REFERENCE_MARKER,
                                            puzzle_type=2)
    solution, acc, board = run()
    np.testing.assert_array_equal(solution.board_locations, g['final_loc'])
    np.testing.assert_array_equal(solution.locations, t2.locations(g))
    np.testing.assert_array_equal(solution.rotations, g['rotations'])
    np.testing.assert_array_equal(solution.order, g['order'])
    assert solution.recalcs == int(g['recalcs'])
    assert [acc['Direct_Standard'], acc['Direct_Modified'], acc['neighbor']] == g['acc'].tolist()
    assert acc['perfect'] == bool(g['perfect']) and acc['wrong_rotation'] == int(g['wrong_rotation'])
    np.testing.assert_array_equal(board.cpu().numpy(), g['board'])
    again = run()                                           # two runs: identical bits
    assert torch.equal(again[2], board) and np.array_equal(again[0].rotations, solution.rotations) and again[1] == acc


def test_type1_calls_keep_their_results(gpu, vited):
    """The default puzzle_type is 1: a PuzzleSolution without rotations, the four accuracy keys, the reference's type-1 board."""
    engine, g = vited.engine, pc.fixture('pixel_puzzle_half_6x5')
    solution, acc, board = engine.solve_pixel_puzzle(np.array(g['image']), 13, 0.25, order=g['perm'], marker=pc.REFERENCE_MARKER)
    assert solution.rotations is None and set(acc) == {'Direct_Standard', 'Direct_Modified', 'neighbor', 'perfect'}
    np.testing.assert_array_equal(solution.board_locations, g['final_loc'])
    np.testing.assert_array_equal(board.cpu().numpy(), g['board'])


def test_two_runs_are_bit_identical(gpu, vited):
    dq2 = _dev(t2.dq2_of(t2.fixture('rot_puzzle_noisy_9x11')), gpu)
    a, b = vited.engine.PuzzleCompatibility(dq2), vited.engine.PuzzleCompatibility(dq2)
    placed = np.random.default_rng(1).random(dq2.shape[1]) < 0.5
    for comp in (a, b):
        comp.recalc(placed)
    for key in ('min_d', 'second_d', 'min_count', 'candidate', 'best_buddy', 'start_count', 'start_order'):
        assert torch.equal(a.state[key], b.state[key]), key
    for key in ('compat', 'mutual', 'start_total'):
        assert torch.equal(a.state[key].view(torch.int32), b.state[key].view(torch.int32)), key
    slots = np.flatnonzero(placed)[:9]
    assert a.best_slot(placed, slots, slots % 4) == b.best_slot(placed, slots, slots % 4)


# ---- the board -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('We,P', [(5, 7), (6, 8), (5, 5)])
def test_reconstruct_puzzle_places_rot90_pieces(gpu, vited, We, P):
    """Forced rotations 0..3 on a 2 x 3 board, odd and even We: every piece enters as numpy.rot90(piece, r), framed by its location alone."""
    engine = vited.engine
    pieces = np.random.default_rng(We).integers(0, 256, size=(6, We, We, 3), dtype=np.uint8)
    true = np.stack([np.arange(6) // 3, np.arange(6) % 3], axis=1)
    loc = true[[1, 0, 2, 3, 5, 4]]                          # four pieces misplaced, two at home
    rot = np.array([0, 1, 2, 3, 1, 3])
    marker = pc.REFERENCE_MARKER if pc.pad_of(P, We) >= 1 else None
    sol = engine.PuzzleSolution(loc, loc, np.arange(6), 0, None, rot)
    board = torch.full((2 * P, 3 * P, 3), SENTINEL, dtype=torch.uint8, device=gpu)
    out = vited.ops.puzzle_assemble2(_dev(pieces, gpu), loc, rot, true, P, marker=marker, out=board)
    assert out is board
    want = t2.board2(pieces, loc, rot, true, P, marker)
    np.testing.assert_array_equal(board.cpu().numpy(), want)
    np.testing.assert_array_equal(engine.reconstruct_puzzle(_dev(pieces, gpu), sol, true, P, marker).cpu().numpy(), want)
    pad = pc.pad_of(P, We)
    for k in range(6):
        y, x = loc[k, 0] * P + pad, loc[k, 1] * P + pad
        np.testing.assert_array_equal(want[y:y + We, x:x + We], np.rot90(pieces[k], rot[k]))
    flat = engine.reconstruct_puzzle(_dev(pieces, gpu), sol._replace(rotations=np.zeros(6, np.int64)), true, P, marker)
    assert torch.equal(flat, engine.reconstruct_puzzle(_dev(pieces, gpu), sol._replace(rotations=None), true, P, marker))


def test_bad_arguments_raise(gpu, vited):
    engine, ops = vited.engine, vited.ops
    with pytest.raises(ValueError):
        engine.solve_puzzle(torch.zeros((4, 6, 6, 4), dtype=torch.int32, device=gpu), (2, 4))
    with pytest.raises(ValueError):
        engine.solve_puzzle(torch.zeros((4, 6, 6, 3), dtype=torch.int32, device=gpu), (2, 3))
    with pytest.raises(ValueError, match='^puzzle_compat2_init: dq2'):
        ops.puzzle_compat2_init(torch.zeros((4, 6, 5, 4), dtype=torch.int32, device=gpu))
    with pytest.raises(ValueError, match='^puzzle_pixel_distances: puzzle_type'):
        engine.puzzle_pixel_distances(torch.zeros((6, 5, 5, 3), dtype=torch.uint8, device=gpu), puzzle_type=0)
