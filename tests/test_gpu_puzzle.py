"""Puzzle evaluation on the MI355X: the Paikin-Tal compatibility kernels (csrc/puzzle_compat.hip) against the reference's own
state (tests/golden/puzzle_*.npz), engine.solve_puzzle against the reference's placements, the slot scan against a brute-force
scan, the logit quantisation against numpy, and engine.puzzle_distances against the model run on stacked pairs."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import vited_oracle as vo

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'puzzle_*.npz')))


def load(name, dev):
    g = dict(np.load(os.path.join(GOLDEN, name + '.npz')))
    dq = torch.from_numpy(g['Dq'].astype(np.int32))
    for s in range(4):
        dq[s].fill_diagonal_(2 ** 31 - 1)
    return g, dq.to(dev)


@pytest.mark.parametrize('name', CASES)
def test_compat_init_matches_the_reference(gpu, name):
    from vited_amd import engine
    g, dq = load(name, gpu)
    comp = engine.PuzzleCompatibility(dq)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(comp.min_d.cpu().numpy(), g['min_d'])
    np.testing.assert_array_equal(comp.second_d.cpu().numpy(), g['second_d'])
    np.testing.assert_array_equal(comp.best_buddy.cpu().numpy(), g['bb'])
    np.testing.assert_array_equal(comp.start_order.cpu().numpy(), g['start_order'])
    order = g['start_order']
    np.testing.assert_array_equal(comp.start_count.cpu().numpy()[order], g['start_count'])
    np.testing.assert_array_equal(comp.start_total.cpu().numpy()[order].view(np.uint32), g['start_total'].view(np.uint32))
    if 'C' in g:
        np.testing.assert_array_equal(comp.compat.cpu().numpy().view(np.uint32), g['C'].view(np.uint32))
        np.testing.assert_array_equal(comp.mutual.cpu().numpy().view(np.uint32), g['M'].view(np.uint32))


@pytest.mark.parametrize('name', CASES)
def test_solve_puzzle_reproduces_the_reference(gpu, name):
    from vited_amd import engine
    g, dq = load(name, gpu)
    sol = engine.solve_puzzle(dq, tuple(int(v) for v in g['grid']))
    np.testing.assert_array_equal(sol.order, g['order'])
    np.testing.assert_array_equal(sol.board_locations, g['final_loc'])
    assert sol.recalcs == int(g['recalcs'])
    acc = engine.puzzle_accuracy(sol, g['true_loc'])
    assert [acc['Direct_Standard'], acc['Direct_Modified'], acc['neighbor']] == g['acc'].tolist()
    assert acc['perfect'] == bool(g['perfect'])


def test_recalc_follows_the_reference_rules(gpu):
    """One recalculation on the tie-heavy case against a numpy statement of recalculate_remaining_piece_compatibilities."""
    from vited_amd import engine
    g, dq = load('puzzle_ties_9x10', gpu)
    n = dq.shape[1]
    comp = engine.PuzzleCompatibility(dq)
    C0, M0 = comp.compat.cpu().numpy().copy(), comp.mutual.cpu().numpy().copy()
    mn0, sec0 = comp.min_d.cpu().numpy().copy(), comp.second_d.cpu().numpy().copy()
    placed = np.random.default_rng(5).random(n) < 0.4
    changed = comp.recalc(placed).cpu().numpy().astype(bool)
    D = g['Dq'].astype(np.int64)
    maxsize = 2 ** 63 - 1
    mn, sec, want_changed = mn0.copy(), sec0.copy(), np.zeros(n, bool)
    for i in np.flatnonzero(~placed):
        for s in range(4):
            row = np.sort(np.concatenate([D[s, i][~placed & (np.arange(n) != i)], [maxsize - 1, maxsize]]))
            mn[i, s], sec[i, s] = row[0], row[1]
        want_changed[i] = (mn[i] != mn0[i]).any() or (sec[i] != sec0[i]).any()
    np.testing.assert_array_equal(changed, want_changed)
    assert want_changed.any() and (~want_changed & ~placed).any()
    np.testing.assert_array_equal(comp.min_d.cpu().numpy(), mn)
    np.testing.assert_array_equal(comp.second_d.cpu().numpy(), sec)
    C = C0.copy()
    for i in np.flatnonzero(want_changed):
        for s in range(4):
            for j in np.flatnonzero(~placed):
                if j == i:
                    continue
                d = D[s, i, j]
                C[s, i, j] = 1.0 if d == 0 else (-maxsize if sec[i, s] == 0 else 1 - 1.0 * d / sec[i, s])
    np.testing.assert_array_equal(comp.compat.cpu().numpy().view(np.uint32), C.view(np.uint32))
    M = M0.copy()
    for s in range(4):
        pair = (want_changed[:, None] | want_changed[None, :]) & ~np.eye(n, dtype=bool)
        M[s][pair] = ((C[s] + C[(s + 2) % 4].T) / np.float32(2))[pair]
    np.testing.assert_array_equal(comp.mutual.cpu().numpy().view(np.uint32), M.view(np.uint32))


def brute_force_slot(M, placed, slot_piece, slot_side):
    best = None
    for p in np.flatnonzero(~placed):
        for k, (q, side) in enumerate(zip(slot_piece, slot_side)):
            v = M[(side + 2) % 4, p, q]
            if best is None or v > best[2]:
                best = (int(p), k, v)
    return best


@pytest.mark.parametrize('seed', range(6))
def test_best_slot_matches_a_brute_force_scan(gpu, seed):
    from vited_amd import engine
    rng = np.random.default_rng(seed)
    n = int(rng.integers(20, 300))
    comp = engine.PuzzleCompatibility(torch.from_numpy(rng.integers(0, 1000, size=(4, n, n)).astype(np.int32)).to(gpu))
    M = rng.choice(np.float32([-2.0, -0.5, 0.0, 0.25, 0.5, 0.75]), size=(4, n, n)).astype(np.float32)
    top = np.float32(0.9)
    placed = rng.random(n) < rng.uniform(0.1, 0.9)
    k = int(rng.integers(1, 60))
    slot_piece = rng.choice(np.flatnonzero(placed), size=k)
    slot_side = rng.integers(0, 4, size=k)
    # planted ties of the maximum: several (piece, slot) pairs, the first in scan order must win
    unplaced = np.flatnonzero(~placed)
    for p, kk in zip(rng.choice(unplaced, size=3), rng.integers(0, k, size=3)):
        M[(slot_side[kk] + 2) % 4, p, slot_piece[kk]] = top
    comp.state['mutual'].copy_(torch.from_numpy(M))
    got = comp.best_slot(placed, slot_piece, slot_side)
    want = brute_force_slot(M, placed, slot_piece, slot_side)
    assert got[:2] == want[:2] and got[2] == float(want[2]) == float(top)


def test_best_slot_negative_zero_and_no_ties(gpu):
    from vited_amd import engine
    n = 8
    comp = engine.PuzzleCompatibility(torch.zeros((4, n, n), dtype=torch.int32, device=gpu))
    M = np.full((4, n, n), -1.0, np.float32)
    placed = np.array([1, 0, 0, 0, 0, 0, 0, 1], bool)
    M[2, 3, 0] = -0.0                        # scanned after (piece 1, ...) entries holding +0.0: equal, so the earlier one wins
    M[2, 1, 7] = 0.0
    comp.state['mutual'].copy_(torch.from_numpy(M))
    assert comp.best_slot(placed, [0, 7], [0, 0])[:2] == (1, 1)


def quantise_numpy(logits):
    """evaluation.py:118-133 into inter_piece_distance.py:206-223: numpy float32 throughout, truncation by the uint32 store."""
    x = logits.astype(np.float32)
    sig = (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)
    return ((np.float32(1) - sig) * np.float32(1000.)).astype(np.float32).astype(np.uint32)


def near_integer(logits):
    x = logits.astype(np.float64)
    v = (1 - 1 / (1 + np.exp(-x))) * 1000
    return np.abs(v - np.round(v)) < 1e-4


def test_distances_from_logits_match_numpy(gpu):
    from vited_amd import ops
    rng = np.random.default_rng(0)
    n = 37
    ii, jj = np.nonzero(~np.eye(n, dtype=bool))
    logits = np.concatenate([rng.normal(0, 4, size=(ii.size - 40, 4)), rng.choice([-30., -8., 0., 8., 30.], size=(40, 4))]).astype(np.float32)
    dq = torch.full((4, n, n), 2 ** 31 - 1, dtype=torch.int32, device=gpu)
    bad = torch.zeros(1, dtype=torch.int32, device=gpu)
    ops.puzzle_distances_from_logits(torch.from_numpy(logits).to(gpu), torch.from_numpy(ii).to(gpu), torch.from_numpy(jj).to(gpu), dq, bad)
    got = dq.cpu().numpy()
    assert int(bad.item()) == 0
    for s in range(4):
        r = (s + 3) % 4
        want = quantise_numpy(logits[:, r])
        keep = ~near_integer(logits[:, r])
        assert keep.mean() > 0.95
        np.testing.assert_array_equal(got[s, ii, jj][keep], want[keep].astype(np.int64))
        assert (np.diagonal(got[s]) == 2 ** 31 - 1).all()


def _model(gpu):
    import vited_amd
    torch.manual_seed(7)
    s = vo.ViTEDShape(depth=1, c_depth=1)
    assert (s.img_size, s.patch_size, s.embed_dim, s.num_classes) == (64, 8, 384, 4)
    m = vited_amd.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, num_classes=s.num_classes, embed_dim=s.embed_dim,
                                          depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads).to(gpu)
    m.load_state_dict(vo.OracleViTED(s).state_dict())
    m.compute_dtype = torch.bfloat16
    return m.eval()


def test_puzzle_distances_match_the_model_on_stacked_pairs(gpu):
    from vited_amd import engine
    model = _model(gpu)
    n = 12
    pieces = torch.randint(0, 256, (n, 3, 64, 64), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    dq, logits = engine.puzzle_distances(model, pieces, pair_batch=29, block=5, return_logits=True)
    ii, jj = np.nonzero(~np.eye(n, dtype=bool))
    x = (pieces.float() / 255 - 0.5) / 0.5                  # ToTensor + Normalize(0.5, 0.5), what the uint8 path does on the device
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        ref = model(torch.stack([x[ii], x[jj]], dim=1).to(gpu)).float()
    got = logits[ii, jj]
    torch.testing.assert_close(got, ref, rtol=3e-2, atol=3e-2)
    lg = got.cpu().numpy()
    dqn = dq.cpu().numpy()
    for s in range(4):
        r = (s + 3) % 4
        keep = ~near_integer(lg[:, r])
        np.testing.assert_array_equal(dqn[s, ii, jj][keep], quantise_numpy(lg[:, r])[keep].astype(np.int64))
        assert (np.diagonal(dqn[s]) == 2 ** 31 - 1).all()
    # a float input and another batching: the same pairs to within the logits' bf16 tolerance
    dq2 = engine.puzzle_distances(model, x.to(gpu), pair_batch=1024, block=64).cpu().numpy()
    assert (np.abs(dq2[:, ii, jj].astype(np.int64) - dqn[:, ii, jj]) <= 10).all()


def test_two_runs_are_bit_identical(gpu):
    from vited_amd import engine
    model = _model(gpu)
    pieces = torch.randint(0, 256, (12, 3, 64, 64), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    runs = []
    for _ in range(2):
        dq = engine.puzzle_distances(model, pieces, pair_batch=40, block=4)
        comp = engine.PuzzleCompatibility(dq)
        runs.append([dq.cpu(), comp.compat.cpu(), comp.mutual.cpu()])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    g, dq = load('puzzle_noisy_14x18', gpu)
    a, b = engine.PuzzleCompatibility(dq), engine.PuzzleCompatibility(dq)
    assert torch.equal(a.mutual.view(torch.int32), b.mutual.view(torch.int32))


def test_bad_arguments_raise(gpu):
    from vited_amd import engine, ops
    with pytest.raises(ValueError):
        engine.solve_puzzle(torch.zeros((4, 6, 6), dtype=torch.int32, device=gpu), (2, 4))
    with pytest.raises(RuntimeError):
        ops.puzzle_compat_init(torch.zeros((4, 6, 6), dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.puzzle_compat_init(torch.zeros((4, 6, 5), dtype=torch.int32, device=gpu))
