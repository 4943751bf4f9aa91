"""The learned type-2 puzzle path on the MI355X: the turned patch extraction against ops.patchify of the physically turned batch, the
turned-pair scatter against the numpy rule (tests/puzzle_rot_cases.py), engine.puzzle_distances(puzzle_type=2) against the type-1 path
in its slice and against the type-1 path run on 4 n physically turned pieces, the turn-0 token cache against today's, and the one-call
driver.  Everything is compared exactly, except the one composition check whose tolerance is named there."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import puzzle_rot_cases as rc

pytestmark = pytest.mark.gpu

UNSET = rc.DQ_UNSET
ATOL = 3e-2         # tests/test_gpu_puzzle.py's tolerance for distances against model(stacked pairs), here without its relative part


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- the turned patch extraction ---------------------------------------------------------------------------------------------------------
def _images(kind, batch, size, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 'u8':
        return torch.randint(0, 256, (batch, 3, size, size), dtype=torch.uint8, generator=g)
    return torch.randn((batch, 3, size, size), generator=g)


@pytest.mark.parametrize('kind', ['u8', 'f32'])
@pytest.mark.parametrize('batch', [1, 3])
def test_turned_patchify_equals_patchify_of_the_turned_batch(gpu, vited, kind, batch):
    ops = vited.ops
    for size, patch in ((32, 8), (24, 4)):
        img = _images(kind, batch, size, 10 * batch + size).to(gpu)
        for dtype in (torch.float32, torch.bfloat16):
            want = [ops.patchify(torch.rot90(img, -k, (2, 3)).contiguous(), patch, dtype) for k in range(4)]
            assert not any(torch.equal(bits(want[0]), bits(want[k])) for k in range(1, 4))
            for k in range(4):
                got = ops.patchify_turned(img, patch, dtype, k)
                assert got.dtype == dtype and torch.equal(bits(got), bits(want[k])), (size, patch, dtype, k)
            turns = torch.tensor([(2 * b + 3) % 4 for b in range(batch)], device=gpu)              # 3, 1, 3 ...: mixed, per image
            rows = (size // patch) ** 2
            mixed = torch.cat([want[int(k)][b * rows:(b + 1) * rows] for b, k in enumerate(turns.tolist())])
            assert torch.equal(bits(ops.patchify_turned(img, patch, dtype, turns)), bits(mixed))
            assert torch.equal(bits(ops.patchify_turned(img, patch, dtype, turns.to(torch.int32))), bits(mixed))
    torch.cuda.synchronize()


@pytest.mark.parametrize('kind', ['u8', 'f32'])
def test_turned_patchify_takes_a_batch_stride_and_a_batch_index(gpu, vited, kind):
    ops = vited.ops
    pairs = torch.stack([_images(kind, 3, 32, 5), _images(kind, 3, 32, 6)], dim=1).to(gpu)          # [3, 2, C, S, S]
    for which in (0, 1):
        view = pairs[:, which]
        assert not view.is_contiguous() and view.stride(0) == 2 * 3 * 32 * 32
        for k in range(4):
            want = ops.patchify(torch.rot90(view, -k, (2, 3)).contiguous(), 8, torch.bfloat16)
            assert torch.equal(bits(ops.patchify_turned(view, 8, torch.bfloat16, k)), bits(want))
    view = pairs[:, 1]
    index = torch.tensor([2, 0, 2, 1, 1], device=gpu)
    turns = torch.tensor([0, 1, 2, 3, 1], device=gpu)
    want = torch.cat([ops.patchify(torch.rot90(view[i:i + 1], -k, (2, 3)).contiguous(), 8, torch.float32)
                      for i, k in zip(index.tolist(), turns.tolist())])
    assert torch.equal(bits(ops.patchify_turned(view, 8, torch.float32, turns, batch_index=index)), bits(want))
    with pytest.raises(ValueError, match='^patchify_turned: turn'):
        ops.patchify_turned(view, 8, torch.float32, torch.tensor([0, 1, 4], device=gpu))


# ---- the scatter -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [2, 3, 5, 17])
def test_scatter_equals_the_numpy_rule_on_all_16_pairings(gpu, vited, n):
    ops = vited.ops
    pi, pjt = rc.all_pairs(n)
    logits, fixed = rc.scatter_logits(pi.size, n)
    if n == 17:
        assert 4 * pi.size > fixed                 # +-40, +-0 and every near-integer logit are among them
    perm = np.random.default_rng(n).permutation(pi.size)           # not k-major: the kernel takes the pairs in any order
    pi, pjt = pi[perm], pjt[perm]
    want, refused = rc.scatter(n, logits, pi, pjt)
    assert refused == 0 and (want[:, ~np.eye(n, dtype=bool), :] != UNSET).all()
    dq2 = torch.full((4, n, n, 4), UNSET, dtype=torch.int32, device=gpu)
    bad = torch.zeros(1, dtype=torch.int32, device=gpu)
    dev = lambda a: torch.from_numpy(a).to(gpu)
    ops.puzzle_distances2_from_logits(dev(logits), dev(pi), dev(pjt), dq2, bad)
    assert int(bad.item()) == 0
    got = dq2.cpu().numpy().astype(np.int64)
    for si in range(4):
        for sj in range(4):
            np.testing.assert_array_equal(got[si, :, :, sj], want[si, :, :, sj], err_msg=f'pairing ({si}, {sj})')
    # the same array through the rule stated entry by entry
    full = np.zeros((n, n, 4, 4), np.float32)
    full[pi, pjt % n, pjt // n] = logits
    np.testing.assert_array_equal(got, rc.dq2_from_logits(full))
    # planted: j == i under a turn, jt >= 4 n, i outside - counted, nothing written
    sentinel = torch.full((4, n, n, 4), -7, dtype=torch.int32, device=gpu)
    planted_i = np.array([1, 0, n, 0], np.int64)
    planted_jt = np.array([2 * n + 1, 4 * n, 0, 1], np.int64)           # only the last pair is a pair
    ops.puzzle_distances2_from_logits(dev(logits[:4]), dev(planted_i), dev(planted_jt), sentinel, bad)
    assert int(bad.item()) == 1
    after = sentinel.cpu().numpy()
    assert (after != -7).sum() == 4
    for b in range(4):
        si, sj = rc.bin_sides(0, b)
        assert after[si, 0, 1, sj] == rc.quantise(logits[3, b])


# ---- the engine --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def models(gpu, vited):
    plain = rc.small_oracle(32)
    scaled = rc.small_oracle(32, weight_scale=6.0, head_scale=100.0)
    return {'bf16': rc.hip_model(vited, plain, gpu, torch.bfloat16), 'fp32': rc.hip_model(vited, plain, gpu, torch.float32),
            'scaled': rc.hip_model(vited, scaled, gpu, torch.float32)}


@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_type2_distances_hold_the_type1_distances_in_their_slice(gpu, vited, models, precision):
    engine, model, n = vited.engine, models[precision], 7
    pieces = torch.from_numpy(rc.pattern_pieces(n, 32))
    kw = dict(pair_batch=11, block=4, amp=precision == 'bf16')          # rows 0..3 and 4..6; 24 and 18 pairs per turn: 3 and 2 batches
    dq, logits = engine.puzzle_distances(model, pieces, return_logits=True, **kw)
    dq2, logits2 = engine.puzzle_distances(model, pieces, return_logits=True, puzzle_type=2, **kw)
    assert dq2.shape == (4, n, n, 4) and dq2.dtype == torch.int32 and logits2.shape == (n, n, 4, 4) and logits2.dtype == torch.float32
    for s in range(4):
        assert torch.equal(dq2[s, :, :, (s + 2) % 4], dq[s]), s
    assert torch.equal(bits(logits2[:, :, 0]), bits(logits))
    diag = torch.arange(n, device=gpu)
    assert (dq2[:, diag, diag, :] == UNSET).all() and (logits2[diag, diag] == 0).all()
    off = ~torch.eye(n, dtype=torch.bool, device=gpu)
    assert (dq2.permute(1, 2, 0, 3)[off] != UNSET).all() and (dq2.permute(1, 2, 0, 3)[off] <= 1000).all()
    assert torch.equal(engine.puzzle_distances(model, pieces, puzzle_type=2, **kw), dq2)            # without the logits; a second run
    assert len(np.unique(dq2.cpu().numpy())) > 10


def test_type2_logits_are_the_type1_logits_of_physically_turned_pieces(gpu, vited, models):
    """The independent composition: the 4 n pieces concat_k turn_k(pieces), turned on the host, through the type-1 path in fp32.
    logits2[i, j, k] must be L[i, k n + j] to within ATOL = 3e-2 absolute - the absolute part of the tolerance tests/test_gpu_puzzle.py
    compares distances against model(stacked pairs) with; its relative part is dropped, which asks more, and which lets '100 x the
    tolerance' mean one number.  A tolerance could hide a wrong turn under near-equal logits, so first, on L alone: for every (i, j) the
    logits of any two different turns differ by more than 100 x ATOL in at least one bin (the weights are scaled for that;
    tests/test_puzzle_rot.py checks the same on the CPU oracle).  Then Dq2 is the numpy quantisation of the returned logits, exactly."""
    engine, model, n = vited.engine, models['scaled'], 4
    upright = rc.pattern_pieces(n, 32)
    turned = torch.from_numpy(np.concatenate([np.ascontiguousarray(rc.turn(upright, k)) for k in range(4)]))
    assert torch.equal(turned[n:2 * n], torch.rot90(torch.from_numpy(upright), -1, (2, 3)))
    _, L = engine.puzzle_distances(model, turned, amp=False, return_logits=True, pair_batch=64, block=8)
    L = L.cpu().numpy()
    want = np.stack([L[:n, k * n:(k + 1) * n] for k in range(4)], axis=2)            # [i, j, k, bin]
    off = ~np.eye(n, dtype=bool)
    separation = rc.turn_separation(want, n)
    print(f'separation of two turns, worst (i, j): {separation:.3f}; largest |logit| {np.abs(want[off]).max():.2f}')
    assert separation > 100 * ATOL
    dq2, logits2 = engine.puzzle_distances(model, torch.from_numpy(upright), amp=False, return_logits=True, puzzle_type=2, pair_batch=5, block=3)
    got = logits2.cpu().numpy()
    print(f'largest |logits2 - L| off the diagonal: {np.abs(got - want)[off].max():.3e}')
    np.testing.assert_allclose(got[off], want[off], rtol=0, atol=ATOL)
    unstable = int((~rc.stable(got[off])).sum())
    print(f'logits whose quantisation hangs on the last bits of exp: {unstable} of {got[off].size}')
    np.testing.assert_array_equal(dq2.cpu().numpy().astype(np.int64), rc.dq2_from_logits(got))


class _Recorder:
    """ops._lib with every status-returning call noted (entry point and its scalar arguments) and passed on."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        return getattr(self.lib, name)

    def call(self, name, *args):
        self.calls.append((name, len(args)))
        return self.lib.call(name, *args)


def test_the_turn0_token_cache_is_todays(gpu, vited, models, monkeypatch):
    model = models['bf16']
    images = torch.from_numpy(rc.pattern_pieces(5, 32)).to(gpu)
    rec = _Recorder(vited.ops._lib)
    monkeypatch.setattr(vited.ops, '_lib', rec)
    runs = []
    for kw in ({}, {'turn': 0}, {'turn': 1}, {'turn': torch.zeros(5, dtype=torch.int64, device=gpu)}):
        del rec.calls[:]
        with torch.autocast('cuda', dtype=torch.bfloat16):
            tokens, q0 = model.cache_image2_tokens(images, **kw)
        runs.append((tokens, q0, list(rec.calls)))
    (t_a, q_a, calls_a), (t_b, q_b, calls_b), (t_1, q_1, calls_1), (t_z, q_z, calls_z) = runs
    assert q_a is not None and torch.equal(bits(t_a), bits(t_b)) and torch.equal(bits(q_a), bits(q_b))
    assert calls_a == calls_b and calls_a[0][0] == 'vited_patchify_u8' and not any('turned' in name for name, _ in calls_a)
    # a turn goes through the turned entry and nothing else changes; a tensor of zero turns gives the upright bits through it
    assert [c[0] for c in calls_1] == ['vited_patchify_turned_u8'] + [c[0] for c in calls_a[1:]] and calls_z == calls_1
    assert torch.equal(bits(t_z), bits(t_a)) and torch.equal(bits(q_z), bits(q_a)) and not torch.equal(bits(t_1), bits(t_a))
    with torch.autocast('cuda', dtype=torch.bfloat16):
        t_r, q_r = model.cache_image2_tokens(torch.rot90(images, -1, (2, 3)).contiguous())
    assert torch.equal(bits(t_1), bits(t_r)) and torch.equal(bits(q_1), bits(q_r))
    with pytest.raises(ValueError, match='^patchify_turned: turn'):
        model.cache_image2_tokens(images, turn=4)


def test_solve_model_puzzle_is_the_steps_run_by_hand(gpu, vited, models):
    engine, model, P = vited.engine, models['bf16'], 14
    y, x = np.meshgrid(np.arange(4 * P + 3), np.arange(5 * P + 2), indexing='ij')
    image = np.stack([(3 * y + x) % 256, (y * y // 7 + 2 * x) % 256, (5 * x + y // 2 + 31 * np.sin(0.2 * x * y / 9)) % 256], axis=2).astype(np.uint8)
    order = np.random.default_rng(3).permutation(20)
    for puzzle_type in (2, 1):
        sol, acc, board = engine.solve_model_puzzle(model, image, P, erosion=0.07, order=order, puzzle_type=puzzle_type, pair_batch=300)
        assert isinstance(sol, engine.PuzzleSolution) and sorted(sol.order.tolist()) == list(range(20))
        assert board.shape == (4 * P, 5 * P, 3) and board.dtype == torch.uint8 and board.is_cuda
        cut = engine.cut_puzzle(image, P, 0.07, order)
        pieces = engine.puzzle_model_pieces(cut.pieces, model.img_size)
        by_hand = engine.solve_puzzle(engine.puzzle_distances(model, pieces, puzzle_type=puzzle_type, pair_batch=300), cut.grid_size)
        for a, b in zip(sol, by_hand):
            assert (a is None and b is None) or np.array_equal(a, b)
        assert acc == engine.puzzle_accuracy(by_hand, cut.true_locations)
        assert torch.equal(board, engine.reconstruct_puzzle(cut.pieces, by_hand, cut.true_locations, P))
        if puzzle_type == 2:
            assert sol.rotations is not None and sol.rotations.shape == (20,) and set(np.unique(sol.rotations)) <= {0, 1, 2, 3}
            assert set(acc) == {'Direct_Standard', 'Direct_Modified', 'neighbor', 'perfect', 'wrong_rotation'}
        else:
            assert sol.rotations is None and set(acc) == {'Direct_Standard', 'Direct_Modified', 'neighbor', 'perfect'}
    with pytest.raises(ValueError, match='puzzle_type'):
        engine.solve_model_puzzle(model, image, P, puzzle_type=3)
