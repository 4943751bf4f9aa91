"""The classical puzzle baseline's pixel kernels on the MI355X (csrc/puzzle_pixels.hip): cut, border distances and board against
the fixtures the reference's own code wrote (tests/golden/pixel_puzzle_*.npz), the resize against Pillow, the distances at the shapes
where the tiling could go wrong against the numpy rule, and engine.solve_pixel_puzzle against the reference's whole run."""
import numpy as np
import pytest
import torch

import puzzle_pixels_cases as pc

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


def _dev(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)                # a copy: the fixtures are read-only


def _locations(g):
    loc = g['final_loc']
    return loc - loc.min(axis=0)


@pytest.mark.parametrize('name', pc.FIXTURES)
def test_cut_distances_and_board_equal_the_reference(gpu, vited, name):
    """Every output buffer starts full of a sentinel no result consists of, so an element the kernels leave out shows."""
    ops, g = vited.ops, pc.fixture(name)
    P, We, n = int(g['piece_width']), g['pieces'].shape[1], g['pieces'].shape[0]
    pieces = torch.full((n, We, We, 3), SENTINEL, dtype=torch.uint8, device=gpu)
    assert ops.puzzle_cut(_dev(g['image'], gpu), P, We, order=g['perm'], out=pieces) is pieces
    np.testing.assert_array_equal(pieces.cpu().numpy(), g['pieces'])
    plain = ops.puzzle_cut(_dev(g['image'], gpu), P, We).cpu().numpy()              # no order: the row-major cells
    np.testing.assert_array_equal(plain[g['perm']], g['pieces'])
    dq = torch.full((4, n, n), -7, dtype=torch.int32, device=gpu)
    assert ops.puzzle_pixel_distances(pieces, out=dq) is dq
    np.testing.assert_array_equal(dq.cpu().numpy(), g['Dq'])
    board = torch.full(g['board'].shape, SENTINEL, dtype=torch.uint8, device=gpu)
    assert ops.puzzle_assemble(pieces, _locations(g), g['true_loc'], P, marker=pc.marker_for(P, We), out=board) is board
    np.testing.assert_array_equal(board.cpu().numpy(), g['board'])
    unframed = ops.puzzle_assemble(pieces, _locations(g), g['true_loc'], P).cpu().numpy()
    np.testing.assert_array_equal(unframed, pc.board(g['pieces'], _locations(g), g['true_loc'], P))


@pytest.mark.parametrize('name,size', [('pixel_puzzle_odd_5x6', 16), ('pixel_puzzle_noisy_8x9', 64), ('pixel_puzzle_half_6x5', 32),
                                       ('pixel_puzzle_poster_7x8', 10), ('pixel_puzzle_poster_7x8', 23)])
def test_resize_equals_pillow(gpu, vited, name, size):
    pieces = pc.fixture(name)['pieces']
    n = pieces.shape[0]
    out = torch.full((n, 3, size, size), SENTINEL, dtype=torch.uint8, device=gpu)
    vited.ops.puzzle_resize_pieces(_dev(pieces, gpu), size, out=out)
    want = pc.pillow_resize(pieces, size)
    if size == pieces.shape[1]:
        np.testing.assert_array_equal(want, pieces.transpose(0, 3, 1, 2))          # We = S: the pieces themselves
    np.testing.assert_array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize('name', sorted(pc.SHAPES))
def test_distances_at_the_tiling_edges(gpu, vited, name):
    pieces = pc.shape_pieces(name)
    n = pieces.shape[0]
    want = pc.distances(pieces)
    dev = _dev(pieces, gpu)
    first = torch.full((4, n, n), -7, dtype=torch.int32, device=gpu)
    vited.ops.puzzle_pixel_distances(dev, out=first)
    second = vited.ops.puzzle_pixel_distances(dev)
    got = first.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert (got[:, np.arange(n), np.arange(n)] == 2 ** 31 - 1).all()
    assert torch.equal(first, second)
    if name == 'extremes':
        We = pieces.shape[1]
        assert got[0, 0, 1] == 255 * 3 * We and got[0, 1, 0] == 255 * 3 * We          # all-0 against all-255, both ways
        assert got[0, 2, 0] == 510 * 3 * We and got[0, 3, 1] == 510 * 3 * We          # predictions 510 against 0, -255 against 255
        assert got[3, 4, 0] == 510 * 3 * We and got[3, 5, 1] == 510 * 3 * We


@pytest.mark.parametrize('name', pc.FIXTURES)
def test_solve_pixel_puzzle_reproduces_the_reference_run(gpu, vited, name):
    engine, g = vited.engine, pc.fixture(name)
    P, We = int(g['piece_width']), g['pieces'].shape[1]
    solution, acc, board = engine.solve_pixel_puzzle(np.array(g['image']), P, float(g['erosion']), order=g['perm'], marker=pc.marker_for(P, We))
    np.testing.assert_array_equal(solution.board_locations, g['final_loc'])
    np.testing.assert_array_equal(solution.locations, _locations(g))
    np.testing.assert_array_equal(solution.order, g['order'])
    assert solution.recalcs == int(g['recalcs'])
    assert [acc['Direct_Standard'], acc['Direct_Modified'], acc['neighbor']] == g['acc'].tolist() and acc['perfect'] == bool(g['perfect'])
    np.testing.assert_array_equal(board.cpu().numpy(), g['board'])
    cut = engine.cut_puzzle(_dev(g['image'], gpu), P, float(g['erosion']), order=g['perm'])
    assert cut.grid_size == tuple(g['grid']) and cut.piece_width == P and cut.true_locations.dtype == np.int64
    np.testing.assert_array_equal(cut.true_locations, g['true_loc'])
    np.testing.assert_array_equal(cut.pieces.cpu().numpy(), g['pieces'])


def test_marker_without_padding_is_refused(gpu, vited):
    g = pc.fixture('pixel_puzzle_odd_5x6')                 # P = 16, We = 15: pad 0
    with pytest.raises(ValueError, match='^puzzle_assemble: marker'):
        vited.engine.solve_pixel_puzzle(np.array(g['image']), 16, 0.07, order=g['perm'], marker=pc.REFERENCE_MARKER)


def test_cut_pieces_feed_the_learned_path(gpu, vited):
    """cut_puzzle -> puzzle_model_pieces -> puzzle_distances on a 1 + 1-block model equals puzzle_distances on the same pieces resized on
    the host with Pillow: the resize is Pillow's bit for bit, and the model path is deterministic."""
    from oracle import vited_oracle as vo
    engine, g = vited.engine, pc.fixture('pixel_puzzle_half_6x5')
    torch.manual_seed(7)
    s = vo.ViTEDShape(depth=1, c_depth=1)
    model = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, num_classes=s.num_classes, embed_dim=s.embed_dim,
                                          depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads).to(gpu)
    model.load_state_dict(vo.OracleViTED(s).state_dict())
    model.compute_dtype = torch.bfloat16
    model.eval()
    cut = engine.cut_puzzle(np.array(g['image']), 13, 0.25, order=g['perm'])
    resized = engine.puzzle_model_pieces(cut.pieces, s.img_size)
    host = pc.pillow_resize(g['pieces'], s.img_size)
    np.testing.assert_array_equal(resized.cpu().numpy(), host)
    dq = engine.puzzle_distances(model, resized)
    want = engine.puzzle_distances(model, torch.from_numpy(host))
    assert torch.equal(dq, want)
    assert len(np.unique(dq.cpu().numpy())) > 10
