"""CPU: type-2 puzzles (pieces of unknown rotation).  The fixtures the reference's own solver wrote hold arrays only and stay under the
size cap; the numpy restatements (tests/puzzle_type2_cases.py) reproduce the distances of all 16 side pairings, the compatibility state
and the boards in them; engine.puzzle_accuracy reproduces the recorded accuracies from the recorded placements; the type-2 text of
csrc/puzzle_pixels.h reproduces distances and boards through a stand-alone host program under the sanitizers; the new entry points are
declared, bound, exported and refuse bad arguments without a launch, and the wrappers refuse before the library is reached."""
import ctypes
import fnmatch
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import puzzle_pixels_cases as pc
import puzzle_type2_cases as t2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('vited_puzzle_pixel_distances2_workspace_bytes', 'vited_puzzle_pixel_distances2', 'vited_puzzle_compat2_init',
           'vited_puzzle_compat2_recalc', 'vited_puzzle_best_slot2', 'vited_puzzle_assemble2')
ARRAYS = {'grid', 'Dq2', 'true_loc', 'min_d', 'second_d', 'bb', 'start_order', 'start_count', 'start_total', 'final_loc', 'rotations',
          'order', 'recalcs', 'acc', 'perfect', 'wrong_rotation'}


# ---- the fixtures as stored --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', t2.SYNTHETIC + t2.PIXEL)
def test_fixtures_hold_arrays_only_under_the_cap(name):
    path = os.path.join(pc.GOLDEN, name + '.npz')
    assert os.path.getsize(path) < os.path.getsize(os.path.join(pc.GOLDEN, 'puzzle_noisy_14x18.npz'))
    assert not fnmatch.fnmatch(name + '.npz', 'puzzle_*.npz') and not fnmatch.fnmatch(name + '.npz', 'pixel_puzzle_*.npz')
    with np.load(path, allow_pickle=False) as z:                   # an object array would need pickle: refused
        g = {k: z[k] for k in z.files}
    extra = {'image', 'piece_width', 'erosion', 'perm', 'pieces', 'board'} if name in t2.PIXEL else ({'C', 'M'} if name == 'rot_puzzle_4x4' else set())
    assert set(g) == ARRAYS | extra
    assert all(a.dtype.kind in 'iuf' for a in g.values())
    rows, cols = g['grid']
    n = rows * cols
    assert g['Dq2'].shape == (4, n, n, 4) and g['Dq2'].dtype == (np.int32 if name in t2.PIXEL else np.uint16)
    assert g['min_d'].shape == g['second_d'].shape == (n, 4) and g['bb'].shape == (n, 4, 2)
    assert sorted(g['order'].tolist()) == list(range(n)) and set(np.unique(g['rotations'])) <= {0, 1, 2, 3}
    assert g['rotations'][g['order'][0]] == 0                       # the seed lies unrotated


def test_fixtures_cover_what_they_are_there_for():
    g = {name: t2.fixture(name) for name in t2.SYNTHETIC + t2.PIXEL}
    for name in ('rot_puzzle_4x4', 'rot_puzzle_clean_8x9'):
        assert g[name]['perfect'] == 1 and g[name]['recalcs'] == 0 and not g[name]['rotations'].any()
    for name in ('rot_puzzle_ties_7x8', 'rot_puzzle_noisy_9x11'):
        assert g[name]['recalcs'] > 50 and set(np.unique(g[name]['rotations'])) == {0, 1, 2, 3}
    ties = g['rot_puzzle_ties_7x8']
    assert (ties['second_d'] == 0).any() and (ties['Dq2'] == 0).sum() > 100
    widths = {name: g[name]['pieces'].shape[1] for name in t2.PIXEL}
    assert widths == {'rot_pixel_puzzle_even_4x5': 12, 'rot_pixel_puzzle_odd_5x4': 11, 'rot_pixel_puzzle_poster_5x6': 10}
    assert all(pc.pad_of(int(g[name]['piece_width']), widths[name]) == 1 for name in t2.PIXEL)      # erosion padding: room for the frame
    poster = g['rot_pixel_puzzle_poster_5x6']['Dq2']
    off = poster[poster != t2.DQ_UNSET]
    assert (off == 0).sum() > 0 and np.unique(off).size < off.size // 10
    # pieces at the right cell but turned: "wrong rotation" in the accuracies, unframed on the reference's board
    assert sum(int(g[name]['wrong_rotation']) for name in t2.PIXEL) >= 3
    assert any(len(np.unique(g[name]['rotations'])) == 4 for name in t2.PIXEL)


@pytest.mark.parametrize('name', t2.PIXEL)
def test_numpy_distances_and_board_reproduce_the_reference(name):
    g = t2.fixture(name)
    P, We = int(g['piece_width']), g['pieces'].shape[1]
    np.testing.assert_array_equal(pc.cut(g['image'], P, We, g['perm']), g['pieces'])
    dq2 = t2.distances2(g['pieces'])
    np.testing.assert_array_equal(dq2, g['Dq2'])                      # all 16 pairings
    type1 = pc.distances(g['pieces'])
    for s in range(4):
        np.testing.assert_array_equal(dq2[s, :, :, (s + 2) % 4], type1[s])
    np.testing.assert_array_equal(t2.board2(g['pieces'], t2.locations(g), g['rotations'], g['true_loc'], P, pc.REFERENCE_MARKER), g['board'])


def test_numpy_compatibility_rules_reproduce_the_reference_on_the_4x4():
    g = t2.fixture('rot_puzzle_4x4')
    mn, sec, cnt, cand, C, M = t2.init_state(t2.dq2_of(g))
    np.testing.assert_array_equal(mn, g['min_d'])
    np.testing.assert_array_equal(sec, g['second_d'])
    np.testing.assert_array_equal(C.view(np.uint32), g['C'].view(np.uint32))
    np.testing.assert_array_equal(M.view(np.uint32), g['M'].view(np.uint32))
    n = mn.shape[0]
    bb = np.full((n, 4, 2), -1, np.int64)
    for i in range(n):
        for s in range(4):
            j, sj = cand[i, s]
            if j >= 0 and tuple(cand[j, sj]) == (i, s):
                bb[i, s] = (j, sj)
    np.testing.assert_array_equal(bb, g['bb'])


# ---- the accuracies ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', t2.SYNTHETIC + t2.PIXEL)
def test_puzzle_accuracy_reproduces_the_recorded_accuracies(vited, name):
    g = t2.fixture(name)
    loc = t2.locations(g)
    grid = np.full(tuple(loc.max(axis=0) + 1), -1, np.int64)
    grid[loc[:, 0], loc[:, 1]] = np.arange(len(loc))
    sol = vited.engine.PuzzleSolution(loc, g['final_loc'], g['order'], int(g['recalcs']), grid, g['rotations'])
    acc = vited.engine.puzzle_accuracy(sol, g['true_loc'])
    assert set(acc) == {'Direct_Standard', 'Direct_Modified', 'neighbor', 'perfect', 'wrong_rotation'}
    assert [acc['Direct_Standard'], acc['Direct_Modified'], acc['neighbor']] == g['acc'].tolist()
    assert acc['perfect'] == bool(g['perfect']) and acc['wrong_rotation'] == int(g['wrong_rotation'])


def test_a_type1_solution_keeps_its_five_fields_and_four_keys(vited):
    g = pc.fixture('pixel_puzzle_noisy_8x9')
    loc = g['final_loc'] - g['final_loc'].min(axis=0)
    grid = np.full(tuple(loc.max(axis=0) + 1), -1, np.int64)
    grid[loc[:, 0], loc[:, 1]] = np.arange(len(loc))
    sol = vited.engine.PuzzleSolution(loc, g['final_loc'], g['order'], int(g['recalcs']), grid)
    assert sol.rotations is None and len(sol) == 6
    acc = vited.engine.puzzle_accuracy(sol, g['true_loc'])
    assert set(acc) == {'Direct_Standard', 'Direct_Modified', 'neighbor', 'perfect'}
    assert [acc['Direct_Standard'], acc['Direct_Modified'], acc['neighbor']] == g['acc'].tolist()
    # all-zero rotations are a type-2 solution that scores what the type-1 one scores
    turned = vited.engine.puzzle_accuracy(sol._replace(rotations=np.zeros(len(loc), np.int64)), g['true_loc'])
    assert turned.pop('wrong_rotation') == 0 and turned == acc


# ---- the header's text on the host, under the sanitizers -----------------------------------------------------------------------------
def _cells(loc, true, cols, framed):
    cells = np.full(len(loc), -1)
    cells[loc[:, 0] * cols + loc[:, 1]] = 2 * np.arange(len(loc)) + ((loc != true).any(axis=1) if framed else 0)
    return cells


def test_host_program_gives_the_golden_values_under_the_sanitizers(tmp_path):
    """tools/puzzle_type2_host_check.cpp: the strips of three kinds, pairing_reversed, strip_distance and board_byte_rotated of
    csrc/puzzle_pixels.h over every pixel fixture and two synthetic piece sets (We = 2 and an odd width with padding) - a stand-alone
    program with its own main, built with -fsanitize=address,undefined."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    cxx = next((c for c in (shutil.which('clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'))
                if c and os.path.exists(c)), None)
    assert cxx is not None, 'no clang++ beside hipcc: the HIP toolchain that builds the library ships one'
    exe = str(tmp_path / 'puzzle_type2_host_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off', '-I',
                    os.path.join(ROOT, 'vit-ed_amd', 'csrc'), os.path.join(ROOT, 'tools', 'puzzle_type2_host_check.cpp'), '-o', exe], check=True)
    blobs, want = [], []

    def add(pieces, P, rows, cols, marker, cells, rotations, dq2, board):
        colour = -1 if marker is None else marker[0] | marker[1] << 8 | marker[2] << 16
        head = np.array([pieces.shape[0], pieces.shape[1], P, rows, cols, colour], '<i4')
        blobs.append(head.tobytes() + np.ascontiguousarray(pieces).tobytes() + np.asarray(cells, '<i4').tobytes()
                     + np.asarray(rotations, '<i4').tobytes())
        want.append((np.ascontiguousarray(dq2, '<i4'), np.ascontiguousarray(board)))

    for name in t2.PIXEL:
        g = t2.fixture(name)
        (rows, cols), loc = g['grid'], t2.locations(g)
        turns = np.zeros(rows * cols, np.int64)
        turns[loc[:, 0] * cols + loc[:, 1]] = g['rotations']
        add(g['pieces'], int(g['piece_width']), rows, cols, pc.REFERENCE_MARKER, _cells(loc, g['true_loc'], cols, True), turns, g['Dq2'], g['board'])
    for name, P, (rows, cols) in (('two_pieces_two_lines', 2, (1, 2)), ('seventeen_odd', 18, (17, 1))):
        pieces = t2.shape_pieces(name)
        n = pieces.shape[0]
        ident = np.stack([np.arange(n) // cols, np.arange(n) % cols], axis=1)
        turns = np.arange(n) % 4
        add(pieces, P, rows, cols, None, _cells(ident, ident, cols, False), turns, t2.distances2(pieces), t2.board2(pieces, ident, turns, ident, P))
    (tmp_path / 'cases.bin').write_bytes(np.array([len(blobs)], '<i4').tobytes() + b''.join(blobs))
    run = subprocess.run([exe, str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.strip() == f'puzzle_type2_host_check ok: {len(want)} cases'
    got = np.fromfile(tmp_path / 'out.bin', np.uint8)
    at = 0
    for q, arrays in enumerate(want):
        for what, a in zip(('dq2', 'board'), arrays):
            np.testing.assert_array_equal(got[at:at + a.nbytes].view(a.dtype).reshape(a.shape), a, err_msg=f'case {q} {what}')
            at += a.nbytes
    assert at == got.size


# ---- the C entry points without a GPU ------------------------------------------------------------------------------------------------
def _ensure_built(vited):
    if not os.path.exists(vited._lib.LIB_PATH):
        subprocess.run(['make', '-C', os.path.join(ROOT, 'vit-ed_amd', 'csrc'), '-j', '8'], check=True)


def test_entry_points_are_declared_bound_and_exported(vited):
    _ensure_built(vited)
    L = vited._lib
    text = re.sub(r'/\*.*?\*/', ' ', open(L.HEADER_PATH).read(), flags=re.S)
    p, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert L.SIGNATURES['vited_puzzle_pixel_distances2_workspace_bytes'] == (i64, [i64, i])
    assert L.SIGNATURES['vited_puzzle_pixel_distances2'] == (i, [p, i64, i, p, p, i64, p])
    assert L.SIGNATURES['vited_puzzle_compat2_init'] == (i, [p, i64] + [p] * 11)
    assert L.SIGNATURES['vited_puzzle_compat2_recalc'] == (i, [p, i64] + [p] * 7)
    assert L.SIGNATURES['vited_puzzle_best_slot2'] == (i, [p, i64, p, p, p, i64, p, p])
    assert L.SIGNATURES['vited_puzzle_assemble2'] == (i, [p, i64, i, i, p, p, i64, i64, i, p, p])
    out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if ' T ' in l}
    for name in ENTRIES:
        assert re.search(rf'\b{name}\s*\(', text) and name in exported, name


def test_entry_points_refuse_bad_arguments_without_a_launch(vited):
    _ensure_built(vited)
    lib = vited._lib.load()
    buf = (ctypes.c_uint8 * 4096)()
    a = ctypes.addressof(buf)
    a += -a % 16
    BAD, UNSUPPORTED, WORKSPACE = 1, 2, 4
    size = lib.vited_puzzle_pixel_distances2_workspace_bytes
    assert size(6, 10) == 3 * 4 * 6 * 32 * 2 and size(6, 15) == 3 * 4 * 6 * 48 * 2 and size(2, 2) == 3 * 4 * 2 * 8 * 2
    assert size(1, 10) == -1 and size(6, 1) == -1 and size(46341, 10) == -1 and size(6, 935723) == -1
    dist = lib.vited_puzzle_pixel_distances2
    assert dist(None, 6, 10, a, a, 4096, None) == BAD and dist(a, 6, 10, None, a, 4096, None) == BAD
    assert dist(a, 6, 10, a, None, 4096, None) == BAD and dist(a, 6, 10, a, a + 4, 4096, None) == BAD
    assert dist(a, 6, 10, a + 8, a, 4096, None) == BAD                      # dq2 leaves in 16-byte stores
    assert dist(a, 1, 10, a, a, 4096, None) == BAD and dist(a, 6, 1, a, a, 4096, None) == BAD
    assert dist(a, 46341, 10, a, a, 1 << 40, None) == UNSUPPORTED and dist(a, 6, 935723, a, a, 1 << 40, None) == UNSUPPORTED
    assert dist(a, 6, 10, a, a, size(6, 10) - 1, None) == WORKSPACE
    init = lib.vited_puzzle_compat2_init
    full = [a] * 10
    assert init(a, 1, *full, None) == BAD and init(a, 46341, *full, None) == BAD and init(a + 4, 6, *full, None) == BAD
    assert init(None, 6, *full, None) == BAD
    for k in range(10):
        assert init(a, 6, *(full[:k] + [None] + full[k + 1:]), None) == BAD, k
    recalc = lib.vited_puzzle_compat2_recalc
    assert recalc(a, 1, *[a] * 6, None) == BAD and recalc(a + 4, 6, *[a] * 6, None) == BAD and recalc(None, 6, *[a] * 6, None) == BAD
    for k in range(6):
        assert recalc(a, 6, *([a] * k + [None] + [a] * (5 - k)), None) == BAD, k
    slot = lib.vited_puzzle_best_slot2
    assert slot(None, 6, a, a, a, 3, a, None) == BAD and slot(a, 6, None, a, a, 3, a, None) == BAD and slot(a, 6, a, None, a, 3, a, None) == BAD
    assert slot(a, 6, a, a, None, 3, a, None) == BAD and slot(a, 6, a, a, a, 3, None, None) == BAD
    assert slot(a, 6, a, a, a, 0, a, None) == BAD and slot(a, 1, a, a, a, 3, a, None) == BAD
    assert slot(a, 1024, a, a, a, 1 << 20, a, None) == UNSUPPORTED           # 4 n slots = 2^32
    board = lib.vited_puzzle_assemble2
    assert board(None, 6, 10, 13, a, a, 2, 3, -1, a, None) == BAD and board(a, 6, 10, 13, None, a, 2, 3, -1, a, None) == BAD
    assert board(a, 6, 10, 13, a, None, 2, 3, -1, a, None) == BAD and board(a, 6, 10, 13, a, a, 2, 3, -1, None, None) == BAD
    assert board(a, 6, 1, 13, a, a, 2, 3, -1, a, None) == BAD and board(a, 6, 10, 9, a, a, 2, 3, -1, a, None) == BAD
    assert board(a, 6, 10, 13, a, a, 2, 2, -1, a, None) == BAD and board(a, 6, 10, 11, a, a, 2, 3, 0xff0000, a, None) == BAD
    assert board(a, 46341, 10, 13, a, a, 1, 46341, -1, a, None) == UNSUPPORTED


# ---- the wrappers, the library replaced by a recorder ---------------------------------------------------------------------------------
class _Library:
    def __getattr__(self, name):
        return lambda *args: 4096


@pytest.fixture
def ops(vited, monkeypatch):
    calls = []
    monkeypatch.setattr(vited.ops, '_need_gpu', lambda *tensors, **kw: None)
    monkeypatch.setattr(vited.ops, '_stream', lambda: 0)
    monkeypatch.setattr(vited.ops, '_scratch', lambda nbytes, device, align=1: (0, 1 << 40))
    monkeypatch.setattr(vited.ops, '_lib', SimpleNamespace(call=lambda name, *args: calls.append((name, args)), load=_Library))
    vited.ops.calls = calls
    yield vited.ops
    del vited.ops.calls


def u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def i32(*shape):
    return torch.zeros(shape, dtype=torch.int32)


def f32(*shape):
    return torch.zeros(shape, dtype=torch.float32)


N = 6


def _state():
    return dict(min_d=torch.zeros(N, 4, dtype=torch.int64), second_d=torch.zeros(N, 4, dtype=torch.int64), compat=f32(4, N, N, 4),
                mutual=f32(4, N, N, 4))


def test_wrappers_are_ops_functions_and_refuse_cpu_tensors(vited):
    names = ('puzzle_pixel_distances2', 'puzzle_compat2_init', 'puzzle_compat2_recalc', 'puzzle_best_slot2', 'puzzle_unpack_slot2',
             'puzzle_assemble2')
    for name in names:
        assert getattr(vited.ops, name) is getattr(vited.ops_puzzle2, name)
    ident = np.stack([np.arange(6) // 3, np.arange(6) % 3], axis=1)
    calls = [lambda: vited.ops.puzzle_pixel_distances2(u8(N, 10, 10, 3)), lambda: vited.ops.puzzle_pixel_distances(u8(N, 10, 10, 3), puzzle_type=2),
             lambda: vited.ops.puzzle_compat2_init(i32(4, N, N, 4)), lambda: vited.ops.puzzle_compat2_recalc(i32(4, N, N, 4), i32(N), _state(), i32(N)),
             lambda: vited.ops.puzzle_best_slot2(f32(4, N, N, 4), i32(N), i32(3), i32(3)),
             lambda: vited.ops.puzzle_assemble2(u8(N, 10, 10, 3), ident, np.zeros(N, np.int64), ident, 13),
             lambda: vited.engine.PuzzleCompatibility(i32(4, N, N, 4)), lambda: vited.engine.solve_puzzle(i32(4, N, N, 4), (2, 3))]
    if not torch.cuda.is_available():                   # where there is a GPU the engine uploads a host image
        calls.append(lambda: vited.engine.solve_pixel_puzzle(np.zeros((26, 39, 3), np.uint8), 13, 0.25, puzzle_type=2))
    for call in calls:
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    in_source = re.findall(r"_lib\.call\('(vited_\w+)'", open(os.path.join(ROOT, 'vit-ed_amd', 'ops_puzzle2.py')).read())
    assert sorted(in_source) == sorted(e for e in ENTRIES if not e.endswith('_bytes'))


def test_valid_calls_reach_their_entry_points(ops):
    ident = np.stack([np.arange(6) // 3, np.arange(6) % 3], axis=1)
    dq2 = ops.puzzle_pixel_distances2(u8(N, 10, 10, 3))
    assert dq2.shape == (4, N, N, 4) and dq2.dtype == torch.int32 and ops.calls.pop()[0] == 'vited_puzzle_pixel_distances2'
    assert ops.puzzle_pixel_distances(u8(N, 10, 10, 3), puzzle_type=2).shape == (4, N, N, 4) and ops.calls.pop()[0] == 'vited_puzzle_pixel_distances2'
    assert ops.puzzle_pixel_distances(u8(N, 10, 10, 3), puzzle_type=1).shape == (4, N, N) and ops.calls.pop()[0] == 'vited_puzzle_pixel_distances'
    st = ops.puzzle_compat2_init(i32(4, N, N, 4))
    assert ops.calls.pop()[0] == 'vited_puzzle_compat2_init'
    assert {k: (tuple(v.shape), v.dtype) for k, v in st.items()} == {
        'min_d': ((N, 4), torch.int64), 'second_d': ((N, 4), torch.int64), 'min_count': ((N, 4), torch.int32),
        'candidate': ((N, 4, 2), torch.int32), 'best_buddy': ((N, 4, 2), torch.int32), 'compat': ((4, N, N, 4), torch.float32),
        'mutual': ((4, N, N, 4), torch.float32), 'start_count': ((N,), torch.int32), 'start_total': ((N,), torch.float32),
        'start_order': ((N,), torch.int32)}
    ops.puzzle_compat2_recalc(i32(4, N, N, 4), i32(N), st, i32(N))
    assert ops.calls.pop()[0] == 'vited_puzzle_compat2_recalc'
    assert ops.puzzle_best_slot2(f32(4, N, N, 4), i32(N), i32(3), i32(3)).shape == (1,)
    name, args = ops.calls.pop()
    assert name == 'vited_puzzle_best_slot2' and args[1] == N and args[5] == 3
    moved = ident[[1, 0, 2, 3, 4, 5]]
    assert ops.puzzle_assemble2(u8(N, 10, 10, 3), moved, [0, 1, 2, 3, 0, 1], ident, 13, marker=(0, 0, 255)).shape == (26, 39, 3)
    name, args = ops.calls.pop()
    assert name == 'vited_puzzle_assemble2' and args[1:4] == (N, 10, 13) and args[6:9] == (2, 3, 255 << 16)
    assert not ops.calls
    # the packed word: piece 5, slot 2 of 3, side 1 -> linear index (5 * 3 + 2) * 4 + 1
    word = (0x80000000 << 32) | (0xffffffff - ((5 * 3 + 2) * 4 + 1))
    assert ops.puzzle_unpack_slot2(word, 3) == (5, 2, 1) and ops.puzzle_unpack_slot2(0, 3) is None


def test_wrappers_refuse_before_the_launch(ops):
    ident = np.stack([np.arange(6) // 3, np.arange(6) % 3], axis=1)
    pieces, dq2, rot = u8(N, 10, 10, 3), i32(4, N, N, 4), np.zeros(N, np.int64)
    wide = torch.zeros(4, N, N, 8, dtype=torch.int32)[..., ::2]
    refused = [
        ('puzzle_pixel_distances2', 'pieces', lambda: ops.puzzle_pixel_distances2(u8(N, 10, 10))),
        ('puzzle_pixel_distances2', 'pieces', lambda: ops.puzzle_pixel_distances2(u8(1, 10, 10, 3))),
        ('puzzle_pixel_distances2', 'pieces', lambda: ops.puzzle_pixel_distances2(pieces.float())),
        ('puzzle_pixel_distances2', 'pieces', lambda: ops.puzzle_pixel_distances2(u8(N, 10, 10, 6)[..., ::2])),
        ('puzzle_pixel_distances2', 'out', lambda: ops.puzzle_pixel_distances2(pieces, out=i32(4, N, N))),
        ('puzzle_pixel_distances2', 'out', lambda: ops.puzzle_pixel_distances(pieces, out=dq2.long(), puzzle_type=2)),
        ('puzzle_pixel_distances', 'puzzle_type', lambda: ops.puzzle_pixel_distances(pieces, puzzle_type=3)),
        ('puzzle_compat2_init', 'dq2', lambda: ops.puzzle_compat2_init(i32(4, N, N))),
        ('puzzle_compat2_init', 'dq2', lambda: ops.puzzle_compat2_init(i32(4, N, N + 1, 4))),
        ('puzzle_compat2_init', 'dq2', lambda: ops.puzzle_compat2_init(dq2.long())),
        ('puzzle_compat2_init', 'dq2', lambda: ops.puzzle_compat2_init(wide)),
        ('puzzle_compat2_recalc', 'dq2', lambda: ops.puzzle_compat2_recalc(wide, i32(N), _state(), i32(N))),
        ('puzzle_compat2_recalc', 'placed', lambda: ops.puzzle_compat2_recalc(dq2, i32(N + 1), _state(), i32(N))),
        ('puzzle_compat2_recalc', 'placed', lambda: ops.puzzle_compat2_recalc(dq2, torch.zeros(N, dtype=torch.bool), _state(), i32(N))),
        ('puzzle_compat2_recalc', 'changed', lambda: ops.puzzle_compat2_recalc(dq2, i32(N), _state(), i32(N - 1))),
        ('puzzle_compat2_recalc', re.escape("st['compat']"), lambda: ops.puzzle_compat2_recalc(dq2, i32(N), dict(_state(), compat=f32(4, N, N)), i32(N))),
        ('puzzle_compat2_recalc', re.escape("st['min_d']"), lambda: ops.puzzle_compat2_recalc(dq2, i32(N), dict(_state(), min_d=i32(N, 4)), i32(N))),
        ('puzzle_best_slot2', 'mutual', lambda: ops.puzzle_best_slot2(f32(4, N, N), i32(N), i32(3), i32(3))),
        ('puzzle_best_slot2', 'mutual', lambda: ops.puzzle_best_slot2(f32(4, N, N, 4).double(), i32(N), i32(3), i32(3))),
        ('puzzle_best_slot2', 'placed', lambda: ops.puzzle_best_slot2(f32(4, N, N, 4), i32(N - 1), i32(3), i32(3))),
        ('puzzle_best_slot2', 'slot_side', lambda: ops.puzzle_best_slot2(f32(4, N, N, 4), i32(N), i32(3), i32(2))),
        ('puzzle_best_slot2', 'slot_piece', lambda: ops.puzzle_best_slot2(f32(4, N, N, 4), i32(N), i32(0), i32(0))),
        ('puzzle_best_slot2', 'out', lambda: ops.puzzle_best_slot2(f32(4, N, N, 4), i32(N), i32(3), i32(3), out=i32(1))),
        ('puzzle_assemble2', 'pieces', lambda: ops.puzzle_assemble2(pieces.float(), ident, rot, ident, 13)),
        ('puzzle_assemble2', 'locations', lambda: ops.puzzle_assemble2(pieces, ident[[0, 0, 2, 3, 4, 5]], rot, ident, 13)),
        ('puzzle_assemble2', 'rotations', lambda: ops.puzzle_assemble2(pieces, ident, rot[:5], ident, 13)),
        ('puzzle_assemble2', 'rotations', lambda: ops.puzzle_assemble2(pieces, ident, rot + 4, ident, 13)),
        ('puzzle_assemble2', 'rotations', lambda: ops.puzzle_assemble2(pieces, ident, rot.astype(np.float64), ident, 13)),
        ('puzzle_assemble2', 'true_locations', lambda: ops.puzzle_assemble2(pieces, ident, rot, ident[:, :1], 13)),
        ('puzzle_assemble2', 'marker', lambda: ops.puzzle_assemble2(pieces, ident, rot, ident, 11, marker=(0, 0, 255))),
        ('puzzle_assemble2', 'needs 2 <= eroded', lambda: ops.puzzle_assemble2(pieces, ident, rot, ident, 9)),
        ('puzzle_assemble2', 'out', lambda: ops.puzzle_assemble2(pieces, ident, rot, ident, 13, out=u8(26, 39))),
    ]
    for op, name, call in refused:
        with pytest.raises(ValueError, match=rf'^{op}: {name}(?!\w)'):
            call()
        assert not ops.calls, (op, name)
