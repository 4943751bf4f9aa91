"""CPU: the pixel rules of the classical puzzle baseline.  The numpy restatement (tests/puzzle_pixels_cases.py) reproduces what the
reference's own code wrote into the fixtures; csrc/puzzle_pixels.h - the text the kernels run - reproduces them through a stand-alone
host program under the sanitizers; the entry points are declared, bound, exported and refuse bad arguments without a launch; the
wrappers refuse what they must before the library is reached."""
import ctypes
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import puzzle_pixels_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('vited_puzzle_cut', 'vited_puzzle_resize_pieces', 'vited_puzzle_pixel_distances_workspace_bytes',
           'vited_puzzle_pixel_distances', 'vited_puzzle_assemble')
RESIZE = {'pixel_puzzle_odd_5x6': 16, 'pixel_puzzle_noisy_8x9': 64, 'pixel_puzzle_half_6x5': 32, 'pixel_puzzle_poster_7x8': 10,
          'pixel_puzzle_clean_6x7': 28}          # We -> S: 15 -> 16, 14 -> 64, 10 -> 32, and We = S twice


def _locations(g):
    loc = g['final_loc']
    return loc - loc.min(axis=0)


# ---- the numpy rules against the reference's fixtures -----------------------------------------------------------------------------
@pytest.mark.parametrize('name', pc.FIXTURES)
def test_numpy_rules_reproduce_the_reference(name):
    g = pc.fixture(name)
    P, We = int(g['piece_width']), g['pieces'].shape[1]
    assert We == pc.eroded_width(P, float(g['erosion']))
    pieces = pc.cut(g['image'], P, We, g['perm'])
    np.testing.assert_array_equal(pieces, g['pieces'])
    rows, cols = g['grid']
    np.testing.assert_array_equal(np.stack([g['perm'] // cols, g['perm'] % cols], axis=1), g['true_loc'])
    np.testing.assert_array_equal(pc.distances(pieces), g['Dq'])
    np.testing.assert_array_equal(pc.board(pieces, _locations(g), g['true_loc'], P, pc.marker_for(P, We)), g['board'])


def test_fixtures_cover_what_they_are_there_for():
    g = {name: pc.fixture(name) for name in pc.FIXTURES}
    widths = {name: (int(f['piece_width']), f['pieces'].shape[1]) for name, f in g.items()}
    assert widths['pixel_puzzle_clean_6x7'] == (28, 28) and g['pixel_puzzle_clean_6x7']['perfect'] == 1
    H, W = g['pixel_puzzle_clean_6x7']['image'].shape[:2]
    assert (H % 28) % 2 == 1 and (W % 28) % 2 == 0 and W % 28 > 0                # an odd and an even remainder
    assert widths['pixel_puzzle_odd_5x6'] == (16, 15) and widths['pixel_puzzle_half_6x5'] == (13, 10)     # offsets round(0.5), round(1.5)
    noisy = g['pixel_puzzle_noisy_8x9']
    assert widths['pixel_puzzle_noisy_8x9'] == (16, 14) and 0.3 < noisy['acc'][2] < 1 and noisy['recalcs'] >= 1
    framed = (_locations(noisy) != noisy['true_loc']).any(axis=1)
    assert framed.any() and not framed.all()                                    # framed and unframed pieces on one board
    poster = g['pixel_puzzle_poster_7x8']['Dq']
    off = poster[poster != pc.DQ_UNSET]
    assert (off == 0).sum() > 0 and np.unique(off).size < off.size // 10        # zeros and many ties
    lo, hi = 0, 0
    for f in g.values():
        border, second = pc.side_lines(f['pieces'])
        lo, hi = min(lo, (2 * border - second).min()), max(hi, (2 * border - second).max())
    assert (lo, hi) == (-255, 510)
    largest = os.path.getsize(os.path.join(pc.GOLDEN, 'puzzle_noisy_14x18.npz'))
    assert all(os.path.getsize(os.path.join(pc.GOLDEN, name + '.npz')) <= largest for name in pc.FIXTURES)


def test_crop_offset_rounds_half_to_even():
    img = np.arange(13 * 16 * 3, dtype=np.uint32).reshape(13, 16, 3).astype(np.uint8)
    np.testing.assert_array_equal(pc.cut(img[:, :13], 13, 10)[0], img[2:12, 2:12])      # P - We = 3: round(1.5) = 2
    np.testing.assert_array_equal(pc.cut(img[:, :13], 13, 12)[0], img[0:12, 0:12])      # P - We = 1: round(0.5) = 0
    np.testing.assert_array_equal(pc.cut(img[:, :13], 13, 8)[0], img[2:10, 2:10])       # P - We = 5: round(2.5) = 2


# ---- the header's text on the host, under the sanitizers -----------------------------------------------------------------------------
def _case_bytes(image, P, We, order, cells, rows, cols, S, marker):
    colour = -1 if marker is None else marker[0] | marker[1] << 8 | marker[2] << 16
    head = np.array([image.shape[0], image.shape[1], P, We, rows * cols, rows, cols, S, colour, order is not None], '<i4')
    parts = [head.tobytes(), np.ascontiguousarray(image).tobytes()]
    if order is not None:
        parts.append(np.asarray(order, '<i4').tobytes())
    return b''.join(parts + [np.asarray(cells, '<i4').tobytes()])


def _fnv(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & (2 ** 64 - 1)
    return f'{h:016x}'


def test_host_program_gives_the_golden_values_under_the_sanitizers(tmp_path):
    """tools/puzzle_pixels_host_check.cpp: the cut, strip, distance, resize and board code of csrc/puzzle_pixels.h over every fixture
    (and an unpermuted, unframed case) - a stand-alone program with its own main, built with -fsanitize=address,undefined."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    cxx = next((c for c in (shutil.which('clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'))
                if c and os.path.exists(c)), None)
    assert cxx is not None, 'no clang++ beside hipcc: the HIP toolchain that builds the library ships one'
    exe = str(tmp_path / 'puzzle_pixels_host_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off', '-I',
                    os.path.join(ROOT, 'vit-ed_amd', 'csrc'), os.path.join(ROOT, 'tools', 'puzzle_pixels_host_check.cpp'), '-o', exe], check=True)
    blobs, want = [], []
    for name in pc.FIXTURES:
        g = pc.fixture(name)
        P, We, (rows, cols), S = int(g['piece_width']), g['pieces'].shape[1], g['grid'], RESIZE[name]
        loc, marker = _locations(g), pc.marker_for(P, We)
        cells = np.full(rows * cols, -1)
        cells[loc[:, 0] * cols + loc[:, 1]] = 2 * np.arange(rows * cols) + ((loc != g['true_loc']).any(axis=1) if marker else 0)
        blobs.append(_case_bytes(g['image'], P, We, g['perm'], cells, rows, cols, S, marker))
        want.append((g['pieces'], g['Dq'], pc.pillow_resize(g['pieces'], S), g['board']))
    g = pc.fixture('pixel_puzzle_half_6x5')             # no order, no marker, one empty cell and one piece id outside [0, n)
    pieces = pc.cut(g['image'], 13, 10)
    ident = np.stack([np.arange(30) // 5, np.arange(30) % 5], axis=1)
    cells = 2 * np.arange(30) + 1
    cells[7], cells[11] = -1, 2 * 30
    expect = pc.board(pieces, ident, ident, 13)
    expect[13:26, 26:39], expect[26:39, 13:26] = 0, 0
    blobs.append(_case_bytes(g['image'], 13, 10, None, cells, 6, 5, 24, None))
    want.append((pieces, pc.distances(pieces), pc.pillow_resize(pieces, 24), expect))
    (tmp_path / 'cases.bin').write_bytes(np.array([len(blobs)], '<i4').tobytes() + b''.join(blobs))
    run = subprocess.run([exe, str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.split('\n')
    assert lines[len(want)] == f'puzzle_pixels_host_check ok: {len(want)} cases'
    got = np.fromfile(tmp_path / 'out.bin', np.uint8)
    at = 0
    for q, arrays in enumerate(want):
        for what, a in zip(('pieces', 'dq', 'resized', 'board'), arrays):
            a = np.ascontiguousarray(a)
            np.testing.assert_array_equal(got[at:at + a.nbytes].view(a.dtype).reshape(a.shape), a, err_msg=f'case {q} {what}')
            at += a.nbytes
        assert lines[q] == f'{q} pieces {_fnv(arrays[0])} dq {_fnv(arrays[1])} resized {_fnv(arrays[2])} board {_fnv(arrays[3])}'
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
    assert L.SIGNATURES['vited_puzzle_cut'] == (i, [p, i64, i64, i, i, p, i64, p, p])
    assert L.SIGNATURES['vited_puzzle_resize_pieces'] == (i, [p, i64, i, i, p, p])
    assert L.SIGNATURES['vited_puzzle_pixel_distances_workspace_bytes'] == (i64, [i64, i])
    assert L.SIGNATURES['vited_puzzle_pixel_distances'] == (i, [p, i64, i, p, p, i64, p])
    assert L.SIGNATURES['vited_puzzle_assemble'] == (i, [p, i64, i, i, p, i64, i64, i, p, p])
    out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if ' T ' in l}
    for name in ENTRIES:
        assert re.search(rf'\b{name}\s*\(', text) and name in exported, name


def test_entry_points_refuse_bad_arguments_without_a_launch(vited):
    _ensure_built(vited)
    lib = vited._lib.load()
    buf = (ctypes.c_uint8 * 4096)()
    a = ctypes.addressof(buf)
    a += -a % 8
    BAD, UNSUPPORTED, WORKSPACE = 1, 2, 4
    cut = lib.vited_puzzle_cut
    assert cut(None, 26, 39, 13, 10, None, 6, a, None) == BAD and cut(a, 26, 39, 13, 10, None, 6, None, None) == BAD
    assert cut(a, 26, 39, 13, 1, None, 6, a, None) == BAD                   # We < 2
    assert cut(a, 26, 39, 13, 14, None, 6, a, None) == BAD                  # P < We
    assert cut(a, 26, 39, 13, 10, None, 5, a, None) == BAD                  # n != rows * cols
    assert cut(a, 12, 39, 13, 10, None, 0, a, None) == BAD                  # no cell
    assert cut(a, 2 ** 31, 39, 13, 10, None, 6, a, None) == UNSUPPORTED
    resize = lib.vited_puzzle_resize_pieces
    assert resize(None, 6, 10, 32, a, None) == BAD and resize(a, 6, 10, 32, None, None) == BAD
    assert resize(a, 6, 1, 32, a, None) == BAD and resize(a, 0, 10, 32, a, None) == BAD
    assert resize(a, 6, 10, 9, a, None) == BAD                              # downscaling
    assert resize(a, 6, 10, 1025, a, None) == UNSUPPORTED
    size = lib.vited_puzzle_pixel_distances_workspace_bytes
    assert size(6, 10) == 2 * 4 * 6 * 32 * 2 and size(6, 15) == 2 * 4 * 6 * 48 * 2 and size(2, 2) == 2 * 4 * 2 * 8 * 2
    assert size(1, 10) == -1 and size(6, 1) == -1 and size(46341, 10) == -1 and size(6, 935723) == -1 and size(6, 935722) > 0
    dist = lib.vited_puzzle_pixel_distances
    assert dist(None, 6, 10, a, a, 4096, None) == BAD and dist(a, 6, 10, None, a, 4096, None) == BAD
    assert dist(a, 6, 10, a, None, 4096, None) == BAD and dist(a, 6, 10, a, a + 4, 4096, None) == BAD
    assert dist(a, 1, 10, a, a, 4096, None) == BAD and dist(a, 6, 1, a, a, 4096, None) == BAD
    assert dist(a, 46341, 10, a, a, 1 << 40, None) == UNSUPPORTED and dist(a, 6, 935723, a, a, 1 << 40, None) == UNSUPPORTED
    assert dist(a, 6, 10, a, a, size(6, 10) - 1, None) == WORKSPACE
    board = lib.vited_puzzle_assemble
    assert board(None, 6, 10, 13, a, 2, 3, -1, a, None) == BAD and board(a, 6, 10, 13, None, 2, 3, -1, a, None) == BAD
    assert board(a, 6, 10, 13, a, 2, 3, -1, None, None) == BAD
    assert board(a, 6, 1, 13, a, 2, 3, -1, a, None) == BAD and board(a, 6, 10, 9, a, 2, 3, -1, a, None) == BAD
    assert board(a, 6, 10, 13, a, 2, 2, -1, a, None) == BAD and board(a, 6, 10, 13, a, 0, 3, -1, a, None) == BAD
    assert board(a, 6, 10, 11, a, 2, 3, 0xff0000, a, None) == BAD             # a marker with pad 0
    assert board(a, 6, 10, 13, a, 2, 3, 0x1000000, a, None) == BAD
    assert board(a, 46341, 10, 13, a, 1, 46341, -1, a, None) == UNSUPPORTED


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


def test_wrappers_are_ops_functions_and_refuse_cpu_tensors(vited):
    for name in ('puzzle_cut', 'puzzle_resize_pieces', 'puzzle_pixel_distances', 'puzzle_assemble'):
        assert getattr(vited.ops, name) is getattr(vited.ops_puzzlepixels, name)
    ident = np.stack([np.arange(6) // 3, np.arange(6) % 3], axis=1)
    calls = [lambda: vited.ops.puzzle_cut(u8(26, 39, 3), 13, 10), lambda: vited.ops.puzzle_resize_pieces(u8(6, 10, 10, 3), 32),
             lambda: vited.ops.puzzle_pixel_distances(u8(6, 10, 10, 3)), lambda: vited.ops.puzzle_assemble(u8(6, 10, 10, 3), ident, ident, 13)]
    if not torch.cuda.is_available():                   # where there is a GPU the engine uploads a host image
        calls.append(lambda: vited.engine.solve_pixel_puzzle(np.zeros((26, 39, 3), np.uint8), 13, 0.25))
    for call in calls:
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    for name in ('cut_puzzle', 'puzzle_model_pieces', 'puzzle_pixel_distances', 'reconstruct_puzzle', 'solve_pixel_puzzle', 'PuzzleCut'):
        assert getattr(vited.engine, name) is getattr(vited.engine.puzzle, name)
    assert vited.ops.puzzle_eroded_width(16, 0.07) == 15 and vited.ops.puzzle_eroded_width(13, 0.25) == 10
    assert vited.ops.puzzle_eroded_width(28, 0.) == 28 and vited.ops.puzzle_eroded_width(28, -0.5) == 28


def test_valid_calls_reach_their_entry_points(ops):
    ident = np.stack([np.arange(6) // 3, np.arange(6) % 3], axis=1)
    assert ops.puzzle_cut(u8(27, 40, 3), 13, 10, order=[5, 4, 3, 2, 1, 0]).shape == (6, 10, 10, 3)
    name, args = ops.calls.pop()
    assert name == 'vited_puzzle_cut' and args[1:5] == (27, 40, 13, 10) and args[5] != 0 and args[6] == 6
    assert ops.puzzle_cut(u8(27, 40, 3), 13).shape == (6, 13, 13, 3) and ops.calls.pop()[1][5] == 0
    assert ops.puzzle_resize_pieces(u8(6, 10, 10, 3), 32).shape == (6, 3, 32, 32) and ops.calls.pop()[0] == 'vited_puzzle_resize_pieces'
    dq = ops.puzzle_pixel_distances(u8(6, 10, 10, 3))
    assert dq.shape == (4, 6, 6) and dq.dtype == torch.int32 and ops.calls.pop()[0] == 'vited_puzzle_pixel_distances'
    moved = ident[[1, 0, 2, 3, 4, 5]]
    assert ops.puzzle_assemble(u8(6, 10, 10, 3), moved, ident, 13, marker=(0, 0, 255)).shape == (26, 39, 3)
    name, args = ops.calls.pop()
    assert name == 'vited_puzzle_assemble' and args[1:4] == (6, 10, 13) and args[5:8] == (2, 3, 255 << 16)
    assert ops.puzzle_assemble(u8(6, 10, 10, 3), moved, ident, 13).shape == (26, 39, 3) and ops.calls.pop()[1][7] == -1
    assert not ops.calls


def test_wrappers_refuse_before_the_launch(ops):
    ident = np.stack([np.arange(6) // 3, np.arange(6) % 3], axis=1)
    pieces = u8(6, 10, 10, 3)
    refused = [
        ('puzzle_cut', 'image', lambda: ops.puzzle_cut(torch.zeros(27, 40, 3), 13, 10)),                       # dtype
        ('puzzle_cut', 'image', lambda: ops.puzzle_cut(u8(27, 40, 4), 13, 10)),
        ('puzzle_cut', 'image', lambda: ops.puzzle_cut(u8(27, 80, 3)[:, ::2], 13, 10)),                        # strided
        ('puzzle_cut', 'image', lambda: ops.puzzle_cut(u8(12, 40, 3), 13, 10)),                                # no cell
        ('puzzle_cut', 'needs 2 <= eroded', lambda: ops.puzzle_cut(u8(27, 40, 3), 13, 14)),
        ('puzzle_cut', 'needs 2 <= eroded', lambda: ops.puzzle_cut(u8(27, 40, 3), 13, 1)),
        ('puzzle_cut', 'order', lambda: ops.puzzle_cut(u8(27, 40, 3), 13, 10, order=[0, 1, 2, 3, 4])),
        ('puzzle_cut', 'order', lambda: ops.puzzle_cut(u8(27, 40, 3), 13, 10, order=[0, 1, 2, 3, 4, 4])),       # not a permutation
        ('puzzle_cut', 'order', lambda: ops.puzzle_cut(u8(27, 40, 3), 13, 10, order=[0, 1, 2, 3, 4, 6])),
        ('puzzle_cut', 'order', lambda: ops.puzzle_cut(u8(27, 40, 3), 13, 10, order=[0., 1., 2., 3., 4., 5.])),
        ('puzzle_cut', 'out', lambda: ops.puzzle_cut(u8(27, 40, 3), 13, 10, out=u8(6, 10, 10, 4))),
        ('puzzle_resize_pieces', 'pieces', lambda: ops.puzzle_resize_pieces(pieces.float(), 32)),
        ('puzzle_resize_pieces', 'pieces', lambda: ops.puzzle_resize_pieces(u8(6, 10, 9, 3), 32)),
        ('puzzle_resize_pieces', 'pieces', lambda: ops.puzzle_resize_pieces(u8(6, 1, 1, 3), 32)),
        ('puzzle_resize_pieces', 'size', lambda: ops.puzzle_resize_pieces(pieces, 9)),
        ('puzzle_resize_pieces', 'size', lambda: ops.puzzle_resize_pieces(pieces, 1025)),
        ('puzzle_resize_pieces', 'out', lambda: ops.puzzle_resize_pieces(pieces, 32, out=u8(6, 32, 32, 3))),
        ('puzzle_pixel_distances', 'pieces', lambda: ops.puzzle_pixel_distances(u8(6, 10, 10))),
        ('puzzle_pixel_distances', 'pieces', lambda: ops.puzzle_pixel_distances(u8(1, 10, 10, 3))),
        ('puzzle_pixel_distances', 'pieces', lambda: ops.puzzle_pixel_distances(u8(6, 10, 10, 6)[..., ::2])),
        ('puzzle_pixel_distances', 'out', lambda: ops.puzzle_pixel_distances(pieces, out=torch.zeros(4, 6, 6, dtype=torch.int64))),
        ('puzzle_assemble', 'locations', lambda: ops.puzzle_assemble(pieces, ident[:5], ident, 13)),
        ('puzzle_assemble', 'locations', lambda: ops.puzzle_assemble(pieces, ident[[0, 0, 2, 3, 4, 5]], ident, 13)),       # colliding
        ('puzzle_assemble', 'locations', lambda: ops.puzzle_assemble(pieces, ident + [0, 1], ident, 13)),                 # outside the board
        ('puzzle_assemble', 'locations', lambda: ops.puzzle_assemble(pieces, ident - [1, 0], ident, 13)),
        ('puzzle_assemble', 'locations', lambda: ops.puzzle_assemble(pieces, ident.astype(np.float64), ident, 13)),
        ('puzzle_assemble', 'true_locations', lambda: ops.puzzle_assemble(pieces, ident, ident[:, :1], 13)),
        ('puzzle_assemble', 'marker', lambda: ops.puzzle_assemble(pieces, ident, ident, 11, marker=(0, 0, 255))),           # pad 0
        ('puzzle_assemble', 'marker', lambda: ops.puzzle_assemble(pieces, ident, ident, 13, marker=(0, 0, 256))),
        ('puzzle_assemble', 'marker', lambda: ops.puzzle_assemble(pieces, ident, ident, 13, marker=(0, 255))),
        ('puzzle_assemble', 'needs 2 <= eroded', lambda: ops.puzzle_assemble(pieces, ident, ident, 9)),
        ('puzzle_assemble', 'out', lambda: ops.puzzle_assemble(pieces, ident, ident, 13, out=u8(26, 39))),
    ]
    for op, name, call in refused:
        with pytest.raises(ValueError, match=rf'^{op}: {name}(?!\w)'):
            call()
        assert not ops.calls, (op, name)
