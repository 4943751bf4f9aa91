"""CPU: the learned type-2 puzzle path (pieces turned by quarter turns under the pair model).  The numpy statement of the rule
(tests/puzzle_rot_cases.py) is checked against numpy.rot90 itself and for covering the 16 side pairings once each; the text of
csrc/puzzle_turn.h reproduces the source pixels and the Dq2 slots through a stand-alone host program under the sanitizers; the new entry
points are declared, bound, exported and refuse bad arguments without a launch; the wrappers refuse before the library is reached; the
engine's new surface exists; and the inputs of the GPU tests have the properties those tests lean on."""
import ctypes
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import puzzle_rot_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('vited_patchify_turned', 'vited_patchify_turned_u8', 'vited_puzzle_distances2_from_logits')


# ---- the rule in numpy -------------------------------------------------------------------------------------------------------------------
def test_a_turn_is_rot90_clockwise_and_moves_the_borders():
    x = rc.border_piece(6)
    for k in range(4):
        t = rc.turn(x, k)
        np.testing.assert_array_equal(t, np.rot90(x, -k))
        for s in range(4):
            inner = rc.side_line(x, s)[1:-1]
            assert len(set(inner.tolist())) == 1
            np.testing.assert_array_equal(rc.side_line(t, rc.moved_side(s, k))[1:-1], inner)
    assert len({int(rc.side_line(x, s)[1]) for s in range(4)}) == 4          # four borders, four values: a wrong direction shows
    once = rc.turn(x, 1)
    assert rc.side_line(once, 1)[1] == 10 and rc.side_line(once, 0)[1] == 40          # clockwise: the top goes right, the left goes top
    batch = np.stack([x, 2 * x])[:, None]
    np.testing.assert_array_equal(rc.turn(batch, 3)[1, 0], np.rot90(2 * x, -3))       # the default axes are the last two


def test_turns_and_bins_cover_the_16_pairings_once():
    seen = {}
    for k in range(4):
        for b in range(4):
            si, sj = rc.bin_sides(k, b)
            assert (si + 3) % 4 == b and rc.pair_turn(si, sj) == k
            assert rc.moved_side(sj, k) == (si + 2) % 4              # the turned side sj faces side si
            seen[(si, sj)] = (k, b)
    assert sorted(seen) == [(si, sj) for si in range(4) for sj in range(4)]
    for b in range(4):
        si, sj = rc.bin_sides(0, b)
        assert sj == (si + 2) % 4                                        # no turn: the type-1 rule


def test_the_two_statements_of_the_scatter_agree_and_hold_type1():
    n = 5
    rng = np.random.default_rng(1)
    logits = rng.normal(0, 3, size=(n, n, 4, 4)).astype(np.float32)
    dq2 = rc.dq2_from_logits(logits)
    pi, pjt = rc.all_pairs(n)
    got, refused = rc.scatter(n, logits[pi, pjt % n, pjt // n], pi, pjt)
    assert refused == 0
    np.testing.assert_array_equal(got, dq2)
    for s in range(4):
        type1 = rc.quantise(logits[:, :, 0, (s + 3) % 4]).astype(np.int64)
        np.fill_diagonal(type1, rc.DQ_UNSET)
        np.testing.assert_array_equal(dq2[s, :, :, (s + 2) % 4], type1)
    assert (dq2[:, np.arange(n), np.arange(n), :] == rc.DQ_UNSET).all()


def test_the_scatter_logits_are_what_the_gpu_test_needs():
    logits, fixed = rc.scatter_logits(4 * 17 * 16, 0)
    flat = logits.reshape(-1)
    assert rc.stable(flat).all()
    assert {40., -40., 0.}.issubset(set(flat[:fixed].tolist())) and np.signbit(flat[:fixed][flat[:fixed] == 0]).any()
    q = rc.quantise(flat[:fixed])
    assert q[0] == 0 and q[1] == 1000 and q[2] == q[3] == 500
    near = rc.near_integer_logits()
    assert near.size >= 30
    x = near.astype(np.float32)
    sig = (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)
    v = ((np.float32(1) - sig) * np.float32(1000.)).astype(np.float32)
    m = np.rint(v).astype(np.float32)
    assert ((v == m) | (v == np.nextafter(m, np.float32(0))) | (v == np.nextafter(m, np.float32(2000)))).all()
    assert (v < m).any() and (v == m).any() and (v > m).any()            # truncation lands on m - 1, m and m
    assert set(flat[:fixed].tolist()) >= set(near.tolist())


def test_the_pattern_pieces_have_no_turn_symmetry_and_the_scaled_model_sees_it():
    """The GPU composition test compares at atol 3e-2 and first needs the logits of different turns to lie more than 100 x that apart:
    checked here on the CPU oracle by the rule itself (stacked pairs of physically turned pieces)."""
    pieces = rc.pattern_pieces(4, 32)
    for k in range(1, 4):
        assert (np.abs(rc.turn(pieces, k).astype(int) - pieces).reshape(4, -1).mean(axis=1) > 10).all()
    oracle = rc.small_oracle(32, weight_scale=6.0, head_scale=100.0)
    assert rc.turn_separation(rc.turned_logits_oracle(oracle, pieces), 4) > 1.5 * 100 * 3e-2


# ---- the header's text on the host, under the sanitizers -----------------------------------------------------------------------------
def test_host_program_walks_the_source_pixels_and_the_pairing_map_under_the_sanitizers(tmp_path):
    """tools/puzzle_turn_host_check.cpp: strip_element (turned_source inside it) of csrc/puzzle_turn.h for every turn, S in {8, 16, 24},
    patch in {4, 8} and 1 and 3 channels against numpy.rot90 of an index image; bin_side_i / bin_side_j, pair_turn and moved_side against
    the numpy rule; pair_in_range and dq2_slot over every pair of n in {2, 3, 5, 17} and planted bad pairs - a stand-alone program with
    its own main, built with -fsanitize=address,undefined."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    cxx = next((c for c in (shutil.which('clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'))
                if c and os.path.exists(c)), None)
    assert cxx is not None, 'no clang++ beside hipcc: the HIP toolchain that builds the library ships one'
    exe = str(tmp_path / 'puzzle_turn_host_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                    os.path.join(ROOT, 'vit-ed_amd', 'csrc'), os.path.join(ROOT, 'tools', 'puzzle_turn_host_check.cpp'), '-o', exe], check=True)
    geometries = [(c, S, p) for c in (1, 3) for S in (8, 16, 24) for p in (4, 8)]
    blob = np.array([len(geometries)], '<i4').tobytes() + np.array(geometries, '<i4').tobytes()
    puzzles = []
    for n in (2, 3, 5, 17):
        pi, pjt = rc.all_pairs(n)
        bad_i = np.array([0, n - 1, -1, n, 1, 0, 0], np.int64)
        bad_jt = np.array([0, 4 * n - 1, 1, 1, 4 * n, -1, 2 * n], np.int64)            # j == i in turns 0, 3 and 2; outside
        puzzles.append((n, np.concatenate([pi, bad_i]), np.concatenate([pjt, bad_jt])))
    blob += np.array([len(puzzles)], '<i4').tobytes()
    for n, pi, pjt in puzzles:
        blob += np.array([n, pi.size], '<i8').tobytes() + np.stack([pi, pjt], axis=1).astype('<i8').tobytes()
    (tmp_path / 'cases.bin').write_bytes(blob)
    run = subprocess.run([exe, str(tmp_path / 'cases.bin'), str(tmp_path / 'out.bin')], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.strip() == f'puzzle_turn_host_check ok: {len(geometries)} geometries, {len(puzzles)} puzzles'
    got = np.fromfile(tmp_path / 'out.bin', np.uint8)
    at = 0

    def take(dtype, *shape):
        nonlocal at
        size = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = got[at:at + size].view(dtype).reshape(shape)
        at += size
        return a

    for c, S, p in geometries:
        index = np.arange(c * S * S, dtype=np.int64).reshape(1, c, S, S)
        for k in range(4):
            want = rc.patch_rows(np.ascontiguousarray(rc.turn(index, k)), p)
            np.testing.assert_array_equal(take('<i8', *want.shape), want, err_msg=f'chans {c} S {S} patch {p} turn {k}')
    sides = take('<i4', 4, 4, 2)
    turns = take('<i4', 4, 4)
    moved = take('<i4', 4, 4)
    for a in range(4):
        for b in range(4):
            assert tuple(sides[a, b]) == rc.bin_sides(a, b) and turns[a, b] == rc.pair_turn(a, b) and moved[a, b] == rc.moved_side(a, b)
    for n, pi, pjt in puzzles:
        filled = np.zeros(16 * n * n, np.int64)
        for i, jt in zip(pi.tolist(), pjt.tolist()):
            ok, slots = int(take('<i4', 1)[0]), take('<i8', 4)
            inside = 0 <= i < n and 0 <= jt < 4 * n and jt % n != i
            assert ok == int(inside), (n, i, jt)
            if not inside:
                assert (slots == -1).all()
                continue
            for b in range(4):
                si, sj = rc.bin_sides(jt // n, b)
                assert slots[b] == ((si * n + i) * n + jt % n) * 4 + sj, (n, i, jt, b)
            filled[slots] += 1
        off = np.broadcast_to((~np.eye(n, dtype=bool))[None, :, :, None], (4, n, n, 4)).reshape(-1)
        np.testing.assert_array_equal(filled, off.astype(np.int64))            # every off-diagonal entry once, the diagonal never
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
    assert L.SIGNATURES['vited_patchify_turned'] == (i, [p, i64, p, p, i, p, i, i64, i, i, i, p])
    assert L.SIGNATURES['vited_patchify_turned_u8'] == (i, [p, i64, p, p, i, p, i, i64, i, i, i, p, p, p])
    assert L.SIGNATURES['vited_puzzle_distances2_from_logits'] == (i, [p, p, p, i64, i64, p, p, p])
    out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if ' T ' in l}
    for name in ENTRIES:
        assert re.search(rf'\b{name}\s*\(', text) and name in exported, name
    # the existing patchify entries keep their signatures
    assert L.SIGNATURES['vited_patchify'] == (i, [p, i64, p, p, i, i64, i, i, i, p])
    assert L.SIGNATURES['vited_patchify_u8'] == (i, [p, i64, p, p, i, i64, i, i, i, p, p, p])


def test_entry_points_refuse_bad_arguments_without_a_launch(vited):
    _ensure_built(vited)
    lib = vited._lib.load()
    buf = (ctypes.c_uint8 * 4096)()
    a = ctypes.addressof(buf)
    a += -a % 16
    BAD, UNSUPPORTED = 1, 2
    F32, I32 = vited._lib.F32, vited._lib.I32
    norm = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    zero = (ctypes.c_float * 3)(0.5, 0.0, 0.5)
    f = lib.vited_patchify_turned
    assert f(None, 192, None, None, 1, a, F32, 2, 3, 8, 4, None) == BAD and f(a, 192, None, None, 1, None, F32, 2, 3, 8, 4, None) == BAD
    assert f(a, 192, None, None, 4, a, F32, 2, 3, 8, 4, None) == BAD and f(a, 192, None, None, -1, a, F32, 2, 3, 8, 4, None) == BAD
    assert f(a, 192, None, None, 1, a, F32, 0, 3, 8, 4, None) == BAD and f(a, 192, None, None, 1, a, F32, 2, 0, 8, 4, None) == BAD
    assert f(a, 192, None, None, 1, a, F32, 2, 3, 8, 3, None) == BAD and f(a, 192, None, None, 1, a, F32, 2, 3, 8, 0, None) == BAD
    assert f(a + 2, 192, None, None, 1, a, F32, 2, 3, 8, 4, None) == BAD and f(a, 192, None, a + 2, 0, a, F32, 2, 3, 8, 4, None) == BAD
    assert f(a, 192, None, None, 1, a, F32, 1 << 31, 3, 8, 4, None) == BAD
    assert f(a, 192, None, None, 1, a, I32, 2, 3, 8, 4, None) == UNSUPPORTED
    g = lib.vited_patchify_turned_u8
    assert g(None, 192, None, None, 1, a, F32, 2, 3, 8, 4, norm, norm, None) == BAD and g(a, 192, None, None, 1, None, F32, 2, 3, 8, 4, norm, norm, None) == BAD
    assert g(a, 192, None, None, 4, a, F32, 2, 3, 8, 4, norm, norm, None) == BAD and g(a, 192, None, None, 1, a, F32, 2, 3, 8, 5, norm, norm, None) == BAD
    assert g(a, 192, None, None, 1, a, F32, 2, 3, 8, 4, None, norm, None) == BAD and g(a, 192, None, None, 1, a, F32, 2, 3, 8, 4, norm, None, None) == BAD
    assert g(a, 192, None, None, 1, a, F32, 2, 3, 8, 4, norm, zero, None) == BAD and g(a, 320, None, None, 1, a, F32, 2, 5, 8, 4, norm, norm, None) == BAD
    assert g(a, 192, None, a + 1, 0, a, F32, 2, 3, 8, 4, norm, norm, None) == BAD
    assert g(a, 192, None, None, 1, a, I32, 2, 3, 8, 4, norm, norm, None) == UNSUPPORTED
    d = lib.vited_puzzle_distances2_from_logits
    full = [a] * 3
    assert d(*full, 5, 1, a, a, None) == BAD and d(*full, 5, 46341, a, a, None) == BAD and d(*full, -1, 6, a, a, None) == BAD
    assert d(*full, 5, 6, None, a, None) == BAD and d(*full, 5, 6, a, None, None) == BAD
    for k in range(3):
        assert d(*(full[:k] + [None] + full[k + 1:]), 5, 6, a, a, None) == BAD, k
    assert d(*full, 0, 6, a, a, None) == 0                                     # no pairs: nothing to launch


# ---- the wrappers, the library replaced by a recorder ---------------------------------------------------------------------------------
@pytest.fixture
def ops(vited, monkeypatch):
    calls = []
    monkeypatch.setattr(vited.ops, '_need_gpu', lambda *tensors, **kw: None)
    monkeypatch.setattr(vited.ops, '_stream', lambda: 0)
    monkeypatch.setattr(vited.ops, '_lib', SimpleNamespace(call=lambda name, *args: calls.append((name, args))))
    vited.ops.calls = calls
    yield vited.ops
    del vited.ops.calls


def u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def f32(*shape):
    return torch.zeros(shape, dtype=torch.float32)


def i64(*shape):
    return torch.zeros(shape, dtype=torch.int64)


def i32(*shape):
    return torch.zeros(shape, dtype=torch.int32)


N = 6


def test_wrappers_are_ops_functions_and_refuse_cpu_tensors(vited):
    for name in ('patchify_turned', 'puzzle_distances2_from_logits'):
        assert getattr(vited.ops, name) is getattr(vited.ops_puzzlerot, name)
    calls = [lambda: vited.ops.patchify_turned(u8(2, 3, 16, 16), 8, torch.float32, 1),
             lambda: vited.ops.patchify_turned(f32(2, 3, 16, 16), 8, torch.float32, i32(2)),
             lambda: vited.ops.puzzle_distances2_from_logits(f32(5, 4), i64(5), i64(5), i32(4, N, N, 4), i32(1))]
    for call in calls:
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    in_source = re.findall(r"_lib\.call\('(vited_\w+)'", open(os.path.join(ROOT, 'vit-ed_amd', 'ops_puzzlerot.py')).read())
    assert sorted(in_source) == sorted(ENTRIES)


def test_valid_calls_reach_their_entry_points(ops):
    out = ops.patchify_turned(u8(2, 3, 16, 16), 8, torch.float32, 3)
    assert out.shape == (8, 192) and out.dtype == torch.float32
    name, args = ops.calls.pop()
    assert name == 'vited_patchify_turned_u8' and args[1] == 768 and args[3:5] == (0, 3) and args[6:11] == (0, 2, 3, 16, 8)
    out = ops.patchify_turned(f32(3, 3, 16, 16), 4, torch.bfloat16, torch.tensor([0, 3, 2]))
    assert out.shape == (48, 48) and out.dtype == torch.bfloat16
    name, args = ops.calls.pop()
    assert name == 'vited_patchify_turned' and args[3] != 0 and args[4] == 0 and args[7:11] == (3, 3, 16, 4)
    wide = f32(2, 2, 3, 16, 16)[:, 0]                                   # a batch stride that is not dense stays a view
    ops.patchify_turned(wide, 8, torch.float32, torch.tensor([1, 2], dtype=torch.int32), batch_index=None)
    assert ops.calls.pop()[1][1] == 2 * 768
    ops.patchify_turned(u8(2, 3, 16, 16), 8, torch.float32, torch.tensor([1, 2, 3]), batch_index=torch.tensor([1, 0, 1]))
    assert ops.calls.pop()[1][7] == 3                                   # one turn per OUTPUT image
    ops.puzzle_distances2_from_logits(f32(5, 4), i64(5), i64(5), i32(4, N, N, 4), i32(1))
    name, args = ops.calls.pop()
    assert name == 'vited_puzzle_distances2_from_logits' and args[3:5] == (5, N)
    assert not ops.calls


def test_wrappers_refuse_before_the_launch(ops):
    img, dq2 = u8(2, 3, 16, 16), i32(4, N, N, 4)
    lg, pi, bad = f32(5, 4), i64(5), i32(1)
    refused = [
        ('patchify_turned', 'img', lambda: ops.patchify_turned(u8(2, 3, 16), 8, torch.float32, 1)),
        ('patchify_turned', 'img', lambda: ops.patchify_turned(u8(2, 3, 16, 8), 8, torch.float32, 1)),
        ('patchify_turned', 'img', lambda: ops.patchify_turned(img.to(torch.int32), 8, torch.float32, 1)),
        ('patchify_turned', 'img', lambda: ops.patchify_turned(img.double(), 8, torch.float32, 1)),
        ('patchify_turned', 'img', lambda: ops.patchify_turned(img, 5, torch.float32, 1)),
        ('patchify_turned', 'img', lambda: ops.patchify_turned(u8(0, 3, 16, 16), 8, torch.float32, 1)),
        ('patchify_turned', 'img', lambda: ops.patchify_turned(u8(2, 5, 16, 16), 8, torch.float32, 1)),
        ('patchify_turned', 'batch_index', lambda: ops.patchify_turned(img, 8, torch.float32, 1, batch_index=i32(2))),
        ('patchify_turned', 'turn', lambda: ops.patchify_turned(img, 8, torch.float32, 4)),
        ('patchify_turned', 'turn', lambda: ops.patchify_turned(img, 8, torch.float32, -1)),
        ('patchify_turned', 'turn', lambda: ops.patchify_turned(img, 8, torch.float32, 1.0)),
        ('patchify_turned', 'turn', lambda: ops.patchify_turned(img, 8, torch.float32, True)),
        ('patchify_turned', 'turn', lambda: ops.patchify_turned(img, 8, torch.float32, None)),
        ('patchify_turned', 'turn', lambda: ops.patchify_turned(img, 8, torch.float32, torch.tensor([0, 4]))),
        ('patchify_turned', 'turn', lambda: ops.patchify_turned(img, 8, torch.float32, torch.tensor([-1, 0]))),
        ('patchify_turned', 'turn', lambda: ops.patchify_turned(img, 8, torch.float32, torch.tensor([0, 1, 2]))),
        ('patchify_turned', 'turn', lambda: ops.patchify_turned(img, 8, torch.float32, torch.tensor([0., 1.]))),
        ('patchify_turned', 'turn', lambda: ops.patchify_turned(img, 8, torch.float32, torch.tensor([[0, 1]]))),
        ('patchify_turned', 'turn', lambda: ops.patchify_turned(img, 8, torch.float32, torch.tensor([0, 1]), batch_index=i64(3))),
        ('puzzle_distances2_from_logits', 'dq2', lambda: ops.puzzle_distances2_from_logits(lg, pi, pi, i32(4, N, N), bad)),
        ('puzzle_distances2_from_logits', 'dq2', lambda: ops.puzzle_distances2_from_logits(lg, pi, pi, i32(4, N, N + 1, 4), bad)),
        ('puzzle_distances2_from_logits', 'dq2', lambda: ops.puzzle_distances2_from_logits(lg, pi, pi, i32(4, 1, 1, 4), bad)),
        ('puzzle_distances2_from_logits', 'dq2', lambda: ops.puzzle_distances2_from_logits(lg, pi, pi, dq2.long(), bad)),
        ('puzzle_distances2_from_logits', 'dq2', lambda: ops.puzzle_distances2_from_logits(lg, pi, pi, i32(4, N, N, 8)[..., ::2], bad)),
        ('puzzle_distances2_from_logits', 'logits', lambda: ops.puzzle_distances2_from_logits(f32(5, 3), pi, pi, dq2, bad)),
        ('puzzle_distances2_from_logits', 'logits', lambda: ops.puzzle_distances2_from_logits(lg.double(), pi, pi, dq2, bad)),
        ('puzzle_distances2_from_logits', 'logits', lambda: ops.puzzle_distances2_from_logits(f32(4, 4), pi, pi, dq2, bad)),
        ('puzzle_distances2_from_logits', 'pi', lambda: ops.puzzle_distances2_from_logits(lg, pi.int(), pi, dq2, bad)),
        ('puzzle_distances2_from_logits', 'pjt', lambda: ops.puzzle_distances2_from_logits(lg, pi, i64(6), dq2, bad)),
        ('puzzle_distances2_from_logits', 'pjt', lambda: ops.puzzle_distances2_from_logits(lg, pi, pi.int(), dq2, bad)),
        ('puzzle_distances2_from_logits', 'bad', lambda: ops.puzzle_distances2_from_logits(lg, pi, pi, dq2, i32(2))),
        ('puzzle_distances2_from_logits', 'bad', lambda: ops.puzzle_distances2_from_logits(lg, pi, pi, dq2, i64(1))),
    ]
    for op, name, call in refused:
        with pytest.raises(ValueError, match=rf'^{op}: {name}(?!\w)'):
            call()
        assert not ops.calls, (op, name)


# ---- the engine's surface ----------------------------------------------------------------------------------------------------------------
def test_the_engine_surface(vited):
    import inspect
    engine = vited.engine
    assert engine.puzzle.solve_model_puzzle is engine.solve_model_puzzle
    sig = inspect.signature(engine.solve_model_puzzle)
    assert list(sig.parameters) == ['model', 'image', 'piece_width', 'erosion', 'order', 'marker', 'puzzle_type', 'distance_kw']
    assert sig.parameters['puzzle_type'].default == 1 and sig.parameters['distance_kw'].kind is inspect.Parameter.VAR_KEYWORD
    assert sig.parameters['erosion'].default == 0. and sig.parameters['order'].default is None and sig.parameters['marker'].default is None
    dist = inspect.signature(engine.puzzle_distances)
    assert dist.parameters['puzzle_type'].default == 1 and dist.parameters['puzzle_type'].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(vited.VisionTransformerCustom.cache_image2_tokens).parameters['turn'].default == 0
    for bad_type in (3, 0, '2', None):
        with pytest.raises(ValueError, match='puzzle_type'):
            engine.puzzle_distances(object(), u8(4, 3, 32, 32), puzzle_type=bad_type)
        with pytest.raises(ValueError, match='puzzle_type'):
            engine.solve_model_puzzle(object(), np.zeros((28, 28, 3), np.uint8), 14, puzzle_type=bad_type)
    with pytest.raises(TypeError, match='HIP model'):                   # the type-1 refusals still come first in their order
        engine.puzzle_distances(object(), u8(4, 3, 32, 32), puzzle_type=2)
