"""Pillow's resize at any scale, the parts that need no GPU: the numpy statement of the rule against Pillow itself, the window / fill /
crop composition and the two evaluation transforms against the same composition built with Pillow, the crop origins as numbers, every
refusal of ``vited_resample_u8`` before a launch, its derived signature, and the host check under the sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 5), (7, 7), (9, 9), (13, 13), (16, 16), (33, 33), (37, 37), (48, 50), (50, 48), (64, 64), (100, 100), (130, 130), (257, 257)]
TARGETS = (1, 4, 8, 16, 32, 64, 65)
EVAL_SIZES = [(500, 530), (512, 512), (700, 300), (40, 900)]           # (H, W)


def _pil_resize(a, Rh, Rw):
    return np.asarray(Image.fromarray(a).resize((Rw, Rh), Image.BILINEAR))


# ---- the rule -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_rule_equals_pillow(vited, shape):
    """Up-scaling, the identity, non-integer and non-square down-scaling, down to one pixel: bit for bit."""
    img = np.random.default_rng(shape[0] * 1000 + shape[1]).integers(0, 256, size=(*shape, 3), dtype=np.uint8)
    for S in TARGETS:
        assert np.array_equal(vited.ops.resample_image(img, S, S), _pil_resize(img, S, S)), S
    assert np.array_equal(vited.ops.resample_image(img, 11, 29), _pil_resize(img, 11, 29))         # two different axes


def test_taps_as_literals(vited):
    first, count, k = vited.ops.resample_taps(2, 4)                    # up: support 1, three taps, clipped at both ends
    assert first.tolist() == [0, 0, 0, 1] and count.tolist() == [1, 2, 2, 1]
    assert k.tolist() == [[4194304, 0, 0], [3145728, 1048576, 0], [1048576, 3145728, 0], [4194304, 0, 0]]
    first, count, k = vited.ops.resample_taps(4, 2)                    # down 2x: support 2, five taps, weights 3 : 3 : 1 of 7
    assert first.tolist() == [0, 1] and count.tolist() == [3, 3]
    assert k.tolist() == [[1797559, 1797559, 599186, 0, 0], [599186, 1797559, 1797559, 0, 0]]
    first, count, k = vited.ops.resample_taps(16, 16)                  # the identity
    assert first.tolist() == list(range(16)) and k[:, 0].tolist() == [1 << 22] * 16 and not k[:, 1:].any()
    for dt in (first, count, k):
        assert dt.dtype == np.int32
    assert vited.ops.resample_ksize(128, 16) == 17 == vited.ops.resample_taps(128, 16)[2].shape[1] == vited.ops.RESAMPLE_MAX_TAPS
    assert vited.ops.resample_ksize(100, 16) == 15 and vited.ops.resample_ksize(5, 16) == 3 and vited.ops.resample_ksize(33, 32) == 5
    with pytest.raises(ValueError, match='resample_taps'):
        vited.ops.resample_taps(0, 4)


def test_tables(vited):
    t = vited.ops.resample_tables([100, 16, 5, 16, 128], 16, 'cpu')
    assert t.lengths.tolist() == [5, 16, 100, 128] and t.ksize == 17 and t.max_len == 128 and t.out_len == 16
    assert t.table.shape == (4, 16, 19) and t.table.dtype == torch.int32
    for c, n in enumerate(t.lengths.tolist()):
        first, count, k = vited.ops.resample_taps(n, 16)
        assert t.table[c, :, 0].tolist() == first.tolist() and t.table[c, :, 1].tolist() == count.tolist()
        assert np.array_equal(t.table[c, :, 2: 2 + k.shape[1]].numpy(), k) and not t.table[c, :, 2 + k.shape[1]:].any()
    for lens, out in (([129], 16), ([64], 1025), ([0], 4)):           # 8.06x, too long, not a length
        with pytest.raises(ValueError, match='resample_tables'):
            vited.ops.resample_tables(lens, out, 'cpu')


# ---- window, fill and crop ----------------------------------------------------------------------------------------------------------
def _store(vited, images):
    return vited.engine.Div2kImageStore(images, 'cpu')


def test_window_fill_and_crop_equal_pillow(vited):
    rng = np.random.default_rng(9)
    images = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((33, 37), (64, 64), (7, 9))]
    st = _store(vited, images)
    image = torch.tensor([0, 1, 2, 0, 1], dtype=torch.int32)
    windows = torch.tensor([[-5, -7, 40, 44], [20, 25, 60, 50], [-10, 2, 30, 9], [3, -300, 12, 12], [0, 0, 64, 64]], dtype=torch.int32)
    for fill in (0, 255):
        out = torch.full((5, 2, 3, 20, 20), 0xA5, dtype=torch.uint8)
        got = vited.ops.resample_u8(st.data, st.offsets, st.sizes, image, windows, fill, None, None, 31, 26, 6, 3, 20, out=out[:, 1])
        assert got.data_ptr() == out[:, 1].data_ptr() and bool((out[:, 0] == 0xA5).all())
        for b in range(5):
            top, left, h, w = windows[b].tolist()
            canvas = Image.new('RGB', (w, h), (fill,) * 3)
            canvas.paste(Image.fromarray(images[int(image[b])]), (-left, -top))
            want = np.asarray(canvas.resize((26, 31), Image.BILINEAR).crop((3, 6, 23, 26)))
            assert np.array_equal(got[b].numpy(), want.transpose(2, 0, 1)), (fill, b)
    whole = vited.ops.resample_u8(st.data, st.offsets, st.sizes, torch.tensor([2, 0]), None, 0, None, None, 12, 15, 0, 0, 12)
    assert np.array_equal(whole[0].numpy(), _pil_resize(images[2], 12, 15)[:, :12].transpose(2, 0, 1))
    assert np.array_equal(whole[1].numpy(), _pil_resize(images[0], 12, 15)[:, :12].transpose(2, 0, 1))
    for bad in (dict(crop_top=12), dict(crop_left=-1), dict(fill=256)):            # a crop outside the resized image; no uint8
        kw = dict(fill=0, crop_top=0, crop_left=0)
        kw.update(bad)
        with pytest.raises(ValueError, match='resample_u8'):
            vited.ops.resample_u8(st.data, st.offsets, st.sizes, image, windows, kw['fill'], None, None, 31, 26, kw['crop_top'], kw['crop_left'], 20)


def _michigan_pil(a, S):
    """PadCenterCrop((S, S), pad_if_needed, fill 255) -> Resize(int(1.15 S)) -> CenterCrop(S) with Pillow, as torchvision composes them."""
    img = Image.fromarray(a)
    for axis in (0, 1):                                                             # the width first, then the height
        n = img.size[axis]
        if n < S:
            d = S - n
            size = (n + 2 * d, img.size[1]) if axis == 0 else (img.size[0], n + 2 * d)
            canvas = Image.new('RGB', size, (255, 255, 255))
            canvas.paste(img, (d, 0) if axis == 0 else (0, d))
            img = canvas
    left, top = int(round((img.size[0] - S) / 2.0)), int(round((img.size[1] - S) / 2.0))
    img = img.crop((left, top, left + S, top + S))
    R = int(S * 1.15)
    c = int(round((R - S) / 2.0))
    return np.asarray(img.resize((R, R), Image.BILINEAR).crop((c, c, c + S, c + S))).transpose(2, 0, 1)


def _center_crop_pil(a, S):
    """torchvision's center_crop(S) with Pillow: zero padding of a short axis, (S - n) // 2 in front and (S - n + 1) // 2 behind."""
    img = Image.fromarray(a)
    w, h = img.size
    if w < S or h < S:
        pl, pt = ((S - w) // 2 if w < S else 0), ((S - h) // 2 if h < S else 0)
        pr, pb = ((S - w + 1) // 2 if w < S else 0), ((S - h + 1) // 2 if h < S else 0)
        canvas = Image.new('RGB', (w + pl + pr, h + pt + pb), (0, 0, 0))
        canvas.paste(img, (pl, pt))
        img = canvas
    left, top = int(round((img.size[0] - S) / 2.0)), int(round((img.size[1] - S) / 2.0))
    return np.asarray(img.crop((left, top, left + S, top + S))).transpose(2, 0, 1)


ORIGINS = {       # S -> (top, left) per image of EVAL_SIZES; the two transforms agree on them (every deficit here is even)
    64: [[218, 233], [224, 224], [318, 118], [-12, 418]],
    512: [[-6, 9], [0, 0], [94, -106], [-236, 194]],
}


@pytest.fixture(scope='module')
def eval_images():
    rng = np.random.default_rng(21)
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in EVAL_SIZES]


@pytest.mark.parametrize('S', (64, 512))
def test_evaluation_sources_equal_pillow(vited, eval_images, S):
    st = _store(vited, eval_images)
    mich, crop = vited.engine.MichiganEvalSource(st, S), vited.engine.CenterCropSource(st, S)
    assert len(mich) == len(crop) == 4
    assert mich.windows.tolist() == crop.windows.tolist() == [o + [S, S] for o in ORIGINS[S]]
    assert (mich.resized, mich.crop, mich.fill) == ({64: 73, 512: 588}[S], {64: 4, 512: 38}[S], 255) and (crop.resized, crop.crop, crop.fill) == (S, 0, 0)
    got_m, got_c = mich(0, 4), crop(0, 4)
    assert got_m.shape == got_c.shape == (4, 3, S, S) and got_m.dtype == torch.uint8
    for k, a in enumerate(eval_images):
        assert np.array_equal(got_m[k].numpy(), _michigan_pil(a, S)), k
        assert np.array_equal(got_c[k].numpy(), _center_crop_pil(a, S)), k
    assert torch.equal(mich(1, 3), got_m[1:3]) and torch.equal(crop(3, 4), got_c[3:])
    with pytest.raises(IndexError):
        mich(2, 5)


def test_crop_origins_round_half_to_even_and_odd_deficits(vited):
    """Where the two transforms differ: an odd deficit d pads d // 2 in front under CenterCrop, d - round(d / 2) under PadCenterCrop."""
    rng = np.random.default_rng(22)
    images = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((67, 69), (59, 61), (64, 71))]
    st = _store(vited, images)
    mich, crop = vited.engine.MichiganEvalSource(st, 64), vited.engine.CenterCropSource(st, 64)
    assert crop.windows[:, :2].tolist() == [[2, 2], [-2, -1], [0, 4]]              # round(1.5) = 2, round(2.5) = 2, round(3.5) = 4
    assert mich.windows[:, :2].tolist() == [[2, 2], [-3, -1], [0, 4]]              # deficit 5: round(2.5) - 5; deficit 3: round(1.5) - 3
    assert [int(64 * 1.15), int(384 * 1.15), int(512 * 1.15)] == [73, 441, 588]
    got_m, got_c = mich(0, 3), crop(0, 3)
    for k, a in enumerate(images):
        assert np.array_equal(got_m[k].numpy(), _michigan_pil(a, 64)) and np.array_equal(got_c[k].numpy(), _center_crop_pil(a, 64)), k


# ---- the entry point ----------------------------------------------------------------------------------------------------------------
def test_entry_point_refuses_before_a_launch(vited):
    """Every bad-argument and unsupported case of vited_resample_u8 returns its code before any launch (no GPU here: a launch would
    fail differently)."""
    lib = vited._lib.load()
    C = ctypes
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    assert vited._lib.SIGNATURES['vited_resample_u8'] == (i, [p, p, p, i, p, p, i, p, p, i, i, p, p, i, i, i, i, i, i, i, i, i, p, i64, i64, p])
    BAD, UNSUPPORTED = 1, 2
    buf = (C.c_int64 * 4096)()
    q = C.addressof(buf)

    def call(store=q, img_off=q, img_hw=q, n_images=3, image=q, windows=None, fill=0, xtab=q, xcls=q, ncx=1, ksx=17, ytab=q, ycls=q, ncy=1,
             ksy=17, max_h=128, max_w=128, Rh=16, Rw=16, crop_top=0, crop_left=0, S=16, out=q + 16384, out_bs=3 * 16 * 16, batch=2):
        return lib.vited_resample_u8(store, img_off, img_hw, n_images, image, windows, fill, xtab, xcls, ncx, ksx, ytab, ycls, ncy, ksy, max_h,
                                     max_w, Rh, Rw, crop_top, crop_left, S, out, out_bs, batch, None)

    assert call(max_h=130) == UNSUPPORTED and call(max_w=130) == UNSUPPORTED                              # a ratio of 8.125
    assert call(Rh=1025, max_h=1025) == UNSUPPORTED and call(Rw=1025, max_w=1025) == UNSUPPORTED          # out_len 1025
    assert call(ksx=19) == UNSUPPORTED and call(ksy=18) == UNSUPPORTED                                    # more taps than 8x needs
    assert call(xtab=None) == BAD and call(ytab=None) == BAD and call(xcls=None) == BAD and call(ycls=None) == BAD      # a null table
    assert call(store=None) == BAD and call(img_off=None) == BAD and call(img_hw=None) == BAD and call(image=None) == BAD
    assert call(out=None) == BAD
    assert call(crop_top=1) == BAD and call(crop_left=-1) == BAD and call(S=17) == BAD                    # a crop outside the resized image
    assert call(Rh=20, Rw=20, max_h=20, max_w=20, crop_top=5, crop_left=4) == BAD
    assert call(out_bs=3 * 16 * 16 - 1) == BAD and call(out_bs=0) == BAD                                  # overlapping samples
    assert call(ksy=15) == BAD and call(ksx=3) == BAD                                                     # tables narrower than max_h / max_w need
    assert call(fill=256) == BAD and call(fill=-1) == BAD
    assert call(batch=0) == BAD and call(batch=65536) == BAD and call(n_images=0) == BAD and call(ncx=0) == BAD and call(S=0) == BAD
    assert call(xtab=q + 2) == BAD and call(img_off=q + 4) == BAD and call(windows=q + 1) == BAD          # misaligned
    assert call(max_h=0) == BAD and call(Rw=0) == BAD


def test_header_ctypes_and_library_agree(vited):
    assert 'vited_resample_u8' in vited._lib.header_declared_functions()
    out = subprocess.run(['nm', '-D', '--defined-only', vited._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-1] == 'vited_resample_u8' and ' T ' in line for line in out.splitlines())
    assert sorted(vited._lib.header_declared_functions()) == sorted(vited._lib.SIGNATURES)
    fn = vited._lib.load().vited_resample_u8
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == vited._lib.SIGNATURES['vited_resample_u8'][1]
    assert (vited.ops.RESAMPLE_MAX_OUT, vited.ops.RESAMPLE_MAX_RATIO, vited.ops.RESAMPLE_MAX_TAPS) == (vited.ops.PUZZLE_MAX_SIZE, 8, 17)
    header = open(os.path.join(ROOT, 'vit-ed_amd', 'csrc', 'resample_u8.h')).read()
    for name, value in (('RS_MAX_OUT', 1024), ('RS_MAX_RATIO', 8), ('RS_MAX_TAPS', 17), ('RS_BITS', 22)):
        assert f'#define {name} {value} ' in header, name


def test_cpu_path_checks_its_operands(vited):
    """The CPU path checks its operands too, by name."""
    st = _store(vited, [np.zeros((8, 8, 3), np.uint8)])
    with pytest.raises(ValueError, match='resample_u8: windows'):
        vited.ops.resample_u8(st.data, st.offsets, st.sizes, torch.tensor([0], dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), 0, None,
                              None, 4, 4, 0, 0, 4)
    with pytest.raises(ValueError, match='resample_u8: out'):
        vited.ops.resample_u8(st.data, st.offsets, st.sizes, torch.tensor([0], dtype=torch.int32), None, 0, None, None, 4, 4, 0, 0, 4,
                              out=torch.zeros(1, 3, 5, 4, dtype=torch.uint8))


def test_host_check_runs_clean_under_the_sanitizers(tmp_path):
    """tools/resample_host_check.cpp: the text of csrc/resample_u8.h driven in the kernel's schedule, band by band, over exactly-sized heap
    buffers against a scalar statement written out a second time - a stand-alone program with its own main, built with
    -fsanitize=address,undefined."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    cxx = next((c for c in (shutil.which('clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'))
                if c and os.path.exists(c)), None)
    assert cxx is not None, 'no clang++ beside hipcc: the HIP toolchain that builds the library ships one'
    exe = str(tmp_path / 'resample_host_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                    os.path.join(ROOT, 'vit-ed_amd', 'csrc'), os.path.join(ROOT, 'tools', 'resample_host_check.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'resample_host_check ok' in run.stdout and not run.stderr.strip(), run.stdout + run.stderr
