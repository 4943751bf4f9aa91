"""The michigan device feed without a GPU: the numpy restatement of the per-pixel definition
(tests/michigan_feed_cases.py) against Pillow itself - resample, GaussianBlur, convert('L'), the flips and one whole chain - and the
batch-level plan against a per-sample restatement of the reference's draws (michigan.py:71-85).  The kernels themselves:
tests/test_gpu_michigan_feed.py."""
import math

import numpy as np
import pytest
import torch

import michigan_feed_cases as mc


def _pil():
    pytest.importorskip('PIL')
    from PIL import Image, ImageFilter, ImageOps
    return Image, ImageFilter, ImageOps


def _resized(Image, win, box, S):
    i, j, h, w = box
    return np.asarray(Image.fromarray(win).crop((j, i, j + w, i + h)).resize((S, S), Image.BILINEAR))


# ---------------------------------------------------------------------------------------------
# the Pillow-defined pieces, against Pillow
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [16, 10, 64])
def test_resample_equals_pillow(S):
    Image, _, _ = _pil()
    rng = np.random.default_rng(70 + S)
    boxes = [(0, 0, S, S), (0, 2, S, S - 5), (3, 0, S - 4, S), (0, S // 2, S, 1), (S - 1, 0, 1, S), (S - 1, S - 1, 1, 1), (1, 1, S - 1, S - 1),
             (0, 0, S - 1, S - 1)]
    fails = 0
    for k in range(40):
        box, failed = mc.resized_crop_box(rng.random(20).tolist(), float(rng.random()), float(rng.random()), S)
        boxes.append(box)
        fails += failed
    for k, box in enumerate(boxes):
        win = rng.integers(0, 256, size=(S, S, 3), dtype=np.uint8)
        if k % 3 == 0:
            win = (win >> 6) * 85                                # four levels: every rounding is between far-apart values
        got = mc.resample_ref(win.astype(np.uint8), *mc.box_tables(box, S))
        assert np.array_equal(got, _resized(Image, win.astype(np.uint8), box, S)), (S, box)
    assert np.array_equal(mc.resample_ref(win, *mc.box_tables((0, 0, S, S), S)), win)          # the whole window: unchanged


@pytest.mark.parametrize('S', [16, 10, 64, 33])
def test_eval_tables_equal_pillow_resize_then_centre_crop(S):
    Image, _, _ = _pil()
    rng = np.random.default_rng(71 + S)
    win = rng.integers(0, 256, size=(S, S, 3), dtype=np.uint8)
    R = int(S * 1.15)
    off = int(round((R - S) / 2.0))                              # torchvision's center_crop: round half to even
    want = np.asarray(Image.fromarray(win).resize((R, R), Image.BILINEAR))[off: off + S, off: off + S]
    assert np.array_equal(mc.resample_ref(win, *mc.eval_tables(S)), want)


def test_tables_have_at_most_three_taps_inside_the_box():
    for S in (10, 16, 64):
        for w in range(1, S + 1):
            x0, kk = mc.coeffs(w, S, first=5)
            for a, k in zip(x0, kk):
                taps = [t for t in range(3) if k[t]]
                assert taps and a >= 5 and a + max(taps) < 5 + w and abs(sum(k) - (1 << 22)) <= 2 and min(k) >= 0


def test_blur_equals_pillow_gaussian_blur():
    Image, ImageFilter, _ = _pil()
    rng = np.random.default_rng(72)
    radii = [0.1, 1.0] + [float(t) for t in rng.uniform(0.1, 1.0, 238)]
    shapes = [(2, 2), (2, 7), (9, 2), (3, 3), (16, 16), (10, 10), (5, 31), (39, 4), (23, 17)]
    for k, r in enumerate(radii):
        H, W = shapes[k % len(shapes)] if k % 2 else (int(rng.integers(2, 40)), int(rng.integers(2, 40)))
        hwc = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        if k % 4 == 1:
            hwc = ((hwc >> 6) * 85).astype(np.uint8)
        want = np.asarray(Image.fromarray(hwc).filter(ImageFilter.GaussianBlur(radius=r))).transpose(2, 0, 1)
        ww, fw = mc.blur_weights(r)
        assert np.array_equal(mc.blur_ref(np.ascontiguousarray(hwc.transpose(2, 0, 1)), ww, fw), want), (k, r, H, W)
    assert len(radii) >= 200
    for r in (0.1, 0.5, 1.0):
        ww, fw = mc.blur_weights(r)
        assert 0 < fw < ww <= 1 << 24 and (1 << 24) - 1 <= ww + 2 * fw <= 1 << 24
        const = np.full((3, 7, 9), 201, dtype=np.uint8)
        assert np.array_equal(mc.blur_ref(const, ww, fw), const)
    assert mc.blur_weights(1.0) == (11184811, 2796202)           # a = 1/4: 2^24 / 1.5 = 11184810.67 rounds to an fp32 integer first


def test_gray_and_flips_equal_pillow():
    Image, _, ImageOps = _pil()
    rng = np.random.default_rng(73)
    for S in (16, 10, 23):
        hwc = rng.integers(0, 256, size=(S, S, 3), dtype=np.uint8)
        im, chw = Image.fromarray(hwc), np.ascontiguousarray(hwc.transpose(2, 0, 1))
        lum = np.asarray(im.convert('L'))
        assert np.array_equal(mc.gray_ref(chw), np.stack([lum] * 3))
        assert np.array_equal(mc.gray_ref(chw), np.asarray(im.convert('L').convert('RGB')).transpose(2, 0, 1))
        tables, none = mc.box_tables((0, 0, S, S), S), [[0, 0, 0, 0]] * 16
        for flags, pil in ((mc.HFLIP, ImageOps.mirror(im)), (mc.VFLIP, ImageOps.flip(im)), (mc.HFLIP | mc.VFLIP, ImageOps.flip(ImageOps.mirror(im)))):
            got = mc.geometry_ref(hwc, flags, (0, 0), *tables, none, 0, S)
            assert np.array_equal(got, np.asarray(pil).transpose(2, 0, 1)), flags


def test_full_chain_equals_the_pillow_calls():
    """feed_ref on plan-drawn samples against RandomCrop's pad + crop, crop().resize(), numpy hole filling, the flips, the jitter's
    Pillow calls (tests/test_hisfrag_feed.py pins jitter_ref itself), GaussianBlur and convert('L'), in the reference's order."""
    Image, ImageFilter, ImageOps = _pil()
    from PIL import ImageEnhance
    S = 32
    sizes = ((70, 90), (20, 45), (32, 32), (40, 25))
    images, plan = mc.plan_drawn_batch(S, sizes, seed=74, rows=8)
    got = mc.feed_ref(images, plan, S)
    rng = np.random.default_rng(74 + S)                          # the radii are not in the plan: redraw them as plan_drawn_batch did
    [rng.integers(1, 255, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
    seen = 0
    for k in range(8):
        u = rng.random(mc.PLAN_COLUMNS).astype(np.float32)
        radius = float(u[102]) * (1.0 - 0.1) + 0.1
        img, f = images[int(plan['image'][k])], int(plan['flags'][k])
        H, W, _ = img.shape
        top, left = (int(t) for t in plan['origin'][k])
        big = np.full((H + 2 * S, W + 2 * S, 3), 255, dtype=np.uint8)
        big[S: S + H, S: S + W] = img
        im = Image.fromarray(big[S + top: 2 * S + top, S + left: 2 * S + left])
        i, j, h, w = (int(t) for t in plan['box'][k])
        arr = np.asarray(im.crop((j, i, j + w, i + h)).resize((S, S), Image.BILINEAR)).copy()
        if f & mc.DROPOUT:
            for x1, y1, x2, y2 in plan['holes'][k][: int(plan['n_holes'][k])]:
                arr[y1:y2, x1:x2] = 255
        im = Image.fromarray(arr)
        if f & mc.HFLIP:
            im = ImageOps.mirror(im)
        if f & mc.VFLIP:
            im = ImageOps.flip(im)
        if f & mc.JITTER:
            for op in plan['order'][k]:
                if op == 3:
                    hh, ss, vv = im.convert('HSV').split()
                    np_h = (np.asarray(hh).astype(np.int64) + int(plan['hue'][k])).astype(np.uint8)
                    im = Image.merge('HSV', (Image.fromarray(np_h, 'L'), ss, vv)).convert('RGB')
                else:
                    enh = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[int(op)]
                    im = enh(im).enhance(float(plan['factors'][k][int(op)]))
        if f & mc.BLUR:
            im = im.filter(ImageFilter.GaussianBlur(radius=radius))
        if f & mc.GRAY:
            im = im.convert('L').convert('RGB')
        assert np.array_equal(got[k], np.asarray(im).transpose(2, 0, 1)), (k, f)
        seen |= f
    assert seen == 63 and len({int(f) for f in plan['flags']}) >= 6


# ---------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------
S = 64
SIZES = [(64, 64), (50, 70), (300, 420), (30, 41), (65, 200), (1200, 900), (63, 64)]
ROWS = 4096


def _uniforms(rows=ROWS, seed=75):
    """Seeded uniforms with the edge rows in front: all 0, all just below 1, the thresholds from both sides, extreme crop draws on
    every image size, a row whose ten RandomResizedCrop attempts all fail and rows whose box is as wide / as high as the window."""
    u = torch.rand(rows, mc.PLAN_COLUMNS, generator=torch.Generator().manual_seed(seed))
    below = lambda t: float(np.nextafter(np.float32(t), np.float32(0))) if float(np.float32(t)) >= t else float(np.float32(t))
    u[0], u[1], u[2], u[3] = 0.0, below(1), 0.5, below(0.5)
    above = lambda t: float(np.float32(t)) if float(np.float32(t)) >= t else float(np.nextafter(np.float32(t), np.float32(1)))
    u[4, 24], u[4, 103], u[5, 24], u[5, 103] = above(0.9), above(0.2), below(0.9), below(0.2)      # the fp32 neighbours of 0.9 and 0.2
    for k in range(6, 6 + 2 * len(SIZES)):
        u[k, 0:2] = below(1) if k % 2 else 0.0
    u[20, 2:22:2], u[20, 3:22:2] = below(1), 0.0                 # area S^2, ratio 3/4: h = round(S / sqrt(3/4)) > S, ten times
    u[21, 2:22:2], u[21, 3:22:2] = below(1), 0.5                 # area just under S^2, ratio 1: w = h = S
    u[22, 2], u[22, 3], u[22, 4], u[22, 5] = below(1), below(1), 0.7, 0.9       # the first attempt fails, the second wins
    return u


def _bits(t):
    return np.asarray(t, dtype=np.float32).view(np.uint32).tolist()


def test_plan_equals_the_per_sample_draws(vited):
    u = _uniforms()
    sizes = torch.tensor(SIZES, dtype=torch.int32)
    image = torch.arange(ROWS) % len(SIZES)
    plan = vited.engine.michigan_augment_plan(u, image, sizes, S)
    assert vited.engine.MICHIGAN_PLAN_COLUMNS == mc.PLAN_COLUMNS == u.shape[1]
    i32, f32 = torch.int32, torch.float32
    assert [t.dtype for t in plan] == [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, f32, i32, i32]
    assert [tuple(t.shape[1:]) for t in plan] == [(), (), (2,), (4,), (S,), (S, 3), (S,), (S, 3), (16, 4), (), (4,), (3,), (), (2,)]
    assert all(t.shape[0] == ROWS and t.is_contiguous() for t in plan) and torch.equal(plan.image.long(), image)
    assert plan.flags[:4].tolist() == [63, 0, 1, 31]            # "u < p" throughout: 0.5 < 0.9 only, just under 0.5 is no grey
    assert int(plan.flags[4]) & 33 == 0 and int(plan.flags[5]) & 33 == 33
    fallbacks = full_side = late = 0
    for k in range(ROWS):
        H, W = SIZES[k % len(SIZES)]
        want = mc.plan_sample(u[k].tolist(), H, W, S)
        assert int(plan.flags[k]) == want['flags'] and tuple(plan.origin[k].tolist()) == want['origin'], k
        assert tuple(plan.box[k].tolist()) == want['box'], (k, plan.box[k].tolist(), want['box'])
        assert plan.x0[k].tolist() == want['x0'] and plan.kx[k].tolist() == want['kx'], k
        assert plan.y0[k].tolist() == want['y0'] and plan.ky[k].tolist() == want['ky'], k
        assert int(plan.n_holes[k]) == want['n_holes'] and plan.holes[k].tolist() == want['holes'], k
        assert plan.order[k].tolist() == want['order'] and int(plan.hue[k]) == want['hue'], k
        assert _bits(plan.factors[k]) == _bits(want['factors']) and plan.blur[k].tolist() == want['blur'], k
        i, j, h, w = want['box']
        assert 0 <= i <= S - h and 0 <= j <= S - w and 0 < h <= S and 0 < w <= S
        pad_y, pad_x = max(S - H, 0), max(S - W, 0)
        assert -pad_y <= want['origin'][0] <= H + pad_y - S and -pad_x <= want['origin'][1] <= W + pad_x - S
        for x1, y1, x2, y2 in want['holes'][: want['n_holes']]:
            assert 0 <= x1 < x2 <= S and 0 <= y1 < y2 <= S and 16 <= x2 - x1 <= 64 and 16 <= y2 - y1 <= 64
        fallbacks += want['failed'] == 10
        late += 0 < want['failed'] < 10
        full_side += (h == S or w == S) and want['failed'] < 10
    assert fallbacks >= 1 and full_side >= 1 and late >= 1, (fallbacks, full_side, late)
    assert mc.plan_sample(u[20].tolist(), 64, 64, S)['failed'] == 10 and tuple(plan.box[20].tolist()) == (0, 0, S, S)
    share = lambda bit: float(plan.flags.bitwise_and(bit).ne(0).float().mean())
    assert all(0.46 < share(b) < 0.54 for b in (mc.HFLIP, mc.VFLIP, mc.JITTER, mc.BLUR)) and 0.87 < share(mc.DROPOUT) < 0.93
    assert 0.17 < share(mc.GRAY) < 0.23
    on = plan.flags.bitwise_and(mc.DROPOUT) != 0
    assert int(plan.n_holes[on].min()) == 3 and int(plan.n_holes[on].max()) == 16 and not plan.n_holes[~on].any() and not plan.holes[~on].any()
    jit = plan.flags.bitwise_and(mc.JITTER) != 0
    assert {tuple(r) for r in plan.order[jit].tolist()} == set(mc.ORDERS)
    assert bool(((plan.hue[jit] <= 25) | (plan.hue[jit] >= 231)).all())                         # |hue| <= 0.1
    assert bool((plan.factors[~jit] == 1).all()) and not plan.hue[~jit].any() and bool((plan.order[~jit] == torch.arange(4)).all())
    fb = plan.factors[jit]
    as32 = lambda t: float(np.float32(t))                        # the factors are fp32: so are their bounds
    assert float(fb[:, 0].min()) >= as32(0.8) and float(fb[:, 0].max()) <= as32(1.2)
    assert float(fb[:, 1:].min()) >= as32(0.7) and float(fb[:, 1:].max()) <= as32(1.3)
    blurred = plan.flags.bitwise_and(mc.BLUR) != 0
    assert plan.blur[~blurred].tolist() == [list(mc.NO_BLUR)] * int((~blurred).sum())
    ww, fw = plan.blur[blurred].long().unbind(1)
    assert bool((fw == ((1 << 24) - ww) // 2).all()) and int(ww.min()) >= mc.blur_weights(1.0)[0] and int(ww.max()) <= mc.blur_weights(0.1)[0]


def test_plan_parameters(vited):
    E = vited.engine
    u = _uniforms(256)
    sizes = torch.tensor(SIZES, dtype=torch.int32)
    image = torch.arange(256) % len(SIZES)
    plan = E.michigan_augment_plan(u, image, sizes, 16, holes=(0, 5), hole_size=(1, 40), radius_max=0.5)
    for k in range(256):
        H, W = SIZES[k % len(SIZES)]
        want = mc.plan_sample(u[k].tolist(), H, W, 16, holes=(0, 5), hole_size=(1, 40), radius_max=0.5)
        assert int(plan.n_holes[k]) == want['n_holes'] and plan.holes[k].tolist() == want['holes'] and plan.blur[k].tolist() == want['blur'], k
        assert all(0 <= x1 < x2 <= 16 and 0 <= y1 < y2 <= 16 for x1, y1, x2, y2 in want['holes'][: want['n_holes']])     # clamped to S
    with pytest.raises(ValueError, match='radius_max'):
        E.michigan_augment_plan(u, image, sizes, 16, radius_max=1.5)
    with pytest.raises(ValueError, match='holes'):
        E.michigan_augment_plan(u, image, sizes, 16, holes=(3, 17))
    # out-of-range image indices are clamped like the kernel clamps them
    far = E.michigan_augment_plan(u[:2], torch.tensor([-3, 99]), sizes, 16)
    near = E.michigan_augment_plan(u[:2], torch.tensor([0, len(SIZES) - 1]), sizes, 16)
    assert torch.equal(far.origin, near.origin) and far.image.tolist() == [-3, 99]


def test_plan_without_augmentation(vited):
    u = _uniforms(64)
    sizes = torch.tensor(SIZES, dtype=torch.int32)
    image = torch.arange(64) % len(SIZES)
    for size in (S, 33, 10):
        plan = vited.engine.michigan_augment_plan(u, image, sizes, size, train=False)
        assert not plan.flags.any() and bool((plan.factors == 1).all()) and not plan.hue.any() and not plan.n_holes.any()
        assert plan.blur.tolist() == [list(mc.NO_BLUR)] * 64 and not plan.holes.any()
        x0, kx, y0, ky = mc.eval_tables(size)
        for k in range(64):
            H, W = SIZES[k % len(SIZES)]
            want = mc.plan_sample(None, H, W, size, train=False)
            assert tuple(plan.origin[k].tolist()) == want['origin'] == (mc.centre_origin(H, size), mc.centre_origin(W, size))
            assert plan.x0[k].tolist() == x0 and plan.kx[k].tolist() == kx and plan.y0[k].tolist() == y0 and plan.ky[k].tolist() == ky
    # PadCenterCrop pads both sides by the whole deficit: an odd deficit lands elsewhere than torchvision's own centre padding
    assert [mc.centre_origin(w, 64) for w in (64, 65, 67, 63, 61, 50, 30)] == [0, 0, 2, -1, -1, -7, -17]
    assert math.floor(-(64 - 61) / 2) == -2                      # section 17's eval origin for the same image


# ---------------------------------------------------------------------------------------------
# the case tables and the loader's bookkeeping
# ---------------------------------------------------------------------------------------------
def test_case_table_shares():
    images = mc.case_images()
    table, names = mc.case_table(images)
    assert len(names) == len(set(names)) and sorted({int(k) for k in table['image']}) == list(range(6))
    want, touch = mc.case_refs(images, table)
    n = len(names)
    assert 3 * sum(touch) >= n and 3 * (n - sum(touch)) >= n, (sum(touch), n)
    assert (want[names.index('all-pad/image2')] == 255).all() and not touch[names.index('identity/image3')]
    a, b = want[names.index('holes-sixteen/image4')], want[names.index('holes-unflagged/image4')]
    assert (a != b).any() and (a[:, 0, 0] == 255).all() and (a[:, 15, 15] == 255).all()


def test_loader_is_the_hisfrag_sampler(vited):
    labels, images = mc.toy_writers()
    E = vited.engine
    store = E.Div2kImageStore(images, 'cpu')
    loader = E.MichiganDeviceLoader(store, labels, 9, 16, m=3, repeat=4, seed=3)
    other = E.HisfragDeviceLoader(store, labels, 9, 16, m=3, repeat=4, seed=3)
    assert len(loader) == len(other) == 31 * 4 // 9 and torch.equal(loader.rank_indices(), other.rank_indices())
    loader.set_epoch(1)
    assert not torch.equal(loader.rank_indices(), other.rank_indices())
    plan = loader.plan(loader.rank_indices()[0], loader._generator(1))
    assert isinstance(plan, E.MichiganPlan) and plan.x0.shape == (9, 16) and plan.holes.shape == (9, 16, 4)
    with pytest.raises(ValueError, match='multiple of m'):
        E.MichiganDeviceLoader(store, labels, 8, 16, m=3)


def test_ops_refuse_cpu_tensors(vited):
    labels, images = mc.toy_writers()
    store = vited.engine.Div2kImageStore(images, 'cpu')
    p = vited.engine.michigan_augment_plan(torch.rand(3, mc.PLAN_COLUMNS), torch.arange(3), store.sizes, 16)
    with pytest.raises(RuntimeError, match='CPU tensor'):
        vited.ops.michigan_windows_u8(store.data, store.offsets, store.sizes, p.image, p.flags, p.origin, p.x0, p.kx, p.y0, p.ky, p.holes,
                                      p.n_holes, 16)
    with pytest.raises(RuntimeError, match='CPU tensor'):
        vited.ops.michigan_blur_gray_u8(torch.zeros(3, 3, 16, 16, dtype=torch.uint8), p.flags, p.blur)
