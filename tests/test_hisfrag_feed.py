"""The HisFrag device feed without a GPU: the numpy restatement of the per-pixel definition
(tests/hisfrag_feed_cases.py) against Pillow itself and against slices that need no package to state, the batch-level plan against a
per-sample restatement of the reference's draws (hisfrag.py:66-78), and the sampler's bookkeeping on a CPU store.  The kernels
themselves: tests/test_gpu_hisfrag_feed.py."""
import numpy as np
import pytest
import torch

import hisfrag_feed_cases as fc


def _pil():
    pytest.importorskip('PIL')
    from PIL import Image, ImageEnhance
    return Image, ImageEnhance


# ---------------------------------------------------------------------------------------------
# the Pillow-defined pieces, against Pillow
# ---------------------------------------------------------------------------------------------
def test_affine_stage_equals_pillow_nearest_transform():
    Image, _ = _pil()
    rng = np.random.default_rng(61)
    extremes = [(5.0, 0.1, 0.1), (-5.0, -0.1, -0.1), (5.0, -0.1, 0.1), (-5.0, 0.1, -0.1)]
    n = 0
    for k in range(44):
        H, W = (int(t) for t in rng.integers(20, 91, size=2))
        img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        draws = [(rng.uniform(-5, 5), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)) for _ in range(3)] + [extremes[k % 4]]
        for angle, fx, fy in draws:
            M = fc.inverse_affine_matrix(W, H, angle, fc.round_half_even(fx * W), fc.round_half_even(fy * H))
            want = np.asarray(Image.fromarray(img).transform((W, H), Image.AFFINE, M, Image.NEAREST, fillcolor=0))
            assert np.array_equal(fc.affine_ref(img, fc.affine_fixed(M)), want), (k, H, W, angle, fx, fy)
            n += 1
    assert n >= 160


def _factors():
    return [0.7, 1.0, 1.3] + [float(t) for t in np.random.default_rng(62).uniform(0.7, 1.3, 30)]


def test_pointwise_colour_equals_pillow():
    Image, ImageEnhance = _pil()
    rng = np.random.default_rng(63)
    for k, f in enumerate(_factors()):
        S = (16, 10, 23)[k % 3]
        hwc = rng.integers(0, 256, size=(S, S, 3), dtype=np.uint8)
        if k % 5 == 0:
            hwc = np.ascontiguousarray(fc.half_mean_image(S).transpose(1, 2, 0))
        im, chw = Image.fromarray(hwc), hwc.transpose(2, 0, 1).astype(np.int64)
        assert np.array_equal(fc.luma(chw), np.asarray(im.convert('L')))
        pil = lambda enh: np.asarray(enh(im).enhance(f)).transpose(2, 0, 1)
        assert np.array_equal(fc.blend(np.zeros_like(chw), chw, f), pil(ImageEnhance.Brightness)), f
        assert np.array_equal(fc.blend(np.broadcast_to(fc.luma(chw)[None], chw.shape), chw, f), pil(ImageEnhance.Color)), f
        mean = fc.contrast_mean(chw)
        assert mean == int(np.asarray(ImageEnhance.Contrast(im).degenerate)[0, 0, 0])
        assert np.array_equal(fc.blend(np.full_like(chw, mean), chw, f), pil(ImageEnhance.Contrast)), f
    half = fc.half_mean_image(16).astype(np.int64)
    assert int(fc.luma(half).sum()) * 2 == 201 * 256 and fc.contrast_mean(half) == 101          # the mean is 100.5: it rounds up


def _all_triples():
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=1).astype(np.uint8).reshape(4096, 4096, 3)


def test_hsv_conversions_equal_pillow_on_all_inputs():
    Image, _ = _pil()
    cube = _all_triples()
    want = np.asarray(Image.fromarray(cube).convert('HSV')).astype(np.int64)
    h, s, v = fc.rgb_to_hsv(cube[..., 0], cube[..., 1], cube[..., 2])
    assert int((np.stack([h, s, v], axis=-1) != want).any(axis=-1).sum()) == 0
    want = np.asarray(Image.frombytes('HSV', (4096, 4096), cube.tobytes()).convert('RGB')).astype(np.int64)
    r, g, b = fc.hsv_to_rgb(cube[..., 0], cube[..., 1], cube[..., 2])
    assert int((np.stack([r, g, b], axis=-1) != want).any(axis=-1).sum()) == 0


def _pil_hue(Image, im, shift):
    h, s, v = im.convert('HSV').split()
    np_h = (np.asarray(h).astype(np.int64) + shift).astype(np.uint8)          # uint8 addition with wrap-around
    return Image.merge('HSV', (Image.fromarray(np_h, 'L'), s, v)).convert('RGB')


def test_hue_shift_equals_the_pillow_round_trip():
    Image, _ = _pil()
    hwc = np.random.default_rng(64).integers(0, 256, size=(48, 40, 3), dtype=np.uint8)
    for shift in (0, 1, 76, 180, 255):
        h, s, v = fc.rgb_to_hsv(hwc[..., 0], hwc[..., 1], hwc[..., 2])
        got = np.stack(fc.hsv_to_rgb((h + shift) & 255, s, v), axis=-1)
        assert np.array_equal(got, np.asarray(_pil_hue(Image, Image.fromarray(hwc), shift))), shift
    assert [fc.hue_shift_of(t) for t in (0.3, -0.3, 0.0, -0.001, 0.004, -0.004)] == [76, 180, 0, 0, 1, 255]


def test_jitter_chain_equals_pillow_in_all_24_orders():
    Image, ImageEnhance = _pil()
    rng = np.random.default_rng(65)
    assert len(fc.ORDERS) == 24 and len(set(fc.ORDERS)) == 24
    for k, order in enumerate(fc.ORDERS):
        hwc = rng.integers(0, 256, size=(16, 16, 3), dtype=np.uint8)
        factors = [np.float32(t) for t in ((0.7, 1.3, 0.7), (1.3, 0.7, 1.3), tuple(rng.uniform(0.7, 1.3, 3)))[k % 3]]
        shift = (76, 180, int(rng.integers(0, 256)))[k % 3]
        im = Image.fromarray(hwc)
        for op in order:
            if op == fc.HUE:
                im = _pil_hue(Image, im, shift)
            else:
                enh = {fc.BRIGHTNESS: ImageEnhance.Brightness, fc.CONTRAST: ImageEnhance.Contrast, fc.SATURATION: ImageEnhance.Color}[op]
                im = enh(im).enhance(float(factors[op]))
        got = fc.jitter_ref(np.ascontiguousarray(hwc.transpose(2, 0, 1)), order, factors, shift)
        assert np.array_equal(got, np.asarray(im).transpose(2, 0, 1)), order


# ---------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------
S = 64
SIZES = [(64, 64), (50, 70), (300, 420), (30, 41), (65, 200), (1200, 900), (63, 64)]


def _uniforms(rows=4096, seed=66):
    """Seeded uniforms with the edge rows in front: all 0, all just below 1, the p = 0.5 thresholds from both sides."""
    u = torch.rand(rows, fc.PLAN_COLUMNS, generator=torch.Generator().manual_seed(seed))
    below_one, below_half = float(np.nextafter(np.float32(1), np.float32(0))), float(np.nextafter(np.float32(0.5), np.float32(0)))
    u[0], u[1], u[2], u[3] = 0.0, below_one, 0.5, below_half
    for k in range(4, 4 + 2 * len(SIZES)):                      # extreme crop draws on every image size
        u[k, 8:10] = below_one if k % 2 else 0.0
    return u


def _bits(t):
    return np.asarray(t, dtype=np.float32).view(np.uint32).tolist()


def test_plan_equals_the_per_sample_draws(vited):
    u = _uniforms()
    sizes = torch.tensor(SIZES, dtype=torch.int32)
    image = torch.arange(u.shape[0]) % len(SIZES)
    plan = vited.engine.hisfrag_augment_plan(u, image, sizes, S)
    assert [t.dtype for t in plan] == [torch.int32, torch.int32, torch.int64, torch.float64, torch.int32, torch.int32, torch.float32,
                                       torch.int32, torch.float32]
    assert [tuple(t.shape[1:]) for t in plan] == [(), (), (6,), (6,), (2,), (4,), (3,), (), (2,)] and all(t.shape[0] == 4096 for t in plan)
    assert torch.equal(plan.image.long(), image) and all(t.is_contiguous() for t in plan)
    assert plan.flags[:4].tolist() == [15, 1, 1, 15]            # p = 0.5 means "u < 0.5"; RandomAffine is unconditional
    worst = 0.0
    for k in range(u.shape[0]):
        H, W = SIZES[k % len(SIZES)]
        want = fc.plan_sample(u[k].tolist(), H, W, S)
        assert int(plan.flags[k]) == want['flags'] and tuple(plan.origin[k].tolist()) == want['origin'], k
        assert plan.order[k].tolist() == want['order'] and int(plan.hue[k]) == want['hue'], k
        assert plan.afix[k].tolist() == want['afix'], k
        assert _bits(plan.factors[k]) == _bits(want['factors']) and _bits(plan.blur[k]) == _bits(want['blur']), k
        # sin / cos of the two sides may differ in the last place; the translation terms multiply them by at most 1,200 and the
        # inversion by 1 / 0.9^2: a few 1e-13 absolute at the most (tests/test_div2k_feed.py has the same bound for 2,040 pixels)
        worst = max(worst, float(np.abs(plan.minv[k].numpy() - np.array(want['minv'])).max()))
        pad_y, pad_x = max(S - H, 0), max(S - W, 0)
        assert -pad_y <= want['origin'][0] <= H + pad_y - S and -pad_x <= want['origin'][1] <= W + pad_x - S
    print(f'plan vs per-sample minv: max |d| = {worst:.3e}')
    assert worst < 1e-10, worst
    on = plan.flags.view(-1, 1).bitwise_and(torch.tensor([2, 4, 8])).ne(0).float().mean(0)
    assert bool(((on > 0.46) & (on < 0.54)).all()), on           # p = 0.5 each
    perms = {tuple(r) for r in plan.order[plan.flags.bitwise_and(4) != 0].tolist()}
    assert perms == set(fc.ORDERS)                               # every order is drawn
    shifts = plan.hue[plan.flags.bitwise_and(4) != 0]
    assert bool(((shifts <= 76) | (shifts >= 180)).all()) and int(shifts.max()) == 255 and int(shifts.min()) == 0
    off = plan.flags.bitwise_and(4) == 0
    assert bool((plan.factors[off] == 1).all()) and bool((plan.hue[off] == 0).all()) and bool((plan.order[off] == torch.arange(4)).all())
    assert bool((plan.minv[plan.flags.bitwise_and(2) == 0] == torch.tensor(fc.IDENTITY, dtype=torch.float64)).all())
    assert bool((plan.blur[plan.flags.bitwise_and(8) == 0] == torch.tensor([0.0, 1.0])).all())
    k_edge, k_mid = plan.blur[plan.flags.bitwise_and(8) != 0].double().unbind(1)
    assert float((2 * k_edge + k_mid - 1).abs().max()) < 2e-7    # a normalised kernel, to fp32 rounding


def test_plan_without_augmentation_is_the_centre_crop(vited):
    u = _uniforms(64)
    sizes = torch.tensor(SIZES, dtype=torch.int32)
    image = torch.arange(64) % len(SIZES)
    plan = vited.engine.hisfrag_augment_plan(u, image, sizes, S, train=False)
    assert not plan.flags.any() and bool((plan.factors == 1).all()) and not plan.hue.any()
    assert plan.afix.tolist() == [list(fc.IDENTITY_FIX)] * 64 and plan.minv.tolist() == [list(fc.IDENTITY)] * 64
    want = {(64, 64): (0, 0), (50, 70): (-7, 3), (300, 420): (118, 178), (30, 41): (-17, -11), (65, 200): (0, 68), (1200, 900): (568, 418),
            (63, 64): (0, 0)}                                    # (65 - 64) / 2 = 0.5 rounds to 0; a 63-row image is padded below only
    for k in range(64):
        H, W = SIZES[k % len(SIZES)]
        assert tuple(plan.origin[k].tolist()) == want[(H, W)] == fc.plan_sample(None, H, W, S, train=False)['origin']
    assert fc.centre_origin(67, 64) == 2 and fc.centre_origin(61, 64) == -1                     # 1.5 rounds to even; 3 // 2 rows above


# ---------------------------------------------------------------------------------------------
# the geometry and blur restatements, against what can be stated without them
# ---------------------------------------------------------------------------------------------
def _padded_slice(img, top, left, S):
    H, W, _ = img.shape
    big = np.zeros((H + 2 * S + 8, W + 2 * S + 8, 3), dtype=np.uint8)
    big[S + 4: S + 4 + H, S + 4: S + 4 + W] = img
    return big[S + 4 + top: S + 4 + top + S, S + 4 + left: S + 4 + left + S].transpose(2, 0, 1)


def test_identity_windows_are_slices():
    images = fc.case_images()
    S = fc.CASE_S
    for img in images:
        H, W, _ = img.shape
        pad_y, pad_x = max(S - H, 0), max(S - W, 0)
        for top, left in ((-pad_y, -pad_x), (H + pad_y - S, W + pad_x - S), ((H - S) // 2, (W - S) // 2), (-S, 0), (H - 1, W - 1)):
            for flags, minv in ((0, fc.IDENTITY), (fc.WARP, fc.IDENTITY), (fc.AFFINE, fc.IDENTITY), (fc.AFFINE | fc.WARP, fc.IDENTITY)):
                got, touch = fc.window_ref(img, flags, fc.IDENTITY_FIX, minv, top, left, S, want_touch=True)
                assert np.array_equal(got, _padded_slice(img, top, left, S)), (img.shape, top, left, flags)
                # a warped identity still evaluates the taps one to the right and below, with weight 0
                inside = 0 <= top and top + S + bool(flags & fc.WARP) <= H and 0 <= left and left + S + bool(flags & fc.WARP) <= W
                assert touch == (not inside), (img.shape, top, left, flags)
    # integer translations through either stage move the slice; the vacated part is 0
    img = images[4]
    got = fc.window_ref(img, fc.AFFINE, fc.affine_fixed((1, 0, 3, 0, 1, -2)), fc.IDENTITY, 5, 7, S)
    assert np.array_equal(got, _padded_slice(img, 5 - 2, 7 + 3, S))
    got = fc.window_ref(img, fc.WARP, fc.IDENTITY_FIX, (1, 0, 3, 0, 1, -2), 0, 40, S)
    want = _padded_slice(img, -2, 43, S).copy()
    want[:, :, 48 - 40:] = 0                                     # the destination columns past the image are pad, not warped content
    assert np.array_equal(got, want)
    # half a pixel: the mean of two neighbours, rounded half up by the 15-bit scheme
    got = fc.window_ref(img, fc.WARP, fc.IDENTITY_FIX, (1, 0, 0.5, 0, 1, 0), 3, 4, S).astype(np.int64)
    a, b = _padded_slice(img, 3, 4, S).astype(np.int64), _padded_slice(img, 3, 5, S).astype(np.int64)
    assert np.array_equal(got, (a + b + 1) >> 1)


def test_case_table_shares():
    images = fc.case_images()
    table, names = fc.case_table(images)
    assert len(names) == len(set(names)) and sorted({int(k) for k in table['image']}) == list(range(6))
    touch = [fc.window_ref(images[int(table['image'][k])], int(table['flags'][k]), table['afix'][k], table['minv'][k],
                           int(table['origin'][k][0]), int(table['origin'][k][1]), fc.CASE_S, want_touch=True)[1] for k in range(len(names))]
    assert 3 * sum(touch) >= len(names) and 3 * (len(names) - sum(touch)) >= len(names), (sum(touch), len(names))


def test_blur_restatement():
    for S in (16, 10):
        for sigma in (1.0, 1.37, 2.0):
            ke, km = fc.blur_weights(sigma)
            const = np.full((3, S, S), 201, dtype=np.uint8)
            assert np.array_equal(fc.blur_ref(const, ke, km), const)
            imp = np.zeros((3, S, S), dtype=np.uint8)
            imp[:, 0, 0] = 200
            got = fc.blur_ref(imp, ke, km)
            # the corner itself is read once (the centre tap); (0, 1) sees it through its left tap, (1, 1) through the corner tap;
            # (1, 0) and (0, 1) mirror each other, and nothing reflects the corner back: index -1 maps to 1, not to 0
            f = lambda w: int(np.clip(np.rint(np.float32(0) + np.float32(w) * np.float32(200)), 0, 255))
            assert got[0, 0, 0] == f(km * km) and got[0, 0, 1] == got[0, 1, 0] == f(np.float32(km * ke)) and got[0, 1, 1] == f(ke * ke)
            assert not got[:, 2:, :].any() and not got[:, :, 2:].any()
            imp[:] = 0
            imp[:, 0, 1] = 200                                   # (0, 0) reads column 1 twice: as its right tap and, reflected, as its left
            got = fc.blur_ref(imp, ke, km)
            w = np.float32(km * ke)
            assert got[0, 0, 0] == int(np.rint((np.float32(0) + w * np.float32(200)) + w * np.float32(200)))
    assert [int(t) for t in np.rint(np.array([0.5, 1.5, 2.5], dtype=np.float32))] == [0, 2, 2]


# ---------------------------------------------------------------------------------------------
# the sampler, on a CPU store
# ---------------------------------------------------------------------------------------------
def _toy(vited, device):
    labels, images = fc.toy_writers()
    return vited.engine.Div2kImageStore(images, device), labels, images


def test_sampler_is_m_per_class(vited):
    store, labels, _ = _toy(vited, 'cpu')
    E = vited.engine
    loader = E.HisfragDeviceLoader(store, labels, 9, 16, m=3, repeat=4, seed=3)
    assert len(loader) == 31 * 4 // 9
    idx = loader.rank_indices()
    assert idx.shape == (13, 9) and idx.dtype == torch.int64 and int(idx.min()) >= 0 and int(idx.max()) < 31
    targets = torch.tensor(labels)[idx]
    runs = targets.view(13, 3, 3)
    assert bool((runs == runs[:, :, :1]).all())                  # m equal targets in a row ...
    for b in range(13):
        assert len(set(runs[b, :, 0].tolist())) == 3             # ... and, a pass being three whole batches, distinct writers per batch
    flat, tflat = idx.view(-1, 3), targets.view(-1, 3)[:, 0]
    for members, t in zip(flat.tolist(), tflat.tolist()):
        n = labels.count(t)
        assert len(set(members)) == min(n, 3)                    # no repetition where the writer has three; one repeat where it has two
        if n == 2:
            assert members[2] == members[0]                      # cycling: a, b, a
    for p in range(4):                                           # every pass visits every writer once
        assert sorted(tflat[9 * p: 9 * p + 9].tolist()) == sorted(set(labels))
    assert len({tuple(tflat[9 * p: 9 * p + 9].tolist()) for p in range(4)}) > 1
    seen = {k for row in flat.tolist() for k in row}
    assert len(seen) > 20                                        # the members are drawn, not always the first three
    assert torch.equal(idx, E.HisfragDeviceLoader(store, labels, 9, 16, m=3, repeat=4, seed=3).rank_indices())
    loader.set_epoch(1)
    assert not torch.equal(idx, loader.rank_indices())
    other = E.HisfragDeviceLoader(store, labels, 9, 16, m=3, repeat=4, seed=3, rank=1, world=2)
    assert len(other) == 31 * 4 // 2 // 9 and not torch.equal(other.rank_indices(), idx[: len(other)])
    with pytest.raises(ValueError, match='multiple of m'):
        E.HisfragDeviceLoader(store, labels, 8, 16, m=3)
    with pytest.raises(ValueError, match='labels'):
        E.HisfragDeviceLoader(store, labels[:-1], 9, 16)
    with pytest.raises(ValueError, match='do not fill'):
        E.HisfragDeviceLoader(store, labels, 33, 16)


def test_ops_refuse_cpu_tensors(vited):
    store, _, _ = _toy(vited, 'cpu')
    plan = vited.engine.hisfrag_augment_plan(torch.rand(3, fc.PLAN_COLUMNS), torch.arange(3), store.sizes, 16)
    with pytest.raises(RuntimeError, match='CPU tensor'):
        vited.ops.hisfrag_windows_u8(store.data, store.offsets, store.sizes, plan.image, plan.flags, plan.afix, plan.minv, plan.origin, 16)
    img = torch.zeros(3, 3, 16, 16, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='CPU tensor'):
        vited.ops.hisfrag_jitter_u8(img, plan.flags, plan.order, plan.factors, plan.hue)
    with pytest.raises(RuntimeError, match='CPU tensor'):
        vited.ops.hisfrag_blur_u8(img, plan.flags, plan.blur)
