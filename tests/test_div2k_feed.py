"""The DIV2K device feed without a GPU: the batch-level augmentation plan against the per-sample restatement of
the reference's draws (data/datasets/div2k_patch.py:89-111), the numpy restatement of the per-pixel definition against slices that
need no package to state, and the loader's bookkeeping on a CPU store.  The kernel itself: tests/test_gpu_div2k_feed.py."""
import numpy as np
import pytest
import torch

import div2k_feed_cases as fc

S = 64
SIZES = [(128, 192), (129, 193), (1356, 2040), (2040, 1356), (300, 420), (128, 500), (477, 192)]     # the first is exactly 2 S x 3 S


def _uniforms(rows=4096, seed=21):
    """Seeded uniforms with the edge rows in front: all 0, all just below 1, the p = 0.5 thresholds from both sides."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(rows, 13, generator=g)
    below_one, below_half = float(np.nextafter(np.float32(1), np.float32(0))), float(np.nextafter(np.float32(0.5), np.float32(0)))
    u[0] = 0.0
    u[1] = below_one
    u[2] = 0.5                  # p = 0.5 means "u < 0.5": exactly 0.5 switches everything off
    u[3] = below_half
    for k in range(4, 4 + len(SIZES) * 2):                      # extreme crop draws on every image size, warp on and off
        u[k, 11:] = below_one if k % 2 else 0.0
    return u


def test_plan_equals_the_per_sample_draws(vited):
    u = _uniforms()
    sizes = torch.tensor(SIZES, dtype=torch.int32)
    image = torch.arange(u.shape[0]) % len(SIZES)
    idx, flags, minv, rgb, crop = vited.engine.div2k_augment_plan(u, image, sizes, S)
    assert (idx.dtype, flags.dtype, minv.dtype, rgb.dtype, crop.dtype) == (torch.int32, torch.int32, torch.float64, torch.float32, torch.int32)
    assert minv.shape == (4096, 6) and rgb.shape == (4096, 3) and crop.shape == (4096, 2) and torch.equal(idx.long(), image)
    assert int(flags[0]) == 15 and int(flags[1]) == 0 and int(flags[2]) == 0 and int(flags[3]) == 15
    worst = worst_id = 0.0
    for k in range(u.shape[0]):
        H, W = SIZES[k % len(SIZES)]
        f, M, inv, shifts, origin = fc.plan_sample(u[k].tolist(), H, W, S)
        assert int(flags[k]) == f and tuple(crop[k].tolist()) == origin, k
        assert rgb[k].tolist() == shifts, k                      # fp64 arithmetic rounded to fp32 once, on both sides
        # sin / cos of the two sides may differ in the last place (2.2e-16 relative); the translation terms multiply them by
        # at most max(H, W) = 2040 and the inversion by 1 / 0.85^2: a few 1e-12 absolute at the most, 1e-10 allows for that
        got = minv[k].numpy()
        worst = max(worst, float(np.abs(got - np.array(inv)).max()))
        if M is not None:                                        # minv . M is the identity (2 x 3 maps composed)
            a, b = np.vstack([got.reshape(2, 3), [0, 0, 1]]), np.vstack([np.array(M).reshape(2, 3), [0, 0, 1]])
            worst_id = max(worst_id, float(np.abs(a @ b - np.eye(3)).max()))
    print(f'plan vs per-sample minv: max |d| = {worst:.3e}; minv . M - I: max |d| = {worst_id:.3e}')
    assert worst < 1e-10, worst
    assert worst_id < 1e-12, worst_id
    on = flags.view(-1, 1).bitwise_and(torch.tensor([1, 2, 4, 8])).ne(0).float().mean(0)
    assert bool(((on > 0.46) & (on < 0.54)).all()), on           # p = 0.5 each
    ident = torch.tensor(fc.IDENTITY, dtype=torch.float64)
    assert bool((minv[flags.bitwise_and(4) == 0] == ident).all()) and bool((rgb[flags.bitwise_and(8) == 0] == 0).all())


def test_plan_without_augmentation_is_the_centre_crop(vited):
    u = _uniforms(64)
    sizes = torch.tensor(SIZES, dtype=torch.int32)
    image = torch.arange(64) % len(SIZES)
    idx, flags, minv, rgb, crop = vited.engine.div2k_augment_plan(u, image, sizes, S, train=False)
    assert int(flags.abs().max()) == 0 and float(rgb.abs().max()) == 0.0
    assert bool((minv == torch.tensor(fc.IDENTITY, dtype=torch.float64)).all())
    for k in range(64):
        H, W = SIZES[k % len(SIZES)]
        assert tuple(crop[k].tolist()) == fc.plan_sample(None, H, W, S, train=False)[4], k
    # torchvision's int(round(.)) rounds half to even: 129 - 128 = 1 -> 0.5 -> 0, 477 - 128 = 349 -> 174.5 -> 174, 193 - 192 -> 0
    assert crop[1].tolist() == [0, 0] and crop[6].tolist() == [174, 0] and crop[4].tolist() == [86, 114]
    assert [fc.round_half_even(v) for v in (0.5, 1.5, 2.5, 174.5, 3.0, 2.49)] == [0, 2, 2, 174, 3, 2]


def test_crop_origins_stay_inside(vited):
    g = torch.Generator().manual_seed(4)
    u = torch.rand(4096, 13, generator=g)
    u[:512, 11:] = float(np.nextafter(np.float32(1), np.float32(0)))
    u[512:1024, 11:] = 0.0
    sizes = torch.tensor(SIZES, dtype=torch.int32)
    image = torch.arange(4096) % len(SIZES)
    for train in (True, False):
        crop = vited.engine.div2k_augment_plan(u, image, sizes, S, train=train)[4].long()
        room = sizes[image].long() - torch.tensor([2 * S, 3 * S])
        assert bool((crop >= 0).all()) and bool((crop <= room).all())
        assert bool((crop[image == 0] == 0).all())                # an image of exactly 2 S x 3 S has one window
    crop = vited.engine.div2k_augment_plan(u, image, sizes, S)[4].long()
    big = image == 2
    assert int(crop[big][:, 0].max()) == 1356 - 128 and int(crop[big][:, 1].max()) == 2040 - 192 and int(crop[big].min()) == 0


# ---------------------------------------------------------------------------------------------
# the restatement against what can be stated without it
# ---------------------------------------------------------------------------------------------
def _img(h=40, w=60, seed=1):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _planar(a):
    return np.ascontiguousarray(a.transpose(2, 0, 1))


def test_restatement_plain_and_flipped_slices():
    img, s = _img(), 8
    top, left = 5, 9
    win = (slice(top, top + 16), slice(left, left + 24))
    assert np.array_equal(fc.region_ref(img, 0, fc.IDENTITY, (0, 0, 0), top, left, s), _planar(img[win]))
    assert np.array_equal(fc.region_ref(img, fc.HFLIP, fc.IDENTITY, (0, 0, 0), top, left, s), _planar(img[:, ::-1][win]))
    assert np.array_equal(fc.region_ref(img, fc.VFLIP, fc.IDENTITY, (0, 0, 0), top, left, s), _planar(img[::-1][win]))
    assert np.array_equal(fc.region_ref(img, fc.HFLIP | fc.VFLIP, fc.IDENTITY, (0, 0, 0), top, left, s), _planar(img[::-1, ::-1][win]))
    # the identity map through the warp path: a = b = 0 reproduces the tap exactly, flipped or not
    assert np.array_equal(fc.region_ref(img, fc.WARP, fc.IDENTITY, (0, 0, 0), top, left, s), _planar(img[win]))
    assert np.array_equal(fc.region_ref(img, fc.WARP | fc.HFLIP, fc.IDENTITY, (0, 0, 0), top, left, s), _planar(img[:, ::-1][win]))


def test_restatement_integer_translation_reflects_101():
    img, s = _img(20, 30), 8
    H, W = 20, 30
    tx, ty = -5, 7                                                # source = destination + (tx, ty): off the left and the bottom edge
    ref101 = lambda i, n: i if 0 <= i < n else (-i if i < 0 else 2 * (n - 1) - i)
    for flags, flipped in ((fc.WARP, img), (fc.WARP | fc.VFLIP, img[::-1])):
        got, touch = fc.region_ref(img, flags, (1, 0, tx, 0, 1, ty), (0, 0, 0), 2, 3, s, want_touch=True)
        want = np.empty((16, 24, 3), dtype=np.uint8)
        for y in range(16):
            for x in range(24):
                want[y, x] = flipped[ref101(y + 2 + ty, H), ref101(x + 3 + tx, W)]
        assert touch and np.array_equal(got, _planar(want))
    assert fc.reflect101([-3, -1, 0, 4, 5, 6, 9, 13], 5).tolist() == [3, 1, 0, 4, 3, 2, 1, 3]      # further than one period: until in range
    assert fc.reflect101([-2, 7], 1).tolist() == [0, 0]


def test_restatement_weights_and_rounding():
    # a half-pixel shift in x: a = 16, b = 0 -> (p0 + p1 + 1) >> 1 after the 15-bit rounding; the weights sum to 32768
    img = _img(20, 30, seed=2)
    got = fc.region_ref(img, fc.WARP, (1, 0, 0.5, 0, 1, 0), (0, 0, 0), 1, 2, 8)
    p = img.astype(np.int64)
    want = (16 * 32 * 32 * p[1:17, 2:26] + 16 * 32 * 32 * p[1:17, 3:27] + 16384) >> 15
    assert np.array_equal(got, _planar(want.astype(np.uint8)))
    for a in range(32):
        for b in range(32):
            assert (32 - a) * (32 - b) * 32 + a * (32 - b) * 32 + (32 - a) * b * 32 + a * b * 32 == 32768
    # rint is round half to even on the 1/1024 grid, and the two terms of a coordinate round separately
    assert fc.fixed1024([0.5 / 1024, 1.5 / 1024, 2.5 / 1024, -0.5 / 1024, -1.5 / 1024, 3e9, -3e9]).tolist() == [0, 2, 2, 0, -2, 2 ** 31 - 1, -2 ** 31]


def test_restatement_colour_shift_saturates():
    img = np.zeros((16, 24, 3), dtype=np.uint8)
    img[..., 0], img[..., 1], img[..., 2] = 250, 5, 100
    got = fc.region_ref(img, fc.COLOUR, fc.IDENTITY, (15.0, -15.0, -0.5), 0, 0, 8)
    assert set(got[0].ravel()) == {255} and set(got[1].ravel()) == {0} and set(got[2].ravel()) == {99}     # floor(99.5)
    got = fc.region_ref(img, fc.COLOUR, fc.IDENTITY, (4.75, 14.25, 0.0), 0, 0, 8)
    assert set(got[0].ravel()) == {254} and set(got[1].ravel()) == {19} and set(got[2].ravel()) == {100}
    assert np.array_equal(fc.region_ref(img, 0, fc.IDENTITY, (15.0, -15.0, 9.0), 0, 0, 8), _planar(img))      # bit 3 clear: no shift


def test_case_table_reaches_the_border():
    images = fc.case_images()
    table, names = fc.case_table(images)
    assert [im.shape[:2] for im in images[:5]] == list(fc.CASE_SIZES) and len(names) == len(set(names)) >= 96
    touch = [fc.region_ref(images[table['image'][k]], int(table['flags'][k]), table['minv'][k], table['rgb'][k], *table['crop'][k],
                           fc.CASE_S, want_touch=True)[1] for k in range(len(names))]
    assert sum(touch) * 3 >= len(names), (sum(touch), len(names))        # the reflected path cannot go untested
    assert len(names) - sum(touch) >= 24                                  # nor the unreflected one
    for k in range(len(images)):
        kinds = {n.split('/')[0] for n in names if n.endswith(f'/image{k}')}
        assert kinds >= {'identity', 'hflip', 'vflip', 'both-flips', 'translate', 'rot90', 'rot180', 'extreme0', 'extreme3', 'corner0',
                         'corner3', 'colour-up', 'colour-down', 'random0', 'random1'}, k


def test_entry_point_rejects_bad_arguments(vited):
    """Host-side checks only: every call returns before a launch (the pointers are never read), so no GPU is needed."""
    fn = vited._lib.load().vited_div2k_regions_u8
    p = 4096                                                     # any non-null value
    good = [p, p, p, 3, p, p, p, p, p, p, 8, 64, None]
    assert vited._lib.SIGNATURES['vited_div2k_regions_u8'][1][10:12] == [__import__('ctypes').c_int64, __import__('ctypes').c_int]
    for k in (0, 1, 2, 4, 5, 6, 7, 8, 9):                        # each pointer null in turn
        assert fn(*[None if i == k else v for i, v in enumerate(good)]) == 1, k
    for k, v in ((10, 0), (10, -1), (10, 65536), (11, 0), (11, -64), (3, 0)):      # batch outside 1..65535, img_size <= 0, no image
        assert fn(*[v if i == k else w for i, w in enumerate(good)]) == 1, (k, v)
    with pytest.raises(RuntimeError, match=r'vited_div2k_regions_u8 failed: .+ \(vited error 1\)'):
        vited._lib.call('vited_div2k_regions_u8', *[0 if i == 10 else w for i, w in enumerate(good)])


# ---------------------------------------------------------------------------------------------
# store and loader bookkeeping (CPU tensors; the kernel call refuses them)
# ---------------------------------------------------------------------------------------------
def _store(vited, n=12, h=20, w=30):
    rng = np.random.default_rng(3)
    return vited.engine.Div2kImageStore([rng.integers(0, 256, size=(h + k, w + 2 * k, 3), dtype=np.uint8) for k in range(n)], 'cpu')


def test_store_packs_images_and_rejects_small_ones(vited):
    store = _store(vited)
    assert len(store) == 12 and store.sizes.dtype == torch.int32 and store.sizes[3].tolist() == [23, 36]
    assert store.offsets.dtype == torch.int64 and store.offsets[1].item() == 20 * 30 * 3 and store.data.numel() == sum(
        (20 + k) * (30 + 2 * k) * 3 for k in range(12))
    rng = np.random.default_rng(3)
    first = rng.integers(0, 256, size=(20, 30, 3), dtype=np.uint8)
    assert np.array_equal(store.data[: first.size].numpy().reshape(20, 30, 3), first)
    assert torch.equal(store.sizes_dev, store.sizes) and torch.equal(store.offsets_dev, store.offsets)
    vited.engine.Div2kDeviceLoader(store, 4, 8, 0.07)                      # 16 x 24 windows fit
    with pytest.raises(ValueError, match='smaller than the 32 x 48 crop window'):
        vited.engine.Div2kDeviceLoader(store, 4, 16, 0.07)
    with pytest.raises(ValueError, match=r'uint8 \[H, W, 3\]'):
        vited.engine.Div2kImageStore([np.zeros((4, 4), dtype=np.uint8)], 'cpu')
    with pytest.raises(RuntimeError, match='CPU tensor'):                  # no CPU fallback behind the loader
        next(iter(vited.engine.Div2kDeviceLoader(store, 4, 8, 0.07)))


def test_loader_epochs_shards_and_seeds(vited):
    store = _store(vited)
    E = vited.engine
    one = E.Div2kDeviceLoader(store, 8, 8, 0.07, repeat=5, seed=3)
    assert len(one) == 12 * 5 // 8 == 7 and one.rank_indices().shape == (7, 8)
    order = one.epoch_order()
    assert sorted(order.tolist()) == sorted(list(range(12)) * 5)          # every image `repeat` times
    assert torch.equal(one.rank_indices().flatten(), order[:56])          # the last incomplete batch is dropped
    shards = [E.Div2kDeviceLoader(store, 4, 8, 0.07, repeat=5, rank=r, world=3, seed=3) for r in range(3)]
    assert [len(s) for s in shards] == [5, 5, 5]
    for r, s in enumerate(shards):
        assert torch.equal(s.epoch_order(), order)                        # one permutation, the same on every rank
        assert torch.equal(s.rank_indices().flatten(), order[r::3][:20])  # disjoint positions of it; together all 60
    assert torch.equal(torch.stack([s.rank_indices().flatten() for s in shards], dim=1).flatten(), order)
    one.set_epoch(1)
    assert not torch.equal(one.epoch_order(), order) and sorted(one.epoch_order().tolist()) == sorted(order.tolist())
    one.set_epoch(0)
    assert torch.equal(one.epoch_order(), order)
    other = E.Div2kDeviceLoader(store, 8, 8, 0.07, repeat=5, seed=4)
    assert not torch.equal(other.epoch_order(), order)
    # the same seed gives the same plan, another rank or epoch another one
    def plans(loader):
        g = loader._generator(1 + loader.rank)
        return [loader.plan(image, g) for image in loader.rank_indices()[:2]]
    again = E.Div2kDeviceLoader(store, 8, 8, 0.07, repeat=5, seed=3)
    for (aug_a, pair_a), (aug_b, pair_b) in zip(plans(one), plans(again)):
        assert all(torch.equal(x, y) for x, y in zip(aug_a + pair_a, aug_b + pair_b))
    assert not torch.equal(plans(one)[0][0][2], plans(other)[0][0][2])
    (idx, flags, minv, rgb, crop), (cells, labels, erode) = plans(one)[0]
    assert torch.equal(idx.long(), one.rank_indices()[0]) and labels.shape == (8, 4) and cells.shape == (8, 2) and erode.shape == (8,)
    with pytest.raises(ValueError, match='do not fill one batch'):
        E.Div2kDeviceLoader(store, 64, 8, 0.07, repeat=5)
    with pytest.raises(ValueError, match='rank 3'):
        E.Div2kDeviceLoader(store, 4, 8, 0.07, rank=3, world=3)
