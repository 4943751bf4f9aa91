"""The HisFrag device feed on the GPU: ``vited_hisfrag_windows_u8``, ``vited_hisfrag_jitter_u8`` and
``vited_hisfrag_blur_u8`` bit for bit against the numpy restatement of their per-pixel definition (tests/hisfrag_feed_cases.py, itself
checked against Pillow in tests/test_hisfrag_feed.py), the clamping of device-side arguments, and ``HisfragDeviceLoader`` feeding the
two-stage step.  Equality is exact everywhere: the definition is integer arithmetic on separately rounded fp64 terms and Pillow's
uncontracted fp32 blends."""
import numpy as np
import pytest
import torch

import hisfrag_feed_cases as fc
from oracle import vited_oracle as vo

pytestmark = pytest.mark.gpu

_DTYPES = {'image': torch.int32, 'flags': torch.int32, 'afix': torch.int64, 'minv': torch.float64, 'origin': torch.int32,
           'order': torch.int32, 'factors': torch.float32, 'hue': torch.int32, 'blur': torch.float32}


def _dev(plan, gpu):
    return {k: torch.as_tensor(np.asarray(v), dtype=_DTYPES[k]).to(gpu).contiguous() for k, v in plan.items()}


def _windows(vited, store, p, S, out=None):
    return vited.ops.hisfrag_windows_u8(store.data, store.offsets_dev, store.sizes_dev, p['image'], p['flags'], p['afix'], p['minv'],
                                        p['origin'], S, out=out)


def _colour_want(imgs, plan):
    return np.stack([fc.colour_ref(imgs[k], int(plan['flags'][k]), [int(t) for t in plan['order'][k]], plan['factors'][k], int(plan['hue'][k]),
                                   plan['blur'][k]) for k in range(len(imgs))])


def _differing(got, want, names=None):
    return [(names[k] if names else k, int((got[k] != want[k]).sum())) for k in range(len(want)) if not np.array_equal(got[k], want[k])]


class _Small:
    """The S = 16 store of the geometry case table, on the device and as numpy, with the table's reference windows (computed once)."""

    def __init__(self, vited, gpu):
        self.images = fc.case_images()
        self.store = vited.engine.Div2kImageStore(self.images, gpu)
        self.table, self.names = fc.case_table(self.images)
        tb = self.table
        refs = [fc.window_ref(self.images[int(tb['image'][k])], int(tb['flags'][k]), tb['afix'][k], tb['minv'][k], int(tb['origin'][k][0]),
                              int(tb['origin'][k][1]), fc.CASE_S, want_touch=True) for k in range(len(self.names))]
        self.want = np.stack([r[0] for r in refs])
        self.want.setflags(write=False)
        self.touch = [r[1] for r in refs]


@pytest.fixture(scope='module')
def small(vited, gpu):
    return _Small(vited, gpu)


def test_geometry_case_table_is_bit_exact(vited, gpu, small):
    n = len(small.names)
    assert 3 * sum(small.touch) >= n and 3 * (n - sum(small.touch)) >= n, (sum(small.touch), n)      # zero-filled taps / none
    got = _windows(vited, small.store, _dev(small.table, gpu), fc.CASE_S)
    assert got.shape == (n, 3, 16, 16) and got.dtype == torch.uint8
    bad = _differing(got.cpu().numpy(), small.want, small.names)
    assert not bad, f'{len(bad)} of {n} cases differ (name, differing bytes): {bad[:12]}'
    pad = small.names.index('in-the-pad/image2')
    assert not small.want[pad].any() and small.want[small.names.index('identity/image3')].all()


@pytest.mark.parametrize('S, sizes', [(64, ((300, 420), (50, 70))), (10, ((30, 25), (8, 12)))])
def test_other_window_sizes_are_bit_exact(vited, gpu, S, sizes):
    """S = 64: eight bands of rows per sample and dword stores; S = 10: two bands, byte stores.  Plans drawn like the loader's, one
    image larger and one smaller than the window, through all three stages."""
    images, plan = fc.plan_drawn_batch(S, sizes)
    store = vited.engine.Div2kImageStore(images, gpu)
    p = _dev(plan, gpu)
    win = _windows(vited, store, p, S)
    want_win = fc.windows_ref(images, plan['image'], plan['flags'], plan['afix'], plan['minv'], plan['origin'], S)
    assert not _differing(win.cpu().numpy(), want_win)
    assert {int(f) & 2 for f in plan['flags']} == {0, 2} and any(int(f) & 4 for f in plan['flags']) and any(int(f) & 8 for f in plan['flags'])
    got = vited.ops.hisfrag_blur_u8(vited.ops.hisfrag_jitter_u8(win, p['flags'], p['order'], p['factors'], p['hue']), p['flags'], p['blur'])
    assert not _differing(got.cpu().numpy(), _colour_want(want_win, plan))


@pytest.mark.parametrize('S', [16, 10])
def test_jitter_is_bit_exact_in_all_24_orders(vited, gpu, S):
    imgs, plan = fc.colour_cases(S)
    assert {tuple(r) for r in plan['order'][:24].tolist()} == set(fc.ORDERS)
    p, x = _dev(plan, gpu), torch.from_numpy(imgs).to(gpu)
    got = vited.ops.hisfrag_jitter_u8(x, p['flags'], p['order'], p['factors'], p['hue'])
    assert torch.equal(x.cpu(), torch.from_numpy(imgs))                                       # the input is left alone ...
    want = _colour_want(imgs, plan)
    assert not _differing(got.cpu().numpy(), want)
    assert vited.ops.hisfrag_jitter_u8(x, p['flags'], p['order'], p['factors'], p['hue'], out=x) is x and np.array_equal(x.cpu().numpy(), want)
    # ... the half-mean crops really round their mean up, and the jitter does something
    assert fc.contrast_mean(imgs[24].astype(np.int64)) == 101 and int(fc.luma(imgs[24].astype(np.int64)).sum()) * 2 == 201 * S * S
    assert sum(not np.array_equal(want[k], imgs[k]) for k in range(26)) == 26
    off = torch.zeros_like(p['flags'])
    x = torch.from_numpy(imgs).to(gpu)
    assert torch.equal(vited.ops.hisfrag_jitter_u8(x, off, p['order'], p['factors'], p['hue']), x)      # jitter off: unchanged


@pytest.mark.parametrize('S', [16, 10])
def test_blur_is_bit_exact(vited, gpu, S):
    imgs, plan = fc.blur_cases(S)
    p, x = _dev(plan, gpu), torch.from_numpy(imgs).to(gpu)
    jittered = vited.ops.hisfrag_jitter_u8(x, p['flags'], p['order'], p['factors'], p['hue'])
    got = vited.ops.hisfrag_blur_u8(jittered, p['flags'], p['blur']).cpu().numpy()
    want = _colour_want(imgs, plan)
    assert not _differing(got, want)
    assert np.array_equal(got[7], imgs[7]) and all(not np.array_equal(got[k], imgs[k]) for k in range(7))     # both off: unchanged
    off = torch.zeros_like(p['flags'])
    assert torch.equal(vited.ops.hisfrag_blur_u8(x, off, p['blur']), x)
    with pytest.raises(ValueError, match='out'):
        vited.ops.hisfrag_blur_u8(x, p['flags'], p['blur'], out=x)                            # a 3 x 3 filter cannot run in place


def test_out_argument(vited, gpu, small):
    n = 10
    p = {k: v[:n].contiguous() for k, v in _dev(small.table, gpu).items()}
    out = torch.zeros(n, 3, 16, 16, dtype=torch.uint8, device=gpu)
    assert _windows(vited, small.store, p, fc.CASE_S, out=out) is out
    assert np.array_equal(out.cpu().numpy(), small.want[:n])
    strided = torch.zeros(n, 2, 3, 16, 16, dtype=torch.uint8, device=gpu)[:, 0]               # batch stride of two windows: refused, like
    with pytest.raises(ValueError, match='out'):                                               # the `out` of ops.div2k_regions_u8
        _windows(vited, small.store, p, fc.CASE_S, out=strided)
    with pytest.raises(ValueError, match='out'):
        _windows(vited, small.store, p, fc.CASE_S, out=torch.zeros(n, 3, 16, 17, dtype=torch.uint8, device=gpu))
    with pytest.raises(ValueError, match='out'):
        vited.ops.hisfrag_jitter_u8(out, p['flags'], p['order'], p['factors'], p['hue'], out=strided)
    with pytest.raises(RuntimeError, match='CPU tensor'):
        _windows(vited, small.store, {k: v.cpu() for k, v in p.items()}, fc.CASE_S)
    with pytest.raises(RuntimeError, match='bad argument|vited error'):                        # the entry point's own range check
        _windows(vited, small.store, p, 1, out=torch.zeros(n, 3, 1, 1, dtype=torch.uint8, device=gpu))


def test_device_side_arguments_are_clamped(vited, gpu, small):
    """image = -1 / n give the result of the clamped index; origins far outside give all zeros; absurd affine coefficients and
    non-finite warp maps give zeros or pixels, deterministically: nothing is read out of bounds."""
    n = len(small.images)
    inv = fc.invert_affine(fc.forward_matrix(40, 56, 7.0, 0.95, 0.02, 0.03))
    image = np.array([-1, n, -7, n + 100, 3, 3, 3, 3, 4, 4], dtype=np.int32)
    clamped = np.array([0, n - 1, 0, n - 1, 3, 3, 3, 3, 4, 4], dtype=np.int32)
    origin = np.array([[0, 0], [3, 5], [-4, -2], [20, 30], [10 ** 9, 10 ** 9], [-2 ** 31, 2 ** 31 - 1], [-10 ** 6, 5], [5, 5], [5, 5], [5, 5]])
    flags = np.array([0, fc.WARP, fc.AFFINE, fc.AFFINE | fc.WARP, 0, fc.WARP, fc.AFFINE | fc.WARP, fc.AFFINE, fc.WARP, fc.WARP], dtype=np.int32)
    afix = np.tile(np.array([fc.affine_fixed(fc.inverse_affine_matrix(56, 40, 3.0, 2, -1))], dtype=np.int64), (len(image), 1))
    afix[7] = [2 ** 62, -2 ** 63, 2 ** 63 - 1, 12345678901234, -2 ** 40, 2 ** 62]
    minv = np.array([inv] * len(image))
    minv[8] = [np.nan, np.inf, -np.inf, 1e300, -1e300, np.nan]
    minv[9] = [1e6, 0, 0, 0, -1e6, 0]
    plan = {'image': image, 'flags': flags, 'afix': afix, 'minv': minv, 'origin': origin.astype(np.int32)}
    got = _windows(vited, small.store, _dev(plan, gpu), fc.CASE_S).cpu().numpy()
    rows = [0, 1, 2, 3, 4, 5, 6, 9]
    want = fc.windows_ref(small.images, clamped[rows], flags[rows], afix[rows], minv[rows], origin[rows], fc.CASE_S)
    assert np.array_equal(got[rows], want)
    assert not got[4:7].any() and got[:4].any(axis=(1, 2, 3)).all()
    # wrapped 64-bit products and NaN maps are outside what numpy restates: the run itself, a second run and zeros where the
    # taps cannot be inside are what is asserted
    again = _windows(vited, small.store, _dev(plan, gpu), fc.CASE_S).cpu().numpy()
    assert np.array_equal(got, again) and not got[8].any()


def _toy(vited, gpu):
    labels, images = fc.toy_writers()
    return vited.engine.Div2kImageStore(images, gpu), labels, images


def test_loader_end_to_end(vited, gpu):
    S, E = 16, vited.engine
    store, labels, images = _toy(vited, gpu)
    mk = lambda **kw: E.HisfragDeviceLoader(store, labels, 9, S, **{'m': 3, 'repeat': 2, 'seed': 5, **kw})
    loader = mk()
    batches = list(loader)
    assert len(batches) == len(loader) == 31 * 2 // 9
    idx = loader.rank_indices()
    for b, (x, t) in enumerate(batches):
        assert x.shape == (9, 3, S, S) and x.dtype == torch.uint8 and x.device.type == 'cuda' and x.is_contiguous()
        assert t.shape == (9,) and t.dtype == torch.int64 and t.device.type == 'cuda'
        runs = t.view(3, 3).tolist()
        assert all(len(set(r)) == 1 for r in runs) and len({r[0] for r in runs}) == 3           # m equal targets, distinct between runs
        assert t.tolist() == [labels[k] for k in idx[b].tolist()]                               # every index belongs to its writer
        for members, r in zip(idx[b].view(3, 3).tolist(), runs):
            assert len(set(members)) == min(labels.count(r[0]), 3)                              # two members: one of them repeats
    assert any(labels.count(t) == 2 for x, tt in batches for t in tt.tolist())
    # the first batch again, stage by stage from the loader's own draws
    plan = loader.plan(idx[0], loader._generator(1))
    assert torch.equal(plan.image.long(), idx[0])
    as_np = {k: v.cpu().numpy() for k, v in plan._asdict().items()}
    assert np.array_equal(batches[0][0].cpu().numpy(), fc.feed_ref(images, as_np, S))
    assert torch.equal(E.hisfrag_feed(store, plan, S), batches[0][0])
    # the same seed gives the same batches, another epoch or rank other ones
    for (xa, ta), (xb, tb) in zip(batches, list(mk())):
        assert torch.equal(xa, xb) and torch.equal(ta, tb)
    loader.set_epoch(1)
    assert not all(torch.equal(xa, xb) for (xa, _), (xb, _) in zip(batches, list(loader)))
    other = list(mk(rank=1, world=2))
    assert len(other) == 31 * 2 // 2 // 9 and not all(torch.equal(xa, xb) for (xa, _), (xb, _) in zip(batches, other))
    # train=False: the centre crops, zero-padded where the image is smaller
    ev = mk(train=False)
    x, t = next(iter(ev))
    for k, i in enumerate(ev.rank_indices()[0].tolist()):
        H, W, _ = images[i].shape
        want = fc.window_ref(images[i], 0, fc.IDENTITY_FIX, fc.IDENTITY, fc.centre_origin(H, S), fc.centre_origin(W, S), S)
        assert np.array_equal(x[k].cpu().numpy(), want) and int(t[k]) == labels[i]
        if H >= S and W >= S:
            top, left = fc.round_half_even((H - S) / 2), fc.round_half_even((W - S) / 2)
            assert np.array_equal(want, images[i][top: top + S, left: left + S].transpose(2, 0, 1))


def test_loader_feeds_the_two_stage_step(vited, gpu):
    """``hisfrag_prepare_data`` on the loader's batches as they come (uint8 images, int64 writer ids), then the decoder forward, the
    loss and the update (hisfrag.py:117-159): finite losses, every Linear weight moved.  Config T's geometry (64-pixel images,
    32-pixel patches, width 32, one class), fp32."""
    s, E = vo.SHAPE_T, vited.engine
    rng = np.random.default_rng(71)
    sizes = [(64, 64), (50, 90), (128, 100), (70, 40), (200, 150), (64, 65), (90, 90), (33, 80)]
    store = E.Div2kImageStore([rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes], gpu)
    loader = E.HisfragDeviceLoader(store, [0, 0, 0, 1, 1, 2, 2, 2], 6, s.img_size, m=3, repeat=2, seed=1)
    assert len(loader) == 2
    torch.manual_seed(0)
    m = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                      embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads)
    m.compute_dtype = torch.float32
    m = m.to(gpu)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt = vited.optim.FlatAdamW(E.param_groups_no_decay_1d(m), lr=1e-3, weight_decay=0.05)
    scaler = E.NativeScalerWithGradNormCount()                    # the reference's call shape (misc/engine.py:208-231)
    losses = []
    opt.zero_grad()
    for images, targets in loader:
        (x, feats), labels = E.hisfrag_prepare_data(m, images, targets, amp=False)
        same = int((targets[:, None] == targets[None, :]).triu(1).sum())                       # 3 positive pairs per run of one writer
        assert x.dtype == torch.uint8 and labels.shape[0] == x.shape[0] and float(labels.sum()) == same >= 6
        loss = torch.nn.functional.binary_cross_entropy_with_logits(m(feats, x), labels)
        scaler(loss, opt, clip_grad=5.0, parameters=m.parameters())
        opt.zero_grad()
        losses.append(float(loss))
    assert len(losses) == 2 and all(np.isfinite(losses)) and all(v > 0 for v in losses), losses
    stuck = [n for n, p in m.named_parameters() if p.ndim == 2 and torch.equal(p.detach(), before[n])]
    assert not stuck, stuck                                       # every Linear weight moved
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
