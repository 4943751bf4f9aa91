"""The michigan device feed on the GPU: ``vited_michigan_windows_u8`` and ``vited_michigan_blur_gray_u8`` bit for
bit against the numpy restatement of their per-pixel definition (tests/michigan_feed_cases.py, itself checked against Pillow in
tests/test_michigan_feed.py), chained with ``vited_hisfrag_jitter_u8``, the clamping of device-side arguments, and
``MichiganDeviceLoader`` feeding the two-stage step.  Equality is exact everywhere: the definition is integer arithmetic."""
import numpy as np
import pytest
import torch

import michigan_feed_cases as mc
from oracle import vited_oracle as vo

pytestmark = pytest.mark.gpu

BLUR_TILE = (16, 128)       # rows x columns of vited_michigan_blur_gray_u8's LDS tile (MB_TH x MB_TW in csrc/michigan_feed.hip)

_DTYPES = {'image': torch.int32, 'flags': torch.int32, 'origin': torch.int32, 'box': torch.int32, 'x0': torch.int32, 'kx': torch.int32,
           'y0': torch.int32, 'ky': torch.int32, 'holes': torch.int32, 'n_holes': torch.int32, 'order': torch.int32, 'factors': torch.float32,
           'hue': torch.int32, 'blur': torch.int32}


def _dev(plan, gpu):
    return {k: torch.as_tensor(np.asarray(v), dtype=_DTYPES[k]).to(gpu).contiguous() for k, v in plan.items()}


def _windows(vited, store, p, S, out=None):
    return vited.ops.michigan_windows_u8(store.data, store.offsets_dev, store.sizes_dev, p['image'], p['flags'], p['origin'], p['x0'], p['kx'],
                                         p['y0'], p['ky'], p['holes'], p['n_holes'], S, out=out)


def _colour_want(imgs, plan):
    return np.stack([mc.colour_ref(imgs[k], int(plan['flags'][k]), [int(t) for t in plan['order'][k]], plan['factors'][k], int(plan['hue'][k]),
                                   plan['blur'][k]) for k in range(len(imgs))])


def _differing(got, want, names=None):
    return [(names[k] if names else k, int((got[k] != want[k]).sum())) for k in range(len(want)) if not np.array_equal(got[k], want[k])]


class _Small:
    """The S = 16 store of the geometry case table, on the device and as numpy, with the table's reference crops (computed once)."""

    def __init__(self, vited, gpu):
        self.images = mc.case_images()
        self.store = vited.engine.Div2kImageStore(self.images, gpu)
        self.table, self.names = mc.case_table(self.images)
        self.want, self.touch = mc.case_refs(self.images, self.table)
        self.want.setflags(write=False)


@pytest.fixture(scope='module')
def small(vited, gpu):
    return _Small(vited, gpu)


def test_geometry_case_table_is_bit_exact(vited, gpu, small):
    n = len(small.names)
    assert 3 * sum(small.touch) >= n and 3 * (n - sum(small.touch)) >= n, (sum(small.touch), n)      # pad pixels among the taps / none
    got = _windows(vited, small.store, _dev(small.table, gpu), mc.CASE_S)
    assert got.shape == (n, 3, 16, 16) and got.dtype == torch.uint8
    bad = _differing(got.cpu().numpy(), small.want, small.names)
    assert not bad, f'{len(bad)} of {n} cases differ (name, differing bytes): {bad[:12]}'
    assert (small.want[small.names.index('all-pad/image2')] == 255).all()
    k = small.names.index('identity/image3')
    top, left = (int(t) for t in small.table['origin'][k])
    assert np.array_equal(small.want[k], small.images[3][top: top + 16, left: left + 16].transpose(2, 0, 1))


@pytest.mark.parametrize('S, sizes', [(64, ((300, 420), (50, 70))), (10, ((30, 25), (8, 12)))])
def test_other_window_sizes_are_bit_exact(vited, gpu, S, sizes):
    """S = 64: eight bands of rows per sample, dword stores; S = 10: two bands, byte stores.  Plans drawn like the loader's, one
    image larger and one smaller than the window, through all three stages."""
    images, plan = mc.plan_drawn_batch(S, sizes)
    store = vited.engine.Div2kImageStore(images, gpu)
    p = _dev(plan, gpu)
    win = _windows(vited, store, p, S)
    want_win = mc.windows_ref(images, plan, S)
    assert not _differing(win.cpu().numpy(), want_win)
    on = lambda bit: {int(f) & bit for f in plan['flags']}
    assert all(on(bit) == {0, bit} for bit in (mc.DROPOUT, mc.JITTER, mc.BLUR, mc.GRAY))
    jit = vited.ops.hisfrag_jitter_u8(win, p['flags'], p['order'], p['factors'], p['hue'])
    got = vited.ops.michigan_blur_gray_u8(jit, p['flags'], p['blur'])
    assert not _differing(got.cpu().numpy(), _colour_want(want_win, plan))


@pytest.mark.parametrize('S', [16, 10, 132, 150])
def test_blur_and_gray_are_bit_exact(vited, gpu, S):
    """S = 132 and 150 are larger than the blur tile in both directions and no multiple of it (132: dword loads and stores, 150: byte
    ones); 16 and 10 fit one tile with room to spare on its right."""
    assert S < BLUR_TILE[1] or (S % BLUR_TILE[0] and S % BLUR_TILE[1] and S > BLUR_TILE[0])
    imgs, flags, weights = mc.blur_cases(S)
    x = torch.from_numpy(imgs).to(gpu)
    f, w = torch.from_numpy(flags).to(gpu), torch.from_numpy(weights).to(gpu)
    got = vited.ops.michigan_blur_gray_u8(x, f, w).cpu().numpy()
    assert torch.equal(x.cpu(), torch.from_numpy(imgs))
    want = np.stack([mc.blur_gray_ref(imgs[k], int(flags[k]), weights[k]) for k in range(len(imgs))])
    assert not _differing(got, want)
    assert np.array_equal(got[7], imgs[7]) and np.array_equal(got[8], imgs[8])                 # neither bit: a copy
    assert all(not np.array_equal(got[k], imgs[k]) for k in range(7)) and np.array_equal(got[9], imgs[9])     # a constant stays constant
    assert np.array_equal(got[4][0], got[4][1]) and np.array_equal(got[4][0], got[4][2])       # grey: three equal channels
    off = torch.zeros_like(f)
    assert torch.equal(vited.ops.michigan_blur_gray_u8(x, off, w), x)
    with pytest.raises(ValueError, match='out'):
        vited.ops.michigan_blur_gray_u8(x, f, w, out=x)                                        # the passes cannot run in place


def test_jitter_then_blur_with_the_plan_ranges(vited, gpu):
    S, n = 16, 24
    rng = np.random.default_rng(81)
    imgs = rng.integers(0, 256, size=(n, 3, S, S), dtype=np.uint8)
    u = torch.rand(n, mc.PLAN_COLUMNS, generator=torch.Generator().manual_seed(82))
    u[:, 92], u[:, 101], u[:, 103] = 0.25, 0.25, 0.6                                           # jitter and blur on, grey off ...
    u[::3, 103] = 0.1                                                                          # ... but in every third
    u[0, 97:101], u[1, 97:101], u[0, 102], u[1, 102] = 0.0, 0.99999, 0.0, 0.99999              # the ends of every range
    plan = vited.engine.michigan_augment_plan(u.to(gpu), torch.zeros(n, dtype=torch.int64), torch.tensor([[40, 40]], dtype=torch.int32), S)
    as_np = {k: v.cpu().numpy() for k, v in plan._asdict().items()}
    assert all(int(f) & 12 == 12 for f in as_np['flags']) and len({tuple(r) for r in as_np['order'].tolist()}) >= 8
    x = torch.from_numpy(imgs).to(gpu)
    jit = vited.ops.hisfrag_jitter_u8(x, plan.flags, plan.order, plan.factors, plan.hue)
    got = vited.ops.michigan_blur_gray_u8(jit, plan.flags, plan.blur).cpu().numpy()
    assert not _differing(got, _colour_want(imgs, as_np))
    assert as_np['blur'][0].tolist() == list(mc.blur_weights(0.1))


def test_plan_on_the_device_equals_the_host_plan(vited, gpu):
    """The plan's fp64 and fp32 arithmetic gives the same integers on the device as on the host (whose plan tests/test_michigan_feed.py
    holds to the per-sample restatement): divisions are true divisions there too."""
    sizes = torch.tensor([(64, 64), (50, 70), (300, 420), (30, 41)], dtype=torch.int32)
    for S, train in ((64, True), (10, True), (33, False)):
        u = torch.rand(512, mc.PLAN_COLUMNS, generator=torch.Generator().manual_seed(84 + S))
        image = torch.arange(512) % 4
        host = vited.engine.michigan_augment_plan(u, image, sizes, S, train=train)
        dev = vited.engine.michigan_augment_plan(u.to(gpu), image.to(gpu), sizes.to(gpu), S, train=train)
        for name, a, b in zip(host._fields, host, dev):
            assert b.device.type == 'cuda' and torch.equal(a, b.cpu()), (S, train, name)


def test_out_argument_and_range_checks(vited, gpu, small):
    n = 10
    p = {k: v[:n].contiguous() for k, v in _dev(small.table, gpu).items()}
    out = torch.zeros(n, 3, 16, 16, dtype=torch.uint8, device=gpu)
    assert _windows(vited, small.store, p, mc.CASE_S, out=out) is out
    assert np.array_equal(out.cpu().numpy(), small.want[:n])
    strided = torch.zeros(n, 2, 3, 16, 16, dtype=torch.uint8, device=gpu)[:, 0]               # batch stride of two crops: refused, like the
    with pytest.raises(ValueError, match='out'):                                               # `out` of ops.hisfrag_windows_u8
        _windows(vited, small.store, p, mc.CASE_S, out=strided)
    with pytest.raises(ValueError, match='out'):
        _windows(vited, small.store, p, mc.CASE_S, out=torch.zeros(n, 3, 16, 17, dtype=torch.uint8, device=gpu))
    blurred = torch.empty_like(out)
    assert vited.ops.michigan_blur_gray_u8(out, p['flags'], p['blur'], out=blurred) is blurred
    with pytest.raises(ValueError, match='out'):
        vited.ops.michigan_blur_gray_u8(out, p['flags'], p['blur'], out=strided)
    with pytest.raises(RuntimeError, match='CPU tensor'):
        _windows(vited, small.store, {k: v.cpu() for k, v in p.items()}, mc.CASE_S)
    with pytest.raises(RuntimeError, match='CPU tensor'):
        vited.ops.michigan_blur_gray_u8(out.cpu(), p['flags'], p['blur'])
    # the entry points' own range checks: S outside 2..4096, a batch outside 1..65535, a null pointer, out == in
    L, st = vited._lib, small.store
    ptr = lambda t: t.data_ptr()
    w_args = lambda b, s, o: (ptr(st.data), ptr(st.offsets_dev), ptr(st.sizes_dev), len(st), ptr(p['image']), ptr(p['flags']), ptr(p['origin']),
                              ptr(p['x0']), ptr(p['kx']), ptr(p['y0']), ptr(p['ky']), ptr(p['holes']), ptr(p['n_holes']), o, b, s, None)
    for b, s, o in ((n, 1, ptr(out)), (n, 4097, ptr(out)), (0, 16, ptr(out)), (65536, 16, ptr(out)), (n, 16, None)):
        with pytest.raises(RuntimeError, match='bad argument'):
            L.call('vited_michigan_windows_u8', *w_args(b, s, o))
        with pytest.raises(RuntimeError, match='bad argument'):
            L.call('vited_michigan_blur_gray_u8', ptr(out), ptr(p['flags']), ptr(p['blur']), ptr(blurred) if o else None, b, s, None)
    with pytest.raises(RuntimeError, match='bad argument'):
        L.call('vited_michigan_blur_gray_u8', ptr(out), ptr(p['flags']), ptr(p['blur']), ptr(out), n, 16, None)
    assert np.array_equal(out.cpu().numpy(), small.want[:n])                                   # nothing was launched


def test_device_side_arguments_are_clamped(vited, gpu, small):
    """image = -1 / n give the result of the clamped index; origins far outside give all 255; a hole count out of range is clamped to
    0..16; a first tap outside the window reads 255 (the pad), whatever lies there in the image; absurd weights give some bytes,
    the same in every run: nothing is read out of bounds."""
    S, n = mc.CASE_S, len(small.images)
    image = np.array([-1, n, -7, n + 100, 3, 3, 3, 4, 4, 4, 4, 4], dtype=np.int32)
    clamped = np.array([0, n - 1, 0, n - 1, 3, 3, 3, 4, 4, 4, 4, 4], dtype=np.int32)
    rows = len(image)
    origin = np.array([[0, 0], [3, 5], [-4, -2], [20, 30]] + [[10 ** 9, 10 ** 9], [-2 ** 31, 2 ** 31 - 1], [-10 ** 6, 5]] + [[5, 5]] * 5)
    x0, kx, y0, ky = (np.array([t] * rows) for t in mc.box_tables((1, 2, 13, 12), S))
    flags = np.array([0, mc.HFLIP, mc.VFLIP, mc.DROPOUT] + [0] * 3 + [mc.DROPOUT] * 2 + [0] * 3, dtype=np.int32)
    holes = np.array([mc.border_holes(S)] * rows)
    n_holes = np.array([0, 0, 0, 3, 0, 0, 0, 10 ** 6, -5, 0, 0, 0])
    x0[9, :4], x0[9, 4:8], x0[9, 8:12], x0[9, 12:] = -2, S - 1, 10 ** 9, -2 ** 31              # taps left of, across and far beyond the window
    y0[10, :5], y0[10, 5:10], y0[10, 10:] = -1, S - 2, 2 ** 31 - 1
    kx[11], ky[11] = [2 ** 31 - 1, -2 ** 31, 12345678], [-1, 2 ** 30, 2 ** 31 - 1]
    plan = {'image': image, 'flags': flags, 'origin': origin, 'x0': x0, 'kx': kx, 'y0': y0, 'ky': ky, 'holes': holes, 'n_holes': n_holes}
    got = _windows(vited, small.store, _dev(plan, gpu), S).cpu().numpy()
    exact = list(range(11))
    want = mc.windows_ref(small.images, dict(plan, image=clamped), S)
    assert not _differing(got[exact], want[exact])
    assert (got[4:7] == 255).all() and not (got[:4] == 255).all(axis=(1, 2, 3)).any()
    sixteen, none = (mc.windows_ref(small.images, dict(plan, image=clamped, n_holes=np.full(rows, k)), S) for k in (16, 0))
    assert np.array_equal(got[7], sixteen[7]) and np.array_equal(got[8], none[8]) and not np.array_equal(sixteen[7], none[7])
    assert (got[9][:, :, 8:] == 255).all() and (got[10][:, 10:, :] == 255).all() and not (got[9] == 255).all()     # the pad, not the image
    again = _windows(vited, small.store, _dev(plan, gpu), S).cpu().numpy()                     # wrapped products are outside what numpy
    assert np.array_equal(got, again)                                                          # restates: run-to-run equality


def _toy(vited, gpu):
    labels, images = mc.toy_writers()
    return vited.engine.Div2kImageStore(images, gpu), labels, images


def test_loader_end_to_end(vited, gpu):
    S, E = 16, vited.engine
    store, labels, images = _toy(vited, gpu)
    mk = lambda **kw: E.MichiganDeviceLoader(store, labels, 9, S, **{'m': 3, 'repeat': 2, 'seed': 5, **kw})
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
    # the first batch again, stage by stage from the loader's own draws
    plan = loader.plan(idx[0], loader._generator(1))
    assert torch.equal(plan.image.long(), idx[0])
    as_np = {k: v.cpu().numpy() for k, v in plan._asdict().items()}
    want_win = mc.windows_ref(images, as_np, S)
    win = _windows(vited, store, plan._asdict(), S)
    assert np.array_equal(win.cpu().numpy(), want_win)
    jit = vited.ops.hisfrag_jitter_u8(win, plan.flags, plan.order, plan.factors, plan.hue)
    want_jit = np.stack([mc.colour_ref(want_win[k], int(as_np['flags'][k]) & mc.JITTER, [int(t) for t in as_np['order'][k]], as_np['factors'][k],
                                       int(as_np['hue'][k]), as_np['blur'][k]) for k in range(9)])
    assert np.array_equal(jit.cpu().numpy(), want_jit)
    assert np.array_equal(batches[0][0].cpu().numpy(), mc.feed_ref(images, as_np, S))
    assert torch.equal(E.michigan_feed(store, plan, S), batches[0][0])
    # the same seed gives the same batches, another epoch or rank other ones
    for (xa, ta), (xb, tb) in zip(batches, list(mk())):
        assert torch.equal(xa, xb) and torch.equal(ta, tb)
    loader.set_epoch(1)
    assert not all(torch.equal(xa, xb) for (xa, _), (xb, _) in zip(batches, list(loader)))
    other = list(mk(rank=1, world=2))
    assert len(other) == 31 * 2 // 2 // 9 and not all(torch.equal(xa, xb) for (xa, _), (xb, _) in zip(batches, other))
    # train=False: the padded centre crop, resized to int(1.15 S) and centre-cropped
    ev = mk(train=False)
    x, t = next(iter(ev))
    tables, none = mc.eval_tables(S), [[0, 0, 0, 0]] * 16
    for k, i in enumerate(ev.rank_indices()[0].tolist()):
        H, W, _ = images[i].shape
        want = mc.geometry_ref(images[i], 0, (mc.centre_origin(H, S), mc.centre_origin(W, S)), *tables, none, 0, S)
        assert np.array_equal(x[k].cpu().numpy(), want) and int(t[k]) == labels[i]


def test_loader_feeds_the_two_stage_step(vited, gpu):
    """``hisfrag_prepare_data`` on the loader's batches as they come (uint8 images, int64 writer ids), then the decoder forward, the
    loss and the update (michigan.py's training step is hisfrag.py:117-159's): finite losses, every Linear weight moved.  Config T's
    geometry (64-pixel images, 32-pixel patches, width 32, one class), fp32."""
    s, E = vo.SHAPE_T, vited.engine
    rng = np.random.default_rng(83)
    sizes = [(64, 64), (50, 90), (128, 100), (70, 40), (200, 150), (64, 65), (90, 90), (33, 80)]
    store = E.Div2kImageStore([rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes], gpu)
    loader = E.MichiganDeviceLoader(store, [0, 0, 0, 1, 1, 2, 2, 2], 6, s.img_size, m=3, repeat=2, seed=1)
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
        losses.append(float(loss.detach()))
    assert len(losses) == 2 and all(np.isfinite(losses)) and all(v > 0 for v in losses), losses
    stuck = [n for n, p in m.named_parameters() if p.ndim == 2 and torch.equal(p.detach(), before[n])]
    assert not stuck, stuck                                       # every Linear weight moved
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
