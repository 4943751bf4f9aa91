"""The DIV2K device feed on the GPU: ``vited_div2k_regions_u8`` bit for bit against the numpy restatement of
its per-pixel definition (tests/div2k_feed_cases.py, itself checked in tests/test_div2k_feed.py), the clamping of device-side
arguments, the tie to the Pillow-pinned pair assembly behind it, and ``Div2kDeviceLoader`` feeding ``TrainStep.step``.
Equality is exact everywhere: the definition is integer arithmetic on separately rounded fp64 terms plus one fp32 clamp."""
import dataclasses

import numpy as np
import pytest
import torch

import div2k_feed_cases as fc
from oracle import vited_oracle as vo

pytestmark = pytest.mark.gpu


class _Small:
    """The S = 8 store of the case table, on the device and as numpy, with the table's reference regions (computed once)."""

    def __init__(self, vited, gpu):
        self.images = fc.case_images()
        self.store = vited.engine.Div2kImageStore(self.images, gpu)
        self.table, self.names = fc.case_table(self.images)
        self.want = fc.regions_ref(self.images, self.table['image'], self.table['flags'], self.table['minv'], self.table['rgb'],
                                   self.table['crop'], fc.CASE_S)
        self.want.setflags(write=False)


@pytest.fixture(scope='module')
def small(vited, gpu):
    return _Small(vited, gpu)


def _run(vited, store, gpu, image, flags, minv, rgb, crop, S, out=None):
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(gpu).contiguous()
    return vited.ops.div2k_regions_u8(store.data, store.offsets_dev, store.sizes_dev, t(image, torch.int32), t(flags, torch.int32),
                                      t(minv, torch.float64), t(rgb, torch.float32), t(crop, torch.int32), S, out=out)


def test_case_table_is_bit_exact(vited, gpu, small):
    tb = small.table
    got = _run(vited, small.store, gpu, tb['image'], tb['flags'], tb['minv'], tb['rgb'], tb['crop'], fc.CASE_S)
    assert got.shape == (len(small.names), 3, 16, 24) and got.dtype == torch.uint8
    got = got.cpu().numpy()
    bad = [(small.names[k], int((got[k] != small.want[k]).sum())) for k in range(len(small.names)) if not np.array_equal(got[k], small.want[k])]
    assert not bad, f'{len(bad)} of {len(small.names)} cases differ (name, differing bytes): {bad[:12]}'


def test_workload_window_is_bit_exact(vited, gpu):
    """S = 64 (windows of 128 x 192: 8 bands of rows per sample), one 300 x 420 image, plans drawn like the loader's."""
    S, B = 64, 8
    rng = np.random.default_rng(31)
    img = rng.integers(0, 256, size=(300, 420, 3), dtype=np.uint8)
    store = vited.engine.Div2kImageStore([img], gpu)
    u = rng.random((B, 13)).astype(np.float32)
    u[:, 2] = [0.1, 0.2, 0.3, 0.4, 0.1, 0.2, 0.9, 0.9]            # six warped samples, two plain
    u[4, 11:] = 0.0                                               # one window in the corner: taps off the image
    u[5, 11:] = 0.999
    plans = [fc.plan_sample(u[k], 300, 420, S) for k in range(B)]
    flags, minv, rgb, crop = [p[0] for p in plans], [p[2] for p in plans], [p[3] for p in plans], [p[4] for p in plans]
    got = _run(vited, store, gpu, [0] * B, flags, minv, rgb, crop, S).cpu().numpy()
    touched = 0
    for k in range(B):
        want, touch = fc.region_ref(img, flags[k], minv[k], rgb[k], crop[k][0], crop[k][1], S, want_touch=True)
        touched += touch
        assert np.array_equal(got[k], want), (k, flags[k], crop[k], int((got[k] != want).sum()))
    assert 1 <= touched < 6                                       # both the reflected and the unreflected path ran warped


def test_out_argument(vited, gpu, small):
    tb, n = small.table, 10
    args = [tb[k][:n] for k in ('image', 'flags', 'minv', 'rgb', 'crop')]
    out = torch.zeros(n, 3, 16, 24, dtype=torch.uint8, device=gpu)
    assert _run(vited, small.store, gpu, *args, fc.CASE_S, out=out) is out
    assert np.array_equal(out.cpu().numpy(), small.want[:n])
    strided = torch.zeros(n, 2, 3, 16, 24, dtype=torch.uint8, device=gpu)[:, 0]       # batch stride of two regions: refused, like
    with pytest.raises(ValueError, match='out'):                                       # the `out` of ops.cast
        _run(vited, small.store, gpu, *args, fc.CASE_S, out=strided)
    with pytest.raises(ValueError, match='out'):
        _run(vited, small.store, gpu, *args, fc.CASE_S, out=torch.zeros(n, 3, 16, 25, dtype=torch.uint8, device=gpu))
    with pytest.raises(RuntimeError, match='CPU tensor'):
        vited.ops.div2k_regions_u8(small.store.data.cpu(), small.store.offsets, small.store.sizes, *[torch.as_tensor(a) for a in args], fc.CASE_S)


def test_device_side_arguments_are_clamped(vited, gpu, small):
    """image = -1 / n and crop origins outside the image give the result of the clamped arguments (crop_pairs_u8_kernel treats
    cells / erode the same way): deterministic, nothing is read out of bounds."""
    n = len(small.images)
    inv = fc.invert_affine(fc.forward_matrix(40, 56, 11.0, 0.9, 0.02, 0.03))
    image = np.array([-1, n, -7, n + 100, 2, 2, 2, 5, 5], dtype=np.int32)
    clamped_image = np.array([0, n - 1, 0, n - 1, 2, 2, 2, 5, 5], dtype=np.int32)
    crop = np.array([[0, 0], [3, 5], [9, 9], [-4, 1000], [-1, -1], [22, 30], [10 ** 6, -10 ** 6], [10 ** 9, 10 ** 9], [24, 33]], dtype=np.int32)
    flags = np.array([0, fc.WARP, fc.HFLIP, fc.WARP | fc.VFLIP, 0, fc.WARP, fc.WARP, fc.WARP | fc.COLOUR, 0], dtype=np.int32)
    minv = np.array([inv] * len(image))
    rgb = np.tile(np.array([[3.5, -2.0, 9.0]], dtype=np.float32), (len(image), 1))
    sizes = [small.images[k].shape[:2] for k in clamped_image]
    clamped_crop = np.array([[min(max(int(t), 0), h - 16), min(max(int(l), 0), w - 24)] for (t, l), (h, w) in zip(crop, sizes)], dtype=np.int32)
    assert clamped_crop.tolist() == [[0, 0], [3, 5], [0, 0], [0, 32], [0, 0], [21, 29], [21, 0], [24, 32], [24, 32]]
    got = _run(vited, small.store, gpu, image, flags, minv, rgb, crop, fc.CASE_S).cpu().numpy()
    assert np.array_equal(got, fc.regions_ref(small.images, clamped_image, flags, minv, rgb, clamped_crop, fc.CASE_S))


def test_evaluation_plan_gives_the_centre_slice_and_feeds_the_pair_assembly(vited, gpu, small):
    """train=False: the regions are the CenterCrop slices, and regions -> assemble_pairs equals assemble_pairs of the sliced
    regions, which ties the new stage to the Pillow-pinned one behind it."""
    S, E = fc.CASE_S, vited.engine
    image = torch.tensor([0, 1, 2, 3, 4, 5, 5, 2], device=gpu)
    u = torch.rand(8, 13, generator=torch.Generator().manual_seed(2)).to(gpu)
    idx, flags, minv, rgb, crop = E.div2k_augment_plan(u, image, small.store.sizes_dev, S, train=False)
    regions = vited.ops.div2k_regions_u8(small.store.data, small.store.offsets_dev, small.store.sizes_dev, idx, flags, minv, rgb, crop, S)
    sliced = []
    for k in image.tolist():
        h, w = small.images[k].shape[:2]
        t, l = fc.round_half_even((h - 2 * S) / 2), fc.round_half_even((w - 3 * S) / 2)
        sliced.append(small.images[k][t: t + 2 * S, l: l + 3 * S].transpose(2, 0, 1))
    sliced = torch.from_numpy(np.stack(sliced)).to(gpu)
    assert torch.equal(regions, sliced)
    cells, labels, erode = E.div2k_pair_plan(torch.rand(8, 4, generator=torch.Generator().manual_seed(3)).to(gpu), S, 0.07, train=False)
    assert torch.equal(E.assemble_pairs(regions, cells, erode, S), E.assemble_pairs(sliced, cells, erode, S))


def test_loader_end_to_end(vited, gpu, small):
    S, E = fc.CASE_S, vited.engine
    mk = lambda **kw: E.Div2kDeviceLoader(small.store, 4, S, 0.07, repeat=3, **{'seed': 5, **kw})
    loader = mk()
    batches = list(loader)
    assert len(batches) == len(loader) == 6 * 3 // 4
    for pairs, labels in batches:
        assert pairs.shape == (4, 2, 3, S, S) and pairs.dtype == torch.uint8 and pairs.device.type == 'cuda'
        assert labels.shape == (4, 4) and labels.dtype == torch.float32 and labels.device.type == 'cuda'
        assert bool(((labels == 0) | (labels == 1)).all()) and bool((labels.sum(1) <= 1).all())
    # the first batch again, stage by stage from the loader's own draws: labels go with the cells, pairs with the regions
    (idx, flags, minv, rgb, crop), (cells, labels, erode) = loader.plan(loader.rank_indices()[0], loader._generator(1))
    assert torch.equal(labels, batches[0][1]) and torch.equal(idx.long(), loader.rank_indices()[0])
    for k in range(4):
        c1, c2, lab = int(cells[k, 0]), int(cells[k, 1]), labels[k].tolist()
        if sum(lab) == 0:
            assert {c1, c2} in ({0, 4}, {0, 2})                                    # the negatives: third / spare cell
        else:
            assert (c1, c2) == {0: (0, 1), 1: (0, 3), 2: (1, 0), 3: (3, 0)}[lab.index(1.0)]
    images = small.images
    sizes = [images[int(i)].shape[:2] for i in idx]
    assert all(0 <= int(crop[k, 0]) <= sizes[k][0] - 2 * S and 0 <= int(crop[k, 1]) <= sizes[k][1] - 3 * S for k in range(4))
    want = fc.regions_ref(images, idx.tolist(), flags.tolist(), minv.cpu().numpy(), rgb.cpu().numpy(), crop.tolist(), S)
    assert torch.equal(batches[0][0], E.assemble_pairs(torch.from_numpy(want).to(gpu), cells, erode, S))
    # the same seed gives the same batches, another epoch or rank other ones
    for (pa, la), (pb, lb) in zip(batches, list(mk())):
        assert torch.equal(pa, pb) and torch.equal(la, lb)
    loader.set_epoch(1)
    assert not all(torch.equal(pa, pb) for (pa, _), (pb, _) in zip(batches, list(loader)))
    assert len(list(mk(rank=1, world=2))) == 6 * 3 // 2 // 4


def test_loader_feeds_a_train_step(vited, gpu):
    """``TrainStep.step`` on the loader's batches as they come (uint8 pairs, fp32 labels, no conversion in between): finite losses and
    updated weights.  Config T's geometry (64-pixel images, 32-pixel patches, width 32) with the 4-bin head the DIV2K labels need;
    T itself has one class."""
    s = dataclasses.replace(vo.SHAPE_T, num_classes=4)
    rng = np.random.default_rng(41)
    store = vited.engine.Div2kImageStore([rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((128, 192), (150, 230), (300, 420))], gpu)
    loader = vited.engine.Div2kDeviceLoader(store, 4, s.img_size, 0.07, repeat=3, seed=1)
    assert len(loader) == 2
    torch.manual_seed(0)
    m = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                      embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads)
    m.compute_dtype = torch.float32
    m = m.to(gpu)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt = vited.optim.FlatAdamW(vited.engine.param_groups_no_decay_1d(m), lr=1e-3, weight_decay=0.05)
    step = vited.engine.TrainStep(m, opt, clip_grad=5.0, amp=False)
    losses = [float(step.step(pairs, labels)) for pairs, labels in loader]
    assert len(losses) == 2 and all(np.isfinite(losses)) and all(v > 0 for v in losses), losses
    assert step.num_updates == 2 and bool(torch.isfinite(step.last_norm)) and float(step.last_norm) > 0
    stuck = [n for n, p in m.named_parameters() if p.ndim == 2 and torch.equal(p.detach(), before[n])]
    assert not stuck, stuck                                       # every Linear weight moved
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
