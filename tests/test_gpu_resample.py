"""GPU: ``vited_resample_u8`` against ``ops.resample_u8`` on CPU tensors (the numpy statement of Pillow's rule, pinned against Pillow in
tests/test_resample.py), exactly and into 0xA5-filled buffers; then its callers - the Pajigsaw loader feeding ``TrainStep``, the puzzle
pieces feeding ``puzzle_distances``, and the evaluation sources feeding ``pairwise_similarity``.  All comparisons are bit for bit."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import vited_oracle as vo

pytestmark = pytest.mark.gpu

SIZES = [(5, 5), (7, 9), (16, 16), (33, 37), (64, 64), (100, 100), (128, 128), (1024, 1024)]       # 75, 189, ... bytes: odd offsets
POISON = 0xA5


@pytest.fixture(scope='module')
def images():
    rng = np.random.default_rng(42)
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in SIZES]


@pytest.fixture(scope='module')
def stores(vited, gpu, images):
    cpu = vited.engine.Div2kImageStore(images, 'cpu')
    assert [int(o) % 4 for o in cpu.offsets[1:5]] == [3, 0, 0, 3]                                  # images start at any byte
    return vited.engine.Div2kImageStore(images, gpu), cpu


def _both(vited, stores, image, windows, fill, Rh, Rw, ct, cl, S, out=None):
    """(kernel, rule) of one call; the kernel writes into a poisoned buffer unless ``out`` is given."""
    dev_store, cpu_store = stores
    ops, dev = vited.ops, dev_store.device
    image = torch.tensor(image, dtype=torch.int32)
    win = None if windows is None else torch.tensor(windows, dtype=torch.int32)
    hs = [SIZES[i][0] for i in image.tolist()] if windows is None else [w[2] for w in windows]
    ws = [SIZES[i][1] for i in image.tolist()] if windows is None else [w[3] for w in windows]
    xt, yt = ops.resample_tables(ws, Rw, dev), ops.resample_tables(hs, Rh, dev)
    if out is None:
        out = torch.full((image.numel(), 3, S, S), POISON, dtype=torch.uint8, device=dev)
    got = ops.resample_u8(dev_store.data, dev_store.offsets_dev, dev_store.sizes_dev, image.to(dev), None if win is None else win.to(dev), fill,
                          xt, yt, Rh, Rw, ct, cl, S, out=out)
    assert got.data_ptr() == out.data_ptr()
    want = ops.resample_u8(cpu_store.data, cpu_store.offsets, cpu_store.sizes, image, win, fill, None, None, Rh, Rw, ct, cl, S)
    return got, want


def _same(got, want):
    got = got.cpu()
    assert got.shape == want.shape and torch.equal(got, want), f'{int((got != want).sum())} of {want.numel()} bytes differ'


@pytest.mark.parametrize('S', (16, 32))
def test_whole_images(vited, stores, S):
    """5 -> S is 3.2x / 6.4x up, 16 -> 16 the identity, 33 x 37 and 100 non-integer, 100 -> 16 is 6.25x, 128 -> 16 is 8x with 17 taps."""
    _same(*_both(vited, stores, [0, 1, 2, 3, 4, 5, 6], None, 0, S, S, 0, 0, S))
    assert vited.ops.resample_ksize(128, 16) == 17


def test_wide_rows_with_17_taps(vited, stores):
    _same(*_both(vited, stores, [7], None, 0, 128, 128, 0, 0, 128))                                # 1024 -> 128


def test_widest_output(vited, stores):
    _same(*_both(vited, stores, [4], None, 0, 1024, 1024, 0, 0, 1024))                             # 64 -> 1024


WINDOWS = [[-5, -7, 40, 44], [20, 25, 40, 44], [-10, 90, 60, 30], [80, -3, 60, 30], [-30, -20, 160, 150], [300, 3, 40, 44], [3, -300, 40, 44],
           [0, 0, 100, 100]]


@pytest.mark.parametrize('fill', (0, 255))
def test_windows_over_every_edge(vited, stores, fill):
    """Negative origins, windows past the right and the bottom edge, around the whole image and wholly outside it."""
    image = [3, 3, 5, 5, 5, 5, 4, 5]
    _same(*_both(vited, stores, image, WINDOWS, fill, 24, 24, 0, 0, 24))                           # down, S % 4 == 0
    _same(*_both(vited, stores, image, WINDOWS, fill, 171, 175, 0, 0, 171))                        # up, byte stores


def test_crop_inside_the_resized_image(vited, stores):
    _same(*_both(vited, stores, [5, 6, 4], None, 255, 73, 73, 4, 5, 64))                           # the evaluation transform's shape
    _same(*_both(vited, stores, [3, 1], None, 0, 50, 41, 17, 20, 21))                              # a partial last band, odd S


def test_batch_strided_destination(vited, stores):
    dev = stores[0].device
    pairs = torch.full((5, 2, 3, 32, 32), POISON, dtype=torch.uint8, device=dev)
    got, want = _both(vited, stores, [6, 0, 5, 2, 4], None, 0, 32, 32, 0, 0, 32, out=pairs[:, 1])
    _same(got, want)
    assert torch.equal(pairs[:, 1].cpu(), want) and bool((pairs[:, 0] == POISON).all())            # the other half keeps its bytes
    odd = torch.full((3, 3 * 21 * 21 + 5), POISON, dtype=torch.uint8, device=dev)                  # an odd batch stride: byte stores
    view = odd[:, :3 * 21 * 21].view(3, 3, 21, 21)
    got, want = _both(vited, stores, [3, 1, 3], None, 0, 50, 41, 17, 20, 21, out=view)
    _same(got, want)
    assert bool((odd[:, 3 * 21 * 21:] == POISON).all())
    with pytest.raises(ValueError, match='resample_u8: out'):                                      # overlapping samples never reach the library
        vited.ops.resample_u8(stores[0].data, stores[0].offsets_dev, stores[0].sizes_dev, torch.zeros(2, dtype=torch.int32, device=dev), None, 0,
                              vited.ops.resample_tables([5], 16, dev), vited.ops.resample_tables([5], 16, dev), 16, 16, 0, 0, 16,
                              out=torch.empty(1, 3, 16, 16, dtype=torch.uint8, device=dev).expand(2, 3, 16, 16))


@pytest.mark.parametrize('n', (1, 130))
def test_batch_sizes(vited, stores, n):
    _same(*_both(vited, stores, [(3 * k) % 7 for k in range(n)], None, 0, 16, 16, 0, 0, 16))


# ---- the callers --------------------------------------------------------------------------------------------------------------------
def _grid(name, rows, cols):
    return {'Fragment1v1Rotate90': [{'im_path': f'{name}/r{r}c{c}.png', 'row': r, 'col': c, 'degree': 0, 'white_percentage': 0.0}
                                    for r in range(rows) for c in range(cols)]}


def _pajigsaw_model(vited, gpu):
    """The Pajigsaw config from the default tree (pajigsaw_patch16_512.yaml's keys at a toy size), fp32."""
    cfg = vited.config._C.clone()
    cfg.defrost()
    cfg.merge_from_list(['DATA.DATASET', 'pajigsaw', 'DATA.IMG_SIZE', 64, 'MODEL.NUM_CLASSES', 4, 'MODEL.PJS.PATCH_SIZE', 32, 'MODEL.PJS.EMBED_DIM', 32,
                         'MODEL.PJS.NUM_HEADS', 1, 'MODEL.PJS.DEPTH', 1, 'MODEL.PJS.C_DEPTH', 1])
    cfg.freeze()
    torch.manual_seed(0)
    m = vited.build_model(cfg)
    m.compute_dtype = torch.float32
    return m.to(gpu), cfg


def test_loader_feeds_the_train_step(vited, gpu):
    E, S, B = vited.engine, 64, 4
    rng = np.random.default_rng(7)
    index = E.pajigsaw_index({'a': _grid('a', 2, 2), 'b': _grid('b', 1, 3), 'c': _grid('c', 2, 1)})
    frags = [rng.integers(0, 256, size=(s, s, 3), dtype=np.uint8) for s in (64, 200, 90, 512, 33, 100, 128, 71, 300)]
    store = E.Div2kImageStore(frags, gpu)
    loader = E.PajigsawDeviceLoader(store, index, B, S, seed=3)
    batches = list(loader)
    assert len(batches) == len(loader) == 2
    idx, g = loader.rank_indices(), loader._generator(1)
    for b, (pairs, labels) in enumerate(batches):                                                  # the CPU composition of plan and rule
        assert pairs.shape == (B, 2, 3, S, S) and pairs.dtype == torch.uint8 and pairs.is_cuda and pairs.is_contiguous()
        first, second, want_labels = loader.plan(idx[b], g)
        assert torch.equal(labels, want_labels) and labels.dtype == torch.float32
        want = np.stack([np.stack([vited.ops.resample_image(frags[int(f)], S, S).transpose(2, 0, 1) for f in (first[k], second[k])]) for k in range(B)])
        assert np.array_equal(pairs.cpu().numpy(), want), b
    # the step on the loader's batches equals the step on the same bytes handed over directly
    results = []
    for feed in (lambda: E.PajigsawDeviceLoader(store, index, B, S, seed=3), lambda: [(p.clone(), l.clone()) for p, l in batches]):
        m, cfg = _pajigsaw_model(vited, gpu)
        assert cfg.DATA.DATASET == 'pajigsaw' and m.num_classes == 4
        step = E.TrainStep(m, vited.optim.FlatAdamW(E.param_groups_no_decay_1d(m), lr=1e-3, weight_decay=0.05), clip_grad=5.0, amp=False)
        losses = [step.step(pairs, labels).detach().clone() for pairs, labels in feed()]
        results.append((losses, [p.detach().clone() for p in m.parameters()]))
    (la, pa), (lb, pb) = results
    assert len(la) == 2 and all(torch.equal(x, y) for x, y in zip(la, lb)) and all(bool(torch.isfinite(x)) for x in la)
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))


def test_pieces_feed_the_puzzle_distances(vited, gpu):
    E, S = vited.engine, 64
    rng = np.random.default_rng(8)
    pieces = [rng.integers(0, 256, size=(100, 100, 3), dtype=np.uint8) for _ in range(6)]         # a 2 x 3 puzzle
    got = E.pajigsaw_pieces(E.Div2kImageStore(pieces, gpu), S)
    want = torch.from_numpy(np.stack([vited.ops.resample_image(p, S, S).transpose(2, 0, 1) for p in pieces]))
    assert got.shape == (6, 3, S, S) and torch.equal(got.cpu(), want)
    m, _ = _pajigsaw_model(vited, gpu)
    assert torch.equal(E.puzzle_distances(m, got, amp=False), E.puzzle_distances(m, want.to(gpu), amp=False))


def test_sources_feed_the_similarity_run(vited, gpu):
    E, S, s = vited.engine, 64, vo.SHAPE_T
    rng = np.random.default_rng(9)
    images = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((64, 64), (50, 90), (128, 100), (70, 40), (200, 150), (33, 59))]
    dev_store, cpu_store = E.Div2kImageStore(images, gpu), E.Div2kImageStore(images, 'cpu')
    torch.manual_seed(0)
    m = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                      embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads)
    m.compute_dtype = torch.float32
    m = m.to(gpu)
    for source in (E.MichiganEvalSource, E.CenterCropSource):
        src, ref = source(dev_store, S), source(cpu_store, S)
        resident = ref(0, 6).to(gpu)                                                               # the rule's images, pre-transformed
        assert len(src) == 6 and torch.equal(src(0, 6), resident) and torch.equal(src(2, 5), resident[2:5])
        kw = dict(block=4, col_block=4, pair_batch=8, amp=False)
        assert torch.equal(E.pairwise_similarity(m, src, n_images=len(src), **kw), E.pairwise_similarity(m, resident, **kw)), source.__name__
