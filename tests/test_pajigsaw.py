"""The Pajigsaw loader, the parts that need no GPU: the index and the pair plan against what the reference's own ``Pajigsaw`` class
computed on a synthetic data set (tests/golden/pajigsaw_pairs.npz, written by tools/make_pajigsaw_golden.py), the plan's boundaries
and branches, and the loader on a CPU store, where ``ops.resample_u8`` runs the numpy statement of the resize rule."""
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pajigsaw_pairs.npz')
BELOW_ONE = 0.9999999


@pytest.fixture(scope='module')
def golden():
    fx = np.load(GOLDEN)
    return fx, json.loads(bytes(fx['json']).decode())


def _grid(name, rows, cols, white=()):
    return {'Fragment1v1Rotate90': [{'im_path': f'{name}/r{r}c{c}.png', 'row': r, 'col': c, 'degree': 0,
                                     'white_percentage': 0.9 if (r, c) in white else 0.0} for r in range(rows) for c in range(cols)]}


def _lists(ptr, idx, names):
    return [[names[int(i)] for i in idx[int(ptr[k]): int(ptr[k + 1])]] for k in range(len(ptr) - 1)]


def test_the_feature_exists(vited):
    """What fails without the feature (AttributeError): the loader, the kernel's wrapper and the names beside them."""
    assert vited.engine.PajigsawDeviceLoader.__module__.endswith('engine.feeds')
    assert vited.ops.resample_u8.__module__.endswith('ops_resample') and vited.ops.resample_taps.__module__.endswith('ops_resample')
    for name in ('resize_images', 'pajigsaw_pieces', 'pajigsaw_index', 'pajigsaw_pair_plan', 'CenterCropSource', 'MichiganEvalSource'):
        assert callable(getattr(vited.engine, name)), name
    assert 'vited_resample_u8' in vited._lib.SIGNATURES


def test_index_equals_the_reference(vited, golden):
    fx, data = golden
    ix = vited.engine.pajigsaw_index(data)
    degree0 = [f['im_path'] for name in data for f in data[name]['Fragment1v1Rotate90'] if f['degree'] == 0]
    assert ix.im_path == degree0 and len(degree0) == 19 and not any(p.endswith('_90.png') for p in ix.im_path)
    assert [ix.im_path[f] for f in ix.samples.tolist()] == fx['sample_path'].tolist()                        # the order
    assert ix.im_names == fx['im_names'].tolist() == sorted(ix.im_names)
    samples = ix.samples.tolist()
    pos, neg = _lists(ix.pos_ptr, ix.pos_idx, ix.im_path), _lists(ix.neg_ptr, ix.neg_idx, ix.im_path)
    assert [pos[f] for f in samples] == _lists(fx['pos_ptr'], np.arange(len(fx['pos_path'])), fx['pos_path'].tolist())
    assert [neg[f] for f in samples] == _lists(fx['neg_ptr'], np.arange(len(fx['neg_path'])), fx['neg_path'].tolist())
    assert _lists(ix.ent_ptr, ix.ent_idx, ix.im_path) == _lists(fx['ent_ptr'], np.arange(len(fx['ent_path'])), fx['ent_path'].tolist())
    # the fragment table: image numbers follow im_names, rows and columns the file
    by_path = {f['im_path']: (name, f['row'], f['col']) for name in data for f in data[name]['Fragment1v1Rotate90']}
    for f, path in enumerate(ix.im_path):
        name, row, col = by_path[path]
        assert ix.fragment[f].tolist() == [ix.im_names.index(name), row, col]
    # the white fragment is a sample and nobody's second fragment
    white = ix.im_path.index('img_a/r1c1.png')
    assert white in samples and white not in ix.pos_idx.tolist() and white not in ix.neg_idx.tolist()


def test_plan_equals_the_reference(vited, golden):
    fx, data = golden
    ix = vited.engine.pajigsaw_index(data)
    first, second, labels = vited.engine.pajigsaw_pair_plan(torch.from_numpy(fx['u']), torch.from_numpy(fx['case_sample']), ix)
    assert [ix.im_path[f] for f in first.tolist()] == [fx['sample_path'][s] for s in fx['case_sample']]
    assert [ix.im_path[f] for f in second.tolist()] == fx['second_path'].tolist()
    assert labels.dtype == torch.float32 and np.array_equal(labels.numpy(), fx['labels'])
    # the cases reach every branch: all four labels, in-image negatives and other images
    assert {tuple(l) for l in fx['labels'].tolist()} == {(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)}
    zero = ~fx['labels'].any(axis=1)
    same = ix.fragment[first, 0] == ix.fragment[second, 0]
    assert bool(same[torch.from_numpy(zero)].any()) and bool((~same[torch.from_numpy(zero)]).any()) and bool(same[torch.from_numpy(~zero)].all())


def test_plan_boundaries(vited):
    E = vited.engine
    ix = E.pajigsaw_index({'a': _grid('a', 2, 2), 'b': _grid('b', 1, 3), 'c': _grid('c', 2, 1)})
    assert ix.im_names == ['a', 'b', 'c'] and ix.samples.numel() == 9
    plan = lambda s, *u: E.pajigsaw_pair_plan(torch.tensor([u], dtype=torch.float32), torch.tensor([s]), ix)
    s = ix.samples.tolist().index(ix.im_path.index('a/r0c0.png'))
    f, g, l = plan(s, 0.75, 0.1, 0.0, 0.0)                                     # u0 = 0.75 is not positive: the in-image negative
    assert ix.im_path[int(g)] == 'a/r1c1.png' and l.tolist() == [[0, 0, 0, 0]]
    f, g, l = plan(s, 0.7499999, 0.1, 0.0, 0.0)                                # the float32 below 0.75 is
    assert ix.im_path[int(g)] == 'a/r0c1.png' and l.tolist() == [[1, 0, 0, 0]]
    f, g, l = plan(s, 0.1, 0.1, BELOW_ONE, 0.0)                                # u2 just below 1: the last of the list, not past it
    assert ix.im_path[int(g)] == 'a/r1c0.png' and l.tolist() == [[0, 1, 0, 0]]
    f, g, l = plan(s, 0.9, 0.1, BELOW_ONE, 0.0)
    assert ix.im_path[int(g)] == 'a/r1c1.png'                                  # one negative only
    f, g, l = plan(s, 0.9, 0.9, BELOW_ONE, BELOW_ONE)                          # the last entry of the last image
    assert ix.im_path[int(g)] == 'c/r1c0.png' and l.tolist() == [[0, 0, 0, 0]]
    # the other two labels
    s = ix.samples.tolist().index(ix.im_path.index('a/r1c1.png'))
    assert plan(s, 0.1, 0.1, 0.0, 0.0)[2].tolist() == [[0, 0, 0, 1]] and plan(s, 0.1, 0.1, 0.6, 0.0)[2].tolist() == [[0, 0, 1, 0]]
    # a sample without negatives takes the other-image branch also at u1 < 0.5
    s = ix.samples.tolist().index(ix.im_path.index('c/r0c0.png'))
    f, g, l = plan(s, 0.9, 0.1, 0.0, 0.0)
    assert int(ix.neg_ptr[f + 1] - ix.neg_ptr[f]) == 0 and ix.im_path[int(g)] == 'a/r0c0.png' and l.tolist() == [[0, 0, 0, 0]]
    # stepping over the sample's own image: k = floor(u3 (m - 1)) counts the other images
    image_of = lambda g: ix.im_names[int(ix.fragment[int(g), 0])]
    own = {name: ix.samples.tolist().index(ix.im_path.index(f'{name}/r0c0.png')) for name in 'abc'}
    assert [image_of(plan(own['a'], 0.9, 0.9, 0.0, u3)[1]) for u3 in (0.0, 0.49, 0.5, BELOW_ONE)] == ['b', 'b', 'c', 'c']      # own = 0: k at it
    assert [image_of(plan(own['b'], 0.9, 0.9, 0.0, u3)[1]) for u3 in (0.0, 0.49, 0.5, BELOW_ONE)] == ['a', 'a', 'c', 'c']      # k below, k at own
    assert [image_of(plan(own['c'], 0.9, 0.9, 0.0, u3)[1]) for u3 in (0.0, 0.49, 0.5, BELOW_ONE)] == ['a', 'a', 'b', 'b']      # k below own
    # a batch is the rows of its samples
    u = torch.tensor([[0.9, 0.9, 0.0, 0.5], [0.1, 0.1, 0.6, 0.0]])
    f, g, l = E.pajigsaw_pair_plan(u, torch.tensor([own['a'], ix.samples.tolist().index(ix.im_path.index('a/r1c1.png'))]), ix)
    assert [ix.im_path[int(t)] for t in g] == ['c/r0c0.png', 'a/r1c0.png'] and l.tolist() == [[0, 0, 0, 0], [0, 0, 1, 0]]


def test_one_image_is_refused(vited):
    E = vited.engine
    ix = E.pajigsaw_index({'a': _grid('a', 2, 2), 'blank': _grid('blank', 1, 1)})            # the second image has no sample
    assert ix.im_names == ['a'] and ix.fragment[:, 0].tolist() == [0, 0, 0, 0, -1]
    with pytest.raises(ValueError, match='another image'):
        E.pajigsaw_pair_plan(torch.rand(2, 4), torch.tensor([0, 1]), ix)
    store = E.Div2kImageStore([np.zeros((8, 8, 3), np.uint8)] * 5, 'cpu')
    with pytest.raises(ValueError, match='another image'):
        E.PajigsawDeviceLoader(store, ix, 2, 8)


def _cpu_store(vited, data, rng):
    ix = vited.engine.pajigsaw_index(data)
    sides = [int(s) for s in rng.integers(9, 60, size=len(ix.im_path))]
    images = [rng.integers(0, 256, size=(s, s, 3), dtype=np.uint8) for s in sides]
    return vited.engine.Div2kImageStore(images, 'cpu'), ix, images


def test_loader_on_a_cpu_store(vited, golden):
    """Batches equal the composition of the plan and the numpy rule; ranks, seeds and epochs."""
    E, S, B = vited.engine, 16, 4
    store, ix, images = _cpu_store(vited, golden[1], np.random.default_rng(3))
    mk = lambda **kw: E.PajigsawDeviceLoader(store, ix, B, S, **{'seed': 11, **kw})
    loader = mk()
    batches = list(loader)
    assert len(batches) == len(loader) == 19 // B
    idx = loader.rank_indices()
    assert sorted(loader.epoch_order().tolist()) == list(range(19)) and idx.shape == (4, B)
    g = loader._generator(1)
    for b, (pairs, labels) in enumerate(batches):
        assert pairs.shape == (B, 2, 3, S, S) and pairs.dtype == torch.uint8 and labels.shape == (B, 4) and labels.dtype == torch.float32
        first, second, want_labels = loader.plan(idx[b], g)
        assert torch.equal(first, loader.index.samples[idx[b]]) and torch.equal(labels, want_labels)
        for k in range(B):
            for half, frag in enumerate((first, second)):
                want = vited.ops.resample_image(images[int(frag[k])], S, S).transpose(2, 0, 1)
                assert np.array_equal(pairs[k, half].numpy(), want), (b, k, half)
    for (xa, la), (xb, lb) in zip(batches, list(mk())):                            # the same seed and epoch: the same batches
        assert torch.equal(xa, xb) and torch.equal(la, lb)
    loader.set_epoch(1)
    assert not torch.equal(loader.rank_indices(), idx)
    assert not all(torch.equal(xa, xb) for (xa, _), (xb, _) in zip(batches, list(loader)))
    r0, r1 = mk(rank=0, world=2), mk(rank=1, world=2)                              # two ranks: disjoint halves of one permutation
    a, b = r0.rank_indices().flatten().tolist(), r1.rank_indices().flatten().tolist()
    assert len(r0) == len(r1) == 19 // 2 // B and len(a) == len(b) == 8 and not set(a) & set(b)
    order = r0.epoch_order().tolist()
    assert a == order[0::2][:8] and b == order[1::2][:8]
    with pytest.raises(ValueError, match='19 fragments'):
        E.PajigsawDeviceLoader(E.Div2kImageStore(images[:5], 'cpu'), ix, B, S)


def test_resize_images_and_pieces_on_a_cpu_store(vited):
    E, rng = vited.engine, np.random.default_rng(5)
    images = [rng.integers(0, 256, size=(s, s, 3), dtype=np.uint8) for s in (40, 16, 9, 100)]
    store = E.Div2kImageStore(images, 'cpu')
    got = E.resize_images(store, [3, 0, 2], 16)
    assert got.shape == (3, 3, 16, 16) and got.dtype == torch.uint8
    for k, i in enumerate((3, 0, 2)):
        assert np.array_equal(got[k].numpy(), vited.ops.resample_image(images[i], 16, 16).transpose(2, 0, 1))
    assert np.array_equal(got[1].numpy(), E.pajigsaw_pieces(store, 16)[0].numpy()) and E.pajigsaw_pieces(store, 16).shape == (4, 3, 16, 16)
    pairs = torch.full((3, 2, 3, 16, 16), 0xA5, dtype=torch.uint8)
    assert E.resize_images(store, torch.tensor([3, 0, 2]), 16, out=pairs[:, 1]) is not None
    assert torch.equal(pairs[:, 1], got) and bool((pairs[:, 0] == 0xA5).all())
    with pytest.raises(ValueError, match='outside the kernel\'s range'):           # 100 -> 8 shrinks 12.5x: refused on every device
        E.resize_images(store, [0], 8)


def test_a_non_square_fragment_is_refused_by_name(vited, golden):
    E = vited.engine
    store, ix, images = _cpu_store(vited, golden[1], np.random.default_rng(4))
    images[7] = np.zeros((20, 24, 3), np.uint8)
    store = E.Div2kImageStore(images, 'cpu')
    with pytest.raises(ValueError, match=f"'{ix.im_path[7]}' \\(image 7\\) is 20 x 24"):
        E.PajigsawDeviceLoader(store, ix, 4, 16)
    with pytest.raises(ValueError, match='image 7 is 20 x 24'):
        E.resize_images(store, [0, 7], 16)
    assert E.resize_images(store, [0, 1], 16).shape == (2, 3, 16, 16)              # the square ones still go through
