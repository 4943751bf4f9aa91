"""CPU: the device pair-mining rule (engine.mine_pairs_device on CPU tensors) against the plain-Python loops
of tests/mine_cases.py, exactly; its consistency with engine.mine_pairs and ops.pair_segments; the capacity arithmetic, the loss,
the binding and the argument checks.  No GPU is used."""
import ctypes

import numpy as np
import pytest
import torch

import mine_cases as mc


def _mine(E, case, capacity, keys):
    return E.mine_pairs_device(torch.tensor(case.targets), capacity, neg_per_pos=case.neg_per_pos, ordered_negatives=case.ordered, keys=keys)


@pytest.mark.parametrize('case', mc.CASES, ids=lambda c: c.name)
def test_restated_rule_against_the_loops(vited, case):
    E, n = vited.engine, len(case.targets)
    keys = mc.make_keys(n, seed=n)
    for label, capacity in mc.capacities(case):
        got = mc.as_numpy(_mine(E, case, capacity, keys))
        want = mc.mine_loops(case.targets, keys, case.neg_per_pos, case.ordered, capacity)
        mc.assert_same(got, want, f'{case.name} {label}')
        found = (int(got['counts'][0]), int(got['counts'][1]))
        assert found == (case.positives, case.candidates), found
        if label != 'cut_negatives':
            assert tuple(got['counts'][2:]) == (case.kept, case.pairs, 0)
            assert float(got['weights'].sum()) == case.pairs and float(got['labels'].sum()) == case.positives
        else:
            assert tuple(got['counts'][2:]) == (case.kept - case.kept // 2, capacity, case.kept // 2)
            assert float(got['weights'].sum()) == capacity
        assert not got['groups'][int(got['counts'][3]):].any()         # padding rows are pair (0, 0)


def test_capacity_that_cuts_into_the_positives(vited):
    case = mc.BY_NAME['hisfrag_24']
    keys = mc.make_keys(24, seed=1)
    got = mc.as_numpy(_mine(vited.engine, case, 20, keys))
    mc.assert_same(got, mc.mine_loops(case.targets, keys, 2.0, False, 20), 'cut into the positives')
    assert tuple(got['counts']) == (24, 252, 0, 20, 52) and float(got['labels'].sum()) == 20
    full = mc.as_numpy(_mine(vited.engine, case, 72, keys))
    assert np.array_equal(got['groups'], full['groups'][:20])          # positives are dropped from the end


def test_equal_keys_go_to_the_lower_cell(vited):
    case = mc.BY_NAME['two_twins']
    got = _mine(vited.engine, case, 6, mc.make_keys(4, seed=0, levels=0))
    assert got.groups.tolist() == [[0, 1], [2, 3], [0, 2], [0, 3], [1, 2], [1, 3]]
    assert got.labels.flatten().tolist() == [1, 1, 0, 0, 0, 0] and got.weights.flatten().tolist() == [1] * 6


@pytest.mark.parametrize('name', ['hisfrag_24', 'michigan_24', 'alternating_7', 'wide_ids', 'ordered_128'])
def test_keys_quantised_to_four_values(vited, name):
    case = mc.BY_NAME[name]
    keys = mc.make_keys(len(case.targets), seed=3, levels=4)
    assert torch.unique(keys).numel() <= 4
    for label, capacity in mc.capacities(case):
        mc.assert_same(mc.as_numpy(_mine(vited.engine, case, capacity, keys)),
                       mc.mine_loops(case.targets, keys, case.neg_per_pos, case.ordered, capacity), f'{name} {label}')


@pytest.mark.parametrize('case', mc.CASES, ids=lambda c: c.name)
def test_consistent_with_mine_pairs_and_pair_segments(vited, case):
    E, n = vited.engine, len(case.targets)
    t = torch.tensor(case.targets)
    mined = E.mine_pairs_device(t, max(case.pairs, 1), neg_per_pos=case.neg_per_pos, ordered_negatives=case.ordered, keys=mc.make_keys(n, seed=5))
    groups, labels = E.mine_pairs(t, neg_per_pos=case.neg_per_pos, generator=torch.Generator().manual_seed(0), ordered_negatives=case.ordered)
    p = case.positives
    assert int(labels.sum()) == p and groups.shape[0] == case.pairs
    assert torch.equal(mined.groups[:p], groups[:p])                   # the positives: the same set in the same order
    ours = {tuple(r) for r in mined.groups[p:case.pairs].tolist()}
    assert len(ours) == case.kept == groups.shape[0] - p               # no duplicates, as many as mine_pairs keeps
    i, j = mined.groups[p:case.pairs, 0], mined.groups[p:case.pairs, 1]
    assert bool((t[i] != t[j]).all()) and (case.ordered or bool((i < j).all()))      # a subset of its candidate set
    seg = vited.ops.pair_segments(mined.groups[:, 1].contiguous(), n)
    for a, b in zip(mined.segments, seg):
        assert a.dtype == b.dtype and torch.equal(a, b)


def test_default_keys_are_drawn_from_the_generator(vited):
    E, t = vited.engine, torch.tensor(mc.BY_NAME['hisfrag_24'].targets)
    a = E.mine_pairs_device(t, 72, generator=torch.Generator().manual_seed(4))
    b = E.mine_pairs_device(t, 72, keys=torch.rand(576, generator=torch.Generator().manual_seed(4)))
    c = E.mine_pairs_device(t, 72, generator=torch.Generator().manual_seed(5))
    assert torch.equal(a.groups, b.groups) and not torch.equal(a.groups, c.groups)
    assert torch.equal(a.groups[:24], c.groups[:24])


def test_mined_pair_capacity(vited):
    cap = vited.engine.mined_pair_capacity
    assert cap(24, 3) == 72 and cap(24, 3, neg_per_pos=1.0, ordered_negatives=True) == 48
    assert cap(128, 64) == 8128 and cap(128, 64, ordered_negatives=True) == 12096
    assert cap(6, 6) == 15 and cap(5, 1) == 1 and cap(1) == 1
    with pytest.raises(ValueError):
        cap(24, 5)
    # the worst case over all labelings, against brute force over every labeling of 6 images
    for ordered, ratio in ((False, 2.0), (True, 1.0), (True, 2.0), (False, 0.5)):
        worst = 1
        for code in range(6 ** 5):
            labels = [0] + [(code // 6 ** k) % 6 for k in range(5)]
            pos = sum(labels[i] == labels[j] for i in range(6) for j in range(i + 1, 6))
            cand = (15 - pos) * (2 if ordered else 1)
            worst = max(worst, pos + min(cand, int(ratio * pos)))
        assert cap(6, neg_per_pos=ratio, ordered_negatives=ordered) == worst
    for case in mc.CASES:                                                # never below what a batch of the table needs
        assert cap(len(case.targets), neg_per_pos=case.neg_per_pos, ordered_negatives=case.ordered) >= case.pairs


def test_mined_bce_with_logits_is_the_loss_of_the_valid_rows(vited):
    E, case = vited.engine, mc.BY_NAME['alternating_7']
    for capacity in (21, 26, 15):
        mined = _mine(E, case, capacity, mc.make_keys(7, seed=2))
        rows = int(mined.counts[3])
        logits = (torch.randn(capacity, 1, generator=torch.Generator().manual_seed(capacity)) * 3).requires_grad_(True)
        for reduction in ('mean', 'sum'):
            want = torch.nn.BCEWithLogitsLoss(reduction=reduction)(logits[:rows], mined.labels[:rows])
            got = E.mined_bce_with_logits(logits, mined, reduction=reduction)
            assert got.dtype == torch.float32 and got.dim() == 0
            torch.testing.assert_close(got, want)
            grad, = torch.autograd.grad(got, logits)
            torch.testing.assert_close(grad[:rows], torch.autograd.grad(want, logits)[0][:rows])
            assert not grad[rows:].any()                                 # padding rows: exact zeros
    empty = _mine(E, mc.BY_NAME['single_image'], 3, torch.zeros(1))
    assert float(E.mined_bce_with_logits(torch.ones(3, 1), empty)) == 0.0
    with pytest.raises(ValueError):
        E.mined_bce_with_logits(torch.ones(3, 1), empty, reduction='none')


def test_header_binding_carries_the_new_symbols(vited):
    sigs, C = vited._lib.SIGNATURES, ctypes
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    assert sigs['vited_mine_pairs_max_images'] == (i, [])
    assert sigs['vited_mine_pairs'] == (i, [p, i, p, C.c_double, i, i64, p, p, p, p, p, p, p, p])
    lib = vited._lib.load()
    assert lib.vited_mine_pairs_max_images() == 128 == vited.ops.mine_pairs_max_images()
    null = [None] * 7
    assert lib.vited_mine_pairs(None, 4, None, 2.0, 0, 6, *null, None) == 1          # null pointers: bad argument, nothing launched


def test_argument_checks_raise_before_any_launch(vited, monkeypatch):
    ops, E = vited.ops, vited.engine

    def no_launch(*a, **k):
        raise AssertionError('a bad argument reached the launch')

    monkeypatch.setattr(vited._lib, 'call', no_launch)
    t, k = torch.zeros(4, dtype=torch.int64), torch.zeros(16)
    bad = [(t.int(), k, 2.0, 6), (t, k.double(), 2.0, 6), (t, k[:15], 2.0, 6), (t, torch.zeros(32)[::2], 2.0, 6), (t.view(2, 2), k, 2.0, 6),
           (t, k, 2.0, 0), (t, k, -1.0, 6), (t, k, float('nan'), 6), (t[:0], k[:0], 2.0, 6),
           (t, k, 2.0, 6)]                                               # the last one: CPU tensors never reach the kernel
    for targets, keys, ratio, capacity in bad:
        with pytest.raises(ValueError):
            ops.mine_pairs(targets, keys, ratio, False, capacity)
    with pytest.raises(ValueError):
        E.mine_pairs_device(t, 0)
    with pytest.raises(ValueError):
        E.mine_pairs_device(t, 6, keys=torch.zeros(15))
    with pytest.raises(ValueError):
        E.mine_pairs_device(t, 6, neg_per_pos=-2.0)
    assert E.mine_pairs_device(torch.zeros(200, dtype=torch.int64), 4, keys=torch.zeros(40000)).counts.tolist() == [19900, 0, 0, 4, 19896]
