"""Cases and a plain-Python statement of the device pair-mining rule (engine.mine_pairs_device), shared by
tests/test_mine_pairs.py (CPU) and tests/test_gpu_mine_pairs.py.  Not collected by pytest.

``mine_loops`` walks the batch the way the reference's ``prepare_data`` does (hisfrag.py:117-145; michigan.py:120-150 with
``ordered``): for every image i the same-writer images behind it, then the different-writer images behind it (hisfrag) or
anywhere in the row (michigan), lists concatenated in that order - with the reference's ``randperm(len(neg))[:keep]`` replaced by
the key rule: the ``keep`` candidates with the smallest (key, cell), ascending."""
from typing import NamedTuple

import numpy as np
import torch


class Case(NamedTuple):
    name: str
    targets: list
    neg_per_pos: float
    ordered: bool
    positives: int
    candidates: int
    kept: int

    @property
    def pairs(self):
        return self.positives + self.kept


def _blocks(classes, per):
    return [c for c in range(classes) for _ in range(per)]


def _alternating(n, classes):
    return [i % classes for i in range(n)]


CASES = [
    Case('hisfrag_24', _blocks(8, 3), 2.0, False, 24, 252, 48),
    Case('michigan_24', _blocks(8, 3), 1.0, True, 24, 504, 24),
    Case('alternating_7', _alternating(7, 2), 2.0, False, 9, 12, 12),
    Case('all_different_5', list(range(5)), 2.0, False, 0, 10, 0),
    Case('one_class_6', [3] * 6, 2.0, False, 15, 0, 0),
    Case('single_image', [9], 2.0, False, 0, 0, 0),
    Case('two_twins', [0, 0, 1, 1], 2.0, False, 2, 4, 4),
    Case('wide_ids', [-5, 2 ** 40, -5, 7, 2 ** 40, -5], 2.0, False, 4, 11, 8),
    Case('ordered_128', _alternating(128, 2), 2.0, True, 4032, 8192, 8064),
    Case('upper_128', _alternating(128, 2), 2.0, False, 4032, 4096, 4096),
]
# cell counts that are no power of two and leave part of a wave idle (GPU table only: 49 and 36 cells)
EXTRA_GPU_CASES = [
    Case('cells_49', [0, 1, 0, 2, 1, 0, 2], 2.0, True, 5, 32, 10),
    Case('cells_36', _alternating(6, 2), 2.0, False, 6, 9, 9),
]
BY_NAME = {c.name: c for c in CASES + EXTRA_GPU_CASES}


def capacities(case):
    """(label, capacity): exact, five padding rows, one that cuts into the negatives (where there are at least two)."""
    out = [('exact', max(case.pairs, 1)), ('padded', case.pairs + 5)]
    if case.kept > 1:
        out.append(('cut_negatives', case.pairs - case.kept // 2))
    return out


def make_keys(n, seed, levels=None):
    """fp32 [n * n] in [0, 1): seeded uniforms; ``levels``: quantised to that many values (ties); 0: all zero."""
    if levels == 0:
        return torch.zeros(n * n)
    u = torch.rand(n * n, generator=torch.Generator().manual_seed(seed))
    return u if levels is None else torch.floor(u * levels) / levels


def mine_loops(targets, keys, neg_per_pos, ordered, capacity):
    """dict of numpy arrays: groups, labels, weights, counts, seg_index, seg_order, seg_offsets."""
    t = [int(v) for v in targets]
    key = np.asarray(keys, dtype=np.float32).reshape(-1)
    n = len(t)
    pos, neg = [], []
    for i in range(n):
        for j in range(i + 1, n):
            if t[j] == t[i]:
                pos.append((i, j))
        for j in (range(n) if ordered else range(i + 1, n)):
            if t[j] != t[i]:
                neg.append((i, j))
    keep = min(len(neg), int(neg_per_pos * len(pos)))
    chosen = sorted(neg, key=lambda p: (key[p[0] * n + p[1]], p[0] * n + p[1]))[:keep]
    pos_rows = min(len(pos), capacity)
    neg_rows = min(keep, capacity - pos_rows)
    rows = pos[:pos_rows] + chosen[:neg_rows]
    groups = np.zeros((capacity, 2), dtype=np.int64)
    labels = np.zeros((capacity, 1), dtype=np.float32)
    weights = np.zeros((capacity, 1), dtype=np.float32)
    for r, (i, j) in enumerate(rows):
        groups[r] = (i, j)
        labels[r, 0] = 1.0 if r < pos_rows else 0.0
        weights[r, 0] = 1.0
    by_item = [[] for _ in range(n)]                 # ascending row number inside an item
    for r, j in enumerate(groups[:, 1].tolist()):
        by_item[j].append(r)
    order, offsets = [], [0]
    for g in range(n):
        order += by_item[g]
        offsets.append(len(order))
    return dict(groups=groups, labels=labels, weights=weights,
                counts=np.array([len(pos), len(neg), neg_rows, len(rows), len(pos) + keep - len(rows)], dtype=np.int32),
                seg_index=groups[:, 1].copy(), seg_order=np.array(order, dtype=np.int64), seg_offsets=np.array(offsets, dtype=np.int64))


def as_numpy(mined):
    """The same dict from an ``engine.MinedPairs`` (any device)."""
    c = lambda x: x.detach().cpu().numpy()
    return dict(groups=c(mined.groups), labels=c(mined.labels), weights=c(mined.weights), counts=c(mined.counts),
                seg_index=c(mined.segments.index), seg_order=c(mined.segments.order), seg_offsets=c(mined.segments.offsets))


def assert_same(got, want, what=''):
    for name in ('counts', 'groups', 'labels', 'weights', 'seg_index', 'seg_order', 'seg_offsets'):
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (what, name, got[name].dtype, got[name].shape)
        assert np.array_equal(got[name], want[name]), f'{what}: {name} differs'
