"""CPU: the index tables of the pair-indexed decoder (ops.pair_segments), michigan's mining rule (mine_pairs(ordered_negatives=True))
and the header binding of vited_attention_bwd_indexed.  No kernel runs here."""
import ctypes

import numpy as np
import pytest
import torch


def _numpy_segments(index, items):
    index = np.asarray(index, dtype=np.int64)
    order = np.argsort(index, kind='stable')
    offsets = np.concatenate([[0], np.cumsum(np.bincount(index, minlength=items))]).astype(np.int64)
    return order, offsets


@pytest.mark.parametrize('index,items', [([2, 0, 2, 2, 0], 3),          # an item nobody reads, three pairs on one item
                                         ([3, 1, 0, 2], 4),             # a permutation
                                         ([1, 1, 1, 1], 2),             # all equal, item 0 empty
                                         ([0, 0, 0], 1),
                                         ([4], 7),                      # empty items on both sides
                                         ([], 3)])                      # no pairs at all
def test_pair_segments_against_numpy(vited, index, items):
    seg = vited.ops.pair_segments(torch.tensor(index, dtype=torch.int64), items)
    order, offsets = _numpy_segments(index, items)
    assert isinstance(seg, vited.ops.PairSegments) and seg.items == items
    assert seg.index.dtype == seg.order.dtype == seg.offsets.dtype == torch.int64
    assert seg.index.tolist() == list(index)
    assert seg.order.tolist() == order.tolist()
    assert seg.offsets.tolist() == offsets.tolist()
    # the grouping the kernel walks: item g's pairs in ascending pair order
    for g in range(items):
        group = seg.order[seg.offsets[g]:seg.offsets[g + 1]].tolist()
        assert group == [p for p, i in enumerate(index) if i == g]


def test_pair_segments_takes_int32_and_rejects_bad_indices(vited):
    ops = vited.ops
    seg = ops.pair_segments(torch.tensor([2, 0, 2, 2, 0], dtype=torch.int32), 3)
    assert seg.index.dtype == torch.int64 and seg.order.tolist() == [1, 4, 0, 2, 3] and seg.offsets.tolist() == [0, 2, 2, 5]
    with pytest.raises(ValueError, match=r'outside \[0, 3\)'):
        ops.pair_segments(torch.tensor([0, -1, 2]), 3)
    with pytest.raises(ValueError, match=r'outside \[0, 3\)'):
        ops.pair_segments(torch.tensor([0, 3, 2]), 3)
    with pytest.raises(ValueError):
        ops.pair_segments(torch.tensor([0]), 0)
    with pytest.raises(ValueError):
        ops.pair_segments(torch.tensor([[0, 1]]), 3)
    with pytest.raises(ValueError):
        ops.pair_segments(torch.tensor([0.0, 1.0]), 3)


def _michigan_rule(targets):
    """michigan.py:120-155 restated: row i pairs with every LATER sample of its label (positives) and with EVERY sample of another
    label (negative candidates, both orders); min(#candidates, #positives) candidates are kept at random."""
    t = targets.tolist()
    n = len(t)
    pos = [(i, j) for i in range(n) for j in range(i + 1, n) if t[j] == t[i]]
    cand = [(i, j) for i in range(n) for j in range(n) if t[j] != t[i]]
    return pos, cand, min(len(cand), len(pos))


@pytest.mark.parametrize('n,classes', [(24, 8), (7, 2), (5, 5)])
def test_mine_pairs_ordered_negatives_is_michigans_rule(vited, n, classes):
    targets = torch.arange(n) % classes
    targets = targets[torch.randperm(n, generator=torch.Generator().manual_seed(n))]
    pos, cand, keep = _michigan_rule(targets)
    g = torch.Generator().manual_seed(3)
    groups, labels = vited.engine.mine_pairs(targets, neg_per_pos=1.0, generator=g, ordered_negatives=True)
    got = [tuple(r) for r in groups.tolist()]
    assert got[:len(pos)] == pos                                     # same positives in the same order
    neg = got[len(pos):]
    assert len(neg) == keep and len(set(neg)) == len(neg) and set(neg) <= set(cand)
    assert labels.view(-1).tolist() == [1.] * len(pos) + [0.] * keep and labels.shape == (len(got), 1)
    if classes < n and classes > 1:
        # both orders are candidates: with every candidate kept (a huge neg_per_pos) the set is the whole candidate list, in row-major order
        every, _ = vited.engine.mine_pairs(targets, neg_per_pos=1e9, generator=g, ordered_negatives=True)
        assert sorted(tuple(r) for r in every.tolist()[len(pos):]) == cand


def test_mine_pairs_default_is_unchanged(vited):
    """The default keeps hisfrag.py's rule: upper-triangle candidates, 2 negatives per positive, the same draw from the same seed."""
    targets = torch.arange(8).repeat_interleave(3)
    a, la = vited.engine.mine_pairs(targets, generator=torch.Generator().manual_seed(1))
    b, lb = vited.engine.mine_pairs(targets, generator=torch.Generator().manual_seed(1), ordered_negatives=False)
    assert torch.equal(a, b) and torch.equal(la, lb)
    assert a.shape == (72, 2) and bool((a[:, 0] < a[:, 1]).all())     # 24 positives + 48 negatives, all with i < j
    i, j = torch.triu_indices(24, 24, offset=1)
    neg = torch.stack([i, j], 1)[targets[i] != targets[j]]
    perm = torch.randperm(neg.shape[0], generator=torch.Generator().manual_seed(1))[:48]
    assert torch.equal(a[24:], neg[perm])


def test_header_binding_knows_the_indexed_backward(vited):
    sigs, C = vited._lib.SIGNATURES, ctypes
    p, i, i64, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    assert sigs['vited_attention_bwd_indexed_workspace_bytes'] == (i64, [i, i64, i, i64, i])
    assert sigs['vited_attention_bwd_indexed'] == (i, [p, i64, i64, p, i64, i64, p, i64, i64,      # q, k, v
                                                       p, p, p, i64,                               # kv_index, seg_order, seg_offsets, kv_items
                                                       p, p, i64, i64, p, p,                       # o, d_o, o_bs, o_ts, lse, delta
                                                       p, i64, i64, p, i64, i64, p, i64, i64,      # dq, dk, dv
                                                       i, i64, i, i64, i64, i, f,                  # dtype, batch, heads, nq, nk, head_dim, scale
                                                       p, i64, p])                                 # workspace, workspace_bytes, stream
    # the backward takes vited_attention_bwd's arguments plus the three tables, the item count and the workspace
    assert len(sigs['vited_attention_bwd_indexed'][1]) == len(sigs['vited_attention_bwd'][1]) + 6


def test_indexed_backward_validates_before_any_launch(vited):
    lib = vited._lib.load()
    wsb = lib.vited_attention_bwd_indexed_workspace_bytes
    assert wsb(vited._lib.BF16, 72, 6, 1024, 64) == 72 * 1024 * 2 * 384 * 2      # one [Nk, dK | dV] slab per pair, operand dtype
    assert wsb(vited._lib.F32, 5, 12, 64, 32) == 5 * 64 * 2 * 384 * 4
    assert wsb(vited._lib.F16, 5, 12, 64, 32) == -1 and wsb(vited._lib.F32, 0, 12, 64, 32) == -1
    null = [None, 0, 0] * 3 + [None, None, None, 3] + [None, None, 0, 0, None, None] + [None, 0, 0] * 3
    assert lib.vited_attention_bwd_indexed(*null, vited._lib.F32, 5, 12, 65, 64, 32, 0.5, None, 0, None) == 1     # VITED_ERR_BAD_ARG
