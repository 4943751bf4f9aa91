"""Pair mining for the two-stage training step (hisfrag.py:117-159): ``mine_pairs`` with a host read per
step, ``mine_pairs_device`` with a fixed shape, none, and a rule restated on the CPU; their loss - as torch ops
and as one HIP launch (``mined_bce_fused``) - and hand-offs."""
from __future__ import annotations

import functools
from typing import NamedTuple

import torch

from .. import ops


def mine_pairs(targets: torch.Tensor, neg_per_pos: float = 2.0, generator=None, ordered_negatives: bool = False):
    """(groups int64 [P, 2], labels fp32 [P, 1]): every same-label pair (i, j), j > i, in row-major order, then a
    random subset of the different-label pairs of size min(#neg, int(neg_per_pos * #pos)) - what
    ``HisfragTrainer.prepare_data`` (hisfrag.py:117-145) builds with a Python loop over the batch and 2n
    ``nonzero`` host syncs.  Here: one ``triu_indices`` + two boolean selects on the device (the pair count is
    data-dependent, so one host sync per step remains).
    ``ordered_negatives``: the negative candidates are ALL ordered pairs (i, j), i != j, with different labels, row-major
    (michigan.py:142-148 scans the whole row, not its upper half); with ``neg_per_pos=1.0`` that is michigan's rule
    (michigan.py:150).  The positives are the upper-triangle pairs either way."""
    t = targets.reshape(-1)
    n = t.numel()
    i, j = torch.triu_indices(n, n, offset=1, device=t.device)
    same = t[i] == t[j]
    pos = torch.stack([i[same], j[same]], dim=1)
    if ordered_negatives:
        neg = torch.nonzero(t.view(-1, 1) != t.view(1, -1))            # row-major: i outer, j ascending
    else:
        neg = torch.stack([i[~same], j[~same]], dim=1)
    keep = min(neg.shape[0], int(neg_per_pos * pos.shape[0]))
    perm = torch.randperm(neg.shape[0], generator=generator, device=neg.device if generator is None else generator.device)[:keep]
    neg = neg[perm.to(neg.device)]
    groups = torch.cat([pos, neg], dim=0)
    labels = torch.cat([torch.ones(pos.shape[0], device=t.device), torch.zeros(neg.shape[0], device=t.device)]).view(-1, 1)
    return groups, labels


def hisfrag_prepare_data(model, samples: torch.Tensor, targets: torch.Tensor, amp: bool = True, generator=None):
    """The first half of the reference's two-stage step (hisfrag.py:117-155): mine pairs, run the encoder ONCE per
    image, gather.  Returns ((x, x1_feats), labels) for ``model(x1_feats, x)`` exactly like the reference's
    ``prepare_data`` -> ``train_step`` hand-off (hisfrag.py:153-159)."""
    groups, labels = mine_pairs(targets, generator=generator)
    with torch.autocast(samples.device.type, dtype=torch.bfloat16, enabled=amp):
        feats = model(samples, forward_first_part=True)
    return (samples[groups[:, 0]], feats[groups[:, 1]]), labels


def hisfrag_prepare_indexed(model, samples: torch.Tensor, targets: torch.Tensor, amp: bool = True, generator=None, neg_per_pos: float = 2.0,
                            ordered_negatives: bool = False):
    """``hisfrag_prepare_data`` without its two gathers: returns ((samples, feats, x2_index, x1_index), labels) with
    x2_index = groups[:, 0] (int64 [P]) and x1_index = ops.pair_segments(groups[:, 1], n) - what hisfrag.py:153-154 gathers - for
    ``model(feats, samples, x2_index=x2_index, x1_index=x1_index)``.  The decoder then embeds image 2 through the index, projects
    the cross-attention keys / values once per IMAGE and sums every image's key / value gradient over its pairs in a fixed order:
    the step is bitwise reproducible, which the gathered form (an atomic scatter-add in ``feats[index]``'s backward) is not.
    ``neg_per_pos`` / ``ordered_negatives``: ``mine_pairs``' rule (1.0 / True: michigan.py:150)."""
    groups, labels = mine_pairs(targets, neg_per_pos=neg_per_pos, generator=generator, ordered_negatives=ordered_negatives)
    with torch.autocast(samples.device.type, dtype=torch.bfloat16, enabled=amp):
        feats = model(samples, forward_first_part=True)
    x2_index = groups[:, 0].contiguous()
    return (samples, feats, x2_index, ops.pair_segments(groups[:, 1], samples.shape[0])), labels


class MinedPairs(NamedTuple):
    """What ``mine_pairs_device`` returns: ``capacity`` rows - positives, kept negatives, padding."""
    groups: torch.Tensor      # int64 [capacity, 2]: (image 2, image 1) like ``mine_pairs``; a padding row is (0, 0)
    labels: torch.Tensor      # fp32 [capacity, 1]: 1 same writer, 0 different (and padding)
    weights: torch.Tensor     # fp32 [capacity, 1]: 1 for a pair, 0 for a padding row
    segments: 'ops.PairSegments'   #  of groups[:, 1] over the batch's images
    counts: torch.Tensor      # int32 [5]: positives, candidates, negatives emitted, pairs emitted, pairs dropped (capacity)


def _mine_pairs_restated(t, keys, neg_per_pos, ordered_negatives, capacity):
    """The rule of ``mine_pairs_device`` in plain torch (any device; used for CPU tensors)."""
    n, dev = t.numel(), t.device
    same = t.view(-1, 1) == t.view(1, -1)
    upper = torch.ones(n, n, dtype=torch.bool, device=dev).triu(1)
    pos = torch.nonzero(same & upper)                                  # row-major = ascending cell
    is_cand = ~same if ordered_negatives else ~same & upper
    cand = torch.nonzero(is_cand)
    keep = max(min(cand.shape[0], int(neg_per_pos * pos.shape[0])), 0)
    by_key = torch.argsort(keys.view(n, n)[is_cand], stable=True)      # equal keys: the lower cell first
    pos_rows = min(pos.shape[0], capacity)
    neg_rows = min(keep, capacity - pos_rows)
    rows = pos_rows + neg_rows
    groups = torch.zeros(capacity, 2, dtype=torch.int64, device=dev)
    labels, weights = (torch.zeros(capacity, 1, dtype=torch.float32, device=dev) for _ in range(2))
    groups[:pos_rows] = pos[:pos_rows]
    groups[pos_rows:rows] = cand[by_key[:neg_rows]]
    labels[:pos_rows] = 1.0
    weights[:rows] = 1.0
    counts = torch.tensor([pos.shape[0], cand.shape[0], neg_rows, rows, pos.shape[0] + keep - rows], dtype=torch.int32, device=dev)
    return MinedPairs(groups, labels, weights, ops.pair_segments(groups[:, 1].contiguous(), n), counts)


def mine_pairs_device(targets: torch.Tensor, capacity: int, neg_per_pos: float = 2.0, generator=None, ordered_negatives: bool = False,
                      keys: torch.Tensor | None = None) -> MinedPairs:
    """``mine_pairs`` with a fixed-shape result and no host read: ``capacity`` rows whatever the batch holds.

    Positives: every (i, j), i < j, of one writer, row-major - ``mine_pairs``' set and order.  Negatives: of the different-writer
    cells (i < j; every i != j with ``ordered_negatives``, michigan.py:142-148) the min(#candidates, int(neg_per_pos * #positives))
    with the smallest key, ``keys`` fp32 [n * n] in [0, 1) holding one key per ordered cell i * n + j; in ascending (key, cell)
    order.  With i.i.d. uniform keys that subset has the distribution of ``randperm(#candidates)[:keep]``; two keys that are equal
    at fp32 resolution go to the lower cell.  Then padding rows (0, 0) with label 0 and weight 0.  Pairs beyond ``capacity`` are
    dropped, negatives from the end first, and ``counts[4]`` says how many.

    On a GPU tensor: ``keys`` are drawn with ``torch.rand`` on the device unless given (from ``generator``, or the device's default
    generator, which a graph capture registers), then one kernel (``ops.mine_pairs``; at most 128 images): capturable.  On a CPU
    tensor: the same rule in plain torch, without the 128-image limit - identical results for identical keys."""
    t = targets.reshape(-1).to(torch.int64).contiguous()
    n, capacity = t.numel(), int(capacity)
    if n < 1 or capacity < 1:
        raise ValueError(f'mine_pairs_device: {n} images, capacity {capacity}: both must be at least 1')
    if keys is None:
        keys = torch.rand(n * n, generator=generator, device=t.device if generator is None else generator.device).to(t.device)
    if keys.dtype != torch.float32 or keys.numel() != n * n or keys.device != t.device:
        raise ValueError(f'mine_pairs_device: keys must be {n * n} float32 values on {t.device}, got {keys.dtype} {tuple(keys.shape)} '
                         f'on {keys.device}')
    neg_per_pos = float(neg_per_pos)
    if not 0.0 <= neg_per_pos < float('inf'):
        raise ValueError(f'mine_pairs_device: neg_per_pos must be a finite number >= 0, got {neg_per_pos}')
    keys = keys.reshape(-1).contiguous()
    if t.is_cuda:
        return MinedPairs(*ops.mine_pairs(t, keys, neg_per_pos, ordered_negatives, capacity))
    return _mine_pairs_restated(t, keys, neg_per_pos, bool(ordered_negatives), capacity)


@functools.lru_cache(maxsize=None)
def _reachable_positive_counts(n: int) -> int:
    """Bit p is set when some labeling of n images has p same-label pairs (i < j): the sums of s (s - 1) / 2 over the class
    sizes of a partition of n."""
    reach = [0] * (n + 1)
    reach[0] = 1
    for s in range(1, n + 1):
        for total in range(0, n - s + 1):          # ascending: a class size may repeat
            if reach[total]:
                reach[total + s] |= reach[total] << (s * (s - 1) // 2)
    return reach[n]


def mined_pair_capacity(n: int, m: int | None = None, neg_per_pos: float = 2.0, ordered_negatives: bool = False) -> int:
    """Rows ``mine_pairs_device`` needs for a batch of ``n`` images (host arithmetic only; at least 1).  With ``m``: the exact
    pair count of n / m distinct classes of m images each, the batch ``MPerClassSampler`` aims for - (24, 3) gives 72, and 48
    under michigan's rule (neg_per_pos 1, ordered).  Without: the largest count over ALL labelings of n images (every partition's
    positive count is tried), so that nothing is ever dropped."""
    n, cells = int(n), int(n) * (int(n) - 1) // 2
    if n < 1:
        raise ValueError(f'mined_pair_capacity: {n} images')

    def pairs(pos):
        cand = 2 * (cells - pos) if ordered_negatives else cells - pos
        return pos + max(min(cand, int(neg_per_pos * pos)), 0)

    if m is not None:
        m = int(m)
        if m < 1 or n % m:
            raise ValueError(f'mined_pair_capacity: {n} images are no multiple of m = {m}')
        return max(pairs(n // m * (m * (m - 1) // 2)), 1)
    reach, best, pos = _reachable_positive_counts(n), 1, 0
    while reach:
        if reach & 1:
            best = max(best, pairs(pos))
        reach >>= 1
        pos += 1
    return best


def mined_bce_with_logits(logits: torch.Tensor, mined: MinedPairs, reduction: str = 'mean') -> torch.Tensor:
    """BCE-with-logits over the valid rows of a ``MinedPairs``: 'mean' = sum(weights * bce) / max(counts[3], 1) (what
    ``BCEWithLogitsLoss()`` gives on the real pairs, hisfrag.py), 'sum' = the weighted sum (michigan.py's reduction).  ``logits``
    [capacity] or [capacity, C]; with C > 1 outputs every column takes the pair's label and the mean divides by C as well.  Plain
    torch on the logits' device, fp32, no host read; a padding row has weight 0 and contributes exact zeros to the loss and to
    every gradient.  Usable as ``TrainStep(criterion=mined_bce_with_logits)`` with ``y = mined``."""
    if reduction not in ('mean', 'sum'):
        raise ValueError(f"mined_bce_with_logits: reduction must be 'mean' or 'sum', got {reduction!r}")
    x = logits.float()
    x = x.unsqueeze(1) if x.dim() == 1 else x
    if x.dim() != 2 or x.shape[0] != mined.labels.shape[0]:
        raise ValueError(f'mined_bce_with_logits: logits {tuple(logits.shape)} for {mined.labels.shape[0]} mined rows')
    total = torch.nn.functional.binary_cross_entropy_with_logits(x, mined.labels.expand_as(x), weight=mined.weights.expand_as(x),
                                                                 reduction='sum')
    if reduction == 'sum':
        return total
    return total / (mined.counts[3].clamp(min=1).to(torch.float32) * x.shape[1])


class _MinedBCEFused(torch.autograd.Function):
    """``ops.mined_bce`` under autograd: the launch that forms the loss also forms d loss / d logits, the backward only scales it."""

    @staticmethod
    def forward(ctx, logits, labels, weights, counts, reduction, scale):
        loss, dlogits = ops.mined_bce(logits, labels, weights, counts, reduction, scale)
        ctx.save_for_backward(dlogits)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        (dlogits,) = ctx.saved_tensors
        return grad_output * dlogits, None, None, None, None, None


def mined_bce_fused(logits: torch.Tensor, mined: MinedPairs, reduction: str = 'mean', scale: float = 1.0) -> torch.Tensor:
    """``scale * mined_bce_with_logits(logits, mined, reduction)`` from one HIP launch (``ops.mined_bce``, csrc/mined_bce.hip) that writes
    the loss and its gradient together; the backward is ``grad_output * dlogits``, one elementwise device op.  No host read in either
    direction (the pair count is read on the device): capturable.  ``logits`` [capacity] or [capacity, C], C <= 64, on the GPU; ``scale``
    is the step's 1 / accumulation_steps.  The sum runs in a fixed order, so the loss and the gradient are bitwise reproducible and the
    loss bits do not depend on the capacity.  Usable as ``TrainStep(criterion=mined_bce_fused)`` with ``y = mined``."""
    x = logits.float()
    x = x.unsqueeze(1) if x.dim() == 1 else x
    return _MinedBCEFused.apply(x.contiguous(), mined.labels, mined.weights, mined.counts, reduction, float(scale))


def hisfrag_prepare_mined(model, samples: torch.Tensor, targets: torch.Tensor, capacity: int, amp: bool = True, generator=None,
                          neg_per_pos: float = 2.0, ordered_negatives: bool = False):
    """``hisfrag_prepare_indexed`` on ``mine_pairs_device``: returns ((samples, feats, x2_index, segments), mined) for
    ``model(feats, samples, x2_index=x2_index, x1_index=segments)`` and ``mined_bce_with_logits(logits, mined)``.  Every tensor
    has ``capacity`` rows, nothing is read back: the host runs ahead of the device, and the decoder's shapes never change."""
    mined = mine_pairs_device(targets, capacity, neg_per_pos=neg_per_pos, generator=generator, ordered_negatives=ordered_negatives)
    with torch.autocast(samples.device.type, dtype=torch.bfloat16, enabled=amp):
        feats = model(samples, forward_first_part=True)
    return (samples, feats, mined.groups[:, 0].contiguous(), mined.segments), mined
