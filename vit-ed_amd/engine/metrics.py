"""Evaluation metrics on the device: retrieval metrics of a distance matrix, group mAP / Pr@k, the geshaem pair-score maps, and
the validation meters of the multi-output classifier."""
from __future__ import annotations

import itertools
from typing import NamedTuple

import torch
import torch.distributed as dist

from .. import ops                  # the ops entry points refuse CPU tensors: there is no CPU fallback
from .feeds import DevicePrefetcher
from .similarity import shard_rows_by_pair_count


# ---- retrieval metrics of the distance matrix (misc/wi19_evaluate.get_metrics, hisfrag.py:309,321)
def _summed_rows(share, n, rows, nsums, device, group):
    """The float64 [nsums] sums ``share(r0, r1)`` returns for ``rows=(r0, r1)`` (default: all n rows), SUM all-reduced over
    ``group`` when one is given.  An empty share (more ranks than rows) contributes zeros but still joins the reduction."""
    r0, r1 = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= r0 <= r1 <= n:
        raise ValueError(f'rows ({r0}, {r1}) is not a range inside [0, {n}]')
    sums = share(r0, r1) if r1 > r0 else torch.zeros(nsums, dtype=torch.float64, device=device)
    if group is not None:
        dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
    return sums


def class_members(labels: torch.Tensor):
    """(class ids int32 [n] in [0, C), offsets int32 [C + 1], members int32 [n]): the columns of class c are
    members[offsets[c]:offsets[c + 1]], in ascending order.  Equal input labels get equal ids, so 'same class' is unchanged."""
    _, ids = torch.unique(labels, return_inverse=True)
    members = torch.argsort(ids, stable=True)
    counts = torch.bincount(ids)
    offsets = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=labels.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return ids.to(torch.int32), offsets.to(torch.int32), members.to(torch.int32)


def metrics_from_sums(sums):
    """(mAP, top-1, Pr@10, Pr@100) from the 7 sums of vited_retrieval_metrics (after any cross-rank SUM).  mAP is NaN when
    no row has a correct retrieval (numpy's mean of an empty array); Pr@k is NaN as soon as one row has none, as in the
    reference."""
    ap, valid, top1, pr10, pr100, _, rows = (float(v) for v in sums.tolist())
    nan = float('nan')
    return (ap / valid if valid else nan,) + ((top1 / rows, pr10 / rows, pr100 / rows) if rows else (nan, nan, nan))


def retrieval_metrics(distance: torch.Tensor, labels, *, rows=None, remove_self_column: bool = True,
                      from_similarity: bool = False, group=None):
    """(mAP, top-1, Pr@10, Pr@100) of ``wi19_evaluate.get_metrics(distance, labels, remove_self_column)`` on the GPU.

    ``distance``: [n, n] float16 / bfloat16 / float32 on the device (with ``from_similarity``: the similarity matrix S, ranked
    by dtype(1 - S)).  ``labels``: int class ids [n] (a device tensor, or anything torch.as_tensor takes).  ``rows=(r0, r1)``
    computes this rank's share of the rows (default: all); with ``group`` (a process group, e.g. ``dist.group.WORLD``) ONE
    all-reduce (SUM, so gloo works too) combines the shares and every rank returns the metrics of all rows.  Without a group
    the result covers ``rows`` only."""
    n = distance.shape[0]
    labels = torch.as_tensor(labels, device=distance.device)
    if labels.dim() != 1 or labels.numel() != n:
        raise ValueError(f'labels must be a vector of length {n}, got shape {tuple(labels.shape)}')
    if labels.is_floating_point() or labels.is_complex():
        raise TypeError(f'labels must be integer class ids, got {labels.dtype}')

    def share(r0, r1):
        ids, offsets, members = class_members(labels)
        return ops.retrieval_metrics_rows(distance, ids, offsets, members, (r0, r1), remove_self_column=remove_self_column,
                                          from_similarity=from_similarity)[1]
    return metrics_from_sums(_summed_rows(share, n, rows, 7, distance.device, group))


@torch.no_grad()
def hisfrag_retrieval_metrics(similarity: torch.Tensor, labels, *, rank: int = 0, world: int = 1, group=None,
                              remove_self_column: bool = True):
    """The evaluation step after ``pairwise_similarity``: every rank holds the [n, n] fp16 similarity, ranks the rows
    ``shard_rows_by_pair_count(n, world)`` gives it by fp16(1 - similarity), and one all-reduce gives every rank the metrics of
    all rows.  Replaces, on every rank (hisfrag.py:294-296,306-309):

        distance_matrix = 1 - similarity_matrix
        labels = utils.list_to_idx(img_names, lambda x: x.split('_')[0])
        m_ap, top1, pr_k10, pr_k100 = wi19_evaluate.get_metrics(distance_matrix.numpy(), np.asarray(labels))

    with ``hisfrag_retrieval_metrics(similarity, labels, rank=rank, world=world)`` (same ``labels``)."""
    n = similarity.shape[0]
    bounds = shard_rows_by_pair_count(n, world)
    if world > 1 and group is None:
        group = dist.group.WORLD
    return retrieval_metrics(similarity, labels, rows=(bounds[rank], bounds[rank + 1]), remove_self_column=remove_self_column,
                             from_similarity=True, group=group if world > 1 else None)


# ---- ranked retrieval lists (wi19_evaluate.get_sorted_retrievals, hisfrag_visualize_results.py) and the ROC / F-score curves
def _row_range(n, rows):
    r0, r1 = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= r0 <= r1 <= n:
        raise ValueError(f'rows ({r0}, {r1}) is not a range inside [0, {n}]')
    return r0, r1


def _class_labels(labels, n, device):
    labels = torch.as_tensor(labels, device=device)
    if labels.dim() != 1 or labels.numel() != n:
        raise ValueError(f'labels must be a vector of length {n}, got shape {tuple(labels.shape)}')
    if labels.is_floating_point() or labels.is_complex():
        raise TypeError(f'labels must be integer class ids, got {labels.dtype}')
    return labels


class RetrievalLists(NamedTuple):
    """``retrieval_topk``: ``indices`` int32 [rows, k] the retrieved columns in rank order, ``values`` float32 [rows, k] the values
    they were ranked by, ``correct`` uint8 [rows, k] (1 where the hit has the row's label) or None without labels."""
    indices: torch.Tensor
    values: torch.Tensor
    correct: torch.Tensor | None


def retrieval_topk(distance: torch.Tensor, k: int, *, labels=None, rows=None, remove_self_column: bool = True,
                   from_similarity: bool = False) -> RetrievalLists:
    """The ``k`` nearest columns of every row of ``rows`` (default: all), on the GPU, without the [n, n] matrix on the host.

    The order is the one ``retrieval_metrics`` ranks by: ascending by (value, column) - a STABLE argsort, ties to the lower column,
    NaN last - of ``distance`` (with ``from_similarity``: of dtype(1 - S)), the first element dropped with ``remove_self_column``
    whatever column it is.  Without ties it is ``np.argsort(D, axis=1)[:, skip:skip + k]``; with ``labels`` (int class ids [n])
    ``correct`` is ``wi19_evaluate.get_sorted_retrievals(D, labels, remove_self_column)[:, :k]``.  1 <= k <= 1024, k + skip <= n."""
    n = distance.shape[0]
    r0, r1 = _row_range(n, rows)
    ids = None
    if labels is not None:
        ids = torch.unique(_class_labels(labels, n, distance.device), return_inverse=True)[1].to(torch.int32)
    if r1 == r0:
        k = int(k)
        empty = lambda dtype: torch.empty((0, k), dtype=dtype, device=distance.device)
        return RetrievalLists(empty(torch.int32), empty(torch.float32), None if ids is None else empty(torch.uint8))
    return RetrievalLists(*ops.retrieval_topk_rows(distance, k, (r0, r1), ids, remove_self_column=remove_self_column,
                                                   from_similarity=from_similarity))


@torch.no_grad()
def hisfrag_retrieval_lists(similarity: torch.Tensor, k: int, labels=None, *, rank: int = 0, world: int = 1,
                            group=None) -> RetrievalLists:
    """The ``k`` most similar fragments of every fragment, after ``pairwise_similarity``: every rank holds the [n, n] similarity,
    ranks the rows ``shard_rows_by_pair_count(n, world)`` gives it by dtype(1 - similarity) behind the dropped first hit (the query
    itself), and ONE all-reduce (SUM of zero-initialised buffers over disjoint row shares, so gloo works too) gives every rank the
    lists of all n rows.  Replaces the CSV of the matrix and, per fragment (scripts/hisfrag_visualize_results.py),

        similarity_matrix[col].nlargest(k + 1)[1:]

    with ``hisfrag_retrieval_lists(similarity, k)``: ``indices[i]`` are the columns, ``1 - values[i]`` the similarities."""
    n = similarity.shape[0]
    bounds = shard_rows_by_pair_count(n, world)
    r0, r1 = bounds[rank], bounds[rank + 1]
    part = retrieval_topk(similarity, k, labels=labels, rows=(r0, r1), remove_self_column=True, from_similarity=True)
    if world == 1:
        return part
    # one int32 buffer [3, n, k]: columns, value bits, hits - integer sums with zeros keep every bit pattern
    both = torch.zeros((3, n, int(k)), dtype=torch.int32, device=similarity.device)
    both[0, r0:r1] = part.indices
    both[1, r0:r1] = part.values.view(torch.int32)
    if part.correct is not None:
        both[2, r0:r1] = part.correct
    dist.all_reduce(both, op=dist.ReduceOp.SUM, group=dist.group.WORLD if group is None else group)
    return RetrievalLists(both[0], both[1].view(torch.float32), None if part.correct is None else both[2].to(torch.uint8))


def _ratio(num, den):
    """num / den in float64 with numpy's zero rule: 0 / 0 is NaN, x / 0 is +-inf."""
    return (torch.tensor(float(num), dtype=torch.float64) / torch.tensor(float(den), dtype=torch.float64)).item()


class RetrievalCurves(NamedTuple):
    """``retrieval_curves``: ``tp_at`` int64 [n - skip] = ``sorted_retrievals.sum(axis=0)`` over the ``rows`` ranked rows,
    ``relevant`` = ``sorted_retrievals.sum()``, and with a ``relevant_estimate`` ``tp_in_estimate`` = the correct retrievals inside
    each row's estimate and ``retrieved`` = the sum of the estimates (both None without one)."""
    tp_at: torch.Tensor
    rows: int
    relevant: int
    tp_in_estimate: int | None
    retrieved: int | None

    def roc(self) -> dict:
        """``wi19_evaluate.compute_roc(sorted_retrievals)``: {'fallout', 'recall'}, float64 [n - skip] - int64 cumulative sums,
        converted to float64, one division each; a zero denominator gives NaN."""
        tp = torch.cumsum(self.tp_at, 0).to(torch.float64)
        fp_at = self.rows - self.tp_at
        fp = torch.cumsum(fp_at, 0).to(torch.float64)
        negatives = fp_at.sum().to(torch.float64)                     # (1 - sorted_retrievals).sum(): FP + TN
        return {'fallout': fp / negatives, 'recall': tp / torch.full_like(tp, float(self.relevant))}

    def fscore(self) -> tuple:
        """``wi19_evaluate.compute_fscore(sorted_retrievals, relevant_estimate)``: (fscore, precision, recall)."""
        if self.tp_in_estimate is None:
            raise ValueError('fscore() needs the curves of a relevant_estimate: pass one to retrieval_curves')
        precision = _ratio(self.tp_in_estimate, self.retrieved)
        recall = _ratio(self.tp_in_estimate, self.relevant)
        two = torch.tensor([precision, recall], dtype=torch.float64)
        return (2 * two[0] * two[1] / (two[0] + two[1])).item(), precision, recall


def retrieval_curves(distance: torch.Tensor, labels, *, rows=None, remove_self_column: bool = True, from_similarity: bool = False,
                     relevant_estimate=None, group=None) -> RetrievalCurves:
    """The counts behind ``wi19_evaluate.compute_roc`` and ``compute_fscore`` of ``get_sorted_retrievals(distance, labels,
    remove_self_column)``, on the GPU: the row kernel of ``retrieval_metrics`` (same order, same arguments) also counts, per
    position, the rows with a correct retrieval there.  ``relevant_estimate``: int [n], the per-row estimate of ``compute_fscore``.
    ``rows=(r0, r1)`` computes this rank's share; with ``group`` ONE int64 SUM all-reduce combines the shares and every rank returns
    the curves of all rows.  Without a group the result covers ``rows`` only."""
    n = distance.shape[0]
    dev = distance.device
    labels = _class_labels(labels, n, dev)
    r0, r1 = _row_range(n, rows)
    skip = 1 if remove_self_column else 0
    estimate = None
    if relevant_estimate is not None:
        estimate = torch.as_tensor(relevant_estimate, device=dev)
        if estimate.dim() != 1 or estimate.numel() != n or estimate.is_floating_point() or estimate.is_complex():
            raise ValueError(f'relevant_estimate must be an integer vector of length {n}, got {estimate.dtype} {tuple(estimate.shape)}')
        estimate = estimate.clamp(-1, n).to(torch.int32)             # beyond [0, n - skip] an estimate selects nothing more
    # [tp_at (n - skip), rows, relevant, tp_in_estimate, retrieved]
    state = torch.zeros(max(n - skip, 0) + 4, dtype=torch.int64, device=dev)
    if r1 > r0:
        ids, offsets, members = class_members(labels)
        tp_at, records = ops.retrieval_curve_rows(distance, ids, offsets, members, (r0, r1), remove_self_column=remove_self_column,
                                                  from_similarity=from_similarity, estimate=estimate)
        state[:n - skip] = tp_at
        state[n - skip] = r1 - r0
        state[n - skip + 1:n - skip + 3] = records.sum(0, dtype=torch.int64)
        if relevant_estimate is not None:
            state[n - skip + 3] = torch.as_tensor(relevant_estimate, device=dev)[r0:r1].sum(dtype=torch.int64)
    if group is not None:
        dist.all_reduce(state, op=dist.ReduceOp.SUM, group=group)
    tail = state[n - skip:].tolist()
    with_estimate = relevant_estimate is not None
    return RetrievalCurves(state[:n - skip], tail[0], tail[1], tail[2] if with_estimate else None, tail[3] if with_estimate else None)


# ---- group mAP / Pr@k (misc/metric.calc_map_prak) and the geshaem evaluation (michigan.py:188-233)
def _relation_csr(uniq, id_of, relation, row_ids, device):
    """(offsets int32 [L + 1], label ids int32): for every label id a whose label is in ``row_ids``, the ascending, duplicate-free
    ids of the labels of ``relation[label]`` that occur among the columns (others cannot match).  A missing key raises KeyError,
    as the reference's ``positive_pairs[labels[i]]`` does; labels of rows outside the range get an empty row."""
    offsets, flat = [0], []
    for a, label in enumerate(uniq):
        if a in row_ids:
            flat.extend(sorted({id_of[b] for b in relation[label] if b in id_of}))
        offsets.append(len(flat))
    return (torch.tensor(offsets, dtype=torch.int32, device=device), torch.tensor(flat, dtype=torch.int32, device=device))


def group_relations(labels, positive_pairs, negative_pairs=None, device='cuda', *, rows=None):
    """The device form of (labels, positive_pairs, negative_pairs) that ``ops.group_retrieval_metrics_rows`` takes:
    (label ids int32 [n], (offsets, members) of every label's columns, positive CSR, negative CSR or None), label ids numbered
    by first appearance.  Only the labels of ``rows`` (default: all) are looked up in the mappings."""
    labels = list(labels)
    r0, r1 = (0, len(labels)) if rows is None else (int(rows[0]), int(rows[1]))
    id_of = {}
    ids = [id_of.setdefault(label, len(id_of)) for label in labels]
    uniq = list(id_of)
    row_ids = set(ids[r0:r1])
    label_ids, col_off, col_mem = class_members(torch.tensor(ids, dtype=torch.int64, device=device))
    pos = _relation_csr(uniq, id_of, positive_pairs, row_ids, device)
    neg = None if negative_pairs is None else _relation_csr(uniq, id_of, negative_pairs, row_ids, device)
    return label_ids, (col_off, col_mem), pos, neg


def map_prak(distances: torch.Tensor, labels, positive_pairs, negative_pairs=None, prak=(1, 5), *, rows=None, group=None):
    """``(m_ap, (pr@k for k in prak))`` of ``misc/metric.calc_map_prak(distances, labels, positive_pairs, negative_pairs, prak)``
    on the GPU.

    ``distances``: [n, n] float16 / bfloat16 / float32 on the device.  ``labels``: n hashables (``dist_df.columns``); row i has
    the label ``labels[i]``.  ``positive_pairs`` / ``negative_pairs``: mappings from a label to an iterable of labels
    (``fragment_to_group``); "correct" and "eligible" are set membership.  A row label missing from a mapping raises KeyError.
    Each row is ordered by a STABLE argsort (ties to the lower column, NaN last; numpy's default sort may order ties otherwise),
    its first eligible element is skipped whatever it is, and rows without a correct retrieval are left out, as in the
    reference.  Where no row has one the reference divides by zero; here every result is then NaN.  ``prak``: up to 8 ints >= 1.
    ``rows=(r0, r1)`` computes this rank's share of the rows (default: all); with ``group`` ONE all-reduce (SUM, so gloo works
    too) combines the shares and every rank returns the metrics of all rows.  Without a group the result covers ``rows`` only."""
    n = distances.shape[0]
    labels = list(labels)
    if len(labels) != n:
        raise ValueError(f'labels must hold {n} labels, got {len(labels)}')
    prak = tuple(int(k) for k in prak)
    if not 1 <= len(prak) <= 8 or min(prak) < 1:
        raise ValueError(f'prak must be 1 to 8 cut-offs >= 1, got {prak}')

    def share(r0, r1):
        rel = group_relations(labels, positive_pairs, negative_pairs, distances.device, rows=(r0, r1))
        return ops.group_retrieval_metrics_rows(distances, *rel, prak, (r0, r1))[1]
    s = [float(v) for v in _summed_rows(share, n, rows, 2 + len(prak), distances.device, group).tolist()]
    if s[1] == 0:
        return float('nan'), tuple(float('nan') for _ in prak)
    return s[0] / s[1], tuple(v / s[1] for v in s[2:])


class PairScoreStats(NamedTuple):
    """What ``PairScoreAggregator.finish`` returns.  mean / min float32 [n, n] of the distances 1 - score of every cell (NaN where
    a cell has no value), count int32 [n, n], std_stats = (avg_std, std_std): the mean and the sample stdev of the per-cell
    sample stdevs over the cells with more than one value (NaN where there are too few), std float64 [n, n] those stdevs."""
    mean: torch.Tensor
    min: torch.Tensor
    count: torch.Tensor
    std_stats: tuple
    std: torch.Tensor


class PairScoreAggregator:
    """The distance maps of ``geshaem_test`` (michigan.py:188-209) on the device.  ``add(pairs, scores)`` takes a validation
    batch's fragment-id pairs [m, 2] (int32 / int64, on the host or the device) and its scores [m] (the model's
    ``output.view(-1)``, float32 / bfloat16 / float16, on the device: never copied to the host).  Every score adds 1 - score to
    cell (i, j) and to cell (j, i).  ``finish()`` reduces every record added so far (PairScoreStats); its result is bit-identical
    whatever the batching and order of the records (include/vited.h)."""

    def __init__(self, n_fragments: int, device):
        self.n = int(n_fragments)
        self.device = torch.device(device)
        self.counts = torch.zeros((self.n, self.n), dtype=torch.int32, device=self.device)
        self.bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.size = 0
        self._cells = torch.empty((0, 2), dtype=torch.int32, device=self.device)
        self._values = torch.empty(0, dtype=torch.float32, device=self.device)

    def _reserve(self, extra: int):
        need = self.size + extra
        if need <= self._values.numel():
            return
        cap = max(need, 2 * self._values.numel(), 1 << 16)
        cells = torch.empty((cap, 2), dtype=torch.int32, device=self.device)
        values = torch.empty(cap, dtype=torch.float32, device=self.device)
        cells[:self.size] = self._cells[:self.size]
        values[:self.size] = self._values[:self.size]
        self._cells, self._values = cells, values

    def add(self, pairs: torch.Tensor, scores: torch.Tensor):
        scores = scores.reshape(-1)
        pairs = pairs.to(self.device, non_blocking=True)
        m = pairs.shape[0]
        if m == 0:
            return
        self._reserve(m)
        ops.pair_scores_add(pairs, scores, self.n, self.counts, self._cells[self.size:self.size + m],
                            self._values[self.size:self.size + m], self.bad)
        self.size += m

    def finish(self) -> PairScoreStats:
        mean, minv, std, stats = ops.pair_scores_finish(self._cells[:self.size], self._values[:self.size], self.n, self.counts,
                                                       self.bad)
        bad = int(self.bad.item())
        if bad & 1:
            raise ValueError(f'a fragment id outside [0, {self.n}) was added (those records were ignored)')
        if bad:
            raise RuntimeError('vited_pair_scores_finish: counts and records disagree')
        avg_std, std_std = (float(v) for v in stats.tolist())
        return PairScoreStats(mean, minv, self.counts.clone(), (avg_std, std_std), std)


class GeshaemMetrics(NamedTuple):
    """``geshaem_pair_metrics``: ``mean`` / ``min`` = (m_ap, (pr@k, ...)) of calc_map_prak on the MEAN / MIN distance maps,
    ``avg_std`` / ``std_std`` as logged by the reference, ``n_categories`` = the number of scored fragments."""
    mean: tuple
    min: tuple
    avg_std: float
    std_std: float
    n_categories: int


@torch.no_grad()
def geshaem_pair_metrics(aggregator: PairScoreAggregator, fragments, fragment_to_group, prak=(1, 5, 10)) -> GeshaemMetrics:
    """The evaluation of ``geshaem_test`` after its loop (michigan.py:211-233): the fragments that were scored, in ascending
    fragment index (the order the reference's dicts and DataFrame get from its unshuffled loader), labelled
    ``fragments[index]`` (``dataset.fragments``), ranked by the MEAN and by the MIN distance map with ``fragment_to_group`` as
    the positive relation.  The reference's return value is ``1 - max(result.mean[0], result.min[0])``."""
    res = aggregator.finish()
    scored = torch.nonzero((res.count > 0).any(dim=1)).flatten()
    idx = scored.tolist()
    labels = [fragments[a] for a in idx]
    out = []
    for matrix in (res.mean, res.min):
        sub = matrix.index_select(0, scored).index_select(1, scored)
        out.append(map_prak(sub, labels, fragment_to_group, prak=prak))
    return GeshaemMetrics(out[0], out[1], res.std_stats[0], res.std_stats[1], len(idx))


# ---- validation of the multi-output binary classifier (main.py:49-132, DefaultTrainer.validate)
_METERS = ('loss', 'acc', 'f1', 'precision', 'recall')


class MeterValue(NamedTuple):
    """AverageMeter's ``val`` (the last batch's value) and ``avg`` (sum / count on this rank)."""
    val: float
    avg: float


class ValidationResult(NamedTuple):
    """The averages ``DefaultTrainer.validate`` logs after its all-reduce; ``loss`` is what it returns.  ``samples``: the
    all-reduced sample count (fp32, as the reference's meters hold it)."""
    loss: float
    acc: float
    f1: float
    precision: float
    recall: float
    samples: int


class ClassificationMeters:
    """The reference's five validation AverageMeters (loss, acc, f1, precision, recall) on the device.

    ``update(logits, targets)`` is one launch of vited_cls_metrics_update per batch (no host sync): it replaces main.py:73-93, the
    host copy of the batch and the 16 sklearn calls.  ``values()`` copies the meters to the host once, for the PRINT_FREQ log
    lines.  ``all_reduce(group)`` replaces the six ``AverageMeter.all_reduce`` calls (main.py:113-119) with ONE fp32 SUM
    all-reduce of every (sum, count), rounded to fp32 first as the reference rounds them (also at world size 1); the bad-target
    flag travels in the same reduction, so every rank raises together."""

    def __init__(self, num_classes: int = 4, device='cuda'):
        self.num_classes = int(num_classes)
        if not 1 <= self.num_classes <= 64:
            raise ValueError(f'num_classes must be in [1, 64], got {num_classes}')
        self.device = torch.device(device)
        self.meters = torch.zeros(2 * len(_METERS), dtype=torch.float64, device=self.device)   # (sum, count) per meter
        self.last = torch.zeros(len(_METERS), dtype=torch.float64, device=self.device)
        self.bad = torch.zeros(1, dtype=torch.int32, device=self.device)

    def reset(self):
        self.meters.zero_()
        self.last.zero_()
        self.bad.zero_()

    def update(self, logits: torch.Tensor, targets: torch.Tensor):
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f'logits must be [B, {self.num_classes}], got {tuple(logits.shape)}')
        ops.cls_metrics_update(logits, targets, self.meters, self.last, self.bad)

    def values(self) -> dict:
        """name -> MeterValue(val, avg) of each meter on this rank (one device-to-host copy)."""
        host = torch.cat([self.last, self.meters]).tolist()
        last, state = host[:len(_METERS)], host[len(_METERS):]
        return {name: MeterValue(last[k], state[2 * k] / state[2 * k + 1] if state[2 * k + 1] else 0.0)
                for k, name in enumerate(_METERS)}

    def all_reduce(self, group=None) -> ValidationResult:
        """The all-reduced averages.  Raises ValueError when a target other than 0 / 1 was seen on any rank, and when no sample
        was added on any rank.  Joins the reduction over ``group`` (None: the default group) when torch.distributed is
        initialised; otherwise the result is this process's."""
        state = torch.cat([self.meters.to(torch.float32), self.bad.to(torch.float32)])   # AverageMeter.all_reduce's fp32 tensor
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(state, op=dist.ReduceOp.SUM, group=group)
        host = state.tolist()
        if host[-1]:
            raise ValueError('validation targets must be 0 or 1: vited_cls_metrics_update saw another value')
        if not host[1]:
            raise ValueError('no validation sample was added before all_reduce')
        avg = [host[2 * k] / host[2 * k + 1] for k in range(len(_METERS))]
        return ValidationResult(*avg, samples=int(host[1]))


@torch.no_grad()
def validate_classifier(model, data_loader, *, amp: bool = True, group=None, print_freq: int | None = None,
                        log=None) -> ValidationResult:
    """``DefaultTrainer.validate`` (main.py:49-132) with its metrics on the device.

    ``model``: the classifier (a DDP wrapper too), run in eval mode under no_grad and bf16 autocast when ``amp``; its previous
    mode is restored.  ``data_loader`` yields (images, targets [B, C] of 0 / 1): batches already on the model's device are used
    as they are, host batches go through DevicePrefetcher.  ``log(idx, values)`` is called with ``ClassificationMeters.values()``
    on every batch with idx % print_freq == 0 (the only batches that wait for the device).  One all-reduce over ``group`` at the
    end; the result's ``loss`` is what the reference's validate() returns."""
    dev = next(model.parameters()).device
    batches = iter(data_loader)
    first = next(batches, None)
    if first is None:
        raise ValueError('the validation loader yielded no batch')
    batches = itertools.chain([first], batches)
    if not (torch.is_tensor(first[0]) and first[0].device == dev):
        batches = DevicePrefetcher(batches, dev)
    meters = None
    was_training = model.training
    model.eval()
    try:
        for idx, (images, target) in enumerate(batches):
            with torch.autocast(dev.type, dtype=torch.bfloat16, enabled=amp):
                output = model(images)
            if meters is None:
                meters = ClassificationMeters(output.shape[1], dev)
            meters.update(output, target)
            if log is not None and print_freq and idx % print_freq == 0:
                log(idx, meters.values())
    finally:
        model.train(was_training)
    return meters.all_reduce(group)
