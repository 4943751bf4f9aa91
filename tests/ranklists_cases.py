"""The numpy restatement of the ranked lists and the wi19 curve counts (vited_retrieval_topk / vited_retrieval_curves), and the
cases the CPU and the GPU tests share.  The order is stated on the key itself: row i ranks its columns by a STABLE argsort of the
64-bit key (order_bits(v) << 32) | column, v = D[i, j] or T(1 - S[i, j]) (fp32 subtract, one rounding to the matrix dtype T)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wi19_curves.npz')


def as_tensor(M):
    return M if torch.is_tensor(M) else torch.from_numpy(np.ascontiguousarray(M))


def rank_value(M, from_similarity=False):
    """float32 numpy array of the values the rows are ranked by; M: a torch tensor or numpy array of fp32 / bf16 / fp16."""
    M = as_tensor(M)
    v = (1.0 - M.float()).to(M.dtype).float() if from_similarity else M.float()
    return v.numpy()


def order_bits(v):
    """uint32 image of float32 values that orders like them: NaN above +inf (all NaNs one value), -0 tied with +0."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    u = v.view(np.uint32)
    u = np.where(v == 0, np.uint32(0), u)
    out = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(v), np.uint32(0xffffffff), out).astype(np.uint32)


def stable_order(V):
    """[rows, n] column order of every row of the ranked values V."""
    keys = (order_bits(V).astype(np.uint64) << np.uint64(32)) | np.arange(V.shape[1], dtype=np.uint64)[None, :]
    return np.argsort(keys, axis=1, kind='stable')


def reference_topk(M, k, labels=None, rows=None, remove_self_column=True, from_similarity=False):
    """(idx int32 [rows, k], val float32 [rows, k], hit uint8 [rows, k] | None) of the rows ``rows = (r0, r1)`` (default: all)."""
    M = as_tensor(M)
    r0, r1 = (0, M.shape[0]) if rows is None else rows
    V = rank_value(M[r0:r1], from_similarity)
    skip = 1 if remove_self_column else 0
    idx = stable_order(V)[:, skip:skip + k]
    val = np.take_along_axis(V, idx, axis=1)
    hit = None
    if labels is not None:
        labels = np.asarray(labels)
        hit = (labels[idx] == labels[r0:r1, None]).astype(np.uint8)
    return idx.astype(np.int32), val, hit


def reference_curves(M, labels, rows=None, remove_self_column=True, from_similarity=False, estimate=None):
    """(tp_at int64 [n - skip], records int32 [rows, 2]) as vited_retrieval_curves writes them."""
    M = as_tensor(M)
    labels = np.asarray(labels)
    r0, r1 = (0, M.shape[0]) if rows is None else rows
    order = stable_order(rank_value(M[r0:r1], from_similarity))[:, 1 if remove_self_column else 0:]
    sr = labels[order] == labels[r0:r1, None]
    inside = np.zeros(r1 - r0, dtype=np.int64)
    if estimate is not None:
        inside = (sr & (np.arange(sr.shape[1])[None, :] < np.asarray(estimate)[r0:r1, None])).sum(axis=1)
    return sr.sum(axis=0).astype(np.int64), np.stack([sr.sum(axis=1), inside], axis=1).astype(np.int32)


def roc_of(tp_at, rows):
    """compute_roc from the counts: int64 cumulative sums, converted to float64, one division each."""
    tp_at = np.asarray(tp_at, dtype=np.int64)
    fp_at = rows - tp_at
    with np.errstate(invalid='ignore', divide='ignore'):
        return {'fallout': fp_at.cumsum().astype('float') / fp_at.sum(),
                'recall': tp_at.cumsum().astype('float') / (np.ones(tp_at.size) * tp_at.sum())}


def fscore_of(tp_in_estimate, retrieved, relevant):
    """compute_fscore from the counts."""
    with np.errstate(invalid='ignore', divide='ignore'):
        precision = float(tp_in_estimate) / np.int64(retrieved)
        recall = float(tp_in_estimate) / np.int64(relevant)
        return 2 * precision * recall / (precision + recall), precision, recall


def golden_cases():
    z = np.load(GOLDEN)
    names = sorted({k.split('__')[0] for k in z.files})
    return {n: {f: z[f'{n}__{f}'] for f in ('D', 'labels', 'remove_self', 'estimate', 'order', 'sorted_retrievals', 'fallout', 'recall',
                                            'fscore')} for n in names}


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_values(got, want):
    """fp32 arrays equal as bit patterns; a NaN's payload is not defined by the arithmetic that made it, so NaNs need only coincide."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


# ---- the matrices of the GPU grid (seeded; built once per process)
def labels_for(n, classes, seed=0):
    return np.random.default_rng(1000 + seed).integers(0, classes, n)


def random_matrix(n, dtype, seed=0, levels=4096):
    """Values on a grid of `levels` steps in [0, 1): exact in every dtype up to 256 levels, with ties in every row beyond n > levels."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy((rng.integers(0, levels, (n, n)) / levels).astype(np.float32)).to(dtype)


def tied_matrix(n, dtype, seed=0):
    """Row 0: one repeated value.  Row 1: 4 of 5 values equal (0.5), the rest below and above it.  Row 2: scores saturated to exactly
    0 and 1.  Row 3: NaN, +inf, -inf, -0.0 mixed into random values, the minimum (-inf) off the diagonal.  Other rows: random."""
    M = random_matrix(n, torch.float32, seed, levels=64)
    rng = np.random.default_rng(50 + seed)
    M[0] = 0.25
    if n > 2:
        M[1, torch.from_numpy(np.arange(n) % 5 != 0)] = 0.5
        M[2] = torch.from_numpy((rng.random(n) < 0.03).astype(np.float32))
    if n > 3:
        special = torch.tensor([float('nan'), float('inf'), float('-inf'), -0.0, 0.0, float('nan'), -1.5, float('inf'), -0.0])
        cols = torch.arange(1, n, 3)
        M[3, cols] = special[torch.arange(cols.numel()) % 9]
    return M.to(dtype)
