"""Writes tests/golden/wi19_metrics.npz: inputs and outputs of the reference's ``misc/wi19_evaluate.get_metrics``.

    python tools/make_wi19_golden.py --reference <checkout of glmanhtu/vit-ed>

The reference module is imported from the checkout, not copied.  Every case is stored as arrays only:
``<case>__D`` (float16 distances, exact in float32 too), ``<case>__labels`` (int64), ``<case>__remove_self`` (bool, 0-d) and
``<case>__metrics`` (float64 [4]: mAP, top-1, Pr@10, Pr@100).  Every row of every matrix is tie-free, so the reference's
(unstable) argsort and a stable one give the same order, in float16 and float32 alike.
"""
import argparse
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'wi19_metrics.npz')

# float16 levels in [0.25, 4): 4 x 1024 distinct values, enough for a tie-free row of up to 4,096 columns
LEVELS = np.unique(np.arange(0x3400, 0x4400, dtype=np.uint16).view(np.float16))


def _labels(rng, n, classes, singletons):
    """n labels over `classes` classes, the last `singletons` of them with one member each, the rest at least two."""
    lab = np.concatenate([np.arange(classes - singletons).repeat(2), np.arange(classes - singletons, classes)])
    lab = np.concatenate([lab, rng.integers(0, classes - singletons, n - lab.size)])
    return rng.permutation(lab).astype(np.int64)


def _distances(rng, labels, self_rank=None):
    """Tie-free float16 rows: a noisy score, lower for same-class columns, mapped by rank onto distinct levels.
    self_rank: None keeps the diagonal where the score puts it; otherwise the diagonal is placed at that rank of its row."""
    n = labels.size
    same = labels[:, None] == labels[None, :]
    score = rng.normal(size=(n, n)) - 1.2 * same
    np.fill_diagonal(score, -10.0)                         # the diagonal first in its row, as a similarity run gives it
    D = np.empty((n, n), dtype=np.float16)
    for i in range(n):
        order = np.argsort(score[i], kind='stable')
        if self_rank is not None:
            order = np.insert(order[order != i], self_rank[i], i)
        levels = np.sort(rng.choice(LEVELS, size=n, replace=False))
        D[i, order] = levels
    return D


def _shifted_rows(rng, n, classes):
    """A tie-free n x n case that compresses: the classes are contiguous blocks and row i + 1 is row i shifted by one column
    except where a class block starts or ends, so the stored file stays small at n = 1,000 (random tie-free rows of that size
    cannot be stored in under 1 MB).  Column j of row i takes a level from its rank p = perm[(j - i) % n]: level 2(p + n // 20 + 1)
    for a column of another class, level 2p + 1 for a column of the same class (n // 10 levels lower), and level 0 on the
    diagonal - so no row has a tie, and same-class columns come early more often than not."""
    lab = np.sort(_labels(rng, n, classes, 0))
    perm = rng.permutation(n)
    i, j = np.indices((n, n))
    p = perm[(j - i) % n]
    same = lab[:, None] == lab[None, :]
    idx = np.where(same, 2 * p + 1, 2 * (p + n // 20 + 1))     # odd / even level indices never meet
    idx[i == j] = 0
    return LEVELS[idx], lab


def cases(rng):
    out = {}
    lab = _labels(rng, 50, 3, 0)
    out['tiefree_n50_c3'] = (_distances(rng, lab), lab, True)
    lab = _labels(rng, 300, 40, 5)                         # singletons: a row without a correct retrieval, NaN Pr@k
    out['tiefree_n300_c40_singletons'] = (_distances(rng, lab), lab, True)
    D, lab = _shifted_rows(rng, 1000, 25)
    out['shifted_n1000_c25'] = (D, lab, True)
    lab = _labels(rng, 150, 12, 0)                         # the self column is not the row minimum in most rows
    out['offdiag_n150_c12'] = (_distances(rng, lab, self_rank=rng.integers(0, 20, 150)), lab, True)
    lab = _labels(rng, 150, 10, 2)
    out['keep_self_n150_c10'] = (_distances(rng, lab), lab, False)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reference', required=True, help='checkout of glmanhtu/vit-ed (provides misc/wi19_evaluate.py)')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location('wi19_evaluate', os.path.join(args.reference, 'misc', 'wi19_evaluate.py'))
    wi19 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(wi19)
    arrays = {}
    for name, (D, lab, remove) in cases(np.random.default_rng(20261015)).items():
        for row in D.astype(np.float32):
            assert np.unique(row).size == row.size, f'{name}: a row has ties'
        with np.errstate(invalid='ignore', divide='ignore'):
            m = np.array(wi19.get_metrics(D.astype(np.float32), lab, remove_self_column=remove), dtype=np.float64)
        arrays.update({f'{name}__D': D, f'{name}__labels': lab, f'{name}__remove_self': np.array(remove),
                       f'{name}__metrics': m})
        print(f'{name}: mAP {m[0]:.6f} top-1 {m[1]:.6f} Pr@10 {m[2]:.6f} Pr@100 {m[3]:.6f}')
    np.savez_compressed(args.out, **arrays)
    print(f'wrote {args.out} ({os.path.getsize(args.out) / 1e6:.2f} MB)')


if __name__ == '__main__':
    main()
