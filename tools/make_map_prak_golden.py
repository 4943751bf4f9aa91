"""Writes tests/golden/map_prak.npz: inputs and outputs of the reference's ``misc/metric.calc_map_prak``.

    python tools/make_map_prak_golden.py --reference <checkout of glmanhtu/vit-ed>

The reference module is imported from the checkout, not copied.  Every case is stored as arrays only:
``<case>__D`` (float16 distances [r, n], exact in float32 too; row i has the label of column i, as calc_map_prak reads it, so a
case with r < n covers the first r rows of an n x n matrix), ``<case>__labels`` (int64 [n], label values in [0, L)),
``<case>__pos_offsets`` / ``<case>__pos_members`` (int64 CSR over the label values: the positive labels of label a are
members[offsets[a]:offsets[a + 1]]; stored for the labels of the rows only), ``<case>__neg_offsets`` / ``<case>__neg_members`` (the same for the negative relation;
absent when the case has none), ``<case>__prak`` (int64) and ``<case>__result`` (float64: m_ap, then pr@k for every k).
Every row is tie-free, so the reference's (unstable) argsort and a stable one give the same order.
"""
import argparse
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'map_prak.npz')

# float16 levels in [0.25, 4): 4 x 1024 distinct values, enough for a tie-free row of up to 4,096 columns
LEVELS = np.unique(np.arange(0x3400, 0x4400, dtype=np.uint16).view(np.float16))


def _groups(rng, labels_count, sizes):
    """Label values 0..labels_count-1 split into groups of the given sizes (the rest singletons): label -> its group's labels."""
    perm = rng.permutation(labels_count)
    rel, at = {}, 0
    for s in sizes:
        g = perm[at:at + s]
        at += s
        for a in g:
            rel[int(a)] = {int(b) for b in g}
    for a in perm[at:]:
        rel[int(a)] = {int(a)}
    return rel


def _distances(rng, labels, rows, rel, self_rank=None):
    """Tie-free float16 rows [rows, n]: a noisy score, lower for positive columns, mapped by rank onto distinct levels.  The
    diagonal comes first unless self_rank puts it at that rank of its row."""
    n = labels.size
    D = np.empty((rows, n), dtype=np.float16)
    for i in range(rows):
        pos = np.array([b in rel[int(labels[i])] for b in labels])
        score = rng.normal(size=n) - 1.5 * pos
        score[i] = -10.0
        order = np.argsort(score, kind='stable')
        if self_rank is not None:
            order = np.insert(order[order != i], self_rank[i], i)
        D[i, order] = np.sort(rng.choice(LEVELS, size=n, replace=False))
    return D


def _negatives(rng, num_labels, rel, frac):
    """label -> a random subset of the other labels (some overlapping its positives)."""
    return {a: {int(b) for b in np.flatnonzero(rng.random(num_labels) < frac)} | ({a} if rng.random() < 0.5 else set())
            for a in range(num_labels)}


def cases(rng):
    out = {}
    # positives only, one label per column (fragments), groups of 2-6
    lab = np.arange(60)
    rel = _groups(rng, 60, [int(s) for s in rng.integers(2, 7, 12)])
    out['pos_n60'] = (_distances(rng, lab, 60, rel), lab, rel, None, (1, 5, 10))
    # with negatives: only the columns whose label is positive or negative for the row take part
    lab = np.arange(80)
    rel = _groups(rng, 80, [int(s) for s in rng.integers(2, 9, 14)])
    neg = _negatives(rng, 80, rel, 0.3)
    out['neg_n80'] = (_distances(rng, lab, 80, rel), lab, rel, neg, (1, 5, 10))
    # rows without a correct retrieval (singleton groups: the diagonal comes first and is skipped), k above the hit counts
    lab = np.arange(70)
    rel = _groups(rng, 70, [2, 2, 3, 3, 4, 20])
    out['singletons_n70_bigk'] = (_distances(rng, lab, 70, rel), lab, rel, None, (1, 3, 7, 50))
    # the self column is not the row minimum, labels repeated across columns, with negatives
    lab = rng.integers(0, 30, 90)
    rel = _groups(rng, 30, [3, 3, 4, 5, 2, 2])
    neg = _negatives(rng, 30, rel, 0.4)
    out['offdiag_repeated_n90'] = (_distances(rng, lab, 90, rel, self_rank=rng.integers(0, 15, 90)), lab, rel, neg, (1, 2, 5, 10, 20))
    out['offdiag_repeated_n90_noneg'] = (out['offdiag_repeated_n90'][0], lab, rel, None, (1, 4))
    # a group of 2,400 members (several LDS passes of correct columns); the first 24 rows of the 2,600 x 2,600 matrix
    lab = np.arange(2600)
    rel = {a: set(range(2400)) if a < 2400 else {a, 2400 + (a - 2400 + 1) % 200} for a in range(2600)}
    perm = rng.permutation(2600)
    lab = perm                                             # the big group spread over the columns
    out['biggroup_n2600_r24'] = (_distances(rng, lab, 24, rel), lab, rel, None, (1, 10, 100, 3000))
    neg = {a: set(range(2400, 2600, 2)) for a in range(2600)}
    out['biggroup_n2600_r24_neg'] = (_distances(rng, lab, 24, rel), lab, rel, neg, (1, 10, 100))
    return out


def _csr(rel, num_labels):
    offsets, members = [0], []
    for a in range(num_labels):
        members.extend(sorted(rel.get(a, ())))
        offsets.append(len(members))
    return np.array(offsets, dtype=np.int64), np.array(members, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reference', required=True, help='checkout of glmanhtu/vit-ed (provides misc/metric.py)')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location('metric', os.path.join(args.reference, 'misc', 'metric.py'))
    metric = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(metric)
    arrays = {}
    for name, (D, lab, rel, neg, prak) in cases(np.random.default_rng(20261015)).items():
        for row in D.astype(np.float32):
            assert np.unique(row).size == row.size, f'{name}: a row has ties'
        row_labels = {int(a) for a in lab[:D.shape[0]]}       # calc_map_prak reads the relations of the row labels only
        rel = {a: rel[a] for a in row_labels}
        neg = None if neg is None else {a: neg[a] for a in row_labels}
        num_labels = int(lab.max() + 1)
        m_ap, pr = metric.calc_map_prak(D.astype(np.float32), lab, rel, neg, prak=prak)
        res = np.array([m_ap, *pr], dtype=np.float64)
        arrays[f'{name}__D'] = D
        arrays[f'{name}__labels'] = lab.astype(np.int64)
        arrays[f'{name}__pos_offsets'], arrays[f'{name}__pos_members'] = _csr(rel, num_labels)
        if neg is not None:
            arrays[f'{name}__neg_offsets'], arrays[f'{name}__neg_members'] = _csr(neg, num_labels)
        arrays[f'{name}__prak'] = np.array(prak, dtype=np.int64)
        arrays[f'{name}__result'] = res
        print(f'{name}: {D.shape} mAP {res[0]:.6f} pr@k {np.round(res[1:], 6).tolist()}')
    np.savez_compressed(args.out, **arrays)
    print(f'wrote {args.out} ({os.path.getsize(args.out) / 1e6:.2f} MB)')


if __name__ == '__main__':
    main()
