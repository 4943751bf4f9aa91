"""Writes tests/golden/wi19_curves.npz: inputs and outputs of the reference's ``misc/wi19_evaluate.get_sorted_retrievals``,
``compute_roc`` and ``compute_fscore``.

    python tools/make_ranklists_golden.py --reference <checkout of glmanhtu/vit-ed>

The reference module is imported from the checkout, not copied.  Every case is stored as arrays only: ``<case>__D`` (float16
distances, exact in float32 too), ``<case>__labels`` (int64), ``<case>__remove_self`` (bool, 0-d), ``<case>__estimate`` (int64 [n],
the relevant_estimate given to compute_fscore), ``<case>__order`` (int32: np.argsort(D, axis=1) behind the dropped column, the
order get_sorted_retrievals ranks by), ``<case>__sorted_retrievals`` (bool), ``<case>__fallout`` / ``<case>__recall`` (float64, of
compute_roc) and ``<case>__fscore`` (float64 [3]: fscore, precision, recall).  No row of any matrix holds two equal values - the
tool asserts it - because np.argsort's default sort is not stable: under ties the reference defines no order.
"""
import argparse
import importlib.util
import os

import numpy as np

from make_wi19_golden import _distances, _labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'wi19_curves.npz')


def _estimate(rng, labels):
    """A per-row estimate of the number of relevant columns: the class size less the query, off by up to two either way."""
    size = (labels[:, None] == labels[None, :]).sum(axis=1) - 1
    return np.maximum(size + rng.integers(-2, 3, labels.size), 0).astype(np.int64)


def cases(rng):
    out = {}
    lab = _labels(rng, 40, 6, 0)
    out['tiefree_n40_c6'] = (_distances(rng, lab), lab, True)
    lab = _labels(rng, 150, 12, 0)                         # the self column is not the row minimum in most rows
    out['offdiag_n150_c12'] = (_distances(rng, lab, self_rank=rng.integers(0, 20, 150)), lab, True)
    lab = _labels(rng, 60, 7, 1)                           # a singleton class: that row has no relevant column
    out['singleton_n60_c7'] = (_distances(rng, lab), lab, True)
    lab = _labels(rng, 40, 6, 0)
    out['keep_self_n40_c6'] = (_distances(rng, lab), lab, False)
    return {name: case + (_estimate(rng, case[1]),) for name, case in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reference', required=True, help='checkout of glmanhtu/vit-ed (provides misc/wi19_evaluate.py)')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location('wi19_evaluate', os.path.join(args.reference, 'misc', 'wi19_evaluate.py'))
    wi19 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(wi19)
    arrays = {}
    for name, (D, lab, remove, estimate) in cases(np.random.default_rng(20261020)).items():
        D32 = D.astype(np.float32)
        for row in D32:
            assert np.unique(row).size == row.size, f'{name}: a row has ties'
        order = np.argsort(D32, axis=1)[:, 1 if remove else 0:]
        sr = wi19.get_sorted_retrievals(D32, lab, remove_self_column=remove)
        assert np.array_equal(sr, lab[order] == lab[:, None])
        with np.errstate(invalid='ignore', divide='ignore'):
            roc = wi19.compute_roc(sr)
            fscore = np.array(wi19.compute_fscore(sr, estimate), dtype=np.float64)
        arrays.update({f'{name}__D': D, f'{name}__labels': lab, f'{name}__remove_self': np.array(remove), f'{name}__estimate': estimate,
                       f'{name}__order': order.astype(np.int32), f'{name}__sorted_retrievals': sr,
                       f'{name}__fallout': np.asarray(roc['fallout'], dtype=np.float64),
                       f'{name}__recall': np.asarray(roc['recall'], dtype=np.float64), f'{name}__fscore': fscore})
        print(f'{name}: relevant {int(sr.sum())} rows without one {int((sr.sum(axis=1) == 0).sum())} fscore {fscore}')
    np.savez_compressed(args.out, **arrays)
    print(f'wrote {args.out} ({os.path.getsize(args.out) / 1e3:.1f} KB)')


if __name__ == '__main__':
    main()
