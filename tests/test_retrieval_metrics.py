"""CPU: a numpy restatement of the retrieval metrics of misc/wi19_evaluate.get_metrics (with a STABLE argsort: ties to the
lower column, NaN last), checked against the reference's own outputs stored in tests/golden/wi19_metrics.npz; and the
binding's argument checks, which run before any launch.  The GPU kernel (vited_retrieval_metrics) is checked against both in
tests/test_gpu_retrieval.py."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wi19_metrics.npz')


def reference_rows(D, labels, remove_self_column=True, rows=None):
    """Per-row records [len(rows), 5]: sum of m / rank_m over the correct retrievals, correct retrievals, top-1 hit, hits in
    the first 10, hits in the first 100 - the record vited_retrieval_metrics writes."""
    rows = np.arange(np.shape(D)[0]) if rows is None else np.asarray(rows)
    return reference_rows_of(np.asarray(D)[rows], labels, rows, remove_self_column)


def reference_rows_of(D_rows, labels, rows, remove_self_column=True):
    """reference_rows from the selected rows D[rows] alone."""
    labels = np.asarray(labels)
    rows = np.asarray(rows)
    order = np.argsort(np.asarray(D_rows, dtype=np.float32), axis=1, kind='stable')   # exact for half-width inputs
    if remove_self_column:
        order = order[:, 1:]                                 # the first element of the order, whatever column it is
    hit = labels[order] == labels[rows, None]
    m = np.cumsum(hit, axis=1)
    rank = np.arange(1, hit.shape[1] + 1)
    ap = np.where(hit, m / rank, 0.0).sum(axis=1)
    return np.stack([ap, hit.sum(axis=1), hit[:, 0], hit[:, :10].sum(axis=1), hit[:, :100].sum(axis=1)], axis=1).astype(np.float64)


def metrics_from_rows(rec):
    """(mAP, top-1, Pr@10, Pr@100) as get_metrics forms them: mAP over rows with a correct retrieval, the rest over all rows,
    Pr@k NaN as soon as one row has no correct retrieval."""
    ap, correct, top1, h10, h100 = rec.T
    valid = correct > 0
    with np.errstate(invalid='ignore', divide='ignore'):
        m_ap = (ap[valid] / correct[valid]).mean() if valid.any() else float('nan')
        return (float(m_ap), float(top1.sum() / len(rec)), float((h10 / np.minimum(correct, 10)).sum() / len(rec)),
                float((h100 / np.minimum(correct, 100)).sum() / len(rec)))


def reference_metrics(D, labels, remove_self_column=True):
    return metrics_from_rows(reference_rows(D, labels, remove_self_column))


def golden_cases():
    z = np.load(GOLDEN)
    names = sorted({k.split('__')[0] for k in z.files})
    return {n: (z[f'{n}__D'], z[f'{n}__labels'], bool(z[f'{n}__remove_self']), z[f'{n}__metrics']) for n in names}


def assert_metrics_equal(got, want, atol, what=''):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f'{what}: NaN in different places: {got} vs {want}'
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= atol), f'{what}: {got} vs {want}'


def test_golden_fixture_covers_the_cases():
    cases = golden_cases()
    assert len(cases) >= 5
    assert any(not remove for _, _, remove, _ in cases.values())                     # remove_self_column=False
    assert any(np.isnan(m).any() for *_, m in cases.values())                        # a row without a correct retrieval
    D, _, _, _ = cases['offdiag_n150_c12']
    assert (np.argmin(D, axis=1) != np.arange(D.shape[0])).sum() > D.shape[0] // 2   # the self-column rule matters there
    assert max(D.shape[0] for D, *_ in cases.values()) >= 1000


@pytest.mark.parametrize('name', sorted(golden_cases()))
def test_restatement_matches_reference(name):
    D, labels, remove, want = golden_cases()[name]
    assert_metrics_equal(reference_metrics(D, labels, remove), want, 1e-12, name)


def test_stable_ties_and_nan_order():
    """Ties go to the lower column and NaN sorts after +inf (np.argsort(kind='stable')); the dropped element is the first of
    that order, not the diagonal."""
    D = np.array([[1.0, 0.0, 0.0, np.nan],
                  [np.inf, 1.0, np.nan, 0.5],
                  [0.0, 0.0, 0.0, 0.0],
                  [np.nan, np.nan, -np.inf, np.nan]], dtype=np.float32)
    labels = np.array([0, 1, 0, 1])
    rec = reference_rows(D, labels)
    # row 0: order 1, 2, 0, 3 -> drop 1; retrievals 2 (hit), 0 (hit), 3
    np.testing.assert_array_equal(rec[0], [1 / 1 + 2 / 2, 2, 1, 2, 2])
    # row 1: order 3, 1, 0, 2 -> drop 3 (a hit!); retrievals 1 (hit, the diagonal), 0, 2
    np.testing.assert_array_equal(rec[1], [1.0, 1, 1, 1, 1])
    # row 2: all tied -> order 0, 1, 2, 3 -> drop 0; retrievals 1, 2 (hit at rank 2), 3
    np.testing.assert_array_equal(rec[2], [0.5, 1, 0, 1, 1])
    # row 3: order 2, 0, 1, 3 -> drop 2; retrievals 0, 1 (hit at 2), 3 (hit at 3)
    np.testing.assert_array_equal(rec[3], [1 / 2 + 2 / 3, 2, 0, 2, 2])


def test_bad_arguments_raise_before_any_launch(vited):
    from vited_amd import engine, ops
    D = torch.rand(8, 8)
    lab = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        engine.retrieval_metrics(D, lab)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.retrieval_metrics_rows(D, lab, torch.tensor([0, 8], dtype=torch.int32), torch.arange(8, dtype=torch.int32), (0, 8))


def test_abi_rejects_bad_arguments(vited):
    """vited_retrieval_metrics validates before launching, so bad arguments are safe to pass without a GPU."""
    import ctypes
    lib = vited._lib.load()
    buf = ctypes.create_string_buffer(1024)
    p = ctypes.addressof(buf)
    call = lambda **kw: lib.vited_retrieval_metrics(*{**dict(D=p, dtype=2, ld=8, n=8, r0=0, r1=8, labels=p, offsets=p, members=p,
                                                             C=1, remove=1, sim=0, rows_out=p, sums=p, stream=None), **kw}.values())
    assert call(D=None) == 1 and call(sums=None) == 1 and call(members=None) == 1
    assert call(ld=7) == 1 and call(n=0) == 1 and call(C=0) == 1 and call(C=9) == 1
    assert call(r0=-1) == 1 and call(r1=9) == 1 and call(r0=4, r1=4) == 1
    assert call(remove=2) == 1 and call(sim=3) == 1 and call(n=1, ld=1, r1=1) == 1
    assert call(dtype=7) == 2
    assert call(D=p + 1) == 1                                       # a half-width matrix must be 2-byte aligned
