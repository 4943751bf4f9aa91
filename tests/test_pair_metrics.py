"""CPU: numpy restatements of the geshaem evaluation of the reference - the distance maps of michigan.py:188-223 (dicts of lists)
and misc/metric.calc_map_prak with a STABLE argsort (ties to the lower column, NaN last) - the latter checked against the
reference's own outputs stored in tests/golden/map_prak.npz; and the new C entries: exported, and rejecting bad arguments before
any launch.  The GPU kernels (vited_group_retrieval_metrics, vited_pair_scores_*) are checked against both in
tests/test_gpu_pair_metrics.py."""
import ctypes
import math
import os
import statistics
import subprocess

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'map_prak.npz')
NEW_ENTRIES = ('vited_group_retrieval_metrics', 'vited_pair_scores_workspace_bytes', 'vited_pair_scores_add',
               'vited_pair_scores_finish')


# ---- calc_map_prak ------------------------------------------------------------------------------
def reference_group_rows(D_rows, labels, rows, positive_pairs, negative_pairs=None, prak=(1, 5)):
    """Per-row records [len(rows), 3 + len(prak)] of calc_map_prak from the selected rows D[rows] alone: AP (0 without a correct
    retrieval), valid (0/1), correct retrievals, then the correct retrievals in the first k positions for every k - the
    record vited_group_retrieval_metrics writes."""
    labels = list(labels)
    id_of = {}
    ids = np.array([id_of.setdefault(label, len(id_of)) for label in labels])
    out = np.zeros((len(rows), 3 + len(prak)))
    for r, i in enumerate(rows):
        pos = np.zeros(len(id_of), bool)
        pos[[id_of[b] for b in set(positive_pairs[labels[i]]) if b in id_of]] = True
        elig = np.ones(len(id_of), bool)
        if negative_pairs is not None:
            elig = pos.copy()
            elig[[id_of[b] for b in set(negative_pairs[labels[i]]) if b in id_of]] = True
        order = np.argsort(np.asarray(D_rows[r], dtype=np.float32), kind='stable')   # exact for half-width inputs
        order = order[elig[ids[order]]][1:]                  # the eligible columns, the first of them skipped
        hit = pos[ids[order]]
        correct = int(hit.sum())
        if correct:
            m = np.cumsum(hit)
            out[r, 0] = (m[hit] / (np.flatnonzero(hit) + 1)).sum() / correct
            out[r, 1] = 1
        out[r, 2] = correct
        for q, k in enumerate(prak):
            out[r, 3 + q] = hit[:k].sum()
    return out


def group_metrics_from_rows(rec, prak):
    """(m_ap, (pr@k, ...)) from the row records: means over the rows with a correct retrieval (NaN where there is none)."""
    valid = rec[:, 1] > 0
    if not valid.any():
        return float('nan'), tuple(float('nan') for _ in prak)
    v = rec[valid]
    return float(v[:, 0].sum() / len(v)), tuple(float((v[:, 3 + q] / np.minimum(v[:, 2], k)).sum() / len(v)) for q, k in enumerate(prak))


def reference_map_prak(D, labels, positive_pairs, negative_pairs=None, prak=(1, 5)):
    D = np.asarray(D)
    rec = reference_group_rows(D, labels, range(D.shape[0]), positive_pairs, negative_pairs, prak)
    return group_metrics_from_rows(rec, prak)


def _relation(offsets, members):
    return {a: set(members[offsets[a]:offsets[a + 1]].tolist()) for a in range(len(offsets) - 1)}


def golden_cases():
    """name -> (D [r, n] float16, labels [n], positive_pairs, negative_pairs or None, prak, result)."""
    z = np.load(GOLDEN)
    names = sorted({k.split('__')[0] for k in z.files})
    out = {}
    for n in names:
        neg = _relation(z[f'{n}__neg_offsets'], z[f'{n}__neg_members']) if f'{n}__neg_offsets' in z.files else None
        out[n] = (z[f'{n}__D'], z[f'{n}__labels'].tolist(), _relation(z[f'{n}__pos_offsets'], z[f'{n}__pos_members']), neg,
                  tuple(z[f'{n}__prak'].tolist()), z[f'{n}__result'])
    return out


def assert_close(got, want, atol, what=''):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f'{what}: NaN in different places: {got} vs {want}'
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= atol), f'{what}: {got} vs {want}'


def flat(result):
    m_ap, pr = result
    return [m_ap, *pr]


# ---- the distance maps of geshaem_test ------------------------------------------------------------
def reference_distance_maps(pairs, scores):
    """michigan.py:188-209 as dicts of lists, then the per-cell reductions of :211-219 in fp64: {(i, j): values},
    {(i, j): fp64 mean}, {(i, j): min}, {(i, j): sample stdev for cells of more than one value}, avg_std, std_std."""
    cells = {}
    for (i, j), s in zip(np.asarray(pairs).tolist(), np.asarray(scores, dtype=np.float32)):
        d = np.float32(1) - s
        cells.setdefault((i, j), []).append(d)
        cells.setdefault((j, i), []).append(d)
    mean = {c: math.fsum(float(x) for x in v) / len(v) for c, v in cells.items()}
    mn = {c: min(v) for c, v in cells.items()}
    std = {c: statistics.stdev([float(x) for x in v]) for c, v in cells.items() if len(v) > 1}
    stds = list(std.values())
    avg_std = math.fsum(stds) / len(stds) if stds else float('nan')
    std_std = statistics.stdev(stds) if len(stds) > 1 else float('nan')
    return cells, mean, mn, std, avg_std, std_std


def reference_geshaem(pairs, scores, fragments, fragment_to_group, prak=(1, 5, 10)):
    """geshaem_test after its loop: the MEAN and MIN maps as matrices over the scored fragments in ascending index (NaN where
    a pair was never scored; the mean rounded once to float32, as the device keeps it), then calc_map_prak on each."""
    cells, mean, mn, _, avg_std, std_std = reference_distance_maps(pairs, scores)
    idx = sorted({i for i, _ in cells})
    at = {a: k for k, a in enumerate(idx)}
    M = np.full((len(idx), len(idx)), np.nan, np.float32)
    N = np.full((len(idx), len(idx)), np.nan, np.float32)
    for (i, j), v in mean.items():
        M[at[i], at[j]] = np.float32(v)
        N[at[i], at[j]] = mn[(i, j)]
    labels = [fragments[a] for a in idx]
    return (reference_map_prak(M, labels, fragment_to_group, prak=prak), reference_map_prak(N, labels, fragment_to_group, prak=prak),
            avg_std, std_std, len(idx))


# ---- tests ----------------------------------------------------------------------------------------
def test_golden_fixture_covers_the_cases():
    cases = golden_cases()
    assert any(neg is None for _, _, _, neg, _, _ in cases.values()) and any(neg is not None for _, _, _, neg, _, _ in cases.values())
    big = cases['biggroup_n2600_r24']
    assert max(len(v) for v in big[2].values()) > 2048                                  # several LDS passes of correct columns
    D, labels, pos, neg, prak, _ = cases['singletons_n70_bigk']
    rec = reference_group_rows(D, labels, range(D.shape[0]), pos, neg, prak)
    assert (rec[:, 1] == 0).any()                                                       # rows without a correct retrieval
    assert (rec[rec[:, 1] > 0, 2] < max(prak)).any()                                    # k above a row's hit count
    D = cases['offdiag_repeated_n90'][0].astype(np.float32)
    assert (np.argmin(D, axis=1) != np.arange(D.shape[0])).sum() > D.shape[0] // 2      # the self column is not first
    assert len(set(cases['offdiag_repeated_n90'][1])) < len(cases['offdiag_repeated_n90'][1])   # labels repeated


@pytest.mark.parametrize('name', sorted(golden_cases()))
def test_restatement_matches_reference(name):
    D, labels, pos, neg, prak, want = golden_cases()[name]
    rec = reference_group_rows(D, labels, range(D.shape[0]), pos, neg, prak)
    assert_close(flat(group_metrics_from_rows(rec, prak)), want, 1e-12, name)


def test_stable_ties_nan_and_negative_filter():
    """Ties go to the lower column, NaN sorts last; the negative filter drops columns before the first one is skipped."""
    D = np.array([[0.0, 0.5, 0.5, np.nan, 0.2],
                  [0.1, 0.0, 0.1, 0.1, 0.1]], dtype=np.float32)
    labels = ['a', 'b', 'c', 'd', 'e']
    pos = {'a': {'a', 'c', 'd'}, 'b': {'b', 'e'}}
    neg = {'a': {'b'}, 'b': {'z'}}
    # row 0: order a, e, b, c, d -> skip a; e (miss), b (miss), c (hit @3), d (hit @4)
    rec = reference_group_rows(D, labels, [0, 1], pos, None, (1, 3))
    np.testing.assert_allclose(rec[0], [(1 / 3 + 2 / 4) / 2, 1, 2, 0, 1])
    # row 1: order b, a, c, d, e -> skip b; a, c, d (misses), e (hit @4)
    np.testing.assert_allclose(rec[1], [1 / 4, 1, 1, 0, 0])
    # with negatives row 0 keeps a, b, c, d: order a, b, c, d -> skip a; b (miss), c (hit @2), d (hit @3)
    rec = reference_group_rows(D, labels, [0, 1], pos, neg, (1, 3))
    np.testing.assert_allclose(rec[0], [(1 / 2 + 2 / 3) / 2, 1, 2, 0, 2])
    # row 1 keeps b, e: skip b; e (hit @1)
    np.testing.assert_allclose(rec[1], [1, 1, 1, 1, 1])


def test_distance_maps_restatement():
    pairs = np.array([[0, 0], [0, 1], [0, 1], [1, 2], [2, 2]])
    scores = np.array([0.25, 0.5, 0.75, 0.125, 0.0], dtype=np.float32)
    cells, mean, mn, std, avg_std, std_std = reference_distance_maps(pairs, scores)
    assert cells[(0, 0)] == [0.75, 0.75] and cells[(0, 1)] == cells[(1, 0)] == [0.5, 0.25] and cells[(2, 2)] == [1.0, 1.0]
    assert mean[(0, 1)] == 0.375 and mn[(1, 0)] == 0.25 and (1, 2) not in std and std[(0, 0)] == 0.0
    want = [0.0, statistics.stdev([0.5, 0.25]), statistics.stdev([0.5, 0.25]), 0.0]
    assert avg_std == pytest.approx(sum(want) / 4) and std_std == pytest.approx(statistics.stdev(want))


def test_new_entries_are_exported(vited):
    for name in NEW_ENTRIES:
        assert name in vited._lib.SIGNATURES
        assert name in vited._lib.header_declared_functions()
    if not os.path.exists(vited._lib.LIB_PATH):
        pytest.fail(f'{vited._lib.LIB_PATH} is not built')
    out = subprocess.run(['nm', '-D', '--defined-only', vited._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if ' T vited_' in l}
    assert set(NEW_ENTRIES) <= exported


def test_group_metrics_abi_rejects_bad_arguments(vited):
    """vited_group_retrieval_metrics validates before launching, so bad arguments are safe to pass without a GPU."""
    lib = vited._lib.load()
    buf = ctypes.create_string_buffer(1024)
    p = ctypes.addressof(buf)
    ks = (ctypes.c_int * 3)(1, 5, 10)
    k0 = (ctypes.c_int * 2)(1, 0)
    call = lambda **kw: lib.vited_group_retrieval_metrics(*{**dict(
        D=p, dtype=2, ld=8, n=8, r0=0, r1=8, labels=p, L=4, col_off=p, col_mem=p, pos_off=p, pos_lab=p, neg_off=None, neg_lab=None,
        ks=ctypes.addressof(ks), nk=3, rows_out=p, sums=p, stream=None), **kw}.values())
    assert call(D=None) == 1 and call(labels=None) == 1 and call(col_mem=None) == 1 and call(pos_off=None) == 1
    assert call(ks=None) == 1 and call(sums=None) == 1 and call(rows_out=None) == 1
    assert call(neg_off=p) == 1 and call(neg_lab=p) == 1                   # the negative CSR comes whole or not at all
    assert call(ld=7) == 1 and call(n=0) == 1 and call(L=0) == 1 and call(L=9) == 1
    assert call(r0=-1) == 1 and call(r1=9) == 1 and call(r0=4, r1=4) == 1
    assert call(nk=0) == 1 and call(nk=9) == 1 and call(ks=ctypes.addressof(k0), nk=2) == 1
    assert call(D=p + 1) == 1
    assert call(dtype=7) == 2


def test_pair_scores_abi_rejects_bad_arguments(vited):
    lib = vited._lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    assert lib.vited_pair_scores_workspace_bytes(0, 10) == -1 and lib.vited_pair_scores_workspace_bytes(46341, 10) == -1
    assert lib.vited_pair_scores_workspace_bytes(4, -1) == -1
    ws = lib.vited_pair_scores_workspace_bytes(4, 10)
    assert ws >= 8 * 17 + 4 * 16 * 2 + 8 * 20 * 2
    add = lambda **kw: lib.vited_pair_scores_add(*{**dict(pairs=p, pdt=3, ld=2, scores=p, sdt=0, m=10, n=4, counts=p, cells=p, vals=p,
                                                          bad=p, stream=None), **kw}.values())
    assert add(pairs=None) == 1 and add(scores=None) == 1 and add(counts=None) == 1 and add(bad=None) == 1
    assert add(m=0) == 1 and add(n=0) == 1 and add(n=46341) == 1 and add(ld=1) == 1
    assert add(pairs=p + 2) == 1 and add(scores=p + 2) == 1
    assert add(pdt=0) == 2 and add(sdt=3) == 2
    fin = lambda **kw: lib.vited_pair_scores_finish(*{**dict(cells=p, vals=p, m=10, n=4, counts=p, mean=p, minv=p, std=p, stats=p, bad=p,
                                                             ws=p, ws_bytes=ws, stream=None), **kw}.values())
    assert fin(counts=None) == 1 and fin(mean=None) == 1 and fin(stats=None) == 1 and fin(ws=None) == 1
    assert fin(cells=None) == 1 and fin(n=0) == 1 and fin(m=-1) == 1 and fin(ws=p + 8) == 1
    assert fin(ws_bytes=ws - 1) == 4


def test_ops_refuse_cpu_tensors(vited):
    from vited_amd import engine, ops
    D = torch.rand(6, 6)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        engine.map_prak(D, list('aabbcc'), {c: {c} for c in 'abc'})
    rel = engine.group_relations(list('aabbcc'), {c: {c} for c in 'abc'}, None, 'cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.group_retrieval_metrics_rows(D, *rel, (1, 5), (0, 6))
    agg = engine.PairScoreAggregator(3, 'cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        agg.add(torch.tensor([[0, 1]]), torch.tensor([0.5]))


def test_map_prak_missing_row_label_raises_key_error(vited):
    from vited_amd import engine
    with pytest.raises(KeyError):
        engine.group_relations(['a', 'b'], {'a': {'a'}}, None, 'cpu')
    with pytest.raises(KeyError):
        engine.group_relations(['a', 'b'], {'a': {'a'}, 'b': {'b'}}, {'a': set()}, 'cpu')
    engine.group_relations(['a', 'b'], {'a': {'a'}}, None, 'cpu', rows=(0, 1))            # row 'b' is not in the share
