"""GPU: vited_group_retrieval_metrics (engine.map_prak) against the reference's own calc_map_prak outputs
(tests/golden/map_prak.npz) and against the stable numpy restatement in test_pair_metrics.py; vited_pair_scores_* (engine.
PairScoreAggregator) against the dict-of-lists restatement of michigan.py:188-223, including its invariance to batching and
order; the end-to-end geshaem evaluation; and two gloo ranks sharing one GPU."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_pair_metrics import (assert_close, flat, golden_cases, group_metrics_from_rows, reference_distance_maps, reference_geshaem,
                               reference_group_rows)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _rows(D, labels, pos, neg, prak, rows=None):
    from vited_amd import engine, ops
    rows = (0, D.shape[0]) if rows is None else rows
    rel = engine.group_relations(labels, pos, neg, D.device, rows=rows)
    rec, sums = ops.group_retrieval_metrics_rows(D, *rel, prak, rows)
    torch.cuda.synchronize()
    return rec.cpu().numpy(), sums.cpu().numpy()


def _check_rows(got, want, what):
    np.testing.assert_array_equal(got[:, 1:], want[:, 1:], err_msg=what)                       # valid, counts, hits: exact
    np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=1e-10, atol=1e-12, err_msg=what)


def _embed(D, dev, dtype):
    """A [r, n] case as the first r rows of an n x n device matrix (the other rows are not ranked)."""
    r, n = D.shape
    full = torch.zeros((n, n), dtype=dtype, device=dev)
    full[:r] = torch.from_numpy(D.astype(np.float32)).to(dev, dtype)
    return full


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('name', sorted(golden_cases()))
def test_golden_cases(gpu, name, dtype):
    from vited_amd import engine
    D, labels, pos, neg, prak, want = golden_cases()[name]
    got = engine.map_prak(_embed(D, gpu, dtype), labels, pos, neg, prak, rows=(0, D.shape[0]))
    assert_close(flat(got), want, 1e-12, f'{name} {dtype}')


def _random_case(rng, n, num_labels, group, neg_frac=None):
    labels = [f'f{v}' for v in rng.integers(0, num_labels, n)]                                   # labels repeated across columns
    perm = rng.permutation(num_labels)
    pos = {}
    for g0 in range(0, num_labels, group):
        g = {f'f{v}' for v in perm[g0:g0 + group]}
        for a in g:
            pos[a] = g
    neg = None
    if neg_frac is not None:                                                                     # overlapping the positives
        neg = {f'f{a}': {f'f{v}' for v in np.flatnonzero(rng.random(num_labels) < neg_frac)} for a in range(num_labels)}
    return labels, pos, neg


@pytest.mark.parametrize('neg_frac', [None, 0.3])
@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float32])
def test_heavy_ties_match_stable_order(gpu, dtype, neg_frac):
    """~40 distinct values: the order inside each tie is the column order.  A strided view (rows at every alignment)."""
    rng = np.random.default_rng(11)
    n = 555
    D = rng.integers(0, 40, size=(n, n)).astype(np.float32) / 256
    labels, pos, neg = _random_case(rng, n, 120, 6, neg_frac)
    big = torch.zeros((n, n + 5), dtype=dtype, device=gpu)
    view = big[:, 3:n + 3]
    view.copy_(torch.from_numpy(D))
    prak = (1, 3, 10, 700)
    got, sums = _rows(view, labels, pos, neg, prak)
    want = reference_group_rows(D, labels, range(n), pos, neg, prak)
    _check_rows(got, want, f'{dtype} neg={neg_frac}')
    from vited_amd import engine
    assert_close(flat(engine.map_prak(view, labels, pos, neg, prak)), flat(group_metrics_from_rows(want, prak)), 1e-12)


@pytest.mark.parametrize('neg_frac', [None, 0.2])
def test_nan_and_inf(gpu, neg_frac):
    rng = np.random.default_rng(12)
    n = 300
    D = rng.integers(0, 30, size=(n, n)).astype(np.float32) / 64 - 0.2
    u = rng.random((n, n))
    D[u < 0.05] = np.nan
    D[(u >= 0.05) & (u < 0.08)] = np.inf
    D[(u >= 0.08) & (u < 0.11)] = -np.inf
    D[(u >= 0.11) & (u < 0.13)] = -0.0
    D[:4] = np.nan
    labels, pos, neg = _random_case(rng, n, 80, 5, neg_frac)
    got, _ = _rows(torch.from_numpy(D).to(gpu), labels, pos, neg, (1, 5))
    _check_rows(got, reference_group_rows(D, labels, range(n), pos, neg, (1, 5)), f'neg={neg_frac}')


@pytest.mark.parametrize('neg_frac', [None, 0.5])
def test_groups_larger_than_one_lds_chunk(gpu, neg_frac):
    """5,000 columns with labels from 40 values in two groups: ~2,500 correct columns per row, two passes."""
    rng = np.random.default_rng(13)
    n = 5000
    labels, pos, neg = _random_case(rng, n, 40, 20, neg_frac)
    D = rng.random((48, n)).astype(np.float32)
    got, _ = _rows(_embed(D, gpu, torch.float32), labels, pos, neg, (1, 100, 3000), rows=(0, 48))
    want = reference_group_rows(D, labels, range(48), pos, neg, (1, 100, 3000))
    assert want[:, 2].min() > 2048
    _check_rows(got, want, f'neg={neg_frac}')


def test_large_n_row_shards_and_determinism(gpu):
    """n = 20,000 fp16 with groups of ~10 fragments and negatives: shards sum to the whole, repeated runs are bit-identical,
    and sampled rows match the restatement."""
    from vited_amd import engine
    rng = np.random.default_rng(14)
    n = 20000
    labels = [f'f{v}' for v in range(n)]
    perm = rng.permutation(n)
    pos = {}
    for g0 in range(0, n, 10):
        g = {f'f{v}' for v in perm[g0:g0 + 10]}
        for a in g:
            pos[a] = g
    D = torch.rand((n, n), device=gpu, dtype=torch.float32).to(torch.float16)
    prak = (1, 5, 10)
    whole = engine.map_prak(D, labels, pos, None, prak)
    again = engine.map_prak(D, labels, pos, None, prak)
    assert flat(whole) == flat(again)                                                             # bit-identical
    rel = engine.group_relations(labels, pos, None, gpu)
    from vited_amd import ops
    _, s_all = ops.group_retrieval_metrics_rows(D, *rel, prak, (0, n))
    bounds = engine.shard_rows_by_pair_count(n, 3)
    parts = [ops.group_retrieval_metrics_rows(D, *rel, prak, (bounds[r], bounds[r + 1]))[1] for r in range(3)]
    np.testing.assert_allclose(sum(p.cpu().numpy() for p in parts), s_all.cpu().numpy(), rtol=1e-12)
    rows = np.sort(rng.choice(n, 40, replace=False))
    Dr = D[torch.from_numpy(rows).to(gpu)].float().cpu().numpy()
    got, _ = _rows(D, labels, pos, None, prak)
    _check_rows(got[rows], reference_group_rows(Dr, labels, rows, pos, None, prak), 'n=20000')
    neg = {labels[i]: {f'f{v}' for v in rng.integers(0, n, 200)} for i in range(100, 140)}   # the rows' labels only
    got_neg = engine.map_prak(D, labels, pos, neg, prak, rows=(100, 140))
    want = group_metrics_from_rows(reference_group_rows(D[100:140].float().cpu().numpy(), labels, range(100, 140), pos, neg, prak), prak)
    assert_close(flat(got_neg), flat(want), 1e-12, 'n=20000 negatives')


# ---- aggregation ---------------------------------------------------------------------------------
def _records(rng, n_patches, n_frag):
    """Every patch pair (i <= j, as combinations(..., with_replacement=True)) of a random patch -> fragment map (some fragments
    with one patch, so cells with one record), scores in (0, 1) as float32."""
    frag = np.sort(np.concatenate([np.arange(3), rng.integers(3, n_frag, n_patches - 3)]))   # fragments 0-2: one patch each
    i, j = np.triu_indices(n_patches)
    pairs = np.stack([frag[i], frag[j]], axis=1)
    scores = rng.random(len(pairs)).astype(np.float32)
    return pairs, scores


def _aggregate(gpu, n, batches):
    from vited_amd import engine
    agg = engine.PairScoreAggregator(n, gpu)
    for p, s in batches:
        agg.add(torch.from_numpy(p), torch.from_numpy(s).to(gpu))
    res = agg.finish()
    torch.cuda.synchronize()
    return res


def _bits(res):
    return [t.cpu().numpy().tobytes() for t in (res.mean, res.min, res.count, res.std)] + [np.float64(res.std_stats).tobytes()]


def test_aggregation_matches_dict_of_lists(gpu):
    rng = np.random.default_rng(21)
    n = 30
    pairs, scores = _records(rng, 150, n)
    res = _aggregate(gpu, n, [(pairs, scores)])
    cells, mean, mn, std, avg_std, std_std = reference_distance_maps(pairs, scores)
    count = res.count.cpu().numpy()
    got_mean, got_min, got_std = res.mean.cpu().numpy(), res.min.cpu().numpy(), res.std.cpu().numpy()
    want_count = np.zeros((n, n), np.int32)
    for (a, b), v in cells.items():
        want_count[a, b] = len(v)
        assert got_min[a, b] == mn[(a, b)]
        assert abs(float(got_mean[a, b]) - mean[(a, b)]) <= np.spacing(np.float32(mean[(a, b)]))
        if len(v) > 1:
            assert abs(got_std[a, b] - std[(a, b)]) <= 1e-12 * max(std[(a, b)], 1e-300)
        else:
            assert np.isnan(got_std[a, b])
    np.testing.assert_array_equal(count, want_count)
    assert (count == 1).any() and (count > 32).any()                                             # one-record and workgroup cells
    assert np.isnan(got_mean[count == 0]).all() and np.isnan(got_min[count == 0]).all()
    assert res.std_stats[0] == pytest.approx(avg_std, rel=1e-12) and res.std_stats[1] == pytest.approx(std_std, rel=1e-12)


def test_aggregation_large_cells(gpu):
    """Cells above the LDS sort (8,192 values) and between: rank placement and bitonic paths against the restatement."""
    rng = np.random.default_rng(22)
    pairs = np.concatenate([np.zeros((9000, 2), int), np.tile([[0, 1]], (3000, 1)), np.tile([[2, 2]], (20, 1))])
    scores = rng.integers(0, 500, len(pairs)).astype(np.float32) / 512                          # many equal values
    res = _aggregate(gpu, 3, [(pairs, scores)])
    cells, mean, mn, std, _, _ = reference_distance_maps(pairs, scores)
    for (a, b), v in cells.items():
        assert res.min[a, b].item() == mn[(a, b)]
        assert abs(res.mean[a, b].item() - mean[(a, b)]) <= np.spacing(np.float32(mean[(a, b)]))
        assert abs(res.std[a, b].item() - std[(a, b)]) <= 1e-12 * std[(a, b)]
    assert res.count[0, 0].item() == 18000


def test_aggregation_is_invariant_to_batching_and_order(gpu):
    rng = np.random.default_rng(23)
    n = 200
    pairs, scores = _records(rng, 600, n)
    ref = _bits(_aggregate(gpu, n, [(pairs, scores)]))
    assert _bits(_aggregate(gpu, n, [(pairs, scores)])) == ref                                   # repeat run
    for sizes in ((1000, 7), (33333,), (4096, 1)):
        perm = rng.permutation(len(pairs))
        cuts, at, batches = list(sizes), 0, []
        while at < len(perm):
            k = cuts[len(batches) % len(cuts)]
            idx = perm[at:at + k]
            batches.append((pairs[idx], scores[idx]))
            at += k
        assert _bits(_aggregate(gpu, n, batches)) == ref, sizes
    # the same records as int32 pairs on the device and bfloat16-exact scores keep the result
    res = _aggregate(gpu, n, [(pairs.astype(np.int32), scores)])
    assert _bits(res) == ref


def test_aggregation_rejects_out_of_range_ids(gpu):
    from vited_amd import engine
    agg = engine.PairScoreAggregator(4, gpu)
    agg.add(torch.tensor([[0, 1], [2, 4]]), torch.tensor([0.5, 0.5], device=gpu))
    with pytest.raises(ValueError, match='outside'):
        agg.finish()


def test_end_to_end_geshaem(gpu):
    """Scores -> aggregator -> geshaem_pair_metrics equals the restated geshaem_test, MEAN and MIN.  Fragment 3 is never scored
    and is left out; batches come in the loader's order, in bfloat16 as autocast gives them."""
    from vited_amd import engine
    rng = np.random.default_rng(24)
    n_frag = 40
    frag = np.sort(np.concatenate([rng.choice([a for a in range(n_frag) if a != 3], 120), np.arange(n_frag)[np.arange(n_frag) != 3]]))
    i, j = np.triu_indices(len(frag))
    pairs = np.stack([frag[i], frag[j]], axis=1)
    scores = torch.rand(len(pairs), device=gpu).to(torch.bfloat16)
    fragments = [f'P{a:03d}' for a in range(n_frag)]
    perm = rng.permutation(n_frag)
    groups = {}
    for g0 in range(0, n_frag, 4):
        g = {fragments[a] for a in perm[g0:g0 + 4]}
        for a in g:
            groups[a] = g
    agg = engine.PairScoreAggregator(n_frag, gpu)
    for b0 in range(0, len(pairs), 4096):
        agg.add(torch.from_numpy(pairs[b0:b0 + 4096]), scores[b0:b0 + 4096])
    got = engine.geshaem_pair_metrics(agg, fragments, groups)
    want_mean, want_min, avg_std, std_std, n_cat = reference_geshaem(pairs, scores.float().cpu().numpy(), fragments, groups)
    assert got.n_categories == n_cat == n_frag - 1
    assert_close(flat(got.mean), flat(want_mean), 1e-12, 'MEAN')
    assert_close(flat(got.min), flat(want_min), 1e-12, 'MIN')
    assert got.avg_std == pytest.approx(avg_std, rel=1e-12) and got.std_std == pytest.approx(std_std, rel=1e-12)


# ---- two gloo ranks on one GPU ---------------------------------------------------------------------
def _gloo_case():
    rng = np.random.default_rng(31)
    n = 400
    labels = [f'f{v}' for v in range(n)]
    perm = rng.permutation(n)
    pos = {}
    for g0 in range(0, n, 8):
        g = {f'f{v}' for v in perm[g0:g0 + 8]}
        for a in g:
            pos[a] = g
    neg = {a: {f'f{v}' for v in rng.integers(0, n, 60)} for a in labels}
    D = rng.random((n, n)).astype(np.float32)
    return D, labels, pos, neg


def _gloo_worker(rank, world, port, out):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import vited_amd  # noqa: F401
    from vited_amd import engine
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', init_method=f'tcp://127.0.0.1:{port}', rank=rank, world_size=world)
    D, labels, pos, neg = _gloo_case()
    Dg = torch.from_numpy(D).cuda()
    bounds = engine.shard_rows_by_pair_count(D.shape[0], world)
    share = (bounds[rank], bounds[rank + 1])
    res = {'pos': engine.map_prak(Dg, labels, pos, None, (1, 5, 10), rows=share, group=dist.group.WORLD),
           'neg': engine.map_prak(Dg, labels, pos, neg, (1, 5, 10), rows=share, group=dist.group.WORLD)}
    torch.cuda.synchronize()
    gathered = [None] * world
    dist.all_gather_object(gathered, res)
    if rank == 0:
        torch.save(gathered, out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_one_process(gpu, tmp_path):
    from vited_amd import engine
    out = str(tmp_path / 'r.pt')
    port = 29700 + (os.getpid() % 90)
    mp.spawn(_gloo_worker, args=(2, port, out), nprocs=2, join=True)
    per_rank = torch.load(out, weights_only=False)
    D, labels, pos, neg = _gloo_case()
    Dg = torch.from_numpy(D).to(gpu)
    for key, rel in (('pos', None), ('neg', neg)):
        one = engine.map_prak(Dg, labels, pos, rel, (1, 5, 10))
        for r, res in enumerate(per_rank):
            assert_close(flat(res[key]), flat(one), 1e-12, f'{key} rank {r}')
