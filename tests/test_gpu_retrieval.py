"""GPU: vited_retrieval_metrics (engine.retrieval_metrics) against the reference's own get_metrics outputs
(tests/golden/wi19_metrics.npz) and against the stable numpy restatement in test_retrieval_metrics.py: heavy ties, NaN / inf,
a class larger than one LDS chunk of positives, from_similarity, row shards, determinism, and n = 20,000."""
import numpy as np
import pytest
import torch

from test_retrieval_metrics import (assert_metrics_equal, golden_cases, metrics_from_rows, reference_metrics, reference_rows,
                                    reference_rows_of)

pytestmark = pytest.mark.gpu


def _csr(labels, dev):
    from vited_amd import engine
    return engine.class_members(torch.as_tensor(labels, device=dev))


def _rows(D, labels, rows=None, remove=True, sim=False):
    from vited_amd import ops
    ids, off, mem = _csr(labels, D.device)
    rows = (0, D.shape[0]) if rows is None else rows
    rec, sums = ops.retrieval_metrics_rows(D, ids, off, mem, rows, remove_self_column=remove, from_similarity=sim)
    torch.cuda.synchronize()
    return rec.cpu().numpy(), sums.cpu()


def _check_rows(got, want, what):
    np.testing.assert_array_equal(got[:, 1:], want[:, 1:], err_msg=what)                 # counts and hits: exact
    np.testing.assert_allclose(got[:, 0], want[:, 0], rtol=1e-10, atol=1e-12, err_msg=what)   # sums of up to n terms, another order


def _tied(rng, n, levels, classes):
    """Values k / 256, k < levels <= 256: exact in float16 and bfloat16 too."""
    D = rng.integers(0, levels, size=(n, n)).astype(np.float32) / 256
    return D, rng.integers(0, classes, size=n)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('name', sorted(golden_cases()))
def test_golden_cases(gpu, name, dtype):
    from vited_amd import engine
    D, labels, remove, want = golden_cases()[name]
    got = engine.retrieval_metrics(torch.from_numpy(D).to(gpu, dtype), torch.from_numpy(labels).to(gpu), remove_self_column=remove)
    assert got[1] == want[1], (got, want)                                               # top-1: exact
    assert_metrics_equal(got, want, 1e-6, f'{name} {dtype}')


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize('remove', [True, False])
def test_heavy_ties_match_stable_order(gpu, dtype, remove):
    """~50 distinct values per matrix: the order inside each tie is the column order.  The matrix is a strided view whose
    rows start at every alignment, so the unaligned head, the 16-byte body and the tail of the row stream all run."""
    rng = np.random.default_rng(1)
    n = 777
    D, labels = _tied(rng, n, 50, 60)
    big = torch.zeros((n, n + 5), dtype=dtype, device=gpu)
    view = big[:, 3:n + 3]
    view.copy_(torch.from_numpy(D))
    assert torch.equal(view.float().cpu(), torch.from_numpy(D))                          # exact in every dtype
    got, sums = _rows(view, labels, remove=remove)
    want = reference_rows(D, labels, remove)
    _check_rows(got, want, f'{dtype} remove={remove}')
    from vited_amd import engine
    assert_metrics_equal(engine.metrics_from_sums(sums), metrics_from_rows(want), 1e-12)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_nan_and_inf(gpu, dtype):
    rng = np.random.default_rng(2)
    n = 300
    D, labels = _tied(rng, n, 40, 30)
    D -= 0.5
    u = rng.random((n, n))
    D[u < 0.05] = np.nan
    D[(u >= 0.05) & (u < 0.08)] = np.inf
    D[(u >= 0.08) & (u < 0.11)] = -np.inf
    D[(u >= 0.11) & (u < 0.13)] = -0.0                                                   # ties with +0.0
    D[:5] = np.nan                                                                       # whole rows of NaN
    got, _ = _rows(torch.from_numpy(D).to(gpu, dtype), labels)
    _check_rows(got, reference_rows(D, labels), str(dtype))


def test_class_larger_than_one_chunk(gpu):
    """6,000 of 8,000 columns in one class: the positives come in several LDS chunks, each re-streaming the row."""
    rng = np.random.default_rng(3)
    n = 8000
    labels = np.where(rng.random(n) < 0.75, 0, rng.integers(1, 200, n))
    labels[rng.permutation(n)[:6000]] = 0
    assert (labels == 0).sum() >= 6000
    D = (rng.integers(0, 3000, size=(n, n)) / 3000.0).astype(np.float16)
    rows = np.concatenate([np.flatnonzero(labels == 0)[:150], np.flatnonzero(labels != 0)[:50]])
    got, _ = _rows(torch.from_numpy(D).to(gpu), labels)
    _check_rows(got[rows], reference_rows(D, labels, rows=rows), 'chunked')


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float32])
def test_from_similarity_is_bit_identical_to_one_minus_s(gpu, dtype):
    torch.manual_seed(4)
    n = 513
    S = (torch.randn(n, n, device=gpu) * 3).to(dtype)
    labels = torch.randint(0, 40, (n,), device=gpu)
    a_rec, a_sums = _rows(S, labels, sim=True)
    b_rec, b_sums = _rows(1 - S, labels)
    assert np.array_equal(a_rec, b_rec) and torch.equal(a_sums, b_sums)
    from vited_amd import engine
    if dtype == torch.float16:                                                           # the hisfrag flow, one rank
        want = reference_metrics((1 - S).cpu().numpy(), labels.cpu().numpy())
        assert_metrics_equal(engine.hisfrag_retrieval_metrics(S, labels), want, 1e-12)


def test_row_shards_combine_and_runs_are_bit_identical(gpu):
    from vited_amd import engine
    rng = np.random.default_rng(5)
    n = 1001
    D, labels = _tied(rng, n, 200, 50)
    Dg = torch.from_numpy(D).to(gpu, torch.float16)
    full, full_sums = _rows(Dg, labels)
    again, again_sums = _rows(Dg, labels)
    assert np.array_equal(full, again) and torch.equal(full_sums, again_sums)
    a = 377
    lo, lo_sums = _rows(Dg, labels, rows=(0, a))
    hi, hi_sums = _rows(Dg, labels, rows=(a, n))
    assert np.array_equal(np.concatenate([lo, hi]), full)
    assert_metrics_equal(engine.metrics_from_sums(lo_sums + hi_sums), engine.metrics_from_sums(full_sums), 1e-12)
    lab = torch.from_numpy(labels).to(gpu)
    one = engine.retrieval_metrics(Dg, lab)
    assert engine.retrieval_metrics(Dg, lab) == one
    assert_metrics_equal(one, reference_metrics(D.astype(np.float16), labels), 1e-12)


def test_bad_arguments_raise(gpu):
    from vited_amd import engine
    D = torch.rand(16, 16, device=gpu)
    lab = torch.randint(0, 3, (16,), device=gpu)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        engine.retrieval_metrics(D.cpu(), lab)
    with pytest.raises(ValueError, match='length 16'):
        engine.retrieval_metrics(D, lab[:15])
    with pytest.raises(ValueError, match='rows'):
        engine.retrieval_metrics(D, lab, rows=(4, 17))
    with pytest.raises(ValueError, match='rows'):
        engine.retrieval_metrics(D, lab, rows=(-1, 3))
    with pytest.raises(ValueError, match='square'):
        engine.retrieval_metrics(D[:8], lab[:8])
    with pytest.raises(TypeError, match='integer'):
        engine.retrieval_metrics(D, lab.float())
    assert all(np.isnan(engine.retrieval_metrics(D, lab, rows=(5, 5))))                 # an empty share alone: no rows


def test_n20000_full_matrix(gpu):
    """The scale of a hisfrag validation: the whole matrix in one call, checked on 200 rows."""
    from vited_amd import engine
    n = 20000
    g = torch.Generator(device=gpu).manual_seed(6)
    labels = torch.randint(0, 2000, (n,), device=gpu, generator=g)
    D = torch.rand((n, n), device=gpu, generator=g).to(torch.float16)
    D -= 0.3 * (labels[:, None] == labels[None, :]).to(torch.float16)
    got, sums = _rows(D, labels)
    assert int(sums[6]) == n and np.isfinite(got).all()
    rows = np.random.default_rng(6).choice(n, 200, replace=False)
    want = reference_rows_of(D[torch.from_numpy(rows).to(gpu)].cpu().numpy(), labels.cpu().numpy(), rows)
    _check_rows(got[rows], want, 'n=20000')
    m = engine.metrics_from_sums(sums)
    assert 0 < m[0] <= 1 and 0 <= m[1] <= 1
