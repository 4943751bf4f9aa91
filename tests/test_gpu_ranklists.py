"""GPU: vited_retrieval_topk (ops.retrieval_topk_rows, engine.retrieval_topk / hisfrag_retrieval_lists) and vited_retrieval_curves
(ops.retrieval_curve_rows, engine.retrieval_curves) against the stable numpy restatement of ranklists_cases.py - exactly: columns,
uint8 hits, tp_at, the int32 records, and the values as fp32 bits (NaNs need only coincide) - and against the reference's own outputs
in tests/golden/wi19_curves.npz.  The large matrices are ranked on a share of their rows only: a row is one workgroup's work,
whatever the other rows hold."""
import numpy as np
import pytest
import torch

import ranklists_cases as rc
from test_retrieval_metrics import assert_metrics_equal, reference_metrics

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16, torch.float32]


def _device_view(M, gpu, misaligned):
    """M on the device; misaligned: with the row stride n + 1 behind an odd element offset, so that the rows start at every alignment."""
    n = M.shape[0]
    if not misaligned:
        return M.to(gpu)
    flat = torch.zeros(n * (n + 1) + 8, dtype=M.dtype, device=gpu)
    view = flat[3:3 + n * (n + 1)].view(n, n + 1)[:, :n]
    view.copy_(M)
    assert view.stride(0) == n + 1 and (view.data_ptr() // M.element_size()) % 2 == 1
    return view


def _topk(Mg, k, rows, labels, remove, sim):
    from vited_amd import ops
    lab = None if labels is None else torch.from_numpy(labels).to(Mg.device, torch.int32)
    idx, val, hit = ops.retrieval_topk_rows(Mg, k, rows, lab, remove_self_column=remove, from_similarity=sim)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy(), None if hit is None else hit.cpu().numpy()


def _check_topk(M, Mg, k, rows, labels, remove, sim, what):
    idx, val, hit = _topk(Mg, k, rows, labels, remove, sim)
    w_idx, w_val, w_hit = rc.reference_topk(M, k, labels, rows, remove, sim)
    assert idx.dtype == np.int32 and val.dtype == np.float32 and idx.shape == (rows[1] - rows[0], k)
    bad = np.flatnonzero((idx != w_idx).any(axis=1))
    assert bad.size == 0, f'{what}: rows {rows[0] + bad[:5]} differ: got {idx[bad[0]][:12]} want {w_idx[bad[0]][:12]}'
    assert rc.same_values(val, w_val), what
    if labels is not None:
        assert hit.dtype == np.uint8 and np.array_equal(hit, w_hit), what


def _curves(Mg, labels, rows, remove, sim, estimate=None, tp_at=None):
    from vited_amd import engine, ops
    ids, off, mem = engine.class_members(torch.from_numpy(labels).to(Mg.device))
    est = None if estimate is None else torch.from_numpy(estimate).to(Mg.device, torch.int32)
    tp, rec = ops.retrieval_curve_rows(Mg, ids, off, mem, rows, remove_self_column=remove, from_similarity=sim, estimate=est, tp_at=tp_at)
    torch.cuda.synchronize()
    return tp, rec


def _check_curves(M, Mg, labels, rows, remove, sim, estimate, what):
    tp, rec = _curves(Mg, labels, rows, remove, sim, estimate)
    w_tp, w_rec = rc.reference_curves(M, labels, rows, remove, sim, estimate)
    assert tp.dtype == torch.int64 and rec.dtype == torch.int32
    assert np.array_equal(tp.cpu().numpy(), w_tp) and np.array_equal(rec.cpu().numpy(), w_rec), what


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('name', sorted(rc.golden_cases()))
def test_golden_cases(gpu, name, dtype):
    """The reference's own order, hits, ROC and F-score (tie-free matrices, so its unstable argsort defines them)."""
    from vited_amd import engine
    c = rc.golden_cases()[name]
    remove, n = bool(c['remove_self']), c['D'].shape[0]
    D = torch.from_numpy(c['D']).to(gpu, dtype)
    labels = torch.from_numpy(c['labels']).to(gpu)
    lists = engine.retrieval_topk(D, n - (1 if remove else 0), labels=labels, remove_self_column=remove)
    assert np.array_equal(lists.indices.cpu().numpy(), c['order'])
    assert np.array_equal(lists.correct.cpu().numpy().astype(bool), c['sorted_retrievals'])
    assert np.array_equal(lists.values.cpu().numpy(), np.take_along_axis(c['D'].astype(np.float32), c['order'].astype(np.int64), axis=1))
    curves = engine.retrieval_curves(D, labels, remove_self_column=remove, relevant_estimate=torch.from_numpy(c['estimate']))
    assert np.array_equal(curves.tp_at.cpu().numpy(), c['sorted_retrievals'].sum(axis=0))
    assert (curves.rows, curves.relevant, curves.retrieved) == (n, int(c['sorted_retrievals'].sum()), int(c['estimate'].sum()))
    roc = curves.roc()
    assert np.array_equal(rc.bits64(roc['fallout'].cpu().numpy()), rc.bits64(c['fallout']))
    assert np.array_equal(rc.bits64(roc['recall'].cpu().numpy()), rc.bits64(c['recall']))
    assert np.array_equal(rc.bits64(curves.fscore()), rc.bits64(c['fscore']))


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('sim', [False, True], ids=['distance', 'similarity'])
@pytest.mark.parametrize('remove', [True, False], ids=['drop', 'keep'])
def test_grid_of_sizes_ties_and_special_values(gpu, dtype, sim, remove):
    """n = 2, 7 and 8 * 256 + 3; rows at every alignment (ld = n + 1, odd offset); k = 1 and k = n - skip (1,024 where that is more);
    rows of one repeated value, of 4 in 5 equal, of scores saturated to 0 and 1, of NaN / inf / -inf / -0 with the minimum off the
    diagonal (ranklists_cases.tied_matrix), and random rows with ties; lists and curves alike."""
    skip = 1 if remove else 0
    for n in (2, 7, 8 * 256 + 3):
        M = rc.tied_matrix(n, dtype, seed=n)
        labels = rc.labels_for(n, 2 if n < 10 else 40, seed=n)
        estimate = np.random.default_rng(n).integers(-1, 60, n)
        rows = (0, min(n, 48))
        for misaligned in (False, True):
            Mg = _device_view(M, gpu, misaligned)
            what = f'n={n} {dtype} sim={sim} remove={remove} misaligned={misaligned}'
            for k in sorted({1, min(n - skip, 1024)}):
                _check_topk(M, Mg, k, rows, labels, remove, sim, f'{what} k={k}')
            _check_topk(M, Mg, min(n - skip, 10), rows, None, remove, sim, what + ' no labels')
            _check_curves(M, Mg, labels, rows, remove, sim, estimate, what)


def test_k_1024_at_n_1500(gpu):
    n = 1500
    M = rc.tied_matrix(n, torch.float16, seed=3)
    Mg = M.to(gpu)
    for remove, sim in ((True, True), (False, False)):
        _check_topk(M, Mg, 1024, (0, 24), rc.labels_for(n, 30), remove, sim, f'k=1024 remove={remove} sim={sim}')


@pytest.mark.parametrize('sim', [False, True], ids=['distance', 'similarity'])
def test_boundary_bin_far_larger_than_the_candidate_buffer(gpu, sim):
    """n = 5,000, k = 100: a row of one value, a row where 4,000 of 5,000 values are equal, a row of saturated scores - the boundary
    bin of every value digit holds thousands of keys, and the column digits cut it down to the lowest columns."""
    n = 5000
    M = rc.tied_matrix(n, torch.float16, seed=4)
    assert int((M[1] == 0.5).sum()) >= 4000 and set(M[2].unique().tolist()) == {0.0, 1.0} and M[0].unique().numel() == 1
    Mg = _device_view(M, gpu, True)
    _check_topk(M, Mg, 100, (0, 8), rc.labels_for(n, 500), True, sim, f'n=5000 sim={sim}')
    _check_topk(M, Mg, 1024, (0, 4), None, False, sim, f'n=5000 k=1024 sim={sim}')


def test_saturated_fp16_scores_in_the_hisfrag_flow(gpu):
    """Sigmoid scores saturated to exactly 0 and 1: every row is two runs of ties.  One rank: all rows."""
    from vited_amd import engine
    n = 300
    rng = np.random.default_rng(5)
    labels = rc.labels_for(n, 30, seed=5)
    S = torch.from_numpy(((labels[:, None] == labels[None, :]) ^ (rng.random((n, n)) < 0.02)).astype(np.float32)).to(torch.float16)
    lists = engine.hisfrag_retrieval_lists(S.to(gpu), 9, torch.from_numpy(labels).to(gpu))
    idx, val, hit = rc.reference_topk(S, 9, labels, None, True, True)
    assert np.array_equal(lists.indices.cpu().numpy(), idx) and np.array_equal(lists.correct.cpu().numpy(), hit)
    assert rc.same_values(lists.values.cpu().numpy(), val) and set(np.unique(val).tolist()) <= {0.0, 1.0}
    assert engine.hisfrag_retrieval_lists(S.to(gpu), 9).correct is None


def test_class_larger_than_one_chunk_in_the_curves(gpu):
    """2,100 of 2,500 columns in one class: the correct columns come in two LDS chunks, each re-streaming the row."""
    n = 2500
    rng = np.random.default_rng(6)
    labels = np.where(np.arange(n) % 25 < 21, 0, rng.integers(1, 60, n))
    assert (labels == 0).sum() == 2100
    M = rc.random_matrix(n, torch.float16, seed=6, levels=512)
    estimate = rng.integers(0, 2400, n)
    Mg = M.to(gpu)
    for remove in (True, False):
        _check_curves(M, Mg, labels, (0, 50), remove, False, estimate, f'chunked remove={remove}')


def test_row_shares_combine_and_runs_are_bit_identical(gpu):
    from vited_amd import engine
    n = 1001
    M = rc.random_matrix(n, torch.float16, seed=7, levels=200)
    labels = rc.labels_for(n, 50, seed=7)
    estimate = np.random.default_rng(7).integers(0, 40, n)
    Mg, a = M.to(gpu), 377
    full = _topk(Mg, 20, (0, n), labels, True, True)
    again = _topk(Mg, 20, (0, n), labels, True, True)
    lo, hi = _topk(Mg, 20, (0, a), labels, True, True), _topk(Mg, 20, (a, n), labels, True, True)
    for f, g, l, h in zip(full, again, lo, hi):
        assert np.array_equal(f.view(np.uint8), g.view(np.uint8)) and np.array_equal(np.concatenate([l, h]).view(np.uint8), f.view(np.uint8))
    _check_topk(M, Mg, 20, (a, a + 40), labels, True, True, 'share r0 > 0')
    tp, rec = _curves(Mg, labels, (0, n), True, True, estimate)
    tp2, rec2 = _curves(Mg, labels, (0, n), True, True, estimate)
    assert torch.equal(tp, tp2) and torch.equal(rec, rec2)
    part, rec_lo = _curves(Mg, labels, (0, a), True, True, estimate)
    part, rec_hi = _curves(Mg, labels, (a, n), True, True, estimate, tp_at=part)                     # added onto the first share
    assert torch.equal(part, tp) and torch.equal(torch.cat([rec_lo, rec_hi]), rec)
    _check_curves(M, Mg, labels, (a, a + 40), True, True, estimate, 'share r0 > 0')
    lab = torch.from_numpy(labels).to(gpu)
    whole = engine.retrieval_curves(Mg, lab, from_similarity=True, relevant_estimate=estimate)
    share = engine.retrieval_curves(Mg, lab, rows=(a, n), from_similarity=True, relevant_estimate=estimate)
    assert torch.equal(whole.tp_at, tp) and whole[1:] == (n, int(rec[:, 0].sum()), int(rec[:, 1].sum()), int(estimate.sum()))
    assert share.rows == n - a and share.retrieved == int(estimate[a:].sum()) and share.relevant == int(rec_hi[:, 0].sum())
    assert engine.retrieval_topk(Mg, 5, rows=(9, 9)).indices.shape == (0, 5)                        # an empty share: no rows


def test_the_metrics_path_is_unchanged_on_the_same_matrices(gpu):
    """engine.retrieval_metrics still equals its restatement on the matrices the new kernels ran on, before and after them."""
    from vited_amd import engine
    for n, dtype in ((7, torch.float32), (8 * 256 + 3, torch.float16), (1001, torch.bfloat16)):
        M = rc.tied_matrix(n, dtype, seed=n)
        labels = rc.labels_for(n, 2 if n < 10 else 40, seed=n)
        Mg, lab = M.to(gpu), torch.from_numpy(labels).to(gpu)
        want = reference_metrics(M.float().numpy(), labels)
        before = engine.retrieval_metrics(Mg, lab)
        engine.retrieval_topk(Mg, min(n - 1, 100), labels=lab)
        engine.retrieval_curves(Mg, lab)
        after = engine.retrieval_metrics(Mg, lab)
        assert_metrics_equal(before, want, 1e-12, f'n={n}')
        assert_metrics_equal(after, before, 0.0, f'n={n}')


def test_every_output_element_is_written_and_nothing_else(gpu, vited):
    """The outputs are pre-filled with a poison pattern, with guard elements behind them: no poison survives inside, all of it outside."""
    from vited_amd import ops
    n, k, r0, r1 = 700, 33, 100, 164
    M = rc.tied_matrix(n, torch.bfloat16, seed=8)
    labels = rc.labels_for(n, 20, seed=8)
    Mg, lab = M.to(gpu), torch.from_numpy(labels).to(gpu, torch.int32)
    m, guard = (r1 - r0) * k, 64
    idx = torch.full((m + guard,), -777, dtype=torch.int32, device=gpu)
    val = torch.full((m + guard,), 0x7fc12345, dtype=torch.int32, device=gpu).view(torch.float32)
    hit = torch.full((m + guard,), 0xAB, dtype=torch.uint8, device=gpu)
    vited._lib.call('vited_retrieval_topk', Mg.data_ptr(), ops._DTYPE[Mg.dtype], Mg.stride(0), n, r0, r1, lab.data_ptr(), k, 1, 0, idx.data_ptr(),
                    val.data_ptr(), hit.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    bits = val.view(torch.int32)
    assert not (idx[:m] == -777).any() and not (bits[:m] == 0x7fc12345).any() and not (hit[:m] == 0xAB).any()
    assert (idx[m:] == -777).all() and (bits[m:] == 0x7fc12345).all() and (hit[m:] == 0xAB).all()
    w_idx, w_val, w_hit = rc.reference_topk(M, k, labels, (r0, r1), True, False)
    assert np.array_equal(idx[:m].view(r1 - r0, k).cpu().numpy(), w_idx) and np.array_equal(hit[:m].view(r1 - r0, k).cpu().numpy(), w_hit)
    assert rc.same_values(val[:m].view(r1 - r0, k).cpu().numpy(), w_val)


def test_bad_arguments_raise(gpu):
    from vited_amd import engine
    D = torch.rand(16, 16, device=gpu)
    lab = torch.randint(0, 3, (16,), device=gpu)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        engine.retrieval_topk(D.cpu(), 3)
    with pytest.raises(ValueError, match='k must be'):
        engine.retrieval_topk(D, 16)
    with pytest.raises(ValueError, match='k must be'):
        engine.retrieval_topk(D, 0, remove_self_column=False)
    with pytest.raises(ValueError, match='length 16'):
        engine.retrieval_topk(D, 3, labels=lab[:15])
    with pytest.raises(TypeError, match='integer'):
        engine.retrieval_curves(D, lab.float())
    with pytest.raises(ValueError, match='rows'):
        engine.retrieval_curves(D, lab, rows=(4, 17))
    assert engine.retrieval_topk(D, 16, remove_self_column=False).indices.sort(dim=1).values.tolist() == [list(range(16))] * 16
