"""CPU: the numpy restatement of the ranked lists and the wi19 curves (ranklists_cases.py, a STABLE argsort of the 64-bit key)
against the reference's own get_sorted_retrievals / compute_roc / compute_fscore outputs stored in tests/golden/wi19_curves.npz;
the tie / NaN / -0 rule on a hand-written row; the argument checks of the wrappers and of the C ABI, which run before any launch;
the host program of the selection arithmetic, plain and under the sanitizers; and the cross-rank combine of
engine.hisfrag_retrieval_lists / retrieval_curves over gloo.  The GPU kernels are checked against the restatement in
tests/test_gpu_ranklists.py."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ranklists_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_golden_fixture_covers_the_cases():
    cases = rc.golden_cases()
    assert {c['D'].shape[0] for c in cases.values()} >= {40, 150}
    assert any(not c['remove_self'] for c in cases.values()) and any(c['remove_self'] for c in cases.values())
    assert any((c['sorted_retrievals'].sum(axis=1) == 0).any() for c in cases.values())          # a singleton class
    D = cases['offdiag_n150_c12']['D']
    assert (np.argmin(D, axis=1) != np.arange(150)).sum() > 75                                    # the self-column rule matters there
    for c in cases.values():
        assert all(np.unique(row).size == row.size for row in c['D'].astype(np.float32))         # the reference defines no order under ties
    assert os.path.getsize(rc.GOLDEN) < 400 * 1024


@pytest.mark.parametrize('name', sorted(rc.golden_cases()))
def test_restatement_matches_reference(name):
    c = rc.golden_cases()[name]
    D, labels, remove = c['D'], c['labels'], bool(c['remove_self'])
    n = D.shape[0]
    skip = 1 if remove else 0
    idx, val, hit = rc.reference_topk(D, n - skip, labels, remove_self_column=remove)
    assert np.array_equal(idx, c['order']) and np.array_equal(hit.astype(bool), c['sorted_retrievals'])
    assert np.array_equal(val, np.take_along_axis(D.astype(np.float32), c['order'].astype(np.int64), axis=1))
    tp_at, rec = rc.reference_curves(D, labels, remove_self_column=remove, estimate=c['estimate'])
    assert np.array_equal(tp_at, c['sorted_retrievals'].sum(axis=0)) and np.array_equal(rec[:, 0], c['sorted_retrievals'].sum(axis=1))
    roc = rc.roc_of(tp_at, n)
    assert np.array_equal(rc.bits64(roc['fallout']), rc.bits64(c['fallout'])) and np.array_equal(rc.bits64(roc['recall']), rc.bits64(c['recall']))
    f = rc.fscore_of(rec[:, 1].sum(), c['estimate'].sum(), rec[:, 0].sum())
    assert np.array_equal(rc.bits64(f), rc.bits64(c['fscore']))


@pytest.mark.parametrize('name', sorted(rc.golden_cases()))
def test_curves_object_forms_roc_and_fscore_as_the_reference(vited, name):
    """RetrievalCurves.roc() / .fscore() from the restated counts: the reference's float64 bits."""
    from vited_amd import engine
    c = rc.golden_cases()[name]
    tp_at, rec = rc.reference_curves(c['D'], c['labels'], remove_self_column=bool(c['remove_self']), estimate=c['estimate'])
    curves = engine.RetrievalCurves(torch.from_numpy(tp_at), c['D'].shape[0], int(rec[:, 0].sum()), int(rec[:, 1].sum()), int(c['estimate'].sum()))
    roc = curves.roc()
    assert roc['fallout'].dtype == torch.float64 and roc['recall'].dtype == torch.float64
    assert np.array_equal(rc.bits64(roc['fallout'].numpy()), rc.bits64(c['fallout']))
    assert np.array_equal(rc.bits64(roc['recall'].numpy()), rc.bits64(c['recall']))
    assert np.array_equal(rc.bits64(curves.fscore()), rc.bits64(c['fscore']))
    empty = engine.RetrievalCurves(torch.zeros(5, dtype=torch.int64), 0, 0, 0, 0)                   # zero denominators: NaN, as numpy
    assert torch.isnan(empty.roc()['fallout']).all() and torch.isnan(empty.roc()['recall']).all() and all(np.isnan(empty.fscore()))
    with pytest.raises(ValueError, match='relevant_estimate'):
        engine.RetrievalCurves(torch.zeros(5, dtype=torch.int64), 1, 0, None, None).fscore()


def test_stable_ties_nan_and_signed_zero_order():
    """Ties go to the lower column, NaN sorts after +inf (NaNs tie with each other), -0 ties with +0; the dropped element is the
    first of that order, not the diagonal."""
    nan, inf = np.nan, np.inf
    D = np.array([[1.0, 0.0, -0.0, nan, -0.0, 0.5],
                  [inf, 1.0, nan, 0.5, -inf, nan],
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                  [nan, nan, -inf, nan, inf, 2.0],
                  [0.5, 0.5, 0.25, 0.5, 0.25, 0.5],
                  [1.0, 0.0, 1.0, 0.0, 1.0, 0.0]], dtype=np.float32)
    labels = np.array([0, 1, 0, 1, 0, 1])
    idx, val, hit = rc.reference_topk(D, 6, labels, remove_self_column=False)
    assert idx.tolist() == [[1, 2, 4, 5, 0, 3], [4, 3, 1, 0, 2, 5], [0, 1, 2, 3, 4, 5], [2, 5, 4, 0, 1, 3], [2, 4, 0, 1, 3, 5],
                            [1, 3, 5, 0, 2, 4]]
    assert hit[0].tolist() == [0, 1, 1, 0, 1, 0]
    assert np.signbit(val[0, :3]).tolist() == [False, True, True]                                   # the values are the matrix' own bits
    idx1, _, hit1 = rc.reference_topk(D, 3, labels, remove_self_column=True)
    assert idx1.tolist() == [row[1:4] for row in idx.tolist()] and hit1[1].tolist() == [1, 1, 0]     # row 1 drops column 4, not itself
    # from_similarity ranks by T(1 - S): the order of row 4 reverses between the two values, ties still to the lower column
    assert rc.reference_topk(D, 6, remove_self_column=False, from_similarity=True)[0][4].tolist() == [0, 1, 3, 5, 2, 4]
    tp_at, rec = rc.reference_curves(D, labels, remove_self_column=True, estimate=np.array([2, 0, 9, 1, 3, -4]))
    assert rec.tolist() == [[3, 2], [3, 0], [2, 2], [3, 1], [2, 2], [2, 0]]                          # the query itself counts when it is not the dropped one
    assert tp_at.tolist() == [5, 5, 0, 3, 2]


def test_wrappers_refuse_bad_arguments_before_any_launch(vited, monkeypatch):
    from vited_amd import engine, ops
    calls = []
    D = torch.rand(8, 8)
    lab = torch.zeros(8, dtype=torch.int32)
    csr = (torch.tensor([0, 8], dtype=torch.int32), torch.arange(8, dtype=torch.int32))
    for call in (lambda: ops.retrieval_topk_rows(D, 3, (0, 8)), lambda: ops.retrieval_curve_rows(D, lab, *csr, (0, 8)),
                 lambda: engine.retrieval_topk(D, 3), lambda: engine.retrieval_curves(D, lab), lambda: engine.hisfrag_retrieval_lists(D, 3)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):                                  # CPU tensors: there is no fallback
            call()
    # past the device gate (stubbed) every other fault is refused by the checker; nothing reaches the library
    monkeypatch.setattr(ops, '_need_gpu', lambda *tensors, **kw: None)
    monkeypatch.setattr(ops, '_stream', lambda: 0)
    monkeypatch.setattr(ops, '_lib', type('L', (), {'call': staticmethod(lambda name, *args: calls.append(name))}))
    topk, curves = ops.retrieval_topk_rows, ops.retrieval_curve_rows
    for k in (0, -1, 8, 1025):                                                                       # k = 0, k + skip > n, k > 1024
        with pytest.raises(ValueError, match=r'^retrieval_topk_rows: k must be'):
            topk(D, k, (0, 8))
    with pytest.raises(ValueError, match='at most 1024'):
        topk(torch.rand(2000, 2000), 1025, (0, 1))
    topk(D, 8, (0, 8), remove_self_column=False)                                                     # k + skip = n is the limit
    topk(D, 7, (0, 8), lab)
    assert calls == ['vited_retrieval_topk'] * 2
    del calls[:]
    with pytest.raises(ValueError, match='retrieval_topk_rows: labels'):
        topk(D, 3, (0, 8), lab.float())                                                              # float labels
    with pytest.raises(ValueError, match='retrieval_topk_rows: labels .*length 8'):
        topk(D, 3, (0, 8), lab[:7])
    with pytest.raises(ValueError, match='rows'):
        topk(D, 3, (4, 9))
    with pytest.raises(ValueError, match='rows'):
        topk(D, 3, (5, 5))
    with pytest.raises(ValueError, match='square'):
        topk(D[:4], 3, (0, 4))
    with pytest.raises(TypeError, match='float32, bfloat16 or float16'):
        topk(D.double(), 3, (0, 8))
    with pytest.raises(ValueError, match='retrieval_topk_rows: matrix'):
        topk(D.t(), 3, (0, 8))                                                                       # rows must be dense
    with pytest.raises(ValueError, match='retrieval_curve_rows: labels'):
        curves(D, lab.float(), *csr, (0, 8))
    with pytest.raises(ValueError, match='retrieval_curve_rows: members'):
        curves(D, lab, csr[0], csr[1][:7], (0, 8))
    with pytest.raises(ValueError, match='retrieval_curve_rows: estimate'):
        curves(D, lab, *csr, (0, 8), estimate=torch.zeros(7, dtype=torch.int32))
    with pytest.raises(ValueError, match='retrieval_curve_rows: estimate'):
        curves(D, lab, *csr, (0, 8), estimate=torch.zeros(8, dtype=torch.int64))
    with pytest.raises(ValueError, match='retrieval_curve_rows: tp_at'):
        curves(D, lab, *csr, (0, 8), tp_at=torch.zeros(8, dtype=torch.int64))                        # n - skip = 7 positions
    with pytest.raises(ValueError, match='retrieval_curve_rows: tp_at'):
        curves(D, lab, *csr, (0, 8), tp_at=torch.zeros(7, dtype=torch.int32))
    assert not calls
    tp_at, rec = curves(D, lab, *csr, (2, 8), estimate=lab)
    assert calls == ['vited_retrieval_curves'] and tp_at.dtype == torch.int64 and tp_at.tolist() == [0] * 7 and rec.shape == (6, 2)
    del calls[:]
    # engine: labels and estimates are checked before anything is built
    with pytest.raises(TypeError, match='integer'):
        engine.retrieval_topk(D, 3, labels=lab.float())
    with pytest.raises(ValueError, match='length 8'):
        engine.retrieval_curves(D, lab[:7])
    with pytest.raises(ValueError, match='relevant_estimate'):
        engine.retrieval_curves(D, lab, relevant_estimate=torch.zeros(8))
    with pytest.raises(ValueError, match='rows'):
        engine.retrieval_topk(D, 3, rows=(3, 9))
    assert not calls


def test_abi_rejects_bad_arguments(vited):
    """Both entries validate before launching, so bad arguments are safe to pass without a GPU."""
    lib = vited._lib.load()
    buf = ctypes.create_string_buffer(1024)
    p = ctypes.addressof(buf)
    topk = lambda **kw: lib.vited_retrieval_topk(*{**dict(D=p, dtype=2, ld=8, n=8, r0=0, r1=8, labels=p, k=3, remove=1, sim=0, idx=p,
                                                          val=p, hit=p, stream=None), **kw}.values())
    assert topk(D=None) == 1 and topk(idx=None) == 1 and topk(val=None) == 1 and topk(labels=None) == 1
    assert topk(ld=7) == 1 and topk(n=0) == 1 and topk(r0=-1) == 1 and topk(r1=9) == 1 and topk(r0=4, r1=4) == 1
    assert topk(remove=2) == 1 and topk(sim=3) == 1 and topk(D=p + 1) == 1
    assert topk(k=0) == 1 and topk(k=8) == 1 and topk(k=9, remove=0) == 1                         # k + skip <= n
    assert topk(dtype=7) == 2 and topk(k=1025, n=4096, ld=4096) == 2                              # k <= 1024
    curves = lambda **kw: lib.vited_retrieval_curves(*{**dict(D=p, dtype=2, ld=8, n=8, r0=0, r1=8, labels=p, offsets=p, members=p, C=1,
                                                              remove=1, sim=0, estimate=None, tp_at=p, rows_out=p, stream=None),
                                                       **kw}.values())
    assert curves(D=None) == 1 and curves(tp_at=None) == 1 and curves(rows_out=None) == 1 and curves(members=None) == 1
    assert curves(ld=7) == 1 and curves(C=0) == 1 and curves(r1=9) == 1 and curves(remove=2) == 1 and curves(n=1, ld=1, r1=1) == 1
    assert curves(tp_at=p + 4) == 1 and curves(dtype=7) == 2
    assert lib.vited_abi_version() == 1


def _clangxx():
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    for cand in (shutil.which('clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++')):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.mark.parametrize('flags', [(), ('-fsanitize=address,undefined', '-fno-sanitize-recover=all')], ids=['plain', 'sanitized'])
def test_host_check_of_the_selection(tmp_path, flags):
    """tools/ranklists_host_check.cpp: the text of csrc/rank_key.h walked in the kernel's schedule over exactly-sized heap blocks,
    against std::stable_sort - a stand-alone program with its own main."""
    cxx = _clangxx()
    assert cxx is not None, 'no clang++ beside hipcc: the HIP toolchain that builds the library ships one'
    exe = str(tmp_path / 'ranklists_host_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', *flags, '-I', os.path.join(ROOT, 'vit-ed_amd', 'csrc'),
                    os.path.join(ROOT, 'tools', 'ranklists_host_check.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert 'ranklists_host_check ok' in run.stdout and not run.stderr.strip(), run.stdout[-3000:] + run.stderr[-3000:]


# ---- 2 processes over gloo: the combine of hisfrag_retrieval_lists and retrieval_curves, the shares from the numpy restatement
def _stub_topk(matrix, k, rows, labels=None, *, remove_self_column=True, from_similarity=False):
    idx, val, hit = rc.reference_topk(matrix, k, None if labels is None else labels.numpy(), rows, remove_self_column, from_similarity)
    return torch.from_numpy(idx), torch.from_numpy(val), None if hit is None else torch.from_numpy(hit)


def _stub_curves(matrix, labels, offsets, members, rows, *, remove_self_column=True, from_similarity=False, estimate=None, tp_at=None):
    tp, rec = rc.reference_curves(matrix, labels.numpy(), rows, remove_self_column, from_similarity,
                                  None if estimate is None else estimate.numpy())
    return torch.from_numpy(tp), torch.from_numpy(rec)


def _gloo_case():
    rng = np.random.default_rng(11)
    n = 90
    labels = rng.integers(0, 8, n)
    labels[70] = 99                                       # a singleton, in the second rank's share of the rows
    S = torch.from_numpy((rng.integers(0, 40, (n, n)) / 32).astype(np.float32)).to(torch.float16)      # ties in every row
    S[5, 7] = float('nan')
    estimate = rng.integers(0, 15, n)
    return S, labels, estimate


def _results(engine, rank, world, group):
    S, labels, estimate = _gloo_case()
    lists = engine.hisfrag_retrieval_lists(S, 9, torch.from_numpy(labels), rank=rank, world=world, group=group)
    plain = engine.hisfrag_retrieval_lists(S, 4, rank=rank, world=world, group=group)
    bounds = engine.shard_rows_by_pair_count(S.shape[0], world)
    curves = engine.retrieval_curves(S, labels, rows=(bounds[rank], bounds[rank + 1]), from_similarity=True, relevant_estimate=estimate,
                                     group=group)
    bare = engine.retrieval_curves(S, labels, rows=(bounds[rank], bounds[rank + 1]), from_similarity=True, remove_self_column=False, group=group)
    return {'idx': lists.indices, 'val': lists.values.view(torch.int32), 'hit': lists.correct, 'plain_idx': plain.indices,
            'plain_correct': plain.correct, 'tp_at': curves.tp_at, 'counts': list(curves[1:]), 'bare_tp_at': bare.tp_at,
            'bare_counts': list(bare[1:])}


def _worker(rank, world, port, out):
    torch.cuda.is_available = lambda: False          # the gloo plumbing, as on a CPU-only machine
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import vited_amd  # noqa: F401
    from vited_amd import engine, ops
    ops.retrieval_topk_rows, ops.retrieval_curve_rows = _stub_topk, _stub_curves
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    engine.configure_ddp()
    assert dist.get_backend() == 'gloo'
    res = _results(engine, rank, world, dist.group.WORLD)
    gathered = [None] * world
    dist.all_gather_object(gathered, res)
    if rank == 0:
        torch.save(gathered, out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_lists_and_curves_equal_one_process(vited, tmp_path, monkeypatch):
    from vited_amd import engine, ops
    out = str(tmp_path / 'r.pt')
    port = 29700 + (os.getpid() % 90)
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    per_rank = torch.load(out, weights_only=False)
    monkeypatch.setattr(ops, 'retrieval_topk_rows', _stub_topk)
    monkeypatch.setattr(ops, 'retrieval_curve_rows', _stub_curves)
    one = _results(engine, 0, 1, None)
    S, labels, estimate = _gloo_case()
    idx, val, hit = rc.reference_topk(S, 9, labels, from_similarity=True)
    assert np.array_equal(one['idx'].numpy(), idx) and np.array_equal(one['hit'].numpy(), hit) and rc.same_values(one['val'].view(torch.float32).numpy(), val)
    assert one['counts'][0] == 90 and one['counts'][3] == int(estimate.sum()) and one['bare_counts'][2:] == [None, None]
    assert one['plain_correct'] is None and one['idx'].dtype == torch.int32 and one['hit'].dtype == torch.uint8
    for r, res in enumerate(per_rank):
        for key, want in one.items():
            got = res[key]
            assert torch.equal(got, want) if torch.is_tensor(want) else got == want, (r, key)
