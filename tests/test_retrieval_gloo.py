"""CPU, 2 processes over gloo: the cross-rank reduction of engine.retrieval_metrics / hisfrag_retrieval_metrics.  The per-row
kernel (ops.retrieval_metrics_rows) is stubbed with the numpy restatement of test_retrieval_metrics.py, so what is tested is the
sharding and the arithmetic of the one SUM all-reduce: two shards give the single-shard metrics, and a row without a correct
retrieval on ONE rank makes Pr@k NaN on every rank."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))


def _stub_rows(matrix, labels, offsets, members, rows, *, remove_self_column=True, from_similarity=False):
    """What vited_retrieval_metrics returns, from the numpy restatement (float64 row records + the 7 sums)."""
    from test_retrieval_metrics import reference_rows
    D = (1 - matrix) if from_similarity else matrix
    rec = reference_rows(D.float().numpy(), labels.numpy(), remove_self_column, rows=np.arange(rows[0], rows[1]))
    ap, correct, top1, h10, h100 = rec.T
    valid = correct > 0
    with np.errstate(invalid='ignore', divide='ignore'):
        sums = [(ap[valid] / correct[valid]).sum(), valid.sum(), top1.sum(), (h10 / np.minimum(correct, 10)).sum(),
                (h100 / np.minimum(correct, 100)).sum(), (~valid).sum(), len(rec)]
    return torch.from_numpy(rec), torch.tensor(sums, dtype=torch.float64)


def _cases():
    rng = np.random.default_rng(7)
    n = 120
    labels = rng.integers(0, 9, n)
    S = rng.random((n, n)).astype(np.float32)
    np.fill_diagonal(S, 1.5)               # an image is most similar to itself: the dropped first retrieval is the diagonal
    S = torch.from_numpy(S).to(torch.float16)
    lone = labels.copy()
    lone[100] = 99                         # one singleton row, in the second rank's share of the rows
    return {'all_have_matches': (S, labels), 'singleton_on_rank1': (S, lone)}


def _worker(rank, world, port, out):
    torch.cuda.is_available = lambda: False          # the gloo plumbing, as on a CPU-only machine
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import vited_amd
    from vited_amd import engine, ops
    ops.retrieval_metrics_rows = _stub_rows
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    engine.configure_ddp()
    assert dist.get_backend() == 'gloo'
    res = {}
    for name, (S, labels) in _cases().items():
        res[name] = engine.hisfrag_retrieval_metrics(S, torch.from_numpy(labels), rank=rank, world=world)
        bounds = engine.shard_rows_by_pair_count(S.shape[0], world)
        res[name + '/explicit'] = engine.retrieval_metrics(1 - S, labels, rows=(bounds[rank], bounds[rank + 1]), group=dist.group.WORLD)
        res[name + '/local'] = engine.retrieval_metrics(1 - S, labels, rows=(bounds[rank], bounds[rank + 1]))
    gathered = [None] * world
    dist.all_gather_object(gathered, res)
    if rank == 0:
        torch.save(gathered, out)
    dist.barrier()
    dist.destroy_process_group()


def _same(a, b):
    return all((np.isnan(x) and np.isnan(y)) or abs(x - y) <= 1e-12 for x, y in zip(a, b))


def test_two_rank_retrieval_metrics_equal_one_shard(tmp_path):
    sys.path.insert(0, HERE)
    from vited_amd import engine, ops
    from test_retrieval_metrics import reference_metrics
    out = str(tmp_path / 'r.pt')
    port = 29900 + (os.getpid() % 90)
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    per_rank = torch.load(out, weights_only=False)
    real = ops.retrieval_metrics_rows
    ops.retrieval_metrics_rows = _stub_rows
    try:
        for name, (S, labels) in _cases().items():
            one_shard = engine.hisfrag_retrieval_metrics(S, torch.from_numpy(labels))                  # world 1: all rows
            want = reference_metrics((1 - S).numpy(), labels)
            assert _same(one_shard, want), (name, one_shard, want)
            for r, res in enumerate(per_rank):
                assert _same(res[name], one_shard), (name, r, res[name], one_shard)
                assert _same(res[name + '/explicit'], one_shard), (name, r)
            # without a group each rank sees its own rows only: rank 0 has no singleton, rank 1 has it
            if name == 'singleton_on_rank1':
                assert np.isnan(one_shard[2]) and np.isnan(one_shard[3]) and not np.isnan(one_shard[0])
                assert not np.isnan(per_rank[0][name + '/local'][2]) and np.isnan(per_rank[1][name + '/local'][2])
    finally:
        ops.retrieval_metrics_rows = real
