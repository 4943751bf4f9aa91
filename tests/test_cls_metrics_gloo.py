"""CPU, 2 processes over gloo: engine.ClassificationMeters.all_reduce across ranks.  The launch (ops.cls_metrics_update) is stubbed
with the numpy restatement of test_cls_metrics.py, so what is tested is the cross-rank arithmetic: two ranks' shards of the
validation batches give the averages of the reference's per-rank AverageMeters followed by its fp32 SUM all-reduces, with ONE
all-reduce call instead of six, and a bad target on one rank makes every rank raise."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ('config_a', 'seven_columns', 'edge_columns')


def _shard(batches, rank, world):
    return batches[rank::world]


def _worker(rank, world, port, out):
    torch.cuda.is_available = lambda: False          # the gloo plumbing, as on a CPU-only machine
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import vited_amd  # noqa: F401
    from vited_amd import engine, ops
    from test_cls_metrics import _case, golden, stub_update
    ops.cls_metrics_update = stub_update
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    engine.configure_ddp()
    assert dist.get_backend() == 'gloo'
    calls = []
    real = dist.all_reduce

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)

    res = {}
    g, _ = golden()
    dist.all_reduce = counting
    try:
        for name in CASES:
            batches = _shard(_case(g, name), rank, world)
            meters = engine.ClassificationMeters(batches[0][0].shape[1], 'cpu')
            for x, y in batches:
                meters.update(torch.from_numpy(x), torch.from_numpy(y))
            before = len(calls)
            res[name] = (tuple(meters.all_reduce(group=dist.group.WORLD)), len(calls) - before)
        meters = engine.ClassificationMeters(4, 'cpu')
        y = torch.zeros(4, 4)
        if rank == 1:
            y[0, 0] = 2.0
        meters.update(torch.randn(4, 4), y)
        try:
            meters.all_reduce()
            res['bad'] = None
        except ValueError as e:
            res['bad'] = str(e)
    finally:
        dist.all_reduce = real
    gathered = [None] * world
    dist.all_gather_object(gathered, res)
    if rank == 0:
        torch.save(gathered, out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_meters_equal_the_reference_all_reduce(tmp_path):
    sys.path.insert(0, HERE)
    from test_cls_metrics import _bits, _case, batch_values, golden, meters_update, reduced_averages
    out = str(tmp_path / 'r.pt')
    port = 29900 + (os.getpid() % 90)
    world = 2
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    per_rank = torch.load(out, weights_only=False)
    g, _ = golden()
    for name in CASES:
        # the reference: each rank's meters over its own batches, then the fp32 SUM of every (sum, count)
        rank_meters = []
        for r in range(world):
            m = np.zeros(10)
            for x, y in _shard(_case(g, name), r, world):
                meters_update(m, batch_values(x, y), x.shape[0])
            rank_meters.append(m)
        want, samples = reduced_averages(rank_meters)
        assert samples == sum(int(b) for b in g[name + '__batches'])
        for r, res in enumerate(per_rank):
            got, n_calls = res[name]
            assert n_calls == 1, (name, r, n_calls)
            np.testing.assert_array_equal(_bits(got[:5]), _bits(want), err_msg=f'{name} rank {r}')
            assert got[5] == samples
    for r, res in enumerate(per_rank):
        assert res['bad'] is not None and 'targets must be 0 or 1' in res['bad'], (r, res['bad'])
