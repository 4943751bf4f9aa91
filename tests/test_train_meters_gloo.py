"""CPU, 2 processes over gloo: engine.TrainMeters.all_reduce is AverageMeter.all_reduce of the loss meter (misc/utils.py:293-303) -
each rank's fp64 (sum, count) rounded to fp32, summed over the ranks in fp32, divided on the host."""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = [8, 8, 5, 8, 3, 8, 7, 1, 8, 2]


def _sequence():
    g = torch.Generator().manual_seed(11)
    return list(torch.rand(len(ROWS), generator=g) + 0.25)


def _worker(rank, world, port, out):
    torch.cuda.is_available = lambda: False          # the gloo plumbing, as on a CPU-only machine
    sys.path.insert(0, os.path.dirname(HERE))
    import vited_amd  # noqa: F401
    from vited_amd import engine
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    engine.configure_ddp()
    assert dist.get_backend() == 'gloo'
    meters = engine.TrainMeters('cpu')
    for loss, n in list(zip(_sequence(), ROWS))[rank::world]:
        meters.update_loss(loss, n)
    res = (meters.all_reduce(group=dist.group.WORLD), meters.values()['loss'])
    gathered = [None] * world
    dist.all_gather_object(gathered, res)
    if rank == 0:
        torch.save(gathered, out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_all_reduce_equals_the_reference_arithmetic(tmp_path):
    out = str(tmp_path / 'r.pt')
    port = 29700 + (os.getpid() % 90)
    world = 2
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    per_rank = torch.load(out, weights_only=False)
    seq = list(zip(_sequence(), ROWS))
    totals, local = [], []
    for r in range(world):
        s = c = 0
        for loss, n in seq[r::world]:
            s += loss.item() * n
            c += n
        totals.append(torch.tensor([s, c], dtype=torch.float32))
        local.append((seq[r::world][-1][0].item(), s / c))
    total = (totals[0] + totals[1]).tolist()                # the fp32 SUM all-reduce
    want = total[0] / total[1]
    assert total[1] == sum(ROWS)                            # the concatenated sequence's count
    for r, (avg, loss) in enumerate(per_rank):
        assert avg == want, (r, avg, want)
        assert tuple(loss) == local[r]                      # the rank's own meter is untouched by the reduction
