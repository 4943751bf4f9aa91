"""The learning-rate range test on the GPU (vited_lr_finder_step, engine.find_lr): the kernel alone against the numpy
rule of tests/lr_finder_cases.py, and ``engine.find_lr`` through ``TrainStep`` / ``TwoStageTrainStep`` - against a host-driven
restatement, eager against replayed, stopped by a divergence, restored, and on two ranks.

Every model is config T's (configs/test/test_pjs_hisfrag20_patch32_64.yaml: 64 px, patch 32, width 32, 1 + 1 blocks) without dropout.

Tolerance: IEEE fp64 + - * and the comparisons round identically on both sides, so the losses, the smoothed losses, the state words and
the halt row are compared bit for bit.  Only the rate goes through pow, where the device's fp64 routine is a few ulp off libm's: the fp64
rate of the history within 4 fp64 ulp, the fp32 rate words numpy's value rounded to fp32 or its neighbour (a few fp64 ulp can only
move a value across a rounding boundary) - the allowance tests/test_gpu_lr_scheduler.py makes for the same routine.  Runs of the same
kernels against each other (a twin, graph against eager, two ranks) are compared bit for bit."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import lr_finder_cases as fc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_T = os.path.join(ROOT, 'configs', 'test', 'test_pjs_hisfrag20_patch32_64.yaml')
N, LABELS = 6, [0, 0, 1, 1, 2, 2]            # the two-stage step's images and their classes
SCALE = 0.5                                  # lr_scale of the second parameter group


def _model(V, dev, state=None):
    m = V.build_model(V.config_from_yaml(CFG_T))          # every dropout and drop-path rate 0
    if state is not None:
        m.load_state_dict(state)
    return m.to(dev).train()


@pytest.fixture(scope='module')
def init(vited, gpu):
    torch.manual_seed(23)
    return {k: v.clone() for k, v in _model(vited, gpu).state_dict().items()}


def _setup(V, dev, init, kind='adamw', two_stage=False, lr=1e-3, **kw):
    m = _model(V, dev, init)
    groups = V.engine.param_groups_no_decay_1d(m)
    groups[1]['lr_scale'] = SCALE
    opt = (V.optim.FlatAdamW(groups, lr=lr, weight_decay=0.05, model=m) if kind == 'adamw' else
           V.optim.FlatSGD(groups, lr=lr, momentum=0.9, nesterov=True, weight_decay=0.05, model=m))
    if two_stage:
        step = V.engine.TwoStageTrainStep(m, opt, capacity=V.engine.mined_pair_capacity(N) + 1, clip_grad=5.0, **kw)
        step.mine_keys = torch.linspace(0, 1, N * N, device=dev)          # every run mines the same pairs
    else:
        step = V.engine.TrainStep(m, opt, clip_grad=5.0, **kw)
    return m, opt, step


def _batches(n, dev, two_stage=False, seed=31, rank=0, world=1):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        if two_stage:
            out.append((torch.randn(N, 3, 64, 64, generator=g).clamp(-1, 1).to(dev), torch.tensor(LABELS, device=dev)))
        else:
            x, y = torch.randn(8, 2, 3, 64, 64, generator=g).clamp(-1, 1), (torch.rand(8, 1, generator=g) > 0.5).float()
            out.append((x[rank::world].to(dev), y[rank::world].to(dev)))
    return out


class _Loader:
    """Yields the batches and notes, before each, the rate words the coming iteration runs at (a host read: the test's, not find_lr's)."""

    def __init__(self, batches, opt):
        self.batches, self.opt, self.words = batches, opt, []

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for b in self.batches:
            self.words.append(self.opt._hyper[fc.HEADER::fc.WORDS].tolist())
            yield b


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32 if t.element_size() == 4 else torch.int16)


def _same_params(a, b):
    return all(torch.equal(_bits(p.detach()), _bits(q.detach())) for p, q in zip(a.parameters(), b.parameters()))


# ---- G1: the kernel alone ---------------------------------------------------------------------------------------------------------
def test_kernel_follows_the_numpy_rule_and_touches_nothing_else(vited, gpu):
    ops, f64 = vited.ops, torch.float64
    halted = 0
    for case in fc.CASES + fc.random_cases():
        groups = len(case['start'])
        hyper = torch.arange(fc.HEADER + fc.WORDS * groups, dtype=torch.float32, device=gpu) - 100.0
        before = hyper.view(torch.int32).clone()
        rate = torch.zeros_like(hyper, dtype=torch.bool)
        rate[fc.HEADER::fc.WORDS] = True
        state = torch.zeros(4, dtype=torch.int64, device=gpu)
        history = torch.full((case['num_iter'], 3), -1.0, dtype=f64, device=gpu)
        start, end = torch.tensor(case['start'], dtype=f64, device=gpu), torch.tensor(case['end'], dtype=f64, device=gpu)
        args = (state, history, start, end, case['num_iter'], case['smooth_f'], case['diverge_th'], hyper, fc.HEADER, fc.WORDS)
        losses = torch.tensor(case['losses'] + [case['losses'][-1]] * case['extra'], dtype=torch.float32, device=gpu)
        want = fc.run(case)
        for n in range(losses.numel()):
            ops.lr_finder_step(losses[n], *args)                          # one launch per row, the loss a device scalar
            for g, (got, w) in enumerate(zip(hyper[fc.HEADER::fc.WORDS].tolist(), want['words'][n])):
                assert (got == 0.0 and fc.bits32(got) == 0) if w == 0.0 else fc.fp32_matches(got, w), (case['id'], n, g, got, float(w))
            assert torch.equal(hyper.view(torch.int32)[~rate], before[~rate]), (case['id'], n)       # every other word keeps its bits
        got_state, got_hist = state.cpu(), history.cpu()
        assert got_state[:2].tolist() == [want['rows'], want['state']], case['id']                # the halt row and the state
        assert [fc.bits64(v) for v in got_state[2:].view(f64).tolist()] == [fc.bits64(want['smoothed']), fc.bits64(want['best'])], case['id']
        rows = want['rows']
        assert torch.equal(_bits(got_hist[:rows, 1:]), _bits(torch.from_numpy(want['history'][:, 1:].copy()))), case['id']
        assert all(fc.ulps64(a, b) <= 4 for a, b in zip(got_hist[:rows, 0].tolist(), want['history'][:, 0])), case['id']
        assert got_hist[0, 0].item() == case['start'][0]                   # the first iteration runs at exactly start
        assert bool((got_hist[rows:] == -1.0).all()), case['id']           # rows behind the halting row do not exist
        if want['state'] != fc.RUNNING:
            halted += 1
            hyper[fc.HEADER::fc.WORDS] = 3.0
            for _ in range(5):                                            # a halted test writes 0.0 and nothing else, launch after launch
                ops.lr_finder_step(torch.tensor(0.25, device=gpu), *args)
            assert hyper.view(torch.int32)[rate].tolist() == [0] * groups, case['id']
            assert torch.equal(hyper.view(torch.int32)[~rate], before[~rate]), case['id']
            assert torch.equal(state.cpu(), got_state) and torch.equal(_bits(history.cpu()), _bits(got_hist)), case['id']
    assert halted > 40
    with pytest.raises(ValueError, match='lr_finder_step: dst'):
        ops.lr_finder_step(losses[0], state, history, start, end, case['num_iter'], 0.05, 5.0, hyper[:fc.HEADER], fc.HEADER, fc.WORDS)
    with pytest.raises(ValueError, match='lr_finder_step: num_iter'):
        ops.lr_finder_step(losses[0], state, history, start, end, case['num_iter'] + 1, 0.05, 5.0, hyper, fc.HEADER, fc.WORDS)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.lr_finder_step(losses[0].cpu(), *args)


# ---- G2: find_lr against a host-driven restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize('two_stage', [False, True], ids=['TrainStep', 'TwoStageTrainStep'])
@pytest.mark.parametrize('kind', ['adamw', 'sgd'])
def test_find_lr_is_the_host_driven_loop_bit_for_bit(vited, gpu, init, kind, two_stage):
    """The twin does what a port of ignite's loop would: sets the rate on the host before every iteration - to the very fp32 values
    the device sweep ran at - reads the loss with ``.item()`` and keeps the statistics in numpy."""
    E, num_iter = vited.engine, 12
    sweep = dict(start_lr=1e-5, end_lr=1.0 if kind == 'adamw' else 10.0, smooth_f=0.3, diverge_th=3.0)
    batches = _batches(num_iter, gpu, two_stage)
    m, opt, step = _setup(vited, gpu, init, kind, two_stage, amp=True)
    loader = _Loader(batches, opt)
    res = E.find_lr(step, loader, restore=False, poll_every=4, **sweep)
    rows = res.iterations
    assert rows >= 2 and res.state != fc.RUNNING and res.lrs.shape == res.losses.shape == res.smoothed.shape == (rows,)
    assert step.num_updates == len(loader.words) >= rows and (res.state == fc.DONE) == (rows == num_iter)
    assert len(loader.words) <= min(num_iter, -(-rows // 4) * 4)                          # the loop ended at the first poll behind the halt
    for i in range(rows):
        assert loader.words[i][0] == float(np.float32(res.lrs[i].item())), i             # the word is the history's rate in fp32
        want = fc.rate(sweep['start_lr'] * SCALE, sweep['end_lr'] * SCALE, i, num_iter)
        assert loader.words[i][1] == float(np.float32(want)) if i == 0 else fc.fp32_matches(loader.words[i][1], want), i
        assert fc.ulps64(res.lrs[i].item(), fc.rate(sweep['start_lr'], sweep['end_lr'], i, num_iter)) <= 4, i
    assert all(w == [0.0, 0.0] for w in loader.words[rows:])                             # behind a halt the rates are 0
    assert res.suggestion == vited.ops.lr_suggestion(res.lrs, res.smoothed)
    # the twin
    m2, opt2, step2 = _setup(vited, gpu, init, kind, two_stage, amp=True)
    f, th = np.float64(sweep['smooth_f']), np.float64(sweep['diverge_th'])
    raw, smoothed, halt = [], [], fc.RUNNING
    for i, (x, y) in enumerate(batches):
        assert i < rows, 'the host-driven loop went on where the device sweep halted'
        for g, lr in zip(opt2.param_groups, loader.words[i]):
            g['lr'] = lr
        loss = np.float64(step2.step(x, y).item())
        s = loss if i == 0 else f * loss + (np.float64(1) - f) * smoothed[-1]
        best = s if i == 0 or s < best else best
        raw.append(loss)
        smoothed.append(s)
        halt = fc.NONFINITE if not np.isfinite(loss) else fc.DIVERGED if s > th * best else fc.DONE if i + 1 == num_iter else fc.RUNNING
        if halt != fc.RUNNING:
            break
    assert (len(raw), halt) == (rows, res.state)                                         # the halt row
    assert [fc.bits64(v) for v in raw] == [fc.bits64(v) for v in res.losses.tolist()]
    assert [fc.bits64(v) for v in smoothed] == [fc.bits64(v) for v in res.smoothed.tolist()]
    if res.state != fc.NONFINITE:                   # the iterations behind the halt ran at 0 and left the parameters where they were
        assert _same_params(m, m2)
    assert opt2.hyper_uploads >= rows - 1 and opt.hyper_uploads == 1                      # the sweep itself uploaded its start, once


# ---- G3: eager against replayed ---------------------------------------------------------------------------------------------------
def test_replayed_sweep_records_what_eager_launches_record(vited, gpu, init):
    E, num_iter = vited.engine, 24
    batches = _batches(num_iter, gpu)
    results, steps = [], []
    for use_graph in (False, True):
        m, opt, step = _setup(vited, gpu, init, 'adamw', amp=True, use_graph=use_graph)
        test = E.LRRangeTest(opt, num_iter, start_lr=1e-6, end_lr=1e-2, diverge_th=1e9)      # nothing stops it: all 24 rows
        for x, y in batches:                          # two eager warm-up steps, the capture, 21 replays
            test.record(step.step(x, y))
        results.append(test.history())
        steps.append((m, step, test))
    eager, graph = results
    assert eager.shape == (num_iter, 3) and steps[1][2].state() == fc.DONE and steps[0][2].rows == num_iter
    assert torch.equal(_bits(eager), _bits(graph))
    assert steps[1][1]._g1 is not None and steps[1][1]._g_opt is not None and steps[1][1].recaptures == 0 and steps[0][1]._g1 is None
    assert _same_params(steps[0][0], steps[1][0])
    assert not torch.equal(eager[:, 1], eager[:1, 1].expand(num_iter))       # the rates took effect: the loss moved
    assert [g['lr'] for g in steps[1][1].optimizer.param_groups] == [0.0, 0.0]       # state() brought param_groups up to the words


# ---- G4: divergence ---------------------------------------------------------------------------------------------------------------
def test_divergence_stops_the_parameters_at_the_halting_update(vited, gpu, init):
    E, num_iter = vited.engine, 48
    batches = _batches(num_iter, gpu)
    m, opt, step = _setup(vited, gpu, init, 'adamw', amp=True)
    loader = _Loader(batches, opt)
    # from 1e-2 the rate passes 1 two thirds of the way: room for the loss to take off and for iterations behind the halt
    res = E.find_lr(step, loader, start_lr=1e-2, end_lr=10.0, restore=False, poll_every=0)
    print(f'divergence: halted in state {res.state} after {res.iterations} of {num_iter} rows at lr {res.lrs[-1].item():.3e}, '
          f'smoothed {res.smoothed[-1].item():.4f} against best {res.smoothed.min().item():.4f}')
    assert res.state == fc.DIVERGED and 2 <= res.iterations < num_iter, 'the sweep to a rate of 10 never crossed diverge_th'
    h = res.iterations - 1
    assert res.smoothed[h] > 5.0 * res.smoothed[:h + 1].min() and bool((res.smoothed[:h] <= 5.0 * torch.cummin(res.smoothed[:h], 0)[0]).all())
    assert len(loader.words) == num_iter == step.num_updates                  # never polled: every batch was stepped
    assert all(w == [0.0, 0.0] for w in loader.words[h + 1:]) and all(w[0] > 0 for w in loader.words[:h + 1])
    assert res.lrs.shape == res.losses.shape == res.smoothed.shape == (h + 1,)          # the history ends at the halting row
    assert opt._hyper[fc.HEADER::fc.WORDS].tolist() == [0.0, 0.0]
    # a twin stopped right behind the halting update
    m2, opt2, step2 = _setup(vited, gpu, init, 'adamw', amp=True)
    for i in range(h + 1):
        for g, lr in zip(opt2.param_groups, loader.words[i]):
            g['lr'] = lr
        step2.step(*batches[i])
    assert _same_params(m, m2)
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


# ---- G5: restore ------------------------------------------------------------------------------------------------------------------
def _shadow_bits(V, m):
    index = {id(p): i for i, p in enumerate(m.parameters())}
    out = {}
    for c, cache in enumerate(V.functions.shadows_of(m)):
        for pid, tags in cache.buffers().items():
            for tag, buf in tags.items():
                out[(c, index[pid], tag)] = _bits(buf).clone()
    return out


def _same_everything(V, a, b):
    (m1, opt1, s1), (m2, opt2, s2) = a, b
    assert _same_params(m1, m2)
    sd1, sd2 = opt1.state_dict(), opt2.state_dict()
    assert sd1['param_groups'] == sd2['param_groups'] and sd1['state'].keys() == sd2['state'].keys()
    for k in sd1['state']:
        assert sd1['state'][k].keys() == sd2['state'][k].keys()
        assert all(torch.equal(_bits(sd1['state'][k][n]), _bits(sd2['state'][k][n])) for n in sd1['state'][k]), k
    assert torch.equal(_bits(opt1._hyper), _bits(opt2._hyper))                 # the rate words, the step and the skip counters
    sh1, sh2 = _shadow_bits(V, m1), _shadow_bits(V, m2)
    assert sh1.keys() == sh2.keys() and len(sh1) > 0 and all(torch.equal(sh1[k], sh2[k]) for k in sh1)
    assert s1.num_updates == s2.num_updates and opt1.num_updates == opt2.num_updates
    assert torch.equal(_bits(s1.meters.state), _bits(s2.meters.state))


@pytest.mark.parametrize('kind', ['adamw', 'sgd'])
def test_restore_puts_back_every_bit_in_place(vited, gpu, init, kind):
    E = vited.engine
    train, sweep = _batches(6, gpu, seed=41), _batches(8, gpu, seed=43)
    swept, twin, kept = [_setup(vited, gpu, init, kind, amp=True, use_graph=True, meters=True) for _ in range(3)]
    for x, y in train[:3]:                           # two eager steps, the capture, one replay
        for _, _, step in (swept, twin, kept):
            step.step(x, y)
    assert swept[2]._g1 is not None
    signature, hyper_ptr = swept[1].shadow_signature(), swept[1]._hyper.data_ptr()
    res = E.find_lr(swept[2], sweep, start_lr=1e-4, end_lr=1e-1, restore=True, poll_every=0)
    assert res.iterations >= 2 and float(res.losses[0]) != float(res.losses[-1])
    assert swept[1].shadow_signature() == signature and swept[1]._hyper.data_ptr() == hyper_ptr      # in place: nothing was re-bound
    _same_everything(vited, swept, twin)
    for x, y in train[3:]:
        la, lb = swept[2].step(x, y), twin[2].step(x, y)
        assert torch.equal(la, lb)
    _same_everything(vited, swept, twin)
    assert swept[2].recaptures == twin[2].recaptures == 0 and swept[2]._g1 is not None
    # without the restore the swept state stays
    E.find_lr(kept[2], sweep, start_lr=1e-4, end_lr=1e-1, restore=False, poll_every=0)
    assert not _same_params(kept[0], twin[0]) and kept[2].num_updates == 3 + 8


# ---- G6: two ranks ----------------------------------------------------------------------------------------------------------------
def _rank(rank, world, port, out):
    import sys
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import vited_amd as V
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0')
    dist.init_process_group('gloo', init_method='env://', world_size=world, rank=rank)
    dev = torch.device('cuda:0')
    torch.manual_seed(200 + rank)
    m = _model(V, dev)
    V.engine.broadcast_parameters(m)
    groups = V.engine.param_groups_no_decay_1d(m)
    groups[1]['lr_scale'] = SCALE
    opt = V.optim.FlatAdamW(groups, lr=1e-3, weight_decay=0.05, model=m)
    step = V.engine.TrainStep(m, opt, clip_grad=5.0, amp=True)
    local, inner = [], step.step

    def noting(x, y):
        loss = inner(x, y)
        local.append(loss.detach().clone())
        return loss

    step.step = noting
    loader = _Loader(_batches(6, dev, rank=rank, world=world), opt)
    res = V.engine.find_lr(step, loader, start_lr=1e-5, end_lr=1e-2, restore=False, poll_every=2)
    mine = torch.cat([torch.stack([res.lrs, res.losses, res.smoothed], 1).reshape(-1), torch.tensor(loader.words, dtype=torch.float64).reshape(-1),
                      torch.stack(local).double().cpu(), torch.tensor([float(res.state), float(res.iterations)], dtype=torch.float64)])
    gathered = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(gathered, mine)
    if rank == 0:
        torch.save({'ranks': gathered, 'rows': res.iterations, 'steps': len(loader.words)}, out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_take_the_same_decisions(vited, gpu, tmp_path):
    out = str(tmp_path / 'ranks.pt')
    mp.spawn(_rank, args=(2, 29400 + os.getpid() % 90, out), nprocs=2, join=True)
    got = torch.load(out, weights_only=True)
    a, b = got['ranks']
    rows, steps = got['rows'], got['steps']
    assert rows == steps == 6 and a[-2:].tolist() == b[-2:].tolist() == [float(fc.DONE), 6.0]
    shared = 3 * rows + 2 * steps
    assert torch.equal(_bits(a[:shared]), _bits(b[:shared]))                   # identical history, identical rate words
    local_a, local_b = a[shared:shared + steps], b[shared:shared + steps]
    assert not torch.equal(local_a, local_b)                                   # on different halves of every batch
    mean = ((local_a.float() + local_b.float()) / 2).double()                  # the fp32 sum, halved: what the record read
    assert torch.equal(_bits(a[:3 * rows].reshape(rows, 3)[:, 1].contiguous()), _bits(mean))
