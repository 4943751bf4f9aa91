"""CPU: engine.TrainMeters against the reference's AverageMeter arithmetic (misc/utils.py:276-303), restated here."""
import math

import pytest
import torch


class AverageMeter:
    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def feed(meters, accum, losses, rows, norms):
    """``losses``: the divided micro-step losses (fp32 tensors), ``rows`` their target rows, ``norms``: one per ``accum`` micro-steps.
    Returns the reference's two meters and its count of non-finite norms."""
    lm, nm, bad = AverageMeter(), AverageMeter(), 0
    for i, (loss, n) in enumerate(zip(losses, rows)):
        meters.update_loss(loss, n)
        lm.update(loss.item() * accum, int(n))
        if (i + 1) % accum == 0:
            norm = norms[i // accum]
            meters.update_norm(norm)
            nm.update(norm.item())
            bad += not math.isfinite(norm.item())
    return lm, nm, bad


@pytest.mark.parametrize('accum', [1, 2])
def test_train_meters_equal_average_meter(vited, accum):
    g = torch.Generator().manual_seed(accum)
    losses = list(torch.rand(8, generator=g) + 0.3)
    rows = [8, 8, 5, 8, 3, 8, 8, 1]                                     # unequal n
    norms = list(torch.rand(8 // accum, generator=g) * 4)
    norms[1] = torch.tensor(float('inf'))                                # a non-finite norm in the middle
    meters = vited.engine.TrainMeters('cpu', accumulation_steps=accum)
    lm, nm, bad = feed(meters, accum, losses, rows, norms)
    v = meters.values()
    assert (v['loss'].val, v['loss'].avg) == (lm.val, lm.avg)           # the same fp64 operations in the same order: exact
    assert v['grad_norm'].val == nm.val and v['grad_norm'].avg == nm.avg == math.inf
    assert v['nonfinite'] == bad == 1
    total = torch.tensor([lm.sum, lm.count], dtype=torch.float32).tolist()
    assert meters.all_reduce() == total[0] / total[1]                    # AverageMeter.all_reduce's fp32 rounding, one process
    # a device scalar as n (MinedPairs.counts[3]) counts like the number
    twin = vited.engine.TrainMeters('cpu', accumulation_steps=accum)
    feed(twin, accum, losses, [torch.tensor(r, dtype=torch.int32) for r in rows], norms)
    assert twin.state.tolist()[:3] == meters.state.tolist()[:3]
    # reset starts an epoch
    meters.reset()
    assert meters.values() == {'loss': (0.0, 0.0), 'grad_norm': (0.0, 0.0), 'nonfinite': 0}
    with pytest.raises(ValueError, match='no training step'):
        meters.all_reduce()
    lm, nm, bad = feed(meters, accum, losses[:4], rows[:4], [torch.tensor(float('nan'))] + norms[2:])
    v = meters.values()
    assert (v['loss'].val, v['loss'].avg) == (lm.val, lm.avg) and v['nonfinite'] == 1
    assert _same(v['grad_norm'].avg, nm.avg) and _same(v['grad_norm'].val, nm.val)


def test_train_step_meters_on_a_cpu_model(vited):
    """TrainStep(meters=True) feeds the meters from its own loop (eager, CPU model, accumulation 2) and trains exactly as without."""
    torch.manual_seed(0)
    models = [torch.nn.Linear(6, 4) for _ in range(2)]
    models[1].load_state_dict(models[0].state_dict())
    steps = [vited.engine.TrainStep(m, torch.optim.SGD(m.parameters(), lr=0.1), amp=False, accumulation_steps=2, meters=flag)
             for m, flag in zip(models, (True, False))]
    assert steps[1].meters is None
    lm, nm = AverageMeter(), AverageMeter()
    for it in range(6):
        x, y = torch.randn(5 + it % 2, 6), (torch.rand(5 + it % 2, 4) > 0.5).float()
        loss = steps[0].step(x, y)
        steps[1].step(x, y)
        lm.update(loss.item() * 2, x.shape[0])
        if it % 2:
            nm.update(steps[0].last_norm.item())
    v = steps[0].meters.values()
    assert (v['loss'].val, v['loss'].avg) == (lm.val, lm.avg) and (v['grad_norm'].val, v['grad_norm'].avg) == (nm.val, nm.avg)
    assert v['nonfinite'] == 0
    for p, q in zip(models[0].parameters(), models[1].parameters()):
        assert torch.equal(p, q)
