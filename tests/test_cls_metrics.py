"""CPU: the arithmetic of vited_cls_metrics_update (csrc/cls_metrics.hip) restated in numpy reproduces the reference's validation
values (tests/golden/cls_metrics.npz, written by tools/make_cls_metrics_golden.py from main.py's loop and sklearn): per batch and
after AverageMeter.all_reduce, bit for bit.  The loss is the one value that is not: the kernel's fp32 sum order and libm are its
own, so it agrees with torch's BCEWithLogitsLoss within a tolerance.  engine.ClassificationMeters runs here with the launch
stubbed by this restatement, which checks its fp32 all-reduce arithmetic at world size 1."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cls_metrics.npz')
THREADS, WAVE = 256, 64                          # the kernel's workgroup: fixes the fp32 loss summation order


def golden():
    g = np.load(GOLDEN)
    names = sorted({k.split('__')[0] for k in g.files if '__' in k})
    return g, names


def _macro(has0, v0, has1, v1):
    return (v0 + v1) / 2.0 if has0 and has1 else (v0 if has0 else v1)


def _ratio(num, den):
    return float(num) / float(den) if den else 0.0


def batch_values(logits, targets):
    """(loss, acc, f1, precision, recall, bad) of one batch as the kernel computes them; fp32 logits / targets [B, C]."""
    x = np.ascontiguousarray(logits, dtype=np.float32)
    y = np.ascontiguousarray(targets, dtype=np.float32)
    b, c = x.shape
    with np.errstate(invalid='ignore', over='ignore'):
        m = np.maximum(-x, np.float32(0))
        m[np.isnan(x)] = 0                               # fmaxf(NaN, 0) = 0
        elem = (np.float32(1) - y) * x + m + np.log(np.exp(-m) + np.exp(-x - m))
    # lane t sums elements t, t + 256, ... in order (Kahan); a xor butterfly inside each wave; the waves in order
    flat = elem.astype(np.float32).reshape(-1)
    lanes, carry = np.zeros(THREADS, dtype=np.float32), np.zeros(THREADS, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        for lo in range(0, flat.size, THREADS):
            k = min(THREADS, flat.size - lo)
            term = flat[lo:lo + k] - carry[:k]
            nxt = lanes[:k] + term
            carry[:k] = np.where(np.isfinite(nxt), (nxt - lanes[:k]) - term, np.float32(0))
            lanes[:k] = nxt
    waves = lanes.reshape(THREADS // WAVE, WAVE)
    for off in (32, 16, 8, 4, 2, 1):
        waves = waves + waves[:, np.arange(WAVE) ^ off]
    total = waves[0, 0]
    for w in range(1, THREADS // WAVE):
        total = np.float32(total + waves[w, 0])
    loss = float(np.float32(total / np.float32(b * c)))

    ok = (y == 0) | (y == 1)
    truth, pred = ok & (y == 1), ok & (x > 0)
    cols = np.zeros((4, c))
    for j in range(c):
        nt1, np1, tp1 = int(truth[:, j].sum()), int(pred[:, j].sum()), int((truth[:, j] & pred[:, j]).sum())
        nt0, np0, tp0 = b - nt1, b - np1, b - nt1 - np1 + tp1
        has0, has1 = nt0 > 0 or np0 > 0, nt1 > 0 or np1 > 0
        cols[0, j] = float(tp0 + tp1) / float(b) * 100.0
        cols[1, j] = _macro(has0, _ratio(2 * tp0, nt0 + np0), has1, _ratio(2 * tp1, nt1 + np1))
        cols[2, j] = _macro(has0, _ratio(tp0, np0), has1, _ratio(tp1, np1))
        cols[3, j] = _macro(has0, _ratio(tp0, nt0), has1, _ratio(tp1, nt1))
    means = []
    for k in range(4):
        s = 0.0
        for v in cols[k]:
            s = s + float(v)
        means.append(s / c)
    return (loss, *means, bool((~ok).any()))


def meters_update(meters, values, n):
    """AverageMeter.update(val, n) on the (sum, count) pairs of the 5 meters, in fp64 (float64 numpy [10], in place)."""
    for k, v in enumerate(values[:5]):
        meters[2 * k] = meters[2 * k] + float(v) * float(n)
        meters[2 * k + 1] = meters[2 * k + 1] + float(n)


def reduced_averages(per_rank_meters):
    """The reference's AverageMeter.all_reduce per meter: each rank's (sum, count) rounded to fp32, summed in fp32 over the
    ranks in rank order, widened back, sum / count."""
    total = np.zeros(10, dtype=np.float32)
    for m in per_rank_meters:
        total = total + np.asarray(m, dtype=np.float64).astype(np.float32)
    t = total.astype(np.float64)
    return [float(t[2 * k] / t[2 * k + 1]) for k in range(5)], int(t[1])


def stub_update(logits, targets, meters, last, bad):
    """What ops.cls_metrics_update does to the device state, on CPU tensors (for the engine tests without a GPU)."""
    vals = batch_values(logits.float().numpy(), targets.float().numpy())
    state = meters.numpy()
    meters_update(state, vals, logits.shape[0])
    last.copy_(torch.tensor(vals[:5], dtype=torch.float64))
    if vals[5]:
        bad.fill_(1)


def _case(g, name):
    x, y = g[name + '__logits'], g[name + '__targets']
    bounds = np.concatenate([[0], np.cumsum(g[name + '__batches'])])
    return [(x[lo:hi], y[lo:hi]) for lo, hi in zip(bounds[:-1], bounds[1:])]


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def test_golden_file_is_small_and_complete():
    g, names = golden()
    assert os.path.getsize(GOLDEN) < 256 * 1024
    assert str(g['sklearn_version']).startswith('1.7')
    assert {'config_a', 'single_row', 'edge_columns', 'signed_zeros', 'nan_logits', 'one_column', 'seven_columns'} <= set(names)
    for name in names:
        assert g[name + '__logits'].dtype == np.float32 and g[name + '__targets'].dtype == np.uint8
        assert g[name + '__values'].shape == (len(g[name + '__batches']), 5)
    x = g['signed_zeros__logits']
    assert ((x == 0) & np.signbit(x)).any() and ((x == 0) & ~np.signbit(x)).any()


@pytest.mark.parametrize('name', golden()[1])
def test_restatement_reproduces_the_reference_per_batch(name):
    g, _ = golden()
    want = g[name + '__values']
    for i, (x, y) in enumerate(_case(g, name)):
        got = batch_values(x, y)
        assert not got[5]
        np.testing.assert_array_equal(_bits(got[1:5]), _bits(want[i, 1:]), err_msg=f'{name} batch {i}')
        np.testing.assert_allclose(got[0], want[i, 0], rtol=1e-6, equal_nan=True)


@pytest.mark.parametrize('name', golden()[1])
def test_meter_arithmetic_reproduces_the_reference_averages(name):
    """The reference's per-batch values through the kernel's meter update and the fp32 all-reduce give its averages exactly."""
    g, _ = golden()
    meters = np.zeros(10)
    for row, (x, _) in zip(g[name + '__values'], _case(g, name)):
        meters_update(meters, row, x.shape[0])
    avg, samples = reduced_averages([meters])
    np.testing.assert_array_equal(_bits(avg), _bits(g[name + '__final']))
    assert samples == int(g[name + '__samples'])


@pytest.mark.parametrize('name', golden()[1])
def test_engine_meters_at_world_size_one(vited, monkeypatch, name):
    """ClassificationMeters with the launch stubbed: update per batch, then all_reduce without a process group."""
    from vited_amd import engine, ops
    monkeypatch.setattr(ops, 'cls_metrics_update', stub_update)
    g, _ = golden()
    batches = _case(g, name)
    meters = engine.ClassificationMeters(num_classes=batches[0][0].shape[1], device='cpu')
    for i, (x, y) in enumerate(batches):
        meters.update(torch.from_numpy(x), torch.from_numpy(y))
        vals = meters.values()
        assert _bits(vals['acc'].val) == _bits(g[name + '__values'][i, 1])
    res = meters.all_reduce()
    want = g[name + '__final']
    np.testing.assert_array_equal(_bits([res.acc, res.f1, res.precision, res.recall]), _bits(want[1:]))
    np.testing.assert_allclose(res.loss, want[0], rtol=1e-6, equal_nan=True)
    assert res.samples == int(g[name + '__samples'])
    meters.reset()
    with pytest.raises(ValueError, match='no validation sample'):
        meters.all_reduce()


def test_engine_meters_raise_on_a_bad_target(vited, monkeypatch):
    from vited_amd import engine, ops
    monkeypatch.setattr(ops, 'cls_metrics_update', stub_update)
    meters = engine.ClassificationMeters(4, 'cpu')
    y = torch.zeros(8, 4)
    y[3, 2] = 0.5
    meters.update(torch.randn(8, 4), y)
    with pytest.raises(ValueError, match='targets must be 0 or 1'):
        meters.all_reduce()


def test_sklearn_agrees_with_the_golden():
    sk = pytest.importorskip('sklearn.metrics')
    import warnings
    g, names = golden()
    for name in names:
        for i, (x, y) in enumerate(_case(g, name)):
            rows = []
            for j in range(x.shape[1]):
                pred, gt = (torch.from_numpy(x[:, j]) > 0).float().numpy(), y[:, j].astype(np.float32)
                with warnings.catch_warnings():
                    warnings.simplefilter('ignore')
                    rows.append([sk.accuracy_score(gt, pred) * 100, sk.f1_score(gt, pred, average='macro'),
                                 sk.precision_score(gt, pred, average='macro'), sk.recall_score(gt, pred, average='macro')])
            means = [sum(col) / len(col) for col in zip(*rows)]
            np.testing.assert_array_equal(_bits(means), _bits(g[name + '__values'][i, 1:]), err_msg=f'{name} batch {i}')


def test_ops_refuse_cpu_tensors(vited):
    from vited_amd import ops
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.cls_metrics_update(torch.zeros(2, 4), torch.zeros(2, 4), torch.zeros(10, dtype=torch.float64),
                               torch.zeros(5, dtype=torch.float64), torch.zeros(1, dtype=torch.int32))


def test_restated_loss_at_infinite_logits_follows_torch():
    """An overflowing logit gives torch's loss: inf for (+inf, 0), NaN where torch gives NaN; the compensated sum keeps inf."""
    inf = float('inf')
    for x, y in ((inf, 0.0), (inf, 1.0), (-inf, 1.0), (-inf, 0.0)):
        logits = np.full((600, 4), 0.5, dtype=np.float32)
        targets = np.zeros((600, 4), dtype=np.float32)
        logits[7, 2], targets[7, 2] = x, y
        want = torch.nn.functional.binary_cross_entropy_with_logits(torch.from_numpy(logits), torch.from_numpy(targets)).item()
        got = batch_values(logits, targets)[0]
        assert (np.isnan(got) and np.isnan(want)) or got == want, (x, y, got, want)
