"""Validation metrics on the MI355X: vited_cls_metrics_update (csrc/cls_metrics.hip) through engine.ClassificationMeters against the
reference's values (tests/golden/cls_metrics.npz), torch's BCEWithLogitsLoss, itself (run to run), its argument checks and the
no-sync contract; engine.validate_classifier against the reference loop restated on the host from the same logits."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import vited_oracle as vo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cls_metrics import _bits, _case, batch_values, golden, meters_update, reduced_averages  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(engine, batches, dev):
    meters = engine.ClassificationMeters(batches[0][0].shape[1], dev)
    lasts = []
    for x, y in batches:
        meters.update(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
        lasts.append(meters.last.clone())
    torch.cuda.synchronize()
    return meters, torch.stack(lasts).cpu().numpy()


@pytest.mark.parametrize('name', golden()[1])
def test_kernel_matches_the_reference(gpu, name):
    from vited_amd import engine
    g, _ = golden()
    batches = _case(g, name)
    meters, lasts = _run(engine, batches, gpu)
    want = g[name + '__values']
    np.testing.assert_array_equal(_bits(lasts[:, 1]), _bits(want[:, 1]))          # accuracy: the correct counts are exact
    np.testing.assert_allclose(lasts[:, 2:], want[:, 2:], rtol=0, atol=1e-12)
    np.testing.assert_allclose(lasts[:, 0], want[:, 0], rtol=1e-6, equal_nan=True)
    # the device meters hold the kernel's per-batch values updated as AverageMeter does
    host = np.zeros(10)
    for row, (x, _) in zip(lasts, batches):
        meters_update(host, row, x.shape[0])
    np.testing.assert_array_equal(_bits(meters.meters.cpu().numpy()), _bits(host))
    res = meters.all_reduce()
    avg, samples = reduced_averages([host])
    np.testing.assert_array_equal(_bits(list(res[:5])), _bits(avg))
    final = g[name + '__final']
    np.testing.assert_array_equal(_bits([res.acc, res.f1, res.precision, res.recall]), _bits(final[1:]))
    np.testing.assert_allclose(res.loss, final[0], rtol=1e-6, equal_nan=True)
    assert res.samples == samples == int(g[name + '__samples'])


def test_loss_matches_torch_and_runs_are_bit_identical(gpu):
    from vited_amd import engine
    torch.manual_seed(3)
    for b, c in ((1024, 4), (777, 7), (1, 1), (5000, 64)):
        x = torch.randn(b, c, device=gpu) * 4
        y = (torch.rand(b, c, device=gpu) < 0.3).float()
        want = torch.nn.functional.binary_cross_entropy_with_logits(x, y)
        runs = []
        for _ in range(2):
            m = engine.ClassificationMeters(c, gpu)
            m.update(x, y)
            m.update(x[: b // 2 + 1], y[: b // 2 + 1])
            runs.append(torch.cat([m.meters, m.last]).cpu().numpy())
        np.testing.assert_array_equal(_bits(runs[0]), _bits(runs[1]))
        m = engine.ClassificationMeters(c, gpu)
        m.update(x, y)
        torch.testing.assert_close(m.last[0].float(), want, rtol=1e-6, atol=0)
        ref = batch_values(x.cpu().numpy(), y.cpu().numpy())
        np.testing.assert_array_equal(_bits(m.last[1].item()), _bits(ref[1]))
        np.testing.assert_allclose(m.last[2:].cpu().numpy(), ref[2:5], rtol=0, atol=1e-12)


def test_loss_at_infinite_logits_follows_torch(gpu):
    from vited_amd import engine
    inf = float('inf')
    for x, y in ((inf, 0.0), (inf, 1.0), (-inf, 1.0), (-inf, 0.0)):
        logits = torch.full((600, 4), 0.5, device=gpu)
        targets = torch.zeros((600, 4), device=gpu)
        logits[7, 2], targets[7, 2] = x, y
        want = torch.nn.functional.binary_cross_entropy_with_logits(logits, targets).item()
        m = engine.ClassificationMeters(4, gpu)
        m.update(logits, targets)
        got = m.last[0].item()
        assert (np.isnan(got) and np.isnan(want)) or got == want, (x, y, got, want)


def test_casts_and_strides(gpu):
    from vited_amd import engine
    torch.manual_seed(4)
    x = torch.randn(300, 10, device=gpu)
    y = (torch.rand(300, 10, device=gpu) < 0.5)
    a = engine.ClassificationMeters(4, gpu)
    a.update(x[:, 2:6], y[:, 2:6].to(torch.uint8))                # strided rows, uint8 targets
    b = engine.ClassificationMeters(4, gpu)
    b.update(x[:, 2:6].contiguous(), y[:, 2:6].float())
    assert torch.equal(a.meters, b.meters)
    c = engine.ClassificationMeters(4, gpu)
    c.update(x[:, 2:6].bfloat16(), y[:, 2:6].float())
    d = engine.ClassificationMeters(4, gpu)
    d.update(x[:, 2:6].bfloat16().float(), y[:, 2:6].float())
    assert torch.equal(c.meters, d.meters)


def test_bad_target_raises_at_all_reduce(gpu):
    from vited_amd import engine
    m = engine.ClassificationMeters(4, gpu)
    y = torch.zeros(16, 4, device=gpu)
    m.update(torch.randn(16, 4, device=gpu), y)
    m.all_reduce()
    y[5, 1] = 0.5
    m.update(torch.randn(16, 4, device=gpu), y)
    with pytest.raises(ValueError, match='targets must be 0 or 1'):
        m.all_reduce()
    m.reset()
    y[5, 1] = float('nan')
    m.update(torch.randn(16, 4, device=gpu), y)
    with pytest.raises(ValueError, match='targets must be 0 or 1'):
        m.all_reduce()


def test_bad_arguments_raise_before_the_launch(gpu):
    from vited_amd import ops
    x, y = torch.randn(8, 4, device=gpu), torch.zeros(8, 4, device=gpu)
    meters, last = torch.zeros(10, dtype=torch.float64, device=gpu), torch.zeros(5, dtype=torch.float64, device=gpu)
    bad = torch.zeros(1, dtype=torch.int32, device=gpu)
    bad_calls = [
        ((x, y[:7], meters, last, bad), ValueError),                                   # shapes differ
        ((x[:0], y[:0], meters, last, bad), ValueError),                               # no rows
        ((torch.randn(8, 65, device=gpu), torch.zeros(8, 65, device=gpu), meters, last, bad), ValueError),   # > 64 columns
        ((x.t(), y.t(), meters, last, bad), ValueError),                               # column stride
        ((x.int(), y, meters, last, bad), TypeError),                                  # integer logits
        ((x, y, meters.float(), last, bad), ValueError),                               # fp32 meters
        ((x, y, meters, last[:4], bad), ValueError),
        ((x, y, meters, last, bad.long()), ValueError),
        ((x.cpu(), y, meters, last, bad), RuntimeError),                               # a CPU tensor
    ]
    for args, err in bad_calls:
        with pytest.raises(err):
            ops.cls_metrics_update(*args)
    torch.cuda.synchronize()
    assert not meters.any() and not last.any() and not bad.any()
    lib = __import__('vited_amd')._lib.load()
    p = lambda t: t.data_ptr()
    assert lib.vited_cls_metrics_update(p(x), 4, p(y), 4, 8, 0, p(meters), p(last), p(bad), None) == 1
    assert lib.vited_cls_metrics_update(p(x), 3, p(y), 4, 8, 4, p(meters), p(last), p(bad), None) == 1
    assert lib.vited_cls_metrics_update(p(x), 4, p(y), 4, 0, 4, p(meters), p(last), p(bad), None) == 1
    assert lib.vited_cls_metrics_update(None, 4, p(y), 4, 8, 4, p(meters), p(last), p(bad), None) == 1
    assert lib.vited_cls_metrics_update(p(x), 4, p(y), 4, 8, 4, p(meters) + 4, p(last), p(bad), None) == 1


def test_update_does_not_synchronise(gpu):
    from vited_amd import engine
    x = torch.randn(1024, 4, device=gpu)
    y = (torch.rand(1024, 4, device=gpu) < 0.25).float()
    m = engine.ClassificationMeters(4, gpu)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for _ in range(3):
            m.update(x, y)
            m.update(x.bfloat16(), y.to(torch.uint8))
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert m.values()['loss'].val > 0


class _Recording(torch.nn.Module):
    """The model, keeping a copy of every output it returns (the logits the reference loop would see)."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.seen = inner, []

    def forward(self, x):
        out = self.inner(x)
        self.seen.append(out.detach().float().cpu())
        return out


def test_validate_classifier_equals_the_reference_loop(gpu):
    import vited_amd
    from vited_amd import engine
    torch.manual_seed(0)
    s = vo.ViTEDShape(depth=1, c_depth=1)
    model = vited_amd.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, num_classes=s.num_classes,
                                              embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads).to(gpu)
    model.train()
    rec = _Recording(model)
    rec.train()
    gen = torch.Generator().manual_seed(1)
    sizes = [64, 64, 64, 64, 23]
    loader = [(torch.randint(0, 256, (b, 2, 3, 64, 64), dtype=torch.uint8, generator=gen),
               (torch.rand(b, 4, generator=gen) < 0.25).float()) for b in sizes]
    logged = []
    res = engine.validate_classifier(rec, loader, amp=True, print_freq=2, log=lambda i, v: logged.append((i, v)))
    assert rec.training and model.training
    assert [i for i, _ in logged] == [0, 2, 4]
    host, last = np.zeros(10), None
    for out, (_, y) in zip(rec.seen, loader):
        last = batch_values(out.numpy(), y.numpy())
        meters_update(host, last, y.shape[0])
    want, samples = reduced_averages([host])
    assert len(rec.seen) == len(sizes) and res.samples == samples == sum(sizes)
    np.testing.assert_array_equal(_bits([res.acc, res.f1, res.precision, res.recall]), _bits(want[1:]))
    np.testing.assert_allclose(res.loss, want[0], rtol=1e-6)
    # the reference's loss of those logits, as torch computes it
    ref_loss = sum(float(torch.nn.functional.binary_cross_entropy_with_logits(o, y)) * y.shape[0]
                   for o, (_, y) in zip(rec.seen, loader)) / sum(sizes)
    np.testing.assert_allclose(res.loss, ref_loss, rtol=1e-5)
    assert logged[-1][1]['acc'].val == pytest.approx(last[1], abs=0)

    # batches already on the device are used as they are; the model stays in eval mode when it was
    rec.eval()
    rec.seen.clear()
    res2 = engine.validate_classifier(rec, [(x.to(gpu), y.to(gpu)) for x, y in loader], amp=True)
    assert not rec.training and not model.training
    host = np.zeros(10)
    for out, (_, y) in zip(rec.seen, loader):
        meters_update(host, batch_values(out.numpy(), y.numpy()), y.shape[0])
    want, samples = reduced_averages([host])
    assert res2.samples == samples
    np.testing.assert_array_equal(_bits([res2.acc, res2.f1, res2.precision, res2.recall]), _bits(want[1:]))
