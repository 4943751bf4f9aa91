#!/usr/bin/env python3
"""Validation of config A (main.py:49-132) on the MI355X: what the metrics cost next to the forward.

    python3 profiles/validation_probe.py [--batches 20] [--batch 1024] [--out FILE]

Config A (64^2 pairs, patch 8, D 384, 8 + 8 blocks, 4 bins), random weights, bf16 autocast, eval mode, no_grad, device-resident
uint8 batches.  Per batch, the three variants run back to back (host clock, each ending in a device synchronise):
  (a) forward alone;
  (b) forward + engine.ClassificationMeters.update (one vited_cls_metrics_update launch);
  (c) forward + the reference's per-batch work: BCEWithLogitsLoss, .cpu() of logits and targets, 16 sklearn calls, loss.item()
      (skipped with a message when sklearn does not import);
and, for the update alone: the device time per call of REPS calls queued back to back between two events (bounded below by
the host's launch rate, so it is the kernel time only where the kernel is the longer of the two) and the host time of one call.
The kernel's own duration comes from a separate run under ``rocprofv3 --kernel-trace --stats`` (the ``cls_metrics_kernel`` row).
Prints one JSON line (medians and the per-batch lists).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vited_amd as v  # noqa: E402

REPS = 500


def reference_batch_metrics(output, target, sk):
    """main.py:71-93 for one batch: the loss and the host metrics (returns the five values the meters would be updated with)."""
    loss = torch.nn.functional.binary_cross_entropy_with_logits(output, target)
    outputs, targets = torch.unbind(output.cpu(), dim=1), torch.unbind(target.cpu(), dim=1)
    acc, f1, prec, rec = [], [], [], []
    for out, y in zip(outputs, targets):
        pred, gt = (out > 0).float().numpy(), y.numpy()
        acc.append(sk.accuracy_score(gt, pred) * 100)
        f1.append(sk.f1_score(gt, pred, average='macro'))
        prec.append(sk.precision_score(gt, pred, average='macro'))
        rec.append(sk.recall_score(gt, pred, average='macro'))
    return [loss.item()] + [sum(v) / len(v) for v in (acc, f1, prec, rec)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=20)
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    try:
        import warnings

        import sklearn.metrics as sk
        warnings.simplefilter('ignore')
    except ImportError as e:
        sk = None
        print(f'variant (c) skipped: sklearn does not import ({e})', file=sys.stderr)

    dev = torch.device('cuda:0')
    v._lib.load()
    torch.manual_seed(0)
    cfg = v.config_from_yaml(os.path.join(ROOT, 'configs', 'puzzle', 'div2k_erosion7_4bin_patch8_64.yaml'))
    model = v.build_model(cfg).to(dev).eval()
    model.compute_dtype = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(1)
    b = args.batch
    xs = [torch.randint(0, 256, (b, 2, 3, 64, 64), dtype=torch.uint8, device=dev, generator=g) for _ in range(args.batches)]
    ys = [(torch.rand(b, 4, device=dev, generator=g) < 0.25).float() for _ in range(args.batches)]
    meters = v.engine.ClassificationMeters(4, dev)

    def forward(x):
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            return model(x)

    for i in range(3):                                         # warm-up of every path
        out = forward(xs[i])
        meters.update(out, ys[i])
        if sk is not None:
            reference_batch_metrics(out, ys[i], sk)
    torch.cuda.synchronize()

    fwd, fwd_upd, fwd_ref = [], [], []
    for x, y in zip(xs, ys):
        fwd.append(timed(lambda: forward(x)))
        fwd_upd.append(timed(lambda: meters.update(forward(x), y)))
        if sk is not None:
            fwd_ref.append(timed(lambda: reference_batch_metrics(forward(x), y, sk)))

    out = forward(xs[0])
    queued = []                                                # events around REPS calls queued back to back
    for _ in range(5):
        torch.cuda.synchronize()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            meters.update(out, ys[0])
        e.record()
        e.synchronize()
        queued.append(a.elapsed_time(e) * 1e3 / REPS)
    host_us = []
    torch.cuda.synchronize()
    for _ in range(200):                                       # the host cost of one update call (validation + launch)
        t0 = time.perf_counter()
        meters.update(out, ys[0])
        host_us.append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize()

    med = lambda xs: round(statistics.median(xs), 3) if xs else None
    res = {'probe': 'validation', 'config': 'A', 'batch': b, 'batches': args.batches, 'dtype': 'bf16',
           'forward_ms': med(fwd), 'forward_update_ms': med(fwd_upd), 'forward_reference_ms': med(fwd_ref),
           'update_queued_us_per_call': med(queued), 'update_host_us': med(host_us), 'sklearn': sk is not None,
           'per_batch_ms': {'forward': [round(t, 3) for t in fwd], 'forward_update': [round(t, 3) for t in fwd_upd],
                            'forward_reference': [round(t, 3) for t in fwd_ref]},
           'device': torch.cuda.get_device_name(dev)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
