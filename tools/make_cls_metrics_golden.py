#!/usr/bin/env python3
"""Writes tests/golden/cls_metrics.npz: validation batches of a 4-bin (and other widths) binary classifier with the values the
reference's validation loop (main.py:49-132) computes from them.

For every case the file holds, as data only:
    <case>__logits   float32 [N, C]      the model outputs of all batches, stacked
    <case>__targets  uint8 [N, C]        0 / 1 targets
    <case>__batches  int64 [nb]          batch sizes (the last one may be partial)
    <case>__values   float64 [nb, 5]     per batch: loss.item(), acc, f1, precision, recall (the values the meters are updated with)
    <case>__final    float64 [5]         the five averages after AverageMeter.all_reduce at world size 1 (fp32 round trip)
    <case>__samples  int64 []            the all-reduced sample count
and ``sklearn_version`` / ``torch_version``.  The loop below restates main.py's literally: torch's BCEWithLogitsLoss, then per
column sklearn's accuracy_score (x 100) and f1 / precision / recall with average="macro", Python sums over the columns, and
AverageMeter's update / all_reduce arithmetic.

    python3 tools/make_cls_metrics_golden.py        (needs scikit-learn; written with 1.7.2)
"""
import os
import warnings

import numpy as np
import sklearn
import torch
from sklearn.metrics import accuracy_score, f1_score, precision_score, recall_score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'cls_metrics.npz')


class AverageMeter:                                         # misc/utils.py:275-303
    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count

    def all_reduce(self):                                   # world size 1: the SUM all-reduce leaves the fp32 values as they are
        total = torch.tensor([self.sum, self.count], dtype=torch.float32)
        self.sum, self.count = total.tolist()
        self.avg = self.sum / self.count


def reference_loop(logits, targets, batches):
    criterion = torch.nn.BCEWithLogitsLoss()
    meters = [AverageMeter() for _ in range(5)]             # loss, acc, f1, precision, recall
    values, lo = [], 0
    for b in batches:
        output = torch.from_numpy(logits[lo:lo + b])
        target = torch.from_numpy(targets[lo:lo + b].astype(np.float32))
        lo += b
        loss = criterion(output, target)
        accuracies, f1s, precisions, recalls = [], [], [], []
        for out, y in zip(torch.unbind(output, dim=1), torch.unbind(target, dim=1)):
            pred, gt = (out > 0).float().numpy(), y.numpy()
            accuracies.append(accuracy_score(gt, pred) * 100)
            f1s.append(f1_score(gt, pred, average="macro"))
            precisions.append(precision_score(gt, pred, average="macro"))
            recalls.append(recall_score(gt, pred, average="macro"))
        row = [loss.item(), sum(accuracies) / len(accuracies), sum(f1s) / len(f1s), sum(precisions) / len(precisions),
               sum(recalls) / len(recalls)]
        for m, v in zip(meters, row):
            m.update(v, target.size(0))
        values.append(row)
    for m in meters:
        m.all_reduce()
    return np.array(values, dtype=np.float64), np.array([m.avg for m in meters], dtype=np.float64), int(meters[0].count)


def random_case(rng, batches, c, p_true=0.25):
    n = sum(batches)
    y = (rng.random((n, c)) < p_true).astype(np.uint8)
    x = (rng.standard_normal((n, c)) * 2.0 + (y * 3.0 - 1.5)).astype(np.float32)
    return x, y


def cases():
    rng = np.random.default_rng(2024)
    out = {}
    out['config_a'] = (*random_case(rng, [1024, 1024, 300], 4), [1024, 1024, 300])   # two full batches and a partial one
    out['single_row'] = (*random_case(rng, [1, 1, 1], 4), [1, 1, 1])
    # column 0: every target and prediction 0; column 1: all 1; column 2: class 1 never predicted; column 3: class 1 never a
    # target but predicted
    n = 96
    x, y = random_case(rng, [n], 4)
    y[:, 0], x[:, 0] = 0, -np.abs(x[:, 0]) - 0.1
    y[:, 1], x[:, 1] = 1, np.abs(x[:, 1]) + 0.1
    x[:, 2] = -np.abs(x[:, 2]) - 0.1
    y[:, 3] = 0
    out['edge_columns'] = (x, y, [64, 32])
    x, y = random_case(rng, [128], 4)
    x[rng.random(x.shape) < 0.3] = 0.0
    x[rng.random(x.shape) < 0.3] = -0.0
    out['signed_zeros'] = (x, y, [100, 28])
    x, y = random_case(rng, [80], 4)
    x[rng.random(x.shape) < 0.05] = np.nan
    out['nan_logits'] = (x, y, [80])
    out['one_column'] = (*random_case(rng, [200, 57], 1, 0.5), [200, 57])
    out['seven_columns'] = (*random_case(rng, [300, 41], 7, 0.4), [300, 41])
    out['sixty_four_columns'] = (*random_case(rng, [48, 16], 64, 0.3), [48, 16])
    return out


def main():
    data = {'sklearn_version': np.array(sklearn.__version__), 'torch_version': np.array(torch.__version__.split('+')[0])}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                     # zero divisions: sklearn warns and uses 0, as the reference does
        for name, (x, y, batches) in cases().items():
            values, final, samples = reference_loop(x, y, batches)
            data.update({f'{name}__logits': x, f'{name}__targets': y, f'{name}__batches': np.array(batches, dtype=np.int64),
                         f'{name}__values': values, f'{name}__final': final, f'{name}__samples': np.array(samples, dtype=np.int64)})
            print(f'{name}: batches {batches}, final {final.tolist()}')
    np.savez_compressed(OUT, **data)
    print(f'wrote {OUT} ({os.path.getsize(OUT)} bytes), sklearn {sklearn.__version__}')


if __name__ == '__main__':
    main()
