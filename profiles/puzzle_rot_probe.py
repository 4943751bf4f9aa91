#!/usr/bin/env python3
"""Learned type-2 puzzles (the pair model on all 16 side pairings) on the MI355X, beside the type-1 path in the same process.

    python3 profiles/puzzle_rot_probe.py [--n 432 540 805] [--reps 2] [--kernel-reps 30] [--out profiles/puzzle_rot_probe.json]

The config-A model (8 + 8 blocks, 64-pixel pieces, bf16, random weights).  Per n (432 / 540 / 805 pieces are the BGU test-set sizes of
DESIGN.md section 14):
  * the wall time of engine.puzzle_distances for puzzle_type 1 and 2 at the default pair_batch / block, synchronised at both ends, after
    one warm-up call of each arm, the arms interleaved (type 1, type 2, type 1, ...); the ratio of the medians;
  * the two new kernels alone, event-timed, --kernel-reps calls after two warm-up calls, interleaved with their upright / type-1
    counterparts: the patch extraction of the n pieces (uint8 -> bf16) upright and under each turn, and the scatter of one pair batch
    (1024 pairs) and of all n (n - 1) pairs of a turn, type 1 and type 2.
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


def _timed(arms, reps):
    """arms: name -> callable.  Interleaved event timing; returns name -> {median, min, max} in ms."""
    for call in arms.values():
        for _ in range(2):
            call()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(reps):
        for name, call in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    return {name: {'median_ms': statistics.median(t), 'min_ms': min(t), 'max_ms': max(t)} for name, t in times.items()}


def _wall(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, nargs='*', default=[432, 540, 805])
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--kernel-reps', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'puzzle_rot_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('puzzle_rot_probe needs the MI355X: nothing is measured without it')
    dev = torch.device('cuda:0')
    ops, engine = v.ops, v.engine
    torch.manual_seed(0)
    model = v.VisionTransformerCustom(img_size=64, patch_size=8, num_classes=4, embed_dim=384, depth=8, c_depth=8, num_heads=12).to(dev).eval()
    model.compute_dtype = torch.bfloat16
    result = {'model': 'config A, 8 + 8 blocks, bf16, random weights', 'reps': args.reps, 'kernel_reps': args.kernel_reps,
              'device': torch.cuda.get_device_name(0), 'boards': {}}
    for n in args.n:
        pieces = torch.randint(0, 256, (n, 3, 64, 64), dtype=torch.uint8, generator=torch.Generator().manual_seed(n)).to(dev)
        arms = {1: lambda: engine.puzzle_distances(model, pieces, puzzle_type=1), 2: lambda: engine.puzzle_distances(model, pieces, puzzle_type=2)}
        for call in arms.values():
            call()
        walls = {1: [], 2: []}
        for _ in range(args.reps):
            for kind, call in arms.items():
                walls[kind].append(_wall(call))
        med = {kind: statistics.median(t) for kind, t in walls.items()}
        pairs = n * (n - 1)
        entry = {'pairs_type1': pairs, 'forwards_type2': 4 * pairs,
                 'puzzle_distances_type1_s': walls[1], 'puzzle_distances_type2_s': walls[2],
                 'type1_pairs_per_s': pairs / med[1], 'type2_forwards_per_s': 4 * pairs / med[2], 'ratio_type2_over_type1': med[2] / med[1]}

        ii, jj = (t.contiguous() for t in torch.nonzero(~torch.eye(n, dtype=torch.bool, device=dev), as_tuple=True))
        logits = torch.randn((pairs, 4), device=dev)
        dq = torch.full((4, n, n), 2 ** 31 - 1, dtype=torch.int32, device=dev)
        dq2 = torch.full((4, n, n, 4), 2 ** 31 - 1, dtype=torch.int32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        jt = (jj + 3 * n).contiguous()
        b = 1024
        kernels = {'patchify_upright': lambda: ops.patchify(pieces, 8, torch.bfloat16),
                   **{f'patchify_turn{k}': (lambda k=k: ops.patchify_turned(pieces, 8, torch.bfloat16, k)) for k in range(4)},
                   'scatter_type1_batch': lambda: ops.puzzle_distances_from_logits(logits[:b], ii[:b], jj[:b], dq, bad),
                   'scatter_type2_batch': lambda: ops.puzzle_distances2_from_logits(logits[:b], ii[:b], jt[:b], dq2, bad),
                   'scatter_type1_all': lambda: ops.puzzle_distances_from_logits(logits, ii, jj, dq, bad),
                   'scatter_type2_all': lambda: ops.puzzle_distances2_from_logits(logits, ii, jt, dq2, bad)}
        entry['kernels'] = _timed(kernels, args.kernel_reps)
        assert int(bad.item()) == 0
        result['boards'][str(n)] = entry
        print(n, json.dumps(entry), flush=True)
        del pieces, logits, dq, dq2
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
