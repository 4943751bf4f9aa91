#!/usr/bin/env python3
"""What the Pillow-exact resize costs on the MI355X: the kernel alone, one Pajigsaw batch, and the two callers it
was built for beside the work they feed.

    python3 profiles/resample_probe.py [--rounds 5] [--images 512] [--steps 10] [--out profiles/resample_probe.json]

One process.  Every figure is the median of ``--rounds`` rounds with the lowest and the highest, between device events; arms that are
compared alternate inside every round.
  kernel      ``ops.resample_u8`` of 48 whole fragments of side 512 / 1024 / 2048 to 512, and of michigan.py's evaluation window (512 ->
              588, the 512 crop at 38) for 256 images; 20 calls captured into one hipGraph per arm, so the events time the device and
              not the host's launches (the class lookup - four small torch kernels - is inside).  Bytes moved = the window's source
              pixels read once + the output written once; GB/s is that over the time.
  batch       one Pajigsaw batch at B = 24 from fragments of side 700 to 512: uniforms, ``pajigsaw_pair_plan``, two resize launches;
              eager, 20 calls per round, so it includes the host's launches.
  similarity  ``engine.pairwise_similarity`` with config H's model on ``--images`` images of 512 x 512: fed by ``MichiganEvalSource``
              from the store, against the same images pre-transformed and resident.
  step        ``engine.TrainStep`` on the Pajigsaw model (pajigsaw_patch16_512: 512-pixel images, patch 16, width 384, 12 + 12 blocks,
              4 classes) at B = 24, bf16: ``--steps`` steps fed by ``PajigsawDeviceLoader`` against the same number on one resident batch.
Prints one JSON line and writes it to ``--out``."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vited_amd as v  # noqa: E402


def graphed(f, calls):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            f()
    return g.replay


def timed(arms, rounds, calls, replays=False, warm=2):
    """{arm: [us per call, one figure per round]}, the arms alternating inside every round."""
    for f in arms.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    us = {name: [] for name in arms}
    for _ in range(rounds):
        for name, f in arms.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(1 if replays else calls):
                f()
            e.record()
            e.synchronize()
            us[name].append(round(a.elapsed_time(e) * 1000.0 / calls, 2))
    return us


def summary(us):
    return {k: [round(statistics.median(t), 2), min(t), max(t)] for k, t in us.items()}


def device_images(n, side, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return [torch.randint(0, 256, (side, side, 3), dtype=torch.uint8, device=dev, generator=g) for _ in range(n)]


def grid(name, rows, cols):
    return {'Fragment1v1Rotate90': [{'im_path': f'{name}/r{r}c{c}.png', 'row': r, 'col': c, 'degree': 0, 'white_percentage': 0.0}
                                    for r in range(rows) for c in range(cols)]}


def kernel_arms(dev, rounds, calls=20):
    E, ops, S = v.engine, v.ops, 512
    res = {}
    for side in (512, 1024, 2048):
        store = E.Div2kImageStore(device_images(48, side, dev, side), dev)
        t = ops.resample_tables([side], S, dev)
        idx = torch.arange(48, dtype=torch.int32, device=dev)
        out = torch.empty(48, 3, S, S, dtype=torch.uint8, device=dev)
        f = lambda: ops.resample_u8(store.data, store.offsets_dev, store.sizes_dev, idx, None, 0, t, t, S, S, 0, 0, S, out=out)
        us = timed({'call': graphed(f, calls)}, rounds, calls, replays=True)['call']
        moved = 48 * (side * side * 3 + 3 * S * S)
        res[f'{side}_to_512_x48'] = {'us': us, 'median_low_high_us': summary({'c': us})['c'], 'bytes_moved': moved,
                                     'gb_per_s_at_median': round(moved / statistics.median(us) / 1e3, 1)}
        del store, out
        torch.cuda.empty_cache()
    store = E.Div2kImageStore(device_images(256, S, dev, 7), dev)
    src = E.MichiganEvalSource(store, S)
    idx = torch.arange(256, dtype=torch.int32, device=dev)
    out = torch.empty(256, 3, S, S, dtype=torch.uint8, device=dev)
    f = lambda: ops.resample_u8(store.data, store.offsets_dev, store.sizes_dev, idx, src.windows, 255, src.tables, src.tables, src.resized, src.resized,
                                src.crop, src.crop, S, out=out)
    us = timed({'call': graphed(f, calls)}, rounds, calls, replays=True)['call']
    moved = 256 * 2 * 3 * S * S
    res['michigan_eval_512_to_588_crop_x256'] = {'us': us, 'median_low_high_us': summary({'c': us})['c'], 'bytes_moved': moved,
                                                 'gb_per_s_at_median': round(moved / statistics.median(us) / 1e3, 1)}
    return res


def pajigsaw_loader(dev, batch, seed=1):
    E = v.engine
    index = E.pajigsaw_index({f'img{k:02d}': grid(f'img{k:02d}', 4, 4) for k in range(16)})
    store = E.Div2kImageStore(device_images(len(index.im_path), 700, dev, 11), dev)
    return E.PajigsawDeviceLoader(store, index, batch, 512, seed=seed)


def batch_arm(dev, rounds, calls=20):
    loader = pajigsaw_loader(dev, 24)
    sample, g = loader.rank_indices()[0], loader._generator(1)
    us = timed({'plan_and_two_resizes': lambda: loader.feed(*loader.plan(sample, g)[:2])}, rounds, calls)
    return {'us': us, 'median_low_high_us': summary(us)}


def similarity_arms(dev, rounds, n_images):
    E, S = v.engine, 512
    cfg = v.config_from_yaml(os.path.join(ROOT, 'configs', 'hisfrag', 'hisfrag20_patch16_512.yaml'))
    torch.manual_seed(0)
    model = v.build_model(cfg).to(dev).eval()
    store = E.Div2kImageStore(device_images(n_images, S, dev, 13), dev)
    src = E.MichiganEvalSource(store, S)
    resident = src(0, n_images)
    arms = {'source_fed': lambda: E.pairwise_similarity(model, src, n_images=len(src)), 'resident': lambda: E.pairwise_similarity(model, resident)}
    same = bool(torch.equal(arms['source_fed'](), arms['resident']()))
    us = timed(arms, rounds, 1, warm=0)
    ms = {k: [round(t / 1000.0, 2) for t in ts] for k, ts in us.items()}
    return {'images': n_images, 'pairs': n_images * (n_images + 1) // 2, 'matrices_equal': same, 'ms': ms, 'median_low_high_ms': summary(ms)}


def step_arms(dev, rounds, steps):
    E = v.engine
    cfg = v.config._C.clone()
    cfg.defrost()
    cfg.merge_from_list(['DATA.DATASET', 'pajigsaw', 'DATA.IMG_SIZE', 512, 'MODEL.NUM_CLASSES', 4, 'MODEL.PJS.PATCH_SIZE', 16, 'MODEL.PJS.EMBED_DIM', 384,
                         'MODEL.PJS.NUM_HEADS', 6, 'MODEL.PJS.DEPTH', 12, 'MODEL.PJS.C_DEPTH', 12])
    cfg.freeze()
    loader = pajigsaw_loader(dev, 24)
    if len(loader) < steps:
        raise RuntimeError(f'{len(loader)} batches per epoch, {steps} steps per round')
    fixed = next(iter(loader))
    runs = {}
    for name in ('loader_fed', 'resident_batch'):
        torch.manual_seed(0)
        model = v.build_model(cfg).to(dev).train()
        opt = v.optim.FlatAdamW(E.param_groups_no_decay_1d(model), lr=1e-4, weight_decay=0.05, model=model)
        runs[name] = E.TrainStep(model, opt, clip_grad=5.0, amp=True)

    def loader_fed():
        for k, (pairs, labels) in enumerate(loader):
            if k == steps:
                break
            runs['loader_fed'].step(pairs, labels)

    def resident_batch():
        for _ in range(steps):
            runs['resident_batch'].step(*fixed)

    us = timed({'loader_fed': loader_fed, 'resident_batch': resident_batch}, rounds, 1, warm=1)
    ms = {k: [round(t / 1000.0 / steps, 3) for t in ts] for k, ts in us.items()}
    return {'batch': 24, 'steps_per_round': steps, 'ms_per_step': ms, 'median_low_high_ms': summary(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--images', type=int, default=512)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--parts', default='kernel,batch,similarity,step')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resample_probe.json'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    v._lib.load()
    res = {'probe': 'resample', 'rounds': args.rounds, 'device': torch.cuda.get_device_name(dev)}
    parts = {'kernel': lambda: kernel_arms(dev, args.rounds), 'batch': lambda: batch_arm(dev, args.rounds),
             'similarity': lambda: similarity_arms(dev, args.rounds, args.images), 'step': lambda: step_arms(dev, args.rounds, args.steps)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.parts.split(','):
        res[name] = parts[name]()
        torch.cuda.empty_cache()
        print(f'{name}: done', file=sys.stderr, flush=True)
        if args.out:                                    # after every part: a run that is cut short keeps what it measured
            with open(args.out, 'w') as f:
                f.write(json.dumps(res) + '\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
