#!/usr/bin/env python3
"""Head-averaged relevancy maps: the fused kernel (ops.attention_cam, csrc/attention_cam.hip) against the KEEP_ATTN slow path
producing the same map (functions._keep_attention + _keep_attention_grad + avg_heads), and the memory peak of
engine.pair_relevancy against that slow path for 8 config-H pairs.

Shapes: config A (12 heads x 32, 65 x 65 self and 65 x 64 cross, B = 256) and config H (6 heads x 64, 1025 x 1025 and
1025 x 1024, B = 4), bf16 operands.  Timing: device events around ``--reps`` calls, after warm-up of both sides at every shape;
the two sides alternate over ``--rounds`` rounds and the median and the spread (min .. max) of the rounds are reported.  The
byte / FLOP figures are what the algorithm needs, from the shapes: operand reads + one fp32 store of the map, 4 Nq Nk hd FLOPs
per head (scores and dP).

    python3 profiles/relevancy_probe.py [--reps 20] [--rounds 5] [--out profiles/relevancy_probe.json] [--skip-memory]
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vited_amd as v  # noqa: E402

ops, F_ = v.ops, v.functions

SHAPES = [('A self', 256, 12, 65, 65, 32), ('A cross', 256, 12, 65, 64, 32), ('H self', 4, 6, 1025, 1025, 64), ('H cross', 4, 6, 1025, 1024, 64)]


def operands(dev, g, B, H, nq, nk, hd):
    D = H * hd
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev).bfloat16()
    if nq == nk:
        qkv = rnd(B, nq, 3 * D)
        q, k, vv = qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:]
    else:
        q, kv = rnd(B, nq, D), rnd(B, nk, 2 * D)
        k, vv = kv[:, :, :D], kv[:, :, D:]
    return q, k, vv, rnd(B, nq, D)


def slow_cam(rt, q, k, vv, do):
    """What the parent offers: both per-head maps in fp32 [B, h, Nq, Nk], then avg_heads per sample."""
    F_._keep_attention(rt, 'probe', q, k)
    F_._keep_attention_grad(rt, 'probe', do, vv)
    ent = rt.attn_store.pop('probe')
    return (ent['attn'] * ent['grad']).clamp(min=0).mean(dim=1)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # us


def kernel_rows(dev, reps, rounds):
    g = torch.Generator(device='cpu').manual_seed(0)
    rows = []
    for name, B, H, nq, nk, hd in SHAPES:
        q, k, vv, do = operands(dev, g, B, H, nq, nk, hd)
        scale = hd ** -0.5
        rt = types.SimpleNamespace(heads=H, head_dim=hd, scale=scale, attn_store={})
        _, lse = ops.attention_fwd(q, k, vv, H, scale)
        out = torch.empty((B, nq, nk), dtype=torch.float32, device=dev)
        fused = lambda: ops.attention_cam(q, k, vv, do, lse, H, scale, mode='grad', out=out)
        slow = lambda: slow_cam(rt, q, k, vv, do)
        want = slow()
        err = float((fused() - want).abs().max() / want.abs().max())
        for _ in range(3):
            fused()
            slow()
        torch.cuda.synchronize()
        tf, ts = [], []
        for _ in range(rounds):
            tf.append(timed(fused, reps))
            ts.append(timed(slow, reps))
        mf, ms = statistics.median(tf), statistics.median(ts)
        bytes_ = (B * (2 * nq + 2 * nk) * H * hd) * 2 + B * H * nq * 4 + B * nq * nk * 4
        flops = 4.0 * B * H * nq * nk * hd
        rows.append(dict(shape=name, batch=B, heads=H, nq=nq, nk=nk, head_dim=hd, fused_us=mf, fused_us_min_max=[min(tf), max(tf)],
                         slow_us=ms, slow_us_min_max=[min(ts), max(ts)], slow_over_fused=ms / mf, max_err_over_max=err,
                         bytes=bytes_, flops=flops, fused_TBps=bytes_ / mf / 1e6, fused_TFLOPs=flops / mf / 1e6,
                         slow_map_bytes=2 * B * H * nq * nk * 4))
        print(f'{name:8s} B={B:3d}  fused {mf:8.1f} us ({min(tf):.1f} .. {max(tf):.1f})   slow {ms:8.1f} us ({min(ts):.1f} .. {max(ts):.1f})'
              f'   x{ms / mf:5.1f}   {bytes_ / mf / 1e6:5.2f} TB/s  {flops / mf / 1e6:6.1f} TFLOP/s   |diff|/max {err:.1e}', flush=True)
    return rows


def memory_peaks(dev, pairs):
    """Config H (12 + 12 blocks, 6 x 64 heads, 512 px / patch 16), bf16: engine.pair_relevancy against the slow path doing the same
    job - keep_attn forward + backward, avg_heads of the 36 attentions, the same propagation."""
    g = torch.Generator(device='cpu').manual_seed(1)
    x = torch.randn(pairs, 2, 3, 512, 512, generator=g).clamp(-1, 1).to(dev)
    res = {}
    for name in ('pair_relevancy', 'slow_path'):
        torch.manual_seed(2)
        model = v.VisionTransformerCustom(img_size=512, patch_size=16, num_classes=1, embed_dim=384, depth=12, c_depth=12, num_heads=6,
                                          keep_attn=name == 'slow_path').to(dev)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if name == 'pair_relevancy':
            rel, _ = v.engine.pair_relevancy(model, x, amp=True, include_cls=True)
        else:
            with torch.autocast('cuda', dtype=torch.bfloat16):
                logits = model(x)
            logits.backward(torch.ones_like(logits))        # one class: the arg-max one-hot
            holders = ([b.attn for b in model.blocks], [b.attn for b in model.cross_blocks], [b.cross_attn for b in model.cross_blocks])
            cams = [[(h.get_attn() * h.get_attn_gradients()).clamp(min=0).mean(dim=1).double() for h in group] for group in holders]
            rel = v.engine.relevancy_from_cams(*cams).float()
        e1.record()
        torch.cuda.synchronize()
        res[name] = dict(peak_bytes=torch.cuda.max_memory_allocated(), model_and_input_bytes=base, first_call_ms=e0.elapsed_time(e1),
                         finite=bool(torch.isfinite(rel).all()))
        if name == 'pair_relevancy':                        # a second call: without the first call's code-object loads and library set-up
            e0.record()
            v.engine.pair_relevancy(model, x, amp=True, include_cls=True)
            e1.record()
            torch.cuda.synchronize()
            res[name]['second_call_ms'] = e0.elapsed_time(e1)
        res[name + '_rel'] = rel
        print(f'{name:15s} {pairs} config-H pairs: peak {res[name]["peak_bytes"] / 2**30:7.2f} GiB (model + input {base / 2**30:.2f} GiB), '
              f'first call {res[name]["first_call_ms"]:.0f} ms' + (f', second call {res[name]["second_call_ms"]:.0f} ms' if 'second_call_ms' in res[name] else ''),
              flush=True)
        del model
    a, b = res.pop('pair_relevancy_rel'), res.pop('slow_path_rel')
    res['max_diff_over_max'] = float((a - b).abs().max() / b.abs().max())
    print(f'pair_relevancy vs slow path R_qi: max|diff| / max {res["max_diff_over_max"]:.2e}')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--pairs', type=int, default=8)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'relevancy_probe.json'))
    ap.add_argument('--skip-memory', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('relevancy_probe.py measures on the GPU: none found')
    dev = torch.device('cuda:0')
    result = dict(device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds, kernel=kernel_rows(dev, a.reps, a.rounds))
    if not a.skip_memory:
        result['memory'] = dict(pairs=a.pairs, **memory_peaks(dev, a.pairs))
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(f'wrote {a.out}')


if __name__ == '__main__':
    main()
