#!/usr/bin/env python3
"""Write tests/golden/pool_head.npz: the reference's OWN ``VisionTransformerCustom`` with timm's head options - global_pool='avg'
(fc_norm by timm's rule), global_pool='avg' with fc_norm=False, global_pool='token' with fc_norm=True - run in fp64 on closed-form
weights and inputs (tests/pool_cases.fill_closed_form_ / golden_inputs), for the two geometries of pool_cases.GOLDEN_SHAPES.  The
fixture pins WHERE the reference's head normalises and what it pools (``cross_part``'s norm, timm's ``forward_head``) and whether the
state_dict holds ``norm.*`` or ``fc_norm.*``; tests/test_pool_head.py holds the restatement of tests/pool_cases.py to it at rtol 1e-9.

It needs the reference checkout that oracle/pin_against_reference.py loads, and exits cleanly without it.
Arrays only are stored, per variant v in pool_cases.VARIANTS and shape s in (0, 1) under the suffix ``_{v}{s}``: logits, loss, the
parameter names with their shapes, and the norm and the first 16 elements (zero-padded) of every gradient.

    python tools/make_pool_head_golden.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from oracle import pin_against_reference as pin  # noqa: E402
import pool_cases as plc  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden', 'pool_head.npz')


def main():
    if not os.path.exists(pin.REF_FILE):
        print('reference not present here - tests/golden/pool_head.npz stays as committed')
        return 0
    ref = pin.load_reference_module()
    blob = {}
    for variant, (global_pool, fc_norm) in plc.VARIANTS.items():
        for i, s in enumerate(plc.GOLDEN_SHAPES):
            model = ref.VisionTransformerCustom(
                img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes, embed_dim=s.embed_dim,
                depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads, mlp_ratio=s.mlp_ratio, qkv_bias=s.qkv_bias, keep_attn=False,
                arch_version='v1', global_pool=global_pool, fc_norm=fc_norm)
            model = plc.fill_closed_form_(model).double().train()
            names = [n for n, _ in model.named_parameters()]
            fc = plc.use_fc_norm(global_pool, fc_norm)
            assert ('fc_norm.weight' in names) == fc and ('norm.weight' in names) == (not fc), names
            x, y = plc.golden_inputs(s)
            logits = model(x.double())
            loss, grads = plc.loss_and_grads(model, logits, y.double())
            shapes = np.zeros((len(names), 4), dtype=np.int64)          # zero-padded to rank 4
            for r, (_, p) in enumerate(model.named_parameters()):
                shapes[r, :p.dim()] = p.shape
            k = f'_{variant}{i}'
            blob.update({f'logits{k}': logits.detach().numpy(), f'loss{k}': loss.numpy(), f'grad_names{k}': np.array(names),
                         f'shapes{k}': shapes, f'grad_norms{k}': np.array([float(grads[n].norm()) for n in names]),
                         f'grad_slices{k}': np.stack([np.resize(np.append(grads[n].reshape(-1)[:16].numpy(), np.zeros(16)), 16)
                                                      for n in names])})
    np.savez_compressed(OUT, **blob)
    print(f'wrote {OUT}: {len(plc.VARIANTS)} variants x {len(plc.GOLDEN_SHAPES)} shapes, {os.path.getsize(OUT)} bytes')
    return 0


if __name__ == '__main__':
    sys.exit(main())
