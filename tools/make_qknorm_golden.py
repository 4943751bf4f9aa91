#!/usr/bin/env python3
"""Write tests/golden/qk_norm.npz: the reference's OWN ``VisionTransformerCustom(qk_norm=True)`` run in fp64 on closed-form weights
and inputs (tests/qknorm_cases.fill_closed_form_ / golden_inputs), for the two geometries of qknorm_cases.GOLDEN_SHAPES - head_dim
32 and head_dim 64.  The fixture pins WHERE the reference normalises (per head, after the projection's split, before the scores,
in both attentions) and the state_dict names of the eight norm parameters per decoder block and four per encoder block;
tests/test_qknorm.py holds the restatement of tests/qknorm_cases.py to it at rtol 1e-9.

It needs the reference checkout that oracle/pin_against_reference.py loads, and exits cleanly without it.
Arrays only are stored, per shape s in (0, 1): logits, loss, the parameter names with their shapes, and the norm and the first 16
elements (zero-padded) of every gradient.

    python tools/make_qknorm_golden.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from oracle import pin_against_reference as pin  # noqa: E402
import qknorm_cases as qc  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden', 'qk_norm.npz')


def main():
    if not os.path.exists(pin.REF_FILE):
        print('reference not present here - tests/golden/qk_norm.npz stays as committed')
        return 0
    ref = pin.load_reference_module()
    blob = {}
    for i, s in enumerate(qc.GOLDEN_SHAPES):
        model = ref.VisionTransformerCustom(
            img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes, embed_dim=s.embed_dim,
            depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads, mlp_ratio=s.mlp_ratio, qkv_bias=s.qkv_bias, keep_attn=False,
            arch_version='v1', qk_norm=True)
        model = qc.fill_closed_form_(model).double().train()
        normed = [n for n, _ in model.named_parameters() if qc.is_qk_norm_key(n)]
        assert len(normed) == 4 * s.depth + 8 * s.c_depth, normed
        x, y = qc.golden_inputs(s)
        logits = model(x.double())
        loss, grads = qc.loss_and_grads(model, logits, y.double())
        names = [n for n, _ in model.named_parameters()]
        shapes = np.zeros((len(names), 4), dtype=np.int64)          # zero-padded to rank 4
        for r, (_, p) in enumerate(model.named_parameters()):
            shapes[r, :p.dim()] = p.shape
        blob.update({f'logits{i}': logits.detach().numpy(), f'loss{i}': loss.numpy(), f'grad_names{i}': np.array(names),
                     f'shapes{i}': shapes, f'grad_norms{i}': np.array([float(grads[n].norm()) for n in names]),
                     f'grad_slices{i}': np.stack([np.resize(np.append(grads[n].reshape(-1)[:16].numpy(), np.zeros(16)), 16) for n in names])})
    np.savez_compressed(OUT, **blob)
    print(f'wrote {OUT}: {len(qc.GOLDEN_SHAPES)} shapes, {os.path.getsize(OUT)} bytes')
    return 0


if __name__ == '__main__':
    sys.exit(main())
