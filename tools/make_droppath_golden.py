#!/usr/bin/env python3
"""Write tests/golden/droppath.npz: the reference's OWN ``VisionTransformerCustom`` with ``drop_path_rate=0.5`` run in fp64 on
closed-form weights and inputs, every ``DropPath`` instance's forward replaced in this process by multiplication with a preset
per-sample scale vector (tests/droppath_cases.golden_inputs).  The fixture pins WHERE the reference scales - two encoder
branches, three decoder branches - and both decay rules (each module's ``drop_prob``); tests/test_droppath.py holds the
composition of tests/droppath_cases.py to it at rtol 1e-9.

It needs the reference checkout that oracle/pin_against_reference.py loads, and exits cleanly without it.
Arrays only are stored: scales, drop probabilities, logits, loss, and the norm and the first 16 elements (zero-padded) of every gradient.

    python tools/make_droppath_golden.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from oracle import pin_against_reference as pin  # noqa: E402
from oracle import vited_oracle as vo  # noqa: E402
import droppath_cases as dc  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden', 'droppath.npz')


def main():
    if not os.path.exists(pin.REF_FILE):
        print('reference not present here - tests/golden/droppath.npz stays as committed')
        return 0
    ref = pin.load_reference_module()
    drop_path_type = sys.modules['timm.layers'].DropPath
    s = dc.GOLDEN_SHAPE
    model = ref.VisionTransformerCustom(
        img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes, embed_dim=s.embed_dim,
        depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads, mlp_ratio=s.mlp_ratio, qkv_bias=s.qkv_bias, keep_attn=False,
        arch_version='v1', drop_path_rate=dc.GOLDEN_RATE)
    model = vo.fill_closed_form_(model).double().train()
    x, y, enc, dec = dc.golden_inputs()
    probs = {'enc': np.zeros((s.depth, 2)), 'dec': np.zeros((s.c_depth, 3))}
    places = [('enc', model.blocks, enc, ('drop_path1', 'drop_path2')),
              ('dec', model.cross_blocks, dec, ('drop_path1', 'drop_path_cross', 'drop_path2'))]
    patched = 0
    for half, blocks, scales, names in places:
        for i, blk in enumerate(blocks):
            for j, name in enumerate(names):
                mod = getattr(blk, name)
                if not isinstance(mod, drop_path_type):       # p == 0: the reference builds nn.Identity there
                    assert torch.all(scales[i, j] == 1), (half, i, name)
                    continue
                probs[half][i, j] = mod.drop_prob
                mod.forward = (lambda t, sc=scales[i, j].double(): t * sc.view(-1, 1, 1))
                patched += 1
    assert patched == sum(isinstance(m, drop_path_type) for m in model.modules()), 'a DropPath instance was left live'
    logits = model(x.double())
    loss, grads = dc.loss_and_grads(model, logits, y.double())
    names = [n for n, _ in model.named_parameters()]
    blob = dict(enc=enc.numpy(), dec=dec.numpy(), drop_prob_enc=probs['enc'], drop_prob_dec=probs['dec'],
                logits=logits.detach().numpy(), loss=loss.numpy(), grad_names=np.array(names),
                grad_norms=np.array([float(grads[n].norm()) for n in names]),
                grad_slices=np.stack([np.resize(np.append(grads[n].reshape(-1)[:16].numpy(), np.zeros(16)), 16) for n in names]))
    np.savez_compressed(OUT, **blob)
    print(f'wrote {OUT}: {patched} DropPath instances forced, {os.path.getsize(OUT)} bytes')
    return 0


if __name__ == '__main__':
    sys.exit(main())
