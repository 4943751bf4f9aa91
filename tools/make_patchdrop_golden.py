#!/usr/bin/env python3
"""Write tests/golden/patch_drop.npz: the reference's OWN ``VisionTransformerCustom`` run in fp64 on closed-form weights and inputs
with ``model.patch_drop`` replaced in this process by tests/patchdrop_cases.ForcedPatchDrop - timm's PatchDropout with its random
draw replaced by two queued index sets, consumed by the two ``patch_drop`` calls of one forward (image 1, then image 2).  The model
is built with rate 0 (the timm stand-in that oracle/pin_against_reference.py loads restates no PatchDropout), so the fixture pins
WHERE the reference calls ``patch_drop`` - after the position embedding, in front of the blocks, the prefix slot on patch 0 of the
image-1 stream and on the cls token of the image-2 stream; tests/test_patchdrop.py holds the composition of tests/patchdrop_cases.py
to it at rtol 1e-9.

It needs the reference checkout that oracle/pin_against_reference.py loads, and exits cleanly without it.
Arrays only are stored: keep indices, logits, loss, and the norm and the first 16 elements (zero-padded) of every gradient.

    python tools/make_patchdrop_golden.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from oracle import pin_against_reference as pin  # noqa: E402
from oracle import vited_oracle as vo  # noqa: E402
import patchdrop_cases as pc  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden', 'patch_drop.npz')


def main():
    if not os.path.exists(pin.REF_FILE):
        print('reference not present here - tests/golden/patch_drop.npz stays as committed')
        return 0
    ref = pin.load_reference_module()
    s = pc.GOLDEN_SHAPE
    model = ref.VisionTransformerCustom(
        img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes, embed_dim=s.embed_dim,
        depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads, mlp_ratio=s.mlp_ratio, qkv_bias=s.qkv_bias, keep_attn=False,
        arch_version='v1', patch_drop_rate=0.)
    model = vo.fill_closed_form_(model).double().train()
    x, y, keep1, keep2 = pc.golden_inputs()
    model.patch_drop = pc.ForcedPatchDrop(keep1, keep2)
    logits = model(x.double())
    assert not model.patch_drop.queue and model.patch_drop.seen == [s.n1, s.n1 + 1], model.patch_drop.seen
    loss, grads = pc.loss_and_grads(model, logits, y.double())
    names = [n for n, _ in model.named_parameters()]
    blob = dict(keep1=keep1.numpy(), keep2=keep2.numpy(), rate=np.array(pc.GOLDEN_RATE), logits=logits.detach().numpy(),
                loss=loss.numpy(), grad_names=np.array(names), grad_norms=np.array([float(grads[n].norm()) for n in names]),
                grad_slices=np.stack([np.resize(np.append(grads[n].reshape(-1)[:16].numpy(), np.zeros(16)), 16) for n in names]))
    np.savez_compressed(OUT, **blob)
    print(f'wrote {OUT}: patch_drop called on {model.patch_drop.seen} tokens, {os.path.getsize(OUT)} bytes')
    return 0


if __name__ == '__main__':
    sys.exit(main())
