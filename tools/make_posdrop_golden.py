#!/usr/bin/env python3
"""Write tests/golden/pos_drop.npz: the reference's OWN ``VisionTransformerCustom(pos_drop_rate=0.25)`` run in fp64 on closed-form
weights and inputs, ``model.pos_drop.forward`` replaced in this process by tests/posdrop_cases.ForcedPosDrop - nn.Dropout with its
random draw replaced by two queued multipliers mask * scale, consumed by the two ``pos_drop`` calls of one forward (image 1 in
``_pos_embed_no_cls``, then image 2 in timm's ``_pos_embed``).  The masks are ``ops.token_dropout_mask`` at the fixed seeds of
posdrop_cases.GOLDEN_SEEDS and are stored in the file (bit-packed), so the fixture pins WHERE the reference drops - behind the
position embedding of either stream, the cls row included, in front of the blocks - and the mask rule itself;
tests/test_posdrop.py holds the composition of tests/posdrop_cases.py to it at rtol 1e-9.

Two geometries: 64-pixel images with 1 + 1 and with 2 + 3 blocks.  It needs the reference checkout that
oracle/pin_against_reference.py loads, and exits cleanly without it.  Arrays only are stored: seeds, packed masks, logits, loss, and
the norm and the first 16 elements (zero-padded) of every gradient.

    python tools/make_posdrop_golden.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
from oracle import pin_against_reference as pin  # noqa: E402
from oracle import vited_oracle as vo  # noqa: E402
import posdrop_cases as pd  # noqa: E402
import vited_amd  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden', 'pos_drop.npz')


def main():
    if not os.path.exists(pin.REF_FILE):
        print('reference not present here - tests/golden/pos_drop.npz stays as committed')
        return 0
    ref = pin.load_reference_module()
    ops = vited_amd.ops
    blob = dict(rate=np.array(pd.GOLDEN_RATE), thr=np.array(ops.dropout_threshold(pd.GOLDEN_RATE)[0], dtype=np.int64),
                scale=np.array(ops.dropout_threshold(pd.GOLDEN_RATE)[1], dtype=np.float64))
    for name, s in pd.GOLDEN_SHAPES.items():
        model = ref.VisionTransformerCustom(
            img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes, embed_dim=s.embed_dim,
            depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads, mlp_ratio=s.mlp_ratio, qkv_bias=s.qkv_bias, keep_attn=False,
            arch_version='v1', pos_drop_rate=pd.GOLDEN_RATE)
        assert model.pos_drop.p == pd.GOLDEN_RATE
        model = vo.fill_closed_form_(model).double().train()
        x, y = pd.golden_inputs(name)
        seeds = pd.GOLDEN_SEEDS[name]
        mask1, mask2, scale = pd.masks_of(ops, seeds, pd.GOLDEN_RATE, pd.GOLDEN_BATCH, pd.GOLDEN_BATCH, s)
        model.pos_drop = pd.ForcedPosDrop(mask1.double() * scale, mask2.double() * scale)
        logits = model(x.double())
        want = [(pd.GOLDEN_BATCH, s.n1, s.embed_dim), (pd.GOLDEN_BATCH, s.n2, s.embed_dim)]
        assert not model.pos_drop.queue and model.pos_drop.seen == want, model.pos_drop.seen
        loss, grads = pd.loss_and_grads(model, logits, y.double())
        names = [n for n, _ in model.named_parameters()]
        blob.update({f'{name}.seeds': np.array(seeds, dtype=np.int64), f'{name}.mask1': np.packbits(mask1.numpy()),
                     f'{name}.mask2': np.packbits(mask2.numpy()), f'{name}.logits': logits.detach().numpy(), f'{name}.loss': loss.numpy(),
                     f'{name}.grad_names': np.array(names), f'{name}.grad_norms': np.array([float(grads[n].norm()) for n in names]),
                     f'{name}.grad_slices': np.stack([np.resize(np.append(grads[n].reshape(-1)[:16].numpy(), np.zeros(16)), 16)
                                                      for n in names])})
        print(f'{name}: pos_drop called on {model.pos_drop.seen}, kept {float(mask1.double().mean()):.4f} / {float(mask2.double().mean()):.4f}')
    np.savez_compressed(OUT, **blob)
    print(f'wrote {OUT}: {os.path.getsize(OUT)} bytes')
    return 0


if __name__ == '__main__':
    sys.exit(main())
