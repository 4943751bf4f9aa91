#!/usr/bin/env python3
"""Writes tests/golden/relevancy.npz: what the reference's relevancy visualisation (scripts/visualise_attentions.py,
Generator.generate_ours) computes on a closed-form model, as data only.

Runs on the CPU where the reference checkout exists (the path oracle/pin_against_reference.py uses); exits cleanly elsewhere.
The reference's ``models/vision_transformer.py`` is loaded as in oracle/pin_against_reference.py; the four rule functions
(avg_heads, apply_self_attention_rules, apply_mm_attention_rules, handle_residual) are taken from the script's syntax tree BY NAME
at generation time - the script itself cannot be imported (cv2, matplotlib, torchvision) and none of its text is kept.  What this
file adds is the order in which generate_ours applies them.

    model case   img 64 / patch 8 / dim 384 / 12 heads / depth 2 / c_depth 2 / 4 classes, VisionTransformerCustom(keep_attn=True)
                 with vited_oracle.fill_closed_form_ weights on closed_form_pairs(2, ...); fp32 forward, backward from the one-hot
                 of the arg-max logit, ONE SAMPLE AT A TIME as the script does (avg_heads averages over whatever leads the map):
        logits        float32 [2, 4]
        target        int64 [2]
        enc_cams      float64 [2 blocks, 2 samples, 64, 64]   avg_heads(get_attn(), get_attn_gradients()) in fp64
        dec_self_cams float64 [2, 2, 65, 65]
        dec_cross_cams float64 [2, 2, 65, 64]
        r_qi          float64 [2, 65, 64]                      the propagation in fp64 from those maps (row 0: the cls query)
    synthetic    N1 5, N2 6, 2 + 2 blocks, 2 samples of random non-negative maps; sample 0 has an all-zero encoder map and an
                 all-zero row in its first decoder self map, so handle_residual divides 0 by 0 and rule 10's NaN -> 0 runs:
        syn_enc_cams / syn_dec_self_cams / syn_dec_cross_cams  float64, laid out as above
        syn_r_qi__norm1_self1, syn_r_qi__norm0_self1, syn_r_qi__norm1_self0   float64 [2, 6, 5] for the three settings of
                 (normalize_self_attention, apply_self_in_rule_10)

    python3 tools/make_relevancy_golden.py
"""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'relevancy.npz')
sys.path.insert(0, ROOT)
from oracle import pin_against_reference as pin  # noqa: E402
from oracle import vited_oracle as vo  # noqa: E402

SCRIPT = os.path.join(os.path.dirname(os.path.dirname(pin.REF_FILE)), 'scripts', 'visualise_attentions.py')
RULES = ('avg_heads', 'apply_self_attention_rules', 'apply_mm_attention_rules', 'handle_residual')
SHAPE = vo.ViTEDShape(depth=2, c_depth=2)


def reference_rules():
    """The four rule functions, compiled from their own definitions in the reference's script."""
    tree = ast.parse(open(SCRIPT).read(), SCRIPT)
    picked = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in RULES]
    assert sorted(node.name for node in picked) == sorted(RULES), [node.name for node in picked]
    space = {'torch': torch}
    exec(compile(ast.Module(body=picked, type_ignores=[]), SCRIPT, 'exec'), space)
    return {name: space[name] for name in RULES}


def propagate(rules, enc, dec_self, dec_cross, normalize=True, self_in_rule_10=True):
    """generate_ours' order for one sample: R_ii over the encoder blocks, then per decoder block rules 6 + 7, then rule 10."""
    n1, n2 = dec_cross[0].shape[1], dec_cross[0].shape[0]
    r_ii, r_qq = torch.eye(n1, dtype=torch.float64), torch.eye(n2, dtype=torch.float64)
    r_qi = torch.zeros(n2, n1, dtype=torch.float64)
    for cam in enc:
        r_ii += torch.matmul(cam, r_ii)
    for cam_qq, cam_qi in zip(dec_self, dec_cross):
        add_qq, add_qi = rules['apply_self_attention_rules'](r_qq, r_qi, cam_qq)
        r_qq += add_qq
        r_qi += add_qi
        r_qi += rules['apply_mm_attention_rules'](r_qq, r_ii, cam_qi.clone(), apply_normalization=normalize,
                                                  apply_self_in_rule_10=self_in_rule_10)
    return r_qi


def model_case(rules):
    ref = pin.load_reference_module()
    s = SHAPE
    model = ref.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                        embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads,
                                        mlp_ratio=s.mlp_ratio, qkv_bias=s.qkv_bias, keep_attn=True, arch_version='v1')
    model = vo.fill_closed_form_(model).eval()
    x = vo.closed_form_pairs(2, s)
    logits, target, r_qi = [], [], []
    cams = {'enc': [], 'dec_self': [], 'dec_cross': []}
    for i in range(x.shape[0]):
        out = model(x[i:i + 1])
        index = int(out.detach().argmax(dim=-1))
        one_hot = torch.zeros_like(out)
        one_hot[0, index] = 1
        model.zero_grad()
        (one_hot * out).sum().backward()
        maps = lambda a: rules['avg_heads'](a.get_attn().detach().double(), a.get_attn_gradients().detach().double())
        enc = [maps(blk.attn) for blk in model.blocks]
        dec_self = [maps(blk.attn) for blk in model.cross_blocks]
        dec_cross = [maps(blk.cross_attn) for blk in model.cross_blocks]
        logits.append(out.detach()[0])
        target.append(index)
        cams['enc'].append(torch.stack(enc))
        cams['dec_self'].append(torch.stack(dec_self))
        cams['dec_cross'].append(torch.stack(dec_cross))
        r_qi.append(propagate(rules, enc, dec_self, dec_cross))
    blob = {f'{k}_cams': torch.stack(v, dim=1).numpy() for k, v in cams.items()}       # [block, sample, Nq, Nk]
    blob.update(logits=torch.stack(logits).numpy(), target=np.array(target, dtype=np.int64), r_qi=torch.stack(r_qi).numpy(),
                shape=np.array([s.img_size, s.patch_size, s.in_chans, s.num_classes, s.embed_dim, s.depth, s.c_depth, s.num_heads],
                               dtype=np.int64))
    return blob


def synthetic_case(rules):
    g = torch.Generator().manual_seed(20)
    n1, n2, samples = 5, 6, 2
    rand = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64) * 0.3
    enc, dec_self, dec_cross = rand(2, samples, n1, n1), rand(2, samples, n2, n2), rand(2, samples, n2, n1)
    enc[1, 0] = 0               # an encoder block that contributes nothing
    dec_self[0, 0, 2, :] = 0    # a query whose self-relevancy is still the identity after the first block: 0 / 0 in handle_residual
    blob = dict(syn_enc_cams=enc.numpy(), syn_dec_self_cams=dec_self.numpy(), syn_dec_cross_cams=dec_cross.numpy())
    for normalize, self10 in ((True, True), (False, True), (True, False)):
        r = [propagate(rules, list(enc[:, i]), list(dec_self[:, i]), list(dec_cross[:, i]), normalize, self10) for i in range(samples)]
        blob[f'syn_r_qi__norm{int(normalize)}_self{int(self10)}'] = torch.stack(r).numpy()
    assert np.isfinite(blob['syn_r_qi__norm1_self1']).all()
    return blob


def main():
    if not (os.path.exists(pin.REF_FILE) and os.path.exists(SCRIPT)):
        print('reference not present here - nothing to generate (tests/golden/relevancy.npz stays as committed)')
        return 0
    torch.manual_seed(0)
    torch.set_num_threads(8)
    rules = reference_rules()
    blob = model_case(rules)
    blob.update(synthetic_case(rules))
    blob['torch_version'] = np.array(torch.__version__)
    np.savez_compressed(OUT, **blob)
    print(f'wrote {OUT}: {os.path.getsize(OUT) / 1024:.0f} KB; logits {blob["logits"].tolist()}, target {blob["target"].tolist()}, '
          f'|r_qi| max {np.abs(blob["r_qi"]).max():.3e}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
