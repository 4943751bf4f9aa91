"""CPU: the config surface and the model factory keep the reference's contract."""
import argparse
import os

import pytest
import torch

from oracle import vited_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_A = os.path.join(ROOT, 'configs', 'puzzle', 'div2k_erosion7_4bin_patch8_64.yaml')
CFG_H = os.path.join(ROOT, 'configs', 'hisfrag', 'hisfrag20_patch16_512.yaml')
CFG_T = os.path.join(ROOT, 'configs', 'test', 'test_pjs_hisfrag20_patch32_64.yaml')


def test_yaml_defaults_and_overrides(vited):
    c = vited.config_from_yaml(CFG_A)
    assert (c.MODEL.TYPE, c.MODEL.NUM_CLASSES, c.DATA.IMG_SIZE) == ('pjs', 4, 64)
    assert (c.MODEL.PJS.EMBED_DIM, c.MODEL.PJS.PATCH_SIZE, c.MODEL.PJS.NUM_HEADS, c.MODEL.PJS.DEPTH, c.MODEL.PJS.C_DEPTH) == (384, 8, 12, 8, 8)
    assert c.TRAIN.CLIP_GRAD == 5.0 and c.AMP_ENABLE is True and c.TRAIN.OPTIMIZER.BETAS == (0.9, 0.999)
    assert c.OUTPUT == os.path.join('', 'div2k_erosion7_4bin_patch8_64', 'default')
    h = vited.config_from_yaml(CFG_H)
    assert (h.MODEL.PJS.NUM_HEADS, h.MODEL.PJS.DEPTH, h.MODEL.PJS.C_DEPTH, h.DATA.IMG_SIZE, h.MODEL.NUM_CLASSES) == (6, 12, 12, 512, 1)
    with pytest.raises(AttributeError):
        c.MODEL.NUM_CLASSES = 7           # frozen
    o = vited.config_from_yaml(CFG_A, ['MODEL.PJS.DEPTH', '2', 'TRAIN.BASE_LR', '3e-4', 'DATA.BATCH_SIZE', '1024'])
    assert o.MODEL.PJS.DEPTH == 2 and o.TRAIN.BASE_LR == 3e-4 and o.DATA.BATCH_SIZE == 1024
    with pytest.raises(KeyError):
        vited.config_from_yaml(CFG_A, ['MODEL.NOPE', '1'])
    with pytest.raises(ValueError):
        vited.config_from_yaml(CFG_A, ['MODEL.PJS.DEPTH', 'deep'])


def test_cli_arguments_and_base_includes(vited, tmp_path):
    child = tmp_path / 'child.yaml'
    child.write_text(f'BASE: ["{CFG_A}"]\nMODEL:\n  NAME: child\n  PJS:\n    C_DEPTH: 3\n')
    ns = argparse.Namespace(cfg=str(child), opts=['SEED', '7'], batch_size=32, output='out', tag='t1', disable_amp=True,
                            accumulation_steps=2, resume='', pretrained=None)
    c = vited.get_config(ns)
    assert c.MODEL.PJS.EMBED_DIM == 384 and c.MODEL.PJS.C_DEPTH == 3 and c.MODEL.NAME == 'child'
    assert c.DATA.BATCH_SIZE == 32 and c.DATA.TEST_BATCH_SIZE == 32 and c.AMP_ENABLE is False and c.SEED == 7
    assert c.TRAIN.ACCUMULATION_STEPS == 2 and c.OUTPUT == os.path.join('out', 'child', 't1')
    assert 'EMBED_DIM: 384' in c.dump()


@pytest.mark.parametrize('cfg,params,flops', [(CFG_A, 33_236_356, 4_433_132_544), (CFG_H, 50_392_321, 160_764_807_936)])
def test_build_model_matches_reference_layout(vited, cfg, params, flops):
    m = vited.build_model(vited.config_from_yaml(cfg))
    assert sum(p.numel() for p in m.parameters()) == params      # SURVEY section 8 counts
    assert m.flops() == flops
    pjs = vited.config_from_yaml(cfg).MODEL.PJS
    s = vo.ViTEDShape(img_size=m.img_size, patch_size=m.patch_size, num_classes=m.num_classes, embed_dim=m.embed_dim,
                      depth=m.depth, c_depth=m.c_depth, num_heads=m.num_heads)
    ref = vo.state_dict_spec(s)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(got.keys()) == list(ref.keys()) and got == dict(ref)
    # optimizer grouping rule of misc/optimizer.py:36-46 sees the same names / ranks
    groups = vited.engine.param_groups_no_decay_1d(m)
    assert sum(p.numel() for p in groups[0]['params']) + sum(p.numel() for p in groups[1]['params']) == params
    assert all(p.ndim >= 2 for p in groups[0]['params']) and groups[1]['weight_decay'] == 0.
    assert pjs.QKV_BIAS is True


ENC_BLOCK_KEYS = ('norm1.weight', 'norm1.bias', 'attn.qkv.weight', 'attn.qkv.bias', 'attn.proj.weight',
                  'attn.proj.bias', 'norm2.weight', 'norm2.bias', 'mlp.fc1.weight', 'mlp.fc1.bias',
                  'mlp.fc2.weight', 'mlp.fc2.bias')
DEC_BLOCK_KEYS = ('norm1.weight', 'norm1.bias', 'attn.qkv.weight', 'attn.qkv.bias', 'attn.proj.weight',
                  'attn.proj.bias', 'norm_cross.weight', 'norm_cross.bias', 'norm_context.weight',
                  'norm_context.bias', 'cross_attn.q.weight', 'cross_attn.q.bias', 'cross_attn.kv.weight',
                  'cross_attn.kv.bias', 'cross_attn.proj.weight', 'cross_attn.proj.bias', 'norm2.weight',
                  'norm2.bias', 'mlp.fc1.weight', 'mlp.fc1.bias', 'mlp.fc2.weight', 'mlp.fc2.bias')
ENC_SHARED_KEYS = ('patch_embed.proj.weight', 'patch_embed.proj.bias', 'pos_embed')
DEC_SHARED_KEYS = ('patch_embed.proj.weight', 'patch_embed.proj.bias', 'pos_embed', 'cls_token', 'norm.weight',
                   'norm.bias', 'head.weight', 'head.bias')
ENC_BLOCK_FIELDS = 'g1 b1 wqkv bqkv wproj bproj g2 b2 w1 bb1 w2 bb2'.split()
DEC_BLOCK_FIELDS = 'g1 b1 wqkv bqkv wproj bproj gc bc gx bx wq bq wkv bkv wcp bcp g2 b2 w1 bb1 w2 bb2'.split()
ENC_SHARED_FIELDS = 'pw pb pos'.split()
DEC_SHARED_FIELDS = 'pw pb pos cls gN bN wh bh'.split()


@pytest.mark.parametrize('cfg', [CFG_A, CFG_H, CFG_T])
def test_parameter_bundles_name_the_modules_parameters(vited, cfg):
    """functions.split_params turns the flat parameter lists that the autograd Functions receive into named bundles: every field
    IS the parameter that the paired state_dict key names on the module (no tensor is created or moved: pure Python), the flat
    order is the key order that model.py and the checkpoints use, and flatten_params undoes the split."""
    F_ = vited.functions
    assert F_.ENC_BLOCK_KEYS == ENC_BLOCK_KEYS and F_.DEC_BLOCK_KEYS == DEC_BLOCK_KEYS
    assert F_.ENC_SHARED_KEYS == ENC_SHARED_KEYS and F_.DEC_SHARED_KEYS == DEC_SHARED_KEYS
    m = vited.build_model(vited.config_from_yaml(cfg))

    def named(module, dotted):
        for part in dotted.split('.'):
            module = getattr(module, part)
        return module

    for flat, types, shared_pairs, block_pairs, modules in (
            (m._encoder_params(), (F_.EncShared, F_.EncBlock), zip(ENC_SHARED_FIELDS, ENC_SHARED_KEYS), zip(ENC_BLOCK_FIELDS, ENC_BLOCK_KEYS), m.blocks),
            (m._decoder_params(), (F_.DecShared, F_.DecBlock), zip(DEC_SHARED_FIELDS, DEC_SHARED_KEYS), zip(DEC_BLOCK_FIELDS, DEC_BLOCK_KEYS), m.cross_blocks)):
        shared, blocks = F_.split_params(flat, *types)
        shared_pairs, block_pairs = list(shared_pairs), list(block_pairs)
        assert list(shared._fields) == [f for f, _ in shared_pairs] and len(blocks) == len(modules) > 0
        for field, key in shared_pairs:
            assert getattr(shared, field) is named(m, key), (field, key)
        for block, module in zip(blocks, modules):
            assert list(block._fields) == [f for f, _ in block_pairs]
            for field, key in block_pairs:
                assert getattr(block, field) is named(module, key), (field, key)
        again = F_.flatten_params(shared, blocks)
        assert len(again) == len(flat) and all(a is b for a, b in zip(again, flat))
        with pytest.raises(ValueError):
            F_.split_params(flat[:-1], *types)       # not a whole number of blocks
    assert blocks[-1].wkv is m.cross_blocks[-1].cross_attn.kv.weight and shared.gN is m.norm.weight


def test_checkpoint_roundtrip_with_oracle_weights(vited):
    s = vo.SHAPE_T
    o = vo.fill_closed_form_(vo.OracleViTED(s))
    m = vited.build_model(vited.config_from_yaml(CFG_T))
    missing, unexpected = m.load_state_dict({'model': o.state_dict()}['model'], strict=False)   # misc/utils.py:27
    assert not missing and not unexpected
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), o.state_dict().values()))
    assert m.head.weight.shape == (1, 32) and m.head.bias.shape == (1,)                          # misc/utils.py:110-118


def test_product_has_no_cpu_fallback(vited):
    m = vited.build_model(vited.config_from_yaml(CFG_T))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m(torch.zeros(2, 2, 3, 64, 64))
    with pytest.raises(AssertionError):
        m.to('cpu')(torch.zeros(2, 3, 3, 64, 64))
    m = vited.VisionTransformerCustom(img_size=64, patch_size=8, embed_dim=384, depth=1, c_depth=1, keep_attn=True)   # visualisation slow path: accepted
    assert m.keep_attn and m.blocks[0].attn.keep_attn and m.cross_blocks[0].cross_attn.keep_attn
    with pytest.raises(NotImplementedError):
        vited.VisionTransformerCustom(img_size=64, patch_size=8, embed_dim=1280, num_heads=16)   # beyond the LayerNorm kernels: says so at build time
    with pytest.raises(NotImplementedError):
        cfg = vited.config_from_yaml(CFG_T, ['MODEL.TYPE', 'vit'])
        vited.build_model(cfg)


def test_product_never_imports_the_oracle():
    """The product package must not route through oracle/ (it is test infrastructure)."""
    pkg = os.path.join(ROOT, 'vit-ed_amd')
    for fn in os.listdir(pkg):
        if fn.endswith('.py'):
            src = open(os.path.join(pkg, fn)).read()
            assert 'import oracle' not in src and 'from oracle' not in src, fn
