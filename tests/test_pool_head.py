"""The pooled head (global_pool='avg', fc_norm), the parts that need no GPU: the pin of the restatement in tests/pool_cases.py against
what the reference's own class computed (tests/golden/pool_head.npz), the constructor and factory surface, the state_dict layout, the
parameter groups, the C entry points' argument checks (they return before anything is launched), and the kernels' index and
reduction arithmetic (csrc/pool_head.h) run on the host, as a stand-alone program, under the address and undefined-behaviour
sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import pool_cases as plc
from oracle import vited_oracle as vo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, 'golden', 'pool_head.npz')
VARIANTS = list(plc.VARIANTS)


def _model(vited, s, **kw):
    return vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                         embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads,
                                         mlp_ratio=s.mlp_ratio, qkv_bias=s.qkv_bias, **kw)


def _options(variant):
    global_pool, fc_norm = plc.VARIANTS[variant]
    return dict(global_pool=global_pool, fc_norm=fc_norm)


@pytest.mark.parametrize('which', [0, 1])
@pytest.mark.parametrize('variant', VARIANTS)
def test_restatement_matches_the_reference_class(variant, which):
    """fp64, closed-form weights: logits, loss and every parameter gradient of the restatement equal what the reference's
    VisionTransformerCustom gave with these head options."""
    fx = np.load(GOLDEN)
    k = f'_{variant}{which}'
    s = plc.GOLDEN_SHAPES[which]
    m = plc.fill_closed_form_(plc.PoolViTED(s, **_options(variant))).double()
    x, y = plc.golden_inputs(s)
    logits = m(x.double())
    assert torch.equal(logits, plc.forward(m, x.double()))              # the module's methods and the functional form are one thing
    loss, grads = plc.loss_and_grads(m, logits, y.double())
    np.testing.assert_allclose(logits.detach().numpy(), fx[f'logits{k}'], rtol=1e-9, atol=0)
    np.testing.assert_allclose(loss.numpy(), fx[f'loss{k}'], rtol=1e-9)
    names = [str(n) for n in fx[f'grad_names{k}']]
    assert names == [n for n, _ in m.named_parameters()]
    want_norms = dict(zip(names, fx[f'grad_norms{k}']))
    for n, want in zip(names, fx[f'grad_slices{k}']):
        got = grads[n].reshape(-1)[:16].numpy()
        np.testing.assert_allclose(float(grads[n].norm()), want_norms[n], rtol=1e-9, err_msg=n)
        np.testing.assert_allclose(got, want[:got.size], rtol=1e-9, atol=1e-9 * want_norms[n], err_msg=n)
    # the options matter: the default head on the same weights gives other logits
    plain = vo.OracleViTED(s).double()
    plain.load_state_dict({name.replace('fc_norm.', 'norm.'): v for name, v in m.state_dict().items()})
    if variant == 'token_fc':       # the same arithmetic as the default under the other keys
        np.testing.assert_allclose(plain(x.double()).detach().numpy(), fx[f'logits{k}'], rtol=1e-9)
    else:
        assert not np.allclose(plain(x.double()).detach().numpy(), fx[f'logits{k}'], rtol=1e-3)


@pytest.mark.parametrize('which', [0, 1])
@pytest.mark.parametrize('variant', VARIANTS)
def test_state_dict_is_the_reference_layout(vited, variant, which):
    fx = np.load(GOLDEN)
    k = f'_{variant}{which}'
    s = plc.GOLDEN_SHAPES[which]
    model = _model(vited, s, **_options(variant))
    names = [str(n) for n in fx[f'grad_names{k}']]
    assert [n for n, _ in model.named_parameters()] == names
    assert list(model.state_dict()) == names
    for (n, p), shape in zip(model.named_parameters(), fx[f'shapes{k}']):
        assert tuple(p.shape) == tuple(int(v) for v in shape[:p.dim()]) and not shape[p.dim():].any(), n
    fc = plc.use_fc_norm(*plc.VARIANTS[variant])
    assert model.use_fc_norm is fc and model.global_pool == plc.VARIANTS[variant][0]
    assert ('fc_norm.weight' in names and 'fc_norm.bias' in names) == fc
    assert ('norm.weight' in names or 'norm.bias' in names) == (not fc)
    assert hasattr(model, 'fc_norm') == fc and hasattr(model, 'norm') == (not fc)
    sd = model.state_dict()
    key = 'fc_norm' if fc else 'norm'
    assert bool((sd[key + '.weight'] == 1.).all()) and bool((sd[key + '.bias'] == 0.).all())     # LayerNorm's own init
    # every parameter is in exactly one bundle of the Functions, under the reference's name
    F_ = vited.functions
    shared, _ = F_.split_params(model._decoder_params(), F_.DecSharedFc if fc else F_.DecShared, F_.DecBlock)
    assert shared.gN is getattr(model, key).weight and shared.bN is getattr(model, key).bias and shared.wh is model.head.weight
    ids = {id(p) for p in model._encoder_params()} | {id(p) for p in model._decoder_params()}
    assert ids == {id(p) for p in model.parameters()}
    rt = model.runtime(torch.bfloat16)
    assert rt.pool_avg is (model.global_pool == 'avg') and rt.fc_norm is fc and rt.dec_shared.__name__ == ('DecSharedFc' if fc else 'DecShared')
    assert rt.cls_tail is (model.global_pool != 'avg')          # every row of the last block reaches the loss under 'avg'


def test_default_has_exactly_the_oracle_keys(vited):
    s = plc.GOLDEN_SHAPES[0]
    spec = vo.state_dict_spec(s)
    for m in (_model(vited, s), _model(vited, s, global_pool='token'), _model(vited, s, global_pool='token', fc_norm=False),
              _model(vited, s, fc_norm=None)):
        assert m.global_pool == 'token' and m.use_fc_norm is False
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == list(spec.items())
        assert not hasattr(m, 'fc_norm')
        rt = m.runtime(torch.bfloat16)
        assert rt.pool_avg is False and rt.fc_norm is False and rt.dec_shared.__name__ == 'DecShared'
    F_ = vited.functions
    assert F_.DEC_SHARED_FC_KEYS == tuple(k.replace('norm.', 'fc_norm.') if k.startswith('norm.') else k for k in F_.DEC_SHARED_KEYS)
    assert F_.DecSharedFc._fields == F_.DecShared._fields


@pytest.mark.parametrize('variant', VARIANTS)
def test_reference_style_checkpoint_loads(vited, variant):
    s = plc.GOLDEN_SHAPES[1]
    ckpt = plc.fill_closed_form_(plc.PoolViTED(s, **_options(variant))).state_dict()
    model = _model(vited, s, **_options(variant))
    result = model.load_state_dict(ckpt, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    key = 'fc_norm' if model.use_fc_norm else 'norm'
    assert torch.equal(getattr(model, key).weight, ckpt[key + '.weight']) and float(getattr(model, key).weight.detach().std()) > 0.01
    other = _model(vited, s, global_pool='token', fc_norm=not model.use_fc_norm)
    with pytest.raises(RuntimeError, match=r'fc_norm\.weight'):
        other.load_state_dict(ckpt, strict=True)           # the other layout says what it cannot hold / misses


def test_factory_forwards_the_options(vited):
    cfg = vited.config_from_yaml(os.path.join(ROOT, 'configs', 'puzzle', 'div2k_erosion7_4bin_patch8_64.yaml'), ['MODEL.PJS.DEPTH', '1',
                                                                                                                   'MODEL.PJS.C_DEPTH', '1'])
    default = vited.build_model(cfg)
    assert default.global_pool == 'token' and default.use_fc_norm is False and hasattr(default, 'norm')
    avg = vited.build_model(cfg, global_pool='avg')
    assert avg.global_pool == 'avg' and avg.use_fc_norm is True and tuple(avg.fc_norm.weight.shape) == (cfg.MODEL.PJS.EMBED_DIM,)
    nofc = vited.build_model(cfg, global_pool='avg', fc_norm=False)
    assert nofc.global_pool == 'avg' and nofc.use_fc_norm is False and hasattr(nofc, 'norm') and not hasattr(nofc, 'fc_norm')
    tok = vited.build_model(cfg, fc_norm=True)
    assert tok.global_pool == 'token' and tok.use_fc_norm is True
    assert avg.runtime(torch.bfloat16).pool_avg is True and default.runtime(torch.bfloat16).pool_avg is False
    with pytest.raises(NotImplementedError, match='global_pool'):
        vited.build_model(cfg, global_pool='')


@pytest.mark.parametrize('variant', VARIANTS)
def test_head_norm_is_in_the_no_decay_group_and_the_decoder_only_bucket(vited, variant):
    model = _model(vited, plc.GOLDEN_SHAPES[0], **_options(variant))
    groups = vited.engine.param_groups_no_decay_1d(model)
    no_decay = [g for g in groups if g.get('weight_decay') == 0.]
    assert len(no_decay) == 1
    held = {id(p) for p in no_decay[0]['params']}
    decayed = {id(p) for g in groups if g.get('weight_decay') != 0. for p in g['params']}
    key = 'fc_norm' if model.use_fc_norm else 'norm'
    norm = [getattr(model, key).weight, getattr(model, key).bias]
    assert all(id(p) in held and id(p) not in decayed for p in norm)
    dec_only = {id(p) for p in vited.engine._decoder_only_parameters(model)}
    assert all(id(p) in dec_only for p in norm) and id(model.head.weight) in dec_only and id(model.pos_embed) not in dec_only


def test_other_pooling_modes_are_refused_by_name(vited):
    s = plc.GOLDEN_SHAPES[0]
    for bad in ('', 'max', 'avgmax', 'map', None):
        with pytest.raises(NotImplementedError, match='global_pool'):
            _model(vited, s, global_pool=bad)
    with pytest.raises(NotImplementedError, match='global_pool'):
        vited.functions.Runtime(img_size=16, patch_size=8, in_chans=3, num_classes=4, embed_dim=64, depth=1, c_depth=1, num_heads=2,
                                global_pool='')
    for name, value in (('no_embed_class', True), ('pre_norm', True)):
        with pytest.raises(NotImplementedError, match=name):
            _model(vited, s, global_pool='avg', **{name: value})


def test_the_pinned_options_still_raise_beside_avg(vited):
    s = plc.GOLDEN_SHAPES[0]
    for name, value in (('init_values', 1e-5), ('drop_rate', 0.1), ('attn_drop_rate', 0.1), ('proj_drop_rate', 0.1)):
        with pytest.raises(NotImplementedError, match=name):
            _model(vited, s, global_pool='avg', **{name: value})
        with pytest.raises(NotImplementedError, match=name):
            _model(vited, s, global_pool='avg', fc_norm=False, **{name: value})


def test_relevancy_maps_are_refused_under_avg(vited):
    model = _model(vited, plc.GOLDEN_SHAPES[0], global_pool='avg')
    model.keep_cam = True
    with pytest.raises(NotImplementedError, match='global_pool'):
        model.runtime(torch.float32)
    model.keep_cam = False
    model.runtime(torch.float32)
    token = _model(vited, plc.GOLDEN_SHAPES[0], fc_norm=True)
    token.keep_cam = True
    assert token.runtime(torch.float32).keep_cam is True            # the cls row's maps exist whenever the cls row is pooled


def test_wrappers_refuse_wrong_tensors_before_the_launch(vited):
    ops = vited.ops
    x = torch.zeros(2, 5, 32)
    with pytest.raises(RuntimeError, match='CPU tensor'):
        ops.token_pool_fwd(x)
    with pytest.raises(RuntimeError, match='CPU tensor'):
        ops.token_pool_bwd(torch.zeros(2, 32), 5)
    assert ops.token_pool_fwd.__module__.endswith('ops_poolhead') and ops.token_pool_bwd.__module__.endswith('ops_poolhead')


def test_entry_points_check_their_arguments(vited):
    """dim outside the LayerNorm kernels' range is unsupported; a null operand, tokens <= first, strides that let rows or items overlap
    and misaligned pointers or strides are bad arguments; a short or missing workspace is the workspace error.  All before any launch."""
    lib = vited._lib.load()
    OK, BAD, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
    buf = (ctypes.c_float * 65536)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    F32, BF16, F16 = vited._lib.F32, vited._lib.BF16, vited._lib.F16
    items, tokens, dim = 2, 5, 32

    need = lib.vited_token_pool_workspace_bytes(items, tokens, 1, dim)
    assert need == items * 1 * 2 * dim * 4
    assert lib.vited_token_pool_workspace_bytes(72, 1025, 1, 384) == 72 * 16 * 2 * 384 * 4        # 1,024 pooled tokens: 16 chunks of 64
    assert lib.vited_token_pool_workspace_bytes(1024, 65, 1, 384) == 1024 * 1 * 2 * 384 * 4
    assert lib.vited_token_pool_workspace_bytes(2, 66, 1, 32) == 2 * 2 * 2 * 32 * 4               # 65 pooled tokens: 64 + 1
    assert lib.vited_token_pool_workspace_bytes(2, 1, 1, 32) == 0 and lib.vited_token_pool_workspace_bytes(2, 5, 1, 30) == 0

    def fwd(x=p, x_is=tokens * dim, x_ts=dim, gamma=None, beta=None, pooled=p, pooled_ld=dim, mean=None, rstd=None, items=items, tokens=tokens,
            first=1, dim=dim, ws=p, ws_bytes=need):
        return lib.vited_token_pool_fwd(x, x_is, x_ts, gamma, beta, 1e-6, pooled, pooled_ld, mean, rstd, items, tokens, first, dim, ws, ws_bytes, None)

    assert fwd(x=None) == BAD and fwd(pooled=None) == BAD
    assert fwd(gamma=p) == BAD and fwd(beta=p) == BAD                       # they go together
    assert fwd(mean=p, rstd=p) == BAD and fwd(gamma=p, beta=p, mean=p) == BAD     # statistics only with a LayerNorm, both or neither
    assert fwd(first=tokens) == BAD and fwd(first=tokens + 1) == BAD and fwd(first=-1) == BAD and fwd(items=0) == BAD
    assert fwd(dim=30) == UNSUPPORTED and fwd(dim=1028, x_ts=1028, x_is=5 * 1028, pooled_ld=1028) == UNSUPPORTED
    assert fwd(x_ts=dim - 4) == BAD and fwd(x_is=tokens * dim - 4) == BAD   # rows / items would overlap
    assert fwd(x=p + 4) == BAD and fwd(x_ts=dim + 2, x_is=tokens * (dim + 2)) == BAD and fwd(pooled=p + 8) == BAD and fwd(pooled_ld=dim - 4) == BAD
    assert fwd(gamma=p + 4, beta=p) == BAD
    big = dict(tokens=130, x_is=130 * dim)                                  # 129 pooled tokens: three chunks, the workspace is needed
    need_big = lib.vited_token_pool_workspace_bytes(items, 130, 1, dim)
    assert fwd(ws=None, ws_bytes=need_big, **big) == WORKSPACE and fwd(ws_bytes=need_big - 4, **big) == WORKSPACE
    assert fwd(ws=p + 4, ws_bytes=need_big, **big) == WORKSPACE

    def bwd(g=p, g_ld=dim, x=p, x_is=tokens * dim, x_ts=dim, gamma=p, mean=p, rstd=p, dx=p, dx_is=tokens * dim, dx_ts=dim, lp=None, lp_dtype=BF16,
            lp_is=tokens * dim, lp_ts=dim, lp_scale=None, dgamma=p, dbeta=p, tokens=tokens, first=1, dim=dim, ws=p, ws_bytes=need):
        return lib.vited_token_pool_bwd(g, g_ld, x, x_is, x_ts, gamma, mean, rstd, dx, dx_is, dx_ts, lp, lp_dtype, lp_is, lp_ts, lp_scale, dgamma,
                                        dbeta, 0, items, tokens, first, dim, ws, ws_bytes, None)

    assert bwd(g=None) == BAD and bwd(dx=None) == BAD and bwd(lp_scale=p) == BAD            # a scale without the copy it scales
    assert bwd(x=None) == BAD and bwd(mean=None) == BAD and bwd(rstd=None) == BAD and bwd(dgamma=None) == BAD and bwd(dbeta=None) == BAD
    assert bwd(first=tokens) == BAD and bwd(dim=36, g_ld=36) == BAD                         # (36-wide rows in 32-wide strides overlap)
    assert bwd(dim=30) == UNSUPPORTED and bwd(lp=p, lp_dtype=F16) == UNSUPPORTED
    assert bwd(dx_ts=dim - 4) == BAD and bwd(dx_is=tokens * dim - 4) == BAD and bwd(x_ts=dim - 4) == BAD
    assert bwd(lp=p, lp_ts=dim - 4) == BAD and bwd(lp=p + 4) == BAD and bwd(lp=p + 8, lp_dtype=F32) == BAD
    assert bwd(dx=p + 4) == BAD and bwd(g=p + 8) == BAD and bwd(g_ld=dim - 4) == BAD and bwd(gamma=p + 4) == BAD
    assert bwd(ws=None) == WORKSPACE and bwd(ws_bytes=need - 4) == WORKSPACE
    assert OK == 0


def _clangxx():
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    for cand in (shutil.which('clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++')):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_host_check_runs_clean_under_the_sanitizers(tmp_path):
    """tools/poolhead_host_check.cpp: the text of csrc/pool_head.h driven lane by lane in the kernels' order over exactly-sized heap
    blocks against a long-double evaluation - a stand-alone program with its own main, built with -fsanitize=address,undefined."""
    cxx = _clangxx()
    assert cxx is not None, 'no clang++ beside hipcc: the HIP toolchain that builds the library ships one'
    exe = str(tmp_path / 'poolhead_host_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                    os.path.join(ROOT, 'vit-ed_amd', 'csrc'), os.path.join(ROOT, 'tools', 'poolhead_host_check.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'poolhead_host_check ok' in run.stdout and not run.stderr.strip(), run.stdout + run.stderr
