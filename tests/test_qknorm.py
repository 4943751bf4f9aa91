"""q/k-norm, the parts that need no GPU: the pin of the restatement in tests/qknorm_cases.py against what the reference's own classes
computed (tests/golden/qk_norm.npz), the constructor and factory surface, the state_dict layout, the parameter groups, and the C
entry points' argument checks (they return before anything is launched).

One property of the function shapes several checks here and in tests/test_gpu_qknorm.py: the gradient of every ``k_norm.bias`` is
ZERO in exact arithmetic.  The bias adds the same vector b to every key of a head, q . (k + b) = q . k + q . b shifts all scores of
a query by the same amount, and the softmax does not see such a shift.  What any implementation returns there is rounding noise
(the fp64 reference: 1e-19 against 1e-2 for the sibling weight), so a relative error against the reference's value has no meaning;
those tensors are held to ``tolerance x the norm of the same module's weight gradient`` instead - the same sum over rows and heads
with factors of order one."""
import ctypes
import os

import numpy as np
import pytest
import torch

import qknorm_cases as qc
from oracle import vited_oracle as vo

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'qk_norm.npz')


def _model(vited, s, **kw):
    return vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                         embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads,
                                         mlp_ratio=s.mlp_ratio, qkv_bias=s.qkv_bias, **kw)


@pytest.mark.parametrize('which', [0, 1])
def test_restatement_matches_the_reference_classes(which):
    """fp64, closed-form weights (norm weights and biases that vary with the index): logits, loss and every parameter gradient of the
    restatement equal what the reference's VisionTransformerCustom(qk_norm=True) gave, head_dim 32 and head_dim 64."""
    fx = np.load(GOLDEN)
    s = qc.GOLDEN_SHAPES[which]
    m = qc.fill_closed_form_(qc.QKNormViTED(s)).double()
    x, y = qc.golden_inputs(s)
    logits = m(x.double())
    loss, grads = qc.loss_and_grads(m, logits, y.double())
    np.testing.assert_allclose(logits.detach().numpy(), fx[f'logits{which}'], rtol=1e-9, atol=0)
    np.testing.assert_allclose(loss.numpy(), fx[f'loss{which}'], rtol=1e-9)
    names = [str(n) for n in fx[f'grad_names{which}']]
    assert names == [n for n, _ in m.named_parameters()]
    want_norms = dict(zip(names, fx[f'grad_norms{which}']))
    zero = [n for n in names if n.endswith('k_norm.bias')]
    assert len(zero) == s.depth + 2 * s.c_depth
    for n, want in zip(names, fx[f'grad_slices{which}']):
        got, norm = grads[n].reshape(-1)[:16].numpy(), float(grads[n].norm())
        if n in zero:           # exactly zero in exact arithmetic (module docstring): rounding noise on both sides
            scale = want_norms[n.replace('.bias', '.weight')]
            assert norm <= 1e-9 * scale and want_norms[n] <= 1e-9 * scale, (n, norm, want_norms[n], scale)
            continue
        np.testing.assert_allclose(norm, want_norms[n], rtol=1e-9, err_msg=n)
        np.testing.assert_allclose(got, want[:got.size], rtol=1e-9, atol=1e-9 * want_norms[n], err_msg=n)
    # the norms matter: the oracle without them, on the same remaining weights, gives other logits
    plain = vo.OracleViTED(s).double()
    plain.load_state_dict({k: v for k, v in m.state_dict().items() if not qc.is_qk_norm_key(k)})
    assert not np.allclose(plain(x.double()).detach().numpy(), fx[f'logits{which}'], rtol=1e-3)


@pytest.mark.parametrize('which', [0, 1])
def test_state_dict_is_the_reference_layout(vited, which):
    fx = np.load(GOLDEN)
    s = qc.GOLDEN_SHAPES[which]
    model = _model(vited, s, qk_norm=True)
    names = [str(n) for n in fx[f'grad_names{which}']]
    assert [n for n, _ in model.named_parameters()] == names
    for (n, p), shape in zip(model.named_parameters(), fx[f'shapes{which}']):
        assert tuple(p.shape) == tuple(int(v) for v in shape[:p.dim()]) and not shape[p.dim():].any(), n
    normed = [n for n in names if qc.is_qk_norm_key(n)]
    assert len(normed) == 4 * s.depth + 8 * s.c_depth
    sd = model.state_dict()
    for n in normed:
        assert tuple(sd[n].shape) == (s.head_dim,)
        assert bool((sd[n] == (1. if n.endswith('weight') else 0.)).all()), n           # LayerNorm's own init, untouched by the timm init
    assert 'blocks.0.attn.q_norm.weight' in sd and f'cross_blocks.{s.c_depth - 1}.cross_attn.k_norm.bias' in sd


def test_off_has_exactly_todays_keys(vited):
    s = qc.GOLDEN_SHAPES[0]
    off, default = _model(vited, s, qk_norm=False), _model(vited, s)
    spec = vo.state_dict_spec(s)
    for m in (off, default):
        assert m.qk_norm is False
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == list(spec.items())
        assert not any('q_norm' in n or 'k_norm' in n for n, _ in m.named_modules())
    F_ = vited.functions
    assert len(off._encoder_params()) == len(F_.ENC_SHARED_KEYS) + s.depth * len(F_.ENC_BLOCK_KEYS)
    assert len(off._decoder_params()) == len(F_.DEC_SHARED_KEYS) + s.c_depth * len(F_.DEC_BLOCK_KEYS)
    on = _model(vited, s, qk_norm=True)
    assert len(on._encoder_params()) == len(F_.ENC_SHARED_KEYS) + s.depth * (len(F_.ENC_BLOCK_KEYS) + 4)
    assert len(on._decoder_params()) == len(F_.DEC_SHARED_KEYS) + s.c_depth * (len(F_.DEC_BLOCK_KEYS) + 8)
    assert set(on.state_dict()) - set(off.state_dict()) == {n for n in on.state_dict() if qc.is_qk_norm_key(n)}
    # the bundles of the Functions: every parameter of the model is in exactly one of them, under the reference's name
    shared, blocks = F_.split_params(on._decoder_params(), F_.DecShared, F_.DecBlockQK)
    assert blocks[1].gckn is on.cross_blocks[1].cross_attn.k_norm.weight and blocks[0].bqn is on.cross_blocks[0].attn.q_norm.bias
    _, eblocks = F_.split_params(on._encoder_params(), F_.EncShared, F_.EncBlockQK)
    assert eblocks[1].gkn is on.blocks[1].attn.k_norm.weight
    ids = {id(p) for p in on._encoder_params()} | {id(p) for p in on._decoder_params()}
    assert ids == {id(p) for p in on.parameters()}


def test_reference_style_checkpoint_loads(vited):
    s = qc.GOLDEN_SHAPES[1]
    ckpt = qc.fill_closed_form_(qc.QKNormViTED(s)).state_dict()
    model = _model(vited, s, qk_norm=True)
    result = model.load_state_dict(ckpt, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    assert torch.equal(model.cross_blocks[1].cross_attn.q_norm.weight, ckpt['cross_blocks.1.cross_attn.q_norm.weight'])
    assert float(model.blocks[0].attn.k_norm.weight.detach().std()) > 0.01
    plain = _model(vited, s)
    with pytest.raises(RuntimeError, match='q_norm'):
        plain.load_state_dict(ckpt, strict=True)           # the model without the option still says what it cannot hold


def test_factory_switches_it_on_only_on_request(vited):
    root = os.path.dirname(HERE)
    cfg = vited.config_from_yaml(os.path.join(root, 'configs', 'puzzle', 'div2k_erosion7_4bin_patch8_64.yaml'), ['MODEL.PJS.DEPTH', '2',
                                                                                                                   'MODEL.PJS.C_DEPTH', '2'])
    assert vited.build_model(cfg).qk_norm is False           # the reference's factory has no key for it
    assert vited.build_model(cfg, qk_norm=False).qk_norm is False
    on = vited.build_model(cfg, qk_norm=True)
    assert on.qk_norm is True and tuple(on.blocks[0].attn.q_norm.weight.shape) == (32,)
    assert on.runtime(torch.bfloat16).qk_norm is True and vited.build_model(cfg).runtime(torch.bfloat16).qk_norm is False


def test_norm_parameters_are_in_the_no_decay_group(vited):
    model = _model(vited, qc.GOLDEN_SHAPES[0], qk_norm=True)
    groups = vited.engine.param_groups_no_decay_1d(model)
    no_decay = [g for g in groups if g.get('weight_decay') == 0.]
    assert len(no_decay) == 1
    held = {id(p) for p in no_decay[0]['params']}
    normed = [p for n, p in model.named_parameters() if qc.is_qk_norm_key(n)]
    assert len(normed) == 4 * 2 + 8 * 2 and all(id(p) in held for p in normed)
    decayed = {id(p) for g in groups if g.get('weight_decay') != 0. for p in g['params']}
    assert not any(id(p) in decayed for p in normed)
    dec_only = {id(p) for p in vited.engine._decoder_only_parameters(model)}
    for n, p in model.named_parameters():
        if qc.is_qk_norm_key(n):
            assert (id(p) in dec_only) == n.startswith('cross_blocks.'), n


def test_the_other_inactive_options_still_raise(vited):
    s = qc.GOLDEN_SHAPES[0]
    with pytest.raises(NotImplementedError, match='init_values'):
        _model(vited, s, init_values=0.1)
    with pytest.raises(NotImplementedError, match='init_values'):
        _model(vited, s, qk_norm=True, init_values=1e-5)
    for name in ('drop_rate', 'attn_drop_rate', 'proj_drop_rate'):
        with pytest.raises(NotImplementedError, match=name):
            _model(vited, s, qk_norm=True, **{name: 0.1})


def test_entry_points_check_their_arguments(vited):
    """head_dim other than 32 / 64 is unsupported; a null pointer of a present operand, no operand at all, a row stride that leaves
    rows overlapping and a misaligned pointer are bad arguments; a short workspace is the workspace error.  All before any launch."""
    lib = vited._lib.load()
    BAD, UNSUPPORTED, WORKSPACE = 1, 2, 4
    buf = (ctypes.c_float * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    F32 = vited._lib.F32

    def fwd(q=p, q_ld=64, k=p, k_ld=64, out_ld=64, heads=2, hd=32, gq=p, q_out=p):
        return lib.vited_qk_norm_fwd(q, q_ld, 4, k, k_ld, 4, gq, p, p, p, q_out, out_ld, p, out_ld, p, p, p, p, F32, heads, hd, 1e-6, None)

    assert fwd(q=None, k=None) == BAD
    assert fwd(hd=16) == UNSUPPORTED and fwd(hd=128) == UNSUPPORTED and fwd(hd=48) == UNSUPPORTED
    assert fwd(q_ld=63) == BAD and fwd(k_ld=32) == BAD and fwd(out_ld=60) == BAD         # rows would overlap
    assert fwd(gq=None) == BAD and fwd(q_out=None) == BAD
    assert fwd(q=p + 4) == BAD and fwd(q_ld=66) == BAD                                   # 16-byte vectors
    assert lib.vited_qk_norm_fwd(p, 64, 4, p, 64, 4, p, p, p, p, p, 64, p, 64, p, p, p, p, vited._lib.F16, 2, 32, 1e-6, None) == UNSUPPORTED

    need = lib.vited_qk_norm_bwd_workspace_bytes(4, 4, 2, 32)
    assert need > 0 and need % (2 * 2 * 32 * 4) == 0
    assert lib.vited_qk_norm_bwd_workspace_bytes(4, 0, 2, 32) == need                     # sized by the larger operand
    assert lib.vited_qk_norm_bwd_workspace_bytes(66560, 65536, 12, 32) == 2 * 1024 * 2 * 32 * 4

    def bwd(dq=p, dq_ld=64, dk=p, hd=32, ws=p, ws_bytes=need, mean=p):
        return lib.vited_qk_norm_bwd(dq, dq_ld, p, 64, mean, p, p, p, p, 4, dk, 64, p, 64, p, p, p, p, p, 4, F32, 0, 2, hd, ws, ws_bytes, None)

    assert bwd(dq=None, dk=None) == BAD and bwd(hd=8) == UNSUPPORTED
    assert bwd(dq_ld=48) == BAD and bwd(mean=None) == BAD
    assert bwd(ws=None) == WORKSPACE and bwd(ws_bytes=need - 4) == WORKSPACE


def test_operator_is_registered_with_fake_kernels(vited):
    assert 'qk_norm' in vited.custom_ops.OPERATORS and 'qk_norm_backward' in vited.custom_ops.OPERATORS
    m = 'meta'
    q, k = torch.empty(3, 65, 384, device=m, dtype=torch.bfloat16), torch.empty(3, 64, 384, device=m, dtype=torch.bfloat16)
    g = torch.empty(32, device=m)
    qo, ko, qm, qs, km, ks = torch.ops.vited.qk_norm(q, k, g, g, g, g, 12, 1e-6)
    assert qo.shape == q.shape and ko.shape == k.shape and qo.dtype == torch.bfloat16
    assert qm.shape == qs.shape == (195, 12) and km.shape == ks.shape == (192, 12) and qm.dtype == torch.float32
    outs = torch.ops.vited.qk_norm_backward(qo, ko, q, k, g, g, qm, qs, km, ks, 12)
    assert [tuple(t.shape) for t in outs] == [(3, 65, 384), (3, 64, 384), (32,), (32,), (32,), (32,)]
    with pytest.raises(NotImplementedError):
        torch.ops.vited.qk_norm(torch.zeros(2, 64), torch.zeros(2, 64), torch.ones(32), torch.zeros(32), torch.ones(32), torch.zeros(32), 2, 1e-6)
