"""Patch dropout, the parts that need no GPU: the constructor surface, timm's keep count, the draw on the CPU, the pin of the
composition in tests/patchdrop_cases.py against what the reference's own classes computed (tests/golden/patch_drop.npz), and the
argument checks of the new entry points and of their wrappers, all before any launch."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import patchdrop_cases as pc
from oracle import vited_oracle as vo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'patch_drop.npz')


def _model(vited, rate, s=pc.GOLDEN_SHAPE, **kw):
    return vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                         embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads,
                                         patch_drop_rate=rate, **kw)


def test_constructor_takes_the_rate(vited):
    """What fails without the feature (NotImplementedError from the constructor): 0.25 and 0.5 are accepted, 1.0 and -0.1 are not."""
    for rate in (0.25, 0.5):
        m = _model(vited, rate)
        assert m.patch_drop_rate == rate and m.last_patch_keep is None
    assert _model(vited, 0.).patch_drop_rate == 0. and _model(vited, None).patch_drop_rate == 0.
    for rate in (1.0, -0.1):
        with pytest.raises(ValueError, match='patch_drop_rate'):
            _model(vited, rate)
    # no parameter, no state_dict key: a checkpoint of the model without it loads
    assert list(_model(vited, 0.5).state_dict()) == list(_model(vited, 0.).state_dict())
    for name in ('init_values', 'drop_rate', 'attn_drop_rate', 'proj_drop_rate'):          # the options that stay refused
        with pytest.raises(NotImplementedError):
            _model(vited, 0.5, **{name: 0.1})


def test_build_model_forwards_the_rate(vited):
    cfg = vited.config_from_yaml(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs', 'test',
                                              'test_pjs_hisfrag20_patch32_64.yaml'))
    assert vited.build_model(cfg).patch_drop_rate == 0.
    assert vited.build_model(cfg, patch_drop_rate=0.25).patch_drop_rate == 0.25


# max(1, int(L * (1. - p))) evaluated by hand in IEEE double arithmetic: e.g. 1. - 0.9 = 0.09999999999999998, times 1024 = 102.39...;
# 1. - 0.3 = 0.7, times 64 = 44.8; 1. - 0.1 = 0.9, times 63 = 56.7
KEEP_TABLE = {
    1: {0.1: 1, 0.3: 1, 0.5: 1, 0.75: 1, 0.9: 1},
    3: {0.1: 2, 0.3: 2, 0.5: 1, 0.75: 1, 0.9: 1},
    63: {0.1: 56, 0.3: 44, 0.5: 31, 0.75: 15, 0.9: 6},
    64: {0.1: 57, 0.3: 44, 0.5: 32, 0.75: 16, 0.9: 6},
    1023: {0.1: 920, 0.3: 716, 0.5: 511, 0.75: 255, 0.9: 102},
    1024: {0.1: 921, 0.3: 716, 0.5: 512, 0.75: 256, 0.9: 102},
}


def test_keep_count_is_timms_expression(vited):
    from vited_amd.model import patch_keep_count
    for tokens, row in KEEP_TABLE.items():
        for rate, want in row.items():
            assert max(1, int(tokens * (1. - rate))) == want, (tokens, rate)          # the table is the Python expression
            assert patch_keep_count(tokens, rate) == want and pc.keep_count(tokens, rate) == want, (tokens, rate)
    # the model's two counts: L1 = n1 - 1 behind patch 0, L2 = n1 behind the cls token
    s = vo.ViTEDShape(depth=1, c_depth=1)                                              # 64 patches
    assert _model(vited, 0.3, s).patch_keep_counts == (44, 44) and _model(vited, 0.5, s).patch_keep_counts == (31, 32)
    assert _model(vited, 0.5).patch_keep_counts == (1, 2)                              # the fixture geometry: 2 / 3 tokens


def test_draw_on_the_cpu(vited):
    s = vo.ViTEDShape(depth=1, c_depth=1)
    m = _model(vited, 0.3, s)
    g = torch.Generator().manual_seed(5)
    keep = m.draw_patch_keep(6, 9, generator=g)
    assert isinstance(keep, vited.PatchKeep) and keep.x1.shape == (6, 44) and keep.x2.shape == (9, 44)
    assert keep.x1.dtype in (torch.int32, torch.int64)
    for t, tokens in ((keep.x1, 63), (keep.x2, 64)):
        assert int(t.min()) >= 0 and int(t.max()) < tokens
        assert all(len(set(row)) == len(row) for row in t.tolist())                    # distinct within a row
    assert any(row != sorted(row) for row in keep.x2.tolist())                         # not re-sorted
    assert not torch.equal(keep.x2[0], keep.x2[1])                                     # independent per sample
    half = m.draw_patch_keep(None, 4)
    assert half.x1 is None and half.x2.shape == (4, 44)
    # the same keys, the same indices: argsort(randn)[:, :K]
    k1 = m.draw_patch_keep(3, None, generator=torch.Generator().manual_seed(7)).x1
    want = torch.argsort(torch.randn(3, 63, generator=torch.Generator().manual_seed(7)), dim=-1, stable=True)[:, :44]
    assert torch.equal(k1, want)


def test_eval_forward_records_no_keep(vited, monkeypatch):
    """Eval mode never drops: the forward asks for no draw and leaves ``last_patch_keep`` None (the launch itself is stubbed out)."""
    m = _model(vited, 0.5).eval()
    seen = []
    monkeypatch.setattr(m, '_check_images', lambda img: None)
    monkeypatch.setattr(m, '_run_fn', lambda fn, drop, keep, *args: seen.append(keep) or torch.zeros(2, 3, 64))
    m.last_patch_keep = 'stale'
    m(torch.zeros(2, 2, 3, 16, 16))
    assert seen == [None, None] and m.last_patch_keep is None
    m.train()
    m(torch.zeros(2, 2, 3, 16, 16))
    assert seen[2] is not None and seen[2][0].shape == (2, 1) and seen[3][1].shape == (2, 2)
    assert m.last_patch_keep.x1 is seen[2][0] and m.last_patch_keep.x2 is seen[2][1]
    for flag in ('keep_attn', 'keep_cam'):                                              # the relevancy paths see every patch
        setattr(m, flag, True)
        m(torch.zeros(2, 2, 3, 16, 16))
        assert seen[-1] is None and m.last_patch_keep is None
        setattr(m, flag, False)
    forced = vited.PatchKeep(torch.tensor([[2], [0]]), torch.tensor([[3, 1], [0, 2]]))
    m.eval()(torch.zeros(2, 2, 3, 16, 16), patch_keep=forced)                           # explicit indices hold in any mode
    assert seen[-1] == (forced.x1, forced.x2) and m.last_patch_keep == forced
    for bad in (vited.PatchKeep(forced.x1, None), vited.PatchKeep(forced.x1[:1], forced.x2), vited.PatchKeep(forced.x1.float(), forced.x2),
                vited.PatchKeep(torch.zeros(2, 4, dtype=torch.int64), forced.x2)):
        with pytest.raises(ValueError, match='patch_keep'):
            m(torch.zeros(2, 2, 3, 16, 16), patch_keep=bad)


def test_composition_matches_the_reference_fixture():
    """The composition of patchdrop_cases (gather behind the prefix after the position embedding, patch 0 as the prefix of the image-1
    stream) in fp64 equals what the reference's VisionTransformerCustom gave with its ``patch_drop`` forced to the same indices."""
    fx = np.load(GOLDEN)
    x, y, keep1, keep2 = pc.golden_inputs()
    np.testing.assert_array_equal(fx['keep1'], keep1.numpy())
    np.testing.assert_array_equal(fx['keep2'], keep2.numpy())
    s = pc.GOLDEN_SHAPE
    assert keep1.shape == (pc.GOLDEN_BATCH, pc.keep_count(s.n1 - 1, float(fx['rate']))) and keep2.shape[1] == pc.keep_count(s.n1, float(fx['rate']))
    m = vo.fill_closed_form_(vo.OracleViTED(s)).double()
    feats = pc.encoder_kept(m, x[:, 0].double(), keep1)
    assert feats.shape == (pc.GOLDEN_BATCH, 2, s.embed_dim)                           # 2 / 3 tokens
    logits = pc.forward_kept(m, x.double(), keep1, keep2)
    loss, grads = pc.loss_and_grads(m, logits, y.double())
    np.testing.assert_allclose(logits.detach().numpy(), fx['logits'], rtol=1e-9, atol=0)
    np.testing.assert_allclose(loss.numpy(), fx['loss'], rtol=1e-9)
    names = [str(n) for n in fx['grad_names']]
    assert names == [n for n, _ in m.named_parameters()]
    norms = np.array([float(grads[n].norm()) for n in names])
    np.testing.assert_allclose(norms, fx['grad_norms'], rtol=1e-9)
    for n, norm, want in zip(names, fx['grad_norms'], fx['grad_slices']):
        got = grads[n].reshape(-1)[:16].numpy()
        np.testing.assert_allclose(got, want[:got.size], rtol=1e-9, atol=1e-9 * norm, err_msg=n)
    # the indices matter: the same weights on every patch, or with the image-1 prefix treated as droppable, give other logits
    assert not np.allclose(m(x.double()).detach().numpy(), fx['logits'], rtol=1e-3)
    # ForcedPatchDrop is the same gather
    tok = m._patch_tokens(x[:, 0].double()) + m.pos_embed[:, 1:]
    got = pc.ForcedPatchDrop(keep1)(tok)
    assert torch.equal(got[:, 0], tok[:, 0]) and torch.equal(got[:, 1], tok[torch.arange(3), 1 + keep1[:, 0]])


def test_entry_points_check_their_arguments(vited):
    """A null pointer, K > L, a keep table that does not fit the patches and a misaligned pointer are bad arguments, L > 4096 is
    unsupported: all before any launch (no GPU here: a launch would fail differently)."""
    lib = vited._lib.load()
    BAD, UNSUPPORTED = 1, 2
    buf = (ctypes.c_float * 8192)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    F32, BF16 = vited._lib.F32, vited._lib.BF16

    def keys(k=p, keep=p, batch=2, L=64, K=32):
        return lib.vited_keep_from_keys(k, keep, batch, L, K, None)

    assert keys(k=None) == BAD and keys(keep=None) == BAD and keys(batch=0) == BAD and keys(L=0) == BAD and keys(K=0) == BAD
    assert keys(K=65) == BAD and keys(L=4097, K=5) == UNSUPPORTED and keys(L=5000, K=6000) == BAD
    assert keys(k=p + 2) == BAD and keys(keep=p + 1) == BAD

    def patchify(img=p, keep=p, K=2, lead=0, out=p, dtype=BF16, batch=2, chans=3, size=16, patch=8):
        return lib.vited_patchify_kept(img, 3 * size * size, None, keep, K, lead, out, dtype, batch, chans, size, patch, None)

    assert patchify(img=None) == BAD and patchify(keep=None) == BAD and patchify(out=None) == BAD and patchify(batch=0) == BAD
    assert patchify(K=5) == BAD and patchify(K=4, lead=1) == BAD and patchify(K=0) == BAD and patchify(lead=2) == BAD      # 4 patches
    assert patchify(size=12) == BAD and patchify(keep=p + 2) == BAD and patchify(img=p + 1) == BAD
    assert patchify(dtype=vited._lib.F16) == UNSUPPORTED

    def patchify_u8(img=p, keep=p, K=2, lead=0, mean=p, std=p, chans=3):
        return lib.vited_patchify_kept_u8(img, 768, None, keep, K, lead, p, BF16, 2, chans, 16, 8, mean, std, None)

    assert patchify_u8(img=None) == BAD and patchify_u8(mean=None) == BAD and patchify_u8(std=None) == BAD and patchify_u8(chans=5) == BAD
    assert patchify_u8(K=5) == BAD and patchify_u8(K=4, lead=1) == BAD
    assert patchify_u8() == BAD                                  # std = 0.0 in the zeroed buffer: refused too, still before a launch

    def tokens(tok=p, pos=p, cls=None, keep=p, K=2, lead=0, x=p, n=4, dim=64):
        return lib.vited_tokens_kept(tok, pos, cls, keep, K, lead, x, 2, n, dim, None)

    assert tokens(tok=None) == BAD and tokens(pos=None) == BAD and tokens(keep=None) == BAD and tokens(x=None) == BAD
    assert tokens(K=5) == BAD and tokens(K=4, lead=1) == BAD and tokens(dim=62) == BAD
    assert tokens(tok=p + 4) == BAD and tokens(pos=p + 8) == BAD and tokens(cls=p + 4) == BAD and tokens(x=p + 12) == BAD      # 16-byte rows

    def inverse(keep=p, K=2, lead=0, inv=p, n=4):
        return lib.vited_keep_inverse(keep, K, lead, inv, 2, n, None)

    assert inverse(keep=None) == BAD and inverse(inv=None) == BAD and inverse(K=5) == BAD and inverse(K=4, lead=1) == BAD
    assert inverse(keep=p + 2) == BAD and inverse(n=0) == BAD

    def bwd(dx=p, inv=p, dpos=p, dcls=None, rows=3, with_cls=0, n=4, dim=64):
        return lib.vited_tokens_kept_bwd(dx, inv, dpos, dcls, 2, rows, with_cls, n, dim, None)

    assert bwd(dx=None) == BAD and bwd(inv=None) == BAD and bwd(dpos=None) == BAD
    assert bwd(rows=5) == BAD and bwd(rows=1, with_cls=1) == BAD and bwd(rows=6, with_cls=1) == BAD and bwd(dcls=p) == BAD
    assert bwd(dim=30) == BAD and bwd(dx=p + 4) == BAD and bwd(dpos=p + 8) == BAD and bwd(inv=p + 2) == BAD


# ---- the wrappers: every tensor is checked before its pointer reaches the library (the protocol of tests/test_ops_args.py) ----------
@pytest.fixture
def ops(vited, monkeypatch):
    calls = []
    monkeypatch.setattr(vited.ops, '_need_gpu', lambda *tensors, **kw: None)
    monkeypatch.setattr(vited.ops, '_stream', lambda: 0)
    monkeypatch.setattr(vited.ops, '_lib', SimpleNamespace(call=lambda name, *args: calls.append((name, args))))
    vited.ops.calls = calls
    yield vited.ops
    del vited.ops.calls


def z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


WRAPPERS = {
    'keep_from_keys': ('vited_keep_from_keys', lambda: dict(keys=z(3, 64), k=44)),
    'patchify_kept': ('vited_patchify_kept', lambda: dict(img=z(4, 3, 16, 16), patch=8, dtype=torch.bfloat16, keep=z(2, 2, dtype=torch.int32),
                                                         lead=False, batch_index=z(2, dtype=torch.int64))),
    'patchify_kept_u8': ('vited_patchify_kept_u8', lambda: dict(img=z(2, 3, 16, 16, dtype=torch.uint8), patch=8, dtype=torch.float32,
                                                               keep=z(2, 3, dtype=torch.int64), lead=True)),
    'tokens_kept': ('vited_tokens_kept', lambda: dict(tok=z(6, 64), pos=z(5, 64), cls=z(64), keep=z(2, 3, dtype=torch.int32), lead=False)),
    'tokens_kept_x1': ('vited_tokens_kept', lambda: dict(tok=z(8, 64), pos=z(5, 64), cls=None, keep=z(2, 3, dtype=torch.int32), lead=True)),
    'keep_inverse': ('vited_keep_inverse', lambda: dict(keep=z(2, 3, dtype=torch.int32), lead=True, n_patches=4)),
    'tokens_kept_bwd': ('vited_tokens_kept_bwd', lambda: dict(dx=z(2, 4, 64), inv=z(2, 4, dtype=torch.int32), with_cls=True)),
}
# mutations that are no fault: a strided image or table is copied dense by the wrapper; one key, one kept index or one patch fewer
# is another valid problem
NOT_A_FAULT = {('patchify_kept', 'img', 'strided'), ('patchify_kept', 'img', 'row-strided'), ('patchify_kept_u8', 'img', 'strided'),
               ('patchify_kept_u8', 'img', 'row-strided'), ('keep_from_keys', 'keys', 'short'), ('keep_inverse', 'keep', 'short'),
               ('patchify_kept', 'keep', 'short'), ('patchify_kept_u8', 'keep', 'short'), ('tokens_kept_bwd', 'inv', 'short')}


def _mutants(t):
    yield 'dtype', t.to(torch.int16 if t.dtype.is_floating_point else torch.float64)
    yield 'short', t[..., :-1].contiguous()
    if t.numel() > 1:
        wide = torch.zeros(*t.shape, 2, dtype=t.dtype)
        yield 'strided', wide[..., 0]
    if t.dim() >= 2 and t.numel() > t.shape[-1]:
        yield 'row-strided', torch.zeros(*t.shape[:-1], t.shape[-1] + 1, dtype=t.dtype)[..., :-1]


@pytest.mark.parametrize('case', sorted(WRAPPERS))
def test_wrappers_refuse_one_fault_before_the_launch(ops, case):
    entry, build = WRAPPERS[case]
    op = case.removesuffix('_u8').removesuffix('_x1')
    getattr(ops, op)(**build())
    assert [name for name, _ in ops.calls] == [entry]
    del ops.calls[:]
    tried = 0
    for key, t in build().items():
        if not torch.is_tensor(t):
            continue
        for fault, bad in _mutants(t):
            keep_table = key == 'keep' and fault in ('strided', 'row-strided')          # copied dense, like the image
            if (case, key, fault) in NOT_A_FAULT or keep_table:
                continue
            tried += 1
            with pytest.raises((ValueError, TypeError), match=rf'^{op}: '):
                getattr(ops, op)(**dict(build(), **{key: bad}))
            assert not ops.calls, (case, key, fault)
    assert tried
    # and the counts the wrappers refuse themselves
    refused = {'keep_from_keys': [dict(k=0), dict(k=65), dict(keys=z(2, 4097), k=5)],
               'patchify_kept': [dict(keep=z(2, 5, dtype=torch.int32)), dict(keep=z(3, 2, dtype=torch.int32)), dict(patch=5)],
               'patchify_kept_u8': [dict(keep=z(2, 4, dtype=torch.int32))],
               'tokens_kept': [dict(keep=z(2, 5, dtype=torch.int32)), dict(tok=z(6, 62), pos=z(5, 62), cls=z(62))],
               'tokens_kept_x1': [dict(keep=z(2, 4, dtype=torch.int32))],
               'keep_inverse': [dict(n_patches=3)],
               'tokens_kept_bwd': [dict(with_cls=False, dx=z(2, 5, 64)), dict(dx=z(2, 1, 64))]}[case]
    for kw in refused:
        with pytest.raises(ValueError, match=rf'^{op}: '):
            getattr(ops, op)(**dict(build(), **kw))
        assert not ops.calls, (case, kw)
