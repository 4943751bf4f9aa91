"""Patch dropout on the MI355X: the kernels of csrc/patch_keep.hip against plain torch, bit for bit, and the model with FORCED keep
indices against the composition of tests/patchdrop_cases.py (pinned to the reference by tests/test_patchdrop.py).

Tolerances of the value tests are those of tests/test_gpu_droppath.py::_check_values, the same method on the same kind of init."""
import pytest
import torch

import droppath_cases as dc
import patchdrop_cases as pc
import qknorm_cases as qc
from oracle import vited_oracle as vo

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
BCE = torch.nn.functional.binary_cross_entropy_with_logits


# ---- the kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b,l,k', [(3, 1, 1), (3, 63, 31), (5, 64, 44), (300, 64, 6), (2, 1024, 512)])
def test_keep_from_keys_is_the_stable_argsort(vited, gpu, b, l, k):
    g = torch.Generator().manual_seed(100 + l)
    keys = torch.randn(b, l, generator=g)
    if l > 1:
        keys[0, ::3] = keys[0, 0]                        # planted equal keys: the lower index first
        keys[1, l // 2:] = keys[1, :l - l // 2].clone()
        keys[1, -1] = -0.0
        keys[1, 0] = 0.0
        keys[-1] = 0.25                                  # a constant row: 0, 1, 2, ...
    want = torch.argsort(keys, dim=-1, stable=True)[:, :k]
    got = vited.ops.keep_from_keys(keys.to(gpu), k)
    assert got.dtype == torch.int32 and got.shape == (b, k)
    assert torch.equal(got.cpu().long(), want)
    if l > 1:
        assert got[-1].tolist() == list(range(k))


def _keeps(batch, n_patches, k, lead, salt):
    return pc.closed_form_keep(batch, n_patches - lead, k, salt)


def _patch_of(keep, lead):
    """[B, R] patch index of every kept row."""
    if not lead:
        return keep
    return torch.cat((torch.zeros(keep.shape[0], 1, dtype=keep.dtype), 1 + keep), dim=1)


@pytest.mark.parametrize('u8', [False, True])
@pytest.mark.parametrize('indexed', [False, True])
def test_patchify_kept_is_patchify_indexed_by_the_keep_table(vited, gpu, u8, indexed):
    ops = vited.ops
    g = torch.Generator().manual_seed(7)
    for size, patch, k in ((64, 8, 31), (48, 16, 3)):              # 64 and 9 patches
        n = (size // patch) ** 2
        img = torch.randint(0, 256, (5, 3, size, size), generator=g, dtype=torch.uint8) if u8 else torch.randn(5, 3, size, size, generator=g)
        img = img.to(gpu)
        index = torch.tensor([4, 0, 0, 2, 3, 1, 4], device=gpu) if indexed else None
        nb = 7 if indexed else 5
        for lead in (0, 1):
            keep = _keeps(nb, n, k, lead, salt=size + lead)
            rows = _patch_of(keep, lead).to(gpu)                    # [nb, R]
            for dtype in DTYPES:
                full = ops.patchify(img, patch, dtype, index, mean=(0.4, 0.5, 0.6), std=(0.2, 0.25, 0.3)).view(nb, n, -1)
                want = full.gather(1, rows.unsqueeze(-1).expand(-1, -1, full.shape[-1])).reshape(-1, full.shape[-1])
                for table in (keep.to(gpu), keep.to(gpu).int()):
                    got = ops.patchify_kept(img, patch, dtype, table, bool(lead), index, mean=(0.4, 0.5, 0.6), std=(0.2, 0.25, 0.3))
                    assert got.dtype == dtype and got.shape == want.shape and torch.equal(got, want), (size, lead, dtype)
    # a strided batch (x[:, 1] of stacked pairs) needs no copy
    pairs = torch.randn(3, 2, 3, 16, 16, generator=g).to(gpu)
    pairs = (pairs * 40 + 128).clamp(0, 255).to(torch.uint8) if u8 else pairs
    keep = _keeps(3, 4, 2, 0, salt=1).to(gpu)
    full = ops.patchify(pairs[:, 1], 8, torch.float32).view(3, 4, -1)
    assert torch.equal(ops.patchify_kept(pairs[:, 1], 8, torch.float32, keep, False).view(3, 2, -1),
                       full.gather(1, keep.unsqueeze(-1).expand(-1, -1, full.shape[-1])))


@pytest.mark.parametrize('with_cls', [False, True])
def test_tokens_kept_is_the_torch_expression(vited, gpu, with_cls):
    g = torch.Generator().manual_seed(11)
    for b, n, k, d in ((5, 64, 31, 384), (3, 4, 2, 64), (2, 1024, 511, 128)):
        for lead in (0, 1):
            keep = _keeps(b, n, k, lead, salt=n + lead)
            rows = _patch_of(keep, lead)
            r = rows.shape[1]
            tok, pos, cls = torch.randn(b * r, d, generator=g), torch.randn(n + 1, d, generator=g), torch.randn(d, generator=g)
            want = tok.view(b, r, d) + pos[1 + rows]
            if with_cls:
                want = torch.cat(((cls + pos[0]).expand(b, 1, d), want), dim=1)
            got = vited.ops.tokens_kept(tok.to(gpu), pos.to(gpu), cls.to(gpu) if with_cls else None, keep.to(gpu), bool(lead))
            assert got.shape == want.shape and torch.equal(got.cpu(), want), (b, n, lead)


@pytest.mark.parametrize('with_cls', [False, True])
def test_dpos_is_index_add_in_a_fixed_order(vited, gpu, with_cls):
    ops = vited.ops
    g = torch.Generator().manual_seed(13)
    for b, n, k, d in ((9, 64, 20, 384), (3, 4, 2, 64), (2, 1024, 511, 128), (301, 16, 5, 32)):
        lead = 0 if with_cls else 1
        keep = _keeps(b, n - 1, k, lead, salt=n)                  # the last patch is kept by nobody
        rows = _patch_of(keep, lead)
        r, first = rows.shape[1], int(with_cls)
        inv = ops.keep_inverse(keep.to(gpu), bool(lead), n)
        want_inv = torch.full((b, n), -1, dtype=torch.int32)
        want_inv.scatter_(1, rows, torch.arange(r, dtype=torch.int32).expand(b, r))
        assert torch.equal(inv.cpu(), want_inv)
        dx = torch.randint(-8, 9, (b, r + first, d), generator=g).float()          # integer-valued: any summation order is exact
        dpos, dcls = ops.tokens_kept_bwd(dx.to(gpu), inv, with_cls)
        want = torch.zeros(n + 1, d)
        want.index_add_(0, (1 + rows).reshape(-1), dx[:, first:].reshape(-1, d))
        if with_cls:
            want[0] = dx[:, 0].sum(0)
            assert torch.equal(dcls.cpu(), want[0])
        else:
            assert dcls is None
        assert torch.equal(dpos.cpu(), want)
        never = sorted(set(range(n)) - set(rows.reshape(-1).tolist()))
        assert n - 1 in never and int(torch.count_nonzero(dpos[1 + torch.tensor(never, device=gpu)])) == 0
        dxr = torch.randn(b, r + first, d, generator=g).to(gpu)                     # random values: two runs agree bit for bit
        one, two = ops.tokens_kept_bwd(dxr, inv, with_cls), ops.tokens_kept_bwd(dxr, inv, with_cls)
        assert torch.equal(one[0], two[0]) and (not with_cls or torch.equal(one[1], two[1]))
        ref = torch.zeros(n + 1, d, dtype=torch.float64)
        ref.index_add_(0, (1 + rows).reshape(-1), dxr.cpu()[:, first:].reshape(-1, d).double())
        torch.testing.assert_close(one[0][1:].cpu().double(), ref[1:], rtol=1e-5, atol=1e-5 * b ** 0.5)


# ---- the model against the composition ------------------------------------------------------------------------------------------
def _hip_model(vited, s, gpu, dtype, state=None, **kw):
    m = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                      embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads,
                                      mlp_ratio=s.mlp_ratio, qkv_bias=s.qkv_bias, **kw)
    m.compute_dtype = dtype
    if state is not None:
        m.load_state_dict(state)
    return m.to(gpu)


def _check_values(dtype, lh, gh, lo, go):
    """fp32: logits rtol 1e-3 / atol 1e-5, every gradient tensor within 1e-3; bf16: logits 3e-2, every tensor 5e-2, 2e-2 globally."""
    exact = dtype == torch.float32
    print(f'{dtype}: logits max|d| = {float((lh - lo).abs().max()):.3e}')
    worst = max((float((gh[n] - go[n]).norm() / (go[n].norm() + 1e-12)), n) for n in go) if go else (0., '')
    num = sum(float((gh[n].double() - go[n].double()).norm() ** 2) for n in go)
    total = (num / max(sum(float(go[n].double().norm() ** 2) for n in go), 1e-300)) ** 0.5
    print(f'{dtype}: worst gradient tensor {worst[1]} rel err {worst[0]:.3e}, global {total:.3e}')
    torch.testing.assert_close(lh, lo, **(dict(rtol=1e-3, atol=1e-5) if exact else dict(rtol=3e-2, atol=3e-2)))
    for n in go:
        err = float((gh[n] - go[n]).norm() / (go[n].norm() + 1e-12))
        assert err < (1e-3 if exact else 5e-2), f'{n}: relative gradient error {err:.3e}'
    if not exact and go:
        assert total < 2e-2, total


def _grads(m):
    return {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}


def _golden_keeps(s, batch, rate, salt=0):
    return (pc.closed_form_keep(batch, s.n1 - 1, pc.keep_count(s.n1 - 1, rate), salt + 1),
            pc.closed_form_keep(batch, s.n1, pc.keep_count(s.n1, rate), salt + 2))


SHAPE_A2 = vo.ViTEDShape(depth=2, c_depth=2)                                                   # config-A geometry, 2 + 2 blocks
SHAPE_FLASH = vo.ViTEDShape(img_size=512, patch_size=16, num_classes=1, embed_dim=128, num_heads=2, depth=1, c_depth=1)
GEOMETRIES = {
    'config_a_half': (SHAPE_A2, 8, 0.5, (32, 33)),
    'config_a_p03': (SHAPE_A2, 8, 0.3, (45, 45)),
    'fixture': (pc.GOLDEN_SHAPE, 3, 0.5, (2, 3)),
    'flash_lengths': (SHAPE_FLASH, 2, 0.5, (512, 513)),      # beyond the 80-token kernels; 513 is no multiple of any tile
}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', sorted(GEOMETRIES))
def test_model_against_the_composition(vited, gpu, dtype, name):
    """Logits and every parameter gradient with forced keep indices (closed form, not ascending, different per sample)."""
    s, batch, rate, tokens = GEOMETRIES[name]
    torch.manual_seed(20)
    oracle = vo.OracleViTED(s)
    model = _hip_model(vited, s, gpu, dtype, state=oracle.state_dict(), patch_drop_rate=rate).train()
    assert tuple(1 + k for k in model.patch_keep_counts) == tokens
    x = torch.randn(batch, 2, 3, s.img_size, s.img_size).clamp(-1, 1)
    y = (torch.rand(batch, s.num_classes) > 0.6).float()
    keep1, keep2 = _golden_keeps(s, batch, rate)
    lo = pc.forward_kept(oracle, x, keep1, keep2)
    _, go = pc.loss_and_grads(oracle, lo, y)
    forced = vited.PatchKeep(keep1.to(gpu), keep2.to(gpu))
    feats = model(x[:, 0].to(gpu), forward_first_part=True, patch_keep=forced)
    assert feats.shape == (batch, tokens[0], s.embed_dim)                      # [B, 1 + K1, D] in keep order
    if dtype == torch.float32:
        torch.testing.assert_close(feats.detach().cpu(), pc.encoder_kept(oracle, x[:, 0], keep1).detach(), rtol=1e-3, atol=1e-4)
    model.zero_grad(set_to_none=True)
    lh = model(x.to(gpu), patch_keep=forced)
    BCE(lh, y.to(gpu)).backward()
    assert model.last_patch_keep.x1 is forced.x1 and model.last_patch_keep.x2 is forced.x2
    _check_values(dtype, lh.detach().cpu(), _grads(model), lo.detach(), go)


def _run(model, x, y, **kw):
    model.zero_grad(set_to_none=True)
    logits = model(x, **kw)
    BCE(logits, y).backward()
    return logits.detach().cpu(), _grads(model)


def _batch(s, batch, gpu, seed=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, 2, 3, s.img_size, s.img_size, generator=g).clamp(-1, 1).to(gpu)
    return x, (torch.rand(batch, s.num_classes, generator=g) > 0.7).float().to(gpu)


def _pair_of_models(vited, gpu, dtype, s, seed, rate=0.5):
    torch.manual_seed(seed)
    state = vo.OracleViTED(s).state_dict()
    return (_hip_model(vited, s, gpu, dtype, state=state, patch_drop_rate=rate).train(),
            _hip_model(vited, s, gpu, dtype, state=state).train())


def test_full_keep_in_order_is_the_model_without_patch_dropout(vited, gpu):
    s = SHAPE_A2
    dropped, plain = _pair_of_models(vited, gpu, torch.float32, s, seed=21)
    x, y = _batch(s, 4, gpu)
    full = vited.PatchKeep(torch.arange(s.n1 - 1, device=gpu).expand(4, -1).contiguous(), torch.arange(s.n1, device=gpu).expand(4, -1).contiguous())
    l1, g1 = _run(dropped, x, y, patch_keep=full)
    l0, g0 = _run(plain, x, y)
    assert plain.last_patch_keep is None
    _check_values(torch.float32, l1, g1, l0, g0)


def test_the_order_of_a_keep_row_does_not_move_the_logits(vited, gpu):
    """Attention and the cls read-out are permutation invariant over the kept tokens (each carries its own position)."""
    s = SHAPE_A2
    model, _ = _pair_of_models(vited, gpu, torch.float32, s, seed=22)
    x, y = _batch(s, 4, gpu)
    keep1, keep2 = _golden_keeps(s, 4, 0.5)
    l0, g0 = _run(model, x, y, patch_keep=vited.PatchKeep(keep1.to(gpu), keep2.to(gpu)))
    l1, g1 = _run(model, x, y, patch_keep=vited.PatchKeep(keep1.flip(1).to(gpu), keep2.roll(5, 1).to(gpu)))
    _check_values(torch.float32, l1, g1, l0, g0)


@pytest.mark.parametrize('dtype', DTYPES)
def test_eval_mode_is_the_model_without_patch_dropout(vited, gpu, dtype):
    s = SHAPE_A2
    dropped, plain = _pair_of_models(vited, gpu, dtype, s, seed=23, rate=0.3)
    x, _ = _batch(s, 8, gpu)
    with torch.no_grad():
        assert torch.equal(dropped.eval()(x), plain.eval()(x))
        assert dropped.last_patch_keep is None
        # training mode draws, for the batch of the call, on the device
        out = dropped.train()(x)
    keep = dropped.last_patch_keep
    assert out.shape == (8, s.num_classes) and keep.x1.shape == (8, 44) and keep.x2.shape == (8, 44) and keep.x1.is_cuda
    assert keep.x1.dtype == torch.int32 and int(keep.x1.min()) >= 0 and int(keep.x1.max()) < 63 and int(keep.x2.max()) < 64
    assert all(len(set(row)) == 44 for row in keep.x2.tolist() + keep.x1.tolist())
    # the caches and the relevancy paths never drop
    with torch.no_grad():
        tokens, _ = dropped.cache_image2_tokens(x[:, 1])
    assert tokens.shape[1] == s.n2


def test_draw_on_the_device_is_argsort_of_the_same_keys(vited, gpu):
    m = _hip_model(vited, SHAPE_A2, gpu, None, patch_drop_rate=0.5)
    keep = m.draw_patch_keep(6, 5, generator=torch.Generator(device=gpu).manual_seed(3))
    g = torch.Generator(device=gpu).manual_seed(3)
    k1 = torch.argsort(torch.randn(6, 63, generator=g, device=gpu), dim=-1, stable=True)[:, :31]
    k2 = torch.argsort(torch.randn(5, 64, generator=g, device=gpu), dim=-1, stable=True)[:, :32]
    assert torch.equal(keep.x1.long(), k1) and torch.equal(keep.x2.long(), k2)


def _keep_avoiding(batch, tokens, k, avoid, salt):
    """closed_form_keep over the tokens other than ``avoid``."""
    keep = pc.closed_form_keep(batch, tokens - 1, k, salt)
    return keep + (keep >= avoid).long()


@pytest.mark.parametrize('dtype', DTYPES)
def test_pos_embed_gradient_is_zero_where_every_sample_dropped(vited, gpu, dtype):
    s = SHAPE_A2
    model, _ = _pair_of_models(vited, gpu, dtype, s, seed=24)
    x, y = _batch(s, 8, gpu)
    # patches 5 and 40 are kept by no sample of either stream (index 4 / 39 behind patch 0 on the image-1 stream)
    keep1 = _keep_avoiding(8, s.n1 - 2, 31, 4, salt=1)
    keep1 = keep1 + (keep1 >= 39).long()
    keep2 = _keep_avoiding(8, s.n1 - 1, 32, 5, salt=2)
    keep2 = keep2 + (keep2 >= 40).long()
    assert not ((1 + keep1 == 5) | (1 + keep1 == 40)).any() and not ((keep2 == 5) | (keep2 == 40)).any()
    _, g = _run(model, x, y, patch_keep=vited.PatchKeep(keep1.to(gpu), keep2.to(gpu)))
    pos = g['pos_embed'][0]
    kept = sorted(set((1 + keep1).reshape(-1).tolist()) | set(keep2.reshape(-1).tolist()) | {0})
    dead = sorted(set(range(s.n1)) - set(kept))
    assert 5 in dead and 40 in dead
    assert int(torch.count_nonzero(pos[1 + torch.tensor(dead)])) == 0
    assert all(bool(pos[1 + p].abs().max() > 0) for p in kept) and bool(pos[0].abs().max() > 0)


# ---- the forms --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_two_stage_and_pair_indexed_forms_match_the_stacked_form(vited, gpu, dtype):
    """3 images, 5 pairs (256-pixel images, patch 16: 128 / 129 of 256 / 257 tokens, head dim 64): the stacked one-shot form on the
    gathered images against the two-stage step with torch's gathers, and against the pair-indexed form that gathers inside the kernels."""
    s = vo.ViTEDShape(img_size=256, patch_size=16, num_classes=1, num_heads=6, depth=2, c_depth=2)
    torch.manual_seed(25)
    state = vo.OracleViTED(s).state_dict()
    model = _hip_model(vited, s, gpu, dtype, state=state, patch_drop_rate=0.5).train()
    imgs = torch.randn(3, 3, 256, 256).clamp(-1, 1).to(gpu)
    gi, gj = torch.tensor([0, 2, 1, 2, 0], device=gpu), torch.tensor([1, 0, 2, 2, 1], device=gpu)
    y = (torch.rand(5, 1) > 0.5).float().to(gpu)
    keep1, keep2 = _golden_keeps(s, 3, 0.5)[0].to(gpu), _golden_keeps(s, 5, 0.5)[1].to(gpu)
    stacked = torch.stack((imgs[gi], imgs[gj]), dim=1)
    l0, g0 = _run(model, stacked, y, patch_keep=vited.PatchKeep(keep1[gi], keep2))

    def two_stage(**index):
        model.zero_grad(set_to_none=True)
        feats = model(imgs, forward_first_part=True, patch_keep=vited.PatchKeep(keep1, None))
        assert feats.shape == (3, 128, s.embed_dim)
        if index:
            logits = model(feats, imgs, patch_keep=vited.PatchKeep(None, keep2), **index)
        else:
            logits = model(feats[gi], imgs[gj], patch_keep=vited.PatchKeep(None, keep2))
        BCE(logits, y).backward()
        assert model.last_patch_keep.x1 is keep1 and model.last_patch_keep.x2 is keep2
        return logits.detach().cpu(), _grads(model)

    _check_values(dtype, *two_stage(), l0, g0)
    _check_values(dtype, *two_stage(x2_index=gj, x1_index=gi), l0, g0)


@pytest.mark.parametrize('dtype', DTYPES)
def test_uint8_inputs_match_the_float_inputs(vited, gpu, dtype):
    s = SHAPE_A2
    model, _ = _pair_of_models(vited, gpu, dtype, s, seed=26)
    g = torch.Generator().manual_seed(5)
    xu = torch.randint(0, 256, (4, 2, 3, 64, 64), generator=g, dtype=torch.uint8).to(gpu)
    xf = (xu.float() / 255 - 0.5) / 0.5
    y = (torch.rand(4, s.num_classes, generator=g) > 0.7).float().to(gpu)
    keep1, keep2 = _golden_keeps(s, 4, 0.5)
    forced = vited.PatchKeep(keep1.to(gpu), keep2.to(gpu))
    _check_values(dtype, *_run(model, xu, y, patch_keep=forced), *_run(model, xf, y, patch_keep=forced))


@pytest.mark.parametrize('dtype', DTYPES)
def test_with_drop_path_and_qk_norm(vited, gpu, dtype):
    s = SHAPE_A2
    torch.manual_seed(27)
    oracle = qc.randomize_norms_(qc.QKNormViTED(s), torch.Generator().manual_seed(28))
    model = _hip_model(vited, s, gpu, dtype, state=oracle.state_dict(), patch_drop_rate=0.5, drop_path_rate=0.5, qk_norm=True).train()
    x = torch.randn(8, 2, 3, 64, 64).clamp(-1, 1)
    y = (torch.rand(8, s.num_classes) > 0.6).float()
    keep1, keep2 = _golden_keeps(s, 8, 0.5)
    enc, dec = dc.irregular_scales(0.5, s.depth, 2, 8, salt=3), dc.irregular_scales(0.5, s.c_depth, 3, 8, salt=5)
    lo = pc.forward_kept(oracle, x, keep1, keep2, enc, dec)
    _, go = pc.loss_and_grads(oracle, lo, y)
    lh, gh = _run(model, x.to(gpu), y.to(gpu), patch_keep=vited.PatchKeep(keep1.to(gpu), keep2.to(gpu)),
                  drop_path=vited.DropPathScales(enc.to(gpu), dec.to(gpu)))
    # the gradient of every k_norm.bias is zero in exact arithmetic (a constant added to all keys of a row moves no softmax): as in
    # tests/test_gpu_qknorm.py::_check those tensors are held to the same figure times the norm of the module's weight gradient
    # instead of a relative error against a reference that is itself rounding noise
    zero = [n for n in go if n.endswith('k_norm.bias')]
    for n in zero:
        bound = (1e-3 if dtype == torch.float32 else 5e-2) * float(go[n.replace('.bias', '.weight')].norm())
        print(f'{dtype}: {n} |g| = {float(gh[n].norm()):.3e} (reference {float(go[n].norm()):.1e}, bound {bound:.3e})')
        assert float(gh[n].norm()) <= bound, n
    assert len(zero) == s.depth + 2 * s.c_depth
    _check_values(dtype, lh, {n: g for n, g in gh.items() if n not in zero}, lo.detach(), {n: g for n, g in go.items() if n not in zero})


# ---- TrainStep --------------------------------------------------------------------------------------------------------------------
def _train_steps(vited, gpu, s, state, use_graph, **kw):
    m = _hip_model(vited, s, gpu, None, state=state, patch_drop_rate=0.5, **kw).train()
    opt = vited.optim.FlatAdamW(vited.engine.param_groups_no_decay_1d(m), lr=1e-3, weight_decay=0.05)
    return m, vited.engine.TrainStep(m, opt, clip_grad=5.0, amp=True, use_graph=use_graph)


def test_train_step_captured_equals_eager_with_forced_keep(vited, gpu):
    """Config-A geometry, 3 + 3 blocks, B = 16, bf16: two eager warm-up steps, then three replays of the captured graphs, against the
    eagerly launched step - the same loss at every step and the same parameters at the end, bit for bit."""
    s = vo.ViTEDShape(depth=3, c_depth=3)
    torch.manual_seed(30)
    state = vo.OracleViTED(s).state_dict()
    (me, eager), (mg, graph) = _train_steps(vited, gpu, s, state, False), _train_steps(vited, gpu, s, state, True)
    keep1, keep2 = _golden_keeps(s, 16, 0.5)
    eager.patch_keep = graph.patch_keep = vited.PatchKeep(keep1.to(gpu).int(), keep2.to(gpu).int())
    g = torch.Generator().manual_seed(12)
    for it in range(5):
        x = torch.randn(16, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)
        y = (torch.rand(16, 4, generator=g) > 0.6).float().to(gpu)
        le, lg = float(eager.step(x, y)), float(graph.step(x, y))
        assert le == lg, (it, le, lg)
    assert graph._g1 is not None and graph._g2 is not None
    for (n, pe), (_, pg) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.equal(pe, pg), n


def test_train_step_replays_draw_anew(vited, gpu):
    """Drawn indices under capture: the keys and the ranking kernel are part of the graph (the device's default generator), so
    consecutive replays leave different indices in the static ``last_patch_keep`` (16 x 2 draws of 31 / 32 out of 63 / 64 patches: two
    replays agree with negligible probability) and the loss stays finite.  Stochastic depth draws in the same graph."""
    s = vo.ViTEDShape(depth=3, c_depth=3)
    torch.manual_seed(31)
    m, step = _train_steps(vited, gpu, s, vo.OracleViTED(s).state_dict(), True, drop_path_rate=0.2)
    g = torch.Generator().manual_seed(13)
    seen = []
    for it in range(5):
        x = torch.randn(16, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)
        y = (torch.rand(16, 4, generator=g) > 0.6).float().to(gpu)
        loss = step.step(x, y)
        assert bool(torch.isfinite(loss)), it
        seen.append(torch.cat([t.reshape(-1) for t in m.last_patch_keep]).clone())
    assert step._g1 is not None
    assert seen[-1].numel() == 16 * (31 + 32)
    assert not torch.equal(seen[-1], seen[-2]) and not torch.equal(seen[-2], seen[-3])      # replays 3, 2 and 1
    assert int(seen[-1].min()) >= 0 and int(seen[-1].max()) < 64
    static = m.last_patch_keep
    step.step(x, y)
    assert m.last_patch_keep.x1 is static.x1 and m.last_patch_keep.x2 is static.x2            # a static buffer, rewritten by the replay


def test_indexed_and_mined_two_stage_steps_train_with_it(vited, gpu):
    """hisfrag_prepare_indexed / hisfrag_prepare_mined: the encoder draws per image, the decoder per pair (padding rows included)."""
    s = vo.ViTEDShape(num_classes=1, depth=2, c_depth=2)
    torch.manual_seed(32)
    model = _hip_model(vited, s, gpu, torch.bfloat16, patch_drop_rate=0.5).train()
    samples = torch.randn(6, 3, 64, 64).clamp(-1, 1).to(gpu)
    targets = torch.tensor([0, 0, 1, 1, 2, 2], device=gpu)
    (x, feats, x2_index, x1_index), labels = vited.engine.hisfrag_prepare_indexed(model, samples, targets, amp=False)
    assert feats.shape == (6, 32, s.embed_dim) and model.last_patch_keep.x1.shape == (6, 31)
    logits = model(feats, x, x2_index=x2_index, x1_index=x1_index)
    assert model.last_patch_keep.x2.shape == (labels.shape[0], 32)
    BCE(logits, labels).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    model.zero_grad(set_to_none=True)
    capacity = vited.engine.mined_pair_capacity(6, 2)
    (x, feats, x2_index, segments), mined = vited.engine.hisfrag_prepare_mined(model, samples, targets, capacity, amp=False)
    logits = model(feats, x, x2_index=x2_index, x1_index=segments)
    assert logits.shape[0] == capacity and model.last_patch_keep.x2.shape == (capacity, 32)
    loss = vited.engine.mined_bce_with_logits(logits, mined)
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
