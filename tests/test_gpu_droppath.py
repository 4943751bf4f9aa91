"""Stochastic depth on the MI355X: the scaled residual epilogues (row-complete kernel, tile kernels, portable GEMM) and the scaled
low-precision gradient copies, against the composition of tests/droppath_cases.py, and the exact identities the scales allow.

Scales are forced unless a test says otherwise, kept and dropped samples interleaved irregularly: a 64-256-row tile then holds
rows of samples with different scales, the smallest way the row -> scale step can go wrong.  Tolerances of the value tests are
those of test_against_oracle_random_init (tests/test_gpu_model.py), the same method on the same kind of init."""
import pytest
import torch

import droppath_cases as dc
from oracle import vited_oracle as vo

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
BCE = torch.nn.functional.binary_cross_entropy_with_logits


def _hip_model(vited, s, gpu, dtype, rate=0., state=None):
    m = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                      embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads,
                                      mlp_ratio=s.mlp_ratio, qkv_bias=s.qkv_bias, drop_path_rate=rate)
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


def _one_shot_case(vited, gpu, dtype, s, batch, seed, prepare=None):
    torch.manual_seed(seed)
    oracle = vo.OracleViTED(s)
    model = _hip_model(vited, s, gpu, dtype, rate=0.5, state=oracle.state_dict()).train()
    if prepare is not None:
        prepare(model)
    x = torch.randn(batch, 2, 3, s.img_size, s.img_size).clamp(-1, 1)
    y = (torch.rand(batch, s.num_classes) > 0.75).float()
    enc = dc.irregular_scales(0.5, s.depth, 2, batch, salt=3)
    dec = dc.irregular_scales(0.5, s.c_depth, 3, batch, salt=5)
    lo, go = dc.forward_scaled(oracle, x, enc, dec), None
    _, go = dc.loss_and_grads(oracle, lo, y)
    drop = vited.DropPathScales(enc.to(gpu), dec.to(gpu))
    lh = model(x.to(gpu), drop_path=drop)
    BCE(lh, y.to(gpu)).backward()
    assert model.last_drop_path.enc is drop.enc and model.last_drop_path.dec is drop.dec
    return model, drop, x, lh.detach().cpu(), _grads(model), lo.detach(), go


@pytest.mark.parametrize('dtype', DTYPES)
def test_config_a_geometry_against_the_composition(vited, gpu, dtype):
    """D 384, 12 heads, 64 / 65 tokens, 3 + 3 blocks, B = 8: in bf16 every residual Linear of the full-row blocks is the row-complete
    Linear + residual + LayerNorm kernel, and the backward's scaled copies come from its backward form."""
    s = vo.ViTEDShape(depth=3, c_depth=3)
    ops = vited.ops
    seen = {'fwd': 0, 'bwd': 0}
    real_fwd, real_bwd = ops.linear_residual_layernorm_fwd, ops.linear_layernorm_bwd

    def spy_fwd(*a, **k):
        seen['fwd'] += k.get('row_scale') is not None
        return real_fwd(*a, **k)

    def spy_bwd(*a, **k):
        seen['bwd'] += k.get('lp_scale') is not None
        return real_bwd(*a, **k)

    ops.linear_residual_layernorm_fwd, ops.linear_layernorm_bwd = spy_fwd, spy_bwd
    try:
        _, _, _, lh, gh, lo, go = _one_shot_case(vited, gpu, dtype, s, 8, seed=0)
    finally:
        ops.linear_residual_layernorm_fwd, ops.linear_layernorm_bwd = real_fwd, real_bwd
    if dtype == torch.bfloat16:
        assert ops.linear_layernorm_supported(8 * s.n1, s.embed_dim, s.embed_dim, dtype)
        assert ops.linear_layernorm_supported(8 * s.n2, s.embed_dim, s.hidden, dtype)
        assert seen['fwd'] >= 10 and seen['bwd'] >= 10, seen          # the scaled row-complete kernels really carried the run
    else:
        assert seen == {'fwd': 0, 'bwd': 0}
    _check_values(dtype, lh, gh, lo, go)


@pytest.mark.parametrize('dtype', DTYPES)
def test_width_192_takes_the_tile_kernel_epilogue(vited, gpu, dtype):
    """D = 192, 6 heads: outside the row-complete kernel, so VITED_EPI_RESIDUAL of the tile kernels (bf16) / the portable GEMM (fp32)
    carries the scale and vited_layernorm_bwd_scaled the backward's copies."""
    s = vo.ViTEDShape(embed_dim=192, num_heads=6, depth=2, c_depth=2)
    ops = vited.ops
    assert not ops.linear_layernorm_supported(8 * s.n1, s.embed_dim, s.embed_dim, torch.bfloat16)
    paths = []                                      # which GEMM carried each scaled residual epilogue: 2 = MFMA tile kernel, 1 = portable
    real_gemm, real_ln_bwd = ops.gemm, ops.layernorm_bwd
    scaled_ln_bwd = [0]

    def spy_gemm(*a, **k):
        out = real_gemm(*a, **k)
        if k.get('row_scale') is not None:
            paths.append(ops.last_paths()[0])
        return out

    def spy_ln_bwd(*a, **k):
        scaled_ln_bwd[0] += k.get('lp_scale') is not None
        return real_ln_bwd(*a, **k)

    ops.gemm, ops.layernorm_bwd = spy_gemm, spy_ln_bwd
    try:
        _, _, _, lh, gh, lo, go = _one_shot_case(vited, gpu, dtype, s, 8, seed=1)
    finally:
        ops.gemm, ops.layernorm_bwd = real_gemm, real_ln_bwd
    # every residual Linear of the 2 + 2 blocks (2 + 2 in the encoder, 3 + 3 in the decoder) went through the scaled epilogue of
    # the kernel this test is about.  The copy that each of the 10 branches reads in the backward comes from the scaled LayerNorm
    # backward, except the one of the encoder's last branch: the cast at the head of EncoderFn.backward writes that
    assert len(paths) >= 10 and set(paths) == {2 if dtype == torch.bfloat16 else 1}, paths
    assert scaled_ln_bwd[0] >= 9, scaled_ln_bwd
    _check_values(dtype, lh, gh, lo, go)


@pytest.mark.parametrize('dtype', DTYPES)
def test_last_decoder_block_on_all_rows(vited, gpu, dtype):
    """With the cls-rows-only form of the last decoder block switched off, the head of the decoder's backward writes the cls rows
    of a zero-filled stream gradient and of its scaled low-precision copy (a scaled fp32 copy on the exact path)."""
    s = vo.ViTEDShape(depth=2, c_depth=2)

    def all_rows(model):
        model.runtime().cls_tail = False

    model, _, _, lh, gh, lo, go = _one_shot_case(vited, gpu, dtype, s, 8, seed=3, prepare=all_rows)
    assert model.runtime().cls_tail is False
    _check_values(dtype, lh, gh, lo, go)


@pytest.mark.parametrize('dtype', DTYPES)
def test_two_stage_with_gathered_pairs(vited, gpu, dtype):
    """The two-stage step: the encoder on 3 images with its own scales, the decoder on 5 pairs gathered from them by index with
    theirs (256 / 257 tokens, head dim 64).  With gradients through torch's gathers, and the no-grad form that gathers image 2
    inside the patch-embedding kernel (x2_index)."""
    s = vo.ViTEDShape(img_size=256, patch_size=16, num_classes=1, num_heads=6, depth=2, c_depth=2)
    torch.manual_seed(2)
    oracle = vo.OracleViTED(s)
    model = _hip_model(vited, s, gpu, dtype, rate=0.5, state=oracle.state_dict()).train()
    imgs = torch.randn(3, 3, 256, 256).clamp(-1, 1)
    i_idx, j_idx = torch.tensor([0, 2, 1, 2, 0]), torch.tensor([1, 0, 2, 2, 1])
    y = (torch.rand(5, 1) > 0.5).float()
    enc = dc.irregular_scales(0.5, s.depth, 2, 3, salt=7)
    dec = dc.irregular_scales(0.5, s.c_depth, 3, 5, salt=9)
    lo = dc.decoder_scaled(oracle, dc.encoder_scaled(oracle, imgs, enc)[i_idx], imgs[j_idx], dec)
    _, go = dc.loss_and_grads(oracle, lo, y)
    g_imgs, gi, gj = imgs.to(gpu), i_idx.to(gpu), j_idx.to(gpu)
    feats = model(g_imgs, forward_first_part=True, drop_path=vited.DropPathScales(enc.to(gpu), None))
    lh = model(feats[gi], g_imgs[gj], drop_path=vited.DropPathScales(None, dec.to(gpu)))
    BCE(lh, y.to(gpu)).backward()
    _check_values(dtype, lh.detach().cpu(), _grads(model), lo.detach(), go)
    with torch.no_grad():
        feats = model(g_imgs, forward_first_part=True, drop_path=vited.DropPathScales(enc.to(gpu), None))
        l2 = model(feats[gi], g_imgs, x2_index=gj, drop_path=vited.DropPathScales(None, dec.to(gpu)))
    _check_values(dtype, l2.cpu(), {}, lo.detach(), {})


def _pair_of_models(vited, gpu, dtype, s, seed, rate=0.5):
    torch.manual_seed(seed)
    state = vo.OracleViTED(s).state_dict()
    return _hip_model(vited, s, gpu, dtype, rate=rate, state=state).train(), _hip_model(vited, s, gpu, dtype, rate=0., state=state).train()


def _batch(s, batch, gpu, seed=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, 2, 3, s.img_size, s.img_size, generator=g).clamp(-1, 1).to(gpu)
    return x, (torch.rand(batch, s.num_classes, generator=g) > 0.7).float().to(gpu)


def _run(model, x, y, drop=None):
    model.zero_grad(set_to_none=True)
    logits = model(x, drop_path=drop)
    BCE(logits, y).backward()
    return logits.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize('dtype', DTYPES)
def test_unit_scales_are_the_model_without_drop_path(vited, gpu, dtype):
    """All scales 1.0, through the scaled kernels: bit for bit the logits and gradients of the rate-0 model."""
    s = vo.ViTEDShape(depth=2, c_depth=2)
    dropped, plain = _pair_of_models(vited, gpu, dtype, s, seed=5)
    x, y = _batch(s, 8, gpu)
    ones = vited.DropPathScales(torch.ones(2, 2, 8, device=gpu), torch.ones(2, 3, 8, device=gpu))
    l1, g1 = _run(dropped, x, y, ones)
    l0, g0 = _run(plain, x, y)
    assert plain.last_drop_path is None and torch.equal(l1, l0)
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n


@pytest.mark.parametrize('dtype', DTYPES)
def test_scale_two_is_doubled_branch_weights(vited, gpu, dtype):
    """keep = 0.5 with everyone kept (scale 2 on the blocks that drop) == the rate-0 model whose proj, cross-proj and fc2 weights and
    biases of those blocks are doubled: equal logits, exactly twice the gradient on those parameters, equal gradients elsewhere -
    a power of two commutes with every rounding on the way."""
    s = vo.ViTEDShape(depth=2, c_depth=2)
    dropped, plain = _pair_of_models(vited, gpu, dtype, s, seed=6)
    assert dropped.drop_path_probs == ([0., 0.5], [0., 0.5])
    doubled = [f'{blocks}.1.{lin}.{wb}' for blocks, lins in (('blocks', ('attn.proj', 'mlp.fc2')),
                                                            ('cross_blocks', ('attn.proj', 'cross_attn.proj', 'mlp.fc2')))
               for lin in lins for wb in ('weight', 'bias')]
    with torch.no_grad():
        params = dict(plain.named_parameters())
        for n in doubled:
            params[n].mul_(2.0)
    x, y = _batch(s, 8, gpu)
    enc, dec = torch.ones(2, 2, 8, device=gpu), torch.ones(2, 3, 8, device=gpu)
    enc[1], dec[1] = 2.0, 2.0
    l1, g1 = _run(dropped, x, y, vited.DropPathScales(enc, dec))
    l0, g0 = _run(plain, x, y)
    assert torch.equal(l1, l0)
    for n in g0:
        assert torch.equal(g1[n], 2.0 * g0[n] if n in doubled else g0[n]), n


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_fully_dropped_branch_has_zero_gradients(vited, gpu, dtype):
    s = vo.ViTEDShape(depth=2, c_depth=2)
    dropped, _ = _pair_of_models(vited, gpu, dtype, s, seed=7)
    x, y = _batch(s, 8, gpu)
    enc = dc.irregular_scales(0.5, 2, 2, 8, salt=11).to(gpu)
    dec = dc.irregular_scales(0.5, 2, 3, 8, salt=13).to(gpu)
    enc[1, 1], dec[0, 0], dec[1, 2] = 0., 0., 0.          # encoder block 1 MLP, decoder block 0 self-attention, decoder block 1 MLP (cls rows only)
    _, g = _run(dropped, x, y, vited.DropPathScales(enc, dec))
    mlp = ('norm2.weight', 'norm2.bias', 'mlp.fc1.weight', 'mlp.fc1.bias', 'mlp.fc2.weight', 'mlp.fc2.bias')
    attn = ('norm1.weight', 'norm1.bias', 'attn.qkv.weight', 'attn.qkv.bias', 'attn.proj.weight', 'attn.proj.bias')
    dead = [f'blocks.1.{k}' for k in mlp] + [f'cross_blocks.0.{k}' for k in attn] + [f'cross_blocks.1.{k}' for k in mlp]
    for n in dead:
        assert int(torch.count_nonzero(g[n])) == 0, n
    live = [n for n in g if n not in dead and int(torch.count_nonzero(g[n])) == 0]
    assert not live, f'gradients that should be live are all zero: {live}'


@pytest.mark.parametrize('dtype', DTYPES)
def test_eval_mode_is_the_model_without_drop_path(vited, gpu, dtype):
    s = vo.ViTEDShape(depth=2, c_depth=2)
    dropped, plain = _pair_of_models(vited, gpu, dtype, s, seed=8, rate=0.3)
    x, _ = _batch(s, 8, gpu)
    with torch.no_grad():
        assert torch.equal(dropped.eval()(x), plain.eval()(x))
    assert dropped.last_drop_path is None
    with torch.no_grad():
        dropped.train()(x)
    enc, dec = dropped.last_drop_path                         # training mode draws, for the batch of the call
    assert enc.shape == (2, 2, 8) and dec.shape == (2, 3, 8) and enc.is_cuda
    inv = (torch.ones(()) / torch.tensor(1.0 - dropped.drop_path_probs[0][1])).item()
    assert bool((enc[0] == 1).all()) and set(enc[1].unique().tolist()) <= {0., inv} and set(dec[1].unique().tolist()) <= {0., inv}


@pytest.mark.parametrize('dtype', DTYPES)
def test_no_grad_forward_honours_forced_scales(vited, gpu, dtype):
    """Training mode under no_grad: the forward must not take the one-kernel inference MLP, which does not know the scale."""
    s = vo.ViTEDShape(depth=3, c_depth=3)
    torch.manual_seed(9)
    oracle = vo.OracleViTED(s)
    model = _hip_model(vited, s, gpu, dtype, rate=0.5, state=oracle.state_dict()).train()
    x = torch.randn(8, 2, 3, 64, 64).clamp(-1, 1)
    enc, dec = dc.irregular_scales(0.5, 3, 2, 8, salt=15), dc.irregular_scales(0.5, 3, 3, 8, salt=17)
    with torch.no_grad():
        lo = dc.forward_scaled(oracle, x, enc, dec)
        lh = model(x.to(gpu), drop_path=vited.DropPathScales(enc.to(gpu), dec.to(gpu)))
    _check_values(dtype, lh.cpu(), {}, lo, {})


def _train_steps(vited, gpu, s, state, use_graph):
    m = _hip_model(vited, s, gpu, None, rate=0.5, state=state).train()
    opt = vited.optim.FlatAdamW(vited.engine.param_groups_no_decay_1d(m), lr=1e-3, weight_decay=0.05)
    return m, vited.engine.TrainStep(m, opt, clip_grad=5.0, amp=True, use_graph=use_graph)


def test_train_step_captured_equals_eager_with_forced_scales(vited, gpu):
    """Config-A geometry, 3 + 3 blocks, B = 16, bf16: two eager warm-up steps, then three replays of the captured graphs, against the
    eagerly launched step - the same loss at every step and the same parameters at the end, bit for bit."""
    s = vo.ViTEDShape(depth=3, c_depth=3)
    torch.manual_seed(10)
    state = vo.OracleViTED(s).state_dict()
    (me, eager), (mg, graph) = _train_steps(vited, gpu, s, state, False), _train_steps(vited, gpu, s, state, True)
    enc, dec = dc.irregular_scales(0.5, 3, 2, 16, salt=19).to(gpu), dc.irregular_scales(0.5, 3, 3, 16, salt=21).to(gpu)
    eager.drop_path = graph.drop_path = vited.DropPathScales(enc, dec)
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
    """Drawn scales under capture: the draw is part of the graph (the device's default generator), so consecutive replays leave
    different scales in the static ``last_drop_path`` (the last blocks drop with p = 0.5: (2 + 3) x 16 = 80 fair draws, two replays
    agree with probability 2^-80 at most) and the loss stays finite."""
    s = vo.ViTEDShape(depth=3, c_depth=3)
    torch.manual_seed(11)
    m, step = _train_steps(vited, gpu, s, vo.OracleViTED(s).state_dict(), True)
    g = torch.Generator().manual_seed(13)
    seen = []
    for it in range(5):
        x = torch.randn(16, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)
        y = (torch.rand(16, 4, generator=g) > 0.6).float().to(gpu)
        loss = step.step(x, y)
        assert bool(torch.isfinite(loss)), it
        seen.append(torch.cat([t.reshape(-1) for t in m.last_drop_path]).clone())
    assert step._g1 is not None
    assert seen[-1].numel() == (3 * 2 + 3 * 3) * 16
    assert not torch.equal(seen[-1], seen[-2]) and not torch.equal(seen[-2], seen[-3])      # replays 3, 2 and 1
    static = m.last_drop_path
    step.step(x, y)
    assert m.last_drop_path.enc is static.enc and m.last_drop_path.dec is static.dec          # a static buffer, rewritten by the replay


def test_constructor_and_training_forward(vited, gpu):
    """What fails at the constructor without the feature: a model built with a live rate trains."""
    s = vo.ViTEDShape(depth=2, c_depth=2)
    torch.manual_seed(14)
    model = _hip_model(vited, s, gpu, torch.bfloat16, rate=0.1).train()
    x, y = _batch(s, 8, gpu)
    loss = BCE(model(x), y)
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert model.last_drop_path.enc.shape == (2, 2, 8) and model.last_drop_path.dec.shape == (2, 3, 8)
