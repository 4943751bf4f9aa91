"""Position dropout on the MI355X: the kernel of csrc/token_dropout.hip against the same rule on CPU tensors, bit for bit, and the model
with FORCED seeds against the composition of tests/posdrop_cases.py (pinned to the reference by tests/test_posdrop.py) driven by the
masks ``ops.token_dropout_mask`` gives for those seeds.

Tolerances of the value tests are those of tests/test_gpu_droppath.py::_check_values, the same method on the same kind of init."""
import os

import pytest
import torch

import droppath_cases as dc
import patchdrop_cases as pc
import posdrop_cases as pd
import qknorm_cases as qc
from oracle import vited_oracle as vo
from test_gpu_droppath import _check_values

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
BCE = torch.nn.functional.binary_cross_entropy_with_logits
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
def _values(shape, dtype, mask, seed):
    """Signed values with one inf in a dropped position (it must come out 0)."""
    x = (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 3).to(dtype)
    dropped = (~mask).nonzero()
    if len(dropped):
        x[tuple(dropped[len(dropped) // 2])] = float('inf')
    return x


def _seed(value, gpu):
    return torch.tensor([value], dtype=torch.int64, device=gpu)


def _nan_like(t):
    return torch.full_like(t, float('nan'))


@pytest.mark.parametrize('stream', [0, 1])
@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(3, 5, 36), (2, 65, 384), (1, 3, 1024)])
def test_kernel_is_the_cpu_rule(vited, gpu, shape, dtype, p, stream):
    """[3, 5, 36]: dim % 8 != 0 and fewer elements than one wave; [2, 65, 384]: an odd row count, config A's decoder stream; [1, 3,
    1024]: the widest row.  Out of place into a NaN-filled buffer and in place, both equal to the CPU op exactly."""
    ops = vited.ops
    seed = -(2 ** 62) + 1000 * shape[2] + stream
    mask = ops.token_dropout_mask(seed, p, *shape, stream)
    x = _values(shape, dtype, mask, seed=shape[1])
    want = ops.token_dropout(x, seed, p, shape[1], stream)
    assert int(torch.count_nonzero(want[~mask])) == 0 and bool(torch.isinf(x).any())
    xg, sg = x.to(gpu), _seed(seed, gpu)
    out = _nan_like(xg)
    got = ops.token_dropout(xg, sg, p, shape[1], stream, out=out)
    assert got is out and got.dtype == dtype and torch.equal(got.cpu(), want)
    assert torch.equal(xg.cpu(), x)                                                     # the input is left alone
    fresh = ops.token_dropout(xg, sg, p, shape[1], stream)
    assert fresh.data_ptr() != xg.data_ptr() and torch.equal(fresh.cpu(), want)
    same = ops.token_dropout(xg, sg, p, shape[1], stream, out=xg)                        # in place
    assert same is xg and torch.equal(xg.cpu(), want)


@pytest.mark.parametrize('dtype', DTYPES)
def test_kernel_on_strided_operands(vited, gpu, dtype):
    """A row stride wider than dim (a column slice), a batch-strided view (every other sample), and a strided destination whose gaps
    stay untouched."""
    ops = vited.ops
    seed, p = 424242, 0.5
    mask = ops.token_dropout_mask(seed, p, 2, 7, 40, 1)
    x = _values((2, 7, 40), dtype, mask, seed=3)
    want = ops.token_dropout(x, seed, p, 7, 1)
    sg = _seed(seed, gpu)
    wide = torch.zeros(2, 7, 56, dtype=dtype, device=gpu)
    wide[..., 8:48] = x.to(gpu)
    assert torch.equal(ops.token_dropout(wide[..., 8:48], sg, p, 7, 1).cpu(), want)
    every_other = torch.zeros(4, 7, 40, dtype=dtype, device=gpu)
    every_other[::2] = x.to(gpu)
    assert torch.equal(ops.token_dropout(every_other[::2], sg, p, 7, 1).cpu(), want)
    dest = _nan_like(wide)
    ops.token_dropout(every_other[::2], sg, p, 7, 1, out=dest[..., 8:48])
    assert torch.equal(dest[..., 8:48].cpu(), want) and bool(dest[..., :8].isnan().all()) and bool(dest[..., 48:].isnan().all())
    view = wide[..., 8:48]
    ops.token_dropout(view, sg, p, 7, 1, out=view)                                       # in place on the strided view
    assert torch.equal(view.cpu(), want) and int(torch.count_nonzero(wide[..., :8])) == 0 and int(torch.count_nonzero(wide[..., 48:])) == 0
    with pytest.raises((ValueError, RuntimeError), match='token_dropout'):
        ops.token_dropout(wide[..., 8:48], sg, p, 7, 1, out=wide[..., 12:52])           # overlapping, not in place


@pytest.mark.parametrize('lead', [False, True])
@pytest.mark.parametrize('dtype', DTYPES)
def test_kernel_under_a_keep_table(vited, gpu, dtype, lead):
    """A table [2, 3] over 9 tokens: row 0 is the prefix token, row r the token of the kept patch, each with the mask of its original
    position - the gathered rows of the full stream's result."""
    ops = vited.ops
    seed, p, stream = 77, 0.5, int(not lead)
    keep = torch.tensor([[5, 0, 7], [2, 6, 3]])
    mask = ops.token_dropout_mask(seed, p, 2, 9, 36, stream)
    x = _values((2, 9, 36), dtype, mask, seed=5)
    want = pc.gather_kept(ops.token_dropout(x, seed, p, 9, stream), keep)
    assert torch.equal(ops.token_dropout(pc.gather_kept(x, keep), seed, p, 9, stream, keep=keep, lead=lead), want)       # the CPU rule
    rows = pc.gather_kept(x, keep).to(gpu)
    for table in (keep.to(gpu), keep.to(gpu).int()):
        out = _nan_like(rows)
        ops.token_dropout(rows, _seed(seed, gpu), p, 9, stream, keep=table, lead=lead, out=out)
        assert torch.equal(out.cpu(), want)


# ---- the model against the composition ------------------------------------------------------------------------------------------------
def _hip_model(vited, s, gpu, dtype, state=None, **kw):
    m = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                      embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads,
                                      mlp_ratio=s.mlp_ratio, qkv_bias=s.qkv_bias, **kw)
    m.compute_dtype = dtype
    if state is not None:
        m.load_state_dict(state)
    return m.to(gpu)


def _grads(m):
    return {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()}


def _run(model, x, y, **kw):
    model.zero_grad(set_to_none=True)
    logits = model(x, **kw)
    BCE(logits, y).backward()
    return logits.detach().cpu(), _grads(model)


def _seeds(vited, gpu, a, b):
    return vited.PosDropSeeds(None if a is None else _seed(a, gpu), None if b is None else _seed(b, gpu))


def _differs(dtype, lh, lo):
    """True where ``lh`` misses ``lo`` by more than _check_values' logits tolerance."""
    rtol, atol = (1e-3, 1e-5) if dtype == torch.float32 else (3e-2, 3e-2)
    return bool(((lh - lo).abs() > atol + rtol * lo.abs()).any())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', sorted(pd.GOLDEN_SHAPES))
def test_model_against_the_composition(vited, gpu, dtype, name):
    """The fixture's geometries (1 + 1 and 2 + 3 blocks) at rate 0.5, B = 4: logits and every parameter gradient with forced seeds
    against the oracle under the rule's masks; and the masks matter - the oracle without them is further away than the tolerance."""
    s, rate, batch = pd.GOLDEN_SHAPES[name], 0.5, 4
    torch.manual_seed(40)
    oracle = vo.OracleViTED(s)
    model = _hip_model(vited, s, gpu, dtype, state=oracle.state_dict(), pos_drop_rate=rate).train()
    x = torch.randn(batch, 2, 3, s.img_size, s.img_size).clamp(-1, 1)
    y = (torch.rand(batch, s.num_classes) > 0.6).float()
    seeds = (31337, -(2 ** 63) + 12345)
    mask1, mask2, scale = pd.masks_of(vited.ops, seeds, rate, batch, batch, s)
    lo = pd.forward_dropped(oracle, x, mask1, mask2, scale)
    _, go = pd.loss_and_grads(oracle, lo, y)
    forced = _seeds(vited, gpu, *seeds)
    lh, gh = _run(model, x.to(gpu), y.to(gpu), pos_drop=forced)
    assert model.last_pos_drop.x1 is forced.x1 and model.last_pos_drop.x2 is forced.x2
    _check_values(dtype, lh, gh, lo.detach(), go)
    plain = oracle(x).detach()
    print(f'{dtype}: the oracle without dropout is max|d| = {float((lh - plain).abs().max()):.3e} away')
    assert _differs(dtype, lh, plain)
    if dtype == torch.float32:                                                         # the features alone, first stage
        feats = model(x[:, 0].to(gpu), forward_first_part=True, pos_drop=_seeds(vited, gpu, seeds[0], None))
        torch.testing.assert_close(feats.detach().cpu(), pd.encoder_dropped(oracle, x[:, 0], mask1, scale).detach(), rtol=1e-3, atol=1e-4)


SHAPE_A2 = vo.ViTEDShape(depth=2, c_depth=2)                                            # config-A geometry, 2 + 2 blocks


def _batch(s, batch, gpu, seed=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, 2, 3, s.img_size, s.img_size, generator=g).clamp(-1, 1).to(gpu)
    return x, (torch.rand(batch, s.num_classes, generator=g) > 0.7).float().to(gpu)


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_shot_and_two_stage_agree_bit_for_bit(vited, gpu, dtype):
    s = SHAPE_A2
    torch.manual_seed(41)
    model = _hip_model(vited, s, gpu, dtype, state=vo.OracleViTED(s).state_dict(), pos_drop_rate=0.5).train()
    x, y = _batch(s, 4, gpu)
    forced = _seeds(vited, gpu, 5, 6)
    l0, g0 = _run(model, x, y, pos_drop=forced)
    model.zero_grad(set_to_none=True)
    feats = model(x[:, 0], forward_first_part=True, pos_drop=vited.PosDropSeeds(forced.x1, None))
    logits = model(feats, x[:, 1], pos_drop=vited.PosDropSeeds(None, forced.x2))
    BCE(logits, y).backward()
    assert model.last_pos_drop.x1 is forced.x1 and model.last_pos_drop.x2 is forced.x2
    g1 = _grads(model)
    assert torch.equal(logits.detach().cpu(), l0)
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n
    # another seed gives other logits: the seed is read
    l2, _ = _run(model, x, y, pos_drop=_seeds(vited, gpu, 5, 7))
    assert not torch.equal(l2, l0)


@pytest.mark.parametrize('dtype', DTYPES)
def test_pair_indexed_form_matches_the_gathered_form(vited, gpu, dtype):
    """4 images, 7 pairs: model(feats, x2, x2_index=j, x1_index=i) drops per PAIR (the row of the pair list), as the gathered form
    model(feats[i], x2[j]) does.  Held to _check_values, the figure tests/test_gpu_pair_index.py holds the indexed form to."""
    s = SHAPE_A2
    torch.manual_seed(42)
    model = _hip_model(vited, s, gpu, dtype, state=vo.OracleViTED(s).state_dict(), pos_drop_rate=0.5).train()
    imgs = torch.randn(4, 3, 64, 64).clamp(-1, 1).to(gpu)
    gi, gj = torch.tensor([1, 3, 1, 2, 3, 3, 1], device=gpu), torch.tensor([0, 1, 2, 0, 2, 3, 3], device=gpu)
    y = (torch.rand(7, s.num_classes) > 0.5).float().to(gpu)
    forced = _seeds(vited, gpu, 15, 16)

    def two_stage(indexed):
        model.zero_grad(set_to_none=True)
        feats = model(imgs, forward_first_part=True, pos_drop=vited.PosDropSeeds(forced.x1, None))
        second = vited.PosDropSeeds(None, forced.x2)
        logits = model(feats, imgs, x2_index=gj, x1_index=gi, pos_drop=second) if indexed else model(feats[gi], imgs[gj], pos_drop=second)
        BCE(logits, y).backward()
        return logits.detach().cpu(), _grads(model)

    _check_values(dtype, *two_stage(True), *two_stage(False))


@pytest.mark.parametrize('dtype', DTYPES)
def test_with_patch_dropout_drop_path_and_qk_norm(vited, gpu, dtype):
    """Forced keep tables, forced stochastic-depth scales and q/k-norm beside forced seeds: the kept rows carry the masks of their
    original tokens (timm drops before it selects)."""
    s = SHAPE_A2
    torch.manual_seed(43)
    oracle = qc.randomize_norms_(qc.QKNormViTED(s), torch.Generator().manual_seed(44))
    model = _hip_model(vited, s, gpu, dtype, state=oracle.state_dict(), pos_drop_rate=0.5, patch_drop_rate=0.5, drop_path_rate=0.5,
                       qk_norm=True).train()
    x = torch.randn(8, 2, 3, 64, 64).clamp(-1, 1)
    y = (torch.rand(8, s.num_classes) > 0.6).float()
    keep1 = pc.closed_form_keep(8, s.n1 - 1, pc.keep_count(s.n1 - 1, 0.5), 1)
    keep2 = pc.closed_form_keep(8, s.n1, pc.keep_count(s.n1, 0.5), 2)
    enc, dec = dc.irregular_scales(0.5, s.depth, 2, 8, salt=3), dc.irregular_scales(0.5, s.c_depth, 3, 8, salt=5)
    seeds = (2 ** 40 + 3, -5)
    mask1, mask2, scale = pd.masks_of(vited.ops, seeds, 0.5, 8, 8, s)
    lo = pd.forward_dropped(oracle, x, mask1, mask2, scale, keep1, keep2, enc, dec)
    _, go = pd.loss_and_grads(oracle, lo, y)
    lh, gh = _run(model, x.to(gpu), y.to(gpu), pos_drop=_seeds(vited, gpu, *seeds), patch_keep=vited.PatchKeep(keep1.to(gpu), keep2.to(gpu)),
                  drop_path=vited.DropPathScales(enc.to(gpu), dec.to(gpu)))
    # the gradient of every k_norm.bias is zero in exact arithmetic: held, as in tests/test_gpu_patchdrop.py, to the same figure times
    # the norm of the module's weight gradient
    zero = [n for n in go if n.endswith('k_norm.bias')]
    for n in zero:
        bound = (1e-3 if dtype == torch.float32 else 5e-2) * float(go[n.replace('.bias', '.weight')].norm())
        assert float(gh[n].norm()) <= bound, n
    _check_values(dtype, lh, {n: g for n, g in gh.items() if n not in zero}, lo.detach(), {n: g for n, g in go.items() if n not in zero})


@pytest.mark.parametrize('dtype', DTYPES)
def test_off_is_the_model_without_the_option(vited, gpu, dtype):
    s = SHAPE_A2
    torch.manual_seed(45)
    state = vo.OracleViTED(s).state_dict()
    plain = _hip_model(vited, s, gpu, dtype, state=state).train()
    zero = _hip_model(vited, s, gpu, dtype, state=state, pos_drop_rate=0.).train()
    live = _hip_model(vited, s, gpu, dtype, state=state, pos_drop_rate=0.3).eval()
    x, y = _batch(s, 4, gpu)
    l0, g0 = _run(plain, x, y)
    l1, g1 = _run(zero, x, y)
    assert torch.equal(l1, l0) and all(torch.equal(g1[n], g0[n]) for n in g0) and zero.last_pos_drop is None
    with torch.no_grad():
        assert torch.equal(live(x).cpu(), l0) and live.last_pos_drop is None
        # the pair caches never drop, in training mode either
        live.train()
        tokens, _ = live.cache_image2_tokens(x[:, 1])
        ref, _ = plain.cache_image2_tokens(x[:, 1])
        assert torch.equal(tokens, ref)
        # training mode draws: one seed per stream, on the device; and the result is another
        out = live(x)
    assert live.last_pos_drop.x1.is_cuda and live.last_pos_drop.x1.dtype == torch.int64 and live.last_pos_drop.x2.shape == (1,)
    assert not torch.equal(out.cpu(), l0)


# ---- TrainStep ------------------------------------------------------------------------------------------------------------------------
def _train_step(vited, gpu, use_graph, state=None):
    cfg = vited.config_from_yaml(os.path.join(ROOT, 'configs', 'test', 'test_pjs_hisfrag20_patch32_64.yaml'))
    m = vited.build_model(cfg, pos_drop_rate=0.1)
    if state is not None:
        m.load_state_dict(state)
    m = m.to(gpu).train()
    opt = vited.optim.FlatAdamW(vited.engine.param_groups_no_decay_1d(m), lr=1e-3, weight_decay=0.05)
    return m, vited.engine.TrainStep(m, opt, clip_grad=5.0, amp=True, use_graph=use_graph)


def _train_batch(m, g, gpu, batch=8):
    x = torch.randn(batch, 2, m.in_chans, m.img_size, m.img_size, generator=g).clamp(-1, 1).to(gpu)
    return x, (torch.rand(batch, m.num_classes, generator=g) > 0.6).float().to(gpu)


def test_train_step_replays_draw_anew(vited, gpu):
    """The draw of the seeds is part of the captured graph (the device's default generator): consecutive replays leave different seeds
    in the static ``last_pos_drop`` (two 64-bit draws agree with probability 2^-64) and the loss stays finite."""
    torch.manual_seed(50)
    m, step = _train_step(vited, gpu, True)
    g = torch.Generator().manual_seed(13)
    seen = []
    for it in range(5):
        x, y = _train_batch(m, g, gpu)
        loss = step.step(x, y)
        assert bool(torch.isfinite(loss)), it
        seen.append(torch.cat(list(m.last_pos_drop)).clone())
    assert step._g1 is not None and seen[-1].shape == (2,) and seen[-1].dtype == torch.int64
    assert not torch.equal(seen[-1], seen[-2]) and not torch.equal(seen[-2], seen[-3])      # replays 3, 2 and 1
    assert int(seen[-1][0]) != int(seen[-1][1])
    static = m.last_pos_drop
    step.step(x, y)
    assert m.last_pos_drop.x1 is static.x1 and m.last_pos_drop.x2 is static.x2              # a static buffer, rewritten by the replay


def test_train_step_captured_equals_eager_with_forced_seeds(vited, gpu):
    """Two eager warm-up steps, then three replays of the captured graphs, against the eagerly launched step: the same loss at every
    step and the same parameters at the end, bit for bit.  The forced seed tensors are static: the graphs read them in place."""
    torch.manual_seed(51)
    me, eager = _train_step(vited, gpu, False)
    mg, graph = _train_step(vited, gpu, True, state=me.state_dict())
    eager.pos_drop = graph.pos_drop = _seeds(vited, gpu, 99, -100)
    g = torch.Generator().manual_seed(12)
    for it in range(5):
        x, y = _train_batch(me, g, gpu)
        le, lg = float(eager.step(x, y)), float(graph.step(x, y))
        assert le == lg, (it, le, lg)
    assert graph._g1 is not None and mg.last_pos_drop.x1 is graph.pos_drop.x1
    for (n, pe), (_, pg) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.equal(pe, pg), n


def test_custom_generator_raises_at_capture(vited, gpu):
    torch.manual_seed(52)
    m, step = _train_step(vited, gpu, True)
    m.pos_drop_generator = torch.Generator(device=gpu).manual_seed(1)
    g = torch.Generator().manual_seed(14)
    for it in range(2):                                                                  # the eager warm-up steps draw from it
        x, y = _train_batch(m, g, gpu)
        assert bool(torch.isfinite(step.step(x, y)))
    with pytest.raises(RuntimeError, match='default generator'):
        step.step(x, y)
    torch.cuda.synchronize()


# ---- the custom operator --------------------------------------------------------------------------------------------------------------
def test_custom_op(vited, gpu):
    x = (torch.randn(2, 9, 64, generator=torch.Generator().manual_seed(1)) * 2).to(gpu)
    seed = _seed(123, gpu)
    torch.library.opcheck(torch.ops.vited.token_dropout.default, (x, seed, 0.25, 9, 1, None, False),
                          test_utils=('test_schema', 'test_faketensor', 'test_autograd_registration'))
    keep = torch.tensor([[5, 0, 7], [2, 6, 3]], device=gpu)
    torch.library.opcheck(torch.ops.vited.token_dropout.default, (x[:, :4].contiguous(), seed, 0.25, 9, 0, keep, True),
                          test_utils=('test_schema', 'test_faketensor', 'test_autograd_registration'))
    xr = x.clone().requires_grad_(True)
    y = torch.ops.vited.token_dropout(xr, seed, 0.25, 9, 1, None, False)
    assert torch.equal(y.detach().cpu(), vited.ops.token_dropout(x.cpu(), 123, 0.25, 9, 1))
    dy = torch.randn(2, 9, 64, generator=torch.Generator().manual_seed(2)).to(gpu)
    y.backward(dy)
    assert torch.equal(xr.grad, torch.ops.vited.token_dropout(dy, seed, 0.25, 9, 1, None, False))      # the op applied to the gradient
    assert torch.equal(xr.grad.cpu(), vited.ops.token_dropout(dy.cpu(), 123, 0.25, 9, 1))
