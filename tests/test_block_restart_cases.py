"""The block-restart machinery itself (tests/block_restart_cases.py), on the CPU:

  * chain rule: with no rounding and fed the fp64 whole-network oracle's own taps, the stage restarts reproduce that oracle - every
    stage output, every d(input), every parameter gradient - to 1e-10, in every layout the HIP path records (cls rows only on the
    last block, keys / values computed ahead) and for the plain, q/k-norm and pooled-head trees;
  * completeness: the stages between them own every parameter of the state_dict, once;
  * the bf16 bound (2 x the rounding model's statistic + 2^-8) lets a second, differently rounding bf16 implementation through ...
  * ... and catches each of five planted glue defects;
  * the same four properties with the options of training in the stages - stochastic-depth scales, patch dropout's keep tables,
    position dropout's masks, the gathered and the pair-indexed two-stage forms: the restarts reproduce droppath_cases' /
    patchdrop_cases' / posdrop_cases' compositions and oracle(feats[i], imgs[j]) to 1e-10, the second rounding model is admitted in
    every case the GPU test runs, whose fp64 references need no small-gradient exemption, and five defects planted in the
    implementation that records (a scale missing from a branch's gradient, the neighbouring branch's scales, d(pos_embed) one row
    off, the position mask missing from the gradient, a pair missing from an image's sum) fail at exactly the labels they touch.
"""
import pytest
import torch

import block_restart_cases as br
import droppath_cases as droppath
import patchdrop_cases as patchdrop
import posdrop_cases as posdrop
from oracle import vited_oracle as vo

SMALL = vo.ViTEDShape(img_size=32, patch_size=8, embed_dim=64, num_heads=2, depth=2, c_depth=3)      # 16 / 17 tokens
GEOMETRIES = {'A': (br.SHAPE_A, br.BATCH_A), 'long': (br.SHAPE_LONG, br.BATCH_LONG)}


def _case(s, batch, kind='plain', seed=0):
    m = br.build_tree(s, kind, seed).double()
    x, y = br.inputs(s, batch, seed)
    return m, x.double(), y.double()


def _straight_oracle(m, x, y):
    """The whole network as the oracle module runs it, untouched by the restart code: logits and parameter gradients."""
    m.zero_grad(set_to_none=True)
    logits = m(x)
    torch.nn.functional.binary_cross_entropy_with_logits(logits, y).backward()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    return logits.detach(), grads


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-300))


@pytest.mark.parametrize('kind,cls_rows,fold', [('plain', False, False), ('plain', True, False), ('plain', False, True), ('plain', True, True),
                                                ('qk', False, False), ('qk', True, True), ('pool', False, False), ('pool', False, True)])
def test_chain_rule_restarts_reproduce_the_fp64_oracle(kind, cls_rows, fold):
    m, x, y = _case(SMALL, 3, kind, seed=3)
    logits0, grads0 = _straight_oracle(m, x, y)
    taps, grads = br.network_taps(m, x, y, br.EXACT, cls_rows=cls_rows, fold=fold)
    # the tapped run IS the oracle's forward + backward
    assert _rel(taps['logits'], logits0) < 1e-12
    assert set(grads) == set(grads0)
    for n in grads0:
        assert _rel(grads[n], grads0[n]) < 1e-12, n
    assert br.layout_of(taps, SMALL) == (cls_rows, fold)
    ref = br.restart_all(m, taps, br.EXACT)
    got = br.observed(taps, grads0, SMALL)
    assert set(got) == set(ref)
    for label, (whole, rowmax), _ in br.compare(got, ref):
        assert whole < 1e-10 and (rowmax is None or rowmax < 1e-10), (label, whole, rowmax)


def test_chain_rule_at_the_a_geometry():
    s, batch = GEOMETRIES['A']
    m, x, y = _case(s, batch)
    _, grads0 = _straight_oracle(m, x, y)
    taps, _ = br.network_taps(m, x, y, br.EXACT, cls_rows=True, fold=True)
    rows = br.compare(br.observed(taps, grads0, s), br.restart_all(m, taps, br.EXACT))
    assert max(whole for _, (whole, _), _ in rows) < 1e-10
    assert max(rowmax for _, (_, rowmax), _ in rows if rowmax is not None) < 1e-10


@pytest.mark.parametrize('kind', ['plain', 'qk', 'pool'])
@pytest.mark.parametrize('fold', [False, True])
def test_the_stages_own_every_parameter(kind, fold):
    m, x, y = _case(SMALL, 2, kind)
    taps, _ = br.network_taps(m, x, y, br.EXACT, fold=fold)
    names = br.checked_parameters(br.restart_all(m, taps, br.EXACT))
    assert names == set(m.state_dict())
    spec = set(vo.state_dict_spec(SMALL))
    if kind == 'plain':
        assert names == spec
    elif kind == 'qk':
        extra = names - spec
        assert names >= spec and extra and all(n.split('.')[-2] in ('q_norm', 'k_norm') for n in extra)
    else:
        assert names == {('fc_' + n) if n.startswith('norm.') else n for n in spec}


@pytest.mark.parametrize('geometry,kind,cls_rows,fold', [('A', 'plain', True, True), ('A', 'plain', False, False), ('long', 'plain', True, True),
                                                         ('long', 'plain', False, False), ('A', 'qk', True, True), ('A', 'pool', False, True)])
def test_the_bf16_bound_admits_a_second_rounding_model(geometry, kind, cls_rows, fold):
    """MODEL2 (rounds also at LayerNorm's and GELU's output and at the gradient entering every residual branch) run as the
    implementation under test: restarted stage by stage from ITS taps, it stays inside 2 x MODEL + 2^-8 on every tensor."""
    s, batch = GEOMETRIES[geometry]
    m, x, y = _case(s, batch, kind)
    taps, grads = br.network_taps(m, x, y, br.MODEL2, cls_rows=cls_rows, fold=fold)
    ref = br.restart_all(m, taps, br.EXACT)
    assert br.exempt_labels(ref) == []
    rows = br.compare(br.observed(taps, grads, s), ref, br.restart_all(m, taps, br.MODEL))
    print(br.table(rows))
    assert br.failures(rows) == []


# ----------------------------------------------------------------------------------------------------------------------------
# the stages with the training options: drop path, patch dropout, position dropout, the two-stage forms
# ----------------------------------------------------------------------------------------------------------------------------
#         form        tree     what the options are made of                          two calls
FORMS = {'droppath':  ('plain', dict(drop_path=0.2),                                  None),
         'patchdrop': ('plain', dict(patch_drop=0.25),                                None),
         'posdrop':   ('plain', dict(pos_drop=0.1),                                   None),
         'all-qk':    ('qk',    dict(drop_path=0.2, patch_drop=0.25, pos_drop=0.1),   None),
         'gathered':  ('plain', dict(),                                               'gathered'),
         'indexed':   ('plain', dict(),                                               'indexed')}


def _small_case(form, ops):
    """(tree fp64, x1, x2, y, Options, images or None for a one-shot form) of ``form`` at SMALL: 16 / 17 tokens (11 + 1 / 12 + 1 kept)."""
    kind, what, calls = FORMS[form]
    m = br.build_tree(SMALL, kind, seed=3).double()
    if calls is None:
        x, y = br.inputs(SMALL, 3, seed=3)
        return m, x[:, 0].double(), x[:, 1].double(), y.double(), br.make_options(SMALL, 3, ops=ops, **what), None
    images, index, x2_index = br.PAIRS_A
    imgs, y = br.pair_inputs(SMALL, images, len(index), seed=3)
    opt = br.make_options(SMALL, images, len(index), ops=ops, index=index, x2_index=x2_index, indexed=calls == 'indexed', **what)
    return m, imgs.double(), imgs[opt.x2_index].double(), y.double(), opt, imgs.double()


def _straight_composition(m, x1, x2, y, opt, imgs, ops):
    """The whole network as the option's own case module composes it, untouched by the restart code: logits and parameter gradients."""
    x = torch.stack((x1, x2), 1) if imgs is None else None
    enc, dec = (None, None) if opt.enc is None else (opt.enc.double(), opt.dec.double())
    m.zero_grad(set_to_none=True)
    if imgs is not None:
        logits = m(m(imgs, forward_first_part=True)[opt.index], imgs[opt.x2_index])      # oracle(feats[i], imgs[j]), the encoder on the images
    elif opt.mult1 is not None:
        mask1, mask2, scale = posdrop.masks_of(ops, opt.seeds, opt.pos_rate, x1.shape[0], x2.shape[0], SMALL)
        logits = posdrop.forward_dropped(m, x, mask1, mask2, scale, opt.keep1, opt.keep2, enc, dec)
    elif opt.keep1 is not None:
        logits = patchdrop.forward_kept(m, x, opt.keep1, opt.keep2)
    else:
        logits = droppath.forward_scaled(m, x, enc, dec)
    _, grads = droppath.loss_and_grads(m, logits, y)
    m.zero_grad(set_to_none=True)
    return logits.detach(), grads


@pytest.mark.parametrize('cls_rows,fold', [(False, False), (True, True)])
@pytest.mark.parametrize('form', list(FORMS))
def test_restarts_under_the_options_reproduce_the_fp64_composition(vited, form, cls_rows, fold):
    m, x1, x2, y, opt, imgs = _small_case(form, vited.ops)
    logits0, grads0 = _straight_composition(m, x1, x2, y, opt, imgs, vited.ops)
    taps, grads = br.network_taps(m, (x1, x2), y, br.EXACT, cls_rows=cls_rows, fold=fold, opt=opt)
    # the tapped run IS the composition's forward + backward
    assert _rel(taps['logits'], logits0) < 1e-12
    assert set(grads) == set(grads0) == {n for n, _ in m.named_parameters()}
    for n in grads0:
        if not n.endswith('k_norm.bias'):        # zero in exact arithmetic (block_restart_cases.scale_of): two runs' rounding noise
            assert _rel(grads[n], grads0[n]) < 1e-10, n
    assert br.layout_of(taps, SMALL) == (cls_rows, fold)
    if opt.keep1 is not None:
        assert taps['enc.in'].shape[1] == 12 and taps['dec.in'].shape[1] == 13      # 1 + 11 of 16 and 1 + 12 of 17 tokens
    ref = br.restart_all(m, taps, br.EXACT, opt)
    got = br.observed(taps, grads0, SMALL)
    assert set(got) == set(ref)
    assert br.checked_parameters(ref) == set(m.state_dict())       # the stages still own every parameter, once (_take_grads)
    for label, (whole, rowmax), _ in br.compare(got, ref):
        assert whole < 1e-10 and (rowmax is None or rowmax < 1e-10), (label, whole, rowmax)
    # what the encoder received is the decoder's d(features): summed over the pairs by autograd, or per image already
    assert _rel(taps[f'enc.dx.{SMALL.depth}'], br.features_gradient(taps, SMALL, opt, dtype=torch.float64)) < 1e-14
    if opt.index is not None:
        items = 5 if opt.indexed else 12
        assert ref['context.dfeats'].shape[0] == ref[f'dec1.{"dkv" if fold else "dctx"}'].shape[0] == items
    if opt.indexed:
        unread = sorted(set(range(5)) - set(opt.index.tolist()))
        assert unread == [2] and torch.bincount(opt.index).tolist() == [3, 2, 0, 5, 2]
        assert not bool(ref['context.dfeats'][2].any()) and bool(ref['context.dfeats'][[0, 1, 3, 4]].flatten(1).any(1).all())


#          every case of the GPU test's option table in the layout its bf16 run has ...
ADMITTED = [(c[0], c[4].get('cls_tail', True), c[4].get('fold_context', True)) for c in br.OPTION_CASES]
#          ... and each kind of option once more with every row of the last block live and the d(context) terms per block (the fp32 runs' layout)
ADMITTED += [(name, False, False) for name in ('droppath', 'patchdrop', 'posdrop', 'all-qk_norm', 'two-stage', 'indexed')]


@pytest.mark.parametrize('name,cls_rows,fold', ADMITTED)
def test_the_bf16_bound_admits_a_second_rounding_model_under_the_options(vited, name, cls_rows, fold):
    """Every case of tests/test_gpu_block_restart.py's option table at its own geometry, with MODEL2 as the implementation: inside
    2 x MODEL + 2^-8 on every tensor.  And the fp64 reference needs no small-gradient exemption."""
    kind, s, images, pairs, switches, opt, (x1, x2, y) = br.option_case(name, vited.ops)
    m = br.build_tree(s, kind).double()
    taps, grads = br.network_taps(m, (x1.double(), x2.double()), y.double(), br.MODEL2, cls_rows=cls_rows, fold=fold, opt=opt)
    ref = br.restart_all(m, taps, br.EXACT, opt)
    assert br.exempt_labels(ref) == []
    rows = br.compare(br.observed(taps, grads, s), ref, br.restart_all(m, taps, br.MODEL, opt))
    print(br.table(rows))
    assert br.failures(rows) == []


class _ForwardOnly(torch.autograd.Function):
    """t * mult in the forward; the gradient comes back multiplied by ``back`` instead."""

    @staticmethod
    def forward(ctx, t, mult, back):
        ctx.back = back
        return t * mult

    @staticmethod
    def backward(ctx, g):
        return g * ctx.back, None, None


class _GatherLosingAPair(torch.autograd.Function):
    """kv[index]; the backward's per-image sum leaves pair ``skip`` out."""

    @staticmethod
    def forward(ctx, kv, index, skip):
        ctx.index, ctx.skip, ctx.items = index, skip, kv.shape[0]
        return kv[index]

    @staticmethod
    def backward(ctx, g):
        g = g.clone()
        g[ctx.skip] = 0
        return torch.zeros((ctx.items,) + tuple(g.shape[1:]), dtype=g.dtype).index_add_(0, ctx.index, g), None, None


def _failing(vited, name, stages=None, alter=None, cls_rows=False, fold=False):
    """The labels at which MODEL, run as the implementation of option case ``name`` with a defect planted in it (``stages(m, opt)``:
    replacement stages; ``alter(taps, grads, opt)``: what it recorded, rewritten), misses the bound - after the same implementation
    without the defect has passed everywhere.  Returns (labels, the failure lines)."""
    kind, s, images, pairs, _, opt, (x1, x2, y) = br.option_case(name, vited.ops)
    m = br.build_tree(s, kind).double()
    out = []
    for defect in (False, True):
        taps, grads = br.network_taps(m, (x1.double(), x2.double()), y.double(), br.MODEL, cls_rows=cls_rows, fold=fold, opt=opt,
                                      stages=stages(m, opt) if defect and stages else None)
        if defect and alter:
            alter(taps, grads, opt)
        rows = br.compare(br.observed(taps, grads, s), br.restart_all(m, taps, br.EXACT, opt), br.restart_all(m, taps, br.MODEL, opt))
        out.append(br.failures(rows))
    assert out[0] == []
    print('\n'.join(out[1]))
    return {line.split(': ', 1)[0] for line in out[1]}, out[1]


def _params(prefix, *names):
    return {f'g:{prefix}.{n}.{p}' for n in names for p in ('weight', 'bias')}


def test_planted_scale_missing_from_a_branch_gradient(vited):
    """Encoder block 1's attention branch scaled in the forward, its incoming gradient not: that block's dx and that branch's parameters
    (the MLP branch runs first in the backward and saw the right gradient)."""
    def stages(m, opt):
        def block(R, blk, x, nh, scales=None):
            if blk is not m.blocks[1]:
                return br.encoder_block(R, blk, x, nh, scales)
            a = R.branch(br.self_attention(R, blk.attn, R.ln(vo._ln(blk.norm1, x)), nh))
            x = x + _ForwardOnly.apply(a, scales[0].view(-1, 1, 1), 1.0)
            return br._add(R, x, br._mlp(R, blk.mlp, R.ln(vo._ln(blk.norm2, x))), scales, 1)
        return dict(encoder_block=block)

    labels, _ = _failing(vited, 'droppath', stages)
    assert labels == {'enc1.dx'} | _params('blocks.1', 'norm1', 'attn.qkv', 'attn.proj')


def test_planted_scales_of_the_neighbouring_branch(vited):
    """Decoder block 1's cross-attention branch scaled with its self-attention branch's scales: that block - its output, its dx, its
    d(kv), and the parameters of all three branches, since the MLP ran on a wrong input and the self-attention received a wrong
    gradient - and nothing else: every other stage saw what block 1 really produced (keys / values computed ahead, so d(features)
    restarts from the block's own d(kv))."""
    def stages(m, opt):
        assert not torch.equal(opt.dec[1, 0], opt.dec[1, 1])

        def block(R, blk, x, c, nh, store=None, scales=None, index=None):
            if blk is m.cross_blocks[1]:
                scales = torch.stack((scales[0], scales[0], scales[2]))
            return br.decoder_block(R, blk, x, c, nh, store, scales, index)
        return dict(decoder_block=block)

    labels, _ = _failing(vited, 'droppath', stages, cls_rows=True, fold=True)
    own = {'dec1.y', 'dec1.dx', 'dec1.dkv'} | _params('cross_blocks.1', 'norm1', 'attn.qkv', 'attn.proj', 'norm_cross', 'cross_attn.q',
                                                      'cross_attn.proj', 'norm2', 'mlp.fc1', 'mlp.fc2')
    # every tensor of the block but one: d fc2.bias is the column sum of s_mlp dy, which no other branch enters
    assert labels == own - {'g:cross_blocks.1.mlp.fc2.bias'}


def test_planted_position_gradient_one_row_off(vited):
    """d(pos_embed) of the image-2 stream scattered to row keep instead of 1 + keep (the prefix slot forgotten): pos_embed alone."""
    def alter(taps, grads, opt):
        dx = taps['dec.dx.0'][:, 1:]
        rows = torch.zeros_like(grads['pos_embed'][0])
        for b in range(dx.shape[0]):
            rows.index_add_(0, opt.keep2[b], dx[b])
            rows.index_add_(0, 1 + opt.keep2[b], -dx[b])
        grads['pos_embed'] = grads['pos_embed'] + rows[None]

    labels, lines = _failing(vited, 'patchdrop', alter=alter)
    assert labels == {'g:pos_embed'} and any('rowmax' in line for line in lines)


def test_planted_position_mask_missing_from_the_gradient(vited):
    """The streams multiplied by mask * scale, their gradients by the scale alone: the embed stage's four parameters."""
    def stages(m, opt):
        def embed(R, m_, img, with_cls, keep=None, mult=None):
            return _ForwardOnly.apply(br.embed(R, m_, img, with_cls, keep), mult, float(mult.max()))
        return dict(embed=embed)

    labels, _ = _failing(vited, 'posdrop', stages)
    assert labels == {'g:pos_embed', 'g:cls_token', 'g:patch_embed.proj.weight', 'g:patch_embed.proj.bias'}


@pytest.mark.parametrize('fold', [False, True])
def test_planted_pair_missing_from_an_image_sum(vited, fold):
    """The last of image 3's five pairs left out of decoder block 1's per-image sum.  Keys / values per block (the running d(context)):
    that block's term, the total - by their worst rows - and the block's own norm_context / kv gradients, which the same sum feeds.
    Keys / values computed ahead: the block's d(kv output) alone - the context stage restarts from what the block really handed it."""
    def stages(m, opt):
        skip = max(p for p, i in enumerate(opt.index.tolist()) if i == 3)
        assert skip == 10

        def lossy(R, kv, index):
            return _GatherLosingAPair.apply(R.seg(kv), index, skip)

        def block(R, blk, x, c, nh, store=None, scales=None, index=None):
            return br.decoder_block(R, blk, x, c, nh, store, scales, index, gather=lossy if blk is m.cross_blocks[1] else br.gather_kv)
        return dict(decoder_block=block)

    labels, lines = _failing(vited, 'indexed', stages, fold=fold)
    if fold:
        assert labels == {'dec1.dkv'}
    else:
        assert labels == {'dec1.dctx', 'context.dfeats'} | _params('cross_blocks.1', 'norm_context', 'cross_attn.kv')
    for label in labels - _params('cross_blocks.1', 'norm_context', 'cross_attn.kv'):
        assert any(line.startswith(label + ': rowmax') for line in lines), label


@pytest.fixture(scope='module')
def planted():
    """The first rounding model's own stage outputs at the A geometry, every row of every block live (no cls tail), the d(context)
    terms per block: what the defects are planted into."""
    s, batch = GEOMETRIES['A']
    m, x, y = _case(s, batch)
    taps, _ = br.network_taps(m, x, y, br.MODEL, cls_rows=False, fold=False)
    return m, taps, br.restart_all(m, taps, br.EXACT), br.restart_all(m, taps, br.MODEL)


def _judge(planted, label, bad):
    _, _, ref, model = planted
    assert br.failures(br.compare({label: model[label]}, {label: ref[label]}, {label: model[label]})) == []      # the honest value passes
    rows = br.compare({label: bad}, {label: ref[label]}, {label: model[label]})
    print(br.table(rows))
    return br.failures(rows)


def test_planted_bias_gradient_without_the_cls_rows(planted):
    """A bias gradient summed over the patch rows alone (the cls-row bookkeeping of the decoder gone wrong): d fc2.bias is the column sum
    of the block's dy, so the defect is exactly the cls rows' sum."""
    _, taps, _, model = planted
    label = 'g:cross_blocks.1.mlp.fc2.bias'
    assert _judge(planted, label, model[label] - taps['dec.dx.2'][:, 0].sum(0))


def test_planted_zeroed_row_of_dx(planted):
    _, _, _, model = planted
    for row in (0, 17):      # a cls row, a patch row
        bad = model['dec1.dx'].clone()
        bad[0, row] = 0
        assert _judge(planted, 'dec1.dx', bad)


def test_planted_missing_context_term(planted):
    """One block's d(context) left out of the total that the encoder receives."""
    _, _, _, model = planted
    for i in range(3):
        assert _judge(planted, 'context.dfeats', model['context.dfeats'] - model[f'dec{i}.dctx'])


def test_planted_layernorm_gradient_of_the_neighbouring_norm(planted):
    """The deferred LayerNorm column sums handed to the wrong norm: norm1 receives norm2's (gamma and beta)."""
    _, _, _, model = planted
    for blk in ('blocks.0', 'cross_blocks.1'):
        for p in ('weight', 'bias'):
            assert _judge(planted, f'g:{blk}.norm1.{p}', model[f'g:{blk}.norm2.{p}'])


def test_planted_weight_gradient_short_of_a_slab(planted):
    """A weight gradient summed over M - 64 rows: fc2's dW is dy^T u over the block's rows, so a backward whose dy lacks the 64 rows of
    sample 0 yields exactly that sum.  M = 256 here; the smallest M at which the batched weight-gradient queue engages is 4,096,
    where a 64-row slab is 1.6 % of the rows and about sqrt(64 / 4096) = 12 % of the norm - still an order above the bound."""
    m, taps, _, _ = planted
    dy = taps['enc.dx.2'].clone()
    dy[0] = 0
    out = {}
    br.restart_enc(m, taps, br.MODEL, out, 1, dy=dy)
    assert _judge(planted, 'g:blocks.1.mlp.fc2.weight', out['g:blocks.1.mlp.fc2.weight'])
