"""Block-local parity of the HIP model (tests/block_restart_cases.py): one forward + BCE backward with ``rt.tap`` set, then every
stage - embed, each encoder block, each decoder block, the context's kv projections, the head - restarted on the CPU in fp64 from
the HIP path's OWN taps.  What functions.py strings together between the kernels (the Functions' backward, the cls-rows-only last
block, the folded norm_context + kv GEMM and its unfold, the LayerNorm handed from one block's fc2 kernel to the next, the batched
and grouped weight-gradient queues, the deferred LayerNorm column sums) is thereby checked per block and per ROW, where the
whole-network tests can only see what survives 16 blocks of compounding and a whole-tensor norm.

Bounds (block_restart_cases.failures):
  * fp32 kernels: whole <= 1e-4 and rowmax <= 1e-3 against the fp64 restart;
  * bf16: each statistic <= 2 x the same statistic of the rounding model (fp64 with bf16 rounding at the operands of every
    contraction), restarted from the same taps, + 2^-8.  No host's bf16 autocast enters.
Both statistics of every compared tensor are printed, pass or fail (pytest -s, or the captured output of a failure).

The same cut under the options of training (block_restart_cases.OPTION_CASES): stochastic depth with explicit irregular scales (the
scale in gemm_row.hip's epilogue; with ``fused_ln`` off in the tile kernels' and in layernorm_bwd_scaled; with ``cls_tail`` off on
every row of the last block), patch dropout (streams of 48 and 49 tokens), position dropout (masks from explicit seeds), all three
on a q/k-norm tree, the gathered two-stage form and the pair-indexed one over 5 images and 12 pairs (folded, unfolded, with per-pair
scales, at 256 / 257 tokens), the kv projection in one launch, and a 768-wide tree.  Every option is passed explicitly, so nothing
is drawn.  Four planted defects on the HIP path itself (two on the plain model, one under stochastic depth, one in the indexed
form) say WHICH labels then fail.
"""
import functools

import pytest
import torch

import block_restart_cases as br
from oracle import vited_oracle as vo

pytestmark = pytest.mark.gpu

# the A geometry at the smallest batch whose token matrices (64 x 64 = 4,096 and 64 x 65 rows) reach the weight-gradient queue of
# functions._weight_grads: below 4,096 rows every product is launched on its own and batch_dw / group_dw switch nothing
SHAPE_A64, BATCH_A64 = vo.ViTEDShape(img_size=64, patch_size=8, embed_dim=384, num_heads=12, depth=2, c_depth=2), 64

#        id                 tree     shape          batch          runtime switches, set before the first forward
CASES = [('A',              'plain', br.SHAPE_A,    br.BATCH_A,    {}),
         ('A-cls_tail',     'plain', br.SHAPE_A,    br.BATCH_A,    {'cls_tail': False}),
         ('A-fold_context', 'plain', br.SHAPE_A,    br.BATCH_A,    {'fold_context': False}),
         ('A-fused_ln',     'plain', br.SHAPE_A,    br.BATCH_A,    {'fused_ln': False}),
         ('A-batch_dw',     'plain', br.SHAPE_A,    br.BATCH_A,    {'batch_dw': False}),
         ('A-group_dw',     'plain', br.SHAPE_A,    br.BATCH_A,    {'group_dw': False}),
         ('long',           'plain', br.SHAPE_LONG, br.BATCH_LONG, {}),
         ('qk_norm',        'qk',    br.SHAPE_A,    br.BATCH_A,    {}),
         ('avg_fc_norm',    'pool',  br.SHAPE_A,    br.BATCH_A,    {}),
         ('A64',            'plain', SHAPE_A64,     BATCH_A64,     {}),
         ('A64-group_dw',   'plain', SHAPE_A64,     BATCH_A64,     {'group_dw': False})]
BF16_ONLY = ('A64', 'A64-group_dw')       # the queues exist on the bf16 path alone

# parameter gradients exempt from ``rowmax`` (fp64 reference norm below 1e-3 of the case's largest; at most 2 per case): with these
# seeds the fp64 reference needs none in any case (checked on the CPU: every 2-D gradient is above 1e-3 of the largest)
EXEMPT = {name: () for name, *_ in CASES}


@functools.lru_cache(maxsize=None)
def _tree_and_inputs(kind, s, batch):
    m = br.build_tree(s, kind)
    state = {k: v.clone() for k, v in m.state_dict().items()}       # fp32, as the HIP model loads it
    x, y = br.inputs(s, batch)
    return m.double(), state, x, y


@functools.lru_cache(maxsize=None)
def _tree_and_option_case(vited, name):
    kind, s, images, pairs, switches, opt, inputs = br.option_case(name, vited.ops)
    m = br.build_tree(s, kind)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    return m.double(), state, kind, s, images, pairs, switches, opt, inputs


def _forward(vited, model, gpu, x, opt):
    """The model's call for the step that ``opt`` describes (None: the plain one-shot forward on stacked pairs ``x``; else ``x`` =
    (images, second images of the pairs)).  Every option goes in explicitly - scales, keep tables, seeds - so nothing is drawn."""
    if opt is None:
        return model(x.to(gpu))
    on = lambda t: None if t is None else t.to(gpu)
    seed = lambda v: torch.tensor([v], dtype=torch.int64, device=gpu)
    both = {}
    if opt.enc is not None:
        both['drop_path'] = vited.DropPathScales(on(opt.enc), on(opt.dec))
    if opt.keep1 is not None:
        both['patch_keep'] = vited.PatchKeep(on(opt.keep1), on(opt.keep2))
    if opt.seeds is not None:
        both['pos_drop'] = vited.PosDropSeeds(seed(opt.seeds[0]), seed(opt.seeds[1]))
    if opt.index is None:
        return model(torch.stack(x, 1).to(gpu), **both)
    half = lambda h: {k: type(v)(*(f if j == h else None for j, f in enumerate(v))) for k, v in both.items()}
    imgs = x[0].to(gpu)
    feats = model(imgs, forward_first_part=True, **half(0))
    if opt.indexed:
        return model(feats, imgs, x2_index=on(opt.x2_index), x1_index=on(opt.index), **half(1))
    return model(feats[on(opt.index)], imgs[on(opt.x2_index)], **half(1))


def _hip_run(vited, gpu, kind, s, batch, dtype, switches, option_case=None):
    """One forward + BCE backward of the HIP model with ``rt.tap`` set.  ``option_case``: the name of a br.OPTION_CASES entry, whose
    tree, options and inputs then replace the plain ones."""
    opt, pairs = None, batch
    if option_case is None:
        m64, state, x, y = _tree_and_inputs(kind, s, batch)
    else:
        m64, state, kind, s, batch, pairs, switches, opt, (x1, x2, y) = _tree_and_option_case(vited, option_case)
        x = (x1, x2)
    extra = {'plain': {}, 'qk': dict(qk_norm=True), 'pool': dict(global_pool='avg', fc_norm=True)}[kind]
    if opt is not None:
        extra.update(drop_path_rate=opt.drop_path_rate, patch_drop_rate=opt.patch_rate, pos_drop_rate=opt.pos_rate)
    model = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                          embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads,
                                          mlp_ratio=s.mlp_ratio, qkv_bias=s.qkv_bias, **extra)
    model.compute_dtype = dtype
    model = model.to(gpu)
    model.load_state_dict(state)
    rt = model.runtime()
    for name, value in switches.items():
        assert getattr(rt, name) is not value, f'{name} already is {value}'
        setattr(rt, name, value)
    rt.tap = {}
    try:
        logits = _forward(vited, model, gpu, x, opt)
        torch.nn.functional.binary_cross_entropy_with_logits(logits, y.to(gpu)).backward()
        torch.cuda.synchronize()
        raw = dict(rt.tap)
    finally:
        rt.tap = None
    x1, x2 = br._halves(x)
    raw.update(x1=x1, x2=x2, target=y, logits=logits)
    taps = br.canonical_taps(raw, s, batch, pairs, indexed=opt is not None and opt.indexed)
    grads = {n: p.grad for n, p in model.named_parameters()}
    assert all(g is not None for g in grads.values())
    return m64, rt, taps, grads, {n for n, _ in model.named_parameters()}


PARAMS = [pytest.param(*case, dtype, id=f'{case[0]}-{tag}') for case in CASES for tag, dtype in (('bf16', torch.bfloat16), ('fp32', torch.float32))
          if not (tag == 'fp32' and case[0] in BF16_ONLY)]


@pytest.mark.parametrize('name,kind,s,batch,switches,dtype', PARAMS)
def test_every_stage_restarted_from_the_hip_taps(vited, gpu, name, kind, s, batch, switches, dtype):
    exact = dtype == torch.float32
    m64, rt, taps, grads, names = _hip_run(vited, gpu, kind, s, batch, dtype, switches)
    # the layout the switches ask for is the layout that ran
    cls_rows, fold = br.layout_of(taps, s)
    assert cls_rows == (switches.get('cls_tail', True) and kind != 'pool')
    assert fold == (switches.get('fold_context', True) and not exact)
    # autograd hands the decoder's total d(features) to the encoder untouched
    assert torch.equal(taps[f'enc.dx.{s.depth}'], taps['dec.dfeats'])
    ref = br.restart_all(m64, taps, br.EXACT)
    model = None if exact else br.restart_all(m64, taps, br.MODEL)
    got = br.observed(taps, grads, s)
    assert br.checked_parameters(ref) == names and set(got) == set(ref)
    exempt = br.exempt_labels(ref)
    assert len(exempt) <= br.MAX_EXEMPT and set(exempt) <= set(EXEMPT[name]), exempt
    rows = br.compare(got, ref, model)
    print(f'\n== {name} {"fp32" if exact else "bf16"}: HIP against the fp64 restart' + ('' if exact else ' | rounding model against it'))
    print(br.table(rows))
    for (stage, what), v in br.by_stage(rows).items():
        print(f'stage {name} {"fp32" if exact else "bf16"} {stage:8s} {what:6s} hip whole {v[0]:.2e} rowmax {v[1]:.2e}'
              + ('' if exact else f'   model whole {v[2]:.2e} rowmax {v[3]:.2e}'))
    bad = br.failures(rows, exempt)
    assert not bad, '\n'.join(bad)


OPTION_PARAMS = [pytest.param(case[0], dtype, id=f'{case[0]}-{tag}') for case in br.OPTION_CASES
                 for tag, dtype in (('bf16', torch.bfloat16), ('fp32', torch.float32)) if not (tag == 'fp32' and case[0] in br.OPTION_BF16_ONLY)]


@pytest.mark.parametrize('name,dtype', OPTION_PARAMS)
def test_every_stage_restarted_from_the_hip_taps_under_the_options(vited, gpu, monkeypatch, name, dtype):
    """The paths training uses - stochastic depth, patch and position dropout, the two-stage and the pair-indexed decoder, the kv
    projection in one launch, a 768-wide tree - cut at the block boundaries like the plain model above, under the same bounds."""
    exact = dtype == torch.float32
    one_launch = []
    if name == 'kv_one_launch':
        real = vited.ops.gemm_nt_wreg
        monkeypatch.setattr(vited.ops, 'gemm_nt_wreg', lambda a, *r, **k: (one_launch.append((a.shape[0], a.stride(0), k.get('groups'))), real(a, *r, **k))[1])
    m64, rt, taps, grads, names = _hip_run(vited, gpu, None, None, None, dtype, None, option_case=name)
    _, _, kind, s, images, pairs, switches, opt, _ = _tree_and_option_case(vited, name)
    # the layout the case means is the layout that ran
    cls_rows, fold = br.layout_of(taps, s)
    assert cls_rows == switches.get('cls_tail', True)
    assert fold == (switches.get('fold_context', True) and not exact)
    if name == 'kv_one_launch':         # the folded kv projection of all blocks went through gemm_nt_wreg, once, and the kernel takes that call
        assert one_launch == [(images * s.n1, s.embed_dim, 2 * s.c_depth)]
        assert vited.ops.gemm_nt_wreg_supported(images * s.n1, 2 * s.c_depth, 2, lda=s.embed_dim)
    if opt.keep1 is not None:           # the shortened streams at rate 0.25: patch 0 + 47 of 63 and cls + 48 of 64 - ragged against 16 and 64
        assert (taps['enc.in'].shape[1], taps['dec.in'].shape[1]) == (1 + opt.keep1.shape[1], 1 + opt.keep2.shape[1]) == (48, 49)
    assert taps['enc.in'].shape[0] == images and taps['dec.in'].shape[0] == pairs
    if opt.index is not None:
        assert taps['dec.dfeats'].shape[0] == (images if opt.indexed else pairs)
    # the encoder received the decoder's total d(features): handed over untouched, or summed over every image's pairs by autograd
    assert torch.equal(taps[f'enc.dx.{s.depth}'], br.features_gradient(taps, s, opt))
    ref = br.restart_all(m64, taps, br.EXACT, opt)
    model = None if exact else br.restart_all(m64, taps, br.MODEL, opt)
    got = br.observed(taps, grads, s)
    assert br.checked_parameters(ref) == names and set(got) == set(ref)
    if opt.indexed:                     # an image that no pair reads: exact zeros in the restart, and rowmax's floor judges what the HIP path wrote
        unread = sorted(set(range(images)) - set(opt.index.tolist()))
        assert len(unread) == 1 and not bool(ref['context.dfeats'][unread].any())
    assert br.exempt_labels(ref) == []          # no small-gradient exemption in any of these cases
    rows = br.compare(got, ref, model)
    tag = 'fp32' if exact else 'bf16'
    print(f'\n== {name} {tag}: HIP against the fp64 restart' + ('' if exact else ' | rounding model against it'))
    print(br.table(rows))
    for (stage, what), v in br.by_stage(rows).items():
        print(f'stage {name} {tag} {stage:8s} {what:6s} hip whole {v[0]:.2e} rowmax {v[1]:.2e}'
              + ('' if exact else f'   model whole {v[2]:.2e} rowmax {v[3]:.2e}'))
    bad = br.failures(rows)
    assert not bad, '\n'.join(bad)


def _failing_labels(vited, gpu, dtype, switches):
    name, kind, s, batch, _ = CASES[0]
    m64, rt, taps, grads, _ = _hip_run(vited, gpu, kind, s, batch, dtype, switches)
    ref = br.restart_all(m64, taps, br.EXACT)
    model = None if dtype == torch.float32 else br.restart_all(m64, taps, br.MODEL)
    rows = br.compare(br.observed(taps, grads, s), ref, model)
    bad = br.failures(rows)
    print('\n'.join(bad))
    return {line.split(': ', 1)[0] for line in bad}


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'fp32'])
def test_a_dropped_context_term_in_the_hip_backward_is_caught_where_it_happens(vited, gpu, monkeypatch, dtype):
    """The check bites on the HIP path itself, and locally: with the middle decoder block's d(context) term thrown away inside
    DecoderFn.backward (the running sum handed on as it came in), exactly that block's term and the total fail - every other stage,
    restarted from the taps it actually saw, still passes."""
    fn = vited.functions
    real = fn._dec_cross_bwd

    def forgetful(rt, dx, dx_lp, xa, P, saved, ctxf, dctx, batch, index, *a, **k):
        before = dctx.clone() if dctx is not None else None
        out = real(rt, dx, dx_lp, xa, P, saved, ctxf, dctx, batch, index, *a, **k)
        if index == 1:
            out[2].copy_(before)        # the sum is accumulated in place: put back what came in
        return out

    monkeypatch.setattr(fn, '_dec_cross_bwd', forgetful)
    assert _failing_labels(vited, gpu, dtype, {'fold_context': False}) == {'dec1.dctx', 'context.dfeats'}


def test_a_zeroed_row_of_the_stream_gradient_in_the_hip_backward_is_caught_where_it_happens(vited, gpu, monkeypatch):
    """One row of the gradient that encoder block 1 hands to block 0 zeroed (fp32 kernels, where the stream gradient and the copy the
    branches read are one tensor): `enc1.dx` fails by its worst row - the whole-tensor norm of that error is 1 / sqrt(256 rows) - and
    block 0, restarted from the gradient it actually received, passes."""
    fn = vited.functions
    real = fn._attn_branch_bwd

    def lossy(rt, dy, dy_lp, x, P, saved, batch, n, key=None, lp_scale=None):
        dx, dx_lp, grads = real(rt, dy, dy_lp, x, P, saved, batch, n, key=key, lp_scale=lp_scale)
        if key == ('blocks', 1, 'attn'):
            dx[5].zero_()
        return dx, dx_lp, grads

    monkeypatch.setattr(fn, '_attn_branch_bwd', lossy)
    assert _failing_labels(vited, gpu, torch.float32, {}) == {'enc1.dx'}


def _failing_option_labels(vited, gpu, dtype, name):
    m64, rt, taps, grads, _ = _hip_run(vited, gpu, None, None, None, dtype, None, option_case=name)
    _, _, _, s, _, _, _, opt, _ = _tree_and_option_case(vited, name)
    ref = br.restart_all(m64, taps, br.EXACT, opt)
    model = None if dtype == torch.float32 else br.restart_all(m64, taps, br.MODEL, opt)
    bad = br.failures(br.compare(br.observed(taps, grads, s), ref, model))
    print('\n'.join(bad))
    return {line.split(': ', 1)[0] for line in bad}


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'fp32'])
def test_an_unscaled_copy_of_the_stream_gradient_in_the_hip_backward_is_caught_where_it_happens(vited, gpu, monkeypatch, dtype):
    """Stochastic depth: the copy of the encoder's output gradient that the last block's MLP branch reads left without that branch's
    scales (_lp_scaled handing out a plain copy).  The residual path still carries dy, so block 1's own dx and all twelve of its
    parameter gradients are wrong - the MLP branch's by the scales themselves, the attention branch's through the gradient it is
    handed - and every other stage, block 0 included, passes: it restarts from the gradient it really received."""
    fn = vited.functions
    real = fn._lp_scaled
    monkeypatch.setattr(fn, '_lp_scaled', lambda rt, t, row_scale: real(rt, t, None))
    block1 = {f'g:blocks.1.{n}.{p}' for n in ('norm1', 'attn.qkv', 'attn.proj', 'norm2', 'mlp.fc1', 'mlp.fc2') for p in ('weight', 'bias')}
    assert _failing_option_labels(vited, gpu, dtype, 'droppath') == {'enc1.dx'} | block1


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'fp32'])
def test_a_dropped_per_image_term_in_the_indexed_hip_backward_is_caught_where_it_happens(vited, gpu, monkeypatch, dtype):
    """The pair-indexed form with the running per-image d(context): the middle decoder block's per-image term (every image's sum over
    its pairs, through that block's kv projection) thrown away - exactly that block's term and the total fail."""
    fn = vited.functions
    real = fn._dec_cross_bwd

    def forgetful(rt, dx, dx_lp, xa, P, saved, ctxf, dctx, batch, index, *a, **k):
        assert k.get('seg') is not None and dctx is not None and dctx.shape[0] == k['seg'].items * rt.n1       # the sum is per image
        before = dctx.clone()
        out = real(rt, dx, dx_lp, xa, P, saved, ctxf, dctx, batch, index, *a, **k)
        if index == 1:
            out[2].copy_(before)
        return out

    def wrapper(rt, dx, dx_lp, xa, P, saved, ctxf, dctx, batch, index, *a, **k):
        return (forgetful if index < 2 else real)(rt, dx, dx_lp, xa, P, saved, ctxf, dctx, batch, index, *a, **k)

    monkeypatch.setattr(fn, '_dec_cross_bwd', wrapper)
    name = 'indexed-fold_context' if dtype == torch.bfloat16 else 'indexed'       # fp32 never folds: the same layout
    assert _failing_option_labels(vited, gpu, dtype, name) == {'dec1.dctx', 'context.dfeats'}
