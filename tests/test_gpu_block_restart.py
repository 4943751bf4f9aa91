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


def _hip_run(vited, gpu, kind, s, batch, dtype, switches):
    m64, state, x, y = _tree_and_inputs(kind, s, batch)
    extra = {'plain': {}, 'qk': dict(qk_norm=True), 'pool': dict(global_pool='avg', fc_norm=True)}[kind]
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
        logits = model(x.to(gpu))
        torch.nn.functional.binary_cross_entropy_with_logits(logits, y.to(gpu)).backward()
        torch.cuda.synchronize()
        raw = dict(rt.tap)
    finally:
        rt.tap = None
    raw.update(x=x, target=y, logits=logits)
    taps = br.canonical_taps(raw, s, batch)
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
