"""The block-restart machinery itself (tests/block_restart_cases.py), on the CPU:

  * chain rule: with no rounding and fed the fp64 whole-network oracle's own taps, the stage restarts reproduce that oracle - every
    stage output, every d(input), every parameter gradient - to 1e-10, in every layout the HIP path records (cls rows only on the
    last block, keys / values computed ahead) and for the plain, q/k-norm and pooled-head trees;
  * completeness: the stages between them own every parameter of the state_dict, once;
  * the bf16 bound (2 x the rounding model's statistic + 2^-8) lets a second, differently rounding bf16 implementation through ...
  * ... and catches each of five planted glue defects.
"""
import pytest
import torch

import block_restart_cases as br
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
