"""engine.relevancy_from_cams against the reference's own rule functions (scripts/visualise_attentions.py), on the CPU in fp64.

tests/golden/relevancy.npz (tools/make_relevancy_golden.py) holds head-averaged maps of a closed-form 2 + 2 block model with the
R_qi that Generator.generate_ours' order of updates gives for them, and a synthetic case (N1 5, N2 6) with an all-zero map and an
all-zero row, where handle_residual divides 0 by 0 and rule 10 replaces the NaN by 0.  Both are pure fp64 arithmetic on the same
inputs, so only the summation order of the matrix products separates the two sides: rtol 1e-9."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'relevancy.npz')


@pytest.fixture(scope='module')
def fx():
    return np.load(GOLDEN)


def _cams(fx, prefix=''):
    return [[torch.from_numpy(block) for block in fx[f'{prefix}{kind}_cams']] for kind in ('enc', 'dec_self', 'dec_cross')]


def test_golden_cams_give_the_golden_relevancy(vited, fx):
    enc, dec_self, dec_cross = _cams(fx)
    r = vited.engine.relevancy_from_cams(enc, dec_self, dec_cross)
    assert r.dtype == torch.float64 and tuple(r.shape) == (2, 65, 64)
    np.testing.assert_allclose(r.numpy(), fx['r_qi'], rtol=1e-9, atol=0)
    assert float(np.abs(fx['r_qi']).max()) > 0


@pytest.mark.parametrize('normalize, self10', [(True, True), (False, True), (True, False)])
def test_synthetic_case_with_zero_rows(vited, fx, normalize, self10):
    enc, dec_self, dec_cross = _cams(fx, 'syn_')
    before = [c.clone() for c in enc + dec_self + dec_cross]
    r = vited.engine.relevancy_from_cams(enc, dec_self, dec_cross, normalize_self_attention=normalize, apply_self_in_rule_10=self10)
    want = fx[f'syn_r_qi__norm{int(normalize)}_self{int(self10)}']
    assert tuple(r.shape) == (2, 6, 5) and torch.isfinite(r).all()
    np.testing.assert_allclose(r.numpy(), want, rtol=1e-9, atol=0)
    assert all(torch.equal(a, b) for a, b in zip(before, enc + dec_self + dec_cross)), 'the maps handed in were modified'


def test_the_zero_over_zero_branch_is_what_the_synthetic_case_exercises(vited, fx):
    """Sample 0's first decoder block leaves query 2's self-relevancy at the identity: its normalised row is 0 / 0, the whole
    rule-10 product of that block is NaN and is dropped, so after ONE decoder block that sample's R_qi is still zero - while
    without the normalisation the same block does contribute."""
    enc, dec_self, dec_cross = _cams(fx, 'syn_')
    one = vited.engine.relevancy_from_cams(enc, dec_self[:1], dec_cross[:1])
    assert torch.count_nonzero(one[0]) == 0 and torch.count_nonzero(one[1]) == one[1].numel()
    plain = vited.engine.relevancy_from_cams(enc, dec_self[:1], dec_cross[:1], normalize_self_attention=False)
    assert torch.count_nonzero(plain[0]) == plain[0].numel()


def test_argument_errors(vited, fx):
    enc, dec_self, dec_cross = _cams(fx, 'syn_')
    with pytest.raises(ValueError, match='one self and one cross map'):
        vited.engine.relevancy_from_cams(enc, dec_self[:1], dec_cross)
    with pytest.raises(ValueError, match='decoder self map'):
        vited.engine.relevancy_from_cams(enc, [dec_cross[0], dec_self[1]], dec_cross)
    with pytest.raises(ValueError, match=r'\[B, Nq, Nk\]'):
        vited.engine.relevancy_from_cams(enc, [c[0] for c in dec_self], [c[0] for c in dec_cross])
