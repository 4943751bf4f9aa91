"""Stochastic depth, the parts that need no GPU: the constructor surface, the two decay rules, the draw, and the pin of the
composition in tests/droppath_cases.py against what the reference's own classes computed (tests/golden/droppath.npz)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import droppath_cases as dc
from oracle import vited_oracle as vo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'droppath.npz')


def _model(vited, rate, depth=3, c_depth=3, **kw):
    s = vo.ViTEDShape(depth=depth, c_depth=c_depth)
    return vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, num_classes=s.num_classes, embed_dim=s.embed_dim,
                                         depth=depth, c_depth=c_depth, num_heads=s.num_heads, drop_path_rate=rate, **kw)


def test_composition_matches_the_reference_classes():
    """fp64, closed-form weights, forced scales: logits, loss and every parameter gradient of the composition equal what the
    reference's VisionTransformerCustom(drop_path_rate=0.5) gave with its DropPath modules forced to the same scales - the
    placement of the two encoder and three decoder branches - and the stored drop_prob of every module is the decay rule."""
    fx = np.load(GOLDEN)
    x, y, enc, dec = dc.golden_inputs()
    np.testing.assert_array_equal(fx['enc'], enc.numpy())
    np.testing.assert_array_equal(fx['dec'], dec.numpy())
    s = dc.GOLDEN_SHAPE
    for key, depth, branches in (('drop_prob_enc', s.depth, 2), ('drop_prob_dec', s.c_depth, 3)):
        want = np.array([[torch.linspace(0, dc.GOLDEN_RATE, depth)[i].item()] * branches for i in range(depth)])
        np.testing.assert_array_equal(fx[key], want)
    m = vo.fill_closed_form_(vo.OracleViTED(s)).double()
    logits = dc.forward_scaled(m, x.double(), enc, dec)
    loss, grads = dc.loss_and_grads(m, logits, y.double())
    np.testing.assert_allclose(logits.detach().numpy(), fx['logits'], rtol=1e-9, atol=0)
    np.testing.assert_allclose(loss.numpy(), fx['loss'], rtol=1e-9)
    names = [str(n) for n in fx['grad_names']]
    assert names == [n for n, _ in m.named_parameters()]
    norms = np.array([float(grads[n].norm()) for n in names])
    np.testing.assert_allclose(norms, fx['grad_norms'], rtol=1e-9)
    for n, norm, want in zip(names, fx['grad_norms'], fx['grad_slices']):
        got = grads[n].reshape(-1)[:16].numpy()
        np.testing.assert_allclose(got, want[:got.size], rtol=1e-9, atol=1e-9 * norm, err_msg=n)
    # the scales matter: the same weights without them give other logits
    assert not np.allclose(m(x.double()).detach().numpy(), fx['logits'], rtol=1e-3)


def test_constructor_takes_the_rate(vited):
    plain, dropped = _model(vited, 0.), _model(vited, 0.3)
    assert dropped.drop_path_rate == pytest.approx(0.3) and plain.drop_path_rate == 0.
    assert list(dropped.state_dict().keys()) == list(plain.state_dict().keys())
    assert [tuple(v.shape) for v in dropped.state_dict().values()] == [tuple(v.shape) for v in plain.state_dict().values()]
    assert dropped.last_drop_path is None


def test_drop_path_probs_are_the_two_linspaces(vited):
    m = _model(vited, 0.4, depth=5, c_depth=2)
    enc, dec = m.drop_path_probs
    assert enc == [torch.linspace(0, 0.4, 5)[i].item() for i in range(5)]
    assert dec == [torch.linspace(0, 0.4, 2)[i].item() for i in range(2)]
    assert enc[0] == 0. and dec[0] == 0. and dec[1] == torch.tensor(0.4).item()
    assert _model(vited, 0.).drop_path_probs == ([0.] * 3, [0.] * 3)


@pytest.mark.parametrize('rate', [1.0, -0.1, 1.5])
def test_bad_rate_raises(vited, rate):
    with pytest.raises(ValueError):
        _model(vited, rate)


def test_factory_forwards_the_rate_only_on_request(vited):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = vited.config_from_yaml(os.path.join(here, 'configs', 'puzzle', 'div2k_erosion7_4bin_patch8_64.yaml'), ['MODEL.PJS.DEPTH', '2'])
    assert cfg.MODEL.DROP_PATH_RATE == pytest.approx(0.1)
    assert vited.build_model(cfg).drop_path_rate == 0.                         # the reference's factory does not forward the key
    assert vited.build_model(cfg, drop_path_rate=0.1).drop_path_rate == pytest.approx(0.1)
    assert vited.build_model(cfg, drop_path_rate=cfg.MODEL.DROP_PATH_RATE).drop_path_probs[0] == [0., torch.tensor(0.1).item()]


def test_draw(vited):
    b = 20000
    m = _model(vited, 0.5)
    g = torch.Generator().manual_seed(123)
    s = m.draw_drop_path(b, b, generator=g, device='cpu')
    assert s.enc.shape == (3, 2, b) and s.dec.shape == (3, 3, b) and s.enc.dtype == s.dec.dtype == torch.float32
    branches = []
    for t, probs in zip(s, m.drop_path_probs):
        for i, p in enumerate(probs):
            keep = 1.0 - p
            inv = (torch.ones((), dtype=torch.float32) / torch.tensor(keep, dtype=torch.float32)).item()
            for j in range(t.shape[1]):
                row = t[i, j]
                assert set(row.unique().tolist()) <= {0.0, inv}, (i, j)
                kept = int((row != 0).sum())
                if p == 0.:
                    assert kept == b and bool((row == 1).all())          # block 0: everyone kept at scale 1
                else:
                    assert abs(kept - b * keep) <= 5 * math.sqrt(b * keep * (1 - keep)), (i, j, kept)
                    branches.append(row)
    assert len(branches) == 2 * 2 + 2 * 3
    for a in range(len(branches)):
        for c in range(a + 1, len(branches)):
            assert not torch.equal(branches[a] != 0, branches[c] != 0)          # every branch draws on its own
    again = m.draw_drop_path(b, b, generator=torch.Generator().manual_seed(123), device='cpu')
    assert torch.equal(again.enc, s.enc) and torch.equal(again.dec, s.dec)
    half = m.draw_drop_path(7, None, generator=g, device='cpu')
    assert half.enc.shape == (3, 2, 7) and half.dec is None


def test_custom_generator_is_refused_inside_a_capture(vited, monkeypatch):
    """A generator that torch has not registered with the graph would freeze one mask into it: the draw says so instead."""
    m = _model(vited, 0.5)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError, match='default generator'):
        m.draw_drop_path(4, 4, generator=torch.Generator(), device='cuda')


def test_gemm_takes_the_public_epilogue_codes_only(vited):
    """The scaled residual epilogue has an id of its own inside the library, the first value after the public VITED_EPI_* codes.
    It is reached through vited_gemm_scaled alone: vited_gemm with that value, or any other outside 0..6, is the bad argument it
    always was, and vited_gemm_scaled wants its residual.  Both return before anything is launched."""
    lib = vited._lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert vited.ops.EPI_GELU_GRAD == 6
    for epilogue in (-1, 7, 8, 1 << 20):
        assert lib.vited_gemm(p, 8, p, 8, 0, 0, 8, 8, 8, epilogue, None, None, p, p, p, 8, 0, 0, 0, 0, None) == 1, epilogue
        assert lib.vited_gemm(p, 8, p, 8, 0, 1, 8, 8, 8, epilogue, None, None, None, p, None, 8, 0, 0, 0, 0, None) == 1, epilogue
    assert lib.vited_gemm_scaled(p, 8, p, 8, 0, 0, 8, 8, 8, None, None, p, p, 8, None) == 1          # a scale without a residual
    assert lib.vited_gemm_scaled(p, 8, p, 8, 0, 0, 8, 8, 8, None, None, None, p, 8, None) == 1
