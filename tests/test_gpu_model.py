"""Whole-path parity on the GPU: the HIP ViT-ED (through the C ABI) against
 (1) the golden fixtures produced by the reference's own classes (tests/golden, see
     oracle/pin_against_reference.py), and
 (2) the CPU fp32 oracle on seeded random inputs / reference-style random init.

Tolerances
  * fp32 kernels ("exact" path): rtol 1e-3 on logits - the tolerance BASELINE.json's north_star
    states - and rtol 2e-3 on per-parameter gradient norms (measured error is ~1e-5).
  * bf16 MFMA path: logits within 3e-2 (abs + rel).  For scale: PyTorch's own CPU bf16-autocast of
    the reference deviates by up to 8e-3 abs on logits of magnitude 0.4, so rtol
    1e-3 is not a bf16 tolerance for anybody.  bf16 GRADIENTS are judged against that same yardstick
    (see _check_bf16_grads_like_torch_autocast) on the closed-form fixtures, and at 6 % per tensor on
    the well-conditioned reference-style random init.
"""
import os

import numpy as np
import pytest
import torch

from oracle import vited_oracle as vo

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _fixture(name):
    return np.load(os.path.join(GOLDEN, f'vited_{name}.npz'))


def _shape_of(fx):
    img, p, c, ncls, d, depth, cdepth, heads = [int(v) for v in fx['shape']]
    return vo.ViTEDShape(img_size=img, patch_size=p, in_chans=c, num_classes=ncls, embed_dim=d, depth=depth,
                         c_depth=cdepth, num_heads=heads)


def _hip_model(vited, s, gpu, dtype):
    m = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans,
                                      num_classes=s.num_classes, embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth,
                                      num_heads=s.num_heads, mlp_ratio=s.mlp_ratio, qkv_bias=s.qkv_bias)
    m.compute_dtype = dtype
    return m.to(gpu)


def _targets(batch, s, dev):
    return (vo.closed_form((batch, s.num_classes), 77, 1.0) > 0.2).float().to(dev)


@pytest.mark.parametrize('name', ['T', 'A_1x1', 'A_2x2', 'H_1x1_128', 'H_1x1_512', 'H_4x4_512', 'A_full', 'H_full'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_against_reference_fixtures(vited, gpu, name, dtype):
    fx = _fixture(name)
    s, batch = _shape_of(fx), int(fx['batch'])
    model = vo.fill_closed_form_(_hip_model(vited, s, gpu, dtype))
    x = vo.closed_form_pairs(batch, s).to(gpu)
    exact = dtype == torch.float32
    ltol = dict(rtol=1e-3, atol=1e-4) if exact else dict(rtol=3e-2, atol=3e-2)
    has_bwd = 'loss' in fx
    with torch.set_grad_enabled(has_bwd):
        feats = model(x[:, 0], forward_first_part=True)
        logits = model(x)
        two_stage = model(feats, x[:, 1])
    assert logits.dtype == torch.float32 and feats.dtype == torch.float32
    if exact or not has_bwd or s.depth + s.c_depth < 8:
        np.testing.assert_allclose(logits.detach().cpu().numpy(), fx['logits'], **ltol)
    else:
        # 8 or more blocks of closed-form weights (A_full: 8 + 8 at 64 tokens; H_4x4_512: near-uniform attention over a thousand
        # keys) make the logits themselves ill-conditioned in bf16: PyTorch's own CPU bf16 autocast of the oracle is 1.5e-2 .. 9e-2
        # off on them, depending on the host's bf16 kernels, and two equally careful bf16 implementations differ from each other
        # by as much (folding norm_context into the kv weights moved A_full's worst logit from 0.040 to 0.044 of an allowed
        # 0.0437 while the per-block comparison with autocast stayed inside its bounds: test_bf16_error_growth_per_block).
        # So the yardstick here is that autocast run on THIS host: within 3e-2, or within 1.5 x its error + 1e-2
        err = float(np.abs(logits.detach().cpu().numpy() - fx['logits']).max())
        m_ac = vo.fill_closed_form_(vo.OracleViTED(s)).eval()
        with torch.no_grad(), torch.autocast('cpu', dtype=torch.bfloat16):
            err_ac = float(np.abs(m_ac(vo.closed_form_pairs(batch, s)).float().numpy() - fx['logits']).max())
        # ... and never beyond 6e-2, whatever the host's autocast does (measured: DESIGN.md section 8)
        print(f'{name}: bf16 logits err {err:.3e}, torch bf16 autocast on this host err_ac {err_ac:.3e}')
        assert err <= min(6e-2, max(3e-2, 1.5 * err_ac + 1e-2)), f'bf16 logits {err:.3e} off the reference fixture; torch bf16 autocast: {err_ac:.3e}'
        ltol = dict(rtol=0, atol=float('inf'))
    # structural invariant the reference's only test relies on: two-stage == one-shot
    assert torch.equal(two_stage, logits)
    ftol = dict(rtol=1e-3, atol=1e-4) if exact else dict(rtol=5e-2, atol=5e-2)
    np.testing.assert_allclose(feats[:, :4, :].detach().cpu().numpy(), fx['feats_slice'], **ftol)
    if not has_bwd:
        return
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, _targets(batch, s, gpu))
    loss.backward()
    np.testing.assert_allclose(loss.item(), float(fx['loss']), rtol=1e-4 if exact else 3e-2)
    grads = dict(model.named_parameters())
    names = [str(n) for n in fx['grad_names']]
    assert names == [n for n, _ in model.named_parameters()]
    want = fx['grad_norms']
    if not exact:
        _check_bf16_grads_like_torch_autocast(s, batch, {n: grads[n].grad.cpu() for n in names})
        return
    got = np.array([float(grads[n].grad.double().norm()) for n in names])
    np.testing.assert_allclose(got, want, rtol=2e-3, atol=1e-6)
    st = dict(rtol=2e-3, atol=1e-5 * float(want.max()))
    np.testing.assert_allclose(grads['head.weight'].grad.cpu().numpy(), fx['grad_head_weight'], **st)
    np.testing.assert_allclose(grads['cls_token'].grad.cpu().numpy(), fx['grad_cls_token'], **st)
    np.testing.assert_allclose(grads['pos_embed'].grad[0, :3, :16].cpu().numpy(), fx['grad_pos_embed_slice'], **st)
    np.testing.assert_allclose(grads['blocks.0.attn.qkv.weight'].grad[:8, :8].cpu().numpy(), fx['grad_qkv0_slice'], **st)
    np.testing.assert_allclose(grads['cross_blocks.0.cross_attn.kv.weight'].grad[:8, :8].cpu().numpy(),
                               fx['grad_kv0_slice'], **st)


def _oracle_grads(s, batch, autocast):
    m = vo.fill_closed_form_(vo.OracleViTED(s))
    x = vo.closed_form_pairs(batch, s)
    y = (vo.closed_form((batch, s.num_classes), 77, 1.0) > 0.2).float()
    with torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
        out = m(x)
    torch.nn.functional.binary_cross_entropy_with_logits(out.float(), y).backward()
    return {n: p.grad for n, p in m.named_parameters()}


def _check_bf16_grads_like_torch_autocast(s, batch, g_hip):
    """bf16 gradients on the closed-form fixtures are ill-conditioned for EVERY bf16 implementation
    (PyTorch's own CPU bf16 autocast of the oracle is off by > 100 % on some tensors), so the
    yardstick for the MFMA path is that autocast run: the HIP path must be about as close to the
    fp32 gradients as PyTorch bf16 autocast is - globally within 1.5x (+1e-2) at every depth, per tensor
    within 3x (+5e-2) on the shallow cases (on the 8+8-block closed-form case individual small tensors are
    chaotic in bf16 - two bf16 implementations differ from each other as much as from fp32 - so per tensor it
    is the per-block comparison of test_bf16_error_growth_per_block that applies there).  Round 1 carried a 4x
    allowance for the deep case; measured at round 2 (tests/diag_bf16_gradients.py) the HIP path is at
    0.74x of autocast's error there (8.98e-2 vs 1.22e-1), so the allowance is gone."""
    g32 = _oracle_grads(s, batch, autocast=False)
    gac = _oracle_grads(s, batch, autocast=True)

    def total(g):
        num = sum(float((g[n].double() - g32[n].double()).norm() ** 2) for n in g32)
        den = sum(float(g32[n].double().norm() ** 2) for n in g32)
        return (num / den) ** 0.5

    t_hip, t_ac = total(g_hip), total(gac)
    deep = s.depth + s.c_depth >= 8
    assert t_hip <= 1.5 * t_ac + 1e-2, f'global bf16 gradient error {t_hip:.3e} vs torch autocast {t_ac:.3e}'
    if deep:
        return
    gmax = max(float(g.norm()) for g in g32.values())
    for n in g32:
        den = float(g32[n].norm()) + 1e-12
        if den < 1e-3 * gmax:
            continue  # cancellation-dominated tensors (e.g. |d norm_cross| ~ 1e-5 of the largest) say nothing in bf16
        e_hip = float((g_hip[n] - g32[n]).norm()) / den
        e_ac = float((gac[n] - g32[n]).norm()) / den
        assert e_hip <= 3 * e_ac + 5e-2, f'{n}: HIP bf16 error {e_hip:.3e}, torch bf16 autocast error {e_ac:.3e}'


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('depth', [2, 8])
def test_against_oracle_random_init(vited, gpu, dtype, depth):
    """Reference-style random init (timm init on the encoder side, PyTorch default on the decoder) +
    seeded gaussian pairs, config A at depth 2+2 and at the full 8+8, batch 8.  Well conditioned, so
    tolerances are tight: fp32 kernels rtol 1e-3 on logits and 1e-3 per gradient tensor (measured
    ~1e-6); bf16 MFMA path 3e-2 on logits, 5e-2 per gradient tensor, 2e-2 globally, and never worse
    than 1.5x what PyTorch's own CPU bf16 autocast of the oracle gives."""
    torch.manual_seed(0)
    s = vo.ViTEDShape(depth=depth, c_depth=depth)
    oracle = vo.OracleViTED(s)
    model = _hip_model(vited, s, gpu, dtype)
    model.load_state_dict(oracle.state_dict())
    x = torch.randn(8, 2, 3, 64, 64).clamp(-1, 1)
    y = (torch.rand(8, 4) > 0.75).float()

    def oracle_run(autocast):
        oracle.zero_grad()
        with torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
            out = oracle(x)
        torch.nn.functional.binary_cross_entropy_with_logits(out.float(), y).backward()
        return out.detach().float(), {n: p.grad.clone() for n, p in oracle.named_parameters()}

    lo, g32 = oracle_run(False)
    lh = model(x.to(gpu))
    torch.nn.functional.binary_cross_entropy_with_logits(lh, y.to(gpu)).backward()
    gh = {n: p.grad.cpu() for n, p in model.named_parameters()}
    exact = dtype == torch.float32
    torch.testing.assert_close(lh.detach().cpu(), lo, **(dict(rtol=1e-3, atol=1e-5) if exact else dict(rtol=3e-2, atol=3e-2)))

    def total(g):
        num = sum(float((g[n].double() - g32[n].double()).norm() ** 2) for n in g32)
        return (num / sum(float(g32[n].double().norm() ** 2) for n in g32)) ** 0.5

    for n in g32:
        err = float((gh[n] - g32[n]).norm() / (g32[n].norm() + 1e-12))
        assert err < (1e-3 if exact else 5e-2), f'{n}: relative gradient error {err:.3e}'
    if exact:
        assert total(gh) < 1e-4
    else:
        _, gac = oracle_run(True)
        assert total(gh) < 2e-2 and total(gh) <= 1.5 * total(gac) + 1e-3, (total(gh), total(gac))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('embed_dim,heads,batch', [(768, 12, 80), (192, 6, 16), (512, 8, 16)])
def test_other_widths_against_oracle(vited, gpu, dtype, embed_dim, heads, batch):
    """Widths other than the shipped 384 (the factory forwards MODEL.PJS.EMBED_DIM / NUM_HEADS, models/build.py:19-32): 768 with
    head dim 64 (two 384-wide k panels in the wide weight-gradient tile at batch 80 = 5,120+ rows, hidden 3072), 192 and 512
    (K not a multiple of 384: the 128 x 128 dW tile; 512 / 8 = head dim 64).  Random init, 1 + 1 blocks, against the fp32 oracle."""
    torch.manual_seed(1)
    s = vo.ViTEDShape(embed_dim=embed_dim, num_heads=heads, depth=1, c_depth=1)
    oracle = vo.OracleViTED(s)
    model = _hip_model(vited, s, gpu, dtype)
    model.load_state_dict(oracle.state_dict())
    x = torch.randn(batch, 2, 3, 64, 64).clamp(-1, 1)
    y = (torch.rand(batch, 4) > 0.75).float()
    out = oracle(x)
    torch.nn.functional.binary_cross_entropy_with_logits(out.float(), y).backward()
    lh = model(x.to(gpu))
    torch.nn.functional.binary_cross_entropy_with_logits(lh, y.to(gpu)).backward()
    exact = dtype == torch.float32
    torch.testing.assert_close(lh.detach().cpu(), out.detach().float(), **(dict(rtol=1e-3, atol=1e-5) if exact else dict(rtol=3e-2, atol=3e-2)))
    num = den = 0.0
    for (n, p), q in zip(model.named_parameters(), oracle.parameters()):
        g, r = p.grad.cpu().double(), q.grad.double()
        err = float((g - r).norm() / (r.norm() + 1e-12))
        assert err < (1e-3 if exact else 6e-2), f'{n}: relative gradient error {err:.3e}'
        num += float((g - r).norm() ** 2)
        den += float(r.norm() ** 2)
    assert (num / den) ** 0.5 < (1e-4 if exact else 2.5e-2)


@pytest.mark.parametrize('case', ['rand8', 'A_full', 'H_4x4_512'])
def test_bf16_error_growth_per_block(vited, gpu, case):
    """Where bf16 error enters, block by block (taps in functions.py): the output of every encoder / decoder block in
    forward and the gradient w.r.t. every block's input in backward, HIP bf16 vs the fp32 oracle, next to PyTorch's own CPU
    bf16 autocast of the oracle on the same inputs.  The MFMA path may not lose accuracy faster than autocast at any block
    (1.3x + 2e-3), on reference-style random init (well conditioned) and on the 8+8-block closed-form fixture (the case whose
    gradient error was 2.9x autocast's in round 1)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('diag_bf16_gradients', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'diag_bf16_gradients.py'))
    diag = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(diag)
    r = diag.anatomy(case, gpu)
    for name, fwd_hip, fwd_ac, dx_hip, dx_ac in r['rows']:
        assert fwd_hip <= 1.3 * fwd_ac + 2e-3, f'{case} {name}: forward error {fwd_hip:.3e} vs autocast {fwd_ac:.3e}'
        assert dx_hip <= 1.3 * dx_ac + 2e-3, f'{case} {name}: d(input) error {dx_hip:.3e} vs autocast {dx_ac:.3e}'
    assert r['grads'][0] <= 1.25 * r['grads'][1] + 1e-3, r['grads']
    assert r['logits'][0] <= 1.3 * r['logits'][1] + 1e-3, r['logits']
    if case == 'A_full':
        # the tensors the textbook delta = rowsum(dO o O) hurt (near-uniform attention): now within reach of autocast
        for n in ('cross_blocks.7.cross_attn.q.weight', 'cross_blocks.0.cross_attn.q.weight'):
            e_hip, e_ac, _ = r['per_param'][n]
            assert e_hip <= 3 * e_ac + 5e-2, f'{n}: HIP {e_hip:.3e} vs autocast {e_ac:.3e}'


def test_train_equals_eval_and_no_grad_saves_nothing(vited, gpu):
    s = vo.ViTEDShape(depth=1, c_depth=1)
    model = vo.fill_closed_form_(_hip_model(vited, s, gpu, torch.bfloat16))
    x = vo.closed_form_pairs(4, s).to(gpu)
    with torch.no_grad():
        a = model.train()(x)
        b = model.eval()(x)
    assert torch.equal(a, b) and not a.requires_grad


def test_autocast_selects_the_mfma_path(vited, gpu):
    s = vo.ViTEDShape(depth=1, c_depth=1)
    model = vo.fill_closed_form_(_hip_model(vited, s, gpu, None))
    x = vo.closed_form_pairs(2, s).to(gpu)
    with torch.no_grad():
        y32 = model(x)
        assert vited.ops.last_paths()[0] == 1          # outside autocast: fp32 kernels
        with torch.autocast('cuda', dtype=torch.bfloat16):
            y16 = model(x)
        assert y16.dtype == torch.float32
    torch.testing.assert_close(y16, y32, rtol=3e-2, atol=3e-2)
    assert not torch.equal(y16, y32)


def test_hisfrag_two_stage_training_step(vited, gpu):
    """hisfrag.py:117-159: encoder once per image, gather pairs, decoder on pairs, one backward."""
    s = vo.ViTEDShape(img_size=128, patch_size=16, num_classes=1, num_heads=6, depth=1, c_depth=1)
    torch.manual_seed(1)
    oracle = vo.OracleViTED(s)
    model = _hip_model(vited, s, gpu, torch.float32)
    model.load_state_dict(oracle.state_dict())
    imgs = torch.randn(6, 3, 128, 128).clamp(-1, 1)
    i0 = torch.tensor([0, 0, 1, 2, 4, 5, 3])
    i1 = torch.tensor([1, 2, 2, 5, 5, 0, 3])
    labels = torch.tensor([1., 1, 1, 0, 0, 0, 1]).view(-1, 1)

    def step(m, imgs, i0, i1, labels):
        feats = m(imgs, forward_first_part=True)
        out = m(feats[i1], imgs[i0])
        torch.nn.functional.binary_cross_entropy_with_logits(out, labels).backward()
        return out

    lo = step(oracle, imgs, i0, i1, labels)
    lh = step(model, imgs.to(gpu), i0.to(gpu), i1.to(gpu), labels.to(gpu))
    torch.testing.assert_close(lh.cpu(), lo.detach(), rtol=1e-3, atol=1e-5)
    og = dict(oracle.named_parameters())
    for n, p in model.named_parameters():
        err = (p.grad.cpu() - og[n].grad).norm() / (og[n].grad.norm() + 1e-12)
        assert err < 1e-3, f'{n}: {err:.3e}'


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_pairwise_similarity_matches_the_oracle(vited, gpu, dtype):
    """BASELINE config 5 on one rank against the CPU ORACLE: encoder once per image + decoder on gathered pairs (image-2
    gather by index inside the patch-embed kernel, features by index, pair batch 64) == the oracle's naive one-shot forward
    on stacked pairs (tests/hisfrag_evaluation_test.py:18-99 ``eval_standard``).  H-shaped block: 6 heads x 64, 256 / 257
    tokens (the flash attention kernels), 1 + 1 blocks.  fp32 kernels: 1e-3; bf16: 3e-2 (scores are stored as fp16)."""
    s = vo.ViTEDShape(img_size=256, patch_size=16, num_classes=1, num_heads=6, depth=1, c_depth=1)
    torch.manual_seed(11)
    oracle = vo.OracleViTED(s).eval()
    model = _hip_model(vited, s, gpu, dtype).eval()
    model.load_state_dict(oracle.state_dict())
    g = torch.Generator().manual_seed(5)
    n = 13
    imgs = torch.randn(n, 3, 256, 256, generator=g).clamp(-1, 1)
    sim = vited.engine.pairwise_similarity(model, imgs.to(gpu), block=5, pair_batch=64, amp=dtype == torch.bfloat16)
    # the uncached form (features gathered per pair batch, image 2 re-embedded per pair: what hisfrag.py:226-229 does) agrees
    plain = vited.engine.pairwise_similarity(model, imgs.to(gpu), block=5, pair_batch=64, amp=dtype == torch.bfloat16, pair_cache=False)
    torch.testing.assert_close(sim.float(), plain.float(), rtol=1e-2, atol=1e-2)
    i, j = torch.triu_indices(n, n)
    with torch.no_grad():
        ref = oracle(torch.stack([imgs[i], imgs[j]], dim=1)).reshape(-1)
    tol = dict(rtol=2e-3, atol=2e-3) if dtype == torch.float32 else dict(rtol=3e-2, atol=3e-2)   # fp16 storage: 1e-3 relative
    torch.testing.assert_close(sim[i, j].float().cpu(), ref, **tol)
    assert torch.equal(sim, sim.t()) and sim.dtype == torch.float16
    with pytest.raises(NotImplementedError):
        model(model(imgs[:2].to(gpu), forward_first_part=True), imgs.to(gpu), x2_index=torch.tensor([0, 1], device=gpu))


def test_batch_1024_rows_match_batch_8(vited, gpu):
    """The bench geometry on the default kernel path: config A, bf16, B = 1024 (token matrices of 65,536 / 66,560 rows:
    512-1,560 output tiles, the XCD remap, the 512-way split weight-gradient GEMMs).  Rows 0..7 of the 1024-batch must give
    the logits - and, with a loss that only sees those rows, the parameter gradients - of the same 8 pairs run alone.
    Both runs round to bf16 at the same places, so they differ only by fp32 summation order inside tiles and splits."""
    s = vo.SHAPE_A
    torch.manual_seed(4)
    model = _hip_model(vited, s, gpu, torch.bfloat16)
    x = torch.randn(1024, 2, 3, 64, 64, device=gpu).clamp_(-1, 1)
    y = (torch.rand(1024, 4, device=gpu) > 0.75).float()

    def run(xb, yb):
        model.zero_grad(set_to_none=True)
        out = model(xb)
        torch.nn.functional.binary_cross_entropy_with_logits(out[:8], yb[:8]).backward()
        return out.detach()[:8].clone(), {n: p.grad.clone() for n, p in model.named_parameters()}

    l_small, g_small = run(x[:8], y[:8])
    l_big, g_big = run(x, y)
    torch.testing.assert_close(l_big, l_small, rtol=2e-2, atol=2e-2)
    num = sum(float((g_big[n].double() - g_small[n].double()).norm() ** 2) for n in g_small)
    den = sum(float(g_small[n].double().norm() ** 2) for n in g_small)
    assert (num / den) ** 0.5 < 2e-2, f'global gradient difference {(num / den) ** 0.5:.3e}'
    gmax = max(float(v.norm()) for v in g_small.values())
    for n in g_small:
        den = float(g_small[n].norm())
        if den < 1e-3 * gmax:
            continue
        err = float((g_big[n] - g_small[n]).norm()) / den
        assert err < 5e-2, f'{n}: B=1024 vs B=8 gradient differs by {err:.3e}'


def test_mine_pairs_on_device(vited, gpu):
    """engine.mine_pairs / hisfrag_prepare_data on GPU tensors (hisfrag.py:117-155): same pairs as the literal loop."""
    eng = vited.engine
    g = torch.Generator().manual_seed(5)
    for n, classes in ((24, 8), (7, 2), (5, 5)):
        targets = torch.randint(0, classes, (n,), generator=g)
        pos_ref = [(i, j) for i in range(n) for j in range(i + 1, n) if targets[i] == targets[j]]
        neg_ref = {(i, j) for i in range(n) for j in range(i + 1, n) if targets[i] != targets[j]}
        groups, labels = eng.mine_pairs(targets.to(gpu))
        assert groups.device.type == 'cuda' and labels.device.type == 'cuda'
        npos, nneg = len(pos_ref), min(len(neg_ref), 2 * len(pos_ref))
        assert groups.shape == (npos + nneg, 2)
        assert [tuple(r) for r in groups[:npos].tolist()] == pos_ref
        got = [tuple(r) for r in groups[npos:].tolist()]
        assert len(set(got)) == nneg and set(got) <= neg_ref
        assert labels[:npos].eq(1).all() and labels[npos:].eq(0).all()
    s = vo.ViTEDShape(img_size=64, patch_size=8, num_classes=1, depth=1, c_depth=1)
    model = vo.fill_closed_form_(_hip_model(vited, s, gpu, torch.float32))
    imgs = torch.randn(6, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)
    targets = torch.tensor([0, 0, 1, 1, 2, 0], device=gpu)
    (x2, feats), labels = eng.hisfrag_prepare_data(model, imgs, targets, amp=False)
    out = model(feats, x2)
    assert out.shape == labels.shape and feats.requires_grad
    torch.nn.functional.binary_cross_entropy_with_logits(out, labels).backward()
    assert model.blocks[0].attn.qkv.weight.grad is not None      # one backward through both forwards (hisfrag.py:150-159)


@pytest.mark.parametrize('shape', ['A2', 'one_class', 'T'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_direct_gradient_accumulation_matches_autograd(vited, gpu, dtype, shape):
    """engine.FlatGradients mode: the weight-gradient / LayerNorm kernels add straight into p.grad (views of
    one flat buffer) instead of returning tensors for autograd to accumulate.  Same numbers, and a second
    backward accumulates (ACCUMULATION_STEPS > 1, misc/engine.py:202-231)."""
    # 'one_class': the [1, 384] head of config H (odd widths in the slab reductions); 'T': the tiny test config
    s = {'A2': vo.ViTEDShape(depth=2, c_depth=2), 'one_class': vo.ViTEDShape(depth=1, c_depth=1, num_classes=1),
         'T': vo.SHAPE_T}[shape]
    torch.manual_seed(2)
    ref = _hip_model(vited, s, gpu, dtype)
    dut = _hip_model(vited, s, gpu, dtype)
    dut.load_state_dict(ref.state_dict())
    x = torch.randn(6, 2, 3, s.img_size, s.img_size, device=gpu).clamp(-1, 1)
    y = (torch.rand(6, s.num_classes, device=gpu) > 0.75).float()
    torch.nn.functional.binary_cross_entropy_with_logits(ref(x), y).backward()
    flat = vited.engine.FlatGradients(dut.parameters())
    dut.direct_param_grads = True
    for rep in (1, 2):
        torch.nn.functional.binary_cross_entropy_with_logits(dut(x), y).backward()
        assert vited.ops.last_paths()[0] in (1, 2)
        for (n, p), (_, q) in zip(ref.named_parameters(), dut.named_parameters()):
            assert q.grad.data_ptr() >= flat.flat.data_ptr() and q.grad.data_ptr() < flat.flat.data_ptr() + flat.flat.numel() * 4, n
            torch.testing.assert_close(q.grad, rep * p.grad, rtol=1e-4, atol=1e-6 * float(p.grad.abs().max() + 1), msg=lambda m: f'{n}: {m}')


@pytest.mark.parametrize('shape', ['A1', 'one_class'])
def test_train_step_graph_replay_matches_eager_steps_and_the_oracle(vited, gpu, shape):
    """engine.TrainStep (misc/engine.py:189-257 + misc/utils.py:212-226 re-plumbed): forward, BCE, backward into the flat
    gradient buffer, clip 5.0, AdamW.  The hipGraph-replayed step (the bench.py path) must produce the parameters of the
    eagerly launched one bit for bit (same kernels, same order, no atomics anywhere), and both must track the CPU oracle
    trained with the same optimizer settings (fp32 kernels: losses within 1e-3, parameters within 5e-3 after 5 steps)."""
    s = {'A1': vo.ViTEDShape(depth=1, c_depth=1), 'one_class': vo.ViTEDShape(depth=1, c_depth=1, num_classes=1)}[shape]
    torch.manual_seed(3)
    oracle = vo.OracleViTED(s)
    models = [_hip_model(vited, s, gpu, torch.float32) for _ in range(2)]
    for m in models:
        m.load_state_dict(oracle.state_dict())
    mk = lambda params: torch.optim.AdamW(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    steps = [vited.engine.TrainStep(m, torch.optim.AdamW(m.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05,
                                                        fused=True, capturable=True), clip_grad=5.0, amp=False, use_graph=g)
             for m, g in zip(models, (False, True))]
    opt_o = mk(oracle.parameters())
    g = torch.Generator().manual_seed(9)
    for it in range(5):
        x = torch.randn(8, 2, 3, 64, 64, generator=g).clamp(-1, 1)
        y = (torch.rand(8, s.num_classes, generator=g) > 0.6).float()
        losses = [float(st.step(x.to(gpu), y.to(gpu))) for st in steps]
        opt_o.zero_grad(set_to_none=True)
        lo = torch.nn.functional.binary_cross_entropy_with_logits(oracle(x), y)
        lo.backward()
        torch.nn.utils.clip_grad_norm_(oracle.parameters(), 5.0)
        opt_o.step()
        assert losses[0] == losses[1], (it, losses)
        assert abs(losses[0] - float(lo.detach())) < 1e-3 * max(1.0, abs(float(lo.detach()))), (it, losses, float(lo.detach()))
    assert steps[1]._g1 is not None          # the graph path really replayed (2 eager warm-ups, then capture)
    po = dict(oracle.named_parameters())
    for (n, pe), (_, pg) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert torch.equal(pe, pg), f'{n}: graph replay differs from eager launches'
        err = (pe.detach().cpu() - po[n].detach()).norm() / (po[n].detach().norm() + 1e-12)
        # AdamW's g / sqrt(v) update is scale-free, so it amplifies fp32 rounding differences of tiny gradients: 5e-3
        assert err < 5e-3, f'{n}: {err:.3e} vs the oracle after 5 AdamW steps'


def test_uint8_inputs_and_prefetcher(vited, gpu):
    """uint8 pixels go straight into the patch-embedding kernel (ToTensor + Normalize(0.5, 0.5) of
    data/transforms.py:14-18 folded in) and ``engine.DevicePrefetcher`` copies batches one ahead on a side stream.  Same logits
    as the reference pipeline's fp32 tensors; same batches, same order as the wrapped loader."""
    s = vo.ViTEDShape(depth=1, c_depth=1)
    model = vo.fill_closed_form_(_hip_model(vited, s, gpu, torch.float32))
    g = torch.Generator().manual_seed(2)
    batches = [(torch.randint(0, 256, (5, 2, 3, 64, 64), generator=g, dtype=torch.uint8), torch.rand(5, 4, generator=g)) for _ in range(5)]
    as_float = lambda u8: (u8.float() / 255.0 - 0.5) / 0.5
    with torch.no_grad():
        want = [model(as_float(x).to(gpu)) for x, _ in batches]
        got = []
        for (x, y), (x0, y0) in zip(vited.engine.DevicePrefetcher(batches, gpu, depth=2), batches):
            assert x.dtype == torch.uint8 and x.device.type == 'cuda' and torch.equal(x.cpu(), x0) and torch.equal(y.cpu(), y0)
            got.append(model(x))
    assert len(got) == len(want)
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
    # op level: bit-equal to the fp32 patchify of the normalised image computed with the same fma
    x = batches[0][0][:, 0].to(gpu)
    ref = vited.ops.patchify(torch.addcmul(torch.full((5, 3, 64, 64), -1.0, device=gpu), x.float(), torch.full((1,), 1.0 / 127.5, device=gpu)), 8, torch.float32)
    torch.testing.assert_close(vited.ops.patchify(x, 8, torch.float32), ref, rtol=0, atol=2e-7)


def test_keep_attn_slow_path_matches_the_oracle(vited, gpu):
    """MODEL.PJS.KEEP_ATTN (vision_transformer.py:67-75,188-195; read by scripts/visualise_attentions.py:218-244): the fused
    kernels still produce the logits, and get_attn() / get_attn_gradients() return the materialised softmax(q k^T / sqrt(hd))
    and d loss / d attn of encoder self-attention, decoder self-attention and decoder cross-attention."""
    s = vo.ViTEDShape(depth=1, c_depth=1)
    torch.manual_seed(6)
    oracle = vo.OracleViTED(s)
    model = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, num_classes=s.num_classes, embed_dim=s.embed_dim,
                                          depth=1, c_depth=1, num_heads=s.num_heads, keep_attn=True).to(gpu)
    model.compute_dtype = torch.float32
    model.load_state_dict(oracle.state_dict())
    with pytest.raises(RuntimeError, match='no attention map'):
        model.blocks[0].attn.get_attn()
    x = torch.randn(3, 2, 3, 64, 64).clamp(-1, 1)
    y = (torch.rand(3, 4) > 0.5).float()
    out = model(x.to(gpu))
    torch.nn.functional.binary_cross_entropy_with_logits(out, y.to(gpu)).backward()
    # the oracle, opened up at the three attentions
    maps = {}

    def attn_of(q, k, key):
        a = torch.softmax((vo._heads(q, s.num_heads) * s.head_dim ** -0.5) @ vo._heads(k, s.num_heads).transpose(-2, -1), dim=-1)
        a.retain_grad()
        maps[key] = a
        return a

    def sdpa(a, v):
        o = a @ vo._heads(v, s.num_heads)
        return o.transpose(1, 2).reshape(o.shape[0], o.shape[2], -1)

    lin = torch.nn.functional.linear
    x1, x2 = torch.unbind(x, 1)
    t = oracle._patch_tokens(x1) + oracle.pos_embed[:, 1:]
    blk = oracle.blocks[0]
    q, k, v = lin(vo._ln(blk.norm1, t), blk.attn.qkv.weight, blk.attn.qkv.bias).chunk(3, -1)
    t = t + lin(sdpa(attn_of(q, k, 'enc'), v), blk.attn.proj.weight, blk.attn.proj.bias)
    feats = t + vo._mlp(blk.mlp, vo._ln(blk.norm2, t))
    u = oracle.prepare_x2(x2)
    blk = oracle.cross_blocks[0]
    q, k, v = lin(vo._ln(blk.norm1, u), blk.attn.qkv.weight, blk.attn.qkv.bias).chunk(3, -1)
    u = u + lin(sdpa(attn_of(q, k, 'dec'), v), blk.attn.proj.weight, blk.attn.proj.bias)
    ca = blk.cross_attn
    q = lin(vo._ln(blk.norm_cross, u), ca.q.weight, ca.q.bias)
    k, v = lin(vo._ln(blk.norm_context, feats), ca.kv.weight, ca.kv.bias).chunk(2, -1)
    u = u + lin(sdpa(attn_of(q, k, 'cross'), v), ca.proj.weight, ca.proj.bias)
    u = u + vo._mlp(blk.mlp, vo._ln(blk.norm2, u))
    lo = oracle.forward_head(vo._ln(oracle.norm, u))
    torch.nn.functional.binary_cross_entropy_with_logits(lo, y).backward()
    torch.testing.assert_close(out.detach().cpu(), lo.detach(), rtol=1e-3, atol=1e-5)
    for key, mod in (('enc', model.blocks[0].attn), ('dec', model.cross_blocks[0].attn), ('cross', model.cross_blocks[0].cross_attn)):
        torch.testing.assert_close(mod.get_attn().cpu(), maps[key].detach(), rtol=1e-3, atol=1e-6, msg=lambda m: f'{key} map: {m}')
        g = maps[key].grad
        torch.testing.assert_close(mod.get_attn_gradients().cpu(), g, rtol=2e-3, atol=1e-6 * float(g.abs().max()) + 1e-9, msg=lambda m: f'{key} grad: {m}')


# ---------------------------------------------------------------------------------------------
# round-3 additions: branches that only the bench shapes reached ("what's weak" 2-5)
# ---------------------------------------------------------------------------------------------
def test_mlp_no_grad_fused_head_plus_unfused_tail(vited, gpu):
    """functions._mlp_fwd on the no-grad path splits a large row count into a head that the one-kernel MLP (vited_mlp_fwd,
    one 128-row workgroup per CU) takes and a tail of < 64 tiles that goes to LayerNorm + fc1/GELU + fc2/residual: config-A
    eval at B = 1024 (66,560 rows -> 8 tail tiles) and H inference at pair batch 512 (524,800 rows -> 4 tail tiles).  Here:
    33,445 rows = 256 full tiles (fused) + 5 tiles + 37 ragged rows (tail), against a plain PyTorch fp32 evaluation of
    x + fc2(gelu(fc1(LayerNorm(x)))) (timm Mlp, vision_transformer.py:115,126) on every row.  bf16 tolerance 3e-2."""
    F_ = vited.functions
    rt = F_.Runtime(img_size=64, patch_size=8, in_chans=3, num_classes=4, embed_dim=384, depth=1, c_depth=1, num_heads=12)
    rows = 256 * 128 + 5 * 128 + 37
    g = torch.Generator(device=gpu).manual_seed(12)
    x = torch.randn(rows, 384, device=gpu, generator=g)
    gamma = 1.0 + 0.1 * torch.randn(384, device=gpu, generator=g)
    beta = 0.1 * torch.randn(384, device=gpu, generator=g)
    w1 = torch.randn(1536, 384, device=gpu, generator=g) * 0.05
    b1 = torch.randn(1536, device=gpu, generator=g) * 0.05
    w2 = torch.randn(384, 1536, device=gpu, generator=g) * 0.05
    b2 = torch.randn(384, device=gpu, generator=g) * 0.05
    head = F_._fused_mlp_rows(rt, x, w1, False)
    assert head == 256 * 128 and 0 < rows - head < 64 * 128, 'the case must split into a fused head and an unfused tail'
    calls = []
    real = vited.ops.mlp_fwd, vited.ops.gemm
    vited.ops.mlp_fwd = lambda *a, **k: (calls.append(('fused', a[0].shape[0])), real[0](*a, **k))[1]
    vited.ops.gemm = lambda *a, **k: (calls.append(('gemm', a[0].shape[0])), real[1](*a, **k))[1]
    try:
        with torch.no_grad():
            block = F_.EncBlock._make([None] * len(F_.EncBlock._fields))._replace(g2=gamma, b2=beta, w1=w1, bb1=b1, w2=w2, bb2=b2)
            y, saved, _ = F_._mlp_fwd(rt, x, block, grad=False)
    finally:
        vited.ops.mlp_fwd, vited.ops.gemm = real
    assert saved is None and ('fused', head) in calls and ('gemm', rows - head) in calls, calls
    h = torch.nn.functional.layer_norm(x, (384,), gamma, beta, 1e-6)
    want = x + torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(h, w1, b1)), w2, b2)
    torch.testing.assert_close(y, want, rtol=3e-2, atol=3e-2)
    # the seam: last fused rows and first tail rows are as accurate as the rest
    err = (y - want).abs().amax(dim=1)
    assert float(err[head - 128: head + 128].max()) <= 2.0 * float(err.median()) + 2e-2


def test_eval_batch_1024_matches_the_oracle(vited, gpu):
    """Config-A evaluation at B = 1024 (no grad, bf16): the decoder's 66,560-row MLPs take the fused-head + unfused-tail
    split, the encoder's 65,536-row ones the fused kernel alone.  Pairs 0-3 and the LAST four pairs (their decoder rows sit
    in the unfused tail: rows >= 65,536 = pairs >= 1008) against the CPU fp32 oracle on the same weights; 3e-2."""
    s = vo.SHAPE_A
    torch.manual_seed(8)
    oracle = vo.OracleViTED(s).eval()
    model = _hip_model(vited, s, gpu, torch.bfloat16).eval()
    model.load_state_dict(oracle.state_dict())
    x = torch.randn(1024, 2, 3, 64, 64).clamp_(-1, 1)
    with torch.no_grad():
        got = model(x.to(gpu)).cpu()
        pick = torch.tensor([0, 1, 2, 3, 1020, 1021, 1022, 1023])
        want = oracle(x[pick])
    torch.testing.assert_close(got[pick], want, rtol=3e-2, atol=3e-2)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_uint8_inputs_match_the_oracle(vited, gpu, dtype):
    """uint8 pixels through ``vited_patchify_u8`` against the ORACLE fed what the reference's transform produces from the same
    pixels: ToTensor + Normalize(0.5, 0.5) = (u8 / 255 - 0.5) / 0.5 (data/transforms.py:14-18).  Logits and gradients."""
    s = vo.ViTEDShape(depth=1, c_depth=1)
    torch.manual_seed(14)
    oracle = vo.OracleViTED(s)
    model = _hip_model(vited, s, gpu, dtype)
    model.load_state_dict(oracle.state_dict())
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (6, 2, 3, 64, 64), generator=g, dtype=torch.uint8)
    y = (torch.rand(6, 4, generator=g) > 0.6).float()
    lo = oracle((u8.float() / 255.0 - 0.5) / 0.5)
    torch.nn.functional.binary_cross_entropy_with_logits(lo, y).backward()
    lh = model(u8.to(gpu))
    torch.nn.functional.binary_cross_entropy_with_logits(lh, y.to(gpu)).backward()
    exact = dtype == torch.float32
    torch.testing.assert_close(lh.detach().cpu(), lo.detach(), **(dict(rtol=1e-3, atol=1e-5) if exact else dict(rtol=3e-2, atol=3e-2)))
    og = dict(oracle.named_parameters())
    for n, p in model.named_parameters():
        err = float((p.grad.cpu() - og[n].grad).norm() / (og[n].grad.norm() + 1e-12))
        assert err < (1e-3 if exact else 6e-2), f'{n}: relative gradient error {err:.3e}'


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_pair_cached_decoder_at_config_h_tokens_pair_batch_512(vited, gpu, dtype):
    """BASELINE config 5's own shape: 1024 / 1025 tokens, 6 x 64 heads, pair batch 512 (README.md:63) through
    ``engine.pairwise_similarity`` with the pair cache (image-2 tokens + block-0 branch cached per image, K / V per row block,
    ``vited_attention_fwd_indexed``), at 1 + 3 blocks so that the decoder runs its three kinds of block: the cached first one,
    a full middle one and the cls-only last one.  32 images -> 528 pairs = one batch of 512 + one of 16; 20 sampled pairs
    (from both batches) against the CPU oracle's naive one-shot forward on stacked pairs (hisfrag.py:226-229)."""
    s = vo.ViTEDShape(img_size=512, patch_size=16, num_classes=1, num_heads=6, depth=1, c_depth=3)
    torch.manual_seed(21)
    oracle = vo.OracleViTED(s).eval()
    model = _hip_model(vited, s, gpu, dtype).eval()
    model.load_state_dict(oracle.state_dict())
    n = 32
    imgs = torch.randn(n, 3, 512, 512, generator=torch.Generator().manual_seed(6)).clamp(-1, 1)
    sim = vited.engine.pairwise_similarity(model, imgs.to(gpu), block=32, pair_batch=512, amp=dtype == torch.bfloat16)
    i, j = torch.triu_indices(n, n)
    assert i.numel() == 528
    pick = torch.cat([torch.arange(0, 512, 32), torch.arange(512, 528, 4)])          # 16 pairs of the first batch + 4 of the second
    with torch.no_grad():
        ref = oracle(torch.stack([imgs[i[pick]], imgs[j[pick]]], dim=1)).reshape(-1)
    tol = dict(rtol=2e-3, atol=2e-3) if dtype == torch.float32 else dict(rtol=3e-2, atol=3e-2)   # fp16 storage: 1e-3 relative
    torch.testing.assert_close(sim[i[pick], j[pick]].float().cpu(), ref, **tol)
    assert torch.equal(sim, sim.t()) and bool(torch.isfinite(sim.float()).all())


def test_streamed_similarity_is_block_resident_resumable_and_matches_the_oracle(vited, gpu, tmp_path):
    """``engine.pairwise_similarity`` with the HIP model streams (hisfrag.py:181-231): images come from the HOST as uint8 blocks
    (a callable source, like the reference's per-row-block DataLoader), only ``block`` row images and ``col_block`` column
    images are resident, finished row blocks are saved and skipped on a restart (hisfrag.py:181-195,243-246).
      * parity: every pair against the CPU oracle's naive one-shot forward on (u8 / 255 - 0.5) / 0.5;
      * resume: a run killed after three row blocks and restarted equals the uninterrupted run bit for bit, and the restart
        does not touch the finished rows again;
      * residency: the peak of allocated device memory does not grow with the number of images (24 vs 96)."""
    s = vo.ViTEDShape(img_size=128, patch_size=16, num_classes=1, num_heads=6, depth=1, c_depth=2)
    torch.manual_seed(23)
    oracle = vo.OracleViTED(s).eval()
    model = _hip_model(vited, s, gpu, torch.bfloat16).eval()
    model.load_state_dict(oracle.state_dict())
    g = torch.Generator().manual_seed(9)
    n = 37
    u8 = torch.randint(0, 256, (96, 3, 128, 128), generator=g, dtype=torch.uint8)
    touched = []

    def source(lo, hi):                       # host-side loader: returns uint8 CPU blocks
        touched.append((lo, hi))
        return u8[lo:hi]

    kw = dict(block=5, col_block=7, pair_batch=16, amp=True)
    sim = vited.engine.pairwise_similarity(model, source, n_images=n, **kw)
    assert sim.shape == (n, n) and sim.dtype == torch.float16 and torch.equal(sim, sim.t())
    i, j = torch.triu_indices(n, n)
    f = (u8[:n].float() / 255.0 - 0.5) / 0.5
    with torch.no_grad():
        ref = torch.cat([oracle(torch.stack([f[i[k:k + 64]], f[j[k:k + 64]]], dim=1)).reshape(-1) for k in range(0, i.numel(), 64)])
    torch.testing.assert_close(sim[i, j].float().cpu(), ref, rtol=3e-2, atol=3e-2)
    # a host tensor works like the callable
    assert torch.equal(vited.engine.pairwise_similarity(model, u8[:n], **kw), sim)

    # kill after the third row block, restart from the saved state
    state = str(tmp_path / 'similarity_rank0.pt')

    class Killed(Exception):
        pass

    def kill_after_three(a0, a1):
        if a1 >= 15:
            raise Killed

    with pytest.raises(Killed):
        vited.engine.pairwise_similarity(model, source, n_images=n, state_path=state, after_row_block=kill_after_three, **kw)
    saved = torch.load(state, weights_only=True)
    assert saved['done_rows'] == 15 and not saved['is_finished']
    touched.clear()
    resumed = vited.engine.pairwise_similarity(model, source, n_images=n, state_path=state, **kw)
    assert torch.equal(resumed, sim), 'a resumed run must equal the uninterrupted one'
    assert min(lo for lo, _ in touched) >= 15, f'finished rows were read again: {touched[:4]}'
    assert torch.load(state, weights_only=True)['is_finished']
    # a state file of another run (different image count) is ignored, not trusted
    again = vited.engine.pairwise_similarity(model, source, n_images=n - 1, state_path=state, **kw)
    assert torch.equal(again, sim[:n - 1, :n - 1])

    # residency: O(block + col_block), not O(n)
    def peak(count):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        vited.engine.pairwise_similarity(model, source, n_images=count, **kw)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    p24, p96 = peak(24), peak(96)
    per_image_cache = 65 * 384 * (4 + 2)           # image-2 tokens fp32 + cached queries bf16, what an all-image cache would hold
    assert p96 - p24 < 8 * per_image_cache + 96 * 96 * 2 + 4 * 96 * 97 // 2 + (1 << 20), (p24, p96)
    assert 72 * per_image_cache > 8 * per_image_cache + (2 << 20)    # i.e. the bound is far below what 72 more resident images cost


def test_folded_context_kv_matches_the_per_block_form(vited, gpu):
    """norm_context + kv of all decoder blocks through folded weights (functions._context_kv_folded, csrc/context_fold.hip) against
    the per-block LayerNorm + Linear it replaces.  Reference-style random init with every LayerNorm's gamma / beta moved away from
    1 / 0 (at the init itself the fold is the identity) - a well-conditioned case, so the comparison is direct: the folded bf16 run
    and the per-block bf16 run must both sit within bf16 distance of the fp32 kernels, per tensor, for the logits, d(features) and
    the gradients that travel through the fold: norm_context.{weight, bias}, cross_attn.kv.{weight, bias} (kv.weight also receives
    the bias path's  db' beta^T  term)."""
    s = vo.ViTEDShape(depth=1, c_depth=3)
    torch.manual_seed(17)
    oracle = vo.OracleViTED(s)
    g = torch.Generator().manual_seed(18)
    with torch.no_grad():
        for n, p in oracle.named_parameters():
            if 'norm' in n and n.endswith('weight'):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
            elif 'norm' in n and n.endswith('bias'):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
    x = torch.randn(6, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)
    y = (torch.rand(6, 4, generator=g) > 0.6).float().to(gpu)
    runs = {}
    for tag, dtype, fold in (('fp32', torch.float32, False), ('folded', torch.bfloat16, True), ('per_block', torch.bfloat16, False)):
        model = _hip_model(vited, s, gpu, dtype)
        model.load_state_dict(oracle.state_dict())
        model.runtime().fold_context = fold
        feats = model(x[:, 0], forward_first_part=True)
        leaf = feats.detach().requires_grad_(True)
        logits = model(leaf, x[:, 1])
        torch.nn.functional.binary_cross_entropy_with_logits(logits, y).backward()
        runs[tag] = (logits.detach(), leaf.grad.clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    rel = lambda a, b: float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))
    l32, d32, g32 = runs['fp32']
    for tag in ('folded', 'per_block'):
        torch.testing.assert_close(runs[tag][0], l32, rtol=3e-2, atol=3e-2)
    e_fold, e_blk = rel(runs['folded'][1], d32), rel(runs['per_block'][1], d32)
    assert e_fold < 3e-2 and e_fold <= 1.5 * e_blk + 5e-3, f'd(features): folded {e_fold:.3e}, per block {e_blk:.3e}'
    checked = 0
    for n in g32:
        if 'norm_context' in n or 'cross_attn.kv' in n:
            e_fold, e_blk = rel(runs['folded'][2][n], g32[n]), rel(runs['per_block'][2][n], g32[n])
            assert e_fold < 4e-2 and e_fold <= 1.5 * e_blk + 1e-2, f'{n}: folded {e_fold:.3e} vs per-block {e_blk:.3e} (error against the fp32 kernels)'
            checked += 1
    assert checked == 12


@pytest.mark.gpu
def test_grouped_weight_gradient_launches_match_one_launch_per_block(vited, gpu):
    """functions._DwBatch sends the weight gradients of several blocks out in one launch (one row range per product
    when the tiles fill a round of workgroups) where round 3's first form launched once per block (up to 7 row ranges + a slab
    sum).  Same products, another fp32 summation order over the rows: every weight / bias gradient agrees to 1e-5 of its norm,
    everything that does not pass through a weight-gradient launch (logits, LayerNorm gradients) bit for bit."""
    s = vo.ViTEDShape(depth=3, c_depth=3)
    torch.manual_seed(5)
    oracle = vo.OracleViTED(s)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(72, 2, 3, 64, 64, generator=g).clamp(-1, 1).to(gpu)      # 72 x 64 = 4,608 rows: the products are queued (>= 4,096)
    y = (torch.rand(72, 4, generator=g) > 0.6).float().to(gpu)
    runs = {}
    for grouped in (True, False):
        model = _hip_model(vited, s, gpu, torch.bfloat16)
        model.load_state_dict(oracle.state_dict())
        model.runtime().group_dw = grouped
        logits = model(x)
        torch.nn.functional.binary_cross_entropy_with_logits(logits, y).backward()
        runs[grouped] = (logits.detach(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    assert torch.equal(runs[True][0], runs[False][0])
    checked = 0
    for n, a in runs[True][1].items():
        b = runs[False][1][n]
        if 'norm' in n or n in ('cls_token', 'pos_embed'):
            assert torch.equal(a, b), n
        else:
            err = float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))
            assert err < 1e-5, f'{n}: {err:.2e}'
            checked += 1
    assert checked >= 40
