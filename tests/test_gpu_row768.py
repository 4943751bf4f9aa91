"""The row-complete Linear + LayerNorm kernels at N == 768 (gemm_row768.hip) on the MI355X: forward, backward, the scaled and
segmented forms, launch-to-launch reproducibility, a 768-wide model against the oracle with the kernels on and off, and a guard
that the 384-wide dispatch did not move.

The kernel tests call the entries directly: those take every shape the kernels compute, while ``linear_layernorm_supported`` also
holds the measured speed rule and sends a model's small products to the two kernels.
Bounds are those of the 384 tests (tests/test_gpu_ops.py, test_linear_residual_layernorm_fwd / test_linear_layernorm_bwd): fp64
references on the same bf16-rounded operands.  Everything here except the 384 guard fails before the 768-wide kernels exist
(``linear_layernorm_supported`` is false and the entries answer "unsupported").

Run as a script (``python tests/test_gpu_row768.py``) this file is the model case alone: the child process of
test_model_768_without_the_fused_kernels, which needs VITED_FUSED_LN read afresh."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

N = 768
BF16_OUT = dict(rtol=1e-2, atol=1e-2)
SMALL_M = (13, 64, 577, 3 * 577, 4096 + 33)
FWD_SHAPES = [(m, k) for m in SMALL_M for k in (768, 3072)] + [(1000, 1536), (24 * 576, 768), (72 * 577, 3072)]
BWD_SHAPES = [(m, k) for m in SMALL_M for k in (768, 1536, 2304, 3072)] + [(1000, 1536), (24 * 576, 768), (72 * 577, 3072)]


def _rand(shape, dev, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev).to(dtype)


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, float('nan'), dtype=dtype, device=dev)


def _fwd_operands(gpu, M, K, n=N):
    a = _rand((M, K), gpu, 1 + M, 1.0, torch.bfloat16)
    w = _rand((n, K), gpu, 2 + K, K ** -0.5, torch.bfloat16)
    bias, res = _rand((n,), gpu, 3, 0.5), _rand((M, n), gpu, 4, 2.0)
    gamma, beta = 1.0 + _rand((n,), gpu, 5, 0.2), _rand((n,), gpu, 6, 0.2)
    return a, w, bias, res, gamma, beta


def _check_fwd(y, h, mean, rstd, ref, gamma, beta, K):
    torch.testing.assert_close(y.double(), ref, rtol=1e-5, atol=2e-5 * K ** 0.5)
    mu = ref.mean(dim=1)
    var = ref.var(dim=1, unbiased=False)
    torch.testing.assert_close(mean.double(), mu, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(rstd.double(), (var + 1e-6).rsqrt(), rtol=1e-4, atol=1e-6)
    href = (ref - mu[:, None]) * (var[:, None] + 1e-6).rsqrt() * gamma.double() + beta.double()
    torch.testing.assert_close(h.double(), href, **BF16_OUT)


@pytest.mark.parametrize('M,K', FWD_SHAPES)
def test_forward(vited, gpu, M, K):
    """y = residual + [scale *] (a W^T + b) and h = LayerNorm(y) against fp64: ragged M (partial last tile, 64- and 96-row tiles, one
    to 433 workgroups), outputs pre-filled with NaN behind padded row strides, h == null, in place, and the scaled form."""
    ops = vited.ops
    a, w, bias, res, gamma, beta = _fwd_operands(gpu, M, K)
    prod = a.double() @ w.double().t() + bias.double()
    ref = res.double() + prod
    y, h, mean, rstd = ops.linear_residual_layernorm_fwd(a, w, bias, res, gamma, beta, 1e-6)
    _check_fwd(y, h, mean, rstd, ref, gamma, beta, K)
    # the same call on NaN-filled outputs with padded row strides: every element written, bit for bit the same, every gap intact
    ldy, ldh = N + 8, N + 4
    yp, hp = _nan((M, ldy), gpu), _nan((M, ldh), gpu, torch.bfloat16)
    mp, rp = _nan((M,), gpu), _nan((M,), gpu)
    vited._lib.call('vited_linear_residual_layernorm_fwd', a.data_ptr(), K, w.data_ptr(), K, bias.data_ptr(), res.data_ptr(), N, yp.data_ptr(),
                    ldy, gamma.data_ptr(), beta.data_ptr(), 1e-6, hp.data_ptr(), ldh, mp.data_ptr(), rp.data_ptr(), M, N, K,
                    torch.cuda.current_stream().cuda_stream)
    assert torch.equal(yp[:, :N], y) and torch.equal(hp[:, :N], h) and torch.equal(mp, mean) and torch.equal(rp, rstd)
    assert bool(yp[:, N:].isnan().all()) and bool(hp[:, N:].isnan().all())
    # without a LayerNorm (h == null), into a NaN-filled out, and in place on the residual
    y3, h3, _, _ = ops.linear_residual_layernorm_fwd(a, w, None, res.clone(), None, None, out=_nan((M, N), gpu))
    assert h3 is None
    torch.testing.assert_close(y3.double(), ref - bias.double(), rtol=1e-5, atol=2e-5 * K ** 0.5)
    inplace = res.clone()
    ops.linear_residual_layernorm_fwd(a, w, bias, inplace, gamma, beta, 1e-6, out=inplace)
    assert torch.equal(inplace, y)
    # stochastic depth: dropped (0), kept at rate 0 (1) and kept at rate 0.1 (1 / 0.9) rows, interleaved irregularly
    scale = torch.tensor([0.0, 1.0, 1.0 / 0.9], device=gpu)[(torch.arange(M, device=gpu) * 7 // 3) % 3].contiguous()
    ys, hs, ms, rs = ops.linear_residual_layernorm_fwd(a, w, bias, res, gamma, beta, 1e-6, row_scale=scale)
    _check_fwd(ys, hs, ms, rs, res.double() + scale.double()[:, None] * prod, gamma, beta, K)
    assert torch.equal(ys[scale == 0], res[scale == 0])
    assert torch.equal(ys[scale == 1], y[scale == 1]) and torch.equal(hs[scale == 1], h[scale == 1])


def _bwd_case(gpu, M, K, n=N):
    dy = _rand((M, K), gpu, 11 + M, 1.0, torch.bfloat16)
    wt = _rand((n, K), gpu, 12 + K, K ** -0.5, torch.bfloat16)
    x = _rand((M, n), gpu, 13, 1.5) + 0.3
    gamma = 1.0 + _rand((n,), gpu, 14, 0.2)
    dx_in = _rand((M, n), gpu, 15, 1.0)
    return dy, wt, x, gamma, dx_in


def _bwd_reference(dh, x, gamma):
    n = x.shape[1]
    xd = x.double().requires_grad_(True)
    gd = gamma.double().requires_grad_(True)
    bd = torch.zeros(n, dtype=torch.float64, device=x.device, requires_grad=True)
    F.layer_norm(xd, (n,), gd, bd, 1e-6).backward(dh)
    mu = x.double().mean(dim=1)
    rs = (x.double().var(dim=1, unbiased=False) + 1e-6).rsqrt()
    return xd.grad, gd.grad, bd.grad, mu.float(), rs.float()


def _check_bwd(M, dx, dg, db, want, gg, bg):
    scale = float(want.abs().max())
    torch.testing.assert_close(dx.double(), want, rtol=1e-4, atol=1e-5 * scale)
    torch.testing.assert_close(dg.double(), gg, rtol=1e-4, atol=1e-5 * float(gg.abs().max()) * M ** 0.5)
    torch.testing.assert_close(db.double(), bg, rtol=1e-4, atol=1e-5 * float(bg.abs().max()) * M ** 0.5)
    return scale


@pytest.mark.parametrize('M,K', BWD_SHAPES)
def test_backward(vited, gpu, M, K):
    """dx = dx_in + LN'(dy Wt^T) with the column sums against fp64 autograd through LayerNorm on the same bf16-rounded operands; dx_in
    absent, aliased and accumulated; deferred column sums; the scale on the bf16 copy alone."""
    ops = vited.ops
    dy, wt, x, gamma, dx_in = _bwd_case(gpu, M, K)
    xg, gg, bg, mean, rstd = _bwd_reference(dy.double() @ wt.double().t(), x, gamma)
    dx, dx_lp, dg, db = ops.linear_layernorm_bwd(dy, wt, x, gamma, mean, rstd, dx_in=dx_in, want_lp=True)
    want = xg + dx_in.double()
    scale = _check_bwd(M, dx, dg, db, want, gg, bg)
    assert torch.equal(dx_lp, dx.to(torch.bfloat16))
    # no incoming residual gradient (into a NaN-filled dx), no bf16 copy, accumulate onto existing column sums, dx in place of dx_in
    acc_g, acc_b = torch.full((N,), 2.0, device=gpu), torch.full((N,), -1.0, device=gpu)
    dx2, lp2, _, _ = ops.linear_layernorm_bwd(dy, wt, x, gamma, mean, rstd, dx_out=_nan((M, N), gpu), dgamma=acc_g, dbeta=acc_b)
    assert lp2 is None
    torch.testing.assert_close(dx2.double(), xg, rtol=1e-4, atol=1e-5 * scale)
    torch.testing.assert_close(acc_g - 2.0, dg, rtol=1e-4, atol=1e-4 * float(dg.abs().max()))
    torch.testing.assert_close(acc_b + 1.0, db, rtol=1e-4, atol=1e-4 * float(db.abs().max()))
    buf = dx_in.clone()
    ops.linear_layernorm_bwd(dy, wt, x, gamma, mean, rstd, dx_in=buf, dx_out=buf)
    assert torch.equal(buf, dx)
    # deferred column sums: two LayerNorms finished by ONE launch (overwrite and accumulate), the immediate form's numbers bit for bit
    queue = []
    d1, _, g1, b1 = ops.linear_layernorm_bwd(dy, wt, x, gamma, mean, rstd, dx_in=dx_in, defer=queue)
    acc_g2, acc_b2 = torch.full((N,), 2.0, device=gpu), torch.full((N,), -1.0, device=gpu)
    ops.linear_layernorm_bwd(dy, wt, x, gamma, mean, rstd, dgamma=acc_g2, dbeta=acc_b2, defer=queue)
    assert len(queue) == 2 and torch.equal(d1, dx)
    assert queue[0][1] == vited._lib.load().vited_linear_layernorm_bwd_partial_rows_n(M, N)
    ops.layernorm_bwd_finish(queue)
    assert not queue and torch.equal(g1, dg) and torch.equal(b1, db) and torch.equal(acc_g2, acc_g) and torch.equal(acc_b2, acc_b)
    # the scale of the branch that consumes the copy: on the copy only
    lps = torch.tensor([0.0, 1.0, 1.0 / 0.9], device=gpu)[(torch.arange(M, device=gpu) * 5 // 3) % 3].contiguous()
    dx3, lp3, dg3, db3 = ops.linear_layernorm_bwd(dy, wt, x, gamma, mean, rstd, dx_in=dx_in, lp_scale=lps)
    assert torch.equal(dx3, dx) and torch.equal(dg3, dg) and torch.equal(db3, db)
    assert torch.equal(lp3, (lps[:, None] * dx).to(torch.bfloat16))


def test_backward_segmented(vited, gpu):
    """[3, 1000, 1536] x [768, 4608]: the contraction read from three tensors is the contraction over their concatenation."""
    ops = vited.ops
    L, M, seg_k = 3, 1000, 1536
    dy3 = _rand((L, M, seg_k), gpu, 31, 1.0, torch.bfloat16)
    wt = _rand((N, L * seg_k), gpu, 32, (L * seg_k) ** -0.5, torch.bfloat16)
    x = _rand((M, N), gpu, 33, 1.5) + 0.3
    gamma = 1.0 + _rand((N,), gpu, 34, 0.2)
    cat = torch.cat(list(dy3), dim=1).contiguous()
    xg, gg, bg, mean, rstd = _bwd_reference(cat.double() @ wt.double().t(), x, gamma)
    dx, lp, dg, db = ops.linear_layernorm_bwd(dy3, wt, x, gamma, mean, rstd, want_lp=True)
    _check_bwd(M, dx, dg, db, xg, gg, bg)
    dxc, lpc, dgc, dbc = ops.linear_layernorm_bwd(cat, wt, x, gamma, mean, rstd, want_lp=True)
    assert torch.equal(dx, dxc) and torch.equal(lp, lpc) and torch.equal(dg, dgc) and torch.equal(db, dbc)


@pytest.mark.parametrize('M,K', [(72 * 577, 3072), (24 * 576, 768)])
def test_every_launch_gives_the_same_bits(vited, gpu, M, K):
    """Full-chip shapes, forward and backward, 5 launches each with unrelated memory traffic in between: a stage that lands late or
    is rewritten early shows as a result that differs between launches."""
    ops = vited.ops
    a, w, bias, res, gamma, beta = _fwd_operands(gpu, M, K)
    noise = torch.empty(64 << 20, device=gpu)
    first = None
    for it in range(5):
        noise.fill_(float(it))
        y, h, mean, rstd = ops.linear_residual_layernorm_fwd(a, w, bias, res, gamma, beta, 1e-6)
        dx, dx_lp, dg, db = ops.linear_layernorm_bwd(a, w, res, gamma, mean, rstd, want_lp=True)
        out = (y, h, mean, rstd, dx, dx_lp, dg, db)
        if first is None:
            first = [t.clone() for t in out]
        else:
            for t, f in zip(out, first):
                assert torch.equal(t, f), (M, K, it)


def test_width_384_keeps_its_kernels(vited, gpu):
    """(520, 384): the forward still is the two-kernel form bit for bit, the backward still tiles as the 384 kernels do."""
    ops, lib = vited.ops, vited._lib.load()
    M, K, n = 520, 384, 384
    a, w, bias, res, gamma, beta = _fwd_operands(gpu, M, K, n)
    y, h, mean, rstd = ops.linear_residual_layernorm_fwd(a, w, bias, res, gamma, beta, 1e-6)
    y2 = ops.gemm(a, w, epilogue=vited._lib.EPI_RESIDUAL, bias=bias, residual=res)
    h2, m2, r2 = ops.layernorm_fwd(y2, gamma, beta, 1e-6, torch.bfloat16)
    assert torch.equal(y, y2) and torch.equal(h, h2) and torch.equal(mean, m2) and torch.equal(rstd, r2)
    dy, wt, x, gamma, dx_in = _bwd_case(gpu, M, K, n)
    xg, gg, bg, mean, rstd = _bwd_reference(dy.double() @ wt.double().t(), x, gamma)
    queue = []
    dx, dx_lp, dg, db = ops.linear_layernorm_bwd(dy, wt, x, gamma, mean, rstd, dx_in=dx_in, want_lp=True, defer=queue)
    assert queue[0][1] == lib.vited_linear_layernorm_bwd_partial_rows(M) == lib.vited_linear_layernorm_bwd_partial_rows_n(M, n)
    ops.layernorm_bwd_finish(queue)
    _check_bwd(M, dx, dg, db, xg + dx_in.double(), gg, bg)
    assert torch.equal(dx_lp, dx.to(torch.bfloat16))


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _model_case(vited, gpu):
    """embed_dim 768, 12 heads, 16 / 17 tokens, 1 + 2 blocks, bf16, train(), forced drop-path scales: logits and every gradient
    against the oracle's composition, with the kernels switched on for every product they compute.  Returns how many row-complete launches of each mode carried N == 768."""
    import droppath_cases as dc
    from oracle import vited_oracle as vo
    from test_gpu_droppath import _check_values, _grads, _hip_model
    ops = vited.ops
    s = vo.ViTEDShape(embed_dim=768, num_heads=12, img_size=64, patch_size=16, depth=1, c_depth=2)
    batch = 8
    torch.manual_seed(20)
    oracle = vo.OracleViTED(s)
    model = _hip_model(vited, s, gpu, torch.bfloat16, rate=0.5, state=oracle.state_dict()).train()
    x = torch.randn(batch, 2, 3, s.img_size, s.img_size).clamp(-1, 1)
    y = (torch.rand(batch, s.num_classes) > 0.75).float()
    enc = dc.irregular_scales(0.5, s.depth, 2, batch, salt=3)
    dec = dc.irregular_scales(0.5, s.c_depth, 3, batch, salt=5)
    lo = dc.forward_scaled(oracle, x, enc, dec)
    _, go = dc.loss_and_grads(oracle, lo, y)
    seen = {'fwd': 0, 'bwd': 0}
    real_fwd, real_bwd, real_supported = ops.linear_residual_layernorm_fwd, ops.linear_layernorm_bwd, ops.linear_layernorm_supported

    def everywhere(m, n, k, dtype):
        """The predicate without its speed rule: a model of this size has too few rows for the kernels to pay,
        and this test is about what they compute inside the model."""
        return (dtype == torch.bfloat16 and n == N and k >= 768 and k % 64 == 0) or real_supported(m, n, k, dtype)

    def spy_fwd(a, w, *rest, **k):
        seen['fwd'] += w.shape[0] == N
        return real_fwd(a, w, *rest, **k)

    def spy_bwd(dy, wt, *rest, **k):
        seen['bwd'] += wt.shape[0] == N
        return real_bwd(dy, wt, *rest, **k)

    ops.linear_residual_layernorm_fwd, ops.linear_layernorm_bwd, ops.linear_layernorm_supported = spy_fwd, spy_bwd, everywhere
    try:
        lh = model(x.to(gpu), drop_path=vited.DropPathScales(enc.to(gpu), dec.to(gpu)))
        F.binary_cross_entropy_with_logits(lh, y.to(gpu)).backward()
    finally:
        ops.linear_residual_layernorm_fwd, ops.linear_layernorm_bwd, ops.linear_layernorm_supported = real_fwd, real_bwd, real_supported
    _check_values(torch.bfloat16, lh.detach().cpu(), _grads(model), lo.detach(), go)
    return seen


def test_model_768_with_the_fused_kernels(vited, gpu):
    assert os.environ.get('VITED_FUSED_LN', '1') != '0'
    seen = _model_case(vited, gpu)
    # 1 + 2 blocks: proj + fc2 of the encoder block, proj + cross-proj (+ fc2 of the first) of the decoder blocks in the forward;
    # qkv / q / fc1 / the folded kv in the backward
    assert seen['fwd'] >= 4 and seen['bwd'] >= 4, seen


def test_model_768_without_the_fused_kernels(gpu):
    """VITED_FUSED_LN=0 (read when the runtime is built, hence a fresh process): the two-kernel path, the same bounds."""
    env = dict(os.environ, VITED_FUSED_LN='0')
    flags = ['-s'] if sys.flags.no_user_site else []
    out = subprocess.run([sys.executable, *flags, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    seen = json.loads(out.stdout.strip().splitlines()[-1])
    assert seen == {'fwd': 0, 'bwd': 0}, seen


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import vited_amd
    vited_amd._lib.load()
    counts = _model_case(vited_amd, torch.device('cuda:0'))
    print(json.dumps({k: int(v) for k, v in counts.items()}))
