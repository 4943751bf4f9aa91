"""Every GEMM kernel instance the dispatchers can select, bit for bit.  The operands are small integers and integers / 16
(tests/exact_cases.py), so every product and every partial sum is an fp32 number and the fp32 accumulator is the SAME number in any
summation order, tile shape, split-K plan or MFMA variant.  fp32 outputs must equal the fp64 product, bf16 outputs its one correct
rounding (to nearest even; 72 % of the outputs need rounding and 16 % are exact ties, tests/test_exact_cases.py): torch.equal, no
tolerance.  A truncating or half-away store, a bf16 rounding before the EPI_MUL multiply, a bf16 hand-off between K halves, a
dropped k-column in a ragged tile, a row counted twice or left out of a column sum all pass the randn tests' rtol = atol = 1e-2 and
fail here.  Every case calls the guard of exact_cases on its inputs before it trusts the truth.

Only the GELU-VALUED outputs (u and gelu' of EPI_GELU / EPI_GELU_GRAD, EPI_MUL_GELU_GRAD) are not exact; they are held to the
allowance of tests/test_gpu_structured.py (_gelu_allow) evaluated at the exact pre-activation, on operands scaled so that the
pre-activations spread over about +-4.5.

ops.last_paths() tells the MFMA kernels from the portable ones and nothing more.  Which INSTANCE a shape takes is the dispatchers'
shape rule, restated once below (_nt_instance: dispatch_nt / nt_areg_waves of gemm_mfma.hip and gemm_nt_areg_supported of
gemm_nt_k384.hip; _tn_instance: tn_use_wide / tn_use_ring; the tile height of gemm_row.hip through its host query).  Every case
names the instance it means to run and asserts the rule; a dispatcher that moves a threshold has to move the rule with it.
"""
import pytest
import torch
import torch.nn.functional as F

import exact_cases as ec
import structured_cases as sc
from test_gpu_structured import _gelu_allow

pytestmark = pytest.mark.gpu
PORTABLE, MFMA = 1, 2                   # ops.last_paths()[0]
BF16, F32 = torch.bfloat16, torch.float32
EPILOGUES = ('STORE', 'STORE_F32', 'RESIDUAL', 'GELU', 'GELU_GRAD', 'MUL', 'MUL_GELU_GRAD')
EXACT_EPILOGUES = ('STORE', 'STORE_F32', 'RESIDUAL', 'GELU', 'MUL')     # GELU: its z output


def _nt_instance(epi, M, N, K):
    """The instance vited_gemm gives a bf16 B_NK product that passes gemm_nt_mfma_supported."""
    if K == 384 and N % 128 == 0 and 768 <= N <= 2048 and M >= 8192:                 # gemm_nt_areg_supported
        if epi == 'MUL':
            return 'areg<MUL, 8>'
        if epi == 'STORE' and N >= 1152 and M >= 65536:
            return 'areg<STORE, 4>'
    shallow = K <= 512 and N >= 768
    tall = epi in ('STORE', 'MUL', 'GELU_GRAD') and shallow and M >= 8192
    if shallow and tall and epi == 'STORE':
        return 'tile<32, 4, 3>'
    return f'tile<{32 if shallow else 64}, {4 if tall else 2}>'


def _tn_instance(dtype, M, N, K):
    """The instance vited_linear_bwd_weight gives dW = dy^T x (16-byte aligned operands, row strides multiples of 8)."""
    if dtype != BF16 or N % 8 or K % 8:
        return 'portable'
    if K % 384 == 0 and M >= 4096:
        return 'wide'
    if N * K >= 1536 * 384 and M >= 16384:
        return 'tn<32, 3>'
    return 'tn<64, 2>'


def _seed(*parts):
    return sum((i + 1) * 7919 * (sum(map(ord, p)) if isinstance(p, str) else int(p)) for i, p in enumerate(parts)) % (2 ** 31)


def _same(name, got, want):
    """torch.equal with the mismatch pattern in the message: how many, where, by how much."""
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = (got != want) | torch.isnan(got)
    idx = bad.nonzero()
    diff = (got.double() - want.double()).abs()[bad]
    lo, hi = idx.min(0).values.tolist(), idx.max(0).values.tolist()
    raise AssertionError(f'{name}: {int(bad.sum())} of {bad.numel()} elements differ, indices from {lo} to {hi}, first {idx[0].tolist()} '
                         f'got {float(got[tuple(idx[0])])!r} want {float(want[tuple(idx[0])])!r}, max |diff| {float(diff.max()):.6g}')


def _gelu_valued(name, got, ref, z, acc=None):
    """bf16 GELU-valued output against fp64 at the exact z within _gelu_allow; with ``acc`` (EPI_MUL_GELU_GRAD: out = acc gelu'(z),
    ref = acc gelu'(z) in fp64) the cdf-error term of the allowance is multiplied by |acc|."""
    assert bool(torch.isfinite(got).all()), name
    allow = _gelu_allow(ref, z, BF16)
    if acc is not None:
        allow = allow + (acc.abs() - 1.0) * _gelu_allow(torch.zeros_like(ref), z, BF16)
    err = (got.double() - ref).abs()
    ratio = float((err / allow.clamp_min(1e-300)).max())
    print(f'\nexact-parity gelu {name} err/allowance={ratio:.3f}')
    assert bool((err <= allow).all()), (name, ratio)


def _nt_case(gpu, M, N, K, scale, dtype=BF16, residual=True):
    """Operands on the device: fp32 exact values c[...] and the kernel's own dtypes d[...]."""
    c = {k: t.to(gpu) for k, t in ec.nt_operands(M, N, K, _seed('nt', M, N, K, scale), scale, residual).items()}
    d = dict(a=c['a'].to(dtype), w=c['w'].to(dtype), bias=c['bias'])
    return c, d


def _run_epilogue(ops, L, gpu, epi, M, N, K, path, dtype=BF16, b_layout=None):
    """One epilogue of vited_gemm at (M, N, K) on exact operands; the exact outputs with torch.equal."""
    kn = b_layout is not None and b_layout == L.B_KN

    def gemm(d, **kw):
        out = ops.gemm(d['a'], d['w'].t().contiguous() if kn else d['w'], b_layout=L.B_KN if kn else L.B_NK, **kw)
        assert ops.last_paths()[0] == path
        return out

    if epi in ('STORE', 'STORE_F32', 'RESIDUAL', 'GELU', 'MUL'):
        c, d = _nt_case(gpu, M, N, K, 'wide', dtype, residual=epi == 'RESIDUAL')
        aux = ec.mul_aux(M, N, _seed('aux', M, N)).to(gpu) if epi == 'MUL' else None
        ec.guard_nt(c['a'], c['w'], c['bias'], c.get('residual'), aux)
        z, acc = ec.nt_truth(c['a'], c['w'], c['bias']), ec.nt_truth(c['a'], c['w'])
        if epi == 'STORE':
            _same('STORE + bias', gemm(d, bias=d['bias']), ec.as_dtype(z, dtype))
            _same('STORE', gemm(d), ec.as_dtype(acc, dtype))
        elif epi == 'STORE_F32':
            _same('STORE_F32 + bias', gemm(d, epilogue=L.EPI_STORE_F32, bias=d['bias']), ec.as_f32(z))
            _same('STORE_F32', gemm(d, epilogue=L.EPI_STORE_F32), ec.as_f32(acc))
        elif epi == 'RESIDUAL':
            y = gemm(d, epilogue=L.EPI_RESIDUAL, bias=d['bias'], residual=c['residual'])
            _same('RESIDUAL', y, ec.as_f32(z + c['residual'].double()))
        elif epi == 'GELU':
            zo, _ = gemm(d, epilogue=L.EPI_GELU, bias=d['bias'])
            _same('GELU z', zo, ec.as_dtype(z, dtype))
        else:
            _same('MUL + bias', gemm(d, epilogue=L.EPI_MUL, bias=d['bias'], aux=aux.to(dtype)), ec.mul_truth(z, aux, dtype))
    if epi in ('GELU', 'GELU_GRAD', 'MUL_GELU_GRAD') and dtype == BF16 and path == MFMA:
        c, d = _nt_case(gpu, M, N, K, 'gelu', residual=False)
        ec.guard_nt(c['a'], c['w'], c['bias'])
        z = ec.nt_truth(c['a'], c['w'], c['bias'])
        u_ref, g_ref = sc.gelu_ref(z)
        if epi == 'GELU':
            zo, u = gemm(d, epilogue=L.EPI_GELU, bias=d['bias'])
            _same('GELU z (gelu scale)', zo, ec.as_bf16(z))
            _gelu_valued('EPI_GELU u', u, u_ref, z)
        elif epi == 'GELU_GRAD':
            gd, u = gemm(d, epilogue=L.EPI_GELU_GRAD, bias=d['bias'])
            _gelu_valued('EPI_GELU_GRAD gd', gd, g_ref, z)
            _gelu_valued('EPI_GELU_GRAD u', u, u_ref, z)
        else:
            # the saved pre-activation: the exact z of another draw, in bf16 as fc1 stores it
            other = ec.nt_operands(M, N, K, _seed('saved', M, N, K), 'gelu', residual=False)
            saved = ec.as_bf16(ec.nt_truth(other['a'].to(gpu), other['w'].to(gpu), other['bias'].to(gpu)))
            dz = gemm(d, epilogue=L.EPI_MUL_GELU_GRAD, bias=d['bias'], aux=saved)
            _gelu_valued('EPI_MUL_GELU_GRAD dz', dz, z * sc.gelu_ref(saved.float())[1], saved.float(), acc=z)


# ---------------------------------------------------------------------------------------------
# vited_gemm, bf16, B_NK: the NT tile kernel and gemm_nt_k384.hip
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('epi', EPILOGUES)
@pytest.mark.parametrize('M,N,K,instance', [(130, 384, 384, 'tile<64, 2>'), (70, 1152, 1536, 'tile<64, 2>'), (257, 768, 384, 'tile<32, 2>')])
def test_nt_tile_kernel_every_epilogue(vited, gpu, M, N, K, instance, epi):
    """gemm_nt_mfma_kernel<EPI, 64, 2> (N < 768, and K > 512) and <EPI, 32, 2> (K <= 512, N >= 768), ragged row counts."""
    assert _nt_instance(epi, M, N, K) == instance
    _run_epilogue(vited.ops, vited._lib, gpu, epi, M, N, K, MFMA)


@pytest.mark.parametrize('epi,M,N,K,instance', [
    ('STORE', 8269, 768, 384, 'tile<32, 4, 3>'),           # the three-stage ring of the plain store, with and without bias
    ('MUL', 8269, 768, 128, 'tile<32, 4>'),
    ('GELU_GRAD', 8269, 768, 384, 'tile<32, 4>'),
    ('MUL', 8269, 768, 384, 'areg<MUL, 8>'),
    ('STORE', 65613, 1152, 384, 'areg<STORE, 4>'),          # with and without bias; the truth is built in row slices
])
def test_nt_instances_of_large_launches(vited, gpu, epi, M, N, K, instance):
    """The 256-row tiles and the A-in-registers kernels, which only launches of >= 8,192 / 65,536 rows select; 8,269 = 32 * 256 + 77
    and 65,613 = 65,536 + 77 end in a ragged tile."""
    assert _nt_instance(epi, M, N, K) == instance
    _run_epilogue(vited.ops, vited._lib, gpu, epi, M, N, K, MFMA)


def test_nt_row_strides_and_column_view_output(vited, gpu):
    """lda > K and out= a column view of a wider buffer (ldo > N): the same exact outputs, nothing written beside them."""
    ops, L = vited.ops, vited._lib
    M, N, K = 257, 768, 384
    assert _nt_instance('STORE', M, N, K) == 'tile<32, 2>'
    c, d = _nt_case(gpu, M, N, K, 'wide', residual=False)
    ec.guard_nt(c['a'], c['w'], c['bias'])
    z = ec.nt_truth(c['a'], c['w'], c['bias'])
    a_wide = torch.full((M, K + 64), 3.0, device=gpu, dtype=BF16)
    a_wide[:, 32:32 + K] = d['a']
    a_view = a_wide[:, 32:32 + K]
    for dtype, epi, want in ((BF16, L.EPI_STORE, ec.as_bf16(z)), (F32, L.EPI_STORE_F32, ec.as_f32(z))):
        buf = torch.full((M, N + 128), 7.0, device=gpu, dtype=dtype)
        out = ops.gemm(a_view, d['w'], epilogue=epi, bias=d['bias'], out=buf[:, 64:64 + N])
        assert ops.last_paths()[0] == MFMA and out.data_ptr() == buf[:, 64:].data_ptr()
        _same(f'strided {dtype}', buf[:, 64:64 + N], want)
        assert bool((buf[:, :64] == 7.0).all()) and bool((buf[:, 64 + N:] == 7.0).all())


@pytest.mark.parametrize('dtype,path', [(BF16, MFMA), (F32, PORTABLE)])
def test_residual_row_remap_with_a_broadcast_table(vited, gpu, dtype, path):
    """EPI_RESIDUAL with the cls-row remap and the broadcast pos_embed table (the patch embedding), exact."""
    ops, L = vited.ops, vited._lib
    B, N1, D, K = 6, 64, 384, 192
    c, d = _nt_case(gpu, B * N1, D, K, 'wide', dtype, residual=False)
    pos = ec.ints((N1 + 1, D), 512, torch.Generator().manual_seed(5), ec.UNIT).to(gpu)
    ec.guard_nt(c['a'], c['w'], c['bias'], pos[1:].repeat(B, 1))
    tok = ec.nt_truth(c['a'], c['w'], c['bias']).view(B, N1, D)
    x = torch.full((B * (N1 + 1), D), float('nan'), device=gpu)
    ops.gemm(d['a'], d['w'], epilogue=L.EPI_RESIDUAL, bias=d['bias'], residual=pos, rows_per_batch=N1, out_rows_per_batch=N1 + 1,
             row_offset=1, residual_bcast=True, out=x)
    assert ops.last_paths()[0] == path
    _same('remap, offset 1', x.view(B, N1 + 1, D)[:, 1:].contiguous(), ec.as_f32(tok + pos[1:].double()))
    assert bool(torch.isnan(x.view(B, N1 + 1, D)[:, 0]).all())                   # the cls rows are not this launch's to write
    x1 = ops.gemm(d['a'], d['w'], epilogue=L.EPI_RESIDUAL, bias=d['bias'], residual=pos[1:], rows_per_batch=N1, out_rows_per_batch=N1,
                  row_offset=0, residual_bcast=True, out_rows=B * N1)
    _same('remap, offset 0', x1.view(B, N1, D), ec.as_f32(tok + pos[1:].double()))


# ---------------------------------------------------------------------------------------------
# vited_gemm, portable kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('epi', EXACT_EPILOGUES)
@pytest.mark.parametrize('dtype,M,N,K,kn', [(F32, 70, 32, 32, False), (F32, 33, 4, 384, False), (BF16, 33, 4, 384, False), (BF16, 70, 32, 32, False),
                                            (BF16, 130, 384, 384, True)])
def test_portable_gemm_exact_epilogues(vited, gpu, dtype, M, N, K, kn, epi):
    """gemm_portable.hip: fp32 operands, and the bf16 shapes the MFMA kernel refuses (N % 16, K % 64, B given as [K, N])."""
    L = vited._lib
    _run_epilogue(vited.ops, L, gpu, epi, M, N, K, PORTABLE, dtype, L.B_KN if kn else L.B_NK)


# ---------------------------------------------------------------------------------------------
# gemm_row.hip: vited_linear_residual_layernorm_fwd / vited_linear_layernorm_bwd
# ---------------------------------------------------------------------------------------------
ROW_N = 384
ROW_TILES = {100: (96, 2), 24601: (128, 193), 32801: (144, 228), 36901: (160, 231)}       # M -> (rows per tile, tiles)


def _row_tiles(vited, M):
    """Asserts the tile height gemm_row.hip picks for M rows through its host query; -> the number of tiles."""
    height, tiles = ROW_TILES[M]
    assert int(vited._lib.load().vited_linear_layernorm_bwd_partial_rows(M)) == tiles == -(-M // height)
    return tiles


def _affine(gpu, seed):
    gen = torch.Generator().manual_seed(seed)
    return (1 + 0.2 * torch.randn(ROW_N, generator=gen)).to(gpu), (0.1 * torch.randn(ROW_N, generator=gen)).to(gpu)


@pytest.mark.parametrize('M,K', [(100, 384), (24601, 384), (32801, 384), (36901, 384), (100, 64), (100, 1536)])
def test_linear_residual_layernorm_fwd_exact(vited, gpu, M, K):
    """y = residual + a w^T + bias with operands on ALL K columns, every tile height, ragged last tiles: bit-equal to the truth,
    also without a LayerNorm and in place on the residual; h, mean, rstd bit-equal to ops.layernorm_fwd of that y."""
    ops = vited.ops
    _row_tiles(vited, M)
    c, d = _nt_case(gpu, M, ROW_N, K, 'wide')
    ec.guard_nt(c['a'], c['w'], c['bias'], c['residual'])
    want = ec.as_f32(ec.nt_truth(c['a'], c['w'], c['bias'], c['residual']))
    gamma, beta = _affine(gpu, 3)
    assert ops.linear_layernorm_supported(M, ROW_N, K, BF16)
    y, h, mean, rstd = ops.linear_residual_layernorm_fwd(d['a'], d['w'], d['bias'], c['residual'], gamma, beta, 1e-6)
    _same('y', y, want)
    h2, m2, r2 = ops.layernorm_fwd(y, gamma, beta, 1e-6, BF16)
    _same('h', h, h2)
    _same('mean', mean, m2)
    _same('rstd', rstd, r2)
    y3, h3, _, _ = ops.linear_residual_layernorm_fwd(d['a'], d['w'], None, c['residual'].clone(), None, None)
    assert h3 is None
    _same('y without LayerNorm and bias', y3, ec.as_f32(ec.nt_truth(c['a'], c['w'], None, c['residual'])))
    inplace = c['residual'].clone()
    ops.linear_residual_layernorm_fwd(d['a'], d['w'], d['bias'], inplace, gamma, beta, 1e-6, out=inplace)
    _same('y in place', inplace, want)


def _ln_bwd_case(gpu, M, K, seed):
    dy, wt = (t.to(gpu) for t in ec.ln_bwd_operands(M, ROW_N, K, seed))
    ec.guard_nt(dy, wt)
    dh = ec.nt_truth(dy, wt)
    gen = torch.Generator().manual_seed(seed + 1)
    x = (1.5 * torch.randn(M, ROW_N, generator=gen) + 0.3).to(gpu)
    gamma, _ = _affine(gpu, seed + 2)
    mean = x.double().mean(1).float()
    rstd = (x.double().var(1, unbiased=False) + 1e-6).rsqrt().float()
    db0 = ec.ints((ROW_N,), 64, gen).to(gpu)
    return dy, wt, dh, x, gamma, mean, rstd, db0


@pytest.mark.parametrize('M', [100, 24601, 32801, 36901])
def test_linear_layernorm_bwd_dbeta_exact(vited, gpu, M):
    """dbeta = column sums of dh = dy wt^T over all rows, tiles and partials, bit-equal to the fp64 column sum: immediate,
    accumulated onto integer-valued content, deferred through layernorm_bwd_finish.  dx and dgamma keep the tolerances of
    test_linear_layernorm_bwd (they depend on x, mean, rstd, which are not exact)."""
    ops = vited.ops
    K = 384
    _row_tiles(vited, M)
    dy, wt, dh, x, gamma, mean, rstd, db0 = _ln_bwd_case(gpu, M, K, _seed('lnbwd', M))
    ec.guard_colsum(dh, db0)
    db_want, db_acc_want = ec.as_f32(dh.sum(0)), ec.as_f32(dh.sum(0) + db0.double())
    dyb, wtb = dy.to(BF16), wt.to(BF16)
    dx, _, dg, db = ops.linear_layernorm_bwd(dyb, wtb, x, gamma, mean, rstd)
    _same('dbeta', db, db_want)
    xd, gd = x.double().requires_grad_(), gamma.double().requires_grad_()
    F.layer_norm(xd, (ROW_N,), gd, torch.zeros_like(gd), 1e-6).backward(dh)
    torch.testing.assert_close(dx.double(), xd.grad, rtol=1e-4, atol=1e-5 * float(xd.grad.abs().max()))
    torch.testing.assert_close(dg.double(), gd.grad, rtol=1e-4, atol=1e-5 * float(gd.grad.abs().max()) * M ** 0.5)
    acc_g, acc_b = torch.full((ROW_N,), 2.0, device=gpu), db0.clone()
    ops.linear_layernorm_bwd(dyb, wtb, x, gamma, mean, rstd, dgamma=acc_g, dbeta=acc_b)
    _same('dbeta accumulated', acc_b, db_acc_want)
    queue = []
    acc_g2, acc_b2 = torch.full((ROW_N,), 2.0, device=gpu), db0.clone()
    _, _, g1, b1 = ops.linear_layernorm_bwd(dyb, wtb, x, gamma, mean, rstd, defer=queue)
    ops.linear_layernorm_bwd(dyb, wtb, x, gamma, mean, rstd, dgamma=acc_g2, dbeta=acc_b2, defer=queue)
    assert len(queue) == 2
    ops.layernorm_bwd_finish(queue)
    _same('dbeta deferred', b1, db_want)
    _same('dbeta deferred and accumulated', acc_b2, db_acc_want)
    _same('dgamma deferred', g1, dg)
    _same('dgamma deferred and accumulated', acc_g2, acc_g)


def test_linear_layernorm_bwd_segmented_dbeta_exact(vited, gpu):
    """The segmented form: dkv [3, M, 768] (one tensor per decoder block) against a [384, 2304] weight."""
    ops = vited.ops
    M, L, seg = 1000, 3, 768
    dy, wt, dh, x, gamma, mean, rstd, db0 = _ln_bwd_case(gpu, M, L * seg, _seed('segmented'))
    ec.guard_colsum(dh, db0)
    dkv = dy.view(M, L, seg).transpose(0, 1).contiguous().to(BF16)                # segment j = k-columns [j seg, (j + 1) seg)
    _, _, _, db = ops.linear_layernorm_bwd(dkv, wt.to(BF16), x, gamma, mean, rstd)
    _same('dbeta segmented', db, ec.as_f32(dh.sum(0)))
    acc_g, acc_b = torch.zeros(ROW_N, device=gpu), db0.clone()
    ops.linear_layernorm_bwd(dkv, wt.to(BF16), x, gamma, mean, rstd, dgamma=acc_g, dbeta=acc_b)
    _same('dbeta segmented and accumulated', acc_b, ec.as_f32(dh.sum(0) + db0.double()))
    _, _, _, db1 = ops.linear_layernorm_bwd(dy.to(BF16), wt.to(BF16), x, gamma, mean, rstd)
    _same('dbeta of the one-tensor form', db1, db)


# ---------------------------------------------------------------------------------------------
# vited_linear_bwd_weight / vited_linear_bwd_weight_batched
# ---------------------------------------------------------------------------------------------
def _wgrad_case(gpu, M, N, K, seed, views=False):
    """dy, x on the device (fp32 exact values), integer-valued dW / dbias content to accumulate onto, the truths of both modes."""
    dy, x = (t.to(gpu) for t in ec.wgrad_operands(M, N, K, seed))
    gen = torch.Generator().manual_seed(seed + 1)
    dw0, db0 = ec.ints((N, K), 64, gen).to(gpu), ec.ints((N,), 64, gen).to(gpu)
    ec.guard_wgrad(dy, x, dw0, db0)
    dw, db = ec.wgrad_truth(dy, x)
    dw1, db1 = ec.wgrad_truth(dy, x, dw0, db0)
    return dy, x, dw0, db0, tuple(ec.as_f32(t) for t in (dw, db, dw1, db1))


def _column_view(t, left, right, dtype):
    """t as a column view of a wider buffer (row stride > width)."""
    buf = torch.full((t.shape[0], left + t.shape[1] + right), 5.0, device=t.device, dtype=dtype)
    buf[:, left:left + t.shape[1]] = t.to(dtype)
    return buf[:, left:left + t.shape[1]]


@pytest.mark.parametrize('dtype,M,N,K,instance,views', [
    (BF16, 1000, 200, 768, 'tn<64, 2>', False),
    (BF16, 4099, 136, 512, 'tn<64, 2>', False),
    (BF16, 4099, 136, 512, 'tn<64, 2>', True),
    (BF16, 16421, 1152, 512, 'tn<32, 3>', False),          # the three-stage ring: fc1 / fc2 of a width-512 model at batch >= 253
    (BF16, 4099, 136, 384, 'wide', False),
    (BF16, 4099, 136, 384, 'wide', True),
    (BF16, 4128, 384, 1536, 'wide', False),
    (F32, 777, 384, 192, 'portable', False),
    (BF16, 777, 4, 384, 'portable', False),
])
def test_linear_bwd_weight_exact(vited, gpu, dtype, M, N, K, instance, views):
    """dW = dy^T x and dbias = column sums of dy, every geometry of the weight-gradient kernels, ragged last row stages and
    ragged n / k tiles: bit-equal overwritten and accumulated onto integer-valued content; ``views``: the operands are column
    views of wider buffers."""
    ops = vited.ops
    assert _tn_instance(dtype, M, N, K) == instance
    dy, x, dw0, db0, (dw, db, dw1, db1) = _wgrad_case(gpu, M, N, K, _seed('wgrad', M, N, K))
    dyk, xk = (_column_view(dy, 64, 8, dtype), _column_view(x, 32, 24, dtype)) if views else (dy.to(dtype), x.to(dtype))
    path = PORTABLE if instance == 'portable' else MFMA
    got_w, got_b = ops.linear_bwd_weight(dyk, xk)
    assert ops.last_paths()[0] == path
    _same('dW', got_w, dw)
    _same('dbias', got_b, db)
    acc_w, acc_b = dw0.clone(), db0.clone()
    ops.linear_bwd_weight(dyk, xk, dw_out=acc_w, db_out=acc_b)
    assert ops.last_paths()[0] == path
    _same('dW accumulated', acc_w, dw1)
    _same('dbias accumulated', acc_b, db1)


@pytest.mark.parametrize('accumulate', [False, True])
def test_linear_bwd_weight_batched_exact(vited, gpu, accumulate):
    """Three products in one launch of the wide kernel: different row counts (two ragged), a ragged n-tile, four k-panels, one
    product without a bias, one with a strided dy."""
    ops = vited.ops
    items, wants = [], []
    for i, (M, N, K) in enumerate([(4160, 1152, 384), (4099, 384, 1536), (5200, 136, 384)]):
        assert _tn_instance(BF16, M, N, K) == 'wide'
        dy, x, dw0, db0, (dw, db, dw1, db1) = _wgrad_case(gpu, M, N, K, _seed('batched', i))
        dyk = _column_view(dy, 64, 8, BF16) if i == 2 else dy.to(BF16)
        has_bias = i != 1
        out_w = dw0.clone() if accumulate else torch.full_like(dw0, float('nan'))
        out_b = (db0.clone() if accumulate else torch.full_like(db0, float('nan'))) if has_bias else None
        items.append((dyk, x.to(BF16), out_w, out_b))
        wants.append((dw1, db1) if accumulate else (dw, db))
    assert ops.linear_bwd_weight_batched(items, accumulate)
    assert ops.last_paths()[0] == MFMA
    for i, ((_, _, got_w, got_b), (want_w, want_b)) in enumerate(zip(items, wants)):
        _same(f'dW of product {i}', got_w, want_w)
        if got_b is not None:
            _same(f'dbias of product {i}', got_b, want_b)


# ---------------------------------------------------------------------------------------------
# riding along: exact column sums elsewhere
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('rows,width', [(4097, 384), (33, 24960)])
def test_sum_rows_exact(vited, gpu, dtype, rows, width):
    ops = vited.ops
    t = ec.ints((rows, width), 8, torch.Generator().manual_seed(rows)).to(gpu)
    ec.guard_colsum(t)
    want = ec.as_f32(t.double().sum(0))
    _same('sum_rows', ops.sum_rows(t.to(dtype)), want)
    _same('sum_rows of a column view', ops.sum_rows(_column_view(t, 8, 24, dtype)), want)


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_layernorm_bwd_dbeta_exact(vited, gpu, dtype):
    """ops.layernorm_bwd (layernorm.hip): dbeta = column sums of dy on dy = integers / 16, overwritten and accumulated."""
    ops = vited.ops
    rows = 657
    gen = torch.Generator().manual_seed(77)
    dy = ec.ints((rows, ROW_N), 64, gen, ec.UNIT).to(gpu)
    db0 = ec.ints((ROW_N,), 64, gen).to(gpu)
    assert torch.equal(ec.bf(dy), dy)
    ec.guard_colsum(dy, db0)
    x = torch.randn(rows, ROW_N, generator=gen).to(gpu)
    gamma, _ = _affine(gpu, 78)
    mean = x.double().mean(1).float()
    rstd = (x.double().var(1, unbiased=False) + 1e-6).rsqrt().float()
    _, _, _, db = ops.layernorm_bwd(dy.to(dtype), x, gamma, mean, rstd)
    _same('dbeta', db, ec.as_f32(dy.double().sum(0)))
    acc_g, acc_b = torch.zeros(ROW_N, device=gpu), db0.clone()
    ops.layernorm_bwd(dy.to(dtype), x, gamma, mean, rstd, dgamma=acc_g, dbeta=acc_b)
    _same('dbeta accumulated', acc_b, ec.as_f32(dy.double().sum(0) + db0.double()))
