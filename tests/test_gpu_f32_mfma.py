"""The matrix-core fp32 GEMMs (gemm_f32_mfma.hip) against the vector-ALU kernels they stand in for (gemm_portable.hip), bit for bit.

v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain, the portable kernels accumulate that chain, and both feed the same epilogue: the
outputs have to be the same BITS, so every comparison here is ``torch.equal`` on the integer view (NaN patterns and the sign of
zero count) and there is no tolerance anywhere.  ``ops.fp32_gemm_kernels('valu')`` runs the unchanged portable kernels, 'auto'
the dispatch a user gets.  Shapes sit on the edges of the 128 x 128 x 16 tile and of its 32 x 32 accumulators."""
import gc

import pytest
import torch

import droppath_cases as dc
from oracle import vited_oracle as vo

pytestmark = pytest.mark.gpu

# the tile edges; grids of up to 576 tiles of 128 x 128 run the 64-wide tile, so the last shape (26 x 25 tiles) is what runs the 128-wide one
SHAPES = [(64, 32, 1), (65, 33, 2), (97, 70, 3), (129, 130, 17), (130, 384, 33), (257, 96, 384), (3201, 3100, 17)]
# bf16 reaches GEMM path 1 where the bf16 MFMA kernels do not tile: K no multiple of 64
CASES = [(torch.float32, s) for s in SHAPES] + [(torch.bfloat16, s) for s in SHAPES if s[2] % 64]
# the middle two have several splits over M (64-wide tile); the last is one split of 25 x 25 tiles, a grid that takes the 128-wide tile
TN_SHAPES = [(64, 32, 32), (777, 70, 33), (1030, 384, 96), (70, 3100, 3080)]
BCE = torch.nn.functional.binary_cross_entropy_with_logits
EPI_SCALED = 'scaled'                                               # vited_gemm_scaled: EPI_RESIDUAL with a live row scale


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _within_chain_error(got, want, magnitude, terms):
    """|got - want| within the bound of an fp32 chain of ``terms`` roundings: terms * 2^-24 * sum |a b| (+ the subnormal spacing)."""
    return bool(((got.double() - want).abs() <= terms * 2.0 ** -24 * magnitude + 2.0 ** -149).all())


def _both(ops, fn, want_auto=2):
    """fn() under 'valu' and under 'auto': the two results, after checking which kernel each reported."""
    with ops.fp32_gemm_kernels('valu'):
        ref = fn()
        assert ops.last_fp32_gemm_kernel() == 1 and ops.last_paths()[0] == 1
    with ops.fp32_gemm_kernels('auto'):
        got = fn()
        assert ops.last_fp32_gemm_kernel() == want_auto and ops.last_paths()[0] == 1
    return ref, got


def _operands(gpu, dtype, m, n, k, layout_kn, seed=0):
    g = torch.Generator().manual_seed(seed * 1000003 + m * 131 + n * 17 + k)
    a = torch.randn(m, k, generator=g)
    b = torch.randn(n, k, generator=g)                              # logical [n, k]; stored [k, n] under B_KN
    extra = dict(bias=torch.randn(n, generator=g), aux=torch.randn(m, n, generator=g), residual=torch.randn(m, n, generator=g),
                 row_scale=torch.where(torch.rand(m, generator=g) < 0.4, torch.zeros(m), torch.full((m,), 1 / 0.7)))
    b = torch.empty(k, n).copy_(b.t()) if layout_kn else b          # row stride n at k == 1 too
    return a.to(gpu, dtype), b.to(gpu, dtype), {key: v.to(gpu, dtype if key == 'aux' else torch.float32) for key, v in extra.items()}


def _call(ops, epi, a, b, layout, x):
    if epi == EPI_SCALED:
        return ops.gemm(a, b, b_layout=layout, epilogue=ops.EPI_RESIDUAL, bias=x['bias'], residual=x['residual'], row_scale=x['row_scale'])
    if epi == ops.EPI_RESIDUAL:
        return ops.gemm(a, b, b_layout=layout, epilogue=epi, bias=x['bias'], residual=x['residual'])
    if epi == ops.EPI_MUL_GELU_GRAD:
        return ops.gemm(a, b, b_layout=layout, epilogue=epi, aux=x['aux'])
    if epi == ops.EPI_MUL:
        return ops.gemm(a, b, b_layout=layout, epilogue=epi, bias=x['bias'], aux=x['aux'])
    return ops.gemm(a, b, b_layout=layout, epilogue=epi, bias=x['bias'])


def _epilogues(ops):
    return [ops.EPI_STORE, ops.EPI_GELU, ops.EPI_RESIDUAL, ops.EPI_MUL_GELU_GRAD, ops.EPI_STORE_F32, ops.EPI_MUL, ops.EPI_GELU_GRAD, EPI_SCALED]


@pytest.mark.parametrize('layout_kn', [False, True], ids=['B_NK', 'B_KN'])
@pytest.mark.parametrize('dtype,shape', CASES, ids=[f'{str(d)[6:]}-{"x".join(map(str, s))}' for d, s in CASES])
def test_every_epilogue_gives_the_vector_alu_kernels_bits(vited, gpu, dtype, shape, layout_kn):
    ops = vited.ops
    m, n, k = shape
    layout = ops.B_KN if layout_kn else ops.B_NK
    a, b, x = _operands(gpu, dtype, m, n, k, layout_kn)
    assert ops.fp32_gemm_supported(m, n, k, b_layout=layout)
    for epi in _epilogues(ops):
        ref, got = _both(ops, lambda: _call(ops, epi, a, b, layout, x))
        assert _same(ref, got), f'epilogue {epi}: the two kernels differ'
    # not vacuous: the result is the product (fp64 reference of the stored operands)
    out = ops.gemm(a, b, b_layout=layout, epilogue=ops.EPI_STORE_F32)
    bt = b.double() if layout_kn else b.double().t()
    assert _within_chain_error(out, a.double() @ bt, a.double().abs() @ bt.abs(), k)


def test_strided_operands_and_a_column_view_output(vited, gpu):
    """lda > K from a misaligned column view (the element-wise staging path), ldo > N, out / residual column views of wider buffers."""
    ops = vited.ops
    m, n, k = 130, 70, 33
    g = torch.Generator().manual_seed(5)
    a = torch.randn(m, k + 7, generator=g).to(gpu)[:, 1:1 + k]
    b = torch.randn(n, k + 4, generator=g).to(gpu)[:, :k]           # aligned rows of 37 floats: ldb % 4 != 0
    bias = torch.randn(n, generator=g).to(gpu)
    res = torch.randn(m, n + 9, generator=g).to(gpu)[:, 3:3 + n]
    outs = []

    def run(epi):
        buf = torch.full((m, n + 9), -7.0, device=gpu)
        ops.gemm(a, b, epilogue=epi, bias=bias, residual=res if epi == ops.EPI_RESIDUAL else None, out=buf[:, 3:3 + n])
        outs.append(buf)
        return buf

    for epi in (ops.EPI_STORE, ops.EPI_RESIDUAL):
        ref, got = _both(ops, lambda: run(epi))
        assert _same(ref, got)
        assert bool((got[:, :3] == -7).all()) and bool((got[:, 3 + n:] == -7).all())       # nothing beside the view was written
    want = a.double() @ b.double().t() + bias.double()
    assert _within_chain_error(outs[1][:, 3:3 + n], want, a.double().abs() @ b.double().abs().t() + bias.double().abs(), k + 1)


def test_cls_row_remap_with_a_broadcast_residual(vited, gpu):
    ops = vited.ops
    m, n, k = 128, 70, 17                                            # 32 images of 4 patch rows, written behind a cls row each
    a, b, x = _operands(gpu, torch.float32, m, n, k, False, seed=2)
    pos = torch.randn(5, n, generator=torch.Generator().manual_seed(3)).to(gpu)

    def run():
        out = torch.full((160, n), 3.0, device=gpu)
        return ops.gemm(a, b, epilogue=ops.EPI_RESIDUAL, bias=x['bias'], residual=pos, out=out, rows_per_batch=4, out_rows_per_batch=5,
                        row_offset=1, residual_bcast=True)

    ref, got = _both(ops, run)
    assert _same(ref, got)
    assert bool((got.view(32, 5, n)[:, 0] == 3).all())               # the cls rows are not this GEMM's
    want = (a.double() @ b.double().t() + x['bias'].double()).view(32, 4, n) + pos[1:].double()
    mag = (a.double().abs() @ b.double().abs().t() + x['bias'].double().abs()).view(32, 4, n) + pos[1:].double().abs()
    assert _within_chain_error(got.view(32, 5, n)[:, 1:], want, mag, k + 2)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
def test_row_scale_of_zeros_and_inverse_keep(vited, gpu, dtype):
    ops = vited.ops
    m, n, k = 130, 96, 33
    a, b, x = _operands(gpu, dtype, m, n, k, False, seed=4)
    assert bool((x['row_scale'] == 0).any()) and bool((x['row_scale'] > 1).any())
    ref, got = _both(ops, lambda: _call(ops, EPI_SCALED, a, b, ops.B_NK, x))
    assert _same(ref, got)
    dropped = x['row_scale'] == 0
    assert _same(got[dropped], x['residual'][dropped])               # a dropped row is its residual, exactly


@pytest.mark.parametrize('layout_kn', [False, True], ids=['B_NK', 'B_KN'])
def test_planted_values(vited, gpu, layout_kn):
    """Subnormal operands, infinities, a NaN and products that cancel exactly: where the chain of an MFMA could differ from fmaf."""
    ops = vited.ops
    m, n, k = 129, 130, 17
    layout = ops.B_KN if layout_kn else ops.B_NK
    g = torch.Generator().manual_seed(11)
    a, b = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g)
    a[5] = 1e-40                                                     # a row of subnormals
    a[6] = -1e-40
    a[7, 3], a[9, 2] = float('inf'), float('-inf')
    a[10, 1], a[10, 16] = float('inf'), float('-inf')                # +inf and -inf in one chain: NaN unless the signs of b agree
    b[11, 4] = float('nan')
    a[20] = 0
    a[20, 0], a[20, 1] = 2.0, -2.0                                   # cancels exactly against the equal columns of b
    a[21] = 0
    a[21, 15], a[21, 16] = -4.0, 4.0
    b[:, 1] = b[:, 0]
    b[:, 16] = b[:, 15]
    a[22] = 0                                                        # a row of zero products
    b[40] = 1e-30                                                    # products that underflow to subnormals with a[23]
    a[23] = torch.randn(k, generator=g) * 1e-12
    a, b = a.to(gpu), (b.t().contiguous() if layout_kn else b).to(gpu)
    bias = torch.zeros(n, device=gpu)
    for epi, kw in ((ops.EPI_STORE_F32, {}), (ops.EPI_STORE, dict(bias=bias)), (ops.EPI_GELU, {})):
        ref, got = _both(ops, lambda: ops.gemm(a, b, b_layout=layout, epilogue=epi, **kw))
        assert _same(ref, got), f'epilogue {epi}'
    out = ops.gemm(a, b, b_layout=layout, epilogue=ops.EPI_STORE_F32)
    assert bool(out[:, 11].isnan().all()) and bool(out[7].isinf().sum() > 100)
    assert bool((out[5, :11] != 0).all()) and float(out[5, :11].abs().max()) < 1e-37         # subnormal operands are not flushed
    assert bool((_bits(out[20, :11]) == 0).all()) and bool((_bits(out[21, :11]) == 0).all())  # exact cancellation: +0
    assert bool((_bits(out[22, :11]) == 0).all())


@pytest.mark.parametrize('accumulate', [False, True], ids=['write', 'accumulate'])
@pytest.mark.parametrize('want_bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('shape', TN_SHAPES, ids=['x'.join(map(str, s)) for s in TN_SHAPES])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
def test_weight_gradient(vited, gpu, dtype, shape, want_bias, accumulate):
    ops = vited.ops
    m, n, k = shape
    g = torch.Generator().manual_seed(m + n + k)
    dy, x = torch.randn(m, n, generator=g).to(gpu, dtype), torch.randn(m, k, generator=g).to(gpu, dtype)
    dw0, db0 = torch.randn(n, k, generator=g).to(gpu), torch.randn(n, generator=g).to(gpu)
    seen = []

    def run():
        if accumulate:
            dw, db = dw0.clone(), db0.clone() if want_bias else None
            ops.linear_bwd_weight(dy, x, want_bias=want_bias, dw_out=dw, db_out=db)
        else:
            dw, db = ops.linear_bwd_weight(dy, x, want_bias=want_bias)
        seen.append((ops.last_paths()[0], ops.last_fp32_gemm_kernel()))
        return dw, db

    with ops.fp32_gemm_kernels('valu'):
        ref = run()
    with ops.fp32_gemm_kernels('auto'):
        got = run()
    assert _same(ref, got)
    if dtype == torch.float32:          # the product is [n, k] over m: the predicate sees that shape
        auto = 2 if ops.fp32_gemm_supported(n, k, m, b_layout=ops.B_KN, epilogue=ops.EPI_STORE_F32) else 1
        assert seen == [(1, 1), (1, auto)], seen
        assert auto == (1 if shape == TN_SHAPES[0] else 2)
    want = dy.double().t() @ x.double() + (dw0.double() if accumulate else 0)
    assert _within_chain_error(got[0], want, dy.double().abs().t() @ x.double().abs() + dw0.double().abs(), m + 2)
    assert (got[1] is not None) == want_bias


def test_the_head_stays_on_the_vector_alu_kernel(vited, gpu):
    ops = vited.ops
    a, b, x = _operands(gpu, torch.float32, 33, 4, 384, False, seed=6)
    ref, got = _both(ops, lambda: ops.gemm(a, b, epilogue=ops.EPI_STORE_F32, bias=x['bias']), want_auto=1)
    assert _same(ref, got)


# ---- the model ----------------------------------------------------------------------------------------------------------------
SHAPE = dict(img_size=16, patch_size=8, embed_dim=64, num_heads=2, depth=1, c_depth=2)
BATCH = 16


def _model(vited, gpu, rate=0.):
    s = vo.ViTEDShape(**SHAPE)
    torch.manual_seed(0)
    oracle = vo.OracleViTED(s)
    m = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                      embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads,
                                      mlp_ratio=s.mlp_ratio, qkv_bias=s.qkv_bias, drop_path_rate=rate)
    m.compute_dtype = torch.float32
    m.load_state_dict(oracle.state_dict())
    x = torch.randn(BATCH, 2, 3, s.img_size, s.img_size).clamp(-1, 1).to(gpu)
    y = (torch.rand(BATCH, s.num_classes) > 0.75).float().to(gpu)
    return s, m.to(gpu), x, y


def _step(ops, model, x, y, mode, **fwd):
    """One forward + backward outside autocast under ``mode``: logits, gradients, and the kernels its GEMMs reported."""
    kernels = []
    real_gemm, real_bww = ops.gemm, ops.linear_bwd_weight

    def spy(fn):
        def wrapped(*a, **k):
            out = fn(*a, **k)
            kernels.append((ops.last_paths()[0], ops.last_fp32_gemm_kernel()))
            return out
        return wrapped

    model.zero_grad(set_to_none=True)
    ops.gemm, ops.linear_bwd_weight = spy(real_gemm), spy(real_bww)
    try:
        with ops.fp32_gemm_kernels(mode):
            logits = model(x, **fwd)
            BCE(logits, y).backward()
    finally:
        ops.gemm, ops.linear_bwd_weight = real_gemm, real_bww
    return logits.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}, kernels


def _check_step(ops, model, x, y, **fwd):
    lr, gr, kr = _step(ops, model, x, y, 'valu', **fwd)
    la, ga, ka = _step(ops, model, x, y, 'auto', **fwd)
    assert kr and set(kr) == {(1, 1)}, kr
    assert len(ka) == len(kr) and (1, 2) in ka and all(p == 1 for p, _ in ka), ka
    assert _same(lr, la), 'logits differ between the kernels'
    assert sorted(gr) == sorted(ga) and len(gr) > 10
    for n in gr:
        assert _same(gr[n], ga[n]), f'{n}: gradients differ between the kernels'
    assert bool(la.isfinite().all()) and float(la.abs().max()) > 0
    return ka


def test_model_outside_autocast(vited, gpu):
    _, model, x, y = _model(vited, gpu)
    ka = _check_step(vited.ops, model.train(), x, y)
    assert (1, 1) in ka                       # ... and the 4-logit head stayed on the vector-ALU kernel


def test_model_with_stochastic_depth_scales(vited, gpu):
    """Forced DropPathScales: the residual Linears of the fp32 mode run the scaled epilogue (vited_gemm_scaled)."""
    ops = vited.ops
    s, model, x, y = _model(vited, gpu, rate=0.5)
    enc = dc.irregular_scales(0.5, s.depth, 2, BATCH, salt=3)
    dec = dc.irregular_scales(0.5, s.c_depth, 3, BATCH, salt=5)
    drop = vited.DropPathScales(enc.to(gpu), dec.to(gpu))
    scaled = []
    real = ops.gemm

    def spy(*a, **k):
        out = real(*a, **k)
        if k.get('row_scale') is not None:
            scaled.append(ops.last_fp32_gemm_kernel())
        return out

    ops.gemm = spy
    try:
        _check_step(ops, model.train(), x, y, drop_path=drop)
    finally:
        ops.gemm = real
    half = len(scaled) // 2            # the 'valu' step, then the 'auto' step; the last decoder block runs on the 16 cls rows only
    assert half >= 1 and set(scaled[:half]) == {1} and 2 in scaled[half:], scaled


def test_captured_forward_replays_the_vector_alu_result(vited, gpu):
    """The kernel is chosen when the launch is recorded: a graph captured under 'auto' replays the matrix-core kernels whatever the
    mode at replay, and gives the eager 'valu' bits."""
    ops = vited.ops
    _, model, x, _ = _model(vited, gpu)
    model.eval()
    static_x = x.clone()
    with torch.no_grad():
        with ops.fp32_gemm_kernels('valu'):
            want = model(x).clone()
            fresh = x.flip(0).contiguous()
            want_fresh = model(fresh).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(static_x)                                          # sizes the workspace before the capture
        torch.cuda.current_stream().wait_stream(side)
        gc.collect()
        torch.cuda.synchronize()
        ops.pin_workspace()
        graph = torch.cuda.CUDAGraph()
        recorded, real = [], ops.gemm

        def spy(*a, **k):
            res = real(*a, **k)
            recorded.append((ops.last_paths()[0], ops.last_fp32_gemm_kernel()))
            return res

        ops.gemm = spy
        try:
            with ops.fp32_gemm_kernels('auto'):
                with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                    out = model(static_x)
        finally:
            ops.gemm = real
        assert (1, 2) in recorded and all(p == 1 for p, _ in recorded), recorded
        with ops.fp32_gemm_kernels('valu'):                          # the mode at replay does not matter
            graph.replay()
            assert _same(out, want)
            static_x.copy_(fresh)
            graph.replay()
            assert _same(out, want_fresh)
    assert not _same(want, want_fresh)
