"""The matrix-core fp32 attention kernels (attention_f32_mfma.hip) against the vector-ALU kernels they stand in for
(attention_portable.hip), bit for bit.

v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain and every product of the portable kernels is such a chain, so forward (o, lse) and
backward (delta, dq, dk, dv) have to be the same BITS: every comparison is ``torch.equal`` on the integer view (NaN patterns and the
sign of zero count) and there is no tolerance anywhere.  ``ops.fp32_attention_kernels('valu')`` runs the unchanged portable kernels,
'auto' the dispatch a user gets.  Shapes sit on the edges of the 32-key tile, of the 32-row accumulator and of the 128-row workgroup."""
import gc

import pytest
import torch

from oracle import vited_oracle as vo

pytestmark = pytest.mark.gpu

BATCH, HEADS = 3, 2
GRID = [(1, 1), (1, 65), (31, 33), (32, 32), (33, 31), (64, 64), (65, 64), (65, 65), (130, 257)]
NEG_ZERO = -2 ** 31
BCE = torch.nn.functional.binary_cross_entropy_with_logits


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _both(ops, fn, want_auto=2):
    """fn() under 'valu' and under 'auto': the two results, after checking which kernels each reported."""
    with ops.fp32_attention_kernels('valu'):
        ref = fn()
        assert ops.last_fp32_attention_kernel() == 1 and ops.last_paths()[1] == 1
    with ops.fp32_attention_kernels('auto'):
        got = fn()
        assert ops.last_fp32_attention_kernel() == want_auto and ops.last_paths()[1] == 1
    return ref, got


def _unaligned(t, gpu, dtype):
    """``t`` on the GPU at a base one element past an aligned one: what keeps bf16 operands off the bf16 MFMA attention."""
    flat = torch.empty(t.numel() + 1, dtype=dtype, device=gpu)
    flat[1:].copy_(t.reshape(-1))
    return flat[1:].view(t.shape)


def _operands(gpu, dtype, nq, nk, hd, seed=0, batch=BATCH, items=None):
    g = torch.Generator().manual_seed(seed * 7919 + nq * 131 + nk * 17 + hd)
    d = HEADS * hd
    q, do = torch.randn(batch, nq, d, generator=g), torch.randn(batch, nq, d, generator=g)
    k, v = torch.randn(items or batch, nk, d, generator=g), torch.randn(items or batch, nk, d, generator=g)
    if dtype == torch.bfloat16:
        return [_unaligned(t, gpu, dtype) for t in (q, k, v, do)]
    return [t.to(gpu) for t in (q, k, v, do)]


def _backward(vited, q, k, v, o, do, lse, scale):
    """vited_attention_bwd with a delta buffer of the test's own: (delta, dq, dk, dv)."""
    ops = vited.ops
    (b, nq, d), nk = q.shape, k.shape[1]
    o, do = o.contiguous(), do.contiguous()
    delta = torch.full((b, HEADS, nq), float('nan'), device=q.device)
    dq, dk, dv = (torch.full(t.shape, float('nan'), dtype=q.dtype, device=q.device) for t in (q, k, v))
    vited._lib.call('vited_attention_bwd', q.data_ptr(), *q.stride()[:2], k.data_ptr(), *k.stride()[:2], v.data_ptr(), *v.stride()[:2],
                    o.data_ptr(), do.data_ptr(), nq * d, d, lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), nq * d, d, dk.data_ptr(),
                    nk * d, d, dv.data_ptr(), nk * d, d, ops._code(q.dtype), b, HEADS, nq, nk, d // HEADS, float(scale), ops._stream())
    return delta, dq, dk, dv


def _check_both_ways(vited, q, k, v, do, scale):
    """Forward and backward under both modes; returns the 'auto' results (o, lse, delta, dq, dk, dv)."""
    ops = vited.ops
    ref, got = _both(ops, lambda: ops.attention_fwd(q, k, v, HEADS, scale))
    assert _same(ref[0], got[0]), 'o differs between the kernels'
    assert _same(ref[1], got[1]), 'lse differs between the kernels'
    o, lse = ref
    rb, gb = _both(ops, lambda: _backward(vited, q, k, v, o, do, lse, scale))
    for name, x, y in zip(('delta', 'dq', 'dk', 'dv'), rb, gb):
        assert _same(x, y), f'{name} differs between the kernels'
    return (*got, *gb)


@pytest.mark.parametrize('shape', GRID, ids=[f'{a}x{b}' for a, b in GRID])
@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
def test_shape_grid(vited, gpu, dtype, hd, shape):
    ops = vited.ops
    nq, nk = shape
    q, k, v, do = _operands(gpu, dtype, nq, nk, hd)
    assert ops.fp32_attention_supported(BATCH, HEADS, nq, nk, hd, dtype=dtype)
    assert ops.fp32_attention_supported(BATCH, HEADS, nq, nk, hd, backward=True, dtype=dtype)
    o, lse, delta, dq, dk, dv = _check_both_ways(vited, q, k, v, do, hd ** -0.5)
    # not vacuous: the result is the attention of the stored operands (fp64 reference), every output element written
    qd, kd, vd, dod = (t.double().view(BATCH, -1, HEADS, hd).transpose(1, 2) for t in (q, k, v, do))
    s = qd @ kd.transpose(2, 3) * hd ** -0.5
    p = s.softmax(-1)
    want = (p @ vd).transpose(1, 2).reshape(BATCH, nq, -1)
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    assert float((o.double() - want).abs().max()) < tol
    assert float((lse.double() - s.logsumexp(-1)).abs().max()) < 1e-5
    dp = dod @ vd.transpose(2, 3)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    for got, ref in ((dq, ds @ kd * hd ** -0.5), (dk, ds.transpose(2, 3) @ qd * hd ** -0.5), (dv, p.transpose(2, 3) @ dod)):
        assert float((got.double() - ref.transpose(1, 2).reshape(got.shape)).abs().max()) < 10 * tol * (1 + float(ref.abs().max()))
    assert bool(delta.isfinite().all())


# pad 3: no vector loads; pad 4: bf16 rows that take vector loads but not the bf16 MFMA kernels (token stride no multiple of 8)
VIEWS = [(torch.float32, 0), (torch.float32, 3), (torch.bfloat16, 3), (torch.bfloat16, 4)]


@pytest.mark.parametrize('dtype,pad', VIEWS, ids=[f'{str(d)[6:]}-pad{p}' for d, p in VIEWS])
def test_views_of_a_packed_projection(vited, gpu, dtype, pad):
    """q / k / v as column slices of one [B, N, 3D (+ pad)] buffer, on the vector and on the element-wise staging path."""
    n, hd = 65, 32
    d = HEADS * hd
    g = torch.Generator().manual_seed(21)
    qkv = torch.randn(BATCH, n, 3 * d + pad, generator=g).to(gpu, dtype)
    do = torch.randn(BATCH, n, d, generator=g).to(gpu, dtype)
    _check_both_ways(vited, qkv[:, :, :d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:3 * d], do, hd ** -0.5)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
def test_kv_index_with_repeated_and_unused_items(vited, gpu, dtype):
    ops = vited.ops
    nq, nk, hd, pairs, items = 33, 65, 64, 5, 4
    q, k, v, do = _operands(gpu, dtype, nq, nk, hd, seed=3, batch=pairs, items=items)
    index = torch.tensor([2, 0, 2, 2, 0], device=gpu)                 # items 1 and 3 have no pair
    ref, got = _both(ops, lambda: ops.attention_fwd(q, k, v, HEADS, hd ** -0.5, kv_index=index))
    assert _same(ref, got)
    plain = ops.attention_fwd(q[3:4], k[2:3], v[2:3], HEADS, hd ** -0.5)
    assert _same(plain[0], got[0][3:4]) and _same(plain[1], got[1][3:4])
    o, lse = ref
    seg = ops.pair_segments(index, items)

    def run():
        dq, dk, dv = torch.full_like(q, 9.0), torch.full_like(k, 9.0), torch.full_like(v, 9.0)
        return ops.attention_bwd(q, k, v, o, do.contiguous(), lse, HEADS, hd ** -0.5, dq, dk, dv, segments=seg)

    rb, gb = _both(ops, run)
    assert _same(rb, gb)
    for grad in gb[1:]:
        assert bool((grad[1] == 0).all()) and bool((grad[3] == 0).all())  # an item without a pair gets zeros
        assert float(grad[0].float().abs().max()) > 0 and float(grad[2].float().abs().max()) > 0


@pytest.mark.parametrize('hd', [32, 64])
def test_planted_values(vited, gpu, hd):
    """A key row of zeros, a query whose scores are all equal, alpha underflowing to 0 between tiles, +-inf and a NaN in V, subnormal K."""
    nq, nk = 33, 70
    q, k, v, do = _operands(gpu, torch.float32, nq, nk, hd, seed=5)
    k[:, 5] = 0
    q[:, 3] = 0                                                       # every score of this query is +0
    k[:, 9] = 1e-40
    k[:, 10] = -1e-40
    # query 7 against keys whose scores are -150 in the first tile and +150 at key 40: exp(m - mn) is 0 when the second tile arrives
    q[:, 7] = 0
    q[:, 7, 0::hd] = 150 * hd ** 0.5
    k[:, :, 0::hd] = -1
    k[:, 40, 0::hd] = 1
    v[0, 2, 1], v[1, 4, 3], v[2, 6, 5] = float('inf'), float('-inf'), float('nan')
    o, lse, delta, dq, dk, dv = _check_both_ways(vited, q, k, v, do, hd ** -0.5)
    assert bool(o[0, :, 1].isnan().logical_or(o[0, :, 1].isinf()).all()) and bool(o[2, :, 5].isnan().all())
    assert bool(lse.isfinite().all())
    assert torch.allclose(lse[:, :, 3], torch.full_like(lse[:, :, 3], float(torch.tensor(float(nk)).log())))
    assert torch.equal(o[:, 7, hd + 1:2 * hd], v[:, 40, hd + 1:2 * hd])          # all the weight on key 40 once the first tile is forgotten


@pytest.mark.parametrize('hd', [32, 64])
def test_gradients_that_end_as_negative_zero(vited, gpu, hd):
    """Chains whose every product rounds to -0 end as -0: a padding product of +0 in the odd slot of the last instruction would
    flip them.  dv: dO column of the smallest negative subnormal (p < 1/2).  dq / dk: a K / Q column of smallest subnormals whose
    signs oppose ds (they are too small to move a score)."""
    nq, nk, col = 33, 33, 5
    tiny = 2.0 ** -149
    q, k, v, do = (t.cpu() for t in _operands(gpu, torch.float32, nq, nk, hd, seed=9))
    q, k, do = q * 0.3, k * 0.3, do * 0.3
    do[:, :, col] = -tiny
    qd, kd, vd, dod = (t.double().view(BATCH, -1, HEADS, hd).transpose(1, 2) for t in (q, k, v, do))
    p = (qd @ kd.transpose(2, 3) * hd ** -0.5).softmax(-1)
    dp = dod @ vd.transpose(2, 3)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))                    # [B, H, nq, nk]
    used = torch.cat([ds[:, 0, 0].reshape(-1), ds[:, 0, :, 0].reshape(-1)]).abs()          # far from 0 (the sign is safe) and below 1/2
    assert float(p.max()) < 0.5 and float(used.max()) < 0.5 and float(used.min()) > 1e-5
    k[:, :, col + 1] = -tiny * ds[:, 0, 0].sign().float()             # dq[b, 0, col + 1] of head 0: every product is -(tiny |ds|)
    q[:, :, col + 2] = -tiny * ds[:, 0, :, 0].sign().float()          # dk[b, 0, col + 2] of head 0
    o, lse, delta, dq, dk, dv = _check_both_ways(vited, q.to(gpu), k.to(gpu), v.to(gpu), do.to(gpu), hd ** -0.5)
    assert bool((_bits(dv[:, :, col]) == NEG_ZERO).all())
    assert bool((_bits(dq[:, 0, col + 1]) == NEG_ZERO).all())
    assert bool((_bits(dk[:, 0, col + 2]) == NEG_ZERO).all())


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _model(vited, gpu, img_size, batch):
    s = vo.ViTEDShape(img_size=img_size, depth=2, c_depth=2)
    torch.manual_seed(0)
    oracle = vo.OracleViTED(s)
    m = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                      embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads,
                                      mlp_ratio=s.mlp_ratio, qkv_bias=s.qkv_bias)
    m.compute_dtype = torch.float32
    m.load_state_dict(oracle.state_dict())
    x = torch.randn(batch, 2, 3, s.img_size, s.img_size).clamp(-1, 1).to(gpu)
    y = (torch.rand(batch, s.num_classes) > 0.75).float().to(gpu)
    return m.to(gpu), x, y


def _spied(ops, record):
    def spy(fn):
        def wrapped(*a, **k):
            out = fn(*a, **k)
            record.append((ops.last_paths()[1], ops.last_fp32_attention_kernel()))
            return out
        return wrapped
    return spy(ops.attention_fwd), spy(ops.attention_bwd)


def _step(ops, model, x, y, mode):
    """One forward + backward outside autocast under ``mode``: logits, gradients, and the kernels its attention calls reported."""
    kernels = []
    real = ops.attention_fwd, ops.attention_bwd
    model.zero_grad(set_to_none=True)
    ops.attention_fwd, ops.attention_bwd = _spied(ops, kernels)
    try:
        with ops.fp32_attention_kernels(mode):
            logits = model(x)
            BCE(logits, y).backward()
    finally:
        ops.attention_fwd, ops.attention_bwd = real
    return logits.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}, kernels


@pytest.mark.parametrize('img_size,batch', [(64, 4), (128, 2)], ids=['64-65-tokens', '256-257-tokens'])
def test_model_step_outside_autocast(vited, gpu, img_size, batch):
    ops = vited.ops
    model, x, y = _model(vited, gpu, img_size, batch)
    model.train()
    lr, gr, kr = _step(ops, model, x, y, 'valu')
    la, ga, ka = _step(ops, model, x, y, 'auto')
    assert kr and set(kr) == {(1, 1)}, kr
    assert len(ka) == len(kr) and set(ka) <= {(1, 1), (1, 2)} and (1, 2) in ka, ka
    assert _same(lr, la), 'logits differ between the kernels'
    assert sorted(gr) == sorted(ga) and len(gr) > 10
    for n in gr:
        assert _same(gr[n], ga[n]), f'{n}: gradients differ between the kernels'
    assert bool(la.isfinite().all()) and float(la.abs().max()) > 0


def test_captured_forward_replays_the_vector_alu_result(vited, gpu):
    """The kernel is chosen when the launch is recorded: a graph captured under 'auto' replays the matrix-core kernels whatever the
    mode at replay, and gives the eager 'valu' bits."""
    ops = vited.ops
    model, x, _ = _model(vited, gpu, 64, 4)
    model.eval()
    static_x = x.clone()
    with torch.no_grad():
        with ops.fp32_attention_kernels('valu'):
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
        recorded, real = [], ops.attention_fwd
        ops.attention_fwd = _spied(ops, recorded)[0]
        try:
            with ops.fp32_attention_kernels('auto'):
                with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                    out = model(static_x)
        finally:
            ops.attention_fwd = real
        assert (1, 2) in recorded and all(p == 1 for p, _ in recorded), recorded
        with ops.fp32_attention_kernels('valu'):                     # the mode at replay does not matter
            graph.replay()
            assert _same(out, want)
            static_x.copy_(fresh)
            graph.replay()
            assert _same(out, want_fresh)
    assert not _same(want, want_fresh)
