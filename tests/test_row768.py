"""CPU: the C ABI of the row-complete Linear + LayerNorm kernels at N == 768 (gemm_row768.hip), through ctypes.  Every call
here is refused by an argument check, or is a plain size query: nothing is launched (there is no GPU here).

The predicate's cases follow the measured rule of DESIGN.md section 35 (the entries themselves take every shape the kernels compute).
Fail on the commit before the 768-wide kernels (marked NEW below): every ``supported(...) == 1`` case at N == 768, the
``workspace_bytes(M, 768) > 0`` cases, and everything that names ``vited_linear_layernorm_bwd_partial_rows_n`` (a missing symbol
there).  The refusals of the five entries at N == 768 were all VITED_ERR_UNSUPPORTED before; the BAD_ARG / WORKSPACE cases that
sit behind the shape check are new as well."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, UNSUPPORTED, LAUNCH, WORKSPACE = 0, 1, 2, 3, 4
N = 768
STEP_ROWS = (24 * 576, 72 * 577, 72)      # ViT-Base at 384 x 384: 24 images, 72 mined pairs, the cls-only last block


@pytest.fixture(scope='module')
def lib(vited):
    if not os.path.exists(vited._lib.LIB_PATH):
        subprocess.run(['make', '-C', os.path.join(ROOT, 'vit-ed_amd', 'csrc'), '-j', '8'], check=True)
    return vited._lib.load()


BIG = 72 * 577             # the decoder's rows of a ViT-Base step: more than one round of 96-row tiles


@pytest.mark.parametrize('K', [1536, 2304, 12 * 1536, 1 << 20])
def test_supported_at_768(lib, K):
    """The predicate is what the kernels compute AND where they measured faster than the two kernels: more
    than 24,576 rows, and K neither N nor 4 N (the forward Linears' contractions, whose fused form only ties)."""
    s = lib.vited_linear_layernorm_supported
    assert s(BIG, N, K) == 1                                                         # NEW
    assert s(256 * 96 + 1, N, K) == 1                                                # NEW
    assert s((1 << 31) - 1, N, K) == 1                                               # NEW
    assert s(256 * 96, N, K) == 0 and s(24 * 576, N, K) == 0 and s(4096, N, K) == 0  # at most one round of tiles: slower or a tie
    assert s(1 << 31, N, K) == 0 and s(0, N, K) == 0


def test_unsupported_shapes(lib):
    s = lib.vited_linear_layernorm_supported
    assert s(BIG, N, 768) == 0 and s(BIG, N, 3072) == 0      # K = N, 4 N: the forward ties with the two kernels there
    assert s(BIG, N, 384) == 0           # below the K >= 768 floor
    assert s(4096, N, 384) == 0 and s(128, N, 384) == 0      # (tests/test_gpu_ops.py pins the second)
    assert s(BIG, N, 704) == 0
    assert s(BIG, N, 800) == 0           # K % 64
    assert s(BIG, N, (1 << 20) + 64) == 0
    assert s(BIG, 512, 768) == 0 and s(4096, 512, 768) == 0  # no such width
    assert s(BIG, 1536, 1536) == 0
    # the 384 answers of test_abi.py hold unchanged
    assert s(4096, 384, 384) == 1 and s(4096, 384, 96) == 0 and s(4096, 512, 384) == 0
    assert s(4096, 384, 64) == 1 and s(4096, 384, 768) == 1 and s(BIG, 384, 1536) == 1


def test_partial_rows_and_workspace(lib):
    rows_n, rows, ws = (lib.vited_linear_layernorm_bwd_partial_rows_n, lib.vited_linear_layernorm_bwd_partial_rows,
                        lib.vited_linear_layernorm_bwd_workspace_bytes)
    for M in (1, 100, 65536, 66560, 72 * 1025, 24576):
        assert rows_n(M, 384) == rows(M)                                             # NEW (symbol)
        assert ws(M, 384) == rows(M) * 2 * 384 * 4
    for M in STEP_ROWS + (1, 13, 64, 65, 97, 4096 + 33, 65536):
        assert ws(M, N) == rows_n(M, N) * 2 * N * 4 and ws(M, N) > 0                 # NEW
    assert rows_n(0, N) == 0 and rows_n(-1, 384) == 0 and rows_n(4096, 512) == 0 and ws(0, N) == 0 and ws(4096, 512) == 0


def test_tile_heights_cover_the_step_rows(lib):
    """64- or 96-row tiles, the smallest makespan over rounds of 256 workgroups: 13,824 rows = 216 x 64 (one round),
    41,544 = 433 x 96 (two rounds), 72 = 2 x 64."""
    rows_n = lib.vited_linear_layernorm_bwd_partial_rows_n
    for M, tiles, height in zip(STEP_ROWS, (216, 433, 2), (64, 96, 64)):
        assert rows_n(M, N) == tiles                                                 # NEW
        assert tiles * height >= M > (tiles - 1) * height


# ---- refusals: fake, suitably aligned device addresses; every case fails a check in front of the launch ----------------------
P = 0x7f0000000000            # "device pointer", 256-byte aligned
M_, K_ = 200, 1536


def _fwd(lib, scaled, **kw):
    a = dict(a=P, lda=K_, w=P, ldw=K_, bias=P, residual=P, ldr=N, row_scale=P, y=P, ldy=N, gamma=P, beta=P, eps=1e-6, h=P, ldh=N, mean=P, rstd=P,
             M=M_, N=N, K=K_)
    a.update(kw)
    head = (a['a'], a['lda'], a['w'], a['ldw'], a['bias'], a['residual'], a['ldr'])
    tail = (a['y'], a['ldy'], a['gamma'], a['beta'], a['eps'], a['h'], a['ldh'], a['mean'], a['rstd'], a['M'], a['N'], a['K'], None)
    if scaled:
        return lib.vited_linear_residual_layernorm_fwd_scaled(*head, a['row_scale'], *tail)
    return lib.vited_linear_residual_layernorm_fwd(*head, *tail)


@pytest.mark.parametrize('scaled', [False, True])
def test_forward_refusals(lib, scaled):
    for name in ('a', 'w', 'residual', 'y'):
        assert _fwd(lib, scaled, **{name: None}) == BAD_ARG, name
    for name, short in (('lda', K_ - 8), ('ldw', K_ - 8), ('ldr', N - 4), ('ldy', N - 4), ('ldh', N - 4)):
        assert _fwd(lib, scaled, **{name: short}) == BAD_ARG, name
    for name in ('gamma', 'beta', 'mean', 'rstd'):       # h given without what the LayerNorm needs
        assert _fwd(lib, scaled, **{name: None}) == BAD_ARG, name
    for name, odd in (('lda', K_ + 4), ('ldw', K_ + 4), ('ldr', N + 2), ('ldy', N + 2), ('ldh', N + 2)):
        assert _fwd(lib, scaled, **{name: odd}) == UNSUPPORTED, name
    for name in ('a', 'w', 'residual', 'y', 'bias', 'gamma', 'beta'):
        assert _fwd(lib, scaled, **{name: P + 8}) == BAD_ARG, name
    assert _fwd(lib, scaled, h=P + 4) == BAD_ARG
    assert _fwd(lib, scaled, M=0) == BAD_ARG and _fwd(lib, scaled, K=0) == BAD_ARG
    assert _fwd(lib, scaled, K=384, lda=384, ldw=384) == UNSUPPORTED
    assert _fwd(lib, scaled, K=800, lda=800, ldw=800) == UNSUPPORTED
    assert _fwd(lib, scaled, N=512, ldr=512, ldy=512, ldh=512) == UNSUPPORTED


def _bwd(lib, form, **kw):
    a = dict(dy=P, lddy=K_, seg_k=K_ // 3, seg_stride=M_ * (K_ // 3), segments=3, wt=P, ldwt=K_, x=P, ldx=N, gamma=P, mean=P, rstd=P, dx_in=P,
             dx_in_ld=N, dx_out=P, dx_out_ld=N, dx_lp=P, dx_lp_ld=N, lp_scale=P, dgamma=P, dbeta=P, accumulate=0, M=M_, N=N, K=K_, workspace=P,
             workspace_bytes=None)
    a.update(kw)
    if a['workspace_bytes'] is None:
        a['workspace_bytes'] = max(lib.vited_linear_layernorm_bwd_workspace_bytes(a['M'], a['N']), 0)
    mid = (a['x'], a['ldx'], a['gamma'], a['mean'], a['rstd'], a['dx_in'], a['dx_in_ld'], a['dx_out'], a['dx_out_ld'], a['dx_lp'], a['dx_lp_ld'])
    sums = (a['dgamma'], a['dbeta'], a['accumulate'])
    ws = (a['workspace'], a['workspace_bytes'], None)
    if form == 'segmented':
        if 'lddy' not in kw:
            a['lddy'] = a['seg_k']
        return lib.vited_linear_layernorm_bwd_segmented(a['dy'], a['lddy'], a['seg_k'], a['seg_stride'], a['segments'], a['wt'], a['ldwt'], *mid,
                                                        *sums, a['M'], a['N'], *ws)
    if form == 'scaled':
        return lib.vited_linear_layernorm_bwd_scaled(a['dy'], a['lddy'], a['wt'], a['ldwt'], *mid, a['lp_scale'], *sums, a['M'], a['N'], a['K'], *ws)
    return lib.vited_linear_layernorm_bwd(a['dy'], a['lddy'], a['wt'], a['ldwt'], *mid, *sums, a['M'], a['N'], a['K'], *ws)


@pytest.mark.parametrize('form', ['plain', 'scaled', 'segmented'])
def test_backward_refusals(lib, form):
    for name in ('dy', 'wt', 'x', 'gamma', 'mean', 'rstd', 'dx_out'):
        assert _bwd(lib, form, **{name: None}) == BAD_ARG, name
    assert _bwd(lib, form, dgamma=None) == BAD_ARG and _bwd(lib, form, dbeta=None) == BAD_ARG      # both or neither
    extent = K_ // 3 if form == 'segmented' else K_
    for name, short in (('lddy', extent - 8), ('ldwt', K_ - 8), ('ldx', N - 4), ('dx_out_ld', N - 4), ('dx_in_ld', N - 4), ('dx_lp_ld', N - 4)):
        assert _bwd(lib, form, **{name: short}) == BAD_ARG, name
    for name, odd in (('lddy', extent + 4), ('ldwt', K_ + 4), ('ldx', N + 2), ('dx_out_ld', N + 2), ('dx_in_ld', N + 2), ('dx_lp_ld', N + 2)):
        assert _bwd(lib, form, **{name: odd}) == UNSUPPORTED, name
    for name in ('dy', 'wt', 'x', 'gamma', 'dx_in', 'dx_out'):
        assert _bwd(lib, form, **{name: P + 8}) == BAD_ARG, name
    assert _bwd(lib, form, dx_lp=P + 4) == BAD_ARG
    assert _bwd(lib, form, M=0) == BAD_ARG
    need = lib.vited_linear_layernorm_bwd_workspace_bytes(M_, N)
    assert need > 0                                                                                  # NEW
    assert _bwd(lib, form, workspace_bytes=need - 4) == WORKSPACE                                    # NEW
    assert _bwd(lib, form, workspace=None) == WORKSPACE                                              # NEW
    assert _bwd(lib, form, N=512, ldx=512, dx_out_ld=512, dx_in_ld=512, dx_lp_ld=512, workspace_bytes=1 << 30) == UNSUPPORTED
    if form == 'scaled':
        assert _bwd(lib, form, dx_lp=None) == BAD_ARG            # the scale applies to the bf16 copy: it must exist
    if form != 'segmented':
        assert _bwd(lib, form, K=384, lddy=384, ldwt=384) == UNSUPPORTED
        assert _bwd(lib, form, K=800, lddy=800, ldwt=800) == UNSUPPORTED
    else:
        assert _bwd(lib, form, segments=0) == BAD_ARG
        assert _bwd(lib, form, seg_k=0) == BAD_ARG
        assert _bwd(lib, form, seg_k=480, lddy=480, segments=2, ldwt=960) == UNSUPPORTED      # seg_k % 64
        assert _bwd(lib, form, seg_stride=M_ * (K_ // 3) + 4) == UNSUPPORTED                  # segments 16-byte aligned
        assert _bwd(lib, form, seg_k=128, lddy=128, segments=3, ldwt=384) == UNSUPPORTED      # K = 384: below the floor
