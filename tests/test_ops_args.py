"""ops.py refuses a wrong tensor before the launch: every entry point is reached by a valid call, and every one-fault mutation of
that call's tensors (wrong dtype, one element short, a strided view where the entry assumes dense memory) raises and launches nothing.
No GPU: the device gate, the stream, the workspace and the library are replaced by stubs, the tensors live on the CPU."""
import ast
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS_PY = os.path.join(ROOT, 'vit-ed_amd', 'ops.py')
R, D, HID, H, S, N = 8, 64, 128, 2, 16, 4          # rows, dim, MLP hidden, heads, image size, images / fragments
B, NQ, NK = 2, 5, 3                                # attention batch, query and key tokens


class _Library:
    """What ``_lib.load()`` returns: every size query answers a number, every *_supported query 1."""

    def __getattr__(self, name):
        return lambda *args: 1 if name.endswith('_supported') else 4096


@pytest.fixture
def ops(vited, monkeypatch):
    calls = []
    monkeypatch.setattr(vited.ops, '_need_gpu', lambda *tensors, **kw: None)
    monkeypatch.setattr(vited.ops, '_stream', lambda: 0)
    monkeypatch.setattr(vited.ops, '_scratch', lambda nbytes, device, align=1: (0, 1 << 40))
    monkeypatch.setattr(vited.ops, '_lib', SimpleNamespace(call=lambda name, *args: calls.append((name, args)), load=_Library))
    vited.ops.calls = calls
    yield vited.ops
    del vited.ops.calls


def z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def bf(*shape):
    return z(*shape, dtype=torch.bfloat16)


def i32(*shape):
    return z(*shape, dtype=torch.int32)


def i64(*shape):
    return z(*shape, dtype=torch.int64)


def u8(*shape):
    return z(*shape, dtype=torch.uint8)


def _store():
    return dict(store=u8(4096), img_off=i64(3), img_hw=i32(3, 2))


def _ln(n=D):
    return dict(gamma=z(n), mean=z(R), rstd=z(R))


def _qkv(dtype=torch.float32, items=B):
    return dict(q=z(B, NQ, D, dtype=dtype), k=z(items, NK, D, dtype=dtype), v=z(items, NK, D, dtype=dtype))


def _attention_bwd(items=B):
    return dict(**_qkv(items=items), o=z(B, NQ, D), do=z(B, NQ, D), lse=z(B, H, NQ), heads=H, scale=0.2, dq=z(B, NQ, D), dk=z(items, NK, D),
                dv=z(items, NK, D))


def _block(cross):
    p = dict(x=z(B, NQ, D), heads=H, wqkv=bf(3 * D, D), bqkv=z(3 * D), wproj=bf(D, D), bproj=z(D), w1=bf(HID, D), b1=z(HID), w2=bf(D, HID), b2=z(D))
    if cross:
        p.update(context=z(B, NK, D), ln1=(z(D), z(D)), lnq=(z(D), z(D)), lnc=(z(D), z(D)), ln2=(z(D), z(D)), wq=bf(D, D), bq=z(D),
                 wkv=bf(2 * D, D), bkv=z(2 * D), wcproj=bf(D, D), bcproj=z(D))
    else:
        p.update(ln1_g=z(D), ln1_b=z(D), ln2_g=z(D), ln2_b=z(D))
    return p


def _segments(ops):
    return ops.pair_segments(torch.tensor([1, 0]), 3)


def _puzzle_state():
    return dict(min_d=i64(N, 4), second_d=i64(N, 4), compat=z(4, N, N), mutual=z(4, N, N))


def _csr():
    return (i32(3), i32(N))


# case -> (the op, its entry point(s), a builder of valid keyword arguments)
CASES = {
    'cast': ('cast', 'vited_cast', lambda ops: dict(src=z(R, D), dtype=torch.bfloat16, out=bf(R, D))),
    'scale_rows_cast': ('scale_rows_cast', 'vited_scale_rows_cast', lambda ops: dict(src=z(R, D), row_scale=z(R), dtype=torch.bfloat16)),
    'cast_transpose': ('cast_transpose', 'vited_cast_transpose', lambda ops: dict(w=z(R, D), dtype=torch.bfloat16, out=bf(D, R))),
    'weight_shadow_plan': ('WeightShadowPlan', 'vited_cast_weights', lambda ops: dict(entries=[(z(R, D), bf(R, D), bf(D, R))])),
    'patchify': ('patchify', 'vited_patchify', lambda ops: dict(img=z(N, 3, S, S), patch=8, dtype=torch.bfloat16, batch_index=i64(2))),
    'patchify_u8': ('patchify', 'vited_patchify_u8', lambda ops: dict(img=u8(N, 3, S, S), patch=8, dtype=torch.bfloat16, batch_index=i64(2))),
    'crop_pairs_u8': ('crop_pairs_u8', 'vited_crop_pairs_u8', lambda ops: dict(
        regions=u8(N, 3, 2 * S, 3 * S), cells=i32(N, 2), erode=i32(N), img_size=S)),
    'div2k_regions_u8': ('div2k_regions_u8', 'vited_div2k_regions_u8', lambda ops: dict(
        **_store(), image=i32(N), flags=i32(N), minv=z(N, 6, dtype=torch.float64), rgb=z(N, 3), crop=i32(N, 2), img_size=S,
        out=u8(N, 3, 2 * S, 3 * S))),
    'hisfrag_windows_u8': ('hisfrag_windows_u8', 'vited_hisfrag_windows_u8', lambda ops: dict(
        **_store(), image=i32(N), flags=i32(N), afix=i64(N, 6), minv=z(N, 6, dtype=torch.float64), origin=i32(N, 2), img_size=S, out=u8(N, 3, S, S))),
    'hisfrag_jitter_u8': ('hisfrag_jitter_u8', 'vited_hisfrag_jitter_u8', lambda ops: dict(
        img=u8(N, 3, S, S), flags=i32(N), order=i32(N, 4), factors=z(N, 3), hue=i32(N), out=u8(N, 3, S, S))),
    'hisfrag_blur_u8': ('hisfrag_blur_u8', 'vited_hisfrag_blur_u8', lambda ops: dict(
        img=u8(N, 3, S, S), flags=i32(N), weights=z(N, 2), out=u8(N, 3, S, S))),
    'michigan_windows_u8': ('michigan_windows_u8', 'vited_michigan_windows_u8', lambda ops: dict(
        **_store(), image=i32(N), flags=i32(N), origin=i32(N, 2), x0=i32(N, S), kx=i32(N, S, 3), y0=i32(N, S), ky=i32(N, S, 3), holes=i32(N, 16, 4),
        n_holes=i32(N), img_size=S, out=u8(N, 3, S, S))),
    'michigan_blur_gray_u8': ('michigan_blur_gray_u8', 'vited_michigan_blur_gray_u8', lambda ops: dict(
        img=u8(N, 3, S, S), flags=i32(N), weights=i32(N, 2), out=u8(N, 3, S, S))),
    'slice_rows_cast': ('slice_rows_cast', 'vited_slice_rows_cast', lambda ops: dict(x=z(B, NQ, D), row_offset=1, rows=NQ - 1, dtype=torch.bfloat16)),
    'write_cls_row': ('write_cls_row', 'vited_write_cls_row', lambda ops: dict(x=z(B, NQ, D), cls=z(D), pos=z(1, 1, D))),
    'sum_rows': ('sum_rows', 'vited_sum_rows', lambda ops: dict(x=z(R, D))),
    'layernorm_fwd': ('layernorm_fwd', 'vited_layernorm_fwd', lambda ops: dict(
        x=z(R, 384), gamma=z(384), beta=z(384), eps=1e-6, out_dtype=torch.bfloat16, out=(bf(R, 384), z(R), z(R)))),
    'layernorm_bwd': ('layernorm_bwd', 'vited_layernorm_bwd', lambda ops: dict(
        dy=bf(R, D), x=z(R, D), **_ln(), dx_in=z(R, D), dx_out=z(R, D), dx_lp=bf(R, D), dgamma=z(D), dbeta=z(D))),
    'layernorm_bwd_scaled': ('layernorm_bwd', 'vited_layernorm_bwd_scaled', lambda ops: dict(dy=z(R, D), x=z(R, D), **_ln(), lp_scale=z(R))),
    'qk_norm_fwd': ('qk_norm_fwd', 'vited_qk_norm_fwd', lambda ops: dict(
        q=z(R, D), k=z(R + 1, D), gq=z(D // H), bq=z(D // H), gk=z(D // H), bk=z(D // H), heads=H, eps=1e-6, out=(z(R, D), z(R + 1, D)))),
    'qk_norm_bwd': ('qk_norm_bwd', 'vited_qk_norm_bwd', lambda ops: dict(
        dq=z(R, D), q=z(R, D), q_stats=(z(R, H), z(R, H)), gq=z(D // H), dk=z(R + 1, D), k=z(R + 1, D), k_stats=(z(R + 1, H), z(R + 1, H)),
        gk=z(D // H), heads=H, dgq=z(D // H), dbq=z(D // H), dgk=z(D // H), dbk=z(D // H))),
    'gemm_store': ('gemm', 'vited_gemm', lambda ops: dict(a=bf(R, D), b=bf(16, D), bias=z(16), out=bf(R, 16))),
    'gemm_gelu': ('gemm', 'vited_gemm', lambda ops: dict(a=bf(R, D), b=bf(16, D), epilogue=ops.EPI_GELU_GRAD, out=bf(R, 16), out2=bf(R, 16))),
    'gemm_mul': ('gemm', 'vited_gemm', lambda ops: dict(a=bf(R, D), b=bf(D, 16), b_layout=ops.B_KN, epilogue=ops.EPI_MUL, aux=bf(R, 16))),
    'gemm_residual': ('gemm', 'vited_gemm', lambda ops: dict(a=bf(R, D), b=bf(16, D), epilogue=ops.EPI_RESIDUAL, residual=z(R, 16), out=z(R, 16))),
    'gemm_remap': ('gemm', 'vited_gemm', lambda ops: dict(
        a=bf(R, D), b=bf(16, D), epilogue=ops.EPI_RESIDUAL, residual=z(5, 16), rows_per_batch=4, out_rows_per_batch=5, row_offset=1,
        residual_bcast=True, out=z(10, 16))),
    'gemm_scaled': ('gemm', 'vited_gemm_scaled', lambda ops: dict(
        a=bf(R, D), b=bf(16, D), epilogue=ops.EPI_RESIDUAL, bias=z(16), residual=z(R, 16), row_scale=z(R), out=z(R, 16))),
    'linear_bwd_weight': ('linear_bwd_weight', 'vited_linear_bwd_weight', lambda ops: dict(dy=bf(R, 16), x=bf(R, D), dw_out=z(16, D), db_out=z(16))),
    'linear_bwd_weight_batched': ('linear_bwd_weight_batched', 'vited_linear_bwd_weight_batched', lambda ops: dict(
        items=[(bf(R, 16), bf(R, D), z(16, D), z(16))], accumulate=True)),
    'linear_residual_layernorm_fwd': ('linear_residual_layernorm_fwd', 'vited_linear_residual_layernorm_fwd', lambda ops: dict(
        a=bf(R, D), w=bf(D, D), bias=z(D), residual=z(R, D), gamma=z(D), beta=z(D), out=z(R, D))),
    'linear_residual_layernorm_fwd_scaled': ('linear_residual_layernorm_fwd', 'vited_linear_residual_layernorm_fwd_scaled', lambda ops: dict(
        a=bf(R, D), w=bf(D, D), bias=z(D), residual=z(R, D), row_scale=z(R))),
    'linear_layernorm_bwd': ('linear_layernorm_bwd', 'vited_linear_layernorm_bwd', lambda ops: dict(
        dy=bf(R, 16), wt=bf(D, 16), x=z(R, D), **_ln(), dx_in=z(R, D), dx_out=z(R, D), dgamma=z(D), dbeta=z(D))),
    'linear_layernorm_bwd_scaled': ('linear_layernorm_bwd', 'vited_linear_layernorm_bwd_scaled', lambda ops: dict(
        dy=bf(R, 16), wt=bf(D, 16), x=z(R, D), **_ln(), lp_scale=z(R))),
    'linear_layernorm_bwd_segmented': ('linear_layernorm_bwd', 'vited_linear_layernorm_bwd_segmented', lambda ops: dict(
        dy=bf(2, R, 16), wt=bf(D, 32), x=z(R, D), **_ln(), defer=[])),
    'layernorm_bwd_finish': ('layernorm_bwd_finish', 'vited_layernorm_bwd_finish_batched', lambda ops: dict(
        entries=[(z(4 * 2 * D), 4, z(D), z(D), True)])),
    'fold_context_weights': ('fold_context_weights', 'vited_fold_context_weights', lambda ops: dict(
        ws=[z(16, D), z(16, D)], biases=[z(16), None], gammas=[z(D), z(D)], betas=[z(D), z(D)], out=(bf(32, D), bf(D, 32), z(32)))),
    'unfold_context_grads': ('unfold_context_grads', 'vited_unfold_context_grads', lambda ops: dict(
        dwf=z(32, D), dbf=z(32), ws=[z(16, D), z(16, D)], gammas=[z(D), z(D)], betas=[z(D), z(D)], dws=[z(16, D), z(16, D)],
        dbiases=[z(16), None], dgammas=[z(D), z(D)], dbetas=[z(D), z(D)], accumulate=True)),
    'mlp_fwd': ('mlp_fwd', 'vited_mlp_fwd', lambda ops: dict(
        x=z(R, D), gamma=z(D), beta=z(D), w1=bf(HID, D), b1=z(HID), w2=bf(D, HID), b2=z(D), eps=1e-6,
        out=(z(R, D), z(R), z(R), bf(R, D), bf(R, HID), bf(R, HID)))),
    'block_fwd': ('block_fwd', 'vited_block_fwd', lambda ops: _block(cross=False)),
    'cross_block_fwd': ('cross_block_fwd', 'vited_cross_block_fwd', lambda ops: _block(cross=True)),
    'attention_fwd': ('attention_fwd', 'vited_attention_fwd_indexed', lambda ops: dict(**_qkv(items=3), heads=H, scale=0.2, kv_index=i64(B))),
    'attention_bwd': ('attention_bwd', 'vited_attention_bwd', lambda ops: _attention_bwd()),
    'attention_bwd_indexed': ('attention_bwd', 'vited_attention_bwd_indexed', lambda ops: dict(**_attention_bwd(items=3), segments=_segments(ops))),
    'attention_cam': ('attention_cam', 'vited_attention_cam', lambda ops: dict(
        **_qkv(), do=z(B, NQ, D), lse=z(B, H, NQ), heads=H, scale=0.2, mode='grad', out=z(B, NQ, NK))),
    'attention_cam_prob': ('attention_cam', 'vited_attention_cam', lambda ops: dict(
        q=z(B, NQ, D), k=z(B, NK, D), v=None, do=None, lse=z(B, H, NQ), heads=H, scale=0.2, mode='prob', head_weight=z(B, H))),
    'retrieval_metrics_rows': ('retrieval_metrics_rows', 'vited_retrieval_metrics', lambda ops: dict(
        matrix=z(N, N), labels=i32(N), offsets=i32(3), members=i32(N), rows=(0, N))),
    'group_retrieval_metrics_rows': ('group_retrieval_metrics_rows', 'vited_group_retrieval_metrics', lambda ops: dict(
        matrix=z(N, N), labels=i32(N), col_csr=_csr(), pos_csr=_csr(), neg_csr=_csr(), ks=(1, 2), rows=(0, N))),
    'pair_scores_add': ('pair_scores_add', 'vited_pair_scores_add', lambda ops: dict(
        pairs=i64(6, 2), scores=z(6), n=N, counts=i32(N, N), rec_cells=i32(6, 2), rec_values=z(6), bad=i32(1))),
    'pair_scores_finish': ('pair_scores_finish', 'vited_pair_scores_finish', lambda ops: dict(
        rec_cells=i32(6, 2), rec_values=z(6), n=N, counts=i32(N, N), bad=i32(1))),
    'puzzle_distances_from_logits': ('puzzle_distances_from_logits', 'vited_puzzle_distances_from_logits', lambda ops: dict(
        logits=z(6, 4), pi=i64(6), pj=i64(6), dq=i32(4, N, N), bad=i32(1))),
    'puzzle_compat_init': ('puzzle_compat_init', 'vited_puzzle_compat_init', lambda ops: dict(dq=i32(4, N, N))),
    'puzzle_compat_recalc': ('puzzle_compat_recalc', 'vited_puzzle_compat_recalc', lambda ops: dict(
        dq=i32(4, N, N), placed=i32(N), st=_puzzle_state(), changed=i32(N))),
    'puzzle_best_slot': ('puzzle_best_slot', 'vited_puzzle_best_slot', lambda ops: dict(
        mutual=z(4, N, N), placed=i32(N), slot_piece=i32(3), slot_side=i32(3), out=i64(1))),
    'cls_metrics_update': ('cls_metrics_update', 'vited_cls_metrics_update', lambda ops: dict(
        logits=z(R, 4), targets=z(R, 4), meters=z(10, dtype=torch.float64), last=z(5, dtype=torch.float64), bad=i32(1))),
    'mine_pairs_out': ('mine_pairs_out', 'vited_mine_pairs', lambda ops: dict(
        targets=i64(N), keys=z(N * N), neg_per_pos=2.0, ordered_negatives=False, groups=i64(6, 2), labels=z(6, 1), weights=z(6, 1),
        seg_index=i64(6), seg_order=i64(6), seg_offsets=i64(N + 1), counts=i32(5))),
}

# (case, argument, fault) -> why that mutation is no fault of the argument.  Everything else the generator makes must be refused.
SIZES = 'it defines the sizes the other arguments are checked against, and nothing is passed beside it that a shorter one contradicts'
COPIED = 'the wrapper copies it dense itself'
NOT_A_FAULT = {
    **{(c, 'src', f): r for c in ('cast', 'scale_rows_cast') for f, r in (('short', SIZES),)},
    ('cast', 'src', 'strided'): COPIED,
    ('patchify', 'img', 'dtype'): 'any other dtype is cast to fp32', ('patchify_u8', 'img', 'dtype'): 'any other dtype is cast to fp32',
    **{(c, 'img', f): r for c in ('patchify', 'patchify_u8') for f, r in (('short', 'S x (S - 1) is refused, a shorter batch is another batch'),
                                                                          ('strided', COPIED))},
    **{(c, 'batch_index', 'short'): 'its length is the batch' for c in ('patchify', 'patchify_u8')},
    ('crop_pairs_u8', 'regions', 'strided'): COPIED,
    ('slice_rows_cast', 'x', 'short'): SIZES, ('sum_rows', 'x', 'short'): SIZES, ('write_cls_row', 'x', 'short'): SIZES,
    **{(c, 'store', 'short'): 'its size is not passed: the offsets into it are device data (the caller guarantees them, see the docstring)'
       for c in ('div2k_regions_u8', 'hisfrag_windows_u8', 'michigan_windows_u8')},
    ('retrieval_metrics_rows', 'offsets', 'short'): 'its length is the class count',
    **{('group_retrieval_metrics_rows', f'{c}[1]', 'short'): 'as long as its offsets say, which is device data' for c in ('pos_csr', 'neg_csr')},
    ('layernorm_bwd_scaled', 'x', 'short'): SIZES,
    ('pair_scores_add', 'pairs', 'strided'): COPIED, ('pair_scores_add', 'scores', 'strided'): COPIED,
    ('cls_metrics_update', 'targets', 'dtype'): 'any real dtype is cast to fp32',
    ('puzzle_compat_init', 'dq', 'short'): 'dq is [4, n, n]: cut along n it is refused, there is no other argument',
    **{('linear_bwd_weight_batched', f'items[0][{i}]', 'dtype'): 'a set the batched kernel does not cover returns False: nothing is launched'
       for i in (0, 1)},
}

# case -> the arguments whose row-strided view is valid: the entry is handed their row (or batch and token) stride, or the wrapper
# copies them dense.  For every other argument of rank 2 and up the row-strided mutant must be refused.
QKV = ('q', 'k', 'v')
ROW_STRIDE = {
    'cast': ('src',), 'scale_rows_cast': ('src',), 'patchify': ('img',), 'patchify_u8': ('img',), 'crop_pairs_u8': ('regions',),
    'sum_rows': ('x',), 'layernorm_fwd': ('x',), 'layernorm_bwd': ('dy', 'x', 'dx_in', 'dx_out', 'dx_lp'), 'layernorm_bwd_scaled': ('dy', 'x'),
    'qk_norm_fwd': ('q', 'k', 'out[0]', 'out[1]'), 'qk_norm_bwd': ('dq', 'q', 'dk', 'k'),
    **{c: ('a', 'b', 'out') for c in ('gemm_store', 'gemm_gelu', 'gemm_mul', 'gemm_residual', 'gemm_remap', 'gemm_scaled')},
    'linear_bwd_weight': ('dy', 'x'), 'linear_bwd_weight_batched': ('items[0][0]', 'items[0][1]'),
    'linear_residual_layernorm_fwd': ('a', 'w', 'residual', 'out'), 'linear_residual_layernorm_fwd_scaled': ('a', 'w', 'residual'),
    'linear_layernorm_bwd': ('dy', 'wt', 'x', 'dx_in', 'dx_out'), 'linear_layernorm_bwd_scaled': ('dy', 'wt', 'x'),
    'linear_layernorm_bwd_segmented': ('dy', 'wt', 'x'), 'mlp_fwd': ('x', 'out[0]'), 'attention_fwd': QKV,
    'attention_bwd': QKV + ('dq', 'dk', 'dv'), 'attention_bwd_indexed': QKV + ('dq', 'dk', 'dv'), 'attention_cam': QKV + ('do', 'out'),
    'attention_cam_prob': ('q', 'k'), 'retrieval_metrics_rows': ('matrix',), 'group_retrieval_metrics_rows': ('matrix',),
    'pair_scores_add': ('pairs',), 'cls_metrics_update': ('logits', 'targets'),
}


def _leaves(value, path):
    """(path, tensor) of every tensor in a keyword argument: itself, or inside tuples / lists / dicts / named tuples, two levels deep."""
    if torch.is_tensor(value):
        yield path, value
    elif isinstance(value, dict):
        for key, v in value.items():
            yield from _leaves(v, path + (key,))
    elif isinstance(value, (tuple, list)):
        for i, v in enumerate(value):
            yield from _leaves(v, path + (i,))


def _replace(value, path, new):
    if not path:
        return new
    if isinstance(value, dict):
        return {k: _replace(v, path[1:], new) if k == path[0] else v for k, v in value.items()}
    items = [_replace(v, path[1:], new) if i == path[0] else v for i, v in enumerate(value)]
    return type(value)(*items) if hasattr(value, '_fields') else type(value)(items)


def _argument(kwargs, path):
    """The tensor at ``path`` by name: the keyword, then the accessors into it.  A refusal names it up to the first accessor."""
    name, value = path[0], kwargs[path[0]]
    if len(path) > 1:
        name += f'.{value._fields[path[1]]}' if hasattr(value, '_fields') else f'[{path[1]!r}]'
    return name + ''.join(f'[{p!r}]' for p in path[2:]), name


def _mutants(t):
    """The one-fault versions of a valid tensor.  A dtype no entry takes in that place: int16 for a float, float64 for an integer.
    One element short along the last dim, still dense.  The same values behind a stride of two (no fault for a single element).
    For rank 2 and up, the same values with dense rows one element apart: a fault wherever the entry takes no row stride."""
    yield 'dtype', t.to(torch.int16 if t.dtype.is_floating_point else torch.float64)
    yield 'short', t[..., :-1].contiguous()
    if t.numel() > 1:
        wide = torch.zeros(*t.shape, 2, dtype=t.dtype)
        wide[..., 0] = t
        yield 'strided', wide[..., 0]
    if t.dim() >= 2 and t.numel() > t.shape[-1]:
        wide = torch.zeros(*t.shape[:-1], t.shape[-1] + 1, dtype=t.dtype)
        wide[..., :-1] = t
        yield 'row-strided', wide[..., :-1]


def _run(ops, case, kwargs):
    op = CASES[case][0]
    if op == 'WeightShadowPlan':
        return ops.WeightShadowPlan(**kwargs).run()
    return getattr(ops, op)(**kwargs)


def test_every_entry_point_is_reached_by_a_valid_call(ops):
    for case, (_, entry, build) in CASES.items():
        del ops.calls[:]
        _run(ops, case, build(ops))
        assert [name for name, _ in ops.calls] == [entry], case
    in_source = set(re.findall(r"_lib\.call\('(vited_\w+)'", open(OPS_PY).read()))
    assert len(in_source) == 50 and {entry for _, entry, _ in CASES.values()} == in_source


@pytest.mark.parametrize('case', sorted(CASES))
def test_one_fault_is_refused_before_the_launch(ops, case):
    """The refusal names the op and the mutated argument.  A shortened operand may instead be named by the argument it no longer
    agrees with: of two extents that differ, the check cannot know which one is wrong."""
    op, _, build = CASES[case]
    op = op.removesuffix('_out')             # mine_pairs_out refuses in the name of mine_pairs
    valid = build(ops)
    tensors = [key for key in valid if any(True for _ in _leaves(valid[key], (key,)))]
    tried, wrong = 0, []
    for key in tensors:
        for path, t in _leaves(valid[key], (key,)):
            for fault, bad in _mutants(t):
                full, name = _argument(valid, path)
                if (case, full, fault) in NOT_A_FAULT or (fault == 'row-strided' and full in ROW_STRIDE.get(case, ())):
                    continue
                tried += 1
                try:
                    _run(ops, case, dict(valid, **{key: _replace(valid[key], path[1:], bad)}))
                    wrong.append((full, fault, 'not refused'))
                except (ValueError, TypeError) as err:
                    named = '|'.join(re.escape(n) for n in ([name] if fault != 'short' else tensors))
                    if not re.match(rf'{op}: ({named})(?!\w)', str(err)):
                        wrong.append((full, fault, str(err)))
                if ops.calls:
                    wrong.append((full, fault, f'launched {ops.calls[0][0]}'))
                    del ops.calls[:]
    assert not wrong, (case, wrong)
    assert tried or any(key[0] == case for key in NOT_A_FAULT)


def test_the_calls_that_used_to_reach_the_library_are_refused(ops):
    a = _attention_bwd()
    refused = [
        ('layernorm_fwd', 'gamma', lambda: ops.layernorm_fwd(z(8, 384), torch.ones(10), z(384), 1e-6, torch.bfloat16)),
        ('write_cls_row', 'cls', lambda: ops.write_cls_row(z(2, 5, 384), bf(3), z(1))),
        ('write_cls_row', 'pos', lambda: ops.write_cls_row(z(2, 5, 384), z(384), z(1))),
        ('gemm', 'out', lambda: ops.gemm(bf(8, 64), bf(16, 64), out=z(4, 16))),
        ('attention_bwd', 'lse', lambda: ops.attention_bwd(**dict(a, lse=z(1)))),
        ('attention_bwd', 'dq', lambda: ops.attention_bwd(**dict(a, dq=bf(B, NQ, D), dk=bf(B, NK, D), dv=bf(B, NK, D)))),
        ('attention_bwd', 'q', lambda: ops.attention_bwd(**dict(a, heads=3))),
        ('attention_bwd', 'dq', lambda: ops.attention_bwd(**dict(a, dq=z(1, NQ, D).expand(B, NQ, D)))),      # items that overlap
        ('gemm', 'residual', lambda: ops.gemm(bf(8, 64), bf(16, 64), epilogue=ops.EPI_RESIDUAL, residual=z(2, 7, 16))),
        ('hisfrag_blur_u8', 'out', lambda: (lambda x: ops.hisfrag_blur_u8(x, i32(N), z(N, 2), out=x))(u8(N, 3, S, S))),
        ('layernorm_bwd_finish', r'entries\[0\]\[2\]', lambda: ops.layernorm_bwd_finish([(z(512), 4, bf(64), z(3), True)])),
        ('layernorm_bwd_finish', r'entries\[0\]\[3\]', lambda: ops.layernorm_bwd_finish([(z(512), 4, z(64), z(3), True)])),
        ('layernorm_bwd_finish', r'entries\[0\]\[0\]', lambda: ops.layernorm_bwd_finish([(z(511), 4, z(64), z(64), True)])),
        ('layernorm_bwd_finish', r'entries\[1\]\[2\]',
         lambda: ops.layernorm_bwd_finish([(z(512), 4, z(64), z(64), True), (z(512), 4, z(32), z(32), True)])),
        ('slice_rows_cast', 'x', lambda: ops.slice_rows_cast(z(2, 5, 64), 3, 4, torch.bfloat16)),
        ('patchify', 'img', lambda: ops.patchify(z(2, 3, 12, 12), 8, torch.bfloat16)),
    ]
    for op, name, call in refused:
        with pytest.raises(ValueError, match=rf'^{op}: {name}(?!\w)'):
            call()
        assert not ops.calls, (op, name)
    ops.gemm(bf(8, 64), bf(16, 64), epilogue=ops.EPI_RESIDUAL, residual=z(1, 8, 16))               # leading unit dims are the same rows
    assert [name for name, _ in ops.calls] == ['vited_gemm']
    del ops.calls[:]
    for call in (lambda: ops.gemm(z(8, 64, dtype=torch.float16), z(16, 64, dtype=torch.float16)), lambda: ops.sum_rows(i32(8, 64)),
                 lambda: ops.cast(z(8, dtype=torch.float64), torch.bfloat16), lambda: ops.cast(z(8), torch.int8)):
        with pytest.raises(TypeError):                  # an activation dtype the kernels do not take: TypeError, as ever
            call()
    assert not ops.calls


def test_the_checker_itself(ops):
    x = z(4, 6)
    check, Min = ops._check, ops._Min
    assert check('op', 'x', x, torch.float32, (4, None), x.device) is x
    assert check('op', 'x', x[:, :3], (torch.float32, torch.int32), (Min(2), 3), x.device, ops.DENSE_LAST) is not None
    assert check('op', 'x', x, None, Min(24), x.device) is x and check('op', 'x', None, None, None, x.device, optional=True) is None
    assert check('op', 'x', z(3, 2, 4, 5)[:, 0], torch.float32, (3, 4, 5), x.device, ops.DENSE_ITEMS) is not None
    for kw in (dict(dtype=torch.int32), dict(shape=(4, 5)), dict(shape=(4,)), dict(shape=25), dict(shape=(Min(5), 6)), dict(t=x.t(), shape=(6, 4)),
               dict(t=x.t(), shape=(6, 4), strides=ops.DENSE_LAST), dict(t=x[:, :3], shape=(4, 3), strides=ops.DENSE_LAST, ld=3), dict(t=None),
               dict(t=z(3, 4, 5, 2)[..., 0], shape=(3, 4, 5), strides=ops.DENSE_ITEMS), dict(dev=torch.device('meta')), dict(t=[1.0])):
        args = dict(dict(t=x, dtype=torch.float32, shape=(4, 6), dev=x.device, strides=ops.CONTIGUOUS), **kw)
        with pytest.raises(ValueError, match=r'^the_op: the_arg must be a .+ on .+, got '):
            check('the_op', 'the_arg', args.pop('t'), args.pop('dtype'), args.pop('shape'), args.pop('dev'), **args)
    with pytest.raises(ValueError, match='length 16'):
        check('op', 'labels', i32(15), torch.int32, (16,), x.device)
    with pytest.raises(ValueError, match='k does not match q'):
        check('op', 'k', x, torch.bfloat16, (4, 6), x.device, like='q')


def test_no_assert_statement_carries_a_check():
    for name in ('ops.py', 'functions.py', 'optim.py'):
        tree = ast.parse(open(os.path.join(ROOT, 'vit-ed_amd', name)).read())
        assert not [node.lineno for node in ast.walk(tree) if isinstance(node, ast.Assert)], name
