"""Attention relevancy maps (scripts/visualise_attentions.py: Generator.generate_ours / generate_raw_attn / generate_attn_gradcam):
relevancy propagation over head-averaged maps, raw attention and attention Grad-CAM for a batch of pairs."""
from __future__ import annotations

import torch

from .. import ops


def _handle_residual(r: torch.Tensor) -> torch.Tensor:
    """Eq. 8 + 9 of Chefer et al. (handle_residual of the script), batched: the part of a self-relevancy beyond the identity,
    rows normalised to sum 1, plus the identity.  A row that is still the identity gives 0 / 0 = NaN, which rule 10 turns into 0.
    (The script also asserts a non-negative diagonal; with the non-negative maps of rule 5 it cannot fail, and the check would
    make the device wait for the host.)"""
    eye = torch.eye(r.shape[-1], dtype=r.dtype, device=r.device)
    rest = r - eye
    return rest / rest.sum(dim=-1, keepdim=True) + eye


def relevancy_from_cams(enc_cams, dec_self_cams, dec_cross_cams, normalize_self_attention: bool = True, apply_self_in_rule_10: bool = True):
    """Relevancy propagation of ``Generator.generate_ours`` for a batch of pairs, from the head-averaged maps of rule 5
    (``get_attn_cam()`` of every attention): ``enc_cams`` depth x [B, N1, N1], ``dec_self_cams`` c_depth x [B, N2, N2],
    ``dec_cross_cams`` c_depth x [B, N2, N1].  Returns R_qi [B, N2, N1] in the maps' dtype: the relevancy of every image-1 token
    for every image-2 token (row 0: the cls token).  Order of the updates as in the script: R_ii += cam R_ii over the encoder
    blocks; then per decoder block rules 6 + 7 (both additions from the OLD R_qq and R_qi) and rule 10,
    R_qi += norm(R_qq)^T (cam norm(R_ii)) with NaN -> 0.  Plain batched torch: works on CPU tensors (fp64 in the tests) too."""
    enc_cams, dec_self_cams, dec_cross_cams = list(enc_cams), list(dec_self_cams), list(dec_cross_cams)
    if not dec_cross_cams or len(dec_self_cams) != len(dec_cross_cams):
        raise ValueError(f'relevancy_from_cams: need one self and one cross map per decoder block, got {len(dec_self_cams)} and '
                         f'{len(dec_cross_cams)}')
    ref = dec_cross_cams[0]
    if ref.dim() != 3:
        raise ValueError(f'relevancy_from_cams: maps are [B, Nq, Nk], got {tuple(ref.shape)}')
    b, n2, n1 = ref.shape
    for name, cams, shape in (('encoder', enc_cams, (b, n1, n1)), ('decoder self', dec_self_cams, (b, n2, n2)), ('decoder cross', dec_cross_cams, (b, n2, n1))):
        for cam in cams:
            if tuple(cam.shape) != shape or cam.dtype != ref.dtype or cam.device != ref.device:
                raise ValueError(f'relevancy_from_cams: a {name} map is {tuple(cam.shape)} {cam.dtype}, expected {shape} {ref.dtype}')
    kw = dict(dtype=ref.dtype, device=ref.device)
    r_ii = torch.eye(n1, **kw).expand(b, n1, n1).clone()
    r_qq = torch.eye(n2, **kw).expand(b, n2, n2).clone()
    r_qi = torch.zeros((b, n2, n1), **kw)
    for cam in enc_cams:
        r_ii = r_ii + torch.bmm(cam, r_ii)
    for cam_qq, cam_qi in zip(dec_self_cams, dec_cross_cams):
        add_qq, add_qi = torch.bmm(cam_qq, r_qq), torch.bmm(cam_qq, r_qi)
        r_qq, r_qi = r_qq + add_qq, r_qi + add_qi
        if apply_self_in_rule_10:
            nqq, nii = (_handle_residual(r_qq), _handle_residual(r_ii)) if normalize_self_attention else (r_qq, r_ii)
            add = torch.bmm(nqq.transpose(1, 2), torch.bmm(cam_qi, nii))
        else:
            add = cam_qi
        r_qi = r_qi + torch.where(torch.isnan(add), torch.zeros_like(add), add)
    return r_qi


_RELEVANCY_METHODS = ('relevance', 'raw', 'gradcam')


def _relevancy_of_store(net, method, include_cls, normalize_self_attention, apply_self_in_rule_10, propagate_dtype):
    store = net._attn_store
    if method == 'relevance':
        cams = lambda kind, n, which: [store[(kind, i, which)]['cam'].to(propagate_dtype) for i in range(n)]
        r_qi = relevancy_from_cams(cams('blocks', net.depth, 'attn'), cams('cross_blocks', net.c_depth, 'attn'),
                                   cams('cross_blocks', net.c_depth, 'cross_attn'), normalize_self_attention, apply_self_in_rule_10)
        return (r_qi if include_cls else r_qi[:, 1:, :]).to(torch.float32)
    # the last cross-attention, cls query (row 0), weighted over the heads: sum_h w[b, h] P_h[0, :]
    q, k, v, do, lse = store[('cross_blocks', net.c_depth - 1, 'cross_attn')]['cam_operands']
    heads, hd = net.num_heads, net.embed_dim // net.num_heads
    weight = None                                   # 'raw': the head mean of the attention
    if method == 'gradcam':
        # mean_ij dP_h = (sum_i dO_i) . (sum_j v_j) / (Nq Nk): the per-head weight without forming dP; / H: the mean over the heads
        b, nq, nk = q.shape[0], q.shape[1], k.shape[1]
        weight = (do.float().sum(1).view(b, heads, hd) * v.float().sum(1).view(b, heads, hd)).sum(-1) / float(nq * nk * heads)
        weight = weight.contiguous()
    cam = ops.attention_cam(q[:, 0:1], k, None, None, lse[:, :, 0:1].contiguous(), heads, hd ** -0.5, mode='prob', head_weight=weight)
    cam = cam[:, 0, :]
    return cam.clamp_(min=0) if method == 'gradcam' else cam


def pair_relevancy(model, images, target=None, amp: bool = True, method: str = 'relevance', include_cls: bool = False, chunk: int | None = None,
                   normalize_self_attention: bool = True, apply_self_in_rule_10: bool = True, propagate_dtype=torch.float64):
    """Which patches made the model decide: the three generators of scripts/visualise_attentions.py for a BATCH of pairs.

    ``images`` [B, 2, 3, S, S] (float, or uint8 normalised in the patch-embedding kernel).  One forward, one backward from a one-hot
    of ``target`` (an int, or int64 [B]; None: every sample's own arg-max logit, taken on the device), with ``model.keep_cam``
    on: every attention's backward also writes its head-averaged map mean_h max(P o dP, 0) [B, Nq, Nk] from one fused kernel
    (ops.attention_cam) - no per-head N x N map exists at any time, which is what makes a batch fit.
    Returns (relevancy, logits [B, C]):
      'relevance'  Generator.generate_ours: R_qi [B, N2 - 1, N1] (all N2 rows with ``include_cls``), relevancy_from_cams;
      'raw'        generate_raw_attn: head mean of the last cross-attention, cls query, [B, N1];
      'gradcam'    generate_attn_gradcam: max(mean_h mean(dP_h) P_h, 0) of the same row, [B, N1].
    The maps are fp32; the propagation over them runs in ``propagate_dtype`` and the result is returned as fp32.  fp64 by default:
    handle_residual subtracts the identity from 1 + (sum of maps), which in fp32 loses whatever of a map lies below 6e-8.
    ``chunk`` bounds the pairs in flight.  The model's keep_cam / keep_attn switches are restored, its attention store is left
    empty and no parameter gradient is touched: under keep_cam the weight-gradient kernels are not launched, the backward returns
    no parameter gradient to autograd, and the direct accumulation into p.grad / FlatGradients.flat is off for that backward."""
    net = getattr(model, 'module', model)
    if method not in _RELEVANCY_METHODS:
        raise ValueError(f'pair_relevancy: method must be one of {_RELEVANCY_METHODS}, got {method!r}')
    if images.dim() != 5 or images.shape[1] != 2:
        raise ValueError(f'pair_relevancy: expected stacked pairs [B, 2, C, S, S], got {tuple(images.shape)}')
    if not hasattr(net, 'keep_cam'):
        raise TypeError('pair_relevancy needs the HIP VisionTransformerCustom (model.keep_cam)')
    if not any(p.requires_grad for p in net.parameters()):
        raise ValueError('pair_relevancy: the maps are recorded by the backward, which only runs for a model with trainable parameters')
    b = images.shape[0]
    chunk = b if chunk is None else int(chunk)
    if chunk <= 0:
        raise ValueError(f'pair_relevancy: chunk must be positive, got {chunk}')
    dev = images.device
    if target is not None:
        target = torch.as_tensor(target, device=dev).to(torch.int64).reshape(-1)
        if target.numel() not in (1, b):
            raise ValueError(f'pair_relevancy: target must be one class or one per pair, got {target.numel()} for {b} pairs')
        target = target.expand(b)
    saved = (net.keep_cam, net.keep_attn)
    rel, out = [], []
    try:
        net.keep_cam, net.keep_attn = True, False
        for lo in range(0, b, chunk):
            net._attn_store.clear()
            with torch.enable_grad():
                with torch.autocast(dev.type, dtype=torch.bfloat16, enabled=amp):
                    logits = net(images[lo:lo + chunk])
                index = target[lo:lo + chunk] if target is not None else logits.detach().argmax(dim=-1)
                one_hot = torch.zeros_like(logits).scatter_(1, index.unsqueeze(1), 1.0)
                logits.backward(one_hot)
            rel.append(_relevancy_of_store(net, method, include_cls, normalize_self_attention, apply_self_in_rule_10, propagate_dtype))
            out.append(logits.detach())
    finally:
        net.keep_cam, net.keep_attn = saved
        net._attn_store.clear()
    return (rel[0], out[0]) if len(rel) == 1 else (torch.cat(rel), torch.cat(out))
