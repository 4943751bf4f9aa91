"""Patch dropout (timm 0.9 PatchDropout as the reference constructs it: prob, num_prefix_tokens=1, ordered=False) with EXPLICIT keep
indices: the value reference of tests/test_patchdrop.py (pinned there against tests/golden/patch_drop.npz, which the reference's own
classes wrote - tools/make_patchdrop_golden.py) and of tests/test_gpu_patchdrop.py.

What timm's module does in training mode for p > 0, restated (timm is not a dependency of the tests):

    prefix, x = x[:, :1], x[:, 1:]                      # num_prefix_tokens = 1
    L = x.shape[1];  K = max(1, int(L * (1. - p)))
    keep = argsort(randn(B, L), dim=-1)[:, :K]          # ordered=False: not re-sorted
    x = cat(prefix, x.gather(1, keep over the channels), dim=1)

The reference calls it after the position embedding, in ``forward_first_part`` (vision_transformer.py:385) and in ``prepare_x2``
(:393).  The image-1 stream has no cls token, so there the prefix slot falls on PATCH 0, which is always kept, and L = n1 - 1; on
the image-2 stream the prefix is the cls token and L = n1.  ``ForcedPatchDrop`` takes the place of ``model.patch_drop`` with the
random draw replaced by queued index sets; ``forward_kept`` is the same thing composed from the oracle's pieces.
"""
import math

import torch
import torch.nn as nn

import droppath_cases as dc
import qknorm_cases as qc
from oracle import vited_oracle as vo


def keep_count(tokens, rate):
    """K of timm's PatchDropout for ``tokens`` tokens behind the prefix, in Python float arithmetic exactly as timm writes it."""
    return max(1, int(tokens * (1. - rate)))


def gather_kept(x, keep):
    """x [B, 1 + L, D], keep int64 [B, K] -> [B, 1 + K, D]: the prefix token, then the tokens 1 + keep[b, :] in keep order."""
    prefix, rest = x[:, :1], x[:, 1:]
    if keep.dim() != 2 or keep.shape[0] != x.shape[0] or int(keep.min()) < 0 or int(keep.max()) >= rest.shape[1]:
        raise ValueError(f'keep {tuple(keep.shape)} does not index {tuple(rest.shape)}')
    return torch.cat((prefix, rest.gather(1, keep.to(torch.int64).unsqueeze(-1).expand(-1, -1, rest.shape[-1]))), dim=1)


class ForcedPatchDrop(nn.Module):
    """Stands where ``model.patch_drop`` stands; every call consumes the next queued index set (one forward of the reference's model
    calls it twice: image 1, then image 2)."""

    def __init__(self, *keeps):
        super().__init__()
        self.queue = list(keeps)
        self.seen = []                      # the token counts it was called with

    def forward(self, x):
        self.seen.append(x.shape[1])
        return gather_kept(x, self.queue.pop(0))


def _attn_fns(m):
    """(self-attention, cross-attention) of the oracle's pieces for this module tree: with q/k-norm where it has the norms."""
    qk = bool(len(m.blocks)) and hasattr(m.blocks[0].attn, 'q_norm') or bool(len(m.cross_blocks)) and hasattr(m.cross_blocks[0].attn, 'q_norm')
    return (qc.self_attention, qc.cross_attention) if qk else (vo.self_attention, vo.cross_attention)


def _scale(s, i, j, like):
    return 1.0 if s is None else s[i, j].to(like.dtype).view(-1, 1, 1)


def encoder_kept(m, x1, keep1, enc=None):
    """m.forward_first_part(x1) on patch 0 and the patches 1 + keep1 (``enc``: stochastic-depth scales as in droppath_cases)."""
    h = m.shape.num_heads
    self_attn, _ = _attn_fns(m)
    x = gather_kept(m._patch_tokens(x1) + m.pos_embed[:, 1:], keep1)
    for i, blk in enumerate(m.blocks):
        x = x + _scale(enc, i, 0, x) * self_attn(blk.attn, vo._ln(blk.norm1, x), h)
        x = x + _scale(enc, i, 1, x) * vo._mlp(blk.mlp, vo._ln(blk.norm2, x))
    return x


def decoder_kept(m, feats, x2, keep2, dec=None):
    """m.forward_head(m.forward_second_part(feats, x2)) on the cls token and the patches keep2."""
    h = m.shape.num_heads
    self_attn, cross_attn = _attn_fns(m)
    x = gather_kept(m.prepare_x2(x2), keep2)
    for i, blk in enumerate(m.cross_blocks):
        x = x + _scale(dec, i, 0, x) * self_attn(blk.attn, vo._ln(blk.norm1, x), h)
        x = x + _scale(dec, i, 1, x) * cross_attn(blk.cross_attn, vo._ln(blk.norm_cross, x), vo._ln(blk.norm_context, feats), h)
        x = x + _scale(dec, i, 2, x) * vo._mlp(blk.mlp, vo._ln(blk.norm2, x))
    return m.forward_head(vo._ln(m.norm, x))


def forward_kept(m, x, keep1, keep2, enc=None, dec=None):
    """The one-shot forward on stacked pairs x [B, 2, C, S, S]."""
    x1, x2 = torch.unbind(x, 1)
    return decoder_kept(m, encoder_kept(m, x1, keep1, enc), x2, keep2, dec)


def closed_form_keep(batch, tokens, k, salt):
    """int64 [batch, k]: per sample the first k entries of a permutation of range(tokens), in closed form and NOT ascending:
    i -> (a i + c_b) mod tokens with a multiplier coprime to tokens and an offset that differs per sample."""
    a = next(a for a in range(max(tokens // 2, 1) | 1, 2 * tokens + 3, 2) if math.gcd(a, tokens) == 1)
    i = torch.arange(k, dtype=torch.int64).view(1, -1)
    b = torch.arange(batch, dtype=torch.int64).view(-1, 1)
    return (a * i + (7 * b + 3 + salt)) % tokens


loss_and_grads = dc.loss_and_grads

# the geometry and inputs of tests/golden/patch_drop.npz: 16-pixel images, patch 8 (4 patches: 2 / 3 tokens at rate 0.5), B = 3
GOLDEN_SHAPE = vo.ViTEDShape(img_size=16, patch_size=8, num_classes=4, embed_dim=64, num_heads=2, depth=2, c_depth=2)
GOLDEN_RATE, GOLDEN_BATCH = 0.5, 3


def golden_inputs():
    s = GOLDEN_SHAPE
    x = vo.closed_form_pairs(GOLDEN_BATCH, s)
    y = (vo.closed_form((GOLDEN_BATCH, s.num_classes), 77, 1.0) > 0.2).float()
    keep1 = closed_form_keep(GOLDEN_BATCH, s.n1 - 1, keep_count(s.n1 - 1, GOLDEN_RATE), salt=1)
    keep2 = closed_form_keep(GOLDEN_BATCH, s.n1, keep_count(s.n1, GOLDEN_RATE), salt=2)
    return x, y, keep1, keep2
