"""Position dropout (timm's ``pos_drop = nn.Dropout(pos_drop_rate)``) with an EXPLICIT mask: the value reference of
tests/test_posdrop.py (pinned there against tests/golden/pos_drop.npz, which the reference's own class wrote -
tools/make_posdrop_golden.py) and of tests/test_gpu_posdrop.py.

The reference applies it at the end of ``_pos_embed_no_cls`` (image 1: patches + position) and of timm's ``_pos_embed`` (image 2: cls
row + patches, + position), in front of ``patch_drop`` and the blocks:

    encoder:  x = (patch_embed(x1) + pos_embed[:, 1:]) * mask1 * scale      [B, n1, D]
    decoder:  x = prepare_x2(x2) * mask2 * scale                            [B, 1 + n1, D]

with mask a 0 / 1 tensor over every element and scale = 1 / (1 - p).  ``ForcedPosDrop`` takes the place of ``model.pos_drop`` with
the random draw replaced by queued masks.  The masks the tests use are ``ops.token_dropout_mask`` at fixed seeds - the rule of the
HIP kernel restated on the CPU - and the scale is the kernel's: the fp32 value of 1 / (1 - p).  Patch dropout selects AFTER the mask
(``patchdrop_cases.gather_kept``), stochastic depth and q/k-norm compose as in ``patchdrop_cases``.
"""
import torch
import torch.nn as nn

import droppath_cases as dc
import patchdrop_cases as pc
from oracle import vited_oracle as vo


class ForcedPosDrop(nn.Module):
    """Stands where ``model.pos_drop`` stands; every call consumes the next queued multiplier mask * scale (one forward of the
    reference's model calls it twice: image 1, then image 2)."""

    def __init__(self, *multipliers):
        super().__init__()
        self.queue = list(multipliers)
        self.seen = []                      # the shapes it was called with

    def forward(self, x):
        self.seen.append(tuple(x.shape))
        return x * self.queue.pop(0).to(x.dtype)


def multiplier(mask, scale, like):
    """mask * scale in ``like``'s dtype: what a stream is multiplied with."""
    return mask.to(like.dtype) * scale


def encoder_dropped(m, x1, mask1, scale, keep1=None, enc=None):
    """m.forward_first_part(x1) with mask1 bool [B, n1, D] behind the position embedding; ``keep1``: patch-dropout indices applied
    after it, ``enc``: stochastic-depth scales."""
    h = m.shape.num_heads
    self_attn, _ = pc._attn_fns(m)
    x = m._patch_tokens(x1) + m.pos_embed[:, 1:]
    x = x * multiplier(mask1, scale, x)
    if keep1 is not None:
        x = pc.gather_kept(x, keep1)
    for i, blk in enumerate(m.blocks):
        x = x + pc._scale(enc, i, 0, x) * self_attn(blk.attn, vo._ln(blk.norm1, x), h)
        x = x + pc._scale(enc, i, 1, x) * vo._mlp(blk.mlp, vo._ln(blk.norm2, x))
    return x


def decoder_dropped(m, feats, x2, mask2, scale, keep2=None, dec=None):
    """m.forward_head(m.forward_second_part(feats, x2)) with mask2 bool [B, 1 + n1, D] behind ``prepare_x2``."""
    h = m.shape.num_heads
    self_attn, cross_attn = pc._attn_fns(m)
    x = m.prepare_x2(x2)
    x = x * multiplier(mask2, scale, x)
    if keep2 is not None:
        x = pc.gather_kept(x, keep2)
    for i, blk in enumerate(m.cross_blocks):
        x = x + pc._scale(dec, i, 0, x) * self_attn(blk.attn, vo._ln(blk.norm1, x), h)
        x = x + pc._scale(dec, i, 1, x) * cross_attn(blk.cross_attn, vo._ln(blk.norm_cross, x), vo._ln(blk.norm_context, feats), h)
        x = x + pc._scale(dec, i, 2, x) * vo._mlp(blk.mlp, vo._ln(blk.norm2, x))
    return m.forward_head(vo._ln(m.norm, x))


def forward_dropped(m, x, mask1, mask2, scale, keep1=None, keep2=None, enc=None, dec=None):
    """The one-shot forward on stacked pairs x [B, 2, C, S, S]."""
    x1, x2 = torch.unbind(x, 1)
    return decoder_dropped(m, encoder_dropped(m, x1, mask1, scale, keep1, enc), x2, mask2, scale, keep2, dec)


def masks_of(ops, seeds, rate, batch_x1, batch_x2, s):
    """(mask1 bool [batch_x1, n1, D], mask2 bool [batch_x2, 1 + n1, D], scale) of the rule at the seeds (seed of stream 0, of stream 1)."""
    _, scale = ops.dropout_threshold(rate)
    return (ops.token_dropout_mask(seeds[0], rate, batch_x1, s.n1, s.embed_dim, 0),
            ops.token_dropout_mask(seeds[1], rate, batch_x2, s.n2, s.embed_dim, 1), scale)


loss_and_grads = dc.loss_and_grads

# the geometries and inputs of tests/golden/pos_drop.npz: 64-pixel images, patch 8 (64 / 65 tokens of 384 channels), 1 + 1 and 2 + 3 blocks
GOLDEN_SHAPES = {'1_1': vo.ViTEDShape(depth=1, c_depth=1), '2_3': vo.ViTEDShape(depth=2, c_depth=3)}
GOLDEN_RATE, GOLDEN_BATCH = 0.25, 2
GOLDEN_SEEDS = {'1_1': (1234567890123, -77), '2_3': (-(2 ** 63) + 5, 2 ** 62 + 11)}


def golden_inputs(name):
    """(x, y) of geometry ``name``: closed form, as every fixture's."""
    s = GOLDEN_SHAPES[name]
    x = vo.closed_form_pairs(GOLDEN_BATCH, s, salt=1000 + len(name) + s.c_depth)
    y = (vo.closed_form((GOLDEN_BATCH, s.num_classes), 77, 1.0) > 0.2).float()
    return x, y
