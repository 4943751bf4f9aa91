"""Stochastic depth (timm DropPath, scale_by_keep) with EXPLICIT scales, composed from the oracle's functional pieces: the value
reference of tests/test_droppath.py (pinned there against tests/golden/droppath.npz, which the reference's own classes wrote -
tools/make_droppath_golden.py) and of tests/test_gpu_droppath.py.

    encoder block i:  x = x + s[i, 0] * attn(norm1(x));   x = x + s[i, 1] * mlp(norm2(x))
    decoder block i:  x = x + s[i, 0] * attn(norm1(x));   x = x + s[i, 1] * cross(norm_cross(x), norm_context(ctx));
                      x = x + s[i, 2] * mlp(norm2(x))

with s[i, j] one value per sample of the call (0: the sample skips the branch, 1 / keep otherwise), models/vision_transformer.py:
125-126 and 269-271 of the reference.  Autograd gives the backward: the residual path unscaled, everything inside a branch s * dy.
"""
import torch

from oracle import vited_oracle as vo


def _per_sample(s, like):
    return s.to(like.dtype).view(-1, 1, 1)


def encoder_scaled(m, x1, enc):
    """m.forward_first_part(x1) with enc [depth, 2, B] scales."""
    h = m.shape.num_heads
    x = m._patch_tokens(x1) + m.pos_embed[:, 1:]
    for i, blk in enumerate(m.blocks):
        x = x + _per_sample(enc[i, 0], x) * vo.self_attention(blk.attn, vo._ln(blk.norm1, x), h)
        x = x + _per_sample(enc[i, 1], x) * vo._mlp(blk.mlp, vo._ln(blk.norm2, x))
    return x


def decoder_scaled(m, feats, x2, dec):
    """m.forward_head(m.forward_second_part(feats, x2)) with dec [c_depth, 3, B] scales."""
    h = m.shape.num_heads
    x = m.prepare_x2(x2)
    for i, blk in enumerate(m.cross_blocks):
        x = x + _per_sample(dec[i, 0], x) * vo.self_attention(blk.attn, vo._ln(blk.norm1, x), h)
        x = x + _per_sample(dec[i, 1], x) * vo.cross_attention(blk.cross_attn, vo._ln(blk.norm_cross, x), vo._ln(blk.norm_context, feats), h)
        x = x + _per_sample(dec[i, 2], x) * vo._mlp(blk.mlp, vo._ln(blk.norm2, x))
    return m.forward_head(vo._ln(m.norm, x))


def forward_scaled(m, x, enc, dec):
    """The one-shot forward on stacked pairs x [B, 2, C, S, S]: both halves see the B samples of the call."""
    x1, x2 = torch.unbind(x, 1)
    return decoder_scaled(m, encoder_scaled(m, x1, enc), x2, dec)


def keep_probs(rate, depth):
    """Keep probability per block under the reference's decay rule, as Python floats: 1 - fp32 linspace(0, rate, depth)[i]."""
    return [1.0 - torch.linspace(0, rate, depth)[i].item() for i in range(depth)]


def irregular_scales(rate, depth, branches, batch, salt):
    """Forced scales fp32 [depth, branches, batch]: kept (fp32(1) / fp32(keep)) and dropped (0) samples in an irregular, closed-form
    pattern that differs per branch; every row holds both kinds where batch >= 2.  Block 0 (p = 0) keeps everyone at scale 1."""
    keep = torch.tensor(keep_probs(rate, depth), dtype=torch.float32).view(-1, 1, 1)
    kept = vo.closed_form((depth, branches, batch), salt, 1.0) > -0.15
    kept[:, :, 0], kept[:, :, -1] = True, (batch < 2)              # never all kept, never all dropped
    kept[0] = True
    return kept.float() * (torch.ones((), dtype=torch.float32) / keep)


def loss_and_grads(m, logits, y):
    """BCE-with-logits loss of ``logits`` and the gradient of every parameter of ``m`` by name."""
    m.zero_grad(set_to_none=True)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, y)
    loss.backward()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


# the geometry and inputs of tests/golden/droppath.npz
GOLDEN_SHAPE = vo.ViTEDShape(depth=3, c_depth=3)          # 64-pixel images, patch 8
GOLDEN_RATE, GOLDEN_BATCH = 0.5, 4


def golden_inputs():
    s = GOLDEN_SHAPE
    x = vo.closed_form_pairs(GOLDEN_BATCH, s)
    y = (vo.closed_form((GOLDEN_BATCH, s.num_classes), 77, 1.0) > 0.2).float()
    enc = irregular_scales(GOLDEN_RATE, s.depth, 2, GOLDEN_BATCH, salt=31)
    dec = irregular_scales(GOLDEN_RATE, s.c_depth, 3, GOLDEN_BATCH, salt=47)
    return x, y, enc, dec
