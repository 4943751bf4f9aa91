"""The ViT-ED forward with q/k-norm (``qk_norm=True``) restated in plain torch from the oracle's functional pieces: the value
reference of tests/test_qknorm.py (pinned there against tests/golden/qk_norm.npz, which the reference's own classes wrote -
tools/make_qknorm_golden.py) and of tests/test_gpu_qknorm.py.  Runs in any dtype, fp64 included.

    self-attention:   q, k, v = qkv(x) split per head;  q, k = q_norm(q), k_norm(k);  softmax(q k^T / sqrt(hd)) v
    cross-attention:  q = q(x), k, v = kv(context) per head;  q, k = q_norm(q), k_norm(k);  ...

with q_norm / k_norm = LayerNorm(head_dim, eps=1e-6) over the last dim of [B, heads, N, head_dim], their weight and bias shared by
all heads (models/vision_transformer.py:35-36,60 and 153-154,180 of the reference).  The module tree carries the reference's
state_dict names, ``*.attn.q_norm.weight`` and so on, in the reference's order.
"""
import zlib
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import vited_oracle as vo

LN_EPS = vo.LN_EPS


def _head_norm(norm, t):
    return F.layer_norm(t, (t.shape[-1],), norm.weight, norm.bias, LN_EPS)


def _sdpa(q, k, v, store=None):
    """vo._sdpa; ``store`` (a dict) receives the softmax map under 'attn' and keeps it in the graph, so that its gradient can be
    asked for (the reference's save_attn / save_attn_gradients hooks)."""
    p = torch.softmax((q * q.shape[-1] ** -0.5) @ k.transpose(-2, -1), dim=-1)
    if store is not None:
        p.retain_grad()
        store['attn'] = p
    o = p @ v
    b, h, n, hd = o.shape
    return o.transpose(1, 2).reshape(b, n, h * hd)


def self_attention(m, x, num_heads, store=None):
    q, k, v = F.linear(x, m.qkv.weight, m.qkv.bias).chunk(3, dim=-1)
    q, k = _head_norm(m.q_norm, vo._heads(q, num_heads)), _head_norm(m.k_norm, vo._heads(k, num_heads))
    return F.linear(_sdpa(q, k, vo._heads(v, num_heads), store), m.proj.weight, m.proj.bias)


def cross_attention(m, x, context, num_heads, store=None):
    q = F.linear(x, m.q.weight, m.q.bias)
    k, v = F.linear(context, m.kv.weight, m.kv.bias).chunk(2, dim=-1)
    q, k = _head_norm(m.q_norm, vo._heads(q, num_heads)), _head_norm(m.k_norm, vo._heads(k, num_heads))
    return F.linear(_sdpa(q, k, vo._heads(v, num_heads), store), m.proj.weight, m.proj.bias)


def _add_norms(bag, head_dim, before='proj'):
    """q_norm / k_norm on an attention bag of the oracle, registered where the reference registers them (before ``proj``)."""
    mods = OrderedDict()
    for name, mod in bag._modules.items():
        if name == before:
            mods['q_norm'] = nn.LayerNorm(head_dim, eps=LN_EPS)
            mods['k_norm'] = nn.LayerNorm(head_dim, eps=LN_EPS)
        mods[name] = mod
    bag._modules = mods


class QKNormViTED(vo.OracleViTED):
    """OracleViTED with q_norm / k_norm in every attention.  ``maps``: None, or a dict that receives the attention map of every
    attention under the keys the HIP model uses, ('blocks' | 'cross_blocks', index, 'attn' | 'cross_attn') -> {'attn': map}."""

    def __init__(self, shape):
        super().__init__(shape)
        for blk in self.blocks:
            _add_norms(blk.attn, shape.head_dim)
        for blk in self.cross_blocks:
            _add_norms(blk.attn, shape.head_dim)
            _add_norms(blk.cross_attn, shape.head_dim)
        self.maps = None

    def _store(self, *key):
        return None if self.maps is None else self.maps.setdefault(key, {})

    def forward_first_part(self, x1):
        h = self.shape.num_heads
        x = self._patch_tokens(x1) + self.pos_embed[:, 1:]
        for i, blk in enumerate(self.blocks):
            x = x + self_attention(blk.attn, vo._ln(blk.norm1, x), h, self._store('blocks', i, 'attn'))
            x = x + vo._mlp(blk.mlp, vo._ln(blk.norm2, x))
        return x

    def cross_part(self, x1, x2):
        h = self.shape.num_heads
        for i, blk in enumerate(self.cross_blocks):
            x2 = x2 + self_attention(blk.attn, vo._ln(blk.norm1, x2), h, self._store('cross_blocks', i, 'attn'))
            x2 = x2 + cross_attention(blk.cross_attn, vo._ln(blk.norm_cross, x2), vo._ln(blk.norm_context, x1), h,
                                      self._store('cross_blocks', i, 'cross_attn'))
            x2 = x2 + vo._mlp(blk.mlp, vo._ln(blk.norm2, x2))
        return vo._ln(self.norm, x2)


def is_qk_norm_key(name):
    parts = name.split('.')
    return len(parts) >= 2 and parts[-2] in ('q_norm', 'k_norm')


def fill_closed_form_(module):
    """vo.fill_closed_form_ plus the closed-form fill of the q/k-norm parameters of any module tree with the reference's names: the
    weights around 1 (1 + 0.2 f(i)), the biases around 0 (0.05 f(i)), both varying with the index - never all 1 / all 0."""
    vo.fill_closed_form_(module)
    with torch.no_grad():
        for name, p in module.state_dict().items():
            if is_qk_norm_key(name):
                salt = zlib.crc32(name.encode()) % 9973
                p.copy_(vo.closed_form(p.shape, salt, 0.2, 1.0) if name.endswith('weight') else vo.closed_form(p.shape, salt, 0.05))
    return module


def randomize_norms_(module, generator):
    """Random-init models keep q_norm / k_norm at weight 1, bias 0, which hides a swapped or dropped parameter: perturb them."""
    with torch.no_grad():
        for name, p in module.state_dict().items():
            if is_qk_norm_key(name):
                noise = torch.randn(p.shape, generator=generator)
                p.copy_(1.0 + 0.2 * noise if name.endswith('weight') else 0.1 * noise)
    return module


def loss_and_grads(m, logits, y):
    """BCE-with-logits loss of ``logits`` and the gradient of every parameter of ``m`` by name."""
    m.zero_grad(set_to_none=True)
    loss = F.binary_cross_entropy_with_logits(logits, y)
    loss.backward()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


# the geometries and inputs of tests/golden/qk_norm.npz: head_dim 32 and head_dim 64, 4 / 5 tokens, 2 + 2 blocks, B = 3
GOLDEN_SHAPES = (vo.ViTEDShape(img_size=16, patch_size=8, num_classes=4, embed_dim=64, num_heads=2, depth=2, c_depth=2),
                 vo.ViTEDShape(img_size=16, patch_size=8, num_classes=4, embed_dim=128, num_heads=2, depth=2, c_depth=2))
GOLDEN_BATCH = 3


def golden_inputs(s):
    x = vo.closed_form_pairs(GOLDEN_BATCH, s)
    y = (vo.closed_form((GOLDEN_BATCH, s.num_classes), 77, 1.0) > 0.2).float()
    return x, y
