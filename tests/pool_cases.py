"""The ViT-ED head under timm's ``global_pool`` / ``fc_norm`` options restated in plain torch on the oracle's pieces: the value
reference of tests/test_pool_head.py (pinned there against tests/golden/pool_head.npz, which the reference's own class wrote -
tools/make_pool_head_golden.py) and of tests/test_gpu_pool_head.py.  Runs in any dtype, fp64 included.

timm's rule is ``use_fc_norm = (global_pool == 'avg') if fc_norm is None else fc_norm``; with x2 the decoder's token stream, cls row
first, ``cross_part`` (vision_transformer.py:397-401 of the reference) and timm's ``forward_head`` give

    global_pool  fc_norm        logits                                              norm keys
    'token'      None / False   head(norm(x2)[:, 0])                                norm.*
    'avg'        None / True    head(fc_norm(x2[:, 1:].mean(1)))                    fc_norm.*   (norm is an Identity)
    'avg'        False          head(norm(x2)[:, 1:].mean(1))                       norm.*
    'token'      True           head(fc_norm(x2[:, 0]))                             fc_norm.*

``fc_norm`` sits where ``norm`` sits in the module tree (timm registers norm, then fc_norm, then the head; the one that is an Identity has
no parameters), so the state_dict order is the oracle's with the two keys renamed.  The encoder and the decoder blocks are the
oracle's, with the q/k-norm, stochastic-depth scales and patch-dropout keep indices of the sibling case modules where asked for.
"""
import zlib
from collections import OrderedDict

import torch
import torch.nn.functional as F

import patchdrop_cases as pc
import qknorm_cases as qc
from oracle import vited_oracle as vo

# (global_pool, fc_norm) of the three rows that differ from the default, under the names the fixture and the tests use
VARIANTS = OrderedDict((('avg', ('avg', None)), ('avg_nofc', ('avg', False)), ('token_fc', ('token', True))))


def use_fc_norm(global_pool, fc_norm):
    return (global_pool == 'avg') if fc_norm is None else bool(fc_norm)


def _pooled(base):
    class Pooled(base):
        """``base`` (vo.OracleViTED or qc.QKNormViTED) with the head options; every forward path ends in final_norm + forward_head."""

        def __init__(self, shape, global_pool='token', fc_norm=None):
            super().__init__(shape)
            if global_pool not in ('token', 'avg'):
                raise ValueError(global_pool)
            self.global_pool, self.use_fc_norm = global_pool, use_fc_norm(global_pool, fc_norm)
            if self.use_fc_norm:        # the LayerNorm keeps its place in the tree under the other name
                self._modules = OrderedDict(('fc_norm' if name == 'norm' else name, mod) for name, mod in self._modules.items())

        def final_norm(self, x):
            return x if self.use_fc_norm else vo._ln(self.norm, x)

        def forward_first_part(self, x1):
            return encoder(self, x1)

        def cross_part(self, x1, x2):
            return self.final_norm(decoder_blocks(self, x1, x2))

        def forward_head(self, x):
            x = x[:, 1:].mean(dim=1) if self.global_pool == 'avg' else x[:, 0]
            if self.use_fc_norm:
                x = vo._ln(self.fc_norm, x)
            return F.linear(x, self.head.weight, self.head.bias)

    Pooled.__name__ = Pooled.__qualname__ = 'Pooled' + base.__name__
    return Pooled


PoolViTED = _pooled(vo.OracleViTED)
PoolQKNormViTED = _pooled(qc.QKNormViTED)


def encoder(m, x1, keep1=None, enc=None):
    """forward_first_part; ``keep1``: patch-dropout indices (patchdrop_cases), ``enc``: stochastic-depth scales (droppath_cases)."""
    h = m.shape.num_heads
    self_attn, _ = pc._attn_fns(m)
    x = m._patch_tokens(x1) + m.pos_embed[:, 1:]
    if keep1 is not None:
        x = pc.gather_kept(x, keep1)
    for i, blk in enumerate(m.blocks):
        x = x + pc._scale(enc, i, 0, x) * self_attn(blk.attn, vo._ln(blk.norm1, x), h)
        x = x + pc._scale(enc, i, 1, x) * vo._mlp(blk.mlp, vo._ln(blk.norm2, x))
    return x


def decoder_blocks(m, feats, x, dec=None):
    """The CrossBlocks on the token stream x [B, tokens, D] (cls row first), before any final norm."""
    h = m.shape.num_heads
    self_attn, cross_attn = pc._attn_fns(m)
    for i, blk in enumerate(m.cross_blocks):
        x = x + pc._scale(dec, i, 0, x) * self_attn(blk.attn, vo._ln(blk.norm1, x), h)
        x = x + pc._scale(dec, i, 1, x) * cross_attn(blk.cross_attn, vo._ln(blk.norm_cross, x), vo._ln(blk.norm_context, feats), h)
        x = x + pc._scale(dec, i, 2, x) * vo._mlp(blk.mlp, vo._ln(blk.norm2, x))
    return x


def decoder(m, feats, x2, keep2=None, dec=None):
    """forward_head(forward_second_part(feats, x2)); with ``keep2`` the mean of 'avg' runs over the K kept tokens."""
    x = m.prepare_x2(x2)
    if keep2 is not None:
        x = pc.gather_kept(x, keep2)
    return m.forward_head(m.final_norm(decoder_blocks(m, feats, x, dec)))


def forward(m, x, keep1=None, keep2=None, enc=None, dec=None):
    """The one-shot forward on stacked pairs x [B, 2, C, S, S]."""
    x1, x2 = torch.unbind(x, 1)
    return decoder(m, encoder(m, x1, keep1, enc), x2, keep2, dec)


def is_fc_norm_key(name):
    return name.startswith('fc_norm.')


def fill_closed_form_(module):
    """qc.fill_closed_form_ plus the closed-form fill of ``fc_norm`` in any module tree with the reference's names (vo.fill_closed_form_
    knows a LayerNorm by a name that starts with 'norm'): the weight around 1 (1 + 0.2 f(i)), the bias around 0 (0.05 f(i))."""
    qc.fill_closed_form_(module)
    with torch.no_grad():
        for name, p in module.state_dict().items():
            if is_fc_norm_key(name):
                salt = zlib.crc32(name.encode()) % 9973
                p.copy_(vo.closed_form(p.shape, salt, 0.2, 1.0) if name.endswith('weight') else vo.closed_form(p.shape, salt, 0.05))
    return module


loss_and_grads = qc.loss_and_grads

# the geometries and inputs of tests/golden/pool_head.npz: 16-pixel images, patch 8 (5 tokens); head_dim 32 with 1 + 2 blocks, head_dim
# 64 with 2 + 1 blocks (the only decoder block is then also the last one); B = 3
GOLDEN_SHAPES = (vo.ViTEDShape(img_size=16, patch_size=8, num_classes=4, embed_dim=64, num_heads=2, depth=1, c_depth=2),
                 vo.ViTEDShape(img_size=16, patch_size=8, num_classes=4, embed_dim=128, num_heads=2, depth=2, c_depth=1))
GOLDEN_BATCH = 3


def golden_inputs(s):
    x = vo.closed_form_pairs(GOLDEN_BATCH, s)
    y = (vo.closed_form((GOLDEN_BATCH, s.num_classes), 77, 1.0) > 0.2).float()
    return x, y
