"""Block-local parity: every stage of the ViT-ED restarted on the CPU from an implementation's own taps.

An implementation under test (the HIP model, or a rounding model standing in for one) runs ONE forward + BCE backward and records, at
the block boundaries, what went in and what came back: the input of every block, the final encoder output (the decoder's context)
and the gradient that arrived at every block's output.  Each stage is then run again ALONE from those taps, in fp64, and whatever
the implementation produced for that stage - its output, the gradient w.r.t. its input, the gradient of every parameter it owns -
is compared with the restart.  Errors of one stage cannot hide behind (or be blamed on) the 16 blocks around it.

The stages, which between them own every parameter of the model:

    embed     images, d(enc block 0 input), d(dec block 0 input)  ->  the two inputs; patch_embed.proj.*, pos_embed, cls_token
    enc i     input, dy                                           ->  y, dx; blocks.i.*
    dec i     input, context, dy                                  ->  y, dx, d(context) or d(kv output); cross_blocks.i.*
    context   d(features) in total; where the implementation computes the keys / values of all decoder blocks ahead (``fold``), also
              norm_context.* and cross_attn.kv.* of every block, restarted from the blocks' d(kv output)
    head      last block's output (its cls rows alone under ``cls_rows``)  ->  logits, dy of the last block; norm.* | fc_norm.*, head.*

Every stage is written once, on the oracle's functional pieces, with a :class:`Rounding` applied at chosen points:

    EXACT     no rounding: the fp64 reference
    MODEL     the rounding model of a bf16 path: round to bf16 (and the gradient that comes back through the same point too) at the
              input and the weight of every Linear, at q, k, v and P of the two attention products and at the attention output; in
              the pair-indexed form also the gradient of the kv projection's output, after the sum over an image's pairs
              (attention_segsum.hip)
    MODEL2    a second bf16 implementation that rounds at more points - every LayerNorm's output, GELU's output, and the gradient
              that enters a residual branch (the stream gradient's low-precision copy).  Only the CPU tests use it, as the stand-in
              "other careful bf16 implementation" that the bound must let through.

The options of training (an :class:`Options`; None = the plain model) enter the same stages:

    drop path      a block takes its per-sample scales, fp64 [branches, B]: x + s[:, None, None] * branch (droppath_cases)
    patch dropout  ``embed`` gathers through a keep table (patchdrop_cases.gather_kept); every later stage runs on the shorter stream
    position drop  ``embed`` multiplies by mask * 1 / (1 - p) (posdrop_cases.multiplier) in front of the gather.  The taps enc.in / dec.in
                   are taken behind the dropout and enc.dx.0 / dec.dx.0 in front of the mask on the gradient, so the mask belongs to the
                   embed stage, forward and backward
    pairs          the two halves have batches of their own - images and pairs - and pair p's context is features[index[p]].  Gathered
                   (``model(feats[i], x2[j])``): the decoder's stages are per pair and autograd sums d(features) over an image's pairs.
                   Indexed (``model(feats, x2, x2_index=j, x1_index=i)``): the kv projections run per image, a block's d(kv output) /
                   d(context) and context.dfeats are per image, and the bf16 path rounds there once more (``Rounding.seg``)

The statistics (:func:`stats`) are ``whole`` = the whole-tensor relative norm and ``rowmax`` = the worst row (last dimension) of
|got - ref| / (|ref| + floor): an error confined to the cls row of 65 is not diluted.
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

import droppath_cases as dc
import patchdrop_cases as pdc
import pool_cases as pc      # noqa: F401  (the pooled-head trees; its patchdrop_cases import needs the tests directory on sys.path)
import posdrop_cases as psc
import qknorm_cases as qc
from oracle import vited_oracle as vo


# ----------------------------------------------------------------------------------------------------------------------------
# rounding
# ----------------------------------------------------------------------------------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


class _RoundBoth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _bf16(x)

    @staticmethod
    def backward(ctx, g):
        return _bf16(g)


class _RoundGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return _bf16(g)


def _same(t):
    return t


class Rounding:
    """Where a stage rounds to bf16: ``op`` the operands of every contraction, ``ln`` a LayerNorm's output, ``act`` GELU's output,
    ``branch`` the gradient entering a residual branch (forward: identity), ``seg`` the gradient of the kv projection's output in the
    pair-indexed form, summed over an image's pairs (forward: identity) - attention_segsum.hip rounds that sum to bf16, and each pair's
    term was rounded before it, which ``op`` at k and v already states."""

    def __init__(self, name, op=False, ln=False, act=False, branch=False, seg=False):
        self.name = name
        self.op = _RoundBoth.apply if op else _same
        self.ln = _RoundBoth.apply if ln else _same
        self.act = _RoundBoth.apply if act else _same
        self.branch = _RoundGrad.apply if branch else _same
        self.seg = _RoundGrad.apply if seg else _same

    def __repr__(self):
        return f'Rounding({self.name})'


EXACT = Rounding('fp64')
MODEL = Rounding('model', op=True, seg=True)
MODEL2 = Rounding('model2', op=True, ln=True, act=True, branch=True, seg=True)


# ----------------------------------------------------------------------------------------------------------------------------
# the network's pieces with the rounding points (vo.encoder_block / vo.decoder_block / qc.self_attention / qc.cross_attention /
# pc's head with R applied; under EXACT they ARE those functions, which test_block_restart_cases.py pins)
# ----------------------------------------------------------------------------------------------------------------------------
def _lin(R, x, m):
    return F.linear(R.op(x), R.op(m.weight), m.bias)


def _sdpa(R, q, k, v):
    p = torch.softmax((R.op(q) * q.shape[-1] ** -0.5) @ R.op(k).transpose(-2, -1), dim=-1)
    o = R.op(p) @ R.op(v)
    b, h, n, hd = o.shape
    return o.transpose(1, 2).reshape(b, n, h * hd)


def _qk(m, q, k):
    """q_norm / k_norm of a qk_norm=True tree (qknorm_cases), per head."""
    if hasattr(m, 'q_norm'):
        return qc._head_norm(m.q_norm, q), qc._head_norm(m.k_norm, k)
    return q, k


def self_attention(R, m, x, nh):
    q, k, v = _lin(R, x, m.qkv).chunk(3, dim=-1)
    q, k = _qk(m, vo._heads(q, nh), vo._heads(k, nh))
    return _lin(R, _sdpa(R, q, k, vo._heads(v, nh)), m.proj)


def cross_attention(R, m, x, kv, nh):
    """``kv``: the kv projection's output on the normalised context (kv_projection), so that a stage can ask for its gradient."""
    q = _lin(R, x, m.q)
    k, v = kv.chunk(2, dim=-1)
    q, k = _qk(m, vo._heads(q, nh), vo._heads(k, nh))
    return _lin(R, _sdpa(R, q, k, vo._heads(v, nh)), m.proj)


def kv_projection(R, blk, context):
    return _lin(R, R.ln(vo._ln(blk.norm_context, context)), blk.cross_attn.kv)


def _mlp(R, m, x):
    return _lin(R, R.act(F.gelu(_lin(R, x, m.fc1))), m.fc2)


def _add(R, x, branch, scales, j):
    """x + branch, or x + s[:, None, None] * branch with s = scales[j], one stochastic-depth scale per sample."""
    b = R.branch(branch)
    return x + b if scales is None else x + scales[j].to(x.dtype).view(-1, 1, 1) * b


def encoder_block(R, blk, x, nh, scales=None):
    """``scales``: this block's stochastic-depth scales [2, B] (attn, mlp) or None; droppath_cases.encoder_scaled's block under EXACT."""
    x = _add(R, x, self_attention(R, blk.attn, R.ln(vo._ln(blk.norm1, x)), nh), scales, 0)
    return _add(R, x, _mlp(R, blk.mlp, R.ln(vo._ln(blk.norm2, x))), scales, 1)


def gather_kv(R, kv, index):
    """The keys / values of the pairs from those of the images: kv [images, n, 2 D] -> [pairs, n, 2 D] (backward: the per-image sum)."""
    return R.seg(kv)[index]


def decoder_block(R, blk, x, context, nh, store=None, scales=None, index=None, gather=gather_kv):
    """``store`` (a dict) receives the kv projection's output under 'kv', kept in the graph.  ``scales``: [3, B] (self, cross, mlp) or
    None.  ``index`` (int64 [pairs]): ``context`` holds one item per image and pair p attends over item index[p] (with q/k-norm trees
    the model's k_norm then runs per pair, behind the gather; the HIP path's runs per image - no case combines the two); ``gather``
    is that gather, which a CPU test replaces to plant a defect in it."""
    x = _add(R, x, self_attention(R, blk.attn, R.ln(vo._ln(blk.norm1, x)), nh), scales, 0)
    kv = kv_projection(R, blk, context)
    if store is not None:
        kv.retain_grad()
        store['kv'] = kv
    if index is not None:
        kv = gather(R, kv, index)
    x = _add(R, x, cross_attention(R, blk.cross_attn, R.ln(vo._ln(blk.norm_cross, x)), kv, nh), scales, 1)
    return _add(R, x, _mlp(R, blk.mlp, R.ln(vo._ln(blk.norm2, x))), scales, 2)


def embed(R, m, img, with_cls, keep=None, mult=None):
    """timm PatchEmbed (a Linear on the patches) + pos_embed: forward_first_part's first line / prepare_x2; then position dropout
    (``mult`` = mask * scale over the whole stream) and patch dropout (``keep``: the prefix row and the rows 1 + keep), in the
    reference's order."""
    s = m.shape
    w, b = m.patch_embed.proj.weight, m.patch_embed.proj.bias
    tok = F.conv2d(R.op(img), R.op(w), b, stride=s.patch_size).flatten(2).transpose(1, 2)
    if not with_cls:
        x = tok + m.pos_embed[:, 1:]
    else:
        x = torch.cat((m.cls_token.expand(tok.shape[0], -1, -1), tok), dim=1) + m.pos_embed
    if mult is not None:
        x = x * mult.to(x.dtype)
    return x if keep is None else pdc.gather_kept(x, keep)


def head(R, m, x):
    """Final norm, pooling and head on the last block's output x [B, rows, D] (row 0: the cls row) - vo's ``cross_part`` last line +
    ``forward_head``, or pool_cases' ``final_norm`` + ``forward_head`` for a tree with the head options."""
    avg = getattr(m, 'global_pool', 'token') == 'avg'
    fc = getattr(m, 'use_fc_norm', False)
    if not fc:
        x = R.ln(vo._ln(m.norm, x))
    x = x[:, 1:].mean(dim=1) if avg else x[:, 0]
    if fc:
        x = R.ln(vo._ln(m.fc_norm, x))
    return _lin(R, x, m.head)


def loss_of(logits, target):
    return F.binary_cross_entropy_with_logits(logits, target)


# ----------------------------------------------------------------------------------------------------------------------------
# an implementation's taps in the canonical layout ([B, tokens, D], fp64 on the CPU)
# ----------------------------------------------------------------------------------------------------------------------------
def _param_grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


class Options:
    """The training options of one forward + backward, as the stages read them (every field None / False: the plain model).

    enc, dec        stochastic-depth scales [depth, 2, images] / [c_depth, 3, pairs] (droppath_cases)
    keep1, keep2    patch-dropout keep tables int64 [images, K1] / [pairs, K2] (patchdrop_cases)
    mult1, mult2    position dropout's mask * scale over the whole streams [images, n1, D] / [pairs, 1 + n1, D] (posdrop_cases)
    index           int64 [pairs]: pair p's context is features[index[p]] (None: pair p reads image p)
    indexed         with ``index``: the implementation projects keys / values per image and sums their gradients per image; False:
                    it was handed the gathered features[index] and everything of the decoder is per pair
    The remaining fields say how the HIP model is called for the same step: ``seeds`` / ``pos_rate`` (the masks' source), ``x2_index``
    (int64 [pairs]: pair p's second image), and the rates the model is built with."""

    def __init__(self, enc=None, dec=None, keep1=None, keep2=None, mult1=None, mult2=None, index=None, indexed=False,
                 seeds=None, pos_rate=0., x2_index=None, drop_path_rate=0., patch_rate=0.):
        self.enc, self.dec, self.keep1, self.keep2, self.mult1, self.mult2 = enc, dec, keep1, keep2, mult1, mult2
        self.index, self.indexed = index, bool(indexed and index is not None)
        self.seeds, self.pos_rate, self.x2_index, self.drop_path_rate, self.patch_rate = seeds, pos_rate, x2_index, drop_path_rate, patch_rate

    def enc_of(self, i):
        return None if self.enc is None else self.enc[i].double()

    def dec_of(self, i):
        return None if self.dec is None else self.dec[i].double()

    def context_of(self, feats):
        """The features as the decoder's stages see them: per image, or gathered per pair."""
        return feats if self.index is None or self.indexed else feats[self.index]

    @property
    def kv_index(self):
        return self.index if self.indexed else None


PLAIN = Options()


def _halves(x):
    """(image-1 batch, image-2 batch) of stacked pairs [B, 2, C, S, S] or of a pair of batches ([images, C, S, S], [pairs, C, S, S])."""
    return torch.unbind(x, 1) if torch.is_tensor(x) else tuple(x)


def network_taps(m, x, target, R=EXACT, cls_rows=False, fold=False, opt=None, stages=None):
    """One forward + BCE backward of the whole network ``m`` (an oracle tree, any dtype) under rounding ``R``, recorded as the HIP
    path records it: returns (taps, parameter gradients by name).  ``cls_rows``: the last decoder block's output and its gradient
    are recorded on the cls rows alone; ``fold``: per block d(kv output) is recorded instead of the running d(context).
    ``x``: stacked pairs, or (images, second images of the pairs); ``opt``: the :class:`Options`.  ``stages`` replaces ``embed`` /
    ``encoder_block`` / ``decoder_block`` by name: how the CPU tests plant a defect in the implementation that records."""
    s, nh = m.shape, m.shape.num_heads
    opt = PLAIN if opt is None else opt
    st = {'embed': embed, 'encoder_block': encoder_block, 'decoder_block': decoder_block, **(stages or {})}
    m.zero_grad(set_to_none=True)
    x1, x2 = _halves(x)
    taps = {'x1': x1, 'x2': x2, 'target': target}
    t, u = st['embed'](R, m, x1, False, opt.keep1, opt.mult1), st['embed'](R, m, x2, True, opt.keep2, opt.mult2)
    taps['enc.in'], taps['dec.in'] = t.detach(), u.detach()
    enc_at, dec_at, ctx_at, kv_at = [], [], [], []
    for i, blk in enumerate(m.blocks):
        t.retain_grad()
        enc_at.append(t)
        t = st['encoder_block'](R, blk, t, nh, opt.enc_of(i))
        taps[f'enc.x.{i}'] = t.detach()
    t.retain_grad()
    enc_at.append(t)
    for i, blk in enumerate(m.cross_blocks):
        u.retain_grad()
        dec_at.append(u)
        # this block's own handle on the features (gathered per pair where the implementation was handed feats[index]): its gradient is
        # the block's d(context) term, and autograd sums the terms - over the pairs of an image too - into the encoder's gradient
        c = opt.context_of(t).clone()
        c.retain_grad()
        ctx_at.append(c)
        store = {}
        u = st['decoder_block'](R, blk, u, c, nh, store, opt.dec_of(i), opt.kv_index)
        kv_at.append(store['kv'])
        taps[f'dec.x.{i}'] = u.detach()
    u.retain_grad()
    dec_at.append(u)
    logits = head(R, m, u)
    taps['logits'] = logits.detach()
    loss_of(logits, target).backward()
    for i, a in enumerate(enc_at):
        taps[f'enc.dx.{i}'] = a.grad.detach()
    for i, a in enumerate(dec_at):
        taps[f'dec.dx.{i}'] = a.grad.detach()
    running = None
    for i in reversed(range(s.c_depth)):
        running = ctx_at[i].grad.detach() if running is None else running + ctx_at[i].grad.detach()
        if fold:
            taps[f'dec.dkvo.{i}'] = kv_at[i].grad.detach()
        else:
            taps[f'dec.dctx.{i}'] = running
    taps['dec.dfeats'] = running
    if cls_rows:
        last = s.c_depth - 1
        taps[f'dec.x.{last}'] = taps[f'dec.x.{last}'][:, 0]
        taps[f'dec.dx.{s.c_depth}'] = taps[f'dec.dx.{s.c_depth}'][:, 0]
    return taps, _param_grads(m)


PER_CONTEXT_ITEM = ('kv', 'dkv', 'dkvo', 'dctx', 'dfeats')       # the decoder's taps on the context's side: per image in the indexed form


def canonical_taps(raw, s, batch, pairs=None, indexed=False):
    """Taps as functions.py records them ([rows, D] device tensors in the compute dtype) -> fp64 CPU tensors [B, tokens, D] (a tensor of
    B rows stays [B, D]: the cls rows of the last decoder block).  ``batch``: the images of the encoder's call; ``pairs``: the pairs of
    the decoder's (None: as many); ``indexed``: the decoder's context-side taps are per image.  The token count is whatever the rows
    give (fewer than the geometry's under patch dropout)."""
    pairs = batch if pairs is None else pairs
    out = {}
    for k, v in raw.items():
        v = v.detach().to('cpu', torch.float64)
        if k in ('x1', 'x2', 'target', 'logits'):
            out[k] = v
            continue
        b = batch if k.startswith('enc.') or (indexed and k.split('.')[1] in PER_CONTEXT_ITEM) else pairs
        width = v.shape[-1]
        rows = v.numel() // width
        assert rows % b == 0, f'{k}: {rows} rows for a batch of {b}'
        out[k] = v.reshape(b, width) if rows == b else v.reshape(b, rows // b, width)
    return out


def layout_of(taps, s):
    """(cls_rows, fold) of a set of taps: how the implementation that recorded them ran the last block and the kv projections."""
    return taps[f'dec.x.{s.c_depth - 1}'].dim() == 2, 'dec.dctx.0' not in taps


KV_PARAMS = ('norm_context.weight', 'norm_context.bias', 'cross_attn.kv.weight', 'cross_attn.kv.bias')


def observed(taps, grads, s):
    """What the implementation itself produced for every stage, under the labels restart_all uses: label -> tensor."""
    cls_rows, fold = layout_of(taps, s)
    out = OrderedDict()
    out['embed.enc_in'], out['embed.dec_in'] = taps['enc.in'], taps['dec.in']
    for i in range(s.depth):
        out[f'enc{i}.y'], out[f'enc{i}.dx'] = taps[f'enc.x.{i}'], taps[f'enc.dx.{i}']
    for i in range(s.c_depth):
        out[f'dec{i}.y'], out[f'dec{i}.dx'] = taps[f'dec.x.{i}'], taps[f'dec.dx.{i}']
        if fold:
            out[f'dec{i}.dkv'] = taps[f'dec.dkvo.{i}']
        else:       # the block's own term of the running sum
            out[f'dec{i}.dctx'] = taps[f'dec.dctx.{i}'] - taps[f'dec.dctx.{i + 1}'] if i + 1 < s.c_depth else taps[f'dec.dctx.{i}']
    out['context.dfeats'] = taps['dec.dfeats']
    out['head.logits'], out['head.dy'] = taps['logits'], taps[f'dec.dx.{s.c_depth}']
    for n, g in grads.items():
        out['g:' + n] = g.detach().to('cpu', torch.float64)
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# the restarts
# ----------------------------------------------------------------------------------------------------------------------------
def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _take_grads(m, out, only=None):
    for n, g in _param_grads(m).items():
        if only is None or only(n):
            assert 'g:' + n not in out, f'{n} belongs to two stages'
            out['g:' + n] = g
    m.zero_grad(set_to_none=True)


def restart_embed(m, taps, R, out, opt=PLAIN):
    """Both embeddings with position and patch dropout inside: the parameters' gradients come back through the gather and the mask."""
    t, u = embed(R, m, taps['x1'], False, opt.keep1, opt.mult1), embed(R, m, taps['x2'], True, opt.keep2, opt.mult2)
    out['embed.enc_in'], out['embed.dec_in'] = t.detach(), u.detach()
    # the encoder's and the decoder's contributions in one backward: summed, as the model's parameters receive them
    ((t * taps['enc.dx.0']).sum() + (u * taps['dec.dx.0']).sum()).backward()
    _take_grads(m, out)


def restart_enc(m, taps, R, out, i, dy=None, opt=PLAIN):
    x = _leaf(taps['enc.x.%d' % (i - 1)] if i else taps['enc.in'])
    y = encoder_block(R, m.blocks[i], x, m.shape.num_heads, opt.enc_of(i))
    y.backward(taps[f'enc.dx.{i + 1}'] if dy is None else dy)
    out[f'enc{i}.y'], out[f'enc{i}.dx'] = y.detach(), x.grad
    _take_grads(m, out)


def restart_dec(m, taps, R, out, i, opt=PLAIN):
    """Returns the block's d(context): per pair, or per image in the indexed form."""
    s = m.shape
    cls_rows, fold = layout_of(taps, s)
    x = _leaf(taps['dec.x.%d' % (i - 1)] if i else taps['dec.in'])
    c = _leaf(opt.context_of(taps[f'enc.x.{s.depth - 1}']))
    store = {}
    y = decoder_block(R, m.cross_blocks[i], x, c, s.num_heads, store, opt.dec_of(i), opt.kv_index)
    dy = taps[f'dec.dx.{i + 1}']
    if cls_rows and i == s.c_depth - 1:         # only the cls rows of this block's output exist, and only they carry gradient
        full = torch.zeros_like(y)
        full[:, 0] = dy
        y.backward(full)
        out[f'dec{i}.y'] = y.detach()[:, 0]
    else:
        y.backward(dy)
        out[f'dec{i}.y'] = y.detach()
    out[f'dec{i}.dx'] = x.grad
    if fold:
        out[f'dec{i}.dkv'] = store['kv'].grad
        _take_grads(m, out, only=lambda n: not n.endswith(KV_PARAMS))
    else:
        out[f'dec{i}.dctx'] = c.grad
        _take_grads(m, out)
    return c.grad


def restart_context(m, taps, R, out, opt=PLAIN):
    """The kv projections of every block on the final encoder output, from the blocks' d(kv output): d(features) in total and the
    gradients of norm_context.* / cross_attn.kv.* (the layout with the keys / values computed ahead) - on the context's items as the
    implementation had them: the gathered features of the pairs, or in the indexed form the images."""
    s = m.shape
    c = _leaf(opt.context_of(taps[f'enc.x.{s.depth - 1}']))
    sum((kv_projection(R, blk, c) * taps[f'dec.dkvo.{i}']).sum() for i, blk in enumerate(m.cross_blocks)).backward()
    out['context.dfeats'] = c.grad
    _take_grads(m, out)


def restart_head(m, taps, R, out):
    s = m.shape
    x = _leaf(taps[f'dec.x.{s.c_depth - 1}'])
    logits = head(R, m, x.unsqueeze(1) if x.dim() == 2 else x)
    loss_of(logits, taps['target']).backward()
    out['head.logits'], out['head.dy'] = logits.detach(), x.grad
    _take_grads(m, out)


def restart_all(m, taps, R, opt=None):
    """Every stage of ``m`` (an fp64 oracle tree) restarted from ``taps`` under rounding ``R`` with the options ``opt``: label ->
    tensor, the parameter gradients under 'g:' + the state_dict name."""
    s = m.shape
    opt = PLAIN if opt is None else opt
    _, fold = layout_of(taps, s)
    m.zero_grad(set_to_none=True)
    out = OrderedDict()
    restart_embed(m, taps, R, out, opt)
    for i in range(s.depth):
        restart_enc(m, taps, R, out, i, opt=opt)
    total = 0
    for i in range(s.c_depth):
        total = total + restart_dec(m, taps, R, out, i, opt)
    if fold:
        restart_context(m, taps, R, out, opt)
    else:
        out['context.dfeats'] = total
    restart_head(m, taps, R, out)
    return out


def features_gradient(taps, s, opt=None, dtype=torch.float32):
    """What the encoder must have received as the gradient of its output, from the decoder's total d(features): that tensor itself, or in
    the gathered form (autograd does the gather's backward) its sum over the pairs of every image, in pair order and in ``dtype`` - the
    fp32 of the HIP path's streams."""
    d = taps['dec.dfeats']
    if opt is None or opt.index is None or opt.indexed:
        return d
    images = taps[f'enc.x.{s.depth - 1}'].shape[0]
    return torch.zeros((images,) + tuple(d.shape[1:]), dtype=dtype).index_add_(0, opt.index, d.to(dtype)).double()


def checked_parameters(out):
    return {k[2:] for k in out if k.startswith('g:')}


# ----------------------------------------------------------------------------------------------------------------------------
# the checker
# ----------------------------------------------------------------------------------------------------------------------------
FP32_WHOLE, FP32_ROWMAX = 1e-4, 1e-3        # the project's own fp32 figures (test_against_oracle_random_init: global, per tensor)
BF16_FACTOR, BF16_FLOOR = 2.0, 2.0 ** -8    # x the rounding model's statistic + one bf16 rounding
SMALL_GRADIENT = 1e-3                       # a parameter gradient below this fraction of the case's largest may skip ``rowmax``
MAX_EXEMPT = 2


def _rowmax(d, r, floor_scale):
    rn = r.norm(dim=1)
    floor = floor_scale * rn.pow(2).mean().sqrt()
    return float((d.norm(dim=1) / (rn + floor)).max()) if float(floor) > 0 else (0.0 if float(d.norm()) == 0 else float('inf'))


def stats(label, got, ref, scale=None):
    """(whole, rowmax | None) of one compared tensor.  Streams: rows = the last dimension, floor 1e-3 x the rms row norm.  2-D
    parameter gradients: rows and columns, floor = the rms row (column) norm - a row of a weight gradient with a tiny norm says
    nothing.  1-D parameters (biases, LayerNorm parameters, cls_token): ``whole`` alone.  ``scale``: the norm that ``whole`` is
    relative to where the reference's own is no scale (scale_of)."""
    got, ref = got.detach().double(), ref.detach().double()
    assert got.numel() == ref.numel(), f'{label}: {tuple(got.shape)} against {tuple(ref.shape)}'
    got = got.reshape(ref.shape)
    whole = float((got - ref).norm() / ((ref.norm() if scale is None else scale) + 1e-300))
    if label.startswith('g:'):
        if ref.numel() == ref.shape[-1]:
            return whole, None
        r = ref.reshape(ref.shape[0], -1) if ref.shape[0] > 1 else ref.reshape(-1, ref.shape[-1])   # conv [D, C p p]; pos_embed [1, n, D]
        d = got.reshape(r.shape) - r
        return whole, max(_rowmax(d, r, 1.0), _rowmax(d.t(), r.t(), 1.0))
    r = ref.reshape(-1, ref.shape[-1])
    return whole, _rowmax(got.reshape(r.shape) - r, r, 1e-3)


def exempt_labels(ref):
    """The parameter gradients whose fp64 reference norm is below SMALL_GRADIENT of the case's largest: exempt from ``rowmax``."""
    norms = {k: float(v.norm()) for k, v in ref.items() if k.startswith('g:')}
    top = max(norms.values())
    return sorted(k for k, v in norms.items() if v < SMALL_GRADIENT * top and stats(k, ref[k], ref[k])[1] is not None)


def scale_of(label, ref):
    """The gradient of a k_norm bias is ZERO in exact arithmetic: the bias adds q . b to every score of a query's row, and softmax does
    not see a constant (the fp64 restart gives 1e-18 of rounding noise where the other gradients are 1e-3 .. 1).  A relative norm
    against that reference measures nothing, so ``whole`` of this one tensor is taken relative to its sibling k_norm.weight's
    reference norm: d bias = sum over keys of d(k normalised), d weight = the same sum weighted by the unit-variance xhat - the
    same terms, the same number of them, so the same rounding noise.  Every other tensor: its own norm (None)."""
    if label.endswith('k_norm.bias'):
        return ref[label[:-len('bias')] + 'weight'].double().norm()
    return None


def compare(got, ref, model=None):
    """[(label, (whole, rowmax) of got, (whole, rowmax) of the rounding model | None)] over the labels of ``ref``."""
    assert set(got) >= set(ref), sorted(set(ref) - set(got))
    return [(k, stats(k, got[k], ref[k], scale_of(k, ref)), stats(k, model[k], ref[k], scale_of(k, ref)) if model is not None else None)
            for k in ref]


def failures(rows, exempt=()):
    """The rows that miss the bound: fp32 (no model statistics) the absolute figures, bf16 2 x the model's statistic + 2^-8."""
    bad = []
    for label, (whole, rowmax), mstat in rows:
        if mstat is None:
            lim_w, lim_r = FP32_WHOLE, FP32_ROWMAX
        else:
            lim_w = BF16_FACTOR * mstat[0] + BF16_FLOOR
            lim_r = BF16_FACTOR * mstat[1] + BF16_FLOOR if mstat[1] is not None else None
        if not whole <= lim_w:
            bad.append(f'{label}: whole {whole:.3e} > {lim_w:.3e}')
        if rowmax is not None and label not in exempt and not rowmax <= lim_r:
            bad.append(f'{label}: rowmax {rowmax:.3e} > {lim_r:.3e}')
    return bad


def table(rows):
    fmt = lambda v: '    -    ' if v is None else f'{v:9.2e}'
    lines = [f'{"tensor":52s} {"whole":>9s} {"rowmax":>9s}   model: {"whole":>9s} {"rowmax":>9s}']
    for label, (whole, rowmax), mstat in rows:
        tail = f'          {fmt(mstat[0])} {fmt(mstat[1])}' if mstat is not None else ''
        lines.append(f'{label:52s} {fmt(whole)} {fmt(rowmax)}{tail}')
    return '\n'.join(lines)


def by_stage(rows):
    """Worst statistics per stage and kind of tensor: {(stage, 'stream' | 'param'): [whole, rowmax, model whole, model rowmax]} - the
    summary DESIGN.md section 8.3 tabulates."""
    out = OrderedDict()
    for label, (whole, rowmax), mstat in rows:
        if label.startswith('g:'):
            n = label[2:]
            stage = ('enc' if n.startswith('blocks.') else 'kv' if n.endswith(KV_PARAMS) else 'dec' if n.startswith('cross_blocks.')
                     else 'head' if n.startswith(('norm.', 'fc_norm.', 'head.')) else 'embed')
            key = (stage, 'param')
        else:
            key = (label.split('.')[0].rstrip('0123456789'), 'stream')
        acc = out.setdefault(key, [0.0, 0.0, 0.0, 0.0])
        vals = (whole, rowmax) + (mstat if mstat is not None else (None, None))
        for j, v in enumerate(vals):
            if v is not None:
                acc[j] = max(acc[j], v)
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# the cases: trees at reference-style random init with every LayerNorm moved off (1, 0), seeded inputs
# ----------------------------------------------------------------------------------------------------------------------------
SHAPE_A = vo.ViTEDShape(img_size=64, patch_size=8, embed_dim=384, num_heads=12, depth=2, c_depth=3)       # 64 / 65 tokens, head dim 32
SHAPE_LONG = vo.ViTEDShape(img_size=256, patch_size=16, num_classes=1, embed_dim=384, num_heads=6, depth=1, c_depth=2)   # 256 / 257, head dim 64
BATCH_A, BATCH_LONG = 4, 2


def build_tree(s, kind='plain', seed=0):
    """An oracle tree (fp32, as a checkpoint would hold it) of ``kind`` 'plain' | 'qk' | 'pool' ('avg' + fc_norm) at the reference's
    random init; every LayerNorm's weight and bias are then perturbed by 0.2 N(0, 1) - at the init itself (1, 0) a LayerNorm gradient
    taken from the wrong norm, or a fold that loses gamma, would go unseen."""
    torch.manual_seed(seed)
    m = {'plain': vo.OracleViTED, 'qk': qc.QKNormViTED, 'pool': lambda sh: pc.PoolViTED(sh, 'avg', None)}[kind](s)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if 'norm' in n:
                p.add_(0.2 * torch.randn(p.shape, generator=g))
    return m


def inputs(s, batch, seed=0):
    g = torch.Generator().manual_seed(seed + 2000)
    x = torch.randn(batch, 2, s.in_chans, s.img_size, s.img_size, generator=g).clamp(-1, 1)
    y = (torch.rand(batch, s.num_classes, generator=g) > 0.6).float()
    return x, y


def pair_inputs(s, images, pairs, seed=0):
    """(images [images, C, S, S], targets [pairs, classes]) of a two-stage step."""
    g = torch.Generator().manual_seed(seed + 3000)
    imgs = torch.randn(images, s.in_chans, s.img_size, s.img_size, generator=g).clamp(-1, 1)
    y = (torch.rand(pairs, s.num_classes, generator=g) > 0.6).float()
    return imgs, y


# ----------------------------------------------------------------------------------------------------------------------------
# the cases with the options: closed-form scales and keep tables, masks from fixed seeds, an uneven and unsorted pair index
# ----------------------------------------------------------------------------------------------------------------------------
SHAPE_W768 = vo.ViTEDShape(img_size=64, patch_size=8, embed_dim=768, num_heads=12, depth=1, c_depth=2)      # 64 / 65 tokens, head dim 64
# 5 images, 12 pairs: image 3 is read five times, image 2 by no pair, and no image's pairs stand together
PAIRS_A = (5, [3, 0, 3, 1, 4, 3, 0, 3, 1, 4, 3, 0], [0, 1, 2, 3, 4, 2, 4, 1, 0, 3, 0, 2])
# 3 images, 5 pairs: image 1 is read by no pair
PAIRS_LONG = (3, [2, 0, 2, 2, 0], [1, 0, 2, 2, 1])
POS_SEEDS = (1234567890123, -77)


def case_scales(rate, depth, branches, batch, salt):
    """droppath_cases.irregular_scales, with block 0 (keep probability 1, so scale 1) made to drop one sample per branch as well:
    every branch of every block keeps at least one sample and drops at least one, so that no reference gradient is exactly zero."""
    sc = dc.irregular_scales(rate, depth, branches, batch, salt)
    for j in range(branches):
        sc[0, j, 1 + j % (batch - 1)] = 0
    kept = sc > 0
    assert bool(kept.any(-1).all()) and not bool(kept.all(-1).any()), 'a branch keeps or drops its whole batch'
    return sc


def make_options(s, images, pairs=None, ops=None, drop_path=0., patch_drop=0., pos_drop=0., index=None, x2_index=None, indexed=False):
    """The :class:`Options` of a case at geometry ``s``.  ``ops`` (the package's ops module) is where the position masks come from:
    ``token_dropout_mask``, the HIP kernel's rule on the CPU, which tests/test_posdrop.py pins bit for bit."""
    pairs = images if pairs is None else pairs
    o = Options(index=None if index is None else torch.tensor(index), indexed=indexed, x2_index=None if x2_index is None else torch.tensor(x2_index),
                drop_path_rate=drop_path, patch_rate=patch_drop, pos_rate=pos_drop)
    if drop_path:
        o.enc, o.dec = case_scales(drop_path, s.depth, 2, images, salt=31), case_scales(drop_path, s.c_depth, 3, pairs, salt=47)
    if patch_drop:
        o.keep1 = pdc.closed_form_keep(images, s.n1 - 1, pdc.keep_count(s.n1 - 1, patch_drop), salt=1)
        o.keep2 = pdc.closed_form_keep(pairs, s.n1, pdc.keep_count(s.n1, patch_drop), salt=2)
    if pos_drop:
        o.seeds = POS_SEEDS
        mask1, mask2, scale = psc.masks_of(ops, o.seeds, pos_drop, images, pairs, s)
        fp64 = torch.zeros((), dtype=torch.float64)
        o.mult1, o.mult2 = psc.multiplier(mask1, scale, fp64), psc.multiplier(mask2, scale, fp64)
    return o


#              id                      tree     shape       what the options are made of                        runtime switches         two calls
OPTION_CASES = [
    ('droppath',             'plain', 'A',    dict(drop_path=0.2),                                  {},                       None),
    ('droppath-fused_ln',    'plain', 'A',    dict(drop_path=0.2),                                  {'fused_ln': False},      None),
    ('droppath-cls_tail',    'plain', 'A',    dict(drop_path=0.2),                                  {'cls_tail': False},      None),
    ('patchdrop',            'plain', 'A',    dict(patch_drop=0.25),                                {},                       None),
    ('posdrop',              'plain', 'A',    dict(pos_drop=0.1),                                   {},                       None),
    ('all-qk_norm',          'qk',    'A',    dict(drop_path=0.2, patch_drop=0.25, pos_drop=0.1),   {},                       None),
    ('two-stage',            'plain', 'A',    dict(),                                               {},                       'gathered'),
    ('indexed',              'plain', 'A',    dict(),                                               {},                       'indexed'),
    ('indexed-fold_context', 'plain', 'A',    dict(),                                               {'fold_context': False},  'indexed'),
    ('indexed-droppath',     'plain', 'A',    dict(drop_path=0.2),                                  {},                       'indexed'),
    ('indexed-long',         'plain', 'long', dict(),                                               {},                       'indexed'),
    ('kv_one_launch',        'plain', 'A',    dict(),                                               {'kv_one_launch': True},  None),
    ('w768',                 'plain', 'w768', dict(),                                               {},                       None),
]
OPTION_BF16_ONLY = ('indexed-fold_context', 'kv_one_launch')
OPTION_SHAPES = {'A': (SHAPE_A, BATCH_A, PAIRS_A), 'long': (SHAPE_LONG, BATCH_LONG, PAIRS_LONG), 'w768': (SHAPE_W768, BATCH_A, None)}


def option_case(name, ops):
    """(tree kind, shape, images, pairs, switches, Options, (images' inputs, second images of the pairs, targets)) of an OPTION_CASES
    entry - what the HIP run and the CPU's reference checks of that case both start from."""
    _, kind, shape, what, switches, form = next(c for c in OPTION_CASES if c[0] == name)
    s, batch, table = OPTION_SHAPES[shape]
    if form is None:
        x, y = inputs(s, batch)
        return kind, s, batch, batch, switches, make_options(s, batch, ops=ops, **what), (x[:, 0], x[:, 1], y)
    images, index, x2_index = table
    imgs, y = pair_inputs(s, images, len(index))
    opt = make_options(s, images, len(index), ops=ops, index=index, x2_index=x2_index, indexed=form == 'indexed', **what)
    return kind, s, images, len(index), switches, opt, (imgs, imgs[opt.x2_index], y)
