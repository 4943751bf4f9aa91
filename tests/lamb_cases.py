"""LAMB as csrc/optim_update.h states it (You et al. 2020, Algorithm 2, with timm's ``Lamb`` conventions), restated per tensor in plain
torch so that it runs in fp64 and in fp32, and the small parameter bag the LAMB tests run on.  With ``c`` the clip coefficient of the
update and ``t`` the count of applied updates:

    g' = g c
    m  = m + (g' - m)(1 - b1)
    v  = b2 v + (1 - b2) g' g'
    u  = (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps) + wd p
    r  = 1                                           if wd == 0 and not always_adapt
         (|p| > 0 and |u| > 0) ? |p| / |u| : 1       otherwise; with trust_clip: min(r, 1)
    p  = p - lr r u

``|.|`` is the 2-norm over the whole tensor; the clip is ``clip_grad_norm_``'s: ``c = min(1, max_norm / (norm + 1e-6))`` over all gradients.
No GPU, no project code."""
import math

import torch

# (shape, kind, group).  Shapes: the smallest at which the 64 x 64 tile kernels can go wrong - 1-D parameters with tails; tails in both
# tile dimensions and rows that are not 16-byte aligned (65 x 67: 4 tiles); exact tiles on the vector path (128 x 64: 2 tiles); narrow
# tiles (130 x 4: 3 tiles); 3-D like pos_embed; 4-D like the patch projection.  Kinds: 'zero_p' is all zero under a non-zero gradient
# (|p| = 0, so r = 1 in the first update), 'zero_g' never sees a gradient (m = v = 0, u = wd p, r = 1 / wd), 'zero_both' has p = 0 and
# g = 0 (|u| = 0, r = 1, nothing non-finite).
BAG = [
    ((65, 67), 'plain', 0), ((128, 64), 'plain', 0), ((130, 4), 'plain', 0), ((4, 6), 'zero_p', 0), ((3, 5), 'zero_g', 0),
    ((2, 3), 'zero_both', 0),
    ((1,), 'plain', 1), ((3,), 'plain', 1), ((64,), 'plain', 1), ((130,), 'plain', 1),
    ((1, 5, 8), 'plain', 2), ((8, 3, 2, 2), 'plain', 2),
]
SHAPES = [b[0] for b in BAG]
KINDS = [b[1] for b in BAG]
GROUP_OF = [b[2] for b in BAG]
NUMEL = [math.prod(s) for s in SHAPES]
TOTAL = sum(NUMEL)
# three groups: decayed, the 1-D group without decay (no trust ratio unless always_adapt), and one with a rate of its own.
# lr, betas and weight_decay are those of the AdamW and SGD parity tests (tests/test_gpu_engine.py, tests/test_gpu_optim_sgd.py).  The
# betas matter: the kernels hold every group word in fp32, and 1 - fl32(0.999) differs from 0.001 by 1.3e-5 of it - which exp_avg_sq of
# FlatAdamW and FlatLAMB alike inherits, past the rtol of 1e-5 those tests hold the moments to - while 1 - fl32(0.98) is 1e-6 off 0.02.
HYPER = dict(lr=2e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.05)
GROUPS = [dict(), dict(weight_decay=0.0), dict(lr=5e-4)]
UPDATES = 5
MAX_NORM = 1.0
GRAD_SCALE = [0.004, 3.0, 0.004, 0.5, 0.004]       # norms of about 0.4, 3e2, 0.4, 5e1, 0.4: the clip at 1.0 bites in updates 1 and 3 only


def group_settings(gi, **override):
    """lr, betas, eps, weight_decay of group ``gi``; ``override`` (e.g. weight_decay=0.0) wins over the group's own."""
    return {**HYPER, **GROUPS[gi], **override}


def param_groups(params, **override):
    """``params`` (one per BAG entry, in order) as optimizer param groups."""
    return [{'params': [p for p, g in zip(params, GROUP_OF) if g == gi], **GROUPS[gi], **override} for gi in range(len(GROUPS))]


def index_in_groups():
    """BAG position -> index in the optimizer's ``state_dict`` (parameters counted group after group)."""
    order = [i for gi in range(len(GROUPS)) for i in range(len(BAG)) if GROUP_OF[i] == gi]
    return {i: k for k, i in enumerate(order)}


def initial_parameters():
    """fp32 tensors of SHAPES: a closed form of the flat index, magnitudes of trained weights (|p| <= 0.12), no two equal neighbours."""
    i = torch.arange(TOTAL, dtype=torch.float64)
    flat = (0.1 * torch.sin(0.37 * i + 0.5) + 0.02 * torch.cos(1.91 * i)).float()
    out, at = [], 0
    for shape, kind, n in zip(SHAPES, KINDS, NUMEL):
        t = flat[at: at + n].reshape(shape).clone()
        out.append(torch.zeros_like(t) if kind in ('zero_p', 'zero_both') else t)
        at += n
    return out


def gradients(step):
    """The fp32 gradients of update ``step`` (0-based), one per BAG entry: a closed form of the flat index, fresh for every update."""
    i = torch.arange(TOTAL, dtype=torch.float64)
    flat = (GRAD_SCALE[step] * torch.sin(0.113 * i + 1.3 * step + 0.25) * (1.0 + 0.5 * torch.cos(0.0071 * i * (step + 1)))).float()
    out, at = [], 0
    for shape, kind, n in zip(SHAPES, KINDS, NUMEL):
        t = flat[at: at + n].reshape(shape).clone()
        out.append(torch.zeros_like(t) if kind in ('zero_g', 'zero_both') else t)
        at += n
    return out


def clip_coef(grads, max_norm, dtype):
    """(norm, c) of ``clip_grad_norm_`` over ``grads``, computed in ``dtype``."""
    norm = torch.sqrt(sum((g.to(dtype) ** 2).sum() for g in grads))
    c = torch.ones((), dtype=dtype)
    if max_norm and max_norm > 0:
        c = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return norm, c


def update(p, g, m, v, t, c, lr, betas, eps, weight_decay, always_adapt=False, trust_clip=False):
    """One LAMB update of one tensor, in the dtype of ``p``: (new p, new m, new v, r as a Python float)."""
    b1, b2 = betas
    gc = g * c
    m = m + (gc - m) * (1 - b1)
    v = b2 * v + (1 - b2) * gc * gc
    u = (m / (1 - b1 ** t)) / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps) + weight_decay * p
    if weight_decay == 0 and not always_adapt:
        r = 1.0
    else:
        pn, un = float(p.norm()), float(u.norm())
        r = pn / un if pn > 0 and un > 0 else 1.0
        if trust_clip:
            r = min(r, 1.0)
    return p - lr * r * u, m, v, r


def run(dtype=torch.float64, updates=UPDATES, max_norm=MAX_NORM, always_adapt=False, trust_clip=False, **override):
    """``updates`` updates of the bag in ``dtype``: a list, one entry per update, of dict(norm, p, m, v, r) with one item per BAG entry."""
    p = [t.to(dtype) for t in initial_parameters()]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    out = []
    for step in range(updates):
        g = gradients(step)
        norm, c = clip_coef(g, max_norm, dtype)
        r = [None] * len(p)
        for i in range(len(p)):
            s = group_settings(GROUP_OF[i], **override)
            p[i], m[i], v[i], r[i] = update(p[i], g[i].to(dtype), m[i], v[i], step + 1, c, s['lr'], s['betas'], s['eps'], s['weight_decay'],
                                            always_adapt, trust_clip)
        out.append(dict(norm=float(norm), p=[t.clone() for t in p], m=[t.clone() for t in m], v=[t.clone() for t in v], r=list(r)))
    return out
