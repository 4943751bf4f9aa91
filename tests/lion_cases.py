"""Lion as csrc/optim_update.h states it (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms", with timm's ``Lion``
conventions), restated per tensor in plain torch so that it runs in fp64 and in fp32, on the parameter bag of tests/lamb_cases.py (its
parameters, gradients, groups, ``UPDATES`` and ``MAX_NORM``; betas (0.9, 0.98)).  With ``c`` the clip coefficient of the update:

    g' = g c
    pe = p (1 - lr wd)
    cc = b1 m + (1 - b1) g'
    s  = sign(cc)                  +1, -1, 0 for cc == 0 (torch.sign)
    p' = pe - lr s
    m' = m + (g' - m)(1 - b2)

Every line above is one torch operation per arithmetic operation, every constant a 0-dim tensor of the run's dtype: in fp32 each product
and each sum is rounded on its own, which is the rule the kernel is pinned to, so the fp32 run gives the kernel's bits when it is handed
the kernel's own gradient norms.

The sign makes the fp64 comparison conditional.  An element is NEAR A TIE in an update if

    0 < |cc| <= TIE (|b1 m| + |(1 - b1) g'|),  TIE = 2^-16

in the fp64 run: there, and only there, fp32 rounding (2^-24 per operation, a few operations) may decide the sign differently and move
the parameter the other way by 2 lr.  ``near_tie`` gives the elements that are ever near a tie; the tests cap their share at
``TIE_SHARE`` and compare the others.  No GPU, no project code."""
import torch

import lamb_cases as lc

BAG, SHAPES, KINDS, GROUP_OF, NUMEL, TOTAL = lc.BAG, lc.SHAPES, lc.KINDS, lc.GROUP_OF, lc.NUMEL, lc.TOTAL
UPDATES, MAX_NORM = lc.UPDATES, lc.MAX_NORM
HYPER = dict(lr=lc.HYPER['lr'], betas=lc.HYPER['betas'], weight_decay=lc.HYPER['weight_decay'])      # lr 2e-3, betas (0.9, 0.98), wd 0.05
TIE = 2.0 ** -16
TIE_SHARE = 1e-3                   # at most 0.1 % of the bag's elements may ever be near a tie


def group_settings(gi, **override):
    s = lc.group_settings(gi, **override)
    return dict(lr=s['lr'], betas=s['betas'], weight_decay=s['weight_decay'])


def param_groups(params, **override):
    return lc.param_groups(params, **override)


def clip_from_norm(norm, max_norm, dtype):
    """c of ``clip_grad_norm_`` from a given norm, in ``dtype``, operation for operation as optim_clip_coef takes it."""
    norm = torch.as_tensor(norm, dtype=dtype)
    if not (max_norm and max_norm > 0):
        return torch.ones((), dtype=dtype)
    c = torch.tensor(max_norm, dtype=dtype) / (norm + torch.tensor(1e-6, dtype=dtype))
    return torch.minimum(c, torch.ones((), dtype=dtype))


def update(p, g, m, c, lr, betas, weight_decay):
    """One Lion update of one tensor in the dtype of ``p``: (new p, new m, cc, |b1 m| + |(1 - b1) g'|)."""
    dt = p.dtype
    lr, b1, b2, wd = (torch.tensor(float(x), dtype=dt) for x in (lr, betas[0], betas[1], weight_decay))
    one, c = torch.ones((), dtype=dt), torch.as_tensor(c, dtype=dt)
    gc = g * c
    product = lr * wd
    decay = one - product
    pe = p * decay
    keep = b1 * m
    take = (one - b1) * gc
    cc = keep + take
    step = lr * torch.sign(cc)
    pn = pe - step
    diff = gc - m
    scaled = diff * (one - b2)
    mn = m + scaled
    return pn, mn, cc, keep.abs() + take.abs()


def run(dtype=torch.float64, updates=UPDATES, max_norm=MAX_NORM, norms=None, **override):
    """``updates`` updates of the bag in ``dtype``: one dict(norm, p, m, cc, scale) per update, one item per BAG entry in each list.
    ``norms`` (one per update): take the clip coefficient from these norms - the kernel's own - instead of the run's."""
    p = [t.to(dtype) for t in lc.initial_parameters()]
    m = [torch.zeros_like(t) for t in p]
    out = []
    for step in range(updates):
        g = lc.gradients(step)
        norm = lc.clip_coef(g, max_norm, dtype)[0] if norms is None else torch.as_tensor(norms[step], dtype=dtype)
        c = clip_from_norm(norm, max_norm, dtype)
        cc, scale = [None] * len(p), [None] * len(p)
        for i in range(len(p)):
            p[i], m[i], cc[i], scale[i] = update(p[i], g[i].to(dtype), m[i], c, **group_settings(GROUP_OF[i], **override))
        out.append(dict(norm=float(norm), p=[t.clone() for t in p], m=[t.clone() for t in m], cc=cc, scale=scale))
    return out


def near_tie(records):
    """One bool tensor per BAG entry: the element was near a tie in some update of ``records`` (an fp64 run)."""
    out = [torch.zeros(s, dtype=torch.bool) for s in SHAPES]
    for rec in records:
        for i, (cc, scale) in enumerate(zip(rec['cc'], rec['scale'])):
            out[i] |= (cc.abs() > 0) & (cc.abs() <= TIE * scale)
    return out
