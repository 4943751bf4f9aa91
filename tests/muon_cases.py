"""Muon as csrc/muon_update.h states it (Jordan et al. 2024, with ``torch.optim.Muon``'s conventions), restated per tensor in plain torch
so that it runs in fp64 and in the kernel's arithmetic, and the operands the Muon tests run on.  With ``c`` the clip coefficient of the
update and ``(a, b, cc)`` the Newton-Schulz coefficients, per tensor ``[rows, cols]`` of a Muon group:

    g'  = g c
    buf = buf + (g' - buf)(1 - momentum)
    u   = g' + (buf - g') momentum   if nesterov else   buf
    X   = bf16(u / max(|u|_F, eps))                       transposed when rows > cols, so that X is [m, n] with m <= n
    k times:  A = bf16(X X^T);  B = bf16(b A + cc A A);  X = bf16(a X + B X)
    O   = X, transposed back when rows > cols
    p   = p (1 - lr wd) - lr adj O
    adj = sqrt(max(1, rows / cols))                       adjust_lr_fn None / 'original'
          0.2 sqrt(max(rows, cols))                       adjust_lr_fn 'match_rms_adamw'

The kernel's arithmetic (``newton_schulz_kernel``): operands are bf16, the products accumulate in fp32, the only roundings to bf16 are at
the three stores, and the fp32 expressions of the two epilogues are SEPARATE rounded operations, never an fma: ``fl(fl(b A) + fl(cc S))``
with ``S = A A`` and ``fl(fl(a X) + T)`` with ``T = B X`` - exactly what torch's fp32 ``*`` and ``+`` do on the CPU.  The order in which a
matrix product adds its terms is the one thing this file cannot restate; the exact-arithmetic operands (``exact_u``) have at most one
non-zero term in every dot product, so that no order can change a bit.  No GPU, no project code."""
import math

import torch

import lamb_cases as lc

NS_COEFFICIENTS = (3.4445, -4.7750, 2.0315)
NS_STEPS = 5
EPS = 1e-7


def adjust(rows, cols, adjust_lr_fn):
    if adjust_lr_fn in (None, 'original'):
        return math.sqrt(max(1, rows / cols))
    assert adjust_lr_fn == 'match_rms_adamw'
    return 0.2 * math.sqrt(max(rows, cols))


def newton_schulz(u, coefficients=NS_COEFFICIENTS, steps=NS_STEPS, eps=EPS, dtype=torch.float64):
    """The iteration without any rounding to bf16, in ``dtype``: O for the momentum ``u`` [rows, cols]."""
    a, b, c = coefficients
    x = u.to(dtype)
    tall = x.shape[0] > x.shape[1]
    if tall:
        x = x.T
    x = x / x.norm().clamp(min=eps)
    for _ in range(steps):
        A = x @ x.T
        B = b * A + c * (A @ A)
        x = a * x + B @ x
    return x.T if tall else x


def newton_schulz_kernel(u, coefficients=NS_COEFFICIENTS, steps=NS_STEPS, eps=EPS):
    """The iteration in the kernel's arithmetic for an fp32 ``u``: O as a bf16 tensor [rows, cols]."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    bf = lambda t: t.bfloat16().float()
    a, b, c = (f32(v) for v in coefficients)
    u = u.float()
    denom = torch.maximum(u.square().sum().sqrt(), f32(eps))
    x = bf(u / denom)
    tall = x.shape[0] > x.shape[1]
    if tall:
        x = x.T.contiguous()
    for _ in range(steps):
        A = bf(x @ x.T)
        B = bf(b * A + c * (A @ A))
        x = bf(a * x + B @ x)
    return (x.T if tall else x).contiguous().bfloat16()


def momentum_step(g, buf, c, momentum, nesterov):
    """(new buf, u) in the dtype of ``buf``."""
    gc = g * c
    buf = buf + (gc - buf) * (1 - momentum)
    return buf, (gc + (buf - gc) * momentum) if nesterov else buf


def update(p, g, buf, c, lr, momentum, nesterov, weight_decay, adjust_lr_fn=None, coefficients=NS_COEFFICIENTS, steps=NS_STEPS, eps=EPS):
    """One Muon update of one tensor without bf16, in the dtype of ``p``: (new p, new buf, O)."""
    buf, u = momentum_step(g, buf, c, momentum, nesterov)
    o = newton_schulz(u, coefficients, steps, eps, p.dtype)
    return p * (1 - lr * weight_decay) - lr * adjust(p.shape[0], p.shape[1], adjust_lr_fn) * o, buf, o


# ---- exact-arithmetic operands ----------------------------------------------------------------------------------------------------------
# (rows, cols): one tile with the K tail in the padding; tall, so transposed; 64 x 96; several Gram tiles and several K steps; 4 x 6.
EXACT_SHAPES = [(16, 40), (72, 16), (64, 96), (256, 320), (4, 6)]


def exact_u(rows, cols, exponent=-3):
    """A signed partial permutation times 2^exponent: one non-zero in every line along the short side, no line along the long side used
    twice.  The short side is a power of four, so |u|_F = sqrt(m) 2^exponent and every scaled entry 1 / sqrt(m) are exact, and every dot
    product of the iteration has at most one non-zero term."""
    m, n = min(rows, cols), max(rows, cols)
    assert math.isqrt(m) ** 2 == m and (math.isqrt(m) & (math.isqrt(m) - 1)) == 0
    x = torch.zeros(m, n)
    for i in range(m):
        x[i, (7 * i + 3) % n if math.gcd(7, n) == 1 else (5 * i + 3) % n] = (1.0 if (i * i + i // 3) % 2 == 0 else -1.0) * 2.0 ** exponent
    assert int((x != 0).sum(dim=0).max()) == 1 and int((x != 0).sum()) == m
    return (x.T if rows > cols else x).contiguous()


# ---- general operands -------------------------------------------------------------------------------------------------------------------
GENERAL_SHAPES = [(65, 67), (128, 64), (130, 4), (48, 96), (64, 256)]


def general_u(rows, cols, seed=0):
    """A closed form of the flat index in the style of lamb_cases.gradients: fp32, full rank, no two equal neighbours."""
    i = torch.arange(rows * cols, dtype=torch.float64)
    flat = 0.004 * torch.sin(0.113 * i + 1.3 * seed + 0.25) * (1.0 + 0.5 * torch.cos(0.0071 * i * (seed + 1))) + 0.001 * torch.cos(2.39 * i * i)
    return flat.float().reshape(rows, cols)


def relative_error(o, o64):
    return float((o.double() - o64).norm() / o64.norm())


def torch_bf16_error(u, coefficients=NS_COEFFICIENTS, steps=NS_STEPS, eps=EPS):
    """e_torch: the error of torch.optim.Muon's own bf16 iteration on the CPU against the fp64 iteration from the same ``u``."""
    from torch.optim._muon import _zeropower_via_newtonschulz
    return relative_error(_zeropower_via_newtonschulz(u.float(), tuple(coefficients), steps, eps), newton_schulz(u, coefficients, steps, eps))


# ---- the bag: lamb_cases.BAG's shapes, the 2-D ones in a Muon group ---------------------------------------------------------------------------
# (4, 6) is all zero under a gradient, (3, 5) never sees a gradient (u = 0: O = 0, only the decay moves it), (2, 3) has p = 0 and g = 0.
IS_MUON = [len(s) == 2 for s in lc.SHAPES]
HYPER = dict(lr=2e-3, momentum=0.95, weight_decay=0.05, betas=(0.9, 0.98), adam_eps=1e-6)
AUX_GROUPS = [dict(weight_decay=0.0), dict(lr=5e-4)]         # lamb_cases' groups 1 (1-D, no decay) and 2 (3-D and 4-D, a rate of its own)


def param_groups(params, **muon_override):
    """``params`` (one per BAG entry, in order) as FlatMuon's groups: the Muon group, then lamb_cases' groups 1 and 2 as aux groups."""
    return [{'params': [p for p, g in zip(params, lc.GROUP_OF) if g == 0], 'use_muon': True, **muon_override},
            {'params': [p for p, g in zip(params, lc.GROUP_OF) if g == 1], **AUX_GROUPS[0]},
            {'params': [p for p, g in zip(params, lc.GROUP_OF) if g == 2], **AUX_GROUPS[1]}]


def run_muon_tensors(dtype=torch.float64, nesterov=True, adjust_lr_fn=None, updates=lc.UPDATES, max_norm=lc.MAX_NORM):
    """``updates`` updates of the bag's Muon tensors without bf16 in ``dtype`` (the clip from ALL gradients of the bag): a list, one
    entry per update, of dict(norm, p_before, p, buf, o) with one item per Muon tensor, in BAG order."""
    idx = [i for i, mu in enumerate(IS_MUON) if mu]
    init = lc.initial_parameters()
    p = [init[i].to(dtype) for i in idx]
    buf = [torch.zeros_like(t) for t in p]
    out = []
    for step in range(updates):
        g = lc.gradients(step)
        norm, c = lc.clip_coef(g, max_norm, dtype)
        before, o = [t.clone() for t in p], [None] * len(p)
        for k, i in enumerate(idx):
            p[k], buf[k], o[k] = update(p[k], g[i].to(dtype), buf[k], c, HYPER['lr'], HYPER['momentum'], nesterov, HYPER['weight_decay'],
                                        adjust_lr_fn)
        out.append(dict(norm=float(norm), p_before=before, p=[t.clone() for t in p], buf=[t.clone() for t in buf], o=o))
    return out
