"""Value-structured operands for the parity tests, their fp64 truth and the elementwise error bounds, and a compact fp32
model of the tiled attention arithmetic.  Plain torch, no GPU dependency: tests/test_structured_cases.py checks it on the CPU,
tests/test_gpu_structured.py drives the kernels with it.

Every attention operand is bf16-representable, so the bf16 and the fp32 kernels and the fp64 truth see the same numbers.
"""
import math

import torch

LOG2E = 1.4426950408889634
ATTENTION_KINDS = ('rising', 'onehot', 'uniform', 'voffset', 'randn')
V_OFFSET = 16.0
# per key tile of 64: how far (nats) the score level of the 'rising' keys moves; the tiled forward moves its reference maximum
# only when a tile maximum exceeds it by more than 8 in log2 units = 8 / log2(e) = 5.545 nats, so both sides are present
RISING_STEPS = (2.0, 5.0, 6.0, 9.0, 3.0, 7.0, 5.5, 12.0)
RISING_QUERY = (1.0, -1.0, 0.5, 0.0, -0.25, 1.0, 0.75, -0.5)   # per query inside every 16-query tile: rising, falling, flat rows
LAZY_NATS = 8.0 / LOG2E


def bf(t):
    """Round to bf16, keep fp32."""
    return t.to(torch.bfloat16).float()


def attention_operands(kind, nq, nk, hd, gen):
    """(q [nq, hd], k [nk, hd], v [nk, hd]) of ONE head, fp32 holding bf16-representable values."""
    randn = lambda *s: torch.randn(*s, generator=gen)
    if kind == 'randn':
        return bf(randn(nq, hd)), bf(randn(nk, hd)), bf(randn(nk, hd))
    if kind == 'rising':
        u = torch.zeros(hd)
        u[:4] = 1.0                                                   # |u|^2 = 4
        ntile = (nk + 63) // 64
        steps = torch.tensor(RISING_STEPS).repeat((ntile + 7) // 8)[:ntile]
        a = torch.cumsum(steps, 0).repeat_interleave(64)[:nk] + 0.5 * torch.rand(nk, generator=gen)
        b = torch.tensor(RISING_QUERY).repeat((nq + 7) // 8)[:nq]
        s = hd ** 0.25 / 2                                            # scale * (a u s) . (b u s) = a b |u|^2 s^2 hd^-1/2 = a b
        k = bf(a[:, None] * u * s + 0.05 * randn(nk, hd))
        q = bf(b[:, None] * u * s + 0.05 * randn(nq, hd))
        return q, k, bf(randn(nk, hd))
    if kind == 'onehot':
        k = bf(3 * randn(nk, hd))
        idx = torch.randint(0, nk, (nq,), generator=gen)
        return bf(1.5 * k[idx]), k, bf(randn(nk, hd))
    if kind == 'uniform':
        k = bf(randn(1, hd)).expand(nk, hd).contiguous()
        return bf(4 * randn(nq, hd)), k, bf(randn(nk, hd))
    if kind == 'voffset':
        return bf(randn(nq, hd)), bf(randn(nk, hd)), bf(V_OFFSET + randn(nk, hd))
    raise ValueError(kind)


def attention_case(kind, batch, kv_batch, heads, nq, nk, hd, seed):
    """q [batch, nq, heads * hd], k, v [kv_batch, nk, heads * hd], do [batch, nq, heads * hd]: every (item, head) its own draw."""
    gen = torch.Generator().manual_seed(seed)
    n = max(batch, kv_batch)
    per = [[attention_operands(kind, nq, nk, hd, gen) for _ in range(heads)] for _ in range(n)]
    stack = lambda i, items: torch.stack([torch.cat([per[b][h][i] for h in range(heads)], -1) for b in range(items)])
    do = bf(torch.randn(batch, nq, heads * hd, generator=gen))
    return stack(0, batch), stack(1, kv_batch), stack(2, kv_batch), do


def _heads(t, heads):
    b, n, d = t.shape
    return t.double().view(b, n, heads, d // heads).transpose(1, 2)       # [B, H, n, hd]


def _merge(t):
    b, h, n, hd = t.shape
    return t.transpose(1, 2).reshape(b, n, h * hd)


def attention_truth(q, k, v, do, heads, scale, unit, kv_index=None):
    """fp64 softmax attention of [B, n, heads * hd] operands and the elementwise bounds of a kernel whose stored
    probabilities / score gradients / outputs carry the relative rounding ``unit`` / 2 each (bf16: unit = 2^-7, fp32
    activations: 2^-18) and whose exponent ``S log2(e) - lse log2(e)`` is evaluated in fp32.

    Returns (truth, bound): dicts over 'o', 'lse', 'dq', 'dk', 'dv' (bound has no 'lse': that one keeps rtol = atol = 1e-4).
      o :  unit * P |V|
      dq:  unit * scale * |dS| |K|  +  eps_i * scale * (sum_j P |dP|) * (P |K|)
      dk:  unit * scale * |dS|^T |Q|  +  scale * (eps_i (sum_j P |dP|) P)^T |Q|
      dv:  unit * P^T |dO|  +  (eps_i P)^T |dO|
    with dS = P o (dP - delta), eps_i = 2^-20 (1 + max_j |S_ij| + |lse_i|): an absolute error of the fp32 exponent in proportion
    to its operands is a relative error of the whole row of P, which the delta subtraction does not cancel.  Each + 1e-6."""
    Q, K, V, dO = (_heads(t, heads) for t in (q, k, v, do))
    if kv_index is not None:
        K, V = K[kv_index], V[kv_index]
    S = (Q @ K.transpose(-1, -2)) * scale
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    dP = dO @ V.transpose(-1, -2)
    delta = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    truth = dict(o=_merge(P @ V), lse=lse, dq=_merge(dS @ K) * scale, dk=_merge(dS.transpose(-1, -2) @ Q) * scale,
                 dv=_merge(P.transpose(-1, -2) @ dO))
    eps = 2.0 ** -20 * (1 + S.abs().amax(-1, keepdim=True) + lse.abs()[..., None])
    w = eps * (P * dP.abs()).sum(-1, keepdim=True)
    bound = dict(
        o=unit * _merge(P @ V.abs()) + 1e-6,
        dq=_merge(unit * scale * (dS.abs() @ K.abs()) + w * scale * (P @ K.abs())) + 1e-6,
        dk=_merge(unit * scale * (dS.abs().transpose(-1, -2) @ Q.abs()) + scale * ((w * P).transpose(-1, -2) @ Q.abs())) + 1e-6,
        dv=_merge(unit * (P.transpose(-1, -2) @ dO.abs()) + (eps * P).transpose(-1, -2) @ dO.abs()) + 1e-6)
    return truth, bound


def ratio(got, truth, bound):
    """max |got - truth| / bound; inf when got holds a NaN / inf."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - truth).abs() / bound).max())


def lse_ratio(got, truth):
    """max |got - truth| / (1e-4 + 1e-4 |truth|): <= 1 is the suite's rtol = atol = 1e-4 on the log-sum-exp."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float(((got - truth).abs() / (1e-4 + 1e-4 * truth.abs())).max())


# ---------------------------------------------------------------------------------------------
# fp32 model of the tiled kernels' arithmetic (one head): 64-key tiles, one wave-uniform branch per 16-query group, the
# reference maximum moving only past + 8 (log2 units), bf16 probabilities into the P V product, bf16 output
# ---------------------------------------------------------------------------------------------
def model_fwd(q, k, v, scale, rescale_l=True):
    """-> (o bf16-rounded, lse, number of rescales with a finite old maximum per 16-query group).  ``rescale_l=False`` is the
    mutant that forgets l *= alpha."""
    nq, hd = q.shape
    nk = k.shape[0]
    sc = scale * LOG2E
    group = torch.arange(nq) // 16
    ngroups = int(group[-1]) + 1
    m = torch.full((nq,), -math.inf)
    l = torch.zeros(nq)
    o = torch.zeros(nq, hd)
    rescales = torch.zeros(ngroups, dtype=torch.int64)
    for t0 in range(0, nk, 64):
        s = q @ k[t0:t0 + 64].t()
        tmax = s.max(1).values * sc
        wants = (tmax > m + 8).long()
        taken = (torch.zeros(ngroups, dtype=torch.int64).index_add_(0, group, wants) > 0)[group]    # __any over the group
        mn = torch.where(taken, torch.maximum(m, tmax), m)
        alpha = torch.exp2(m - mn)                     # 1 where the branch is not taken; 0 on the first tile (m = -inf)
        alpha = torch.where(taken, alpha, torch.ones_like(alpha))
        if t0 > 0:
            rescales.index_add_(0, group, (alpha < 1).long())
        if rescale_l:
            l = l * alpha
        o = o * alpha[:, None]
        m = mn
        p = torch.exp2(s * sc - m[:, None])
        l = l + p.sum(1)
        o = o + bf(p) @ v[t0:t0 + 64]
    return bf(o / l[:, None]), (m + torch.log2(l)) * math.log(2), rescales


def model_bwd(q, k, v, o_bf, do, lse, scale, corr_sign=1.0):
    """dQ with delta estimated from the saved bf16 O and corrected at the end by the exact one (``corr_sign=-1``: the mutant that
    adds the correction); dK, dV with the exact delta; bf16 P and dS operands, bf16 outputs.  -> (dq, dk, dv)."""
    p = torch.exp2((q @ k.t()) * (scale * LOG2E) - (lse * LOG2E)[:, None])
    dp = do @ v.t()
    estimate = (o_bf * do).sum(1)
    exact = (p * dp).sum(1)
    dq = bf(p * (dp - estimate[:, None])) @ k - corr_sign * (exact - estimate)[:, None] * (bf(p) @ k)
    ds = bf(p * (dp - exact[:, None]))
    return bf(dq * scale), bf((ds.t() @ q) * scale), bf(bf(p).t() @ do)


def tile_steps(q, k, scale):
    """Tile-to-tile differences (nats) of every query's per-64-key-tile score maximum: [nq, ntiles - 1]."""
    s = (q.double() @ k.double().t()) * scale
    tiles = [s[:, t0:t0 + 64].amax(1) for t0 in range(0, k.shape[0], 64)]
    return torch.stack(tiles, 1).diff(dim=1)


# ---------------------------------------------------------------------------------------------
# LayerNorm rows
# ---------------------------------------------------------------------------------------------
LN_CONSTANTS = (3.0, -0.5, 1024.0)      # few mantissa bits: the fp32 row sum is exact, y = beta and rstd = eps^-1/2 as in fp64
LN_KINDS = ('mean1024', 'randn', 'spike', 'const0', 'randn', 'const1', 'mean1024', 'const2', 'spike', 'randn')


def layernorm_rows(rows, dim, seed):
    """fp32 [rows, dim] mixing, row by row (kind of row i = LN_KINDS[i % 10]):
      mean1024  1024 + round(8 randn) / 8: 13-bit values, the fp32 sum of a row is exact in any order;
      spike     randn with one channel set to 300;
      const*    one of LN_CONSTANTS everywhere;
      randn     ordinary rows in between.
    -> (x, kinds) with kinds a list of names per row."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, dim, generator=gen)
    kinds = [LN_KINDS[i % len(LN_KINDS)] for i in range(rows)]
    for i, kind in enumerate(kinds):
        if kind == 'mean1024':
            x[i] = 1024 + torch.round(8 * x[i]) / 8
        elif kind == 'spike':
            x[i, (7 * i) % dim] = 300.0
        elif kind.startswith('const'):
            x[i] = LN_CONSTANTS[int(kind[-1])]
    return x, kinds


def layernorm_bwd_ref(dy, x, gamma, mean, rstd):
    """fp64 LayerNorm backward AT THE GIVEN statistics (the fp32 numbers the kernel is handed, not the row's exact ones):
    xhat = (x - mean) rstd, g = dy gamma, dx = rstd (g - mean_c(g) - xhat mean_c(g xhat)), dgamma = sum_rows dy xhat,
    dbeta = sum_rows dy.  Equal to autograd through F.layer_norm when mean / rstd are the row's own.  -> (dx, dgamma, dbeta)."""
    dy, x, gamma, mean, rstd = (t.double() for t in (dy, x, gamma, mean, rstd))
    xhat = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    dx = rstd[:, None] * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    return dx, (dy * xhat).sum(0), dy.sum(0)


def ulp32(t):
    """fp32 unit in the last place at |t| (t fp64)."""
    return torch.exp2(torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -126))) - 23)


# ---------------------------------------------------------------------------------------------
# GELU grid
# ---------------------------------------------------------------------------------------------
def gelu_grid():
    """Pre-activation values, fp32 and bf16-representable: 0, -0, +-2^-20, a dense grid over [-12, 12], +-30, +-1e4 (rounded)."""
    dense = bf(torch.arange(-12 * 64, 12 * 64 + 1, dtype=torch.float32) / 64)      # step 2^-6, rounded where bf16 is coarser
    edge = torch.tensor([0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 30.0, -30.0, 1e4, -1e4])
    return torch.cat([bf(edge), dense])


def gelu_ref(z):
    """fp64 (gelu(z), gelu'(z))."""
    z = z.double()
    cdf = 0.5 * torch.erfc(-z / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    return z * cdf, cdf + z * pdf
