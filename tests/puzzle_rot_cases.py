"""The rule of the learned type-2 puzzle path in numpy, and the inputs its tests share.

Sides: top 0, right 1, bottom 2, left 3, clockwise.  A turn k is k clockwise quarter turns, ``numpy.rot90(x, -k)`` over the two pixel
axes; the border that was side s becomes side (s + k) % 4.  The model scores the pair (piece i, turn_k(piece j)); bin b of its four
logits speaks of side si = (b + 1) % 4 of piece i (the type-1 rule: side s reads bin (s + 3) % 4) against the side of the turned j that
faces it, (si + 2) % 4, which is side sj = (si + 2 - k) % 4 of the upright j."""
import numpy as np

DQ_UNSET = 2 ** 31 - 1


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def turn(x, k, axes=(-2, -1)):
    return np.rot90(x, -k, axes=axes)


def moved_side(s, k):
    return (s + k) % 4


def pair_turn(si, sj):
    """The turn of piece j under which its side sj faces side si of piece i."""
    return (si + 2 - sj) % 4


def bin_sides(k, b):
    """(si, sj) that bin b of the pair (i, turn_k(j)) fills."""
    si = (b + 1) % 4
    return si, (si + 2 - k) % 4


def side_line(x, s):
    """The border line of side s of x [..., S, S]."""
    return (x[..., 0, :], x[..., :, -1], x[..., -1, :], x[..., :, 0])[s]


def quantise(logits):
    """evaluation.py:118-133 into inter_piece_distance.py:206-223: numpy float32 throughout, truncation by the uint32 store."""
    x = np.asarray(logits, np.float32)
    sig = (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)
    return ((np.float32(1) - sig) * np.float32(1000.)).astype(np.float32).astype(np.uint32)


def dq2_from_logits(logits):
    """Dq2 int64 [4, n, n, 4] of logits fp32 [n, n, 4, 4] indexed [i, j, k, bin]: the rule as the issue states it, entry by entry."""
    n = logits.shape[0]
    dq2 = np.full((4, n, n, 4), DQ_UNSET, np.int64)
    q = quantise(logits).astype(np.int64)
    off = ~np.eye(n, dtype=bool)
    for si in range(4):
        for sj in range(4):
            dq2[si, :, :, sj][off] = q[:, :, pair_turn(si, sj), (si + 3) % 4][off]
    return dq2


def scatter(n, logits, pi, pjt, dq2=None):
    """What vited_puzzle_distances2_from_logits does to dq2 (default: all unset), pair by pair and bin by bin; returns (dq2, the number of
    pairs refused)."""
    dq2 = np.full((4, n, n, 4), DQ_UNSET, np.int64) if dq2 is None else dq2
    q = quantise(logits).astype(np.int64)
    refused = 0
    for r, (i, jt) in enumerate(zip(pi.tolist(), pjt.tolist())):
        if not (0 <= i < n and 0 <= jt < 4 * n) or jt % n == i:
            refused += 1
            continue
        for b in range(4):
            si, sj = bin_sides(jt // n, b)
            dq2[si, i, jt % n, sj] = q[r, b]
    return dq2, refused


def patch_rows(img, patch):
    """[B, C, S, S] -> [B * (S / p)^2, C p p]: the im2col of the patch embedding, whatever the dtype."""
    b, c, s, _ = img.shape
    g = s // patch
    return img.reshape(b, c, g, patch, g, patch).transpose(0, 2, 4, 1, 3, 5).reshape(b * g * g, c * patch * patch)


# ---- logits whose quantisation does not hang on the last bit of exp ----------------------------------------------------------------------
def stable(logits, ulps=2):
    """True where the quantisation of a logit is the same for every exp(-x) within ``ulps`` fp32 steps of numpy's: such a logit has one
    right answer whatever faithful single-precision exp computes it - the device's expf and numpy's differ in the last bit on some inputs
    - so the kernel is compared on it exactly."""
    x = np.asarray(logits, np.float32)
    e0 = np.exp(-x).astype(np.float32)
    want = quantise(x)
    ok = np.ones(x.shape, bool)
    exact = x == 0                      # exp(+-0) is 1 in every implementation: nothing to perturb
    for direction in (-np.inf, np.inf):
        e = e0.copy()
        for _ in range(ulps):
            e = np.nextafter(e, np.float32(direction)).astype(np.float32)
            sig = (np.float32(1) / (np.float32(1) + e)).astype(np.float32)
            ok &= ((np.float32(1) - sig) * np.float32(1000.)).astype(np.float32).astype(np.uint32) == want
    return ok | exact


def near_integer_logits():
    """fp32 logits whose fp32(fp32(1 - sigmoid) * 1000) lies within one fp32 step of an integer - on it, one step below (truncates to the
    integer before) and one step above - and is ``stable``.  Found where the value is insensitive to exp's last bits: for x << 0 the
    sigmoid is small, and its rounding error vanishes under the rounding of 1 - sigmoid.  A scan of fp32 neighbours of the real-valued
    solution, in a fixed order: no random numbers."""
    found = []
    for m in range(901, 1000, 7):
        lo = np.float32(np.log(1000.0 / m - 1.0))            # (1 - sigmoid(x)) * 1000 = m
        for _ in range(2000):
            lo = np.nextafter(lo, np.float32(-np.inf))
        xs = [lo]
        for _ in range(4000):
            xs.append(np.nextafter(xs[-1], np.float32(np.inf)))
        xs = np.array(xs, np.float32)
        sig = (np.float32(1) / (np.float32(1) + np.exp(-xs))).astype(np.float32)
        v = ((np.float32(1) - sig) * np.float32(1000.)).astype(np.float32)
        target = np.float32(m)
        for want in (np.nextafter(target, np.float32(0)), target, np.nextafter(target, np.float32(2000))):
            hit = np.flatnonzero((v == want) & stable(xs))
            if hit.size:
                found.append(xs[hit[0]])
    return np.array(found, np.float32)


def scatter_logits(count, seed):
    """``count`` x 4 fp32 logits for the scatter test: the corner values (+-40: distances 0 and 1000; +-0: 500), every near-integer
    logit, and stable draws of N(0, 4) behind them."""
    fixed = np.concatenate([np.float32([40., -40., 0., -0., 30., -30., 8., -8.]), near_integer_logits()])
    rng = np.random.default_rng(seed)
    draws = rng.normal(0, 4, size=8 * count + 64).astype(np.float32)
    draws = draws[stable(draws)]
    flat = np.concatenate([fixed, draws])
    reps = -(-4 * count // flat.size)
    return np.tile(flat, reps)[:4 * count].reshape(count, 4), fixed.size


def all_pairs(n):
    """(pi, pjt) of every pair (i, j != i) under every turn, k-major."""
    ii, jj = np.nonzero(~np.eye(n, dtype=bool))
    return np.tile(ii, 4).astype(np.int64), np.concatenate([k * n + jj for k in range(4)]).astype(np.int64)


# ---- pieces ----------------------------------------------------------------------------------------------------------------------------
def border_piece(size):
    """[size, size]: the four borders carry the four values 10 (top), 20 (right), 30 (bottom), 40 (left); corners 0, inside 99."""
    x = np.full((size, size), 99, np.int64)
    x[0, :], x[:, -1], x[-1, :], x[:, 0] = 10, 20, 30, 40
    x[0, 0] = x[0, -1] = x[-1, 0] = x[-1, -1] = 0
    return x


def pattern_pieces(n, size):
    """uint8 [n, 3, size, size], closed form, no symmetry under a quarter or half turn: a ramp along each axis with a different slope per
    channel and piece, a diagonal wave, and one bright corner block."""
    y, x = np.meshgrid(np.arange(size), np.arange(size), indexing='ij')
    out = np.zeros((n, 3, size, size), np.float64)
    for i in range(n):
        for c in range(3):
            out[i, c] = (40 + 150 * y / size * (0.3 + 0.2 * c) + 90 * x / size * (0.9 - 0.25 * c)
                         + 35 * np.sin(0.31 * (i + 1) * x + 0.17 * (c + 2) * y + i) + 20 * ((i + c) % 3))
            out[i, c, :size // 4, size // 2:] += 60 - 15 * c
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


# ---- the small model ---------------------------------------------------------------------------------------------------------------------
def small_shape(img_size):
    from oracle import vited_oracle as vo
    return vo.ViTEDShape(img_size=img_size, patch_size=8, embed_dim=192, num_heads=6, depth=2, c_depth=2, num_classes=4)


def small_oracle(img_size, seed=7, weight_scale=1.0, head_scale=1.0):
    """The fp32 CPU oracle of the small model with random weights; ``weight_scale`` multiplies every matrix of the attention and MLP
    branches (the random initialisation alone leaves the logits nearly blind to the image), ``head_scale`` the head's."""
    import torch
    from oracle import vited_oracle as vo
    torch.manual_seed(seed)
    m = vo.OracleViTED(small_shape(img_size)).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 2 and not name.startswith('head'):
                p.mul_(weight_scale)
        m.head.weight.mul_(head_scale)
    return m


def hip_model(vited, oracle, dev, dtype):
    s = oracle.shape
    m = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, num_classes=s.num_classes, embed_dim=s.embed_dim,
                                      depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads).to(dev)
    m.load_state_dict(oracle.state_dict())
    m.compute_dtype = dtype
    return m.eval()


def normalise(pieces_u8):
    """ToTensor + Normalize(0.5, 0.5): what the uint8 path does on the device."""
    import torch
    return (torch.as_tensor(pieces_u8).float() / 255 - 0.5) / 0.5


def turned_logits_oracle(oracle, pieces_u8):
    """fp32 [n, n, 4, 4] ([i, j, k, bin]) by the rule itself on the CPU oracle: the stacked pair (piece i, turn_k(piece j))."""
    import torch
    n = pieces_u8.shape[0]
    x = normalise(pieces_u8)
    out = torch.zeros(n, n, 4, 4)
    with torch.no_grad():
        feats = oracle(x, forward_first_part=True)
        for k in range(4):
            xk = torch.rot90(x, -k, (2, 3)).contiguous()
            for i in range(n):
                out[i, :, k] = oracle(feats[i:i + 1].expand(n, -1, -1), xk)
    out[torch.arange(n), torch.arange(n)] = 0
    return out.numpy()


def turn_separation(logits, n):
    """min over (i, j != i) and pairs of different turns of the largest |difference| over the four bins; logits [n, n, 4, 4]."""
    worst = np.inf
    for k in range(4):
        for l in range(k + 1, 4):
            gap = np.abs(logits[:, :, k] - logits[:, :, l]).max(axis=-1)
            worst = min(worst, gap[~np.eye(n, dtype=bool)].min())
    return float(worst)
