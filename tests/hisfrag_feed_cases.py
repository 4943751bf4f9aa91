"""Test-side restatement of the HisFrag device feed (hisfrag.py:63-81) in plain numpy and Python floats, and
the case tables the GPU tests launch.  No GPU dependency and no use of the product's code: tests/test_hisfrag_feed.py checks the
restatement against Pillow and against slices it can state without any package, tests/test_gpu_hisfrag_feed.py holds the kernels
to it bit for bit.

Geometry, per window pixel (x, y), X = x + left, Y = y + top, (top, left) in unpadded image coordinates (may be negative):
  A(u, v)   the image after RandomAffine: 0 outside [0, W) x [0, H); with the affine off src[v][u]; with it on Pillow's 16.16
            nearest transform, xi = (a2 + u a0 + v a1) >> 16, yi = (a5 + u a3 + v a4) >> 16, src[yi][xi] if inside, else 0;
  T(u, v)   the image after ShiftScaleRotate: 0 outside the image; with the warp off A(u, v); with it on cv2's 1/32-pixel 15-bit
            scheme of section 16 (tests/div2k_feed_cases.py) over the four taps A(u0 + i, v0 + j), 0 where a tap is outside.
Colour jitter, blur: see the functions below, each a literal restatement of Pillow's C (jitter) and of the section 17 text (blur).
"""
import math

import numpy as np

from div2k_feed_cases import fixed1024, forward_matrix, invert_affine, round_half_even

AFFINE, WARP, JITTER, BLUR = 1, 2, 4, 8
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
IDENTITY_FIX = (65536, 0, 32768, 0, 65536, 32768)
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
F32 = np.float32


# ---------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------
def fix16(t):
    """Pillow's FIX: floor(t * 65536.0 + 0.5) on a double."""
    return int(math.floor(float(t) * 65536.0 + 0.5))


def affine_fixed(M):
    """The six 16.16 coefficients Pillow's affine_fixed derives from the output -> input matrix M (pixel centres folded into a2, a5)."""
    M = [float(v) for v in M]
    return [fix16(M[0]), fix16(M[1]), fix16(M[2] + M[0] * 0.5 + M[1] * 0.5), fix16(M[3]), fix16(M[4]), fix16(M[5] + M[3] * 0.5 + M[4] * 0.5)]


def inverse_affine_matrix(W, H, angle_deg, tx, ty):
    """torchvision's _get_inverse_affine_matrix for scale 1, no shear, centre (0.5 W, 0.5 H)."""
    r = math.radians(angle_deg)
    a, b, c, d = math.cos(r), -math.sin(r), math.sin(r), math.cos(r)
    cx, cy = W * 0.5, H * 0.5
    m = [d, -b, 0.0, -c, a, 0.0]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def stage_a(src, flags, afix, u, v):
    """A(u, v) for int64 arrays u, v: (values int64 [..., 3], mask of the lookups that were not zero-filled)."""
    H, W, _ = src.shape
    ok = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    xi, yi = u, v
    if flags & AFFINE:
        a0, a1, a2, a3, a4, a5 = (int(t) for t in afix)
        xi = (a2 + u * a0 + v * a1) >> 16
        yi = (a5 + u * a3 + v * a4) >> 16
        ok = ok & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
    val = src[np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1), :] * ok[..., None]
    return val, ok


def affine_ref(img, afix):
    """The whole image after the affine stage, uint8 [H, W, 3]: what Image.transform(size, AFFINE, M, NEAREST, fillcolor=0) gives."""
    H, W, _ = img.shape
    v, u = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing='ij')
    return stage_a(img.astype(np.int64), AFFINE, afix, u, v)[0].astype(np.uint8)


def window_ref(img, flags, afix, minv, top, left, S, want_touch=False):
    """One sample: img uint8 [H, W, 3] -> uint8 [3, S, S].  With ``want_touch`` also whether any lookup was zero-filled."""
    H, W, _ = img.shape
    src = img.astype(np.int64)
    ys = np.arange(S, dtype=np.int64) + int(top)
    xs = np.arange(S, dtype=np.int64) + int(left)
    X, Y = np.broadcast_to(xs[None, :], (S, S)), np.broadcast_to(ys[:, None], (S, S))
    here = (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
    if flags & WARP:
        m = [np.float64(t) for t in minv]
        xf = fixed1024(m[0] * xs.astype(np.float64))[None, :] + fixed1024(m[1] * ys.astype(np.float64) + m[2])[:, None] + 16
        yf = fixed1024(m[3] * xs.astype(np.float64))[None, :] + fixed1024(m[4] * ys.astype(np.float64) + m[5])[:, None] + 16
        xq, yq = xf >> 5, yf >> 5
        u0, a, v0, b = xq >> 5, (xq & 31)[..., None], yq >> 5, (yq & 31)[..., None]
        p00, k00 = stage_a(src, flags, afix, u0, v0)
        p01, k01 = stage_a(src, flags, afix, u0 + 1, v0)
        p10, k10 = stage_a(src, flags, afix, u0, v0 + 1)
        p11, k11 = stage_a(src, flags, afix, u0 + 1, v0 + 1)
        acc = (32 - a) * (32 - b) * 32 * p00 + a * (32 - b) * 32 * p01 + (32 - a) * b * 32 * p10 + a * b * 32 * p11
        val = ((acc + 16384) >> 15) * here[..., None]           # the pad comes after the warp: outside the image it is 0
        filled = ~here | ~(k00 & k01 & k10 & k11)
    else:
        val, ok = stage_a(src, flags, afix, X, Y)
        filled = ~ok
    out = np.ascontiguousarray(val.astype(np.uint8).transpose(2, 0, 1))
    return (out, bool(filled.any())) if want_touch else out


def windows_ref(images, image, flags, afix, minv, origin, S):
    """A batch with in-range image indices: uint8 [B, 3, S, S]."""
    return np.stack([window_ref(images[int(image[k])], int(flags[k]), afix[k], minv[k], int(origin[k][0]), int(origin[k][1]), S)
                     for k in range(len(image))])


# ---------------------------------------------------------------------------------------------
# colour jitter: Pillow's ImageEnhance.Brightness / Contrast / Color and its HSV conversions
# ---------------------------------------------------------------------------------------------
def blend(d, p, f):
    """Image.blend(degenerate, image, f) per byte: int arrays d, p, fp32 factor; separate multiply and add in fp32."""
    f = F32(f)
    d32, p32 = np.asarray(d).astype(F32), np.asarray(p).astype(F32)
    t = d32 + f * (p32 - d32)
    if F32(0) <= f <= F32(1):
        return t.astype(np.int64)                                # truncation
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.where((t > 0) & (t < 255), t, 0).astype(np.int64)))


def luma(rgb):
    """convert('L') of int64 [3, ...]."""
    return (rgb[0] * 19595 + rgb[1] * 38470 + rgb[2] * 7471 + 32768) >> 16


def contrast_mean(rgb):
    """int(ImageStat.Stat(convert('L')).mean[0] + 0.5)."""
    lum = luma(rgb)
    return int(math.floor(float(int(lum.sum())) / float(lum.size) + 0.5))


def rgb_to_hsv(r, g, b):
    """Pillow's rgb2hsv_row on int arrays: (H, S, V) int64 arrays."""
    r, g, b = (np.asarray(t, dtype=np.int64) for t in (r, g, b))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = mx == mn
    with np.errstate(divide='ignore', invalid='ignore'):
        cr = (mx - mn).astype(F32)
        s = np.clip(((cr / mx.astype(F32)) * F32(255.0)).astype(np.int64), 0, 255)
        rc, gc, bc = (mx - r).astype(F32) / cr, (mx - g).astype(F32) / cr, (mx - b).astype(F32) / cr
        h_r = bc - gc                                                                      # fp32
        h_g = ((2.0 + rc.astype(np.float64)) - bc.astype(np.float64)).astype(F32)
        h_b = ((4.0 + gc.astype(np.float64)) - rc.astype(np.float64)).astype(F32)
        h = np.where(r == mx, h_r, np.where(g == mx, h_g, h_b))
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(F32)
        hh = np.clip((h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    return np.where(grey, 0, hh), np.where(grey, 0, s), mx


def hsv_to_rgb(h, s, v):
    """Pillow's hsv2rgb on int arrays: (R, G, B) int64 arrays."""
    h, s, v = (np.asarray(t, dtype=np.int64) for t in (h, s, v))
    hf = h.astype(F32) * F32(6.0) / F32(255.0)
    fs = s.astype(F32) / F32(255.0)
    i = np.floor(hf)
    f = hf - i
    vf = v.astype(F32)
    rnd = lambda t: np.clip(np.floor(t + F32(0.5)), 0, 255).astype(np.int64)
    p = rnd(vf * (F32(1.0) - fs))
    q = rnd(vf * (F32(1.0) - fs * f))
    t = rnd(vf * (F32(1.0) - fs * (F32(1.0) - f)))
    k = i.astype(np.int64) % 6
    pick = lambda six: np.select([k == j for j in range(6)], six)
    r, g, b = pick([v, q, p, p, t, v]), pick([t, v, v, q, p, p]), pick([p, p, t, v, v, q])
    grey = s == 0
    return np.where(grey, v, r), np.where(grey, v, g), np.where(grey, v, b)


def hue_shift_of(hue):
    """The uint8 added to H for a hue factor in [-0.5, 0.5]: trunc(hue * 255) mod 256."""
    return int(math.trunc(float(hue) * 255.0)) % 256


def jitter_ref(img, order, factors, hue_shift):
    """ColorJitter on one crop: img uint8 [3, S, S]; ``order`` the four operation ids in the order they run; factors = (brightness,
    contrast, saturation) as fp32; hue_shift the uint8 added to H."""
    rgb = img.astype(np.int64)
    for op in order:
        if op == BRIGHTNESS:
            rgb = blend(np.zeros_like(rgb), rgb, factors[0])
        elif op == CONTRAST:
            rgb = blend(np.full_like(rgb, contrast_mean(rgb)), rgb, factors[1])
        elif op == SATURATION:
            rgb = blend(np.broadcast_to(luma(rgb)[None], rgb.shape), rgb, factors[2])
        else:
            h, s, v = rgb_to_hsv(rgb[0], rgb[1], rgb[2])
            rgb = np.stack(hsv_to_rgb((h + int(hue_shift)) & 255, s, v))
    return rgb.astype(np.uint8)


# ---------------------------------------------------------------------------------------------
# blur
# ---------------------------------------------------------------------------------------------
def blur_weights(sigma):
    """(k_edge, k_mid) as fp32: e = exp(-0.5 (1 / sigma)^2) evaluated on doubles and rounded to fp32 once, then fp32 arithmetic."""
    inv = 1.0 / float(sigma)
    e = F32(math.exp(-0.5 * (inv * inv)))
    den = (e + F32(1.0)) + e
    return F32(e / den), F32(F32(1.0) / den)


def blur_ref(img, k_edge, k_mid):
    """3 x 3 blur of uint8 [3, S, S]: fp32 products with the weights k[i] k[j], added in row-major order from 0, rint, clamp; the
    border reflects without repeating the edge."""
    S = img.shape[-1]
    k = [F32(k_edge), F32(k_mid), F32(k_edge)]
    idx = np.arange(-1, S + 1)
    idx = np.where(idx < 0, -idx, np.where(idx >= S, 2 * (S - 1) - idx, idx))
    p = img.astype(F32)[:, idx][:, :, idx]
    acc = np.zeros(img.shape, dtype=F32)
    for i in range(3):
        for j in range(3):
            acc = acc + F32(k[i] * k[j]) * p[:, i: i + S, j: j + S]
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def colour_ref(img, flags, order, factors, hue_shift, blur):
    """Jitter and blur of one crop as the flags say."""
    if flags & JITTER:
        img = jitter_ref(img, order, factors, hue_shift)
    if flags & BLUR:
        img = blur_ref(img, blur[0], blur[1])
    return img


def feed_ref(images, plan, S):
    """The whole per-batch pipeline on a plan (dict of arrays as ``plan_rows`` / the engine's plan give them): uint8 [B, 3, S, S]."""
    win = windows_ref(images, plan['image'], plan['flags'], plan['afix'], plan['minv'], plan['origin'], S)
    return np.stack([colour_ref(win[k], int(plan['flags'][k]), [int(t) for t in plan['order'][k]], plan['factors'][k], int(plan['hue'][k]),
                                plan['blur'][k]) for k in range(len(win))])


# ---------------------------------------------------------------------------------------------
# the plan's draws, one sample at a time (hisfrag.py:66-78 with the libraries' draws written out)
# ---------------------------------------------------------------------------------------------
PLAN_COLUMNS = 21     # affine angle, tx, ty | warp, angle, scale, dx, dy | top, left | jitter, 4 order keys, b, c, s, h | blur, sigma


def centre_origin(H, S):
    return round_half_even((H - S) / 2) if H >= S else -((S - H) // 2)


def plan_sample(u, H, W, S, train=True):
    """u: 21 uniforms in [0, 1) -> dict(flags, afix, minv, origin, order, factors, hue, blur)."""
    if not train:
        return dict(flags=0, afix=list(IDENTITY_FIX), minv=list(IDENTITY), origin=(centre_origin(H, S), centre_origin(W, S)),
                    order=[0, 1, 2, 3], factors=[F32(1), F32(1), F32(1)], hue=0, blur=[F32(0), F32(1)])
    u = [float(t) for t in u]
    angle = u[0] * 10.0 - 5.0
    tx = round_half_even((u[1] * 2.0 - 1.0) * (0.1 * W))
    ty = round_half_even((u[2] * 2.0 - 1.0) * (0.1 * H))
    afix = affine_fixed(inverse_affine_matrix(W, H, angle, tx, ty))
    flags, minv = AFFINE, list(IDENTITY)
    if u[3] < 0.5:
        flags |= WARP
        minv = invert_affine(forward_matrix(H, W, u[4] * 20.0 - 10.0, u[5] * 0.2 + 0.9, u[6] * 0.1 - 0.05, u[7] * 0.1 - 0.05))
    pad_y, pad_x = max(S - H, 0), max(S - W, 0)
    origin = (int(math.floor(u[8] * (H + 2 * pad_y - S + 1))) - pad_y, int(math.floor(u[9] * (W + 2 * pad_x - S + 1))) - pad_x)
    order, factors, hue = [0, 1, 2, 3], [F32(1), F32(1), F32(1)], 0
    if u[10] < 0.5:
        flags |= JITTER
        order = sorted(range(4), key=lambda k: u[11 + k])
        factors = [F32(u[15 + k] * 0.6 + 0.7) for k in range(3)]
        hue = hue_shift_of(u[18] * 0.6 - 0.3)
    blur = [F32(0), F32(1)]
    if u[19] < 0.5:
        flags |= BLUR
        blur = list(blur_weights(u[20] + 1.0))
    return dict(flags=flags, afix=afix, minv=minv, origin=origin, order=order, factors=factors, hue=hue, blur=blur)


def plan_rows(rows):
    """A list of (image, plan_sample-style dict) -> the dict of arrays the kernels take."""
    col = lambda key, dt: np.array([r[1][key] for r in rows], dtype=dt)
    return {'image': np.array([r[0] for r in rows], dtype=np.int32), 'flags': col('flags', np.int32), 'afix': col('afix', np.int64),
            'minv': col('minv', np.float64), 'origin': col('origin', np.int32), 'order': col('order', np.int32),
            'factors': col('factors', np.float32), 'hue': col('hue', np.int32), 'blur': col('blur', np.float32)}


# ---------------------------------------------------------------------------------------------
# the geometry case table (S = 16)
# ---------------------------------------------------------------------------------------------
CASE_S = 16
CASE_SIZES = ((9, 30), (12, 11), (17, 40), (40, 56), (64, 48), (90, 75))       # two smaller than the window, one barely larger


def case_images(seed=51):
    """Five images of seeded random content and (in place of the fourth) a ramp whose neighbouring pixels all differ."""
    rng = np.random.default_rng(seed)
    images = [rng.integers(1, 256, size=(h, w, 3), dtype=np.uint8) for h, w in CASE_SIZES]      # no 0: a zero fill always shows
    y, x, c = np.meshgrid(np.arange(40), np.arange(56), np.arange(3), indexing='ij')
    images[3] = (1 + (x * 3 + y * 37 + c * 101) % 251).astype(np.uint8)
    return images


def case_table(images, S=CASE_S, seed=52):
    """Per image: identity, affine only, warp only, both, the extreme draws of either stage, integer translations, windows at the
    four corners of the padded image, a window entirely in the pad, seeded plan draws.  Returns (dict of arrays, names)."""
    rng = np.random.default_rng(seed)
    rows, names = [], []

    def add(name, k, flags, afix=IDENTITY_FIX, minv=IDENTITY, origin=(0, 0)):
        rows.append((k, dict(flags=flags, afix=[int(t) for t in afix], minv=[float(t) for t in minv], origin=(int(origin[0]), int(origin[1])),
                             order=[0, 1, 2, 3], factors=[1, 1, 1], hue=0, blur=[0, 1])))
        names.append(f'{name}/image{k}')

    for k, img in enumerate(images):
        H, W, _ = img.shape
        pad_y, pad_x = max(S - H, 0), max(S - W, 0)
        lo, hi = (-pad_y, -pad_x), (H + pad_y - S, W + pad_x - S)             # the padded image's first and last origins
        mid = ((lo[0] + hi[0]) // 2, (lo[1] + hi[1]) // 2)
        aff = lambda ang, fx, fy: affine_fixed(inverse_affine_matrix(W, H, ang, round_half_even(fx * W), round_half_even(fy * H)))
        inv = lambda *a: invert_affine(forward_matrix(H, W, *a))
        add('identity', k, 0, origin=mid)
        add('identity-first', k, 0, origin=lo)
        add('identity-last', k, 0, origin=hi)
        add('affine-shift', k, AFFINE, afix=affine_fixed((1, 0, 2, 0, 1, -1)), origin=mid)
        add('affine-small', k, AFFINE, afix=aff(0.7, 0.0, 0.0), origin=mid)
        add('affine', k, AFFINE, afix=aff(3.0, 0.04, -0.03), origin=mid)
        add('warp-shift', k, WARP, minv=(1, 0, 1, 0, 1, 1), origin=mid)
        add('warp-half', k, WARP, minv=(1, 0, 0.5, 0, 1, 0.25), origin=mid)
        add('warp-small', k, WARP, minv=inv(1.0, 1.0, 0.0, 0.0), origin=mid)
        add('warp', k, WARP, minv=inv(7.0, 1.05, 0.01, -0.02), origin=mid)
        add('both-small', k, AFFINE | WARP, afix=aff(-0.7, 0.0, 0.0), minv=inv(-1.0, 0.98, 0.0, 0.0), origin=mid)
        add('both', k, AFFINE | WARP, afix=aff(-4.0, -0.05, 0.06), minv=inv(-6.0, 0.95, 0.02, 0.03), origin=mid)
        for j, (ang, fx, fy) in enumerate(((5.0, 0.1, 0.1), (-5.0, -0.1, -0.1), (5.0, -0.1, 0.1), (-5.0, 0.1, -0.1))):
            add(f'affine-extreme{j}', k, AFFINE, afix=aff(ang, fx, fy), origin=lo if j & 1 else hi)
        for j, (ang, sc, dx, dy) in enumerate(((10.0, 0.9, 0.05, 0.05), (-10.0, 1.1, -0.05, -0.05), (10.0, 1.1, -0.05, 0.05), (-10.0, 0.9, 0.05, -0.05))):
            add(f'warp-extreme{j}', k, WARP | (AFFINE if j & 2 else 0), afix=aff(2.0, 0.01, 0.01), minv=inv(ang, sc, dx, dy), origin=mid)
        for j, origin in enumerate(((lo[0], lo[1]), (lo[0], hi[1]), (hi[0], lo[1]), (hi[0], hi[1]))):
            add(f'corner{j}', k, AFFINE | WARP, afix=aff(1.5, 0.02, -0.02), minv=inv(4.0, 1.02, -0.01, 0.02), origin=origin)
        add('in-the-pad', k, AFFINE | WARP, afix=aff(1.5, 0.02, -0.02), minv=inv(4.0, 1.02, -0.01, 0.02), origin=(H + 3, -S - 5))
        for j in range(2):
            u = rng.random(PLAN_COLUMNS).astype(np.float32)
            u[3] = 0.25 if j else 0.75
            plan = plan_sample(u, H, W, S)
            add(f'random{j}', k, plan['flags'] & (AFFINE | WARP), afix=plan['afix'], minv=plan['minv'], origin=plan['origin'])
    return plan_rows(rows), names


# ---------------------------------------------------------------------------------------------
# colour cases
# ---------------------------------------------------------------------------------------------
ORDERS = [(a, b, c, d) for a in range(4) for b in range(4) for c in range(4) for d in range(4) if len({a, b, c, d}) == 4]


def half_mean_image(S):
    """A crop whose L mean is exactly x.5: grey 100 everywhere (L = 100) except S S / 2 pixels of grey 101."""
    img = np.full((3, S, S), 100, dtype=np.uint8)
    img.reshape(3, -1)[:, : S * S // 2] = 101
    return img


def colour_cases(S, seed=53):
    """26 crops: one per order of the four operations, then the half-mean image twice (contrast first; contrast behind a
    brightness of exactly 1).  Returns (images uint8 [26, 3, S, S], plan dict).  Factors cycle through 0.7, 1.3 and seeded random
    ones, hue shifts through 0, 76, 180."""
    rng = np.random.default_rng(seed + S)
    imgs = rng.integers(0, 256, size=(len(ORDERS) + 2, 3, S, S), dtype=np.uint8)
    imgs[1, :, : S // 2] = imgs[1, :1, : S // 2]                 # greys (S = 0 in HSV) and saturated primaries
    imgs[2, 0], imgs[2, 1, :, ::2], imgs[2, 2] = 255, 0, 0
    imgs[24:] = half_mean_image(S)
    rows = []

    def add(order, f, hue):
        rows.append((0, dict(flags=JITTER, afix=list(IDENTITY_FIX), minv=list(IDENTITY), origin=(0, 0), order=list(order),
                             factors=[F32(t) for t in f], hue=hue, blur=[0, 1])))

    for k, order in enumerate(ORDERS):
        add(order, [(0.7, 0.7, 0.7), (1.3, 1.3, 1.3), (0.7, 1.3, 1.0), tuple(rng.uniform(0.7, 1.3, 3))][k % 4], (0, 76, 180)[k % 3])
    add((CONTRAST, BRIGHTNESS, SATURATION, HUE), (0.7, 1.3, 1.3), 76)
    add((BRIGHTNESS, CONTRAST, HUE, SATURATION), (1.0, 1.3, 0.7), 0)
    return imgs, plan_rows(rows)


def blur_cases(S, seed=55):
    """(images uint8 [8, 3, S, S], plan dict): blur alone at sigma 1, 2 and two seeded ones, jitter and blur together (three rows),
    and a row with neither."""
    rng = np.random.default_rng(seed + S)
    imgs = rng.integers(0, 256, size=(8, 3, S, S), dtype=np.uint8)
    imgs[1, :, 0, :], imgs[1, :, :, -1] = 255, 0                 # strong edges on the border rows and columns
    rows = []
    for k, sigma in enumerate((1.0, 2.0, float(rng.uniform(1, 2)), float(rng.uniform(1, 2)))):
        rows.append((0, dict(flags=BLUR, afix=list(IDENTITY_FIX), minv=list(IDENTITY), origin=(0, 0), order=[0, 1, 2, 3], factors=[1, 1, 1],
                             hue=0, blur=list(blur_weights(sigma)))))
    for k in range(3):
        rows.append((0, dict(flags=JITTER | BLUR, afix=list(IDENTITY_FIX), minv=list(IDENTITY), origin=(0, 0), order=list(ORDERS[5 + 7 * k]),
                             factors=[F32(t) for t in rng.uniform(0.7, 1.3, 3)], hue=(76, 180, 13)[k],
                             blur=list(blur_weights(float(rng.uniform(1, 2)))))))
    rows.append((0, dict(flags=0, afix=list(IDENTITY_FIX), minv=list(IDENTITY), origin=(0, 0), order=[3, 2, 1, 0], factors=[F32(0.7)] * 3,
                         hue=99, blur=list(blur_weights(1.5)))))
    return imgs, plan_rows(rows)


def plan_drawn_batch(S, sizes, seed=54, rows=8):
    """(images, plan dict): ``rows`` samples drawn the way the loader draws them, alternating over images of ``sizes``; the warp is on
    in three of four, one window sits at the first origin of the padded image and one at the last."""
    rng = np.random.default_rng(seed + S)
    images = [rng.integers(1, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
    out = []
    for k in range(rows):
        u = rng.random(PLAN_COLUMNS).astype(np.float32)
        u[3] = 0.75 if k % 4 == 3 else 0.25
        if k == 4:
            u[8:10] = 0.0
        if k == 5:
            u[8:10] = 0.999
        i = k % len(images)
        out.append((i, plan_sample(u, images[i].shape[0], images[i].shape[1], S)))
    return images, plan_rows(out)


def toy_writers(seed=67):
    """(labels, images) of a 9-writer toy set with 2-5 images per writer, in shuffled order; images of 9-39 pixels per side."""
    rng = np.random.default_rng(seed)
    counts = [2, 3, 5, 4, 2, 3, 4, 5, 3]                         # 31 images
    labels = [100 + 7 * w for w, c in enumerate(counts) for _ in range(c)]
    labels = [labels[k] for k in rng.permutation(len(labels))]
    images = [rng.integers(0, 256, size=(int(rng.integers(9, 40)), int(rng.integers(9, 40)), 3), dtype=np.uint8) for _ in labels]
    return labels, images
