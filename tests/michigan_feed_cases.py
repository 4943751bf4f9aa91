"""Test-side restatement of the michigan device feed (michigan.py:68-101) in plain numpy and Python floats, and
the case tables the GPU tests launch.  No GPU dependency and no use of the product's code: tests/test_michigan_feed.py checks the
restatement against Pillow itself, tests/test_gpu_michigan_feed.py holds the kernels to it bit for bit.

Geometry, all integer:
  Wd(u, v)  the RandomCrop window, 0 <= u, v < S: src[v + top][u + left] inside the image, else 255; (top, left) in unpadded image
            coordinates (may be negative).  A tap outside the window reads 255 as well (no plan produces one).
  T(x, r)   clip8((2^21 + sum_i kx[x][i] Wd(x0[x] + i, r)) >> 22)            Pillow's horizontal pass
  R(x, y)   clip8((2^21 + sum_j ky[y][j] T(x, y0[y] + j)) >> 22)             its vertical pass on the uint8 intermediate
  holes     R inside any of the first n_holes rectangles (x1, y1, x2, y2), half-open, becomes 255 (if flag bit 0 is set)
  flips     out(x, y) = holed(fx ? S - 1 - x : x, fy ? S - 1 - y : y)
Colour jitter: tests/hisfrag_feed_cases.py (the same kernel).  Blur and grey: the functions below.
"""
import math

import numpy as np

from div2k_feed_cases import round_half_even
from hisfrag_feed_cases import ORDERS, case_images, hue_shift_of, jitter_ref, luma, toy_writers      # noqa: F401 (re-exported)

DROPOUT, HFLIP, JITTER, BLUR, VFLIP, GRAY = 1, 2, 4, 8, 16, 32
MAX_HOLES = 16
BITS = 22
F32 = np.float32
NO_BLUR = (1 << 24, 0)


# ---------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------
def coeffs(in_size, out_size, indices=None, first=0):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter where it scales up (in_size <= out_size, support 1,
    ksize 3), for the output indices ``indices`` (all by default): (first taps + ``first``, [n][3] fixed-point weights)."""
    assert 0 < in_size <= out_size
    scale = in_size / out_size
    x0, kk = [], []
    for xx in (range(out_size) if indices is None else indices):
        center = (xx + 0.5) * scale
        xmin = max(int(center - 1.0 + 0.5), 0)
        xmax = min(int(center + 1.0 + 0.5), in_size) - xmin
        assert 1 <= xmax <= 3
        w = [max(0.0, 1.0 - abs(x + xmin - center + 0.5)) for x in range(xmax)]
        ww = sum(w)
        w = [v / ww for v in w] + [0.0] * (3 - xmax)
        x0.append(xmin + first)
        kk.append([int(0.5 + v * (1 << BITS)) for v in w])
    return x0, kk


def box_tables(box, S):
    """(x0, kx, y0, ky) of RandomResizedCrop's box (i, j, h, w) resized to S x S."""
    i, j, h, w = (int(t) for t in box)
    x0, kx = coeffs(w, S, first=j)
    y0, ky = coeffs(h, S, first=i)
    return x0, kx, y0, ky


def eval_tables(S):
    """The tables of Resize(R = int(1.15 S)) then CenterCrop(S) on an S x S window, the same on both axes."""
    R = int(S * 1.15)
    off = round_half_even((R - S) / 2)
    x0, kx = coeffs(S, R, indices=range(off, off + S))
    return x0, kx, list(x0), [list(k) for k in kx]


def window_hwc(img, top, left, S):
    """The padded RandomCrop window of one image: uint8 [S, S, 3], 255 outside the image."""
    H, W, _ = img.shape
    ys, xs = np.arange(S, dtype=np.int64) + int(top), np.arange(S, dtype=np.int64) + int(left)
    ok = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
    val = img[np.clip(ys, 0, H - 1)[:, None], np.clip(xs, 0, W - 1)[None, :], :]
    return np.where(ok[..., None], val, 255).astype(np.uint8)


def clip8(a):
    return np.clip(a, 0, 255)


def resample_ref(win, x0, kx, y0, ky, inside=None):
    """R of the module docstring from the window ``win`` uint8 [S, S, 3]: uint8 [S, S, 3].  With ``inside`` (bool [S, S], the window
    pixels that come from the image) also whether any tap of non-zero weight read a pad pixel."""
    S = win.shape[0]
    x0, kx, y0, ky = np.asarray(x0, dtype=np.int64), np.asarray(kx, dtype=np.int64), np.asarray(y0, dtype=np.int64), np.asarray(ky, dtype=np.int64)
    big = np.full((S + 8, S + 8, 3), 255, dtype=np.int64)                  # taps outside the window read 255
    big[4: 4 + S, 4: 4 + S] = win
    ok = np.zeros((S + 8, S + 8), dtype=bool)
    if inside is not None:
        ok[4: 4 + S, 4: 4 + S] = inside
    at = lambda t: np.clip(t + 4, 0, S + 7)                                 # beyond the margin it is 255 all the same
    rows = np.arange(-4, S + 4, dtype=np.int64)
    T = np.full((S + 8, S, 3), 1 << (BITS - 1), dtype=np.int64)            # T[r + 4][x]
    padded_x = np.zeros((S + 8, S), dtype=bool)
    for i in range(3):
        T += kx[None, :, i, None] * big[at(rows)[:, None], at(x0 + i)[None, :], :]
        padded_x |= (kx[None, :, i] != 0) & ~ok[at(rows)[:, None], at(x0 + i)[None, :]]
    T = clip8(T >> BITS)
    R = np.full((S, S, 3), 1 << (BITS - 1), dtype=np.int64)
    touched = np.zeros((S, S), dtype=bool)
    for j in range(3):
        R += ky[:, j, None, None] * T[at(y0 + j), :, :]
        touched |= (ky[:, j, None] != 0) & padded_x[at(y0 + j), :]
    R = clip8(R >> BITS).astype(np.uint8)
    return (R, bool(touched.any())) if inside is not None else R


def holes_ref(R, holes, n_holes):
    """CoarseDropout's fill on uint8 [S, S, 3]: the first n_holes (clamped to 0..16) rectangles (x1, y1, x2, y2) become 255."""
    out = R.copy()
    for x1, y1, x2, y2 in list(holes)[: max(0, min(int(n_holes), MAX_HOLES))]:
        out[max(int(y1), 0): max(int(y2), 0), max(int(x1), 0): max(int(x2), 0)] = 255
    return out


def geometry_ref(img, flags, origin, x0, kx, y0, ky, holes, n_holes, S, want_touch=False):
    """One sample: img uint8 [H, W, 3] -> uint8 [3, S, S]."""
    H, W, _ = img.shape
    top, left = int(origin[0]), int(origin[1])
    ys, xs = np.arange(S) + top, np.arange(S) + left
    inside = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
    R, touch = resample_ref(window_hwc(img, top, left, S), x0, kx, y0, ky, inside=inside)
    if flags & DROPOUT:
        R = holes_ref(R, holes, n_holes)
    if flags & HFLIP:
        R = R[:, ::-1]
    if flags & VFLIP:
        R = R[::-1]
    out = np.ascontiguousarray(R.transpose(2, 0, 1))
    return (out, touch) if want_touch else out


def windows_ref(images, plan, S):
    """A batch with in-range image indices: uint8 [B, 3, S, S]."""
    return np.stack([geometry_ref(images[int(plan['image'][k])], int(plan['flags'][k]), plan['origin'][k], plan['x0'][k], plan['kx'][k],
                                  plan['y0'][k], plan['ky'][k], plan['holes'][k], int(plan['n_holes'][k]), S) for k in range(len(plan['image']))])


# ---------------------------------------------------------------------------------------------
# ImageFilter.GaussianBlur(radius <= 1) and convert('L')
# ---------------------------------------------------------------------------------------------
def blur_weights(radius):
    """(ww, fw) of Pillow's box blur for a Gaussian radius <= 1: the radius becomes a C float, ImagingGaussianBlur's sigma^2 and box
    radius `a` and ImagingHorizontalBoxBlur's ww are fp32 arithmetic, one rounding per operation; the integer box radius is 0."""
    r = F32(radius)
    s2 = F32(F32(r * r) / F32(3.0))
    a = F32(F32(-F32(F32(3.0) * s2)) / F32(F32(6.0) * F32(s2 - F32(1.0))))
    assert 0.0 <= float(a) < 1.0, (radius, a)
    ww = int(F32(F32(16777216.0) / F32(F32(a * F32(2.0)) + F32(1.0))))
    return ww, ((1 << 24) - ww) // 2


def box_pass(a, ww, fw, axis):
    """One pass of the 3-tap box blur along ``axis`` of an int64 array, edges replicated."""
    a = np.moveaxis(a, axis, -1)
    prev, nxt = np.concatenate([a[..., :1], a[..., :-1]], axis=-1), np.concatenate([a[..., 1:], a[..., -1:]], axis=-1)
    out = (a * int(ww) + (prev + nxt) * int(fw) + (1 << 23)) >> 24
    assert int(out.max()) <= 255
    return np.moveaxis(out, -1, axis)


def blur_ref(img, ww, fw):
    """uint8 [C, H, W] -> uint8: three passes along x, then three along y, an 8-bit intermediate after each."""
    a = img.astype(np.int64)
    for axis in (-1, -1, -1, -2, -2, -2):
        a = box_pass(a, ww, fw, axis)
    return a.astype(np.uint8)


def gray_ref(img):
    """RandomGrayscale's convert('L') copied to three channels: uint8 [3, H, W]."""
    lum = luma(img.astype(np.int64)).astype(np.uint8)
    return np.stack([lum, lum, lum])


def blur_gray_ref(img, flags, blur):
    if flags & BLUR:
        img = blur_ref(img, int(blur[0]), int(blur[1]))
    if flags & GRAY:
        img = gray_ref(img)
    return img


def colour_ref(img, flags, order, factors, hue_shift, blur):
    """Jitter, blur and grey of one crop as the flags say."""
    if flags & JITTER:
        img = jitter_ref(img, order, factors, hue_shift)
    return blur_gray_ref(img, flags, blur)


def feed_ref(images, plan, S):
    """The whole per-batch pipeline on a plan (dict of arrays as ``plan_rows`` / the engine's plan give them): uint8 [B, 3, S, S]."""
    win = windows_ref(images, plan, S)
    return np.stack([colour_ref(win[k], int(plan['flags'][k]), [int(t) for t in plan['order'][k]], plan['factors'][k], int(plan['hue'][k]),
                                plan['blur'][k]) for k in range(len(win))])


# ---------------------------------------------------------------------------------------------
# the plan's draws, one sample at a time (michigan.py:71-85 with the libraries' draws written out)
# ---------------------------------------------------------------------------------------------
PLAN_COLUMNS = 104    # top, left | 10 x (area, ratio) | i, j | dropout, count | 16 x (height, width, y1, x1) | hflip, vflip |
#                       jitter, 4 order keys, b, c, s, h | blur, radius | grey
LOG_LO, LOG_HI = math.log(3.0 / 4.0), math.log(4.0 / 3.0)


def randint(u, lo, hi):
    """An inclusive integer draw from a uniform in [0, 1)."""
    return int(lo) + min(int(math.floor(u * (int(hi) - int(lo) + 1))), int(hi) - int(lo))


def resized_crop_box(u20, u_i, u_j, S):
    """RandomResizedCrop.get_params on an S x S window for scale (0.6, 1), ratio (3/4, 4/3): ((i, j, h, w), attempts that failed)."""
    for k in range(10):
        area = (u20[2 * k] * 0.4 + 0.6) * float(S * S)
        ratio = math.exp(u20[2 * k + 1] * (LOG_HI - LOG_LO) + LOG_LO)
        w, h = round_half_even(math.sqrt(area * ratio)), round_half_even(math.sqrt(area / ratio))
        if 0 < w <= S and 0 < h <= S:
            return (randint(u_i, 0, S - h), randint(u_j, 0, S - w), h, w), k
    return (0, 0, S, S), 10                                   # the window's ratio is 1: the fallback is the whole window


def centre_origin(W, S):
    """PadCenterCrop: the reference pads BOTH sides by the whole deficit, then centre-crops."""
    d = S - W
    return round_half_even((W - S) / 2) if W >= S else round_half_even(d / 2) - d


def plan_sample(u, H, W, S, train=True, holes=(3, 16), hole_size=(16, 64), radius_max=1.0):
    """u: 104 uniforms in [0, 1) -> dict of one sample's arguments (and 'failed', the RandomResizedCrop attempts that failed)."""
    ident = dict(flags=0, holes=[[0, 0, 0, 0]] * MAX_HOLES, n_holes=0, order=[0, 1, 2, 3], factors=[F32(1), F32(1), F32(1)], hue=0,
                 blur=list(NO_BLUR), failed=0)
    if not train:
        x0, kx, y0, ky = eval_tables(S)
        return dict(ident, origin=(centre_origin(H, S), centre_origin(W, S)), box=(0, 0, S, S), x0=x0, kx=kx, y0=y0, ky=ky)
    u = [float(t) for t in u]
    pad_y, pad_x = max(S - H, 0), max(S - W, 0)
    origin = (randint(u[0], 0, H + 2 * pad_y - S) - pad_y, randint(u[1], 0, W + 2 * pad_x - S) - pad_x)
    box, failed = resized_crop_box(u[2:22], u[22], u[23], S)
    x0, kx, y0, ky = box_tables(box, S)
    flags, rects, n = 0, [[0, 0, 0, 0]] * MAX_HOLES, 0
    if u[24] < 0.9:
        flags |= DROPOUT
        n = randint(u[25], holes[0], holes[1])
        rects = []
        for h in range(MAX_HOLES):
            hh, hw = (min(randint(u[26 + 4 * h + t], hole_size[0], hole_size[1]), S) for t in range(2))
            y1, x1 = randint(u[26 + 4 * h + 2], 0, S - hh), randint(u[26 + 4 * h + 3], 0, S - hw)
            rects.append([x1, y1, x1 + hw, y1 + hh] if h < n else [0, 0, 0, 0])
    flags |= (HFLIP if u[90] < 0.5 else 0) | (VFLIP if u[91] < 0.5 else 0)
    order, factors, hue = [0, 1, 2, 3], [F32(1), F32(1), F32(1)], 0
    if u[92] < 0.5:
        flags |= JITTER
        order = sorted(range(4), key=lambda k: u[93 + k])
        factors = [F32(u[97] * 0.4 + 0.8), F32(u[98] * 0.6 + 0.7), F32(u[99] * 0.6 + 0.7)]
        hue = hue_shift_of(u[100] * 0.2 - 0.1)
    blur = list(NO_BLUR)
    if u[101] < 0.5:
        flags |= BLUR
        blur = list(blur_weights(u[102] * (radius_max - 0.1) + 0.1))
    if u[103] < 0.2:
        flags |= GRAY
    return dict(flags=flags, origin=origin, box=box, x0=x0, kx=kx, y0=y0, ky=ky, holes=rects, n_holes=n, order=order, factors=factors,
                hue=hue, blur=blur, failed=failed)


_PLAN_DTYPES = (('flags', np.int32), ('origin', np.int32), ('box', np.int32), ('x0', np.int32), ('kx', np.int32), ('y0', np.int32),
                ('ky', np.int32), ('holes', np.int32), ('n_holes', np.int32), ('order', np.int32), ('factors', np.float32), ('hue', np.int32),
                ('blur', np.int32))


def plan_rows(rows):
    """A list of (image, plan_sample-style dict) -> the dict of arrays the kernels take."""
    out = {'image': np.array([r[0] for r in rows], dtype=np.int32)}
    for key, dt in _PLAN_DTYPES:
        out[key] = np.array([r[1][key] for r in rows], dtype=dt)
    return out


# ---------------------------------------------------------------------------------------------
# the geometry case table (S = 16)
# ---------------------------------------------------------------------------------------------
CASE_S = 16


def border_holes(S):
    """Sixteen rectangles: the four corners, the four edges, overlapping ones in the middle, an empty one and one over the window."""
    return [[0, 0, 3, 2], [S - 2, 0, S, 3], [0, S - 3, 2, S], [S - 1, S - 1, S, S], [5, 0, 9, 1], [0, 6, 1, 9], [S - 1, 4, S, 8], [6, S - 1, 11, S],
            [4, 4, 9, 8], [6, 6, 12, 10], [7, 3, 8, 13], [10, 10, 10, 14], [3, 11, 6, 12], [-4, 12, 2, 14], [12, 12, S + 5, 13], [8, 8, 9, 9]]


def case_table(images, S=CASE_S, seed=57):
    """Per image: the identity at three origins, boxes touching each window edge, 1-pixel boxes, windows that reach into the 255 pad
    (origins outside the image), 0 / 1 / 16 holes, each flip and both, the train=False tables, seeded plan draws.  Returns (dict of
    arrays, names)."""
    rng = np.random.default_rng(seed)
    rows, names = [], []
    none = [[0, 0, 0, 0]] * MAX_HOLES

    def add(name, k, origin, box=None, flags=0, holes=none, n_holes=0, tables=None):
        x0, kx, y0, ky = tables if tables is not None else box_tables(box, S)
        rows.append((k, dict(flags=flags, origin=(int(origin[0]), int(origin[1])), box=box or (0, 0, S, S), x0=x0, kx=kx, y0=y0, ky=ky,
                             holes=[list(h) for h in holes], n_holes=n_holes, order=[0, 1, 2, 3], factors=[1, 1, 1], hue=0, blur=list(NO_BLUR))))
        names.append(f'{name}/image{k}')

    whole = (0, 0, S, S)
    for k, img in enumerate(images):
        H, W, _ = img.shape
        pad_y, pad_x = max(S - H, 0), max(S - W, 0)
        lo, hi = (-pad_y, -pad_x), (H + pad_y - S, W + pad_x - S)             # the padded image's first and last origins
        mid = ((lo[0] + hi[0]) // 2, (lo[1] + hi[1]) // 2)
        add('identity', k, mid, whole)
        add('identity-first', k, lo, whole)
        add('identity-last', k, hi, whole)
        add('box-top-left', k, mid, (0, 0, 11, 13))
        add('box-bottom-right', k, mid, (S - 12, S - 10, 12, 10))
        add('box-top-right', k, lo, (0, S - 13, 14, 13))
        add('box-bottom-left', k, hi, (S - 11, 0, 11, 15))
        add('box-inner', k, mid, (2, 3, 11, 12))
        add('box-full-height', k, mid, (0, 2, S, 11))
        add('box-column', k, mid, (0, 7, S, 1))
        add('box-row', k, mid, (9, 0, 1, S))
        add('box-pixel', k, mid, (S - 1, S - 1, 1, 1))
        add('pad-above-left', k, (-5, -3), (1, 1, 13, 12))
        add('pad-below-right', k, (H - S + 6, W - S + 4), (2, 3, 14, 13))
        add('all-pad', k, (H + 2, -S - 3), (2, 2, 12, 12))
        add('holes-one', k, mid, (1, 2, 13, 12), flags=DROPOUT, holes=border_holes(S), n_holes=1)
        add('holes-sixteen', k, mid, (1, 2, 13, 12), flags=DROPOUT, holes=border_holes(S), n_holes=16)
        add('holes-unflagged', k, mid, (1, 2, 13, 12), flags=0, holes=border_holes(S), n_holes=16)
        add('hflip', k, mid, (1, 2, 13, 12), flags=HFLIP)
        add('vflip', k, mid, (1, 2, 13, 12), flags=VFLIP)
        add('flips-holes', k, mid, (3, 0, 12, 14), flags=HFLIP | VFLIP | DROPOUT, holes=border_holes(S), n_holes=7)
        add('hflip-holes', k, hi, (0, 1, 15, 12), flags=HFLIP | DROPOUT | JITTER | BLUR | GRAY, holes=border_holes(S), n_holes=16)
        add('eval', k, (centre_origin(H, S), centre_origin(W, S)), tables=eval_tables(S))
        for j in range(2):
            plan = plan_sample(rng.random(PLAN_COLUMNS).astype(np.float32), H, W, S, holes=(0, 16), hole_size=(1, 6))
            add(f'random{j}', k, plan['origin'], plan['box'], flags=plan['flags'] & (DROPOUT | HFLIP | VFLIP), holes=plan['holes'],
                n_holes=plan['n_holes'])
    return plan_rows(rows), names


def case_refs(images, table, S=CASE_S):
    """(reference windows uint8 [n, 3, S, S], per case whether a tap of non-zero weight read a pad pixel)."""
    refs = [geometry_ref(images[int(table['image'][k])], int(table['flags'][k]), table['origin'][k], table['x0'][k], table['kx'][k],
                         table['y0'][k], table['ky'][k], table['holes'][k], int(table['n_holes'][k]), S, want_touch=True)
            for k in range(len(table['image']))]
    return np.stack([r[0] for r in refs]), [r[1] for r in refs]


# ---------------------------------------------------------------------------------------------
# blur / grey cases
# ---------------------------------------------------------------------------------------------
def blur_cases(S, seed=58):
    """(images uint8 [10, 3, S, S], flags int32 [10], weights int32 [10, 2]): blur only at radius 0.1, 1.0 and two seeded ones, grey
    only, both (twice), neither (twice, once with blur weights present), a constant image blurred.  Image 1 has strong edges on its
    border rows and columns, image 2 has four levels only."""
    rng = np.random.default_rng(seed + S)
    imgs = rng.integers(0, 256, size=(10, 3, S, S), dtype=np.uint8)
    imgs[1, :, 0, :], imgs[1, :, :, -1], imgs[1, :, -1, :], imgs[1, :, :, 0] = 255, 0, 0, 255
    imgs[2] = (imgs[2] >> 6) * 85
    imgs[9] = 201
    radii = [0.1, 1.0, float(rng.uniform(0.1, 1)), float(rng.uniform(0.1, 1)), 0.5, 1.0, float(rng.uniform(0.1, 1)), 0.7, 0.3, 1.0]
    flags = [BLUR, BLUR, BLUR, BLUR, GRAY, BLUR | GRAY, BLUR | GRAY | JITTER | DROPOUT | HFLIP | VFLIP, 0, JITTER | DROPOUT, BLUR]
    return imgs, np.array(flags, dtype=np.int32), np.array([blur_weights(r) for r in radii], dtype=np.int32)


def plan_drawn_batch(S, sizes, seed=59, rows=8):
    """(images, plan dict): ``rows`` samples drawn the way the loader draws them, alternating over images of ``sizes``; one window sits
    at the first origin of the padded image and one at the last; dropout, jitter, blur and grey are each on in some and off in some."""
    rng = np.random.default_rng(seed + S)
    images = [rng.integers(1, 255, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
    out = []
    for k in range(rows):
        u = rng.random(PLAN_COLUMNS).astype(np.float32)
        u[24] = 0.95 if k == 3 else 0.5
        u[92], u[101], u[103] = (0.25, 0.75)[k % 2], (0.25, 0.75)[(k // 2) % 2], (0.1, 0.6)[(k // 4) % 2]
        if k == 4:
            u[0:2] = 0.0
        if k == 5:
            u[0:2] = 0.999
        i = k % len(images)
        out.append((i, plan_sample(u, images[i].shape[0], images[i].shape[1], S, hole_size=(max(S // 16, 1), max(S // 4, 1)))))
    return images, plan_rows(out)
