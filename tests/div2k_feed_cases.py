"""Test-side restatement of the DIV2K device feed (data/datasets/div2k_patch.py:84-111) in plain numpy and
Python floats, and the case table the GPU test launches.  No GPU dependency and no use of the product's code: tests/test_div2k_feed.py
checks the restatement against slices it can state without any package, tests/test_gpu_div2k_feed.py holds the kernel to it bit
for bit.

Per window pixel (x, y), X = x + left, Y = y + top:
  warp off   the source pixel is (X, Y);
  warp on    Xf = rint(m0 X 1024) + rint((m1 Y + m2) 1024) + 16 on IEEE doubles (every product and sum rounded on its own),
             Xq = Xf >> 5, u0 = Xq >> 5, a = Xq & 31, likewise Yf, v0, b from m3, m4, m5; taps (u0, v0), (u0 + 1, v0), (u0, v0 + 1),
             (u0 + 1, v0 + 1) with weights (32 - a)(32 - b) 32, a (32 - b) 32, (32 - a) b 32, a b 32; value (sum + 16384) >> 15;
  border     tap indices are reflected (-i below 0, 2 (n - 1) - i at or above n) until in range, THEN flipped (u -> W - 1 - u,
             v -> H - 1 - v): the flips come first in the reference, so the warp reads the flipped image;
  colour     floor(min(max(float32(p) + shift_c, 0), 255)) in fp32.
"""
import math

import numpy as np

HFLIP, VFLIP, WARP, COLOUR = 1, 2, 4, 8
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


# ---------------------------------------------------------------------------------------------
# the per-pixel definition
# ---------------------------------------------------------------------------------------------
def fixed1024(t):
    """rint(t * 1024) (round half to even on doubles) as int64, saturated to the int32 range."""
    return np.clip(np.rint(np.asarray(t, dtype=np.float64) * 1024.0), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def reflect101(i, n):
    """BORDER_REFLECT_101, literally: -i below 0, 2 (n - 1) - i at or above n, until in range."""
    i = np.array(i, dtype=np.int64, copy=True)
    if n == 1:
        return np.zeros_like(i)
    while ((i < 0) | (i >= n)).any():
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * (n - 1) - i, i)
    return i


def region_ref(img, flags, minv, rgb, top, left, S, want_touch=False):
    """One sample: img uint8 [H, W, 3] -> uint8 [3, 2 S, 3 S].  With ``want_touch`` also whether a tap fell outside the image."""
    H, W, _ = img.shape
    assert 0 <= top <= H - 2 * S and 0 <= left <= W - 3 * S, 'the restatement takes clamped origins'
    ys = np.arange(2 * S, dtype=np.int64) + top
    xs = np.arange(3 * S, dtype=np.int64) + left
    src = img.astype(np.int64)

    def fetch(u, v):
        u, v = reflect101(u, W), reflect101(v, H)
        if flags & HFLIP:
            u = W - 1 - u
        if flags & VFLIP:
            v = H - 1 - v
        return src[v, u, :]

    touch = False
    if flags & WARP:
        m = [np.float64(v) for v in minv]
        xf = fixed1024(m[0] * xs.astype(np.float64))[None, :] + fixed1024(m[1] * ys.astype(np.float64) + m[2])[:, None] + 16
        yf = fixed1024(m[3] * xs.astype(np.float64))[None, :] + fixed1024(m[4] * ys.astype(np.float64) + m[5])[:, None] + 16
        xq, yq = xf >> 5, yf >> 5
        u0, a, v0, b = xq >> 5, (xq & 31)[..., None], yq >> 5, (yq & 31)[..., None]
        touch = bool((u0 < 0).any() or (u0 + 1 > W - 1).any() or (v0 < 0).any() or (v0 + 1 > H - 1).any())
        acc = ((32 - a) * (32 - b) * 32 * fetch(u0, v0) + a * (32 - b) * 32 * fetch(u0 + 1, v0)
               + (32 - a) * b * 32 * fetch(u0, v0 + 1) + a * b * 32 * fetch(u0 + 1, v0 + 1))
        val = (acc + 16384) >> 15
    else:
        val = fetch(np.broadcast_to(xs[None, :], (2 * S, 3 * S)), np.broadcast_to(ys[:, None], (2 * S, 3 * S)))
    if flags & COLOUR:
        shifted = val.astype(np.float32) + np.asarray(rgb, dtype=np.float32)[None, None, :]
        val = np.floor(np.minimum(np.maximum(shifted, np.float32(0)), np.float32(255)))
    out = np.ascontiguousarray(val.astype(np.uint8).transpose(2, 0, 1))
    return (out, touch) if want_touch else out


def regions_ref(images, image, flags, minv, rgb, crop, S):
    """A batch with in-range arguments: uint8 [B, 3, 2 S, 3 S]."""
    return np.stack([region_ref(images[int(image[k])], int(flags[k]), minv[k], rgb[k], int(crop[k][0]), int(crop[k][1]), S)
                     for k in range(len(image))])


# ---------------------------------------------------------------------------------------------
# the plan's draws, one sample at a time (div2k_patch.py:89-111 with the libraries' draws written out)
# ---------------------------------------------------------------------------------------------
def forward_matrix(H, W, angle_deg, scale, dx, dy):
    """cv2.getRotationMatrix2D((W / 2 - 0.5, H / 2 - 0.5), angle, scale) with (dx W, dy H) added to the translation."""
    cx, cy = W / 2 - 0.5, H / 2 - 0.5
    rad = angle_deg * (math.pi / 180.0)
    alpha, beta = math.cos(rad) * scale, math.sin(rad) * scale
    return [alpha, beta, (1 - alpha) * cx - beta * cy + dx * W, -beta, alpha, beta * cx + (1 - alpha) * cy + dy * H]


def invert_affine(M):
    """The inversion cv2.warpAffine applies to a forward matrix."""
    det = M[0] * M[4] - M[1] * M[3]
    d = 1.0 / det if det != 0 else 0.0
    i0, i1, i3, i4 = M[4] * d, M[1] * -d, M[3] * -d, M[0] * d
    return [i0, i1, -(i0 * M[2]) - i1 * M[5], i3, i4, -(i3 * M[2]) - i4 * M[5]]


def round_half_even(v):
    f = math.floor(v)
    if v - f != 0.5:
        return int(math.floor(v + 0.5))
    return int(f) if int(f) % 2 == 0 else int(f) + 1


def plan_sample(u, H, W, S, train=True):
    """u: 13 uniforms in [0, 1) -> (flags, forward matrix or None, minv, rgb, (top, left))."""
    room_y, room_x = H - 2 * S, W - 3 * S
    if not train:
        return 0, None, list(IDENTITY), [0.0, 0.0, 0.0], (round_half_even(room_y / 2), round_half_even(room_x / 2))
    u = [float(v) for v in u]
    flags = (HFLIP if u[0] < 0.5 else 0) | (VFLIP if u[1] < 0.5 else 0) | (WARP if u[2] < 0.5 else 0) | (COLOUR if u[7] < 0.5 else 0)
    M, minv = None, list(IDENTITY)
    if flags & WARP:
        M = forward_matrix(H, W, -20.0 + 40.0 * u[3], 0.85 + 0.3 * u[4], -0.05 + 0.1 * u[5], -0.05 + 0.1 * u[6])
        minv = invert_affine(M)
    rgb = [float(np.float32(-15.0 + 30.0 * v)) for v in u[8:11]] if flags & COLOUR else [0.0, 0.0, 0.0]
    crop = (min(int(math.floor(u[11] * (room_y + 1))), room_y), min(int(math.floor(u[12] * (room_x + 1))), room_x))
    return flags, M, minv, rgb, crop


# ---------------------------------------------------------------------------------------------
# the case table of the bit-exactness test (S = 8: windows of 16 x 24)
# ---------------------------------------------------------------------------------------------
CASE_S = 8
CASE_SIZES = ((16, 24), (17, 25), (37, 53), (64, 40), (121, 200))


def case_images(seed=11):
    """Five images of seeded random content and one ramp whose neighbouring pixels all differ, so that a tap one off shows."""
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in CASE_SIZES]
    y, x, c = np.meshgrid(np.arange(40), np.arange(56), np.arange(3), indexing='ij')
    images.append(((x * 3 + y * 37 + c * 101) % 251).astype(np.uint8))
    return images


def case_table(images, S=CASE_S, seed=12):
    """Per image: identity, the three flips, an integer translation, 90 and 180 degrees at scale 1, the four extreme draws, a
    rotated window at each of the four corner origins, colour shifts saturating both ways, two seeded random plans.
    Returns a dict of arrays (image, flags, minv, rgb, crop) and the list of case names."""
    rng = np.random.default_rng(seed)
    rows, names = [], []

    def add(name, k, flags, minv=IDENTITY, rgb=(0.0, 0.0, 0.0), crop=(0, 0)):
        rows.append((k, flags, tuple(float(v) for v in minv), tuple(float(np.float32(v)) for v in rgb), (int(crop[0]), int(crop[1]))))
        names.append(f'{name}/image{k}')

    for k, img in enumerate(images):
        H, W, _ = img.shape
        ry, rx = H - 2 * S, W - 3 * S
        mid = (ry // 2, rx // 2)
        inv = lambda *a: invert_affine(forward_matrix(H, W, *a))
        add('identity', k, 0, crop=mid)
        add('hflip', k, HFLIP, crop=(0, rx))
        add('vflip', k, VFLIP, crop=(ry, 0))
        add('both-flips', k, HFLIP | VFLIP, crop=mid)
        add('translate', k, WARP | HFLIP, minv=(1, 0, 3, 0, 1, -2), crop=(0, rx))
        add('rot90', k, WARP, minv=inv(90.0, 1.0, 0.0, 0.0), crop=mid)
        add('rot180', k, WARP | VFLIP, minv=inv(180.0, 1.0, 0.0, 0.0), crop=(ry, rx))
        for j, (ang, sc, dx, dy) in enumerate(((20.0, 0.85, 0.05, 0.05), (-20.0, 1.15, -0.05, -0.05), (20.0, 1.15, -0.05, 0.05),
                                               (-20.0, 0.85, 0.05, -0.05))):
            add(f'extreme{j}', k, WARP | (HFLIP if j & 1 else 0) | (COLOUR if j & 2 else 0), minv=inv(ang, sc, dx, dy),
                rgb=(-15.0, 15.0, 3.25), crop=mid if j < 2 else (0, 0))
        for j, origin in enumerate(((0, 0), (0, rx), (ry, 0), (ry, rx))):
            add(f'corner{j}', k, WARP | (VFLIP if j & 1 else 0), minv=inv(7.0, 1.05, 0.01, -0.02), crop=origin)
        add('colour-up', k, COLOUR, rgb=(15.0, 14.999999, 300.0), crop=mid)
        add('colour-down', k, COLOUR | HFLIP, rgb=(-15.0, -0.5, -300.0), crop=mid)
        for j in range(2):
            u = rng.random(13).astype(np.float32)
            u[2] = 0.25                                        # the warp is on: the plain paths have their own cases above
            flags, _, minv, rgb, crop = plan_sample(u, H, W, S)
            add(f'random{j}', k, flags, minv=minv, rgb=rgb, crop=crop)
    table = {'image': np.array([r[0] for r in rows], dtype=np.int32), 'flags': np.array([r[1] for r in rows], dtype=np.int32),
             'minv': np.array([r[2] for r in rows], dtype=np.float64), 'rgb': np.array([r[3] for r in rows], dtype=np.float32),
             'crop': np.array([r[4] for r in rows], dtype=np.int32)}
    return table, names
