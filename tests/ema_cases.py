"""The parameter-EMA rule of csrc/optim_update.h (ema_decay_at, ema_blend) as numpy fp32 code, and the small parameter set the EMA
tests run on.  Every operation below is one IEEE fp32 operation on fp32 operands, in the order the header states them:

    d_t = warmup ? min(d, (1 + n) / (10 + n)) : d
    e'  = fl( fl(d_t * e) + fl((1.0f - d_t) * p') )

so a device that follows the header agrees bit for bit.  No torch, no GPU."""
import numpy as np

F = np.float32

# Every tiling edge of the 64 x 64 update tile: one element, a 1-D tail (65 = 64 + 1, no 16-byte rows), exactly one tile, a tail in both
# directions with an odd row length (63: no vector access, rows of the transposed shadow of 65), and 3 x 2 tiles with a row length that
# is no multiple of 4 (70) under rows that are none either (130).
SHAPES = [(1,), (65,), (64, 64), (65, 63), (130, 70)]
NUMEL = [int(np.prod(s)) for s in SHAPES]
TOTAL = sum(NUMEL)


def decay_at(d, warmup, n):
    """The decay of the update after ``n`` EMA updates (fp32)."""
    d, n = F(d), F(n)
    if warmup:
        w = (F(1.0) + n) / (F(10.0) + n)
        d = w if w < d else d
    return F(d)


def blend(dt, e, p):
    """e' for fp32 arrays ``e`` and ``p`` (the new parameter): two rounded products, one rounded sum."""
    dt = F(dt)
    e, p = np.asarray(e, dtype=F), np.asarray(p, dtype=F)
    keep = dt * e
    take = (F(1.0) - dt) * p
    assert keep.dtype == F and take.dtype == F
    return keep + take


def update(e, p, d, warmup, n):
    """One EMA update: the new average and the new count."""
    return blend(decay_at(d, warmup, n), e, p), n + 1


def swap(p, e):
    """vited_ema_swap on one parameter [rows, cols]: (new p, new e, bf16-rounded source of shadow, of shadow_t) - the shadows are the
    new p, and its transpose, cast to bf16 by the caller's own cast."""
    return e.copy(), p.copy(), e.copy(), np.ascontiguousarray(e.T)


def initial_parameters():
    """fp32 arrays of SHAPES: a closed form of the flat index, magnitudes of trained weights (|p| <= 0.12), no two equal neighbours."""
    i = np.arange(TOTAL, dtype=np.float64)
    flat = (0.1 * np.sin(0.37 * i + 0.5) + 0.02 * np.cos(1.91 * i)).astype(F)
    out, at = [], 0
    for shape, n in zip(SHAPES, NUMEL):
        out.append(flat[at: at + n].reshape(shape).copy())
        at += n
    return out


def gradient(step, numel=TOTAL):
    """The flat gradient of update ``step`` (0-based): a closed form of the flat index, fp32 [numel].  Update 1 is large (norm about 3e2), so that
    a clip at norm 1.0 is active; the others (norm about 0.4) stay below it."""
    i = np.arange(numel, dtype=np.float64)
    scale = 3.0 if step == 1 else 0.004
    return (scale * np.sin(0.113 * i + 1.3 * step + 0.25) * (1.0 + 0.5 * np.cos(0.0071 * i * (step + 1)))).astype(F)
