"""Exact operands for the GEMM parity tests: small integers (and integers / 16), so that every product and every partial sum of
a contraction is a multiple of 2^-4 below 2^20 and therefore an fp32 number.  The fp32 accumulator of such a GEMM is the same number
in ANY summation order, tile shape, split-K plan or MFMA variant: fp32 outputs must equal the fp64 product bit for bit and bf16
outputs its single correct rounding (to nearest, ties to even).  No tolerance is involved; `guard_*` states the condition on the
INPUTS under which that holds, and every case calls it before it trusts the truth.

Plain torch and device-agnostic: tests/test_exact_cases.py checks it on the CPU (the truth is order-free, the outputs need rounding
and hit ties, each torch-restated kernel defect differs from the truth), tests/test_gpu_exact.py moves the tensors to the device and
drives the kernels with them (the fp64 truth of the large cases is computed there, in row slices).
"""
import torch

UNIT = 16                   # every operand is an integer / UNIT (a multiple of 2^-4)
EXACT_LIMIT = 2 ** 24       # integers below it are fp32 numbers

# |integer| ranges; w, bias and residual are divided by UNIT
SCALES = {
    'wide': dict(a=8, w=32, bias=64, residual=512),
    # pre-activations of spread ~4.5 at K = 384 (measured on the CPU): the GELU-valued outputs see both tails and the middle
    'gelu': dict(a=2, w=4, bias=16, residual=0),
}
GRAD_RANGE = 8              # dy and x of a weight gradient: integers in [-8, 8]
LN_BWD_RANGES = (2, 8)      # vited_linear_layernorm_bwd: dy integers in [-2, 2], wt integers in [-8, 8] / 16


def bf(t):
    """Round to bf16, keep the dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def ints(shape, bound, gen, div=1):
    """fp32 integers drawn uniformly from [-bound, bound], divided by ``div``."""
    return torch.randint(-bound, bound + 1, tuple(shape), generator=gen).float() / div


def nt_operands(M, N, K, seed, scale='wide', residual=True):
    """a [M, K], w [N, K], bias [N], residual [M, N] (fp32 tensors holding the exact values) of out = a w^T + bias (+ residual);
    ``residual=False`` leaves the [M, N] draw out (the large plain-store cases)."""
    r = SCALES[scale]
    gen = torch.Generator().manual_seed(seed)
    out = dict(a=ints((M, K), r['a'], gen), w=ints((N, K), r['w'], gen, UNIT), bias=ints((N,), r['bias'], gen, UNIT))
    if residual:
        out['residual'] = ints((M, N), r['residual'], gen, UNIT)
    return out


def mul_aux(M, N, seed):
    """The second factor of EPI_MUL: randn rounded to bf16 (8 significant bits; guard_nt checks that z * aux still fits fp32)."""
    return bf(torch.randn(M, N, generator=torch.Generator().manual_seed(seed)))


def wgrad_operands(M, N, K, seed):
    """dy [M, N], x [M, K] of dW = dy^T x, dbias = column sums of dy."""
    gen = torch.Generator().manual_seed(seed)
    return ints((M, N), GRAD_RANGE, gen), ints((M, K), GRAD_RANGE, gen)


def ln_bwd_operands(M, N, K, seed):
    """dy [M, K], wt [N, K] of dh = dy wt^T, whose column sum over the rows is the dbeta of vited_linear_layernorm_bwd."""
    gen = torch.Generator().manual_seed(seed)
    return ints((M, K), LN_BWD_RANGES[0], gen), ints((N, K), LN_BWD_RANGES[1], gen, UNIT)


# ---------------------------------------------------------------------------------------------
# the guard: a condition on the inputs, not a measurement of any output
# ---------------------------------------------------------------------------------------------
def _on_grid(name, t):
    assert bool(torch.equal(t * UNIT, torch.round(t * UNIT))), f'{name} is not a multiple of 1 / {UNIT}'


def _bf16_exact(name, t):
    assert bool(torch.equal(bf(t), t)), f'{name} does not survive a round trip through bf16'


def _slices(rows, chunk):
    return [(r0, min(rows, r0 + chunk)) for r0 in range(0, rows, chunk)]


def guard_nt(a, w, bias=None, residual=None, aux=None, chunk=8192):
    """out = a w^T + bias + residual is exact in fp32 in any order:
      * a, w, bias (and aux) survive a round trip through bf16, so the bf16 kernels, the fp32 kernels and the truth see the same
        numbers; the residual is an fp32 stream in every kernel and is held to the 1 / 16 grid only;
      * everything is a multiple of 1 / 16 and max(|a| |w|^T + |bias| + |residual|) * 16 < 2^24: every partial sum, in whatever
        order and grouping, is an integer / 16 below 2^24 / 16 in magnitude - an fp32 number;
      * with aux (EPI_MUL): z * aux, exact in fp64, survives a round trip through fp32, so the fp32 product of the epilogue is exact
        and its bf16 store is the ONE rounding of the output.
    -> the bound max(...) * 16, for the record."""
    for name, t in (('a', a), ('w', w), ('bias', bias), ('aux', aux)):
        if t is not None:
            _bf16_exact(name, t)
    for name, t in (('a', a), ('w', w), ('bias', bias), ('residual', residual)):
        if t is not None:
            _on_grid(name, t)
    worst = 0.0
    wd = w.double()
    for r0, r1 in _slices(a.shape[0], chunk):
        mag = a[r0:r1].double().abs() @ wd.abs().t()
        z = a[r0:r1].double() @ wd.t()
        if bias is not None:
            mag, z = mag + bias.double().abs(), z + bias.double()
        if residual is not None:
            mag = mag + residual[r0:r1].double().abs()
        worst = max(worst, float(mag.max()) * UNIT)
        if aux is not None:
            p = z * aux[r0:r1].double()
            assert bool(torch.equal(p.float().double(), p)), 'z * aux does not survive a round trip through fp32'
    assert worst < EXACT_LIMIT, f'|a| |w|^T + |bias| + |residual| reaches {worst / UNIT}: a partial sum may round in fp32'
    return worst


def guard_wgrad(dy, x, dw0=None, db0=None, chunk=256):
    """dW = dw0 + dy^T x and dbias = db0 + column sums of dy are exact in fp32 in any order: operands bf16-exact and on the grid,
    max(|dw0| + |dy|^T |x|) * 16 < 2^24 and max(|db0| + sum_rows |dy|) * 16 < 2^24.  -> the bound."""
    for name, t in (('dy', dy), ('x', x)):
        _bf16_exact(name, t)
        _on_grid(name, t)
    for name, t in (('dw0', dw0), ('db0', db0)):
        if t is not None:
            _on_grid(name, t)
    xd = x.double().abs()
    worst = 0.0
    for c0, c1 in _slices(dy.shape[1], chunk):
        mag = dy[:, c0:c1].double().abs().t() @ xd
        if dw0 is not None:
            mag = mag + dw0[c0:c1].double().abs()
        worst = max(worst, float(mag.max()) * UNIT)
    col = dy.double().abs().sum(0)
    if db0 is not None:
        col = col + db0.double().abs()
    worst = max(worst, float(col.max()) * UNIT)
    assert worst < EXACT_LIMIT, f'|dy|^T |x| reaches {worst / UNIT}: a partial sum may round in fp32'
    return worst


def guard_colsum(t, base=None):
    """base + column sums of t (fp64 or fp32 values on the 1 / 16 grid) are exact in fp32 in any order and grouping:
    max(|base| + sum_rows |t|) * 16 < 2^24.  -> the bound."""
    _on_grid('summand', t)
    col = t.double().abs().sum(0)
    if base is not None:
        _on_grid('base', base)
        col = col + base.double().abs()
    worst = float(col.max()) * UNIT
    assert worst < EXACT_LIMIT, f'sum_rows |t| reaches {worst / UNIT}: a partial sum may round in fp32'
    return worst


# ---------------------------------------------------------------------------------------------
# the truth: exact in fp64 (every value is an integer / 16 far below 2^53), then the output format's one rounding
# ---------------------------------------------------------------------------------------------
def nt_truth(a, w, bias=None, residual=None, chunk=8192):
    """fp64 a w^T + bias + residual, built in row slices."""
    wd = w.double()
    parts = []
    for r0, r1 in _slices(a.shape[0], chunk):
        z = a[r0:r1].double() @ wd.t()
        if bias is not None:
            z = z + bias.double()
        if residual is not None:
            z = z + residual[r0:r1].double()
        parts.append(z)
    return torch.cat(parts)


def as_f32(truth):
    """What an fp32 output must hold: the truth itself (it is an fp32 number)."""
    return truth.float()


def as_bf16(truth):
    """What a bf16 output must hold: the fp32 accumulator (= the truth) rounded once, to nearest even."""
    return truth.float().bfloat16()


def as_dtype(truth, dtype):
    return as_f32(truth) if dtype == torch.float32 else as_bf16(truth)


def mul_truth(z, aux, dtype=torch.bfloat16):
    """EPI_MUL: the fp32 product z * aux (exact under guard_nt) in the output format."""
    return as_dtype(z * aux.double(), dtype)


def wgrad_truth(dy, x, dw0=None, db0=None):
    """fp64 (dw0 + dy^T x, db0 + column sums of dy)."""
    dw = dy.double().t() @ x.double()
    db = dy.double().sum(0)
    if dw0 is not None:
        dw = dw + dw0.double()
    if db0 is not None:
        db = db + db0.double()
    return dw, db


# ---------------------------------------------------------------------------------------------
# what the operands exercise
# ---------------------------------------------------------------------------------------------
def _bits(x32):
    return x32.contiguous().view(torch.int32)


def needs_rounding(x32):
    """Elementwise: the fp32 value is not a bf16 number."""
    return (_bits(x32) & 0xFFFF) != 0


def is_tie(x32):
    """Elementwise: the fp32 value lies exactly half way between two neighbouring bf16 numbers."""
    return (_bits(x32) & 0xFFFF) == 0x8000


# ---------------------------------------------------------------------------------------------
# torch restatements of kernel defects (the mutants of tests/test_exact_cases.py)
# ---------------------------------------------------------------------------------------------
def store_truncating(x32):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero)."""
    return (_bits(x32) & -65536).view(torch.float32).bfloat16()


def store_half_away(x32):
    """fp32 -> bf16 to nearest, halves away from zero (add 0x8000 to the magnitude, then truncate)."""
    return ((_bits(x32) + 0x8000) & -65536).view(torch.float32).bfloat16()


def mul_double_rounding(z32, aux):
    """EPI_MUL that rounds z = acc + bias to bf16 before the multiply."""
    return (bf(z32) * aux).bfloat16()


def k_halves_through_bf16(a, w, bias=None):
    """The partial sum over the first half of K handed to the second half in bf16."""
    h = a.shape[1] // 2
    acc = bf(a[:, :h] @ w[:, :h].t()) + a[:, h:] @ w[:, h:].t()
    return (acc if bias is None else acc + bias).bfloat16()


def ragged_tile_drops_k(a, w, bias=None, tile=128, drop=8):
    """The rows of the last, ragged row tile lose their last ``drop`` k-columns."""
    acc = a @ w.t()
    r0 = (a.shape[0] // tile) * tile
    acc[r0:] = a[r0:, :-drop] @ w[:, :-drop].t()
    return (acc if bias is None else acc + bias).bfloat16()


def wgrad_last_row_twice(dy, x):
    """dW with the last row of the contraction counted twice."""
    return dy.t() @ x + torch.outer(dy[-1], x[-1])


def bias_grad_row_left_out(dy, row):
    """dbias without row ``row``."""
    return dy.sum(0) - dy[row]
