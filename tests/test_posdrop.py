"""Position dropout, the parts that need no GPU: the constructor surface, the mask rule (Philox4x32-10 known answers, thresholds,
statistics, streams, keep tables), the seeds' draw and bookkeeping, the pin of the composition in tests/posdrop_cases.py against what
the reference's own class computed (tests/golden/pos_drop.npz), the argument checks of ``vited_token_dropout`` before any launch,
and the fake kernel of ``torch.ops.vited.token_dropout``."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import patchdrop_cases as pc
import posdrop_cases as pd
from oracle import vited_oracle as vo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pos_drop.npz')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = pc.GOLDEN_SHAPE            # 16-pixel images, 4 patches, 64 channels


def _model(vited, rate, s=SMALL, **kw):
    return vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                         embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads,
                                         pos_drop_rate=rate, **kw)


# ---- the constructor ----------------------------------------------------------------------------------------------------------------
def test_constructor_takes_the_rate(vited):
    """What fails without the feature (NotImplementedError from the constructor's catch-all): 0.1 and 0.5 are accepted, 1.0 and -0.1
    are not; None and 0 are off; no parameter and no state_dict key; the options that stay refused still say so beside it."""
    for rate in (0.1, 0.5):
        m = _model(vited, rate)
        assert m.pos_drop_rate == rate and m.last_pos_drop is None and m.pos_drop_generator is None
    assert _model(vited, 0.).pos_drop_rate == 0. and _model(vited, None).pos_drop_rate == 0.
    for rate in (1.0, -0.1):
        with pytest.raises(ValueError, match='pos_drop_rate'):
            _model(vited, rate)
    assert list(_model(vited, 0.5).state_dict()) == list(_model(vited, 0.).state_dict())
    assert [n for n, _ in _model(vited, 0.5).named_modules()] == [n for n, _ in _model(vited, 0.).named_modules()]
    for name, value in (('init_values', 1e-5), ('drop_rate', 0.1), ('attn_drop_rate', 0.1), ('proj_drop_rate', 0.1), ('no_embed_class', True),
                        ('pre_norm', True)):
        with pytest.raises(NotImplementedError, match=name):
            _model(vited, 0.5, **{name: value})


def test_build_model_forwards_the_rate(vited):
    cfg = vited.config_from_yaml(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs', 'test',
                                              'test_pjs_hisfrag20_patch32_64.yaml'))
    assert vited.build_model(cfg).pos_drop_rate == 0.
    assert vited.build_model(cfg, pos_drop_rate=0.1).pos_drop_rate == 0.1
    assert 'token_dropout' in vited.custom_ops.OPERATORS and vited.ops.token_dropout.__module__.endswith('ops_tokendrop')


# ---- the rule -----------------------------------------------------------------------------------------------------------------------
KNOWN_ANSWERS = [      # counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers(vited):
    for counter, key, want in KNOWN_ANSWERS:
        got = vited.ops.philox4x32(np.array(counter, dtype=np.uint32), key)
        assert got.dtype == np.uint32 and tuple(int(v) for v in got) == want
    stacked = vited.ops.philox4x32(np.zeros((3, 2, 4), dtype=np.uint32), (0, 0))                                   # vectorised
    assert stacked.shape == (3, 2, 4) and all(tuple(int(v) for v in row) == KNOWN_ANSWERS[0][2] for row in stacked.reshape(6, 4))


def test_threshold_and_scale(vited):
    thr = vited.ops.dropout_threshold
    assert thr(0.1)[0] == 429496729 and thr(0.25)[0] == 1073741824 and thr(0.5)[0] == 2147483648 and thr(0.)[0] == 0
    assert thr(1. - 2. ** -40)[0] == 2 ** 32 - 1                                        # the cap
    for p in (0.1, 0.25, 0.5):
        assert thr(p)[1] == float(np.float32(1.0 / (1.0 - p)))
    assert thr(0.1)[1] == 1.1111111640930176 and thr(0.5)[1] == 2.0 and thr(0.)[1] == 1.0
    for p in (1.0, -0.1):
        with pytest.raises(ValueError):
            thr(p)


def test_the_mask_is_the_rule_element_by_element(vited):
    """A handful of elements of a mask against the rule written out one element at a time (Python integers)."""
    ops = vited.ops
    seed, p, batch, tokens, dim, stream = -987654321987654321, 0.25, 3, 5, 36, 1
    mask = ops.token_dropout_mask(seed, p, batch, tokens, dim, stream)
    assert mask.shape == (batch, tokens, dim) and mask.dtype == torch.bool
    thr, _ = ops.dropout_threshold(p)
    useed = seed & (2 ** 64 - 1)
    for b, t, d in ((0, 0, 0), (0, 0, 3), (0, 1, 4), (1, 2, 17), (2, 4, 35), (2, 0, 1)):
        e = (b * tokens + t) * dim + d
        g = e >> 2
        words = ops.philox4x32(np.array([g & 0xffffffff, g >> 32, stream, 0], dtype=np.uint32), (useed & 0xffffffff, useed >> 32))
        assert bool(mask[b, t, d]) == (int(words[e & 3]) >= thr), (b, t, d)


SEEDS = {0.1: 11, 0.25: 12, 0.5: 13}


@pytest.mark.parametrize('p', sorted(SEEDS))
def test_kept_fraction(vited, p):
    """[2, 65, 384] = 49,920 elements: the kept fraction lies within 5 binomial standard deviations of 1 - thr / 2^32 (at p = 0.25:
    +-0.0097) at the fixed seed of each rate."""
    ops = vited.ops
    mask = ops.token_dropout_mask(SEEDS[p], p, 2, 65, 384, 1)
    n = mask.numel()
    q = 1.0 - ops.dropout_threshold(p)[0] / 2.0 ** 32
    bound = 5 * math.sqrt(q * (1 - q) / n)
    got = float(mask.double().mean())
    print(f'p = {p}: kept {got:.5f}, expected {q:.5f} +- {bound:.5f}')
    assert n == 49920 and abs(got - q) <= bound
    if p == 0.25:
        assert abs(bound - 0.0097) < 5e-5


def test_streams_seeds_and_keep_tables(vited):
    ops = vited.ops
    full = ops.token_dropout_mask(12, 0.25, 2, 65, 384, 1)
    assert not torch.equal(full, ops.token_dropout_mask(12, 0.25, 2, 65, 384, 0))      # the streams of one seed differ
    assert not torch.equal(full, ops.token_dropout_mask(13, 0.25, 2, 65, 384, 1))      # and so do two seeds
    assert torch.equal(full, ops.token_dropout_mask(torch.tensor([12]), 0.25, 2, 65, 384, 1))      # a seed tensor is its value
    # a kept row under a table carries the mask of its original token: image-2 form (cls + patches keep + 1) ...
    keep2 = pc.closed_form_keep(2, 64, 32, salt=2)
    kept = ops.token_dropout_mask(12, 0.25, 2, 65, 384, 1, keep=keep2, lead=False)
    assert kept.shape == (2, 33, 384) and torch.equal(kept, pc.gather_kept(full, keep2))
    # ... and image-1 form (patch 0 + patches 1 + keep) of the stream without a cls token
    full1 = ops.token_dropout_mask(12, 0.25, 2, 64, 384, 0)
    keep1 = pc.closed_form_keep(2, 63, 31, salt=1)
    kept1 = ops.token_dropout_mask(12, 0.25, 2, 64, 384, 0, keep=keep1.int(), lead=True)
    assert kept1.shape == (2, 32, 384) and torch.equal(kept1, pc.gather_kept(full1, keep1))
    # the CPU op applies it: kept elements scaled by the fp32 scale, dropped ones 0 whatever they held
    x = torch.randn(2, 65, 384, generator=torch.Generator().manual_seed(1))
    dropped = (~full).nonzero()
    x[tuple(dropped[0])], x[tuple(dropped[-1])] = float('inf'), float('nan')            # in dropped positions: they come out 0
    y = ops.token_dropout(x, 12, 0.25, 65, 1)
    scale = torch.tensor(ops.dropout_threshold(0.25)[1], dtype=torch.float32)
    assert torch.equal(y[full], (x * scale)[full])
    assert int(torch.count_nonzero(y[~full])) == 0 and not bool(y[~full].isnan().any())
    yb = ops.token_dropout(x.bfloat16(), 12, 0.25, 65, 1)
    assert yb.dtype == torch.bfloat16 and torch.equal(yb[full], (x.bfloat16().float() * scale).bfloat16()[full])
    assert int(torch.count_nonzero(yb[~full])) == 0
    assert torch.equal(ops.token_dropout(pc.gather_kept(x, keep2), 12, 0.25, 65, 1, keep=keep2), pc.gather_kept(y, keep2))
    with pytest.raises(ValueError, match='token_dropout'):
        ops.token_dropout(x, 12, 0.25, 64, 1)                                            # 65 rows of a 64-token stream, no table


# ---- seeds --------------------------------------------------------------------------------------------------------------------------
def test_draw_on_the_cpu(vited):
    m = _model(vited, 0.1)
    seeds = m.draw_pos_drop(True, True, generator=torch.Generator().manual_seed(5))
    assert isinstance(seeds, vited.PosDropSeeds)
    for t in seeds:
        assert t.dtype == torch.int64 and t.shape == (1,) and t.device.type == 'cpu'
    assert int(seeds.x1) != int(seeds.x2)
    again = m.draw_pos_drop(True, True, generator=torch.Generator().manual_seed(5))
    assert torch.equal(again.x1, seeds.x1) and torch.equal(again.x2, seeds.x2)
    half = m.draw_pos_drop(None, True)
    assert half.x1 is None and half.x2.shape == (1,)
    assert m.draw_pos_drop(True, False).x2 is None


def test_custom_generator_is_refused_inside_a_capture(vited, monkeypatch):
    m = _model(vited, 0.1)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError, match='default generator'):
        m.draw_pos_drop(True, True, generator=torch.Generator(), device='cuda')


def test_forward_records_the_seeds(vited, monkeypatch):
    """The launches are stubbed out: what reaches the Functions and what ``last_pos_drop`` holds, per mode."""
    m = _model(vited, 0.5).eval()
    seen = []
    monkeypatch.setattr(m, '_check_images', lambda img: None)
    monkeypatch.setattr(m, '_run_fn', lambda fn, drop, keep, pdrop, *args: seen.append(pdrop) or torch.zeros(2, 4, 64))
    x = torch.zeros(2, 2, 3, 16, 16)
    m.last_pos_drop = 'stale'
    m(x)
    assert seen == [None, None] and m.last_pos_drop is None                            # eval() never drops
    m.train()
    m(x)
    assert seen[2] is seen[3] and seen[2][2] == 0.5 and m.last_pos_drop == vited.PosDropSeeds(seen[2][0], seen[2][1])
    assert seen[2][0].dtype == torch.int64 and seen[2][0].shape == (1,) and seen[2][1].shape == (1,)
    m.keep_cam = True                                                                    # a relevancy backward never drops
    m(x)
    assert seen[-1] is None and m.last_pos_drop is None
    m.keep_cam = False
    forced = vited.PosDropSeeds(torch.tensor([7]), torch.tensor([-9]))
    m.eval()(x, pos_drop=forced)                                                         # explicit seeds hold in any mode
    assert seen[-1] == (forced.x1, forced.x2, 0.5) and m.last_pos_drop.x1 is forced.x1 and m.last_pos_drop.x2 is forced.x2
    # a two-stage step: each call records its half and leaves the other's in place
    other = vited.PosDropSeeds(torch.tensor([21]), None)
    m(x[:, 0], forward_first_part=True, pos_drop=other)
    assert seen[-1] == (other.x1, None, 0.5) and m.last_pos_drop.x1 is other.x1 and m.last_pos_drop.x2 is forced.x2
    m(torch.zeros(2, 4, 64), x[:, 1], pos_drop=vited.PosDropSeeds(None, forced.x1))
    assert seen[-1][0] is None and m.last_pos_drop.x1 is other.x1 and m.last_pos_drop.x2 is forced.x1
    for bad in (vited.PosDropSeeds(forced.x1, None), vited.PosDropSeeds(forced.x1.int(), forced.x2),
                vited.PosDropSeeds(torch.zeros(2, dtype=torch.int64), forced.x2), vited.PosDropSeeds(5, forced.x2)):
        with pytest.raises(ValueError, match='pos_drop'):
            m(x, pos_drop=bad)
    off = _model(vited, 0.).train()
    monkeypatch.setattr(off, '_check_images', lambda img: None)
    monkeypatch.setattr(off, '_run_fn', lambda fn, drop, keep, pdrop, *args: seen.append(pdrop) or torch.zeros(2, 4, 64))
    off(x)
    assert seen[-1] is None and off.last_pos_drop is None                              # rate 0 never drops


def test_train_step_hands_forced_seeds_on(vited):
    m = _model(vited, 0.1)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    step = vited.engine.TrainStep(m, opt, use_graph=False, amp=False)
    assert step.pos_drop is None and 'pos_drop' not in step._forced()
    step.pos_drop = vited.PosDropSeeds(torch.tensor([1]), torch.tensor([2]))
    assert step._forced()['pos_drop'] is step.pos_drop


# ---- the composition against the reference's class ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(pd.GOLDEN_SHAPES))
def test_composition_matches_the_reference_fixture(vited, name):
    """fp64, closed-form weights, the masks of the rule at fixed seeds: logits, loss and every parameter gradient of posdrop_cases'
    composition equal what the reference's VisionTransformerCustom(pos_drop_rate=0.25) gave with its ``pos_drop`` forced to the same
    masks; the masks in the file are the rule's at the file's seeds."""
    fx = np.load(GOLDEN)
    s = pd.GOLDEN_SHAPES[name]
    x, y = pd.golden_inputs(name)
    seeds = tuple(int(v) for v in fx[f'{name}.seeds'])
    assert seeds == pd.GOLDEN_SEEDS[name] and float(fx['rate']) == pd.GOLDEN_RATE
    thr, scale = vited.ops.dropout_threshold(pd.GOLDEN_RATE)
    assert int(fx['thr']) == thr and float(fx['scale']) == scale
    mask1, mask2, _ = pd.masks_of(vited.ops, seeds, pd.GOLDEN_RATE, pd.GOLDEN_BATCH, pd.GOLDEN_BATCH, s)
    np.testing.assert_array_equal(fx[f'{name}.mask1'], np.packbits(mask1.numpy()))
    np.testing.assert_array_equal(fx[f'{name}.mask2'], np.packbits(mask2.numpy()))
    m = vo.fill_closed_form_(vo.OracleViTED(s)).double()
    logits = pd.forward_dropped(m, x.double(), mask1, mask2, scale)
    loss, grads = pd.loss_and_grads(m, logits, y.double())
    np.testing.assert_allclose(logits.detach().numpy(), fx[f'{name}.logits'], rtol=1e-9, atol=0)
    np.testing.assert_allclose(loss.numpy(), fx[f'{name}.loss'], rtol=1e-9)
    names = [str(n) for n in fx[f'{name}.grad_names']]
    assert names == [n for n, _ in m.named_parameters()]
    norms = np.array([float(grads[n].norm()) for n in names])
    np.testing.assert_allclose(norms, fx[f'{name}.grad_norms'], rtol=1e-9)
    for n, norm, want in zip(names, fx[f'{name}.grad_norms'], fx[f'{name}.grad_slices']):
        got = grads[n].reshape(-1)[:16].numpy()
        np.testing.assert_allclose(got, want[:got.size], rtol=1e-9, atol=1e-9 * norm, err_msg=n)
    # the mask matters: the same weights without it give other logits
    assert not np.allclose(m(x.double()).detach().numpy(), fx[f'{name}.logits'], rtol=1e-3)
    # ForcedPosDrop is the same multiply
    tok = m._patch_tokens(x[:, 0].double()) + m.pos_embed[:, 1:]
    assert torch.equal(pd.ForcedPosDrop(mask1.double() * scale)(tok), tok * pd.multiplier(mask1, scale, tok))


# ---- the entry point ----------------------------------------------------------------------------------------------------------------
def test_entry_point_checks_its_arguments(vited):
    """Every bad-argument and unsupported case of vited_token_dropout returns its code before any launch (no GPU here: a launch would
    fail differently)."""
    lib = vited._lib.load()
    C = ctypes
    assert vited._lib.SIGNATURES['vited_token_dropout'] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                                                       C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                                       C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_float, C.c_void_p])
    BAD, UNSUPPORTED = 1, 2
    buf = (ctypes.c_float * 65536)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    q = p + 131072                                        # a second operand that lies apart
    F32, BF16 = vited._lib.F32, vited._lib.BF16

    def call(x=p, x_bs=5 * 64, x_rs=64, out=q, out_bs=5 * 64, out_rs=64, dtype=F32, batch=2, rows=5, dim=64, tokens=5, stream=0, keep=None,
             K=0, lead=0, seed=p, thr=429496729, scale=1.25):
        return lib.vited_token_dropout(x, x_bs, x_rs, out, out_bs, out_rs, dtype, batch, rows, dim, tokens, stream, keep, K, lead, seed, thr,
                                       scale, None)

    assert call(x=None) == BAD and call(out=None) == BAD and call(seed=None) == BAD                    # null operands
    assert call(batch=0) == BAD and call(rows=0, tokens=0) == BAD and call(dim=0) == BAD
    assert call(dim=62, x_rs=62, out_rs=62) == BAD                                                     # dim % 4
    assert call(x_rs=60) == BAD and call(out_rs=32) == BAD                                             # rows would overlap
    assert call(x_bs=4 * 64) == BAD and call(out_bs=64) == BAD                                         # samples would overlap
    assert call(x_rs=66, x_bs=5 * 66) == BAD and call(out_bs=5 * 64 + 2) == BAD                        # strides that break the vectors
    assert call(x=p + 4) == BAD and call(out=q + 8) == BAD and call(seed=p + 4) == BAD                 # misaligned pointers
    assert call(dtype=BF16, x=p + 4) == BAD and call(dtype=BF16, out=q + 2) == BAD                     # bf16: four elements are 8 bytes
    assert call(out=p + 64 * 4) == BAD                                                                 # overlapping, not in place
    assert call(thr=-1) == BAD and call(thr=2 ** 32) == BAD                                            # thr outside [0, 2^32 - 1]
    assert call(stream=2) == BAD and call(stream=-1) == BAD
    assert call(rows=4) == BAD and call(tokens=6) == BAD                                               # no table: rows == tokens
    assert call(keep=p, K=3, tokens=9) == BAD and call(keep=p, K=5, tokens=9) == BAD                   # a table's K + 1 == rows
    assert call(keep=p, K=4, tokens=4) == BAD                                                          # more rows than tokens
    assert call(keep=p, K=4, tokens=9, lead=2) == BAD and call(keep=p + 2, K=4, tokens=9) == BAD
    assert call(dtype=vited._lib.F16) == UNSUPPORTED and call(dtype=vited._lib.I32) == UNSUPPORTED     # other dtypes
    assert call(dim=1028, x_rs=1028, out_rs=1028, x_bs=5 * 1028, out_bs=5 * 1028) == UNSUPPORTED       # wider than a LayerNorm row


def test_fake_kernel(vited):
    x = torch.empty(3, 65, 384, device='meta')
    seed = torch.empty(1, dtype=torch.int64, device='meta')
    y = torch.ops.vited.token_dropout(x, seed, 0.1, 65, 1, None, False)
    assert y.shape == x.shape and y.dtype == x.dtype and y.device.type == 'meta'
    keep = torch.empty(3, 32, dtype=torch.int32, device='meta')
    yb = torch.ops.vited.token_dropout(x.bfloat16()[:, :33], seed, 0.1, 65, 1, keep, False)
    assert yb.shape == (3, 33, 384) and yb.dtype == torch.bfloat16
    with pytest.raises(NotImplementedError):
        torch.ops.vited.token_dropout(torch.zeros(1, 2, 4), torch.zeros(1, dtype=torch.int64), 0.1, 2, 0, None, False)     # no CPU kernel


def test_host_check_runs_clean_under_the_sanitizers(tmp_path):
    """tools/tokendrop_host_check.cpp: the text of csrc/token_dropout.h driven in the kernel's schedule over exactly-sized heap buffers
    against a scalar Philox written out a second time - a stand-alone program with its own main, built with
    -fsanitize=address,undefined."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    cxx = next((c for c in (shutil.which('clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'))
                if c and os.path.exists(c)), None)
    assert cxx is not None, 'no clang++ beside hipcc: the HIP toolchain that builds the library ships one'
    exe = str(tmp_path / 'tokendrop_host_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                    os.path.join(ROOT, 'vit-ed_amd', 'csrc'), os.path.join(ROOT, 'tools', 'tokendrop_host_check.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'tokendrop_host_check ok' in run.stdout and not run.stderr.strip(), run.stdout + run.stderr
