"""CPU: Muon's restatement (tests/muon_cases.py) against torch.optim.Muon, FlatMuon's constructor, group words, state_dict and its three
loading paths on unbound optimizers, engine.build_optimizer's refusal off the HIP path, the Muon entries of the C ABI, the workspace size,
the tile tables, and the host build of the elementwise bodies (tools/muon_host_check.cpp) under the address and undefined-behaviour
sanitizers."""
import math
import os
import re
import shutil
import subprocess
import types
from unittest import mock

import pytest
import torch

import lamb_cases as lc
import muon_cases as mc
from test_abi import _ensure_built

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nesterov', [True, False])
@pytest.mark.parametrize('adjust_lr_fn', [None, 'match_rms_adamw'])
def test_the_fp64_form_is_torch_muon_in_fp64(nesterov, adjust_lr_fn):
    """torch.optim.Muon on fp64 parameters still rounds the iteration's operand to bf16 (``grad.bfloat16()``); with that one cast made
    the identity the whole class runs in fp64, and the restatement differs from it by roundings of 2^-53 only, over 5 updates."""
    idx = [i for i, mu in enumerate(mc.IS_MUON) if mu]
    init = lc.initial_parameters()
    ref = [torch.nn.Parameter(init[i].double()) for i in idx]
    topt = torch.optim.Muon(ref, lr=mc.HYPER['lr'], momentum=mc.HYPER['momentum'], weight_decay=mc.HYPER['weight_decay'], nesterov=nesterov,
                            adjust_lr_fn=adjust_lr_fn, ns_coefficients=mc.NS_COEFFICIENTS, ns_steps=mc.NS_STEPS, eps=mc.EPS)
    runs = mc.run_muon_tensors(torch.float64, nesterov, adjust_lr_fn)
    for step, rec in enumerate(runs):
        grads = lc.gradients(step)
        _, c = lc.clip_coef(grads, lc.MAX_NORM, torch.float64)
        for q, i in zip(ref, idx):
            q.grad = grads[i].double() * c
        with mock.patch.object(torch.Tensor, 'bfloat16', lambda self, *a, **k: self.clone()):
            topt.step()
        for k, q in enumerate(ref):
            torch.testing.assert_close(rec['buf'][k], topt.state[q]['momentum_buffer'], rtol=1e-12, atol=1e-18)
            torch.testing.assert_close(rec['p'][k], q.detach(), rtol=1e-12, atol=1e-15, msg=lambda m: f'update {step} {lc.SHAPES[idx[k]]}: {m}')
    assert [rec['norm'] > lc.MAX_NORM for rec in runs] == [False, True, False, True, False]      # the clip bites in two updates


def test_the_exact_operands_are_exact_and_the_issue_figure_holds():
    for rows, cols in mc.EXACT_SHAPES:
        u = mc.exact_u(rows, cols)
        o = mc.newton_schulz_kernel(u)
        assert o.shape == (rows, cols) and int((o != 0).sum()) == min(rows, cols)
        assert bool(((o != 0) == (u != 0)).all()) and bool((torch.sign(o.float()) == torch.sign(u)).all())
        assert o.float().abs().max() == o.float()[o != 0].abs().min()                       # one magnitude: every line went the same way
    o = mc.newton_schulz_kernel(mc.exact_u(64, 96))
    assert int((o != 0).sum()) == 64 and set(o.float().abs()[o != 0].tolist()) == {0.69140625}


def test_the_kernel_arithmetic_is_as_good_as_torchs_bf16_iteration():
    for rows, cols in mc.GENERAL_SHAPES:
        u = mc.general_u(rows, cols)
        e, e_torch = mc.relative_error(mc.newton_schulz_kernel(u), mc.newton_schulz(u)), mc.torch_bf16_error(u)
        assert 1e-3 < e_torch < 5e-2 and e <= 2 * e_torch, ((rows, cols), e, e_torch)


# ---- the constructor, the group words, state_dict -----------------------------------------------------------------------------------
def _bag():
    return [torch.nn.Parameter(t) for t in lc.initial_parameters()]


def test_flat_muon_constructor_checks(vited):
    FlatMuon = vited.optim.FlatMuon
    w, b = torch.nn.Parameter(torch.zeros(3, 5)), torch.nn.Parameter(torch.zeros(3))
    groups = lambda: [{'params': [w], 'use_muon': True}, {'params': [b]}]
    for kw, match in ((dict(lr=-1.0), 'learning rate'), (dict(momentum=1.0), 'momentum'), (dict(weight_decay=-0.1), 'weight_decay'),
                      (dict(eps=-1e-7), 'epsilon'), (dict(adam_eps=-1e-8), 'epsilon'), (dict(ns_steps=0), 'ns_steps'),
                      (dict(ns_steps=17), 'ns_steps'), (dict(ns_steps=2.5), 'ns_steps'), (dict(ns_coefficients=(1.0, 2.0)), 'ns_coefficients'),
                      (dict(adjust_lr_fn='rms'), 'adjust_lr_fn'), (dict(betas=(1.0, 0.9)), 'beta'), (dict(ema_decay=1.0), 'ema_decay')):
        with pytest.raises(ValueError, match=match):
            FlatMuon(groups(), **kw)
    for bad in (b, torch.nn.Parameter(torch.zeros(2, 3, 4)), torch.nn.Parameter(torch.zeros(8, 3, 2, 2))):
        with pytest.raises(ValueError, match=r'parameter 1 of group 0 has the shape .*2-D tensors only'):
            FlatMuon([{'params': [w, bad], 'use_muon': True}])
    model = torch.nn.Sequential(torch.nn.Linear(4, 4))
    with pytest.raises(ValueError, match=r'0\.bias has the shape \(4,\)'):                   # named where a model names it
        FlatMuon([{'params': list(model.parameters()), 'use_muon': True}], model=model)
    opt = FlatMuon(groups())
    assert opt.defaults == dict(lr=1e-3, momentum=0.95, nesterov=True, weight_decay=0.1, eps=1e-7, adjust_lr_fn=None, betas=(0.9, 0.999),
                                adam_eps=1e-8, use_muon=False)
    assert opt.ns_steps == 5 and opt.ns_coefficients == (3.4445, -4.7750, 2.0315)
    with pytest.raises(AttributeError):
        opt.ns_steps = 3                                                                     # a captured update bakes the launch count in
    assert isinstance(opt, vited.optim._FlatOptimizer) and not isinstance(opt, vited.optim.FlatAdamW)
    assert opt._entry == 'vited_muon_step' and opt.num_updates == 0 and opt.skipped_updates == 0 and opt.state_dict()['state'] == {}
    assert [g['use_muon'] for g in opt.param_groups] == [True, False]
    assert [g['use_muon'] for g in FlatMuon([w, b]).param_groups] == [False]                 # no group asked for Muon: all aux
    with pytest.raises(RuntimeError, match='no CPU path'):
        opt.bind_flat(vited.engine.FlatGradients([w, b]))
    with pytest.raises(RuntimeError, match='bind_flat'):
        opt.orthogonalized(w)


def test_group_words(vited):
    w, b = torch.nn.Parameter(torch.zeros(3, 5)), torch.nn.Parameter(torch.zeros(3))
    opt = vited.optim.FlatMuon([{'params': [w], 'use_muon': True, 'adjust_lr_fn': 'match_rms_adamw'}, {'params': [b], 'weight_decay': 0.0}],
                               lr=3e-3, momentum=0.9, nesterov=False, weight_decay=0.05, eps=1e-6, betas=(0.8, 0.9), adam_eps=1e-5)
    assert opt._group_words(opt.param_groups[0]) == [3e-3, 0.9, 0.0, 1e-6, 0.05, 1.0, 1.0, 0.0]      # kind = 1 in word 6
    assert opt._group_words(opt.param_groups[1]) == [3e-3, 0.8, 0.9, 1e-5, 0.0, 0.0, 0.0, 0.0]      # AdamW's words, kind = 0
    opt.param_groups[0].update(nesterov=True, adjust_lr_fn='original')
    assert opt._group_words(opt.param_groups[0])[2:7] == [1.0, 1e-6, 0.05, 0.0, 1.0]
    assert opt.hyper_lr_words() == (8, 8)                                        # word 0 of every group is its rate
    opt.param_groups[0]['adjust_lr_fn'] = 'rms'
    with pytest.raises(ValueError, match='adjust_lr_fn'):
        opt._group_words(opt.param_groups[0])


def test_state_dict_layout_and_the_three_loading_paths(vited):
    FlatMuon, FlatAdamW = vited.optim.FlatMuon, vited.optim.FlatAdamW
    params = _bag()
    opt = FlatMuon(mc.param_groups(params), **mc.HYPER)
    order = lc.index_in_groups()
    muon_idx = {order[i] for i, mu in enumerate(mc.IS_MUON) if mu}
    # 1. a FlatAdamW checkpoint over the same groups of parameters: exp_avg becomes momentum_buffer on the Muon tensors
    adamw = FlatAdamW(lc.param_groups(_bag()), lr=7e-4, betas=(0.8, 0.9), eps=1e-5, weight_decay=0.02)
    sd = adamw.state_dict()
    for i, shape in enumerate(lc.SHAPES):
        sd['state'][order[i]] = dict(step=torch.tensor(3.0), exp_avg=torch.full(shape, 1.0 + i), exp_avg_sq=torch.full(shape, 0.5 + i))
    opt.load_state_dict(sd)
    assert [g['use_muon'] for g in opt.param_groups] == [True, False, False] and opt.num_updates == 3
    assert opt.param_groups[0]['lr'] == 7e-4 and opt.param_groups[0]['eps'] == 1e-7 and opt.param_groups[0]['momentum'] == 0.95
    assert opt.param_groups[1]['betas'] == (0.8, 0.9) and opt.param_groups[1]['adam_eps'] == 1e-5 and opt.param_groups[1]['weight_decay'] == 0.0
    out = opt.state_dict()
    for i in range(len(lc.SHAPES)):
        st = out['state'][order[i]]
        if order[i] in muon_idx:
            assert set(st) == {'momentum_buffer'} and float(st['momentum_buffer'].flatten()[0]) == 1.0 + i
        else:
            assert set(st) == {'step', 'exp_avg', 'exp_avg_sq'} and float(st['step']) == 3.0 and float(st['exp_avg_sq'].flatten()[0]) == 0.5 + i
    # 2. its own state_dict goes back in
    again = FlatMuon(mc.param_groups(_bag()), **mc.HYPER)
    again.load_state_dict(out)
    back = again.state_dict()
    assert back['param_groups'] == out['param_groups'] and again.num_updates == 3
    for k, st in out['state'].items():
        assert set(back['state'][k]) == set(st) and all(torch.equal(back['state'][k][n], st[n]) for n in st)
    # a Lion checkpoint (exp_avg alone): the second moment of an aux tensor starts from zero
    lion = vited.optim.FlatLion(lc.param_groups(_bag()))
    sd = lion.state_dict()
    for i, shape in enumerate(lc.SHAPES):
        sd['state'][order[i]] = dict(exp_avg=torch.full(shape, 2.0))
    third = FlatMuon(mc.param_groups(_bag()), **mc.HYPER)
    third.load_state_dict(sd)
    assert all(set(st) == ({'momentum_buffer'} if k in muon_idx else {'step', 'exp_avg'}) for k, st in third.state_dict()['state'].items())
    # 3. a torch.optim.Muon state loads into the Muon tensors
    ws = [torch.nn.Parameter(torch.randn(6, 4)), torch.nn.Parameter(torch.randn(3, 5))]
    tmu = torch.optim.Muon(ws, lr=5e-3, momentum=0.9, nesterov=False, adjust_lr_fn='match_rms_adamw')
    for q in ws:
        q.grad = torch.ones_like(q)
    tmu.step()
    mine = FlatMuon([{'params': [torch.nn.Parameter(q.detach().clone()) for q in ws], 'use_muon': True}])
    mine.load_state_dict(tmu.state_dict())
    g = mine.param_groups[0]
    assert (g['lr'], g['momentum'], g['nesterov'], g['adjust_lr_fn'], g['use_muon']) == (5e-3, 0.9, False, 'match_rms_adamw', True)
    for k, q in enumerate(ws):
        assert torch.equal(mine.state_dict()['state'][k]['momentum_buffer'], tmu.state[q]['momentum_buffer'])


def _config(name):
    opt = types.SimpleNamespace(NAME=name, EPS=1e-6, BETAS=(0.9, 0.999), MOMENTUM=0.9)
    return types.SimpleNamespace(TRAIN=types.SimpleNamespace(OPTIMIZER=opt, BASE_LR=1e-3, WEIGHT_DECAY=0.05))


@pytest.mark.parametrize('name', ['muon', 'Muon', 'MUON'])
def test_build_optimizer_has_no_muon_for_a_cpu_model(vited, name):
    model = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.LayerNorm(4))
    for kw in (dict(), dict(fused_hip=False), dict(fused_hip=True)):
        with pytest.raises(ValueError, match='unknown optimizer muon .*HIP optimizer only'):
            vited.engine.build_optimizer(_config(name), model, **kw)


def test_range_test_names_the_fused_optimizers(vited):
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(NotImplementedError, match='optim.FlatMuon / optim.FlatLion / optim.FlatLAMB / optim.FlatAdamW / optim.FlatSGD; Adam has none'):
        vited.engine.LRRangeTest(torch.optim.Adam(p, lr=1e-3), 10)
    with pytest.raises(RuntimeError, match='bind_flat'):                         # accepted as a fused optimizer: only the binding is missing
        vited.engine.LRRangeTest(vited.optim.FlatMuon(p), 10)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_muon_entry_points_are_declared_bound_and_exported(vited):
    _ensure_built(vited)
    import ctypes as C
    sig = vited._lib.SIGNATURES
    extras = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float]
    # the argument list of vited_lamb_step / _ema in front, then the tile tables, the steps and the coefficients by value
    assert sig['vited_muon_step'] == (sig['vited_lamb_step'][0], sig['vited_lamb_step'][1] + extras)
    assert sig['vited_muon_step_ema'] == (sig['vited_lamb_step_ema'][0], sig['vited_lamb_step_ema'][1] + extras)
    assert sig['vited_muon_workspace_bytes'] == (C.c_int64, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
    out = subprocess.run(['nm', '-D', '--defined-only', vited._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if ' T ' in l}
    assert {'vited_muon_step', 'vited_muon_step_ema', 'vited_muon_workspace_bytes'} <= exported
    lib = vited._lib.load()
    assert lib.vited_abi_version() == 1
    nothing = (None, 0, 0, None, 0, None, 0.0, 0, None, None, 0)
    tail = (None, None, 0, None, 0, None, None, None, 0, 5, 3.4445, -4.775, 2.0315)
    assert lib.vited_muon_step(*nothing, *tail) == 1                             # validated before any launch
    assert lib.vited_muon_step_ema(*nothing, None, 0, *tail) == 1
    text = open(os.path.join(ROOT, 'vit-ed_amd', 'csrc', 'muon_update.h')).read()
    for name in ('muon_coef', 'muon_buf', 'muon_u', 'muon_denom', 'muon_moments_piece', 'muon_pack_piece', 'muon_apply_piece', 'muon_ns_poly',
                 'muon_ns_next'):
        assert re.search(r'\b%s\s*\(' % name, text), name


def _host_arrays(shapes, is_muon):
    rows = [s[0] if len(s) >= 2 else 1 for s in shapes]
    cols = [math.prod(s) // r for s, r in zip(shapes, rows)]
    return [torch.tensor(v, dtype=torch.int64) for v in (rows, cols, [int(m) for m in is_muon])]


def test_workspace_bytes_from_the_shapes(vited):
    _ensure_built(vited)
    lib = vited._lib.load()
    pad = lambda v: (v + 63) // 64 * 64
    for shapes, is_muon in ((lc.SHAPES, mc.IS_MUON), ([(384, 384), (1152, 384), (384, 1536), (1000, 384), (384,)], [True, True, True, False, False]),
                            ([(16, 40), (72, 16)], [True, True]), ([(5,), (2, 3)], [False, False])):
        rows, cols, mu = _host_arrays(shapes, is_muon)
        tiles = sum(((r + 63) // 64) * ((c + 63) // 64) for r, c in zip(rows.tolist(), cols.tolist()))
        elems = 0
        for r, c, m in zip(rows.tolist(), cols.tolist(), is_muon):
            if m:
                mp, np_ = pad(min(r, c)), pad(max(r, c))
                elems += 4 * mp * np_ + 2 * mp * mp                              # X0, X1, XT0, XT1, A, B
        want = pad(1028 + len(shapes) + tiles) * 4 + elems * 2
        assert lib.vited_muon_workspace_bytes(len(shapes), rows.data_ptr(), cols.data_ptr(), mu.data_ptr()) == want
        assert vited.optim.muon_layout(shapes, is_muon)['nbytes'] == want
    rows, cols, mu = _host_arrays([(16, 40)], [True])
    assert lib.vited_muon_workspace_bytes(0, rows.data_ptr(), cols.data_ptr(), mu.data_ptr()) == 0
    assert lib.vited_muon_workspace_bytes(1, None, cols.data_ptr(), mu.data_ptr()) == 0
    rows, cols, mu = _host_arrays([(1088, 2048)], [True])                        # a short side above 1024
    assert lib.vited_muon_workspace_bytes(1, rows.data_ptr(), cols.data_ptr(), mu.data_ptr()) == 0
    with pytest.raises(ValueError, match='short side above 1024'):
        vited.optim.muon_layout([(1088, 2048)], [True])
    rows, cols, mu = (torch.tensor([v], dtype=torch.int64) for v in (0, 4, 1))                # an empty tensor
    assert lib.vited_muon_workspace_bytes(1, rows.data_ptr(), cols.data_ptr(), mu.data_ptr()) == 0


def test_tile_tables_cover_every_tile_of_every_muon_tensor_once(vited):
    lay = vited.optim.muon_layout(lc.SHAPES, mc.IS_MUON)
    muon = {i for i, m in enumerate(mc.IS_MUON) if m}
    end = 0
    for i, (shape, (base, mp, np_, tall)) in enumerate(zip(lc.SHAPES, lay['tensor_tab'])):
        if i not in muon:
            assert base == -1
            continue
        rows, cols = shape
        assert (mp, np_, tall) == ((min(shape) + 63) // 64 * 64, (max(shape) + 63) // 64 * 64, int(rows > cols))
        assert base == end                                                       # regions in table order, without gaps or overlap
        end = base + 4 * mp * np_ + 2 * mp * mp
        for table, width in ((lay['tiles_sq'], mp // 64), (lay['tiles_x'], np_ // 64)):
            mine = [row for row in table if row[0] == i]
            assert sorted((row[1], row[2]) for row in mine) == [(a, b) for a in range(mp // 64) for b in range(width)]
            assert all(row[3:] == [base, mp, np_, tall, 0] for row in mine)
    assert end == lay['scratch_elems'] and lay['nbytes'] == 4 * lay['float_words'] + 2 * end
    assert {row[0] for row in lay['tiles_sq']} == muon == {row[0] for row in lay['tiles_x']}          # no aux tensor is named
    assert [m[3] for m in lay['meta']] == [int(m) for m in mc.IS_MUON] and [m[2] for m in lay['meta']] == [len(s) for s in lc.SHAPES]
    assert [m[4] for m in lay['meta']] == [0] * len(lc.SHAPES)
    assert [m[4] for m in vited.optim.muon_layout(lc.SHAPES, mc.IS_MUON, lc.GROUP_OF)['meta']] == lc.GROUP_OF
    assert lay['total_tiles'] == sum(((m[0] + 63) // 64) * ((m[1] + 63) // 64) for m in lay['meta'])
    # several tiles per tensor
    big = vited.optim.muon_layout([(256, 320), (7,), (72, 16)], [True, False, True])
    assert len(big['tiles_sq']) == 16 + 1 and len(big['tiles_x']) == 4 * 5 + 2 and big['tensor_tab'][2][3] == 1
    with pytest.raises(ValueError, match='2-D tensors only'):
        vited.optim.muon_layout([(2, 3, 4)], [True])


# ---- the elementwise bodies on the host, under the sanitizers -----------------------------------------------------------------------
def test_elementwise_bodies_under_the_sanitizers(tmp_path):
    """tools/muon_host_check.cpp compiles csrc/muon_update.h for the host - the text the kernels run - and drives the momentum, pack
    (padding included; the transposed image is the GPU tests') and apply passes over exactly-sized buffers against a double-precision loop: a stand-alone
    program with its own main."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    cxx = next((c for c in (shutil.which('clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'))
                if c and os.path.exists(c)), None)
    assert cxx is not None, 'no clang++ beside hipcc: the HIP toolchain that builds the library ships one'
    exe = str(tmp_path / 'muon_host_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I',
                    os.path.join(ROOT, 'vit-ed_amd', 'csrc'), os.path.join(ROOT, 'tools', 'muon_host_check.cpp'), '-o', exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and 'muon_host_check ok' in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_a_two_group_checkpoint_is_regrouped_by_the_models_parameter_order(vited):
    """build_optimizer('adamw' | 'lamb' | 'lion') writes two groups, decayed and not; build_optimizer('muon') has three.  The decayed
    group is the Muon group and the decayed aux group together, in the model's order, and load_state_dict finds that from the group
    sizes and the state tensors' shapes."""
    from oracle import vited_oracle as vo
    s = vo.SHAPE_T
    model = vited.VisionTransformerCustom(img_size=s.img_size, patch_size=s.patch_size, in_chans=s.in_chans, num_classes=s.num_classes,
                                          embed_dim=s.embed_dim, depth=s.depth, c_depth=s.c_depth, num_heads=s.num_heads)
    named = list(model.named_parameters())
    two = vited.engine.param_groups_no_decay_1d(model)
    adamw = vited.optim.FlatAdamW(two, lr=7e-4, betas=(0.8, 0.9), eps=1e-5, weight_decay=0.02)
    sd = adamw.state_dict()
    mark = {id(p): float(k + 1) for k, (_, p) in enumerate(named)}                 # every parameter's state carries its own number
    at = 0
    for g in two:
        for p in g['params']:
            sd['state'][at] = dict(step=torch.tensor(6.0), exp_avg=torch.full(p.shape, mark[id(p)]), exp_avg_sq=torch.full(p.shape, -mark[id(p)]))
            at += 1
    decay, no_decay = ({id(p) for p in g['params']} for g in two)
    is_mu = {id(p) for n, p in named if p.ndim == 2 and n.startswith(('blocks.', 'cross_blocks.'))}
    groups = [{'params': [p for _, p in named if id(p) in is_mu], 'use_muon': True},
              {'params': [p for _, p in named if id(p) in decay and id(p) not in is_mu]},
              {'params': [p for _, p in named if id(p) in no_decay], 'weight_decay': 0.0}]
    opt = vited.optim.FlatMuon(groups, model=model)
    opt.load_state_dict(sd)
    assert opt.num_updates == 6 and [g['use_muon'] for g in opt.param_groups] == [True, False, False]
    assert [g['lr'] for g in opt.param_groups] == [7e-4] * 3 and [g['weight_decay'] for g in opt.param_groups] == [0.02, 0.02, 0.0]
    assert opt.param_groups[1]['betas'] == (0.8, 0.9) and opt.param_groups[1]['adam_eps'] == 1e-5 and opt.param_groups[0]['eps'] == 1e-7
    for _, p in named:
        st = opt.state[p]
        if id(p) in is_mu:
            assert set(st) == {'momentum_buffer'} and bool((st['momentum_buffer'] == mark[id(p)]).all())
        else:
            assert set(st) == {'exp_avg', 'exp_avg_sq'} and bool((st['exp_avg'] == mark[id(p)]).all()) and bool((st['exp_avg_sq'] == -mark[id(p)]).all())
    with pytest.raises(ValueError, match='build the optimizer with model='):       # without the model there is no order to go by
        vited.optim.FlatMuon(groups).load_state_dict(sd)
    wrong = {'state': {}, 'param_groups': [dict(sd['param_groups'][0], params=list(range(5))), dict(sd['param_groups'][1], params=list(range(5, 12)))]}
    with pytest.raises(ValueError, match='in 0 ways'):
        opt.load_state_dict(wrong)
