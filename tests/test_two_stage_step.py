"""The two-stage training step and its fused loss, as far as they go without a GPU: the public names, every refusal of ``ops.mined_bce``
(before the launch, in the op's name) and of ``engine.TwoStageTrainStep``'s constructor, and the header's statement of the entry."""
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(rows=8, classes=1):
    return dict(logits=torch.zeros(rows, classes), labels=torch.zeros(rows, 1), weights=torch.ones(rows, 1),
                counts=torch.tensor([2, 4, 4, 6, 0], dtype=torch.int32))


@pytest.fixture
def stubbed(vited, monkeypatch):
    """``ops`` with the device gate open and the library replaced by a recorder, as tests/test_ops_args.py does."""
    calls = []
    monkeypatch.setattr(vited.ops, '_need_gpu', lambda *tensors, **kw: None)
    monkeypatch.setattr(vited.ops, '_stream', lambda: 0)
    monkeypatch.setattr(vited.ops, '_lib', SimpleNamespace(call=lambda name, *args: calls.append((name, args))))
    return calls


def test_the_names_and_their_homes(vited):
    E, ops = vited.engine, vited.ops
    assert E.TwoStageTrainStep is E.train.TwoStageTrainStep and issubclass(E.TwoStageTrainStep, E.TrainStep)
    assert E.mined_bce_fused is E.mining.mined_bce_fused and callable(E.mined_bce_with_logits)
    assert ops.mined_bce.__module__.endswith('ops_minedloss') and ops.MINED_BCE_MAX_CLASSES == 64
    # the inherited pieces are TrainStep's own functions, not copies
    for name in ('_eager', '_capture', '_capture_update', '_update', '_after_update', '_sync_lr', 'set_lr', '_enc_bwd'):
        assert getattr(E.TwoStageTrainStep, name) is getattr(E.TrainStep, name), name


def test_the_header_declares_the_entry_with_these_types(vited):
    p, i, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    assert vited._lib.SIGNATURES['vited_mined_bce'] == (i, [p, p, p, p, i64, i64, i, f, p, p, p])


def test_the_library_refuses_bad_arguments_before_a_launch(vited):
    lib = vited._lib.load()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    assert lib.vited_mined_bce(None, a, a, a, 4, 1, 1, 1.0, a, a, None) == 1            # VITED_ERR_BAD_ARG
    assert lib.vited_mined_bce(a, a, a, a, 0, 1, 1, 1.0, a, a, None) == 1
    assert lib.vited_mined_bce(a, a, a, a, 4, 1, 1, float('nan'), a, a, None) == 1
    assert lib.vited_mined_bce(a, a, a, a, 4, 1, 1, float('inf'), a, a, None) == 1
    assert lib.vited_mined_bce(a, a, a, a + 2, 4, 1, 1, 1.0, a, a, None) == 1
    assert lib.vited_mined_bce(a, a, a, a, 4, 65, 1, 1.0, a, a, None) == 2              # VITED_ERR_UNSUPPORTED
    assert lib.vited_mined_bce(a, a, a, a, vited.ops.MINE_MAX_CAPACITY + 1, 1, 1, 1.0, a, a, None) == 2


def test_cpu_tensors_are_refused_in_the_ops_name(vited):
    with pytest.raises(RuntimeError, match=r'^mined_bce: .*CPU tensor'):
        vited.ops.mined_bce(**_args())


@pytest.mark.parametrize('fault,change', [
    ('logits dtype', dict(logits=torch.zeros(8, 1, dtype=torch.bfloat16))),
    ('labels dtype', dict(labels=torch.zeros(8, 1, dtype=torch.float64))),
    ('counts dtype', dict(counts=torch.zeros(5, dtype=torch.int64))),
    ('labels rows', dict(labels=torch.zeros(7, 1))),
    ('weights rows', dict(weights=torch.zeros(9, 1))),
    ('labels rank', dict(labels=torch.zeros(8))),
    ('counts extent', dict(counts=torch.zeros(4, dtype=torch.int32))),
    ('65 outputs', dict(logits=torch.zeros(8, 65))),
    ('no rows', dict(logits=torch.zeros(0, 1), labels=torch.zeros(0, 1), weights=torch.zeros(0, 1))),
    ('strided logits', dict(logits=torch.zeros(8, 4)[:, :2])),
    ('1-D logits', dict(logits=torch.zeros(8))),
    ('reduction', dict(reduction='none')),
    ('scale', dict(scale=float('nan'))),
    ('not a tensor', dict(weights=None)),
], ids=lambda v: v if isinstance(v, str) else '')
def test_one_fault_is_refused_before_the_launch(vited, stubbed, fault, change):
    with pytest.raises(ValueError, match=r'^mined_bce: '):
        vited.ops.mined_bce(**dict(_args(), **change))
    assert not stubbed


def test_too_many_rows_are_refused(vited, stubbed):
    rows = vited.ops.MINE_MAX_CAPACITY + 1
    with pytest.raises(ValueError, match=r'^mined_bce: logits \[24577, 1\]'):
        vited.ops.mined_bce(**_args(rows))
    assert not stubbed


def test_a_valid_call_reaches_the_entry_once(vited, stubbed):
    a = _args(8, 4)
    loss, dlogits = vited.ops.mined_bce(**a, reduction='sum', scale=0.5)
    assert [name for name, _ in stubbed] == ['vited_mined_bce']
    args = stubbed[0][1]
    assert args[:4] == (a['logits'].data_ptr(), a['labels'].data_ptr(), a['weights'].data_ptr(), a['counts'].data_ptr())
    assert args[4:8] == (8, 4, 0, 0.5) and args[8:10] == (loss.data_ptr(), dlogits.data_ptr())
    assert loss.shape == (1,) and dlogits.shape == (8, 4) and loss.dtype == dlogits.dtype == torch.float32
    del stubbed[:]
    vited.ops.mined_bce(**_args(1, 64))                                 # the largest width, the smallest height, the mean
    assert stubbed[0][1][4:8] == (1, 64, 1, 1.0)


def test_the_fused_loss_refuses_a_cpu_call_too(vited):
    E = vited.engine
    mined = E.mine_pairs_device(torch.tensor([0, 0, 1, 1]), 8, keys=torch.linspace(0, 0.9, 16))
    with pytest.raises(RuntimeError, match=r'^mined_bce: '):
        E.mined_bce_fused(torch.zeros(8, 1), mined)
    with pytest.raises(ValueError, match=r'^mined_bce: reduction'):
        E.mined_bce_fused(torch.zeros(8, 1), mined, reduction='none')


def _model(vited):
    return vited.VisionTransformerCustom(img_size=64, patch_size=8, num_classes=1, embed_dim=384, depth=1, c_depth=1, num_heads=12)


def test_constructor_refusals_name_the_argument(vited):
    E, model = vited.engine, _model(vited)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    limit = vited.ops.MINE_MAX_CAPACITY
    for capacity in (0, -3, limit + 1):
        with pytest.raises(ValueError, match=r'^TwoStageTrainStep: capacity'):
            E.TwoStageTrainStep(model, opt, capacity=capacity)
    with pytest.raises(TypeError):
        E.TwoStageTrainStep(model, opt)                                # capacity has no default
    with pytest.raises(ValueError, match=r'^TwoStageTrainStep: reduction'):
        E.TwoStageTrainStep(model, opt, capacity=8, reduction='none')
    with pytest.raises(ValueError, match=r'^TwoStageTrainStep: neg_per_pos'):
        E.TwoStageTrainStep(model, opt, capacity=8, neg_per_pos=-1.0)
    with pytest.raises(ValueError, match=r'^TwoStageTrainStep: forward_fn and criterion'):
        E.TwoStageTrainStep(model, opt, capacity=8, forward_fn=lambda m, x: m(x))
    with pytest.raises(ValueError, match=r'^TwoStageTrainStep: forward_fn and criterion'):
        E.TwoStageTrainStep(model, opt, capacity=8, criterion=E.mined_bce_with_logits)
    plain = torch.nn.Linear(4, 1)
    with pytest.raises(ValueError, match=r'^TwoStageTrainStep: model .*supports_x1_index'):
        E.TwoStageTrainStep(plain, torch.optim.SGD(plain.parameters(), lr=0.1), capacity=8)


def test_step_refusals_come_before_any_work(vited, monkeypatch):
    E, model = vited.engine, _model(vited)
    step = E.TwoStageTrainStep(model, torch.optim.SGD(model.parameters(), lr=0.1), capacity=8, amp=False)
    assert step.mine_keys is None and step.last_mined is None and step.capacity == 8 and step.reduction == 'mean'

    def no_work(*a, **k):
        raise AssertionError('a refused batch reached the step')

    monkeypatch.setattr(E.TrainStep, 'step', no_work)
    x, t = torch.zeros(4, 3, 64, 64), torch.tensor([0, 0, 1, 1])
    for name in ('drop_path', 'patch_keep', 'pos_drop'):
        setattr(step, name, object())
        with pytest.raises(ValueError, match=rf'^TwoStageTrainStep: step\.{name}'):
            step.step(x, t)
        setattr(step, name, None)
    with pytest.raises(ValueError, match=r'^TwoStageTrainStep: samples'):
        step.step(torch.zeros(4, 2, 3, 64, 64), t)
    with pytest.raises(ValueError, match=r'^TwoStageTrainStep: targets'):
        step.step(x, t[:3])
    with pytest.raises(ValueError, match=r'^TwoStageTrainStep: targets'):
        step.step(x, t.float())
    step.mine_keys = torch.zeros(15)
    with pytest.raises(ValueError, match=r'^TwoStageTrainStep: mine_keys'):
        step.step(x, t)
