"""vited_mined_bce on the MI355X: loss and gradient against torch's binary_cross_entropy_with_logits in fp64 on
the CPU, the exact properties the rule promises (padding rows are selected away, the bits do not depend on the capacity, two runs
agree bit for bit), capture into a hipGraph and the autograd Function over it.

Bounds (from the number formats, not from what the kernel gives):
  loss      |got - want| <= (16 + ceil(log2(R C))) 2^-24 * want,  want = scale * sum(w term_64) / denom: 16 units of 2^-24 for the
            device library's <= 2-ulp exp and log and the handful of roundings of one term, ceil(log2(R C)) for the summation tree;
  gradient  |got - want| <= 8 * 2^-24 * max(|want|, 2^-24 scale / denom) per element.
Shapes: one element; 8 rows of which 6 are pairs; 72 rows (config H's capacity); 80 x 4 = 320 elements, more than one per thread;
300 rows, more than one per thread and a ragged last round.  Where there are at least 8 rows the first four pairs hold the logits
+80, -80, +1e4, -1e4 (each case runs with and without them: 1e4 would otherwise hide every other term of the sum).  The form of the
term drops what lies under fp32's 1 + e (at most 2^-24 per element), so the one-element case holds an ordinary logit.
Worst error / bound observed on an MI355X: loss 0.34 ([1, 1]; 0.05 - 0.12 elsewhere), gradient 0.50 ([300, 1])."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
CASES = [(1, 1, 1), (8, 1, 6), (72, 1, 72), (80, 4, 67), (300, 1, 291)]          # rows, outputs, rows that are pairs
EXTREMES = (80.0, -80.0, 1e4, -1e4)
EXTREME_LABELS = (1.0, 1.0, 0.0, 0.0)          # terms ~ 2e-35 (below fp32's 1 + e), 80, 1e4, 0
BCE = torch.nn.functional.binary_cross_entropy_with_logits


def _case(rows, classes, pairs, extremes, seed=0):
    g = torch.Generator().manual_seed(1000 * rows + classes + seed)
    logits = torch.randn(rows, classes, generator=g) * 2
    labels = (torch.rand(rows, 1, generator=g) < 0.4).float()
    if extremes and rows >= 8:
        logits[:4, 0] = torch.tensor(EXTREMES)
        labels[:4, 0] = torch.tensor(EXTREME_LABELS)
    weights = torch.zeros(rows, 1)
    weights[:pairs] = 1.0
    counts = torch.tensor([int(labels[:pairs].sum()), 0, pairs - int(labels[:pairs].sum()), pairs, 0], dtype=torch.int32)
    return logits, labels, weights, counts


def _reference(logits, labels, weights, counts, reduction, scale):
    """(loss, gradient, scale / denom) in fp64 on the CPU: torch's own loss and its autograd gradient."""
    x = logits.double().requires_grad_(True)
    total = BCE(x, labels.double().expand_as(x), weight=weights.double().expand_as(x), reduction='sum')
    factor = scale / (max(int(counts[3]), 1) * logits.shape[1]) if reduction == 'mean' else scale
    (total * factor).backward()
    return float(total.detach()) * factor, x.grad, factor


def _run(ops, gpu, logits, labels, weights, counts, reduction, scale):
    loss, dlogits = ops.mined_bce(logits.to(gpu), labels.to(gpu), weights.to(gpu), counts.to(gpu), reduction, scale)
    return loss.cpu(), dlogits.cpu()


@pytest.mark.parametrize('rows,classes,pairs', CASES)
def test_against_the_fp64_restatement(vited, gpu, rows, classes, pairs):
    worst = [0.0, 0.0]
    for extremes in (False, True):
        for reduction in ('mean', 'sum'):
            for scale in (1.0, 0.5):
                case = _case(rows, classes, pairs, extremes)
                loss, dlogits = _run(vited.ops, gpu, *case, reduction, scale)
                want, grad, factor = _reference(*case, reduction, scale)
                assert loss.shape == (1,) and dlogits.shape == (rows, classes)
                bound = (16 + math.ceil(math.log2(rows * classes))) * 2.0 ** -24 * want
                err = abs(float(loss.double()) - want)
                gbound = 8 * 2.0 ** -24 * torch.maximum(grad.abs(), torch.tensor(2.0 ** -24 * factor, dtype=torch.float64))
                gerr = (dlogits.double() - grad).abs()
                ratios = err / bound, float((gerr / gbound).max())
                print(f'[{rows}, {classes}] extremes {extremes} {reduction} scale {scale}: loss {float(loss):.9g} want {want:.17g} '
                      f'err / bound {ratios[0]:.3f}; gradient worst err / bound {ratios[1]:.3f}')
                worst = [max(a, b) for a, b in zip(worst, ratios)]
                assert err <= bound, (extremes, reduction, scale, float(loss), want, err, bound)
                assert bool((gerr <= gbound).all()), (extremes, reduction, scale, float((gerr / gbound).max()))
                pad = dlogits[pairs:]
                assert not bool(pad.any()) and not bool(torch.signbit(pad).any()), 'a padding row has an exact +0 gradient'
    print(f'[{rows}, {classes}] worst err / bound: loss {worst[0]:.3f} gradient {worst[1]:.3f}')


def test_capacity_invariance_and_the_weight_select(vited, gpu):
    ops = vited.ops
    for extremes in (False, True):
        for reduction in ('mean', 'sum'):
            logits, labels, weights, counts = _case(8, 1, 6, extremes)
            loss8, d8 = _run(ops, gpu, logits, labels, weights, counts, reduction, 0.5)
            loss6, d6 = _run(ops, gpu, logits[:6].contiguous(), labels[:6].contiguous(), weights[:6].contiguous(), counts, reduction, 0.5)
            assert torch.equal(loss8.view(torch.int32), loss6.view(torch.int32)), 'the loss bits depend on the capacity'
            assert torch.equal(d8[:6].view(torch.int32), d6.view(torch.int32))
            for poison in (float('nan'), float('inf'), -float('inf')):
                bad = logits.clone()
                bad[6:] = poison                                           # padding rows: selected away, not multiplied by 0
                loss_p, d_p = _run(ops, gpu, bad, labels, weights, counts, reduction, 0.5)
                assert torch.equal(loss_p.view(torch.int32), loss8.view(torch.int32)), poison
                assert torch.equal(d_p.view(torch.int32), d8.view(torch.int32)), poison
            for poison in (float('nan'), float('inf')):
                bad = logits.clone()
                bad[5] = poison                                            # a weighted row: the loss says so, as torch's does
                loss_p, d_p = _run(ops, gpu, bad, labels, weights, counts, reduction, 0.5)
                assert not bool(torch.isfinite(loss_p).any()), poison
                assert not bool(d_p[6:].any())
    # no pair at all: the mean divides by max(0, 1) outputs and the loss is an exact +0
    logits, labels, weights, counts = _case(8, 1, 0, False)
    loss0, d0 = _run(ops, gpu, logits, labels, weights, counts, 'mean', 1.0)
    assert loss0.view(torch.int32).item() == 0 and not bool(d0.any())


@pytest.mark.parametrize('rows,classes,pairs', CASES)
def test_two_runs_agree_bit_for_bit(vited, gpu, rows, classes, pairs):
    case = [t.to(gpu) for t in _case(rows, classes, pairs, True)]
    a = vited.ops.mined_bce(*case, 'mean', 1.0)
    b = vited.ops.mined_bce(*case, 'mean', 1.0)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_replays_of_a_captured_launch_equal_the_eager_call(vited, gpu):
    ops, (rows, classes, pairs) = vited.ops, CASES[3]
    static = [t.to(gpu) for t in _case(rows, classes, pairs, False)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.mined_bce(*static, 'mean', 0.5)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, dlogits = ops.mined_bce(*static, 'mean', 0.5)
    seen = []
    for seed, live in ((1, 67), (2, 31)):                                  # the pair count changes too: it is read on the device
        fresh = [t.to(gpu) for t in _case(rows, classes, live, True, seed=seed)]
        for dst, src in zip(static, fresh):
            dst.copy_(src)
        graph.replay()
        want_loss, want_d = ops.mined_bce(*fresh, 'mean', 0.5)
        assert torch.equal(loss.view(torch.int32), want_loss.view(torch.int32)) and torch.equal(dlogits.view(torch.int32), want_d.view(torch.int32))
        seen.append(float(loss))
    assert seen[0] != seen[1]


def test_the_autograd_function_hands_out_the_kernels_gradient(vited, gpu):
    E, ops = vited.engine, vited.ops
    logits, labels, weights, counts = (t.to(gpu) for t in _case(80, 4, 67, True))
    mined = E.MinedPairs(torch.zeros(80, 2, dtype=torch.int64, device=gpu), labels, weights, None, counts)
    for reduction, scale in (('mean', 1.0), ('sum', 0.5)):
        want_loss, want_d = ops.mined_bce(logits, labels, weights, counts, reduction, scale)
        leaf = logits.clone().requires_grad_(True)
        loss = E.mined_bce_fused(leaf, mined, reduction, scale)
        assert loss.shape == () and torch.equal(loss.detach().view(torch.int32), want_loss[0].view(torch.int32))
        loss.backward()
        assert torch.equal(leaf.grad.view(torch.int32), want_d.view(torch.int32))
        leaf.grad = None
        (E.mined_bce_fused(leaf, mined, reduction, scale) * 3.0).backward()
        assert torch.equal(leaf.grad, want_d * 3.0)
    # a [capacity] logit vector and bf16 logits (what autocast may hand over) go through the same launch
    flat = logits[:, 0].clone().requires_grad_(True)
    E.mined_bce_fused(flat, mined).backward()
    assert flat.grad.shape == (80,) and torch.equal(flat.grad, ops.mined_bce(logits[:, :1].contiguous(), labels, weights, counts)[1][:, 0])
    low = logits.clamp(-50, 50).to(torch.bfloat16).requires_grad_(True)
    E.mined_bce_fused(low, mined).backward()
    assert low.grad.dtype == torch.bfloat16
    assert torch.equal(low.grad, ops.mined_bce(low.detach().float(), labels, weights, counts)[1].to(torch.bfloat16))
    # against the plain-torch loss the drivers used so far (fp32 both): same number up to fp32 summation
    torch.testing.assert_close(E.mined_bce_fused(logits, mined), E.mined_bce_with_logits(logits, mined), rtol=1e-5, atol=0)
