"""The per-iteration learning-rate rules (misc/lr_scheduler.py over timm.scheduler) written out in plain Python,
independently of the package, and the case table the CPU and GPU tests share.

Two parameter groups, the second with ``lr_scale`` 0.1; base rate 1e-4, WARMUP_LR 5e-7, MIN_LR 5e-6; 5 iterations per epoch, 6 epochs,
2 or 0 warm-up epochs; t = 0 ... 39 and, for the width of the index, 10^6 and 2^33."""
import bisect
import math
import types

import numpy as np

BASE_LR, WARMUP_LR, MIN_LR = 1e-4, 5e-7, 5e-6
N_ITER, EPOCHS = 5, 6
LR_SCALES = (None, 0.1)                      # group 0 has no 'lr_scale' key
T_VALUES = list(range(40)) + [10 ** 6, 2 ** 33]
DECAY_EPOCHS, DECAY_RATE, MULTISTEPS, GAMMA = 1, 0.5, [3, 5], 0.1


def _case(name, warmup_epochs, warmup_prefix=True, step_warmup_prefix=False):
    flag = {'cosine': warmup_prefix, 'step': step_warmup_prefix}.get(name)
    tag = name if flag is None else name + ('_prefix' if flag else '_noprefix')
    return dict(id=f'{tag}_warm{warmup_epochs}', name=name, warmup_epochs=warmup_epochs, warmup_prefix=warmup_prefix,
                step_warmup_prefix=step_warmup_prefix)


CASES = [_case('cosine', w, warmup_prefix=p) for w in (2, 0) for p in (True, False)]
CASES += [_case('linear', w) for w in (2, 0)]
CASES += [_case('step', w, step_warmup_prefix=p) for w in (2, 0) for p in (False, True)]
CASES += [_case('multistep', w) for w in (2, 0)]
BY_ID = {c['id']: c for c in CASES}


def config(case):
    """The config keys build_scheduler reads."""
    ns = types.SimpleNamespace
    sched = ns(NAME=case['name'], DECAY_EPOCHS=DECAY_EPOCHS, DECAY_RATE=DECAY_RATE, WARMUP_PREFIX=case['warmup_prefix'], GAMMA=GAMMA,
               MULTISTEPS=list(MULTISTEPS))
    return ns(TRAIN=ns(EPOCHS=EPOCHS, WARMUP_EPOCHS=case['warmup_epochs'], BASE_LR=BASE_LR, WARMUP_LR=WARMUP_LR, MIN_LR=MIN_LR,
                       LR_SCHEDULER=sched))


def group_specs(params):
    """param_groups over two lists of parameters: the second group carries lr_scale."""
    return [{'params': params[0]}, {'params': params[1], 'lr_scale': LR_SCALES[1]}]


def warmup_t(case):
    return int(case['warmup_epochs'] * N_ITER)


def value(case, t, base=BASE_LR):
    """_get_lr(t) of one group with the base rate ``base``, before lr_scale: the issue's rule, term for term."""
    name, wt = case['name'], warmup_t(case)
    num_steps = int(EPOCHS * N_ITER)
    if t < wt:
        return WARMUP_LR + t * ((base - WARMUP_LR) / wt)
    if name == 'cosine':
        t_initial = num_steps - wt if case['warmup_prefix'] else num_steps
        if case['warmup_prefix']:
            t = t - wt
        i = t // t_initial
        t_curr = t - t_initial * i
        if i < 1:
            return MIN_LR + 0.5 * (base * 1.0 ** i - MIN_LR) * (1 + math.cos(math.pi * t_curr / t_initial))
        return MIN_LR
    if name == 'linear':
        t = t - wt
        total = num_steps - wt
        return base - (base - base * 0.01) * (t / total)
    if name == 'step':
        if case['step_warmup_prefix']:
            t = t - wt
        return base * DECAY_RATE ** (t // int(DECAY_EPOCHS * N_ITER))
    return base * GAMMA ** bisect.bisect_right([i * N_ITER for i in MULTISTEPS], t)


def group_rates(case, t):
    """What update_groups writes for _get_lr(t): [value, value * 0.1] as Python floats."""
    v = value(case, t)
    return [v if s is None else v * s for s in LR_SCALES]


def initial_rates(case):
    """The groups' rates after the constructor: the warm-up start, or the base rates without warm-up."""
    v = WARMUP_LR if warmup_t(case) else BASE_LR
    return [v if s is None else v * s for s in LR_SCALES]


def exact_branch(case, t):
    """Whether the value at t comes from + - * / alone (warm-up, linear, cosine's constant tail): IEEE fp64 rounds those identically on
    the host and the device.  The other branches call cos or pow, whose device versions are a few fp64 ulp off libm's."""
    if t < warmup_t(case) or case['name'] == 'linear':
        return True
    if case['name'] == 'cosine':
        wt = warmup_t(case)
        t_initial = EPOCHS * N_ITER - wt if case['warmup_prefix'] else EPOCHS * N_ITER
        return ((t - wt) if case['warmup_prefix'] else t) // t_initial >= 1
    return False


def fp32_matches(got, want, exact):
    """The tolerance of the device-stepped rate words: ``got`` (an fp32 value) is ``want`` (fp64) rounded to fp32 - exactly in an exact
    branch, else that or one of its two fp32 neighbours (a few fp64 ulp of difference can only move a value across a rounding
    boundary, onto the neighbour)."""
    w = np.float32(want)
    g = np.float32(got)
    if g == w:
        return True
    return (not exact) and g in (np.nextafter(w, np.float32(-np.inf)), np.nextafter(w, np.float32(np.inf)))
