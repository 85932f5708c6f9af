"""Host side of optim.FusedSGD and the closed-form schedules (PolyLR, CosineAnnealingLR, StepLR): constructor validation, the
C-ABI table of ltu_sgd / ltu_sgd_guarded, every schedule against torch's own scheduler on a dummy torch.optim.SGD, the
upload_lr() hook and the state dicts.  No GPU.
The schedule gate is 1e-12 relative: torch's recursive forms differ from the closed forms by a few ulp per step (at most 2.3e-15
measured over these runs); a 1000-step recursion in double is bounded by about 1000 * 2^-53 = 1.1e-13."""
import inspect
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('ltu_sgd', 'ltu_sgd_guarded')
RTOL = 1e-12


def _cpu_reducer():
    from lintransunet_amd import train
    return train.GradReducer(torch.nn.Linear(3, 2))


class _Stub:
    """an optimizer as the schedulers see one, with the upload hook"""

    def __init__(self, lr=1e-2):
        self.param_groups = [dict(lr=lr)]
        self.uploads = []

    def upload_lr(self):
        self.uploads.append(self.param_groups[0]['lr'])


class _Bare:
    def __init__(self, lr=1e-2):
        self.param_groups = [dict(lr=lr)]


# ---------------------------------------------------------------------------------------------- constructor and C-ABI table

@pytest.mark.parametrize('kw', [dict(lr=-1e-3), dict(lr=float('nan')), dict(momentum=-0.1), dict(weight_decay=-1e-5),
                                dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1),
                                dict(max_grad_norm=0), dict(max_grad_norm=-1), dict(max_grad_norm=float('inf')),
                                dict(max_grad_norm=float('nan')), dict(ema_decay=-0.1), dict(ema_decay=1.0)])
def test_bad_arguments_raise_before_the_gpu_check(kw):
    from lintransunet_amd import optim
    with pytest.raises(ValueError):
        optim.FusedSGD(_cpu_reducer(), **kw)


@pytest.mark.parametrize('kw', [dict(), dict(lr=0.0), dict(momentum=0.9, dampening=0.1, weight_decay=1e-2),
                                dict(momentum=0.99, nesterov=True, max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.0)])
def test_valid_arguments_reach_the_gpu_check(kw):
    """a reducer over a CPU model: valid arguments get as far as the GPU-only refusal (no CPU fallback)"""
    from lintransunet_amd import optim, _lib
    with pytest.raises(_lib.LtuError):
        optim.FusedSGD(_cpu_reducer(), **kw)


def test_nnunet_helper_reaches_the_gpu_check_and_refuses_a_second_lr():
    from lintransunet_amd import optim, _lib
    with pytest.raises(_lib.LtuError):
        optim.nnunet_sgd(_cpu_reducer(), ema_decay=0.5)
    with pytest.raises(TypeError):
        optim.nnunet_sgd(_cpu_reducer(), lr=1e-3)


def test_constructor_signature():
    from lintransunet_amd import optim
    params = inspect.signature(optim.FusedSGD.__init__).parameters
    assert list(params) == ['self', 'reducer', 'lr', 'momentum', 'dampening', 'weight_decay', 'nesterov', 'max_grad_norm',
                            'skip_nonfinite', 'ema_decay']
    assert [p.default for p in list(params.values())[2:]] == [1e-3, 0.0, 0.0, 0.0, False, None, False, None]
    for name in ('step', 'zero_grad', 'counters', 'state_dict', 'load_state_dict', 'ema_state_dict', 'ema_weights', 'upload_lr'):
        assert callable(getattr(optim.FusedSGD, name)), name


def test_new_symbols_match_the_header():
    from lintransunet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ltu_hip.h')).read()
    protos = dict(re.findall(r'^(?:int|long long)\s+(ltu_\w+)\s*\(([^;]*)\);', header, flags=re.M | re.S))
    ctype = {'float': _lib.F, 'int': _lib.I, 'long long': _lib.L}
    for name in NEW_SYMBOLS:
        assert name in protos and name in _lib.SIGNATURES, name
        params = [re.sub(r'/\*.*?\*/', '', a, flags=re.S).strip() for a in protos[name].split(',')]
        assert len(params) == len(_lib.SIGNATURES[name]), name
        for p, t in zip(params, _lib.SIGNATURES[name]):          # pointers and the stream are P, scalars by their C type
            want = _lib.P if ('*' in p or p.startswith('ltu_stream_t')) else ctype[p.rsplit(' ', 1)[0]]
            assert t is want, (name, p)
    names = [p.split()[-1].lstrip('*') for p in re.sub(r'/\*.*?\*/', '', protos['ltu_sgd_guarded'], flags=re.S).split(',')]
    assert names[5] == 'lr_dev' and 'lr' not in names          # the learning rate is a device pointer, not a launch argument
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


# ---------------------------------------------------------------------------------------------- schedules against torch

def _torch_opt(lr):
    return torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)


def _run_pair(mine, theirs, topt, steps):
    """lr after construction and after each of `steps` steps, (mine, torch's)"""
    out = [(mine.optimizer.param_groups[0]['lr'], topt.param_groups[0]['lr'])]
    for _ in range(steps):
        topt.step()
        mine.step(); theirs.step()
        out.append((mine.optimizer.param_groups[0]['lr'], topt.param_groups[0]['lr']))
    return out


def _assert_sequence(pairs):
    worst = 0.0
    for t, (a, b) in enumerate(pairs):
        if b == 0.0:
            assert a == 0.0, (t, a)
        else:
            worst = max(worst, abs(a - b) / abs(b))
            assert abs(a - b) <= RTOL * abs(b), (t, a, b)
    print(f'worst relative difference {worst:.2e}')


def test_poly_matches_torch():
    from lintransunet_amd import optim
    topt = _torch_opt(1e-2)
    pairs = _run_pair(optim.PolyLR(_Stub(1e-2), 1000, 0.9), torch.optim.lr_scheduler.PolynomialLR(topt, 1000, 0.9), topt, 1100)
    _assert_sequence(pairs)
    assert pairs[0][0] == 1e-2 and pairs[999][0] > 0 and all(a == 0.0 and b == 0.0 for a, b in pairs[1000:])
    assert optim.PolyLR(_Stub(), 1000).power == 0.9          # nnU-Net's exponent is the default


def test_cosine_matches_torch():
    from lintransunet_amd import optim
    topt = _torch_opt(1e-4)
    pairs = _run_pair(optim.CosineAnnealingLR(_Stub(1e-4), 100, 1e-6),
                      torch.optim.lr_scheduler.CosineAnnealingLR(topt, T_max=100, eta_min=1e-6), topt, 250)
    _assert_sequence(pairs)
    assert abs(pairs[100][0] - 1e-6) <= 1e-18 and abs(pairs[200][0] - 1e-4) <= 1e-16          # the bottom, and back up like torch


def test_step_matches_torch():
    from lintransunet_amd import optim
    topt = _torch_opt(1e-4)
    pairs = _run_pair(optim.StepLR(_Stub(1e-4), 250, 0.5), torch.optim.lr_scheduler.StepLR(topt, 250, 0.5), topt, 800)
    _assert_sequence(pairs)
    assert [pairs[t][0] for t in (249, 250, 499, 500, 750)] == [1e-4, 5e-5, 5e-5, 2.5e-5, 1.25e-5]


def test_helpers_build_the_named_schedules():
    from lintransunet_amd import optim
    s = optim.nnunet_schedule(_Stub())
    assert isinstance(s, optim.PolyLR) and (s.total_iters, s.power) == (1000, 0.9)
    assert optim.nnunet_schedule(_Stub(), epochs=250).total_iters == 250
    s = optim.reference_step_schedule(_Stub())
    assert isinstance(s, optim.StepLR) and (s.step_size, s.gamma) == (250, 0.5)
    s = optim.reference_cosine_schedule(_Stub())
    assert isinstance(s, optim.CosineAnnealingLR) and (s.T_max, s.eta_min) == (100, 1e-6)


# ---------------------------------------------------------------------------------------------- upload_lr

def _schedules(opt):
    from lintransunet_amd import optim
    return [optim.PolyLR(opt, 10), optim.CosineAnnealingLR(opt, 10, 1e-6), optim.StepLR(opt, 2, 0.5)]


def test_schedulers_call_upload_lr_after_writing():
    for k in range(3):
        opt = _Stub()
        sched = _schedules(opt)[k]
        for _ in range(3):
            sched.step()
        assert len(opt.uploads) == 3 and opt.uploads[-1] == opt.param_groups[0]['lr'], k          # called after the write
        assert opt.uploads[0] == sched._lr(1e-2, 1)


def test_schedulers_work_without_upload_lr():
    for k in range(3):
        opt = _Bare()
        sched = _schedules(opt)[k]
        sched.step()
        assert opt.param_groups[0]['lr'] == sched._lr(1e-2, 1)


METRICS = [1.0, 0.9, 0.95, 0.95, 0.95, 0.95, 0.95, 0.95, 0.95, 0.8, 0.85, 0.85, 0.85, 0.85, 0.85, 0.85, 0.85, 0.85, 0.85, 0.85, 0.85,
           0.85, 0.85, 0.85, 0.85, 0.85, 0.85, 0.85, 0.85, 0.85]


def test_plateau_sequence_is_unchanged_and_uploads():
    from lintransunet_amd import optim
    kw = dict(mode='min', factor=0.8, patience=5, threshold=1e-2, cooldown=1, min_lr=1e-7)
    topt = _torch_opt(1e-4)
    theirs = torch.optim.lr_scheduler.ReduceLROnPlateau(topt, **kw)
    with_hook, without = _Stub(1e-4), _Bare(1e-4)
    a, b = optim.reference_schedule(with_hook), optim.ReduceLROnPlateau(without, **kw)
    seq = []
    for m in METRICS:
        theirs.step(m); a.step(m); b.step(m)
        assert with_hook.param_groups[0]['lr'] == without.param_groups[0]['lr'] == topt.param_groups[0]['lr']
        seq.append(topt.param_groups[0]['lr'])
    reductions = sum(x != y for x, y in zip(seq, seq[1:]))
    assert reductions >= 2, seq
    assert with_hook.uploads == sorted(set(seq[1:]) - {1e-4}, reverse=True)          # one upload per reduction, with the new value


# ---------------------------------------------------------------------------------------------- state dicts

def test_schedule_state_dicts_round_trip():
    for k in range(3):
        opt = _Stub()
        sched = _schedules(opt)[k]
        for _ in range(5):
            sched.step()
        sd = sched.state_dict()
        assert sd['last_epoch'] == 5 and sd['base_lrs'] == [1e-2] and 'optimizer' not in sd
        # a resumed run: the optimizer carries the decayed lr, the schedule is built on it and then restored
        opt2 = _Stub(opt.param_groups[0]['lr'])
        sched2 = _schedules(opt2)[k]
        sched2.load_state_dict(sd)
        assert sched2.last_epoch == 5 and sched2.base_lrs == [1e-2]
        assert opt2.param_groups[0]['lr'] == opt.param_groups[0]['lr'] and opt2.uploads[-1] == opt.param_groups[0]['lr']
        for _ in range(6):
            sched.step(); sched2.step()
            assert opt2.param_groups[0]['lr'] == opt.param_groups[0]['lr']
        assert sched2.state_dict() == sched.state_dict()
    assert math.isclose(_schedules(_Stub())[0]._lr(1e-2, 5), 1e-2 * 0.5 ** 0.9, rel_tol=1e-15)
