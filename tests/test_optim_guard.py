"""Host side of the guarded AdamW step (optim.FusedAdamW's max_grad_norm / skip_nonfinite / ema_decay): constructor validation,
signature order and the C-ABI table of the new entry points.  No GPU."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('ltu_grad_sumsq_parts', 'ltu_grad_sumsq', 'ltu_adamw_guard', 'ltu_adamw_guarded')


def _cpu_reducer():
    from lintransunet_amd import train
    return train.GradReducer(torch.nn.Linear(3, 2))


@pytest.mark.parametrize('kw', [dict(max_grad_norm=0), dict(max_grad_norm=-1), dict(max_grad_norm=float('inf')),
                                dict(max_grad_norm=float('nan')), dict(ema_decay=-0.1), dict(ema_decay=1.0)])
def test_bad_guard_arguments_raise_before_the_gpu_check(kw):
    from lintransunet_amd import optim
    with pytest.raises(ValueError):
        optim.FusedAdamW(_cpu_reducer(), **kw)


def test_valid_guard_arguments_reach_the_gpu_check():
    """a reducer over a CPU model: valid guard arguments get as far as the GPU-only refusal (no CPU fallback)"""
    from lintransunet_amd import optim, _lib
    with pytest.raises(_lib.LtuError):
        optim.FusedAdamW(_cpu_reducer(), max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.0)


def test_constructor_keeps_its_positional_order():
    from lintransunet_amd import optim
    names = list(inspect.signature(optim.FusedAdamW.__init__).parameters)
    assert names == ['self', 'reducer', 'lr', 'betas', 'eps', 'weight_decay', 'max_grad_norm', 'skip_nonfinite', 'ema_decay']
    d = {k: v.default for k, v in inspect.signature(optim.FusedAdamW.__init__).parameters.items()}
    assert (d['max_grad_norm'], d['skip_nonfinite'], d['ema_decay']) == (None, False, None)


def test_new_symbols_match_the_header():
    from lintransunet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ltu_hip.h')).read()
    protos = dict(re.findall(r'^(?:int|long long)\s+(ltu_\w+)\s*\(([^;]*)\);', header, flags=re.M | re.S))
    for name in NEW_SYMBOLS:
        assert name in protos and name in _lib.SIGNATURES, name
        params = [re.sub(r'/\*.*?\*/', '', a, flags=re.S).strip() for a in protos[name].split(',')]
        assert len(params) == len(_lib.SIGNATURES[name]), name
        names = [p.split()[-1].lstrip('*') for p in params]
        if 'scratch' in names:        # the workspace contract: a scratch pointer is followed by its capacity, a long long
            i = names.index('scratch')
            assert params[i + 1].startswith('long long') and _lib.SIGNATURES[name][i + 1] is _lib.L, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert re.search(r'^long long\s+ltu_grad_sumsq_parts', header, flags=re.M)
    assert lib.ltu_grad_sumsq_parts.restype is _lib.c_longlong
    assert '#define LTU_GUARD_STATE_BYTES 48' in header
