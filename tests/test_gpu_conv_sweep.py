"""Conv shapes on both sides of every launcher's shape rule, and a seeded random fill, against float64.

tests/test_gpu_conv_paths.py enters every conv kernel at a shape well inside its domain.  Here the shapes come from the rules
that pick the kernel (tests/conv_sweep_common.py RULES: adjacent shapes on the two sides of each clause, 127 | 128 bricks,
W = 3 | 4, N = 32 | 40, 1023 | 1024 rows ...) and from random_cases; tests/test_conv_sweep.py holds that table against the sources.
Operands, float64 references and gates are reference / run_case of test_gpu_conv_paths.py, unchanged:

* bf16 outputs and data gradients element-wise: |got - ref| <= 2^-8 |ref| + 1e-5 max|ref|;
* fp32 weight and bias gradients: max|got - ref| / max|ref| <= 1e-4;
* padded head columns exactly 0, every output finite.

test_rule witnesses the kernels of each side with torch.profiler: the kernel named for a side ran in its direction's window, the
other side's did not.  A side marked REFUSED raises LtuError.  test_random_sweep runs 240 cases through the gates alone; a case
that raises fails, since the generator's space is the accepted one.  test_refusals: what the C ABI refuses leaves its outputs
untouched.  LTU_CONV_SWEEP_REPORT=<file> appends one JSON line per case: shape, knobs, kernels seen, worst error / bound.
"""
import json
import os

import pytest
import torch

from tests import conv_sweep_common as S
from tests import test_gpu_conv_paths as CP
from tests.test_gpu_conv_paths import gpu  # noqa: F401  (fixture)

SEED, NRANDOM, NCHUNK = 20261021, 240, 8


def _report(**line):
    path = os.environ.get('LTU_CONV_SWEEP_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(line, default=str) + '\n')


def _bases(seen):
    """{'fwd' | 'bwd': kernel names without template arguments}"""
    return {k: sorted({n.split('<')[0] for n in v}) for k, v in seen.items()}


def _run(case):
    return CP.run_case(case, witness=True, backward=case.backward, seed=S.case_seed(case.name))


@pytest.mark.gpu
@pytest.mark.parametrize('rule', S.RULES, ids=[r.name for r in S.RULES])
def test_rule(gpu, rule):  # noqa: F811
    from lintransunet_amd._lib import LtuError
    problems = []
    for sd in rule.sides:
        case = rule.case(sd)
        if sd.kernels == S.REFUSED:
            try:
                _run(case)
                problems.append(f'{case.name}: no LtuError')
            except LtuError as e:
                _report(rule=rule.name, case=case.name, shape=case.shape, knobs=case.knobs, refused=str(e))
            continue
        res = _run(case)
        seen = _bases(res['seen'])
        _report(rule=rule.name, case=case.name, shape=case.shape, knobs=case.knobs, expected=sd.kernels, seen=seen, ratio=res['ratio'])
        problems += [f'{case.name}: {f}' for f in res['fails']]
        for direction, names in sd.kernels.items():
            window = seen['fwd' if direction == 'fwd' else 'bwd']
            others = {k for o in rule.sides if o is not sd and o.kernels != S.REFUSED for k in o.kernels.get(direction, ())} - set(names)
            problems += [f'{case.name} {direction}: {k} did not run; launched {window}' for k in names if k not in window]
            problems += [f'{case.name} {direction}: {k}, the kernel of another side, ran' for k in others if k in window]
    assert not problems, f'{rule.name} ({rule.sources[0][2]}):\n' + '\n'.join(problems)


@pytest.mark.gpu
@pytest.mark.parametrize('chunk', range(NCHUNK))
def test_random_sweep(gpu, chunk):  # noqa: F811
    from lintransunet_amd._lib import LtuError
    per = NRANDOM // NCHUNK
    problems = []
    for case in S.random_cases(SEED, NRANDOM)[chunk * per:(chunk + 1) * per]:
        try:
            res = CP.run_case(case, witness=False, backward=case.backward, seed=S.case_seed(case.name))
            problems += [f'{case.name}: {f}' for f in res['fails']]
            _report(case=case.name, shape=case.shape, ratio=res['ratio'])
        except (LtuError, AssertionError) as e:
            problems.append(f'{case.name}: {type(e).__name__}: {e}')
            _report(case=case.name, shape=case.shape, error=str(e))
        CP._REF.pop(case.name, None)
    assert not problems, f'{len(problems)} of {per} cases:\n' + '\n'.join(problems)


@pytest.mark.gpu
def test_refusals(gpu):  # noqa: F811
    """the shapes refusal() rejects, through the C ABI: LtuError, and the NaN-filled outputs stay as they were"""
    from lintransunet_amd import _lib, ops
    from lintransunet_amd.ops import _p, _s
    B, H, W, D = 1, 3, 5, 9

    def bf(*shape):
        return torch.zeros(shape, device=CP.DEV, dtype=torch.bfloat16)

    def nan(*shape, dtype=torch.bfloat16):
        return torch.full(shape, float('nan'), device=CP.DEV, dtype=dtype)

    def fwd(c0, c1, co, st=(1, 1, 1)):
        assert S.refusal('conv3d', CP.conv(B, c0, co, H, W, D, stride=st, C1=c1), backward=False)
        y = nan(B, H, W, D, co)
        return [y], lambda: _lib.call('ltu_conv3d_fwd', _p(bf(B, H, W, D, c0)), _p(bf(B, H, W, D, c1)) if c1 else 0, _p(bf(co, 27, c0 + c1)),
                                      _p(torch.zeros(co, device=CP.DEV)), _p(y), B, H, W, D, c0, c1, co, *st, 0, 0, 0, ops.BF16, _s())

    def dgrad(c0, co, st=(1, 1, 1)):
        dx = nan(B, H, W, D, c0)
        return [dx], lambda: _lib.call('ltu_conv3d_dgrad', _p(bf(B, H, W, D, co)), _p(bf(c0, 27, co)), _p(dx), 0, B, H, W, D, c0, 0, co, *st,
                                       0, 0, ops.BF16, _s())

    def wgrad(c0, co):
        dw, db = nan(co, c0, 3, 3, 3, dtype=torch.float32), nan(co, dtype=torch.float32)
        return [dw, db], lambda: _lib.call('ltu_conv3d_wgrad', _p(bf(B, H, W, D, co)), _p(bf(B, H, W, D, c0)), 0, _p(dw), _p(db), B, H, W, D,
                                           c0, 0, co, 1, 1, 1, 0, co, c0, 0, 0, ops.BF16, _s())

    def pair_fwd(c, n0, n1):
        assert S.refusal('pair', CP.pair(B, c, n0, 1, n1, H, W, D), backward=False)
        y0, y1 = nan(B, H, W, D, n0), nan(B, H, W, D, n1)
        return [y0, y1], lambda: _lib.call('ltu_conv3d_pair_fwd', _p(bf(B, H, W, D, c)), _p(bf(n0 + n1, 27, c)), _p(torch.zeros(n0 + n1, device=CP.DEV)),
                                           _p(y0), _p(y1), B, H, W, D, c, n0, n1, 0, 0, ops.BF16, _s())

    def up_fwd(ci, co):
        assert S.refusal('upconv', CP.up(B, ci, co, H, W, D), backward=False)
        y = nan(B, 2 * H, 2 * W, 2 * D, co)
        return [y], lambda: _lib.call('ltu_upconv_fwd', _p(bf(B, H, W, D, ci)), _p(bf(8, co, 8, ci)), _p(torch.zeros(co, device=CP.DEV)), _p(y),
                                      B, H, W, D, ci, co, ops.BF16, _s())

    calls = {'fwd C0 % 4': fwd(6, 0, 16), 'fwd C1 % 4': fwd(16, 6, 16), 'fwd C0 % 8': fwd(12, 0, 16), 'fwd Co % 4': fwd(16, 0, 6),
             'fwd stride 3': fwd(16, 0, 16, (1, 3, 1)), 'dgrad Co % 4': dgrad(16, 6), 'dgrad Co % 8': dgrad(16, 12),
             'dgrad stride 3': dgrad(16, 16, (3, 1, 1)), 'wgrad Co % 4': wgrad(16, 6), 'wgrad Co % 8': wgrad(16, 12),
             'pair N0 % 4': pair_fwd(16, 6, 8), 'pair N1 % 4': pair_fwd(16, 8, 6), 'upconv Ci % 4': up_fwd(6, 32), 'upconv Co % 4': up_fwd(32, 6)}
    problems = []
    for what, (outs, call) in calls.items():
        try:
            call()
            problems.append(f'{what}: no LtuError')
        except _lib.LtuError:
            pass
        torch.cuda.synchronize()
        if not all(bool(torch.isnan(o).all()) for o in outs):
            problems.append(f'{what}: the refused call wrote to its output')
    assert not problems, '\n'.join(problems)
