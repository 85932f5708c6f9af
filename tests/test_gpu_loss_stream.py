"""The streaming passes of the level losses (csrc/loss_stream.h under csrc/loss.hip and csrc/loss_ext.hip) at shapes that reach every
branch of their loops.  The other loss tests stop at S = 4948, where a block of the sums pass has 256 voxels: no thread makes a second
trip and the loop with two trips in flight is never entered.  With B = 2 (csrc/common.h loss_rows):

  S = 600 004    1172 voxels a block, 512 blocks, the last with 1112: threads below 37 take one double trip, the rest the single tail
  S = 1 700 004  3324 voxels a block: two iterations of the double-trip loop
  S = 600 003    S % 4 != 0: one voxel per thread, five trips
  B = 3, S = 4100  17 blocks, the last with 4 voxels; three samples share the fold of the partials and 256 is no multiple of its rows

Base family: tests/test_gpu_manyclass.py's float64 check and tolerances (values 1e-4, gradient 1e-4 of its maximum, two calls
bit-identical); C <= 4 runs two trips in flight, C >= 5 one.  Wider family: the float64 restatement of tests/test_losses_ext.py with
the tolerances of tests/test_gpu_losses_ext.py::test_against_restatement (values 1e-5, gradient 1e-4 of its maximum; measured
here: values 6e-8 at the most, gradient 1.1e-7).  Backward alone: four voxels per thread against one (LTU_LOSS_SCALAR) on hand-made
coefficients, bit for bit: the rounding of a voxel's gradient is written out in the kernels, so both paths do the same arithmetic."""
import pytest
import torch

from oracle import losses as O_loss
from tests.test_gpu_manyclass import _check_level_loss, _loss_inputs, G
from tests.test_gpu_ops import _with_knob
from tests.test_losses_ext import restate

pytestmark = pytest.mark.gpu

DEV = 'cuda'
S_DOUBLE, S_DOUBLE2, S_SCALAR, S_FOLD = 600004, 1700004, 600003, 4100      # the shapes of the table above (S_FOLD with B = 3)


@pytest.fixture(scope='module')
def ops():
    from lintransunet_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


# ---------------------------------------------------------------------------------------------- base family

BASE = ([(C, S_DOUBLE, 2) for C in (2, 4, 5, 8)] + [(C, S_DOUBLE2, 2) for C in (2, 5)] + [(C, S_SCALAR, 2) for C in (1, 2, 4, 5, 8)]
        + [(C, S_FOLD, 3) for C in (2, 4, 5, 8)])


@pytest.mark.parametrize('C,S,B', BASE, ids=[f'C{c}-S{s}-B{b}' for c, s, b in BASE])
def test_level_loss_long_blocks(ops, C, S, B):
    _check_level_loss(ops, C, S, wide=C > 4, B=B)


# ---------------------------------------------------------------------------------------------- wider family

EXT_WEIGHTS = {'CE': 1.0, 'SS': 0.5, 'FOCAL': 0.8, 'CE0': 1.5, 'CLASSIFY': 0.3}      # every flag of the kernels: E, Q, F, E0b, classify
EXT_NAMES = {'SS': 'SSLoss', 'FOCAL': 'FocalLoss', 'CE0': 'CrossEntroLoss0', 'CLASSIFY': 'ClassifyLoss'}
EXT = [(C, S, B, gamma) for C in (2, 4) for S, B in ((S_DOUBLE, 2), (S_SCALAR, 2), (S_FOLD, 3)) for gamma in (2.0, 1.5)]


def _ext_inputs(C, S, B, seed):
    g = G(seed)
    p = torch.softmax(torch.randn(B, S, C, generator=g) * 1.5, -1)
    lab = torch.randint(0, C, (B, S), generator=g).to(torch.uint8)
    return p, lab


def _ext_reference(p, lab, gamma):
    """float64: {term: value}, total and gradient of the EXT_WEIGHTS spec"""
    B, S, C = p.shape
    pr = p.double().requires_grad_(True)
    pred = pr.permute(0, 2, 1)                                                        # [B, C, S]
    onehot = (lab.long()[:, None, :] == torch.arange(C)[None, :, None]).double()
    terms = {'CE': O_loss._multi_ce(pred, onehot)}
    for k, name in EXT_NAMES.items():
        terms[k] = restate(name, pred, lab[:, None, :], gamma=gamma)
    total = sum(EXT_WEIGHTS[k] * v for k, v in terms.items())
    total.backward()
    return {k: v.item() for k, v in terms.items()}, total.item(), pr.grad


@pytest.mark.parametrize('C,S,B,gamma', EXT, ids=[f'C{c}-S{s}-B{b}-gamma{g}' for c, s, b, g in EXT])
def test_level_loss_ext_long_blocks(ops, C, S, B, gamma):
    p, lab = _ext_inputs(C, S, B, 500 + C + S)
    terms_ref, total_ref, dp_ref = _ext_reference(p, lab, gamma)
    runs = []
    for _ in range(2):
        pd = p.to(DEV).requires_grad_(True)
        tot, values = ops.level_loss_ext(pd, lab.to(DEV), EXT_WEIGHTS, {'gamma': gamma})
        tot.backward()
        torch.cuda.synchronize()
        runs.append((tot.detach().clone(), values.detach().clone(), pd.grad.clone()))
    (t0, v0, g0), (t1, v1, g1) = runs
    assert torch.equal(t0, t1) and torch.equal(v0, v1) and torch.equal(g0, g1), 'two calls must be bit-identical'
    err = {k: abs(v0[1 + ops.LOSS_EXT_TERMS.index(k)].item() - r) / max(1.0, abs(r)) for k, r in terms_ref.items()}
    err['total'] = abs(t0.item() - total_ref) / max(1.0, abs(total_ref))
    gerr = rel_err(g0, dp_ref)
    print(f'[ext C = {C}, S = {S}, B = {B}, gamma = {gamma}] value errors {err} gradient {gerr:.3e}')
    assert t0.item() == v0[0].item()
    assert all(e <= 1e-5 for e in err.values()), err
    assert gerr < 1e-4


# ---------------------------------------------------------------------------------------------- backward alone

def _bwd_pair(run):
    a = run()
    b = _with_knob(b'LTU_LOSS_SCALAR', 1, run)
    return a, b


@pytest.mark.parametrize('C', [2, 5, 8])
def test_level_loss_bwd_paths_bit_identical(ops, C):
    """ltu_loss_bwd (C = 2; above 4 classes it hands on to ltu_loss_wide_bwd) with coefficients of the size a loss gives them"""
    from lintransunet_amd import _lib
    B, S = 2, S_DOUBLE
    p, lab, _ = _loss_inputs(C, S, 600 + C)
    g = G(610 + C)
    coef = ((torch.rand(B, C, 3, generator=g) - 0.5) * 1e-5).to(DEV)
    gs = torch.tensor([0.7], device=DEV)
    pd, labd = p.to(DEV), lab.to(DEV)

    def run():
        dp = torch.full_like(pd, float('nan'))
        _lib.call('ltu_loss_bwd', ops._p(pd), ops._p(labd), ops._p(coef), ops._p(gs), ops._p(dp), B, S, C, ops._s())
        torch.cuda.synchronize()
        return dp
    a, b = _bwd_pair(run)
    assert torch.isfinite(a).all() and a.abs().max().item() > 0
    assert torch.equal(a, b)


@pytest.mark.parametrize('gamma', [2.0, 1.5])
def test_level_loss_ext_bwd_paths_bit_identical(ops, gamma):
    """ltu_loss_ext_bwd at C = 3 with every derivative term switched on"""
    from lintransunet_amd import _lib
    B, S, C = 2, S_DOUBLE, 3
    p, lab = _ext_inputs(C, S, B, 700)
    g = G(710)
    coef = ((torch.rand(B, C, 8, generator=g) - 0.5) * 1e-5).to(DEV)
    gs = torch.tensor([0.7], device=DEV)
    cfg = ops.loss_ext_cfg(EXT_WEIGHTS, {'gamma': gamma})
    pd, labd = p.to(DEV), lab.to(DEV)

    def run():
        dp = torch.full_like(pd, float('nan'))
        _lib.call('ltu_loss_ext_bwd', ops._p(pd), ops._p(labd), ops._p(coef), cfg, ops._p(gs), ops._p(dp), B, S, C, ops._s())
        torch.cuda.synchronize()
        return dp
    a, b = _bwd_pair(run)
    assert torch.isfinite(a).all() and a.abs().max().item() > 0
    assert torch.equal(a, b)
