"""ops.level_loss_chain on the GPU: combinations of two to four stages (base of each loss family, boundary, top-k, imbalance), and
the imbalance stage alone, against the same stages run alone - total and gradient to one joined fp32 add, every report bit for
bit - on a shape the four-voxel kernels take and one the scalar kernels take (S % 4 != 0).  Inputs are those of
tests/topk_common.py."""
import functools

import pytest
import torch

from tests.topk_common import make_labels, make_probs

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SHAPES = [(2, (12, 10, 8)), (1, (9, 7, 5))]
# classes of the prediction.  4 for ltu_loss: it writes the Dice slot of every class the prediction has and leaves the slots of absent
# classes of its 4-class report unwritten, so only there is the whole report defined
FAMILIES = {'orig': 4, 'wide': 5, 'ext': 3}
STAGES = ('base', 'boundary', 'topk', 'imbalance')
COMBOS = [(f, s) for f in FAMILIES for s in (('base', 'boundary'), ('base', 'topk'), STAGES[:3])] + [('orig', ('boundary', 'topk'))]
# appended, so that the cases above keep their ids: the imbalance stage behind each base, behind all stages, without a base, and alone
COMBOS += [(f, s) for f in FAMILIES for s in (('base', 'imbalance'), STAGES)]
COMBOS += [('orig', s) for s in (('boundary', 'imbalance'), ('topk', 'imbalance'), ('imbalance',))]


@functools.lru_cache(maxsize=None)
def _inputs(B, spatial, C):
    """p [B, *spatial, C], label u8 [B, *spatial] and the signed distance maps of classes 1 and 2, on the device; read only"""
    from lintransunet_amd import ops
    p = torch.from_numpy(make_probs(B, spatial, C, 7 * B + C)).to(DEV)
    lab = torch.from_numpy(make_labels(B, spatial, C, 9 * B + C)).to(DEV)
    return p, lab, ops.signed_distance_maps(lab, (1, 2), (1.0, 1.0, 2.0))


def _stage(family, name, phi):
    from lintransunet_amd import ops
    if name == 'boundary':
        return (phi, (1, 2), (0.05, 0.02), None)
    if name == 'topk':
        return (0.7, 0.2, None)
    if name == 'imbalance':      # a focal Tversky term of classes 1 and 2, which every family's prediction has, and a focal cross-entropy
        return (((1, 2), (0.6, 0.4), {'gamma': 4.0 / 3.0}), (0.5, 2.0, None))
    if family == 'ext':
        return ('ltu_loss_ext', ops.loss_ext_cfg({'CE': 1.0, 'FOCAL': 1.0, 'DICE': 0.5}))
    wd = (0.0, 1.0, 1.0, 0.5, 0.5) if family == 'orig' else (0.0, 1.0, 1.0, 0.0, 1.0, 0.5)
    return ('ltu_loss' if family == 'orig' else 'ltu_loss_wide', (10.0, 0.5, wd))


def _run(family, stages, B, spatial):
    """-> (total, gradient, reports of the four stages) of the chain of `stages`"""
    from lintransunet_amd import ops
    p, lab, phi = _inputs(B, spatial, FAMILIES[family])
    pg = p.clone().requires_grad_(True)
    total, *reports = ops.level_loss_chain(pg, lab, **{s: _stage(family, s, phi) for s in stages})
    total.backward()
    return total.detach(), pg.grad, reports


@functools.lru_cache(maxsize=None)
def _alone(family, stage, B, spatial):
    return _run(family, (stage,), B, spatial)


@pytest.mark.parametrize('B,spatial', SHAPES)
@pytest.mark.parametrize('family,stages', COMBOS)
def test_chain_is_the_sum_of_its_stages(family, stages, B, spatial):
    total, grad, reports = _run(family, stages, B, spatial)
    alone = [_alone(family, s, B, spatial) for s in stages]
    for k, name in enumerate(STAGES):
        if name not in stages:
            assert reports[k] is None
        else:
            want = alone[stages.index(name)][2][k]
            assert not reports[k].requires_grad and torch.equal(reports[k], want), name
    want = sum(t.item() for t, _, _ in alone)
    # the boundary term is signed: the relative bound below means something only if the stages' totals do not cancel
    assert abs(want) >= 0.5 * sum(abs(t.item()) for t, _, _ in alone)
    gsum = sum(g.double() for _, g, _ in alone)
    eg = (grad.double() - gsum).abs().max().item() / gsum.abs().max().item()
    print(f'{family} {"+".join(stages)} B={B} {spatial}: total {total.item():.8f} separate {want:.8f}, gradient max |diff| / max {eg:.2e}')
    assert abs(total.item() - want) <= 1e-6 * abs(want)
    assert eg <= 1e-6
    # a second call: bit for bit
    total2, grad2, reports2 = _run(family, stages, B, spatial)
    assert torch.equal(total2, total) and torch.equal(grad2, grad)
    assert all(a is None if b is None else torch.equal(a, b) for a, b in zip(reports2, reports))


def test_no_stage_raises():
    from lintransunet_amd import ops
    p, lab, _ = _inputs(1, (9, 7, 5), 3)
    with pytest.raises(ValueError):
        ops.level_loss_chain(p, lab)
