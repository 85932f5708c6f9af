"""soft-clDice on the CPU: the two oracles of tests/cldice_common.py against each other, the uniqueness of the gradient on tie-free
inputs that the GPU comparison against the published composition rests on, the label skeleton being 0 / 1, and the host surface
(names, modules, argument checks) that runs without a GPU."""
import numpy as np
import pytest
import torch

from tests.cldice_common import (SHAPES, blob_labels, field_error, noise, noise_probs, plateau_case, pub_cldice, pub_label_skeletons,
                                 pub_op, rule_cldice, rule_morph, rule_morph_bwd, rule_skeleton)

ITERS = (1, 3, 6)


@pytest.mark.parametrize('B,spatial', SHAPES)
def test_oracles_agree_on_tie_free_input(B, spatial):
    x = noise((B,) + spatial, 3)
    g = np.random.default_rng(4).standard_normal(x.shape)
    for name, dilate in (('erode', False), ('dilate', True)):
        y, dx = pub_op(name, x, g)
        yr, tap = rule_morph(x.astype(np.float64), dilate)
        assert np.array_equal(y, yr) and field_error(rule_morph_bwd(g, tap, dilate), dx) <= 1e-14      # up to 27 float64 adds in another order
    for iters in ITERS:
        y, dx = pub_op('skeleton', x, g, iters)
        yr, dxr, _ = rule_skeleton(x, g, iters)
        assert np.abs(y - yr).max() <= 1e-15 and field_error(dxr, dx) <= 1e-14, iters
    p, lab = noise_probs(B, spatial, 3, 5), blob_labels(B, spatial, 3, 6)
    total, values, dp = pub_cldice(p, lab, (1, 2), (1.0, 0.5), 3)
    total_r, values_r, dp_r, _ = rule_cldice(p, lab, (1, 2), (1.0, 0.5), 3)
    assert abs(total - total_r) <= 1e-14 and np.abs(values - values_r).max() <= 1e-14 and field_error(dp_r, dp) <= 1e-13


@pytest.mark.parametrize('shape', [(1, 9, 7, 5), (2, 12, 10, 8), (1, 37, 22, 70)])
@pytest.mark.parametrize('iters', ITERS)
def test_gradient_is_unique_on_tie_free_input(shape, iters):
    """every I_j, D_j is a copy of one input voxel, so flipping the volume (which reverses every scan order a tie rule could follow)
    and flipping back leaves the published gradient where it was"""
    x = noise(shape, 11)
    g = np.random.default_rng(12).standard_normal(x.shape)
    _, dx = pub_op('skeleton', x, g, iters)
    flip = lambda a: np.ascontiguousarray(a[:, ::-1, ::-1, ::-1])
    _, dxf = pub_op('skeleton', flip(x), flip(g), iters)
    diff = field_error(flip(dxf), dx)
    print(f'{shape} iters {iters}: max difference / max |gradient| {diff:.2e}')
    assert diff <= 1e-14          # the flipped pass adds a voxel's up to 34 contributions in the reverse order: 34 x 2^-53 of their size


@pytest.mark.parametrize('iters', ITERS)
def test_label_skeleton_is_binary(iters):
    lab = blob_labels(2, (12, 10, 8), 3, 21)
    sk = pub_label_skeletons(lab, (0, 1, 2, 3), iters)
    assert np.isin(sk, (0.0, 1.0)).all() and sk[:, 1].sum() > 0 and sk[:, 3].sum() == 0
    ones = pub_label_skeletons(np.ones((1, 6, 5, 4), np.uint8), (1,), iters)
    assert np.isin(ones, (0.0, 1.0)).all()
    # the rule oracle on 0 / 1 maps gives the same bytes, plateaus throughout
    for k, c in enumerate((0, 1, 2, 3)):
        G = (lab == c).astype(np.float64)
        assert np.array_equal(rule_skeleton(G, np.zeros_like(G), iters)[0], sk[:, k])


def test_plateau_input_has_stable_masks():
    """the condition the GPU plateau test puts on its input: no relu mask of the chain depends on the precision"""
    p, lab = plateau_case()
    for iters in ITERS:
        m64 = rule_cldice(p, lab, (1, 2), (1.0, 0.5), iters)[3]
        m32 = rule_cldice(p, lab, (1, 2), (1.0, 0.5), iters, np.float32)[3]
        assert len(m64) == len(m32) and all(np.array_equal(a, b) for a, b in zip(m64, m32))
        assert any(m.any() for m in m64)


def test_host_surface():
    from lintransunet_amd import losses as L, ops, train
    crit = L.LevelCriterion({'ClDiceLoss': 1.0, 'ClDiceLoss2': 0.5, 'DiceClassLoss': 1.0})
    assert crit.cldice_classes == (1, 2) and crit.cldice_iters == 3
    assert L.stage_names({'ClDiceLoss0c': 1.0, 'CrossEntroLoss': 1.0})['cldice'] == ['ClDiceLoss0c']
    assert list(L.LevelCriterion.OWNED)[-1] == 'cldice' and set(L.LevelCriterion.CLDICE.values()) == set(range(8))
    assert L.cldice_name(7) == 'ClDiceLoss7' and L.cldice_classes({'ClDiceLoss2': 1.0}) == (2,)
    mods = L.get_criterions(['ClDiceLoss'])
    assert isinstance(mods['ClDiceLoss'], L.ClDiceLoss) and mods['ClDiceLoss'].impl.cldice_iters == 3
    assert L.ClDiceLoss(class_index=2, iters=5).impl.cldice_classes == (2,)
    for bad in (0, 11, 2.5):
        with pytest.raises(ValueError):
            L.LevelCriterion({'ClDiceLoss': 1.0}, cldice_iters=bad)
        with pytest.raises(ValueError):
            L.ClDiceLoss(iters=bad)
    predict, target = torch.rand(1, 2, 6, 5, 4), torch.zeros(1, 1, 6, 5, 4, dtype=torch.uint8)
    with pytest.raises(ValueError):          # a class the prediction lacks
        L.LevelCriterion({'ClDiceLoss2': 1.0})(predict, target)
    with pytest.raises(ValueError):          # 2-D patches: p would be 4-D
        L.LevelCriterion({'ClDiceLoss': 1.0})(predict[..., 0], target[..., 0])
    p, lab = torch.rand(1, 6, 5, 2), torch.zeros(1, 6, 5, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.level_loss_cldice(p, lab, (1,), (1.0,))
    p, lab = torch.rand(1, 6, 5, 4, 2), torch.zeros(1, 6, 5, 4, dtype=torch.uint8)
    for kw in (dict(classes=(2,), weights=(1.0,)), dict(classes=(1, 1), weights=(1.0, 1.0)), dict(classes=(1,), weights=(1.0,), iters=0),
               dict(classes=(1,), weights=(1.0, 2.0)), dict(classes=(), weights=())):
        with pytest.raises(ValueError):
            ops.level_loss_cldice(p, lab, **kw)
    with pytest.raises(ValueError):
        ops.soft_skeleton(torch.rand(1, 4, 4, 4), 11)
    # levels without a name get no skeleton (nothing is launched for them)
    specs = train.level_specs(5, ('CrossEntroLoss', 'DiceClassLoss'))
    assert train.skeleton_maps([None] * 5, specs, 3) == [None] * 5
