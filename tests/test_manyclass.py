"""CPU tests of the 5 .. 8-class training path: C-ABI surface and contract errors of ltu_loss_wide_*, the criterion names, the
state_dict surface, the synthetic many-class patches, and the oracle against the fixtures generated from the reference
(tests/golden/make_golden_manyclass.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import net as O_net
from oracle import seedgen
from oracle import step as O_step
from tests import manyclass_common as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('ltu_loss_wide_ws_floats', 'ltu_loss_wide_fwd', 'ltu_loss_wide_bwd')


def test_entry_points_declared_bound_and_exported():
    from lintransunet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ltu_hip.h')).read()
    declared = set(re.findall(r'^(?:int|long long)\s+(ltu_\w+)\s*\(', header, flags=re.M))
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    # the scratch pair is named sums / sums_floats, and the capacity is a long long right behind the pointer
    proto = re.search(r'int ltu_loss_wide_fwd\(([^;]*)\);', header, flags=re.S).group(1)
    names = [a.split()[-1].lstrip('*') for a in proto.split(',')]
    i = names.index('sums')
    assert names[i + 1] == 'sums_floats' and _lib.SIGNATURES['ltu_loss_wide_fwd'][i + 1] is _lib.L
    assert len(names) == len(_lib.SIGNATURES['ltu_loss_wide_fwd'])


def test_contract_errors_return_before_any_launch():
    """fake pointers: an entry that launched anything would fault; every refusal comes back as a code"""
    from lintransunet_amd import _lib
    lib = _lib.load()
    fake = 1 << 20
    B, S = 2, 4096
    for C in range(2, 9):
        need = lib.ltu_loss_wide_ws_floats(B, S, C)
        assert need >= 2 * B * C * 4, C
    assert lib.ltu_loss_wide_ws_floats(B, S, 1) == 0 and lib.ltu_loss_wide_ws_floats(B, S, 9) == 0
    assert lib.ltu_loss_wide_ws_floats(9, S, 8) == 0                            # 9 * 8 * 4 > 256
    C = 8
    need = lib.ltu_loss_wide_ws_floats(B, S, C)
    wd = (ctypes.c_float * (C + 1))(*([1.0] * (C + 1)))
    fwd = lambda c=C, ws=need, b=B, sums=fake: lib.ltu_loss_wide_fwd(fake, fake, sums, ws, fake, fake, b, S, c, 1.0, 1.0, wd, None, None)
    bwd = lambda c=C, b=B, dp=fake: lib.ltu_loss_wide_bwd(fake, fake, fake, fake, dp, b, S, c, None)
    assert fwd(c=1) == -2 and fwd(c=9) == -2                                    # LTU_E_SHAPE
    assert bwd(c=1) == -2 and bwd(c=9) == -2
    assert fwd(b=9, ws=1 << 30) == -2 and bwd(b=9) == -2                        # B * C * 4 > 256: beyond the finalize's rows
    assert fwd(ws=need - 1) == -4                                               # short scratch: LTU_E_ARG
    assert fwd(sums=None) == -4 and bwd(dp=None) == -4                          # NULL
    assert lib.ltu_loss_wide_fwd(fake, fake, fake, need, fake, fake, B, S, C, 1.0, 1.0, None, None, None) == -4
    # the refusals of the narrower entries stay: 9 and 0 classes in the heads, 5 in ltu_loss_fwd
    assert lib.ltu_head_softmax_fwd(fake, fake, 16, 9, 16, 0, None) == -2
    assert lib.ltu_head_softmax_bwd(fake, fake, fake, 16, 9, 16, 0, None) == -2
    assert lib.ltu_final_softmax_fwd(fake, fake, 1, 2, 2, 2, 9, 36, 0, None) == -2
    assert lib.ltu_final_softmax_bwd(fake, fake, fake, 1, 2, 2, 2, 9, 36, 0, None) == -2
    assert lib.ltu_head_softmax_fwd(fake, fake, 16, 0, 16, 0, None) == -2
    assert lib.ltu_head_softmax_bwd(fake, fake, fake, 16, 0, 16, 0, None) == -2
    assert lib.ltu_final_softmax_fwd(fake, fake, 1, 2, 2, 2, 0, 8, 0, None) == -2
    assert lib.ltu_final_softmax_bwd(fake, fake, fake, 1, 2, 2, 2, 0, 8, 0, None) == -2
    assert lib.ltu_final_softmax_fwd(fake, fake, 1, 2, 2, 2, 8, 28, 0, None) == -2      # CP < 4 C
    assert lib.ltu_head_softmax_fwd(fake, fake, 16, 8, 7, 0, None) == -2                # CP < C
    wd5 = (ctypes.c_float * 5)(*([1.0] * 5))
    assert lib.ltu_loss_fwd(fake, fake, fake, 1 << 30, fake, fake, B, S, 5, 1.0, 1.0, wd5, None, None) == -2


def test_level_criterion_names():
    from lintransunet_amd import losses as L
    from lintransunet_amd import train
    names = MC.criterion_names(8)
    assert names == ['CrossEntroLoss', 'DiceClassLoss', 'DiceClassLoss2', 'DiceClassLoss3', 'DiceClassLoss4', 'DiceClassLoss5',
                     'DiceClassLoss6', 'DiceClassLoss7']
    crit = L.LevelCriterion({n: 1.0 for n in names + ['DiceClassLoss0', 'DiceClassLoss0c', 'BalanceDiceLoss']})
    # the foreground union and class 4 have slots of their own, in both layouts
    assert L.LevelCriterion._DICE['DiceClassLoss0'] != L.LevelCriterion._DICE['DiceClassLoss4']
    wd = L.LevelCriterion({'DiceClassLoss0': 3.0, 'DiceClassLoss4': 5.0, 'DiceClassLoss': 7.0}).dice_weights(8)
    assert wd == [0.0, 7.0, 0.0, 0.0, 5.0, 0.0, 0.0, 0.0, 3.0]
    assert crit.dice_weights(8) == [1.0] * 9
    assert L.LevelCriterion({'DiceClassLoss0': 3.0, 'DiceClassLoss2': 2.0}, scale=0.5).dice_weights(3) == [0.0, 0.0, 1.0, 0.0, 1.5]
    # a class the prediction does not have, and the wider family above its limit: ValueError before anything is launched
    # (CPU tensors: a launch would be an error of another kind)
    p5 = torch.softmax(torch.randn(1, 5, 4, 4, 4), 1)
    lab = torch.zeros(1, 1, 4, 4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match='DiceClassLoss6'):
        L.LevelCriterion({'CrossEntroLoss': 1.0, 'DiceClassLoss6': 1.0})(p5, lab)
    with pytest.raises(ValueError, match='DiceClassLoss4'):
        L.LevelCriterion({'DiceClassLoss4': 1.0})(p5[:, :3], lab)
    with pytest.raises(ValueError, match=r'FocalLoss.*C <= 4'):
        L.LevelCriterion({'CrossEntroLoss': 1.0, 'FocalLoss': 1.0})(p5, lab)
    with pytest.raises(ValueError, match='C <= 8'):
        L.LevelCriterion({'CrossEntroLoss': 1.0})(torch.softmax(torch.randn(1, 9, 4, 4, 4), 1), lab)
    with pytest.raises(KeyError):
        L.LevelCriterion({'DiceClassLoss8': 1.0})
    # DiceClassLoss(class_index) selects the name as the reference's multi_criterions.DiceClassLoss does the class
    assert L.DiceClassLoss(class_index=5).impl.spec == {'DiceClassLoss5': 1.0}
    assert L.DiceClassLoss().impl.spec == {'DiceClassLoss': 1.0} and L.DiceClassLoss(class_index=1).impl.spec == {'DiceClassLoss': 1.0}
    assert L.DiceClassLoss(class_index=0).impl.spec == {'DiceClassLoss0c': 1.0}
    assert L.DiceClassLoss(class_index=2).impl.spec == {'DiceClassLoss2': 1.0}
    with pytest.raises(ValueError):
        L.DiceClassLoss(class_index=8)
    # the multi-class script's weighting: the same dict at every level
    cw = MC.criterion_weights(8)
    specs = train.level_specs(5, tuple(names), criterion_weight=cw)
    assert len(specs) == 5 and all(s == dict(zip(names, cw)) for s in specs)


@pytest.mark.parametrize('dim_output', [5, 8])
def test_state_dict_surface_matches_reference(dim_output):
    from lintransunet_amd.model import get_model_dict
    cfg = O_net.NetConfig(dim_output=dim_output)
    model = get_model_dict('MaskTransUnet')(cfg.num_layers, cfg.roi_size_list, cfg.is_roi_list, 1, dim_output)
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    want = O_net.param_shapes(cfg)
    assert got == want
    assert len(got) == 614
    assert got['decode.final_block.weight'][0] == 4 * dim_output
    model.load_state_dict(seedgen.seeded_params(want, 1), strict=True)
    bf = get_model_dict('MaskTransUnet')(cfg.num_layers, cfg.roi_size_list, cfg.is_roi_list, 1, dim_output, act_dtype=torch.bfloat16)
    assert bf._final_cop() == {5: 24, 8: 32}[dim_output] and model._final_cop() == 4 * dim_output


def _old_synthetic_labels(batch, size, seed, n_classes, n_blobs=2):
    """the generator of data.synthetic_patches as it stood for 2 and 3 label values"""
    from lintransunet_amd import data
    g = torch.Generator().manual_seed(seed)
    H, W, D = size
    x = torch.randn((batch, 1, H, W, D), generator=g).clamp_((data.LOW_CLIP - data.MEAN) / data.STD, (data.HIGH_CLIP - data.MEAN) / data.STD)
    hh = torch.arange(H, dtype=torch.float32).view(H, 1, 1)
    ww = torch.arange(W, dtype=torch.float32).view(1, W, 1)
    dd = torch.arange(D, dtype=torch.float32).view(1, 1, D)
    lab = torch.zeros((batch, 1, H, W, D), dtype=torch.uint8)
    for b in range(batch):
        for _ in range(n_blobs):
            c = 0.25 + 0.5 * torch.rand(3, generator=g)
            r = 0.12 + 0.15 * torch.rand(3, generator=g)
            dist = ((hh - c[0] * H) / (r[0] * H)) ** 2 + ((ww - c[1] * W) / (r[1] * W)) ** 2 + ((dd - c[2] * D) / (r[2] * D)) ** 2
            lab[b, 0][dist <= 1.0] = 1
            if n_classes == 3:
                lab[b, 0][dist <= 0.25] = 2
    return x, lab


def test_synthetic_patches_many_classes():
    from lintransunet_amd import data
    for k in (4, 5, 8):
        for seed in (1, 2, 3):
            x, lab = data.synthetic_patches(3, (32, 24, 16), seed, 'cpu', n_classes=k)
            assert lab.dtype == torch.uint8 and lab.shape == (3, 1, 32, 24, 16)
            for b in range(3):
                assert lab[b].unique().tolist() == list(range(k)), (k, seed, b)
    for k in (2, 3):
        x, lab = data.synthetic_patches(2, (32, 24, 16), 7, 'cpu', n_classes=k)
        x0, lab0 = _old_synthetic_labels(2, (32, 24, 16), 7, k)
        assert torch.equal(x, x0) and torch.equal(lab, lab0), k


@pytest.fixture(scope='module', params=[5, 8])
def oracle_run(request, golden_dir):
    """one oracle step (forward, loss, backward) per fixture, shared by the checks below"""
    C = request.param
    G = np.load(os.path.join(golden_dir, f'model_c{C}_small.npz'))
    cfg = O_net.NetConfig(dim_output=C, **MC.SMALL)
    wseed = MC.WSEED[C]
    P = seedgen.seeded_params(O_net.param_shapes(cfg), wseed, requires_grad=True)
    x = seedgen.seeded_volume((MC.BATCH, 1) + MC.SIZE, wseed + 1)
    label = MC.seeded_label((MC.BATCH, 1) + MC.SIZE, wseed + 2, C)
    boxes = []
    pred, masks = O_net.forward(P, cfg, x, True, boxes)
    total, levels = MC.total_loss(pred, masks, label, tuple(G['weights']), C)
    total.backward()
    return C, G, P, label, pred.detach(), [m.detach() for m in masks], boxes, total.detach(), levels


def test_oracle_reproduces_fixture(oracle_run):
    C, G, P, label, pred, masks, boxes, total, levels = oracle_run
    # every class at every level of the label pyramid
    for lab in O_step.label_pyramid(label, 5):
        assert torch.bincount(lab.long().flatten(), minlength=C).min().item() > 0
    assert np.allclose(G['weights'], O_step.dynamic_weights(0))
    idx = torch.from_numpy(G['out_idx'].astype(np.int64))
    assert torch.equal(idx, MC.out_indices(C)) and idx.numel() == C * MC.OUT_SAMPLES
    assert np.abs(pred.flatten()[idx].numpy() - G['out_sample']).max() <= 1e-5
    assert len(masks) == 4
    for i, m in enumerate(masks):
        assert np.abs(m.numpy() - G[f'mask{i}']).max() <= 1e-5, i
    for i, b in enumerate(boxes):
        assert np.array_equal(b.numpy(), G[f'box{i}']), i
    assert abs(total.item() - float(G['total'])) <= 1e-5 * max(1.0, abs(float(G['total'])))
    got = np.array([[v.item() for v in vals] for vals in levels])
    assert got.shape == (5, C) and np.allclose(got, G['level_losses'], rtol=1e-5, atol=1e-6)
    from oracle import losses as O_loss
    t = MC.onehot(label, C)
    dice = [O_loss.dice_class_onehot(pred, t, c).item() for c in range(C)]
    assert np.allclose(dice, G['dice'], rtol=0, atol=1e-5)
    norms = dict(zip(G['grad_keys'], G['grad_norms']))
    assert len(norms) == 600
    for k, n in norms.items():
        assert abs(P[k].grad.double().norm().item() - n) <= 2e-4 * max(1.0, n), k
