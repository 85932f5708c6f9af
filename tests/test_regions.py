"""Region-based training, host side: the restatement of tests/region_common.py that the GPU tests compare against (its analytic
gradients against torch.autograd on a float64 CPU restatement, its named special cases against the imbalance oracle, nnU-Net's
labelling loop, max-pooling), the losses.Regions record, the region names of losses.LevelCriterion, the new keywords of the step and
the model, and the C-ABI surface of csrc/region.hip and the sigmoid heads."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import region_common as RC
from tests.imbalance_common import imbalance_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ltu_region_bits', 'ltu_bits_orpool', 'ltu_loss_region_ws_floats', 'ltu_loss_region_fwd', 'ltu_loss_region_bwd',
       'ltu_region_labels', 'ltu_region_prob_bits', 'ltu_region_counts', 'ltu_head_sigmoid_fwd', 'ltu_head_sigmoid_bwd',
       'ltu_final_sigmoid_fwd', 'ltu_final_sigmoid_bwd', 'ltu_prob_indicator', 'ltu_roi_plan_union')
NON_NESTED = ((1, 2), (2, 3), (4,))


# ---------------------------------------------------------------------------------------------- the oracle
def _torch_total(p, bits, w_bce, w_dice, batch, eps):
    """the formulas once more, in torch float64, written for autograd (no analytic derivative anywhere)"""
    B, R = p.shape[0], p.shape[-1]
    pf = p.reshape(B, -1, R)
    t = ((bits.reshape(B, -1, 1) >> torch.arange(R).reshape(1, 1, R)) & 1).double()
    I, FP, FN = (pf * t).sum(1), (pf * (1 - t)).sum(1), (t * (1 - pf)).sum(1)
    c = float(RC.CLAMP32)
    E = -(t * torch.log(torch.clamp(pf, min=c)) + (1 - t) * torch.log(torch.clamp(1 - pf, min=c)))
    if batch:
        I, FP, FN = I.sum(0), FP.sum(0), FN.sum(0)
    D = (FP + FN) / (2 * I + FP + FN + 2 * eps)
    if not batch:
        D = D.mean(0)
    return w_bce * E.sum() / (B * pf.shape[1] * R) + w_dice * D.mean()


@pytest.mark.parametrize('batch', [False, True])
@pytest.mark.parametrize('kind', ['random', 'late'])
def test_oracle_gradients_against_autograd(kind, batch):
    B, spatial, R = 2, (6, 5, 4), 3
    p, _, bits, _ = RC.make_region_case(B, spatial, R, 3, NON_NESTED)
    if kind == 'late':
        p = RC.late_region_probs(bits, R, 5, confident=0.8, wrong=0.05)
        assert (p == 0).any() and (p == 1).any()                     # p exactly 0 and 1, on the right and on the wrong side
    r = RC.region_ref(p, bits, 0.7, 1.3, batch, 1e-5)
    pt = torch.from_numpy(p.astype(np.float64)).requires_grad_(True)
    total = _torch_total(pt, torch.from_numpy(bits.astype(np.int64)), 0.7, 1.3, batch, 1e-5)
    total.backward()
    assert abs(total.item() - r['total']) <= 1e-12 * abs(r['total'])
    g = pt.grad.numpy()
    # torch's clamp passes no gradient below the clamp: the same rule
    assert np.isfinite(g).all() and np.isfinite(r['grad']).all() and np.abs(g - r['grad']).max() <= 1e-11 * np.abs(g).max()
    assert all((x >= 0).all() for x in r['sums'])


@pytest.mark.parametrize('batch', [False, True])
def test_dice_term_is_tversky_half_half(batch):
    B, spatial = 3, (7, 5, 4)
    p1, label, bits, _ = RC.make_region_case(B, spatial, 1, 7, ((1,),))
    r = RC.region_ref(p1, bits, 0.0, 1.0, batch, 1e-5)
    lab2 = (bits & 1).astype(np.uint8)                               # class 1 = the region; stray labels are background
    p2 = np.concatenate([1.0 - p1.astype(np.float64), p1.astype(np.float64)], -1)
    im = imbalance_ref(p2, lab2, (1,), (1.0,), alpha=0.5, beta=0.5, gamma=1.0, eps=1e-5, batch=batch)
    assert abs(r['D'][0] - im['values'][0]) <= 1e-12 and abs(r['dice'] - im['values'][0]) <= 1e-12
    assert np.abs(r['grad'][..., 0] - im['grad'][..., 1]).max() <= 1e-12 * np.abs(im['grad']).max()


def test_bce_term_is_focal_gamma_zero_on_two_channels():
    B, spatial = 2, (9, 7, 5)
    p1, label, bits, _ = RC.make_region_case(B, spatial, 1, 9, ((1,),))
    p1 = RC.late_region_probs(bits, 1, 10, confident=0.6, wrong=0.05)
    r = RC.region_ref(p1, bits, 1.0, 0.0, True, 1e-5)
    lab2 = (bits & 1).astype(np.uint8)
    p2 = np.concatenate([1.0 - p1.astype(np.float64), p1.astype(np.float64)], -1)
    im = imbalance_ref(p2, lab2, w_focal=1.0, gf=0.0)
    assert abs(r['bce'] - im['focal']) <= 1e-14 * max(1.0, abs(im['focal'])) and abs(r['total'] - im['total']) <= 1e-13
    # d/dp of the two-channel form: channel 1 directly, channel 0 through 1 - p
    g2 = im['grad'][..., 1] - im['grad'][..., 0]
    assert np.abs(r['grad'][..., 0] - g2).max() <= 1e-12 * np.abs(g2).max()


def test_labelling_is_nnunets_loop():
    rng = np.random.default_rng(11)
    for R, order in ((3, (1, 2, 3)), (2, (7, 200)), (8, (8, 7, 6, 5, 4, 3, 2, 1))):
        p = (rng.integers(0, 9, (2, R, 4, 5, 3)) / 8.0).astype(np.float32)      # a grid that holds 0.5 exactly
        assert (p == 0.5).any()
        got = RC.labels_ref(p, order, 0.5)
        for b in range(2):                                           # nnU-Net: seg = zeros; for i, c in enumerate(regions_class_order): seg[pred[i] > 0.5] = c
            seg = np.zeros(p.shape[2:], np.uint8)
            for i, c in enumerate(order):
                seg[p[b, i] > 0.5] = c
            assert np.array_equal(got[b], seg)
        assert not got[np.all(p <= 0.5, axis=1)].any()               # 0.5 itself is not painted


def test_orpool_of_one_region_is_maxpool_of_the_binary_label():
    rng = np.random.default_rng(13)
    label = rng.integers(0, 4, (2, 8, 12, 6)).astype(np.uint8)
    binary = (label == 2).astype(np.uint8)
    for kd in (1, 2):
        assert np.array_equal(RC.orpool_ref(RC.bits_ref(label, ((2,),)), kd), RC.maxpool_ref(binary, kd))
    # and for regions that are not nested in label order, pooling the raw label first is a different thing
    bits = RC.bits_ref(label, NON_NESTED)
    assert not np.array_equal(RC.orpool_ref(bits, 1), RC.bits_ref(RC.maxpool_ref(label, 1), NON_NESTED))


def test_lut():
    lut = RC.lut_ref(NON_NESTED)
    assert lut[0] == 0 and lut[1] == 1 and lut[2] == 3 and lut[3] == 2 and lut[4] == 4 and not lut[5:].any()
    from lintransunet_amd import losses as L
    assert L.Regions(NON_NESTED).lut == lut.tobytes()


# ---------------------------------------------------------------------------------------------- the record and the names
@pytest.mark.parametrize('bad', [dict(members=()), dict(members=((1,),) * 9), dict(members=((1,), ())), dict(members=((256,),)),
                                 dict(members=((-1,),)), dict(members=((1,), (2,)), class_order=(1,)),
                                 dict(members=((1,),), class_order=(300,)), dict(members=((1,),), eps=0.0), dict(members=7)])
def test_regions_refusals(bad):
    from lintransunet_amd import losses as L
    with pytest.raises(ValueError):
        L.Regions(**bad)


def test_regions_record():
    from lintransunet_amd import losses as L
    b = L.Regions.brats()
    assert b.members == ((1, 2, 3), (2, 3), (3,)) and b.class_order == (1, 2, 3) and b.batch is True and b.eps == 1e-5
    assert list(b.lut[:5]) == [0, 1, 3, 7, 0] and len(b.lut) == 256
    assert L.Regions([[1, 2], [2]], class_order=[5, 6]) == L.Regions(((1, 2), (2,)), (5, 6))      # equal records compare equal
    assert L.Regions(((1,),) * 8).lut[1] == 255
    with pytest.raises(dataclasses_frozen()):
        b.eps = 1.0


def dataclasses_frozen():
    import dataclasses
    return dataclasses.FrozenInstanceError


def test_level_criterion_refusals_need_no_device():
    from lintransunet_amd import losses as L
    from lintransunet_amd import train
    b = L.Regions.brats()
    crit = L.LevelCriterion({'RegionBCELoss': 1, 'RegionDiceLoss': 0.5}, regions=b)
    assert crit.region == ['RegionBCELoss', 'RegionDiceLoss'] and not crit.base_names
    assert set(L.LevelCriterion.OWNED['region']) == {'RegionBCELoss', 'RegionDiceLoss'}
    assert [row[0] for row in L.LevelCriterion._STAGES][-1] == 'region' and len(L.LevelCriterion._STAGES) == 6
    with pytest.raises(ValueError):
        L.LevelCriterion({'RegionBCELoss': 1})                       # a region name without the record
    with pytest.raises(ValueError):
        L.LevelCriterion({'RegionBCELoss': 1, 'CrossEntroLoss': 1}, regions=b)      # mixed with a class name
    with pytest.raises(ValueError):
        L.LevelCriterion({'RegionDiceLoss': 1, 'TverskyLoss': 1}, regions=b)
    with pytest.raises(ValueError):
        L.LevelCriterion({'RegionDiceLoss': 1}, regions={'members': ((1,),)})
    lab = torch.zeros(1, 1, 4, 4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError):
        crit(torch.zeros(1, 2, 4, 4, 4), lab)                        # 2 channels, 3 regions
    assert isinstance(L.RegionBCELoss(b).impl, L.LevelCriterion) and L.RegionDiceLoss(b).impl.region == ['RegionDiceLoss']
    assert 'RegionBCELoss' not in L.Loss_Dict and 'RegionDiceLoss' not in L.Loss_Dict
    specs = train.level_specs(5, ('RegionBCELoss', 'RegionDiceLoss'), criterion_weight=[1, 1])
    assert len(specs) == 5 and all(s == {'RegionBCELoss': 1, 'RegionDiceLoss': 1} for s in specs)
    assert train.region_specs(specs, 5, b) == specs and train.region_specs(None, 5, b) == specs
    with pytest.raises(ValueError):
        train.region_specs(train.level_specs(5), 5, b)               # a region model with class names
    with pytest.raises(ValueError):
        train.region_specs(specs, 5, None)                           # a class model with region names
    with pytest.raises(ValueError):
        train.region_specs(specs[:4] + [{'RegionBCELoss': 1, 'DiceClassLoss': 1}], 5, b)


def test_chain_refuses_a_second_stage_before_any_launch():
    from lintransunet_amd import ops
    p, bits = torch.zeros(1, 4, 4, 4, 2), torch.zeros(1, 4, 4, 4, dtype=torch.uint8)      # CPU tensors: a launch would raise LtuError
    with pytest.raises(ValueError):
        ops.level_loss_chain(p, bits, base=('ltu_loss', (1.0, 0.0, (0.0,) * 5)), region=(1.0, 1.0, True, 1e-5))
    with pytest.raises(ValueError):
        ops.level_loss_chain(p, bits, topk=(1.0, 0.1, None), region=(1.0, 1.0, True, 1e-5))
    for bad in ((float('nan'), 1.0, True, 1e-5), (1.0, 1.0, True, 0.0), (1.0, float('inf'), False, 1e-5)):
        with pytest.raises(ValueError):
            ops.level_loss_chain(p, bits, region=bad)
    with pytest.raises(ValueError):
        ops.level_loss_chain(torch.zeros(1, 4, 4, 4, 9), bits, region=(1.0, 1.0, True, 1e-5))


def test_signatures_carry_the_keywords():
    from lintransunet_amd import model, train
    for fn in (train.deep_supervision_loss, train.train_step, train.GraphedStep.__init__, model.MaskTransUnet.__init__):
        params = inspect.signature(fn).parameters
        assert params['regions'].default is None and list(params)[-1] == 'regions', fn
    assert list(inspect.signature(model.MaskTransUnet.__init__).parameters)[:10] == [
        'self', 'num_layers', 'roi_size_list', 'is_roi_list', 'dim_input', 'dim_output', 'kernel_size', 'dropout', 'act_dtype', 'regions']
    assert list(inspect.signature(train.train_step).parameters)[:5] == ['model', 'images', 'labels', 'weights', 'step_times']
    assert list(inspect.signature(train.GraphedStep.__init__).parameters)[:6] == ['self', 'model', 'images', 'labels', 'weights', 'reducer']
    from lintransunet_amd import losses as L
    with pytest.raises(ValueError):
        model.MaskTransUnet([8, 8], [4], [False], 1, 2, regions=L.Regions.brats())      # dim_output 2, 3 regions
    with pytest.raises(ValueError):
        model.MaskTransUnet([8, 8], [4], [False], 1, 3, regions=((1,), (2,), (3,)))


def test_region_labels_needs_a_class_order():
    from lintransunet_amd import infer
    from lintransunet_amd import losses as L
    with pytest.raises(ValueError):
        infer.region_labels(torch.zeros(1, 2, 4, 4, 4), L.Regions(((1,), (2,))))


# ---------------------------------------------------------------------------------------------- C-ABI surface
def test_cabi_surface():
    from lintransunet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ltu_hip.h')).read()
    protos = dict(re.findall(r'^(?:int|long long)\s+(ltu_\w+)\s*\(([^;]*)\);', header, flags=re.M | re.S))
    lib = _lib.load()
    for name in NEW:
        assert name in protos and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len([a for a in protos[name].split(',') if a.strip()]) == len(_lib.SIGNATURES[name]), name
    assert _lib.SIGNATURES['ltu_roi_plan_union'] == _lib.SIGNATURES['ltu_roi_plan']
    for kind in ('head', 'final'):
        for d in ('fwd', 'bwd'):
            assert _lib.SIGNATURES[f'ltu_{kind}_sigmoid_{d}'] == _lib.SIGNATURES[f'ltu_{kind}_softmax_{d}']
    ws = lib.ltu_loss_region_ws_floats
    assert ws.restype is _lib.L
    # (1 + blocks) * B * R * 4 floats; 0 for what the calls refuse: R outside 1 .. 8, B * R * 4 > 256
    assert ws(2, 960, 3) == 5 * 2 * 3 * 4 and ws(8, 64 * 64 * 96, 8) == (1 + 128) * 256 and ws(1, 315, 1) == 3 * 4
    assert ws(2, 960, 0) == 0 and ws(2, 960, 9) == 0 and ws(9, 960, 8) == 0 and ws(0, 960, 3) == 0 and ws(2, 0, 3) == 0
    # the shape checks come before any pointer is looked at
    E_SHAPE = -2
    for R in (0, 9):
        assert lib.ltu_loss_region_fwd(0, 0, 0, 0, 0, 0, 0, 1.0, 1.0, 1, 1e-5, 0, 1, 64, R, 0) == E_SHAPE
        assert lib.ltu_loss_region_bwd(0, 0, 0, 0, 0, 0, 0, 1, 64, R, 0) == E_SHAPE
        assert lib.ltu_head_sigmoid_fwd(0, 0, 16, R, 16, 0, 0) == E_SHAPE and lib.ltu_head_sigmoid_bwd(0, 0, 0, 16, R, 16, 0, 0) == E_SHAPE
        assert lib.ltu_final_sigmoid_fwd(0, 0, 1, 2, 2, 2, R, 64, 0, 0) == E_SHAPE
        assert lib.ltu_final_sigmoid_bwd(0, 0, 0, 1, 2, 2, 2, R, 64, 0, 0) == E_SHAPE
        assert lib.ltu_region_labels(0, 0, 0, 0.5, 0, 1, 64, R, 0) == E_SHAPE and lib.ltu_region_prob_bits(0, 0, 0.5, 0, 1, 64, R, 0) == E_SHAPE
        assert lib.ltu_region_counts(0, 0, 0, 0, 1, 64, R, 0) == E_SHAPE
        assert lib.ltu_roi_plan_union(0, 1, 8, 8, 4, R, 4, 0.5, 0, 0, 0, 0, 0) == E_SHAPE
    assert lib.ltu_head_sigmoid_fwd(0, 0, 16, 3, 2, 0, 0) == E_SHAPE and lib.ltu_head_sigmoid_bwd(0, 0, 0, 16, 3, 2, 0, 0) == E_SHAPE      # CP < R
    assert lib.ltu_final_sigmoid_fwd(0, 0, 1, 2, 2, 2, 3, 8, 0, 0) == E_SHAPE and lib.ltu_final_sigmoid_bwd(0, 0, 0, 1, 2, 2, 2, 3, 14, 0, 0) == E_SHAPE
    assert lib.ltu_bits_orpool(0, 0, 1, 7, 8, 4, 1, 0) == E_SHAPE and lib.ltu_bits_orpool(0, 0, 1, 8, 8, 3, 2, 0) == E_SHAPE
    assert lib.ltu_bits_orpool(0, 0, 1, 8, 8, 4, 3, 0) == E_SHAPE
    src = open(os.path.join(ROOT, 'lintransunet_amd', 'csrc', 'region.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    assert 'hipDeviceSynchronize' not in code and 'hipStreamSynchronize' not in code and 'hipMemcpy' not in code and 'hipMalloc' not in code
    # integer atomics only (the counts): every atomic's target is an integer array, and the loss stage has none at all
    atomics = re.findall(r'atomic\w*\s*\(([^,]*),', code)
    assert atomics and all(re.match(r'\s*(&blk\[|counts\b)', a) for a in atomics), atomics
    stage = code[code.index('reg_add'):code.index('region_labels_kernel')]
    assert not re.search(r'atomic\w*\s*\(', stage)
    for helper in ('ls_walk_block', 'ls_store_partial', 'ls_fold', 'ls_walk_grid', 'loss_rows', 'loss_v4', 'loss_bwd_grid', 'LTU_DISPATCH_C'):
        assert helper in code, helper
    mk = open(os.path.join(ROOT, 'lintransunet_amd', 'csrc', 'Makefile')).read()
    assert 'region.hip' in mk
    # the kernels the path tables pin keep their names and template lists; the sigmoid heads are the Sigmoid policy of the head family
    pw = open(os.path.join(ROOT, 'lintransunet_amd', 'csrc', 'pointwise.hip')).read()
    roi = open(os.path.join(ROOT, 'lintransunet_amd', 'csrc', 'roi.hip')).read()
    for text, name in ((pw, 'template <typename A, typename T, int C, bool VEC>\n__global__ void __launch_bounds__(256) head_fwd_kernel('),
                       (pw, 'template <typename A, typename T, int C>\n__global__ void __launch_bounds__(256) final_fwd_kernel('),
                       (pw, 'struct Sigmoid {'), (pw, 'head_fwd<Sigmoid>('), (pw, 'final_bwd<Sigmoid>('),
                       (roi, '__global__ void __launch_bounds__(256) roi_hist_kernel(const float* __restrict__ prob, int H, int W, int D, int C, float thr,'),
                       (roi, 'roi_hist_union_kernel('), (roi, '__global__ void roi_plan_kernel(const RoiArgs a, const int* __restrict__ hist)')):
        assert name in text, name
