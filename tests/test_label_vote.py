"""The label vote without a device: the float64 oracle of tests/label_vote_common.py against scipy's interpolated one-hot maps, the
exact cases, the ball measurement, the two entry points in header, binding and library, and the host-side arguments
(label_order in data.resample / sample_affine / Augmentation / SpacedScan, order in data.to_native)."""
import os
import re
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data  # noqa: E402
from tests import label_vote_common as lv  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ltu_resample_vote', 'ltu_sample_vote')


def test_oracle_is_the_argmax_of_scipys_linear_one_hot_maps():
    lab = lv.blob_label()
    M = lv.patch_mats(('oblique',), lv.SIZES['vec'])[0]
    c = lv.patch_coords(M, lv.SIZES['vec'])
    voted, margin, _ = lv.vote(lab, c, 'zero')
    values = np.unique(lab)
    maps = np.stack([ndimage.map_coordinates((lab == v).astype(np.float64), c, order=1, mode='constant', cval=0.0) for v in values])
    top = (np.array(lab.shape, dtype=np.float64) - 1).reshape(3, 1, 1, 1)
    away = ((c >= 0) & (c <= top)).all(0) & (margin > 1e-9)             # inside the scan, and not a tie scipy's rounding may turn
    assert away.mean() > 0.4
    assert np.array_equal(values[np.argmax(maps, 0)][away], voted[away])
    # the scores themselves: the margin is the gap between scipy's two best maps
    srt = np.sort(maps, 0)
    assert np.abs((srt[-1] - srt[-2]) - margin)[away].max() < 1e-12


@pytest.mark.parametrize('outside', ['zero', 'clamp'])
def test_an_integer_matrix_gives_the_nearest_labels(outside):
    lab = lv.blob_label()
    size = (16, 16, 8)
    M = data.patch_matrix((5, -2, 3), size, True, 1)                     # crop + flip + rot90, partly outside the scan
    assert np.array_equal(M, np.round(M))
    voted, margin, nearest = lv.vote(lab, lv.patch_coords(M, size), outside)
    assert np.array_equal(voted, nearest) and len(np.unique(voted)) == 4
    assert (margin == 1.0).all()


def test_the_smallest_value_wins_a_tie():
    lab = np.zeros((2, 2, 2), dtype=np.uint8)
    lab[1] = 7
    lab[0, 1] = 200                                                      # scores at the centre: 0 -> 0.25, 7 -> 0.5, 200 -> 0.25
    c = np.array([0.5, 0.5, 0.5]).reshape(3, 1, 1, 1)
    assert lv.vote(lab, c, 'clamp')[0].item() == 7
    lab[1, 0] = 3                                                        # 0, 3, 7, 200 at 0.25 each: the smallest
    voted, margin, _ = lv.vote(lab, c, 'clamp')
    assert voted.item() == 0 and margin.item() == 0.0
    lab[0, 0] = 9                                                        # 3, 7, 9, 200
    assert lv.vote(lab, c, 'clamp')[0].item() == 3
    # a tap outside the scan counts for label 0 under 'zero' and is the clamped voxel under 'clamp'
    c = np.array([-0.75, 0.0, 0.0]).reshape(3, 1, 1, 1)
    assert lv.vote(lab, c, 'zero')[0].item() == 0 and lv.vote(lab, c, 'clamp')[0].item() == 9


def test_ball_vote_is_closer_to_the_directly_rasterised_ball():
    coarse, fine, c = lv.ball()
    voted, margin, nearest = lv.vote(coarse, c, 'clamp')
    assert not (margin < lv.BAND).any()                                  # no voxel inside the tie band
    by_vote, by_nearest = int((voted != fine).sum()), int((nearest != fine).sum())
    print(f'ball 16^3 -> 37^3: {by_vote} voxels differ from the direct ball by vote, {by_nearest} nearest')
    assert (by_vote, by_nearest) == (671, 1177)
    assert by_vote < by_nearest


def test_the_inputs_stay_inside_both_caps():
    """the conditions of the device cases, checked on the oracle alone: little skipped, enough changed against nearest"""
    refs = [(f'{c} {s} {g}', r[1:]) for s in lv.SIZES for c in lv.CALLS for g in (None,) + lv.LATTICES[s] for r in lv.gather_reference(c, s, g)]
    refs += [(f'{v} {O}', lv.resample_reference(v, O)) for v in ((0, 1), tuple(range(5)), tuple(range(8)), lv.ANY_VALUES) for O in lv.RS_OUTPUTS]
    for what, (voted, keep, nearest) in refs:
        assert 1.0 - keep.mean() <= lv.MAX_SKIP, what
        assert (voted != nearest).mean() >= lv.MIN_DIFF, what
    assert 2.5e-4 < lv.band_elastic(lv.patch_mats(('oblique',), lv.SIZES['vec'])[0]) < 4e-4


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'ltu_hip.h')).read()
    protos = dict(re.findall(r'^int\s+(ltu_\w+)\s*\(([^;]*)\);', header, flags=re.M | re.S))
    lib = _lib.load()
    for name in NEW:
        assert name in protos, name
        assert name in _lib.SIGNATURES, name
        assert len(protos[name].split(',')) == len(_lib.SIGNATURES[name]), name
        assert hasattr(lib, name), name


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """fake pointers: every refusal comes before a launch, so nothing is dereferenced"""
    lib = _lib.load()
    p = 0x1000
    S, ss, O, os_ = (4, 4, 4), (1, 4, 16), (4, 4, 4), (16, 4, 1)
    assert lib.ltu_resample_vote(0, *S, *ss, p, *O, *os_, p, 0, None) == -4
    assert lib.ltu_resample_vote(p, *S, *ss, 0, *O, *os_, p, 0, None) == -4
    assert lib.ltu_resample_vote(p, *S, *ss, p, *O, *os_, 0, 0, None) == -4
    assert lib.ltu_resample_vote(p, *S, *ss, p, *O, *os_, p, 3, None) == -4
    assert lib.ltu_resample_vote(p, 0, 4, 4, *ss, p, *O, *os_, p, 0, None) == -2
    assert lib.ltu_resample_vote(p, *S, *ss, p, *O, 0, 4, 1, p, 0, None) == -2
    m = np.zeros(12)
    assert lib.ltu_sample_vote(0, p, m.ctypes.data, 0, 0, 0, 0, 1, 8, 8, 8, 4, 4, 4, None) == -4
    assert lib.ltu_sample_vote(p, 0, m.ctypes.data, 0, 0, 0, 0, 1, 8, 8, 8, 4, 4, 4, None) == -4
    assert lib.ltu_sample_vote(p, p, 0, 0, 0, 0, 0, 1, 8, 8, 8, 4, 4, 4, None) == -4
    assert lib.ltu_sample_vote(p, p, m.ctypes.data, 0, 0, 0, 0, _lib.SAMPLE_AFFINE_MAX + 1, 8, 8, 8, 4, 4, 4, None) == -4
    assert lib.ltu_sample_vote(p, p, m.ctypes.data, 0, 0, 0, 0, 0, 8, 8, 8, 4, 4, 4, None) == 0        # n == 0: nothing to do
    assert lib.ltu_sample_vote(p, p, m.ctypes.data, 0, 0, 0, 0, 1, 0, 8, 8, 4, 4, 4, None) == -2
    assert lib.ltu_sample_vote(p, p, m.ctypes.data, p, 3, 4, 4, 1, 8, 8, 8, 4, 4, 4, None) == -2       # a lattice extent below 4
    assert lib.ltu_sample_vote(p, p + 1, m.ctypes.data, 0, 0, 0, 0, 1, 8, 8, 8, 4, 4, 4, None) == -3   # d % 4 == 0: 4-byte stores
    m[5] = np.nan
    assert lib.ltu_sample_vote(p, p, m.ctypes.data, 0, 0, 0, 0, 1, 8, 8, 8, 4, 4, 4, None) == -4


class _Scan:
    shape, native_shape, matrix = (4, 4, 4), (4, 4, 4), np.eye(4)[:3]


@pytest.mark.parametrize('bad', [2, -1, 3, 1.0, True, None, 'vote'])
def test_label_order_outside_0_and_1_is_a_value_error(bad, tmp_path):
    lab = torch.zeros((4, 4, 4), dtype=torch.uint8)
    with pytest.raises(ValueError):
        data.resample(None, lab, np.eye(4)[:3], (4, 4, 4), label_order=bad)
    with pytest.raises(ValueError):
        data.sample_affine(None, lab, np.eye(4)[:3][None], (2, 2, 2), label_order=bad)
    with pytest.raises(ValueError):
        data.Augmentation(label_order=bad)
    with pytest.raises(ValueError):
        data.SpacedScan(str(tmp_path / 'missing.nii'), str(tmp_path / 'missing_lab.nii'), device='cpu', label_order=bad)
    with pytest.raises(ValueError):
        data.MultiScan([str(tmp_path / 'missing.nii')], str(tmp_path / 'missing_lab.nii'), device='cpu', label_order=bad)
    with pytest.raises(ValueError):
        data.to_native(lab, _Scan(), order=bad)


def test_label_order_makes_no_draw_and_keeps_the_defaults():
    a, b = np.random.RandomState(4), np.random.RandomState(4)
    kw = dict(elastic_prob=0.5, contrast_prob=0.2, lowres_prob=0.2, invgamma_prob=0.2)
    for _ in range(3):
        pa, pb = data.Augmentation(label_order=1, **kw).draw(a), data.Augmentation(label_order=0, **kw).draw(b)
        assert pa.keys() == pb.keys()
        assert all(np.array_equal(pa[k], pb[k]) for k in pa)
    sa, sb = a.get_state(), b.get_state()
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
    assert data.Augmentation().label_order == 0 and data.Augmentation(label_order=1).label_order == 1
    assert data.Augmentation.nnunet().label_order == 0 and data.Augmentation.nnunet(label_order=1).label_order == 1
    assert 'order 1' in data.Augmentation.nnunet.__doc__
