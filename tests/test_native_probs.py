"""The arg-max on the scan's own grid without a device (csrc/resample.hip ltu_resample_argmax, data.to_native_probs,
infer.segment_scan): the conditions the GPU test's comparison rests on (few near-ties in the inputs, the kernel's fp32 arithmetic
within 2e-6 of float64 and its arg-max stable outside the near-ties), the C-ABI refusals and the host-side validation."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import data, infer  # noqa: E402
from tests import native_probs_common as nc  # noqa: E402

GRID = [(case, C, kind) for case in nc.CASE_NAMES for C, kind in nc.INPUTS]


def test_case_table():
    """every case has two output axes above the 64-wide tile that are no multiple of it and a third of at least 2; the general case
    clamps about a tenth of its output, on both ends"""
    for name, cfg in nc.cases().items():
        big = [n for n in cfg['O'] if n > 64 and n % 64]
        assert len(big) == 2 and min(cfg['O']) >= 2, (name, cfg['O'])
    g = nc.cases()['general']
    assert 0.08 <= nc.outside_share(g['M'], g['O'], g['S']) <= 0.15
    c = nc.coords(g['M'], g['O'])
    assert (c[0] < 0).any() and (c[0] > g['S'][0] - 1).any() and (c[2] < 0).any() and (c[2] > g['S'][2] - 1).any()
    # the two plan cases pull one RAS grid: lanes along file z, which is the slowest axis of 'msd' and the fastest of 'slices_first'
    from lintransunet_amd import geometry
    for name, want in (('msd', 2), ('slices_first', 0)):
        cfg = nc.cases()[name]
        assert geometry.lane_axis(cfg['M'], nc.src_strides(cfg['S'])) == want


@pytest.mark.parametrize('case,C,kind', GRID)
def test_near_tie_share(case, C, kind):
    """a condition on the inputs: the voxels the GPU test leaves out of the label comparison are at most 1e-3 of the output"""
    _, _, _, mg = nc.reference(case, C, kind)
    share = float((mg < nc.MARGIN).mean())
    print(f'{case} C={C} {kind}: near-tie share {share:.3g}')
    assert share <= nc.NEAR_TIE_CAP, share


@pytest.mark.parametrize('case,C,kind', GRID)
def test_fp32_emulation(case, C, kind):
    """weights and running sum in float32, taps 0 .. 7: within 2e-6 of float64, and the same arg-max wherever the margin is >= 4e-6"""
    cfg = nc.cases()[case]
    P, want, lab, mg = nc.reference(case, C, kind)
    got = nc.sample32(P.numpy(), cfg['M'], cfg['O'])
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f'{case} C={C} {kind}: fp32 emulation max error {err:.3g}')
    assert err <= nc.VALUE_TOL, err
    assert np.array_equal(nc.argmax_first(got)[mg >= nc.MARGIN], lab[mg >= nc.MARGIN])


def test_oracle_is_grid_sample():
    """the float64 oracle against torch's float64 grid_sample (align_corners False in voxel units, border padding)"""
    import torch.nn.functional as F
    cfg = nc.cases()['general']
    P, want, _, _ = nc.reference('general', 3, 'random')
    c = nc.coords(cfg['M'], cfg['O'])
    S = cfg['S']
    g = np.stack([(2 * c[s] + 1) / S[s] - 1 for s in (2, 1, 0)], -1)          # grid_sample's (x, y, z) = the reversed axes
    ref = F.grid_sample(P.to(torch.float64)[None], torch.as_tensor(g)[None], mode='bilinear', padding_mode='border',
                        align_corners=False)[0].numpy()
    assert np.abs(ref - want).max() <= 1e-12


def test_cabi_refusals_without_launch():
    """NULL pointers, a class count outside 2 .. 8, a mask beyond the classes or without its output, empty extents, bad strides and a
    bad lane axis are refused before anything is launched"""
    from lintransunet_amd import _lib
    lib = _lib.load()
    fake = 1 << 20                                                                # never dereferenced: every call below is refused
    #      0     1  2    3  4  5  6   7  8  9     10    11 12   13 14 15 16 17 18  19    20 21
    ok = [fake, 3, 512, 8, 8, 8, 64, 8, 1, fake, fake, 5, 512, 8, 8, 8, 1, 8, 64, fake, 2, None]
    f = lib.ltu_resample_argmax

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return a
    for i in (0, 9, 19):                                                          # probs, out_lab, mat
        assert f(*with_(i, None)) == -4
    for C in (1, 9, 0, -3):
        assert f(*with_(1, C)) == -2
    assert f(*with_(11, 8)) == -4                                                 # class 3 of C = 3
    assert f(*with_(11, -1)) == -4
    assert f(*with_(10, None)) == -4                                              # a mask without out_prob
    for i in (3, 4, 5, 13, 14, 15, 2, 6, 7, 8, 12, 16, 17, 18):                   # extents, then strides
        assert f(*with_(i, 0)) == -2, i
        assert f(*with_(i, -1)) == -2, i
    for lane in (-1, 3):
        assert f(*with_(20, lane)) == -4


class _Scan:
    shape, native_shape = (6, 5, 4), (3, 4, 5)
    matrix = np.eye(4)[:3]


def test_host_side_validation():
    with pytest.raises(ValueError):
        data.to_native_probs(torch.zeros((3, 6, 5, 5)), _Scan())                 # spatial shape
    with pytest.raises(ValueError):
        data.to_native_probs(torch.zeros((2, 3, 6, 5, 4)), _Scan())              # a batch of two
    with pytest.raises(ValueError):
        data.to_native_probs(torch.zeros((3, 6, 5, 4), dtype=torch.float64), _Scan())
    with pytest.raises(ValueError):
        data.to_native_probs(torch.zeros((1, 3, 6, 5, 4), dtype=torch.float16), _Scan())
    with pytest.raises(ValueError):
        infer.segment_scan([], _Scan())
    with pytest.raises(ValueError):
        infer.segment_scan((), _Scan())
