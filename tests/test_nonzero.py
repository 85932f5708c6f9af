"""Host side of the nonzero crop: geometry.crop_plan, the numpy / scipy oracle the device tests compare against, the C-ABI surface
and the refusals that are made before a file is read or the GPU touched.  The kernels are judged in tests/test_gpu_nonzero.py."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data, geometry, infer  # noqa: E402
import nonzero_common as nc  # noqa: E402

# a flipped, anisotropic file affine with a permuted axis: x runs to the left at 0.9 mm, y up at 1.1 mm, z forward at 2.5 mm
AFFINE = np.array([[-0.9, 0.0, 0.0, 100.0], [0.0, 0.0, 2.5, -50.0], [0.0, 1.1, 0.0, 7.0], [0.0, 0.0, 0.0, 1.0]])


def test_crop_plan_against_a_hand_computed_affine():
    shape, affine = geometry.crop_plan((10, 12, 8), AFFINE, ((2, 9), (0, 12), (3, 5)))
    assert shape == (7, 12, 2)
    # the crop's voxel (0, 0, 0) is the file's (2, 0, 3): world = (-0.9 * 2 + 100, 2.5 * 3 - 50, 1.1 * 0 + 7)
    want = AFFINE.copy()
    want[:3, 3] = [98.2, -42.5, 7.0]
    assert np.allclose(affine, want, rtol=0, atol=1e-12) and affine.dtype == np.float64
    assert np.array_equal(affine[:3, :3], AFFINE[:3, :3])
    for v in ((0, 0, 0), (6, 11, 1), (3, 5, 1)):      # both affines put a voxel of the crop at the same place
        a = affine @ np.array([*v, 1.0])
        b = AFFINE @ np.array([v[0] + 2, v[1], v[2] + 3, 1.0])
        assert np.allclose(a, b, rtol=0, atol=1e-12)


def test_crop_plan_full_box_returns_the_inputs():
    shape, affine = geometry.crop_plan((10, 12, 8), AFFINE, ((0, 10), (0, 12), (0, 8)))
    assert shape == (10, 12, 8) and np.array_equal(affine, AFFINE)


@pytest.mark.parametrize('box', [((0, 11), (0, 12), (0, 8)), ((3, 3), (0, 12), (0, 8)), ((-1, 4), (0, 12), (0, 8)), ((0, 10), (0, 12))])
def test_crop_plan_refuses_a_box_outside_the_volume(box):
    with pytest.raises(ValueError, match='box'):
        geometry.crop_plan((10, 12, 8), AFFINE, box)


def test_crop_plan_then_spacing_plan_samples_the_same_world_points():
    """the pull matrix of the box leads to box voxels: shifted by the box's corner it leads to file voxels of the same world point"""
    box = ((2, 9), (1, 12), (3, 8))
    bshape, baffine = geometry.crop_plan((10, 12, 8), AFFINE, box)
    matrix, shape, out_affine = geometry.spacing_plan(bshape, baffine, (1.0, 1.0, 2.0), 'RAS')
    for v in ((0, 0, 0), (shape[0] - 1, shape[1] - 1, shape[2] - 1)):
        world = out_affine @ np.array([*v, 1.0])
        src = matrix @ np.array([*v, 1.0]) + np.array([lo for lo, _ in box])
        assert np.allclose(AFFINE @ np.array([*src, 1.0]), world, rtol=0, atol=1e-9)


def test_the_oracle_on_the_phantom():
    """crop, then fill, then the masked z-score: each step against scipy / numpy directly"""
    vols, lab = nc.head_phantom((24, 30, 36))
    scalings = [(2.0, 0.0), (0.5, 0.0)]
    o = nc.oracle(vols, scalings)
    raw = (vols[0] != 0) | (vols[1] != 0)
    assert np.array_equal(nc.union_nonzero(vols, scalings), raw)
    filled = ndimage.binary_fill_holes(raw)
    assert np.array_equal(o['mask'], filled) and filled.sum() > raw.sum()              # the cavity and the sprinkled zeros are holes
    zs, ys, xs = np.nonzero(filled)
    assert o['box'] == ((zs.min(), zs.max() + 1), (ys.min(), ys.max() + 1), (xs.min(), xs.max() + 1)) and o['count'] == filled.sum()
    assert 0.1 < o['count'] / filled.size < 0.2                                         # about 85 % exact zeros
    sl = nc.box_slices(o['box'])
    assert not lab[~filled].any() and lab[sl].any()                                     # the label lies inside the box
    for c, (v, (slope, inter)) in enumerate(zip(vols, scalings)):
        y = v.astype(np.float64) * slope + inter
        assert o['means'][c] == np.mean(y[filled]) and o['stds'][c] == np.std(y[filled])
        z = o['z'][c]
        assert z.shape == tuple(hi - lo for lo, hi in o['box'])
        inside = z[filled[sl]]
        assert abs(inside.mean()) <= 1e-12 and abs(inside.std() - 1.0) <= 1e-12 and not z[~filled[sl]].any()
    # the mean over ALL voxels, which 'zscore' takes, is dragged towards zero: the reason for 'zscore_nonzero'
    assert vols[1].astype(np.float64).mean() < 0.25 * o['means'][1]


@pytest.mark.parametrize('shape', nc.SHAPES[1:3])
def test_hole_cases_mean_what_their_names_say(shape):
    cases = nc.hole_cases(shape)
    for conn in (1, 2, 3):
        assert nc.fill(cases['shell'], conn).sum() > cases['shell'].sum()
        assert np.array_equal(nc.fill(cases['shell_channel'], conn), cases['shell_channel'])          # open: nothing is filled
        inner = np.zeros(shape, bool)
        inner[1:-1, 1:-1, 1:-1] = True
        assert np.array_equal(nc.fill(cases['nested'], conn), inner)
        assert np.array_equal(nc.fill(cases['empty'], conn), cases['empty']) and nc.fill(cases['full'], conn).all()
    for name, open_from in (('edge_link', 2), ('corner_link', 3), ('face_ends', 3)):
        for conn in (1, 2, 3):
            grew = nc.fill(cases[name], conn).sum() > cases[name].sum()
            assert grew == (conn < open_from), (name, conn)


def test_abi_symbols_resolve():
    want = {'ltu_nonzero_mask': 8, 'ltu_mask_box': 8, 'ltu_normalize_masked': 16, 'ltu_fill_holes_ws_elems': 4, 'ltu_fill_holes': 10}
    lib = _lib.load()
    for name, nargs in want.items():
        assert len(_lib.SIGNATURES[name]) == nargs and hasattr(lib, name), name
    assert lib.ltu_fill_holes_ws_elems(2, 5, 4, 3) == 2 * 60
    assert lib.ltu_fill_holes_ws_elems(1, 2048, 1024, 1024) == 0 and lib.ltu_fill_holes_ws_elems(0, 4, 4, 4) == 0


def test_abi_refusals_launch_nothing():
    """every contract error is returned before a launch: the pointers are fakes that no kernel may touch"""
    fake = 0x1000
    with pytest.raises(_lib.LtuError, match='LTU_E_SHAPE'):                           # S = 2^31
        _lib.call('ltu_fill_holes', fake, fake, fake, 1 << 40, 1, 2048, 1024, 1024, 1, 0)
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):                             # a short scratch
        _lib.call('ltu_fill_holes', fake, fake, fake, 2 * 60 - 1, 2, 5, 4, 3, 1, 0)
    for conn in (0, 4):
        with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):
            _lib.call('ltu_fill_holes', fake, fake, fake, 120, 2, 5, 4, 3, conn, 0)
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):
        _lib.call('ltu_fill_holes', 0, fake, fake, 120, 2, 5, 4, 3, 1, 0)
    with pytest.raises(_lib.LtuError, match='LTU_E_DTYPE'):
        _lib.call('ltu_nonzero_mask', fake, 1, 100, 1.0, 0.0, fake, 0, 0)             # bf16 is no stored dtype
    with pytest.raises(_lib.LtuError, match='LTU_E_SHAPE'):
        _lib.call('ltu_nonzero_mask', fake, 0, 0, 1.0, 0.0, fake, 0, 0)
    with pytest.raises(_lib.LtuError, match='LTU_E_ALIGN'):
        _lib.call('ltu_nonzero_mask', fake + 2, 0, 100, 1.0, 0.0, fake, 0, 0)         # an f32 image at an odd half-word
    with pytest.raises(_lib.LtuError, match='LTU_E_SHAPE'):
        _lib.call('ltu_mask_box', fake, 1, 2048, 1024, 1024, fake, fake, 0)
    with pytest.raises(_lib.LtuError, match='LTU_E_ALIGN'):
        _lib.call('ltu_mask_box', fake, 1, 4, 4, 4, fake, fake + 4, 0)
    for lo, size in (((0, 0, 3), (8, 6, 3)), ((-1, 0, 0), (2, 2, 2)), ((0, 0, 0), (9, 6, 5)), ((1, 1, 1), (0, 1, 1))):
        with pytest.raises(_lib.LtuError, match='LTU_E_SHAPE'):                       # the box leaves the 8 x 6 x 5 volume, or is empty
            _lib.call('ltu_normalize_masked', fake, 0, fake, 8, 6, 5, *lo, *size, 1.0, 0.0, fake, 0)
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):
        _lib.call('ltu_normalize_masked', fake, 0, 0, 8, 6, 5, 0, 0, 0, 8, 6, 5, 1.0, 0.0, fake, 0)


def test_refusals_before_any_gpu_call(tmp_path):
    """a misspelt option is refused before the file is read (the path does not exist) and before the device is touched"""
    missing = str(tmp_path / 'no_such_scan.nii')
    with pytest.raises(ValueError, match="crop is None or 'nonzero'"):
        data.SpacedScan(missing, crop='brain')
    with pytest.raises(ValueError, match='zscore_brain'):
        data.SpacedScan(missing, intensity='zscore_brain')
    with pytest.raises(ValueError, match="crop is None or 'nonzero'"):
        data.MultiScan([missing, missing], crop='brain')
    with pytest.raises(ValueError, match='zscore_brain'):
        data.MultiScan([missing, missing], intensity=['zscore_nonzero', 'zscore_brain'])
    with pytest.raises(_lib.LtuError, match='connectivity'):
        infer.fill_holes(torch.zeros((1, 4, 4, 4), dtype=torch.uint8), connectivity=4)
    with pytest.raises(_lib.LtuError, match='GPU only'):
        infer.fill_holes(torch.zeros((1, 4, 4, 4), dtype=torch.uint8))
    with pytest.raises(_lib.LtuError, match='GPU only'):
        data.nonzero_mask(torch.zeros((4, 4, 4), dtype=torch.int16))


def test_scan_fill_prefers_the_scans_outside_value():
    """data.sample(augment=) fills beyond the scan with scan.outside where the scan names one, else with the window's floor"""
    class Scan:
        pass
    window = (-3.0, 5.0, -1.5, 2.5)
    one, multi = Scan(), Scan()
    one.img, one.intensity = torch.zeros((4, 4, 4)), window
    multi.img, multi.intensity = torch.zeros((2, 4, 4, 4)), [window, window]
    aug = data.Augmentation()
    assert data._scan_fill(one, aug) == -1.5 and data._scan_fill(multi, aug) == [-1.5, -1.5]          # no `outside`: as before
    one.outside, multi.outside = None, [None, 0.0]
    assert data._scan_fill(one, aug) == -1.5 and data._scan_fill(multi, aug) == [-1.5, 0.0]
    one.outside = 0.0
    assert data._scan_fill(one, aug) == 0.0
    assert data._scan_fill(one, data.Augmentation(fill=7.0)) == 7.0 and data._scan_fill(one, None) == 0.0
