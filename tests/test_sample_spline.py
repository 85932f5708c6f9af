"""The cubic patch gather without a GPU: the float64 oracle of tests/sample_spline_common.py against scipy's map_coordinates, its
tolerance constants against what it measures, the `order` arguments, and the entry point's declaration and host-side refusals."""
import os
import re
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data  # noqa: E402
from tests import sample_spline_common as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('size_name', list(sc.SIZES))
def test_oracle_is_map_coordinates_constant_at_order_3(size_name):
    """(3, 3, 3) without clamp: scipy.ndimage.map_coordinates(order=3, mode='constant', cval=fill) on the four matrices, the
    integer one included (an interpolating spline returns the source voxels at integer coordinates)"""
    size = sc.SIZES[size_name]
    v = sc.scan_image().astype(np.float64)
    coef = sc.coefficients(v, (3, 3, 3))
    for name, M in zip(sc.CALLS['mixed'], sc.patch_mats(sc.CALLS['mixed'], size)):
        c = sc.coords(M, size)
        got = sc.tap_sum(coef, c, (3, 3, 3), sc.FILL)
        want = ndimage.map_coordinates(v, c.reshape(3, -1), order=3, mode='constant', cval=sc.FILL, output=np.float64).reshape(size)
        err = np.abs(got - want).max()
        print(f'{size_name} {name}: max |oracle - map_coordinates| {err:.2e}, inside {sc.inside(c).mean():.3f}')
        assert err <= 1e-12, (name, err)
        if not sc.is_cubic(M):
            assert np.abs(sc.source_voxels(v, c) - want).max() <= 1e-12


def test_tolerances_are_the_measured_ones():
    """the constants are what the oracle measures here (rounded down), not something tuned to a kernel"""
    fdev, cdev, ddev, vmax, row = sc.measure_tolerances()
    print(f'float32 oracle {fdev:.3e}, coordinates +-{sc.COORD_BOUND:g}: {cdev:.3e}, deformed: {ddev:.3e}, |value| <= {vmax:.2f}, '
          f'row sum {row:.3f}; TOL {sc.TOL:.3e}, TOL_DEFORMED {sc.TOL_DEFORMED:.3e}')
    assert sc.VALUE_F32_DEV <= fdev <= 1.25 * sc.VALUE_F32_DEV, fdev
    assert sc.COORD_DEV <= cdev <= 1.25 * sc.COORD_DEV, cdev
    assert sc.COORD_DEV_DEFORMED <= ddev <= 1.25 * sc.COORD_DEV_DEFORMED, ddev
    assert sc.TOL == 4 * sc.VALUE_F32_DEV + sc.COORD_DEV and sc.TOL_DEFORMED == 4 * sc.VALUE_F32_DEV + sc.COORD_DEV_DEFORMED
    assert sc.TOL_DEFORMED <= 1e-3                      # what the trilinear gathers are held to; a wrong tap is 1e-2 or more
    assert vmax == sc.CLAMP[1]                          # the clamp shows


def test_the_patches_reach_what_they_are_there_for():
    size = sc.SIZES['vec']
    mats = dict(zip(sc.CALLS['mixed'], sc.patch_mats(sc.CALLS['mixed'], size)))
    c = sc.coords(mats['oblique'], size)
    assert 0.67 <= sc.inside(c).mean() <= 0.69           # 68 % inside the scan
    assert sc.edge_band(c).sum() == 1                    # 1 voxel of 6912 within 1e-3 of an edge
    assert not sc.is_cubic(mats['integer']) and all(sc.is_cubic(mats[n]) for n in ('oblique', 'inplane', 'zoom'))
    zdec = sc.patch_mats(sc.CALLS['zdec'], size)
    assert (zdec[:, [0, 1, 2, 2], [2, 2, 0, 1]] == 0).all() and not (mats['oblique'][[0, 1, 2, 2], [2, 2, 0, 1]] == 0).all()
    assert len(np.unique(sc.scan_label())) == 3


def test_order_arguments():
    assert data.sample_order(1) == (1, 1, 1) and data.sample_order(3) == (3, 3, 3)
    assert data.sample_order([3, 3, 1]) == (3, 3, 1) and data.sample_order((3, 3, 3)) == (3, 3, 3)
    for bad in (2, 0, 4, 5, (1, 3, 3), (3, 1, 3), (3, 3, 0), (3, 3), (3, 3, 3, 3), (3.5, 3, 3), 'cubic', None, True):
        with pytest.raises(ValueError, match=r'order 1, 3, \(3, 3, 3\) and \(3, 3, 1\)'):
            data.sample_order(bad)
    with pytest.raises(ValueError):
        data.Augmentation(order=2)
    assert data.Augmentation().order == (1, 1, 1) and data.Augmentation(order=(3, 3, 1)).order == (3, 3, 1)
    v = torch.zeros((4, 5, 6))
    with pytest.raises(ValueError):                       # the order is refused before anything else is looked at
        data.sample_affine(v, None, np.eye(4)[None, :3], (2, 2, 2), order=(1, 3, 3))
    with pytest.raises(_lib.LtuError):                    # and a CPU tensor after it: no fallback
        data.sample_affine(v, None, np.eye(4)[None, :3], (2, 2, 2), order=3)


def test_order_makes_no_draw():
    draws, states = [], []
    for order in (1, 3, (3, 3, 1)):
        rs = np.random.RandomState(21)
        aug = data.Augmentation(order=order, elastic_prob=0.5)
        draws.append([aug.draw(rs) for _ in range(3)])
        states.append(rs.get_state())
    for d, st in zip(draws[1:], states[1:]):
        for a, b in zip(d, draws[0]):
            assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
        assert st[0] == states[0][0] and np.array_equal(st[1], states[0][1]) and st[2:] == states[0][2:]


def test_entry_point_is_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'ltu_hip.h')).read()
    lib = _lib.load()
    decl = re.search(r'^int\s+ltu_sample_spline\s*\(([^;]*)\);', header, flags=re.M)
    assert decl, 'ltu_sample_spline is not declared'
    assert 'ltu_sample_spline' in _lib.SIGNATURES and hasattr(lib, 'ltu_sample_spline')
    assert len(_lib.SIGNATURES['ltu_sample_spline']) == decl.group(1).count(',') + 1 == 26
    # refused before any launch and before any pointer is followed, so it can be asked without a GPU
    f = lib.ltu_sample_spline
    one = torch.zeros(64)
    lab = torch.zeros(64, dtype=torch.uint8)
    m = np.ascontiguousarray(np.eye(4)[:3].reshape(1, 12))
    fill, lo, hi = (np.array([v], dtype=np.float32) for v in (0.0, -1.0, 1.0))
    cubic = np.ones(1, dtype=np.uint8)

    def call(coef=one.data_ptr(), lo=lo, hi=hi, cubic=cubic.ctypes.data, order_d=3, K=1, n=1, mats=m.ctypes.data):
        return f(one.data_ptr(), coef, lab.data_ptr(), one.data_ptr(), lab.data_ptr(), mats, 0, 0, 0, 0, 0, 0, fill.ctypes.data,
                 lo.ctypes.data, hi.ctypes.data, cubic, n, K, 4, 4, 4, 2, 2, 2, order_d, None)

    assert call(coef=0) == -4 and call(cubic=0) == -4 and call(order_d=2) == -4 and call(order_d=0) == -4
    assert call(lo=hi, hi=lo) == -4 and call(lo=np.array([np.nan], dtype=np.float32)) == -4
    assert call(K=0) == -2 and call(K=5) == -2
    assert call(mats=0) == -4 and call(n=_lib.SAMPLE_AFFINE_MAX + 1) == -4          # what ltu_sample_channels refuses, with its codes
