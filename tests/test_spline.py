"""Host side of the cubic B-spline resampling path: the float64 oracle against scipy's own interpolation, nnU-Net's order rule,
the argument checks that need no GPU, and the C-ABI surface of the two entry points."""
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

from lintransunet_amd import _lib, data, geometry
from tests import spline_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _matrix_for(S, O, seed):
    """a scaled, sheared pull matrix that sends part of the output outside the source"""
    rs = np.random.RandomState(seed)
    m = np.zeros((3, 4))
    m[:, :3] = np.diag([(S[a] + 1.5) / O[a] for a in range(3)]) + 0.03 * rs.standard_normal((3, 3))
    m[:, 3] = -0.8
    return m


@pytest.mark.parametrize('S', sc.MAP_COORDINATES_SHAPES)
def test_oracle_is_map_coordinates_at_order_3(S):
    v = np.random.RandomState(5).standard_normal(S)
    O = tuple(max(2, int(1.3 * n) + 1) for n in S)
    M = _matrix_for(S, O, 6)
    got = sc.resample64(v, M, O, (3, 3, 3))
    u = np.stack(sc.clamped(sc.coords(M, O), S))
    want = ndimage.map_coordinates(v, u.reshape(3, -1), order=3, mode='mirror', output=np.float64).reshape(O)
    assert np.abs(got - want).max() <= 4e-15 * max(1.0, np.abs(want).max())
    # at integer coordinates the spline interpolates: the data come back
    eye = np.eye(4)[:3]
    assert np.abs(sc.resample64(v, eye, S, (3, 3, 3)) - v).max() <= 6e-15 * max(1.0, np.abs(v).max())


def test_oracle_lower_orders():
    """order 0 is the nearest voxel along that axis, order 1 linear: checked where they have a closed form"""
    S = (7, 6, 5)
    v = np.random.RandomState(8).standard_normal(S)
    shift = np.eye(4)[:3].copy()
    shift[2, 3] = 0.4                                   # 0.4 voxels along axis 2
    near = sc.resample64(v, shift, S, (3, 3, 0))
    assert np.abs(near - v).max() <= 6e-15 * np.abs(v).max()      # floor(k + 0.4 + 0.5) = k, axes 0 and 1 at integers
    shift0 = np.eye(4)[:3].copy()
    shift0[0, 3] = 0.25
    lin = sc.resample64(v, shift0, S, (1, 3, 3))
    nxt = np.concatenate([v[1:], v[-1:]], 0)
    assert np.abs(lin - (0.75 * v + 0.25 * nxt)).max() <= 1e-14
    assert sc.mirror(np.array([-1, 0, 4, 5, 6]), 5).tolist() == [1, 0, 4, 3, 2]
    assert sc.mirror(np.array([-1, 2, 3]), 2).tolist() == [1, 0, 1] and sc.mirror(np.array([-1, 2]), 1).tolist() == [0, 0]


def test_tolerances_are_the_measured_ones():
    """the constants of spline_common are what its float32 oracle measures here (rounded down), not something tuned to a kernel"""
    cdev, cmax, vdev, vmax = sc.measure_tolerances()
    assert sc.COEF_F32_DEV <= cdev <= 1.25 * sc.COEF_F32_DEV, cdev
    assert sc.VALUE_F32_DEV <= vdev <= 1.25 * sc.VALUE_F32_DEV, vdev
    assert sc.COEF_TOL == 4 * sc.COEF_F32_DEV and sc.VALUE_TOL == 4 * sc.VALUE_F32_DEV
    assert cmax > 10 and vmax > 3                       # a wrong tap is an error of order 1e-2 or more on such values
    share = sc.outside_share(sc.gather_cases()['oblique']['M'], sc.gather_cases()['oblique']['O'], sc.gather_cases()['oblique']['S'])
    assert 0.18 <= share <= 0.22, share


def test_resample_orders():
    ro = geometry.resample_orders
    assert ro((1.0, 1.0, 1.0), (1.0, 1.0, 1.0)) == (3, 3, 3)
    assert ro((0.7, 0.7, 2.5), (0.5, 0.5, 2.0)) == (3, 3, 0)
    assert ro((2.5, 0.7, 0.7), (2.0, 0.5, 0.5)) == (0, 3, 3)
    assert ro((0.7, 2.5, 2.5), (1.0, 1.0, 1.0)) == (3, 3, 3)          # two coarse axes: no single axis to separate
    assert ro((1.0, 1.0, 2.9), (1.0, 1.0, 2.9)) == (3, 3, 3)          # below the threshold
    assert ro((1.0, 1.0, 2.9), (1.0, 1.0, 2.9), threshold=2.5) == (3, 3, 0)
    assert ro((1.0, 1.0, 1.0), (0.5, 2.0, 0.5)) == (3, 0, 3)          # triggered by the target spacing alone
    assert ro((0.7, 2.5, 2.5), (0.5, 0.5, 2.0)) == (3, 3, 0)          # the file's test fails, the target's decides
    with pytest.raises(ValueError):
        ro((1.0, 0.0, 1.0), (1.0, 1.0, 1.0))
    aff = sc.affine((0.7, 0.7, 2.5), perm=(1, 0, 2))
    assert np.allclose(geometry.voxel_spacing(aff), (0.7, 0.7, 2.5))


def test_order_arguments():
    assert data.resolve_order(1) == (1, 1, 1) and data.resolve_order(3) == (3, 3, 3)
    assert data.resolve_order([3, 0, 3]) == (3, 0, 3) and data.resolve_order((1, 3, 3)) == (1, 3, 3)
    for bad in (2, 0, 4, 5, (3, 3, 2), (3, 3), (3, 3, 3, 3), (3.5, 3, 3), 'cubic', None, True):
        with pytest.raises(ValueError):
            data.resolve_order(bad)
    for unbuilt in ((0, 0, 3), (1, 1, 3), (0, 0, 0), (0, 1, 3), (1, 1, 0)):
        with pytest.raises(ValueError):
            data.resolve_order(unbuilt)
    with pytest.raises(ValueError):
        data._scan_order('nearest', np.eye(4), (1.0, 1.0, 1.0))
    assert data._scan_order('auto', sc.affine((0.7, 0.7, 2.5)), (0.5, 0.5, 2.0)) == (3, 3, 0)
    assert data._scan_order('auto', sc.affine((1.0, 1.0, 1.0)), (1.0, 1.0, 1.0)) == (3, 3, 3)


def test_cpu_tensors_are_refused():
    v = torch.zeros((4, 5, 6))
    eye = np.eye(4)[:3]
    for order in (1, 3, (3, 3, 0)):
        with pytest.raises(_lib.LtuError):
            data.resample(v, None, eye, (6, 5, 4), order=order)
    with pytest.raises(_lib.LtuError):
        data.spline_coefficients(v, (3, 3, 3))


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, 'include', 'ltu_hip.h')).read()
    lib = _lib.load()
    for name in ('ltu_spline_prefilter', 'ltu_resample_spline'):
        assert re.search(r'^int\s+' + name + r'\s*\(', header, flags=re.M), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert 'spline.hip' in open(os.path.join(ROOT, 'lintransunet_amd', 'csrc', 'Makefile')).read()
    # refused before any launch, so it can be asked without a GPU: a triple that is not built, an order outside {0, 1, 3}, NULL
    one = torch.zeros(8)
    mat = torch.zeros(12, dtype=torch.float64)
    p = one.data_ptr()
    inf = float('inf')
    assert lib.ltu_resample_spline(p, 2, 2, 2, 0, 0, 3, p, 2, 2, 2, 4, 2, 1, mat.data_ptr(), 0, -inf, inf, 0) == -4
    assert lib.ltu_resample_spline(p, 2, 2, 2, 3, 3, 2, p, 2, 2, 2, 4, 2, 1, mat.data_ptr(), 0, -inf, inf, 0) == -4
    assert lib.ltu_resample_spline(0, 2, 2, 2, 3, 3, 3, p, 2, 2, 2, 4, 2, 1, mat.data_ptr(), 0, -inf, inf, 0) == -4
    assert lib.ltu_resample_spline(p, 2, 2, 0, 3, 3, 3, p, 2, 2, 2, 4, 2, 1, mat.data_ptr(), 0, -inf, inf, 0) == -2
    assert lib.ltu_spline_prefilter(p, 0, 2, 2, 2, 1, 2, 4, p, 3, 3, 5, 1.0, 0.0, -inf, inf, 0) == -4
    assert lib.ltu_spline_prefilter(p, 7, 2, 2, 2, 1, 2, 4, p, 3, 3, 3, 1.0, 0.0, -inf, inf, 0) == -1
    assert lib.ltu_spline_prefilter(p, 0, 2, 2, 2, 1, 2, 0, p, 3, 3, 3, 1.0, 0.0, -inf, inf, 0) == -2
