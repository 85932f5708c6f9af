"""Host side of the B-spline elastic deformation of the one-gather patch sampler (lintransunet_amd/data.py: elastic_displacement,
Augmentation's elastic draws, the fold guard of sample / sample_draws, the lattice checks of sample_affine(elastic=)) and the C-ABI
refusals of ltu_sample_elastic, which are decided before any launch (the library loads without a GPU)."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data  # noqa: E402

E_SHAPE, E_ALIGN, E_ARG = -2, -3, -4
ORIGINAL_KEYS = ['rotate', 'angles', 'zoom', 'zoom_factor', 'noise', 'noise_std', 'seed', 'blur', 'sigma', 'bright', 'mul', 'contrast',
                 'gamma']


def _basis(f):
    return np.array([(1 - f) ** 3, 3 * f ** 3 - 6 * f ** 2 + 4, -3 * f ** 3 + 3 * f ** 2 + 3 * f + 1, f ** 3]) / 6


def _direct(phi, size, p):
    """the definition at one patch voxel, written out as the 64-tap sum"""
    i, B = [], []
    for t, n, g in zip(p, size, phi.shape[1:]):
        s = t * (g - 3) / (n - 1) if n > 1 else 0.0
        ia = min(int(np.floor(s)), g - 4)
        i.append(ia)
        B.append(_basis(s - ia))
    u = np.zeros(3)
    for l in range(4):
        for m in range(4):
            for n in range(4):
                u += B[0][l] * B[1][m] * B[2][n] * phi[:, i[0] + l, i[1] + m, i[2] + n]
    return u


def test_zero_and_constant_lattices():
    size, grid = (9, 7, 6), (5, 4, 8)
    u = data.elastic_displacement(np.zeros((3, *grid)), size)
    assert u.shape == (3, *size) and u.dtype == np.float64 and not u.any()
    const = np.broadcast_to(np.array([2.0, -1.0, 0.37]).reshape(3, 1, 1, 1), (3, *grid))
    u = data.elastic_displacement(const, size)
    assert np.abs(u - const[:, :1, :1, :1]).max() <= 1e-12                 # partition of unity


def test_matches_the_64_tap_definition_and_is_linear():
    rs = np.random.RandomState(0)
    size, grid = (9, 7, 6), (5, 4, 8)
    a, b = rs.uniform(-3, 3, (3, *grid)), rs.uniform(-3, 3, (3, *grid))
    ua, ub = data.elastic_displacement(a, size), data.elastic_displacement(b, size)
    for p in [(0, 0, 0), (8, 6, 5), (4, 3, 2), (7, 0, 5), (3, 6, 1)]:      # corners (the far-end clamp), interior, cell boundaries
        assert np.abs(ua[(slice(None), *p)] - _direct(a, size, p)).max() <= 1e-12, p
    assert np.abs(data.elastic_displacement(2.5 * a - 0.75 * b, size) - (2.5 * ua - 0.75 * ub)).max() <= 1e-12


def test_far_end_is_the_last_cell_at_f_1():
    rs = np.random.RandomState(1)
    size, grid = (10, 8, 5), (6, 4, 7)
    phi = rs.uniform(-2, 2, (3, *grid))
    u = data.elastic_displacement(phi, size)
    B1 = _basis(1.0)                                                       # (0, 1, 4, 1) / 6
    assert B1[0] == 0.0
    want = np.einsum('l,m,n,clmn->c', B1, B1, B1, phi[:, -4:, -4:, -4:])   # i = g - 4 on every axis
    assert np.abs(u[:, -1, -1, -1] - want).max() <= 1e-12
    # along one axis alone: last voxel of H, first of W and D
    want = np.einsum('l,m,n,clmn->c', B1, _basis(0.0), _basis(0.0), phi[:, -4:, :4, :4])
    assert np.abs(u[:, -1, 0, 0] - want).max() <= 1e-12


def test_thin_axis():
    rs = np.random.RandomState(2)
    phi = rs.uniform(-1, 1, (3, 4, 5, 4))
    u = data.elastic_displacement(phi, (1, 6, 1))
    assert u.shape == (3, 1, 6, 1) and np.isfinite(u).all()
    for y in (0, 3, 5):
        assert np.abs(u[:, 0, y, 0] - _direct(phi, (1, 6, 1), (0, y, 0))).max() <= 1e-12
    with pytest.raises(ValueError):
        data.elastic_displacement(np.zeros((3, 3, 4, 4)), (4, 4, 4))


def test_default_draws_unchanged():
    ra, rb, rc = np.random.RandomState(6), np.random.RandomState(6), np.random.RandomState(6)
    p = data.Augmentation().draw(ra)
    assert list(p) == ORIGINAL_KEYS
    # the 16 original draws, replayed
    rb.rand(), [rb.uniform(-r, r) for r in (0.0, 0.0, np.pi)], rb.rand(), rb.uniform(0.7, 1.4), rb.rand(), rb.uniform(0.0, 0.1)
    rb.randint(2 ** 31), rb.randint(2 ** 31), rb.rand(), rb.uniform(0.5, 1.0), rb.rand(), rb.uniform(0.75, 1.25), rb.rand(), rb.uniform(0.7, 1.5)
    assert ra.randint(1 << 30) == rb.randint(1 << 30)
    q = data.Augmentation(elastic_prob=0.5).draw(rc)
    assert list(q) == ORIGINAL_KEYS + ['elastic', 'elastic_mm', 'phi']
    assert all(p[key] == q[key] for key in ORIGINAL_KEYS)


def test_elastic_draws_are_always_made():
    states = []
    for prob in (1e-9, 1.0):
        rs, rr = np.random.RandomState(8), np.random.RandomState(8)
        aug = data.Augmentation(elastic_prob=prob, elastic_mm=(1.0, 3.0), elastic_grid=(5, 7, 4))
        p = aug.draw(rs)
        data.Augmentation().draw(rr)                                       # the 16 draws in front
        assert p['elastic'] == (rr.rand() < prob) and p['elastic_mm'] == rr.uniform(1.0, 3.0)
        assert p['phi'].shape == (3, 5, 7, 4) and np.array_equal(p['phi'], rr.uniform(-1, 1, (3, 5, 7, 4)))
        assert np.abs(p['phi']).max() <= 1.0 and 1.0 <= p['elastic_mm'] <= 3.0
        states.append(rs.randint(1 << 30))
    assert states[0] == states[1]
    with pytest.raises(ValueError):
        data.Augmentation(elastic_grid=(3, 6, 4))
    with pytest.raises(ValueError):
        data.Augmentation(elastic_grid=(6, 9, 4))


def _fake_scan(pixdim=(0.5, 0.5, 2.0)):
    lab = np.zeros((40, 36, 12), np.uint8)
    lab[10:20, 8:30, 3:9] = 1
    return types.SimpleNamespace(lab=lab, img=None, label_host=lab, pixdim=pixdim, intensity=None)


def test_fold_guard_raises_before_any_draw():
    scan, size = _fake_scan(), (16, 16, 8)
    # in plane: 0.4 * 15 / 3 = 2 voxels = 1 mm at 0.5 mm; along D: 0.4 * 7 / 1 = 2.8 voxels = 5.6 mm at 2 mm
    ok = data.Augmentation(elastic_prob=0.5, elastic_mm=(0.0, 1.0), zoom_range=(0.7, 1.0))
    draws, params = data.sample_draws(scan, size, np.random.RandomState(3), 2, host_centers=True, augment=ok)
    assert len(params) == 2 and all('phi' in p and 'elastic' in p and 'elastic_mm' in p for p in params)
    for bad in (data.Augmentation(elastic_prob=0.5, elastic_mm=(0.0, 1.0), zoom_range=(0.7, 1.01)),        # zoom magnifies the lattice
                data.Augmentation(elastic_prob=0.5, elastic_mm=(0.0, 1.01), zoom_range=(0.7, 1.0)),
                data.Augmentation(elastic_prob=0.5, elastic_mm=(0.0, 1.0), zoom_range=(0.7, 1.0), elastic_grid=(6, 7, 4)),
                data.Augmentation(elastic_prob=0.5, elastic_mm=(0.0, 1.2), zoom_range=(0.7, 1.0), elastic_grid=(4, 4, 8))):     # along D only
        for fn in (data.sample_draws, data.sample):
            rs, rr = np.random.RandomState(3), np.random.RandomState(3)
            with pytest.raises(ValueError, match='fold'):
                fn(scan, size, rs, 2, host_centers=True, augment=bad)
            assert rs.randint(1 << 30) == rr.randint(1 << 30)               # no draw was consumed
    # the same ranges pass while the deformation is off, and the default record passes at the driver's patch size
    off = data.Augmentation(elastic_mm=(0.0, 50.0))
    data.sample_draws(scan, size, np.random.RandomState(3), 1, host_centers=True, augment=off)
    data.Augmentation(elastic_prob=1.0).check_fold((512, 512, 32), (0.5, 0.5, 2.0))
    # an odd rot90 maps patch axis H onto scan axis W: the finer in-plane spacing counts for both, unless no rot90 can fire
    aniso = data.Augmentation(elastic_prob=1.0, elastic_mm=(0.0, 1.0), zoom_range=(1.0, 1.0))
    aniso.check_fold(size, (0.5, 1.0, 2.0), swap=False)
    with pytest.raises(ValueError, match='fold'):
        aniso.check_fold(size, (1.0, 0.4, 2.0))
    aniso.check_fold((16, 16, 8), (1.0, 0.5, 2.0))


def test_sample_affine_checks_the_lattice_on_the_host():
    mats = np.stack([data.patch_matrix((0, 0, 0), (8, 8, 4), False, 0)] * 2)

    def call(lat):
        return data.sample_affine(None, None, mats, (8, 8, 4), elastic=lat)        # the lattice is checked before the device is asked for

    good = np.zeros((2, 3, 4, 5, 8), np.float32)
    with pytest.raises(_lib.LtuError, match='GPU only'):
        call(good)
    for shape in [(2, 3, 3, 4, 4), (2, 3, 4, 9, 4), (2, 3, 4, 4), (2, 2, 4, 4, 4), (2, 3, 4, 4, 4, 1)]:
        with pytest.raises(ValueError, match='lattice extents'):
            call(np.zeros(shape, np.float32))
    for bad in (np.nan, np.inf, -np.inf, 64.5, -65.0):
        lat = good.copy()
        lat[1, 2, 3, 4, 7] = bad
        with pytest.raises(ValueError, match='finite'):
            call(lat)
    lat = good.copy()
    lat[0, 0, 0, 0, 0], lat[1, 1, 1, 1, 1] = 64.0, -64.0                    # the bound itself is allowed
    with pytest.raises(_lib.LtuError, match='GPU only'):
        call(lat)


def _ptr(a):
    return a.ctypes.data


def test_sample_elastic_refusals_before_any_launch():
    lib = _lib.load()
    f = lib.ltu_sample_elastic
    X = 4096                                    # stands for a device pointer: every call below is refused before it is used
    n = 2
    mats = np.ascontiguousarray(np.stack([data.patch_matrix((0, 0, 0), (4, 4, 4), False, 0)] * n).reshape(n, 12))
    sig, seeds = np.zeros(n, np.float32), np.zeros(n, np.uint64)

    def call(img=X, lab=X, oi=X, ol=X, m=mats, phi=X, g=(4, 4, 4), s=None, sd=None, cnt=n, fill=0.0, shape=(16, 16, 8, 4, 4, 4)):
        return f(img, lab, oi, ol, _ptr(m) if m is not None else 0, phi, *g, _ptr(s) if s is not None else 0,
                 _ptr(sd) if sd is not None else 0, cnt, *shape, ctypes.c_float(fill), None)

    # what ltu_sample_affine refuses, with its codes
    assert call(oi=0) == E_ARG and call(img=0) == E_ARG and call(ol=0) == E_ARG and call(lab=0) == E_ARG      # unpaired
    assert call(img=0, lab=0, oi=0, ol=0) == E_ARG
    assert call(m=None) == E_ARG
    assert call(cnt=_lib.SAMPLE_AFFINE_MAX + 1) == E_ARG and call(cnt=-1) == E_ARG
    assert call(s=sig) == E_ARG                                                                                 # sigma without seeds
    for bad in (np.nan, np.inf, -np.inf):
        m = mats.copy()
        m[1, 7] = bad
        assert call(m=m) == E_ARG
    s = sig.copy()
    s[1] = -0.1
    assert call(s=s, sd=seeds) == E_ARG
    s[1] = np.nan
    assert call(s=s, sd=seeds) == E_ARG
    assert call(fill=float('nan')) == E_ARG
    assert call(shape=(16, 16, 8, 4, 0, 4)) == E_SHAPE
    assert call(shape=(16, 16, 8, 65536, 4, 4)) == E_SHAPE
    assert call(oi=X + 4) == E_ALIGN and call(ol=X + 2) == E_ALIGN                                              # d % 4 == 0: vector stores
    # its own
    assert call(phi=0) == E_ARG
    for a in range(3):
        for ext in (3, _lib.ELASTIC_MAX_GRID + 1, 0, -4):
            g = [4, 4, 4]
            g[a] = ext
            assert call(g=g) == E_SHAPE, g
    assert call(phi=X + 2) == E_ALIGN
    assert call(cnt=0) == 0 and call(cnt=0, g=(8, 8, 8)) == 0                                                   # nothing to do
