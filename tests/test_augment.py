"""Host side of the NIfTI pipeline's augmentation (lintransunet_amd/data.py: patch_matrix, Augmentation and the draw order of
sample(augment=), blur_weights, noise_reference) and the C-ABI refusals of ltu_sample_affine / ltu_gauss_blur3, which are decided
before any launch (the library loads without a GPU)."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import scipy.ndimage as ndi

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data  # noqa: E402

E_SHAPE, E_ARG = -2, -4


def _grid(size):
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in size], indexing='ij')
    return np.stack(list(g) + [np.ones(size)], 0).reshape(4, -1)


@pytest.mark.parametrize('k', range(4))
@pytest.mark.parametrize('flip', [False, True])
def test_patch_matrix_identity_selects_crop_orient_voxels(flip, k):
    vol = np.random.RandomState(0).rand(20, 18, 9)
    start, size = (3, 2, 1), (8, 8, 4)
    M = data.patch_matrix(start, size, flip, k)
    assert M.shape == (3, 4) and M.dtype == np.float64
    c = M @ _grid(size)
    assert np.array_equal(c, np.round(c))
    c = c.astype(np.int64)
    got = vol[c[0], c[1], c[2]].reshape(size)
    crop = vol[3:11, 2:10, 1:5]
    assert np.array_equal(got, np.rot90(np.flip(crop, 0) if flip else crop, k))


def test_patch_matrix_rotates_in_millimetres():
    sp = (0.5, 0.5, 2.0)
    lin = data.patch_matrix((0, 0, 0), (1, 1, 1), False, 0, (0.0, 0.0, np.pi / 2), 1.0, sp)[:, :3]
    v = lin @ np.array([20.0, 0.0, 0.0])                      # 20 voxels along H = 10 mm -> 20 voxels along W
    np.testing.assert_allclose(np.abs(v), [0.0, 20.0, 0.0], atol=1e-12)
    lin = data.patch_matrix((0, 0, 0), (1, 1, 1), False, 0, (np.pi / 2, 0.0, 0.0), 1.0, sp)[:, :3]
    v = lin @ np.array([0.0, 0.0, 4.0])                       # 4 voxels along D = 8 mm -> 16 voxels along W
    np.testing.assert_allclose(np.abs(v), [0.0, 16.0, 0.0], atol=1e-12)
    # zoom > 1 magnifies: a patch step covers 1 / zoom of a scan step
    lin = data.patch_matrix((0, 0, 0), (1, 1, 1), False, 0, (0.0, 0.0, 0.0), 2.0, sp)[:, :3]
    np.testing.assert_allclose(lin, np.eye(3) / 2, atol=1e-15)
    # the rotation convention is rotate_matrix's
    ang = (0.2, -0.3, 0.5)
    np.testing.assert_allclose(data.patch_matrix((0, 0, 0), (9, 7, 5), False, 0, ang), data.rotate_matrix(ang, (9, 7, 5)), atol=1e-5)


def _fake_scan():
    lab = np.zeros((40, 36, 12), np.uint8)
    lab[10:20, 8:30, 3:9] = 1
    return types.SimpleNamespace(lab=lab, img=None, label_host=lab, pixdim=(0.5, 0.5, 2.0), intensity=None)


def _all(p):
    return data.Augmentation(rot_prob=p, zoom_prob=p, noise_prob=p, blur_prob=p, brightness_prob=p, gamma_prob=p)


def test_draw_order_keeps_the_plain_draws(monkeypatch):
    scan, size, N = _fake_scan(), (8, 8, 4), 6
    seen = {}
    monkeypatch.setattr(data, 'crop_orient', lambda img, lab, draws, size: seen.setdefault('plain', draws))
    monkeypatch.setattr(data, '_augmented', lambda scan, draws, params, *a: seen.setdefault('aug', (draws, params)))
    rs0, rs1 = np.random.RandomState(5), np.random.RandomState(5)
    data.sample(scan, size, rs0, num_samples=N, host_centers=True)
    data.sample(scan, size, rs1, num_samples=N, host_centers=True, augment=_all(0.5))
    draws, params = seen['aug']
    assert len(seen['plain']) == N and draws == seen['plain'] and len(params) == N
    # augment=None leaves the generator where it was left before this feature: N samples of 6 draws (centre 2, flip, k, rot90)
    rs2 = np.random.RandomState(5)
    for _ in range(N):
        data.draw_monai_sample(scan.label_host, size, rs2)
    assert rs0.randint(1 << 30) == rs2.randint(1 << 30)
    # every augmentation draw is made whether or not its transform fires
    ra, rb = np.random.RandomState(9), np.random.RandomState(9)
    da, pa = data.sample_draws(scan, size, ra, N, host_centers=True, augment=_all(0.0))
    db, pb = data.sample_draws(scan, size, rb, N, host_centers=True, augment=_all(1.0))
    assert da == db and ra.randint(1 << 30) == rb.randint(1 << 30)
    for a, b in zip(pa, pb):
        assert not any(a[f] for f in ('rotate', 'zoom', 'noise', 'blur', 'bright', 'contrast'))
        assert all(b[f] for f in ('rotate', 'zoom', 'noise', 'blur', 'bright', 'contrast'))
        assert a['angles'] == b['angles'] and a['seed'] == b['seed'] and a['gamma'] == b['gamma']
    # the fixed order of one sample's draws
    rc, rd = np.random.RandomState(3), np.random.RandomState(3)
    p = data.Augmentation().draw(rc)
    assert (rd.rand() < 0.2) == p['rotate']
    assert [rd.uniform(-r, r) for r in (0.0, 0.0, np.pi)] == p['angles'] and p['angles'][:2] == [0.0, 0.0]
    assert (rd.rand() < 0.2) == p['zoom'] and rd.uniform(0.7, 1.4) == p['zoom_factor']
    assert (rd.rand() < 0.1) == p['noise'] and rd.uniform(0.0, 0.1) == p['noise_std']
    assert ((int(rd.randint(2 ** 31)) << 31) | int(rd.randint(2 ** 31))) == p['seed']
    assert (rd.rand() < 0.2) == p['blur'] and rd.uniform(0.5, 1.0) == p['sigma']
    assert (rd.rand() < 0.15) == p['bright'] and rd.uniform(0.75, 1.25) == p['mul']
    assert (rd.rand() < 0.3) == p['contrast'] and rd.uniform(0.7, 1.5) == p['gamma']
    assert data.Augmentation().fill is None


@pytest.mark.parametrize('sigma', [0.5, 1.0, 1.4, 2.0])
def test_blur_weights_match_scipy(sigma):
    w = data.blur_weights(sigma)
    r = int(4 * sigma + 0.5)
    assert w.dtype == np.float64 and w.shape == (2 * r + 1,)
    imp = np.zeros(2 * r + 9)
    imp[r + 4] = 1.0
    ref = ndi.gaussian_filter1d(imp, sigma, mode='constant', truncate=4.0)
    assert np.abs(ref[4:4 + 2 * r + 1] - w).max() <= 1e-12
    assert ref[:4].max() == 0.0 and ref[-4:].max() == 0.0
    assert np.array_equal(data.blur_weights(0.0), np.ones(1))


def test_noise_reference_statistics():
    N = 1 << 20
    z = data.noise_reference(0x1234_5678_9ABC_DEF0, N)
    assert z.shape == (N,) and z.dtype == np.float64
    assert abs(z.mean()) <= 5 / np.sqrt(N)
    assert abs(z.var() - 1) <= 5 * np.sqrt(2 / N)
    zc = z - z.mean()
    assert abs((zc ** 4).mean() / (zc ** 2).mean() ** 2 - 3) <= 5 * np.sqrt(24 / N)
    assert abs(np.corrcoef(z[:-1], z[1:])[0, 1]) <= 5 / np.sqrt(N)
    z2 = data.noise_reference(0x1234_5678_9ABC_DEF1, N)
    assert abs(np.corrcoef(z, z2)[0, 1]) <= 5 / np.sqrt(N)
    assert np.array_equal(z, data.noise_reference(0x1234_5678_9ABC_DEF0, N))
    assert np.array_equal(z[:1001], data.noise_reference(0x1234_5678_9ABC_DEF0, 1001))      # a prefix, odd counts included


def _ptr(a):
    return a.ctypes.data


def test_sample_affine_refusals_before_any_launch():
    lib = _lib.load()
    f = lib.ltu_sample_affine
    X = 4096                                    # stands for a device pointer: every call below is refused before it is used
    n = 2
    mats = np.ascontiguousarray(np.stack([data.patch_matrix((0, 0, 0), (4, 4, 4), False, 0)] * n).reshape(n, 12))
    sig, seeds = np.zeros(n, np.float32), np.zeros(n, np.uint64)
    shape = (16, 16, 8, 4, 4, 4)

    def call(img=X, lab=X, oi=X, ol=X, m=mats, s=None, sd=None, cnt=n, fill=0.0):
        return f(img, lab, oi, ol, _ptr(m) if m is not None else 0, _ptr(s) if s is not None else 0,
                 _ptr(sd) if sd is not None else 0, cnt, *shape, ctypes.c_float(fill), None)

    assert call(oi=0) == E_ARG and call(img=0) == E_ARG and call(ol=0) == E_ARG and call(lab=0) == E_ARG      # unpaired
    assert call(img=0, lab=0, oi=0, ol=0) == E_ARG                                                              # both pairs NULL
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
    assert f(X, X, X, X, _ptr(mats), 0, 0, n, 16, 16, 8, 4, 0, 4, ctypes.c_float(0.0), None) == E_SHAPE
    assert call(cnt=0) == 0                                                                                     # nothing to do


def test_gauss_blur3_refusals_before_any_launch():
    lib = _lib.load()
    f = lib.ltu_gauss_blur3
    X, Y = 4096, 8192
    n, taps = 2, _lib.BLUR_MAX_RADIUS + 1
    wts = np.zeros((n, 3, taps), np.float32)
    wts[:, :, 0] = 1.0
    rad = np.zeros((n, 3), np.int32)
    mul = np.ones(n, np.float32)
    H, W, D = 20, 18, 12

    def call(x=X, out=Y, w=wts, r=rad, m=mul, cnt=n):
        return f(x, out, _ptr(w) if w is not None else 0, _ptr(r) if r is not None else 0, _ptr(m) if m is not None else 0, cnt,
                 H, W, D, None)

    assert call(x=0) == E_ARG and call(out=0) == E_ARG and call(w=None) == E_ARG and call(r=None) == E_ARG
    assert call(out=X) == E_ARG                                       # in place
    assert call(cnt=_lib.BLUR_MAX_N + 1) == E_ARG and call(cnt=-1) == E_ARG
    r = rad.copy()
    r[1, 0] = _lib.BLUR_MAX_RADIUS + 1                                # radius 9
    assert call(r=r) == E_SHAPE
    r = rad.copy()
    r[0, 2] = D                                                       # a radius equal to the axis extent (12 would also be above 8)
    assert call(r=r) == E_SHAPE
    H, W, D = 20, 18, 5
    r = rad.copy()
    r[0, 2] = 5                                                       # within the maximum, equal to the extent
    assert call(r=r) == E_SHAPE
    r[0, 2] = -1
    assert call(r=r) == E_ARG
    m = mul.copy()
    m[0] = np.inf
    assert call(m=m) == E_ARG
    assert call(cnt=0) == 0
