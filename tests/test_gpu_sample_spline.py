"""ltu_sample_spline on the device (csrc/augment.hip) behind data.sample_affine(order=3 / (3, 3, 1)): the cubic B-spline patch gather
against the float64 oracle of tests/sample_spline_common.py (scipy's map_coordinates(order=3, mode='constant') plus the clamp), held
to the tolerance that module measures on the oracle; labels, exact patches, channels, deformation, noise and data.sample around it.

Shapes, the smallest that reach every path: a (29, 23, 11) white-noise scan, patches (24, 24, 12) (vector store) and (20, 20, 7)
(scalar), one call of four patches (oblique + zoom leaving the scan, in-plane rotation, integer flip + rot90, zoom) for the general
kernel and one of the three z-decoupled ones for the other."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data, nifti  # noqa: E402
from tests import sample_spline_common as sc  # noqa: E402
from tests import spline_common  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KW = dict(fill=sc.FILL, clamp=sc.CLAMP)


@pytest.fixture(scope='module')
def scan():
    return torch.from_numpy(sc.scan_image()).to(DEV), torch.from_numpy(sc.scan_label()).to(DEV)


@pytest.fixture(scope='module')
def gathered(scan):
    """{(call, size name, orders): (mats, image [n, h, w, d] float64 on the host, label tensor, image tensor)}, each gathered once"""
    di, dl = scan
    out = {}
    for call, names in sc.CALLS.items():
        for sn, size in sc.SIZES.items():
            mats = sc.patch_mats(names, size)
            for orders in sc.ORDERS:
                oi, ol = data.sample_affine(di, dl, mats, size, order=orders, **KW)
                assert oi.shape == (len(names), 1, *size) and oi.dtype == torch.float32 and ol.shape == oi.shape and ol.dtype == torch.uint8
                out[call, sn, orders] = (mats, oi.cpu().numpy()[:, 0].astype(np.float64), ol, oi)
    return out


@pytest.mark.parametrize('orders', sc.ORDERS)
@pytest.mark.parametrize('size_name', list(sc.SIZES))
@pytest.mark.parametrize('call', list(sc.CALLS))
def test_values_match_the_float64_oracle(gathered, call, size_name, orders):
    mats, got, _, _ = gathered[call, size_name, orders]
    clamped = False
    for i, (name, (want, c, keep)) in enumerate(zip(sc.CALLS[call], sc.reference(call, size_name, orders))):
        ins = sc.inside(c)
        err = np.abs(got[i] - want)[keep].max()
        share = 1.0 - keep.mean()
        outside = (~ins).mean()
        print(f'{call} {size_name} {orders} {name}: max err {err:.2e} (tolerance {sc.TOL:.2e}), edge band {share:.5f}, outside {outside:.3f}')
        assert share <= 1e-3, (name, share)
        assert err <= sc.TOL, (name, err)
        assert (got[i][~ins & keep] == sc.FILL).all(), name             # no blending across the edge
        if name == 'oblique' and size_name == 'vec':
            assert outside >= 0.3                                        # the case is there to leave the scan
        if sc.is_cubic(mats[i]):
            clamped = clamped or bool((np.abs(want[ins]) == sc.CLAMP[1]).any())
    assert clamped                                                       # an inside value reaches the clamp


@pytest.mark.parametrize('size_name', list(sc.SIZES))
@pytest.mark.parametrize('call', list(sc.CALLS))
def test_labels_and_exact_patches_are_order_1(scan, gathered, call, size_name):
    di, dl = scan
    size = sc.SIZES[size_name]
    mats = gathered[call, size_name, sc.ORDERS[0]][0]
    pi, pl = data.sample_affine(di, dl, mats, size, fill=sc.FILL)
    k = sc.CALLS[call].index('integer')
    for orders in sc.ORDERS:
        _, _, ol, oi = gathered[call, size_name, orders]
        assert torch.equal(ol, pl), orders
        assert torch.equal(oi[k], pi[k]), orders                         # the integer matrix inside a call that interpolates
        assert not torch.equal(oi[0], pi[0])
    assert len(torch.unique(pl)) == 3                                    # the label patches are not trivially empty


def test_a_call_of_integer_matrices_is_order_1(scan):
    di, dl = scan
    for size in sc.SIZES.values():
        mats = np.stack([data.patch_matrix(st, size, f, k) for st, f, k in (((2, -3, 1), True, 1), ((0, 0, 0), False, 0), ((5, 1, -2), False, 3))])
        pi, pl = data.sample_affine(di, dl, mats, size, fill=sc.FILL)
        for orders in sc.ORDERS:
            oi, ol = data.sample_affine(di, dl, mats, size, order=orders, **KW)
            assert torch.equal(oi, pi) and torch.equal(ol, pl), (size, orders)
        assert (pi.abs() > sc.CLAMP[1]).any()                            # the clamp would have shown


@pytest.mark.parametrize('orders', sc.ORDERS)
def test_channels_are_single_channel_calls(scan, orders):
    di, dl = scan
    size = sc.SIZES['vec']
    mats = sc.patch_mats(sc.CALLS['mixed'], size)
    n = len(mats)
    img = torch.stack([di, torch.from_numpy(spline_common.unit_volume(sc.SCAN, seed=1)).to(DEV), 0.5 * di.flip(0) + 0.25])
    fills, clamps = (sc.FILL, 2.0, -0.5), ((-1.5, 1.5), (-0.7, 2.5), (-np.inf, np.inf))
    sg = np.array([[0.1, 0.0, 0.05]] * n, dtype=np.float32)
    seeds = np.array([[(0x9E3779B97F4A7C15 * (3 * i + c + 1)) % (1 << 64) for c in range(3)] for i in range(n)], dtype=np.uint64)
    oi, ol = data.sample_affine(img, dl, mats, size, fill=fills, noise_sigma=sg, seeds=seeds, order=orders, clamp=clamps)
    assert oi.shape == (n, 3, *size) and ol.shape == (n, 1, *size)
    for c in range(3):
        si, sl = data.sample_affine(img[c].contiguous(), dl, mats, size, fill=fills[c], noise_sigma=sg[:, c], seeds=seeds[:, c],
                                    order=orders, clamp=clamps[c])
        assert torch.equal(oi[:, c], si[:, 0]) and torch.equal(ol, sl), c
    assert not torch.equal(oi[:, 0], oi[:, 1])
    one, _ = data.sample_affine(di[None], dl, mats, size, order=orders, **KW)          # K = 1 through a 4-D image
    flat, _ = data.sample_affine(di, dl, mats, size, order=orders, **KW)
    assert torch.equal(one, flat)


@pytest.mark.parametrize('orders', sc.ORDERS)
@pytest.mark.parametrize('size_name', list(sc.SIZES))
def test_deformation(scan, size_name, orders):
    di, dl = scan
    size = sc.SIZES[size_name]
    mats = sc.patch_mats(sc.DEFORMED, size)
    phi = sc.lattices(size, len(mats))
    oi, ol = data.sample_affine(di, dl, mats, size, elastic=phi, order=orders, **KW)
    pl = data.sample_affine(None, dl, mats, size, elastic=phi)[1]
    assert torch.equal(ol, pl)
    got = oi.cpu().numpy()[:, 0].astype(np.float64)
    still = sc.reference('mixed', size_name, orders)
    for i, (name, (want, c, keep)) in enumerate(zip(sc.DEFORMED, sc.reference('mixed', size_name, orders, deformed=True))):
        err = np.abs(got[i] - want)[keep].max()
        moved = np.abs(want - still[sc.CALLS['mixed'].index(name)][0]).max()
        print(f'{size_name} {orders} {name} deformed: max err {err:.2e} (tolerance {sc.TOL_DEFORMED:.2e}), edge band {1 - keep.mean():.5f}, '
              f'the deformation moves the image by up to {moved:.2f}')
        assert 1 - keep.mean() <= 1e-3 and err <= sc.TOL_DEFORMED, (name, err)
        assert moved >= 50 * sc.TOL_DEFORMED                            # the test cannot pass with the lattice ignored
    zero, zl = data.sample_affine(di, dl, mats, size, elastic=np.zeros_like(phi), order=orders, **KW)
    none, nl = data.sample_affine(di, dl, mats, size, order=orders, **KW)
    assert torch.equal(zero, none) and torch.equal(zl, nl)


def test_noise_is_added_after_the_clamp(scan, gathered):
    di, dl = scan
    size, orders = sc.SIZES['vec'], sc.ORDERS[0]
    mats, _, clean_l, clean = gathered['mixed', 'vec', orders]
    n, count, sigma = len(mats), int(np.prod(size)), 0.1
    seeds = np.array([(0x9E3779B97F4A7C15 * (i + 1)) % (1 << 64) for i in range(n)], dtype=np.uint64)
    noisy, nl = data.sample_affine(di, dl, mats, size, noise_sigma=np.full(n, sigma), seeds=seeds, order=orders, **KW)
    assert torch.equal(nl, clean_l)
    z = ((noisy.double() - clean.double()) / sigma).cpu().numpy().reshape(n, count)
    for i in range(n):
        err = np.abs(z[i] - data.noise_reference(seeds[i], count)).max()
        print(f'noise patch {i}: max |z - reference| {err:.2e}')
        assert err <= 1e-3, (i, err)
    assert (noisy > sc.CLAMP[1] + 0.05).any()                            # past the clamp: the noise came after it
    ssize = sc.SIZES['scalar']
    sm, _, _, sclean = gathered['mixed', 'scalar', orders]
    snoisy, _ = data.sample_affine(di, dl, sm, ssize, noise_sigma=np.full(n, sigma), seeds=seeds, order=orders, **KW)
    zs = ((snoisy.double() - sclean.double()) / sigma).cpu().numpy().reshape(n, -1)
    assert np.abs(zs[0] - data.noise_reference(seeds[0], zs.shape[1])).max() <= 1e-3


def test_two_calls_give_the_same_bytes(scan, gathered):
    di, dl = scan
    for (call, sn, orders), (mats, _, ol, oi) in gathered.items():
        ai, al = data.sample_affine(di, dl, mats, sc.SIZES[sn], order=orders, **KW)
        assert torch.equal(ai, oi) and torch.equal(al, ol), (call, sn, orders)


@pytest.fixture(scope='module')
def nifti_scan(tmp_path_factory):
    """a small SpacedScan from a NIfTI pair: 40 x 36 x 9 at 0.7 / 0.7 / 2.5 mm in the driver's CT window, a tenth of it clipped"""
    d = tmp_path_factory.mktemp('sample_spline')
    X, Y, Z = 40, 36, 9
    img = spline_common.raw_scan((X, Y, Z), 'i16').transpose(2, 1, 0)
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing='ij')
    lab = (((xx - 18) / 9.0) ** 2 + ((yy - 20) / 8.0) ** 2 + ((zz - 4) / 3.0) ** 2 <= 1).astype(np.uint8)
    aff = spline_common.affine((0.7, 0.7, 2.5), (20.0, 15.0, -30.0))
    nifti.save(str(d / 'img.nii.gz'), img, aff)
    nifti.save(str(d / 'lab.nii.gz'), lab, aff)
    return data.SpacedScan(str(d / 'img.nii.gz'), str(d / 'lab.nii.gz'), pixdim=(0.5, 0.5, 2.0), device=DEV)


def test_sample_with_cubic_augmentation_from_nifti(nifti_scan, monkeypatch):
    scan = nifti_scan
    size, n = (32, 32, 8), 4
    built = []
    prefilter = data.spline_coefficients
    monkeypatch.setattr(data, 'spline_coefficients', lambda *a, **k: built.append(1) or prefilter(*a, **k))
    geo = dict(rot_prob=1, zoom_prob=1, noise_prob=0.5, blur_prob=0.0, brightness_prob=0.0, gamma_prob=0.0)
    rs1, rs3, rsd = (np.random.RandomState(6) for _ in range(3))
    i1, l1 = data.sample(scan, size, rs1, num_samples=n, augment=data.Augmentation(**geo))
    i3, l3 = data.sample(scan, size, rs3, num_samples=n, augment=data.Augmentation(order=3, **geo))
    assert torch.equal(l3, l1) and i3.shape == i1.shape == (n, 1, *size)
    for a, b in zip(rs1.get_state(), rs3.get_state()):
        assert np.array_equal(a, b)
    d1 = data.sample_draws(scan, size, np.random.RandomState(6), n, augment=data.Augmentation(**geo))
    d3 = data.sample_draws(scan, size, rsd, n, augment=data.Augmentation(order=3, **geo))
    assert [(tuple(c), f, k) for c, f, k in d1[0]] == [(tuple(c), f, k) for c, f, k in d3[0]]          # the crops
    diff = (i3 - i1).abs().max().item()
    print(f'order 3 against order 1 from the same draws: the image differs by up to {diff:.3f}')
    assert diff > 10 * sc.TOL
    lo, hi = data.intensity_map(scan.intensity)[2:4]
    quiet = [k for k, p in enumerate(d3[1]) if not p['noise']]
    assert quiet and len(quiet) < n
    assert (i3[quiet] >= lo).all() and (i3[quiet] <= hi).all() and (i3[quiet] == hi).any()
    again, _ = data.sample(scan, size, np.random.RandomState(6), num_samples=n, augment=data.Augmentation(order=3, **geo))
    assert torch.equal(again, i3)
    assert len(built) == 1                                               # one coefficient build over the calls
    assert scan.spline_coefficients(3) is scan.spline_coefficients((3, 3, 3)) and len(built) == 1
    assert scan.spline_coefficients((3, 3, 1)).shape == scan.img.shape and len(built) == 2
    scan.drop_coefficients()
    scan.spline_coefficients(3)
    assert len(built) == 3
    with pytest.raises(ValueError):
        scan.spline_coefficients(1)


def test_refusals_with_device_arrays(scan):
    di, dl = scan
    size = sc.SIZES['vec']
    mats = sc.patch_mats(sc.CALLS['mixed'], size)
    with pytest.raises(ValueError):
        data.sample_affine(di, dl, mats, size, order=3, clamp=(1.0, -1.0))
    with pytest.raises(ValueError):
        data.sample_affine(di, dl, mats, size, order=3, coef=torch.zeros((4, 4, 4), device=DEV))
    with pytest.raises(ValueError):
        data.sample_affine(di, dl, mats, size, order=2)
    only_l = data.sample_affine(None, dl, mats, size, order=3)          # a label alone has nothing to interpolate
    assert only_l[0] is None and torch.equal(only_l[1], data.sample_affine(None, dl, mats, size)[1])
    # the C entry point with real device pointers: refused by code, nothing launched or written
    n = len(mats)
    oi = torch.full((n, *size), 7.0, device=DEV)
    ol = torch.full((n, *size), 7, device=DEV, dtype=torch.uint8)
    m = np.ascontiguousarray(mats.reshape(n, 12))
    fill, lo, hi = (np.array([v], dtype=np.float32) for v in (0.0, -1.0, 1.0))
    cubic = np.ones(n, dtype=np.uint8)
    f = _lib.load().ltu_sample_spline
    H, W, D = sc.SCAN

    def call(coef=di.data_ptr(), out=oi.data_ptr(), order_d=3, lo=lo):
        return f(di.data_ptr(), coef, dl.data_ptr(), out, ol.data_ptr(), m.ctypes.data, 0, 0, 0, 0, 0, 0, fill.ctypes.data,
                 lo.ctypes.data, hi.ctypes.data, cubic.ctypes.data, n, 1, H, W, D, *size, order_d, None)

    assert call(coef=0) == -4 and call(order_d=0) == -4 and call(lo=np.array([2.0], dtype=np.float32)) == -4
    assert call(out=oi.data_ptr() + 4) == -3
    torch.cuda.synchronize()
    assert (oi == 7.0).all() and (ol == 7).all()
