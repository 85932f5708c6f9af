"""The augmentation kernels of the NIfTI pipeline on the device (csrc/augment.hip): ltu_sample_affine against torch's float64
grid_sample on a source padded by one voxel of fill (exactly "a tap outside reads fill"), its noise against the numpy restatement of
the generator, ltu_gauss_blur3 against float64 scipy.ndimage.gaussian_filter, and data.sample(augment=) from a NIfTI pair."""
import os
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data  # noqa: E402
from tests.test_nifti_spacing import write_nii  # noqa: E402

DEV = 'cuda'
SHAPE, SPACING, FILL = (40, 36, 20), (0.5, 0.5, 2.0), -0.75
# (start, flip, k, angles, zoom)
CASES = {
    'identity': ((3, 2, 1), False, 0, (0.0, 0.0, 0.0), 1.0),
    'flip_k1': ((20, 18, 10), True, 1, (0.0, 0.0, 0.0), 1.0),
    'inplane': ((12, 10, 6), False, 0, (0.0, 0.0, 0.5), 1.0),
    'oblique_out': ((1, 1, 0), False, 0, (0.2, -0.3, 0.5), 0.7),
    'zoom_in': ((24, 20, 12), True, 1, (0.0, 0.0, -1.1), 1.4),
    'corner': ((28, 24, 13), False, 0, (0.1, 0.15, 2.0), 0.8),
}
SIZES = {'vec': (16, 16, 8), 'scalar': (12, 12, 6)}
# a call takes the z-decoupled kernel only when every matrix in it rotates about D alone: these cases go in a call of their own
INPLANE = ['identity', 'flip_k1', 'inplane', 'zoom_in']


def _source():
    """smooth unit-scale image and a 3-valued label [H][W][D]"""
    g = torch.Generator().manual_seed(3)
    v = F.avg_pool3d(torch.randn((1, 1, *SHAPE), generator=g, dtype=torch.float64), 3, stride=1, padding=1)[0, 0].numpy()
    img = (v / np.abs(v).max()).astype(np.float32)
    hh, ww, dd = np.meshgrid(*[np.arange(n) for n in SHAPE], indexing='ij')
    r = ((hh - 18) / 14.0) ** 2 + ((ww - 19) / 13.0) ** 2 + ((dd - 9) / 8.0) ** 2
    lab = (r <= 1).astype(np.uint8) + (r <= 0.3).astype(np.uint8)
    return img, lab


def _mats(size):
    return np.stack([data.patch_matrix(st, size, f, k, ang, zm, SPACING) for st, f, k, ang, zm in CASES.values()])


def _ref(src, M, size, mode, fill):
    """float64 grid_sample of src [H][W][D], padded by one voxel of fill, at c = M (p, 1) + 1 with border padding"""
    p = np.stack(list(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in size], indexing='ij')) + [np.ones(size)], 0).reshape(4, -1)
    c = (np.asarray(M, dtype=np.float64) @ p).reshape(3, *size)
    pad = np.pad(np.asarray(src, dtype=np.float64), 1, constant_values=fill)
    n = np.array(pad.shape, dtype=np.float64)
    g = np.stack([(2 * (c[s] + 1) + 1) / n[s] - 1 for s in (2, 1, 0)], -1)       # grid_sample's (x, y, z) = (D, W, H) order
    out = F.grid_sample(torch.as_tensor(pad)[None, None], torch.as_tensor(g)[None], mode=mode, padding_mode='border',
                        align_corners=False)
    return out[0, 0].numpy(), c


@pytest.fixture(scope='module')
def sampled():
    """two calls per patch size: all six cases (the general kernel: two of them are oblique) and the four in-plane cases alone
    (the z-decoupled kernel).  (source, {(size name, kernel): (case names, mats, image patches, label patches)})"""
    img, lab = _source()
    di, dl = torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)
    out = {}
    for name, size in SIZES.items():
        m = _mats(size)
        for kernel, cases in (('general', list(CASES)), ('zdec', INPLANE)):
            mk = np.stack([m[list(CASES).index(c)] for c in cases])
            assert (kernel == 'zdec') == bool((mk[:, [0, 1, 2, 2], [2, 2, 0, 1]] == 0).all())      # what the entry point looks at
            oi, ol = data.sample_affine(di, dl, mk, size, fill=FILL)
            assert oi.shape == (len(cases), 1, *size) and oi.dtype == torch.float32 and ol.dtype == torch.uint8
            out[name, kernel] = (cases, mk, oi, ol)
    return (img, lab, di, dl), out


@pytest.mark.gpu
@pytest.mark.parametrize('kernel', ['general', 'zdec'])
@pytest.mark.parametrize('size_name', list(SIZES))
def test_sample_affine_matches_grid_sample_float64(sampled, size_name, kernel):
    (img, lab, _, _), out = sampled
    size = SIZES[size_name]
    cases, mats, oi, ol = out[size_name, kernel]
    oi, ol = oi.cpu().numpy()[:, 0], ol.cpu().numpy()[:, 0]
    for i, case in enumerate(cases):
        ref_i, c = _ref(img, mats[i], size, 'bilinear', FILL)
        err = np.abs(oi[i] - ref_i).max()
        ref_l, _ = _ref(lab, mats[i], size, 'nearest', 0)
        f = c - np.floor(c)
        tie = (np.abs(f - 0.5) < 1e-4).any(0)
        share = tie.mean()
        wrong = int(((ol[i] != ref_l.astype(np.uint8)) & ~tie).sum())
        outside = ((c < 0) | (c > (np.array(SHAPE) - 1).reshape(3, 1, 1, 1))).any(0).mean()
        print(f'{size_name} {kernel} {case}: image max err {err:.2e}, label mismatches away from ties {wrong}, tie share {share:.4f}, '
              f'outside {outside:.2f}')
        assert err <= 1e-3, (case, err)
        assert share <= 0.01, (case, share)
        assert wrong == 0, (case, wrong)
        if case == 'oblique_out':
            assert outside >= 0.3                # the case is there to leave the scan
    assert len(np.unique(ol)) == 3               # the label patches are not trivially empty
    if kernel == 'zdec':                         # the two kernels agree on the cases both ran (each is within 1e-3 of float64)
        gcases, _, gi, gl = out[size_name, 'general']
        for i, case in enumerate(cases):
            j = gcases.index(case)
            diff = np.abs(oi[i] - gi[j, 0].cpu().numpy()).max()
            print(f'{size_name} {case}: z-decoupled against general {diff:.2e}')
            assert diff <= 1e-3, (case, diff)


@pytest.mark.gpu
@pytest.mark.parametrize('kernel', ['general', 'zdec'])
@pytest.mark.parametrize('size_name', list(SIZES))
def test_sample_affine_identity_cases_equal_crop_orient(sampled, size_name, kernel):
    (_, _, di, dl), out = sampled
    size = SIZES[size_name]
    cases, m, oi, ol = out[size_name, kernel]
    for i, case in enumerate(cases):
        if case not in ('identity', 'flip_k1'):
            continue
        st, f, k, _, _ = CASES[case]
        centre = [st[a] + size[a] // 2 for a in range(3)]
        ci, cl = data.crop_orient(di, dl, [(centre, f, k)], size)
        assert torch.equal(oi[i], ci[0]) and torch.equal(ol[i], cl[0]), case
    # image alone and label alone give the same bits as the pair
    only_i, none_l = data.sample_affine(di, None, m, size, fill=FILL)
    none_i, only_l = data.sample_affine(None, dl, m, size, fill=FILL)
    assert none_l is None and none_i is None and torch.equal(only_i, oi) and torch.equal(only_l, ol)


@pytest.mark.gpu
def test_sample_affine_more_patches_than_one_launch():
    img, lab = _source()
    di, dl = torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)
    n, size = _lib.SAMPLE_AFFINE_MAX + 3, (4, 4, 4)
    starts = [(i, (3 * i) % 32, i % 16) for i in range(n)]
    mats = np.stack([data.patch_matrix(st, size, False, 0) for st in starts])
    oi, ol = data.sample_affine(di, dl, mats, size)
    ci, cl = data.crop_orient(di, dl, [([st[a] + 2 for a in range(3)], False, 0) for st in starts], size)
    assert torch.equal(oi, ci) and torch.equal(ol, cl)


@pytest.mark.gpu
@pytest.mark.parametrize('kernel', ['general', 'zdec'])
def test_sample_affine_noise(sampled, kernel):
    (_, _, di, dl), out = sampled
    size = SIZES['vec']
    cases, mats, clean, clean_l = out['vec', kernel]
    n, count, sigma = len(cases), int(np.prod(size)), 0.1
    seeds = np.array([(0x9E3779B97F4A7C15 * (i + 1)) % (1 << 64) for i in range(n)], dtype=np.uint64)
    zero, zl = data.sample_affine(di, dl, mats, size, fill=FILL, noise_sigma=np.zeros(n), seeds=seeds)
    assert torch.equal(zero, clean) and torch.equal(zl, clean_l)
    noisy, nl = data.sample_affine(di, dl, mats, size, fill=FILL, noise_sigma=np.full(n, sigma), seeds=seeds)
    again, _ = data.sample_affine(di, dl, mats, size, fill=FILL, noise_sigma=np.full(n, sigma), seeds=seeds)
    assert torch.equal(noisy, again) and torch.equal(nl, clean_l)
    z = ((noisy.double() - clean.double()) / sigma).cpu().numpy().reshape(n, count)
    for i in range(n):
        err = np.abs(z[i] - data.noise_reference(seeds[i], count)).max()
        print(f'noise patch {i}: max |z - reference| {err:.2e}')
        assert err <= 1e-3, (i, err)
    assert abs(np.corrcoef(z[0], z[1])[0, 1]) < 5 / np.sqrt(2048)
    # a mixed call: only the patches with sigma > 0 change; the scalar store path draws the same deviates per voxel index
    sg = np.array([0.0, sigma] * (n // 2))
    mixed, _ = data.sample_affine(di, dl, mats, size, fill=FILL, noise_sigma=sg, seeds=seeds)
    assert torch.equal(mixed[0::2], clean[0::2]) and torch.equal(mixed[1::2], noisy[1::2])
    ssize = SIZES['scalar']
    _, sm, sclean, _ = out['scalar', kernel]
    snoisy, _ = data.sample_affine(di, dl, sm, ssize, fill=FILL, noise_sigma=np.full(n, sigma), seeds=seeds)
    zs = ((snoisy.double() - sclean.double()) / sigma).cpu().numpy().reshape(n, -1)
    assert np.abs(zs[2] - data.noise_reference(seeds[2], zs.shape[1])).max() <= 1e-3


def _blur_ref(x, sig, mul):
    return np.stack([ndi.gaussian_filter(x[k].astype(np.float64), sig[k], mode='reflect', truncate=4.0) * mul[k] for k in range(len(x))])


@pytest.mark.gpu
def test_gauss_blur3_matches_scipy_float64():
    rs = np.random.RandomState(7)
    x = rs.randn(4, 20, 18, 12).astype(np.float32)
    sig = [(0.0, 0.0, 0.0), (0.5, 0.5, 0.5), (1.0, 1.0, 1.0), (2.0, 0.6, 1.3)]
    mul = [1.0, 1.0, 1.2, 1.0]
    dx = torch.from_numpy(x).to(DEV)
    out = data.gaussian_blur(dx, sig, mul)
    assert out.shape == dx.shape and out.data_ptr() != dx.data_ptr()
    assert torch.equal(out[0], dx[0])                                              # sigma 0: a copy, bit-exact
    err = np.abs(out.cpu().numpy() - _blur_ref(x, sig, mul)).max(axis=(1, 2, 3))
    print('blur 20x18x12 max err per patch', err, 'bound', 1e-5 * np.abs(x).max())
    assert (err <= 1e-5 * np.abs(x).max()).all(), err
    # scalar sigmas [n] and no multiplier; the channel axis is kept
    out1 = data.gaussian_blur(dx[:, None], [0.0, 0.5, 1.0, 0.7])
    assert out1.shape == (4, 1, 20, 18, 12)
    ref1 = _blur_ref(x, [0.0, 0.5, 1.0, 0.7], [1.0] * 4)
    assert np.abs(out1.cpu().numpy()[:, 0] - ref1).max() <= 1e-5 * np.abs(x).max()
    # shorter than a tile on every axis, D % 4 != 0
    y = rs.randn(2, 9, 10, 7).astype(np.float32)
    sy = [(1.4, 1.0, 0.6)] * 2
    oy = data.gaussian_blur(torch.from_numpy(y).to(DEV), sy)
    erry = np.abs(oy.cpu().numpy() - _blur_ref(y, sy, [1.0, 1.0])).max()
    print('blur 9x10x7 max err', erry)
    assert erry <= 1e-5 * np.abs(y).max()
    # several tiles along every axis, odd sizes
    t = rs.randn(1, 37, 21, 41).astype(np.float32)
    ot = data.gaussian_blur(torch.from_numpy(t).to(DEV), [(1.0, 0.8, 1.2)], [0.9])
    assert np.abs(ot.cpu().numpy() - _blur_ref(t, [(1.0, 0.8, 1.2)], [0.9])).max() <= 1e-5 * np.abs(t).max()
    # a constant volume stays constant
    cst = torch.full((2, 20, 18, 12), 3.25, device=DEV)
    oc = data.gaussian_blur(cst, [(2.0, 0.6, 1.3), (1.0, 1.0, 1.0)])
    assert (oc - 3.25).abs().max().item() <= 1e-6 * 3.25
    # more patches than one launch carries
    many = torch.from_numpy(rs.randn(_lib.BLUR_MAX_N + 2, 8, 8, 8).astype(np.float32)).to(DEV)
    om = data.gaussian_blur(many, [0.5] * len(many))
    assert np.abs(om.cpu().numpy() - _blur_ref(many.cpu().numpy(), [0.5] * len(many), [1.0] * len(many))).max() <= 1e-5 * many.abs().max().item()
    with pytest.raises(_lib.LtuError, match='LTU_E_SHAPE'):
        data.gaussian_blur(dx, [2.2] * 4)                                          # radius 9


@pytest.mark.gpu
def test_sample_with_augmentation_from_nifti(tmp_path):
    X, Y, Z = 48, 44, 20
    g = torch.Generator().manual_seed(1)
    raw = (F.avg_pool3d(torch.randn((1, 1, Z, Y, X), generator=g), 3, stride=1, padding=1)[0, 0].numpy() * 600 + 40).astype(np.int16)
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing='ij')
    r = ((xx - 22) / 15.0) ** 2 + ((yy - 24) / 14.0) ** 2 + ((zz - 10) / 7.0) ** 2
    lab = (r <= 1).astype(np.uint8) + (r <= 0.3).astype(np.uint8)
    srow = [[-0.8, 0, 0, 20.0], [0, -0.8, 0, 15.0], [0, 0, 2.5, -30.0]]
    ip = write_nii(tmp_path / 'img.nii.gz', raw, pixdim=(0.8, 0.8, 2.5), sform_code=1, srow=srow)
    lp = write_nii(tmp_path / 'lab.nii.gz', lab, pixdim=(0.8, 0.8, 2.5), sform_code=1, srow=srow)
    scan = data.SpacedScan(ip, lp, device=DEV)
    size = (32, 32, 8)

    def every(p):
        return data.Augmentation(rot_prob=p, zoom_prob=p, noise_prob=p, blur_prob=p, brightness_prob=p, gamma_prob=p)

    a = data.sample(scan, size, np.random.RandomState(4), num_samples=4, augment=every(1.0))
    b = data.sample(scan, size, np.random.RandomState(4), num_samples=4, augment=every(1.0))
    assert a[0].shape == (4, 1, *size) and a[0].dtype == torch.float32 and a[1].shape == (4, 1, *size) and a[1].dtype == torch.uint8
    assert torch.isfinite(a[0]).all()
    assert set(torch.unique(a[1]).tolist()) <= set(torch.unique(scan.lab).tolist())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    plain = data.sample(scan, size, np.random.RandomState(4), num_samples=4)
    assert not torch.equal(a[0], plain[0])                                         # the augmentation did something
    off = data.sample(scan, size, np.random.RandomState(4), num_samples=4, augment=every(0.0))
    assert torch.equal(off[0], plain[0]) and torch.equal(off[1], plain[1])
    # class ratios keep working, and the default fill is the floor of the intensity window
    c = data.sample(scan, size, np.random.RandomState(4), num_samples=2, ratios=[1, 1, 2], augment=data.Augmentation(rot_prob=1.0, zoom_prob=1.0, zoom_range=(0.3, 0.3), noise_prob=0.0, blur_prob=0.0, brightness_prob=0.0, gamma_prob=0.0))
    floor = data.MONAI_CT_WINDOW[2]              # a tap outside reads it; the eight weights sum to 1 within an ulp or two
    assert c[0].shape == (2, 1, *size) and ((c[0] - floor).abs() <= 1e-5).any() and c[0].min().item() >= floor - 1e-5
