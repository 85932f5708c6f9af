"""ltu_sample_elastic on the device (csrc/augment.hip): the one-gather patch sampler with a cubic B-spline free-form deformation
folded in, against data.elastic_displacement plus torch's float64 grid_sample (the construction of tests/test_gpu_augment.py, on its
source, spacing, fill and six matrix cases), against ltu_sample_affine for a zero lattice, against shifted crops for a constant
lattice, and data.sample(augment=Augmentation(elastic_prob=...)) from a NIfTI pair.

Three (patch size, lattice) settings, the smallest at which the kernel can still go wrong:
  one_cell  (16, 16, 8) with (4, 4, 4): one lattice cell, vector stores, a run of 4 voxels inside one cell (5 lattice columns);
  scalar    (12, 12, 6) with (5, 4, 4): one voxel per lane, ragged tiles, two cells along H;
  max_grid  (16, 16, 8) with (8, 8, 8): a cell boundary inside every run of 4 voxels along z (8 lattice columns), the largest
            lattice, the far-end clamp on every axis."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data  # noqa: E402
from tests.test_gpu_augment import CASES, FILL, SHAPE, _mats, _source  # noqa: E402
from tests.test_nifti_spacing import write_nii  # noqa: E402

DEV = 'cuda'
SETTINGS = {'one_cell': ((16, 16, 8), (4, 4, 4)), 'scalar': ((12, 12, 6), (5, 4, 4)), 'max_grid': ((16, 16, 8), (8, 8, 8))}


def _lattices():
    """{setting: [6, 3, gh, gw, gd] float32}: RandomState(11).uniform(-1, 1) times 0.4 lattice cells per axis, drawn in the order of
    SETTINGS and CASES"""
    rs = np.random.RandomState(11)
    out = {}
    for name, (size, grid) in SETTINGS.items():
        cell = np.array([(size[a] - 1) / (grid[a] - 3) for a in range(3)]).reshape(1, 3, 1, 1, 1)
        out[name] = (rs.uniform(-1, 1, (len(CASES), 3, *grid)) * 0.4 * cell).astype(np.float32)
    return out


def _ref(src, M, phi, size, mode, fill):
    """float64 grid_sample of src [H][W][D], padded by one voxel of fill, at c = M (p + u(p), 1) + 1 with border padding"""
    p = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in size], indexing='ij'), 0)
    q = p + data.elastic_displacement(phi, size)
    M = np.asarray(M, dtype=np.float64)
    c = np.einsum('sa,axyz->sxyz', M[:, :3], q) + M[:, 3].reshape(3, 1, 1, 1)
    pad = np.pad(np.asarray(src, dtype=np.float64), 1, constant_values=fill)
    n = np.array(pad.shape, dtype=np.float64)
    g = np.stack([(2 * (c[s] + 1) + 1) / n[s] - 1 for s in (2, 1, 0)], -1)       # grid_sample's (x, y, z) = (D, W, H) order
    out = F.grid_sample(torch.as_tensor(pad)[None, None], torch.as_tensor(g)[None], mode=mode, padding_mode='border',
                        align_corners=False)
    return out[0, 0].numpy(), c


@pytest.fixture(scope='module')
def scan():
    img, lab = _source()
    return img, lab, torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)


@pytest.fixture(scope='module')
def plain(scan):
    """{size: (mats, image, label)} of ltu_sample_affine on the six cases in one call (two of them are oblique: the general kernel)"""
    _, _, di, dl = scan
    out = {}
    for size in {s for s, _ in SETTINGS.values()}:
        m = _mats(size)
        assert not (m[:, [0, 1, 2, 2], [2, 2, 0, 1]] == 0).all()
        out[size] = (m, *data.sample_affine(di, dl, m, size, fill=FILL))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('setting', list(SETTINGS))
def test_sample_elastic_matches_float64(scan, setting):
    img, lab, di, dl = scan
    size, grid = SETTINGS[setting]
    phi, mats = _lattices()[setting], _mats(size)
    oi, ol = data.sample_affine(di, dl, mats, size, fill=FILL, elastic=phi)
    assert oi.shape == (len(CASES), 1, *size) and oi.dtype == torch.float32 and ol.shape == oi.shape and ol.dtype == torch.uint8
    oi, ol = oi.cpu().numpy()[:, 0], ol.cpu().numpy()[:, 0]
    for i, case in enumerate(CASES):
        ref_i, c = _ref(img, mats[i], phi[i], size, 'bilinear', FILL)
        err = np.abs(oi[i] - ref_i).max()
        ref_l, _ = _ref(lab, mats[i], phi[i], size, 'nearest', 0)
        f = c - np.floor(c)
        tie = (np.abs(f - 0.5) < 1e-4).any(0)
        share = tie.mean()
        wrong = int(((ol[i] != ref_l.astype(np.uint8)) & ~tie).sum())
        outside = ((c < 0) | (c > (np.array(SHAPE) - 1).reshape(3, 1, 1, 1))).any(0).mean()
        moved = np.abs(ref_i - _ref(img, mats[i], np.zeros_like(phi[i]), size, 'bilinear', FILL)[0]).max()
        print(f'{setting} {case}: image max err {err:.2e}, label mismatches away from ties {wrong}, tie share {share:.4f}, '
              f'outside {outside:.2f}, the deformation moves the image by up to {moved:.2e}')
        assert err <= 1e-3, (case, err)
        assert share <= 0.01, (case, share)
        assert wrong == 0, (case, wrong)
        assert moved >= 0.05, (case, moved)          # the lattice is not trivially small against the 1e-3 asked above
        if case == 'oblique_out':
            assert outside >= 0.3                    # the case is there to leave the scan
    assert len(np.unique(ol)) == 3                   # the label patches are not trivially empty


@pytest.mark.gpu
@pytest.mark.parametrize('setting', list(SETTINGS))
def test_zero_lattice_is_sample_affine_bit_for_bit(scan, plain, setting):
    _, _, di, dl = scan
    size, grid = SETTINGS[setting]
    mats, pi, pl = plain[size]
    n = len(CASES)
    zero = np.zeros((n, 3, *grid), np.float32)
    oi, ol = data.sample_affine(di, dl, mats, size, fill=FILL, elastic=zero)
    assert torch.equal(oi, pi) and torch.equal(ol, pl)
    for i, case in enumerate(CASES):                 # integer matrices: the source voxels themselves
        if case in ('identity', 'flip_k1'):
            st, f, k, _, _ = CASES[case]
            ci, cl = data.crop_orient(di, dl, [([st[a] + size[a] // 2 for a in range(3)], f, k)], size)
            assert torch.equal(oi[i], ci[0]) and torch.equal(ol[i], cl[0]), case
    # a device tensor is taken as it is
    ti, tl = data.sample_affine(di, dl, mats, size, fill=FILL, elastic=torch.zeros((n, 3, *grid), device=DEV))
    assert torch.equal(ti, pi) and torch.equal(tl, pl)
    # noise in the store draws the same deviates
    seeds = np.array([(0x9E3779B97F4A7C15 * (i + 1)) % (1 << 64) for i in range(n)], dtype=np.uint64)
    sg = np.array([0.1, 0.0, 0.05] * 2)
    ni, nl = data.sample_affine(di, dl, mats, size, fill=FILL, noise_sigma=sg, seeds=seeds)
    ei, el = data.sample_affine(di, dl, mats, size, fill=FILL, noise_sigma=sg, seeds=seeds, elastic=zero)
    assert torch.equal(ei, ni) and torch.equal(el, nl) and not torch.equal(ni[0], pi[0]) and torch.equal(ni[1], pi[1])


@pytest.mark.gpu
@pytest.mark.parametrize('setting', list(SETTINGS))
def test_constant_lattice_shifts_the_crop(scan, setting):
    img, lab, di, dl = scan
    size, grid = SETTINGS[setting]
    st = CASES['identity'][0]
    m = _mats(size)[list(CASES).index('identity')][None]
    shift = (2, -1, 1)
    phi = np.broadcast_to(np.array(shift, np.float32).reshape(1, 3, 1, 1, 1), (1, 3, *grid)).copy()
    oi, ol = data.sample_affine(di, dl, m, size, fill=FILL, elastic=phi)
    sl = tuple(slice(st[a] + shift[a], st[a] + shift[a] + size[a]) for a in range(3))
    assert np.array_equal(ol.cpu().numpy()[0, 0], lab[sl])
    err = np.abs(oi.cpu().numpy()[0, 0] - img[sl]).max()
    print(f'{setting}: constant lattice {shift}, image max |patch - shifted crop| {err:.2e}')
    assert err <= 1e-5
    only_i, none_l = data.sample_affine(di, None, m, size, fill=FILL, elastic=phi)
    none_i, only_l = data.sample_affine(None, dl, m, size, fill=FILL, elastic=phi)
    assert none_l is None and none_i is None and torch.equal(only_i, oi) and torch.equal(only_l, ol)


@pytest.mark.gpu
def test_a_lattice_per_patch_across_launches(scan):
    _, _, di, dl = scan
    n, size, grid = _lib.SAMPLE_AFFINE_MAX + 3, (6, 5, 4), (4, 5, 4)
    rs = np.random.RandomState(5)
    mats = np.stack([data.patch_matrix((i, (3 * i) % 30, i % 15), size, bool(i % 2), 0, (0.0, 0.0, 0.1 * i)) for i in range(n)])
    phi = rs.uniform(-2, 2, (n, 3, *grid)).astype(np.float32)
    oi, ol = data.sample_affine(di, dl, mats, size, fill=FILL, elastic=phi)
    zi, _ = data.sample_affine(di, dl, mats, size, fill=FILL)
    for i in range(n):
        si, sl = data.sample_affine(di, dl, mats[i:i + 1], size, fill=FILL, elastic=phi[i:i + 1])
        assert torch.equal(oi[i], si[0]) and torch.equal(ol[i], sl[0]), i
        assert not torch.equal(oi[i], zi[i]), i
    # this narrow, shallow patch folds more rows into a workgroup than the kernel keeps lattices for (the rest of the lanes idle),
    # and its run of 4 voxels spans the whole lattice along z: the first and last patch of each launch against float64
    img = scan[0]
    for i in (0, _lib.SAMPLE_AFFINE_MAX - 1, _lib.SAMPLE_AFFINE_MAX, n - 1):
        err = np.abs(oi[i, 0].cpu().numpy() - _ref(img, mats[i], phi[i], size, 'bilinear', FILL)[0]).max()
        print(f'patch {i} of {n}, {size} with lattice {grid}: image max err {err:.2e}')
        assert err <= 1e-3, (i, err)


@pytest.mark.gpu
def test_wide_patch_one_row_per_workgroup(scan):
    """(4, 130, 8): the tile of a workgroup is one row of 128 y (the shape of the driver's 512 x 512 x 32 patches: the lattice enters
    LDS contracted for a single x), two tiles along y with the second ragged, lattice cells of different counts per axis"""
    img, lab, di, dl = scan
    size, grid = (4, 130, 8), (4, 6, 5)
    mats = np.stack([data.patch_matrix((18, -47, 6), size, False, 0, ang, 3.6, (1.0, 1.0, 1.0)) for ang in ((0.0, 0.0, 0.0), (0.3, 0.0, 0.1))])
    cell = np.array([(size[a] - 1) / (grid[a] - 3) for a in range(3)]).reshape(1, 3, 1, 1, 1)
    phi = (np.random.RandomState(13).uniform(-1, 1, (2, 3, *grid)) * 0.4 * cell).astype(np.float32)
    oi, ol = data.sample_affine(di, dl, mats, size, fill=FILL, elastic=phi)
    for i in range(2):
        ref_i, c = _ref(img, mats[i], phi[i], size, 'bilinear', FILL)
        ref_l, _ = _ref(lab, mats[i], phi[i], size, 'nearest', 0)
        tie = (np.abs(c - np.floor(c) - 0.5) < 1e-4).any(0)
        err = np.abs(oi[i, 0].cpu().numpy() - ref_i).max()
        wrong = int(((ol[i, 0].cpu().numpy() != ref_l.astype(np.uint8)) & ~tie).sum())
        inside = ((c >= 0) & (c <= (np.array(SHAPE) - 1).reshape(3, 1, 1, 1))).all(0).mean()
        print(f'wide patch {i}: image max err {err:.2e}, label mismatches away from ties {wrong}, tie share {tie.mean():.4f}, inside {inside:.2f}')
        assert err <= 1e-3 and wrong == 0 and tie.mean() <= 0.01 and inside >= 0.5, (i, err, wrong, tie.mean(), inside)
    assert len(np.unique(ol.cpu().numpy())) >= 2


def _nifti_scan(tmp_path):
    X, Y, Z = 48, 44, 20
    g = torch.Generator().manual_seed(1)
    raw = (F.avg_pool3d(torch.randn((1, 1, Z, Y, X), generator=g), 3, stride=1, padding=1)[0, 0].numpy() * 600 + 40).astype(np.int16)
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing='ij')
    r = ((xx - 22) / 15.0) ** 2 + ((yy - 24) / 14.0) ** 2 + ((zz - 10) / 7.0) ** 2
    lab = (r <= 1).astype(np.uint8) + (r <= 0.3).astype(np.uint8)
    srow = [[-0.8, 0, 0, 20.0], [0, -0.8, 0, 15.0], [0, 0, 2.5, -30.0]]
    ip = write_nii(tmp_path / 'img.nii.gz', raw, pixdim=(0.8, 0.8, 2.5), sform_code=1, srow=srow)
    lp = write_nii(tmp_path / 'lab.nii.gz', lab, pixdim=(0.8, 0.8, 2.5), sform_code=1, srow=srow)
    return data.SpacedScan(ip, lp, device=DEV)


@pytest.mark.gpu
def test_sample_with_elastic_augmentation_from_nifti(tmp_path):
    scan = _nifti_scan(tmp_path)
    size = (32, 32, 8)
    # the fold guard at 0.5 mm in plane: 0.4 * 31 / 3 = 4.1 voxels >= 1.0 mm * 1.4 / 0.5 mm = 2.8 voxels

    def every(p, **kw):
        return data.Augmentation(rot_prob=p, zoom_prob=p, noise_prob=p, blur_prob=p, brightness_prob=p, gamma_prob=p, **kw)

    el = dict(elastic_mm=(0.5, 1.0), elastic_grid=(6, 6, 4))
    a = data.sample(scan, size, np.random.RandomState(4), num_samples=4, augment=every(1.0, elastic_prob=1.0, **el))
    b = data.sample(scan, size, np.random.RandomState(4), num_samples=4, augment=every(1.0, elastic_prob=1.0, **el))
    assert a[0].shape == (4, 1, *size) and a[0].dtype == torch.float32 and a[1].shape == (4, 1, *size) and a[1].dtype == torch.uint8
    assert torch.isfinite(a[0]).all()
    assert set(torch.unique(a[1]).tolist()) <= set(torch.unique(scan.lab).tolist())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # elastic_prob == 0 is today's call: the same draws, the same patches
    today = data.sample(scan, size, np.random.RandomState(4), num_samples=4, augment=every(1.0))
    off = data.sample(scan, size, np.random.RandomState(4), num_samples=4, augment=every(1.0, elastic_prob=0.0, **el))
    assert torch.equal(off[0], today[0]) and torch.equal(off[1], today[1])
    # one sample: its other draws are those of the undeformed call, so what differs is the deformation; a deformation that is
    # drawn but does not fire leaves the undeformed patch
    geo = dict(rot_prob=1.0, zoom_prob=1.0, noise_prob=0.0, blur_prob=0.0, brightness_prob=0.0, gamma_prob=0.0)
    one = data.sample(scan, size, np.random.RandomState(9), augment=data.Augmentation(**geo))
    bent = data.sample(scan, size, np.random.RandomState(9), augment=data.Augmentation(elastic_prob=1.0, **geo, **el))
    idle = data.sample(scan, size, np.random.RandomState(9), augment=data.Augmentation(elastic_prob=1e-12, **geo, **el))
    assert not torch.equal(bent[0], one[0]) and not torch.equal(bent[1], one[1])
    assert torch.equal(idle[0], one[0]) and torch.equal(idle[1], one[1])
    print(f'end to end: the deformation changes {(bent[1] != one[1]).float().mean().item():.3f} of the label voxels')
    # in a call where some patches fire, the others keep a zero lattice: their patches are the undeformed ones of the general
    # kernel (oblique rotations, so that the undeformed call takes it too; the z-decoupled kernel rounds differently)
    aug = data.Augmentation(elastic_prob=1.0, rot_range=(0.1, 0.1, np.pi), **geo, **el)
    draws, params = data.sample_draws(scan, size, np.random.RandomState(12), 6, augment=aug)
    fired = [i % 2 == 0 for i in range(6)]
    params = [dict(p, elastic=f) for p, f in zip(params, fired)]
    mixed = data._augmented(scan, draws, params, size, aug, scan.pixdim)
    still = data._augmented(scan, draws, [dict(p, elastic=False) for p in params], size, aug, scan.pixdim)
    for i, f in enumerate(fired):
        assert torch.equal(mixed[0][i], still[0][i]) != f and (f or torch.equal(mixed[1][i], still[1][i])), i


@pytest.mark.gpu
def test_refusals_with_device_arrays(scan):
    _, _, di, dl = scan
    size = (16, 16, 8)
    mats = _mats(size)
    n = len(mats)
    for bad in (torch.full((n, 3, 4, 4, 4), float('nan'), device=DEV), torch.full((n, 3, 4, 4, 4), 64.5, device=DEV),
                torch.zeros((n, 3, 4, 4, 9), device=DEV), torch.zeros((n, 3, 3, 4, 4), device=DEV), np.zeros((n, 2, 4, 4, 4), np.float32)):
        with pytest.raises(ValueError):
            data.sample_affine(di, dl, mats, size, fill=FILL, elastic=bad)
    with pytest.raises(ValueError, match='lattices for'):
        data.sample_affine(di, dl, mats, size, fill=FILL, elastic=np.zeros((n - 1, 3, 4, 4, 4), np.float32))
    # the C entry point with real device pointers: refused by code, nothing launched or written
    oi = torch.full((n, *size), 7.0, device=DEV)
    ol = torch.full((n, *size), 7, device=DEV, dtype=torch.uint8)
    phi = torch.zeros((n, 3, 4, 4, 4), device=DEV)
    m = np.ascontiguousarray(mats.reshape(n, 12))
    f = _lib.load().ltu_sample_elastic
    H, W, D = SHAPE

    def call(p=phi.data_ptr(), g=(4, 4, 4), cnt=n):
        return f(di.data_ptr(), dl.data_ptr(), oi.data_ptr(), ol.data_ptr(), m.ctypes.data, p, *g, 0, 0, cnt, H, W, D, *size, FILL, None)

    assert call(p=0) == -4 and call(g=(4, 4, 9)) == -2 and call(g=(3, 4, 4)) == -2 and call(cnt=_lib.SAMPLE_AFFINE_MAX + 1) == -4
    assert call(p=phi.data_ptr() + 2) == -3
    torch.cuda.synchronize()
    assert (oi == 7.0).all() and (ol == 7).all()
