"""The label vote on the device: ltu_resample_vote (csrc/resample.hip) behind data.resample(label_order=1), SpacedScan(label_order=1)
and data.to_native(order=1); ltu_sample_vote (csrc/augment.hip) behind data.sample_affine(label_order=1) and
data.sample(augment=Augmentation(label_order=1)).  Exact where the rule makes it exact (ltu_resample_argmax on float32 one-hot
channels, integer matrices, the same patches in other calls), against the float64 oracle of tests/label_vote_common.py outside its
derived tie bands everywhere else.

Shapes, the smallest that reach every path: a (23, 19, 11) source onto (70, 67, 3) and (5, 70, 9) (the 64-wide tile crossed on each
axis, every lane axis, both layouts); a (24, 20, 12) blob label, patches of depth 8 (4 voxels per lane) and 5 (one), a z-decoupled
and a general call, lattices (4, 4, 4) and, at depth 8, (4, 4, 6) (the wider column window of the elastic kernel)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data, geometry, nifti  # noqa: E402
from tests import label_vote_common as lv  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
S = lv.RS_SOURCE
TO_NATIVE_SRC = (S[1] * S[2], S[2], 1)                        # the strides data.to_native reads an [H, W, D] label map through


def _to_native_out(O):
    return (1, O[0], O[0] * O[1])                             # ... and writes the file's [Z][Y][X] grid through


def _poo(t):
    """a tensor of the to_native output layout [O2][O1][O0] as [O0, O1, O2]"""
    return t.permute(2, 1, 0)


# ---- 1. the resampler, exact ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('O', lv.RS_OUTPUTS)
@pytest.mark.parametrize('C', [2, 5, 8])
def test_resample_vote_is_resample_argmax_on_one_hot_channels(C, O):
    src = lv.source_label(tuple(range(C)))                                # [s0, s1, s2]
    M = lv.resample_matrix(S, O)
    voted, keep, nearest = lv.resample_reference(tuple(range(C)), O)
    for layout in ('default', 'to_native'):
        if layout == 'default':
            lab = torch.from_numpy(np.ascontiguousarray(src.transpose(2, 1, 0))).to(DEV)              # [S2][S1][S0]
            kw = {}
        else:
            lab = torch.from_numpy(src).to(DEV)                                                       # [S0][S1][S2], S2 fastest
            kw = dict(src_strides=TO_NATIVE_SRC, out_strides=_to_native_out(O))
        onehot = torch.stack([(lab == c).float() for c in range(C)])
        for lane in (0, 1, 2):
            _, got = data.resample(None, lab, M, O, lane_axis=lane, label_order=1, **kw)
            want, _ = data.resample_argmax(onehot, M, O, lane_axis=lane, **kw)
            assert got.dtype == torch.uint8 and got.shape == want.shape
            assert torch.equal(got, want), (layout, lane)
            if lane == 0:
                first = got
            assert torch.equal(got, first), (layout, lane)                                            # the lane axis changes no byte
        host = (first if layout == 'default' else _poo(first)).cpu().numpy()
        lv.check_case(host, voted, keep, nearest, f'resampler C={C} {O} {layout}')
        _, near = data.resample(None, lab, M, O, **kw)                                                # label_order 0: as it always was
        assert torch.equal(near, data.resample(None, lab, M, O, label_order=0, **kw)[1])
        assert (near != first).float().mean().item() >= lv.MIN_DIFF


def test_resample_vote_into_a_box_view_leaves_the_rest_untouched():
    O = (5, 70, 9)
    src = lv.source_label(lv.ANY_VALUES)
    lab = torch.from_numpy(src).to(DEV)
    M = lv.resample_matrix(S, O)
    X, Y, Z = O[0] + 3, O[1] + 2, O[2] + 4
    big = torch.full((Z, Y, X), 77, device=DEV, dtype=torch.uint8)
    box = big[1:1 + O[2], 2:2 + O[1], 3:3 + O[0]]
    data.resample(None, lab, M, O, src_strides=TO_NATIVE_SRC, out_strides=(1, X, X * Y), out=(None, box), label_order=1)
    _, alone = data.resample(None, lab, M, O, src_strides=TO_NATIVE_SRC, out_strides=_to_native_out(O), label_order=1)
    assert torch.equal(box, alone)
    rest = torch.ones_like(big, dtype=torch.bool)
    rest[1:1 + O[2], 2:2 + O[1], 3:3 + O[0]] = False
    assert (big[rest] == 77).all()
    assert set(torch.unique(alone).tolist()) <= set(lv.ANY_VALUES)


# ---- 2. the resampler, any value -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('O', lv.RS_OUTPUTS)
def test_resample_vote_of_any_u8_values_matches_the_oracle(O):
    src = lv.source_label(lv.ANY_VALUES)
    lab = torch.from_numpy(np.ascontiguousarray(src.transpose(2, 1, 0))).to(DEV)
    M = lv.resample_matrix(S, O)
    _, a = data.resample(None, lab, M, O, label_order=1)
    _, b = data.resample(None, lab, M, O, label_order=1)
    assert torch.equal(a, b)
    lv.check_case(a.cpu().numpy(), *lv.resample_reference(lv.ANY_VALUES, O), f'resampler any value {O}')
    assert set(torch.unique(a).tolist()) == set(lv.ANY_VALUES)
    # beside an image: the image has the bits of the call without label_order, the label the bytes of the label-only call
    img = torch.from_numpy(np.random.RandomState(1).standard_normal(lab.shape).astype(np.float32)).to(DEV)
    for order in (1, 3):
        wi, _ = data.resample(img, lab, M, O, order=order)
        gi, gl = data.resample(img, lab, M, O, order=order, label_order=1)
        assert torch.equal(gi, wi) and torch.equal(gl, a), order


# ---- 3. the gather ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def blob():
    return torch.from_numpy(lv.blob_label()).to(DEV)


@pytest.fixture(scope='module')
def blob_image():
    return torch.from_numpy(np.random.RandomState(2).standard_normal((4,) + lv.BLOB_SCAN).astype(np.float32)).to(DEV)


@pytest.mark.parametrize('size_name', list(lv.SIZES))
@pytest.mark.parametrize('call', list(lv.CALLS))
def test_sample_vote_matches_the_oracle(blob, call, size_name):
    size = lv.SIZES[size_name]
    mats = lv.patch_mats(lv.CALLS[call], size)
    for grid in (None,) + lv.LATTICES[size_name]:
        phi = lv.lattices(size, grid, len(mats)) if grid is not None else None
        _, got = data.sample_affine(None, blob, mats, size, elastic=phi, label_order=1)
        assert got.shape == (len(mats), 1, *size) and got.dtype == torch.uint8
        assert torch.equal(got, data.sample_affine(None, blob, mats, size, elastic=phi, label_order=1)[1])
        host = got.cpu().numpy()[:, 0]
        for i, (name, voted, keep, nearest) in enumerate(lv.gather_reference(call, size_name, grid)):
            lv.check_case(host[i], voted, keep, nearest, f'{call} {size_name} lattice {grid} {name}')
        _, near = data.sample_affine(None, blob, mats, size, elastic=phi)
        assert (near != got).float().mean().item() >= lv.MIN_DIFF
    # the z-decoupled and the general kernel give a shared patch the same bytes
    if call == 'general':
        _, z = data.sample_affine(None, blob, lv.patch_mats(lv.CALLS['zdec'], size), size, label_order=1)
        _, g = data.sample_affine(None, blob, mats, size, label_order=1)
        for name in lv.CALLS['zdec']:
            assert torch.equal(z[lv.CALLS['zdec'].index(name)], g[lv.CALLS['general'].index(name)]), name


@pytest.mark.parametrize('size_name', list(lv.SIZES))
def test_image_beside_a_voted_label_is_untouched(blob, blob_image, size_name):
    size = lv.SIZES[size_name]
    mats = lv.patch_mats(lv.CALLS['general'], size)
    n = len(mats)
    _, voted = data.sample_affine(None, blob, mats, size, label_order=1)
    sg, seeds = np.full(n, 0.1, dtype=np.float32), np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    phi = lv.lattices(size, (4, 4, 4), n)
    _, voted_phi = data.sample_affine(None, blob, mats, size, elastic=phi, label_order=1)
    for img in (blob_image[0].contiguous(), blob_image):                  # K = 1 and K = 4
        for order in (1, (3, 3, 1)):
            kw = dict(fill=-2.0, noise_sigma=sg, seeds=seeds, order=order)
            wi, wl = data.sample_affine(img, blob, mats, size, **kw)
            gi, gl = data.sample_affine(img, blob, mats, size, label_order=1, **kw)
            assert torch.equal(gi, wi) and torch.equal(gl, voted), (order, img.dim())
            assert not torch.equal(gl, wl)
            gi, gl = data.sample_affine(img, blob, mats, size, elastic=phi, label_order=1, **kw)
            assert torch.equal(gi, data.sample_affine(img, blob, mats, size, elastic=phi, **kw)[0]) and torch.equal(gl, voted_phi)


def test_an_integer_matrix_gives_the_nearest_label_bytes(blob):
    for size in ((16, 16, 8), (15, 15, 5)):
        mats = np.stack([data.patch_matrix(st, size, f, k) for st, f, k in (((5, -2, 3), True, 1), ((0, 0, 0), False, 0), ((7, 3, -2), False, 3))])
        _, near = data.sample_affine(None, blob, mats, size)
        _, got = data.sample_affine(None, blob, mats, size, label_order=1)
        assert torch.equal(got, near) and len(torch.unique(got)) == 4
        zero = np.zeros((len(mats), 3, 4, 4, 4), dtype=np.float32)       # a zero lattice: the elastic kernel, the same bytes
        assert torch.equal(data.sample_affine(None, blob, mats, size, elastic=zero, label_order=1)[1], near)


def test_more_patches_than_one_launch_carries(blob):
    size = lv.SIZES['scalar']
    n = _lib.SAMPLE_AFFINE_MAX + 3
    rs = np.random.RandomState(9)
    mats = np.stack([data.patch_matrix(rs.uniform(-3, 8, 3), size, False, 0, (0.0, 0.0, rs.uniform(-1, 1)), rs.uniform(0.7, 1.4)) for _ in range(n)])
    _, got = data.sample_affine(None, blob, mats, size, label_order=1)
    _, near = data.sample_affine(None, blob, mats, size)
    assert got.shape[0] == n and (got != near).float().mean().item() >= lv.MIN_DIFF
    for k in (0, _lib.SAMPLE_AFFINE_MAX - 1, _lib.SAMPLE_AFFINE_MAX, n - 1):
        assert torch.equal(got[k:k + 1], data.sample_affine(None, blob, mats[k:k + 1], size, label_order=1)[1]), k
    one_by_one = torch.cat([data.sample_affine(None, blob, mats[k:k + 1], size, label_order=1)[1] for k in range(n)])
    assert torch.equal(got, one_by_one)


# ---- 4. the scan level -----------------------------------------------------------------------------------------------------------------
def _nifti_pair(tmp_path, affine, margin=0):
    """a 20 x 18 x 9 (x, y, z) image and blob label, stored [Z][Y][X]; margin: that many zero voxels of image around the rest"""
    shape = (9, 18, 20)
    img = (np.random.RandomState(3).uniform(0.5, 1.5, shape)).astype(np.float32)
    if margin:
        keep = np.zeros(shape, dtype=bool)
        keep[1:-1, margin:-margin, margin:-margin - 1] = True
        img[~keep] = 0.0
    lab = lv.blob_label(shape, 4, (0, 1, 2, 3))
    nifti.save(tmp_path / 'img.nii.gz', img, affine)
    nifti.save(tmp_path / 'lab.nii.gz', lab, affine)
    return str(tmp_path / 'img.nii.gz'), str(tmp_path / 'lab.nii.gz'), torch.from_numpy(lab).to(DEV)


ANISO = np.diag([-0.7, -0.8, 2.5, 1.0])
KW = dict(intensity=None, device=DEV)


def test_spaced_scan_label_order(tmp_path):
    ip, lp, rl = _nifti_pair(tmp_path, ANISO, margin=3)
    plain = data.SpacedScan(ip, lp, **KW)
    zero = data.SpacedScan(ip, lp, label_order=0, **KW)
    assert zero.label_order == 0 and plain.label_order == 0
    assert torch.equal(zero.img, plain.img) and torch.equal(zero.lab, plain.lab)
    scan = data.SpacedScan(ip, lp, label_order=1, **KW)
    assert scan.label_order == 1 and scan.shape == plain.shape
    assert torch.equal(scan.img, plain.img)
    _, direct = data.resample(None, rl, scan.matrix, scan.shape, label_order=1)
    assert torch.equal(scan.lab, direct)
    assert (scan.lab != plain.lab).float().mean().item() >= lv.MIN_DIFF
    assert np.array_equal(scan.label_host, scan.lab.cpu().numpy()) and scan.crop_index.counts[:4] == tuple(int((scan.label_host == c).sum()) for c in range(4))
    # crop='nonzero': the label is read from the box
    crop = data.SpacedScan(ip, lp, crop='nonzero', label_order=1, **KW)
    (z0, z1), (y0, y1), (x0, x1) = crop.crop_box
    assert (z1 - z0, y1 - y0, x1 - x0) != tuple(rl.shape)
    Z, Y, X = rl.shape
    _, direct = data.resample(None, rl[z0:z1, y0:y1, x0:x1].permute(2, 1, 0), crop.matrix, crop.shape, src_strides=(1, X, X * Y), label_order=1)
    assert torch.equal(crop.lab, direct)
    assert not torch.equal(crop.lab, data.SpacedScan(ip, lp, crop='nonzero', **KW).lab)
    multi = data.MultiScan([ip, ip], lp, label_order=1, **KW)
    assert multi.label_order == 1 and torch.equal(multi.lab, scan.lab)
    # back to the file's grid by vote: the whole grid and the crop box
    back = data.to_native(scan.lab, scan, order=1)
    want = data.resample(None, scan.lab.contiguous(), geometry.invert(scan.matrix), (X, Y, Z), src_strides=(scan.shape[1] * scan.shape[2], scan.shape[2], 1),
                         out_strides=(1, X, X * Y), label_order=1)[1]
    assert back.shape == (Z, Y, X) and torch.equal(back, want)
    assert not torch.equal(back, data.to_native(scan.lab, scan)) and torch.equal(data.to_native(scan.lab, scan), data.to_native(scan.lab, scan, order=0))
    boxed = data.to_native(crop.lab, crop, order=1)
    outside = torch.ones_like(boxed, dtype=torch.bool)
    outside[z0:z1, y0:y1, x0:x1] = False
    assert boxed.shape == (Z, Y, X) and (boxed[outside] == 0).all() and not torch.equal(boxed, data.to_native(crop.lab, crop))


def test_to_native_by_vote_on_an_identity_spacing_scan_returns_the_stored_label(tmp_path):
    ip, lp, rl = _nifti_pair(tmp_path, np.diag([-0.5, -0.5, 2.0, 1.0]))
    scan = data.SpacedScan(ip, lp, label_order=1, **KW)                  # flips only: an integer matrix
    assert torch.equal(data.to_native(scan.lab, scan, order=1), rl)
    assert torch.equal(scan.lab, data.SpacedScan(ip, lp, **KW).lab)


def test_sample_carries_label_order_into_the_gather(tmp_path):
    ip, lp, _ = _nifti_pair(tmp_path, ANISO)
    scan = data.SpacedScan(ip, lp, **KW)
    size, n = (12, 12, 4), 5
    aug = dict(rot_prob=1.0, zoom_prob=1.0, noise_prob=0.5, blur_prob=0.5)
    a, b, c = (np.random.RandomState(6) for _ in range(3))
    wi, wl = data.sample(scan, size, a, num_samples=n, augment=data.Augmentation(label_order=0, **aug))
    gi, gl = data.sample(scan, size, b, num_samples=n, augment=data.Augmentation(label_order=1, **aug))
    assert torch.equal(gi, wi)
    assert a.get_state()[2] == b.get_state()[2] and np.array_equal(a.get_state()[1], b.get_state()[1])
    draws, params = data.sample_draws(scan, size, c, n, augment=data.Augmentation(label_order=1, **aug))
    mats = np.stack([data.patch_matrix([max(ce[x] - size[x] // 2, 0) for x in range(3)], size, f, k, p['angles'], p['zoom_factor'], scan.pixdim)
                     for (ce, f, k), p in zip(draws, params)])
    _, direct = data.sample_affine(None, scan.lab, mats, size, label_order=1)
    assert torch.equal(gl, direct)
    assert (gl != wl).float().mean().item() >= lv.MIN_DIFF
    # order 3 for the image: the same voted label
    ci, cl = data.sample(scan, size, np.random.RandomState(6), num_samples=n, augment=data.Augmentation(label_order=1, order=3, **aug))
    assert torch.equal(cl, gl) and not torch.equal(ci, gi)


# ---- 5. the ball ---------------------------------------------------------------------------------------------------------------------------
def test_ball_by_vote_is_closer_to_the_direct_ball_than_nearest():
    coarse, fine, _ = lv.ball()
    lab = torch.from_numpy(np.ascontiguousarray(coarse.transpose(2, 1, 0))).to(DEV)
    _, voted = data.resample(None, lab, lv.ball_matrix(), lv.BALL_FINE, label_order=1)
    _, near = data.resample(None, lab, lv.ball_matrix(), lv.BALL_FINE)
    by_vote, by_nearest = int((voted.cpu().numpy() != fine).sum()), int((near.cpu().numpy() != fine).sum())
    print(f'ball 16^3 -> 37^3 on the device: {by_vote} voxels differ from the direct ball by vote, {by_nearest} nearest')
    assert by_vote < by_nearest
    assert by_vote == 671                                                # no voxel of this input lies in the tie band: the oracle's count
