"""The nonzero crop on the device (csrc/nonzero.hip, the hole filling of csrc/components.hip; infer.fill_holes, data.nonzero_mask,
data.normalize_masked, SpacedScan / MultiScan(crop='nonzero', intensity='zscore_nonzero'), data.to_native / to_native_probs of a
cropped scan) against scipy / numpy on the host copies.  Masks, boxes, counts and labels are compared exactly, resampled images
bit for bit against data.resample of the same source (resampling is judged in its own tests); normalize_masked within the
roundings of its operands: out = fma(v, fl(alpha), fl(beta)) has three roundings of relative size 2^-24 each (alpha, beta, the
fma), so |out - (v alpha + beta)| <= 3 * 2^-24 * (|v alpha| + |beta|) to first order."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data, geometry, infer, nifti  # noqa: E402
from lintransunet_amd.ops import _p, _s  # noqa: E402
import nonzero_common as nc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- fill_holes -----------------------------------------------------------------------------------------------------------------

_FILLED = {}


def _filled(shape, name, conn, mask):
    """scipy's answer, computed once per case"""
    key = (shape, name, conn)
    if key not in _FILLED:
        _FILLED[key] = nc.fill(mask, conn)
    return _FILLED[key]


@pytest.mark.parametrize('conn', [1, 2, 3])
@pytest.mark.parametrize('shape', nc.SHAPES)
def test_fill_holes_matches_scipy(shape, conn):
    cases = nc.hole_cases(shape)
    names = sorted(cases)
    for name in names:                                                    # B = 1
        got = infer.fill_holes(_dev(cases[name].astype(np.uint8))[None], conn)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1,) + shape
        assert np.array_equal(got[0].cpu().numpy() != 0, _filled(shape, name, conn, cases[name])), name
        assert int(got.max()) <= 1
    for a, b in zip(names, names[1:] + names[:1]):                        # B = 2: two different samples, each filled on its own
        pair = _dev(np.stack([cases[a], cases[b]]).astype(np.uint8))
        got = infer.fill_holes(pair, conn)
        again = infer.fill_holes(pair, conn)
        assert torch.equal(got, again)                                    # integer work only: the same bytes
        g = got.cpu().numpy() != 0
        assert np.array_equal(g[0], _filled(shape, a, conn, cases[a])) and np.array_equal(g[1], _filled(shape, b, conn, cases[b])), (a, b)


def test_fill_holes_takes_any_dtype_and_five_dims_and_works_in_place():
    shape = (33, 17, 40)
    m = nc.hole_cases(shape)['nested']
    want = nc.fill(m, 1)
    for t in (_dev(m), _dev(m.astype(np.float32) * 2.5), _dev(m.astype(np.int32) * -3), _dev(m.astype(np.uint8) * 255)):
        got = infer.fill_holes(t[None], 1)
        assert np.array_equal(got[0].cpu().numpy() != 0, want)
    got = infer.fill_holes(_dev(m.astype(np.uint8))[None, None], 1)      # [B, 1, H, W, D]
    assert tuple(got.shape) == (1,) + shape and np.array_equal(got[0].cpu().numpy() != 0, want)
    inplace = _dev(m.astype(np.uint8))[None].contiguous()
    assert data.fill_holes_u8(inplace, inplace, 1) is inplace            # out == mask is allowed
    assert np.array_equal(inplace[0].cpu().numpy() != 0, want)


def test_fill_holes_refusals_launch_nothing():
    m = torch.zeros((2, 5, 4, 3), device=DEV, dtype=torch.uint8)
    out = torch.full_like(m, 7)
    scratch = torch.empty(120, device=DEV, dtype=torch.int32)
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):                 # a short scratch
        _lib.call('ltu_fill_holes', _p(m), _p(out), _p(scratch), 119, 2, 5, 4, 3, 1, _s())
    with pytest.raises(_lib.LtuError, match='LTU_E_SHAPE'):               # S = 2^31
        _lib.call('ltu_fill_holes', _p(m), _p(out), _p(scratch), 1 << 40, 1, 2048, 1024, 1024, 1, _s())
    with pytest.raises(_lib.LtuError, match='connectivity'):
        infer.fill_holes(m, 0)
    torch.cuda.synchronize()
    assert int(out.min()) == 7 and int(out.max()) == 7                    # nothing was written


# ---- nonzero mask, box and count ------------------------------------------------------------------------------------------------

def _volume(shape, kind, seed, zeros=0.6):
    rs = np.random.RandomState(seed)
    if kind == 'u1':
        v = rs.randint(1, 256, size=shape).astype(np.uint8)
    elif kind == 'i2':
        v = rs.randint(-2000, 2000, size=shape).astype(np.int16)
        v[v == 0] = 5
    else:
        v = rs.normal(0.0, 3.0, shape).astype(np.float32)
        v[v == 0] = 1.0
    v[rs.rand(*shape) < zeros] = 0
    return v


def _check_mask(vols, scalings=None):
    got, box, count = data.nonzero_mask([_dev(v) for v in vols], scalings, fill_holes=False)
    want = nc.union_nonzero(vols, scalings)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want.astype(np.uint8))
    assert (box, count) == nc.box_of(want)


@pytest.mark.parametrize('kind', ['u1', 'i2', 'f4'])
@pytest.mark.parametrize('shape', nc.SHAPES)
def test_nonzero_mask_box_and_count_match_numpy(shape, kind):
    v = _volume(shape, kind, 31)
    _check_mask([v])
    margin = v.copy()                                                     # zeros around a block that ends inside the volume: a proper box
    margin[:1], margin[:, -2:], margin[:, :, :1] = 0, 0, 0
    _check_mask([margin])
    _check_mask([margin], [(-2.0, 0.0)])


@pytest.mark.parametrize('K', [1, 2, 3, 4])
def test_nonzero_mask_accumulates_the_channels(K):
    shape = (37, 29, 23)
    kinds = ['i2', 'f4', 'u1', 'i2'][:K]
    vols = [_volume(shape, kind, 40 + c, zeros=0.85) for c, kind in enumerate(kinds)]
    _check_mask(vols)
    union = nc.union_nonzero(vols)
    assert K == 1 or union.sum() > nc.union_nonzero(vols[:1]).sum()      # the later channels add voxels


def test_nonzero_mask_with_an_intercept_a_nan_and_negative_zero():
    shape = (33, 17, 40)
    v = _volume(shape, 'i2', 50)
    v[3, 4, 5], v[8, 9, 10] = 3, 7
    want = nc.union_nonzero([v], [(1.0, -3.0)])
    assert not want[3, 4, 5] and want[v == 0].all() and want[8, 9, 10]    # the stored 3 is the zero, the stored zeros are not
    _check_mask([v], [(1.0, -3.0)])
    _check_mask([v], [(2.0, -6.0)])
    f = np.zeros(shape, np.float32)
    f[5:9, 3:8, 7:30] = 1.25
    f[20, 11, 33] = np.nan                                                # a NaN counts as nonzero: the box reaches it
    f[1, 1, 1] = -0.0                                                     # -0.0 is zero
    got, box, count = data.nonzero_mask(_dev(f), fill_holes=False)
    assert bool(got[20, 11, 33]) and not bool(got[1, 1, 1])
    assert box == ((5, 21), (3, 12), (7, 34)) and count == 4 * 5 * 23 + 1


@pytest.mark.parametrize('shape', [(5, 4, 3), (33, 17, 40)])
def test_mask_box_of_single_corner_voxels_and_the_empty_sentinel(shape):
    Z, Y, X = shape
    for corner in [(z, y, x) for z in (0, Z - 1) for y in (0, Y - 1) for x in (0, X - 1)]:
        v = np.zeros(shape, np.uint8)
        v[corner] = 200
        _, box, count = data.nonzero_mask(_dev(v), fill_holes=False)
        assert box == tuple((c, c + 1) for c in corner) and count == 1
    both = np.zeros(shape, np.uint8)
    both[0, 0, 0] = both[-1, -1, -1] = 1
    _, box, count = data.nonzero_mask(_dev(both), fill_holes=False)
    assert box == ((0, Z), (0, Y), (0, X)) and count == 2
    empty = torch.zeros((2,) + shape, device=DEV, dtype=torch.uint8)
    empty[1, Z // 2, Y // 2, X // 2] = 1                                  # B = 2: an empty sample beside one voxel
    box = torch.full((2, 6), 99, device=DEV, dtype=torch.int32)
    count = torch.full((2,), 99, device=DEV, dtype=torch.int64)
    _lib.call('ltu_mask_box', _p(empty), 2, Z, Y, X, _p(box), _p(count), _s())
    assert box.cpu().tolist() == [[Z, -1, Y, -1, X, -1], [Z // 2, Z // 2, Y // 2, Y // 2, X // 2, X // 2]]
    assert count.cpu().tolist() == [0, 1]
    with pytest.raises(ValueError, match='no nonzero voxel'):
        data.nonzero_mask(torch.zeros(shape, device=DEV, dtype=torch.int16))


@pytest.mark.parametrize('kind', ['u1', 'i2', 'f4'])
def test_nonzero_kernels_on_unaligned_pointers(kind):
    """views that begin one element into their buffers: the image, the mask, or both are off the 16-byte grid"""
    shape = (37, 29, 23)
    n = int(np.prod(shape))
    v = _volume(shape, kind, 60)
    want = (v != 0).astype(np.uint8)
    code = {'u1': _lib.U8, 'i2': _lib.I16, 'f4': 0}[kind]
    for img_off, mask_off in ((1, 1), (1, 0), (0, 1)):
        buf = torch.zeros(n + 1, device=DEV, dtype=_dev(v).dtype)
        img = buf[img_off:img_off + n]
        img.copy_(_dev(v).reshape(-1))
        mbuf = torch.full((n + 17,), 9, device=DEV, dtype=torch.uint8)
        mask = mbuf[mask_off:mask_off + n]
        _lib.call('ltu_nonzero_mask', _p(img), code, n, 1.0, 0.0, _p(mask), 0, _s())
        assert np.array_equal(mask.cpu().numpy(), want.ravel())
        assert mbuf[:mask_off].eq(9).all() and mbuf[mask_off + n:].eq(9).all()          # not a byte beside the mask is written
        _lib.call('ltu_nonzero_mask', _p(img), code, n, 0.0, 0.0, _p(mask), 1, _s())   # accumulating nothing keeps the mask
        assert np.array_equal(mask.cpu().numpy(), want.ravel())
        box = torch.empty(6, device=DEV, dtype=torch.int32)
        count = torch.empty(1, device=DEV, dtype=torch.int64)
        _lib.call('ltu_mask_box', _p(mask), 1, *shape, _p(box), _p(count), _s())
        (b0, b1, b2), cnt = nc.box_of(want)
        assert box.cpu().tolist() == [b0[0], b0[1] - 1, b1[0], b1[1] - 1, b2[0], b2[1] - 1] and int(count) == cnt


def test_nonzero_mask_fills_the_phantoms_holes():
    vols, _ = nc.head_phantom((24, 30, 36))
    o = nc.oracle(vols)
    mask, box, count = data.nonzero_mask([_dev(v) for v in vols])
    assert np.array_equal(mask.cpu().numpy() != 0, o['mask']) and (box, count) == (o['box'], o['count'])
    again = data.nonzero_mask([_dev(v) for v in vols])
    assert torch.equal(mask, again[0]) and again[1:] == (box, count)


# ---- normalize_masked -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['u1', 'i2', 'f4'])
@pytest.mark.parametrize('shape', nc.SHAPES[:3])
def test_normalize_masked_against_float64(shape, kind):
    Z, Y, X = shape
    v = _volume(shape, kind, 70, zeros=0.1)
    mask = (np.random.RandomState(71).rand(*shape) < 0.7).astype(np.uint8)
    alpha, beta = 1.0 / 37.3, -411.7 / 37.3
    tv, tm = _dev(v), _dev(mask)
    full = ((0, Z), (0, Y), (0, X))
    boxes = [full, ((0, Z - 1), (0, Y - 1), (0, X - 1)), ((1, Z), (1, Y), (1, X)), ((Z - 1, Z), (0, Y), (X - 1, X)),
             ((0, 1), (Y - 1, Y), (0, 1)), ((1, Z - 1), (1, Y - 2), (1, X - 1))]
    for box in boxes:
        sl = nc.box_slices(box)
        got = data.normalize_masked(tv, tm, box, alpha, beta)
        assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == tuple(hi - lo for lo, hi in box)
        g = got.cpu().numpy().astype(np.float64)
        y = v[sl].astype(np.float64)
        ref = np.where(mask[sl] != 0, y * alpha + beta, 0.0)
        bound = 3 * 2.0 ** -24 * (np.abs(y * alpha) + abs(beta))
        assert (np.abs(g - ref) <= bound).all(), (box, np.abs(g - ref).max())
        assert not g[mask[sl] == 0].any()                                 # exactly 0 outside the mask
        assert torch.equal(got, data.normalize_masked(tv, tm, box, alpha, beta))
    with pytest.raises(ValueError, match='box'):
        data.normalize_masked(tv, tm, ((0, Z + 1), (0, Y), (0, X)), alpha, beta)


# ---- scans ----------------------------------------------------------------------------------------------------------------------

# x runs to the left at 0.875 mm, y to the front at 1.125 mm, z up at 2.5 mm: 'LAS', not the RAS the scans are resampled to (the
# numbers are float32 values, as a NIfTI header stores them; the tests plan with the affine the file gives back all the same)
AFFINE = np.array([[-0.875, 0.0, 0.0, 40.0], [0.0, 1.125, 0.0, -20.0], [0.0, 0.0, 2.5, 7.0], [0.0, 0.0, 0.0, 1.0]])
FILE_PIXDIM = (0.875, 1.125, 2.5)
SCAN_SHAPE = (24, 30, 36)                                                 # [Z][Y][X]
PIXDIM = (1.0, 1.0, 2.0)


@pytest.fixture(scope='module')
def phantom(tmp_path_factory):
    d = tmp_path_factory.mktemp('nonzero')
    vols, lab = nc.head_phantom(SCAN_SHAPE)
    nc.save_i16(nifti, str(d / 'c0.nii'), vols[0], AFFINE)
    nifti.save(str(d / 'c1.nii'), vols[1], AFFINE)
    nifti.save(str(d / 'lab.nii'), lab, AFFINE)
    return {'paths': [str(d / 'c0.nii'), str(d / 'c1.nii')], 'lab_path': str(d / 'lab.nii'), 'vols': vols, 'lab': lab,
            'oracle': nc.oracle(vols), 'codes': [_lib.I16, 0], 'affine': nifti.load(str(d / 'c0.nii')).affine}


def _box_plan(ph, box, pixdim=PIXDIM, axcodes='RAS'):
    bshape, baffine = geometry.crop_plan(SCAN_SHAPE[::-1], ph['affine'], box[::-1])
    return geometry.spacing_plan(bshape, baffine, pixdim, axcodes)


def _masked_stats(raw, mask):
    return data.intensity_stats(raw, lab=mask, mask=data.FG_MASK, percentiles=())


def _expected_channel(ph, c, mask, box, matrix, shape, order):
    """(image, window) of channel c as the issue defines them: statistics inside the mask, alpha and beta in float64,
    normalize_masked, then data.resample with the identity map"""
    raw = _dev(ph['vols'][c])
    st = _masked_stats(raw, mask)
    sd = max(st['std'], 1e-8)
    norm = data.normalize_masked(raw, mask, box, 1.0 / sd, (0.0 - st['mean']) / sd, ph['codes'][c])
    img, _ = data.resample(norm, None, matrix, shape, order=order)
    return img, (st['min'], st['max'], (st['min'] - st['mean']) / sd, (st['max'] - st['mean']) / sd)


def _boxed_label(ph, box, matrix, shape):
    lab = _dev(np.ascontiguousarray(ph['lab'][nc.box_slices(box)]))
    return data.resample(None, lab, matrix, shape)[1]


def test_masked_statistics_match_the_oracle(phantom):
    o = phantom['oracle']
    mask, box, count = data.nonzero_mask([_dev(v) for v in phantom['vols']])
    assert (box, count) == (o['box'], o['count'])
    st = _masked_stats(_dev(phantom['vols'][0]), mask)                    # int16: exact integer sums (test_gpu_intensity's tolerance)
    assert st['count'] == count
    assert abs(st['mean'] - o['means'][0]) <= 1e-12 * abs(o['means'][0]) and abs(st['std'] - o['stds'][0]) <= 1e-12 * o['stds'][0]
    st = _masked_stats(_dev(phantom['vols'][1]), mask)                    # float32: fp64 sums in a fixed order
    bound = 2.0 ** -30 * np.abs(phantom['vols'][1].astype(np.float64)[o['mask']]).mean()
    assert st['count'] == count and abs(st['mean'] - o['means'][1]) <= bound and abs(st['std'] - o['stds'][1]) <= bound


@pytest.mark.parametrize('order', [1, 3])
def test_multiscan_cropped_and_normalised_under_the_mask(phantom, order):
    o = phantom['oracle']
    scan = data.MultiScan(phantom['paths'], phantom['lab_path'], pixdim=PIXDIM, intensity='zscore_nonzero', crop='nonzero', order=order)
    assert scan.crop_box == o['box'] and scan.nonzero_count == o['count']
    assert scan.nonzero_fraction == np.prod([hi - lo for lo, hi in o['box']]) / np.prod(SCAN_SHAPE) and scan.nonzero_fraction < 0.75
    assert scan.outside == [0.0, 0.0] and scan.channels == 2
    assert scan.native_shape == SCAN_SHAPE[::-1] and np.array_equal(scan.native_affine, phantom['affine'])      # the file's own
    matrix, shape, affine = _box_plan(phantom, o['box'])
    assert np.array_equal(scan.matrix, matrix) and tuple(scan.shape) == tuple(shape) and np.array_equal(scan.affine, affine)
    assert tuple(scan.img.shape) == (2,) + tuple(shape)
    mask = _dev(o['mask'].astype(np.uint8))
    for c in range(2):
        img, window = _expected_channel(phantom, c, mask, o['box'], matrix, shape, order)
        assert scan.intensity[c] == window
        assert torch.equal(scan.img[c], img), c                           # bit for bit: resampling is not re-judged here
    assert torch.equal(scan.lab, _boxed_label(phantom, o['box'], matrix, shape))
    if order == 1:                                                        # trilinear weights are convex: what was 0 outside the head stays 0
        inside = scan.img[0][scan.lab > 0]
        assert abs(float(inside.mean())) < 2.0 and float(scan.img.abs().max()) < 20.0


def test_zscore_nonzero_without_crop(phantom):
    o = phantom['oracle']
    scan = data.MultiScan(phantom['paths'], phantom['lab_path'], pixdim=PIXDIM, intensity='zscore_nonzero')
    assert scan.crop_box is None and scan.nonzero_count == o['count'] and scan.outside == [0.0, 0.0]
    matrix, shape, affine = geometry.spacing_plan(SCAN_SHAPE[::-1], phantom['affine'], PIXDIM, 'RAS')
    assert np.array_equal(scan.matrix, matrix) and tuple(scan.shape) == tuple(shape)
    full = tuple((0, n) for n in SCAN_SHAPE)
    mask = _dev(o['mask'].astype(np.uint8))
    for c in range(2):
        img, window = _expected_channel(phantom, c, mask, full, matrix, shape, 1)
        assert scan.intensity[c] == window and torch.equal(scan.img[c], img)
    assert torch.equal(scan.lab, _boxed_label(phantom, full, matrix, shape))


def test_crop_with_a_ct_window_and_mixed_specs(phantom):
    o = phantom['oracle']
    window = (100.0, 900.0, 0.0, 1.0)
    scan = data.SpacedScan(phantom['paths'][0], phantom['lab_path'], pixdim=PIXDIM, intensity=window, crop='nonzero')
    # one channel alone: the mask is that channel's own, holes filled (the other channel's voxels are not seen)
    own = nc.oracle(phantom['vols'][:1])
    assert scan.crop_box == own['box'] and scan.nonzero_count == own['count'] and scan.outside is None
    assert scan.intensity == window
    matrix, shape, _ = _box_plan(phantom, own['box'])
    boxed = _dev(np.ascontiguousarray(phantom['vols'][0][nc.box_slices(own['box'])]))      # a dense copy: the scan reads the box through strides
    ref, _ = data.resample(boxed, None, matrix, shape, data.intensity_map(window), _lib.I16)
    assert torch.equal(scan.img, ref) and torch.equal(scan.lab, _boxed_label(phantom, own['box'], matrix, shape))
    matrix, shape, _ = _box_plan(phantom, o['box'])
    boxed = _dev(np.ascontiguousarray(phantom['vols'][0][nc.box_slices(o['box'])]))
    mixed = data.MultiScan(phantom['paths'], None, pixdim=PIXDIM, intensity=[window, 'zscore_nonzero'], crop='nonzero', order=3)
    assert mixed.outside == [None, 0.0] and mixed.lab is None and mixed.intensity[0] == window
    ref3, _ = data.resample(boxed, None, matrix, shape, data.intensity_map(window), _lib.I16, order=3)
    img1, window1 = _expected_channel(phantom, 1, _dev(o['mask'].astype(np.uint8)), o['box'], matrix, shape, 3)
    assert torch.equal(mixed.img[0], ref3) and torch.equal(mixed.img[1], img1) and mixed.intensity[1] == window1


def test_spacedscan_single_channel_zscore_nonzero(phantom):
    own = nc.oracle(phantom['vols'][1:])
    scan = data.SpacedScan(phantom['paths'][1], phantom['lab_path'], pixdim=PIXDIM, intensity='zscore_nonzero', crop='nonzero')
    assert scan.crop_box == own['box'] and scan.nonzero_count == own['count'] and scan.outside == 0.0
    matrix, shape, _ = _box_plan(phantom, own['box'])
    img, window = _expected_channel(phantom, 1, _dev(own['mask'].astype(np.uint8)), own['box'], matrix, shape, 1)
    assert scan.intensity == window and torch.equal(scan.img, img) and tuple(scan.img.shape) == tuple(shape)


def test_the_way_back_fills_the_file_grid(phantom):
    """pixdim = the file's spacing and axcodes = its orientation: resampling is the identity, so the label comes back exactly"""
    o = phantom['oracle']
    scan = data.MultiScan(phantom['paths'], phantom['lab_path'], pixdim=FILE_PIXDIM, axcodes='LAS', intensity='zscore_nonzero',
                          crop='nonzero')
    assert tuple(scan.shape) == tuple(hi - lo for lo, hi in o['box'])[::-1]
    back = data.to_native(scan.lab, scan)
    assert tuple(back.shape) == SCAN_SHAPE and np.array_equal(back.cpu().numpy(), phantom['lab'])    # the zeros outside the box included
    C = 3
    onehot = torch.stack([(scan.lab == k).to(torch.float32) for k in range(C)])
    lab, probs = data.to_native_probs(onehot, scan, classes=(0, 2))
    assert np.array_equal(lab.cpu().numpy(), phantom['lab'])
    p = probs.cpu().numpy()
    outside = np.ones(SCAN_SHAPE, bool)
    outside[nc.box_slices(o['box'])] = False
    assert tuple(p.shape) == (2,) + SCAN_SHAPE and (p[0][outside] == 1.0).all() and not p[1][outside].any()
    assert np.array_equal(p[0], (phantom['lab'] == 0).astype(np.float32)) and np.array_equal(p[1], (phantom['lab'] == 2).astype(np.float32))
    lab_only, none = data.to_native_probs(onehot[None], scan)
    assert none is None and torch.equal(lab_only, lab)


def test_augmented_samples_hold_zero_beyond_the_scan(phantom):
    scan = data.MultiScan(phantom['paths'], phantom['lab_path'], pixdim=PIXDIM, intensity='zscore_nonzero', crop='nonzero')
    floors = [data.intensity_map(w)[2] for w in scan.intensity]
    assert all(f < -1.0 for f in floors)                                  # the z-score of a stored zero: what the fill used to be
    far = data.Augmentation(rot_prob=1, rot_range=(0.0, 0.0, np.pi / 4), zoom_prob=1, zoom_range=(0.3, 0.3), noise_prob=0, blur_prob=0,
                            brightness_prob=0, gamma_prob=0)
    img, _ = data.sample(scan, (12, 12, 8), np.random.RandomState(25), augment=far)
    assert tuple(img.shape) == (1, 2, 12, 12, 8)
    for c in range(2):
        assert int((img[0, c] == 0.0).sum()) > img[0, c].numel() // 4    # rotated and zoomed out: most of the patch lies beyond the scan
        assert int((img[0, c] == np.float32(floors[c])).sum()) == 0
    assert img[0, :, 0, 0, 0].eq(0.0).all() and img[0, :, -1, -1, -1].eq(0.0).all()          # the patch's corners are far outside


def test_defaults_are_the_path_without_crop(phantom):
    a = data.SpacedScan(phantom['paths'][0], phantom['lab_path'], pixdim=PIXDIM)
    b = data.SpacedScan(phantom['paths'][0], phantom['lab_path'], pixdim=PIXDIM, crop=None)
    assert torch.equal(a.img, b.img) and torch.equal(a.lab, b.lab) and a.intensity == b.intensity == data.MONAI_CT_WINDOW
    assert a.crop_box is None and a.nonzero_count is None and a.nonzero_fraction is None and a.outside is None
    raw = _dev(phantom['vols'][0])
    ref, _ = data.resample(raw, None, a.matrix, a.shape, data.intensity_map(data.MONAI_CT_WINDOW), _lib.I16)
    assert torch.equal(a.img, ref) and tuple(data.to_native(a.lab, a).shape) == SCAN_SHAPE
