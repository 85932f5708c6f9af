"""The intensity fingerprint on the device (csrc/intensity.hip; data.intensity_histogram, intensity_stats, IntensityFingerprint,
SpacedScan(intensity=)) against numpy on the host copies.  Histograms, counts, order statistics and percentiles are compared
exactly; the fp64 moments of float scans within the bound of an fp64 sum."""
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import data, nifti  # noqa: E402
import intensity_common as ic  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(5, 4, 3), (37, 29, 23), (32, 16, 16), (96, 96, 40)]      # a partial chunk; a ragged tail; exact multiples; many workgroups
MASKS = [None, data.FG_MASK, data.BG_MASK, 1 << 2, 1 << 8]


def _contents(shape, dtype):
    if dtype == np.uint8:
        return {'uniform': np.random.RandomState(11).randint(0, 256, size=shape).astype(np.uint8),
                'ct_like': np.clip(ic.ct_like(shape, 12) // 8 + 128, 0, 255).astype(np.uint8),
                'equal': np.full(shape, 77, np.uint8)}
    return {'uniform': ic.uniform_i16(shape, 11), 'ct_like': ic.ct_like(shape, 12), 'equal': np.full(shape, -1024, np.int16),
            'lowest': np.full(shape, -32768, np.int16), 'highest': np.full(shape, 32767, np.int16)}


def _reference(x, lab, mask):
    sel = slice(None) if mask is None else ic.selected(lab, mask)
    return ic.bincount(x.ravel()[sel], 0 if x.dtype == np.uint8 else -32768)


def _hist(x, lab, mask):
    h, rejected = data.intensity_histogram(torch.from_numpy(x).to(DEV), None if mask is None else torch.from_numpy(lab).to(DEV),
                                           data.FG_MASK if mask is None else mask)
    assert h.dtype == torch.int64 and tuple(h.shape) == (65536,) and rejected == 0
    return h.cpu().numpy()


@pytest.mark.parametrize('dtype', [np.int16, np.uint8], ids=['i16', 'u8'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_histogram_equals_bincount(shape, dtype):
    lab = ic.labels(shape, 13)
    for name, x in _contents(shape, dtype).items():
        for mask in MASKS:
            assert np.array_equal(_hist(x, lab, mask), _reference(x, lab, mask)), (name, mask)


@pytest.mark.parametrize('shape', SHAPES[:2] + SHAPES[3:], ids=lambda s: 'x'.join(str(v) for v in s))
def test_single_voxel_and_empty_selections(shape):
    x = ic.uniform_i16(shape, 14)
    n = x.size
    for at in (0, n - 1):
        lab = np.zeros(shape, np.uint8)
        lab.ravel()[at] = 3
        h = _hist(x, lab, data.FG_MASK)
        assert h.sum() == 1 and h[int(x.ravel()[at]) + 32768] == 1
    assert not _hist(x, np.zeros(shape, np.uint8), data.FG_MASK).any()          # an all-background label: count 0, no bin touched
    fp = data.IntensityFingerprint()
    fp.add_arrays(torch.from_numpy(x).to(DEV), torch.zeros(shape, dtype=torch.uint8, device=DEV))
    assert (fp.scans, fp.empty_scans) == (1, 1)


@pytest.mark.parametrize('dtype,poison', [(np.int16, 31000), (np.uint8, 255), (np.float32, 31000.0)], ids=['i16', 'u8', 'f32'])
def test_repeatable_and_blind_beyond_n(dtype, poison):
    shape = (37, 29, 23)                               # 24 679 voxels: the last chunk holds 7 of them
    x = ic.ct_like(shape, 15)
    x = np.clip(x // 8 + 128, 0, 200).astype(np.uint8) if dtype == np.uint8 else x.astype(dtype)
    lab = ic.labels(shape, 16)
    n = x.size
    bx = torch.full((n + 64,), poison, dtype=torch.from_numpy(x).dtype, device=DEV)
    bl = torch.full((n + 64,), 1, dtype=torch.uint8, device=DEV)                 # the poison would be selected
    bx[:n], bl[:n] = torch.from_numpy(x.ravel()).to(DEV), torch.from_numpy(lab.ravel()).to(DEV)
    for lb, mask in ((None, data.FG_MASK), (bl[:n], data.FG_MASK), (bl[:n], 1 << 1)):
        a, ra = data.intensity_histogram(bx[:n], lb, mask)
        b, rb = data.intensity_histogram(bx[:n], lb, mask)
        assert torch.equal(a, b) and ra == rb == 0
        ref = _reference(x.astype(np.int16) if dtype == np.float32 else x, lab, None if lb is None else mask)
        assert np.array_equal(a.cpu().numpy(), ref)
        assert ref[int(poison) + (0 if dtype == np.uint8 else 32768)] == 0        # the poison's bin is otherwise empty


def test_f32_int_histogram_and_rejects():
    shape = (37, 29, 23)
    x = ic.ct_like(shape, 17)
    lab = ic.labels(shape, 18)
    xf = x.astype(np.float32)
    for mask in (None, data.FG_MASK):
        assert np.array_equal(_hist(xf, lab, mask), _reference(x, lab, mask))
    bad = xf.copy()
    at = [3, 1000, x.size - 2]
    bad.ravel()[at] = [0.5, 40000.0, np.nan]
    h, rejected = data.intensity_histogram(torch.from_numpy(bad).to(DEV))
    assert rejected == 3
    assert np.array_equal(h.cpu().numpy(), ic.bincount(np.delete(x.ravel(), at), -32768))
    with pytest.raises(ValueError, match='zscore'):
        data.IntensityFingerprint().add_arrays(torch.from_numpy(bad).to(DEV))


def _float_cases():
    rs = np.random.RandomState(19)
    normal = rs.normal(0.0, 1.0, (96, 96, 40)).astype(np.float32)              # 368 640 voxels
    ties = rs.normal(0.0, 1.0, 1001).astype(np.float32)
    ties[:420] = 0.25                                  # a block of ties across the ranks of 37.3 % and 50 %
    ties[420:440] = [0.0, -0.0] * 10
    ties[440:460] = np.array([1e-40, -1e-40, 3e-45, -3e-45] * 5, np.float32)  # denormals
    apart = np.array([-3.0] * 5 + [1.0e6] * 5, np.float32)                     # the median's two order statistics: -3 and 1e6
    return {'normal': normal, 'ties': rs.permutation(ties), 'apart': rs.permutation(apart), 'equal': np.full((37, 29, 23), 2.5, np.float32)}


FLOATS = _float_cases()


def _check_float_stats(got, x, slope=1.0, inter=0.0):
    y = x.astype(np.float64).ravel() * slope + inter
    ref = ic.numpy_stats(y, ic.PERCENTILES)
    assert got['count'] == ref['count'] and got['min'] == ref['min'] and got['max'] == ref['max']
    assert got['percentiles'] == ref['percentiles']                     # bit for bit np.percentile of the float64 values
    bound = 2.0 ** -30 * np.abs(y).mean()              # an fp64 sum of N <= 2^20 terms in any order: N 2^-52, a factor 4 to spare
    assert abs(got['mean'] - ref['mean']) <= bound and abs(got['std'] - ref['std']) <= bound


@pytest.mark.parametrize('name', sorted(FLOATS))
def test_float_stats_against_numpy(name):
    x = FLOATS[name]
    t = torch.from_numpy(x).to(DEV)
    got = data.intensity_stats(t, percentiles=ic.PERCENTILES)
    _check_float_stats(got, x)
    assert got == data.intensity_stats(t, percentiles=ic.PERCENTILES)           # fixed-order sums: the same bits again


def test_float_stats_under_a_label_and_a_negative_slope():
    x = FLOATS['normal']
    lab = ic.labels(x.shape, 20)
    t, lb = torch.from_numpy(x).to(DEV), torch.from_numpy(lab).to(DEV)
    _check_float_stats(data.intensity_stats(t, lb, 1 << 2, ic.PERCENTILES), x.ravel()[ic.selected(lab, 1 << 2)])
    _check_float_stats(data.intensity_stats(t, percentiles=ic.PERCENTILES, slope=-2.0, inter=3.0), x, -2.0, 3.0)
    empty = data.intensity_stats(t, torch.zeros_like(lb), data.FG_MASK)
    assert empty['count'] == 0 and np.isnan(empty['mean'])


def test_float_stats_refuse_non_finite():
    x = FLOATS['ties'].copy()
    x[17] = np.nan
    with pytest.raises(ValueError, match='non-finite'):
        data.intensity_stats(torch.from_numpy(x).to(DEV))


@pytest.mark.parametrize('slope,inter', [(3.0, -1024.0), (-1.5, 200.0)])
def test_integer_stats_with_slope_and_intercept(slope, inter):
    x = ic.ct_like((37, 29, 23), 21)
    got = data.intensity_stats(torch.from_numpy(x).to(DEV), percentiles=ic.PERCENTILES, slope=slope, inter=inter)
    ref = ic.numpy_stats(x.astype(np.float64) * slope + inter, ic.PERCENTILES)
    assert (got['count'], got['min'], got['max'], got['percentiles']) == (ref['count'], ref['min'], ref['max'], ref['percentiles'])
    assert abs(got['mean'] - ref['mean']) <= 1e-12 * abs(ref['mean']) and abs(got['std'] - ref['std']) <= 1e-12 * ref['std']


# ---- end to end: files -> fingerprint -> SpacedScan -> sample --------------------------------------------------------------------

AFFINE = np.diag([0.8, 0.8, 2.5, 1.0])


def _save_i16(path, vol_zyx, inter=0.0):
    """nifti.save writes float32: its header is kept, the datatype, the intercept and the voxels are replaced by int16 ones"""
    nifti.save(path, vol_zyx.astype(np.float32), AFFINE)
    with open(path, 'rb') as f:
        hdr = bytearray(f.read()[:352])
    struct.pack_into('<2h', hdr, 70, 4, 16)
    struct.pack_into('<2f', hdr, 112, 1.0, inter)
    with open(path, 'wb') as f:
        f.write(bytes(hdr) + vol_zyx.astype('<i2').tobytes())


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp('intensity')
    shape = (20, 36, 40)                                # [Z][Y][X] of a (40, 36, 20) scan
    a = ic.ct_like(shape, 22)
    b = (ic.ct_like(shape, 23) + 1024).astype(np.int16)              # stored without the intercept: values v + 1024, scl_inter -1024
    labs = []
    for k, (vol, inter) in enumerate(((a, 0.0), (b, -1024.0))):
        lab = np.zeros(shape, np.uint8)
        lab[6:14, 10:26, 12:30] = 1 + k
        _save_i16(str(d / f'img{k}.nii'), vol, inter)
        nifti.save(str(d / f'lab{k}.nii'), lab, AFFINE)
        labs.append(lab)
    scaled_fg = np.concatenate([a[labs[0] > 0].astype(np.int64), b[labs[1] > 0].astype(np.int64) - 1024])
    return d, scaled_fg


def test_fingerprint_of_files_and_the_scan_it_normalises(files):
    d, scaled_fg = files
    fp = data.IntensityFingerprint()
    for k in range(2):
        fp.add(str(d / f'img{k}.nii'), str(d / f'lab{k}.nii'))
    assert np.array_equal(fp.hist.cpu().numpy(), ic.bincount(scaled_fg, -32768)) and (fp.scans, fp.empty_scans) == (2, 0)
    assert fp.stats((0.5, 50.0, 99.5)) == data.histogram_stats(ic.bincount(scaled_fg, -32768))
    by_fp = data.SpacedScan(str(d / 'img1.nii'), str(d / 'lab1.nii'), intensity=fp)
    by_window = data.SpacedScan(str(d / 'img1.nii'), str(d / 'lab1.nii'), intensity=fp.window())
    assert by_fp.intensity == fp.window() and torch.equal(by_fp.img, by_window.img)


def test_zscore_scan_and_its_augmented_samples(files):
    d, _ = files
    path, lab = str(d / 'img1.nii'), str(d / 'lab1.nii')
    scan = data.SpacedScan(path, lab, pixdim=(0.8, 0.8, 2.5), axcodes='RAS', intensity='zscore')
    assert isinstance(scan.intensity, tuple) and len(scan.intensity) == 4 and tuple(scan.shape) == (40, 36, 20)
    ni = nifti.load(path)
    raw = torch.from_numpy(np.ascontiguousarray(ni.data)).to(DEV)
    ref, _ = data.resample(raw, None, scan.matrix, scan.shape, data.intensity_map(scan.intensity, ni.slope, ni.inter), 3)
    assert torch.equal(scan.img, ref)
    v = scan.img.cpu().numpy().astype(np.float64)
    assert abs(v.mean()) <= 1e-4 and abs(v.std() - 1.0) <= 1e-4
    fill = data.intensity_map(scan.intensity)[2]
    img, _ = data.sample(scan, (16, 16, 8), np.random.RandomState(24), num_samples=2, augment=data.Augmentation())
    assert tuple(img.shape) == (2, 1, 16, 16, 8) and bool(torch.isfinite(img).all())
    # zoomed out to 0.3 and nothing else: most of the patch lies outside the scan and holds the fill value
    far = data.Augmentation(rot_prob=0, zoom_prob=1, zoom_range=(0.3, 0.3), noise_prob=0, blur_prob=0, brightness_prob=0, gamma_prob=0)
    img, _ = data.sample(scan, (16, 16, 8), np.random.RandomState(25), augment=far)
    assert int((img == np.float32(fill)).sum()) > img.numel() // 4
