"""Cubic B-spline resampling on the device (csrc/spline.hip) against the float64 oracle of tests/spline_common.py: the prefilter
against scipy's spline_filter1d, the gather against the explicit tap sum, the clamp to the intensity window, the untouched order-1
path, determinism, and the chain from a NIfTI pair to SpacedScan / MultiScan.  Tolerances: spline_common (4 x the deviation of the
float32 oracle from the float64 one, measured on these inputs on the CPU)."""
import numpy as np
import pytest
import torch

from lintransunet_amd import _lib, data, geometry, nifti
from tests import spline_common as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CODE = {'u8': _lib.U8, 'i16': _lib.I16, 'f32': 0}


def _stored(logical):
    """logical [S0, S1, S2] -> the device array as a file stores it, [S2][S1][S0] (x fastest)"""
    return torch.as_tensor(np.ascontiguousarray(np.transpose(logical, (2, 1, 0)))).to(DEV)


def _logical(t):
    """a device result [S2][S1][S0] back as logical float64 numpy [S0, S1, S2]"""
    return t.permute(2, 1, 0).cpu().numpy().astype(np.float64)


@pytest.mark.parametrize('kind', ['u8', 'i16', 'f32'])
@pytest.mark.parametrize('orders', sc.PREFILTER_ORDERS)
@pytest.mark.parametrize('S', sc.PREFILTER_SHAPES)
def test_prefilter_matches_scipy(S, orders, kind):
    raw, imap = sc.raw_scan(S, kind), sc.stored_map(kind)
    v = sc.mapped(raw, imap)
    if v.size >= 100:
        assert (v == imap[2]).any()                                       # the map clips
    want = sc.coefficients(v, orders)
    coef = data.spline_coefficients(_stored(raw), orders, imap, CODE[kind])
    assert coef.dtype == torch.float32 and tuple(coef.shape) == S[::-1] and coef.is_contiguous()
    err = np.abs(_logical(coef) - want).max()
    print(f'prefilter {S} {orders} {kind}: max |c| {np.abs(want).max():.3g}, err {err:.3g}, tol {sc.COEF_TOL:.3g}')
    assert err <= sc.COEF_TOL, err


@pytest.mark.parametrize('S', [(67, 5, 3), (5, 130, 3), (3, 5, 130)])
def test_prefilter_reads_a_permuted_view(S):
    """the source stored with its LAST axis fastest, read through src_strides: the same coefficients, bit for bit"""
    raw, imap = sc.raw_scan(S, 'i16'), sc.stored_map('i16')
    plain = data.spline_coefficients(_stored(raw), (3, 3, 3), imap, _lib.I16)
    view = torch.as_tensor(np.ascontiguousarray(raw)).to(DEV)              # [S0][S1][S2]
    strided = data.spline_coefficients(view, (3, 3, 3), imap, _lib.I16, src_strides=(S[1] * S[2], S[2], 1))
    assert torch.equal(plain, strided)
    assert np.abs(_logical(strided) - sc.coefficients(sc.mapped(raw, imap), (3, 3, 3))).max() <= sc.COEF_TOL


def _run_case(case, orders, lane, **kw):
    cfg = sc.gather_cases()[case]
    v, _ = sc.gather_reference(case, orders)
    out, _ = data.resample(_stored(v), None, cfg['M'], cfg['O'], lane_axis=lane, order=orders, **kw)
    return out


@pytest.mark.parametrize('orders', sc.GATHER_ORDERS)
@pytest.mark.parametrize('case', sc.GATHER_CASES)
def test_gather_matches_oracle(case, orders):
    cfg = sc.gather_cases()[case]
    S, O = cfg['S'], cfg['O']
    assert all(n % 64 for n in O) and max(O) > 64                         # no multiple of the tile, more than one tile
    if case == 'oblique':
        assert 0.18 <= sc.outside_share(cfg['M'], O, S) <= 0.22
    _, want = sc.gather_reference(case, orders)
    for lane, transposed in zip(cfg['lanes'], cfg['transposed']):
        chosen = geometry.lane_axis(cfg['M'], (1, S[0], S[0] * S[1])) if lane is None else lane
        assert (chosen != 2) == transposed                                # the output's fastest axis is its last: both tile paths run
        out = _run_case(case, orders, lane)
        assert tuple(out.shape) == O and out.dtype == torch.float32
        err = np.abs(out.cpu().numpy().astype(np.float64) - want).max()
        print(f'gather {case} {orders} lane {chosen}: max |v| {np.abs(want).max():.3g}, err {err:.3g}, tol {sc.VALUE_TOL:.3g}')
        assert err <= sc.VALUE_TOL, (lane, err)


def test_gather_into_a_strided_output():
    """out_strides of a file's layout (the first axis fastest): the same values as the default layout"""
    cfg = sc.gather_cases()['oblique']
    O = cfg['O']
    v, want = sc.gather_reference('oblique', (3, 3, 3))
    out, _ = data.resample(_stored(v), None, cfg['M'], O, out_strides=(1, O[0], O[0] * O[1]), order=3)
    assert tuple(out.shape) == O[::-1]
    assert np.abs(out.permute(2, 1, 0).cpu().numpy().astype(np.float64) - want).max() <= sc.VALUE_TOL


@pytest.mark.parametrize('S', [(67, 5, 3), (3, 70, 66), (1, 1, 1)])
def test_identity_returns_the_mapped_voxels(S):
    raw, imap = sc.raw_scan(S, 'i16'), sc.stored_map('i16')
    out, _ = data.resample(_stored(raw), None, np.eye(4)[:3], S, imap, _lib.I16, order=3)
    err = np.abs(out.cpu().numpy().astype(np.float64) - sc.mapped(raw, imap)).max()
    assert err <= sc.VALUE_TOL, err


def test_result_stays_inside_the_window():
    """the spline rings past a clipped window; the gather clamps to the map's [lo, hi], which the unclamped oracle leaves"""
    S, O = (37, 41, 29), (70, 45, 33)
    M = sc.gather_cases()['oblique']['M']
    raw, imap = sc.raw_scan(S, 'i16'), sc.stored_map('i16')
    lo, hi = imap[2], imap[3]
    v = sc.mapped(raw, imap)
    free = sc.resample64(v, M, O, (3, 3, 3))
    assert free.min() < lo - 0.05 and free.max() > hi + 0.05              # the input does ring
    out, _ = data.resample(_stored(raw), None, M, O, imap, _lib.I16, order=3)
    got = out.cpu().numpy()
    assert got.min() >= np.float32(lo) and got.max() <= np.float32(hi)
    assert (got == np.float32(lo)).any() and (got == np.float32(hi)).any()
    assert np.abs(got.astype(np.float64) - np.clip(free, lo, hi)).max() <= sc.VALUE_TOL


def test_order_1_is_the_plain_call():
    cfg = sc.gather_cases()['plan']
    S = cfg['S']
    raw, imap = sc.raw_scan(S, 'i16'), sc.stored_map('i16')
    lab = torch.as_tensor((sc.raw_scan(S, 'u8') > 180).astype(np.uint8).transpose(2, 1, 0).copy()).to(DEV)
    src = _stored(raw)
    pi, pl = data.resample(src, lab, cfg['M'], cfg['O'], imap, _lib.I16)
    for order in (1, (1, 1, 1)):
        oi, ol = data.resample(src, lab, cfg['M'], cfg['O'], imap, _lib.I16, order=order)
        assert torch.equal(oi, pi) and torch.equal(ol, pl)
    # the label does not depend on the image's order
    ci, cl = data.resample(src, lab, cfg['M'], cfg['O'], imap, _lib.I16, order=3)
    assert torch.equal(cl, pl) and not torch.equal(ci, pi)


def test_two_calls_agree_bit_for_bit():
    for case in ('oblique', 'plan'):
        for orders in ((3, 3, 3), (3, 3, 0)):
            assert torch.equal(_run_case(case, orders, None), _run_case(case, orders, None))
    raw, imap = sc.raw_scan((67, 5, 3), 'f32'), sc.stored_map('f32')
    assert torch.equal(data.spline_coefficients(_stored(raw), (3, 3, 3), imap), data.spline_coefficients(_stored(raw), (3, 3, 3), imap))


def test_unbuilt_orders_are_refused_with_the_argument_code():
    coef = torch.zeros((4, 4, 4), device=DEV)
    out = torch.empty((4, 4, 4), device=DEV)
    mat = torch.as_tensor(np.eye(4)[:3].ravel().copy()).to(DEV)
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):
        _lib.call('ltu_resample_spline', coef.data_ptr(), 4, 4, 4, 0, 0, 3, out.data_ptr(), 4, 4, 4, 16, 4, 1, mat.data_ptr(), 2,
                  -np.inf, np.inf, torch.cuda.current_stream().cuda_stream)
    with pytest.raises(ValueError):
        data.resample(coef, None, np.eye(4)[:3], (4, 4, 4), order=(0, 0, 3))


AFFINE = sc.affine((0.7, 0.7, 2.5), (20.0, 15.0, -30.0))
PIXDIM = (0.5, 0.5, 2.0)


@pytest.fixture(scope='module')
def nifti_pair(tmp_path_factory):
    """a tiny anisotropic pair, 40 x 36 x 9 at 0.7 / 0.7 / 2.5 mm: two int16-valued images (nifti.save stores what is not uint8 as
    float32) and a label"""
    d = tmp_path_factory.mktemp('spline')
    X, Y, Z = 40, 36, 9
    a = sc.raw_scan((X, Y, Z), 'i16').transpose(2, 1, 0)
    b = sc.raw_scan((X, Y, Z), 'i16', seed=1).transpose(2, 1, 0)
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing='ij')
    lab = (((xx - 18) / 9.0) ** 2 + ((yy - 20) / 8.0) ** 2 + ((zz - 4) / 3.0) ** 2 <= 1).astype(np.uint8)
    paths = {}
    for name, arr in (('a', a), ('b', b), ('lab', lab)):
        paths[name] = str(d / f'{name}.nii.gz')
        nifti.save(paths[name], arr, AFFINE)
    paths['a_logical'] = a.transpose(2, 1, 0)
    return paths


def test_spaced_scan_orders(nifti_pair):
    p = nifti_pair
    plain = data.SpacedScan(p['a'], p['lab'], pixdim=PIXDIM, device=DEV)
    assert plain.order == (1, 1, 1)
    v = sc.mapped(p['a_logical'], data.intensity_map(data.MONAI_CT_WINDOW))
    lo, hi = data.MONAI_CT_WINDOW[2], data.MONAI_CT_WINDOW[3]
    for order, resolved in ((3, (3, 3, 3)), ('auto', (3, 3, 0))):
        scan = data.SpacedScan(p['a'], p['lab'], pixdim=PIXDIM, device=DEV, order=order)
        assert scan.order == resolved and scan.shape == plain.shape
        want = sc.resample64(v, scan.matrix, scan.shape, resolved, lo, hi)
        err = np.abs(scan.img.cpu().numpy().astype(np.float64) - want).max()
        assert err <= sc.VALUE_TOL, (order, err)
        assert torch.equal(scan.lab, plain.lab)
        assert not torch.equal(scan.img, plain.img)
    with pytest.raises(ValueError):
        data.SpacedScan(p['a'], p['lab'], pixdim=PIXDIM, device=DEV, order=2)


def test_multiscan_channels_are_spaced_scans_at_order_3(nifti_pair):
    p = nifti_pair
    ms = data.MultiScan([p['a'], p['b']], p['lab'], pixdim=PIXDIM, device=DEV, order=3)
    assert ms.order == (3, 3, 3)
    for c, name in enumerate(('a', 'b')):
        single = data.SpacedScan(p[name], p['lab'], pixdim=PIXDIM, device=DEV, order=3)
        assert torch.equal(ms.img[c], single.img)
        assert torch.equal(ms.lab, single.lab)
    assert data.MultiScan([p['a']], pixdim=PIXDIM, device=DEV).order == (1, 1, 1)
