"""The monai driver's data side on the device (csrc/resample.hip): Spacingd + Orientationd as one resampling kernel against
torch's float64 grid_sample (the call monai's AffineTransform makes: align_corners False, border padding, reversed coordinate
order), the crop + flip + rot90 gather against numpy, the label's way back onto the file grid, and the whole driver chain from a
NIfTI pair to a saved prediction."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import data, geometry, nifti  # noqa: E402
from tests.test_nifti_spacing import write_nii  # noqa: E402

DEV = 'cuda'


def _affine(pix, origin=(0.0, 0.0, 0.0), perm=(0, 1, 2), signs=(-1, -1, 1), rot_deg=0.0):
    """file axis i -> world axis perm[i] with sign signs[i] and spacing pix[i], then a rotation about world z"""
    a = np.eye(4)
    a[:3, :3] = 0
    for i in range(3):
        a[perm[i], i] = signs[i] * pix[i]
    c, s = np.cos(np.deg2rad(rot_deg)), np.sin(np.deg2rad(rot_deg))
    r = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    a[:3, :3] = r @ a[:3, :3]
    a[:3, 3] = origin
    return a


def _scan(shape_xyz, dtype, seed):
    """smooth CT-like volume [Z][Y][X] of dtype with a 3-class ellipsoid label"""
    X, Y, Z = shape_xyz
    g = torch.Generator().manual_seed(seed)
    v = F.avg_pool3d(torch.randn((1, 1, Z, Y, X), generator=g, dtype=torch.float64), 3, stride=1, padding=1)[0, 0].numpy()
    v = v / (np.abs(v).max() + 1e-12)
    if dtype == np.uint8:
        raw = np.clip(v * 127 + 128, 0, 255).astype(np.uint8)
    elif dtype == np.int16:
        raw = np.clip(v * 400 + 40, -1024, 3000).astype(np.int16)
    else:
        raw = (v * 300 + 40).astype(np.float32)
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing='ij')
    d = ((xx - 0.45 * X) / (0.3 * X)) ** 2 + ((yy - 0.55 * Y) / (0.3 * Y)) ** 2 + ((zz - 0.5 * Z) / (0.35 * Z)) ** 2
    lab = (d <= 1).astype(np.uint8) + (d <= 0.3).astype(np.uint8)
    return raw, lab


def _mapped(raw, imap):
    alpha, beta, lo, hi = imap
    return np.clip(raw.astype(np.float64) * alpha + beta, lo, hi)


def _ref(src_zyx, M, out_shape, mode):
    """float64 torch grid_sample of src [Z][Y][X] at c = M (p, 1) for every output voxel p, normalised as (2c + 1) / size - 1"""
    O = out_shape
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in O], indexing='ij')
    p = np.stack(list(grids) + [np.ones(O)], 0).reshape(4, -1)
    c = (np.asarray(M, dtype=np.float64) @ p).reshape(3, *O)
    size = np.array(src_zyx.shape[::-1], dtype=np.float64)             # (X, Y, Z)
    g = np.stack([(2 * c[s] + 1) / size[s] - 1 for s in range(3)], -1)  # (x, y, z) = grid_sample's reversed (W, H, D) order
    src = torch.as_tensor(np.asarray(src_zyx, dtype=np.float64))[None, None]
    out = F.grid_sample(src, torch.as_tensor(g)[None], mode=mode, padding_mode='border', align_corners=False)
    return out[0, 0].numpy(), c


def _near_tie(c, size):
    cc = np.stack([np.clip(c[s], 0, size[s] - 1) for s in range(3)])
    f = cc - np.floor(cc)
    return (np.abs(f - 0.5) < 1e-4).any(0)


CASES = {
    'msd': dict(shape=(40, 36, 12), aff=_affine((0.8, 0.8, 2.5), (20.0, 15.0, -30.0)), pixdim=(0.5, 0.5, 2.0)),
    'slices_first': dict(shape=(12, 40, 36), aff=_affine((2.5, 0.8, 0.8), (5.0, -3.0, 7.0), perm=(2, 0, 1), signs=(1, -1, 1)),
                         pixdim=(2.0, 0.5, 0.5)),
    'oblique5': dict(shape=(40, 36, 12), aff=_affine((0.8, 0.8, 2.5), (1.0, 2.0, 3.0), rot_deg=5.0), pixdim=(0.5, 0.5, 2.0)),
    'downsample': dict(shape=(40, 36, 12), aff=_affine((0.8, 0.8, 2.5)), pixdim=(1.6, 1.3, 5.0)),
    'odd': dict(shape=(37, 29, 11), aff=_affine((0.77, 0.81, 2.3), (3.3, -1.1, 0.5)), pixdim=(0.5, 0.5, 2.0)),
}


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.uint8, np.int16, np.float32])
@pytest.mark.parametrize('case', list(CASES))
def test_resample_matches_grid_sample_float64(case, dtype):
    cfg = CASES[case]
    raw, lab = _scan(cfg['shape'], dtype, 11)
    M, out_shape, _ = geometry.spacing_plan(cfg['shape'], cfg['aff'], cfg['pixdim'])
    slope, inter = (1.5, -200.0) if dtype == np.uint8 else (1.0, 0.0)
    imap = data.intensity_map(data.MONAI_CT_WINDOW, slope, inter)
    code = {np.uint8: 2, np.int16: 3, np.float32: 0}[dtype]
    oi, ol = data.resample(torch.as_tensor(raw).to(DEV), torch.as_tensor(lab).to(DEV), M, out_shape, imap, code)
    assert tuple(oi.shape) == tuple(out_shape) and oi.dtype == torch.float32 and ol.dtype == torch.uint8
    want, c = _ref(_mapped(raw, imap), M, out_shape, 'bilinear')
    err = np.abs(oi.cpu().numpy().astype(np.float64) - want).max()
    assert err <= 1e-3, err
    want_l, _ = _ref(lab, M, out_shape, 'nearest')
    diff = ol.cpu().numpy() != want_l.astype(np.uint8)
    assert not (diff & ~_near_tie(c, cfg['shape'])).any(), int(diff.sum())
    # image-only and label-only launches give the fused launch's values
    oi2, _ = data.resample(torch.as_tensor(raw).to(DEV), None, M, out_shape, imap, code)
    _, ol2 = data.resample(None, torch.as_tensor(lab).to(DEV), M, out_shape)
    assert torch.equal(oi2, oi) and torch.equal(ol2, ol)


@pytest.mark.gpu
def test_identity_reproduces_scaled_input():
    raw, lab = _scan((33, 20, 9), np.int16, 5)
    imap = data.intensity_map(data.MONAI_CT_WINDOW)
    M = np.eye(4)[:3]
    oi, ol = data.resample(torch.as_tensor(raw).to(DEV), torch.as_tensor(lab).to(DEV), M, (33, 20, 9), imap, 3)
    np.testing.assert_allclose(oi.cpu().numpy(), _mapped(raw, imap).transpose(2, 1, 0), rtol=0, atol=1e-6)
    assert np.array_equal(ol.cpu().numpy(), lab.transpose(2, 1, 0))


def _ras(raw, aff, pixdim):
    M, shape, out_aff = geometry.spacing_plan(raw.shape[::-1], aff, pixdim)
    oi, _ = data.resample(torch.as_tensor(raw).to(DEV), None, M, shape, data.intensity_map(data.MONAI_CT_WINDOW), 0)
    return oi.cpu().numpy(), out_aff


@pytest.mark.gpu
def test_storage_order_and_flip_invariance():
    """(S - 1) * p_file / p_out is an integer on every axis, so the stored-flipped scan lands on the same output grid"""
    raw, _ = _scan((41, 51, 13), np.float32, 9)
    aff = _affine((0.8, 0.8, 2.5), (10.0, 20.0, -5.0))
    pix = (0.5, 0.5, 2.0)
    base, base_aff = _ras(raw, aff, pix)
    # stored transposed (file x <-> y) with the affine's columns and the target spacing permuted alike
    t_raw = np.ascontiguousarray(raw.transpose(0, 2, 1))
    t_aff = aff.copy()
    t_aff[:, [0, 1]] = aff[:, [1, 0]]
    got, got_aff = _ras(t_raw, t_aff, (pix[1], pix[0], pix[2]))
    assert got.shape == base.shape
    np.testing.assert_allclose(got_aff, base_aff, atol=1e-9)
    np.testing.assert_allclose(got, base, rtol=0, atol=1e-6)
    # stored flipped along x: negated column, origin moved to the old last voxel
    f_raw = np.ascontiguousarray(raw[:, :, ::-1])
    f_aff = aff.copy()
    f_aff[:3, 0] = -aff[:3, 0]
    f_aff[:3, 3] = aff[:3, 3] + aff[:3, 0] * (raw.shape[2] - 1)
    got, got_aff = _ras(f_raw, f_aff, pix)
    assert got.shape == base.shape
    np.testing.assert_allclose(got_aff, base_aff, atol=1e-9)
    np.testing.assert_allclose(got, base, rtol=0, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize('d', [16, 7])                     # 4 depth voxels per lane / one
def test_crop_orient_bit_exact(d):
    H, W, D = 40, 40, 23
    g = torch.Generator().manual_seed(3)
    img = torch.randn((H, W, D), generator=g)
    lab = torch.randint(0, 3, (H, W, D), generator=g, dtype=torch.uint8)
    h = w = 12
    rs = np.random.RandomState(4)
    draws = []
    for flip in (False, True):
        for k in range(4):
            c = [int(rs.randint(h // 2, H - h // 2)), int(rs.randint(w // 2, W - w // 2)), int(rs.randint(d // 2, D - d // 2 + 1))]
            c = data.correct_crop_centers(c, (h, w, d), (H, W, D))
            draws.append((c, flip, k))
    oi, ol = data.crop_orient(img.to(DEV), lab.to(DEV), draws, (h, w, d))
    assert oi.shape == (8, 1, h, w, d) and ol.shape == (8, 1, h, w, d)
    for n, (c, flip, k) in enumerate(draws):
        s = [max(c[0] - h // 2, 0), max(c[1] - w // 2, 0), max(c[2] - d // 2, 0)]
        for vol, out in ((img.numpy(), oi), (lab.numpy(), ol)):
            crop = vol[s[0]:s[0] + h, s[1]:s[1] + w, s[2]:s[2] + d]
            want = np.rot90(np.flip(crop, 0) if flip else crop, k, (0, 1))
            assert np.array_equal(out[n, 0].cpu().numpy(), want), (n, flip, k)
    # k even on a non-square patch
    oi, ol = data.crop_orient(img.to(DEV), None, [([20, 20, 11], True, 2)], (10, 14, d))
    crop = img.numpy()[15:25, 13:27, 11 - d // 2:11 - d // 2 + d]
    assert ol is None and np.array_equal(oi[0, 0].cpu().numpy(), np.rot90(np.flip(crop, 0), 2, (0, 1)))
    with pytest.raises(ValueError):
        data.crop_orient(img.to(DEV), lab.to(DEV), [([20, 20, 11], False, 1)], (10, 14, d))


@pytest.mark.gpu
def test_label_round_trip_on_finer_grid(tmp_path):
    raw, lab = _scan((30, 26, 13), np.int16, 21)
    aff = _affine((1.0, 0.9, 2.5), (4.0, -7.0, 12.0))
    ip = write_nii(tmp_path / 'img.nii.gz', raw, pixdim=(1.0, 0.9, 2.5), sform_code=1, srow=aff[:3])
    lp = write_nii(tmp_path / 'lab.nii.gz', lab, pixdim=(1.0, 0.9, 2.5), sform_code=1, srow=aff[:3])
    scan = data.SpacedScan(ip, lp, pixdim=(0.5, 0.5, 2.0), device=DEV)
    back = data.to_native(scan.lab, scan)
    assert back.shape == (13, 26, 30) and back.dtype == torch.uint8
    assert np.array_equal(back.cpu().numpy(), lab)


@pytest.mark.gpu
def test_driver_chain_nifti_to_saved_prediction(tmp_path):
    """NIfTI pair -> SpacedScan -> two patches -> one train_step of the small 3-class model with the monai driver's level specs ->
    infer_volume on the whole RAS scan -> evaluate_multiclass -> to_native -> save -> load"""
    from lintransunet_amd import infer, train
    from lintransunet_amd.model import get_model_dict
    from oracle import net as O_net, seedgen
    raw, lab = _scan((40, 40, 28), np.int16, 31)
    aff = _affine((0.8, 0.8, 2.5), (100.0, 80.0, -200.0))
    ip = write_nii(tmp_path / 'imagesTr_case.nii.gz', raw, pixdim=(0.8, 0.8, 2.5), qform_code=1, sform_code=1, quatern=(0, 0, 1),
                   qoffset=aff[:3, 3], srow=aff[:3], slope=1.0, inter=0.0)
    lp = write_nii(tmp_path / 'labelsTr_case.nii.gz', lab, pixdim=(0.8, 0.8, 2.5), qform_code=1, sform_code=1, quatern=(0, 0, 1),
                   qoffset=aff[:3, 3], srow=aff[:3])
    scan = data.SpacedScan(ip, lp, device=DEV)
    assert scan.shape == (63, 63, 35) and scan.img.shape == (63, 63, 35)
    assert set(np.unique(scan.label_host).tolist()) == {0, 1, 2}
    x, y = data.sample(scan, (32, 32, 32), np.random.RandomState(0), num_samples=2)
    assert x.shape == (2, 1, 32, 32, 32) and y.shape == (2, 1, 32, 32, 32)

    cfg = O_net.NetConfig(num_layers=[8, 8, 8, 16, 32], roi_size_list=[20, 12, 9, 10, 6], dim_output=3)
    model = get_model_dict('MaskTransUnet')(cfg.num_layers, cfg.roi_size_list, cfg.is_roi_list, 1, 3, dropout=0.0)
    model.load_state_dict(seedgen.seeded_params(O_net.param_shapes(cfg), 51), strict=True)
    model = model.to(DEV).train()
    specs = train.level_specs(5, ('CrossEntroLoss', 'DiceClassLoss', 'DiceClassLoss2'), criterion_weight=[10, 1, 2])
    weights = train.get_dynamic_weight(1, initial_weight=(0.2, 0.2, 0.3, 0.3, 0.4), final_weight=(2., 1.5, 0.5, 0.5, 0.4))[0]
    totals, _ = train.train_step(model, x, y, weights, specs=specs)
    torch.cuda.synchronize()
    assert all(np.isfinite(t.item()) for t in totals)

    predict = infer.infer_volume(model, scan.img[None, None], depth_size=32, roi_xy=32, sw_batch_size=2, overlap=0.6)
    assert predict.shape == (1, 3, 63, 63, 35)
    ev = infer.evaluate_multiclass(predict, scan.lab[None, None], return_label_map=True)
    assert all(np.isfinite(ev[n].item()) for n in ('DiceClassLoss0', 'DiceClassLoss', 'DiceClassLoss2'))
    native = data.to_native(ev['label_map'], scan)
    out = tmp_path / 'pred.nii.gz'
    nifti.save(out, native.cpu().numpy(), scan.native_affine, like=scan.native)
    back = nifti.load(out)
    src = nifti.load(ip)
    assert back.shape == src.shape == (40, 40, 28)
    np.testing.assert_array_equal(back.affine, src.affine)
    assert np.array_equal(back.data, native.cpu().numpy())
