"""The arg-max on the scan's own grid on the device (csrc/resample.hip ltu_resample_argmax): against the float64 numpy oracle of
tests/native_probs_common.py, bit for bit against the loop it replaces (data.resample per channel + torch.argmax), the tie rule, and
the two callers data.to_native_probs and infer.segment_scan."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import data, geometry, infer, nifti  # noqa: E402
from tests import native_probs_common as nc  # noqa: E402
from tests.test_nifti_spacing import write_nii  # noqa: E402

DEV = 'cuda'
RUNS = [(case, lane, C, kind) for case in nc.CASE_NAMES for lane in nc.cases()[case]['lanes'] for C, kind in nc.INPUTS]


def _call(P, cfg, lane=None, classes=()):
    """resample_argmax in the cases' layouts -> (label, probabilities or None) indexed logically [.., O0, O1, O2]"""
    lab, pr = data.resample_argmax(P, cfg['M'], cfg['O'], src_strides=nc.src_strides(cfg['S']), out_strides=nc.out_strides(cfg['O']),
                                   lane_axis=lane, classes=classes)
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == tuple(cfg['O'][::-1]) and lab.is_contiguous()
    if not classes:
        assert pr is None
        return lab.permute(2, 1, 0), None
    assert pr.dtype == torch.float32 and tuple(pr.shape) == (len(classes),) + tuple(cfg['O'][::-1]) and pr.is_contiguous()
    return lab.permute(2, 1, 0), pr.permute(0, 3, 2, 1)


@pytest.mark.gpu
@pytest.mark.parametrize('case,lane,C,kind', RUNS)
def test_against_float64_and_the_loop(case, lane, C, kind):
    cfg = nc.cases()[case]
    P, want, want_lab, mg = nc.reference(case, C, kind)
    Pd = P.to(DEV)
    lab, pr = _call(Pd, cfg, lane, tuple(range(C)))
    # float64: values within 2e-6, labels equal outside the near-ties, which are few
    err = float(np.abs(pr.cpu().numpy().astype(np.float64) - want).max())
    print(f'{case} lane={lane} C={C} {kind}: max error against float64 {err:.3g}')
    assert err <= nc.VALUE_TOL, err
    sure = mg >= nc.MARGIN
    assert float((~sure).mean()) <= nc.NEAR_TIE_CAP
    assert np.array_equal(lab.cpu().numpy()[sure], want_lab[sure])
    # the loop the call replaces: every channel through ltu_resample_grid with the identity map, then torch.argmax
    chans = [data.resample(Pd[c], None, cfg['M'], cfg['O'], (1.0, 0.0, -np.inf, np.inf), 0, src_strides=nc.src_strides(cfg['S']),
                           out_strides=nc.out_strides(cfg['O']), lane_axis=lane)[0].permute(2, 1, 0) for c in range(C)]
    for c in range(C):
        assert torch.equal(pr[c], chans[c]), c
    assert torch.equal(lab, torch.argmax(torch.stack(chans), 0).to(torch.uint8))
    # labels only, a subset of the classes, a second call
    assert torch.equal(_call(Pd, cfg, lane)[0], lab)
    lab1, pr1 = _call(Pd, cfg, lane, (C - 1,))
    assert torch.equal(lab1, lab) and torch.equal(pr1[0], pr[C - 1])
    lab2, pr2 = _call(Pd, cfg, lane, tuple(range(C)))
    assert torch.equal(lab2, lab) and torch.equal(pr2, pr)


@pytest.mark.gpu
def test_subset_of_classes():
    cfg = nc.cases()['msd']
    P = nc.reference('msd', 3, 'random')[0].to(DEV)
    lab, pr = _call(P, cfg, None, (0, 1, 2))
    lab2, pr2 = _call(P, cfg, None, (2,))
    assert torch.equal(lab2, lab) and pr2.shape[0] == 1 and torch.equal(pr2[0], pr[2])
    lab02, pr02 = _call(P, cfg, None, (2, 0))                      # ascending class order, whatever order is asked for
    assert torch.equal(lab02, lab) and torch.equal(pr02[0], pr[0]) and torch.equal(pr02[1], pr[2])
    with pytest.raises(ValueError):
        _call(P, cfg, None, (3,))


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['msd', 'slices_first'])          # through LDS / straight stores
def test_exact_ties(case):
    """two channels identically 0.5 over a block and a third smaller there: the first of the tied pair wins inside the block"""
    cfg = nc.cases()[case]
    S = cfg['S']
    g = torch.Generator().manual_seed(7)
    base = torch.rand((3,) + S, generator=g) * 0.4                 # below 0.5 everywhere
    blk = (slice(20, 90), slice(15, 95), slice(2, 9))
    c = nc.coords(cfg['M'], cfg['O'])
    inside = np.ones(cfg['O'], dtype=bool)                          # output voxels whose eight taps all lie in the block
    for s in range(3):
        inside &= (c[s] >= blk[s].start) & (c[s] <= blk[s].stop - 1)
    assert inside.mean() > 0.2
    inside = torch.as_tensor(inside)
    for tied, first in (((0, 1), 0), ((1, 2), 1), ((0, 2), 0)):
        P = base.clone()
        for k in tied:
            P[k][blk] = 0.5
        lab, pr = _call(P.to(DEV), cfg, None, (0, 1, 2))
        lab, pr = lab.cpu(), pr.cpu()
        assert torch.equal(pr[tied[0]][inside], pr[tied[1]][inside])         # the weights sum the same constant: an exact tie
        assert bool((lab[inside] == first).all()), (tied, first)
        P = P.flip(0)                                                          # channel k becomes 2 - k
        lab = _call(P.to(DEV), cfg)[0].cpu()
        assert bool((lab[inside] == min(2 - tied[0], 2 - tied[1])).all()), tied


@pytest.mark.gpu
@pytest.mark.parametrize('C', [2, 5, 6, 8])                 # label-only calls change kernels between 5 and 6 classes
def test_identity_matrix(C):
    S = (70, 9, 67)
    P = nc.make_probs(C, S, 'random', seed=3).to(DEV)
    M = np.eye(4)[:3]
    for lane in (0, 2):
        lab, pr = data.resample_argmax(P, M, S, src_strides=nc.src_strides(S), out_strides=nc.out_strides(S), lane_axis=lane,
                                       classes=range(C))
        assert torch.equal(pr.permute(0, 3, 2, 1), P)
        assert torch.equal(lab.permute(2, 1, 0), torch.argmax(P, 0).to(torch.uint8))
    # the default layouts of data.resample: the source an [S2][S1][S0] array per channel, the output [O0][O1][O2]
    lab, pr = data.resample_argmax(P, M, S[::-1], classes=(1,))
    assert tuple(lab.shape) == S[::-1] and torch.equal(pr[0].permute(2, 1, 0), P[1])
    assert torch.equal(lab.permute(2, 1, 0), torch.argmax(P, 0).to(torch.uint8))
    lab = data.resample_argmax(P, M, S[::-1])[0]                   # labels only
    assert torch.equal(lab.permute(2, 1, 0), torch.argmax(P, 0).to(torch.uint8))


def _pair(tmp_path, shape_xyz=(70, 66, 9)):
    X, Y, Z = shape_xyz
    g = torch.Generator().manual_seed(17)
    raw = (torch.randn((Z, Y, X), generator=g) * 200 + 40).numpy().astype(np.int16)
    aff = nc.affine((0.8, 0.8, 2.5), (20.0, 15.0, -30.0))
    return write_nii(tmp_path / 'img.nii.gz', raw, pixdim=(0.8, 0.8, 2.5), sform_code=1, srow=aff[:3])


@pytest.mark.gpu
def test_to_native_probs_on_a_scan(tmp_path):
    ip = _pair(tmp_path)
    scan = data.SpacedScan(ip, device=DEV)
    assert scan.shape == (111, 105, 11) and scan.native_shape == (70, 66, 9)
    P = nc.make_probs(3, scan.shape, 'smooth', seed=5).to(DEV)
    lab, pr = data.to_native_probs(P, scan, classes=(1, 2))
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == (9, 66, 70) and lab.is_contiguous()
    assert pr.dtype == torch.float32 and tuple(pr.shape) == (2, 9, 66, 70)
    H, W, D = scan.shape
    X, Y, Z = scan.native_shape
    lab2, pr2 = data.resample_argmax(P, geometry.invert(scan.matrix), (X, Y, Z), src_strides=(W * D, D, 1), out_strides=(1, X, X * Y),
                                     classes=(1, 2))
    assert torch.equal(lab, lab2) and torch.equal(pr, pr2)
    lab3, none = data.to_native_probs(P[None], scan)               # a leading batch axis of one; labels only
    assert none is None and torch.equal(lab3, lab)
    want = nc.argmax_first(nc.sample64(P.cpu().numpy(), geometry.invert(scan.matrix), (X, Y, Z)))
    assert (lab.permute(2, 1, 0).cpu().numpy() != want).mean() <= nc.NEAR_TIE_CAP
    out = tmp_path / 'pred.nii.gz'
    nifti.save(out, lab.cpu().numpy(), scan.native_affine, like=scan.native)
    back = nifti.load(out)
    assert back.shape == (70, 66, 9) and np.array_equal(back.data, lab.cpu().numpy())
    np.testing.assert_array_equal(back.affine, nifti.load(ip).affine)


@pytest.mark.gpu
def test_segment_scan(tmp_path):
    from lintransunet_amd.model import get_model_dict
    from oracle import net as O_net, seedgen
    ip = _pair(tmp_path, (26, 24, 14))                            # RAS 41 x 38 x 17: four windows of 32 x 32 x 32
    scan = data.SpacedScan(ip, device=DEV)
    assert scan.shape == (41, 38, 17), scan.shape
    cfg = O_net.NetConfig(num_layers=[8, 8, 8, 16, 32], roi_size_list=[20, 12, 9, 10, 6], dim_output=3)
    model = get_model_dict('MaskTransUnet')(cfg.num_layers, cfg.roi_size_list, cfg.is_roi_list, 1, 3, dropout=0.0)
    model.load_state_dict(seedgen.seeded_params(O_net.param_shapes(cfg), 51), strict=True)
    model = model.to(DEV)
    kw = dict(depth_size=32, roi_xy=32, sw_batch_size=4, overlap=0.6)
    probs = infer.infer_volume(model, scan.img[None, None], probs=True, mode='gaussian', mirror_axes=(0, 1), **kw)
    want_lab, want_pr = data.to_native_probs(probs[0], scan, classes=(1,))
    lab, pr = infer.segment_scan(model, scan, **kw)
    assert pr is None and tuple(lab.shape) == (14, 24, 26) and torch.equal(lab, want_lab)
    lab2, pr2 = infer.segment_scan([model, model], scan, **kw)     # p + p is exact
    assert pr2 is None and torch.equal(lab2, want_lab)
    lab3, pr3 = infer.segment_scan([model, model], scan, classes=(1,), **kw)          # (p + p) / 2 is exact
    assert torch.equal(lab3, want_lab) and torch.equal(pr3, want_pr)
    lab4, _ = infer.segment_scan(model, scan, mode='constant', mirror_axes=(), **kw)  # the keywords reach infer_volume
    plain = infer.infer_volume(model, scan.img[None, None], probs=True, **kw)
    assert torch.equal(lab4, data.to_native_probs(plain, scan)[0])
