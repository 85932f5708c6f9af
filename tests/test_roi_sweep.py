"""The ROI case family of tests/roi_common.py on the CPU: it reaches every branch of the box finder (asserted on oracle.roi alone,
before any kernel is involved), the oracle equals the reference's fixture tests/golden/roi_sweep.npz bit for bit on it, and so does
the scalar float32 replay of the two index maps, which writes the rounding order of csrc/roi.hip down once in executable form."""
import functools
import os

import numpy as np
import torch

from oracle import roi as O_roi
from tests import roi_common as RC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
AXES = ('h', 'w')
MIN_COUNT = 5


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(GOLDEN, 'roi_sweep.npz')))


@functools.lru_cache(maxsize=None)
def family():
    """[(g, j, ks, C, thr, prob [8, H, W, D, C], reference mask [8, 1, H, W, D])]"""
    out = []
    for g, j, ks, C, thr in RC.batches():
        prob = RC.make_batch(g, ks, C, thr)
        out.append((g, j, ks, C, thr, prob, RC.reference_mask(prob, thr)))
    return out


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def axis_branches(hist, full, min_len):
    """which branches of occupancy_quantiles / _fit_extent one axis of one case takes, from the oracle's own quantiles"""
    lo, hi, c = O_roi.occupancy_quantiles(hist)
    size = float(torch.as_tensor(hi).float() - torch.as_tensor(lo).float())
    pad, shrink = size < min_len, size > full - min_len
    out = {'both' if pad and shrink else 'pad only' if pad else 'shrink only' if shrink else 'neither'}
    if pad or shrink:
        half = (full - min_len) / 2 if shrink else min_len / 2
        if float(c) - half < 0:
            out.add('x0 clamped to 0')
        if float(c) + half > full:
            out.add('x1 clamped to full')
    nz = torch.nonzero(hist).reshape(-1)
    if len(nz):
        if int(lo) != int(nz[0]):
            out.add('lo trimmed')
        if int(hi) != int(nz[-1]):
            out.add('hi trimmed')
        if int(lo) > int(nz[0]) and int(hi) < int(nz[-1]) and int(hist.sum()) > 3000:
            out.add('lo and hi inside the outliers of a body of more than 3000 voxels')
    else:
        out.add('empty')
    return out


def test_family_reaches_every_branch():
    want = ('pad only', 'shrink only', 'both', 'neither', 'x0 clamped to 0', 'x1 clamped to full', 'lo trimmed', 'hi trimmed')
    count = {ax: {k: 0 for k in want + ('empty', 'lo and hi inside the outliers of a body of more than 3000 voxels')} for ax in AXES}
    pkinds, classes, thrs, n_nan, n_edge = set(), set(), set(), 0, 0
    for g, j, ks, C, thr, prob, mask in family():
        H, W, D, roi_size = RC.GEOMETRIES[g]
        geo = O_roi.roi_geometry(roi_size)
        assert geo == RC.roi_sizes(roi_size)
        assert prob.shape == (RC.BATCH, H, W, D, C) and prob.dtype == torch.float32
        classes.add(C)
        thrs.add(thr)
        p0 = prob[..., 0]
        n_nan += int(torch.isnan(p0).sum())
        n_edge += int(((1 - p0) == torch.tensor(thr, dtype=torch.float32)).sum())
        for b, k in enumerate(ks):
            target, _ = RC.make_case(g, k, C, thr)
            nan = torch.isnan(p0[b])
            assert torch.equal(mask[b, 0] | nan, torch.from_numpy(target) | nan), (g, k)       # the probabilities realise the mask
            assert not (mask[b, 0] & nan).any()                                                   # NaN is background
            pkinds.add(RC.PKINDS[(g + k) % len(RC.PKINDS)])
            for ax, hist, full, min_len in (('h', mask[b].sum(dim=(2, 3)).reshape(H), H, geo['min_h']),
                                            ('w', mask[b].sum(dim=(1, 3)).reshape(W), W, geo['min_w'])):
                for br in axis_branches(hist, full, min_len):
                    count[ax][br] += 1
        box = O_roi.find_boxes(mask, geo['min_h'], geo['min_w'])
        x0, y0, _, x1, y1, _ = torch.split(box, 1, dim=1)
        for m in (O_roi.index_map_fwd(x0, x1, H - 1, geo['h_roi'], geo['eval_h']), O_roi.index_map_fwd(y0, y1, W - 1, geo['w_roi'], geo['eval_w']),
                  O_roi.index_map_back(x0, x1, H - 1, geo['h_roi'], geo['eval_h']), O_roi.index_map_back(y0, y1, W - 1, geo['w_roi'], geo['eval_w'])):
            assert torch.isfinite(m).all(), (g, j)
        assert len({tuple(r.tolist()) for r in box}) >= 4, (g, j)           # a batch mixes boxes
    print('branch counts', count)
    for ax in AXES:
        for k in want:
            assert count[ax][k] >= MIN_COUNT, (ax, k, count[ax])
        assert count[ax]['lo and hi inside the outliers of a body of more than 3000 voxels'] >= 1, count[ax]
        assert count[ax]['empty'] >= 1
    assert pkinds == set(RC.PKINDS) and classes == {2, 3, 8} and thrs == {RC.THR_DEFAULT, RC.THR_OTHER[2]}
    assert n_nan > 0 and n_edge > 1000
    blocks = [max(1, min(256, H * W * D // 4096)) for H, W, D, _ in RC.GEOMETRIES]
    assert any(n > 1 and (-(-H * W * D // n)) % (W * D) for n, (H, W, D, _) in zip(blocks, RC.GEOMETRIES))      # a block ends inside a row
    assert any(n == 1 for n in blocks)


def test_threshold_neighbours_are_the_nearest_reachable_values():
    for thr in (RC.THR_DEFAULT, RC.THR_OTHER[2]):
        t = np.float32(thr)
        at, above, below = RC.threshold_neighbours(thr)
        assert np.float32(1) - at == t
        # p0 lies in [0.5, 1), where float32 values are 2^-24 apart: no reachable 1 - p0 is further than that from thr
        assert 0 < np.float64(np.float32(1) - above) - np.float64(t) <= 2.0 ** -24
        assert 0 < np.float64(t) - np.float64(np.float32(1) - below) <= 2.0 ** -24
        if thr == 0.5:
            assert np.float32(1) - above == np.nextafter(t, np.float32(1))          # one ulp above
        got = RC.fg_of_p0(np.array([at, above, below, np.nan], np.float32), thr)
        assert got.tolist() == [True, True, False, False]
        ref = RC.reference_mask(torch.tensor([at, above, below, float('nan')]).reshape(1, 4, 1, 1, 1), thr)
        assert ref.reshape(-1).tolist() == [True, True, False, False]


def test_oracle_equals_reference_on_family():
    """oracle.roi.find_boxes, index_map_fwd and index_map_back against the reference's get_mask_boundary2, get_transfer_index and
    get_transfer_back_index (tests/golden/make_golden_roi_sweep.py), bit for bit"""
    Gd = fixture()
    for g, j, ks, C, thr, prob, mask in family():
        H, W, D, roi_size = RC.GEOMETRIES[g]
        assert Gd[f'g{g}_geometry'].tolist() == [H, W, D, roi_size]
        geo = O_roi.roi_geometry(roi_size)
        idx = list(ks)
        assert Gd[f'g{g}_seed'][idx].tolist() == [RC.case_seed(g, k) for k in ks]
        assert (Gd[f'g{g}_classes'][idx] == C).all() and (Gd[f'g{g}_thr'][idx] == np.float32(thr)).all()
        box = O_roi.find_boxes(mask, geo['min_h'], geo['min_w'])
        assert np.array_equal(bits(box.numpy()), bits(Gd[f'g{g}_box'][idx])), (g, j)
        x0, y0, _, x1, y1, _ = torch.split(box, 1, dim=1)
        for key, got in (('fx', O_roi.index_map_fwd(x0, x1, H - 1, geo['h_roi'], geo['eval_h'])),
                         ('fy', O_roi.index_map_fwd(y0, y1, W - 1, geo['w_roi'], geo['eval_w'])),
                         ('bx', O_roi.index_map_back(x0, x1, H - 1, geo['h_roi'], geo['eval_h'])),
                         ('by', O_roi.index_map_back(y0, y1, W - 1, geo['w_roi'], geo['eval_w']))):
            assert np.array_equal(bits(got.numpy()), bits(Gd[f'g{g}_{key}'][idx])), (g, j, key)


def test_float32_replay_equals_reference_on_family():
    """the scalar float32 replay in csrc/roi.hip's order (reciprocal-then-multiply slopes in the back map) gives the reference's maps
    bit for bit from the reference's boxes; rounding the back map's slopes once does not"""
    Gd = fixture()
    n_coord = {k: 0 for k in ('fx', 'fy', 'bx', 'by')}
    n_single = 0
    with np.errstate(all='ignore'):
        for g, (H, W, D, roi_size) in enumerate(RC.GEOMETRIES):
            geo = RC.roi_sizes(roi_size)
            for k in range(len(RC.KINDS)):
                x0, y0, _, x1, y1, _ = Gd[f'g{g}_box'][k]
                for key, got in (('fx', RC.replay_fwd(x0, x1, H - 1, geo['h_roi'], geo['eval_h'])),
                                 ('fy', RC.replay_fwd(y0, y1, W - 1, geo['w_roi'], geo['eval_w'])),
                                 ('bx', RC.replay_back(x0, x1, H - 1, geo['h_roi'], geo['eval_h'])),
                                 ('by', RC.replay_back(y0, y1, W - 1, geo['w_roi'], geo['eval_w']))):
                    assert np.array_equal(bits(got), bits(Gd[f'g{g}_{key}'][k])), (g, k, key)
                    n_coord[key] += got.size
                n_single += int((bits(RC.replay_back(x0, x1, H - 1, geo['h_roi'], geo['eval_h'], single_division=True)) != bits(Gd[f'g{g}_bx'][k])).sum())
                n_single += int((bits(RC.replay_back(y0, y1, W - 1, geo['w_roi'], geo['eval_w'], single_division=True)) != bits(Gd[f'g{g}_by'][k])).sum())
    print('coordinates', n_coord, 'single-division back map differs in', n_single)
    assert n_single > 100


def test_taps_match_grid_sample():
    """taps_f32 / dense_f64 are what F.grid_sample does with a coordinate: sampling a one-hot row reads the tap weights back"""
    import torch.nn.functional as F
    rs = np.random.RandomState(5)
    for size in (5, 12, 20):
        g = np.concatenate((rs.uniform(-1.3, 1.3, 40), [-1.0, 1.0, 0.0, -1.0 - 2.0 / (size - 1), 1.0 + 1.0 / (size - 1)])).astype(np.float32)
        for dtype, dense in ((torch.float32, None), (torch.float64, RC.dense_f64(g, size))):
            eye = torch.eye(size, dtype=dtype).reshape(1, size, size, 1)                     # channel s = one-hot at source index s
            grid = torch.stack((torch.zeros(len(g), dtype=dtype), torch.from_numpy(g).to(dtype)), -1).reshape(1, len(g), 1, 2)
            got = F.grid_sample(eye, grid, align_corners=True)[0, :, :, 0].T.numpy()          # [len(g)][size]
            if dense is None:
                s0, w0, w1 = RC.taps_f32(g, size)
                dense = np.zeros((len(g), size), np.float32)
                for i in range(len(g)):
                    if w0[i] != 0: dense[i, s0[i]] += w0[i]
                    if w1[i] != 0: dense[i, s0[i] + 1] += w1[i]
            assert np.array_equal(got, dense), (size, dtype)


def test_roi_plan_refusals_before_launch():
    """an axis above ROI_MAX_LEN = 512 is LTU_E_SHAPE and a missing histogram scratch LTU_E_ARG, before anything touches the (here
    fake) device pointers"""
    from lintransunet_amd import _lib
    lib = _lib.load()
    fake = 1 << 20
    args = lambda H, W, hist: (fake, 1, H, W, 1, 2, 40, 0.5, fake, fake, fake, hist, None)
    assert lib.ltu_roi_plan(*args(513, 512, fake)) == -2
    assert lib.ltu_roi_plan(*args(512, 513, fake)) == -2
    assert lib.ltu_roi_plan(*args(512, 512, None)) == -4
    assert lib.ltu_roi_plan(*args(40, 36, None)) == -4
