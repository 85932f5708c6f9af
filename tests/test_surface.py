"""Surface-distance metrics (HD, HD95, ASSD, NSD) of infer.surface_metrics / csrc/surface.hip against a CPU restatement of the
definition: boundaries from numpy shifts with zero padding, distances from a chunked brute-force nearest-point search between the
two boundary point sets (independent of any distance transform)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = 'cuda'
NAMES = ('HD', 'HD95', 'ASSD', 'NSD')
SURFACE_ENTRY_POINTS = ('ltu_surface_boundary', 'ltu_surface_ws_elems', 'ltu_surface_edt', 'ltu_surface_stats',
                        'ltu_surface_finalize')


# ---------------------------------------------------------------------------------------------- CPU restatement
def boundary(x):
    """voxels of x with a face neighbour outside x; beyond the volume counts as outside"""
    x = np.asarray(x, dtype=bool)
    p = np.pad(x, 1, constant_values=False)
    inner = x.copy()
    n0, n1, n2 = x.shape
    for ax in range(3):
        for sh in (-1, 1):
            sl = [slice(1, n0 + 1), slice(1, n1 + 1), slice(1, n2 + 1)]
            sl[ax] = slice(1 + sh, 1 + sh + x.shape[ax])
            inner &= p[tuple(sl)]
    return x & ~inner


def directed(P, Q, spacing, chunk=512):
    """for each point of P (int [n, 3]) the distance to the nearest point of Q, sqrt(sum ((p - q) * s)^2), float64"""
    if len(Q) == 0:
        return np.full(len(P), np.inf)
    s = np.asarray(spacing, dtype=np.float64)
    out = np.empty(len(P))
    for i in range(0, len(P), chunk):
        diff = (P[i:i + chunk, None, :] - Q[None, :, :]) * s
        out[i:i + chunk] = np.sqrt((diff * diff).sum(-1).min(1))
    return out


def metrics_of_sets(A, B, spacing=(1.0, 1.0, 1.0), tol=1.0):
    ea, eb = boundary(A), boundary(B)
    pa, pb = np.argwhere(ea), np.argwhere(eb)
    if len(pa) == 0 and len(pb) == 0:
        return 0.0, 0.0, 0.0, 1.0
    if len(pa) == 0 or len(pb) == 0:
        return math.inf, math.inf, math.inf, 0.0
    da, db = directed(pa, pb, spacing), directed(pb, pa, spacing)
    n = len(da) + len(db)
    return (max(da.max(), db.max()), max(np.percentile(da, 95), np.percentile(db, 95)), (da.sum() + db.sum()) / n,
            ((da <= tol).sum() + (db <= tol).sum()) / n)


def surface_ref(predict, masks, classes=(1,), spacing=(1.0, 1.0, 1.0), threshold=0.5, tol=1.0):
    predict, masks = np.asarray(predict), np.asarray(masks)
    B = predict.shape[0]
    out = {n: np.zeros((B, len(classes))) for n in NAMES}
    for b in range(B):
        for j, k in enumerate(classes):
            vals = metrics_of_sets(predict[b, k] >= threshold, masks[b, 0] == k, spacing, tol)
            for n, v in zip(NAMES, vals):
                out[n][b, j] = v
    return out


def brute_sq_edt(src, spacing):
    """squared distance of every voxel to the nearest True voxel of src, float64 (+inf without one)"""
    pts = np.argwhere(src)
    grid = np.indices(src.shape).reshape(3, -1).T
    if len(pts) == 0:
        return np.full(src.shape, np.inf)
    s = np.asarray(spacing, dtype=np.float64)
    out = np.empty(len(grid))
    for i in range(0, len(grid), 2048):
        diff = (grid[i:i + 2048, None, :] - pts[None, :, :]) * s
        out[i:i + 2048] = (diff * diff).sum(-1).min(1)
    return out.reshape(src.shape)


def _blob_labels(seed, B=2, shape=(24, 20, 16), touch_border=True):
    """3-label volumes (0 / 1 / 2) from random boxes and ellipsoids, and a perturbed one-hot prediction of them"""
    rng = np.random.default_rng(seed)
    H, W, D = shape
    masks = np.zeros((B, 1) + shape, dtype=np.int64)
    pred_lab = np.zeros((B,) + shape, dtype=np.int64)
    g = np.indices(shape)
    for b in range(B):
        for lab, out in ((1, 0), (2, 0), (1, 1), (2, 1)):
            for _ in range(2):
                c = rng.uniform(0, 1, 3) * np.array(shape)
                r = rng.uniform(2, 6, 3)
                ell = (((g - c[:, None, None, None]) / r[:, None, None, None]) ** 2).sum(0) <= 1
                (masks[b, 0] if out == 0 else pred_lab[b])[ell] = lab
        if touch_border:
            masks[b, 0, :4, :5, :3] = 1
            pred_lab[b, :3, :6, :3] = 1
            masks[b, 0, -3:, -4:, -5:] = 2
        noise = rng.random(shape) < 0.01
        pred_lab[b][noise] = rng.integers(0, 3, noise.sum())
    pred = np.moveaxis(np.eye(3, dtype=np.float32)[pred_lab], -1, 1)      # [B, 3, H, W, D] one-hot
    return pred, masks


# ---------------------------------------------------------------------------------------------- CPU tests
def test_surface_entry_points_declared_and_exported():
    from lintransunet_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ltu_hip.h')).read()
    lib = _lib.load()
    for name in SURFACE_ENTRY_POINTS:
        assert name in _lib.SIGNATURES, name
        assert f' {name}(' in header, name
        assert hasattr(lib, name), name
    assert lib.ltu_surface_ws_elems(10, 20, 30) == 4 * 10 * 20 * 30          # 64-bit return of a size query
    assert lib.ltu_surface_ws_elems(2048, 2048, 1024) == 4 * 2048 * 2048 * 1024


def test_surface_contract_errors_before_launch():
    """argument errors come back before anything touches the (here fake) device pointers"""
    from lintransunet_amd import _lib
    lib = _lib.load()
    fake = 1 << 20
    need = 4 * 4 * 5 * 6                                    # what the EDT of a 4 x 5 x 6 box needs (the query may say more)
    assert lib.ltu_surface_ws_elems(4, 5, 6) >= need
    edt = (fake, fake, fake, need, 8, 8, 8, 1, 1, 1, 4, 5, 6, 1.0, 1.0, 1.0, None)
    assert lib.ltu_surface_edt(*edt[:3], need - 1, *edt[4:]) == -4                          # short scratch: LTU_E_ARG
    assert lib.ltu_surface_edt(*edt[:2], None, *edt[3:]) == -4                              # no scratch
    assert lib.ltu_surface_edt(*edt[:13], 1.0, 0.0, 1.0, None) == -4                       # spacing must be > 0
    assert lib.ltu_surface_edt(*edt[:10], 8, 5, 6, *edt[13:]) == -2                        # box beyond the volume
    stats = (fake, fake, fake, fake, need, 8, 8, 8, 1, 1, 1, 4, 5, 6, 1.0, None)
    assert lib.ltu_surface_stats(*stats[:4], 100, *stats[5:]) == -4
    assert lib.ltu_surface_boundary(fake, fake, fake, fake, 1, 2, 2, 4, 4, 4, 0.5, None) == -4   # class outside C
    assert lib.ltu_surface_finalize(fake, fake, 0, 1, None) == -2


def test_surface_metrics_rejects_cpu_input():
    from lintransunet_amd import _lib, infer as P
    with pytest.raises(_lib.LtuError):
        P.surface_metrics(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4, dtype=torch.int64))
    assert P.SURFACE_METRIC_NAMES == NAMES


@pytest.mark.parametrize('seed,spacing', [(0, (1.0, 1.0, 1.0)), (1, (0.7, 0.7, 2.5)), (2, (1.5, 0.8, 1.0))])
def test_restatement_matches_scipy(seed, spacing):
    ndi = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(seed)
    for _ in range(3):
        A = ndi.binary_dilation(rng.random((14, 11, 9)) < 0.03, iterations=2)
        B = ndi.binary_dilation(rng.random((14, 11, 9)) < 0.03, iterations=1)
        A[0, :3, :3] = True                                 # touching the volume border
        cross = ndi.generate_binary_structure(3, 1)
        for X in (A, B):
            assert np.array_equal(boundary(X), X & ~ndi.binary_erosion(X, cross, border_value=0))
        ea, eb = boundary(A), boundary(B)
        da = directed(np.argwhere(ea), np.argwhere(eb), spacing)
        ref = ndi.distance_transform_edt(~eb, sampling=spacing)[ea]
        np.testing.assert_allclose(da, ref, rtol=1e-12, atol=0)
        sq = brute_sq_edt(eb, spacing)
        np.testing.assert_allclose(np.sqrt(sq), ndi.distance_transform_edt(~eb, sampling=spacing), rtol=1e-12, atol=0)


def test_restatement_analytic():
    A = np.zeros((10, 10, 10), bool); A[2:6, 3:7, 4:8] = True
    assert metrics_of_sets(A, A) == (0.0, 0.0, 0.0, 1.0)
    assert metrics_of_sets(A, np.zeros_like(A)) == (math.inf, math.inf, math.inf, 0.0)
    assert metrics_of_sets(np.zeros_like(A), np.zeros_like(A)) == (0.0, 0.0, 0.0, 1.0)
    S = np.zeros_like(A); S[2:6, 3, 4:8] = True
    hd, hd95, assd, nsd = metrics_of_sets(S, np.roll(S, 3, axis=1), (1.0, 0.7, 2.5))
    assert hd == hd95 == assd == pytest.approx(2.1, rel=1e-12) and nsd == 0.0


# ---------------------------------------------------------------------------------------------- GPU
def _edt(edges, spacing, box=None):
    from lintransunet_amd import _lib
    from lintransunet_amd.ops import _p, _s
    H, W, D = edges.shape
    h0, w0, d0, h, w, d = box or (0, 0, 0, H, W, D)
    e = torch.from_numpy(edges).to(DEV)
    dist = torch.empty((2, h, w, d), device=DEV, dtype=torch.float32)
    ws = _lib.load().ltu_surface_ws_elems(h, w, d)
    scratch = torch.empty(ws, device=DEV, dtype=torch.float32)
    _lib.call('ltu_surface_edt', _p(e), _p(dist), _p(scratch), ws, H, W, D, h0, w0, d0, h, w, d, *[float(v) for v in spacing], _s())
    return dist.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(37, 21, 12), (1, 63, 1), (1, 1, 700), (700, 1, 1), (3, 700, 2), (9, 1, 17), (20, 13, 1)])
def test_edt_matches_brute_force(shape):
    rng = np.random.default_rng(sum(shape))
    vol = int(np.prod(shape))
    edges = np.zeros(shape, dtype=np.uint8)
    for bit, count in ((1, max(1, vol // 200)), (2, 3)):
        idx = rng.choice(vol, count, replace=False)
        edges.reshape(-1)[idx] |= bit
    for spacing in ((1.0, 1.0, 1.0), (0.7, 0.7, 2.5)):
        dist = _edt(edges, spacing)
        for c in range(2):
            ref = brute_sq_edt(edges & (1 << c) != 0, np.float32(spacing).astype(np.float64))
            if spacing == (1.0, 1.0, 1.0):
                assert np.array_equal(dist[c], ref.astype(np.float32)), (shape, c)
            else:
                np.testing.assert_allclose(dist[c], ref, rtol=1e-6, atol=0)


@pytest.mark.gpu
def test_edt_crop_and_no_source():
    """a box inside a larger volume holding every source gives the distances of the whole volume there; no source: +inf"""
    rng = np.random.default_rng(7)
    edges = np.zeros((30, 26, 22), dtype=np.uint8)
    box = (5, 3, 7, 17, 20, 11)
    h0, w0, d0, h, w, d = box
    sub = edges[h0:h0 + h, w0:w0 + w, d0:d0 + d]
    sub.reshape(-1)[rng.choice(sub.size, 12, replace=False)] = 1
    dist = _edt(edges, (1.0, 1.0, 1.0), box)
    full = brute_sq_edt(edges & 1 != 0, (1.0, 1.0, 1.0))
    assert np.array_equal(dist[0], full[h0:h0 + h, w0:w0 + w, d0:d0 + d].astype(np.float32))
    assert np.all(np.isposinf(dist[1]))


@pytest.mark.gpu
def test_edt_short_scratch_is_refused_without_launch():
    from lintransunet_amd import _lib
    from lintransunet_amd.ops import _p, _s
    e = torch.ones((6, 5, 4), device=DEV, dtype=torch.uint8)
    dist = torch.full((2, 6, 5, 4), -7.0, device=DEV)
    ws = 4 * 6 * 5 * 4
    scratch = torch.empty(ws - 1, device=DEV)
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):
        _lib.call('ltu_surface_edt', _p(e), _p(dist), _p(scratch), ws - 1, 6, 5, 4, 0, 0, 0, 6, 5, 4, 1.0, 1.0, 1.0, _s())
    torch.cuda.synchronize()
    assert torch.all(dist == -7.0)


def _check(got, ref, hd_ulps=1):
    for n in NAMES:
        g = got[n].cpu().numpy().astype(np.float64)
        r = ref[n]
        assert g.shape == r.shape, n
        inf = np.isinf(r)
        assert np.array_equal(np.isinf(g), inf), (n, g, r)
        g, r = g[~inf], r[~inf]
        if n == 'HD':
            r32 = r.astype(np.float32)
            assert np.all(np.abs(g - r32) <= hd_ulps * np.spacing(r32)), (n, g, r)
        else:
            assert np.all(np.abs(g - r) <= 1e-6 * np.abs(r) + (1e-7 if n == 'NSD' else 0)), (n, g, r)


@pytest.mark.gpu
@pytest.mark.parametrize('seed,spacing,tol', [(0, (1.0, 1.0, 1.0), 1.0), (1, (0.7, 0.7, 2.5), 1.5), (2, (1.0, 2.0, 0.5), 2.0)])
def test_surface_metrics_matches_restatement(seed, spacing, tol):
    from lintransunet_amd import infer as P
    pred, masks = _blob_labels(seed)
    got = P.surface_metrics(torch.from_numpy(pred).to(DEV), torch.from_numpy(masks).to(DEV), class_indices=(1, 2),
                            spacing=spacing, nsd_tolerance=tol)
    ref = surface_ref(pred, masks, (1, 2), np.float32(spacing).astype(np.float64), 0.5, tol)
    _check(got, ref)
    # the votes of a blended prediction, threshold elsewhere than 0.5
    soft = (pred * 0.8 + 0.1).astype(np.float32)
    got = P.surface_metrics(torch.from_numpy(soft).to(DEV), torch.from_numpy(masks).to(DEV), class_indices=(2, 0), threshold=0.3)
    _check(got, surface_ref(soft, masks, (2, 0), (1.0, 1.0, 1.0), 0.3, 1.0))


@pytest.mark.gpu
@pytest.mark.parametrize('axis', [0, 1, 2])
@pytest.mark.parametrize('spacing', [(1.0, 1.0, 1.0), (0.7, 0.7, 2.5)])
def test_shifted_box(axis, spacing):
    from lintransunet_amd import infer as P
    k = 3
    s = float(np.float32(spacing[axis]))
    shape = (20, 22, 18)
    box = np.zeros(shape, np.int64); box[4:12, 5:13, 3:11] = 1
    slab = np.zeros(shape, np.int64)
    sl = [slice(4, 12), slice(5, 13), slice(3, 11)]; sl[axis] = slice(6, 7)
    slab[tuple(sl)] = 1
    for vol, flat in ((box, False), (slab, True)):
        masks = torch.from_numpy(vol[None, None]).to(DEV)
        pred = torch.from_numpy(np.roll(vol, k, axis=axis)[None, None].astype(np.float32)).to(DEV)
        pred = torch.cat((1 - pred, pred), 1)
        got = {n: v.item() for n, v in P.surface_metrics(pred, masks, spacing=spacing, nsd_tolerance=1.0).items()}
        assert got['HD'] == pytest.approx(k * s, rel=1e-6)
        assert got['HD95'] == pytest.approx(k * s, rel=1e-6)
        if flat:          # every boundary voxel is k voxels from the other slab
            assert got['ASSD'] == pytest.approx(k * s, rel=1e-6) and got['NSD'] == 0.0


@pytest.mark.gpu
def test_analytic_and_empty_cases():
    from lintransunet_amd import infer as P
    shape = (9, 8, 7)
    full, empty = np.ones(shape, np.int64), np.zeros(shape, np.int64)
    blob = empty.copy(); blob[2:6, 1:5, 3:7] = 1
    one = empty.copy(); one[4, 3, 2] = 1
    other = empty.copy(); other[1, 6, 5] = 1

    def run(a, b, spacing=(1.0, 1.0, 1.0), tol=1.0):
        pred = torch.from_numpy(np.stack((1 - a, a))[None].astype(np.float32)).to(DEV)
        got = P.surface_metrics(pred, torch.from_numpy(b[None, None]).to(DEV), spacing=spacing, nsd_tolerance=tol)
        return tuple(got[n].item() for n in NAMES)

    assert run(blob, blob) == (0.0, 0.0, 0.0, 1.0)
    assert run(one, one) == (0.0, 0.0, 0.0, 1.0)
    assert run(full, full) == (0.0, 0.0, 0.0, 1.0)
    assert run(empty, empty) == (0.0, 0.0, 0.0, 1.0)
    assert run(empty, blob) == (math.inf, math.inf, math.inf, 0.0)
    assert run(blob, empty) == (math.inf, math.inf, math.inf, 0.0)
    d = math.sqrt(3 ** 2 * 0.25 + 3 ** 2 * 4.0 + 3 ** 2)
    hd, hd95, assd, nsd = run(one, other, spacing=(0.5, 2.0, 1.0), tol=100.0)
    assert hd == pytest.approx(d, rel=1e-6) and hd95 == pytest.approx(d, rel=1e-6) and assd == pytest.approx(d, rel=1e-6)
    assert nsd == 1.0


@pytest.mark.gpu
def test_whole_scan_pancreas_sized_blob():
    """a 512 x 512 x 48 scan with a pancreas-sized blob (and a prediction that misses part of it, plus a stray island):
    against the restatement, and two calls bit-identical"""
    from lintransunet_amd import infer as P
    shape = (512, 512, 48)
    g = [np.arange(n, dtype=np.float64) for n in shape]
    hh, ww, dd = np.meshgrid(*g, indexing='ij', sparse=True)
    tgt = (((hh - 300) / 38) ** 2 + ((ww - 250) / 22) ** 2 + ((dd - 24) / 11) ** 2 <= 1) \
        | (((hh - 340) / 15) ** 2 + ((ww - 275) / 14) ** 2 + ((dd - 20) / 8) ** 2 <= 1)
    prd = (((hh - 303) / 36) ** 2 + ((ww - 248) / 23) ** 2 + ((dd - 25) / 10) ** 2 <= 1) \
        | (((hh - 200) / 5) ** 2 + ((ww - 100) / 4) ** 2 + ((dd - 30) / 3) ** 2 <= 1)
    masks = torch.from_numpy(tgt.astype(np.uint8)[None, None]).to(DEV)
    pred = torch.from_numpy(np.stack((~prd, prd)).astype(np.float32)[None]).to(DEV)
    spacing = (0.7, 0.7, 2.5)
    got = P.surface_metrics(pred, masks, spacing=spacing, nsd_tolerance=2.0)
    again = P.surface_metrics(pred, masks, spacing=spacing, nsd_tolerance=2.0)
    for n in NAMES:
        assert torch.equal(got[n], again[n]), n
    ref = surface_ref(np.stack((~prd, prd))[None], tgt[None, None].astype(np.int64), (1,), np.float32(spacing).astype(np.float64),
                      0.5, 2.0)
    _check(got, ref)


@pytest.mark.gpu
def test_chain_sliding_window_largest_component_surface():
    """sliding_window_inference -> keep_largest_component -> surface_metrics with the stand-in one-hot predictor of
    tests/test_infer.py, against the restatement on the same post-processed prediction"""
    from lintransunet_amd import infer as P
    from tests.test_infer import _onehot_predictor
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2, 1, 40, 36, 20), generator=g)
    x = torch.nn.functional.avg_pool3d(x, 5, stride=1, padding=2) * 4          # smooth: blobs of either class
    votes = P.sliding_window_inference(x.to(DEV), (32, 32, 16), 4, _onehot_predictor, overlap=0.6)
    post = P.keep_largest_component(votes)
    masks = ((x > 0.2).long() + (x > 0.9).long())                             # labels 0 / 1 / 2 that differ from the prediction
    got = P.surface_metrics(post, masks.to(DEV), class_indices=(1, 2))
    ref = surface_ref(post.cpu().numpy(), masks.numpy(), (1, 2))
    assert got['HD'].shape == (2, 2)
    _check(got, ref)
