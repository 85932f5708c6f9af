"""Connected-component labelling, small-component removal and lesion-wise detection metrics of infer.label_components /
infer.remove_small_components / infer.lesion_metrics (csrc/components.hip).  No reference counterpart: scipy.ndimage.label is the
labelling oracle, and a numpy/scipy restatement of the definitions in the docstrings (checked on hand-built volumes whose answers
are written here) is the oracle of the removal and of the lesion metrics.  infer.keep_largest_component runs on the same labeller:
oracle.infer.keep_largest_component is its oracle, on volumes built around the labeller's 8 x 16 x 32 tile."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lintransunet_amd.infer import (LESION_METRIC_NAMES, keep_largest_component, label_components, lesion_metrics,  # noqa: E402
                                    remove_small_components)
from oracle import infer as O  # noqa: E402

DEV = 'cuda'
ENTRY_POINTS = ('ltu_label_ws_elems', 'ltu_label_components', 'ltu_remove_small_ws_elems', 'ltu_remove_small_components',
                'ltu_keep_largest_ws_elems', 'ltu_keep_largest_component', 'ltu_lesion_ws_elems', 'ltu_lesion_heads',
                'ltu_lesion_stats')
INT_NAMES, RATE_NAMES = LESION_METRIC_NAMES[:5], LESION_METRIC_NAMES[5:]


# ---------------------------------------------------------------------------------------------- CPU restatement
def _structure(conn):
    return ndimage.generate_binary_structure(3, conn)


def restate_remove(pred, min_voxels, classes=None, conn=3):
    """round, clear the components of out[b, k] > 0 smaller than min_voxels per class, channel 0 = 1 - the rest"""
    out = np.round(np.asarray(pred, np.float32))
    if min_voxels <= 1:
        return out
    B, C = out.shape[:2]
    for b in range(B):
        for k in (range(1, C) if classes is None else classes):
            lab, n = ndimage.label(out[b, k] > 0, _structure(conn))
            small = np.bincount(lab.ravel(), minlength=n + 1) < min_voxels
            small[0] = False
            out[b, k][small[lab]] = 0
    out[:, 0] = 1 - out[:, 1:].sum(1, dtype=np.float32)
    return out


def restate_lesion(pred, masks, classes=(1,), threshold=0.5, conn=3):
    """float64 restatement of lesion_metrics: {name: [B, K]}"""
    pred, masks = np.asarray(pred), np.asarray(masks)
    B, K = pred.shape[0], len(classes)
    res = {name: np.zeros((B, K), np.float64) for name in LESION_METRIC_NAMES}
    for b in range(B):
        for kk, k in enumerate(classes):
            P, G = pred[b, k] >= threshold, masks[b, 0] == k
            lp, m = ndimage.label(P, _structure(conn))
            lg, n = ndimage.label(G, _structure(conn))
            size_p = np.bincount(lp.ravel(), minlength=m + 1)
            tp, dsum = 0, 0.0
            for j in range(1, n + 1):
                gj = lg == j
                o = int((gj & P).sum())
                touch = np.unique(lp[gj & P])
                u = int(size_p[touch[touch > 0]].sum())
                tp += o >= 1
                dsum += 2.0 * o / (gj.sum() + u)
            fp = sum(1 for i in range(1, m + 1) if not (G & (lp == i)).any())
            sens = 1.0 if n == 0 else tp / n
            prec = 1.0 if m == 0 else (m - fp) / m
            vals = (n, m, tp, n - tp, fp, sens, prec, 0.0 if sens + prec == 0 else 2 * sens * prec / (sens + prec),
                    1.0 if n + fp == 0 else dsum / (n + fp))
            for name, v in zip(LESION_METRIC_NAMES, vals):
                res[name][b, kk] = v
    return res


def _onehot(lab, C=3):
    return np.moveaxis(np.eye(C, dtype=np.float32)[lab], -1, 1)          # [B, H, W, D] ids -> [B, C, H, W, D]


def _expect(res, want, col=0, b=0):
    for name, v in zip(LESION_METRIC_NAMES, want):
        assert res[name][b, col] == pytest.approx(v, abs=1e-12), (name, res[name][b, col], v)


# ---------------------------------------------------------------------------------------------- CPU tests
def test_entry_points_declared_and_contract_errors():
    from lintransunet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ltu_hip.h')).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and f' {name}(' in header and hasattr(lib, name), name
    assert lib.ltu_label_ws_elems(2, 8, 8, 8) >= 2 * 512
    assert lib.ltu_label_ws_elems(1, 2048, 1024, 1024) == 0                      # S = 2^31: refused
    assert lib.ltu_remove_small_ws_elems(1, 2048, 1024, 1024) == 0
    assert lib.ltu_lesion_ws_elems(1, 2048, 1024, 1024, 0) == 0
    assert lib.ltu_lesion_ws_elems(1, 8, 8, 8, -1) == 0
    assert lib.ltu_lesion_ws_elems(1, 8, 8, 8, 100) > lib.ltu_lesion_ws_elems(1, 8, 8, 8, 0)
    fake = 1 << 20                                                                # never dereferenced: every call below is refused
    need = lib.ltu_label_ws_elems(2, 8, 8, 8)
    lab = (fake, fake, fake, fake, need, 2, 8, 8, 8, 3, None)
    assert lib.ltu_label_components(*lab[:4], need - 1, *lab[5:]) == -4          # short scratch: LTU_E_ARG, nothing launched
    assert lib.ltu_label_components(*lab[:3], None, *lab[4:]) == -4
    assert lib.ltu_label_components(*lab[:9], 0, None) == -4                     # connectivity 0 / 4
    assert lib.ltu_label_components(*lab[:9], 4, None) == -4
    assert lib.ltu_label_components(*lab[:5], 1, 2048, 1024, 1024, 3, None) == -2   # S >= 2^31
    need = lib.ltu_remove_small_ws_elems(2, 8, 8, 8)
    rm = (fake, fake, need, 2, 3, 0b110, 8, 8, 8, 5, 3, None)
    assert lib.ltu_remove_small_components(fake, fake, need - 1, *rm[3:]) == -4
    assert lib.ltu_remove_small_components(*rm[:10], 0, None) == -4
    assert lib.ltu_remove_small_components(*rm[:10], 4, None) == -4
    assert lib.ltu_remove_small_components(*rm[:5], 0b111, *rm[6:]) == -4        # channel 0 is not a class to clean
    assert lib.ltu_remove_small_components(*rm[:3], 1, 3, 0b110, 2048, 1024, 1024, 5, 3, None) == -2
    assert lib.ltu_keep_largest_ws_elems(1, 2048, 1024, 1024) == 0
    need = lib.ltu_keep_largest_ws_elems(3, 5, 7, 9)                             # par + size + an aligned 64-bit key per sample
    assert need >= 2 * 3 * 315 + 2 * 3
    kl = (fake, fake, need, 3, 3, 5, 7, 9, 3, None)
    assert lib.ltu_keep_largest_component(fake, fake, need - 1, *kl[3:]) == -4
    assert lib.ltu_keep_largest_component(fake, None, *kl[2:]) == -4
    assert lib.ltu_keep_largest_component(None, *kl[1:]) == -4
    assert lib.ltu_keep_largest_component(*kl[:8], 0, None) == -4
    assert lib.ltu_keep_largest_component(*kl[:8], 4, None) == -4
    assert lib.ltu_keep_largest_component(*kl[:4], 1, *kl[5:]) == -2             # C = 1: no foreground channel
    assert lib.ltu_keep_largest_component(*kl[:4], 32, *kl[5:]) == -2
    assert lib.ltu_keep_largest_component(*kl[:3], 0, *kl[4:]) == -2
    assert lib.ltu_keep_largest_component(*kl[:3], 1, 3, 2048, 1024, 1024, 3, None) == -2
    need = lib.ltu_lesion_ws_elems(2, 8, 8, 8, 10)
    st = [fake, fake, fake, fake, fake, need, 10, 2, 3, 1, 0, 2, 8, 8, 8, 0.5, 3, None]
    assert lib.ltu_lesion_stats(*st[:5], need - 1, *st[6:]) == -4
    assert lib.ltu_lesion_stats(*st[:6], 40, *st[7:]) == -4                       # a larger pair bound needs a larger hash set
    assert lib.ltu_lesion_stats(*st[:16], 0, None) == -4
    assert lib.ltu_lesion_stats(*st[:16], 4, None) == -4
    assert lib.ltu_lesion_stats(*st[:15], float('nan'), 3, None) == -4
    assert lib.ltu_lesion_stats(*st[:9], 3, *st[10:]) == -4                       # class outside 0 .. C-1
    assert lib.ltu_lesion_stats(*st[:10], 2, *st[11:]) == -2                      # column kk outside 0 .. K-1
    assert lib.ltu_lesion_stats(*st[:7], 1, 3, 1, 0, 2, 2048, 1024, 1024, 0.5, 3, None) == -2
    hd = [fake, fake, fake, 2, 3, 1, 8, 8, 8, 0.5, 3, None]
    assert lib.ltu_lesion_heads(*hd[:10], 0, None) == -4
    assert lib.ltu_lesion_heads(*hd[:3], 1, 3, 1, 2048, 1024, 1024, 0.5, 3, None) == -2


def test_rejects_cpu_and_bad_arguments():
    from lintransunet_amd import _lib
    with pytest.raises(_lib.LtuError):
        label_components(torch.zeros(1, 4, 4, 4))
    with pytest.raises(_lib.LtuError):
        remove_small_components(torch.zeros(1, 3, 4, 4, 4), 5)
    with pytest.raises(_lib.LtuError):
        lesion_metrics(torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4, dtype=torch.int64))
    assert LESION_METRIC_NAMES == ('NumTrue', 'NumPred', 'TruePositives', 'FalseNegatives', 'FalsePositives', 'Sensitivity',
                                   'Precision', 'F1', 'LesionDice')


def _hand_volume():
    """one detected lesion (Dice 1/2), one missed lesion, one false-positive blob; class 1 in an 8^3 volume"""
    masks = np.zeros((1, 1, 8, 8, 8), np.int64)
    lab = np.zeros((1, 8, 8, 8), np.int64)
    masks[0, 0, 1:3, 1:3, 1:3] = 1               # G_1, 8 voxels
    lab[0, 1:3, 1:3, 2:4] = 1                    # P_1, 8 voxels, 4 inside G_1
    masks[0, 0, 5:7, 5:7, 0:2] = 1               # G_2: missed
    lab[0, 6, 1, 6] = 1                          # P_2: a one-voxel false positive
    return _onehot(lab), masks


def test_restatement_hand_built_lesions():
    pred, masks = _hand_volume()
    r = restate_lesion(pred, masks)
    # n, m, TP, FN, FP, Sensitivity, Precision, F1, LesionDice = Dice_1 / (n + FP) = 0.5 / 3
    _expect(r, (2, 2, 1, 1, 1, 0.5, 0.5, 0.5, 0.5 / 3))


def test_restatement_bridge_shares_the_union():
    """one predicted component touching two GT lesions: U_1 = U_2 = P, Dice_j = 2 * 1 / (2 + 4)"""
    masks = np.zeros((1, 1, 1, 1, 8), np.int64)
    masks[0, 0, 0, 0, [0, 1, 4, 5]] = 1
    lab = np.zeros((1, 1, 1, 8), np.int64)
    lab[0, 0, 0, 1:5] = 1
    _expect(restate_lesion(_onehot(lab), masks), (2, 1, 2, 0, 0, 1.0, 1.0, 1.0, 1 / 3))


def test_restatement_diagonal_contact():
    """G = two voxels meeting at a corner: one lesion at connectivity 3, two at 1 (and 2)"""
    masks = np.zeros((1, 1, 2, 2, 2), np.int64)
    masks[0, 0, 0, 0, 0] = masks[0, 0, 1, 1, 1] = 1
    lab = np.zeros((1, 2, 2, 2), np.int64)
    lab[0, 0, 0, 0] = 1
    pred = _onehot(lab)
    _expect(restate_lesion(pred, masks, conn=3), (1, 1, 1, 0, 0, 1.0, 1.0, 1.0, 2 / 3))
    for conn in (1, 2):
        _expect(restate_lesion(pred, masks, conn=conn), (2, 1, 1, 1, 0, 0.5, 1.0, 2 / 3, 0.5))


def test_restatement_empty_cases():
    z = np.zeros((1, 3, 4, 4, 4), np.float32)
    z[:, 0] = 1
    none = np.zeros((1, 1, 4, 4, 4), np.int64)
    one = none.copy()
    one[0, 0, 0, 0, 0] = 1
    p_one = z.copy()
    p_one[0, 1, 3, 3, 3], p_one[0, 0, 3, 3, 3] = 1, 0
    _expect(restate_lesion(z, none), (0, 0, 0, 0, 0, 1.0, 1.0, 1.0, 1.0))          # n = 0, m = 0
    _expect(restate_lesion(p_one, none), (0, 1, 0, 0, 1, 1.0, 0.0, 0.0, 0.0))      # n = 0, m = 1
    _expect(restate_lesion(z, one), (1, 0, 0, 1, 0, 0.0, 1.0, 0.0, 0.0))           # n = 1, m = 0
    _expect(restate_lesion(p_one, one), (1, 1, 0, 1, 1, 0.0, 0.0, 0.0, 0.0))       # S + P = 0: F1 = 0


def test_restatement_remove_small():
    lab = np.zeros((1, 6, 6, 6), np.int64)
    lab[0, 0, 0, 0] = 1                                      # size 1
    lab[0, 3, 0, 0:3] = 1                                    # size 3
    lab[0, 5, 3:5, 3] = 2                                    # class 2, size 2
    lab[0, 2, 4, 4] = lab[0, 3, 5, 5] = 1                    # diagonal pair: one component of 2 at connectivity 3, two of 1 at 1
    pred = _onehot(lab)
    out = restate_remove(pred, 2, conn=3)
    want = lab.copy()
    want[0, 0, 0, 0] = 0
    np.testing.assert_array_equal(out, _onehot(want))
    out = restate_remove(pred, 2, conn=1)
    want[0, 2, 4, 4] = want[0, 3, 5, 5] = 0
    np.testing.assert_array_equal(out, _onehot(want))
    out = restate_remove(pred, 3, classes=(1,), conn=1)      # class 2 untouched
    want = lab.copy()
    want[0, 0, 0, 0] = want[0, 2, 4, 4] = want[0, 3, 5, 5] = 0
    np.testing.assert_array_equal(out, _onehot(want))
    np.testing.assert_array_equal(restate_remove(pred * 0.8, 1), np.round(pred * 0.8))   # min_voxels <= 1: rounded input


# ---------------------------------------------------------------------------------------------- largest component: the cases
def restate_keep(pred, conn=3):
    """oracle.infer.keep_largest_component with generate_binary_structure(3, conn) in place of the full 3x3x3 structure"""
    out = np.round(np.asarray(pred, np.float32))
    for b in range(out.shape[0]):
        fg = out[b, 1:].sum(0) > 0
        lab, n = ndimage.label(fg, _structure(conn))
        if n > 0:
            keep = np.argmax(np.bincount(lab.ravel())[1:]) + 1
            out[b, 1:][:, fg & (lab != keep)] = 0
        out[b, 0] = 1 - out[b, 1:].sum(0)
    return out


def _corner_labels():
    """9 x 17 x 33, one voxel past the 8 x 16 x 32 tile on every axis: a class-1 and a class-2 voxel that meet only diagonally across
    the tile corner, a class-1 pair at the origin, a lone class-1 voxel"""
    lab = np.zeros((1, 9, 17, 33), np.int64)
    lab[0, 7, 15, 31], lab[0, 8, 16, 32] = 1, 2
    lab[0, 0, 0, 0:2] = 1
    lab[0, 4, 8, 16] = 1
    return lab


def _face_labels(axis):
    """12 x 20 x 36: a class-2 line of 6 inside the first tile against a class-1 bar of 8 that crosses the tile face of `axis`
    (h = 7|8, w = 15|16 or d = 31|32) with 4 voxels on each side: no tile-local piece of the bar beats the line, the whole bar does"""
    lab = np.zeros((1, 12, 20, 36), np.int64)
    lab[0, 0, 0, 0:6] = 2
    idx = [2, 10, 20]
    idx[axis] = slice((8, 16, 32)[axis] - 4, (8, 16, 32)[axis] + 4)
    lab[(0,) + tuple(idx)] = 1
    return lab


def _fold_labels(shape=(16, 16, 40), rows_w=(7, 9, 11, 13, 15), short=3):
    """a class-1 boustrophedon path (rows along D on even h and the given w, joined at alternating ends, layers joined at the turn:
    its raster order and its order along the path disagree everywhere) beside a compact class-2 block in w < rows_w[0] - 1 that
    comes first in raster order and is `short` voxels smaller.  Returns (labels [1, H, W, D], path voxels)."""
    H, W, D = shape
    path = np.zeros(shape, bool)
    rows = [(h, w) for i, h in enumerate(range(0, H, 2)) for w in (rows_w if i % 2 == 0 else rows_w[::-1])]
    for i, (h, w) in enumerate(rows):
        path[h, w, :] = True
        if i + 1 < len(rows):
            h2, w2 = rows[i + 1]
            end = D - 1 if i % 2 == 0 else 0
            if h2 == h:
                path[h, min(w, w2) + 1, end] = True
            else:
                path[h + 1, w, end] = True
    n = int(path.sum())
    wb = rows_w[0] - 1
    block = np.zeros(H * wb * D, bool)
    block[:n - short] = True
    lab = np.zeros((1,) + shape, np.int64)
    lab[0][path] = 1
    lab[0, :, :wb][block.reshape(H, wb, D)] = 2
    return lab, n


def _batch_labels():
    """B = 3 over 10 x 18 x 34: sample 0 a block of 8 then a block of 27 (the later one wins), sample 1 without foreground,
    sample 2 all foreground in stripes of both classes"""
    lab = np.zeros((3, 10, 18, 34), np.int64)
    lab[0, 0:2, 0:2, 0:2] = 1
    lab[0, 6:9, 14:17, 30:33] = 2
    lab[2] = 1 + (np.arange(34) // 3) % 2
    return lab


@functools.lru_cache(maxsize=None)
def _keep_cases():
    """{name: (predict tensor [B, C, H, W, D] on the CPU, connectivity, expected f32 tensor)}: expected from
    oracle.infer.keep_largest_component (connectivity 3) or restate_keep; built once, never modified"""
    rng = np.random.default_rng(31)
    cases = {}

    def add(name, pred, conn=3):
        pred = pred if torch.is_tensor(pred) else torch.from_numpy(np.ascontiguousarray(pred, np.float32))
        want = O.keep_largest_component(pred) if conn == 3 else torch.from_numpy(restate_keep(pred.float().numpy(), conn))
        cases[name] = (pred, conn, want)

    corner = _onehot(_corner_labels())
    add('corner', corner)
    add('corner_c1', corner, 1)
    add('corner_c2', corner, 2)
    for ax in range(3):
        add(f'face_{ax}', _onehot(_face_labels(ax)))
    add('fold', _onehot(_fold_labels()[0]))
    add('batch', _onehot(_batch_labels()))
    noise = rng.random((2, 20, 33, 35)) < P_C[3]                                  # many components, ties among the largest likely
    add('noise_c2ch', _onehot(noise.astype(np.int64), 2))
    add('noise_c1', _onehot(noise * rng.integers(1, 4, noise.shape), 4), 1)
    line = np.zeros((1, 1, 1, 40), np.int64)
    line[0, 0, 0, 3:9], line[0, 0, 0, 20:33] = 1, 1
    add('axes_1x1xd', _onehot(line, 2))
    add('axes_hx1x1', _onehot(np.array([1, 1, 0, 1, 1, 1, 0, 0, 1]).reshape(1, 9, 1, 1), 2))
    votes = 0.9 * _onehot(noise * rng.integers(1, 3, noise.shape)) + 0.04
    add('votes', votes)
    add('votes_bf16', torch.from_numpy(votes).to(torch.bfloat16))
    wide = torch.from_numpy(np.repeat(votes, 2, axis=4))
    add('strided', wide[..., ::2])                                                # a non-contiguous view
    return cases


def _fg(t):
    return t[:, 1:].sum(1) > 0


def test_keep_largest_cases_make_the_oracle_do_what_they_claim():
    """which component survives in each constructed input, by the oracle alone"""
    cases = _keep_cases()
    for name, (pred, conn, want) in cases.items():
        assert want.dtype == torch.float32 and want.shape == pred.shape, name
        if conn == 3:                                                            # the restatement is the oracle at connectivity 3
            assert torch.equal(torch.from_numpy(restate_keep(pred.float().numpy(), 3)), want), name
    origin = torch.zeros((1, 9, 17, 33), dtype=torch.bool)
    origin[0, 0, 0, 0:2] = True
    lab = _corner_labels()
    for name in ('corner', 'corner_c1', 'corner_c2'):                           # a 2 : 2 tie (c = 3) or 2 : 1 : 1: the origin pair stays
        assert torch.equal(_fg(cases[name][2]), origin), name
    assert ndimage.label(lab[0] > 0, _structure(3))[1] == 3 and ndimage.label(lab[0] > 0, _structure(1))[1] == 4
    for ax in range(3):                                                          # the bar of 8 beats the line of 6
        assert torch.equal(_fg(cases[f'face_{ax}'][2]), torch.from_numpy(_face_labels(ax) == 1)), ax
    lab, n = _fold_labels()
    assert n >= 1000 and ndimage.label(lab[0] == 1, _structure(1))[1] == 1 and int((lab == 2).sum()) == n - 3
    assert ndimage.label(lab[0] > 0, _structure(3))[1] == 2 and np.flatnonzero(lab)[0] == np.flatnonzero(lab == 2)[0]
    assert torch.equal(_fg(cases['fold'][2]), torch.from_numpy(lab == 1))       # the path wins, though the block comes first
    pred, _, want = cases['batch']
    assert int(_fg(want)[0].sum()) == 27 and bool(_fg(want)[0, 7, 15, 31])
    assert torch.equal(want[1], pred[1]) and bool((want[1, 0] == 1).all()) and torch.equal(want[2], pred[2])
    assert torch.equal(cases['votes'][2], cases['strided'][2]) and not cases['strided'][0].is_contiguous()
    assert cases['votes_bf16'][0].dtype == torch.bfloat16
    for name in ('noise_c2ch', 'noise_c1', 'votes'):                            # something is cleared and something is kept
        pred, _, want = cases[name]
        kept, had = _fg(want).sum((1, 2, 3)), _fg(torch.round(pred.float())).sum((1, 2, 3))
        assert bool((kept > 0).all()) and bool((kept < had).all()), name


# ---------------------------------------------------------------------------------------------- GPU tests
P_C = {1: 0.3116, 2: 0.1372, 3: 0.0976}         # site-percolation thresholds of the simple-cubic lattice per neighbourhood


def _serpentine(n=40):
    """a boustrophedon path through a cube: rows along D on even (h, w), joined at alternating ends, layers joined at the last row"""
    v = np.zeros((n, n, n), bool)
    rows = [(h, w) for h in range(0, n, 2) for w in (range(0, n, 2) if (h // 2) % 2 == 0 else range(n - 2 - (n % 2), -1, -2))]
    for i, (h, w) in enumerate(rows):
        v[h, w, :] = True
        if i + 1 < len(rows):
            h2, w2 = rows[i + 1]
            end = n - 1 if i % 2 == 0 else 0
            if h2 == h:
                v[h, min(w, w2) + 1, end] = True
            else:
                v[h + 1, w, end] = True
    return v


def _volumes(conn):
    rng = np.random.default_rng(100 + conn)
    cases = {}
    for f in (0.9, 1.0, 1.2):
        cases[f'random_{f}'] = rng.random((1, 48, 40, 56)) < P_C[conn] * f
    cases['serpentine'] = _serpentine()[None]
    for ax in range(3):
        shape = [3, 3, 3]
        shape[ax] = 733
        v = np.zeros(shape, bool)
        idx = [1, 1, 1]
        idx[ax] = slice(None)
        v[tuple(idx)] = True
        idx2 = [0, 2, 2]
        idx2[ax] = slice(5, 720, 3)                                               # dotted line: 239 components at any c
        v[tuple(idx2)] = True
        cases[f'line_{ax}'] = v[None]
    cases['axes_1xwxd'] = rng.random((1, 1, 50, 61)) < 0.5
    cases['axes_hx1xd'] = rng.random((1, 40, 1, 33)) < 0.5
    cases['axes_hxwx1'] = rng.random((1, 37, 45, 1)) < 0.5
    cases['single'] = np.ones((1, 1, 1, 1), bool)
    cases['all_fg'] = np.ones((1, 33, 34, 35), bool)
    cases['all_bg'] = np.zeros((1, 33, 34, 35), bool)
    g = np.indices((20, 21, 22)).sum(0)
    cases['checker'] = (g % 2 == 0)[None]
    cases['batch3'] = np.stack([rng.random((30, 31, 40)) < 0.3, np.ones((30, 31, 40), bool), rng.random((30, 31, 40)) < 0.05])
    return cases


def _check_labels(vol, conn):
    labels, counts = label_components(torch.from_numpy(vol).to(DEV), connectivity=conn)
    torch.cuda.synchronize()
    got, cnt = labels.cpu().numpy(), counts.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == vol.shape and cnt.shape == (vol.shape[0],)
    for b in range(vol.shape[0]):
        ref, n = ndimage.label(vol[b], _structure(conn))
        assert cnt[b] == n, (b, cnt[b], n)
        np.testing.assert_array_equal(got[b], ref)
    return labels, counts


@pytest.mark.gpu
@pytest.mark.parametrize('conn', (1, 2, 3))
def test_label_components_matches_scipy(conn):
    for name, vol in _volumes(conn).items():
        try:
            _check_labels(vol, conn)
        except AssertionError as e:
            raise AssertionError(f'case {name}, connectivity {conn}: {e}') from None


@pytest.mark.gpu
def test_serpentine_is_one_component():
    v = _serpentine()
    assert v.sum() > 5000 and ndimage.label(v, _structure(1))[1] == 1
    for conn in (1, 3):
        _, counts = _check_labels(v[None], conn)
        assert int(counts[0]) == 1


@pytest.mark.gpu
def test_label_components_ct_sized_scan_and_repeat():
    rng = np.random.default_rng(7)
    vol = np.zeros((1, 512, 512, 48), bool)
    g = np.indices((512, 512, 48), dtype=np.float32)
    for _ in range(12):
        c, r = rng.uniform(0, 1, 3) * np.array([512, 512, 48]), rng.uniform(4, 60, 3)
        vol[0] |= (((g - c[:, None, None, None]) / r[:, None, None, None]) ** 2).sum(0) <= 1
    vol |= rng.random(vol.shape) < 0.002
    labels, counts = _check_labels(vol, 3)
    m = torch.from_numpy(vol).to(DEV)
    for again_in in (m, m[:, None].to(torch.float32)):                          # bit-identical repeat; any dtype, nonzero = fg
        again, counts2 = label_components(again_in)
        assert torch.equal(labels, again) and torch.equal(counts, counts2)


@pytest.mark.gpu
def test_short_scratch_is_refused_with_nothing_written():
    from lintransunet_amd import _lib
    from lintransunet_amd.ops import _p
    lib = _lib.load()
    m = torch.ones((1, 8, 8, 8), device=DEV, dtype=torch.uint8)
    labels = torch.full((1, 8, 8, 8), -7, device=DEV, dtype=torch.int32)
    counts = torch.full((1,), -7, device=DEV, dtype=torch.int32)
    need = lib.ltu_label_ws_elems(1, 8, 8, 8)
    scratch = torch.full((need,), -7, device=DEV, dtype=torch.int32)
    assert lib.ltu_label_components(_p(m), _p(labels), _p(counts), _p(scratch), need - 1, 1, 8, 8, 8, 3, None) == -4
    pred = torch.ones((1, 2, 8, 8, 8), device=DEV)
    need = lib.ltu_remove_small_ws_elems(1, 8, 8, 8)
    assert lib.ltu_remove_small_components(_p(pred), _p(scratch), need - 1, 1, 2, 2, 8, 8, 8, 5, 3, None) == -4
    ints = torch.full((5, 1, 1), -7, device=DEV, dtype=torch.int32)
    rates = torch.full((4, 1, 1), -7.0, device=DEV)
    tgt = torch.ones((1, 8, 8, 8), device=DEV, dtype=torch.uint8)
    need = lib.ltu_lesion_ws_elems(1, 8, 8, 8, 4)
    big = torch.full((need,), -7, device=DEV, dtype=torch.int32)
    assert lib.ltu_lesion_stats(_p(pred), _p(tgt), _p(ints), _p(rates), _p(big), need - 1, 4, 1, 2, 1, 0, 1, 8, 8, 8, 0.5, 3, None) == -4
    torch.cuda.synchronize()
    assert (labels == -7).all() and (counts == -7).all() and (scratch == -7).all() and (big == -7).all()
    assert (pred == 1).all() and (ints == -7).all() and (rates == -7).all()


def _blob_case(seed, B=2, shape=(40, 36, 28), votes=False):
    """class ids 0 / 1 / 2 from random ellipsoids (several small lesions per class), a prediction that moves, drops and adds some
    of them plus specks; one-hot, or soft votes whose arg-max is that prediction"""
    rng = np.random.default_rng(seed)
    g = np.indices(shape)
    masks = np.zeros((B, 1) + shape, np.int64)
    lab = np.zeros((B,) + shape, np.int64)
    for b in range(B):
        for k in (1, 2):
            for _ in range(6):
                c, r = rng.uniform(0, 1, 3) * np.array(shape), rng.uniform(1.5, 5, 3)
                ell = lambda c=c, r=r: (((g - c[:, None, None, None]) / r[:, None, None, None]) ** 2).sum(0) <= 1  # noqa: E731
                if rng.random() < 0.85:
                    masks[b, 0][ell()] = k
                if rng.random() < 0.8:
                    lab[b][ell(c + rng.normal(0, 1.5, 3), r * rng.uniform(0.7, 1.3, 3))] = k
        specks = rng.random(shape) < 0.004
        lab[b][specks] = rng.integers(1, 3, specks.sum())
    pred = _onehot(lab)
    if votes:
        soft = rng.uniform(0, 0.45, pred.shape).astype(np.float32)
        soft = np.where(pred > 0, 0.5 + soft, soft * 0.5)
        pred = (soft / soft.sum(1, keepdims=True)).astype(np.float32)
    return pred, masks


@pytest.mark.gpu
@pytest.mark.parametrize('seed,votes', [(1, False), (2, True), (3, False)])
def test_remove_small_components_matches_restatement(seed, votes):
    pred, _ = _blob_case(seed, votes=votes)
    x = torch.from_numpy(pred).to(DEV)
    for conn in (1, 2, 3):
        for min_voxels, classes in ((1, None), (4, None), (30, None), (12, (2,))):
            got = remove_small_components(x, min_voxels, class_indices=classes, connectivity=conn)
            ref = restate_remove(pred, min_voxels, classes, conn)
            np.testing.assert_array_equal(got.cpu().numpy(), ref, err_msg=f'conn {conn} min {min_voxels} classes {classes}')
    assert torch.equal(x, torch.from_numpy(pred).to(DEV))                         # the input is not modified


def _check_lesion(got, ref):
    for name in INT_NAMES:
        assert got[name].dtype == torch.int32
        np.testing.assert_array_equal(got[name].cpu().numpy(), ref[name].astype(np.int32), err_msg=name)
    for name in RATE_NAMES:
        assert got[name].dtype == torch.float32
        np.testing.assert_allclose(got[name].cpu().numpy(), ref[name], rtol=2e-7, atol=1e-7, err_msg=name)


@pytest.mark.gpu
@pytest.mark.parametrize('seed,votes', [(4, False), (5, True), (6, True)])
def test_lesion_metrics_matches_restatement(seed, votes):
    pred, masks = _blob_case(seed, votes=votes)
    x, m = torch.from_numpy(pred).to(DEV), torch.from_numpy(masks).to(DEV)
    for conn in (1, 3):
        for thr in (0.3, 0.5, 0.7):
            got = lesion_metrics(x, m, class_indices=(1, 2), threshold=thr, connectivity=conn)
            assert got['NumTrue'].shape == (2, 2)
            _check_lesion(got, restate_lesion(pred, masks, (1, 2), thr, conn))
    again = lesion_metrics(x, m, class_indices=(1, 2), threshold=0.7, connectivity=3)
    for name in LESION_METRIC_NAMES:                                              # bit-identical repeat
        assert torch.equal(got[name], again[name]), name


@pytest.mark.gpu
def test_lesion_metrics_hand_built_and_empty_cases():
    pred, masks = _hand_volume()
    got = lesion_metrics(torch.from_numpy(pred).to(DEV), torch.from_numpy(masks).to(DEV))
    _check_lesion(got, restate_lesion(pred, masks))
    assert float(got['LesionDice'][0, 0]) == pytest.approx(0.5 / 3, rel=1e-6)
    z = np.zeros((2, 3, 6, 5, 4), np.float32)
    z[:, 0] = 1
    z[1, 2, 1, 1, 1], z[1, 0, 1, 1, 1] = 1, 0                                     # sample 1: a class-2 false positive only
    mk = np.zeros((2, 1, 6, 5, 4), np.int64)
    mk[0, 0, 4, 4, 3] = 1                                                          # sample 0: a missed class-1 lesion only
    got = lesion_metrics(torch.from_numpy(z).to(DEV), torch.from_numpy(mk).to(DEV), class_indices=(1, 2))
    _check_lesion(got, restate_lesion(z, mk, (1, 2)))


@pytest.mark.gpu
def test_chain_sliding_window_remove_small_lesion_metrics():
    """sliding_window_inference -> remove_small_components -> lesion_metrics with the stand-in one-hot predictor of
    tests/test_infer.py, against the restatement on the same votes"""
    from lintransunet_amd import infer as P
    from tests.test_infer import _onehot_predictor
    g = torch.Generator().manual_seed(12)
    x = torch.randn((2, 1, 40, 36, 20), generator=g)
    x = torch.nn.functional.avg_pool3d(x, 5, stride=1, padding=2) * 4
    votes = P.sliding_window_inference(x.to(DEV), (32, 32, 16), 4, _onehot_predictor, overlap=0.6)
    post = P.remove_small_components(votes, 20)
    ref_post = restate_remove(votes.cpu().numpy(), 20)
    np.testing.assert_array_equal(post.cpu().numpy(), ref_post)
    masks = ((x > 0.2).long() + (x > 0.9).long())
    got = P.lesion_metrics(post, masks.to(DEV), class_indices=(1, 2))
    ref = restate_lesion(ref_post, masks.numpy(), (1, 2))
    assert ref['NumTrue'].sum() > 2 and ref['NumPred'].sum() > 2
    _check_lesion(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ('corner', 'corner_c1', 'corner_c2', 'face_0', 'face_1', 'face_2', 'fold', 'batch', 'noise_c2ch',
                                  'noise_c1', 'axes_1x1xd', 'axes_hx1x1', 'votes', 'votes_bf16', 'strided'))
def test_keep_largest_component_matches_oracle_around_the_tile(name):
    pred, conn, want = _keep_cases()[name]
    x = pred.to(DEV)
    got = keep_largest_component(x, connectivity=conn)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), want)
    assert torch.equal(x.cpu(), pred)                                             # the input is not modified


@pytest.mark.gpu
def test_keep_largest_component_repeats_and_never_reads_the_host():
    pred, _, want = _keep_cases()['batch']
    x = pred.to(DEV)
    first = keep_largest_component(x)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        again = keep_largest_component(x)                                         # a host read (.item(), .cpu()) would raise here
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(first, again) and torch.equal(again.cpu(), want) and torch.equal(x.cpu(), pred)
