"""Sliding-window whole-volume inference on the MI355X.

Mirrors the reference driver inference_embed_attn.py:92-185:
    predict = sliding_window_inference(images, (512, 512, depth), 4, model, overlap=0.6, sigma_scale=0)   # monai 0.7.0
    predict2 = (predict >= 0.5).float()
    DiceClassLoss / Recall / Precision / LocalizationLoss (predict2, masks)
with the same argument meaning.  Window scheduling is host integer logic; the windows, the weighted votes of the model's eval
output (its one-hot arg-max, or its softmax with probs) and the metrics stay in HBM and go through the C-ABI.  No CPU fallback.
Every mode runs one window loop on the gather and blend kernels of csrc/blend.hip: the reference's call is the constant
weight 1 without mirrors, mode='gaussian' and mirror_axes are the same loop with other tables and more items.  The division
and the driver's metrics are csrc/infer.hip.
"""
import math

import numpy as np
import torch

from . import _lib, data, ops
from .ops import _p, _s


def scan_interval(image_size, roi_size, overlap):
    """monai/inferers/utils.py::_get_scan_interval"""
    out = []
    for img, roi in zip(image_size, roi_size):
        if roi == img:
            out.append(int(roi))
        else:
            iv = int(roi * (1 - overlap))
            out.append(iv if iv > 0 else 1)
    return tuple(out)


def patch_starts(image_size, roi_size, interval):
    """monai/data/utils.py::dense_patch_slices: window starts, first dimension slowest"""
    per_dim = []
    for img, roi, iv in zip(image_size, roi_size, interval):
        if iv == 0:
            num = 1
        else:
            cnt = int(math.ceil(float(img) / iv))
            first = next((d for d in range(cnt) if d * iv + roi >= img), None)
            num = first + 1 if first is not None else 1
        per_dim.append([idx * iv - max(idx * iv + roi - img, 0) for idx in range(num)])
    out = [()]
    for starts in per_dim:
        out = [o + (s,) for o in out for s in starts]
    return out


BLEND_MODES = ('constant', 'gaussian')


def _blend_options(mode, sigma_scale, mirror_axes):
    """(mode, sigma_scale per axis, mirror_axes) checked; ValueError on anything else"""
    if not isinstance(mode, str) or mode not in BLEND_MODES:
        raise ValueError(f"mode must be one of {BLEND_MODES}, got {mode!r}")
    try:
        sig = tuple(float(v) for v in sigma_scale) if isinstance(sigma_scale, (tuple, list)) else (float(sigma_scale),) * 3
    except (TypeError, ValueError):
        raise ValueError(f'sigma_scale must be a number or one number per axis, got {sigma_scale!r}') from None
    if len(sig) != 3:
        raise ValueError(f'sigma_scale must be a number or one number per axis, got {sigma_scale!r}')
    if mode == 'gaussian' and not all(v > 0 and math.isfinite(v) for v in sig):
        raise ValueError(f"mode='gaussian' needs sigma_scale > 0 (finite), got {sigma_scale!r}")
    if not isinstance(mirror_axes, (tuple, list)) or not all(isinstance(a, int) and not isinstance(a, bool) for a in mirror_axes) \
            or not all(0 <= a <= 2 for a in mirror_axes) or len(set(mirror_axes)) != len(mirror_axes):
        raise ValueError(f'mirror_axes must be distinct spatial axes from (0, 1, 2), got {mirror_axes!r}')
    return mode, sig, tuple(mirror_axes)


def importance_tables(roi, mode='gaussian', sigma_scale=0.125):
    """The blending weight of sliding_window_inference as three float64 per-axis tables and a floor: the weight of window voxel u
    (in volume orientation) is w(u) = max(g0[u0] g1[u1] g2[u2], wmin).  Returns (g0, g1, g2, wmin), numpy arrays of the roi's
    extents and a float.  mode='constant': tables of ones, wmin = 1.  mode='gaussian' restates monai 0.7.0's
    compute_importance_map (GaussianFilter(truncated=4.0, approx="erf") on a delta at the centre, normalised to a maximum of 1,
    clamped to its smallest non-zero value) axis by axis, for an axis of extent r:
        c = r // 2, sigma = r * sigma_scale, tail = int(max(4 sigma, 0.5) + 0.5)
        k(x) = max(0, (erf((x + 1/2) / (sigma sqrt 2)) - erf((x - 1/2) / (sigma sqrt 2))) / 2)
        g[i] = k(i - c) / k(0), and 0 where |i - c| > tail
    wmin = the product of each axis's smallest non-zero entry = the smallest non-zero value of the 3-D map."""
    mode, sig, _ = _blend_options(mode, sigma_scale, ())
    roi = tuple(int(r) for r in roi)
    if len(roi) != 3 or min(roi) < 1:
        raise ValueError(f'roi must be three extents >= 1, got {roi}')
    if mode == 'constant':
        return np.ones(roi[0]), np.ones(roi[1]), np.ones(roi[2]), 1.0
    tabs, wmin = [], 1.0
    for r, s in zip(roi, sig):
        c, sigma = r // 2, r * s
        tail = int(max(4.0 * sigma, 0.5) + 0.5)
        den = sigma * math.sqrt(2.0)

        def k(x):
            return max(0.0, 0.5 * (math.erf((x + 0.5) / den) - math.erf((x - 0.5) / den)))

        k0 = k(0)
        g = np.array([k(i - c) / k0 if abs(i - c) <= tail else 0.0 for i in range(r)])
        wmin *= float(g[g > 0].min())
        tabs.append(g)
    return tabs[0], tabs[1], tabs[2], wmin


def mirror_masks(mirror_axes=()):
    """flip masks of the 2^|A| variants of a window, variant m first to last: variant m flips axis A[j] for every bit j set in m;
    bit a of a mask is axis a (0 = H, 1 = W, 2 = D), so variant 0 is the window as it is"""
    return [sum(1 << a for j, a in enumerate(mirror_axes) if (m >> j) & 1) for m in range(1 << len(mirror_axes))]


def window_items(batch, starts, mirror_axes=()):
    """the blending items in order: (b, h0, w0, d0, mask) for idx in range(batch * len(starts)) (sample-major, b = idx // nwin,
    start = starts[idx % nwin]) and, within a window, its mirror variants (mirror_masks) - the variants of a window are adjacent"""
    nwin, masks = len(starts), mirror_masks(mirror_axes)
    return [(idx // nwin, *starts[idx % nwin], m) for idx in range(batch * nwin) for m in masks]


def item_batches(items, sw_batch_size):
    """the predictor's batches: consecutive chunks of sw_batch_size items"""
    return [items[g:g + sw_batch_size] for g in range(0, len(items), sw_batch_size)]


def channel_items(items, channels):
    """window descriptors of a [B, K, ...] volume viewed as B K single-channel volumes: every item (b, ...) becomes its K
    descriptors (b K + c, ...), c = 0 .. K-1, adjacent and in channel order, so that a gather kernel, which writes its items
    consecutively, fills windows [n, K, h, w, d].  channels == 1 returns the items as they are."""
    K = int(channels)
    if K == 1:
        return list(items)
    return [(it[0] * K + c, *it[1:]) for it in items for c in range(K)]


def sliding_window_inference(inputs, roi_size, sw_batch_size, predictor, overlap=0.25, mode='constant', sigma_scale=0.125,
                             mirror_axes=()):
    """inputs f32 [B, K, H, W, D] on the GPU, K = 1 .. 4 input channels; predictor(windows [n, K, h, w, d]) -> [n, C, h, w, d],
    C = 1 .. 8 (the eval-mode MaskTransUnet: channels-last one-hot exposed in the reference's shape, or its softmax with
    probs=True).  Returns f32 [B, C, H, W, D], the per-voxel weighted average of the window outputs.  The K channels of a window
    are gathered as K items of the single-channel gather kernel (channel_items); an output channel's sums do not depend on C.

    One loop for every mode (csrc/blend.hip): window voxel u is weighted by importance_tables(roi, mode, sigma_scale), which is 1
    for mode='constant' (monai's mode="constant", the reference's call: the plain average) and monai's mode="gaussian" map for
    mode='gaussian'; mirror_axes = A (distinct axes of (0, 1, 2) = H, W, D) predicts every window 2^|A| times, variant m flipped
    along the axes of mirror_masks(A)[m], and blends each prediction flipped back, with the weight of its un-flipped position.
    The predictor sees consecutive chunks of sw_batch_size items of window_items (sample-major, the variants of a window
    adjacent).  Each voxel's sums are formed in fp32 in item order: the result is bit-identical between calls and for every
    sw_batch_size; with weight 1 and a one-hot predictor they are small integers, exact in any order.  Bad mode, sigma_scale or
    mirror_axes raise ValueError before anything runs; more than 8 output channels raise LtuError once the predictor has
    returned its first batch, before anything is blended (the blend kernel, like the heads, the losses and class_metrics, stops
    at 8 classes)."""
    mode, sig, axes = _blend_options(mode, sigma_scale, mirror_axes)
    if not inputs.is_cuda:
        raise _lib.LtuError('sliding_window_inference runs on the GPU only (no CPU fallback)')
    if inputs.dim() != 5 or not 1 <= inputs.shape[1] <= _lib.MAX_INPUT_CHANNELS:
        raise _lib.LtuError(f'inputs must be [B, K, H, W, D] with K = 1 .. {_lib.MAX_INPUT_CHANNELS}')
    if int(sw_batch_size) < 1:
        raise ValueError(f'sw_batch_size must be >= 1, got {sw_batch_size}')
    B, K, dev = inputs.shape[0], inputs.shape[1], inputs.device
    img0 = tuple(int(v) for v in inputs.shape[2:])
    roi = tuple(int(r) if r and r > 0 else i for r, i in zip(roi_size, img0))
    pad_lo = tuple(max(r - i, 0) // 2 for r, i in zip(roi, img0))
    img = tuple(max(i, r) for i, r in zip(img0, roi))
    starts = patch_starts(img, roi, scan_interval(img, roi, overlap))
    vol = inputs.to(torch.float32).contiguous()
    g0, g1, g2, wmin = importance_tables(roi, mode, sig)
    tab = torch.tensor(np.concatenate((g0, g1, g2)), dtype=torch.float32).to(dev)
    t0, t1, t2 = tab[:roi[0]], tab[roi[0]:roi[0] + roi[1]], tab[roi[0] + roi[1]:]
    votes = wsum = None
    C = None
    for chunk in item_batches(window_items(B, starts, axes), int(sw_batch_size)):
        n = len(chunk)
        parts = [(s, np.ascontiguousarray(chunk[s:s + _lib.BLEND_ITEMS_MAX], dtype=np.int32))
                 for s in range(0, n, _lib.BLEND_ITEMS_MAX)]
        win = torch.empty((n, K) + roi, device=dev, dtype=torch.float32)
        flat, expanded = win.view((n * K,) + roi), channel_items(chunk, K)        # the gather's items: one per window and channel
        for s in range(0, n * K, _lib.BLEND_ITEMS_MAX):
            desc = np.ascontiguousarray(expanded[s:s + _lib.BLEND_ITEMS_MAX], dtype=np.int32)
            _lib.call('ltu_window_gather_mirror', _p(vol), _p(flat[s:]), desc.ctypes.data, len(desc), B * K, *img0, *img, *roi, _s())
        seg = predictor(win)
        if seg.dim() != 5 or tuple(seg.shape[2:]) != roi or seg.shape[0] != n:
            raise _lib.LtuError(f'predictor returned {tuple(seg.shape)} for windows {(n, K) + roi}')
        seg_cl = seg.permute(0, 2, 3, 4, 1)
        if seg_cl.dtype != torch.float32 or not seg_cl.is_contiguous():
            seg_cl = seg_cl.to(torch.float32).contiguous()
        if votes is None:
            C = seg.shape[1]
            if not 1 <= C <= 8:
                raise _lib.LtuError(f'sliding_window_inference blends 1 .. 8 output channels, the predictor returned {C}')
            votes = torch.zeros((B, C) + img, device=dev, dtype=torch.float32)
            wsum = torch.zeros((B,) + img, device=dev, dtype=torch.float32)
        elif seg.shape[1] != C:
            raise _lib.LtuError(f'predictor returned {seg.shape[1]} channels after {C}')
        for s, desc in parts:
            _lib.call('ltu_window_blend', _p(seg_cl[s:]), _p(votes), _p(wsum), _p(t0), _p(t1), _p(t2), wmin, desc.ctypes.data,
                      len(desc), B, C, *img, *roi, _s())
    out = torch.empty((B, C) + img0, device=dev, dtype=torch.float32)
    _lib.call('ltu_vote_finalize', _p(votes), _p(wsum), _p(out), B, C, *img0, *img, *pad_lo, _s())
    return out


METRIC_NAMES = ('DiceClassLoss', 'Recall', 'Precision', 'LocalizationLoss')


def evaluate(predict, masks, threshold=0.5, class_index=1):
    """The driver's metrics on predict2 = (predict >= threshold) against masks [B, 1, H, W, D] (0/1):
    returns {name: device scalar} for DiceClassLoss, Recall, Precision, LocalizationLoss (loss/criterions.py)."""
    if not predict.is_cuda:
        raise _lib.LtuError('evaluate runs on the GPU only (no CPU fallback)')
    B, C, H, W, D = predict.shape
    pred = predict.to(torch.float32).contiguous()
    tgt = masks.reshape(B, H, W, D).to(torch.uint8).contiguous()
    rows = torch.empty((B, 3, H), device=pred.device, dtype=torch.float32)
    values = torch.empty(4, device=pred.device, dtype=torch.float32)
    _lib.call('ltu_seg_metrics', _p(pred), _p(tgt), _p(rows), _p(values), B, C, class_index, H, W * D, float(threshold), _s())
    return {name: values[i] for i, name in enumerate(METRIC_NAMES)}


def keep_largest_component(predict, connectivity=3):
    """inference_multi_classes.py:146-151 on predict [B, C, H, W, D] (the blended votes): round, keep the largest component of
    the foreground union (monai KeepLargestConnectedComponent(applied_labels=[1, 2], independent=False, connectivity=3); see
    label_components for the connectivity; of equally large components the raster-first), channel 0 = 1 - the rest
    (csrc/components.hip).  Returns a new tensor; one call for the batch, no host synchronisation."""
    if not predict.is_cuda:
        raise _lib.LtuError('keep_largest_component runs on the GPU only (no CPU fallback)')
    conn = _connectivity(connectivity)
    B, C, H, W, D = (int(v) for v in predict.shape)
    out = torch.round(predict.to(torch.float32)).contiguous()
    ws = _lib.load().ltu_keep_largest_ws_elems(B, H, W, D)
    if ws <= 0:
        raise _lib.LtuError(f'keep_largest_component: shape {tuple(predict.shape)} refused (H * W * D must be < 2^31)')
    scratch = torch.empty(ws, device=out.device, dtype=torch.int32)
    _lib.call('ltu_keep_largest_component', _p(out), _p(scratch), ws, B, C, H, W, D, conn, _s())
    return out


SURFACE_METRIC_NAMES = ('HD', 'HD95', 'ASSD', 'NSD')


def surface_metrics(predict, masks, class_indices=(1,), spacing=(1.0, 1.0, 1.0), threshold=0.5, nsd_tolerance=1.0):
    """Boundary metrics of predict [B, C, H, W, D] (the votes of sliding_window_inference or the one-hot output of
    keep_largest_component) against the integer label volume masks [B, 1, H, W, D], on the GPU (csrc/surface.hip).

    For sample b and class k: A = predict[b, k] >= threshold, B = masks[b, 0] == k.  The boundary dX holds the voxels of X with
    at least one of their 6 face neighbours outside X; voxels beyond the volume count as outside (X & ~binary_erosion(X,
    6-connected cross, border_value=0)).  d(x, dY) = min over y in dY of sqrt(sum_i ((x_i - y_i) * s_i)^2) with the spacing
    s = (s_H, s_W, s_D) in tensor-axis order; DA = {d(a, dB) : a in dA}, DB = {d(b, dA) : b in dB}.
        HD   = max(max DA, max DB)
        HD95 = max(P95(DA), P95(DB))                          numpy's default linear percentile
        ASSD = (sum DA + sum DB) / (|dA| + |dB|)
        NSD  = (#{DA <= tol} + #{DB <= tol}) / (|dA| + |dB|)  boundary-voxel counts, not the surfel-area form
    Both boundaries empty: HD = HD95 = ASSD = 0, NSD = 1; exactly one empty: HD = HD95 = ASSD = +inf, NSD = 0.

    Returns {name: f32 device tensor [B, len(class_indices)]} for SURFACE_METRIC_NAMES.  The exact Euclidean distance transform
    runs over the bounding box of the two boundaries only; the boxes are read to the host once per call (launch geometry).
    No CPU fallback."""
    if not predict.is_cuda:
        raise _lib.LtuError('surface_metrics runs on the GPU only (no CPU fallback)')
    if predict.dim() != 5 or masks.dim() != 5 or masks.shape[1] != 1 or masks.shape[0] != predict.shape[0] \
            or tuple(masks.shape[2:]) != tuple(predict.shape[2:]):
        raise _lib.LtuError(f'predict [B, C, H, W, D] and masks [B, 1, H, W, D] expected, got {tuple(predict.shape)} and '
                            f'{tuple(masks.shape)}')
    sp = tuple(float(v) for v in spacing)
    if len(sp) != 3 or not all(v > 0 and math.isfinite(v) for v in sp):
        raise _lib.LtuError(f'spacing must be three finite values > 0, got {spacing}')
    B, C, H, W, D = (int(v) for v in predict.shape)
    classes = tuple(int(k) for k in class_indices)
    if not classes or not all(0 <= k < C for k in classes):
        raise _lib.LtuError(f'class_indices {class_indices} outside 0 .. {C - 1}')
    K = len(classes)
    dev = predict.device
    pred = predict.to(torch.float32).contiguous()
    tgt = masks.to(dev).reshape(B, H, W, D).to(torch.uint8).contiguous()
    edges = torch.empty((K, B, H, W, D), device=dev, dtype=torch.uint8)
    bbox = torch.empty((K, B, 6), device=dev, dtype=torch.int32)
    for kk, k in enumerate(classes):
        _lib.call('ltu_surface_boundary', _p(pred), _p(tgt), _p(edges[kk]), _p(bbox[kk]), B, C, k, H, W, D, float(threshold), _s())
    rec = torch.zeros((K, B, 12), device=dev, dtype=torch.float64)
    boxes = bbox.cpu().tolist()              # the one host read of the call: crop geometry
    crops = [(kk, b, box[:3], [box[3 + i] - box[i] + 1 for i in range(3)])
             for kk, per in enumerate(boxes) for b, box in enumerate(per) if box[3] >= 0]     # both boundaries empty: no crop
    if crops:
        most = max(h * w * d for _, _, _, (h, w, d) in crops)
        dist = torch.empty(2 * most, device=dev, dtype=torch.float32)
        ws = max(_lib.load().ltu_surface_ws_elems(h, w, d) for _, _, _, (h, w, d) in crops)
        scratch = torch.empty(ws, device=dev, dtype=torch.float32)
        for kk, b, (h0, w0, d0), (h, w, d) in crops:
            e = edges[kk, b]
            _lib.call('ltu_surface_edt', _p(e), _p(dist), _p(scratch), ws, H, W, D, h0, w0, d0, h, w, d, *sp, _s())
            _lib.call('ltu_surface_stats', _p(e), _p(dist), _p(rec[kk, b]), _p(scratch), ws, H, W, D, h0, w0, d0, h, w, d,
                      float(nsd_tolerance), _s())
    out = torch.empty((4, B, K), device=dev, dtype=torch.float32)
    _lib.call('ltu_surface_finalize', _p(rec), _p(out), B, K, _s())
    return {name: out[i] for i, name in enumerate(SURFACE_METRIC_NAMES)}


MULTI_METRIC_NAMES = ('DiceClassLoss0', 'DiceClassLoss', 'DiceClassLoss2', 'Recall', 'Precision', 'Recall2', 'Precision2',
                      'LocalizationLoss')


def _class_metrics_run(predict, masks, threshold, label_map):
    """one statistics pass + one finalize (csrc/class_metrics.hip): f32 [B + 1, 3C + 2] (row b < B: Dice[C], Recall[C],
    Precision[C], foreground Dice, LocalizationLoss of sample b; row B: 1 - mean Dice[C], mean Recall[C], mean Precision[C],
    1 - mean foreground Dice, mean LocalizationLoss) and the u8 label map [B, H, W, D] when asked for"""
    from .losses import _labels
    if not predict.is_cuda:
        raise _lib.LtuError('class_metrics runs on the GPU only (no CPU fallback)')
    if predict.dim() != 5:
        raise _lib.LtuError(f'predict [B, C, H, W, D] expected, got {tuple(predict.shape)}')
    B, C, H, W, D = (int(v) for v in predict.shape)
    if not 2 <= C <= 8:
        raise _lib.LtuError(f'class_metrics supports 2 .. 8 classes, got C = {C}')
    if masks.dim() != 5 or masks.shape[0] != B or masks.shape[1] not in (1, C) or tuple(masks.shape[2:]) != (H, W, D):
        raise _lib.LtuError(f'masks [B, 1, H, W, D] (class ids) or [B, C, H, W, D] (one-hot) expected for predict '
                            f'{tuple(predict.shape)}, got {tuple(masks.shape)}')
    thr = -1.0 if threshold is None else float(threshold)
    if threshold is not None and not thr >= 0.0:
        raise _lib.LtuError(f'threshold must be >= 0 or None, got {threshold}')
    dev = predict.device
    pred = predict.to(torch.float32).contiguous()
    tgt = _labels(masks.to(dev), C)
    lmap = torch.empty((B, H, W, D), device=dev, dtype=torch.uint8) if label_map else None
    ws = _lib.load().ltu_class_metrics_ws_elems(B, C, H, W, D)
    scratch = torch.empty(ws, device=dev, dtype=torch.float64)
    out = torch.empty((B + 1, 3 * C + 2), device=dev, dtype=torch.float32)
    _lib.call('ltu_class_metrics_pass', _p(pred), _p(tgt), _p(lmap) if label_map else None, _p(scratch), ws, B, C, H, W, D, thr, _s())
    _lib.call('ltu_class_metrics_finalize', _p(scratch), ws, _p(out), B, C, H, W, D, _s())
    return out, lmap


def class_metrics(predict, masks, class_indices=None, threshold=None, return_label_map=False):
    """Overlap metrics of loss/multi_criterions.py per sample and class, on the GPU (csrc/class_metrics.hip), from one read of
    predict [B, C, H, W, D] f32 (2 <= C <= 8: the votes of sliding_window_inference or the output of keep_largest_component)
    and masks, the class ids [B, 1, H, W, D] (a one-hot [B, C, H, W, D] is reduced to ids as losses._labels does; ids >= C count
    as foreground of no class).  p = predict as given (threshold=None) or [predict >= threshold]; t_c = [mask == c]:
        Dice      = (2 sum p_c t_c + 1e-9) / (sum p_c + sum t_c + 1e-9)       DiceClassLoss / DiceClassLoss2 = 1 - its batch mean
        Recall    = (sum p_c t_c + 1e-5) / (sum t_c + 1e-5)                   Recall / Recall2 = its batch mean
        Precision = (sum p_c t_c + 1e-5) / (sum p_c + 1e-5)                   Precision / Precision2 = its batch mean
        ForegroundDice of 1 - p_0 against [mask != 0] (eps 1e-9)                DiceClassLoss0 = 1 - its batch mean
        LocalizationLoss (multi_criterions.py:219-281, no factor 8): the H profiles of 1 - p_0 and [mask != 0] (sums over W, D)
                    through sigmoid(x - 10), cumulative sums over H divided by (their sum + 1e-6), mean over H of |cp - ct|
    Sums are exact for integer-valued inputs and folded in fp64 in a fixed order: two calls are bit-identical.

    Returns f32 device tensors {'Dice', 'Recall', 'Precision'} [B, K] (column j = class class_indices[j], all C classes when
    None), 'ForegroundDice' [B], 'LocalizationLoss' [B], and with return_label_map 'label_map' u8 [B, H, W, D] = the arg-max
    over C of predict (the first maximal index on ties, as torch.argmax).  No host synchronisation; an int64 or one-hot masks
    costs a conversion pass of its own (uint8 class ids are read as they are)."""
    if predict.dim() == 5 and class_indices is not None:
        C = int(predict.shape[1])
        if not all(0 <= int(k) < C for k in class_indices) or not len(class_indices):
            raise _lib.LtuError(f'class_indices {class_indices} outside 0 .. {C - 1}')
    out, lmap = _class_metrics_run(predict, masks, threshold, return_label_map)
    B, C = int(predict.shape[0]), int(predict.shape[1])
    res = {}
    for i, name in enumerate(('Dice', 'Recall', 'Precision')):
        block = out[:B, i * C:(i + 1) * C]
        res[name] = block if class_indices is None else torch.stack([block[:, int(k)] for k in class_indices], 1)
    res['ForegroundDice'] = out[:B, 3 * C]
    res['LocalizationLoss'] = out[:B, 3 * C + 1]
    if return_label_map:
        res['label_map'] = lmap
    return res


def evaluate_multiclass(predict, masks, threshold=None, return_label_map=False):
    """The metrics of inference_multi_classes.py:153 (loss/multi_criterions.py, its default criterion_list) on predict
    [B, C >= 3, H, W, D] against masks (class ids [B, 1, H, W, D] or their one-hot): {name: device scalar} for
    MULTI_METRIC_NAMES, the values `[l(predict, label).item() for l in criterions.values()]` prints (see class_metrics for the
    definitions).  One statistics pass and one finalize; the scalars are views of the finalize output, so no further launch and
    no host synchronisation.  With return_label_map, 'label_map' is the driver's is_save map argmax(predict, 1) as u8
    [B, H, W, D] from the same pass."""
    if predict.dim() == 5 and predict.shape[1] < 3:
        raise _lib.LtuError(f'evaluate_multiclass needs C >= 3 (classes 1 and 2), got C = {predict.shape[1]}')
    out, lmap = _class_metrics_run(predict, masks, threshold, return_label_map)
    B, C = int(predict.shape[0]), int(predict.shape[1])
    m = out[B]
    res = {'DiceClassLoss0': m[3 * C], 'DiceClassLoss': m[1], 'DiceClassLoss2': m[2], 'Recall': m[C + 1],
           'Precision': m[2 * C + 1], 'Recall2': m[C + 2], 'Precision2': m[2 * C + 2], 'LocalizationLoss': m[3 * C + 1]}
    if return_label_map:
        res['label_map'] = lmap
    return res


def _region_probs(p, R, what):
    """fp32 probabilities [B,R,...] (or [R,...]: one sample) of a region model -> (tensor, planes, B, N, spatial shape, one sample) as
    csrc/region.hip reads it: channels-last memory behind the view (what the model and infer_volume return; planes 0) as it is,
    anything else as contiguous planes [B][R][N] (what data.to_native_probs returns; planes 1)"""
    if p.dtype != torch.float32 or not p.is_cuda or p.dim() < 2:
        raise ValueError(f'{what}: fp32 device probabilities [B,R,...] or [R,...]')
    single = p.dim() == 4 and p.shape[0] == R      # [R,H,W,D]
    if single:
        p = p.unsqueeze(0)
    if p.shape[1] != R:
        raise ValueError(f'{what}: {p.shape[1]} channels for the {R} regions of the record')
    B, spatial = p.shape[0], tuple(p.shape[2:])
    N = math.prod(spatial)
    if p.permute(0, *range(2, p.dim()), 1).is_contiguous() and R > 1:
        return p, 0, B, N, spatial, single
    return p.contiguous(), 1, B, N, spatial, single


def region_labels(p, regions, threshold=0.5):
    """The label map of a region model's probabilities by nnU-Net's rule (csrc/region.hip): p fp32 [B,R,...] in either memory
    layout (channels-last behind the view, as the model and infer_volume return it, or planes, as data.to_native_probs does), or
    [R,H,W,D] for one volume; the label starts at 0 and for r = 0 .. R-1 in order regions.class_order[r] is written where p_r >
    threshold, so a later region wins and p == threshold is not painted.  Returns uint8 [B,...] (or [H,W,D]); no host read."""
    if regions.class_order is None:
        raise ValueError('region_labels: the record has no class_order to paint the regions with')
    R = len(regions.members)
    p, planes, B, N, spatial, single = _region_probs(p, R, 'region_labels')
    out = torch.empty((B, *spatial), device=p.device, dtype=torch.uint8)
    ops._lib.call('ltu_region_labels', p.data_ptr(), planes, ops._int_array(regions.class_order), float(threshold), out.data_ptr(), B, N, R,
                  torch.cuda.current_stream().cuda_stream)
    return out[0] if single else out


def region_metrics(predict, masks, regions, threshold=0.5):
    """Per (sample, region) overlap of a prediction with the label `masks` (uint8 [B,1,...] or [B,...]) under the record
    `regions`: predict is a uint8 label map of that shape, scored through the record's membership table, or fp32 probabilities
    [B,R,...] (either memory layout), region r predicted where p_r > threshold.  Returns {'Dice', 'TP', 'FP', 'FN'} as [B, R] device
    tensors (Dice fp32, the counts int64): Dice = 2 TP / (2 TP + FP + FN), and 1 where the region is empty on both sides (BraTS's
    convention).  Integer counts with integer atomics (csrc/region.hip); no host read."""
    R = len(regions.members)
    if masks.dtype != torch.uint8 or not masks.is_cuda:
        raise ValueError('region_metrics: masks must be a uint8 device label volume')
    B = masks.shape[0]
    truth = ops.region_bits(masks.contiguous(), regions.lut)
    N = truth.numel() // B
    if predict.dtype == torch.uint8:
        if predict.numel() != truth.numel() or predict.shape[0] != B:
            raise ValueError('region_metrics: the predicted label map must have the shape of masks')
        pred = ops.region_bits(predict.contiguous(), regions.lut)
    else:
        p, planes, pB, pN, _, _ = _region_probs(predict, R, 'region_metrics')
        if (pB, pN) != (B, N):
            raise ValueError('region_metrics: the probabilities must cover the voxels of masks')
        pred = torch.empty_like(truth)
        ops._lib.call('ltu_region_prob_bits', p.data_ptr(), planes, float(threshold), pred.data_ptr(), B, N, R,
                      torch.cuda.current_stream().cuda_stream)
    counts = torch.zeros((B, R, 3), device=masks.device, dtype=torch.int64)
    dice = torch.empty((B, R), device=masks.device, dtype=torch.float32)
    ops._lib.call('ltu_region_counts', pred.data_ptr(), truth.data_ptr(), counts.data_ptr(), dice.data_ptr(), B, N, R,
                  torch.cuda.current_stream().cuda_stream)
    return {'Dice': dice, 'TP': counts[:, :, 0], 'FP': counts[:, :, 1], 'FN': counts[:, :, 2]}


def _connectivity(connectivity):
    if connectivity not in (1, 2, 3):
        raise _lib.LtuError(f'connectivity must be 1, 2 or 3 (6-, 18-, 26-neighbourhood), got {connectivity}')
    return int(connectivity)


def label_components(mask, connectivity=3):
    """Connected components of every sample of mask [B, H, W, D] or [B, 1, H, W, D] (any dtype, nonzero = foreground), on the GPU
    (csrc/components.hip).  connectivity 1 / 2 / 3: the 6- / 18- / 26-neighbourhood (voxels whose coordinates differ by at most 1
    on at most that many axes), as scipy.ndimage.generate_binary_structure(3, connectivity); voxels beyond the volume are
    background.  Returns (labels int32 [B, H, W, D], counts int32 [B]): background 0, the components of sample b numbered
    1 .. counts[b] in raster order of their first voxel, exactly scipy.ndimage.label(mask[b], structure).  A union-find in a fixed
    number of launches: no host synchronisation, two calls are bit-identical.  S = H W D < 2^31."""
    if not mask.is_cuda:
        raise _lib.LtuError('label_components runs on the GPU only (no CPU fallback)')
    if mask.dim() == 5 and mask.shape[1] == 1:
        mask = mask[:, 0]
    if mask.dim() != 4:
        raise _lib.LtuError(f'mask [B, H, W, D] or [B, 1, H, W, D] expected, got {tuple(mask.shape)}')
    conn = _connectivity(connectivity)
    B, H, W, D = (int(v) for v in mask.shape)
    if mask.dtype == torch.bool:
        m = mask.contiguous().view(torch.uint8)
    elif mask.dtype == torch.uint8:
        m = mask.contiguous()
    else:
        m = (mask != 0).contiguous().view(torch.uint8)
    ws = _lib.load().ltu_label_ws_elems(B, H, W, D)
    if ws <= 0:
        raise _lib.LtuError(f'label_components: shape {tuple(mask.shape)} refused (H * W * D must be < 2^31)')
    dev = mask.device
    labels = torch.empty((B, H, W, D), device=dev, dtype=torch.int32)
    counts = torch.empty(B, device=dev, dtype=torch.int32)
    scratch = torch.empty(ws, device=dev, dtype=torch.int32)
    _lib.call('ltu_label_components', _p(m), _p(labels), _p(counts), _p(scratch), ws, B, H, W, D, conn, _s())
    return labels, counts


def fill_holes(mask, connectivity=1):
    """Hole filling of every sample of mask [B, H, W, D] or [B, 1, H, W, D] (any dtype, nonzero = set), on the GPU
    (csrc/components.hip): u8 [B, H, W, D] = 1 on the mask and on every background voxel that no path of background voxels joins
    to a face of the volume, 0 elsewhere; exactly scipy.ndimage.binary_fill_holes(mask[b], generate_binary_structure(3,
    connectivity)) (its default structure is connectivity 1), and monai's FillHoles on one class with fill_holes(label == c).
    The background is labelled with label_components' union-find under `connectivity`, the components that reach a face are
    marked, the rest is filled: five launches, no host synchronisation, two calls are bit-identical.  S = H W D < 2^31."""
    conn = _connectivity(connectivity)
    if not mask.is_cuda:
        raise _lib.LtuError('fill_holes runs on the GPU only (no CPU fallback)')
    if mask.dim() == 5 and mask.shape[1] == 1:
        mask = mask[:, 0]
    if mask.dim() != 4:
        raise _lib.LtuError(f'mask [B, H, W, D] or [B, 1, H, W, D] expected, got {tuple(mask.shape)}')
    if mask.dtype == torch.bool:
        m = mask.contiguous().view(torch.uint8)
    elif mask.dtype == torch.uint8:
        m = mask.contiguous()
    else:
        m = (mask != 0).contiguous().view(torch.uint8)
    return data.fill_holes_u8(m, torch.empty_like(m), conn)


def _binary_u8(mask, what):
    """mask [N, H, W, D] or [N, 1, H, W, D] of any dtype as a contiguous u8 device tensor [N, H, W, D] (nonzero = object)"""
    if not mask.is_cuda:
        raise _lib.LtuError(f'{what} runs on the GPU only (no CPU fallback)')
    if mask.dim() == 5 and mask.shape[1] == 1:
        mask = mask[:, 0]
    if mask.dim() != 4:
        raise _lib.LtuError(f'mask [N, H, W, D] or [N, 1, H, W, D] expected, got {tuple(mask.shape)}')
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8)
    if mask.dtype == torch.uint8:
        return mask.contiguous()
    return (mask != 0).contiguous().view(torch.uint8)


THIN_BATCH = 4      # thinning iterations enqueued between two host reads of the deletion counters


def _thin_inplace(vol):
    """thins the u8 volumes vol [N, H, W, D] in place (csrc/thinning.hip); returns the number of iterations that deleted a voxel.
    Host reads: the object counts once, then the deletion counters once per THIN_BATCH iterations."""
    N, H, W, D = (int(v) for v in vol.shape)
    dev = vol.device
    counts = torch.empty(8, device=dev, dtype=torch.int64)
    if _lib.load().ltu_thin_ws_elems(N, H, W, D, 0) <= 0:
        raise _lib.LtuError(f'skeletonize: shape {tuple(vol.shape)} refused (N <= 65535, H * W * D < 2^31, N * H * W * D < 2^32)')
    _lib.call('ltu_thin_count', _p(vol), _p(counts), N, H, W, D, _s())
    objects = int(counts.sum().item())
    if objects == 0:
        return 0
    ws = _lib.load().ltu_thin_ws_elems(N, H, W, D, objects)
    scratch = torch.empty(ws, device=dev, dtype=torch.int32)
    deleted = torch.empty(THIN_BATCH, device=dev, dtype=torch.int64)
    iterations = 0
    while True:
        _lib.call('ltu_thin_iterate', _p(vol), _p(counts), _p(deleted), THIN_BATCH, _p(scratch), ws, objects, N, H, W, D, _s())
        done = deleted.tolist()
        iterations += sum(1 for n in done if n > 0)
        if min(done) == 0:
            return iterations


def skeletonize(mask):
    """Curve skeleton of every volume of mask [N, H, W, D] or [N, 1, H, W, D] (any dtype, nonzero = object), on the GPU
    (csrc/thinning.hip).  Returns (skeleton u8 [N, H, W, D], iterations).

    8-subfield sequential curve thinning with iteration-level border marking (Palagyi / Nemeth / Kardos).  One iteration marks
    every object voxel with a background face neighbour (beyond the volume is background), then for s = 0 .. 7 deletes every marked
    voxel with (h & 1) | (w & 1) << 1 | (d & 1) << 2 == s that, in the image as it stands, is simple for the (26, 6) pair
    (Malandain-Bertrand) and not an endpoint (exactly one object neighbour among its 26).  Iterations repeat until one deletes
    nothing; `iterations` counts those that deleted a voxel, over all N volumes together.  Deleting simple points only, the
    skeleton has the components, tunnels and cavities of the mask (a cavity keeps a closed surface around it), and thinning a
    skeleton again changes nothing.  Voxels of one subfield are never neighbours, so the result does not depend on scheduling: two
    calls are bit-identical, and the bytes equal a sequential restatement.  It is not Lee's 1994 thinning (skimage), whose
    skeletons differ voxel by voxel.

    Host reads: one of the object counts (it sizes the candidate lists), then one of the deletion counters per THIN_BATCH = 4
    iterations, so 1 + ceil((iterations + 1) / 4) per call.  H W D < 2^31 and N H W D < 2^32.  No CPU fallback."""
    vol = _binary_u8(mask, 'skeletonize')
    if mask.dtype == torch.uint8:
        vol = (vol != 0).view(torch.uint8)      # a copy with values 0 / 1
    elif mask.dtype == torch.bool:
        vol = vol.clone()                       # _binary_u8 returned a view of the caller's tensor
    iterations = _thin_inplace(vol)
    return vol, iterations


def betti_numbers(mask):
    """Betti numbers of every volume of mask [N, H, W, D] or [N, 1, H, W, D] (any dtype, nonzero = object) under 26-connectivity of
    the object and 6-connectivity of the background, on the GPU: int32 device tensors {'Betti0', 'Betti1', 'Betti2', 'Euler'},
    each [N].  Betti0 = label_components(connectivity=3)'s count; Betti2 = the 6-connected background components that reach no
    face of the volume (the labelling of fill_holes, counted); Euler = V - E + F - C of the union of the closed unit cubes of the
    object voxels (distinct lattice vertices, edges, faces and cubes: the cell complex that matches 26-connectivity);
    Betti1 = Betti0 + Betti2 - Euler.  Integer work, no host synchronisation.  H W D < 2^31 and N H W D < 2^32."""
    vol = _binary_u8(mask, 'betti_numbers')
    N, H, W, D = (int(v) for v in vol.shape)
    ws = _lib.load().ltu_fill_holes_ws_elems(N, H, W, D)
    if ws <= 0 or _lib.load().ltu_thin_ws_elems(N, H, W, D, 0) <= 0:
        raise _lib.LtuError(f'betti_numbers: shape {tuple(vol.shape)} refused (N <= 65535, H * W * D < 2^31, N * H * W * D < 2^32)')
    dev = vol.device
    _, b0 = label_components(vol, connectivity=3)
    b2 = torch.empty(N, device=dev, dtype=torch.int32)
    scratch = torch.empty(ws, device=dev, dtype=torch.int32)
    _lib.call('ltu_count_cavities', _p(vol), _p(b2), _p(scratch), ws, N, H, W, D, _s())
    chi = torch.empty(N, device=dev, dtype=torch.int64)
    _lib.call('ltu_euler_characteristic', _p(vol), _p(chi), N, H, W, D, _s())
    chi = chi.to(torch.int32)
    return {'Betti0': b0, 'Betti1': b0 + b2 - chi, 'Betti2': b2, 'Euler': chi}


TOPOLOGY_METRIC_NAMES = ('clDice', 'Tprec', 'Tsens', 'Betti0Error', 'Betti1Error', 'Betti2Error')


def topology_metrics(predict, masks, class_indices=(1,), threshold=0.5):
    """Connectivity metrics of predict [B, C, H, W, D] against the integer label volume masks [B, 1, H, W, D], on the GPU
    (csrc/thinning.hip).  For sample b and class k: P = predict[b, k] >= threshold, G = masks[b, 0] == k, S_X = skeletonize(X).
        Tprec  = |S_P n G| / |S_P|            Tsens = |S_G n P| / |S_G|            clDice = 2 Tprec Tsens / (Tprec + Tsens)
    (the hard-skeleton clDice of Shit et al., with this project's skeleton).  P and G both empty: all three are 1; exactly one
    empty: all three are 0; Tprec + Tsens = 0: clDice 0.  Betti{0,1,2}Error = |b_i(P) - b_i(G)| with betti_numbers.

    Returns {name: device tensor [B, len(class_indices)]} for TOPOLOGY_METRIC_NAMES, the rates f32 (quotients of exact integers,
    one rounding), the errors int32.  One thinning call and one betti_numbers call serve all 2 B K volumes; host reads as
    skeletonize.  No CPU fallback."""
    if not predict.is_cuda:
        raise _lib.LtuError('topology_metrics runs on the GPU only (no CPU fallback)')
    if predict.dim() != 5 or masks.dim() != 5 or masks.shape[1] != 1 or masks.shape[0] != predict.shape[0] \
            or tuple(masks.shape[2:]) != tuple(predict.shape[2:]):
        raise _lib.LtuError(f'predict [B, C, H, W, D] and masks [B, 1, H, W, D] expected, got {tuple(predict.shape)} and '
                            f'{tuple(masks.shape)}')
    B, C, H, W, D = (int(v) for v in predict.shape)
    classes = tuple(int(k) for k in class_indices)
    if not classes or not all(0 <= k < C for k in classes):
        raise _lib.LtuError(f'class_indices {class_indices} outside 0 .. {C - 1}')
    K = len(classes)
    if _lib.load().ltu_thin_ws_elems(min(2 * B * K, 1 << 20), H, W, D, 0) <= 0:
        raise _lib.LtuError(f'topology_metrics: 2 B K = {2 * B * K} volumes of {(H, W, D)} refused (at most 65535 volumes, '
                            f'H * W * D < 2^31, 2 B K H W D < 2^32)')
    dev = predict.device
    pred = predict.to(torch.float32).contiguous()
    tgt = masks.to(dev).reshape(B, H, W, D).to(torch.uint8).contiguous()
    thr = float(threshold)
    sides = torch.empty((2, B, K, H, W, D), device=dev, dtype=torch.uint8)
    for kk, k in enumerate(classes):
        _lib.call('ltu_topology_binarize', _p(pred), _p(tgt), _p(sides), B, C, k, kk, K, H, W, D, thr, _s())
    betti = betti_numbers(sides.view(2 * B * K, H, W, D))
    _thin_inplace(sides.view(2 * B * K, H, W, D))
    counts = torch.empty((B, K, 4), device=dev, dtype=torch.int32)
    rates = torch.empty((3, B, K), device=dev, dtype=torch.float32)
    for kk, k in enumerate(classes):
        _lib.call('ltu_topology_overlap', _p(pred), _p(tgt), _p(sides), _p(counts), _p(rates), B, C, k, kk, K, H, W, D, thr, _s())
    out = {name: rates[i] for i, name in enumerate(TOPOLOGY_METRIC_NAMES[:3])}
    for i in range(3):
        b = betti[f'Betti{i}'].view(2, B, K)
        out[f'Betti{i}Error'] = (b[0] - b[1]).abs()
    return out


def remove_small_components(predict, min_voxels, class_indices=None, connectivity=3):
    """Small-object removal on predict [B, C, H, W, D] f32 (the votes of sliding_window_inference or a one-hot), on the GPU
    (csrc/components.hip): out = torch.round(predict); then for each class k of class_indices (default 1 .. C-1), each class on its
    own, every component (see label_components for the connectivity) of out[b, k] > 0 with fewer than min_voxels voxels is
    cleared in channel k; channel 0 = 1 - the sum of the other channels.  min_voxels <= 1 returns the rounded input unchanged.
    Returns a new tensor; no host synchronisation."""
    if not predict.is_cuda:
        raise _lib.LtuError('remove_small_components runs on the GPU only (no CPU fallback)')
    if predict.dim() != 5:
        raise _lib.LtuError(f'predict [B, C, H, W, D] expected, got {tuple(predict.shape)}')
    conn = _connectivity(connectivity)
    B, C, H, W, D = (int(v) for v in predict.shape)
    if not 2 <= C <= 31:
        raise _lib.LtuError(f'remove_small_components supports 2 .. 31 classes, got C = {C}')
    classes = tuple(range(1, C)) if class_indices is None else tuple(int(k) for k in class_indices)
    if not classes or not all(1 <= k < C for k in classes):
        raise _lib.LtuError(f'class_indices {class_indices} outside 1 .. {C - 1}')
    out = torch.round(predict.to(torch.float32)).contiguous()
    if min_voxels <= 1:
        return out
    ws = _lib.load().ltu_remove_small_ws_elems(B, H, W, D)
    if ws <= 0:
        raise _lib.LtuError(f'remove_small_components: shape {tuple(predict.shape)} refused (H * W * D must be < 2^31)')
    bits = 0
    for k in classes:
        bits |= 1 << k
    scratch = torch.empty(ws, device=out.device, dtype=torch.int32)
    _lib.call('ltu_remove_small_components', _p(out), _p(scratch), ws, B, C, bits, H, W, D, int(min(min_voxels, 2 ** 31 - 1)), conn,
              _s())
    return out


LESION_METRIC_NAMES = ('NumTrue', 'NumPred', 'TruePositives', 'FalseNegatives', 'FalsePositives', 'Sensitivity', 'Precision', 'F1',
                       'LesionDice')


def lesion_metrics(predict, masks, class_indices=(1,), threshold=0.5, connectivity=3):
    """Lesion-wise (object) detection metrics of predict [B, C, H, W, D] against the class ids masks [B, 1, H, W, D], on the GPU
    (csrc/components.hip).  For sample b and class k: P = predict[b, k] >= threshold and G = masks[b, 0] == k, both labelled with
    the given connectivity (see label_components) into components P_1 .. P_m and G_1 .. G_n.  o_j = |G_j n P|; GT lesion j is
    detected iff o_j >= 1; predicted component i is a false positive iff P_i n G is empty; U_j = the union of the P_i touching G_j;
    Dice_j = 2 o_j / (|G_j| + |U_j|) (0 for a missed lesion; |G_j n U_j| = o_j).
        NumTrue = n, NumPred = m, TruePositives = detected GT lesions, FalseNegatives = n - TruePositives, FalsePositives
        Sensitivity = TP / n, 1 when n = 0                 Precision = (m - FP) / m, 1 when m = 0
        F1 = 2 S P / (S + P), 0 when S + P = 0            LesionDice = sum_j Dice_j / (n + FP), 1 when n + FP = 0
    (LesionDice is the BraTS-2023 lesion-wise form without its GT dilation.)  Returns {name: [B, len(class_indices)] device
    tensor} for LESION_METRIC_NAMES: the five counts int32, the four rates f32; callers pool counts across scans themselves.
    Integer statistics and a fixed-order fp64 fold: two calls are bit-identical.  One host read per call, for sizing: the bound
    on distinct (P_i, G_j) pairs that sizes the device hash set."""
    if not predict.is_cuda:
        raise _lib.LtuError('lesion_metrics runs on the GPU only (no CPU fallback)')
    if predict.dim() != 5 or masks.dim() != 5 or masks.shape[1] != 1 or masks.shape[0] != predict.shape[0] \
            or tuple(masks.shape[2:]) != tuple(predict.shape[2:]):
        raise _lib.LtuError(f'predict [B, C, H, W, D] and masks [B, 1, H, W, D] expected, got {tuple(predict.shape)} and '
                            f'{tuple(masks.shape)}')
    conn = _connectivity(connectivity)
    B, C, H, W, D = (int(v) for v in predict.shape)
    classes = tuple(int(k) for k in class_indices)
    if not classes or not all(0 <= k < min(C, 256) for k in classes):
        raise _lib.LtuError(f'class_indices {class_indices} outside 0 .. {min(C, 256) - 1}')
    thr = float(threshold)
    if thr != thr:
        raise _lib.LtuError('threshold must not be NaN')
    K = len(classes)
    dev = predict.device
    lib = _lib.load()
    if lib.ltu_label_ws_elems(B, H, W, D) <= 0:
        raise _lib.LtuError(f'lesion_metrics: shape {tuple(predict.shape)} refused (H * W * D must be < 2^31)')
    pred = predict.to(torch.float32).contiguous()
    tgt = masks.to(dev).reshape(B, H, W, D).to(torch.uint8).contiguous()
    heads = torch.empty((K, B), device=dev, dtype=torch.int32)
    for kk, k in enumerate(classes):
        _lib.call('ltu_lesion_heads', _p(pred), _p(tgt), _p(heads[kk]), B, C, k, H, W, D, thr, conn, _s())
    pairs = int(heads.max().item())          # the one host read of the call: sizes the pair hash set
    ws = lib.ltu_lesion_ws_elems(B, H, W, D, pairs)
    scratch = torch.empty(ws, device=dev, dtype=torch.int32)
    ints = torch.empty((5, B, K), device=dev, dtype=torch.int32)
    rates = torch.empty((4, B, K), device=dev, dtype=torch.float32)
    for kk, k in enumerate(classes):
        _lib.call('ltu_lesion_stats', _p(pred), _p(tgt), _p(ints), _p(rates), _p(scratch), ws, pairs, B, C, k, kk, K, H, W, D, thr,
                  conn, _s())
    res = {name: ints[i] for i, name in enumerate(LESION_METRIC_NAMES[:5])}
    res.update({name: rates[i] for i, name in enumerate(LESION_METRIC_NAMES[5:])})
    return res


class GraphedPredictor:
    """The eval-mode forward for a fixed window batch captured once into a HIP graph and replayed per window batch: an eager
    forward is ~500 launches of ~35 us host time each, several times what the kernels need.  A short last batch is padded with
    copies of its first window (their outputs are dropped).  probs=True captures model(x, probs=True), the softmax the one-hot
    arg-max is taken from (the input of mode='gaussian' / mirrored blending)."""

    def __init__(self, model, batch, roi, device, probs=False):
        self.model, self.n, self.probs = model, batch, bool(probs)
        self.x = torch.zeros((batch, model.dim_input) + tuple(roi), device=device, dtype=torch.float32)
        self.ctx = ops.Context()          # own scratch arena: the graph bakes its addresses in, nobody else may move it
        fwd = (lambda x: model(x, probs=True)) if self.probs else model
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side), torch.no_grad(), ops.use(self.ctx):
            for _ in range(2):
                fwd(self.x)
        torch.cuda.current_stream(device).wait_stream(side)
        torch.cuda.synchronize(device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode='thread_local'), torch.no_grad(), ops.use(self.ctx):
            self.y = fwd(self.x)
        self.ctx.freeze()
        self.sig = tuple(p.data_ptr() for p in model.parameters())

    def __call__(self, win):
        if tuple(p.data_ptr() for p in self.model.parameters()) != self.sig:
            raise _lib.LtuError('GraphedPredictor: parameter storage moved since capture (build the predictor after .to() / '
                                'optimizer construction, or build a new one)')
        n = win.shape[0]
        self.x[:n].copy_(win)
        if n < self.n:
            self.x[n:].copy_(win[:1].expand(self.n - n, *win.shape[1:]))
        self.graph.replay()
        return self.y[:n]


def infer_volume(model, images, depth_size=32, roi_xy=512, sw_batch_size=4, overlap=0.6, graph=False, mode='constant',
                 sigma_scale=0.125, mirror_axes=(), probs=False):
    """one patient of inference_embed_attn.py:main: eval-mode model, (roi_xy, roi_xy, depth_size) windows, overlap 0.6.
    graph=True (or a GraphedPredictor built earlier) replays the forward from a captured HIP graph.  mode, sigma_scale and
    mirror_axes go to sliding_window_inference; probs=True blends the model's softmax instead of its one-hot arg-max (a
    GraphedPredictor passed as graph brings its own probs).  The defaults are the reference's call."""
    _blend_options(mode, sigma_scale, mirror_axes)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            predictor = (lambda w: model(w, probs=True)) if probs else model
            if isinstance(graph, GraphedPredictor):
                predictor = graph
            elif graph:
                roi = tuple(r if r and r > 0 else i for r, i in zip((roi_xy, roi_xy, depth_size), images.shape[2:]))
                predictor = GraphedPredictor(model, sw_batch_size, roi, images.device, probs=probs)
            return sliding_window_inference(images, (roi_xy, roi_xy, depth_size), sw_batch_size, predictor, overlap=overlap,
                                            mode=mode, sigma_scale=sigma_scale, mirror_axes=mirror_axes)
    finally:
        model.train(was_training)


def segment_scan(models, scan, classes=(), **infer_volume_kwargs):
    """a data.SpacedScan (or MultiScan) to its prediction on the file's grid: infer_volume(model, scan.img[None, None] (a
    MultiScan: scan.img[None]), probs=True, ...) per
    member of `models` (one model or a sequence: the folds or checkpoints of an ensemble), the members' softmaxes summed in fp32 in
    member order, then one data.to_native_probs.  Defaults here: mode='gaussian', mirror_axes=(0, 1); every other default is
    infer_volume's.  The sum is not divided for the label (the arg-max does not change under a positive scale); with `classes` it is
    scaled by 1 / len(models) first, so the returned probabilities are the members' mean.
    Returns to_native_probs' pair (u8 label [Z][Y][X], f32 [K][Z][Y][X] or None).
    Region models (MaskTransUnet(..., regions=...); all members must carry equal records, with a class_order and R >= 2 regions,
    which is what to_native_probs takes): the members' sigmoids are summed and always divided by the member count, every region's
    plane goes through to_native_probs(classes=range(R)), and region_labels paints the label from the planes on the file's grid
    (threshold 0.5; outside a cropped scan's box every region is 0).  `classes` is not used.  Returns (u8 label [Z][Y][X], f32
    [R][Z][Y][X])."""
    members = [models] if isinstance(models, torch.nn.Module) else list(models)
    if not members:
        raise ValueError('segment_scan needs at least one model')
    regions = getattr(members[0], 'regions', None)
    if any(getattr(model, 'regions', None) != regions for model in members):
        raise ValueError('segment_scan: the members of an ensemble must all be class models or carry equal Regions records')
    if regions is not None and (regions.class_order is None or len(regions.members) < 2):
        raise ValueError('segment_scan: a region model needs a class_order and at least 2 regions (data.to_native_probs takes 2 .. 8 planes)')
    kw = dict(mode='gaussian', mirror_axes=(0, 1))
    kw.update(infer_volume_kwargs)
    total = None
    images = scan.img.view(1, -1, *scan.img.shape[-3:])          # [1, K, H, W, D]; a SpacedScan is K = 1
    for model in members:
        p = infer_volume(model, images, probs=True, **kw)
        total = p if total is None else total.add_(p)
    if regions is not None:
        if len(members) > 1:
            total.mul_(1.0 / len(members))
        _, planes = data.to_native_probs(total, scan, classes=range(len(regions.members)))
        box = getattr(scan, 'crop_box', None)
        if box is not None:      # to_native_probs fills plane 0 with 1 outside the box (a class model's background): no region lives there
            (z0, z1), (y0, y1), (x0, x1) = box
            inside = planes[:, z0:z1, y0:y1, x0:x1]
            planes = torch.zeros_like(planes)
            planes[:, z0:z1, y0:y1, x0:x1].copy_(inside)
        return region_labels(planes, regions), planes
    if classes and len(members) > 1:
        total.mul_(1.0 / len(members))
    return data.to_native_probs(total, scan, classes)
