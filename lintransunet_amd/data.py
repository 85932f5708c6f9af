"""Data side of the training scripts on the device.

dataset/CT_pancreas_ids.py:143-173: `.npy` scan [D,H,W] -> HU clip [-91, 250] -> (x - 86.9) / 39.4 -> [H,W,D] float32, label uint8;
then RandCropByPosNegLabeld(pos=0.7, neg=0.3, num_samples) and RandFlipd(prob=0.4, spatial_axis=(0, 1)) of monai 0.7.0.  A scan
is uploaded once; preprocessing, cropping and flipping are HIP kernels (csrc/data.hip).  Crop centres are drawn on the host from
the label's foreground / background index lists exactly as monai does (`crop_centers`), or, without a pass over the label per
sample, from a `CropIndex` of the device label (csrc/crop_index.hip): the host keeps the draws and needs only the populations.
`augment` applies the remaining augmentations of the reference (RandRotated, RandAdjustContrastd, RandZoomd, RandFlipd;
CT_pancreas_ids.py:121-134) to a batch of patches on the device; the random draws stay on the host.
The third driver's data side (train3D_monai_version.py with dataset/CT_pancreas_monai.py: NIfTI scans of the Medical
Segmentation Decathlon layout, ScaleIntensityRanged -> Spacingd -> Orientationd('RAS'), then crop + RandFlipd + RandRotate90d) is
`SpacedScan` / `sample` / `to_native` / `to_native_probs` at the end of this file.  Scans and patches have 1 to 4 channels and one
path each: `SpacedScan` and `MultiScan` load through `SpacedScan._load` and `_load_channel`, and `sample_affine` gathers a 3-D image
as the one-channel case of `ltu_sample_channels` (order 1) or `ltu_sample_spline` (cubic).
"""
import functools
import warnings

import numpy as np
import torch

from . import _lib, geometry, nifti
from .ops import _p, _s

LOW_CLIP, HIGH_CLIP, MEAN, STD = -91.0, 250.0, 86.9, 39.4


def preprocess(raw_img, raw_label, device='cuda'):
    """raw [D,H,W] numpy arrays / tensors -> (img f32 [H,W,D], label u8 [H,W,D]) on the device"""
    ri = torch.as_tensor(np.ascontiguousarray(raw_img), dtype=torch.float32).to(device)
    rl = torch.as_tensor(np.ascontiguousarray(raw_label)).to(torch.uint8).to(device)
    if not ri.is_cuda:
        raise _lib.LtuError('data.preprocess runs on the GPU only (no CPU fallback)')
    D, H, W = ri.shape
    img = torch.empty((H, W, D), device=ri.device, dtype=torch.float32)
    lab = torch.empty((H, W, D), device=ri.device, dtype=torch.uint8)
    _lib.call('ltu_ct_preprocess', _p(ri), _p(img), _p(rl), _p(lab), D, H, W, LOW_CLIP, HIGH_CLIP, MEAN, STD, _s())
    return img, lab


def correct_crop_centers(centers, spatial_size, label_shape):
    """monai/transforms/utils.py::correct_crop_centers (0.7.0)"""
    out = []
    for c, s, n in zip(centers, spatial_size, label_shape):
        if n < s:
            raise ValueError('The size of the proposed random crop ROI is larger than the image size.')
        lo = s // 2
        hi = int(np.uint16(n + 1 - s / 2))
        if lo == hi:
            hi += 1
        out.append(int(min(max(c, lo), hi - 1)))
    return out


def crop_centers(label, spatial_size, num_samples, pos=0.7, neg=0.3, rand_state=None):
    """centres of RandCropByPosNegLabeld; label: host array [H,W,D]"""
    rs = rand_state or np.random.RandomState()
    flat = (np.asarray(label) > 0).ravel()
    fg, bg = np.nonzero(flat)[0], np.nonzero(~flat)[0]
    pos_ratio = pos / (pos + neg)
    if fg.size == 0 and bg.size == 0:
        raise ValueError('No sampling location available.')
    if fg.size == 0 or bg.size == 0:
        pos_ratio = 0 if fg.size == 0 else 1
    centers = []
    for _ in range(num_samples):
        use = fg if rs.rand() < pos_ratio else bg
        idx = use[rs.randint(len(use))]
        centers.append(correct_crop_centers(list(np.unravel_index(idx, np.asarray(label).shape)), spatial_size, np.asarray(label).shape))
    return centers


FG_MASK, BG_MASK = 0x1fe, 0x001        # bin sets of ltu_crop_index_select: bit b = label value b, bit 8 = every value >= 8


def _posneg_queries(n_fg, n_bg, num_samples, pos, neg, rs):
    """crop_centers' draws from the two populations alone: (bin mask, rank) per sample"""
    pos_ratio = pos / (pos + neg)
    if n_fg == 0 and n_bg == 0:
        raise ValueError('No sampling location available.')
    if n_fg == 0 or n_bg == 0:
        pos_ratio = 0 if n_fg == 0 else 1
    queries = []
    for _ in range(num_samples):
        mask, count = (FG_MASK, n_fg) if rs.rand() < pos_ratio else (BG_MASK, n_bg)
        queries.append((mask, int(rs.randint(count))))
    return queries


def _class_queries(counts, num_samples, ratios, rs):
    """generate_label_classes_crop_centers' draws from the class populations alone: (bin mask, rank) per sample"""
    if num_samples < 1:
        raise ValueError('num_samples must be an int number and greater than 0.')
    ratios = [1] * len(counts) if ratios is None else list(ratios)
    if len(ratios) != len(counts):
        raise ValueError('random crop ratios must match the number of indices of classes.')
    if any(r < 0 for r in ratios):
        raise ValueError('ratios should not contain negative number.')
    for c, count in enumerate(counts):
        if count == 0:
            warnings.warn(f'no available indices of class {c} to crop, set the crop ratio of this class to zero.')
            ratios[c] = 0
    classes = rs.choice(len(ratios), size=num_samples, p=np.asarray(ratios) / np.sum(ratios))
    return [(1 << int(c), int(rs.randint(counts[c]))) for c in classes]


def _default_num_classes(counts):
    """the highest populated class bin + 1 (the bin of the values >= 8 is never a class)"""
    return max([c + 1 for c in range(8) if counts[c] > 0], default=1)


def class_crop_centers(label, spatial_size, num_samples, ratios=None, num_classes=None, rand_state=None):
    """centres of RandCropByLabelClassesd; label: host array [H,W,D] of class ids.  A numpy restatement of monai 0.7.0's
    map_classes_to_indices + generate_label_classes_crop_centers (recalled, not pinned: monai is absent): the indices of class c
    < num_classes are np.nonzero((label == c).ravel())[0]; ratios (default: all ones) must be non-negative and one per class, the
    ratio of an empty class becomes 0 with a warning; classes = rs.choice(len(ratios), size=num_samples, p=ratios / sum), then per
    sample rs.randint(len(indices[c])), unravel, correct_crop_centers.  num_classes None (monai demands it for a label that is not
    one-hot) = the highest class 0 .. 7 present + 1."""
    rs = rand_state or np.random.RandomState()
    label = np.asarray(label)
    flat = label.ravel()
    if num_classes is None:
        num_classes = _default_num_classes(np.bincount(flat.astype(np.int64), minlength=8))
    indices = [np.nonzero(flat == c)[0] for c in range(num_classes)]
    queries = _class_queries([len(i) for i in indices], num_samples, ratios, rs)
    return [correct_crop_centers(list(np.unravel_index(indices[mask.bit_length() - 1][rank], label.shape)), spatial_size, label.shape)
            for mask, rank in queries]


class CropIndex:
    """Per-scan crop index of a u8 device label [H, W, D] (csrc/crop_index.hip): built once, it answers "the r-th voxel of this set
    of label values in raster order" on the device, so drawing a crop centre costs one block of the label instead of np.nonzero
    passes over all of it.  Construction builds the index and reads the 9 populations back (the one synchronisation per scan):
    counts[b] = voxels of value b for b < 8, counts[8] = voxels of every value >= 8 (foreground to crop_centers, never a class)."""

    def __init__(self, lab):
        if not torch.is_tensor(lab) or not lab.is_cuda:
            raise _lib.LtuError('data.CropIndex is built from the device label (no CPU fallback)')
        if lab.dtype != torch.uint8 or lab.dim() != 3:
            raise ValueError(f'CropIndex takes a uint8 label [H, W, D], got {lab.dtype} {tuple(lab.shape)}')
        self.lab = lab.contiguous()
        self.shape = tuple(int(n) for n in lab.shape)
        self.n_voxels = self.lab.numel()
        elems = _lib.load().ltu_crop_index_elems(self.n_voxels)
        if elems == 0 and self.n_voxels > 0:
            raise ValueError(f'CropIndex: a label of {self.n_voxels} voxels is beyond 2^32 - 1')
        self.index = torch.empty(elems, device=lab.device, dtype=torch.int32)          # uint32 words
        if self.n_voxels == 0:                       # nothing to build: every draw from it raises as crop_centers does
            self.counts = (0,) * 9
        else:
            totals = torch.empty(9, device=lab.device, dtype=torch.int64)
            _lib.call('ltu_crop_index_build', _p(self.lab), self.n_voxels, _p(self.index), elems, _p(totals), _s())
            self.counts = tuple(int(v) for v in totals.cpu().tolist())
        self.n_background = self.counts[0]
        self.n_foreground = sum(self.counts[1:])

    def select(self, queries):
        """queries [(bin mask, rank)] -> int64 numpy [n] of linear voxel indices (-1: rank not below the set's population); one
        launch and one read-back"""
        n = len(queries)
        if n == 0:
            return np.zeros(0, dtype=np.int64)
        q = torch.from_numpy(np.asarray(queries, dtype=np.uint32).reshape(n, 2).view(np.int32)).to(self.lab.device)
        out = torch.empty(n, device=self.lab.device, dtype=torch.int64)
        _lib.call('ltu_crop_index_select', _p(self.lab), self.n_voxels, _p(self.index), self.index.numel(), _p(q), _p(out), n, _s())
        return out.cpu().numpy()

    def resolve(self, queries, spatial_size):
        """the corrected centres [h, w, d] of drawn queries"""
        idx = self.select(queries)
        if (idx < 0).any():
            raise _lib.LtuError('CropIndex: a drawn rank is beyond its population (the label changed after the index was built)')
        return [correct_crop_centers(list(np.unravel_index(i, self.shape)), spatial_size, self.shape) for i in idx]

    def centers(self, spatial_size, num_samples, pos=0.7, neg=0.3, rand_state=None):
        """crop_centers(label_host, ...) from the index: the same draws from rand_state in the same order, the same centres"""
        rs = rand_state or np.random.RandomState()
        return self.resolve(_posneg_queries(self.n_foreground, self.n_background, num_samples, pos, neg, rs), spatial_size)

    def class_queries(self, num_samples, ratios=None, num_classes=None, rand_state=None):
        rs = rand_state or np.random.RandomState()
        if num_classes is None:
            num_classes = _default_num_classes(self.counts)
        if not 1 <= num_classes <= 8:
            raise ValueError(f'CropIndex keeps 8 classes, got num_classes {num_classes}')
        return _class_queries(list(self.counts[:num_classes]), num_samples, ratios, rs)

    def class_centers(self, spatial_size, num_samples, ratios=None, num_classes=None, rand_state=None):
        """class_crop_centers(label_host, ...) from the index: the same draws, the same centres; num_classes <= 8"""
        return self.resolve(self.class_queries(num_samples, ratios, num_classes, rand_state), spatial_size)


def crop_flip(img, lab, centers, flips, spatial_size):
    """device patches: ([n,1,h,w,d] f32, [n,1,h,w,d] u8) from img / lab [H,W,D] at the given centres; flips[k] mirrors H and W"""
    H, W, D = img.shape
    h, w, d = spatial_size
    desc = torch.tensor([[max(c[0] - h // 2, 0), max(c[1] - w // 2, 0), max(c[2] - d // 2, 0), int(f), int(f)] for c, f in zip(centers, flips)],
                        dtype=torch.int32).to(img.device)
    n = len(centers)
    oi = torch.empty((n, 1, h, w, d), device=img.device, dtype=torch.float32)
    ol = torch.empty((n, 1, h, w, d), device=img.device, dtype=torch.uint8)
    _lib.call('ltu_crop_flip', _p(img), _p(oi), _p(desc), n, H, W, D, h, w, d, 4, _s())
    _lib.call('ltu_crop_flip', _p(lab), _p(ol), _p(desc), n, H, W, D, h, w, d, 1, _s())
    return oi, ol


def sample_patches(img, lab, label_host, spatial_size, num_samples, rand_state, flip_prob=0.4, index=None):
    """one `__getitem__` of IdPosPanCTDataset without the rotate / contrast / zoom augmentations; with index, the CropIndex of
    lab, the centres come from it (the same centres from the same draws) and label_host is not read (it may be None)"""
    if index is not None:
        centers = index.centers(spatial_size, num_samples, rand_state=rand_state)
    else:
        centers = crop_centers(label_host, spatial_size, num_samples, rand_state=rand_state)
    flips = [rand_state.rand() < flip_prob for _ in range(num_samples)]
    return crop_flip(img, lab, centers, flips, spatial_size)


# ---- augmentations (CT_pancreas_ids.py:121-134) -----------------------------------------------------------------------------

def rotate_matrix(angles, shape):
    """monai create_rotate (Rx @ Ry @ Rz) about the patch centre, as a 3x4 float32 pull matrix (output voxel -> input location)"""
    ax, ay, az = (float(a) for a in angles)
    rx = np.array([[1, 0, 0, 0], [0, np.cos(ax), -np.sin(ax), 0], [0, np.sin(ax), np.cos(ax), 0], [0, 0, 0, 1]], dtype=np.float64)
    ry = np.array([[np.cos(ay), 0, np.sin(ay), 0], [0, 1, 0, 0], [-np.sin(ay), 0, np.cos(ay), 0], [0, 0, 0, 1]], dtype=np.float64)
    rz = np.array([[np.cos(az), -np.sin(az), 0, 0], [np.sin(az), np.cos(az), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    c = (np.asarray(shape, dtype=np.float64) - 1) / 2
    sh, sh1 = np.eye(4), np.eye(4)
    sh[:3, 3], sh1[:3, 3] = c, -c
    return (sh @ rx @ ry @ rz @ sh1)[:3].astype(np.float32)


_IDENTITY = np.eye(4, dtype=np.float32)[:3]


def draw_augmentation(rs, rot_prob=0.1, rot_range=np.pi / 9, prob=0.4, zoom=(0.7, 1.3), gamma=(0.5, 4.5)):
    """one sample's random parameters in the reference's transform order; every draw is made whether or not the transform fires"""
    p = {}
    p['rotate'] = rs.rand() < rot_prob
    p['angles'] = [rs.uniform(-rot_range, rot_range) for _ in range(3)]
    p['contrast'] = rs.rand() < prob
    p['gamma'] = rs.uniform(*gamma)
    p['zoom'] = rs.rand() < prob
    p['zoom_factor'] = rs.uniform(*zoom)
    p['flip'] = rs.rand() < prob
    return p


def _vol4(t):
    if not t.is_cuda:
        raise _lib.LtuError('data augmentations run on the GPU only (no CPU fallback)')
    n = t.shape[0]
    return t.reshape(n, *t.shape[-3:]).contiguous()


def rotate(x, mats):
    """x [n,(1,)H,W,D] f32, mats [n,3,4]: trilinear pull resampling with border padding (monai Rotate, keep_size)"""
    v = _vol4(x)
    n, H, W, D = v.shape
    m = torch.as_tensor(np.ascontiguousarray(mats, dtype=np.float32).reshape(n, 12)).to(v.device)
    out = torch.empty_like(v)
    _lib.call('ltu_affine_sample', _p(v), _p(out), _p(m), n, H, W, D, _s())
    return out.view(x.shape)


def zoom(x, factors):
    """monai Zoom(keep_size=True): trilinear align_corners interpolation to floor(size*f) + centred edge pad / crop"""
    v = _vol4(x)
    n, H, W, D = v.shape
    # output size of F.interpolate(scale_factor=f): floor(size * f) in double precision
    z = torch.tensor([[max(int(np.floor(float(sz) * float(f))), 1) for sz in (H, W, D)] for f in factors], dtype=torch.int32).to(v.device)
    out = torch.empty_like(v)
    _lib.call('ltu_zoom_sample', _p(v), _p(out), _p(z), n, H, W, D, _s())
    return out.view(x.shape)


def adjust_contrast(x, gammas):
    """monai AdjustContrast per patch; gamma <= 0 leaves a patch untouched"""
    v = _vol4(x)
    n = v.shape[0]
    g = torch.as_tensor(np.asarray(gammas, dtype=np.float32)).to(v.device)
    ws = torch.empty(2 * n, device=v.device, dtype=torch.int32)
    out = torch.empty_like(v)
    _lib.call('ltu_adjust_contrast', _p(v), _p(out), _p(g), _p(ws), n, v.numel() // n, _s())
    return out.view(x.shape)


def augment(img, lab, params):
    """img f32 [n,1,h,w,d], lab u8 [n,1,h,w,d], params: one draw_augmentation() dict per patch -> augmented (f32, u8).
    The label is resampled in float and truncated back to uint8 as the reference does (CT_pancreas_ids.py:171)."""
    n = img.shape[0]
    shape = tuple(img.shape[-3:])
    lf = lab.to(torch.float32)
    if any(p['rotate'] for p in params):
        mats = np.stack([rotate_matrix(p['angles'], shape) if p['rotate'] else _IDENTITY for p in params])
        img, lf = rotate(img, mats), rotate(lf, mats)
    if any(p['contrast'] for p in params):
        img = adjust_contrast(img, [p['gamma'] if p['contrast'] else -1.0 for p in params])
    if any(p['zoom'] for p in params):
        f = [p['zoom_factor'] if p['zoom'] else 1.0 for p in params]
        img, lf = zoom(img, f), zoom(lf, f)
    lab8 = lf.to(torch.uint8)
    if any(p['flip'] for p in params):
        h, w, d = shape
        flips = [p['flip'] for p in params]
        oi = torch.empty_like(img)
        ol = torch.empty_like(lab8)
        desc = torch.tensor([[0, 0, 0, int(f), int(f)] for f in flips], dtype=torch.int32).to(img.device)
        for k in range(n):                       # every patch is its own "volume" here: crop of the full extent, optional mirror
            _lib.call('ltu_crop_flip', _p(img[k]), _p(oi[k]), _p(desc[k]), 1, h, w, d, h, w, d, 4, _s())
            _lib.call('ltu_crop_flip', _p(lab8[k]), _p(ol[k]), _p(desc[k]), 1, h, w, d, h, w, d, 1, _s())
        img, lab8 = oi, ol
    return img, lab8


def synthetic_patches(batch, size, seed, device, n_classes=2, n_blobs=2, n_channels=1):
    """Synthetic CT-like training patches for benchmarks and soak runs: N(0,1) intensities clipped to
    the dataset's normalised HU range [(-91 - 86.9) / 39.4, (250 - 86.9) / 39.4] and a label volume that is a union of `n_blobs`
    random ellipsoids per patch (nested twice for 3 label values; for 4 .. 8 label values one further ellipsoid per class 2 .. k-1, every
    class 1 .. k-1 present in every patch).  Host generators (seeded), uploaded once: a benchmark keeps its
    inputs resident in HBM.  Returns (x f32 [B,n_channels,H,W,D], label u8 [B,1,H,W,D]); n_channels > 1 draws that many intensity
    volumes per patch ahead of the label's draws (1 draws what it always drew)."""
    g = torch.Generator().manual_seed(seed)
    H, W, D = size
    x = torch.randn((batch, int(n_channels), H, W, D), generator=g).clamp_((LOW_CLIP - MEAN) / STD, (HIGH_CLIP - MEAN) / STD)
    hh = torch.arange(H, dtype=torch.float32).view(H, 1, 1)
    ww = torch.arange(W, dtype=torch.float32).view(1, W, 1)
    dd = torch.arange(D, dtype=torch.float32).view(1, 1, D)
    lab = torch.zeros((batch, 1, H, W, D), dtype=torch.uint8)
    for b in range(batch):
        for _ in range(n_blobs):
            c = 0.25 + 0.5 * torch.rand(3, generator=g)
            r = 0.12 + 0.15 * torch.rand(3, generator=g)
            dist = ((hh - c[0] * H) / (r[0] * H)) ** 2 + ((ww - c[1] * W) / (r[1] * W)) ** 2 + ((dd - c[2] * D) / (r[2] * D)) ** 2
            lab[b, 0][dist <= 1.0] = 1
            if n_classes == 3:
                lab[b, 0][dist <= 0.25] = 2
        if n_classes >= 4 and n_blobs > 0:
            # 4 .. 8 label values: one more ellipsoid per class 2 .. k-1, painted in class order; then the centre voxel of every
            # class's ellipsoid (class 1: the last blob's) is set to its own value, so that no later ellipsoid covers a class completely
            centres = [(1, c)]
            for k in range(2, n_classes):
                c = 0.2 + 0.6 * torch.rand(3, generator=g)
                r = 0.08 + 0.10 * torch.rand(3, generator=g)
                dist = ((hh - c[0] * H) / (r[0] * H)) ** 2 + ((ww - c[1] * W) / (r[1] * W)) ** 2 + ((dd - c[2] * D) / (r[2] * D)) ** 2
                lab[b, 0][dist <= 1.0] = k
                centres.append((k, c))
            taken = set()
            for k, c in centres:
                pos = [min(int(c[a] * n), n - 1) for a, n in enumerate((H, W, D))]
                while tuple(pos) in taken:                  # two centres in one voxel: the next one along D
                    pos[2] = (pos[2] + 1) % D
                taken.add(tuple(pos))
                lab[b, 0, pos[0], pos[1], pos[2]] = k
    return x.to(device), lab.to(device)


# ---- the monai driver's data side (dataset/CT_pancreas_monai.py:37-58 training, :91-105 evaluation) ---------------------------
# LoadImaged (nifti.py) -> ScaleIntensityRanged(a_min -96, a_max 215, b = (a - 77.99) / 75.4, clip) -> Spacingd((0.5, 0.5, 2.0),
# bilinear / nearest) -> Orientationd('RAS') as ONE resampling kernel through the float64 pull matrix of geometry.spacing_plan
# (csrc/resample.hip), then RandCropByPosNegLabeld -> RandFlipd(0.5, axis 0) -> RandRotate90d(0.5, axes (0, 1)) as one gather.

MONAI_CT_WINDOW = (-96.0, 215.0, (-96.0 - 77.99) / 75.4, (215.0 - 77.99) / 75.4)      # a_min, a_max, b_min, b_max (clip=True)


def intensity_map(window=MONAI_CT_WINDOW, slope=1.0, inter=0.0):
    """(alpha, beta, lo, hi) with clamp(alpha * v + beta, lo, hi) = ScaleIntensityRange(window, clip)(v * slope + inter);
    window None leaves the (slope / intercept-scaled) voxels unchanged"""
    if window is None:
        return float(slope), float(inter), -np.inf, np.inf
    a_min, a_max, b_min, b_max = (float(v) for v in window)
    if a_max - a_min == 0.0:                       # monai: img - a_min + b_min
        return float(slope), float(inter) - a_min + b_min, min(b_min, b_max), max(b_min, b_max)
    k = (b_max - b_min) / (a_max - a_min)
    return float(slope) * k, (float(inter) - a_min) * k + b_min, min(b_min, b_max), max(b_min, b_max)


def _source_dtype(a):
    """the three source dtypes the kernel reads; anything else goes through float32"""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return a, _lib.U8
    if a.dtype == np.int16:
        return a, _lib.I16
    return a.astype(np.float32), 0


def label_u8(a):
    """label voxels as uint8 class ids; values outside 0..255 or not integral are refused"""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return a
    if a.size and (a.min() < 0 or a.max() > 255 or not np.array_equal(a, np.round(a))):
        raise ValueError('labels must be integers in 0..255')
    return a.astype(np.uint8)


SPLINE_ORDERS = (0, 1, 3)             # per source axis: nearest, linear, cubic B-spline


def _order_tuple(order):
    """an `order` argument as a 3-tuple of ints: the int 1 or 3 stands for all three axes, a sequence must be exactly three ints;
    None for anything else.  resolve_order and sample_order each admit their own tuples and word their own refusal."""
    if isinstance(order, (int, np.integer)) and not isinstance(order, bool):
        return (int(order),) * 3 if int(order) in (1, 3) else None
    try:
        orders = tuple(int(o) for o in order)
        exact = len(orders) == 3 and all(o == v for o, v in zip(orders, order))
    except (TypeError, ValueError):
        return None
    return orders if exact else None


def resolve_order(order):
    """an interpolation `order` (1, 3, or one of 0 / 1 / 3 per source axis) as the 3-tuple the kernels take.  Built: (1, 1, 1) (the
    trilinear kernel), (3, 3, 3), and 3 on two axes with 0 or 1 on the third; anything else is a ValueError."""
    orders = _order_tuple(order)
    if orders is None or any(o not in SPLINE_ORDERS for o in orders):
        raise ValueError(f'order is 1, 3 or a 3-tuple of {SPLINE_ORDERS}, got {order!r}')
    if orders != (1, 1, 1) and sum(o == 3 for o in orders) < 2:
        raise ValueError(f'orders {orders} are not built: (1, 1, 1), (3, 3, 3), or 3 on two axes with 0 or 1 on the third')
    return orders


LABEL_ORDERS = (0, 1)                 # the label's interpolation: nearest, or the class vote over the 8 trilinear taps


def label_order_of(label_order):
    """a `label_order` argument as 0 (nearest, the default everywhere) or 1 (the class vote: every class's indicator map interpolated
    linearly and the arg-max taken, nnU-Net's "one-hot, order 1"; ltu_resample_vote / ltu_sample_vote); anything else is a
    ValueError"""
    if isinstance(label_order, (int, np.integer)) and not isinstance(label_order, bool) and int(label_order) in LABEL_ORDERS:
        return int(label_order)
    raise ValueError(f'label_order is 0 (nearest) or 1 (class vote), got {label_order!r}')


def _source_layout(src, src_strides):
    """(shape, element strides) per source axis of a device source: x fastest ([S2][S1][S0]) unless strides are given"""
    if src_strides is None:
        S = tuple(int(n) for n in src.shape[::-1])
        return S, (1, S[0], S[0] * S[1])
    return tuple(int(n) for n in src.shape), tuple(int(s) for s in src_strides)


def spline_coefficients(src, orders, imap=(1.0, 0.0, -np.inf, np.inf), src_dtype=0, src_strides=None):
    """ltu_spline_prefilter: the cubic B-spline coefficients of a device scan as stored (src_dtype, shape and `src_strides` as
    data.resample), every voxel mapped first (clamp(alpha * v + beta, lo, hi)): an axis of order 3 is filtered as
    scipy.ndimage.spline_filter1d(order=3, mode='mirror') filters it, an axis of order 0 or 1 (or of length 1) is left alone.
    Returns a dense f32 tensor [S2][S1][S0] (the source's axes, x fastest)."""
    if not torch.is_tensor(src) or not src.is_cuda:
        raise _lib.LtuError('data.spline_coefficients runs on the GPU only (no CPU fallback)')
    orders = tuple(int(o) for o in orders)
    if len(orders) != 3 or any(o not in SPLINE_ORDERS for o in orders):
        raise ValueError(f'orders is a 3-tuple of {SPLINE_ORDERS}, got {orders}')
    if src.dim() != 3:
        raise ValueError(f'spline_coefficients takes one volume, got {tuple(src.shape)}')
    S, ss = _source_layout(src, src_strides)
    coef = torch.empty(S[::-1], device=src.device, dtype=torch.float32)
    _lib.call('ltu_spline_prefilter', _p(src), int(src_dtype), *S, *ss, _p(coef), *orders, *(float(v) for v in imap), _s())
    return coef


def resample(src_img, src_lab, matrix, out_shape, imap=(1.0, 0.0, -np.inf, np.inf), src_dtype=0, src_strides=None,
             out_strides=None, lane_axis=None, order=1, out=None, label_order=0):
    """ltu_resample_grid: device sources (image of src_dtype / u8 label, either None) of shape (S0, S1, S2) read through
    `src_strides` (default: x fastest, i.e. a [S2][S1][S0] array), resampled through the 3x4 float64 pull matrix to outputs of
    out_shape (default layout: [O0][O1][O2], the last axis fastest).  Returns (f32 image or None, u8 label or None).
    order: the image's interpolation, 1 (trilinear, the call as it always was), 3 (cubic B-spline) or one of 0 / 1 / 3 per source
    axis (resolve_order).  Anything but 1 prefilters the mapped scan (spline_coefficients) and gathers the coefficients through the
    same matrix (ltu_resample_spline), clamped to the map's [lo, hi]; the label still goes nearest through ltu_resample_grid.
    label_order: 0, the default, is that nearest label (round half even of the clamped coordinate).  1 takes the label by class
    vote (ltu_resample_vote, a launch of its own; the image goes through its present call with the label left out): the 8 trilinear
    taps and fp32 weights of the order-1 image path, the weights summed per label value, the smallest value of maximal score wins.
    That is the arg-max of the linearly interpolated one-hot maps, byte for byte resample_argmax on float32 one-hot channels, for
    any u8 values and without the one-hot volume.
    out: (f32 image or None, u8 label or None) to write into instead of fresh tensors: device tensors (views allowed) whose
    element [0, 0, 0] is output voxel (0, 0, 0) and whose memory `out_strides` describes, e.g. a box of a larger volume."""
    vote = label_order_of(label_order) == 1 and src_lab is not None
    src = src_img if src_img is not None else src_lab
    if src is None or not src.is_cuda:
        raise _lib.LtuError('data.resample runs on the GPU only (no CPU fallback)')
    orders = resolve_order(order)
    if src_img is not None and src_lab is not None and (src_img.shape != src_lab.shape or src_img.stride() != src_lab.stride()):
        raise ValueError(f'image {tuple(src_img.shape)} and label {tuple(src_lab.shape)} are sampled through one matrix: same layout needed')
    spline = src_img is not None and orders != (1, 1, 1)
    coef = spline_coefficients(src_img, orders, imap, src_dtype, src_strides) if spline else None
    S, src_strides = _source_layout(src, src_strides)
    O = tuple(int(n) for n in out_shape)
    if out_strides is None:
        out_strides, alloc = (O[1] * O[2], O[2], 1), O
    else:
        alloc = tuple(O[a] for a in np.argsort(out_strides)[::-1])
    m = np.asarray(matrix, dtype=np.float64).reshape(3, 4)
    mat = torch.as_tensor(m.ravel().copy()).to(src.device)
    if out is not None:
        oi, ol = out
        if (oi is None) != (src_img is None) or (ol is None) != (src_lab is None) or \
                (oi is not None and oi.dtype != torch.float32) or (ol is not None and ol.dtype != torch.uint8):
            raise ValueError('out holds a float32 tensor for the image and a uint8 tensor for the label, one per source given')
    else:
        oi = torch.empty(alloc, device=src.device, dtype=torch.float32) if src_img is not None else None
        ol = torch.empty(alloc, device=src.device, dtype=torch.uint8) if src_lab is not None else None
    if spline:
        # the coefficients are dense with x fastest whatever the source's strides were: the lane axis follows THEIR layout
        lane = geometry.lane_axis(m, (1, S[0], S[0] * S[1])) if lane_axis is None else lane_axis
        _lib.call('ltu_resample_spline', _p(coef), *S, *orders, _p(oi), *O, *(int(s) for s in out_strides), _p(mat), lane,
                  float(imap[2]), float(imap[3]), _s())
        del coef
        if src_lab is None:
            return oi, ol
    gi, go = (None, None) if spline else (src_img, oi)          # after the spline gather only the label is left, nearest
    lane = geometry.lane_axis(m, src_strides) if lane_axis is None else lane_axis
    gl, gol = (None, None) if vote else (src_lab, ol)           # a voted label is a launch of its own
    if gi is not None or gl is not None:
        _lib.call('ltu_resample_grid', _p(gi), int(src_dtype), _p(gl), *S, *src_strides, _p(go), _p(gol),
                  *O, *(int(s) for s in out_strides), _p(mat), lane, *(float(v) for v in imap), _s())
    if vote:
        _lib.call('ltu_resample_vote', _p(src_lab), *S, *src_strides, _p(ol), *O, *(int(s) for s in out_strides), _p(mat), lane, _s())
    return oi, ol


def resample_argmax(probs, matrix, out_shape, src_strides=None, out_strides=None, lane_axis=None, classes=(), out=None):
    """ltu_resample_argmax: probs f32 [C, ...] on the device, C = 2 .. 8 channels of one volume of shape (S0, S1, S2) read through
    `src_strides` (default: x fastest, i.e. every channel a [S2][S1][S0] array), pulled through the 3x4 float64 matrix onto out_shape
    (layouts and the lane axis as data.resample) with the arg-max taken there: the first maximal class wins, as torch.argmax.
    Every channel is resampled bit for bit as data.resample resamples it alone; the coordinates and taps are formed once for all.
    classes: class ids whose resampled probabilities are returned too, in ascending order.
    out: (u8 label, f32 probabilities [K, ...] or None) to write into instead of fresh tensors (views allowed, as data.resample's).
    Returns (label u8, probabilities f32 [K, ...] or None)."""
    if not torch.is_tensor(probs) or not probs.is_cuda:
        raise _lib.LtuError('data.resample_argmax runs on the GPU only (no CPU fallback)')
    if probs.dim() != 4 or probs.dtype != torch.float32 or not 2 <= probs.shape[0] <= 8:
        raise ValueError(f'resample_argmax takes float32 probabilities [C, S0, S1, S2] with C = 2 .. 8, got {probs.dtype} {tuple(probs.shape)}')
    C = int(probs.shape[0])
    ks = sorted({int(k) for k in classes})
    if ks and not (0 <= ks[0] and ks[-1] < C):
        raise ValueError(f'classes {tuple(classes)} are not all in 0 .. {C - 1}')
    probs = probs.contiguous()
    if src_strides is None:
        S = tuple(int(n) for n in probs.shape[:0:-1])
        src_strides = (1, S[0], S[0] * S[1])
    else:
        S = tuple(int(n) for n in probs.shape[1:])
    O = tuple(int(n) for n in out_shape)
    if out_strides is None:
        out_strides, alloc = (O[1] * O[2], O[2], 1), O
    else:
        alloc = tuple(O[a] for a in np.argsort(out_strides)[::-1])
    m = np.asarray(matrix, dtype=np.float64).reshape(3, 4)
    mat = torch.as_tensor(m.ravel().copy()).to(probs.device)
    lane = geometry.lane_axis(m, src_strides) if lane_axis is None else lane_axis
    if out is not None:
        ol, op = out
        if ol.dtype != torch.uint8 or (op is None) != (not ks) or (op is not None and (op.dtype != torch.float32 or op.shape[0] != len(ks))):
            raise ValueError('out holds a uint8 label and float32 probabilities [K, ...], K = len(classes) (None for no class)')
    else:
        ol = torch.empty(alloc, device=probs.device, dtype=torch.uint8)
        op = torch.empty((len(ks),) + alloc, device=probs.device, dtype=torch.float32) if ks else None
    _lib.call('ltu_resample_argmax', _p(probs), C, probs.stride(0), *S, *(int(s) for s in src_strides), _p(ol), _p(op),
              sum(1 << k for k in ks), int(op.stride(0)) if op is not None else O[0] * O[1] * O[2], *O,
              *(int(s) for s in out_strides), _p(mat), lane, _s())
    return ol, op


# ---- intensity fingerprint (csrc/intensity.hip; nnU-Net's dataset fingerprint and CTNormalization, no reference counterpart: the
# driver's window is four constants) -------------------------------------------------------------------------------------------------
# A stored scan, optionally under its label, becomes an exact value histogram on the device; everything after that is integer
# arithmetic on at most 65536 bins on the host.

def _percentile_ranks(n, q):
    """numpy's default ('linear') percentile on n sorted values: (lo, hi, g) with result lerp(x[lo], x[hi], g)"""
    q = float(q)
    if not 0.0 <= q <= 100.0:
        raise ValueError(f'percentiles must be in 0 .. 100, got {q}')
    h = np.float64(n - 1) * (np.float64(q) / 100.0)
    lo = int(np.floor(h))
    return lo, min(lo + 1, n - 1), h - np.float64(lo)


def _lerp(a, b, g):
    """numpy's _lerp on two float64 order statistics"""
    a, b = np.float64(a), np.float64(b)
    return float(b - (b - a) * (1.0 - g)) if g >= 0.5 else float(a + (b - a) * g)


def _nan_stats(percentiles):
    nan = float('nan')
    return {'count': 0, 'min': nan, 'max': nan, 'mean': nan, 'std': nan, 'percentiles': [nan] * len(percentiles)}


def _order_stats(n, stat, percentiles, slope, inter):
    """min, max and percentiles of v * slope + inter from stat(r), the r-th smallest stored value as float64: the map is applied
    to the order statistics in float64 (a negative slope reverses their order), the interpolation happens in scaled units"""
    slope, inter = np.float64(slope), np.float64(inter)

    def scaled(r):
        return np.float64(stat(n - 1 - r if slope < 0 else r)) * slope + inter
    pct = []
    for q in percentiles:
        lo, hi, g = _percentile_ranks(n, q)
        pct.append(_lerp(scaled(lo), scaled(hi), g))
    return float(scaled(0)), float(scaled(n - 1)), pct


def histogram_stats(hist, percentiles=(0.5, 50.0, 99.5), offset=-32768, slope=1.0, inter=0.0):
    """statistics of the values counted in an integer histogram whose bin b holds the value b + offset (pure host arithmetic):
    {'count', 'min', 'max', 'mean', 'std' (population, ddof 0, as nnU-Net's np.std), 'percentiles'}.  The mean and the variance
    numerator n sum c v^2 - (sum c v)^2 are exact integers, rounded once; a percentile is numpy's default ('linear') definition on
    the exact order statistics, bit for bit np.percentile of the expanded values as float64.  slope / inter: the statistics of
    v * slope + inter instead.  An empty histogram gives count 0 and NaN for the rest."""
    h = np.asarray(hist).ravel()
    bins = np.nonzero(h)[0]
    cnts = [int(c) for c in h[bins]]
    vals = [int(b) + int(offset) for b in bins]
    n = sum(cnts)
    if n == 0:
        return _nan_stats(percentiles)
    if min(cnts) < 0:
        raise ValueError('a histogram holds no negative counts')
    s1 = sum(c * v for c, v in zip(cnts, vals))
    s2 = sum(c * v * v for c, v in zip(cnts, vals))
    cum = np.cumsum(np.asarray(cnts, dtype=np.int64))
    vmin, vmax, pct = _order_stats(n, lambda r: vals[int(np.searchsorted(cum, r, side='right'))], percentiles, slope, inter)
    mean, std = s1 / n, float(np.sqrt((n * s2 - s1 * s1) / (n * n)))
    return {'count': n, 'min': vmin, 'max': vmax, 'mean': float(np.float64(mean) * np.float64(slope) + np.float64(inter)),
            'std': std * abs(float(slope)), 'percentiles': pct}


def _hist_source(img, lab):
    if not torch.is_tensor(img) or not img.is_cuda:
        raise _lib.LtuError('the intensity histogram is taken on the GPU only (no CPU fallback)')
    code = {torch.uint8: _lib.U8, torch.int16: _lib.I16, torch.float32: 0}.get(img.dtype)
    if code is None or not img.is_contiguous() or img.numel() == 0:
        raise ValueError(f'the intensity histogram takes a contiguous, non-empty uint8, int16 or float32 scan, got {img.dtype} {tuple(img.shape)}')
    if lab is not None and (not torch.is_tensor(lab) or lab.dtype != torch.uint8 or lab.device != img.device
                            or lab.numel() != img.numel() or not lab.is_contiguous()):
        raise ValueError('the label is a contiguous uint8 tensor with the scan\'s voxel count, on its device')
    return code


def _hist_launch(img, lab, mask, code, mode, prefix=0):
    """one ltu_intensity_hist launch into fresh buffers: (uint32 histogram as int32 words [65536], int64 {binned, rejected})"""
    hist = torch.zeros(65536, device=img.device, dtype=torch.int32)
    counts = torch.zeros(2, device=img.device, dtype=torch.int64)
    _lib.call('ltu_intensity_hist', _p(img), code, _p(lab) if lab is not None else 0, img.numel(), int(mask) & 0x1ff, mode, int(prefix),
              _p(hist), _p(counts), _s())
    return hist, counts


def intensity_histogram(img, lab=None, mask=FG_MASK):
    """the exact value histogram of a device scan (uint8, int16, or float32 holding integers of the int16 range; any shape,
    contiguous) over the voxels whose label value is in `mask` (the bin sets of CropIndex.select: FG_MASK, BG_MASK, 1 << c), all
    voxels without a label.  Returns (int64 [65536] on the device, rejected): bin b counts the value b for a uint8 scan and b -
    32768 otherwise; rejected = the selected float32 voxels that are not finite or no integer of the range (they are in no bin)."""
    code = _hist_source(img, lab)
    mode = {_lib.U8: _lib.HIST_U8, _lib.I16: _lib.HIST_I16, 0: _lib.HIST_F32_INT}[code]
    hist, counts = _hist_launch(img, lab, mask, code, mode)
    return hist.to(torch.int64) & 0xffffffff, int(counts[1].item())


def _float_stats(img, lab, mask, percentiles, slope, inter):
    """intensity_stats of a float32 scan: a histogram of the top 16 bits of the floats' ordered keys finds the bin of every wanted
    rank, one histogram of the low 16 bits per distinct bin finds the value; the moments come from ltu_intensity_moments"""
    hist, counts = _hist_launch(img, lab, mask, 0, _lib.HIST_F32_HI)
    n, rejected = (int(v) for v in counts.cpu().tolist())
    if rejected:
        raise ValueError(f'{rejected} non-finite voxels in the scan')
    if n == 0:
        return _nan_stats(percentiles)
    ranks = {0, n - 1}
    for q in percentiles:                            # _order_stats asks for the mirrored ranks under a negative slope
        ranks.update(n - 1 - r if slope < 0 else r for r in _percentile_ranks(n, q)[:2])
    cum = np.cumsum(hist.cpu().numpy().view(np.uint32).astype(np.int64))
    where = {r: int(np.searchsorted(cum, r, side='right')) for r in ranks}
    value = {}
    for prefix in sorted(set(where.values())):
        low, _ = _hist_launch(img, lab, mask, 0, _lib.HIST_F32_LO, prefix)
        cl = np.cumsum(low.cpu().numpy().view(np.uint32).astype(np.int64))
        before = int(cum[prefix - 1]) if prefix else 0
        for r, p in where.items():
            if p == prefix:
                key = (prefix << 16) | int(np.searchsorted(cl, r - before, side='right'))
                bits = key ^ 0x80000000 if key & 0x80000000 else ~key & 0xffffffff
                value[r] = np.float64(np.array([bits], dtype=np.uint32).view(np.float32)[0])
    vmin, vmax, pct = _order_stats(n, value.__getitem__, percentiles, slope, inter)
    parts = torch.empty(2 * _lib.INTENSITY_MOMENT_PARTS, device=img.device, dtype=torch.float64)
    out = torch.empty(2, device=img.device, dtype=torch.float64)

    def moments(centre):
        _lib.call('ltu_intensity_moments', _p(img), _p(lab) if lab is not None else 0, img.numel(), int(mask) & 0x1ff, float(centre),
                  _p(parts), parts.numel(), _p(out), _s())
        return out.cpu().tolist()
    mean = moments(0.0)[0] / n
    d1, d2 = moments(mean)                           # about the mean: sum d^2 / n - (sum d / n)^2 cancels nothing
    mean += d1 / n
    std = float(np.sqrt(max(d2 / n - (d1 / n) ** 2, 0.0)))
    return {'count': n, 'min': vmin, 'max': vmax, 'mean': mean * float(slope) + float(inter), 'std': std * abs(float(slope)),
            'percentiles': pct}


def intensity_stats(img, lab=None, mask=FG_MASK, percentiles=(0.5, 50.0, 99.5), slope=1.0, inter=0.0):
    """histogram_stats' record for one device scan (selection as intensity_histogram), in units of v * slope + inter.  uint8 and
    int16 go through the exact histogram.  float32 (any finite values) goes through the two-level histogram of the floats' ordered
    bits, so min, max and the percentiles are exact too; its mean and std are fp64 sums in a fixed order.  A non-finite float32
    voxel raises ValueError.  A load-time call: it reads 256 KiB histograms back between its passes."""
    code = _hist_source(img, lab)
    if code == 0:
        return _float_stats(img, lab, mask, tuple(percentiles), slope, inter)
    hist, _ = intensity_histogram(img, lab, mask)
    return histogram_stats(hist.cpu().numpy(), percentiles, 0 if code == _lib.U8 else -32768, slope, inter)


def _percentile_key(q):
    """nnU-Net's name of a percentile in its fingerprint: 0.5 -> percentile_00_5, 99.5 -> percentile_99_5"""
    whole, _, frac = repr(float(q)).partition('.')
    return f'percentile_{int(whole):02d}_{frac}'


class IntensityFingerprint:
    """The intensity statistics of a training set's foreground, as nnU-Net's dataset fingerprint keeps them for CTNormalization:
    an int64 histogram [65536] of the scaled values v * slope + inter (bin b counts the value b - 32768) that every scan is added
    into by one kernel launch.  window() is the `intensity` of SpacedScan: (p_lo, p_hi, (p_lo - mean) / std, (p_hi - mean) / std)
    for percentiles (lo, hi).  scans / empty_scans: the scans added / those among them whose selection was empty (a label without
    foreground contributes nothing).  The histogram lives where the first scan lives; merge() adds another rank's part."""

    def __init__(self, percentiles=(0.5, 99.5), device='cuda'):
        self.percentiles = tuple(float(q) for q in percentiles)
        if len(self.percentiles) != 2 or not 0.0 <= self.percentiles[0] <= self.percentiles[1] <= 100.0:
            raise ValueError(f'a fingerprint keeps a (low, high) pair of percentiles, got {percentiles}')
        self.device, self.hist, self.scans, self.empty_scans = device, None, 0, 0

    def add_histogram(self, hist, offset=-32768, slope=1.0, inter=0.0, name='scan'):
        """add a scan's histogram (integer tensor [65536] on any device, bin b = the stored value b + offset) under the scan's
        slope / intercept: the bins are re-indexed onto the scaled values.  ValueError, naming the scan, unless slope is an
        integer >= 1, inter an integer and every scaled value an int16."""
        if float(slope) != int(slope) or int(slope) < 1 or float(inter) != int(inter):
            raise ValueError(f'{name}: the fingerprint counts integer values, slope {slope} / intercept {inter} do not keep them integral '
                             "(normalise such scans with intensity='zscore')")
        h = torch.as_tensor(hist).to(torch.int64).reshape(-1)
        if h.numel() != 65536:
            raise ValueError(f'{name}: a histogram has 65536 bins, got {h.numel()}')
        self.scans += 1
        live = torch.nonzero(h).reshape(-1)
        if live.numel() == 0:
            self.empty_scans += 1
            return
        to = (live + int(offset)) * int(slope) + int(inter)
        lo, hi = int(to[0].item()), int(to[-1].item())
        if lo < -32768 or hi > 32767:
            self.scans -= 1
            raise ValueError(f'{name}: scaled values {lo} .. {hi} do not fit int16')
        if self.hist is None:
            self.hist = torch.zeros(65536, device=h.device, dtype=torch.int64)
        self.hist.index_add_(0, (to + 32768).to(self.hist.device), h[live].to(self.hist.device))

    def add_arrays(self, img, lab=None, slope=1.0, inter=0.0, mask=FG_MASK, name='scan'):
        """add a device scan as stored (uint8, int16, or float32 holding integers) under its device label: one histogram launch"""
        hist, rejected = intensity_histogram(img, lab, mask)
        if rejected:
            raise ValueError(f"{name}: {rejected} selected voxels are not integers of the int16 range; a fingerprint needs integral "
                             "values (normalise such scans with intensity='zscore')")
        self.add_histogram(hist, 0 if img.dtype == torch.uint8 else -32768, slope, inter, name)

    def add(self, img_path, lab_path=None, mask=FG_MASK):
        """add one NIfTI scan under its label file (all voxels without one): loaded, uploaded as stored, one histogram launch"""
        ni = nifti.load(img_path)
        rl = None
        if lab_path is not None:
            nl = nifti.load(lab_path)
            geometry.check_pair(ni.shape, ni.affine, nl.shape, nl.affine)
            lv = nl.data if (nl.slope, nl.inter) == (1.0, 0.0) else nl.scaled()
            rl = torch.as_tensor(np.ascontiguousarray(label_u8(lv))).to(self.device)
        raw, _ = _source_dtype(ni.data)
        self.add_arrays(torch.as_tensor(np.ascontiguousarray(raw)).to(self.device), rl, ni.slope, ni.inter, mask, str(img_path))

    def merge(self, other):
        """add the scans another fingerprint saw (another rank's, or one restored by from_dict)"""
        if other.hist is not None:
            if self.hist is None:
                self.hist = torch.zeros_like(other.hist)
            self.hist += other.hist.to(self.hist.device)
        self.scans += other.scans
        self.empty_scans += other.empty_scans
        return self

    def _host_hist(self):
        return np.zeros(65536, dtype=np.int64) if self.hist is None else self.hist.cpu().numpy()

    def stats(self, percentiles=None):
        """histogram_stats of everything added, at the fingerprint's percentiles (or the given ones)"""
        return histogram_stats(self._host_hist(), self.percentiles if percentiles is None else percentiles)

    def window(self):
        """(p_lo, p_hi, (p_lo - mean) / std, (p_hi - mean) / std), std floored at 1e-8 as nnU-Net's CTNormalization does"""
        st = self.stats()
        if st['count'] == 0:
            raise ValueError('window() of an empty fingerprint: no scan with a selected voxel was added')
        (lo, hi), sd = st['percentiles'], max(st['std'], 1e-8)
        return lo, hi, (lo - st['mean']) / sd, (hi - st['mean']) / sd

    def to_dict(self):
        """JSON-able: nnU-Net's foreground_intensity_properties keys (max, mean, median, min, percentile_00_5, percentile_99_5,
        std; absent while empty), plus the non-empty bins [[value, count], ...] so that a saved fingerprint can still be merged"""
        h = self._host_hist()
        d = {'percentiles': list(self.percentiles), 'scans': self.scans, 'empty_scans': self.empty_scans,
             'bins': [[int(b) - 32768, int(h[b])] for b in np.nonzero(h)[0]]}
        st = self.stats(self.percentiles + (50.0,))
        if st['count']:
            d.update({'max': st['max'], 'mean': st['mean'], 'median': st['percentiles'][2], 'min': st['min'], 'std': st['std'],
                      _percentile_key(self.percentiles[0]): st['percentiles'][0], _percentile_key(self.percentiles[1]): st['percentiles'][1]})
        return d

    @classmethod
    def from_dict(cls, d, device='cpu'):
        fp = cls(tuple(d['percentiles']), device)
        fp.scans, fp.empty_scans = int(d['scans']), int(d['empty_scans'])
        if d['bins']:
            h = np.zeros(65536, dtype=np.int64)
            for value, count in d['bins']:
                h[int(value) + 32768] = int(count)
            fp.hist = torch.from_numpy(h).to(device)
        return fp


# ---- nonzero cropping and masked normalisation (csrc/nonzero.hip, the hole filling of csrc/components.hip; nnU-Net's
# crop_to_nonzero and ZScoreNormalization under the nonzero mask, no reference counterpart) -----------------------------------------
# The nonzero mask of a scan is the union over its channels of value != 0 with holes filled; the scan is cropped to the mask's
# bounding box and every channel z-scored with the statistics of its voxels inside the mask, 0 outside.

def fill_holes_u8(mask, out, connectivity=1):
    """ltu_fill_holes on a contiguous u8 device mask [B, H, W, D] into out (the same shape; `mask` itself for in place); returns
    out.  infer.fill_holes is the public form."""
    B, H, W, D = (int(v) for v in mask.shape)
    ws = _lib.load().ltu_fill_holes_ws_elems(B, H, W, D)
    if ws <= 0:
        raise _lib.LtuError(f'fill_holes: shape {tuple(mask.shape)} refused (B <= 65535 and H * W * D < 2^31)')
    scratch = torch.empty(ws, device=mask.device, dtype=torch.int32)
    _lib.call('ltu_fill_holes', _p(mask), _p(out), _p(scratch), ws, B, H, W, D, int(connectivity), _s())
    return out


_STORED_CODES = {torch.uint8: _lib.U8, torch.int16: _lib.I16, torch.float32: 0}


def _stored_volume(raw, what):
    """the dtype code of a device volume as stored: contiguous [Z, Y, X] uint8, int16 or float32"""
    if not torch.is_tensor(raw) or not raw.is_cuda:
        raise _lib.LtuError(f'{what} runs on the GPU only (no CPU fallback)')
    code = _STORED_CODES.get(raw.dtype)
    if code is None or raw.dim() != 3 or not raw.is_contiguous() or raw.numel() == 0:
        raise ValueError(f'{what} takes a contiguous, non-empty uint8, int16 or float32 volume [Z, Y, X], got {raw.dtype} {tuple(raw.shape)}')
    return code


def nonzero_mask(raws, scalings=None, fill_holes=True):
    """the nonzero mask of a scan, nnU-Net's create_nonzero_mask: raws is one device volume as stored (uint8, int16 or float32
    [Z, Y, X]) or a sequence of K of them on one grid, scalings one (slope, inter) per volume (default (1, 0)): the union over the
    volumes of v * slope + inter != 0 (one fmaf in float32; a NaN counts as nonzero), then, with fill_holes, the background that no
    6-connected path joins to a face of the volume (infer.fill_holes, scipy's binary_fill_holes).
    Returns (mask u8 [Z, Y, X] on the device, box, count): box = one (lo, hi exclusive) pair per axis of the stored array, the
    bounding box of the mask, count = its voxels.  One launch per volume, the hole filling, one box reduction and ONE host read (32
    bytes).  An all-zero scan raises ValueError."""
    vols = [raws] if torch.is_tensor(raws) else list(raws)
    if not vols:
        raise ValueError('nonzero_mask takes at least one volume')
    scalings = [(1.0, 0.0)] * len(vols) if scalings is None else [(float(a), float(b)) for a, b in scalings]
    if len(scalings) != len(vols):
        raise ValueError(f'{len(scalings)} scalings for {len(vols)} volumes')
    codes = [_stored_volume(v, 'data.nonzero_mask') for v in vols]
    shape = tuple(int(n) for n in vols[0].shape)
    if any(tuple(v.shape) != shape or v.device != vols[0].device for v in vols):
        raise ValueError('the volumes of one scan share a grid and a device')
    mask = torch.empty(shape, device=vols[0].device, dtype=torch.uint8)
    for c, (v, code, (slope, inter)) in enumerate(zip(vols, codes, scalings)):
        _lib.call('ltu_nonzero_mask', _p(v), code, v.numel(), slope, inter, _p(mask), int(c > 0), _s())
    if fill_holes:
        fill_holes_u8(mask.view(1, *shape), mask.view(1, *shape), 1)
    res = torch.empty(4, device=mask.device, dtype=torch.int64)          # count, then the six int32 bounds
    _lib.call('ltu_mask_box', _p(mask), 1, *shape, _p(res[1:]), _p(res), _s())
    host = res.cpu().numpy()
    count, bounds = int(host[0]), host[1:].view(np.int32)
    if count == 0:
        raise ValueError('the scan holds no nonzero voxel: there is nothing to crop to')
    return mask, tuple((int(bounds[2 * a]), int(bounds[2 * a + 1]) + 1) for a in range(3)), count


def _check_box(box, shape):
    pairs = tuple(tuple(int(v) for v in p) for p in box)
    if len(pairs) != 3 or any(len(p) != 2 or not 0 <= p[0] < p[1] <= n for p, n in zip(pairs, shape)):
        raise ValueError(f'box {box!r} is not three (lo, hi) pairs inside a volume of shape {tuple(shape)}')
    return pairs


def normalize_masked(raw, mask, box, alpha, beta, src_dtype=None):
    """ltu_normalize_masked: the box (one (lo, hi exclusive) pair per axis) of a device volume as stored (uint8, int16 or float32
    [Z, Y, X]; src_dtype: its code, default from the tensor) under the u8 mask of the same shape, as a dense f32 volume of the box's
    shape: mask ? fmaf(v, alpha, beta) : 0, alpha and beta rounded to float32 once.  One launch."""
    code = _stored_volume(raw, 'data.normalize_masked')
    if src_dtype is not None and int(src_dtype) != code:
        raise ValueError(f'src_dtype {src_dtype} does not name the dtype of a {raw.dtype} volume')
    if not torch.is_tensor(mask) or mask.dtype != torch.uint8 or mask.shape != raw.shape or mask.device != raw.device \
            or not mask.is_contiguous():
        raise ValueError('the mask is a contiguous uint8 tensor of the volume\'s shape, on its device')
    Z, Y, X = (int(n) for n in raw.shape)
    (z0, z1), (y0, y1), (x0, x1) = _check_box(box, (Z, Y, X))
    out = torch.empty((z1 - z0, y1 - y0, x1 - x0), device=raw.device, dtype=torch.float32)
    _lib.call('ltu_normalize_masked', _p(raw), code, _p(mask), X, Y, Z, x0, y0, z0, x1 - x0, y1 - y0, z1 - z0, float(alpha), float(beta),
              _p(out), _s())
    return out


INTENSITY_NAMES = ('zscore', 'zscore_nonzero')
CROP_NAMES = ('nonzero',)


def _check_scan_options(crop, specs):
    """the refusals SpacedScan / MultiScan make before a file is read or the GPU touched"""
    if crop is not None and crop not in CROP_NAMES:
        raise ValueError(f"crop is None or 'nonzero', got {crop!r}")
    for spec in specs:
        if isinstance(spec, str) and spec not in INTENSITY_NAMES:
            raise ValueError(f"intensity is a window, None, an IntensityFingerprint, 'zscore' or 'zscore_nonzero', got {spec!r}")


def _masked_spec(spec):
    return isinstance(spec, str) and spec == 'zscore_nonzero'


def _masked_zscore(raw, mask, slope, inter):
    """'zscore_nonzero': (window 4-tuple, alpha, beta) from the statistics of the voxels of raw inside the mask, in units of
    v * slope + inter: the z-score is fmaf(v, alpha, beta), alpha = slope / sd, beta = (inter - mean) / sd, sd = max(std, 1e-8),
    formed in float64"""
    st = intensity_stats(raw, lab=mask, mask=FG_MASK, percentiles=(), slope=slope, inter=inter)
    sd = max(st['std'], 1e-8)
    window = (st['min'], st['max'], (st['min'] - st['mean']) / sd, (st['max'] - st['mean']) / sd)
    return window, float(slope) / sd, (float(inter) - st['mean']) / sd


def _load_channel(ri, rl, code, spec, slope, inter, mask, box, plan, order, label_order=0):
    """one channel of a scan, for every crop and every spec: (f32 image, u8 label or None, window).  ri / rl: the device volumes as
    stored [Z, Y, X] (rl None: no label, or not channel 0); box: the part to load in their axes, the whole volume without a crop;
    mask: the scan's nonzero mask, None where it needs none; plan: (matrix, shape) of the box's resampling.
    The box is read through the stored volume's strides, no copy; the whole volume's box is the layout data.resample assumes of a
    source without strides.  'zscore_nonzero' normalises the box first (normalize_masked) and resamples the f32 result with the
    identity map, the label from its box in a call of its own; every other spec resamples image and label in ONE call (at order 1
    one launch).  The label is nearest at label_order 0 and the class vote at 1 (data.resample's label_order; read from the box
    like the image)."""
    matrix, shape = plan
    Z, Y, X = (int(n) for n in ri.shape)
    (z0, z1), (y0, y1), (x0, x1) = box
    strides = (1, X, X * Y)

    def boxed(t):                                     # the box as a view with x first, as `strides` describes it
        return None if t is None else t[z0:z1, y0:y1, x0:x1].permute(2, 1, 0)
    if _masked_spec(spec):
        ol = resample(None, boxed(rl), matrix, shape, src_strides=strides, label_order=label_order)[1] if rl is not None else None
        window, alpha, beta = _masked_zscore(ri, mask, slope, inter)
        oi, _ = resample(normalize_masked(ri, mask, box, alpha, beta, code), None, matrix, shape, order=order)
    else:
        window = _resolve_intensity(spec, ri, slope, inter)
        oi, ol = resample(boxed(ri), boxed(rl), matrix, shape, intensity_map(window, slope, inter), code, src_strides=strides,
                          order=order, label_order=label_order)
    return oi, ol, window


def _resolve_intensity(intensity, raw, slope, inter):
    """SpacedScan's `intensity` as a window 4-tuple or None: a fingerprint gives its window(); 'zscore' the statistics of all voxels
    of this scan (no label, so training and inference agree) as the window (vmin, vmax, (vmin - mean) / std, (vmax - mean) / std),
    the z-score with a clamp that never bites"""
    if isinstance(intensity, IntensityFingerprint):
        return intensity.window()
    if isinstance(intensity, str):
        if intensity != 'zscore':
            raise ValueError(f"intensity is a window, None, an IntensityFingerprint or 'zscore', got {intensity!r}")
        st = intensity_stats(raw, percentiles=(), slope=slope, inter=inter)
        sd = max(st['std'], 1e-8)
        return st['min'], st['max'], (st['min'] - st['mean']) / sd, (st['max'] - st['mean']) / sd
    return intensity


class SpacedScan:
    """The deterministic half of the driver's CacheDataset: one NIfTI image (and label) read, uploaded once as stored, and
    resampled on the device to `pixdim` in `axcodes` orientation: the K = 1 case of the loader it shares with MultiScan (_load, every
    channel through _load_channel), presented without the channel axis.  img: f32 [H, W, D]; lab: u8 [H, W, D] (or None);
    crop_index: the label's CropIndex, built on first use (crop centres are drawn from it); label_host: the resampled label on the
    host, copied on first use (a scan that is only sampled through the index never copies it); affine: the output's 4x4 affine;
    matrix: the 3x4 float64 pull matrix (RAS voxel -> file voxel); native_shape / native_affine / native: the file's grid and header.
    intensity: a ScaleIntensityRange window (a_min, a_max, b_min, b_max) applied with its clip, None for the scaled voxels as they
    are, an IntensityFingerprint for its window(), or 'zscore' for this scan's own mean and standard deviation over all voxels; the
    attribute `intensity` keeps the resulting 4-tuple (or None).
    order: the image's interpolation as data.resample takes it (1: trilinear, the driver's; 3: cubic B-spline; a 3-tuple per FILE
    axis), or 'auto' for geometry.resample_orders of the file's voxel sizes and pixdim (nnU-Net's rule: the coarse axis of an
    anisotropic scan goes nearest); the attribute `order` keeps the resolved 3-tuple.  The label is nearest whatever the order.
    label_order: 0 (nearest, the default) or 1: the label resampled by class vote (data.resample's label_order; nnU-Net resamples
    labels "one-hot, order 1"), also from the box of a cropped scan; the attribute `label_order` keeps it, crop_index and label_host
    follow from `lab` as before.
    crop='nonzero' (nnU-Net's crop_to_nonzero; for skull-stripped MR, where most voxels are exact zeros): the scan's nonzero mask
    (data.nonzero_mask: scaled value != 0, holes filled) is built on the device, and image and label are resampled from its
    bounding box only: matrix, shape and affine are then those of the box (geometry.crop_plan, then spacing_plan), matrix: RAS voxel
    -> BOX voxel; native, native_shape and native_affine stay the file's, and to_native / to_native_probs write into the box of a
    file-sized volume.  intensity='zscore_nonzero' (with or without crop) z-scores with the mean and standard deviation of the
    voxels inside that mask and puts 0 outside it, BEFORE resampling (nnU-Net's order): normalize_masked, then the f32 volume is
    resampled at `order` with the identity map; `intensity` keeps (vmin, vmax, (vmin - mean) / std, (vmax - mean) / std) of the
    masked statistics.  crop_box: the box per axis of the stored array [Z, Y, X] as (lo, hi exclusive) pairs, None without crop;
    nonzero_count / nonzero_fraction: the mask's voxels / its bounding box's share of the file's voxels (nnU-Net uses the mask for
    normalisation when the crop removes a quarter: fraction < 0.75), None when no mask was built; outside: the image value outside
    the scan that data.sample(augment=) fills with, 0.0 under 'zscore_nonzero', else None (the window's floor)."""

    def __init__(self, img_path, lab_path=None, pixdim=(0.5, 0.5, 2.0), axcodes='RAS', intensity=MONAI_CT_WINDOW, device='cuda',
                 order=1, crop=None, label_order=0):
        img, (self.intensity,), (self.outside,) = self._load([img_path], lab_path, pixdim, axcodes, [intensity], device, order, crop,
                                                             label_order)
        self.img = img[0]

    def _load(self, paths, lab_path, pixdim, axcodes, specs, device, order, crop, label_order=0):
        """the loader of SpacedScan and MultiScan: K files with one intensity spec each -> (img f32 [K, H, W, D], the K windows, the
        K `outside` values); every other attribute is set here.  A scan that needs no nonzero mask is uploaded, resampled and
        released one channel at a time; a crop or a 'zscore_nonzero' channel uploads all K volumes first, because the mask is their
        union.  The label is resampled with channel 0."""
        _check_scan_options(crop, specs)
        self.label_order = label_order_of(label_order)
        nis = [nifti.load(p) for p in paths]
        nl = nifti.load(lab_path) if lab_path is not None else None
        ni, K = nis[0], len(nis)
        for other in nis[1:] + ([nl] if nl is not None else []):
            geometry.check_pair(ni.shape, ni.affine, other.shape, other.affine)
        self.native, self.native_shape, self.native_affine = ni, ni.shape, ni.affine
        self.matrix, self.shape, self.affine = geometry.spacing_plan(ni.shape, ni.affine, pixdim, axcodes)
        self.order = _scan_order(order, ni.affine, pixdim)
        self.pixdim = tuple(float(p) for p in pixdim)                # sample(augment=) rotates in millimetres
        self._label_host = self._crop_index = None
        rl = None
        if nl is not None:
            lv = nl.data if (nl.slope, nl.inter) == (1.0, 0.0) else nl.scaled()
            rl = torch.as_tensor(np.ascontiguousarray(label_u8(lv))).to(device)

        def upload(nc):
            raw, code = _source_dtype(nc.data)
            return torch.as_tensor(np.ascontiguousarray(raw)).to(device), code
        self.crop_box = self.nonzero_count = self.nonzero_fraction = mask = None
        box = tuple((0, n) for n in ni.shape[::-1])                   # the whole stored array [Z, Y, X]
        raws = []
        if crop is not None or any(_masked_spec(spec) for spec in specs):
            raws = [upload(nc) for nc in nis]
            mask, bbox, self.nonzero_count = nonzero_mask([raw for raw, _ in raws], [(nc.slope, nc.inter) for nc in nis])
            self.nonzero_fraction = float(np.prod([hi - lo for lo, hi in bbox], dtype=np.float64) / raws[0][0].numel())
            if crop is not None:                         # matrix, shape and affine become the box's
                self.crop_box = box = bbox
                box_shape, affine = geometry.crop_plan(self.native_shape, self.native_affine, bbox[::-1])
                self.matrix, self.shape, self.affine = geometry.spacing_plan(box_shape, affine, pixdim, axcodes)
        img, windows = None, []
        for c, (nc, spec) in enumerate(zip(nis, specs)):
            ri, code = raws.pop(0) if raws else upload(nc)
            oi, ol, window = _load_channel(ri, rl if c == 0 else None, code, spec, nc.slope, nc.inter, mask, box,
                                           (self.matrix, self.shape), self.order, self.label_order)
            del ri                                       # every stored volume is dropped after its channel
            if c == 0:
                self.lab = ol
                img = oi[None] if K == 1 else torch.empty((K,) + tuple(oi.shape), device=oi.device, dtype=torch.float32)
            if K > 1:
                img[c].copy_(oi)
            windows.append(window)
        return img, windows, [0.0 if _masked_spec(spec) else None for spec in specs]

    @property
    def label_host(self):
        if self._label_host is None and self.lab is not None:
            self._label_host = self.lab.cpu().numpy()
        return self._label_host

    @property
    def crop_index(self):
        if self._crop_index is None and self.lab is not None:
            self._crop_index = CropIndex(self.lab)
        return self._crop_index

    def spline_coefficients(self, order):
        """the cubic B-spline coefficients of `img` (same shape, every channel of a MultiScan) for the gather's `order` (sample_order:
        3, (3, 3, 3) or (3, 3, 1) per scan axis H, W, D), as sample_affine(order=, coef=) reads them: built on first use by
        data.spline_coefficients and kept per order tuple.  While held they double the image's bytes on the device;
        drop_coefficients() frees them."""
        orders = sample_order(order)
        if orders == (1, 1, 1):
            raise ValueError('order 1 reads the image itself: there are no coefficients to build')
        cache = self.__dict__.setdefault('_spline_coefficients', {})
        if orders not in cache:
            cache[orders] = _gather_coefficients(self.img, orders)
        return cache[orders]

    def drop_coefficients(self):
        """free every coefficient volume spline_coefficients holds (the next call builds them again)"""
        self.__dict__.pop('_spline_coefficients', None)


def _scan_order(order, affine, pixdim):
    """SpacedScan's `order` as the 3-tuple per file axis; 'auto' asks geometry.resample_orders"""
    if isinstance(order, str):
        if order != 'auto':
            raise ValueError(f"order is 1, 3, a 3-tuple or 'auto', got {order!r}")
        return resolve_order(geometry.resample_orders(geometry.voxel_spacing(affine), pixdim))
    return resolve_order(order)


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


class MultiScan(SpacedScan):
    """SpacedScan for K = 1 .. 4 NIfTI images on ONE grid (T1 / T1c / T2 / FLAIR, T2 + ADC, PET + CT): img_paths is their sequence,
    channel 0 first.  Every other image and the label must match channel 0 in shape and affine (geometry.check_pair: ValueError).
    Each channel is resampled exactly as SpacedScan resamples it alone, by the same code (SpacedScan._load, which this class only
    hands its K paths and K specs); img: one contiguous f32 [K, H, W, D]; lab, crop_index,
    label_host, matrix, affine, shape, pixdim as on SpacedScan, native / native_shape / native_affine are channel 0's.
    intensity: one spec for all channels (a window 4-tuple, None, an IntensityFingerprint or 'zscore') or a sequence of K specs;
    the attribute `intensity` is the list of the K resulting tuples (or None).  channels == K.  order: as SpacedScan's, one for all
    channels, and label_order as SpacedScan's.  crop and 'zscore_nonzero' as SpacedScan's: ONE nonzero mask, the union over all K
    channels, crops the scan and selects the voxels of every channel's statistics; crop_box, nonzero_count, nonzero_fraction as
    there, outside: a list of K (0.0 for a 'zscore_nonzero' channel, else None)."""

    def __init__(self, img_paths, lab_path=None, pixdim=(0.5, 0.5, 2.0), axcodes='RAS', intensity=MONAI_CT_WINDOW, device='cuda',
                 order=1, crop=None, label_order=0):
        paths = [img_paths] if isinstance(img_paths, (str, bytes)) or hasattr(img_paths, '__fspath__') else list(img_paths)
        K = len(paths)
        if not 1 <= K <= _lib.MAX_INPUT_CHANNELS:
            raise ValueError(f'a MultiScan holds 1 .. {_lib.MAX_INPUT_CHANNELS} images, got {K}')
        one = intensity is None or isinstance(intensity, (str, IntensityFingerprint)) or \
            (len(intensity) == 4 and all(_is_number(v) for v in intensity))
        specs = [intensity] * K if one else list(intensity)
        if len(specs) != K:
            raise ValueError(f'intensity is one spec or one per image: {len(specs)} specs for {K} images')
        self.img, self.intensity, self.outside = self._load(paths, lab_path, pixdim, axcodes, specs, device, order, crop, label_order)
        self.channels = K


def channel_seed(seed, c):
    """the noise seed of channel c of a patch whose Augmentation.draw seed is `seed`: seed itself for c = 0, otherwise
    seed ^ (c * 0x9E3779B97F4A7C15 mod 2^64); noise_reference(channel_seed(seed, c), count) replays channel c"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed if c == 0 else seed ^ ((int(c) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)


def orient_desc(flip, k):
    """(flip_h, flip_w, swap_hw) of "flip along axis 0 (if flip), then np.rot90(k, axes=(0, 1))" as the signed permutation
    out[x][y] = crop[a][b], (u, v) = swap ? (y, x) : (x, y), a = flip_h ? h-1-u : u, b = flip_w ? w-1-v : v"""
    k %= 4
    h, w = (3, 3) if k % 2 else (2, 3)
    idx = np.arange(h * w).reshape(h, w)
    out = np.rot90(np.flip(idx, 0) if flip else idx, k, (0, 1))
    a, b = divmod(int(out[0, 0]), w)
    return int(a != 0), int(b != 0), k % 2


def draw_monai_sample(label_host, spatial_size, rs, flip_prob=0.5, rot90_prob=0.5, max_k=3, index=None):
    """one sample's draws in the driver's transform order from one RandomState: the crop centre (RandCropByPosNegLabeld,
    num_samples 1), the flip (RandFlipd), then RandRotate90d's k = randint(max_k) + 1 before its probability draw (monai 0.7.0's
    RandRotate90.randomize; recalled, not pinned).  Every draw is made whether or not its transform fires.
    Returns (centre, flip, k) with k = 0 when the rotation does not fire.  With index, the label's CropIndex, the centre comes
    from it and label_host is not read."""
    if index is not None:
        center = index.centers(spatial_size, 1, rand_state=rs)[0]
    else:
        center = crop_centers(label_host, spatial_size, 1, rand_state=rs)[0]
    flip = rs.rand() < flip_prob
    k = rs.randint(max_k) + 1
    rot = rs.rand() < rot90_prob
    return center, bool(flip), int(k) if rot else 0


def crop_orient(img, lab, draws, spatial_size):
    """device patches ([n,1,h,w,d] f32 or None, [n,1,h,w,d] u8 or None) = rot90(flip(crop, 0), k, (0, 1)) from img / lab
    [H,W,D] for draws [(centre, flip, k)]; an odd k needs h == w (the patch would change shape)"""
    vol = img if img is not None else lab
    if vol is None or not vol.is_cuda:
        raise _lib.LtuError('data.crop_orient runs on the GPU only (no CPU fallback)')
    H, W, D = vol.shape
    h, w, d = (int(s) for s in spatial_size)
    desc = np.array([[max(c[0] - h // 2, 0), max(c[1] - w // 2, 0), max(c[2] - d // 2, 0), *orient_desc(f, k)]
                     for c, f, k in draws], dtype=np.int32).reshape(-1, 6)
    if (desc[:, 5] != 0).any() and h != w:
        raise ValueError(f'rot90 by an odd k of a non-square patch ({h} x {w}) is not supported')
    n = len(draws)
    oi = torch.empty((n, 1, h, w, d), device=vol.device, dtype=torch.float32) if img is not None else None
    ol = torch.empty((n, 1, h, w, d), device=vol.device, dtype=torch.uint8) if lab is not None else None
    for s in range(0, n, _lib.CROP_ORIENT_MAX):
        e = min(n, s + _lib.CROP_ORIENT_MAX)
        chunk = np.ascontiguousarray(desc[s:e])
        _lib.call('ltu_crop_orient', _p(img), _p(lab), _p(oi[s:e]) if oi is not None else 0, _p(ol[s:e]) if ol is not None else 0,
                  chunk.ctypes.data, e - s, H, W, D, h, w, d, _s())
    return oi, ol


# ---- augmentation of the NIfTI pipeline (csrc/augment.hip; no reference counterpart) --------------------------------------------
# Rotation, zoom, flip, rot90 and the crop are ONE gather from the scan (a rotated patch shows the anatomy around it, not replicated
# borders), with Gaussian noise added in the store; blur and brightness are one launch over the patches; gamma is adjust_contrast.

def patch_matrix(start, size, flip, k, angles=(0.0, 0.0, 0.0), zoom=1.0, spacing=(1.0, 1.0, 1.0)):
    """3x4 float64 pull matrix (patch voxel -> scan voxel) of a patch of `size` whose unrotated crop begins at `start`:
    M = T(start + (size-1)/2) S^-1 Rx Ry Rz (1/zoom) S P T(-(size-1)/2), S = diag(spacing) (the rotation happens in millimetres),
    P the signed permutation of orient_desc(flip, k), angles in radians about H, W, D in rotate_matrix's convention, zoom > 1
    magnifies.  With zero angles and zoom 1 the entries are integers and the matrix selects the voxels crop_orient selects."""
    size = np.asarray(size, dtype=np.float64)
    c = (size - 1) / 2
    fh, fw, swap = orient_desc(flip, k)
    if swap and size[0] != size[1]:
        raise ValueError(f'rot90 by an odd k of a non-square patch ({int(size[0])} x {int(size[1])}) is not supported')
    sa, sb = (-1.0 if fh else 1.0), (-1.0 if fw else 1.0)
    P = np.eye(4)
    P[:2, :2] = [[0.0, sa], [sb, 0.0]] if swap else [[sa, 0.0], [0.0, sb]]
    t0, t1 = np.eye(4), np.eye(4)
    t0[:3, 3], t1[:3, 3] = -c, np.asarray(start, dtype=np.float64) + c
    if not any(float(a) != 0.0 for a in angles) and float(zoom) == 1.0:
        return (t1 @ P @ t0)[:3]                         # exact integers (and halves that cancel)
    ax, ay, az = (float(a) for a in angles)
    rx = np.array([[1, 0, 0, 0], [0, np.cos(ax), -np.sin(ax), 0], [0, np.sin(ax), np.cos(ax), 0], [0, 0, 0, 1]], dtype=np.float64)
    ry = np.array([[np.cos(ay), 0, np.sin(ay), 0], [0, 1, 0, 0], [-np.sin(ay), 0, np.cos(ay), 0], [0, 0, 0, 1]], dtype=np.float64)
    rz = np.array([[np.cos(az), -np.sin(az), 0, 0], [np.sin(az), np.cos(az), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    sp = np.asarray(spacing, dtype=np.float64)
    S, Si = np.diag([*sp, 1.0]), np.diag([*(1.0 / sp), 1.0])
    Z = np.diag([1.0 / float(zoom)] * 3 + [1.0])
    return (t1 @ Si @ rx @ ry @ rz @ Z @ S @ P @ t0)[:3]


def elastic_displacement(phi, size):
    """the displacement field of ltu_sample_elastic in float64 numpy (no GPU): phi [3, gh, gw, gd], the control lattice of one patch
    (displacements in patch voxels along the patch axes H, W, D), size (h, w, d) -> u [3, h, w, d], the uniform cubic B-spline
    free-form deformation of csrc/augment.hip's header comment.  Per axis a with patch coordinate t and extent n_a:
    s = t (g_a - 3) / (n_a - 1) (0 when n_a == 1), i = min(floor(s), g_a - 4), f = s - i,
    B(f) = ((1-f)^3, 3f^3 - 6f^2 + 4, -3f^3 + 3f^2 + 3f + 1, f^3) / 6, u_c(p) = sum_lmn B_l(fx) B_m(fy) B_n(fz) phi[c][ix+l][iy+m][iz+n];
    patch voxel p reads the scan at M (p + u(p), 1)."""
    phi = np.asarray(phi, dtype=np.float64)
    if phi.ndim != 4 or phi.shape[0] != 3 or min(phi.shape[1:]) < 4:
        raise ValueError(f'a control lattice is [3, gh, gw, gd] with extents >= 4, got {phi.shape}')
    wts = []
    for n, g in zip((int(v) for v in size), phi.shape[1:]):
        t = np.arange(n, dtype=np.float64)
        sc = t * (g - 3) / (n - 1) if n > 1 else np.zeros(n)
        i = np.minimum(np.floor(sc), g - 4).astype(np.int64)
        f = sc - i
        B = np.stack([(1 - f) ** 3, 3 * f ** 3 - 6 * f ** 2 + 4, -3 * f ** 3 + 3 * f ** 2 + 3 * f + 1, f ** 3], 1) / 6
        wa = np.zeros((n, g))
        for l in range(4):
            wa[np.arange(n), i + l] += B[:, l]
        wts.append(wa)
    return np.einsum('xl,ym,zn,clmn->cxyz', *wts, phi)


def _check_lattice(elastic):
    """sample_affine's elastic argument, checked on the host: [n, 3, gh, gw, gd] float32 (ndarray or tensor as given), extents 4 ..
    LTU_ELASTIC_MAX_GRID, finite, |phi| <= LTU_ELASTIC_MAX_DISP"""
    if torch.is_tensor(elastic):
        lat = elastic.to(torch.float32).contiguous()
        ok = bool((lat.abs() <= _lib.ELASTIC_MAX_DISP).all())
    else:
        lat = np.ascontiguousarray(np.asarray(elastic, dtype=np.float32))
        ok = bool((np.abs(lat) <= _lib.ELASTIC_MAX_DISP).all())          # False for a NaN
    if lat.ndim != 5 or lat.shape[1] != 3 or not all(4 <= int(g) <= _lib.ELASTIC_MAX_GRID for g in lat.shape[2:]):
        raise ValueError(f'elastic is [n, 3, gh, gw, gd] with lattice extents 4 .. {_lib.ELASTIC_MAX_GRID}, got {tuple(lat.shape)}')
    if not ok:
        raise ValueError(f'elastic must be finite with |phi| <= {_lib.ELASTIC_MAX_DISP} patch voxels')
    return lat


SAMPLE_ORDERS = ((1, 1, 1), (3, 3, 3), (3, 3, 1))      # the gather's interpolation per scan axis H, W, D, as built


def sample_order(order):
    """the `order` of sample_affine / Augmentation / SpacedScan.spline_coefficients as a 3-tuple per scan axis H, W, D: 1 (trilinear),
    3 (cubic B-spline on every axis) or one of SAMPLE_ORDERS; anything else is a ValueError"""
    orders = _order_tuple(order)
    if orders not in SAMPLE_ORDERS:
        raise ValueError(f'the patch gather is built for order 1, 3, (3, 3, 3) and (3, 3, 1) per scan axis H, W, D, got {order!r}')
    return orders


def _gather_coefficients(img, orders):
    """the B-spline coefficients of img [H, W, D] or [K, H, W, D] in its shape for the gather's orders per scan axis H, W, D: one
    spline_coefficients per channel (looked up in this module at call time)"""
    axes = (orders[2], orders[1], orders[0])               # spline_coefficients counts the axes from the fastest: D, W, H
    vols = img if img.dim() == 4 else img[None]
    return torch.stack([spline_coefficients(v, axes) for v in vols]).view(img.shape)


def _channel_bounds(clamp, K):
    """sample_affine's clamp as float32 (lo [K], hi [K]): None, one (lo, hi) pair or one pair per channel"""
    if clamp is None:
        return np.full(K, -np.inf, dtype=np.float32), np.full(K, np.inf, dtype=np.float32)
    c = np.asarray(clamp, dtype=np.float32)
    if c.shape not in ((2,), (K, 2)) or not bool((np.broadcast_to(c, (K, 2))[:, 0] <= np.broadcast_to(c, (K, 2))[:, 1]).all()):
        raise ValueError(f'clamp is (lo, hi) with lo <= hi, or one such pair per channel ({K}), got {clamp!r}')
    c = np.broadcast_to(c, (K, 2))
    return np.ascontiguousarray(c[:, 0]), np.ascontiguousarray(c[:, 1])


def sample_affine(img, lab, mats, size, fill=0.0, noise_sigma=None, seeds=None, elastic=None, order=1, coef=None, clamp=None,
                  label_order=0):
    """ltu_sample_channels (order 1) or ltu_sample_spline (any other order), for every image: device patches ([n,1,h,w,d] f32 or
    None, [n,1,h,w,d] u8 or None) gathered from img / lab [H,W,D] through mats [n,3,4] (float64 pull matrices, patch voxel -> scan
    voxel): image trilinear with `fill` outside the scan, label nearest (round half even) with 0 outside.  noise_sigma [n] with
    seeds [n] (uint64) adds sigma_k * N(0, 1) to patch k in the store (noise_reference restates the generator).  elastic: [n, 3,
    gh, gw, gd] (ndarray or device tensor), one B-spline control lattice per patch in patch voxels; patch voxel p then reads the
    scan at M (p + u(p), 1), u = elastic_displacement; without it the call passes no lattice and runs the affine kernels.
    The lattice is checked on the host (extents 4 .. 8, finite, |phi| <= 64: ValueError) and uploaded once.
    A 3-D img is the K = 1 case (the kernels ltu_sample_affine / ltu_sample_elastic run, which no call here goes through).  A 4-D
    img [K,H,W,D] (K = 1 .. 4 channels on the label's grid, e.g. MultiScan.img) returns
    [n,K,h,w,d]: one gather whose coordinates, taps and label voxel are formed once for all channels.  fill is then a number or one
    per channel, noise_sigma [n] or [n,K], seeds [n,K] (or [n]: channel c of patch k gets channel_seed(seeds[k], c)); channel c has
    the bits of the 3-D call on img[c] with fill[c], noise_sigma[:, c] and seeds[:, c].
    order (sample_order: 1, 3, (3, 3, 3) or (3, 3, 1) per scan axis H, W, D): 1, the default, is everything above.  Any other
    interpolates the image as scipy.ndimage.map_coordinates(order=3, mode='constant', cval=fill) does
    (nnU-Net's spatial transform): the cubic tap sum where the coordinate lies inside [0, S - 1] on every axis, fill elsewhere, no
    blending across the edge; (3, 3, 1) is linear along D, the coarse axis of an anisotropic scan.  coef: the B-spline coefficients
    of img in its shape (SpacedScan.spline_coefficients(order) caches them); None builds them here with spline_coefficients, per
    channel.  clamp: (lo, hi) or one pair per channel, applied to the tap sum, not to fill (the spline rings past a clipped
    intensity window); None = no clamp.  A patch is cubic unless all 12 entries of its matrix are integers and it has no lattice or
    an all-zero one: such a patch keeps the trilinear expressions, that is the source voxels.  The label is order 1's, byte for byte.
    label_order: 0, the default, is the nearest label above.  1 takes it by class vote (ltu_sample_vote, a second, label-only launch
    through the same matrices and lattice; the image is gathered as above with the label left out, so it has the bits of the
    label_order 0 call whatever order, coef, elastic and K are): the 8 taps and fp32 weights of the TRILINEAR bracket (also under a
    cubic image), a tap outside the scan counting for label 0, the weights summed per label value, the smallest value of maximal
    score wins: nnU-Net's "one-hot, order 1".  An integer matrix gives the nearest label byte for byte."""
    orders = sample_order(order)
    vote = label_order_of(label_order) == 1 and lab is not None
    if elastic is not None:
        elastic = _check_lattice(elastic)
    vol = img if img is not None else lab
    if vol is None or not vol.is_cuda:
        raise _lib.LtuError('data.sample_affine runs on the GPU only (no CPU fallback)')
    if img is not None and lab is not None and img.shape[-3:] != lab.shape:
        raise ValueError(f'image {tuple(img.shape)} and label {tuple(lab.shape)} differ in shape')
    if (img is not None and (img.dtype != torch.float32 or not img.is_contiguous())) or \
            (lab is not None and (lab.dtype != torch.uint8 or not lab.is_contiguous())):
        raise ValueError('sample_affine takes a contiguous float32 image and uint8 label')
    K = int(img.shape[0]) if img is not None and img.dim() == 4 else 1          # a 3-D image is the one-channel case of the same call
    if not 1 <= K <= _lib.MAX_INPUT_CHANNELS:
        raise ValueError(f'sample_affine takes 1 .. {_lib.MAX_INPUT_CHANNELS} channels, got {K}')
    H, W, D = vol.shape[-3:]
    h, w, d = (int(s) for s in size)
    m = np.ascontiguousarray(np.asarray(mats, dtype=np.float64).reshape(-1, 12))
    n = m.shape[0]
    sg = sd = None
    if noise_sigma is not None:
        if seeds is None:
            raise ValueError('noise_sigma needs seeds')
        sg = np.ascontiguousarray(np.broadcast_to(np.asarray(noise_sigma, dtype=np.float32).reshape(n, -1), (n, K)))
        sd = np.asarray(seeds, dtype=np.uint64).reshape(n, -1)
        if sd.shape[1] == 1 and K > 1:
            sd = np.array([[channel_seed(s, c) for c in range(K)] for s in sd[:, 0]], dtype=np.uint64)
        sd = np.ascontiguousarray(sd.reshape(n, K))
    oi = torch.empty((n, K, h, w, d), device=vol.device, dtype=torch.float32) if img is not None else None
    ol = torch.empty((n, 1, h, w, d), device=vol.device, dtype=torch.uint8) if lab is not None else None
    lat, g = None, (0, 0, 0)
    if elastic is not None:
        if elastic.shape[0] != n:
            raise ValueError(f'elastic holds {elastic.shape[0]} lattices for {n} matrices')
        lat = (elastic if torch.is_tensor(elastic) else torch.from_numpy(elastic)).to(vol.device)
        g = tuple(int(v) for v in lat.shape[2:])
    cubic = orders != (1, 1, 1) and img is not None        # a label alone has nothing to interpolate
    fl = np.full(K, fill, dtype=np.float32)                # a number for all channels, or one per channel
    if cubic:
        if coef is None:
            coef = _gather_coefficients(img, orders)
        if not torch.is_tensor(coef) or coef.device != img.device or coef.dtype != torch.float32 or not coef.is_contiguous() or \
                coef.numel() != img.numel() or coef.shape[-3:] != img.shape[-3:]:
            raise ValueError(f'coef is a contiguous float32 tensor of the image\'s shape {tuple(img.shape)} on its device')
        lo, hi = _channel_bounds(clamp, K)
        which = (m != np.round(m)).any(1)
        if elastic is not None:
            which = which | (lat.reshape(n, -1) != 0).any(1).cpu().numpy()
        which = np.ascontiguousarray(which.astype(np.uint8))
    def row(a, s):                          # the address of a[s], a contiguous tensor or ndarray (None: 0), without a view object
        if a is None:
            return 0
        return a.data_ptr() + s * a.stride(0) * a.element_size() if torch.is_tensor(a) else a.ctypes.data + s * a.strides[0]
    gl, gol = (None, None) if vote else (lab, ol)          # a voted label is a launch of its own, behind the image's
    for s in range(0, n, _lib.SAMPLE_AFFINE_MAX):
        e = min(n, s + _lib.SAMPLE_AFFINE_MAX)
        common = (row(oi, s), row(gol, s), row(m, s), row(lat, s), *g, row(sg, s), row(sd, s), fl.ctypes.data)
        if cubic:
            _lib.call('ltu_sample_spline', _p(img), _p(coef), _p(gl), *common, lo.ctypes.data, hi.ctypes.data, row(which, s),
                      e - s, K, H, W, D, h, w, d, orders[2], _s())
        elif img is not None or gl is not None:
            _lib.call('ltu_sample_channels', _p(img), _p(gl), *common, e - s, K, H, W, D, h, w, d, _s())
        if vote:
            _lib.call('ltu_sample_vote', _p(lab), row(ol, s), row(m, s), row(lat, s), *g, e - s, H, W, D, h, w, d, _s())
    return oi, ol


def blur_weights(sigma):
    """the 1-D table of scipy.ndimage.gaussian_filter1d(truncate=4.0): float64 [2 r + 1], r = int(4 sigma + 0.5), exp(-k^2 / (2
    sigma^2)) normalised to sum 1; sigma 0 is the unit impulse"""
    sigma = float(sigma)
    r = int(4.0 * sigma + 0.5)
    if r == 0:
        return np.ones(1)
    k = np.arange(-r, r + 1, dtype=np.float64)
    wt = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    return wt / wt.sum()


def gaussian_blur(x, sigmas, mul=None):
    """ltu_gauss_blur3: x [n,(1,)H,W,D] f32 -> mul_k * gaussian_filter(x_k, sigma_k, mode='reflect', truncate=4.0), out of place, one
    launch per LTU_BLUR_MAX_N patches.  sigmas: [n] or [n][3] (per axis H, W, D) in voxels, 0 leaves an axis untouched; a radius
    int(4 sigma + 0.5) above 8 or not below the axis's extent is refused."""
    v = _vol4(x)
    if v.dtype != torch.float32:
        raise ValueError(f'gaussian_blur takes float32 patches, got {v.dtype}')
    n, H, W, D = v.shape
    sg = np.asarray(sigmas, dtype=np.float64)
    sg = np.repeat(sg.reshape(n, 1), 3, 1) if sg.ndim <= 1 else sg.reshape(n, 3)
    taps = _lib.BLUR_MAX_RADIUS + 1
    wts = np.zeros((n, 3, taps), dtype=np.float32)
    rad = np.zeros((n, 3), dtype=np.int32)
    for k in range(n):
        for a in range(3):
            t = blur_weights(sg[k, a])
            r = len(t) // 2
            rad[k, a] = r
            if r < taps:                                  # a larger radius is refused by the call
                wts[k, a, :r + 1] = t[r:]
    ml = np.ascontiguousarray(np.asarray(mul, dtype=np.float32).reshape(n)) if mul is not None else None
    out = torch.empty_like(v)
    for s in range(0, n, _lib.BLUR_MAX_N):
        e = min(n, s + _lib.BLUR_MAX_N)
        _lib.call('ltu_gauss_blur3', _p(v[s:e]), _p(out[s:e]), wts[s:e].ctypes.data, rad[s:e].ctypes.data,
                  ml[s:e].ctypes.data if ml is not None else 0, e - s, H, W, D, _s())
    return out.view(x.shape)


def _f32_volumes(x, what):
    v = _vol4(x)
    if v.dtype != torch.float32:
        raise ValueError(f'{what} takes float32 patches, got {v.dtype}')
    return v, v.shape[0], v.numel() // max(v.shape[0], 1)


def _stats_parts(n, per, device):
    """the scratch of one statistics launch over n volumes of per floats (4 doubles per workgroup)"""
    return torch.empty(max(int(_lib.load().ltu_patch_stats_parts_elems(n, per)), 4), dtype=torch.float64, device=device)


def patch_stats(x):
    """ltu_patch_stats: x [n,(1,)H,W,D] f32 -> [n, 4] float64 on the device, {min, max, sum, sum of squares} of every volume (the sums
    in fp64, bit-reproducible).  Nothing is read back."""
    v, n, per = _f32_volumes(x, 'patch_stats')
    out = torch.empty((n, 4), dtype=torch.float64, device=v.device)
    if n:
        parts = _stats_parts(n, per, v.device)
        _lib.call('ltu_patch_stats', _p(v), n, per, _p(parts), parts.numel(), _p(out), _s())
    return out


def _intensity_apply(v, ops, params, retain):
    """ltu_intensity_apply (+ ltu_intensity_rescale on the volumes of `retain`) over v [n,H,W,D], LTU_INTENSITY_AUG_MAX_N volumes per
    launch; ops, params, retain: host lists of n"""
    n, per = v.shape[0], v.numel() // max(v.shape[0], 1)
    ops = np.ascontiguousarray(ops, dtype=np.int32)
    par = np.ascontiguousarray(params, dtype=np.float32)
    if not np.isfinite(par).all():
        raise ValueError(f'an intensity parameter is a finite number, got {list(params)}')
    par = np.where(par > 0, par, np.float32(0.0)).astype(np.float32)          # non-positive: the volume is left untouched
    on = np.ascontiguousarray(np.asarray(retain, dtype=bool) & (par > 0) & (ops >= _lib.IAUG_GAMMA), dtype=np.uint8)
    out = torch.empty_like(v)
    step = _lib.INTENSITY_AUG_MAX_N
    for s in range(0, n, step):
        e = min(n, s + step)
        m = e - s
        parts = _stats_parts(m, per, v.device)
        sx = torch.empty((m, 4), dtype=torch.float64, device=v.device)
        _lib.call('ltu_patch_stats', _p(v[s:e]), m, per, _p(parts), parts.numel(), _p(sx), _s())
        if on[s:e].any():
            sy = torch.empty((m, 4), dtype=torch.float64, device=v.device)
            _lib.call('ltu_intensity_apply', _p(v[s:e]), _p(out[s:e]), ops[s:e].ctypes.data, par[s:e].ctypes.data, _p(sx), m, per,
                      _p(parts), parts.numel(), _p(sy), _s())
            _lib.call('ltu_intensity_rescale', _p(out[s:e]), on[s:e].ctypes.data, _p(sx), _p(sy), m, per, _s())
        else:
            _lib.call('ltu_intensity_apply', _p(v[s:e]), _p(out[s:e]), ops[s:e].ctypes.data, par[s:e].ctypes.data, _p(sx), m, per,
                      0, 0, 0, _s())
    return out


def contrast(x, factors):
    """nnU-Net's contrast augmentation per volume of x [n,(1,)H,W,D] f32: clip((x - mean) * f + mean, min, max) with the volume's own
    mean, min and max (taken on the device, never read back).  A factor <= 0 leaves that volume untouched, bit for bit."""
    v, n, _ = _f32_volumes(x, 'contrast')
    f = np.asarray(factors, dtype=np.float64).reshape(n)
    return _intensity_apply(v, np.full(n, _lib.IAUG_CONTRAST), f, np.zeros(n, bool)).view(x.shape)


def gamma_transform(x, gammas, invert=False, retain_stats=True):
    """nnU-Net's gamma transform per volume of x [n,(1,)H,W,D] f32, on u = -x when invert (one flag or one per volume):
    v = ((u - min u) / max(r, 1e-7))^g * r + min u with r = max u - min u; retain_stats then rescales v to the mean and standard
    deviation of u; the result is -v when invert.  g <= 0 leaves that volume untouched, a constant volume comes back unchanged.
    Statistics stay on the device: the call can be captured."""
    v, n, _ = _f32_volumes(x, 'gamma_transform')
    g = np.asarray(gammas, dtype=np.float64).reshape(n)
    inv = np.broadcast_to(np.asarray(invert, dtype=bool), (n,))
    ops = np.where(inv, _lib.IAUG_GAMMA_INV, _lib.IAUG_GAMMA)
    return _intensity_apply(v, ops, g, np.broadcast_to(np.asarray(retain_stats, dtype=bool), (n,))).view(x.shape)


def lowres_tables(size, scale, axes=(0, 1, 2)):
    """the gather tables of nnU-Net's low-resolution simulation for one volume of extents size = (H, W, D): nearest-exact down to
    S' = max(int(round(S * scale)), 1) on the axes in `axes` (S' = S on the others), then trilinear up, composed per output index o:
      src = max((o + 0.5) * S' / S - 0.5, 0),  j0 = min(floor(src), S' - 1),  j1 = min(j0 + 1, S' - 1),  l = src - j0 (0 where j0 == j1)
    in float64, and the low index j reads the high index min(((2 j + 1) S) // (2 S'), S - 1).  Returns (idx int32 [2][H + W + D], lam
    float32 [H + W + D]): the high-resolution indices of the lower and the upper tap and the upper tap's weight, axis H first.  An
    axis with S' == S gives idx[0] == o and l == 0: the identity.  scale outside (0, 1] raises ValueError."""
    t = _lowres_packed(size, [scale], axes)[0]
    return t[:2].copy(), t[2].view(np.float32).copy()


@functools.lru_cache(maxsize=4096)
def _lowres_axis(S, Sl):
    """one axis of extent S through a low extent Sl, int32 [3][S]: lower tap, upper tap, the float32 weight's bits.  Kept per (S, Sl):
    a training run draws scales without end but meets at most S low extents per axis"""
    src = np.maximum((np.arange(S, dtype=np.float64) + 0.5) * Sl / S - 0.5, 0.0)
    j0 = np.minimum(np.floor(src).astype(np.int64), Sl - 1)
    j1 = np.minimum(j0 + 1, Sl - 1)
    out = np.empty((3, S), dtype=np.int32)
    out[0] = np.minimum(((2 * j0 + 1) * S) // (2 * Sl), S - 1)
    out[1] = np.minimum(((2 * j1 + 1) * S) // (2 * Sl), S - 1)
    out[2].view(np.float32)[...] = np.where(j0 == j1, 0.0, src - j0)
    out.setflags(write=False)
    return out


def _lowres_packed(size, scales, axes):
    """lowres_tables of n scales as ltu_lowres_gather takes them, int32 [n][3][H + W + D] (plane 2: the float32 weights' bits)"""
    size = tuple(int(v) for v in size)
    sc = [float(s) for s in scales]
    for s in sc:
        if not 0.0 < s <= 1.0:
            raise ValueError(f'a low-resolution scale lies in (0, 1], got {s}')
    axes = tuple(int(a) for a in axes)
    if any(a not in (0, 1, 2) for a in axes):
        raise ValueError(f'lowres axes are patch axes 0, 1, 2, got {axes}')
    out = np.empty((len(sc), 3, sum(size)), dtype=np.int32)
    off = 0
    for a, S in enumerate(size):
        for k, s in enumerate(sc):
            out[k, :, off:off + S] = _lowres_axis(S, max(int(round(S * s)), 1) if a in axes else S)
        off += S
    return out


def lowres_device_tables(size, scales, axes=(0, 1, 2), device='cuda'):
    """lowres_tables of every scale as ltu_lowres_gather takes them: int32 [n][3][H + W + D] on the device (the third plane holds the
    float32 weights' bits).  A scale <= 0 gives the identity table (that volume stays untouched)."""
    sc = np.asarray(scales, dtype=np.float64).reshape(-1)
    return torch.from_numpy(_lowres_packed(size, np.where(sc > 0, sc, 1.0), axes)).to(device)


def simulate_lowres(x, scales, axes=(0, 1, 2), tables=None):
    """nnU-Net's SimulateLowResolution per volume of x [n,(1,)H,W,D] f32: F.interpolate(F.interpolate(x, size=S', mode='nearest-exact'),
    size=S, mode='trilinear') as one 8-tap gather (ltu_lowres_gather), no low-resolution volume in between.  scales: one per volume
    in (0, 1]; above 1 raises ValueError, <= 0 leaves that volume untouched; an axis outside `axes`, or scale 1, returns the input's
    bits.  tables: lowres_device_tables(...) made beforehand (their upload is the one step of this call that cannot be captured);
    scales and axes are then not looked at."""
    v, n, _ = _f32_volumes(x, 'simulate_lowres')
    _, H, W, D = v.shape
    if tables is None:
        tables = lowres_device_tables((H, W, D), np.asarray(scales, dtype=np.float64).reshape(n), axes, v.device)
    if tables.dtype != torch.int32 or tuple(tables.shape) != (n, 3, H + W + D) or tables.device != v.device or not tables.is_contiguous():
        raise ValueError(f'tables are a contiguous int32 [{n}][3][{H + W + D}] on {v.device}')
    out = torch.empty_like(v)
    _lib.call('ltu_lowres_gather', _p(v), _p(out), _p(tables), n, H, W, D, _s())
    return out.view(x.shape)


def _fmix32(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def noise_reference(seed, count):
    """the N(0, 1) deviates ltu_sample_affine adds (times sigma) to voxels 0 .. count-1 (linear index in the patch) of a patch with
    this seed: the generator of csrc/augment.hip's header comment on the same 32-bit words, Box-Muller in float64"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    with np.errstate(over='ignore'):
        lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)
        g = np.uint32(0x9E3779B1)
        ka = _fmix32(lo ^ np.uint32(0x243F6A88)) + _fmix32(hi ^ np.uint32(0x85A308D3)) * g
        kb = _fmix32(hi ^ np.uint32(0x13198A2E)) + _fmix32(lo ^ np.uint32(0x03707344)) * g
        j = np.arange((int(count) + 1) // 2, dtype=np.uint32)
        w1 = _fmix32(j ^ ka)
        w2 = _fmix32((j + np.uint32(0x9E3779B9)) ^ kb)
    u1 = ((w1 >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = ((w2 >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)], 1).ravel()
    return z[:int(count)]


class Augmentation:
    """The random augmentations of data.sample(..., augment=): a plain record of probabilities and ranges.  rot_range: the largest
    |angle| in radians about H, W, D (the default rotates about D only: slices are 2 mm against 0.5 mm in plane); zoom > 1
    magnifies; noise_std, blur_sigma (voxels), brightness and gamma are uniform ranges; fill: the image value outside the scan, None =
    the lower bound of the scan's intensity window (0.0 when it has none).  elastic_prob > 0 adds a B-spline free-form deformation
    (elastic_displacement): a control lattice of elastic_grid points per patch axis, uniform in +-elastic_mm millimetres of the scan
    with elastic_mm drawn from its range; 0 (the default) makes no draw for it.  order (sample_order: 1, 3, (3, 3, 3) or (3, 3, 1)
    per scan axis H, W, D): the image interpolation of the patches that rotate, zoom or deform; 1, the default, is trilinear, any
    other is sample_affine's cubic B-spline from scan.spline_coefficients(order) (nnU-Net interpolates at order 3), clamped to each
    channel's intensity window.  It makes no draw: draw() returns the same values and leaves the generator in the same state.
    label_order: 0 (nearest, the default) or 1: the label of every patch by class vote (sample_affine's label_order), carried into
    data.sample's gather.  It makes no draw either.
    contrast_prob, lowres_prob, invgamma_prob > 0 add nnU-Net's contrast (data.contrast, factor from `contrast`), low-resolution
    simulation (data.simulate_lowres, scale from lowres_scale on the patch axes lowres_axes) and gamma on the inverted image
    (data.gamma_transform(invert=True), exponent from invgamma); each draws (fire, value) behind the elastic draws, in this order,
    and 0 (the default) makes no draw for it.  retain_stats=True runs both gammas through data.gamma_transform with the patch's mean
    and standard deviation restored (nnU-Net's GammaTransform); False keeps the gamma draw on monai's adjust_contrast.  It makes no
    draw either.  Augmentation.nnunet() is the record with nnU-Net's default probabilities and ranges."""

    def __init__(self, rot_prob=0.2, rot_range=(0.0, 0.0, np.pi), zoom_prob=0.2, zoom_range=(0.7, 1.4), noise_prob=0.1,
                 noise_std=(0.0, 0.1), blur_prob=0.2, blur_sigma=(0.5, 1.0), brightness_prob=0.15, brightness=(0.75, 1.25),
                 gamma_prob=0.3, gamma=(0.7, 1.5), fill=None, elastic_prob=0.0, elastic_mm=(0.0, 4.0), elastic_grid=(6, 6, 4), order=1,
                 contrast_prob=0.0, contrast=(0.75, 1.25), lowres_prob=0.0, lowres_scale=(0.5, 1.0), lowres_axes=(0, 1, 2),
                 invgamma_prob=0.0, invgamma=(0.7, 1.5), retain_stats=False, label_order=0):
        self.label_order = label_order_of(label_order)
        self.contrast_prob, self.contrast = contrast_prob, tuple(float(v) for v in contrast)
        self.lowres_prob, self.lowres_scale = lowres_prob, tuple(float(v) for v in lowres_scale)
        self.lowres_axes = tuple(int(a) for a in lowres_axes)
        if not all(a in (0, 1, 2) for a in self.lowres_axes):
            raise ValueError(f'lowres_axes are patch axes 0, 1, 2, got {lowres_axes}')
        if not 0.0 < min(self.lowres_scale) <= max(self.lowres_scale) <= 1.0:
            raise ValueError(f'lowres_scale is a range inside (0, 1], got {lowres_scale}')
        self.invgamma_prob, self.invgamma = invgamma_prob, tuple(float(v) for v in invgamma)
        self.retain_stats = bool(retain_stats)
        self.order = sample_order(order)
        self.elastic_prob, self.elastic_mm = elastic_prob, tuple(float(v) for v in elastic_mm)
        self.elastic_grid = tuple(int(g) for g in elastic_grid)
        if len(self.elastic_grid) != 3 or not all(4 <= g <= _lib.ELASTIC_MAX_GRID for g in self.elastic_grid):
            raise ValueError(f'elastic_grid is three lattice extents 4 .. {_lib.ELASTIC_MAX_GRID}, got {elastic_grid}')
        self.rot_prob, self.rot_range = rot_prob, tuple(rot_range)
        self.zoom_prob, self.zoom_range = zoom_prob, tuple(zoom_range)
        self.noise_prob, self.noise_std = noise_prob, tuple(noise_std)
        self.blur_prob, self.blur_sigma = blur_prob, tuple(blur_sigma)
        self.brightness_prob, self.brightness = brightness_prob, tuple(brightness)
        self.gamma_prob, self.gamma = gamma_prob, tuple(gamma)
        self.fill = fill

    def draw(self, rs):
        """one sample's draws in their fixed order; every draw is made whether or not its transform fires (draw_augmentation's
        convention)"""
        p = {}
        p['rotate'] = rs.rand() < self.rot_prob
        p['angles'] = [rs.uniform(-r, r) for r in self.rot_range]
        p['zoom'] = rs.rand() < self.zoom_prob
        p['zoom_factor'] = rs.uniform(*self.zoom_range)
        p['noise'] = rs.rand() < self.noise_prob
        p['noise_std'] = rs.uniform(*self.noise_std)
        p['seed'] = (int(rs.randint(2 ** 31)) << 31) | int(rs.randint(2 ** 31))
        p['blur'] = rs.rand() < self.blur_prob
        p['sigma'] = rs.uniform(*self.blur_sigma)
        p['bright'] = rs.rand() < self.brightness_prob
        p['mul'] = rs.uniform(*self.brightness)
        p['contrast'] = rs.rand() < self.gamma_prob
        p['gamma'] = rs.uniform(*self.gamma)
        if self.elastic_prob > 0:
            p['elastic'] = rs.rand() < self.elastic_prob
            p['elastic_mm'] = rs.uniform(*self.elastic_mm)
            p['phi'] = rs.uniform(-1, 1, (3, *self.elastic_grid))
        if self.contrast_prob > 0:
            p['scale_contrast'] = rs.rand() < self.contrast_prob
            p['contrast_factor'] = rs.uniform(*self.contrast)
        if self.lowres_prob > 0:
            p['lowres'] = rs.rand() < self.lowres_prob
            p['lowres_scale'] = rs.uniform(*self.lowres_scale)
        if self.invgamma_prob > 0:
            p['invgamma'] = rs.rand() < self.invgamma_prob
            p['invgamma_g'] = rs.uniform(*self.invgamma)
        return p

    @classmethod
    def nnunet(cls, **overrides):
        """nnU-Net's default training augmentation: rotation 0.2, zoom 0.2 over (0.7, 1.4), noise 0.1, blur 0.2, brightness 0.15,
        contrast 0.15, low resolution 0.25 over (0.5, 1), inverted gamma 0.1 and gamma 0.3 over (0.7, 1.5) with retain_stats, order-3
        interpolation.  overrides replace any of them.  nnU-Net's own spatial transform interpolates the label at order 1 on
        one-hot maps; this record keeps label_order 0 (nearest), as it always has: pass label_order=1 for nnU-Net's label."""
        kw = dict(rot_prob=0.2, zoom_prob=0.2, zoom_range=(0.7, 1.4), noise_prob=0.1, blur_prob=0.2, brightness_prob=0.15,
                  contrast_prob=0.15, contrast=(0.75, 1.25), lowres_prob=0.25, lowres_scale=(0.5, 1.0), invgamma_prob=0.1,
                  invgamma=(0.7, 1.5), gamma_prob=0.3, gamma=(0.7, 1.5), retain_stats=True, order=3)
        kw.update(overrides)
        return cls(**kw)

    def check_fold(self, spatial_size, pixdim, swap=True):
        """ValueError unless the largest control displacement this record can draw stays within 0.4 lattice cells on every patch
        axis: max(elastic_mm) * max(zoom_range) / pixdim_a <= 0.4 (size_a - 1) / (g_a - 3).  0.4 cells is the known injectivity
        bound of the cubic B-spline free-form deformation (Choi and Lee: 1 / 2.48), so the deformed patch cannot fold.  swap: a
        rot90 by an odd k may map patch axis H onto scan axis W and W onto H, the finer of the two in-plane spacings then counts
        for both.  Nothing is checked while elastic_prob == 0."""
        if not self.elastic_prob > 0:
            return
        pix = [float(v) for v in pixdim]
        if swap:
            pix[0] = pix[1] = min(pix[0], pix[1])
        for a in range(3):
            vox = max(self.elastic_mm) * max(self.zoom_range) / pix[a]
            cap = 0.4 * (int(spatial_size[a]) - 1) / (self.elastic_grid[a] - 3)
            if not vox <= cap:
                raise ValueError(f'elastic deformation may fold along patch axis {a}: up to {vox:.3g} voxels (elastic_mm '
                                 f'{max(self.elastic_mm):g} mm x zoom {max(self.zoom_range):g} / {pix[a]:g} mm) against 0.4 lattice cells '
                                 f'= {cap:.3g} voxels (size {int(spatial_size[a])}, lattice {self.elastic_grid[a]})')


def _channels(scan):
    """any scan object as channels: (K, the K intensity windows, the K `outside` values).  A 3-D img (or none) is one channel whose
    `intensity` and `outside` are single values; a 4-D img [K, H, W, D] carries lists of K (`outside` may be missing: K Nones)"""
    img = getattr(scan, 'img', None)
    windows, outside = getattr(scan, 'intensity', None), getattr(scan, 'outside', None)
    if img is None or img.dim() != 4:
        return 1, [windows], [outside]
    K = int(img.shape[0])
    return K, list(windows) if windows is not None else [None] * K, list(outside) if outside is not None else [None] * K


def _scan_fill(scan, augment):
    """the image value outside the scan: augment.fill, or (None) scan.outside where the scan names one (0.0 under
    'zscore_nonzero': the value of everything outside the mask), else the floor of the scan's intensity window, 0.0 where it has
    none.  One value per channel, in the scan's own presentation: a list of K for a 4-D img, the number itself for a 3-D one"""
    K, windows, outside = _channels(scan)
    if augment is None:
        fills = [0.0] * K
    elif augment.fill is not None:
        fills = [float(augment.fill)] * K
    else:
        lows = [intensity_map(wd)[2] for wd in windows]
        fills = [float(named) if named is not None else float(lo) if np.isfinite(lo) else 0.0 for named, lo in zip(outside, lows)]
    return fills if scan.img is not None and scan.img.dim() == 4 else fills[0]


def _augmented(scan, draws, params, spatial_size, augment, spacing):
    """the patches of draws [(centre, flip, k)] under params (one Augmentation.draw per patch): one sample_affine, then one
    gaussian_blur if a patch blurs or brightens, then contrast, simulate_lowres and gamma_transform(invert=True) where a patch fires
    them, then the gamma draw: adjust_contrast, or gamma_transform under augment.retain_stats.  A MultiScan's K channels come out of
    the one gather (noise per channel from channel_seed); every later stage sees [n K, h, w, d] with each patch's parameters repeated
    K times (statistics are per channel).  params None: the plain patches through patch_matrix's integer matrices (a MultiScan only)."""
    size = tuple(int(s) for s in spatial_size)
    fill = _scan_fill(scan, augment)
    if params is None:
        mats = [patch_matrix([max(c[a] - size[a] // 2, 0) for a in range(3)], size, f, k) for c, f, k in draws]
        return sample_affine(scan.img, scan.lab, np.stack(mats), size, fill)          # integer matrices: either label_order's bytes
    mats = [patch_matrix([max(c[a] - size[a] // 2, 0) for a in range(3)], size, f, k,
                         p['angles'] if p['rotate'] else (0.0, 0.0, 0.0), p['zoom_factor'] if p['zoom'] else 1.0, spacing)
            for (c, f, k), p in zip(draws, params)]
    noisy = any(p['noise'] for p in params)
    lattice = None
    if any(p.get('elastic') for p in params):
        # millimetres of the scan -> patch voxels: patch axis c runs along scan axis axis(c) (an odd k swaps H and W), and a patch
        # voxel covers pixdim / zoom of it; a patch that does not fire keeps a zero lattice (the bits of sample_affine's general kernel)
        lattice = np.zeros((len(params), 3, *augment.elastic_grid), dtype=np.float32)
        for i, ((_, f, k), p) in enumerate(zip(draws, params)):
            if p['elastic']:
                swap = orient_desc(f, k)[2]
                zf = p['zoom_factor'] if p['zoom'] else 1.0
                for c, a in enumerate((1, 0, 2) if swap else (0, 1, 2)):
                    lattice[i, c] = p['phi'][c] * (p['elastic_mm'] * zf / float(spacing[a]))
    cubic = {}
    if augment.order != (1, 1, 1):
        # the patches that rotate, zoom or deform are the ones without an integer matrix and a zero lattice: sample_affine's own
        # rule picks them; the others stay the source voxels.  The clamp is each channel's window, +-inf where it has none
        cubic = dict(order=augment.order, coef=scan.spline_coefficients(augment.order),
                     clamp=[intensity_map(wd)[2:4] for wd in _channels(scan)[1]])
    img, lab = sample_affine(scan.img, scan.lab, np.stack(mats), size, fill,
                             [p['noise_std'] if p['noise'] else 0.0 for p in params] if noisy else None,
                             [p['seed'] for p in params] if noisy else None, elastic=lattice, label_order=augment.label_order,
                             **cubic)
    shape, K = img.shape, img.shape[1]
    img = img.view(-1, 1, *size)

    def per_channel(values):
        return [v for v in values for _ in range(K)]
    if any(p['blur'] or p['bright'] for p in params):
        img = gaussian_blur(img, per_channel(p['sigma'] if p['blur'] else 0.0 for p in params),
                            per_channel(p['mul'] if p['bright'] else 1.0 for p in params))
    if any(p.get('scale_contrast') for p in params):
        img = contrast(img, per_channel(p['contrast_factor'] if p.get('scale_contrast') else -1.0 for p in params))
    if any(p.get('lowres') for p in params):
        img = simulate_lowres(img, per_channel(p['lowres_scale'] if p.get('lowres') else -1.0 for p in params), augment.lowres_axes)
    if any(p.get('invgamma') for p in params):
        img = gamma_transform(img, per_channel(p['invgamma_g'] if p.get('invgamma') else -1.0 for p in params), invert=True,
                              retain_stats=augment.retain_stats)
    if any(p['contrast'] for p in params):
        gammas = per_channel(p['gamma'] if p['contrast'] else -1.0 for p in params)
        img = gamma_transform(img, gammas, invert=False, retain_stats=True) if augment.retain_stats else adjust_contrast(img, gammas)
    return img.view(shape), lab


def sample_draws(scan, spatial_size, rand_state, num_samples=1, flip_prob=0.5, rot90_prob=0.5, host_centers=False, ratios=None,
                 augment=None):
    """every host draw of one data.sample call: ([(centre, flip, k)], [Augmentation.draw dict] or None).  The four draws of every
    sample come first, exactly as without augment (so the crops, flips and rot90s of an augmented call are those of the plain
    call from the same generator); the augmentation draws of sample 0, 1, ... follow.  An augment that deforms is checked against
    folding first (Augmentation.check_fold: ValueError before any draw is consumed)."""
    if augment is not None:
        augment.check_fold(spatial_size, getattr(scan, 'pixdim', (1.0, 1.0, 1.0)), swap=rot90_prob > 0)
    if host_centers and ratios is None:
        draws = [draw_monai_sample(scan.label_host, spatial_size, rand_state, flip_prob, rot90_prob) for _ in range(num_samples)]
    else:
        index = None if host_centers else scan.crop_index
        centres, rest = [], []
        for _ in range(num_samples):
            if host_centers:
                centres.append(class_crop_centers(scan.label_host, spatial_size, 1, ratios, len(ratios), rand_state)[0])
            elif ratios is not None:
                centres.extend(index.class_queries(1, ratios, len(ratios), rand_state))
            else:
                centres.extend(_posneg_queries(index.n_foreground, index.n_background, 1, 0.7, 0.3, rand_state))
            flip = rand_state.rand() < flip_prob
            k = rand_state.randint(3) + 1
            rot = rand_state.rand() < rot90_prob
            rest.append((bool(flip), int(k) if rot else 0))
        if index is not None:
            centres = index.resolve(centres, spatial_size)
        draws = [(c, f, k) for c, (f, k) in zip(centres, rest)]
    return draws, ([augment.draw(rand_state) for _ in range(num_samples)] if augment is not None else None)


def sample(scan, spatial_size, rand_state, num_samples=1, flip_prob=0.5, rot90_prob=0.5, host_centers=False, ratios=None,
           augment=None):
    """the random half of the driver's dataset: num_samples patches ([n,1,h,w,d] f32, u8) of a SpacedScan, each with its own
    crop centre, flip and rot90 in draw_monai_sample's order.  The centres come from scan.crop_index: every host draw of every
    sample is made first (per sample: centre, flip, k, rotation probability), then one select launch resolves all centres.
    host_centers=True draws them from scan.label_host instead (np.nonzero passes over the label per sample): the same patches
    from the same generator.  ratios: one weight per class 0 .. num_classes - 1 switches the centre draw from
    RandCropByPosNegLabeld to RandCropByLabelClassesd (class_centers / class_crop_centers, num_samples 1 per sample).
    augment: an Augmentation.  The draws above keep their place; behind them come, per sample, Augmentation.draw's (rotation fire,
    three angles; zoom fire, factor; noise fire, std, two seed words; blur fire, sigma; brightness fire, multiplier; gamma fire,
    gamma; with elastic_prob > 0 also: deformation fire, its amplitude in millimetres, the control lattice; with contrast_prob,
    lowres_prob, invgamma_prob > 0 also, in this order and each only for its own probability: fire and factor, fire and scale, fire
    and exponent).  The patches are then
    gathered through patch_matrix by one sample_affine (rotation in millimetres of scan.pixdim, the B-spline deformation of the
    patches that fire it folded into the same gather, noise in the store), blurred / brightened by one gaussian_blur, then
    contrast, simulate_lowres and the inverted gamma_transform where fired, and gamma-adjusted by adjust_contrast (gamma_transform
    with augment.retain_stats).  None changes nothing: the same draws, patches and generator state.
    A MultiScan gives ([n,K,h,w,d] f32, [n,1,h,w,d] u8): the host draws do not depend on K, the K channels of a patch share its
    geometry, blur, brightness and gamma and get independent noise (channel c from channel_seed(seed, c)); fill=None takes each
    channel's own window floor.  Its plain path is the same gather through patch_matrix's integer matrices (the source voxels)."""
    if scan.lab is None:
        raise ValueError('sampling needs a label (RandCropByPosNegLabeld draws centres from it)')
    draws, params = sample_draws(scan, spatial_size, rand_state, num_samples, flip_prob, rot90_prob, host_centers, ratios, augment)
    if augment is None and (scan.img is None or scan.img.dim() == 3):          # the plain crop of one volume is its own kernel
        return crop_orient(scan.img, scan.lab, draws, spatial_size)
    return _augmented(scan, draws, params, spatial_size, augment, getattr(scan, 'pixdim', (1.0, 1.0, 1.0)))


def to_native(label_map, scan, order=0):
    """nearest resampling of an RAS u8 label map [H,W,D] (leading size-1 axes allowed; e.g. evaluate_multiclass's 'label_map')
    back onto the file's grid through the inverse pull matrix: u8 [Z][Y][X] on the device, ready for nifti.save(...,
    scan.native_affine, like=scan.native).  order: 0 is that nearest label; 1 pulls the label map back by class vote
    (data.resample's label_order 1), into the whole file grid and into the box of a cropped scan alike."""
    order = label_order_of(order)
    lm = label_map.reshape(scan.shape)
    if lm.dtype != torch.uint8:
        raise ValueError(f'to_native takes a uint8 label map, got {lm.dtype}')
    lm = lm.contiguous()
    H, W, D = scan.shape
    X, Y, Z = scan.native_shape
    box = getattr(scan, 'crop_box', None)
    if box is None:
        _, out = resample(None, lm, geometry.invert(scan.matrix), (X, Y, Z), src_strides=(W * D, D, 1), out_strides=(1, X, X * Y),
                          label_order=order)
        return out
    # a cropped scan: its matrix leads into the box, which is written in place inside a file-sized volume of zeros
    (z0, z1), (y0, y1), (x0, x1) = box
    out = torch.zeros((Z, Y, X), device=lm.device, dtype=torch.uint8)
    resample(None, lm, geometry.invert(scan.matrix), (x1 - x0, y1 - y0, z1 - z0), src_strides=(W * D, D, 1),
             out_strides=(1, X, X * Y), out=(None, out[z0:z1, y0:y1, x0:x1]), label_order=order)
    return out


def to_native_probs(probs, scan, classes=()):
    """the arg-max on the file's grid: RAS f32 probabilities [C, H, W, D] (a leading size-1 batch axis allowed, e.g.
    infer_volume(..., probs=True)[0:1]) are pulled back through the inverse pull matrix with trilinear sampling and the arg-max is
    taken there (nnU-Net's export order; to_native resamples a ready-made label map with nearest sampling instead).
    Returns (u8 label [Z][Y][X] on the device, ready for nifti.save(..., scan.native_affine, like=scan.native), f32 [K][Z][Y][X]
    probabilities of `classes` on that grid or None)."""
    if probs.dim() == 5 and probs.shape[0] == 1:
        probs = probs[0]
    if probs.dim() != 4 or tuple(probs.shape[1:]) != tuple(scan.shape):
        raise ValueError(f'to_native_probs takes probabilities [C, {", ".join(str(n) for n in scan.shape)}], got {tuple(probs.shape)}')
    if probs.dtype != torch.float32:
        raise ValueError(f'to_native_probs takes float32 probabilities, got {probs.dtype}')
    H, W, D = scan.shape
    X, Y, Z = scan.native_shape
    box = getattr(scan, 'crop_box', None)
    if box is None:
        return resample_argmax(probs, geometry.invert(scan.matrix), (X, Y, Z), src_strides=(W * D, D, 1), out_strides=(1, X, X * Y),
                               classes=classes)
    # a cropped scan: outside the box the label is 0 and a requested map holds 1 for class 0, 0 for every other class
    (z0, z1), (y0, y1), (x0, x1) = box
    ks = sorted({int(k) for k in classes})
    ol = torch.zeros((Z, Y, X), device=probs.device, dtype=torch.uint8)
    op = None
    if ks:
        op = torch.zeros((len(ks), Z, Y, X), device=probs.device, dtype=torch.float32)
        if ks[0] == 0:
            op[0].fill_(1.0)
    resample_argmax(probs, geometry.invert(scan.matrix), (x1 - x0, y1 - y0, z1 - z0), src_strides=(W * D, D, 1),
                    out_strides=(1, X, X * Y), classes=classes, out=(ol[z0:z1, y0:y1, x0:x1], op[:, z0:z1, y0:y1, x0:x1] if ks else None))
    return ol, op
