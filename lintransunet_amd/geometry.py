"""Voxel geometry of monai's Spacingd + Orientationd (dataset/CT_pancreas_monai.py:47-48), on the host in float64.

Restated from monai 0.7.0 (`zoom_affine`, `compute_shape_offset`, `Spacing`, `Orientation`) and nibabel (`io_orientation`,
`axcodes2ornt`, `ornt_transform`, `inv_ornt_aff`); neither library is a dependency, so parity with them is unpinned (the
algorithms are restated from their published sources, as data.py does for monai's crop logic).

`spacing_plan` composes both transforms into one 3x4 pull matrix that takes an output voxel index (the RAS grid) to a source voxel
index (the file's grid).  The composition is exact: Spacingd resamples, and the Orientationd that follows is a pure flip and
transpose of the resampled grid, which folds into the matrix without changing a value.
"""
import numpy as np

LABELS = (('L', 'R'), ('P', 'A'), ('I', 'S'))


def io_orientation(affine, tol=None):
    """nibabel io_orientation: [[out axis, +-1]] per input axis of the affine's closest shear-free rotation"""
    affine = np.asarray(affine, dtype=np.float64)
    q, p = affine.shape[0] - 1, affine.shape[1] - 1
    RZS = affine[:q, :p]
    zooms = np.sqrt(np.sum(RZS * RZS, axis=0))
    zooms[zooms == 0] = 1
    RS = RZS / zooms
    P, S, Qs = np.linalg.svd(RS, full_matrices=False)
    if tol is None:
        tol = S.max() * max(RS.shape) * np.finfo(S.dtype).eps
    keep = S > tol
    R = np.dot(P[:, keep], Qs[keep])
    ornt = np.full((p, 2), np.nan)
    for in_ax in range(p):
        col = R[:, in_ax]
        if not np.allclose(col, 0):
            out_ax = int(np.argmax(np.abs(col)))
            ornt[in_ax] = (out_ax, -1 if col[out_ax] < 0 else 1)
            R[out_ax, :] = 0
    return ornt


def axcodes2ornt(axcodes, labels=LABELS):
    """nibabel axcodes2ornt: 'RAS' -> [[0, 1], [1, 1], [2, 1]]"""
    ornt = np.full((len(axcodes), 2), np.nan)
    for i, code in enumerate(axcodes):
        for j, (lo, hi) in enumerate(labels):
            if code == lo:
                ornt[i] = (j, -1)
            elif code == hi:
                ornt[i] = (j, 1)
        if np.isnan(ornt[i, 0]):
            raise ValueError(f'axis code {code!r} is not one of {labels}')
    if len(set(ornt[:, 0])) != len(axcodes):
        raise ValueError(f'axis codes {axcodes!r} name an axis twice')
    return ornt


def ornt_transform(start_ornt, end_ornt):
    """nibabel ornt_transform: the orientation that takes an array in start_ornt to end_ornt"""
    start_ornt, end_ornt = np.asarray(start_ornt), np.asarray(end_ornt)
    result = np.empty_like(start_ornt)
    for end_in_idx, (end_out_idx, end_flip) in enumerate(end_ornt):
        for start_in_idx, (start_out_idx, start_flip) in enumerate(start_ornt):
            if end_out_idx == start_out_idx:
                result[start_in_idx] = (end_in_idx, 1 if start_flip == end_flip else -1)
                break
        else:
            raise ValueError(f'unable to take orientation {start_ornt.tolist()} to {end_ornt.tolist()}')
    return result


def inv_ornt_aff(ornt, shape):
    """nibabel inv_ornt_aff: the affine from the re-oriented array's voxel indices to the original's"""
    ornt = np.asarray(ornt)
    p = ornt.shape[0]
    shape = np.asarray(shape, dtype=np.float64)[:p]
    undo_reorder = np.eye(p + 1)[[int(i) for i in ornt[:, 0]] + [p], :]
    undo_flip = np.diag(list(ornt[:, 1]) + [1.0])
    center_trans = -(shape - 1) / 2.0
    undo_flip[:p, p] = (ornt[:, 1] * center_trans) - center_trans
    return undo_flip @ undo_reorder


def zoom_affine(affine, pixdim, diagonal=False):
    """monai zoom_affine: keep the direction cosines of `affine` (Cholesky of RZS^T RZS) and rescale its columns to `pixdim`"""
    affine = np.array(affine, dtype=np.float64, copy=True)
    d = len(affine) - 1
    scale = np.array(pixdim, dtype=np.float64, copy=True)
    if len(scale) < d:
        norm = np.sqrt(np.sum(np.square(affine), 0))[:-1]
        scale = np.append(scale, norm[len(scale):])
    scale = scale[:d]
    scale[scale == 0] = 1.0
    if diagonal:
        return np.diag(np.append(scale, [1.0]))
    rzs = affine[:-1, :-1]
    zs = np.linalg.cholesky(rzs.T @ rzs).T
    rotation = rzs @ np.linalg.inv(zs)
    s = np.sign(np.diag(zs)) * np.abs(scale)
    new_affine = np.eye(len(affine))
    new_affine[:-1, :-1] = rotation @ np.diag(s)
    return new_affine


def compute_shape_offset(spatial_shape, in_affine, out_affine):
    """monai compute_shape_offset: output shape = round(ptp of the transformed input corners + 1) (numpy rounds half to even);
    offset = the input origin when the orientations agree, else the minimum corner"""
    shape = np.array(spatial_shape, dtype=np.float64)
    sr = len(shape)
    in_coords = [(0.0, dim - 1.0) for dim in shape]
    corners = np.asarray(np.meshgrid(*in_coords, indexing='ij')).reshape((sr, -1))
    corners = np.concatenate((corners, np.ones_like(corners[:1])))
    corners = in_affine @ corners
    corners_out = np.linalg.inv(out_affine) @ corners
    corners_out = corners_out[:-1] / corners_out[-1]
    out_shape = np.round(np.ptp(corners_out, axis=1) + 1.0)
    if np.allclose(io_orientation(in_affine), io_orientation(out_affine)):
        offset = in_affine @ ([0] * sr + [1])
        offset = offset[:-1] / offset[-1]
    else:
        corners = corners[:-1] / corners[-1]
        offset = np.min(corners, 1)
    return out_shape.astype(int), offset


def spacing_plan(shape, affine, pixdim=(0.5, 0.5, 2.0), axcodes='RAS'):
    """Spacingd(pixdim, diagonal=False) then Orientationd(axcodes) of a volume of `shape` (x, y, z) with `affine`:
    (pull matrix 3x4 float64: output voxel -> source voxel, output shape, output affine 4x4).
    monai skips the resampling when the spacing transform is the identity within 1e-3; the matrix is then exactly the identity
    before the re-orientation, so the kernel copies voxels as monai does."""
    affine = np.asarray(affine, dtype=np.float64)
    new_affine = zoom_affine(affine, pixdim, diagonal=False)
    out_shape, offset = compute_shape_offset(shape, affine, new_affine)
    new_affine[:3, 3] = offset[:3]
    transform = np.linalg.inv(affine) @ new_affine
    if np.allclose(transform, np.eye(4), atol=1e-3):
        transform, out_shape = np.eye(4), np.asarray(shape, dtype=int)
    src = io_orientation(new_affine)
    ornt = ornt_transform(src, axcodes2ornt(axcodes))
    undo = inv_ornt_aff(ornt, out_shape)
    final_shape = [0, 0, 0]
    for i in range(3):
        final_shape[int(ornt[i, 0])] = int(out_shape[i])
    return (transform @ undo)[:3], tuple(final_shape), new_affine @ undo


def crop_plan(shape, affine, box):
    """the grid of a crop of a volume of `shape` (x, y, z) with `affine`: box = one (lo, hi exclusive) pair per axis of `shape`.
    Returns (box shape, affine') with affine' = affine . T(box lo) in float64: voxel i of the crop is voxel lo + i of the volume,
    so both affines put it at the same place.  The full box returns the shape and the affine as they are.  ValueError for a box
    that is empty or not inside the volume."""
    affine = np.asarray(affine, dtype=np.float64)
    shape = tuple(int(n) for n in shape)
    pairs = [tuple(int(v) for v in p) for p in box]
    if len(pairs) != len(shape) or any(len(p) != 2 for p in pairs):
        raise ValueError(f'a box holds one (lo, hi) pair per axis of {shape}, got {box!r}')
    if any(not 0 <= lo < hi <= n for (lo, hi), n in zip(pairs, shape)):
        raise ValueError(f'box {pairs} is empty or not inside a volume of shape {shape}')
    shift = np.eye(len(shape) + 1)
    shift[:-1, -1] = [lo for lo, _ in pairs]
    return tuple(hi - lo for lo, hi in pairs), affine @ shift


def voxel_spacing(affine):
    """the voxel sizes of a 4x4 affine per file axis: its column norms"""
    return tuple(float(v) for v in np.sqrt(np.sum(np.square(np.asarray(affine, dtype=np.float64)[:3, :3]), axis=0)))


def resample_orders(spacing, new_spacing, threshold=3.0):
    """nnU-Net's interpolation orders for an image, per file axis (restated from its resample_data_or_seg_to_shape /
    get_do_separate_z / get_lowres_axis; nnU-Net is no dependency, so parity with it is unpinned): cubic (3) on every axis, unless
    the scan is anisotropic - max / min of `spacing` (the file's voxel sizes) above `threshold` with exactly one axis holding the
    maximum, which then gets 0 (nearest across slices); failing that, the same test on `new_spacing` (the target's)."""
    for sp in (spacing, new_spacing):
        sp = np.asarray(sp, dtype=np.float64).reshape(3)
        if not np.all(np.isfinite(sp)) or np.any(sp <= 0):
            raise ValueError(f'spacings are positive and finite, got {tuple(sp)}')
        if sp.max() / sp.min() > threshold and np.count_nonzero(sp == sp.max()) == 1:
            return tuple(0 if a == int(np.argmax(sp)) else 3 for a in range(3))
    return (3, 3, 3)


def check_pair(img_shape, img_affine, lab_shape, lab_affine, atol=1e-3):
    """an image / label pair is sampled through one matrix: shapes equal and affines within `atol`"""
    if tuple(img_shape) != tuple(lab_shape):
        raise ValueError(f'image {tuple(img_shape)} and label {tuple(lab_shape)} shapes differ')
    diff = np.abs(np.asarray(img_affine, dtype=np.float64) - np.asarray(lab_affine, dtype=np.float64)).max()
    if diff > atol:
        raise ValueError(f'image and label affines differ by {diff:.3g} (> {atol})')


def invert(matrix):
    """inverse of a 3x4 pull matrix (the push direction: source voxel -> output voxel), as 3x4"""
    m = np.eye(4)
    m[:3] = matrix
    return np.linalg.inv(m)[:3]


def lane_axis(matrix, src_strides):
    """the output axis whose unit step moves the source address least (sum over source axes of |M[s][a]| * stride_s)"""
    m = np.abs(np.asarray(matrix, dtype=np.float64)[:, :3])
    cost = (m * np.asarray(src_strides, dtype=np.float64)[:, None]).sum(0)
    return int(np.argmin(cost))
