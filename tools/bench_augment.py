"""Time of the augmented patch sampler on a synthetic scan of 819x819x125 (the MSD example at 0.5 x 0.5 x 2.0 mm) and the driver's
batch of 12 patches of 512x512x32.  Four ways to get the batch alternate in one process, each call between two device events
(host draws, the crop-centre select and its read-back included), after a warm-up; medians with min - max of the repeats:
  (a) data.sample plain (crop + flip + rot90: ltu_crop_orient);
  (b) data.sample with rotation (about D, the default) and zoom firing on every patch: ltu_sample_affine, z-decoupled;
  (c) the same with oblique angles: the general instantiation;
  (d) crop_orient followed by data.rotate + data.zoom on image and label: what a user had to do before, on cut patches.
Then the kernels alone on fixed matrices (identity; 0.5 rad about D at zoom 1.2; the same matrices pushed through the general
instantiation by a 1e-9 rad tilt; oblique (0.2, -0.3, 0.5) at zoom 1.2; the in-plane case with noise), and ltu_gauss_blur3 on the 12
patches at sigma 1.0 and 2.0, and the deformed gather (ltu_sample_elastic, lattice (6, 6, 4) of +-11.2 voxels in plane and +-2.8 along D, given as a host array
as data.sample gives it: checked and uploaded in the call) beside ltu_sample_affine's general instantiation on the same matrices, in
plane and oblique, with their ratio; a zero lattice on the device shows the kernel without the upload and with the undeformed
access pattern.  (e) is data.sample with the deformation firing on every patch beside rotation and zoom.  Algorithmic bytes of a gather: 5 per patch voxel written + 5 per source voxel touched (patch voxels
/ zoom^3); of a blur: 8 per voxel.  One JSON line.
usage: bench_augment.py [repeats]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import data  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device('cuda')
SHAPE, SIZE, N, SPACING = (819, 819, 125), (512, 512, 32), 12, (0.5, 0.5, 2.0)


class _Scan:
    pass


scan = _Scan()
g = torch.Generator(device=dev).manual_seed(0)
scan.img = torch.randn(SHAPE, device=dev, generator=g)
hh, ww, dd = torch.meshgrid(*(torch.arange(n, device=dev, dtype=torch.float32) for n in SHAPE), indexing='ij')
r = ((hh - 400) / 90) ** 2 + ((ww - 430) / 60) ** 2 + ((dd - 60) / 25) ** 2
scan.lab = ((r <= 1).to(torch.uint8) + (r <= 0.2).to(torch.uint8)).contiguous()
del hh, ww, dd, r
scan.crop_index = data.CropIndex(scan.lab)
scan.pixdim, scan.intensity = SPACING, data.MONAI_CT_WINDOW


def spread(ts):
    return {'median': round(statistics.median(ts), 1), 'min': round(min(ts), 1), 'max': round(max(ts), 1)}


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def alternate(fns):
    """{name: [us]} of `reps` rounds in which the callables take turns, after three warm-up rounds"""
    ts = {k: [] for k in fns}
    for rnd in range(-3, reps):
        for k, fn in fns.items():
            t = event_us(fn)
            if rnd >= 0:
                ts[k].append(t)
    return ts


def only(**kw):
    off = dict(rot_prob=0.0, zoom_prob=0.0, noise_prob=0.0, blur_prob=0.0, brightness_prob=0.0, gamma_prob=0.0)
    off.update(kw)
    return data.Augmentation(**off)


inplane = only(rot_prob=1.0, zoom_prob=1.0)
oblique = only(rot_prob=1.0, zoom_prob=1.0, rot_range=(0.3, 0.3, np.pi))
elastic = only(rot_prob=1.0, zoom_prob=1.0, elastic_prob=1.0)
rs = {k: np.random.RandomState(1) for k in 'abcde'}


def old_way():
    draws, _ = data.sample_draws(scan, SIZE, rs['d'], N)
    img, lab = data.crop_orient(scan.img, scan.lab, draws, SIZE)
    mats = np.stack([data.rotate_matrix((0.0, 0.0, 0.5), SIZE)] * N)
    zf = [1.2] * N
    lf = lab.to(torch.float32)
    return data.zoom(data.rotate(img, mats), zf), data.zoom(data.rotate(lf, mats), zf).to(torch.uint8)


res = {'scan': list(SHAPE), 'patch': list(SIZE), 'patches': N, 'repeats': reps}
ts = alternate({
    'a_sample_plain_us': lambda: data.sample(scan, SIZE, rs['a'], num_samples=N),
    'b_sample_inplane_us': lambda: data.sample(scan, SIZE, rs['b'], num_samples=N, augment=inplane),
    'c_sample_oblique_us': lambda: data.sample(scan, SIZE, rs['c'], num_samples=N, augment=oblique),
    'd_crop_rotate_zoom_us': old_way,
    'e_sample_elastic_us': lambda: data.sample(scan, SIZE, rs['e'], num_samples=N, augment=elastic),
})
res.update({k: spread(v) for k, v in ts.items()})

starts = [(150 + 7 * n, 160 - 5 * n, 40 + n) for n in range(N)]
vox = N * int(np.prod(SIZE))


def mats(angles, zoom):
    return np.stack([data.patch_matrix(st, SIZE, bool(n % 2), n % 4, angles, zoom, SPACING) for n, st in enumerate(starts)])


kern = {
    'identity': (mats((0.0, 0.0, 0.0), 1.0), 1.0, None),
    'inplane_zdec': (mats((0.0, 0.0, 0.5), 1.2), 1.2, None),
    'inplane_general': (mats((1e-9, 0.0, 0.5), 1.2), 1.2, None),
    'oblique': (mats((0.2, -0.3, 0.5), 1.2), 1.2, None),
    'inplane_zdec_noise': (mats((0.0, 0.0, 0.5), 1.2), 1.2, [0.1] * N),
}
seeds = list(range(1, N + 1))
ts = alternate({k: (lambda m=m, sg=sg: data.sample_affine(scan.img, scan.lab, m, SIZE, -2.3, sg, seeds if sg else None))
                for k, (m, _, sg) in kern.items()})
for k, (_, zoom, _) in kern.items():
    nbytes = 5 * vox * (1 + 1 / zoom ** 3)
    res['affine_' + k] = dict(spread(ts[k]), gb=round(nbytes / 1e9, 3), tbps=round(nbytes / statistics.median(ts[k]) / 1e6, 2))

GRID = (6, 6, 4)
amp = np.array([4.0 * 1.4 / sp for sp in SPACING]).reshape(1, 3, 1, 1, 1)      # Augmentation's largest: 4 mm at zoom 1.4, in voxels
phi = (np.random.RandomState(11).uniform(-1, 1, (N, 3, *GRID)) * amp).astype(np.float32)
zero = torch.zeros((N, 3, *GRID), device=dev)
pairs = {'inplane': kern['inplane_general'][0], 'oblique': kern['oblique'][0]}
fns = {}
for k, m in pairs.items():
    fns['elastic_' + k] = lambda m=m: data.sample_affine(scan.img, scan.lab, m, SIZE, -2.3, elastic=phi)
    fns['elastic_zero_' + k] = lambda m=m: data.sample_affine(scan.img, scan.lab, m, SIZE, -2.3, elastic=zero)
    fns['general_' + k] = lambda m=m: data.sample_affine(scan.img, scan.lab, m, SIZE, -2.3)
ts = alternate(fns)
for k in pairs:
    for name in ('elastic_', 'elastic_zero_', 'general_'):
        res[name + k + '_us'] = spread(ts[name + k])
    res['elastic_over_general_' + k] = round(statistics.median(ts['elastic_' + k]) / statistics.median(ts['general_' + k]), 3)
    res['elastic_zero_over_general_' + k] = round(statistics.median(ts['elastic_zero_' + k]) / statistics.median(ts['general_' + k]), 3)

patches, _ = data.sample_affine(scan.img, None, kern['identity'][0], SIZE)
ts = alternate({'blur_sigma1_us': lambda: data.gaussian_blur(patches, [1.0] * N, [1.1] * N),
                'blur_sigma2_us': lambda: data.gaussian_blur(patches, [2.0] * N, [1.1] * N),
                'blur_inplane_sigma1_us': lambda: data.gaussian_blur(patches, [(1.0, 1.0, 0.0)] * N)})
for k, v in ts.items():
    res[k] = dict(spread(v), gb=round(8 * vox / 1e9, 3), tbps=round(8 * vox / statistics.median(v) / 1e6, 2))
print(json.dumps(res))
