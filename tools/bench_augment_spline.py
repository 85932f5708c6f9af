"""Time of the cubic patch gather (ltu_sample_spline) beside the trilinear one, in bench_augment.py's setting: a synthetic scan of
819x819x125 (the MSD example at 0.5 x 0.5 x 2.0 mm) and the driver's batch of 12 patches of 512x512x32.  Every group alternates its
callables in one process, each call between two device events (host work included), after three warm-up rounds; medians with
min - max of the repeats:
  sample_*   data.sample with rotation and zoom firing on every patch at order 1, (3, 3, 1) and 3: rotation about D (the default:
             the z-decoupled matrices), oblique angles (the general kernel), and the oblique call with the deformation on top;
  gather_*   the gather alone on fixed matrices (0.5 rad about D at zoom 1.2; oblique (0.2, -0.3, 0.5) at zoom 1.2), K = 1 and K = 4
             channels: ltu_sample_channels (K = 1: ltu_sample_affine) against ltu_sample_spline at (3, 3, 1) and 3 on cached
             coefficients, with the ratio to the trilinear call of the same run.  The tap count alone predicts 4x at 32 taps and
             8x at 64;
  coef_*     the one-off coefficient build of the scan (data.spline_coefficients), per order.
One JSON line.
usage: bench_augment_spline.py [repeats]"""
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
ORDERS = {'o1': 1, 'o331': (3, 3, 1), 'o333': 3}


class _Scan(data.SpacedScan):
    def __init__(self):                  # a synthetic scan: no file behind it
        pass


scan = _Scan()
g = torch.Generator(device=dev).manual_seed(0)
scan.img = torch.randn(SHAPE, device=dev, generator=g).clamp_(-2.0, 2.0)
hh, ww, dd = torch.meshgrid(*(torch.arange(n, device=dev, dtype=torch.float32) for n in SHAPE), indexing='ij')
r = ((hh - 400) / 90) ** 2 + ((ww - 430) / 60) ** 2 + ((dd - 60) / 25) ** 2
scan.lab = ((r <= 1).to(torch.uint8) + (r <= 0.2).to(torch.uint8)).contiguous()
del hh, ww, dd, r
scan._label_host, scan._crop_index = None, data.CropIndex(scan.lab)
scan.pixdim, scan.intensity, scan.outside = SPACING, (-2.0, 2.0, -2.0, 2.0), None


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


res = {'scan': list(SHAPE), 'patch': list(SIZE), 'patches': N, 'repeats': reps}

# the one-off coefficient build, first: the calls below read the cached volumes
fns = {}
for name, order in ORDERS.items():
    if order != 1:
        def build(order=order):
            scan.drop_coefficients()
            scan.spline_coefficients(order)
        fns['coef_' + name + '_us'] = build
res.update({k: spread(v) for k, v in alternate(fns).items()})
for order in ORDERS.values():
    if order != 1:
        scan.spline_coefficients(order)

settings = {'inplane': dict(), 'oblique': dict(rot_range=(0.3, 0.3, np.pi)), 'oblique_elastic': dict(rot_range=(0.3, 0.3, np.pi), elastic_prob=1.0)}
fns = {}
for sname, kw in settings.items():
    for oname, order in ORDERS.items():
        aug = only(rot_prob=1.0, zoom_prob=1.0, order=order, **kw)
        rs = np.random.RandomState(1)
        fns[f'sample_{sname}_{oname}'] = lambda aug=aug, rs=rs: data.sample(scan, SIZE, rs, num_samples=N, augment=aug)
ts = alternate(fns)
for sname in settings:
    for oname in ORDERS:
        k = f'sample_{sname}_{oname}'
        res[k + '_us'] = spread(ts[k])
        if oname != 'o1':
            res[k + '_over_o1'] = round(statistics.median(ts[k]) / statistics.median(ts[f'sample_{sname}_o1']), 2)

starts = [(150 + 7 * n, 160 - 5 * n, 40 + n) for n in range(N)]


def mats(angles, zoom):
    return np.stack([data.patch_matrix(st, SIZE, bool(n % 2), n % 4, angles, zoom, SPACING) for n, st in enumerate(starts)])


cases = {'inplane': mats((0.0, 0.0, 0.5), 1.2), 'oblique': mats((0.2, -0.3, 0.5), 1.2)}
for K in (1, 4):
    img = scan.img if K == 1 else torch.stack([scan.img] * K)
    coefs = {name: (scan.spline_coefficients(order) if K == 1 else torch.stack([scan.spline_coefficients(order)] * K))
             for name, order in ORDERS.items() if order != 1}
    fns = {}
    for cname, m in cases.items():
        for oname, order in ORDERS.items():
            kw = dict(order=order, coef=coefs[oname], clamp=(-2.0, 2.0)) if order != 1 else {}
            fns[f'gather_k{K}_{cname}_{oname}'] = lambda m=m, kw=kw: data.sample_affine(img, scan.lab, m, SIZE, -2.3, **kw)
    ts = alternate(fns)
    for cname in cases:
        for oname in ORDERS:
            k = f'gather_k{K}_{cname}_{oname}'
            res[k + '_us'] = spread(ts[k])
            if oname != 'o1':
                res[k + '_over_o1'] = round(statistics.median(ts[k]) / statistics.median(ts[f'gather_k{K}_{cname}_o1']), 2)
    del img, coefs
print(json.dumps(res))
