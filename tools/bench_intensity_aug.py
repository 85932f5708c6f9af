"""Time of the contrast, gamma and low-resolution augmentations (csrc/intensity_aug.hip) beside the eager-torch composition a user
would otherwise write from the same formulas (mean / amin / amax, clamp, pow, two F.interpolate calls per patch), on the two batches
the drivers use: 2 patches of 128^3 and 12 patches of 512x512x32.  Every group alternates its callables in one process, each call
between two device events (host work included), after three warm-up rounds; medians with min - max of the repeats:
  stats / contrast / gamma / invgamma_retain / lowres   the stage alone, `hip` against `torch`, and torch / hip;
  lowres_tables_ready   the gather alone on tables built and uploaded beforehand (lowres builds them on the host in the call);
  sample_*   data.sample on a synthetic scan (320x320x160 for the 128^3 patches, 819x819x125 for the others) with
             Augmentation.nnunet() (its own probabilities), with the three new stages switched off and retain_stats=False (the
             call as it was), and with the four intensity stages firing on every patch.
One JSON line.
usage: bench_intensity_aug.py [repeats]"""
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import data  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device('cuda')
BATCHES = {'2x128^3': (2, (128, 128, 128)), '12x512x512x32': (12, (512, 512, 32))}
DIMS = (1, 2, 3, 4)


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


def col(values):
    return torch.tensor(values, dtype=torch.float32, device=dev).view(-1, 1, 1, 1, 1)


def torch_stats(x):
    return x.amin(DIMS), x.amax(DIMS), x.sum(DIMS, dtype=torch.float64), (x.double() ** 2).sum(DIMS)


def torch_contrast(x, f):
    m, lo, hi = x.mean(DIMS, keepdim=True), x.amin(DIMS, keepdim=True), x.amax(DIMS, keepdim=True)
    return torch.minimum(torch.maximum((x - m) * col(f) + m, lo), hi)


def torch_gamma(x, g, invert, retain):
    u = -x if invert else x
    lo = u.amin(DIMS, keepdim=True)
    r = u.amax(DIMS, keepdim=True) - lo
    v = ((u - lo) / r.clamp_min(1e-7)).pow(col(g)) * r + lo
    if retain:
        sv, mv = torch.std_mean(v, DIMS, unbiased=False, keepdim=True)
        su, mu = torch.std_mean(u, DIMS, unbiased=False, keepdim=True)
        v = (v - mv) * (su / sv.clamp_min(1e-7)) + mu
    return -v if invert else v


def torch_lowres(x, scales):
    size = tuple(x.shape[-3:])
    out = torch.empty_like(x)
    for k, s in enumerate(scales):                 # the low size differs per patch: one pair of calls each
        low = tuple(max(int(round(S * s)), 1) for S in size)
        out[k:k + 1] = F.interpolate(F.interpolate(x[k:k + 1], size=low, mode='nearest-exact'), size=size, mode='trilinear')
    return out


res = {'repeats': reps}
for bname, (n, size) in BATCHES.items():
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((n, 1, *size), device=dev, generator=g)
    rs = np.random.RandomState(2)
    f, gm, sc = rs.uniform(0.75, 1.25, n), rs.uniform(0.7, 1.5, n), rs.uniform(0.5, 1.0, n)
    tabs = data.lowres_device_tables(size, sc, device=dev)
    pairs = {
        'stats': (lambda: data.patch_stats(x), lambda: torch_stats(x)),
        'contrast': (lambda: data.contrast(x, f), lambda: torch_contrast(x, f)),
        'gamma': (lambda: data.gamma_transform(x, gm, False, False), lambda: torch_gamma(x, gm, False, False)),
        'invgamma_retain': (lambda: data.gamma_transform(x, gm, True, True), lambda: torch_gamma(x, gm, True, True)),
        'lowres': (lambda: data.simulate_lowres(x, sc), lambda: torch_lowres(x, sc)),
        'lowres_tables_ready': (lambda: data.simulate_lowres(x, None, tables=tabs), lambda: torch_lowres(x, sc)),
    }
    out = {}
    for stage, (hip, ref) in pairs.items():
        ts = alternate({'hip': hip, 'torch': ref})
        out[stage] = {'hip_us': spread(ts['hip']), 'torch_us': spread(ts['torch']),
                      'torch_over_hip': round(statistics.median(ts['torch']) / statistics.median(ts['hip']), 2)}
    res[bname] = out
    del x


class _Scan(data.SpacedScan):
    def __init__(self):                  # a synthetic scan: no file behind it
        pass


def make_scan(shape):
    scan = _Scan()
    scan.img = torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).clamp_(-2.0, 2.0)
    hh, ww, dd = torch.meshgrid(*(torch.arange(n, device=dev, dtype=torch.float32) for n in shape), indexing='ij')
    r = ((hh - shape[0] / 2) / (shape[0] / 9)) ** 2 + ((ww - shape[1] / 2) / (shape[1] / 13)) ** 2 + ((dd - shape[2] / 2) / (shape[2] / 5)) ** 2
    scan.lab = ((r <= 1).to(torch.uint8) + (r <= 0.2).to(torch.uint8)).contiguous()
    scan._label_host, scan._crop_index = None, data.CropIndex(scan.lab)
    scan.pixdim, scan.intensity, scan.outside = (0.5, 0.5, 2.0), (-2.0, 2.0, -2.0, 2.0), None
    scan.spline_coefficients(3)
    return scan


SCANS = {'2x128^3': (320, 320, 160), '12x512x512x32': (819, 819, 125)}
augs = {'nnunet': data.Augmentation.nnunet(),
        'nnunet_without_new_stages': data.Augmentation.nnunet(contrast_prob=0.0, lowres_prob=0.0, invgamma_prob=0.0, retain_stats=False),
        'nnunet_intensity_always': data.Augmentation.nnunet(contrast_prob=1.0, lowres_prob=1.0, invgamma_prob=1.0, gamma_prob=1.0)}
for bname, (n, size) in BATCHES.items():
    scan = make_scan(SCANS[bname])
    fns = {}
    for aname, aug in augs.items():
        rs = np.random.RandomState(1)
        fns[aname] = lambda aug=aug, rs=rs: data.sample(scan, size, rs, num_samples=n, augment=aug)
    ts = alternate(fns)
    res[bname].update({'sample_' + k + '_us': spread(v) for k, v in ts.items()})
print(json.dumps(res))
