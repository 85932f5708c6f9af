"""Time of the label vote ("one-hot, order 1": ltu_resample_vote, ltu_sample_vote) beside the nearest label it replaces and beside
the loop a user had to write before it (float32 one-hot volumes + data.resample_argmax).  Every group alternates its callables in
one process, each call between two device events (host work included), after three warm-up rounds; medians with min - max of the
repeats:
  resample_c*   a 512x512x100 u8 label with 3 and with 8 values -> 819x819x125 (the MSD example's Spacingd + Orientationd matrix):
                nearest (ltu_resample_grid, label only), by vote (ltu_resample_vote), and the one-hot loop (C float32 volumes built
                with torch, then ltu_resample_argmax), whose label the vote must equal byte for byte (asserted here at this size);
  gather_*      12 patches of 512x512x32 from an 819x819x125 scan on fixed matrices - 0.5 rad about D at zoom 1.2 (the z-decoupled
                kernel), oblique (0.2, -0.3, 0.5) at zoom 1.2 (the general kernel), and the oblique matrices with a (6, 6, 4) lattice
                (the elastic kernel) - label only at label_order 0 and 1 (one launch each: kernel against kernel), and image + label
                at both (label_order 1 is the image's launch plus the label-only launch: the difference is the second launch's cost);
  sample_*      data.sample end to end with rotation and zoom firing on every patch, label_order 0 and 1.
bytes_per_voxel: what the algorithm moves per output voxel - nearest 1 tap + 1 store, the vote 8 byte taps + 1 store, the one-hot
loop C x 8 taps of 4 bytes + 1 store for the gather alone (its one-hot build writes another 4 C bytes per SOURCE voxel).  The taps of
neighbouring voxels overlap, so the caches see far fewer distinct bytes than that: the figures say how the three calls scale, not
what they reach.  One JSON line.
usage: bench_label_vote.py [repeats]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import data, geometry  # noqa: E402

reps = max(20, int(sys.argv[1]) if len(sys.argv) > 1 else 20)
dev = torch.device('cuda')


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


def ratio(ts, a, b):
    return round(statistics.median(ts[a]) / statistics.median(ts[b]), 2)


res = {'repeats': reps}

# ---- the scan resampler -----------------------------------------------------------------------------------------------------------
X, Y, Z = 512, 512, 100
aff = np.diag([-0.8, -0.8, 2.5, 1.0])
aff[:3, 3] = (200.0, 150.0, -300.0)
M, shape, _ = geometry.spacing_plan((X, Y, Z), aff, (0.5, 0.5, 2.0))
assert shape == (819, 819, 125), shape
res.update(source=[X, Y, Z], ras=list(shape))
zz, yy, xx = torch.meshgrid(*(torch.arange(n, device=dev, dtype=torch.float32) for n in (Z, Y, X)), indexing='ij')
field = torch.sin(xx / 37.0) + torch.sin(yy / 29.0 + 1.0) + torch.sin(zz / 11.0 + 2.0) + 0.5 * torch.sin((xx + yy) / 13.0)
del zz, yy, xx
lo_f, hi_f = float(field.min()), float(field.max())
for C in (3, 8):
    lab = ((field - lo_f) / (hi_f - lo_f) * C).floor().clamp_(0, C - 1).to(torch.uint8).contiguous()
    assert len(torch.unique(lab)) == C

    def loop(lab=lab, C=C):
        onehot = torch.stack([(lab == c).to(torch.float32) for c in range(C)])
        return data.resample_argmax(onehot, M, shape)[0]

    def vote(lab=lab):
        return data.resample(None, lab, M, shape, label_order=1)[1]
    assert torch.equal(vote(), loop())
    ts = alternate({'nearest': lambda lab=lab: data.resample(None, lab, M, shape), 'vote': vote, 'onehot_loop': loop})
    for k in ts:
        res[f'resample_c{C}_{k}_us'] = spread(ts[k])
    res[f'resample_c{C}_vote_over_nearest'] = ratio(ts, 'vote', 'nearest')
    res[f'resample_c{C}_loop_over_vote'] = ratio(ts, 'onehot_loop', 'vote')
    res[f'resample_c{C}_bytes_per_voxel'] = {'nearest': 2, 'vote': 9, 'onehot_loop': 32 * C + 1}
    res[f'resample_c{C}_onehot_temporaries_mb'] = round(C * 4 * X * Y * Z / 1e6, 1)
    del lab
del field
torch.cuda.empty_cache()

# ---- the augmentation gather ------------------------------------------------------------------------------------------------------
SHAPE, SIZE, N, SPACING = (819, 819, 125), (512, 512, 32), 12, (0.5, 0.5, 2.0)


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
scan.pixdim, scan.intensity, scan.outside, scan.label_order = SPACING, (-2.0, 2.0, -2.0, 2.0), None, 0
res.update(scan=list(SHAPE), patch=list(SIZE), patches=N)

starts = [(150 + 7 * n, 160 - 5 * n, 40 + n) for n in range(N)]


def mats(angles, zoom):
    return np.stack([data.patch_matrix(st, SIZE, bool(n % 2), n % 4, angles, zoom, SPACING) for n, st in enumerate(starts)])


grid = (6, 6, 4)
cell = np.array([(SIZE[a] - 1) / (grid[a] - 3) for a in range(3)]).reshape(1, 3, 1, 1, 1)
phi = torch.from_numpy((np.random.RandomState(3).uniform(-1, 1, (N, 3, *grid)) * 0.1 * cell).astype(np.float32)).to(dev)
cases = {'inplane': (mats((0.0, 0.0, 0.5), 1.2), None), 'oblique': (mats((0.2, -0.3, 0.5), 1.2), None),
         'deformed': (mats((0.2, -0.3, 0.5), 1.2), phi)}
fns = {}
for cname, (m, lat) in cases.items():
    for lo in (0, 1):
        fns[f'gather_{cname}_label_only_lo{lo}'] = lambda m=m, lat=lat, lo=lo: data.sample_affine(None, scan.lab, m, SIZE, elastic=lat, label_order=lo)
        fns[f'gather_{cname}_image_label_lo{lo}'] = lambda m=m, lat=lat, lo=lo: data.sample_affine(scan.img, scan.lab, m, SIZE, -2.3, elastic=lat,
                                                                                                     label_order=lo)
ts = alternate(fns)
for k in ts:
    res[k + '_us'] = spread(ts[k])
for cname in cases:
    res[f'gather_{cname}_label_only_lo1_over_lo0'] = ratio(ts, f'gather_{cname}_label_only_lo1', f'gather_{cname}_label_only_lo0')
    res[f'gather_{cname}_second_launch_us'] = round(statistics.median(ts[f'gather_{cname}_image_label_lo1']) -
                                                    statistics.median(ts[f'gather_{cname}_image_label_lo0']), 1)
res['gather_bytes_per_voxel'] = {'nearest': 2, 'vote': 9}

# ---- data.sample end to end -------------------------------------------------------------------------------------------------------
off = dict(noise_prob=0.0, blur_prob=0.0, brightness_prob=0.0, gamma_prob=0.0)
fns = {}
for lo in (0, 1):
    aug = data.Augmentation(rot_prob=1.0, zoom_prob=1.0, label_order=lo, **off)
    rs = np.random.RandomState(1)
    fns[f'sample_lo{lo}'] = lambda aug=aug, rs=rs: data.sample(scan, SIZE, rs, num_samples=N, augment=aug)
ts = alternate(fns)
for k in ts:
    res[k + '_us'] = spread(ts[k])
res['sample_lo1_over_lo0'] = ratio(ts, 'sample_lo1', 'sample_lo0')
print(json.dumps(res))
