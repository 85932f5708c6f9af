"""Cost of more than one input channel, on one MI355X.  One JSON line.

(a) The gather.  A synthetic 4-channel scan of 240x240x155 at 1 mm (the BraTS grid) and 2 patches of 128^3 on fixed matrices:
plain (patch_matrix's integer matrices), rotation about D + zoom (the z-decoupled instantiation), oblique rotation + zoom (the
general one), and the oblique case with a (6, 6, 4) B-spline lattice on top.  Per row two ways alternate in one process, each
call between two device events after a warm-up, medians with min - max of the repeats:
  one   data.sample_affine(img [K, H, W, D], lab, ...): ltu_sample_channels, coordinates, taps and label once for all channels;
  loop  what a user could write before: K x data.sample_affine(img[c], ...) (the label with the first only) + torch.cat.
The K = 1 row of every case is the single-channel entry point on img[0] (the path existing callers take), and `sample_*` are
data.sample end to end on the 4-channel scan (host draws and the crop-centre select included).
(b) The step.  train.GraphedStep at 2 x 128^3, bf16, the full configuration with dropout 0.3, dim_input 1 against 4: medians of
alternated replays and their difference (the stem conv reads 16 instead of 8 channels on the 64 x 64 x 128 grid, and so does its
weight gradient).
usage: bench_multichannel.py [repeats] [gather|step]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import data, train  # noqa: E402
from lintransunet_amd.model import get_model_dict  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
what = sys.argv[2] if len(sys.argv) > 2 else 'all'
dev = torch.device('cuda')
SHAPE, SIZE, N, K, SPACING = (240, 240, 155), (128, 128, 128), 2, 4, (1.0, 1.0, 1.0)


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


res = {'scan': list(SHAPE), 'patch': list(SIZE), 'patches': N, 'channels': K, 'repeats': reps}

if what in ('all', 'gather'):
    class _Scan:
        pass

    scan = _Scan()
    g = torch.Generator(device=dev).manual_seed(0)
    scan.img = torch.randn((K,) + SHAPE, device=dev, generator=g)
    hh, ww, dd = torch.meshgrid(*(torch.arange(n, device=dev, dtype=torch.float32) for n in SHAPE), indexing='ij')
    r = ((hh - 120) / 50) ** 2 + ((ww - 130) / 40) ** 2 + ((dd - 80) / 30) ** 2
    scan.lab = ((r <= 1).to(torch.uint8) + (r <= 0.2).to(torch.uint8)).contiguous()
    del hh, ww, dd, r
    scan.crop_index = data.CropIndex(scan.lab)
    scan.pixdim, scan.intensity = SPACING, [None] * K
    fills = [-1.0, -0.5, 0.0, 0.5]
    starts = [(40, 50, 10), (70, 30, 20)]

    def mats(angles, zoom):
        return np.stack([data.patch_matrix(st, SIZE, bool(n % 2), 2 * n, angles, zoom, SPACING) for n, st in enumerate(starts)])

    phi = (np.random.RandomState(11).uniform(-1, 1, (N, 3, 6, 6, 4)) * 4.0).astype(np.float32)
    cases = {'plain': (mats((0.0, 0.0, 0.0), 1.0), None), 'inplane': (mats((0.0, 0.0, 0.5), 1.2), None),
             'oblique': (mats((0.2, -0.3, 0.5), 1.2), None), 'elastic': (mats((0.2, -0.3, 0.5), 1.2), phi)}

    def loop(m, lat, k):
        parts = [data.sample_affine(scan.img[c], scan.lab if c == 0 else None, m, SIZE, fills[c], elastic=lat) for c in range(k)]
        return torch.cat([p[0] for p in parts], 1), parts[0][1]

    fns = {}
    for name, (m, lat) in cases.items():
        for k in (2, 4):
            sub = scan.img[:k]
            fns[f'{name}_one_k{k}'] = lambda m=m, lat=lat, sub=sub, k=k: data.sample_affine(sub, scan.lab, m, SIZE, fills[:k], elastic=lat)
            fns[f'{name}_loop_k{k}'] = lambda m=m, lat=lat, k=k: loop(m, lat, k)
        fns[f'{name}_k1'] = lambda m=m, lat=lat: data.sample_affine(scan.img[0], scan.lab, m, SIZE, fills[0], elastic=lat)
    ts = alternate(fns)
    for name in cases:
        row = {'k1_us': spread(ts[f'{name}_k1'])}
        for k in (2, 4):
            one, lp = ts[f'{name}_one_k{k}'], ts[f'{name}_loop_k{k}']
            row[f'one_k{k}_us'], row[f'loop_k{k}_us'] = spread(one), spread(lp)
            row[f'one_over_loop_k{k}'] = round(statistics.median(one) / statistics.median(lp), 3)
        res['gather_' + name] = row

    def only(**kw):
        off = dict(rot_prob=0.0, zoom_prob=0.0, noise_prob=0.0, blur_prob=0.0, brightness_prob=0.0, gamma_prob=0.0)
        off.update(kw)
        return data.Augmentation(**off)

    rs = {k: np.random.RandomState(1) for k in 'abc'}
    ts = alternate({'sample_plain_us': lambda: data.sample(scan, SIZE, rs['a'], num_samples=N),
                    'sample_rot_zoom_us': lambda: data.sample(scan, SIZE, rs['b'], num_samples=N, augment=only(rot_prob=1.0, zoom_prob=1.0)),
                    'sample_elastic_us': lambda: data.sample(scan, SIZE, rs['c'], num_samples=N,
                                                             augment=only(rot_prob=1.0, zoom_prob=1.0, elastic_prob=1.0))})
    res.update({k: spread(v) for k, v in ts.items()})
    del scan, fns

if what in ('all', 'step'):
    steps = {}
    for k in (1, 4):
        torch.manual_seed(1234)
        model = get_model_dict('MaskTransUnet')([16, 32, 64, 128, 256], [100, 65, 40, 25, 10], [False, True, True, True, True],
                                                k, 2, dropout=0.3, act_dtype=torch.bfloat16).to(dev).train()
        reducer = train.GradReducer(model, unused=train.UNUSED_PARAMETERS)
        x, lab = data.synthetic_patches(2, SIZE, 100, dev, n_channels=k)
        graphed = train.GraphedStep(model, x, lab, train.get_dynamic_weight(1)[0], reducer)
        steps[f'step_k{k}'] = lambda graphed=graphed, x=x, lab=lab: graphed(x, lab)
    ts = alternate(steps)
    res['step_k1_us'], res['step_k4_us'] = spread(ts['step_k1']), spread(ts['step_k4'])
    res['step_k4_minus_k1_us'] = round(statistics.median(ts['step_k4']) - statistics.median(ts['step_k1']), 1)
print(json.dumps(res))
