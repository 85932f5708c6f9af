"""Window blending (csrc/blend.hip) on one MI355X.  usage: bench_infer_blend.py [kernels|scan|all] [reps]

kernels: ltu_window_blend on 4 items of 512x512x32, C = 2, Gaussian tables - once the four (0, 1) mirror variants of one window,
         once four distinct windows of a 512x512x96 scan (D starts 0, 12, 24, 36 at overlap 0.6) - and on the same windows with
         one-hot predictions and tables of ones (the constant mode).  Algorithmic bytes = the seg reads
         (n h w d C 4) + one read and one write of votes and wsum per covered voxel ((C + 1) 4 2 per voxel of the union).
scan:    whole 512x512x96 scans through infer_volume with the reference model in bf16, graph replay, sw_batch_size 4, overlap 0.6:
         constant / one-hot (the reference's call), Gaussian / probs, Gaussian / probs + mirror (0, 1) and (0, 1, 2), alternated.
Times are device events, median of `reps` (default 20) after warm-up; kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of `bench_infer_blend.py kernels`."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, infer  # noqa: E402
from lintransunet_amd.ops import _p, _s  # noqa: E402

PART = sys.argv[1] if len(sys.argv) > 1 else 'all'
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
DEV = 'cuda'


def _time(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def _union_voxels(items, roi):
    cover = set()
    for b, h0, w0, d0, _ in items:
        cover.add((b, h0, w0, d0))
    box = np.zeros((1, 512, 512, 96), dtype=bool)
    for b, h0, w0, d0 in cover:
        box[b, h0:h0 + roi[0], w0:w0 + roi[1], d0:d0 + roi[2]] = True
    return int(box.sum())


def kernels():
    roi, img, C, B = (512, 512, 32), (512, 512, 96), 2, 1
    g0, g1, g2, wmin = infer.importance_tables(roi, 'gaussian', 0.125)
    gauss = torch.tensor(np.concatenate((g0, g1, g2)), dtype=torch.float32, device=DEV)
    ones = torch.ones(sum(roi), device=DEV)
    votes = torch.zeros((B, C) + img, device=DEV)
    wsum = torch.zeros((B,) + img, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(0)
    p1 = torch.rand((4,) + roi, device=DEV, generator=gen)
    soft = torch.stack((p1, 1 - p1), -1).contiguous()                          # [4, h, w, d, 2]
    onehot = (soft > 0.5).to(torch.float32).contiguous()
    layouts = {'mirror_01_one_window': [(0, 0, 0, 0, m) for m in infer.mirror_masks((0, 1))],
               'four_distinct_windows': [(0, 0, 0, d0, 0) for d0 in (0, 12, 24, 36)]}
    res = {}
    for name, items in layouts.items():
        desc = np.ascontiguousarray(items, dtype=np.int32)
        vox = _union_voxels(items, roi)
        nbytes = len(items) * roi[0] * roi[1] * roi[2] * C * 4 + vox * (C + 1) * 4 * 2

        def blend(seg, tab, w):
            _lib.call('ltu_window_blend', _p(seg), _p(votes), _p(wsum), _p(tab), _p(tab[roi[0]:]), _p(tab[roi[0] + roi[1]:]), w,
                      desc.ctypes.data, len(items), B, C, *img, *roi, _s())

        t_g = _time(lambda: blend(soft, gauss, wmin), REPS)
        t_b1 = _time(lambda: blend(onehot, ones, 1.0), REPS)
        res[name] = {'gaussian_ms': statistics.median(t_g), 'gaussian_TBps': nbytes / statistics.median(t_g) / 1e9,
                     'bytes': nbytes, 'covered_voxels': vox,
                     'onehot_blend_ms': statistics.median(t_b1), 'spread_gaussian_ms': [min(t_g), max(t_g)]}
        print(f'{name}: ltu_window_blend gaussian {statistics.median(t_g) * 1e3:.1f} us ({nbytes / 1e6:.0f} MB algorithmic, '
              f'{nbytes / statistics.median(t_g) / 1e9:.2f} TB/s event-timed); one-hot, unit tables: '
              f'{statistics.median(t_b1) * 1e3:.1f} us', flush=True)
    return res


def scan():
    from lintransunet_amd.model import get_model_dict
    torch.manual_seed(0)
    model = get_model_dict('MaskTransUnet')([16, 32, 64, 128, 256], [100, 65, 40, 25, 10], [False, True, True, True, True], 1, 2,
                                            act_dtype=torch.bfloat16).to(DEV).eval()
    x = torch.randn(1, 1, 512, 512, 96, device=DEV)
    roi = (512, 512, 32)
    g_onehot = infer.GraphedPredictor(model, 4, roi, x.device)
    g_probs = infer.GraphedPredictor(model, 4, roi, x.device, probs=True)
    cfgs = {'constant_onehot': dict(graph=g_onehot), 'gaussian_probs': dict(graph=g_probs, mode='gaussian'),
            'gaussian_probs_mirror01': dict(graph=g_probs, mode='gaussian', mirror_axes=(0, 1)),
            'gaussian_probs_mirror012': dict(graph=g_probs, mode='gaussian', mirror_axes=(0, 1, 2))}
    times = {k: [] for k in cfgs}
    for kw in cfgs.values():                     # warm-up of every configuration
        infer.infer_volume(model, x, **kw)
    torch.cuda.synchronize()
    for _ in range(REPS):                        # alternated, so drift hits every configuration alike
        for k, kw in cfgs.items():
            times[k] += _time(lambda: infer.infer_volume(model, x, **kw), 1, warmup=0)
    res = {k: {'ms_per_scan': statistics.median(v), 'spread_ms': [min(v), max(v)]} for k, v in times.items()}
    for k, v in res.items():
        print(f'512x512x96 scan, {k}: {v["ms_per_scan"]:.2f} ms per scan (min {v["spread_ms"][0]:.2f}, max {v["spread_ms"][1]:.2f})',
              flush=True)
    return res


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('bench_infer_blend.py needs a GPU')
    out = {}
    if PART in ('kernels', 'all'):
        out['kernels'] = kernels()
    if PART in ('scan', 'all'):
        out['scan'] = scan()
    print(json.dumps(out))
