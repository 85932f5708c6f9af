"""Time of a scan's intensity statistics (csrc/intensity.hip) on a synthetic CT-like scan 512 x 512 x 100 int16: 60 % of the voxels at
-1024 (air), the rest around 40 +- 100, under a label with 0.5 % foreground.  Cases:
  a  data.intensity_histogram under the label        b  of the whole scan
  c  of a whole scan of uniformly random int16 (no hot bin; b over c is what the hot bin costs or saves)
  d  data.intensity_stats of the float32 copy of the scan, three percentiles
Next to a, b and d: what a user could do on the device before (torch.sort of the selected voxels, the order statistics picked from
it, mean and std in float64) and, for a and b, np.percentile + mean + std on the host copy (3 repeats: it takes seconds).  Every
contender is a whole call, host work and read-backs included: wall clock between two device synchronisations; the contenders
alternate inside every repeat; median with min - max.  kernel_*: the ltu_intensity_hist launch alone between device events, and
its ratio to the byte floor: 3 bytes per voxel under a label, 2 without, at the 2.52 TB/s that data.to_native_probs streams on this
machine (1.03 GB in 0.408 ms).  One JSON line.
usage: bench_intensity.py [repeats]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data  # noqa: E402

reps = max(20, int(sys.argv[1]) if len(sys.argv) > 1 else 20)
dev = torch.device('cuda')
X, Y, Z = 512, 512, 100
n = X * Y * Z
STREAM_TBPS = 1.03e9 / 0.408e-3 / 1e12
QS = (0.5, 50.0, 99.5)

rs = np.random.RandomState(0)
host = np.rint(rs.normal(40.0, 100.0, n))
host[rs.rand(n) < 0.6] = -1024
host = host.astype(np.int16).reshape(Z, Y, X)
lab_host = np.zeros((Z, Y, X), np.uint8)
lab_host[40:60, 224:288, 205:307] = 1                      # 20 x 64 x 102 = 130 560 voxels = 0.5 %
img, lab = torch.from_numpy(host).to(dev), torch.from_numpy(lab_host).to(dev)
uniform = torch.from_numpy(rs.randint(-32768, 32768, size=(Z, Y, X)).astype(np.int16)).to(dev)
imgf = img.to(torch.float32)


def sort_stats(v):
    s, _ = torch.sort(v.flatten())
    m = s.numel()
    picks = [0, m - 1] + [r for q in QS for r in data._percentile_ranks(m, q)[:2]]
    f = s.to(torch.float64)
    return torch.stack([*(f[r] for r in picks), f.mean(), f.std(unbiased=False)]).cpu()


def host_stats(v):
    v = v.astype(np.float64)
    return [np.percentile(v, QS), v.min(), v.max(), v.mean(), v.std()]


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6


def measure(fns, repeats):
    for _ in range(2):
        for fn in fns.values():
            fn()
    ts = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            ts[name].append(wall(fn))
    return ts


def kernel_us(x, lb, code, mode):
    hist = torch.zeros(65536, device=dev, dtype=torch.int32)
    counts = torch.zeros(2, device=dev, dtype=torch.int64)
    ts = []
    for k in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.call('ltu_intensity_hist', x.data_ptr(), code, lb.data_ptr() if lb is not None else 0, x.numel(), data.FG_MASK, mode, 0,
                  hist.data_ptr(), counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
        b.record()
        b.synchronize()
        if k >= 3:
            ts.append(a.elapsed_time(b) * 1e3)
    return ts


def put(res, name, t):
    res[name + '_us'] = round(statistics.median(t), 1)
    res[name + '_min_max_us'] = [round(min(t), 1), round(max(t), 1)]


# the histogram gives what the sort gives
st = data.histogram_stats(data.intensity_histogram(img, lab)[0].cpu().numpy(), QS)
ref = sort_stats(img[lab > 0]).tolist()
assert (st['min'], st['max']) == (ref[0], ref[1]) and abs(st['mean'] - ref[8]) < 1e-9 and abs(st['std'] - ref[9]) < 1e-9

res = {'scan': [X, Y, Z], 'foreground': int(lab_host.sum()), 'repeats': reps, 'stream_tbps': round(STREAM_TBPS, 2)}
ts = measure({'a_hist_label': lambda: data.intensity_histogram(img, lab),
              'a_sort_label': lambda: sort_stats(img[lab > 0]),
              'b_hist_scan': lambda: data.intensity_histogram(img),
              'b_sort_scan': lambda: sort_stats(img),
              'c_hist_uniform': lambda: data.intensity_histogram(uniform),
              'a_stats_label': lambda: data.intensity_stats(img, lab, percentiles=QS),
              'b_stats_scan': lambda: data.intensity_stats(img, percentiles=QS),
              'd_stats_f32': lambda: data.intensity_stats(imgf, percentiles=QS),
              'd_sort_f32': lambda: sort_stats(imgf)}, reps)
for name, t in ts.items():
    put(res, name, t)
fg = host[lab_host > 0]
for name, t in measure({'a_numpy_label': lambda: host_stats(fg), 'b_numpy_scan': lambda: host_stats(host)}, 3).items():
    put(res, name, t)
for name, (x, lb, code, mode, nbytes) in {'kernel_a': (img, lab, _lib.I16, _lib.HIST_I16, 3), 'kernel_b': (img, None, _lib.I16, _lib.HIST_I16, 2),
                                          'kernel_c': (uniform, None, _lib.I16, _lib.HIST_I16, 2),
                                          'kernel_f32_hi': (imgf, None, 0, _lib.HIST_F32_HI, 4)}.items():
    put(res, name, kernel_us(x, lb, code, mode))
    res[name + '_floor_us'] = round(nbytes * n / (STREAM_TBPS * 1e12) * 1e6, 1)
    res[name + '_over_floor'] = round(res[name + '_us'] / res[name + '_floor_us'], 2)
res['a_sort_over_hist'] = round(res['a_sort_label_us'] / res['a_hist_label_us'], 2)
res['b_sort_over_hist'] = round(res['b_sort_scan_us'] / res['b_hist_scan_us'], 2)
res['d_sort_over_stats'] = round(res['d_sort_f32_us'] / res['d_stats_f32_us'], 2)
res['kernel_b_over_c'] = round(res['kernel_b_us'] / res['kernel_c_us'], 3)
print(json.dumps(res))
