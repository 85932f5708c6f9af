"""Time of one `data.sample_patches` call (4 patches of 512x512x32: centres, flips, crop + flip of image and label) with the crop
centres drawn from the host label (`crop_centers`: np.nonzero passes over the whole label) and from the label's `CropIndex`
(`index=`), on synthetic u8 labels of 512x512x100 and 820x820x118 with one box of foreground.  The two paths alternate in one
process from equal generators (their patches are compared bit for bit before timing); each timed window is a host clock around
the call and a device synchronise; a warm-up, then medians, minima and maxima of the repeats.  Also the index build alone (device
events; it reads the label once, n_voxels bytes) and the size of the index.  One JSON line per label.
usage: bench_sampler.py [repeats]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import data  # noqa: E402

reps = max(20, int(sys.argv[1]) if len(sys.argv) > 1 else 20)
dev = torch.device('cuda')
SIZE, SAMPLES = (512, 512, 32), 4


def spread(ts):
    return {'median': round(statistics.median(ts), 3), 'min': round(min(ts), 3), 'max': round(max(ts), 3)}


def call_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for H, W, D in ((512, 512, 100), (820, 820, 118)):
    host = np.zeros((H, W, D), np.uint8)
    host[H // 3:H // 3 + 90, W // 2:W // 2 + 60, D // 3:D // 3 + 40] = 1
    lab = torch.from_numpy(host).to(dev)
    img = torch.randn((H, W, D), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    index = data.CropIndex(lab)
    assert index.n_foreground == int(host.sum())

    a, b = np.random.RandomState(1), np.random.RandomState(1)
    hi, hl = data.sample_patches(img, lab, host, SIZE, SAMPLES, a)
    di, dl = data.sample_patches(img, lab, None, SIZE, SAMPLES, b, index=index)
    assert torch.equal(hi, di) and torch.equal(hl, dl) and a.randint(1 << 30) == b.randint(1 << 30)
    del hi, hl, di, dl

    rs_host, rs_index = np.random.RandomState(2), np.random.RandomState(2)
    t_host, t_index = [], []
    for r in range(-3, reps):                        # three warm-up rounds, then the two paths alternate
        th = call_ms(lambda: data.sample_patches(img, lab, host, SIZE, SAMPLES, rs_host))
        ti = call_ms(lambda: data.sample_patches(img, lab, None, SIZE, SAMPLES, rs_index, index=index))
        if r >= 0:
            t_host.append(th)
            t_index.append(ti)

    elems = index.index.numel()
    totals = torch.empty(9, device=dev, dtype=torch.int64)
    t_build = []
    for r in range(-3, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        data._lib.call('ltu_crop_index_build', lab.data_ptr(), lab.numel(), index.index.data_ptr(), elems, totals.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
        e1.record()
        e1.synchronize()
        if r >= 0:
            t_build.append(e0.elapsed_time(e1) * 1e3)
    t_new = [call_ms(lambda: data.CropIndex(lab)) * 1e3 for _ in range(reps)]      # with allocations and the read-back of the totals

    mh, mi = statistics.median(t_host), statistics.median(t_index)
    print(json.dumps({'label': [H, W, D], 'patch': list(SIZE), 'num_samples': SAMPLES, 'repeats': reps,
                      'host_centres_ms': spread(t_host), 'index_centres_ms': spread(t_index), 'ratio_of_medians': round(mh / mi, 1),
                      'build_us': spread(t_build), 'build_bytes_read': lab.numel(),
                      'build_tbps': round(lab.numel() / statistics.median(t_build) / 1e6, 2),
                      'crop_index_ctor_us': spread(t_new), 'index_bytes': elems * 4}), flush=True)
