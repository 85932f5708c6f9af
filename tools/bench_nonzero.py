"""Time of the nonzero crop (csrc/nonzero.hip, the hole filling of csrc/components.hip) on a synthetic skull-stripped head, four
channels 240 x 240 x 155 (int16, float32, int16, float32): an ellipsoid of tissue in exact zeros (about 85 % of the voxels), a
zero-valued cavity inside it.  Cases:
  kernel_*   each entry point alone between device events: ltu_nonzero_mask (int16 / float32 source), ltu_fill_holes (on the
             phantom's mask; on a full mask, which has no background to label: the floor of its passes; on an empty one, whose
             background is ONE component of every voxel), ltu_mask_box, ltu_normalize_masked (int16 / float32 source, the box)
  mask_*     data.nonzero_mask of the four device volumes (four mask launches, the hole filling, the box, one host read) against
             scipy.ndimage.binary_fill_holes + numpy on the host copies (3 repeats: it takes seconds)
  load_*     data.MultiScan of the four files at the file's own spacing, with crop='nonzero', intensity='zscore_nonzero' and
             without (intensity='zscore'): file reading, upload, statistics and resampling included
Wall clock between two device synchronisations unless named kernel_*; the contenders alternate inside every repeat; median with
min - max.  One JSON line.
usage: bench_nonzero.py [repeats]"""
import json
import os
import statistics
import struct
import sys
import tempfile
import time

import numpy as np
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data, nifti  # noqa: E402

reps = max(20, int(sys.argv[1]) if len(sys.argv) > 1 else 20)
dev = torch.device('cuda')
X, Y, Z = 240, 240, 155
n = X * Y * Z

rs = np.random.RandomState(0)
z, y, x = np.meshgrid(np.arange(Z, dtype=np.float32), np.arange(Y, dtype=np.float32), np.arange(X, dtype=np.float32), indexing='ij')
d2 = ((z - 0.5 * Z) / (0.36 * Z)) ** 2 + ((y - 0.52 * Y) / (0.33 * Y)) ** 2 + ((x - 0.48 * X) / (0.3 * X)) ** 2
head, cavity = d2 <= 1.0, d2 <= 0.03
del z, y, x, d2
host = []
for c in range(4):
    if c % 2 == 0:
        v = np.clip(np.rint(rs.normal(600.0, 150.0, (Z, Y, X))), 1, 4000).astype(np.int16)
    else:
        v = np.maximum(rs.normal(1.5, 0.4, (Z, Y, X)), 0.01).astype(np.float32)
    v[~head | cavity] = 0
    host.append(v)
vols = [torch.from_numpy(v).to(dev) for v in host]
codes = [_lib.I16, 0, _lib.I16, 0]
stream = torch.cuda.current_stream().cuda_stream


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6


def measure(fns, repeats, warm=2):
    for _ in range(warm):
        for fn in fns.values():
            fn()
    ts = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            ts[name].append(wall(fn))
    return ts


def events(fn):
    ts = []
    for k in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k >= 3:
            ts.append(a.elapsed_time(b) * 1e3)
    return ts


def put(res, name, t):
    res[name + '_us'] = round(statistics.median(t), 1)
    res[name + '_min_max_us'] = [round(min(t), 1), round(max(t), 1)]


def host_mask():
    m = np.zeros((Z, Y, X), bool)
    for v in host:
        m |= v != 0
    m = ndimage.binary_fill_holes(m)
    idx = np.nonzero(m)
    return m, tuple((int(i.min()), int(i.max()) + 1) for i in idx), int(m.sum())


# the device gives what the host gives
mask, box, count = data.nonzero_mask(vols)
ref_mask, ref_box, ref_count = host_mask()
assert np.array_equal(mask.cpu().numpy() != 0, ref_mask) and (box, count) == (ref_box, ref_count)
(z0, z1), (y0, y1), (x0, x1) = box

res = {'scan': [X, Y, Z], 'channels': 4, 'repeats': reps, 'zeros': round(1.0 - float(np.mean(host[0] != 0)), 3), 'mask_voxels': count,
       'box': [x1 - x0, y1 - y0, z1 - z0], 'box_fraction': round((x1 - x0) * (y1 - y0) * (z1 - z0) / n, 3)}

work = torch.empty((Z, Y, X), device=dev, dtype=torch.uint8)
filled = torch.empty_like(work)
full, empty = torch.ones_like(work), torch.zeros_like(work)
raw_mask = torch.empty_like(work)
for c in range(4):
    _lib.call('ltu_nonzero_mask', vols[c].data_ptr(), codes[c], n, 1.0, 0.0, raw_mask.data_ptr(), int(c > 0), stream)
ws = _lib.load().ltu_fill_holes_ws_elems(1, Z, Y, X)
scratch = torch.empty(ws, device=dev, dtype=torch.int32)
bx = torch.empty(6, device=dev, dtype=torch.int32)
cnt = torch.empty(1, device=dev, dtype=torch.int64)
out = torch.empty((z1 - z0, y1 - y0, x1 - x0), device=dev, dtype=torch.float32)


def fill(src):
    return lambda: _lib.call('ltu_fill_holes', src.data_ptr(), filled.data_ptr(), scratch.data_ptr(), ws, 1, Z, Y, X, 1, stream)


def normalize(c):
    return lambda: _lib.call('ltu_normalize_masked', vols[c].data_ptr(), codes[c], mask.data_ptr(), X, Y, Z, x0, y0, z0, x1 - x0, y1 - y0,
                             z1 - z0, 0.01, -1.0, out.data_ptr(), stream)


kernels = {'kernel_mask_i16': lambda: _lib.call('ltu_nonzero_mask', vols[0].data_ptr(), codes[0], n, 1.0, 0.0, work.data_ptr(), 0, stream),
           'kernel_mask_f32_accumulate': lambda: _lib.call('ltu_nonzero_mask', vols[1].data_ptr(), codes[1], n, 1.0, 0.0, work.data_ptr(), 1, stream),
           'kernel_fill_holes': fill(raw_mask), 'kernel_fill_holes_full_mask': fill(full), 'kernel_fill_holes_empty_mask': fill(empty),
           'kernel_mask_box': lambda: _lib.call('ltu_mask_box', mask.data_ptr(), 1, Z, Y, X, bx.data_ptr(), cnt.data_ptr(), stream),
           'kernel_normalize_i16': normalize(0), 'kernel_normalize_f32': normalize(1)}
for name, fn in kernels.items():
    put(res, name, events(fn))

put(res, 'mask_device', measure({'m': lambda: data.nonzero_mask(vols)}, reps)['m'])
put(res, 'mask_host_scipy', measure({'m': host_mask}, 3, warm=0)['m'])
res['mask_host_over_device'] = round(res['mask_host_scipy_us'] / res['mask_device_us'], 1)

with tempfile.TemporaryDirectory() as d:
    paths = []
    for c, v in enumerate(host):
        paths.append(os.path.join(d, f'c{c}.nii'))
        nifti.save(paths[-1], v.astype(np.float32), np.eye(4))
        if v.dtype == np.int16:                       # nifti.save writes float32: the int16 channels get an int16 header and voxels
            with open(paths[-1], 'rb') as f:
                hdr = bytearray(f.read()[:352])
            struct.pack_into('<2h', hdr, 70, 4, 16)
            with open(paths[-1], 'wb') as f:
                f.write(bytes(hdr) + v.astype('<i2').tobytes())
    loads = {'load_crop_zscore_nonzero': lambda: data.MultiScan(paths, pixdim=(1.0, 1.0, 1.0), intensity='zscore_nonzero', crop='nonzero'),
             'load_zscore': lambda: data.MultiScan(paths, pixdim=(1.0, 1.0, 1.0), intensity='zscore')}
    for name, t in measure(loads, reps, warm=1).items():
        put(res, name, t)
    scan = loads['load_crop_zscore_nonzero']()
    res['loaded_shape'], res['nonzero_fraction'] = list(scan.img.shape), round(scan.nonzero_fraction, 3)
print(json.dumps(res))
