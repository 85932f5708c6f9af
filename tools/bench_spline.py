"""Time of the cubic B-spline resampling path on a synthetic MSD-sized scan: 512x512x100 int16 + u8 label at diag(-0.8, -0.8, 2.5)
brought to 819x819x125 (Spacingd (0.5, 0.5, 2.0) + Orientationd RAS, the window folded in), beside the trilinear kernel it extends.
Measured: ltu_resample_grid (image only), ltu_spline_prefilter alone at orders (3, 3, 3) and (3, 3, 0) with its algorithmic bytes
per source voxel (csrc/spline.hip: 2 + 12 for the int16 axis-0 pass, 16 per further filtered axis), ltu_resample_spline alone at both
orders, and what SpacedScan launches for order 1, 3 and 'auto' (image and label; 'auto' resolves to (3, 3, 0) for this scan).
Device events around each call after warm-up; the calls are alternated (one of each per round), so that drift of the device's
clocks lands on all of them alike; median, min and max of the rounds.  One JSON line.
usage: bench_spline.py [rounds]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data, geometry  # noqa: E402
from lintransunet_amd.ops import _p, _s  # noqa: E402

rounds = max(20, int(sys.argv[1]) if len(sys.argv) > 1 else 20)
dev = torch.device('cuda')
X, Y, Z = 512, 512, 100
aff = np.diag([-0.8, -0.8, 2.5, 1.0])
aff[:3, 3] = (200.0, 150.0, -300.0)
pixdim = (0.5, 0.5, 2.0)
M, shape, _ = geometry.spacing_plan((X, Y, Z), aff, pixdim)
assert shape == (819, 819, 125), shape
auto = geometry.resample_orders(geometry.voxel_spacing(aff), pixdim)
assert auto == (3, 3, 0), auto
g = torch.Generator(device=dev).manual_seed(0)
raw = (torch.randn((Z, Y, X), device=dev, generator=g) * 300 + 40).clamp_(-1024, 3000).to(torch.int16)
lab = (raw > 340).to(torch.uint8).contiguous()
imap = data.intensity_map(data.MONAI_CT_WINDOW)
S, O = (X, Y, Z), shape
mat = torch.as_tensor(np.asarray(M, dtype=np.float64).ravel().copy()).to(dev)
lane = geometry.lane_axis(M, (1, X, X * Y))
out = torch.empty(O, device=dev, dtype=torch.float32)
coefs = {o: data.spline_coefficients(raw, o, imap, _lib.I16) for o in ((3, 3, 3), (3, 3, 0))}


def gather(orders):
    _lib.call('ltu_resample_spline', _p(coefs[orders]), *S, *orders, _p(out), *O, O[1] * O[2], O[2], 1, _p(mat), lane, float(imap[2]),
              float(imap[3]), _s())


calls = {
    'trilinear_image': lambda: data.resample(raw, None, M, shape, imap, _lib.I16),
    'prefilter_333': lambda: data.spline_coefficients(raw, (3, 3, 3), imap, _lib.I16),
    'prefilter_330': lambda: data.spline_coefficients(raw, (3, 3, 0), imap, _lib.I16),
    'gather_333': lambda: gather((3, 3, 3)),
    'gather_330': lambda: gather((3, 3, 0)),
    'scan_order_1': lambda: data.resample(raw, lab, M, shape, imap, _lib.I16, order=1),
    'scan_order_3': lambda: data.resample(raw, lab, M, shape, imap, _lib.I16, order=3),
    'scan_order_auto': lambda: data.resample(raw, lab, M, shape, imap, _lib.I16, order=auto),
}
for fn in calls.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in calls}
for _ in range(rounds):
    for k, fn in calls.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times[k].append(a.elapsed_time(b) * 1e3)

src_vox, out_vox = X * Y * Z, int(np.prod(shape))
res = {'scan': [X, Y, Z], 'ras': list(shape), 'auto_orders': list(auto), 'rounds': rounds}
for k, ts in times.items():
    res[k + '_us'] = {'median': round(statistics.median(ts), 1), 'min': round(min(ts), 1), 'max': round(max(ts), 1)}
for name, filtered in (('prefilter_333', 3), ('prefilter_330', 2)):
    per_voxel = 2 + 12 + 16 * (filtered - 1)
    res[name + '_bytes_per_voxel'] = per_voxel
    res[name + '_tbps'] = round(per_voxel * src_vox / res[name + '_us']['median'] / 1e6, 2)
res['trilinear_image_tbps'] = round((src_vox * 2 + out_vox * 4) / res['trilinear_image_us']['median'] / 1e6, 2)
for name, taps in (('gather_333', 64), ('gather_330', 16)):
    res[name + '_gtaps_per_s'] = round(taps * out_vox / res[name + '_us']['median'] / 1e3, 1)
print(json.dumps(res))
