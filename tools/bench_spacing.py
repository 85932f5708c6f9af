"""Time of the monai driver's data side on a synthetic MSD-sized scan: 512x512x100 int16 + u8 label at diag(-0.8, -0.8, 2.5),
resampled (Spacingd (0.5, 0.5, 2.0) + Orientationd RAS, ScaleIntensityRanged folded in) to 819x819x125 by one ltu_resample_grid
launch, and ltu_crop_orient for the driver's batch of 12 patches of 512x512x32 (flip / rot90 mixed).  Device events around each
call after warm-up, median of the repeats.  Algorithmic bytes: the resample reads the int16 scan and the u8 label once and writes
the f32 image and the u8 label once; a patch batch reads and writes 5 bytes per patch voxel.  One JSON line.
usage: bench_spacing.py [repeats]"""
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
X, Y, Z = 512, 512, 100
aff = np.diag([-0.8, -0.8, 2.5, 1.0])
aff[:3, 3] = (200.0, 150.0, -300.0)
M, shape, _ = geometry.spacing_plan((X, Y, Z), aff, (0.5, 0.5, 2.0))
assert shape == (819, 819, 125), shape
g = torch.Generator(device=dev).manual_seed(0)
raw = (torch.randn((Z, Y, X), device=dev, generator=g) * 300 + 40).clamp_(-1024, 3000).to(torch.int16)
zz, yy, xx = torch.meshgrid(*(torch.arange(n, device=dev, dtype=torch.float32) for n in (Z, Y, X)), indexing='ij')
d = ((xx - 260) / 60) ** 2 + ((yy - 300) / 35) ** 2 + ((zz - 50) / 20) ** 2
lab = ((d <= 1).to(torch.uint8) + (d <= 0.2).to(torch.uint8)).contiguous()
del zz, yy, xx, d
imap = data.intensity_map(data.MONAI_CT_WINDOW)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts)


out_vox = int(np.prod(shape))
res = {'scan': [X, Y, Z], 'ras': list(shape)}
t, tmin = timed(lambda: data.resample(raw, lab, M, shape, imap, 3))
nbytes = X * Y * Z * 3 + out_vox * 5
res.update(resample_us=round(t, 1), resample_min_us=round(tmin, 1), resample_gb=round(nbytes / 1e9, 3),
           resample_tbps=round(nbytes / t / 1e6, 2))
t, _ = timed(lambda: data.resample(raw, None, M, shape, imap, 3))
nb = X * Y * Z * 2 + out_vox * 4
res.update(image_only_us=round(t, 1), image_only_tbps=round(nb / t / 1e6, 2))
t, _ = timed(lambda: data.resample(None, lab, M, shape))
nb = X * Y * Z + out_vox
res.update(label_only_us=round(t, 1), label_only_tbps=round(nb / t / 1e6, 2))

img, lab_ras = data.resample(raw, lab, M, shape, imap, 3)
draws = [([409 + 7 * n, 409 - 5 * n, 62], bool(n % 2), n % 4) for n in range(12)]
t, _ = timed(lambda: data.crop_orient(img, lab_ras, draws, (512, 512, 32)))
nb = 12 * 512 * 512 * 32 * 5 * 2
res.update(crop_orient_us=round(t, 1), crop_orient_gb=round(nb / 1e9, 3), crop_orient_tbps=round(nb / t / 1e6, 2))


class _Scan:
    pass


scan = _Scan()
scan.shape, scan.native_shape, scan.matrix = shape, (X, Y, Z), M
t, _ = timed(lambda: data.to_native(lab_ras, scan))
nb = out_vox + X * Y * Z
res.update(to_native_us=round(t, 1), to_native_tbps=round(nb / t / 1e6, 2))
res['to_native_round_trip_exact'] = bool(torch.equal(data.to_native(lab_ras, scan), lab))   # finer on every axis: bit for bit
res['repeats'] = reps
print(json.dumps(res))
