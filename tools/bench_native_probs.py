"""Time of a prediction's way back onto the file's grid, on DESIGN.md's worked example: softmax probabilities on the RAS grid
819 x 819 x 125 (the 512 x 512 x 100 scan at diag(-0.8, -0.8, 2.5) resampled to (0.5, 0.5, 2.0)), C = 3 and C = 8, pulled back to 512 x
512 x 100.  Three contenders per C:
  fused    data.to_native_probs: one ltu_resample_argmax launch, labels only (and once more with every class's probabilities)
  loop     what a user wrote before it: C x data.resample (one f32 volume on the file's grid each) + torch.stack + torch.argmax
  nearest  data.to_native of the ready-made u8 label map (torch.argmax on the RAS grid is not timed): the old path, for scale
Device events around each call after warm-up; the contenders alternate inside every repeat; median with min - max of the repeats.
The fused call and the loop are checked to give the same labels first.  Algorithmic bytes: the fused call reads the C channels once
and writes one byte per file voxel; the loop reads the same and moves C f32 volumes on the file's grid three more times (resample
writes them, stack copies them, argmax reads the copy: 4 + 8 + 4 bytes per voxel and channel) before it writes 8-byte indices.  The
loop's peak extra device memory is measured with torch's allocator statistics.  One JSON line.
usage: bench_native_probs.py [repeats]"""
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


class _Scan:
    pass


scan = _Scan()
scan.matrix, scan.shape, _ = geometry.spacing_plan((X, Y, Z), aff, (0.5, 0.5, 2.0))
scan.native_shape = (X, Y, Z)
assert scan.shape == (819, 819, 125), scan.shape
H, W, D = scan.shape
back = geometry.invert(scan.matrix)
identity = (1.0, 0.0, -np.inf, np.inf)
ras_vox, file_vox = H * W * D, X * Y * Z


def loop(probs):
    chans = [data.resample(probs[c], None, back, (X, Y, Z), identity, 0, src_strides=(W * D, D, 1), out_strides=(1, X, X * Y))[0]
             for c in range(probs.shape[0])]
    return torch.argmax(torch.stack(chans), 0)


def measure(fns):
    """{name: [microseconds]}: every contender once per repeat, in turn"""
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b) * 1e3)
    return ts


res = {'ras': list(scan.shape), 'file': [X, Y, Z], 'repeats': reps}
for C in (3, 8):
    g = torch.Generator(device=dev).manual_seed(C)
    probs = torch.empty((C, H, W, D), device=dev, dtype=torch.float32)
    for c in range(C):                                         # smooth along D and noisy in plane; normalised below
        probs[c] = torch.rand((H, W, 1), device=dev, generator=g) + torch.rand((H, W, D), device=dev, generator=g)
    probs /= probs.sum(0, keepdim=True)
    label_map = torch.argmax(probs, 0).to(torch.uint8)
    fused = data.to_native_probs(probs, scan)[0]
    same = bool(torch.equal(fused, loop(probs).to(torch.uint8)))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    loop(probs)
    torch.cuda.synchronize()
    loop_peak = torch.cuda.max_memory_allocated() - held
    ts = measure({'fused': lambda: data.to_native_probs(probs, scan),
                  'fused_all_probs': lambda: data.to_native_probs(probs, scan, classes=range(C)),
                  'loop': lambda: loop(probs),
                  'nearest': lambda: data.to_native(label_map, scan)})
    r = {'labels_equal_loop': same, 'loop_peak_extra_mib': round(loop_peak / 2 ** 20, 1),
         'fused_gb': round((C * ras_vox * 4 + file_vox) / 1e9, 3),
         'loop_gb': round((C * ras_vox * 4 + C * file_vox * 16 + file_vox * 8) / 1e9, 3)}
    for name, t in ts.items():
        r[name + '_us'] = round(statistics.median(t), 1)
        r[name + '_min_max_us'] = [round(min(t), 1), round(max(t), 1)]
    r['loop_over_fused'] = round(r['loop_us'] / r['fused_us'], 2)
    r['fused_over_nearest'] = round(r['fused_us'] / r['nearest_us'], 2)
    r['fused_tbps'] = round(r['fused_gb'] * 1e3 / r['fused_us'], 2)
    res[f'C{C}'] = r
    del probs, label_map, fused
    torch.cuda.empty_cache()
print(json.dumps(res))
