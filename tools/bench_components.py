"""Time of infer.label_components (connectivity 3), infer.remove_small_components (2 classes), infer.lesion_metrics (2 classes) and
infer.keep_largest_component on a synthetic 1x512x512xD CT-sized scan with a pancreas-sized organ (class 1), three tumour-sized
lesions (class 2) and a few hundred noise specks; hip events around each call after warm-up, median of the repeats.  For context
also times scipy.ndimage.label on the host, and prints the ratio to the labelling floor (one read of the u8 mask plus one write of
the int32 labels at 4.67 TB/s); with scipy the labels and the kept component are compared with the host's.
usage: bench_components.py [D] [repeats]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import infer  # noqa: E402
from oracle import infer as oracle_infer  # noqa: E402

D = int(sys.argv[1]) if len(sys.argv) > 1 else 200
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev = torch.device('cuda')
h, w, d = (torch.arange(n, device=dev, dtype=torch.float32) for n in (512, 512, D))
hh, ww, dd = h[:, None, None], w[None, :, None], d[None, None, :]


def ell(c, r):
    return ((hh - c[0]) / r[0]) ** 2 + ((ww - c[1]) / r[1]) ** 2 + ((dd - c[2]) / r[2]) ** 2 <= 1


zc = D / 2
gen = torch.Generator(device=dev).manual_seed(3)
masks = torch.zeros((1, 1, 512, 512, D), device=dev, dtype=torch.uint8)
masks[0, 0][ell((300, 250, zc), (40, 22, D / 8))] = 1
for c in ((318, 262, zc + 3), (285, 240, zc - 6), (305, 230, zc + 8)):
    masks[0, 0][ell(c, (7, 6, D / 40 + 2))] = 2
lab = torch.zeros((512, 512, D), device=dev, dtype=torch.long)
lab[ell((303, 248, zc + 1), (38, 23, D / 8 - 1))] = 1
for c in ((316, 262, zc + 2), (287, 241, zc - 5)):                  # two of the three lesions found
    lab[ell(c, (8, 5, D / 40 + 2))] = 2
lab[ell((200, 100, zc - 10), (5, 4, 3))] = 2                        # a false-positive lesion
specks = torch.rand((512, 512, D), device=dev, generator=gen) < 400 / (512 * 512 * D)
lab[specks] = torch.randint(1, 3, (int(specks.sum()),), device=dev, generator=gen)
predict = torch.nn.functional.one_hot(lab, 3).permute(3, 0, 1, 2)[None].to(torch.float32).contiguous()
fg = lab[None] != 0


def timed(fn):
    for _ in range(3):
        out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times), out


floor_ms = 512 * 512 * D * 5 / 4.67e12 * 1e3
fg_u8 = fg.to(torch.uint8)
med, lo, hi, (labels, counts) = timed(lambda: infer.label_components(fg_u8, connectivity=3))
print(f'label_components 1x512x512x{D} u8, c = 3: {med:.3f} ms (min {lo:.3f}, max {hi:.3f}, {reps} calls), '
      f'{int(counts[0])} components; floor {floor_ms:.3f} ms, ratio {med / floor_ms:.1f}', flush=True)
med, lo, hi, post = timed(lambda: infer.remove_small_components(predict, 10))
print(f'remove_small_components, 2 classes, min 10 voxels: {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); '
      f'kept {int(post[0, 1:].sum())} of {int(predict[0, 1:].sum())} fg voxels', flush=True)
med, lo, hi, vals = timed(lambda: infer.lesion_metrics(predict, masks, class_indices=(1, 2)))
print(f'lesion_metrics, 2 classes: {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); '
      + ', '.join(f'{k} {v[0].tolist()}' for k, v in vals.items()), flush=True)
med, lo, hi, kept = timed(lambda: infer.keep_largest_component(predict))
print(f'keep_largest_component: {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); '
      f'kept {int(kept[0, 1:].sum())} of {int(predict[0, 1:].sum())} fg voxels', flush=True)
try:
    from scipy import ndimage
    host = fg[0].cpu().numpy()
    t0 = time.perf_counter()
    ref, n = ndimage.label(host, ndimage.generate_binary_structure(3, 3))
    t1 = time.perf_counter()
    same = np.array_equal(ref, labels[0].cpu().numpy())
    print(f'scipy.ndimage.label on the host (context): {(t1 - t0) * 1e3:.1f} ms, {n} components, GPU labels identical: {same}',
          flush=True)
    assert torch.equal(kept.cpu(), oracle_infer.keep_largest_component(predict.cpu())), 'keep_largest_component differs from the oracle'
    print('keep_largest_component identical to oracle.infer.keep_largest_component', flush=True)
except ImportError:
    print('scipy not installed: host timing skipped', flush=True)
