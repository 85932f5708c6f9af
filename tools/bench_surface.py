"""Time of one infer.surface_metrics call (HD, HD95, ASSD, NSD of two classes) on a synthetic 512x512xD CT-sized scan with a
pancreas-sized organ (class 1) and a tumour-sized lesion (class 2), spacing (0.7, 0.7, 2.5) mm; hip events around each call after
warm-up, median of the repeats.  Also times the whole-volume crop (both boundaries spread over the scan: the worst case for the
distance transform).  usage: bench_surface.py [D] [repeats] [organ|whole|both]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import infer  # noqa: E402

D = int(sys.argv[1]) if len(sys.argv) > 1 else 200
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
cases = sys.argv[3] if len(sys.argv) > 3 else 'both'
dev = torch.device('cuda')
h, w, d = (torch.arange(n, device=dev, dtype=torch.float32) for n in (512, 512, D))
hh, ww, dd = h[:, None, None], w[None, :, None], d[None, None, :]


def ell(c, r):
    return ((hh - c[0]) / r[0]) ** 2 + ((ww - c[1]) / r[1]) ** 2 + ((dd - c[2]) / r[2]) ** 2 <= 1


zc = D / 2
masks = torch.zeros((1, 1, 512, 512, D), device=dev, dtype=torch.uint8)
masks[0, 0][ell((300, 250, zc), (40, 22, D / 8))] = 1
masks[0, 0][ell((318, 262, zc + 3), (7, 6, D / 40 + 2))] = 2
lab = torch.zeros((512, 512, D), device=dev, dtype=torch.long)
lab[ell((303, 248, zc + 1), (38, 23, D / 8 - 1))] = 1
lab[ell((316, 262, zc + 2), (8, 5, D / 40 + 2))] = 2
lab[ell((200, 100, zc - 10), (5, 4, 3))] = 1                  # a stray false-positive island
predict = torch.nn.functional.one_hot(lab, 3).permute(3, 0, 1, 2)[None].to(torch.float32).contiguous()
spacing = (0.7, 0.7, 2.5)


def timed(pred, msk):
    for _ in range(3):
        vals = infer.surface_metrics(pred, msk, class_indices=(1, 2), spacing=spacing, nsd_tolerance=2.0)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        vals = infer.surface_metrics(pred, msk, class_indices=(1, 2), spacing=spacing, nsd_tolerance=2.0)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times), vals


if cases in ('organ', 'both'):
    med, lo, hi, vals = timed(predict, masks)
    print(f'512x512x{D}, 2 classes, organ-sized crop: {med:.2f} ms per call (min {lo:.2f}, max {hi:.2f}, {reps} calls); '
          + ', '.join(f'{k} {v[0].tolist()}' for k, v in vals.items()), flush=True)
# worst case: boundaries in opposite corners of the scan, so the crop is the whole volume
if cases in ('whole', 'both'):
    masks2 = torch.zeros_like(masks)
    masks2[0, 0, :6, :6, :6] = 1
    masks2[0, 0, -6:, :6, -6:] = 2
    lab2 = torch.zeros_like(lab)
    lab2[-5:, -5:, -5:] = 1
    lab2[:5, -5:, :5] = 2
    pred2 = torch.nn.functional.one_hot(lab2, 3).permute(3, 0, 1, 2)[None].to(torch.float32).contiguous()
    med, lo, hi, vals = timed(pred2, masks2)
    print(f'512x512x{D}, 2 classes, whole-volume crop: {med:.2f} ms per call (min {lo:.2f}, max {hi:.2f}, {reps} calls); '
          + ', '.join(f'{k} {v[0].tolist()}' for k, v in vals.items()), flush=True)
