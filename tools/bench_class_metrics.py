"""Time of one infer.evaluate_multiclass call with the label map (the eight criteria of inference_multi_classes.py:153 and the
is_save map of line 158) on a synthetic 512x512xD scan with 3 classes of blended f32 votes, against an eager-torch restatement of
the same eight criteria written the way loss/multi_criterions.py computes them (one-hot label, one reduction per criterion).
Device events around each call after warm-up, median of the repeats; effective bandwidth = the bytes the statistics pass must
move (B*H*W*D*(4C + 1), + 1 per voxel for the map) over the call time.  usage: bench_class_metrics.py [D] [repeats]"""
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import infer  # noqa: E402

D = int(sys.argv[1]) if len(sys.argv) > 1 else 200
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
B, C, H, W = 1, 3, 512, 512
dev = torch.device('cuda')
g = torch.Generator(device=dev).manual_seed(0)
h, w, d = (torch.arange(n, device=dev, dtype=torch.float32) for n in (H, W, D))
hh, ww, dd = h[:, None, None], w[None, :, None], d[None, None, :]


def ell(c, r):
    return ((hh - c[0]) / r[0]) ** 2 + ((ww - c[1]) / r[1]) ** 2 + ((dd - c[2]) / r[2]) ** 2 <= 1


masks = torch.zeros((B, 1, H, W, D), device=dev, dtype=torch.uint8)
masks[0, 0][ell((300, 250, D / 2), (40, 22, D / 8))] = 1
masks[0, 0][ell((318, 262, D / 2 + 3), (7, 6, D / 40 + 2))] = 2
# blended votes of 5 windows: one-hot of the labels with 10 % of the voxels voted elsewhere per window
votes = torch.zeros((B, C, H, W, D), device=dev, dtype=torch.float32)
for _ in range(5):
    lab = masks[:, 0].long()
    flip = torch.rand(lab.shape, device=dev, generator=g) < 0.1
    lab = torch.where(flip, torch.randint(0, C, lab.shape, device=dev, generator=g), lab)
    votes += F.one_hot(lab, C).permute(0, 4, 1, 2, 3).float()
predict = (votes / 5).contiguous()
del votes


def eager(predict, masks):
    """loss/multi_criterions.py restated in eager torch: the driver's one-hot label, then one reduction per criterion"""
    n, _, hx, wx, dx = masks.shape
    label = F.one_hot(masks.long().flatten(2).transpose(1, 2).squeeze(2), num_classes=C).transpose(1, 2)
    label = label.reshape(n, C, hx, wx, dx)
    p, t = predict.flatten(2).transpose(2, 1), label.flatten(2).transpose(2, 1)
    out = {}
    fp, ft = 1 - p[:, :, 0], 1 - t[:, :, 0]
    out['DiceClassLoss0'] = 1 - torch.mean((2 * torch.sum(fp * ft, -1) + 1e-9) / (torch.sum(fp + ft, -1) + 1e-9))
    for k, sfx in ((1, ''), (2, '2')):
        pc, tc = p[:, :, k], t[:, :, k]
        out[f'DiceClassLoss{sfx}'] = 1 - torch.mean((2 * torch.sum(pc * tc, -1) + 1e-9) / (torch.sum(pc + tc, -1) + 1e-9))
        out[f'Recall{sfx}'] = torch.mean((torch.sum(pc * tc, -1) + 1e-5) / (torch.sum(tc, -1) + 1e-5))
        out[f'Precision{sfx}'] = torch.mean((torch.sum(pc * tc, -1) + 1e-5) / (torch.sum(pc, -1) + 1e-5))
    pr = torch.sigmoid((1 - predict[:, 0]).flatten(2).sum(-1) - 10)
    tr = torch.sigmoid((1 - label[:, 0]).flatten(2).sum(-1).float() - 10)
    cp = torch.cumsum(pr, -1) / (pr.sum(-1, keepdim=True) + 1e-6)
    ct = torch.cumsum(tr, -1) / (tr.sum(-1, keepdim=True) + 1e-6)
    out['LocalizationLoss'] = torch.mean(torch.abs(cp - ct))
    out['label_map'] = torch.argmax(predict, 1)
    return out


def timed(fn):
    for _ in range(3):
        vals = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        vals = fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times), vals


vox = B * H * W * D
nbytes = vox * (4 * C + 1) + vox
med, lo, hi, vals = timed(lambda: infer.evaluate_multiclass(predict, masks, return_label_map=True))
print(f'{B}x{C}x{H}x{W}x{D}: evaluate_multiclass + label map {med:.3f} ms per call (min {lo:.3f}, max {hi:.3f}, {reps} calls); '
      f'{nbytes / 1e6:.1f} MB moved, {nbytes / med / 1e9:.2f} TB/s effective', flush=True)
emed, elo, ehi, evals = timed(lambda: eager(predict, masks))
print(f'eager torch restatement of the eight criteria + argmax: {emed:.3f} ms per call (min {elo:.3f}, max {ehi:.3f}); '
      f'speed-up {emed / med:.1f}x', flush=True)
worst = max(abs(vals[n].item() - evals[n].item()) / max(abs(evals[n].item()), 1e-6) for n in infer.MULTI_METRIC_NAMES)
same_map = torch.equal(vals['label_map'].long(), evals['label_map'])
print('values: ' + ', '.join(f'{n} {vals[n].item():.6f}' for n in infer.MULTI_METRIC_NAMES)
      + f'; largest relative difference to the eager restatement {worst:.2e}; label maps equal: {same_map}', flush=True)
