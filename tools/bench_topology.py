"""Time of infer.skeletonize, infer.betti_numbers and infer.topology_metrics (one class) on two synthetic 512x512xD masks: a vessel
tree (a trunk that branches four times, tubes of radius 6 down to 2 voxels) and a compact organ (a ball of radius 60).  The
yardstick is infer.label_components (connectivity 3) on the same masks in the same run; the calls are alternated round-robin, hip
events around each, median of the repeats with min - max.  Also the voxels deleted per second, and what the simple-point predicate
costs alone: ltu_thin_simple_codes on 10^7 random codes.
usage: bench_topology.py [D] [repeats]"""
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, infer  # noqa: E402
from lintransunet_amd.ops import _p, _s  # noqa: E402

D = int(sys.argv[1]) if len(sys.argv) > 1 else 200
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev = torch.device('cuda')
H = W = 512


def tube(mask, a, b, r):
    """sets the voxels within r of the segment a - b, inside the segment's box only"""
    lo = [max(int(min(a[i], b[i]) - r - 1), 0) for i in range(3)]
    hi = [min(int(max(a[i], b[i]) + r + 2), n) for i, n in enumerate((H, W, D))]
    if any(h <= l for l, h in zip(lo, hi)):
        return
    g = torch.stack(torch.meshgrid(*[torch.arange(l, h, device=dev, dtype=torch.float32) for l, h in zip(lo, hi)], indexing='ij'), -1)
    a, b = torch.tensor(a, device=dev), torch.tensor(b, device=dev)
    ab = b - a
    t = (((g - a) @ ab) / (ab @ ab)).clamp(0, 1)
    mask[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] |= ((g - (a + t[..., None] * ab)).norm(dim=-1) <= r).to(torch.uint8)


def vessel_tree():
    mask = torch.zeros((H, W, D), device=dev, dtype=torch.uint8)
    gen = torch.Generator().manual_seed(5)
    ends = [((40.0, 256.0, D / 2), (1.0, 0.0, 0.0), 6.0, 110.0)]          # start, direction, radius, length
    for level in range(5):
        nxt = []
        for start, direction, r, length in ends:
            stop = tuple(s + length * c for s, c in zip(start, direction))
            tube(mask, start, stop, r)
            for sign in (-1.0, 1.0):                                         # two children, turned in W and a little in D
                turn = sign * (0.5 + 0.3 * torch.rand(1, generator=gen).item())
                dz = 0.5 * (torch.rand(1, generator=gen).item() - 0.5)
                v = (direction[0] * math.cos(turn) - direction[1] * math.sin(turn), direction[0] * math.sin(turn) + direction[1] * math.cos(turn), dz)
                n = math.sqrt(sum(c * c for c in v))
                nxt.append((stop, tuple(c / n for c in v), max(r - 1.0, 2.0), length * 0.72))
        ends = nxt
    return mask


def organ():
    h, w, d = (torch.arange(n, device=dev, dtype=torch.float32) for n in (H, W, D))
    return ((h[:, None, None] - 256) ** 2 + (w[None, :, None] - 256) ** 2 + (d[None, None, :] - D / 2) ** 2 <= 60.0 ** 2).to(torch.uint8)


def alternated(fns):
    """{name: (median, min, max, last result)} of the calls taken round-robin"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times, out = {n: [] for n in fns}, {}
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out[name] = fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    return {n: (statistics.median(t), min(t), max(t), out[n]) for n, t in times.items()}


for title, mask in (('vessel tree', vessel_tree()), ('organ', organ())):
    m4 = mask[None]
    moved = torch.roll(mask, 1, 1)                                          # the prediction: the mask one voxel aside
    predict = torch.stack([1 - moved, moved])[None].to(torch.float32).contiguous()
    res = alternated({'label_components': lambda: infer.label_components(m4, connectivity=3),
                      'skeletonize': lambda: infer.skeletonize(m4),
                      'betti_numbers': lambda: infer.betti_numbers(m4),
                      'topology_metrics': lambda: infer.topology_metrics(predict, mask[None, None], class_indices=(1,))})
    objects = int(mask.sum())
    print(f'{title}, 1x{H}x{W}x{D} u8, {objects} object voxels ({reps} alternated calls, median (min - max) ms)', flush=True)
    for name, (med, lo, hi, out) in res.items():
        print(f'  {name}: {med:.3f} ({lo:.3f} - {hi:.3f})', end='')
        if name == 'skeletonize':
            skel, its = out
            left = int(skel.sum())
            batches = -(-(its + 1) // infer.THIN_BATCH)
            print(f'; {its} iterations, {left} skeleton voxels, {2 + 10 * infer.THIN_BATCH * batches} launches and memsets, '
                  f'{1 + batches} host reads, {(objects - left) / (med * 1e-3):.3e} voxels deleted per second', end='')
        elif name == 'betti_numbers':
            print('; ' + ', '.join(f'{k} {v.tolist()}' for k, v in out.items()), end='')
        elif name == 'topology_metrics':
            print('; ' + ', '.join(f'{k} {v.flatten().tolist()}' for k, v in out.items()), end='')
        elif name == 'label_components':
            print(f'; {int(out[1][0])} components', end='')
        print(flush=True)
    b_mask, b_skel = infer.betti_numbers(m4), infer.betti_numbers(res['skeletonize'][3][0])
    assert all(torch.equal(b_mask[k], b_skel[k]) for k in b_mask), 'the skeleton changed the topology'

n = 10 ** 7
codes = torch.randint(0, 1 << 27, (n,), device=dev, dtype=torch.int64).to(torch.int32)
flags = torch.empty(n, device=dev, dtype=torch.uint8)
med, lo, hi, _ = alternated({'codes': lambda: _lib.call('ltu_thin_simple_codes', _p(codes), _p(flags), n, _s())})['codes']
print(f'ltu_thin_simple_codes on {n} random codes: {med:.3f} ({lo:.3f} - {hi:.3f}) ms, {n / (med * 1e-3):.3e} codes per second, '
      f'{float((flags & 1).float().mean()):.3f} simple', flush=True)
