"""What the boundary loss costs.  Medians of alternated calls (hip events around each call after warm-up) with min - max:
  (a) ops.signed_distance_maps (csrc/distmap.hip, one call for the batch) against the route the library offered before it: a host
      loop of ltu_surface_edt over (sample, class) - one call carries both polarities in its two bit channels, G in bit 0 and
      not-G in bit 1 - plus the torch ops that turn its squared distances into the same phi; on 2 x 128^3 and 4 x 512x512x32, K = 2;
  (b) the boundary forward + backward alone (csrc/loss_boundary.hip) on the same shapes, C = 3;
  (c) train.GraphedStep at the benchmarked configuration (2 x 128^3, bf16, 3 classes) with and without BoundaryLoss + BoundaryLoss2
      at all five levels.
usage: bench_boundary.py [maps|loss|step|all] [repeats]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data, ops, train  # noqa: E402
from lintransunet_amd.model import get_model_dict  # noqa: E402
from lintransunet_amd.ops import _p, _s  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else 'all'
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev = torch.device('cuda')
CLASSES = (1, 2)
SPACING = (0.7, 0.7, 2.5)


def labels(B, size):
    """an organ-sized class 1 and a lesion-sized class 2 per sample"""
    H, W, D = size
    h, w, d = (torch.arange(n, device=dev, dtype=torch.float32) for n in size)
    hh, ww, dd = h[:, None, None], w[None, :, None], d[None, None, :]
    lab = torch.zeros((B,) + size, device=dev, dtype=torch.uint8)
    for b in range(B):
        c = (H * (0.45 + 0.03 * b), W * 0.5, D * 0.5)
        lab[b][((hh - c[0]) / (0.16 * H)) ** 2 + ((ww - c[1]) / (0.09 * W)) ** 2 + ((dd - c[2]) / (0.25 * D)) ** 2 <= 1] = 1
        lab[b][((hh - c[0] - 0.05 * H) / (0.03 * H)) ** 2 + ((ww - c[1]) / (0.025 * W)) ** 2 + ((dd - c[2]) / (0.08 * D)) ** 2 <= 1] = 2
    return lab


def maps_by_surface_edt(lab, scratch, dist):
    """phi [B,K,H,W,D] through ltu_surface_edt, one call per (sample, class) over the whole volume"""
    B, H, W, D = lab.shape
    out = torch.empty((B, len(CLASSES), H, W, D), device=dev, dtype=torch.float32)
    for b in range(B):
        for k, c in enumerate(CLASSES):
            g = lab[b] == c
            edges = g.to(torch.uint8) + 2 * (~g).to(torch.uint8)
            _lib.call('ltu_surface_edt', _p(edges), _p(dist), _p(scratch), scratch.numel(), H, W, D, 0, 0, 0, H, W, D, *SPACING, _s())
            phi = torch.where(g, 1.0 - dist[1].sqrt(), dist[0].sqrt())
            out[b, k] = torch.where(torch.isfinite(phi), phi, torch.zeros_like(phi))
    return out


def alternate(fns):
    """`reps` timed calls of each function, taken in turn; (median, min, max) in ms per function"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[i].append(e0.elapsed_time(e1))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def fmt(t):
    return f'{t[0]:.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})'


for B, size in ((2, (128, 128, 128)), (4, (512, 512, 32))):
    tag = f'{B} x {size[0]}x{size[1]}x{size[2]}, K = {len(CLASSES)}'
    if what in ('maps', 'all'):
        lab = labels(B, size)
        scratch = torch.empty(_lib.load().ltu_surface_ws_elems(*size), device=dev, dtype=torch.int32)
        dist = torch.empty((2,) + size, device=dev, dtype=torch.float32)
        new = ops.signed_distance_maps(lab, CLASSES, SPACING)
        old = maps_by_surface_edt(lab, scratch, dist)
        diff = (new - old).abs().max().item()
        a, b = alternate([lambda: ops.signed_distance_maps(lab, CLASSES, SPACING), lambda: maps_by_surface_edt(lab, scratch, dist)])
        print(f'(a) {tag}: signed_distance_maps {fmt(a)}; loop of ltu_surface_edt + torch {fmt(b)}; {b[0] / a[0]:.2f}x; '
              f'max |difference| {diff:.2e}, max |phi| {new.abs().max().item():.1f}', flush=True)
        del scratch, dist, new, old
    if what in ('loss', 'all'):
        lab = labels(B, size)
        phi = ops.signed_distance_maps(lab, CLASSES, SPACING)
        p = torch.softmax(torch.randn((B,) + size + (3,), device=dev), -1).requires_grad_(True)
        one = torch.ones((), device=dev)

        def loss():
            total, _, _ = ops.level_loss_boundary(p, lab, phi, CLASSES, (0.01, 0.01))
            torch.autograd.backward([total], [one], inputs=[p])
            p.grad = None

        (t,) = alternate([loss])
        print(f'(b) {tag}, C = 3: boundary forward + backward {fmt(t)}', flush=True)
        del phi, p

if what in ('step', 'all'):
    size, batch = (128, 128, 128), 2
    weights = train.get_dynamic_weight(1)[0]
    names, cw = ('CrossEntroLoss', 'DiceClassLoss', 'DiceClassLoss2'), [10, 1, 2]
    steps = []
    for boundary in (False, True):
        torch.manual_seed(1234)
        model = get_model_dict('MaskTransUnet')([16, 32, 64, 128, 256], [100, 65, 40, 25, 10], [False, True, True, True, True], 1, 3,
                                                dropout=0.3, act_dtype=torch.bfloat16).to(dev).train()
        red = train.GradReducer(model, bucket_mb=32.0, unused=train.UNUSED_PARAMETERS)
        x, lab = data.synthetic_patches(batch, size, 100, dev, n_classes=3)
        if boundary:
            specs = train.level_specs(5, names + ('BoundaryLoss', 'BoundaryLoss2'), criterion_weight=cw + [0.01, 0.01])
        else:
            specs = train.level_specs(5, names, criterion_weight=cw)
        g = train.GraphedStep(model, x, lab, weights, red, specs=specs, spacing=SPACING)
        steps.append((g, x, lab))
    a, b = alternate([lambda s=s: s[0](s[1], s[2]) for s in steps])
    print(f'(c) GraphedStep 2 x 128^3, bf16, 3 classes: without boundary terms {fmt(a)}; with BoundaryLoss + BoundaryLoss2 at five levels '
          f'{fmt(b)}; difference of the medians {b[0] - a[0]:+.3f} ms', flush=True)
