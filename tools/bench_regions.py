"""What region-based training costs (csrc/region.hip, the sigmoid heads of csrc/pointwise.hip).  Medians of alternated calls (hip
events around each call after warm-up) with min - max:
  (a) ltu_loss_region_fwd / ltu_loss_region_bwd (BCE + Dice on batch sums) beside ltu_loss_imb_fwd / ltu_loss_imb_bwd (two Tversky
      terms and the focal cross-entropy) on the same tensors, at 2 x 128^3 with R = 3 and 4 x 512x512x32 with R = 2: the same bytes
      (p and one byte a voxel forward; p, the byte and dp backward), so the expectation is a ratio of 1;
  (b) the sigmoid heads beside the softmax heads: the mask head on bf16 rows padded to 16 columns and the final head at the
      benchmarked step's shape, forward and backward;
  (c) ops.region_bits plus its OR-pooled pyramid (train.region_pyramid) beside train.label_pyramid on the same label patch;
  (d) train.GraphedStep at the benchmarked configuration (2 x 128^3, bf16): 3 regions (Regions.brats(), BCE + Dice at five levels)
      against 3 classes with CE + Dice + Dice2.
usage: bench_regions.py [kernels|heads|pyramid|step|all] [repeats]"""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data, losses, ops, train  # noqa: E402
from lintransunet_amd.model import get_model_dict  # noqa: E402
from lintransunet_amd.ops import _p, _s  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else 'all'
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev = torch.device('cuda')


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
    return f'{t[0]:.3f} ms ({t[1]:.3f} - {t[2]:.3f})'


def stage(B, size, R):
    S = size[0] * size[1] * size[2]
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(7)
    p = torch.rand((B,) + size + (R,), device=dev, generator=g)
    bits = torch.randint(0, 1 << R, (B,) + size, device=dev, generator=g, dtype=torch.uint8)
    lab = torch.randint(0, R, (B,) + size, device=dev, generator=g, dtype=torch.uint8)
    one = torch.ones(1, device=dev)
    dp = torch.empty_like(p)
    rsums = torch.empty(lib.ltu_loss_region_ws_floats(B, S, R), device=dev)
    rvalues, rcoef = torch.empty(R + 4, device=dev), torch.empty((B, R, 3), device=dev)
    isums = torch.empty(lib.ltu_loss_imb_ws_floats(B, S, R), device=dev)
    ivalues, icoef = torch.empty(5, device=dev), torch.empty((B, R, 3), device=dev)
    cls, wv = (ctypes.c_int * 2)(1, 0), (ctypes.c_float * 2)(1.0, 1.0)
    params = (ctypes.c_float * 5)(0.5, 0.5, 1.0, 1e-5, 1.0)

    def reg_fwd():
        _lib.call('ltu_loss_region_fwd', _p(p), _p(bits), _p(rsums), rsums.numel(), _p(rvalues), _p(rcoef), 0, 1.0, 1.0, 1, 1e-5, 0, B, S, R, _s())

    def reg_bwd():
        _lib.call('ltu_loss_region_bwd', _p(p), _p(bits), _p(rcoef), rcoef.numel(), _p(one), _p(dp), 0, B, S, R, _s())

    def imb_fwd():
        _lib.call('ltu_loss_imb_fwd', _p(p), _p(lab), _p(isums), isums.numel(), _p(ivalues), _p(icoef), 0, cls, wv, 2, params, 1.0, 0.0, None,
                  0, B, S, R, _s())

    def imb_bwd():
        _lib.call('ltu_loss_imb_bwd', _p(p), _p(lab), _p(icoef), icoef.numel(), 0.0, _p(one), _p(dp), 0, B, S, R, _s())

    rf, rb, jf, jb = alternate([reg_fwd, reg_bwd, imb_fwd, imb_bwd])
    gf, gb = B * S * (4 * R + 1) / 1e9, B * S * (8 * R + 1) / 1e9
    print(f'(a) {B} x {size[0]}x{size[1]}x{size[2]}, R = {R}: BCE {rvalues[1].item():.6f}, Dice {rvalues[2].item():.6f}', flush=True)
    print(f'    ltu_loss_region_fwd {fmt(rf)} ({gf / rf[0] * 1e3:.0f} GB/s); ltu_loss_imb_fwd {fmt(jf)}; ratio {rf[0] / jf[0]:.2f}', flush=True)
    print(f'    ltu_loss_region_bwd {fmt(rb)} ({gb / rb[0] * 1e3:.0f} GB/s); ltu_loss_imb_bwd {fmt(jb)}; ratio {rb[0] / jb[0]:.2f}', flush=True)


def heads():
    g = torch.Generator(device=dev).manual_seed(9)
    B, R = 2, 3
    M, CP = B * 64 * 64 * 128, 16                                    # level 0 of the benchmarked step: rows padded to 16 columns
    z = torch.randn((M, CP), device=dev, generator=g).bfloat16()
    p, gp, dz = torch.empty((M, R), device=dev), torch.randn((M, R), device=dev, generator=g), torch.empty_like(z)
    zf = torch.randn((B, 64, 64, 128, 16), device=dev, generator=g).bfloat16()      # the final head: 4 R = 12 columns padded to 16
    pf = torch.empty((B, 128, 128, 128, R), device=dev)
    gf, dzf = torch.randn(pf.shape, device=dev, generator=g), torch.empty_like(zf)

    def head(kind, d):
        if d == 'fwd':
            return lambda: _lib.call(f'ltu_head_{kind}_fwd', _p(z), _p(p), M, R, CP, ops.BF16, _s())
        return lambda: _lib.call(f'ltu_head_{kind}_bwd', _p(gp), _p(p), _p(dz), M, R, CP, ops.BF16, _s())

    def final(kind, d):
        if d == 'fwd':
            return lambda: _lib.call(f'ltu_final_{kind}_fwd', _p(zf), _p(pf), B, 64, 64, 128, R, 16, ops.BF16, _s())
        return lambda: _lib.call(f'ltu_final_{kind}_bwd', _p(gf), _p(pf), _p(dzf), B, 64, 64, 128, R, 16, ops.BF16, _s())

    names = [(fn, kind, d) for fn in (head, final) for d in ('fwd', 'bwd') for kind in ('sigmoid', 'softmax')]
    ts = alternate([fn(kind, d) for fn, kind, d in names])
    for k in range(0, len(names), 2):
        fn, _, d = names[k]
        print(f'(b) {fn.__name__} {d}, bf16, R = C = 3, {B} x 128^3: sigmoid {fmt(ts[k])}; softmax {fmt(ts[k + 1])}; ratio '
              f'{ts[k][0] / ts[k + 1][0]:.2f}', flush=True)


def pyramid():
    _, lab = data.synthetic_patches(2, (128, 128, 128), 100, dev, n_classes=4)
    rec = losses.Regions.brats()
    a, b = alternate([lambda: train.region_pyramid(lab, rec, 5), lambda: train.label_pyramid(lab, 5)])
    print(f'(c) 2 x 128^3 label patch, five levels: region_bits + OR-pooled pyramid {fmt(a)}; label_pyramid {fmt(b)}; difference of the '
          f'medians {a[0] - b[0]:+.3f} ms', flush=True)


def step():
    size, batch = (128, 128, 128), 2
    weights = train.get_dynamic_weight(1)[0]
    steps = []
    for rec in (None, losses.Regions.brats()):
        torch.manual_seed(1234)
        model = get_model_dict('MaskTransUnet')([16, 32, 64, 128, 256], [100, 65, 40, 25, 10], [False, True, True, True, True], 1, 3,
                                                dropout=0.3, act_dtype=torch.bfloat16, regions=rec).to(dev).train()
        red = train.GradReducer(model, bucket_mb=32.0, unused=train.UNUSED_PARAMETERS)
        if rec is None:
            x, lab = data.synthetic_patches(batch, size, 100, dev, n_classes=3)
            specs = train.level_specs(5, ('CrossEntroLoss', 'DiceClassLoss', 'DiceClassLoss2'), criterion_weight=[10, 1, 2])
        else:
            x, lab = data.synthetic_patches(batch, size, 100, dev, n_classes=4)
            specs = train.level_specs(5, train.REGION_CRITERIA, criterion_weight=[1, 1])
        steps.append((train.GraphedStep(model, x, lab, weights, red, specs=specs), x, lab))
    a, b = alternate([lambda s=s: s[0](s[1], s[2]) for s in steps])
    print(f'(d) GraphedStep 2 x 128^3, bf16: 3 classes, CE + Dice + Dice2 {fmt(a)}; 3 regions, BCE + Dice {fmt(b)}; difference of the '
          f'medians {b[0] - a[0]:+.3f} ms', flush=True)


if what in ('kernels', 'all'):
    stage(2, (128, 128, 128), 3)
    stage(4, (512, 512, 32), 2)
if what in ('heads', 'all'):
    heads()
if what in ('pyramid', 'all'):
    pyramid()
if what in ('step', 'all'):
    step()
