"""What the imbalance stage of the level loss costs (csrc/loss_imbalance.hip: Tversky, focal Tversky, focal cross-entropy).  Medians
of alternated calls (hip events around each call after warm-up) with min - max:
  (a) ltu_loss_imb_fwd / ltu_loss_imb_bwd alone (two Tversky terms at gamma 4/3 plus the focal cross-entropy at gamma 2), at
      2 x 128^3 C = 3 and 4 x 512x512x32 C = 2, on a random softmax and on a "late training" input, beside ltu_loss_fwd /
      ltu_loss_bwd on the same tensors (the same bytes: p and label once forward, p, label and dp backward);
  (b) FocalCELoss at gamma 0 (the plain mean cross-entropy) beside TopKCELoss at fraction 1.0 (the same number through three
      histogram passes and a radix select), forward and backward, on the same tensors;
  (c) train.GraphedStep at the benchmarked configuration (2 x 128^3, bf16, 3 classes) with and without FocalCELoss, TverskyLoss and
      TverskyLoss2 at all five levels.
usage: bench_imbalance.py [kernels|step|all] [repeats]"""
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


def random_input(B, size, C, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    p = torch.softmax(1.5 * torch.randn((B,) + size + (C,), device=dev, generator=g), -1)
    lab = torch.randint(0, C, (B,) + size, device=dev, generator=g, dtype=torch.uint8)
    return p, lab


def late_input(B, size, C, seed):
    """97 % of the voxels with p[label] >= 0.999, half of those exactly 1.0; the other 3 % keep the random softmax"""
    p, lab = random_input(B, size, C, seed)
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    u = torch.rand(lab.shape, device=dev, generator=g)
    pl = torch.where(u < 0.485, torch.ones_like(u), 0.999 + 0.001 * torch.rand(lab.shape, device=dev, generator=g).clamp(max=0.999))
    easy = torch.zeros_like(p).add_(((1.0 - pl) / (C - 1)).unsqueeze(-1))
    easy.scatter_(-1, lab.long().unsqueeze(-1), pl.unsqueeze(-1))
    p = torch.where((u < 0.97).unsqueeze(-1), easy, p)
    return p.contiguous(), lab


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


def kernels(B, size, C, kind, p, lab):
    S = size[0] * size[1] * size[2]
    lib = _lib.load()
    one = torch.ones(1, device=dev)
    dp = torch.empty_like(p)
    # the stage
    isums = torch.empty(lib.ltu_loss_imb_ws_floats(B, S, C), device=dev)
    ivalues, icoef = torch.empty(5, device=dev), torch.empty((B, C, 3), device=dev)
    cls, wv = (ctypes.c_int * 2)(1, 0), (ctypes.c_float * 2)(1.0, 1.0)
    params = (ctypes.c_float * 5)(0.3, 0.7, 4.0 / 3.0, 1e-5, 0.0)
    # the base loss
    sums = torch.empty(lib.ltu_loss_ws_floats(B, S, C), device=dev)
    base_values, coef = torch.empty(9, device=dev), torch.empty((B, C, 3), device=dev)
    wd = (ctypes.c_float * 5)(0.0, 1.0, 0.0, 0.0, 0.0)
    # focal at gamma 0 and top-k at fraction 1
    fvalues, fcoef = torch.empty(3, device=dev), torch.empty((B, C, 3), device=dev)
    none = (ctypes.c_float * 5)(0.3, 0.7, 1.0, 1e-5, 0.0)
    scratch = torch.empty(lib.ltu_loss_topk_scratch_elems(B, S), device=dev, dtype=torch.int32)
    tvalues = torch.empty(3, device=dev)

    def imb_fwd():
        _lib.call('ltu_loss_imb_fwd', _p(p), _p(lab), _p(isums), isums.numel(), _p(ivalues), _p(icoef), 0, cls, wv, 2, params, 1.0, 2.0, None,
                  0, B, S, C, _s())

    def imb_bwd():
        _lib.call('ltu_loss_imb_bwd', _p(p), _p(lab), _p(icoef), icoef.numel(), 2.0, _p(one), _p(dp), 0, B, S, C, _s())

    def imb_bwd_acc():          # into the gradient an earlier stage wrote, as in a chain
        _lib.call('ltu_loss_imb_bwd', _p(p), _p(lab), _p(icoef), icoef.numel(), 2.0, _p(one), _p(dp), 1, B, S, C, _s())

    def base_fwd():
        _lib.call('ltu_loss_fwd', _p(p), _p(lab), _p(sums), sums.numel(), _p(base_values), _p(coef), B, S, C, 1.0, 0.0, wd, 0, _s())

    def base_bwd():
        _lib.call('ltu_loss_bwd', _p(p), _p(lab), _p(coef), _p(one), _p(dp), B, S, C, _s())

    def ce_fwd():
        _lib.call('ltu_loss_imb_fwd', _p(p), _p(lab), _p(isums), isums.numel(), _p(fvalues), _p(fcoef), 0, None, None, 0, none, 1.0, 0.0, None,
                  0, B, S, C, _s())

    def ce_bwd():
        _lib.call('ltu_loss_imb_bwd', _p(p), _p(lab), _p(fcoef), fcoef.numel(), 0.0, _p(one), _p(dp), 0, B, S, C, _s())

    def topk_fwd():
        _lib.call('ltu_loss_topk_fwd', _p(p), _p(lab), _p(scratch), scratch.numel(), _p(tvalues), 0, 1.0, 1.0, 0, 0, B, S, C, _s())

    def topk_bwd():
        _lib.call('ltu_loss_topk_bwd', _p(p), _p(lab), _p(scratch), scratch.numel(), 1.0, 0, _p(one), _p(dp), 0, B, S, C, _s())

    f, b, ba, bf, bb, cf, cb, tf, tb = alternate([imb_fwd, imb_bwd, imb_bwd_acc, base_fwd, base_bwd, ce_fwd, ce_bwd, topk_fwd, topk_bwd])
    tag = f'{B} x {size[0]}x{size[1]}x{size[2]}, C = {C}, {kind}'
    gb = B * S * (4 * C + 1) / 1e9
    print(f'(a) {tag}: Tversky values {ivalues[1].item():.6f} {ivalues[2].item():.6f}, focal value {ivalues[3].item():.6f}', flush=True)
    print(f'    ltu_loss_imb_fwd {fmt(f)} ({gb / f[0] * 1e3:.0f} GB/s); ltu_loss_fwd {fmt(bf)}; ratio {f[0] / bf[0]:.2f}', flush=True)
    print(f'    ltu_loss_imb_bwd write {fmt(b)}, accumulate {fmt(ba)}; ltu_loss_bwd {fmt(bb)}; ratio {b[0] / bb[0]:.2f} (write), '
          f'{ba[0] / bb[0]:.2f} (accumulate; bytes predict {(12 * C + 1) / (8 * C + 1):.2f})', flush=True)
    print(f'(b) {tag}: mean cross-entropy {fvalues[1].item():.6f} as FocalCELoss at gamma 0, {tvalues[1].item():.6f} as TopKCELoss at '
          f'fraction 1.0', flush=True)
    print(f'    forward {fmt(cf)} against {fmt(tf)}, {tf[0] / cf[0]:.2f}x; backward {fmt(cb)} against {fmt(tb)}, {tb[0] / cb[0]:.2f}x',
          flush=True)


if what in ('kernels', 'all'):
    for B, size, C in ((2, (128, 128, 128), 3), (4, (512, 512, 32), 2)):
        for kind, make in (('random softmax', random_input), ('late training', late_input)):
            p, lab = make(B, size, C, 7)
            kernels(B, size, C, kind, p, lab)
            del p, lab

if what in ('step', 'all'):
    size, batch = (128, 128, 128), 2
    weights = train.get_dynamic_weight(1)[0]
    names, cw = ('CrossEntroLoss', 'DiceClassLoss', 'DiceClassLoss2'), [10, 1, 2]
    rec = losses.Imbalance(alpha=0.3, beta=0.7, tversky_gamma=4.0 / 3.0, batch=True, focal_gamma=2.0)
    steps = []
    for new in (False, True):
        torch.manual_seed(1234)
        model = get_model_dict('MaskTransUnet')([16, 32, 64, 128, 256], [100, 65, 40, 25, 10], [False, True, True, True, True], 1, 3,
                                                dropout=0.3, act_dtype=torch.bfloat16).to(dev).train()
        red = train.GradReducer(model, bucket_mb=32.0, unused=train.UNUSED_PARAMETERS)
        x, lab = data.synthetic_patches(batch, size, 100, dev, n_classes=3)
        if new:
            specs = train.level_specs(5, names + ('FocalCELoss', 'TverskyLoss', 'TverskyLoss2'), criterion_weight=cw + [1, 1, 1])
        else:
            specs = train.level_specs(5, names, criterion_weight=cw)
        g = train.GraphedStep(model, x, lab, weights, red, specs=specs, imbalance=rec)
        steps.append((g, x, lab))
    a, b = alternate([lambda s=s: s[0](s[1], s[2]) for s in steps])
    print(f'(c) GraphedStep 2 x 128^3, bf16, 3 classes: without the names {fmt(a)}; with FocalCELoss, TverskyLoss and TverskyLoss2 at five '
          f'levels {fmt(b)}; difference of the medians {b[0] - a[0]:+.3f} ms', flush=True)
