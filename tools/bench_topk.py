"""What the top-k cross-entropy costs.  Medians of alternated calls (hip events around each call after warm-up) with min - max:
  (a) ltu_loss_topk_fwd / ltu_loss_topk_bwd (csrc/loss_topk.hip), fraction 0.1, at 2 x 128^3 C = 3 and 4 x 512x512x32 C = 2, on a
      random softmax and on a "late training" input (97 % of the voxels with p[label] >= 0.999, half of those exactly 1.0: one
      histogram bin takes half the batch), against ltu_loss_fwd / ltu_loss_bwd on the same tensors (the cost of one streaming pass)
      and against torch.topk on the same vector of per-voxel losses;
      `hot` adds the two inputs that put EVERY voxel into one histogram bin: p[label] == 1.0 everywhere (bin 0) and p[label] == 0
      everywhere (the clamp value -log 1e-6);
  (b) train.GraphedStep at the benchmarked configuration (2 x 128^3, bf16, 3 classes) with and without TopKCELoss at all five levels.
usage: bench_topk.py [kernels|hot|step|all] [repeats]"""
import ctypes
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
FRAC = 0.1


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


def one_bin_input(value):
    def make(B, size, C, seed):
        _, lab = random_input(B, size, C, seed)
        p = torch.full((B,) + size + (C,), (1.0 - value) / (C - 1), device=dev)
        p.scatter_(-1, lab.long().unsqueeze(-1), value)
        return p, lab
    return make


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
    N = B * S
    k = ops.topk_count(FRAC, N)
    lib = _lib.load()
    scratch = torch.empty(lib.ltu_loss_topk_scratch_elems(B, S), device=dev, dtype=torch.int32)
    values, one = torch.empty(3, device=dev), torch.ones(1, device=dev)
    sums = torch.empty(lib.ltu_loss_ws_floats(B, S, C), device=dev)
    base_values, coef = torch.empty(9, device=dev), torch.empty((B, C, 3), device=dev)
    wd = (ctypes.c_float * 5)(0.0, 1.0, 0.0, 0.0, 0.0)
    dp = torch.empty_like(p)
    lvec = -torch.log(p.gather(-1, lab.long().unsqueeze(-1)).clamp(min=1e-6)).reshape(-1) + 0.0

    def topk_fwd():
        _lib.call('ltu_loss_topk_fwd', _p(p), _p(lab), _p(scratch), scratch.numel(), _p(values), 0, 1.0, FRAC, 0, 0, B, S, C, _s())

    def topk_bwd():          # into the gradient the base backward wrote, as in the step
        _lib.call('ltu_loss_topk_bwd', _p(p), _p(lab), _p(scratch), scratch.numel(), 1.0, 0, _p(one), _p(dp), 1, B, S, C, _s())

    def topk_bwd_alone():
        _lib.call('ltu_loss_topk_bwd', _p(p), _p(lab), _p(scratch), scratch.numel(), 1.0, 0, _p(one), _p(dp), 0, B, S, C, _s())

    def base_fwd():
        _lib.call('ltu_loss_fwd', _p(p), _p(lab), _p(sums), sums.numel(), _p(base_values), _p(coef), B, S, C, 1.0, 0.0, wd, 0, _s())

    def base_bwd():
        _lib.call('ltu_loss_bwd', _p(p), _p(lab), _p(coef), _p(one), _p(dp), B, S, C, _s())

    def torch_topk():
        return torch.topk(lvec, k, sorted=False)[0].mean()

    base_fwd(); base_bwd(); topk_fwd()
    ref = torch_topk().item()
    f, b, ba, bf, bb, tt = alternate([topk_fwd, topk_bwd, topk_bwd_alone, base_fwd, base_bwd, torch_topk])
    tag = f'{B} x {size[0]}x{size[1]}x{size[2]}, C = {C}, {kind}'
    print(f'(a) {tag}: k = {k}, value {values[1].item():.6f} (torch.topk mean {ref:.6f}), tau {values[2].item():.6e}', flush=True)
    print(f'    ltu_loss_topk_fwd {fmt(f)}; ltu_loss_fwd {fmt(bf)}; ratio {f[0] / bf[0]:.2f} (bytes predict {(4 * C + 1 + 12) / (4 * C + 1):.2f}); '
          f'torch.topk on the loss vector {fmt(tt)}, {tt[0] / f[0]:.1f}x', flush=True)
    print(f'    ltu_loss_topk_bwd accumulate {fmt(b)}, alone {fmt(ba)}; ltu_loss_bwd {fmt(bb)}; ratio {b[0] / bb[0]:.2f}', flush=True)
    return f[0], b[0]


if what in ('kernels', 'hot', 'all'):
    kinds = [('random softmax', random_input), ('late training', late_input)]
    if what == 'hot':
        kinds += [('every p[label] == 1', one_bin_input(1.0)), ('every p[label] == 0', one_bin_input(0.0))]
    for B, size, C in ((2, (128, 128, 128), 3), (4, (512, 512, 32), 2)):
        t = {}
        for kind, make in kinds:
            p, lab = make(B, size, C, 7)
            t[kind] = kernels(B, size, C, kind, p, lab)
            del p, lab
        for kind, _ in kinds[2:]:
            print(f'    {kind} / random softmax: forward {t[kind][0] / t["random softmax"][0]:.2f}, backward '
                  f'{t[kind][1] / t["random softmax"][1]:.2f}', flush=True)
        print(f'    late training / random softmax: forward {t["late training"][0] / t["random softmax"][0]:.2f}, backward '
              f'{t["late training"][1] / t["random softmax"][1]:.2f}', flush=True)

if what in ('step', 'all'):
    size, batch = (128, 128, 128), 2
    weights = train.get_dynamic_weight(1)[0]
    names, cw = ('CrossEntroLoss', 'DiceClassLoss', 'DiceClassLoss2'), [10, 1, 2]
    steps = []
    for topk in (False, True):
        torch.manual_seed(1234)
        model = get_model_dict('MaskTransUnet')([16, 32, 64, 128, 256], [100, 65, 40, 25, 10], [False, True, True, True, True], 1, 3,
                                                dropout=0.3, act_dtype=torch.bfloat16).to(dev).train()
        red = train.GradReducer(model, bucket_mb=32.0, unused=train.UNUSED_PARAMETERS)
        x, lab = data.synthetic_patches(batch, size, 100, dev, n_classes=3)
        if topk:
            specs = train.level_specs(5, names + ('TopKCELoss',), criterion_weight=cw + [1])
        else:
            specs = train.level_specs(5, names, criterion_weight=cw)
        g = train.GraphedStep(model, x, lab, weights, red, specs=specs, topk_fraction=FRAC)
        steps.append((g, x, lab))
    a, b = alternate([lambda s=s: s[0](s[1], s[2]) for s in steps])
    print(f'(b) GraphedStep 2 x 128^3, bf16, 3 classes: without the term {fmt(a)}; with TopKCELoss at five levels {fmt(b)}; difference of '
          f'the medians {b[0] - a[0]:+.3f} ms', flush=True)
