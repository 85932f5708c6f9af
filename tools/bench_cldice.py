"""What soft-clDice costs (csrc/softmorph.hip).  Medians of alternated calls (hip events around each call after warm-up) with min - max:
  (a) ops.soft_skeleton forward and backward, ops.label_skeletons, and the stage alone (ltu_loss_cldice_fwd / _bwd, one term), at
      2 x 128^3 and 4 x 512x512x32 with 3 and 10 iterations, each beside the eager-torch composition of the published code on the same
      tensors (max_pool3d, autograd), with the bytes per voxel the kernels move against the time;
  (b) train.GraphedStep at the benchmarked configuration (2 x 128^3, bf16, 3 classes) without the name, with 'ClDiceLoss' at level 0,
      and with it at all five levels.
usage: bench_cldice.py [kernels|step|all] [repeats]"""
import ctypes
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data, ops, train  # noqa: E402
from lintransunet_amd.model import get_model_dict  # noqa: E402
from lintransunet_amd.ops import _p, _s  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else 'all'
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev = torch.device('cuda')


# the published composition (Shit et al., soft_skeleton.py), on [N,1,H,W,D]
def t_erode(x):
    p1 = -F.max_pool3d(-x, (3, 1, 1), (1, 1, 1), (1, 0, 0))
    p2 = -F.max_pool3d(-x, (1, 3, 1), (1, 1, 1), (0, 1, 0))
    p3 = -F.max_pool3d(-x, (1, 1, 3), (1, 1, 1), (0, 0, 1))
    return torch.min(torch.min(p1, p2), p3)


def t_open(x):
    return F.max_pool3d(t_erode(x), (3, 3, 3), (1, 1, 1), (1, 1, 1))


def t_skeleton(x, iters):
    skel = F.relu(x - t_open(x))
    for _ in range(iters):
        x = t_erode(x)
        delta = F.relu(x - t_open(x))
        skel = skel + F.relu(delta - skel * delta)
    return skel


def t_cldice(P, G, iters):
    SP, SG = t_skeleton(P, iters), t_skeleton(G, iters)
    tprec = ((SP * G).sum() + 1.0) / (SP.sum() + 1.0)
    tsens = ((SG * P).sum() + 1.0) / (SG.sum() + 1.0)
    return 1.0 - 2.0 * tprec * tsens / (tprec + tsens)


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


def kernels(B, size, iters):
    H, W, D = size
    S, C = H * W * D, 2
    g = torch.Generator(device=dev).manual_seed(7)
    p = torch.softmax(1.5 * torch.randn((B,) + size + (C,), device=dev, generator=g), -1)
    lab = (torch.rand((B,) + size, device=dev, generator=g) < 0.3).to(torch.uint8)
    x = p[..., 1].contiguous()
    gout = torch.randn(x.shape, device=dev, generator=g)
    lib = _lib.load()
    L = iters + 1
    # the operators through the C-ABI: the scratch is allocated once, as a captured step holds it
    scratch = torch.empty(lib.ltu_soft_skeleton_scratch_elems(B, H, W, D, iters), device=dev)
    y, dx = torch.empty_like(x), torch.empty_like(x)

    def skel_fwd():
        _lib.call('ltu_soft_skeleton_fwd', _p(x), _p(y), _p(scratch), scratch.numel(), B, H, W, D, iters, _s())

    def skel_bwd():
        _lib.call('ltu_soft_skeleton_bwd', _p(x), _p(gout), _p(dx), _p(scratch), scratch.numel(), B, H, W, D, iters, _s())

    cls, wv = (ctypes.c_int * 1)(1), (ctypes.c_float * 1)(1.0)
    skel = torch.empty((B, 1) + size, device=dev, dtype=torch.uint8)

    def label_skel():
        _lib.call('ltu_label_skeletons', _p(lab), cls, 1, _p(skel), B, H, W, D, iters, _s())

    need = lib.ltu_loss_cldice_scratch_elems(B, H, W, D, 1, iters)
    sscratch = torch.empty((need + 1) // 2, device=dev, dtype=torch.float64).view(torch.float32)
    values, one, dp = torch.empty(2, device=dev), torch.ones(1, device=dev), torch.empty_like(p)

    def stage_fwd():
        _lib.call('ltu_loss_cldice_fwd', _p(p), _p(lab), _p(skel), cls, wv, 1, iters, _p(sscratch), sscratch.numel(), _p(values), 0, 0,
                  B, H, W, D, C, _s())

    def stage_bwd():
        _lib.call('ltu_loss_cldice_bwd', _p(p), _p(lab), cls, 1, iters, _p(sscratch), sscratch.numel(), _p(one), _p(dp), 0, B, H, W, D, C, _s())

    # the torch composition: forward alone (no graph kept), and forward + backward
    xt = x.unsqueeze(1).requires_grad_(True)
    G = (lab == 1).float().unsqueeze(1)
    pt = p.clone().requires_grad_(True)

    def torch_skel_fwd():
        with torch.no_grad():
            t_skeleton(xt, iters)

    def torch_skel_fwd_bwd():
        xt.grad = None
        t_skeleton(xt, iters).backward(gout.unsqueeze(1))

    def torch_label_skel():
        with torch.no_grad():
            t_skeleton(G, iters)

    def torch_stage_fwd():
        with torch.no_grad():
            t_cldice(pt[..., 1].unsqueeze(1), G, iters)

    def torch_stage_fwd_bwd():
        pt.grad = None
        t_cldice(pt[..., 1].unsqueeze(1), G, iters).backward()

    label_skel()
    sf, sb, ls, gf, gb, tf, tfb, tl, tsf, tsfb = alternate([skel_fwd, skel_bwd, label_skel, stage_fwd, stage_bwd, torch_skel_fwd,
                                                            torch_skel_fwd_bwd, torch_label_skel, torch_stage_fwd, torch_stage_fwd_bwd])
    tag = f'{B} x {H}x{W}x{D}, iters {iters}'
    vox = B * S
    # bytes the kernels read and write per voxel, neighbour taps counted once (they come from cache): forward per iteration erode 4 + 5,
    # dilate-update 4 + 4 + 4 + 5; backward point pass (8 + 1) L + 4 + 4 L, gather per level about 4 + 4 + 1 + 1 + 4
    fb, bb = 26 * L, 13 * L + 4 + 14 * (L + 1)
    print(f'(a) {tag}', flush=True)
    print(f'    soft_skeleton forward {fmt(sf)} ({fb} B/voxel, {vox * fb / sf[0] / 1e6:.0f} GB/s); torch {fmt(tf)}; torch / ours {tf[0] / sf[0]:.2f}', flush=True)
    print(f'    soft_skeleton backward {fmt(sb)} ({bb} B/voxel, {vox * bb / sb[0] / 1e6:.0f} GB/s); forward + backward {sf[0] + sb[0]:.3f} ms against torch '
          f'{fmt(tfb)}; torch / ours {tfb[0] / (sf[0] + sb[0]):.2f}', flush=True)
    print(f'    label_skeletons {fmt(ls)}; torch on the float map {fmt(tl)}; torch / ours {tl[0] / ls[0]:.2f}', flush=True)
    print(f'    stage forward {fmt(gf)}, backward {fmt(gb)} (value {values[1].item():.6f}); torch forward {fmt(tsf)}, forward + backward {fmt(tsfb)}; '
          f'torch / ours {tsf[0] / gf[0]:.2f} forward, {tsfb[0] / (gf[0] + gb[0]):.2f} forward + backward (torch skeletonises the label too)', flush=True)


if what in ('kernels', 'all'):
    for B, size in ((2, (128, 128, 128)), (4, (512, 512, 32))):
        for iters in (3, 10):
            kernels(B, size, iters)
            torch.cuda.empty_cache()

if what in ('step', 'all'):
    size, batch = (128, 128, 128), 2
    weights = train.get_dynamic_weight(1)[0]
    names, cw = ('CrossEntroLoss', 'DiceClassLoss', 'DiceClassLoss2'), [10, 1, 2]
    plain = train.level_specs(5, names, criterion_weight=cw)
    level0 = list(plain)
    level0[-1] = dict(plain[-1], ClDiceLoss=1.0)           # deep_supervision_loss reads specs[-lvl - 1]: the last spec is level 0's
    every = [dict(spec, ClDiceLoss=1.0) for spec in plain]
    steps = []
    for specs in (plain, level0, every):
        torch.manual_seed(1234)
        model = get_model_dict('MaskTransUnet')([16, 32, 64, 128, 256], [100, 65, 40, 25, 10], [False, True, True, True, True], 1, 3,
                                                dropout=0.3, act_dtype=torch.bfloat16).to(dev).train()
        red = train.GradReducer(model, bucket_mb=32.0, unused=train.UNUSED_PARAMETERS)
        x, lab = data.synthetic_patches(batch, size, 100, dev, n_classes=3)
        steps.append((train.GraphedStep(model, x, lab, weights, red, specs=specs, cldice_iters=3), x, lab))
    a, b, c = alternate([lambda s=s: s[0](s[1], s[2]) for s in steps])
    print(f'(b) GraphedStep 2 x 128^3, bf16, 3 classes, 3 iterations: without the name {fmt(a)}; ClDiceLoss at level 0 {fmt(b)} ({b[0] - a[0]:+.3f} ms); '
          f'at all five levels {fmt(c)} ({c[0] - a[0]:+.3f} ms)', flush=True)
