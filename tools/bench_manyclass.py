"""Cost of training with 8 classes next to 3, on the reference configuration (channels [16, 32, 64, 128, 256], 2 x 128^3, bf16).

(a) the label-sized kernels alone, C = 8 next to C = 3 in one process, alternated: the level-0 loss (forward, backward), the final
    head (forward, backward) and the level-1 mask head (forward, backward).  Device events around each call after warm-up, median
    of the repeats; achieved bytes/s from the algorithmic bytes (every operand read or written once, computed below).  The
    C = 3 instantiation of the same run is the yardstick.  Kernel-only times come from a separate `rocprofv3 --kernel-trace
    --stats -- python tools/bench_manyclass.py --kernels` run: the event times here include the launch of one to two kernels.
(b) the whole step: train.GraphedStep at C = 8 against C = 3 (the configuration of `bench.py --classes 3`), ms per step and peak
    memory, and the bytes of the label-sized tensors ([B, S, C] fp32 probabilities and their gradients at every level).

usage: bench_manyclass.py [--kernels] [--step] [--size 128] [--batch 2] [--reps 20]      (neither flag: both parts)
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import data, ops, train  # noqa: E402
from lintransunet_amd.model import get_model_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--kernels', action='store_true')
ap.add_argument('--step', action='store_true')
ap.add_argument('--size', type=int, default=128)
ap.add_argument('--batch', type=int, default=2)
ap.add_argument('--reps', type=int, default=20)
args = ap.parse_args()
both = not (args.kernels or args.step)
dev = torch.device('cuda')
B, N = args.batch, args.size
CLASSES = (3, 8)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def names(C):
    return ['CrossEntroLoss', 'DiceClassLoss'] + [f'DiceClassLoss{c}' for c in range(2, C)]


def kernel_cases(C):
    """name -> (callable, algorithmic bytes) of the six label-sized passes at C classes"""
    g = torch.Generator(device=dev).manual_seed(C)
    S0 = N * N * N                                   # level 0: the full lattice
    p0 = torch.softmax(torch.randn(B, S0, C, device=dev, generator=g), -1).contiguous()
    lab0 = torch.randint(0, C, (B, S0), device=dev, generator=g).to(torch.uint8)
    wd = [0.0] + [1.0] * (C - 1) + [0.0]
    loss = (lambda p, l: ops.level_loss(p, l, 10.0, 0.0, wd[:C] + [0.0] * (4 - C) + [0.0])) if C <= 4 else \
           (lambda p, l: ops.level_loss_wide(p, l, 10.0, 0.0, wd))
    pg = p0.clone().requires_grad_(True)
    tot, _ = loss(pg, lab0)
    one = torch.ones((), device=dev)
    # final head: z bf16 [B, N/2, N/2, N, cop], cop = 4C rounded up to 8
    cop = (4 * C + 7) // 8 * 8
    zf = torch.randn(B, N // 2, N // 2, N, cop, device=dev, generator=g).bfloat16().requires_grad_(True)
    pf = ops.final_softmax(zf, C)
    gf = torch.randn(pf.shape, device=dev, generator=g)
    # level-1 mask head: logits bf16 [B, N/4, N/4, N, 32] (the conv pair pads the head to 32 columns)
    M1 = B * (N // 4) * (N // 4) * N
    zh = torch.randn(M1, 32, device=dev, generator=g).bfloat16().requires_grad_(True)
    ph = ops.head_softmax(zh, C)
    gh = torch.randn(ph.shape, device=dev, generator=g)
    M0 = B * S0
    return {
        'loss_fwd_l0': (lambda: loss(p0, lab0), M0 * (4 * C + 1)),                                   # p, label
        'loss_bwd_l0': (lambda: torch.autograd.grad(tot, pg, one, retain_graph=True), M0 * (8 * C + 1)),      # p, label, dp
        'final_fwd': (lambda: ops.final_softmax(zf.detach(), C), M0 // 4 * cop * 2 + M0 * 4 * C),    # z, p
        'final_bwd': (lambda: torch.autograd.grad(pf, zf, gf, retain_graph=True), M0 * 8 * C + M0 // 4 * cop * 2),      # dp, p, dz
        'head_fwd_l1': (lambda: ops.head_softmax(zh.detach(), C), M1 * (16 + 4 * C)),                # the row's first 8 logits, p
        'head_bwd_l1': (lambda: torch.autograd.grad(ph, zh, gh, retain_graph=True), M1 * (8 * C + 64)),       # dp, p, dz
    }


if both or args.kernels:
    cases = {C: kernel_cases(C) for C in CLASSES}
    times = {C: {k: [] for k in cases[C]} for C in CLASSES}
    rounds = 4
    for _ in range(rounds):                          # alternated: C = 3 and C = 8 see the same machine state
        for C in CLASSES:
            for k, (fn, _) in cases[C].items():
                times[C][k] += timed(fn, max(1, args.reps // rounds))
    for k in cases[CLASSES[0]]:
        row = {'part': 'kernel', 'pass': k, 'shape': f'{B}x{N}^3 bf16'}
        for C in CLASSES:
            t, nb = times[C][k], cases[C][k][1]
            med = statistics.median(t)
            row[f'C{C}'] = {'ms': round(med, 4), 'min_ms': round(min(t), 4), 'max_ms': round(max(t), 4), 'MB': round(nb / 1e6, 1),
                            'TB_per_s': round(nb / med / 1e9, 3)}
        row['C8_over_C3_bytes_per_s'] = round(row['C8']['TB_per_s'] / row['C3']['TB_per_s'], 3)
        print(json.dumps(row), flush=True)
    del cases
    torch.cuda.empty_cache()

if both or args.step:
    weights = train.get_dynamic_weight(1)[0]
    res = {}
    steps = {}
    for C in CLASSES:
        torch.manual_seed(1234)
        model = get_model_dict('MaskTransUnet')([16, 32, 64, 128, 256], [100, 65, 40, 25, 10], [False, True, True, True, True],
                                                1, C, dropout=0.3, act_dtype=torch.bfloat16).to(dev).train()
        red = train.GradReducer(model, bucket_mb=32.0, unused=train.UNUSED_PARAMETERS)
        x, lab = data.synthetic_patches(B, (N, N, N), 100, dev, n_classes=C)
        cw = [10.0, 1.0, 2.0] if C == 3 else [10.0] + [1.0] * (C - 1)
        specs = train.level_specs(5, tuple(names(C)), criterion_weight=cw)
        torch.cuda.reset_peak_memory_stats(dev)
        steps[C] = (train.GraphedStep(model, x, lab, weights, red, specs=specs), x, lab)
        steps[C][0](x, lab)
        torch.cuda.synchronize()
        res[C] = {'peak_memory_gb': round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 3), 't': []}
    for _ in range(4):
        for C in CLASSES:
            step, x, lab = steps[C]
            res[C]['t'] += timed(lambda: step(x, lab), max(1, args.reps // 4))
    # label-sized tensors of one step: probabilities and their gradients, fp32 [B, S_l, C] at the five levels
    S = [N ** 3, N ** 3 // 4, N ** 3 // 16, N ** 3 // 128, N ** 3 // 512]
    for C in CLASSES:
        t = res[C].pop('t')
        res[C].update(ms_per_step=round(statistics.median(t), 3), min_ms=round(min(t), 3), max_ms=round(max(t), 3),
                      label_sized_MB=round(2 * 4 * C * B * sum(S) / 1e6, 1))
    print(json.dumps({'part': 'step', 'shape': f'{B}x{N}^3 bf16, GraphedStep', 'C3': res[3], 'C8': res[8],
                      'extra_ms': round(res[8]['ms_per_step'] - res[3]['ms_per_step'], 3),
                      'extra_label_sized_MB': round(res[8]['label_sized_MB'] - res[3]['label_sized_MB'], 1)}), flush=True)
