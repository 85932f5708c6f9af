"""The optimizer step at the full configuration (channels [16, 32, 64, 128, 256], 20.87 M parameters) on the reducer's real bucket
layout: the plain step (ltu_adamw per bucket) against the guarded step of csrc/optim.hip (sum of squares per bucket + guard +
guarded update per bucket) as guard only (skip_nonfinite), guard + clip, and guard + clip + EMA.  Four optimizers share one
reducer (each owns its parameter / moment / EMA buffers, 0.33 - 0.42 GB, more than the 256 MB cache: no variant finds its
operands resident), warmed up, then alternated in one process; each step is timed by device events and queued behind a spin
kernel, so the events bracket back-to-back device work and not the host's launch latency.  Medians, the ratio to the plain step and
the bandwidth of the bytes the shapes make a step move (plain 7 words per parameter, guard 8, with EMA 10).
One JSON line per variant.  usage: bench_optim.py [repeats]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import optim, train  # noqa: E402
from lintransunet_amd.model import get_model_dict  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
SLEEP_CYCLES = 2_000_000
VARIANTS = {'plain': (dict(), 7), 'guard': (dict(skip_nonfinite=True), 8),
            'guard+clip': (dict(skip_nonfinite=True, max_grad_norm=1.0), 8),
            'guard+clip+ema': (dict(skip_nonfinite=True, max_grad_norm=1.0, ema_decay=0.999), 10)}


def main():
    dev = torch.device('cuda')
    torch.manual_seed(0)
    model = get_model_dict('MaskTransUnet')([16, 32, 64, 128, 256], [100, 65, 40, 25, 10], [False, True, True, True, True], 1, 2).to(dev)
    reducer = train.GradReducer(model, unused=train.UNUSED_PARAMETERS)
    n = sum(f.numel() for f in reducer.flat)
    for f in reducer.flat:
        f.copy_(2e-3 * torch.randn(f.numel(), device=dev))          # norm about 9: the clipped branch
    opts = {k: optim.FusedAdamW(reducer, lr=1e-4, **kw) for k, (kw, _) in VARIANTS.items()}
    for opt in opts.values():          # warm-up of every variant
        for _ in range(5):
            opt.step()
    torch.cuda.synchronize()
    ev = {k: [] for k in opts}
    for _ in range(reps):              # alternated in one process
        for k, opt in opts.items():
            torch.cuda._sleep(SLEEP_CYCLES)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            opt.step()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    us = {k: statistics.median(a.elapsed_time(b) for a, b in v) * 1e3 for k, v in ev.items()}
    for k, (kw, words) in VARIANTS.items():
        opt = opts[k]
        print(json.dumps({'variant': k, 'parameters': n, 'buckets': [f.numel() for f in reducer.flat],
                          'launches': len(reducer.flat) * (2 if opt.guarded else 1) + (1 if opt.guarded else 0),
                          'us': round(us[k], 1), 'ratio_to_plain': round(us[k] / us['plain'], 3), 'byte_ratio': round(words / 7, 3),
                          'GBps': round(4 * words * n / us[k] / 1e3, 1), 'counters': list(opt.counters()),
                          'grad_norm': round(opt.grad_norm.item(), 4) if opt.guarded else None}))


if __name__ == '__main__':
    main()
