"""The wider loss family (csrc/loss_ext.hip) against the original level loss (csrc/loss.hip) on the same inputs: 2 patches of
128^3, C = 2 and C = 3, specs {CE + DiceClass} and {CE + DiceClass + Focal + IoU}.  Per configuration the original pair
ltu_loss_fwd + ltu_loss_bwd (CE + DiceClass only: it has no Focal / IoU) and the new pair ltu_loss_ext_fwd + ltu_loss_ext_bwd are
called directly through the C-ABI, alternated in one process after a warm-up of both, each forward and backward timed by device
events (each round of calls queued behind a spin kernel, so host launch latency is not timed); the median of the repeats is
reported with the effective bandwidth of the bytes the shapes make them move (forward reads
4 C B S + B S bytes; backward reads as much and writes 4 C B S).  One JSON line per (C, spec, pair).
usage: bench_losses.py [repeats] [side]"""
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, ops  # noqa: E402
from lintransunet_amd.ops import _n, _p, _s  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
side = int(sys.argv[2]) if len(sys.argv) > 2 else 128
B, S = 2, side ** 3
dev = torch.device('cuda')
SLEEP_CYCLES = 2_000_000
SPECS = {'ce+dice': {'CE': 1.0, 'DICE1': 1.0}, 'ce+dice+focal+iou': {'CE': 1.0, 'DICE1': 1.0, 'FOCAL': 1.0, 'IOU': 1.0}}


def pair_old(p, lab, C):
    sums = torch.empty(_lib.load().ltu_loss_ws_floats(B, S, C), device=dev)
    values, coef = torch.empty(9, device=dev), torch.empty(B * C * 3, device=dev)
    w = (ctypes.c_float * 5)(0.0, 1.0, 0.0, 0.0, 0.0)
    g, dp = torch.ones(1, device=dev), torch.empty_like(p)
    fwd = lambda: _lib.call('ltu_loss_fwd', _p(p), _p(lab), _p(sums), _n(sums), _p(values), _p(coef), B, S, C, 1.0, 0.0, w, None, _s())
    bwd = lambda: _lib.call('ltu_loss_bwd', _p(p), _p(lab), _p(coef), _p(g), _p(dp), B, S, C, _s())
    return fwd, bwd


def pair_new(p, lab, C, spec):
    sums = torch.empty(_lib.load().ltu_loss_ext_ws_floats(B, S, C), device=dev)
    values, coef = torch.empty(len(ops.LOSS_EXT_TERMS) + 2, device=dev), torch.empty(B * C * 8, device=dev)
    cfg = ops.loss_ext_cfg(spec)
    g, dp = torch.ones(1, device=dev), torch.empty_like(p)
    fwd = lambda: _lib.call('ltu_loss_ext_fwd', _p(p), _p(lab), _p(sums), _n(sums), _p(values), _p(coef), B, S, C, cfg, None, _s())
    bwd = lambda: _lib.call('ltu_loss_ext_bwd', _p(p), _p(lab), _p(coef), cfg, _p(g), _p(dp), B, S, C, _s())
    return fwd, bwd


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def main():
    gen = torch.Generator(device=dev).manual_seed(0)
    for C in (2, 3):
        p = torch.softmax(torch.randn((B, S, C), device=dev, generator=gen), -1).contiguous()
        lab = torch.randint(0, C, (B, S), device=dev, generator=gen).to(torch.uint8)
        rd, wr = 4 * C * B * S + B * S, 4 * C * B * S
        for sname, spec in SPECS.items():
            pairs = {'loss': pair_old(p, lab, C), 'loss_ext': pair_new(p, lab, C, spec)}
            for f, b in pairs.values():          # warm-up of both
                for _ in range(5):
                    f(); b()
            torch.cuda.synchronize()
            ev = {k: ([], []) for k in pairs}
            for _ in range(reps):                # alternated in one process
                # a spin kernel ahead of each round keeps the device busy while the host enqueues the calls, so the events bracket
                # back-to-back device work and not the host's launch latency
                torch.cuda._sleep(SLEEP_CYCLES)
                for k, (f, b) in pairs.items():
                    ev[k][0].append(timed(f))
                    ev[k][1].append(timed(b))
            torch.cuda.synchronize()
            for k in pairs:
                tf = statistics.median(a.elapsed_time(b) for a, b in ev[k][0]) * 1e3
                tb = statistics.median(a.elapsed_time(b) for a, b in ev[k][1]) * 1e3
                print(json.dumps({'C': C, 'spec': sname, 'pair': k, 'note': 'CE + DiceClass only' if k == 'loss' else '',
                                  'fwd_us': round(tf, 1), 'bwd_us': round(tb, 1), 'fwd_GBps': round(rd / tf / 1e3, 1),
                                  'bwd_GBps': round((rd + wr) / tb / 1e3, 1)}))


if __name__ == '__main__':
    main()
