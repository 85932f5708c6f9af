"""The FusedSGD step at the full configuration (channels [16, 32, 64, 128, 256], 20.87 M parameters, the reducer's real 3 buckets)
next to the guarded AdamW step of the same alternated run: momentum; momentum + Nesterov; + clip; + EMA.  All optimizers share
one reducer (each owns its parameter / moment / EMA buffers, more than the 256 MB cache between two steps of one variant), are
warmed up and then alternated in one process; each step is timed by device events and queued behind a spin kernel, so the events
bracket back-to-back device work and not the host's launch latency.  Medians with min - max, the ratio to the guarded AdamW step
and the ratio of the bytes the shapes make a step move (fp32 words per parameter: the sum of squares reads 1; AdamW reads and
writes p, m, v and reads g: 7, so 8; SGD with momentum p, buf, g: 5, so 6; an EMA adds 2).
Then one FusedSGD step captured with torch.cuda.graph and replayed, with upload_lr() of a new learning rate between the replays,
next to the same optimizer stepping eagerly under the same schedule: what the upload costs.
One JSON line per variant.  usage: bench_sgd.py [repeats]"""
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
MOM = dict(lr=1e-2, momentum=0.99, weight_decay=3e-5)
# name: (class, keywords, words of the update pass per parameter); every variant also runs the sum of squares (1 word)
VARIANTS = {'adamw guard': ('adamw', dict(lr=1e-4, skip_nonfinite=True), 7),
            'adamw guard+clip+ema': ('adamw', dict(lr=1e-4, skip_nonfinite=True, max_grad_norm=1.0, ema_decay=0.999), 9),
            'sgd momentum': ('sgd', dict(MOM), 5),
            'sgd nesterov': ('sgd', dict(MOM, nesterov=True), 5),
            'sgd nesterov+clip': ('sgd', dict(MOM, nesterov=True, skip_nonfinite=True, max_grad_norm=1.0), 5),
            'sgd nesterov+clip+ema': ('sgd', dict(MOM, nesterov=True, skip_nonfinite=True, max_grad_norm=1.0, ema_decay=0.999), 7)}


def timed(fn):
    torch.cuda._sleep(SLEEP_CYCLES)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def stats(pairs):
    us = [a.elapsed_time(b) * 1e3 for a, b in pairs]
    return round(statistics.median(us), 1), round(min(us), 1), round(max(us), 1)


def main():
    dev = torch.device('cuda')
    torch.manual_seed(0)
    model = get_model_dict('MaskTransUnet')([16, 32, 64, 128, 256], [100, 65, 40, 25, 10], [False, True, True, True, True], 1, 2).to(dev)
    reducer = train.GradReducer(model, unused=train.UNUSED_PARAMETERS)
    n = sum(f.numel() for f in reducer.flat)
    for f in reducer.flat:
        f.copy_(2e-3 * torch.randn(f.numel(), device=dev))          # norm about 9: the clipped branch
    opts = {k: (optim.FusedAdamW if cls == 'adamw' else optim.FusedSGD)(reducer, **kw) for k, (cls, kw, _) in VARIANTS.items()}
    for opt in opts.values():          # warm-up of every variant
        for _ in range(5):
            opt.step()
    torch.cuda.synchronize()
    ev = {k: [] for k in opts}
    for _ in range(reps):              # alternated in one process
        for k, opt in opts.items():
            ev[k].append(timed(opt.step))
    torch.cuda.synchronize()
    res = {k: stats(v) for k, v in ev.items()}
    guard, guard_ema = res['adamw guard'][0], res['adamw guard+clip+ema'][0]
    for k, (cls, kw, words) in VARIANTS.items():
        med, lo, hi = res[k]
        ema = 'ema' in k
        print(json.dumps({'variant': k, 'parameters': n, 'buckets': [f.numel() for f in reducer.flat], 'launches': 2 * len(reducer.flat) + 1,
                          'us': med, 'min_us': lo, 'max_us': hi, 'against': 'adamw guard+clip+ema' if ema else 'adamw guard',
                          'ratio': round(med / (guard_ema if ema else guard), 3),
                          'byte_ratio_update_pass': round(words / (9 if ema else 7), 3),
                          'byte_ratio_whole_step': round((words + 1) / (10 if ema else 8), 3),
                          'GBps': round(4 * (words + 1) * n / med / 1e3, 1), 'counters': list(opts[k].counters())}))

    # one captured step replayed under a moving learning rate, next to the eager step under the same schedule
    eager, captured = (optim.FusedSGD(reducer, **dict(MOM, nesterov=True)) for _ in range(2))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            captured.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.step()
    total, t = 2 * reps + 20, 0

    def move_lr():                     # what a schedule writes: the host float only; the timed calls below upload it
        nonlocal t
        t += 1
        eager.param_groups[0]['lr'] = captured.param_groups[0]['lr'] = 1e-2 * (1 - t / total) ** 0.9

    def replay_with_upload():
        captured.upload_lr()           # one stream-ordered fill ahead of the replay
        graph.replay()

    for _ in range(5):
        move_lr()
        eager.step(); replay_with_upload()
    torch.cuda.synchronize()
    ev = {'eager step, lr moved (uploads it itself)': [], 'replay after upload_lr, lr moved': [], 'replay, lr unchanged': []}
    for _ in range(reps):
        move_lr()
        ev['eager step, lr moved (uploads it itself)'].append(timed(eager.step))
        ev['replay after upload_lr, lr moved'].append(timed(replay_with_upload))
        ev['replay, lr unchanged'].append(timed(graph.replay))
    torch.cuda.synchronize()
    for k, v in ev.items():
        med, lo, hi = stats(v)
        print(json.dumps({'variant': k, 'us': med, 'min_us': lo, 'max_us': hi, 'lr_on_device': captured._lr_dev.item(),
                          'lr_host': captured.param_groups[0]['lr']}))
    assert eager._lr_dev.item() == captured._lr_dev.item() < 1e-2


if __name__ == '__main__':
    main()
