"""Optimizer / schedule / checkpoint shell of train3D.py.

  train3D.py:193       optimizer = torch.optim.AdamW(model.parameters(), lr=1e-4)
  train3D.py:195-201   ReduceLROnPlateau(mode='min', factor=0.8, patience=5, threshold=1e-2, cooldown=1, min_lr=1e-7)
  train3D.py:226-291   dynamic level weights with a 10-epoch warm-up (train.get_dynamic_weight), best-checkpoint logic that
                       saves `model.state_dict()` as temp_model.pt

The AdamW step is one HIP launch per gradient bucket (`ltu_adamw`): parameters and moments live in flat fp32 buffers laid out
exactly like the reducer's gradient buckets (each `nn.Parameter` becomes a view into them; `state_dict()` is unaffected).
The schedule and checkpoint logic are host code with the same argument meaning as the torch classes the reference uses.
"""
import contextlib
import math
import os

import torch

from . import _lib
from .ops import _p, _s


class FusedAdamW:
    """torch.optim.AdamW semantics (defaults lr 1e-3, betas (0.9, 0.999), eps 1e-8, weight_decay 1e-2, no amsgrad) for the
    parameters held by a `train.GradReducer`.  Parameters that never receive a gradient are not updated (torch skips
    `p.grad is None` the same way).

    Guarded mode (any of the three keywords set; with all three at their defaults `step()` is the plain `ltu_adamw` step):
      max_grad_norm   clip by the global gradient norm like `torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm)`
      skip_nonfinite  a step whose gradient holds an inf or a NaN (or whose squared norm overflows fp32) changes nothing: what
                      `GradScaler.step` does for the reference's monai driver (utils/utils_3D_monai.py:103-105)
      ema_decay       keep `ema = ema_decay * ema + (1 - ema_decay) * p` of every bucketed parameter, updated in the pass that
                      updates the parameter; starts at the parameters' values at construction
    `step()` then issues, on the current stream, one sum-of-squares launch per bucket, one guard launch and one guarded update
    per bucket (csrc/optim.hip).  The decision and both counters (applied / skipped steps) stay in a device-resident state record:
    `step()` reads nothing back, does not synchronise and allocates nothing, so it can be captured with `torch.cuda.graph` as a
    linear chain.  `lr` (like every other scalar) is a launch argument and therefore baked into such a capture: capture again
    after the schedule changed it.  `grad_norm` is a device fp32 scalar (a view into the state) holding the last step's norm of
    the scaled gradient before clipping; `counters()` reads (applied, skipped) back.  In guarded mode the host's `step_count` counts
    calls of `step()`, applied or not; the bias corrections use the device's applied count.
    Data-parallel: `step()` runs after `reducer.finish()`, every rank folds identical buckets in the same order and takes the same
    decision with no communication added (like every N > 1 path here, not yet run on hardware)."""

    def __init__(self, reducer, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, skip_nonfinite=False,
                 ema_decay=None):
        if max_grad_norm is not None and not (math.isfinite(max_grad_norm) and max_grad_norm > 0):
            raise ValueError(f'max_grad_norm must be finite and > 0, got {max_grad_norm}')
        if ema_decay is not None and not 0.0 <= ema_decay < 1.0:
            raise ValueError(f'ema_decay must be in [0, 1), got {ema_decay}')
        self.reducer = reducer
        self.generation = reducer.generation          # the flat layout this optimizer's parameter / moment buffers mirror
        self.param_groups = [dict(lr=float(lr), betas=tuple(betas), eps=float(eps), weight_decay=float(weight_decay))]
        self.step_count = 0
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite or self.ema_decay is not None
        self.flat_p, self.m, self.v = [], [], []
        for params, flat_g in zip(reducer.buckets, reducer.flat):
            if not flat_g.is_cuda:
                raise _lib.LtuError('FusedAdamW runs on the GPU only (no CPU fallback)')
            flat = torch.empty_like(flat_g)
            off = 0
            for p in params:
                n = p.numel()
                flat[off:off + n].copy_(p.data.reshape(-1))
                p.data = flat[off:off + n].view_as(p)          # the model's weight store notices the move and rebuilds its table
                off += n
            self.flat_p.append(flat)
            self.m.append(torch.zeros_like(flat))
            self.v.append(torch.zeros_like(flat))
        self.ema = [f.clone() for f in self.flat_p] if self.ema_decay is not None else []
        if self.guarded:
            # one scratch row of per-workgroup partial sums per bucket, side by side, and the guard state (include/ltu_hip.h)
            parts = [int(_lib.load().ltu_grad_sumsq_parts(f.numel())) for f in self.flat_p]
            self._part_off = [sum(parts[:i]) for i in range(len(parts))]
            self._parts = sum(parts)
            dev = self.flat_p[0].device
            self._scratch = torch.zeros(max(self._parts, 1), device=dev, dtype=torch.float32)
            self._state = torch.zeros(12, device=dev, dtype=torch.float32)
            self.grad_norm = self._state[0]
            self._counters = self._state[6:10].view(torch.int64)          # applied, skipped

    def zero_grad(self):
        self.reducer.zero_grad()

    def step(self, grad_scale=1.0):
        if self.reducer.generation != self.generation:
            raise RuntimeError('the reducer re-assigned its gradient buckets (rebucket) after this optimizer was built: its flat '
                               'parameter / moment buffers no longer match; call rebucket() before constructing the optimizer')
        g = self.param_groups[0]
        self.step_count += 1
        if not self.guarded:
            for p, gr, m, v in zip(self.flat_p, self.reducer.flat, self.m, self.v):
                _lib.call('ltu_adamw', _p(p), _p(gr), _p(m), _p(v), p.numel(), g['lr'], g['betas'][0], g['betas'][1], g['eps'],
                          g['weight_decay'], self.step_count, float(grad_scale), _s())
            return
        s, scale = _s(), float(grad_scale)
        for gr, off in zip(self.reducer.flat, self._part_off):
            _lib.call('ltu_grad_sumsq', _p(gr), gr.numel(), scale, _p(self._scratch) + 4 * off, self._scratch.numel() - off, s)
        _lib.call('ltu_adamw_guard', _p(self._scratch), self._parts, _p(self._state), scale, self.max_grad_norm or 0.0,
                  int(self.skip_nonfinite), g['betas'][0], g['betas'][1], s)
        for i, (p, gr, m, v) in enumerate(zip(self.flat_p, self.reducer.flat, self.m, self.v)):
            _lib.call('ltu_adamw_guarded', _p(p), _p(gr), _p(m), _p(v), _p(self.ema[i]) if self.ema else 0, p.numel(), g['lr'],
                      g['betas'][0], g['betas'][1], g['eps'], g['weight_decay'], self.ema_decay or 0.0, _p(self._state), s)

    def counters(self):
        """(applied, skipped) steps; a host read of the device-resident counters (guarded mode), else (step_count, 0)"""
        if not self.guarded:
            return self.step_count, 0
        applied, skipped = self._counters.tolist()
        return applied, skipped

    def state_dict(self):
        sd = dict(step=self.step_count, param_groups=[dict(g) for g in self.param_groups],
                  m=[t.clone() for t in self.m], v=[t.clone() for t in self.v])
        if self.guarded:
            sd['step'], sd['skipped'] = self.counters()
            if self.ema:
                sd['ema'] = [t.clone() for t in self.ema]
        return sd

    def load_state_dict(self, sd):
        """accepts dictionaries written without the guard as well: counters from 'step', the EMA left as it is"""
        self.step_count = int(sd['step'])
        self.param_groups = [dict(g) for g in sd['param_groups']]
        for dst, src in zip(self.m, sd['m']):
            dst.copy_(src)
        for dst, src in zip(self.v, sd['v']):
            dst.copy_(src)
        if self.guarded:
            skipped = int(sd.get('skipped', 0))
            self.step_count += skipped
            self._counters.copy_(torch.tensor([int(sd['step']), skipped], dtype=torch.int64))
            if self.ema and 'ema' in sd:
                for dst, src in zip(self.ema, sd['ema']):
                    dst.copy_(src)

    def ema_state_dict(self, model):
        """`model.state_dict()` with every bucketed parameter replaced by its average (loadable by the reference like the plain
        one); parameters outside the buckets (train.UNUSED_PARAMETERS) and buffers keep their own value"""
        if not self.ema:
            raise RuntimeError('this optimizer keeps no EMA (ema_decay=None)')
        name_of = {id(p): n for n, p in model.named_parameters()}
        sd = model.state_dict()
        for params, ema in zip(self.reducer.buckets, self.ema):
            off = 0
            for p in params:
                n = p.numel()
                if id(p) in name_of:
                    sd[name_of[id(p)]] = ema[off:off + n].view_as(p).clone()
                off += n
        return sd

    @contextlib.contextmanager
    def ema_weights(self):
        """inside the block the parameters hold the averaged weights: the CONTENTS of the flat parameter buffers and the EMA
        buffers are exchanged (the storage stays where it is, so captured graphs remain valid) and exchanged back, bit-exactly, on
        exit.  The model re-prepares its operands from the parameters on every forward, so an eval() forward inside the block
        runs on the average."""
        if not self.ema:
            raise RuntimeError('this optimizer keeps no EMA (ema_decay=None)')
        self._exchange_ema()
        try:
            yield self
        finally:
            self._exchange_ema()

    def _exchange_ema(self):
        for p, e in zip(self.flat_p, self.ema):
            tmp = p.clone()
            p.copy_(e)
            e.copy_(tmp)


class ReduceLROnPlateau:
    """torch.optim.lr_scheduler.ReduceLROnPlateau for any object with `param_groups` (same arguments, same state machine:
    relative/absolute threshold, patience counted in bad epochs, cooldown, per-group min_lr, eps)."""

    def __init__(self, optimizer, mode='min', factor=0.1, patience=10, threshold=1e-4, threshold_mode='rel', cooldown=0,
                 min_lr=0.0, eps=1e-8):
        if factor >= 1.0:
            raise ValueError('Factor should be < 1.0.')
        if mode not in ('min', 'max') or threshold_mode not in ('rel', 'abs'):
            raise ValueError('unknown mode')
        self.optimizer, self.mode, self.factor, self.patience = optimizer, mode, factor, patience
        self.threshold, self.threshold_mode, self.cooldown, self.eps = threshold, threshold_mode, cooldown, eps
        n = len(optimizer.param_groups)
        self.min_lrs = list(min_lr) if isinstance(min_lr, (list, tuple)) else [min_lr] * n
        self.best = math.inf if mode == 'min' else -math.inf
        self.num_bad_epochs = 0
        self.cooldown_counter = 0
        self.last_epoch = 0

    def _is_better(self, a):
        if self.mode == 'min':
            return a < (self.best * (1.0 - self.threshold) if self.threshold_mode == 'rel' else self.best - self.threshold)
        return a > (self.best * (self.threshold + 1.0) if self.threshold_mode == 'rel' else self.best + self.threshold)

    def step(self, metrics):
        current = float(metrics)
        self.last_epoch += 1
        if self._is_better(current):
            self.best = current
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0
        if self.num_bad_epochs > self.patience:
            for i, g in enumerate(self.optimizer.param_groups):
                old = float(g['lr'])
                new = max(old * self.factor, self.min_lrs[i])
                if old - new > self.eps:
                    g['lr'] = new
            self.cooldown_counter = self.cooldown
            self.num_bad_epochs = 0


def reference_schedule(optimizer):
    """the scheduler of train3D.py:195-201"""
    return ReduceLROnPlateau(optimizer, mode='min', factor=0.8, patience=5, threshold=1e-2, cooldown=1, min_lr=1e-7)


def monai_schedule(optimizer):
    """the scheduler of train3D_monai_version.py:199-205"""
    return ReduceLROnPlateau(optimizer, mode='min', factor=0.6, patience=4, threshold=1e-2, cooldown=1, min_lr=1e-7)


class BestCheckpoint:
    """Best-checkpoint logic of train3D.py:254-268: whenever the eval loss does not exceed the best so far, write
    `model.state_dict()` to `<dir>/temp_model.pt` (loadable by the reference's get_model, train3D.py:104-120).  What the
    reference does not keep -- optimizer moments, step, learning rate, RNG state -- goes to a side file."""

    def __init__(self, model_dir, rank=None):
        self.dir = model_dir
        self.best_eval = math.inf
        self.best_train = math.inf
        if rank is None:       # data-parallel run: every rank holds the same weights, only rank 0 writes
            import torch.distributed as dist
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self.rank = rank
        if self.rank == 0:
            os.makedirs(model_dir, exist_ok=True)

    def update(self, model, eval_loss, train_loss, optimizer=None):
        if eval_loss > self.best_eval:
            return False
        self.best_eval, self.best_train = eval_loss, train_loss
        if self.rank != 0:
            return True
        torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, os.path.join(self.dir, 'temp_model.pt'))
        if optimizer is not None:
            side = dict(optimizer={k: ([t.cpu() for t in v] if isinstance(v, list) and v and torch.is_tensor(v[0]) else v)
                                   for k, v in optimizer.state_dict().items()},
                        rng_cpu=torch.get_rng_state(), rng_cuda=torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None)
            torch.save(side, os.path.join(self.dir, 'temp_model.extra.pt'))
        return True
