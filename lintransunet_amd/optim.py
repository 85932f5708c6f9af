"""Optimizer / schedule / checkpoint shell of train3D.py.

  train3D.py:193       optimizer = torch.optim.AdamW(model.parameters(), lr=1e-4)
  train3D.py:195-201   ReduceLROnPlateau(mode='min', factor=0.8, patience=5, threshold=1e-2, cooldown=1, min_lr=1e-7)
  train3D.py:226-291   dynamic level weights with a 10-epoch warm-up (train.get_dynamic_weight), best-checkpoint logic that
                       saves `model.state_dict()` as temp_model.pt

The AdamW step is one HIP launch per gradient bucket (`ltu_adamw`): parameters and moments live in flat fp32 buffers laid out
exactly like the reducer's gradient buckets (each `nn.Parameter` becomes a view into them; `state_dict()` is unaffected).
The schedule and checkpoint logic are host code with the same argument meaning as the torch classes the reference uses.

The reference's alternatives and nnU-Net's recipe:
  train3D.py:194       torch.optim.SGD(lr=1e-4, momentum=0.9)            -> FusedSGD (csrc/optim.hip, learning rate on the device)
  train3D.py:203-208   StepLR(250, 0.5), CosineAnnealingLR(100, 1e-6)    -> StepLR, CosineAnnealingLR (closed forms)
  nnU-Net              SGD(1e-2, 0.99, nesterov, wd 3e-5), (1 - t/T)^0.9 -> nnunet_sgd, nnunet_schedule (PolyLR)
"""
import contextlib
import math
import os
import struct

import torch

from . import _lib
from .ops import _p, _s


class _BucketOptimizer:
    """what the fused optimizers share: they mirror the reducer's flat gradient buckets with flat parameter buffers `flat_p`, may keep
    an EMA of them in `ema`, and (guarded) hold the device-resident counters"""

    def zero_grad(self):
        self.reducer.zero_grad()

    def counters(self):
        """(applied, skipped) steps; a host read of the device-resident counters (guarded mode), else (step_count, 0)"""
        if not self.guarded:
            return self.step_count, 0
        applied, skipped = self._counters.tolist()
        return applied, skipped

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


class FusedAdamW(_BucketOptimizer):
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


def _f32(x):
    """the float32 nearest to a host float, as a host float: what a device fp32 scalar holds after a fill with x"""
    return struct.unpack('f', struct.pack('f', x))[0]


def _upload(optimizer):
    """schedulers call this after writing the groups' lr: optimizers with a device-resident learning rate refresh it"""
    upload = getattr(optimizer, 'upload_lr', None)
    if upload is not None:
        upload()


class FusedSGD(_BucketOptimizer):
    """torch.optim.SGD semantics (momentum, dampening, coupled weight decay, Nesterov; defaults lr 1e-3 and everything else off)
    for the parameters held by a `train.GradReducer`, with FusedAdamW's interface and guard: flat parameter buffers mirroring the
    reducer's buckets, `max_grad_norm`, `skip_nonfinite`, `ema_decay`, `grad_norm`, `counters()`, `state_dict()` (holding `buf`, the
    momentum buffers, in place of `m` and `v`), `ema_state_dict()`, `ema_weights()`.  With `momentum == 0` there is no momentum
    storage at all (`buf == []`) and the kernel neither loads nor stores one.

    `step()` ALWAYS runs the guarded sequence (csrc/optim.hip): one sum-of-squares launch per bucket, one guard launch, one
    `ltu_sgd_guarded` launch per bucket, 2 per bucket + 1 launches.  Without clipping or skipping the first two kinds still run,
    because the count of applied steps, which decides torch's "first step" (`buf = g`, which differs from the recurrence when
    `dampening != 0`), lives in the guard state: a skipped first step leaves that case to the next applied one.

    Capture.  `step()` reads nothing back, does not synchronise and allocates nothing, so it can be captured with
    `torch.cuda.graph` as a linear chain.  Unlike FusedAdamW's, its learning rate is NOT a launch argument: it lives in a device
    fp32 scalar this optimizer owns, and the kernel loads it.  `param_groups[0]['lr']` stays the plain float that schedulers
    assign; `upload_lr()` writes it to the device scalar when it differs from the value uploaded last, with one stream-ordered
    fill on the current stream (no pinned staging buffer, no synchronisation, no allocation).  An eager `step()` calls
    `upload_lr()` itself; a `step()` issued while the stream is capturing does not (the fill would be baked into the graph with
    that one value).  Between replays of a captured step the caller, or one of this module's schedulers (each calls
    `upload_lr()` after writing the groups), uploads the new value, and the replay reads it: a captured step stays valid under
    a schedule that moves the learning rate every step.  The value stored is the float32 nearest to the host float, so an eager
    run and a replayed run with the same lr sequence agree bit for bit.  Every other scalar (momentum, weight decay, ...) is
    still a launch argument and baked into a capture."""

    def __init__(self, reducer, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, max_grad_norm=None,
                 skip_nonfinite=False, ema_decay=None):
        if not lr >= 0.0:
            raise ValueError(f'lr must be >= 0, got {lr}')
        if not momentum >= 0.0:
            raise ValueError(f'momentum must be >= 0, got {momentum}')
        if not weight_decay >= 0.0:
            raise ValueError(f'weight_decay must be >= 0, got {weight_decay}')
        if math.isnan(dampening):
            raise ValueError('dampening is NaN')
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        if max_grad_norm is not None and not (math.isfinite(max_grad_norm) and max_grad_norm > 0):
            raise ValueError(f'max_grad_norm must be finite and > 0, got {max_grad_norm}')
        if ema_decay is not None and not 0.0 <= ema_decay < 1.0:
            raise ValueError(f'ema_decay must be in [0, 1), got {ema_decay}')
        self.reducer = reducer
        self.generation = reducer.generation
        self.param_groups = [dict(lr=float(lr), momentum=float(momentum), dampening=float(dampening), weight_decay=float(weight_decay),
                                  nesterov=bool(nesterov))]
        self.step_count = 0
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.guarded = True
        self.flat_p = []
        for params, flat_g in zip(reducer.buckets, reducer.flat):
            if not flat_g.is_cuda:
                raise _lib.LtuError('FusedSGD runs on the GPU only (no CPU fallback)')
            flat = torch.empty_like(flat_g)
            off = 0
            for p in params:
                n = p.numel()
                flat[off:off + n].copy_(p.data.reshape(-1))
                p.data = flat[off:off + n].view_as(p)
                off += n
            self.flat_p.append(flat)
        self.buf = [torch.zeros_like(f) for f in self.flat_p] if momentum != 0 else []
        self.ema = [f.clone() for f in self.flat_p] if self.ema_decay is not None else []
        parts = [int(_lib.load().ltu_grad_sumsq_parts(f.numel())) for f in self.flat_p]
        self._part_off = [sum(parts[:i]) for i in range(len(parts))]
        self._parts = sum(parts)
        dev = self.flat_p[0].device
        self._scratch = torch.zeros(max(self._parts, 1), device=dev, dtype=torch.float32)
        self._state = torch.zeros(12, device=dev, dtype=torch.float32)
        self.grad_norm = self._state[0]
        self._counters = self._state[6:10].view(torch.int64)          # applied, skipped
        self._lr_uploaded = _f32(float(lr))
        self._lr_dev = torch.full((1,), self._lr_uploaded, device=dev, dtype=torch.float32)

    def upload_lr(self):
        """write param_groups[0]['lr'] to the device scalar if it differs from the value uploaded last (see the class docstring)"""
        lr = _f32(self.param_groups[0]['lr'])
        if lr != self._lr_uploaded:
            self._lr_dev.fill_(lr)
            self._lr_uploaded = lr

    def step(self, grad_scale=1.0):
        if self.reducer.generation != self.generation:
            raise RuntimeError('the reducer re-assigned its gradient buckets (rebucket) after this optimizer was built: its flat '
                               'parameter / momentum buffers no longer match; call rebucket() before constructing the optimizer')
        if not torch.cuda.is_current_stream_capturing():
            self.upload_lr()
        g = self.param_groups[0]
        self.step_count += 1
        s, scale = _s(), float(grad_scale)
        for gr, off in zip(self.reducer.flat, self._part_off):
            _lib.call('ltu_grad_sumsq', _p(gr), gr.numel(), scale, _p(self._scratch) + 4 * off, self._scratch.numel() - off, s)
        _lib.call('ltu_adamw_guard', _p(self._scratch), self._parts, _p(self._state), scale, self.max_grad_norm or 0.0,
                  int(self.skip_nonfinite), 0.0, 0.0, s)
        for i, (p, gr) in enumerate(zip(self.flat_p, self.reducer.flat)):
            _lib.call('ltu_sgd_guarded', _p(p), _p(gr), _p(self.buf[i]) if self.buf else 0, _p(self.ema[i]) if self.ema else 0,
                      p.numel(), _p(self._lr_dev), g['momentum'], g['dampening'], g['weight_decay'], int(g['nesterov']),
                      self.ema_decay or 0.0, _p(self._state), s)

    def state_dict(self):
        sd = dict(param_groups=[dict(g) for g in self.param_groups], buf=[t.clone() for t in self.buf])
        sd['step'], sd['skipped'] = self.counters()
        if self.ema:
            sd['ema'] = [t.clone() for t in self.ema]
        return sd

    def load_state_dict(self, sd):
        self.param_groups = [dict(g) for g in sd['param_groups']]
        for dst, src in zip(self.buf, sd['buf']):
            dst.copy_(src)
        skipped = int(sd.get('skipped', 0))
        self.step_count = int(sd['step']) + skipped
        self._counters.copy_(torch.tensor([int(sd['step']), skipped], dtype=torch.int64))
        if self.ema and 'ema' in sd:
            for dst, src in zip(self.ema, sd['ema']):
                dst.copy_(src)
        self.upload_lr()


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
            _upload(self.optimizer)


class _ClosedFormLR:
    """lr(t) = f(lr0, t) from each group's initial lr, t counted by step(): no recursion, so a restored schedule continues exactly"""

    def __init__(self, optimizer):
        self.optimizer = optimizer
        self.base_lrs = [float(g['lr']) for g in optimizer.param_groups]
        self.last_epoch = 0

    def _lr(self, base, t):
        raise NotImplementedError

    def _write(self):
        for g, base in zip(self.optimizer.param_groups, self.base_lrs):
            g['lr'] = self._lr(base, self.last_epoch)
        _upload(self.optimizer)

    def step(self):
        self.last_epoch += 1
        self._write()

    def get_last_lr(self):
        return [g['lr'] for g in self.optimizer.param_groups]

    def state_dict(self):
        return {k: (list(v) if isinstance(v, list) else v) for k, v in self.__dict__.items() if k != 'optimizer'}

    def load_state_dict(self, sd):
        """restores the counter, the initial rates and the arguments, and writes lr(last_epoch) to the groups"""
        self.__dict__.update({k: (list(v) if isinstance(v, list) else v) for k, v in sd.items()})
        self._write()


class PolyLR(_ClosedFormLR):
    """torch.optim.lr_scheduler.PolynomialLR: lr0 * (1 - min(t, total_iters) / total_iters) ** power; with power 0.9 nnU-Net's
    PolyLRScheduler, held at 0 from total_iters on"""

    def __init__(self, optimizer, total_iters, power=0.9):
        if total_iters < 1:
            raise ValueError(f'total_iters must be >= 1, got {total_iters}')
        super().__init__(optimizer)
        self.total_iters, self.power = total_iters, power

    def _lr(self, base, t):
        return base * (1.0 - min(self.total_iters, t) / self.total_iters) ** self.power


class CosineAnnealingLR(_ClosedFormLR):
    """torch.optim.lr_scheduler.CosineAnnealingLR (train3D.py:206-208): eta_min + (lr0 - eta_min) * (1 + cos(pi t / T_max)) / 2,
    periodic beyond T_max like the torch class"""

    def __init__(self, optimizer, T_max, eta_min=0.0):
        if T_max < 1:
            raise ValueError(f'T_max must be >= 1, got {T_max}')
        super().__init__(optimizer)
        self.T_max, self.eta_min = T_max, eta_min

    def _lr(self, base, t):
        return self.eta_min + (base - self.eta_min) * (1.0 + math.cos(math.pi * t / self.T_max)) / 2.0


class StepLR(_ClosedFormLR):
    """torch.optim.lr_scheduler.StepLR (train3D.py:203-205): lr0 * gamma ** (t // step_size)"""

    def __init__(self, optimizer, step_size, gamma=0.1):
        if step_size < 1:
            raise ValueError(f'step_size must be >= 1, got {step_size}')
        super().__init__(optimizer)
        self.step_size, self.gamma = step_size, gamma

    def _lr(self, base, t):
        return base * self.gamma ** (t // self.step_size)


def reference_schedule(optimizer):
    """the scheduler of train3D.py:195-201"""
    return ReduceLROnPlateau(optimizer, mode='min', factor=0.8, patience=5, threshold=1e-2, cooldown=1, min_lr=1e-7)


def monai_schedule(optimizer):
    """the scheduler of train3D_monai_version.py:199-205"""
    return ReduceLROnPlateau(optimizer, mode='min', factor=0.6, patience=4, threshold=1e-2, cooldown=1, min_lr=1e-7)


def reference_step_schedule(optimizer):
    """the StepLR alternative of train3D.py:203-205"""
    return StepLR(optimizer, step_size=250, gamma=0.5)


def reference_cosine_schedule(optimizer):
    """the CosineAnnealingLR alternative of train3D.py:206-208"""
    return CosineAnnealingLR(optimizer, T_max=100, eta_min=1e-6)


def nnunet_sgd(reducer, **kw):
    """nnU-Net's optimizer (nnUNetTrainer.configure_optimizers): SGD, lr 1e-2, momentum 0.99, Nesterov, weight decay 3e-5"""
    return FusedSGD(reducer, lr=1e-2, momentum=0.99, nesterov=True, weight_decay=3e-5, **kw)


def nnunet_schedule(optimizer, epochs=1000):
    """nnU-Net's PolyLRScheduler: lr0 * (1 - epoch / epochs) ** 0.9, stepped once per epoch"""
    return PolyLR(optimizer, total_iters=epochs, power=0.9)


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
