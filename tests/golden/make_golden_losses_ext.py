#!/usr/bin/env python3
"""Generate tests/golden/losses_ext.npz: the training losses of the wider loss family (csrc/loss_ext.hip) computed by the
REFERENCE itself, values and gradients with respect to `predict`.

Runs only in the build container (needs the reference checkout, which never travels to the GPU box), like make_golden.py.
Inputs are seeded softmax probabilities [B, C, H, W, D] and class ids [B, 1, H, W, D]; every loss runs on float64 copies:
  c2   binary labels, loss/criterions.py modules (the target is the label volume, as train3D.py passes it)
  c2m  the same inputs through loss/multi_criterions.py with one-hot targets (the multi-class-only losses at C = 2)
  c3m  three classes through loss/multi_criterions.py with one-hot targets
Keys: <case>_p, <case>_lab, and <case>_<name> / <case>_<name>_dp for every loss (a name may carry a suffix for a non-default
parameter, listed in <case>_<name>_param).

    python tests/golden/make_golden_losses_ext.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference')

from loss import criterions as R_loss           # noqa: E402  (reference)
from loss import multi_criterions as R_mloss     # noqa: E402  (reference)

SHAPE = (12, 10, 8)
B = 2

# (key, module factory, forward kwargs, parameter recorded beside the key)
BINARY = [
    ('DiceLoss', lambda: R_loss.DiceLoss(), {}, None),
    ('IOULoss', lambda: R_loss.IOULoss(), {}, None),
    ('SSLoss', lambda: R_loss.SSLoss(), {}, None),
    ('SSLoss_s02', lambda: R_loss.SSLoss(sigma=0.2), {}, 0.2),
    ('FocalLoss', lambda: R_loss.FocalLoss(), {}, None),
    ('FocalLoss_g15', lambda: R_loss.FocalLoss(gamma=1.5), {}, 1.5),
    ('MSELoss', lambda: R_loss.MSEcLoss(), {}, None),
    ('ContainLoss', lambda: R_loss.ContainLoss(), {}, None),
    ('ContainLoss_a06', lambda: R_loss.ContainLoss(), {'alpha': 0.6}, 0.6),
    ('ContainLoss2', lambda: R_loss.ContainLoss2(), {}, None),
    ('Recall', lambda: R_loss.Recall(), {}, None),
    ('Precision', lambda: R_loss.Precision(), {}, None),
]
MULTI = [
    ('DiceLoss', lambda: R_mloss.DiceLoss(), {}, None),
    ('IOULoss', lambda: R_mloss.IOULoss(), {}, None),
    ('FocalLoss', lambda: R_mloss.FocalLoss(), {}, None),
    ('MSELoss', lambda: R_mloss.MSEcLoss(), {}, None),
    ('BalanceDiceLoss2', lambda: R_mloss.BalanceDiceLoss2(), {}, None),
    ('CrossEntroLoss0', lambda: R_mloss.CrossEntroLoss0(), {}, None),
    ('ClassifyLoss', lambda: R_mloss.ClassifyLoss(), {}, None),
]


def inputs(rng, C):
    """softmax probabilities of smooth random logits, labels = argmax of a noisy copy (so the prediction is informative)"""
    logits = rng.normal(0, 1.5, (B, C) + SHAPE)
    p = np.exp(logits) / np.exp(logits).sum(1, keepdims=True)
    lab = (logits + rng.normal(0, 1.5, logits.shape)).argmax(1)[:, None].astype(np.uint8)
    return p.astype(np.float32), lab


def run(table, p, target, tag, out):
    for key, make, kw, param in table:
        pd = torch.from_numpy(p.astype(np.float64)).requires_grad_(True)
        v = make()(pd, target, **kw)
        out[f'{tag}_{key}'] = np.float64(v.item())
        if v.requires_grad:
            v.backward()
            out[f'{tag}_{key}_dp'] = pd.grad.numpy().astype(np.float32)
        if param is not None:
            out[f'{tag}_{key}_param'] = np.float64(param)


def main():
    rng = np.random.default_rng(20261016)
    out = {}
    p2, lab2 = inputs(rng, 2)
    out['c2_p'], out['c2_lab'] = p2, lab2
    run(BINARY, p2, torch.from_numpy(lab2.astype(np.int64)), 'c2', out)
    out['c2m_p'], out['c2m_lab'] = p2, lab2
    onehot2 = F.one_hot(torch.from_numpy(lab2[:, 0].astype(np.int64)), 2).permute(0, 4, 1, 2, 3).double()
    run(MULTI, p2, onehot2, 'c2m', out)
    p3, lab3 = inputs(rng, 3)
    out['c3m_p'], out['c3m_lab'] = p3, lab3
    onehot3 = F.one_hot(torch.from_numpy(lab3[:, 0].astype(np.int64)), 3).permute(0, 4, 1, 2, 3).double()
    run(MULTI, p3, onehot3, 'c3m', out)
    # DistributionLoss: the reference module itself fails on an ordinary input (recorded as a flag, not a value)
    try:
        R_loss.DistributionLoss()(torch.from_numpy(p2.astype(np.float64)), torch.from_numpy(lab2.astype(np.int64)))
        out['distribution_loss_fails'] = np.int64(0)
    except (RuntimeError, IndexError, ValueError):
        out['distribution_loss_fails'] = np.int64(1)
    path = os.path.join(HERE, 'losses_ext.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path)} bytes, {len(out)} arrays)')


if __name__ == '__main__':
    main()
