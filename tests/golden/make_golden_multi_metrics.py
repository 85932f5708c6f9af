#!/usr/bin/env python3
"""Generate tests/golden/multi_metrics.npz: the eight evaluation criteria of the multi-class driver
(inference_multi_classes.py:57-58 default criterion_list, loss/multi_criterions.py) computed by the REFERENCE itself.

Runs only in the build container (needs /root/reference, which never travels to the GPU box), like make_golden.py.  Per
case the file holds the inputs (pred f32 [B, C, H, W, D], masks u8 [B, 1, H, W, D]) and the reference's values
`[l(pred, label).item() for l in criterions.values()]` with label = the one-hot of masks (lines 131-137), evaluated on float64
copies of the inputs (the float32 evaluation is checked against them to 1e-5).

    python tests/golden/make_golden_multi_metrics.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference')

from loss import multi_criterions as R_mloss     # noqa: E402  (reference)

NAMES = ['DiceClassLoss0', 'DiceClassLoss', 'DiceClassLoss2', 'Recall', 'Precision', 'Recall2', 'Precision2', 'LocalizationLoss']


def blobs(rng, B, shape, C):
    """integer labels 0 .. C-1: a few ellipsoids per class on background"""
    g = np.indices(shape).astype(np.float64)
    lab = np.zeros((B,) + shape, np.uint8)
    for b in range(B):
        for c in range(1, C):
            for _ in range(2):
                ctr = rng.uniform(0, 1, 3) * np.array(shape)
                rad = rng.uniform(0.15, 0.35, 3) * np.array(shape)
                inside = (((g - ctr[:, None, None, None]) / rad[:, None, None, None]) ** 2).sum(0) <= 1
                lab[b][inside] = c
    return lab


def onehot(lab, C):
    return np.moveaxis(np.eye(C, dtype=np.float32)[lab], -1, 1)


def perturb(rng, lab, C, frac=0.05):
    out = lab.copy()
    flip = rng.random(lab.shape) < frac
    out[flip] = rng.integers(0, C, int(flip.sum()))
    return out


def case(tag, rng):
    if tag in ('onehot', 'soft', 'absent2_both', 'absent2_pred'):
        B, C, shape = 2, 3, ((24, 20, 13) if tag != 'soft' else (24, 21, 13))
    elif tag == 'empty_fg':
        B, C, shape = 2, 3, (24, 21, 13)
    else:                                            # c4
        B, C, shape = 2, 4, (20, 18, 11)
    masks = blobs(rng, B, shape, C)
    plab = perturb(rng, blobs(rng, B, shape, C) if tag == 'c4' else masks, C)
    if tag == 'absent2_both':
        masks[masks == 2] = 1
        plab[plab == 2] = 0
    elif tag == 'absent2_pred':
        plab[plab == 2] = 1
    elif tag == 'empty_fg':
        masks[0] = 0                                 # sample 0: no foreground on either side
        plab[0] = 0
        plab[1] = 0                                  # sample 1: foreground in the label only
    pred = onehot(plab, C)
    if tag == 'soft':
        # blended votes: the average of 5 perturbed one-hot windows, as sliding_window_inference produces them
        pred = np.mean([onehot(perturb(rng, masks, C, 0.2), C) for _ in range(5)], axis=0).astype(np.float32)
    return pred, masks[:, None]


def reference_values(pred, masks, dtype):
    C = pred.shape[1]
    crit = R_mloss.get_criterions(NAMES)
    p = torch.from_numpy(pred).to(dtype)
    m = torch.from_numpy(masks).long()
    n, _, h, w, d = m.shape
    label = F.one_hot(m.flatten(2).transpose(1, 2).squeeze(2), num_classes=C).transpose_(1, 2)
    label = torch.reshape(label, (n, C, h, w, d)).to(dtype)
    with torch.no_grad():
        return np.array([crit[k](p, label).item() for k in NAMES], np.float64)


def main():
    out = {'names': np.array(NAMES)}
    for i, tag in enumerate(('onehot', 'soft', 'absent2_both', 'absent2_pred', 'empty_fg', 'c4')):
        pred, masks = case(tag, np.random.default_rng(1000 + i))
        ref64 = reference_values(pred, masks, torch.float64)
        ref32 = reference_values(pred, masks, torch.float32)
        assert np.all(np.abs(ref32 - ref64) <= 1e-5 * np.maximum(np.abs(ref64), 1e-2)), (tag, ref32, ref64)
        out.update({f'{tag}_pred': pred, f'{tag}_masks': masks, f'{tag}_values': ref64})
        print(tag, pred.shape, dict(zip(NAMES, np.round(ref64, 6))))
    np.savez_compressed(os.path.join(HERE, 'multi_metrics.npz'), **out)
    print('multi_metrics.npz written', os.path.getsize(os.path.join(HERE, 'multi_metrics.npz')), 'bytes')


if __name__ == '__main__':
    main()
