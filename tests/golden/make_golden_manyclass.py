#!/usr/bin/env python3
"""Generate tests/golden/model_c5_small.npz and model_c8_small.npz by running the REFERENCE itself with dim_output = 5 / 8.

Runs only where the reference tree is present (/root/reference), in the manner of make_golden.py:fx_model_multi: the reference
model (dropout replaced by a clone) + loss/multi_criterions.py (CrossEntroLoss weighted 10, DiceClassLoss(class_index=c) for
c = 1 .. C-1 weighted 1) on one-hot targets of the max-pooled integer labels, level weights dynamic_weights(0); then the oracle on
the same inputs, asserted to agree.  Inputs are regenerated from seeds (tests/manyclass_common.py).

    python tests/golden/make_golden_manyclass.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, '/root/reference')

from model.trans_3DUnet import get_model_dict    # noqa: E402  (reference)
from loss import multi_criterions as R_mloss     # noqa: E402  (reference)

from oracle import net as O_net                  # noqa: E402
from oracle import step as O_step                # noqa: E402
from oracle import seedgen                       # noqa: E402
from tests import manyclass_common as MC         # noqa: E402

TOL = 1e-5          # make_golden.py's
MAX_BYTES = os.path.getsize(os.path.join(HERE, 'model_multi_small.npz'))


def close(a, b, what, tol=TOL):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    err = (a - b).abs().max().item() if a.numel() else 0.0
    scale = max(1.0, b.abs().max().item()) if b.numel() else 1.0
    assert err <= tol * scale, f'{what}: oracle differs from reference by {err:.3e}'
    return err


def np32(t):
    return t.detach().to(torch.float32).numpy()


def kill_dropout(model):
    for m in model.modules():
        if isinstance(m, (torch.nn.Dropout, torch.nn.Dropout3d)):
            m.forward = lambda t: t.clone()


def fx_model_manyclass(C):
    tag = f'c{C}_small'
    cfg = O_net.NetConfig(dim_output=C, **MC.SMALL)
    wseed = MC.WSEED[C]
    P = seedgen.seeded_params(O_net.param_shapes(cfg), wseed)
    x = seedgen.seeded_volume((MC.BATCH, 1) + MC.SIZE, wseed + 1)
    label = MC.seeded_label((MC.BATCH, 1) + MC.SIZE, wseed + 2, C)
    weights = O_step.dynamic_weights(0)
    # every class is present in the label at all five pyramid levels
    counts = []
    for lvl, lab in enumerate(O_step.label_pyramid(label, len(weights))):
        n = torch.bincount(lab.long().flatten(), minlength=C)
        assert n.numel() == C and int(n.min()) > 0, f'{tag}: level {lvl} misses a class: {n.tolist()}'
        counts.append(int(n.min()))
    model = get_model_dict('MaskTransUnet')(num_layers=cfg.num_layers, roi_size_list=cfg.roi_size_list, is_roi_list=cfg.is_roi_list,
                                            dim_input=cfg.dim_input, dim_output=C, kernel_size=3)
    model.load_state_dict(P, strict=True)
    kill_dropout(model)
    model.train()
    predict, masks = model(x)
    crit = [R_mloss.CrossEntroLoss()] + [R_mloss.DiceClassLoss(class_index=c) for c in range(1, C)]
    cw = MC.criterion_weights(C)
    Fn = torch.nn.functional
    temp = Fn.max_pool3d(label.float(), kernel_size=(2, 2, 1), stride=(2, 2, 1))
    loss_list = []
    for lvl in range(len(weights)):
        if lvl == 0:
            vals = [w * l(predict, MC.onehot(label, C)) for l, w in zip(crit, cw)]
        else:
            vals = [w * l(masks[-lvl], MC.onehot(temp, C)) for l, w in zip(crit, cw)]
            k = 2 if lvl % 2 == 0 else (2, 2, 1)
            temp = Fn.max_pool3d(temp, kernel_size=k, stride=k)
        loss_list.append(vals)
    total = sum(sum(v) * w for v, w in zip(loss_list, weights))
    total.backward()
    grads = {k: p.grad for k, p in model.named_parameters()}

    # the oracle reproduces the reference's output, total and gradients
    Pq = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    boxes = []
    o_pred, o_masks = O_net.forward(Pq, cfg, x, True, boxes)
    o_total, o_levels = MC.total_loss(o_pred, o_masks, label, weights, C)
    o_total.backward()
    close(o_pred, predict, tag + '.out')
    for i, (a, b) in enumerate(zip(o_masks, masks)):
        close(a, b, f'{tag}.mask{i}')
    close(o_total, total, tag + '.total')
    gerr = 0.0
    for k, gr in grads.items():
        if gr is not None:
            gerr = max(gerr, close(Pq[k].grad, gr, f'{tag}.grad[{k}]', 2e-4))
    dice = [R_mloss.DiceClassLoss(class_index=c)(predict, MC.onehot(label, C)).item() for c in range(C)]
    keys = sorted(k for k, v in grads.items() if v is not None)
    idx = MC.out_indices(C)
    out = dict(total=np32(total), dice=np.array(dice, dtype=np.float64),
               level_losses=np.array([[v.item() for v in vals] for vals in loss_list], dtype=np.float64),
               weights=np.array(weights, dtype=np.float64),
               grad_keys=np.array(keys), grad_norms=np.array([grads[k].double().norm().item() for k in keys]),
               out_idx=idx.numpy().astype(np.int32), out_sample=np32(predict.flatten()[idx]))
    for i, m in enumerate(masks):
        out[f'mask{i}'] = np32(m)
    for i, b in enumerate(boxes):          # ROI boxes of the oracle's forward (integer)
        out[f'box{i}'] = b.numpy()
    path = os.path.join(HERE, f'model_{tag}.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f'[{tag}] total {total.item():.6f}, grad err {gerr:.2e}, least voxels of a class per level {counts}, '
          f'{len(keys)} gradients, {size} bytes')
    assert size <= MAX_BYTES, (size, MAX_BYTES)


if __name__ == '__main__':
    torch.manual_seed(0)
    for C in (5, 8):
        fx_model_manyclass(C)
