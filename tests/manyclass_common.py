"""Shared pieces of the 5 .. 8-class fixtures (tests/golden/model_c5_small.npz, model_c8_small.npz): the seeded label generator,
the step's criterion list and the oracle-side restatement of the multi-class deep-supervision loss for any class count.
Imported by tests/golden/make_golden_manyclass.py (which writes the fixtures) and by the tests that read them."""
import torch
import torch.nn.functional as F

from oracle import losses as O_loss
from oracle import step as O_step

SMALL = dict(num_layers=[8, 8, 8, 16, 32], roi_size_list=[20, 12, 9, 10, 6])
SIZE, BATCH = (32, 32, 32), 2
WSEED = {5: 705, 8: 708}          # parameters: WSEED, volume: WSEED + 1, label: WSEED + 2 (707 / 710)
CE_WEIGHT = 10.0
OUT_SAMPLES = 4096                # sampled voxels of `out`, every class channel of each


def seeded_label(shape, seed: int, n_classes: int) -> torch.Tensor:
    """uint8 label volume [B,1,H,W,D] with the values 0 .. n_classes-1: one ellipsoid per class 1 .. n_classes-1 and sample, centre in
    [0.2, 0.8] and radii 0.10 .. 0.22 of each axis, painted in class order (a later class covers an earlier one where they meet)"""
    g = torch.Generator().manual_seed(seed)
    B, _, H, W, D = shape
    hh = torch.arange(H).view(H, 1, 1).float()
    ww = torch.arange(W).view(1, W, 1).float()
    dd = torch.arange(D).view(1, 1, D).float()
    lab = torch.zeros(shape, dtype=torch.uint8)
    for b in range(B):
        for k in range(1, n_classes):
            c = 0.2 + 0.6 * torch.rand(3, generator=g)
            r = 0.10 + 0.12 * torch.rand(3, generator=g)
            dist = ((hh - c[0] * H) / (r[0] * H)) ** 2 + ((ww - c[1] * W) / (r[1] * W)) ** 2 + ((dd - c[2] * D) / (r[2] * D)) ** 2
            lab[b, 0][dist <= 1.0] = k
    return lab


def criterion_names(n_classes: int):
    """CrossEntroLoss, then the Dice of every class 1 .. C-1 under the names of lintransunet_amd.losses.LevelCriterion"""
    return ['CrossEntroLoss', 'DiceClassLoss'] + [f'DiceClassLoss{c}' for c in range(2, n_classes)]


def criterion_weights(n_classes: int):
    return [CE_WEIGHT] + [1.0] * (n_classes - 1)


def onehot(label, n_classes: int):
    """integer labels [N,1,...] -> one-hot float [N,C,...]"""
    return F.one_hot(label.long().squeeze(1), n_classes).movedim(-1, 1).float()


def total_loss(predict, masks, label, weights, n_classes: int):
    """oracle.step.total_loss_multi for any class count: 10 * CE + sum_{c >= 1} Dice_c at every level on the one-hot of the
    max-pooled integer labels.  Returns (total, [[weighted values in criterion_names order] per level])."""
    pyramid = O_step.label_pyramid(label, len(weights))
    per_level = []
    for lvl in range(len(weights)):
        pred = predict if lvl == 0 else masks[-lvl]
        t = onehot(pyramid[lvl], n_classes)
        per_level.append([CE_WEIGHT * O_loss._multi_ce(pred, t)] + [O_loss.dice_class_onehot(pred, t, c) for c in range(1, n_classes)])
    total = sum(sum(vals) * w for vals, w in zip(per_level, weights))
    return total, per_level


def out_indices(n_classes: int):
    """flat indices into predict [B,C,H,W,D] of the stored samples: OUT_SAMPLES seeded (sample, voxel) positions, all C channels of each"""
    g = torch.Generator().manual_seed(4242 + n_classes)
    S = SIZE[0] * SIZE[1] * SIZE[2]
    pos = torch.randperm(BATCH * S, generator=g)[:OUT_SAMPLES]
    b, s = pos // S, pos % S
    return ((b[:, None] * n_classes + torch.arange(n_classes)[None, :]) * S + s[:, None]).flatten()
