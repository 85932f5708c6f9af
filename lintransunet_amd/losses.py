"""Loss surface of loss/criterions.py (binary labels) and loss/multi_criterions.py (class labels) over
the fused HIP loss kernels.

`get_criterions(name_list) -> {name: nn.Module}` keeps the reference contract (loss/criterions.py:773-782);
`get_multi_criterions(name_list)` is its multi-class counterpart (loss/multi_criterions.py:704-714):
every module is `forward(predict[N,C,...], target) -> 0-dim tensor`.  `target` is an integer label
volume [N,1,...] (or a one-hot [N,C,...] tensor, as the multi-class scripts pass).  All losses of one
decoder level share one streaming reduction (`LevelCriterion`).
"""
import dataclasses
import math
import types
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import ops


@dataclasses.dataclass(frozen=True)
class Imbalance:
    """Parameters of the imbalance names of a LevelCriterion spec ('TverskyLoss..', 'FocalCELoss'; csrc/loss_imbalance.hip), checked
    on the host (ValueError).  alpha, beta: weights of the false positives and false negatives in every Tversky term of the spec,
    both >= 0 and not both 0 (0.5, 0.5: Dice; beta > alpha favours recall); tversky_gamma in [1, 3]: the term is (1 - TI)^(1 /
    gamma), 1 the plain Tversky loss, 4/3 the focal Tversky loss of Abraham & Khan; batch: sum I, FP and FN over the batch before
    the ratio (nnU-Net's batch_dice; the batch is this rank's); eps > 0.  focal_gamma: 0 (plain cross-entropy) or in [1, 5];
    focal_alpha: None or one weight >= 0 per class.  The record is fixed when a step is captured: there is no run-time setter."""
    alpha: float = 0.3
    beta: float = 0.7
    tversky_gamma: float = 1.0
    batch: bool = False
    eps: float = 1e-5
    focal_gamma: float = 2.0
    focal_alpha: Optional[Tuple[float, ...]] = None

    def __post_init__(self):
        if self.focal_alpha is not None:
            object.__setattr__(self, 'focal_alpha', tuple(float(a) for a in self.focal_alpha))
        ops.imbalance_stage(((0,), (1.0,), self.tversky_params), (1.0, self.focal_gamma, self.focal_alpha))      # raises ValueError
        if self.focal_alpha is not None and not 2 <= len(self.focal_alpha) <= ops.LOSS_WIDE_MAXC:
            raise ValueError(f'focal_alpha: one weight per class, 2 .. {ops.LOSS_WIDE_MAXC} classes')

    @property
    def tversky_params(self):
        return {'alpha': self.alpha, 'beta': self.beta, 'gamma': self.tversky_gamma, 'eps': self.eps, 'batch': bool(self.batch)}


@dataclasses.dataclass(frozen=True)
class Regions:
    """Overlapping label regions for region-based training (nnU-Net's `regions_class_order`; csrc/region.hip), checked on the host
    (ValueError).  members: 1 .. 8 tuples of uint8 label values; region r is the set of labels whose voxels are positive for
    sigmoid channel r, and a label in no region is background for all of them.  class_order: None, or one label per region, used
    only on the way back to a label map (infer.region_labels): starting from 0, the label of region r = 0, 1, .. in order is
    written where p_r > threshold, so a later region wins.  batch: the Dice sums of 'RegionDiceLoss' run over the batch (nnU-Net's
    batch_dice; the batch is this rank's), False: per-sample ratios, averaged; eps > 0 of that ratio.  The record is fixed when a
    step is captured."""
    members: Tuple[Tuple[int, ...], ...]
    class_order: Optional[Tuple[int, ...]] = None
    batch: bool = True
    eps: float = 1e-5

    def __post_init__(self):
        try:
            members = tuple(tuple(int(v) for v in region) for region in self.members)
            order = None if self.class_order is None else tuple(int(v) for v in self.class_order)
        except TypeError as e:
            raise ValueError(f'Regions: members is a sequence of sequences of labels, class_order a sequence of labels ({e})')
        if not 1 <= len(members) <= ops.REGION_MAX:
            raise ValueError(f'Regions: 1 .. {ops.REGION_MAX} regions (one bit each of a byte), got {len(members)}')
        if any(not region for region in members):
            raise ValueError('Regions: an empty region')
        if any(not 0 <= v <= 255 for region in members for v in region):
            raise ValueError('Regions: labels are uint8, 0 .. 255')
        if order is not None and (len(order) != len(members) or any(not 0 <= v <= 255 for v in order)):
            raise ValueError(f'Regions: class_order needs one uint8 label for each of the {len(members)} regions')
        if not (math.isfinite(float(self.eps)) and float(self.eps) > 0.0):
            raise ValueError(f'Regions: eps {self.eps} must be positive')
        object.__setattr__(self, 'members', members)
        object.__setattr__(self, 'class_order', order)
        object.__setattr__(self, 'batch', bool(self.batch))
        object.__setattr__(self, 'eps', float(self.eps))

    @property
    def lut(self):
        """256 bytes, lut[v] = sum_r [v in members[r]] << r: a label's membership of every region (ops.region_bits)"""
        table = bytearray(256)
        for r, region in enumerate(self.members):
            for v in region:
                table[v] |= 1 << r
        return bytes(table)

    @classmethod
    def brats(cls):
        """nnU-Net's BraTS21 convention - labels 0 background, 1 edema, 2 non-enhancing tumour, 3 enhancing tumour: whole tumour =
        {1, 2, 3}, tumour core = {2, 3}, enhancing tumour = {3}, painted back in that order"""
        return cls(members=((1, 2, 3), (2, 3), (3,)), class_order=(1, 2, 3))


def _channels_last(predict):
    """[N,C,...] (any strides) -> contiguous fp32 [N,...,C]"""
    nd = predict.dim()
    cl = predict.permute(0, *range(2, nd), 1)
    if cl.dtype != torch.float32:
        cl = cl.float()
    return cl.contiguous()


def _labels(target, n_class):
    """[N,1,...] integer labels, or one-hot [N,C,...], -> uint8 [N,...]"""
    if target.dim() >= 2 and target.shape[1] == n_class and n_class > 1 and target.shape[1] != 1:
        target = target.argmax(dim=1, keepdim=True)
    return target.reshape(target.shape[0], *target.shape[2:]).to(torch.uint8).contiguous()


def _class_name(stem, class_index):
    if not 0 <= int(class_index) < ops.LOSS_WIDE_MAXC:
        raise ValueError(f'{stem}: class_index {class_index} outside 0 .. {ops.LOSS_WIDE_MAXC - 1}')
    return {0: stem + '0c', 1: stem}.get(int(class_index), f'{stem}{int(class_index)}')


def _class_names(stem):
    """{the spec name of `stem` for class c: c}, every class the kernels take"""
    return {_class_name(stem, c): c for c in range(ops.LOSS_WIDE_MAXC)}


class LevelCriterion(nn.Module):
    """Weighted sum of the training losses of one decoder level on one prediction, one kernel pass.

    spec: {name: weight}.  Every spec runs through ops.level_loss_chain, one autograd node with one stage for each row of `_STAGES`
    that owns a name of the spec (`OWNED`); a stage without a name is not launched, whatever its parameters hold.  The stages take
    up to 8 classes, or 4 beside a name of `EXT`:
    base - the names of the original family, {'CrossEntroLoss', 'BalanceDiceLoss', 'DiceClassLoss' (class 1), 'DiceClassLoss2' ..
      'DiceClassLoss7' (classes 2 .. 7, the reference's multi_criterions.DiceClassLoss(class_index)), 'DiceClassLoss0c' (class 0),
      'DiceClassLoss0' (foreground union 1 - class 0, multi_criterions.py:30-56)}: ltu_loss on predictions of up to 4 classes and
      ltu_loss_wide on 5 .. 8 (both csrc/loss.hip), or, with any name of `EXT`, ltu_loss_ext (csrc/loss_ext.hip), which also carries
      the original terms; `params`: the parameters of the wider family (ops.LOSS_EXT_PARAMS: gamma, sigma, alpha, alpha2, eps;
      defaults ops.LOSS_EXT_DEFAULTS).  A spec without any name runs it too, at weight 0.
    boundary - 'BoundaryLoss' (class 1), 'BoundaryLoss2' .. 'BoundaryLoss7' and 'BoundaryLoss0c' (class 0): Kervadec's boundary term
      w * mean(p_c * phi_c) on the signed distance maps of the label (ops.signed_distance_maps with `spacing`, or the `phi` given to
      forward: [B,K,...] in the order of `boundary_classes`; csrc/loss_boundary.hip); `term_scale_dev` (1-element fp32 device
      tensor) scales the boundary terms alone at run time.
    topk - 'TopKCELoss': nnU-Net's top-k cross-entropy (csrc/loss_topk.hip), the mean of -log(max(p[label], 1e-6)) over the hardest
      `topk_fraction` of the voxels of the whole batch; `topk_fraction_dev` (1-element fp32 device tensor) replaces the fraction at
      run time.  Voxels tied at the threshold share the remaining weight (see ops.level_loss_topk).
    imbalance - with the parameters of `imbalance` (an `Imbalance` record, None = its defaults; csrc/loss_imbalance.hip): 'TverskyLoss'
      (class 1), 'TverskyLoss2' .. 'TverskyLoss7' and 'TverskyLoss0c' (class 0) are (1 - TI_c)^(1 / gamma) with TI the Tversky index
      of the class, per sample or over the batch; 'FocalCELoss' is the mean of alpha[label] (1 - p[label])^gamma (-log max(p[label],
      1e-6)) over all voxels (see ops.level_loss_imbalance).
    cldice - 'ClDiceLoss' (class 1), 'ClDiceLoss2' .. 'ClDiceLoss7' and 'ClDiceLoss0c' (class 0): the soft-clDice of Shit et al. of the
      class, 1 - 2 Tprec Tsens / (Tprec + Tsens) on soft skeletons of `cldice_iters` (1 .. 10) iterations, sums over the batch
      (ops.level_loss_cldice; csrc/softmorph.hip).  Needs 3-D patches; the label skeletons are built from the label patch
      (ops.label_skeletons) or given to forward as `skeletons` [B,K,...] in the order of `cldice_classes`.
    region - with a `regions` record (`Regions`; csrc/region.hip), on a prediction of one sigmoid channel per region: 'RegionBCELoss',
      the mean over all voxels and regions of the binary cross-entropy against the region's membership mask, and 'RegionDiceLoss',
      the mean over the regions of (FP + FN) / (2 I + FP + FN + 2 eps) (ops.level_loss_region).  The two run alone: a spec that
      mixes them with a class name is refused, as every other stage reads class indicators and softmax probabilities.  forward
      takes the label [B,1,...] or, as `bits`, its bit-masks already built (ops.region_bits).
    Returns (total, {name: w * value}) with values detached: what the reference scripts log (`criterions_w * l(...)`,
    utils_3D_multi_class.py:85; all weights are 1 in the single-class script).
    """
    FG = 'fg'           # key of the foreground union in _DICE (every other value is a class index)
    _DICE = dict(_class_names('DiceClassLoss'), DiceClassLoss0=FG)
    # every name -> its term of the wider family (ops.LOSS_EXT_TERMS)
    _TERM = {'CrossEntroLoss': 'CE', 'BalanceDiceLoss': 'BAL', 'DiceClassLoss0c': 'DICE0', 'DiceClassLoss': 'DICE1',
             'DiceClassLoss2': 'DICE2', 'DiceClassLoss3': 'DICE3', 'DiceClassLoss0': 'FG'}
    EXT = {'DiceLoss': 'DICE', 'IOULoss': 'IOU', 'SSLoss': 'SS', 'FocalLoss': 'FOCAL', 'MSELoss': 'MSE', 'ContainLoss': 'CONTAIN',
           'ContainLoss2': 'CONTAIN2', 'BalanceDiceLoss2': 'BAL2', 'CrossEntroLoss0': 'CE0', 'ClassifyLoss': 'CLASSIFY'}
    EXT_MAXC = 4        # class limit of the wider family (csrc/loss_ext.hip)
    BOUNDARY = _class_names('BoundaryLoss')     # boundary term (csrc/loss_boundary.hip) of class ...
    TOPK = 'TopKCELoss'     # top-k cross-entropy (csrc/loss_topk.hip)
    TVERSKY = _class_names('TverskyLoss')       # Tversky term (csrc/loss_imbalance.hip) of class ...
    FOCALCE = 'FocalCELoss'     # focal cross-entropy (csrc/loss_imbalance.hip)
    CLDICE = _class_names('ClDiceLoss')         # soft-clDice term (csrc/softmorph.hip) of class ...
    REGION = {'RegionBCELoss': 1, 'RegionDiceLoss': 2}      # region terms (csrc/region.hip) -> where the stage's report holds them
    # the names each stage of ops.level_loss_chain owns and the class a name stands for (None: no single class): the region stage,
    # which runs alone, then the stages that combine, in chain order
    OWNED = {'region': dict.fromkeys(REGION), 'base': dict(dict.fromkeys([*_TERM, *EXT]), **_class_names('DiceClassLoss')),
             'boundary': BOUNDARY, 'topk': {TOPK: None}, 'imbalance': dict(TVERSKY, **{FOCALCE: None}), 'cldice': CLDICE}

    def __init__(self, spec: dict, scale: float = 1.0, scale_dev=None, params=None, spacing=(1.0, 1.0, 1.0), term_scale_dev=None,
                 topk_fraction: float = 0.1, topk_fraction_dev=None, imbalance=None, cldice_iters: int = 3, regions=None):
        super().__init__()
        if 'DistributionLoss' in spec:
            raise KeyError(_DISTRIBUTION_REFUSED)
        self.names = stage_names(spec)
        unknown = set(spec) - set().union(*self.names.values())
        if unknown:
            raise KeyError(f'no HIP kernel for losses {sorted(unknown)}')
        self.spec = dict(spec)
        self.scale = scale
        self.scale_dev = scale_dev          # 1-element fp32 device tensor: run-time factor on top of `scale` (captured graphs)
        self.params = dict(params or {})
        self.extended = any(name in self.EXT for name in self.spec)
        self.base_names, self.boundary = self.names['base'], self.names['boundary']      # what the base entry runs; the boundary names
        self.tversky = [name for name in self.names['imbalance'] if name != self.FOCALCE]
        self.focalce, self.topk = self.FOCALCE in self.spec, self.TOPK in self.spec
        if imbalance is not None and not isinstance(imbalance, Imbalance):
            raise ValueError('imbalance: a losses.Imbalance record')
        self.imbalance = imbalance      # parameters of the Tversky and focal cross-entropy names (None: the record's defaults)
        self.spacing = tuple(float(v) for v in spacing)      # of the label's voxels (H, W, D): the maps' unit of length
        self.term_scale_dev = term_scale_dev      # 1-element fp32 device tensor: run-time factor of the boundary terms alone
        self.topk_fraction = float(topk_fraction)
        if self.topk and topk_fraction_dev is None and not 0.0 < self.topk_fraction <= 1.0:
            raise ValueError(f'topk_fraction {topk_fraction} outside (0, 1]')
        self.topk_fraction_dev = topk_fraction_dev      # 1-element fp32 device tensor: the fraction, read at run time
        self.cldice = self.names['cldice']
        self.cldice_iters = ops._check_iters(cldice_iters, 'cldice_iters')      # of the soft skeletons; raises ValueError
        if regions is not None and not isinstance(regions, Regions):
            raise ValueError('regions: a losses.Regions record')
        self.regions = regions          # the record of the region names (None: a class model)
        self.region = self.names['region']
        if self.region and regions is None:
            raise ValueError(f'{self.region}: region names need a `regions` record')
        if self.region and len(self.region) != len(self.spec):
            raise ValueError(f'{sorted(set(self.spec) - set(self.region))} beside {self.region}: the region terms run alone, every other '
                             'name reads class indicators and softmax probabilities')

    @property
    def cldice_classes(self):
        """the classes of the spec's clDice names, in the order of the label skeletons that forward builds or takes"""
        return tuple(self.CLDICE[name] for name in self.cldice)

    @property
    def boundary_classes(self):
        """the classes of the spec's boundary names, in the order of the maps (`phi`) that forward builds or takes"""
        return tuple(self.BOUNDARY[name] for name in self.boundary)

    def _check_classes(self, C):
        """the names of the spec against the C classes of a prediction; raises before anything is launched.  (Up to 4 classes
        ltu_loss_fwd takes a weight for each of its 4 class slots and ignores those of absent classes, as it always did.)"""
        for key, what, _, _ in self._STAGES:
            names, limit = self.names[key], C if key != 'base' or self.extended or C > 4 else 4
            absent = [name for name in names if (self.OWNED[key][name] or 0) >= limit]
            if absent or (names and key not in ('base', 'region') and C < 2):
                raise ValueError(f'{absent or names}: {what} ({C} classes)')
        fa = self.imbalance.focal_alpha if self.imbalance is not None else None
        if self.focalce and fa is not None and len(fa) != C:
            raise ValueError(f'{self.FOCALCE}: focal_alpha has {len(fa)} weights, the prediction has {C} classes')

    def dice_weights(self, C):
        """the Dice weights of the spec as the kernels take them: per class, then the foreground union - 5 entries for C <= 4
        (ltu_loss_fwd), C + 1 for 5 .. 8 classes (ltu_loss_wide_fwd)"""
        n = 4 if C <= 4 else C
        wd = [0.0] * (n + 1)
        for name, cls in self._DICE.items():
            if name in self.spec:
                wd[n if cls == self.FG else cls] += self.spec[name] * self.scale
        return wd

    def forward(self, predict, target, params=None, phi=None, skeletons=None, bits=None):
        C = predict.shape[1]
        self._check_classes(C)
        if self.region and C != len(self.regions.members):
            raise ValueError(f'{self.region}: the prediction has {C} channels, the record {len(self.regions.members)} regions')
        if self.regions is not None and not self.region and self.spec:
            raise ValueError(f'{sorted(self.spec)}: class names on the prediction of a region model (use {sorted(self.REGION)})')
        if self.extended and C > self.EXT_MAXC:
            ext = sorted(name for name in self.spec if name in self.EXT)
            raise ValueError(f'{ext}: the wider loss family has kernels for C <= {self.EXT_MAXC} classes only, the prediction has {C}')
        if C > ops.LOSS_WIDE_MAXC:
            raise ValueError(f'the level losses have kernels for C <= {ops.LOSS_WIDE_MAXC} classes, the prediction has {C}')
        p = _channels_last(predict)
        if not self.region:
            lab = _labels(target, C)
        elif bits is not None:
            lab = bits
        else:
            if target.dim() < 2 or target.shape[1] != 1:
                raise ValueError(f'{self.region}: target must be an integer label volume [N,1,...]')
            lab = ops.region_bits(_labels(target, 1), self.regions.lut)      # the region stage reads bit-masks where the others read labels
        present = [key for key, names in self.names.items() if names] or ['base']      # no name at all: the base, at weight 0
        side = types.SimpleNamespace(phi=phi, skeletons=skeletons)      # what a stage may take ready-made instead of building it from the label
        args = {key: arg(self, C, lab, params, side) for key, _, arg, _ in self._STAGES if key in present}
        total, *reports = ops.level_loss_chain(p, lab, scale_dev=self.scale_dev, **args)
        value = {}
        for (key, _, _, entries), report in zip(self._STAGES, reports):
            value.update(zip(self.names[key], (report[k] for k in entries(self, C))))
        return total, {name: value[name] if w == 1.0 else value[name] * w for name, w in self.spec.items()}

    def _term(self, name):
        """the term of the wider family (ops.LOSS_EXT_TERMS) behind a base name"""
        return self.EXT.get(name) or self._TERM[name]

    def _base_entry(self, C, params):
        """the spec's base names as the `base` of ops.level_loss_chain: the wider family beside any name of `EXT`, else the original
        one (ltu_loss up to 4 classes, ltu_loss_wide for 5 .. 8)"""
        if self.extended:
            weights = {}
            for name in self.base_names:
                weights[self._term(name)] = weights.get(self._term(name), 0.0) + self.spec[name] * self.scale
            return 'ltu_loss_ext', ops.loss_ext_cfg(weights, params)
        w_ce, w_bal = self.spec.get('CrossEntroLoss', 0.0) * self.scale, self.spec.get('BalanceDiceLoss', 0.0) * self.scale
        return 'ltu_loss' if C <= 4 else 'ltu_loss_wide', (w_ce, w_bal, tuple(float(w) for w in self.dice_weights(C)))

    def _value_index(self, name, C):
        """where the base entry's report holds the value of a base name: [total, CE, balanced Dice, Dice per class .., union Dice]
        of the original family, [total, terms of ops.LOSS_EXT_TERMS ..] of the wider one"""
        if self.extended:
            return 1 + ops.LOSS_EXT_TERMS.index(self._term(name))
        if name not in self._DICE:
            return 1 if name == 'CrossEntroLoss' else 2
        cls = self._DICE[name]
        return 3 + ((4 if C <= 4 else C) if cls == self.FG else cls)

    def _boundary_arg(self, C, lab, params, side):
        phi = side.phi
        if phi is None:
            if lab.dim() != 4:
                raise ValueError('the boundary term builds its distance maps from 3-D label patches [B,1,H,W,D]; pass `phi` otherwise')
            phi = ops.signed_distance_maps(lab, self.boundary_classes, self.spacing)
        return phi, self.boundary_classes, [self.spec[name] * self.scale for name in self.boundary], self.term_scale_dev

    def _imbalance_arg(self, C, lab, params, side):
        im = self.imbalance or Imbalance()
        tversky = [self.TVERSKY[name] for name in self.tversky], [self.spec[name] * self.scale for name in self.tversky], im.tversky_params
        focal = self.spec.get(self.FOCALCE, 0.0) * self.scale, im.focal_gamma, im.focal_alpha
        return tversky if self.tversky else None, focal if self.focalce else None

    def _cldice_arg(self, C, lab, params, side):
        if lab.dim() != 4:
            raise ValueError('the clDice term skeletonises 3-D patches: predict [B,C,H,W,D], target [B,1,H,W,D]')
        return side.skeletons, self.cldice_classes, [self.spec[name] * self.scale for name in self.cldice], self.cldice_iters

    # one row per stage of ops.level_loss_chain, in chain order: its keyword there, what the check of its names' classes says,
    # (self, C, lab, params, side: the maps and skeletons given to forward) -> its argument, (self, C) -> where its report holds the value of each of its names
    _STAGES = (('base', 'the Dice of a class the prediction does not have',
                lambda self, C, lab, params, side: self._base_entry(C, dict(self.params, **(params or {}))),
                lambda self, C: [self._value_index(name, C) for name in self.base_names]),
               ('boundary', 'the boundary term of a class the prediction does not have', _boundary_arg,
                lambda self, C: range(len(self.boundary))),
               ('topk', 'needs a prediction of at least 2 classes',
                lambda self, C, lab, params, side: (self.spec[self.TOPK] * self.scale, self.topk_fraction, self.topk_fraction_dev),
                lambda self, C: [0]),
               ('imbalance', 'a term of a class the prediction does not have', _imbalance_arg,
                lambda self, C: [self.tversky.index(name) if name != self.FOCALCE else len(self.tversky) for name in self.names['imbalance']]),
               ('cldice', 'the clDice term of a class the prediction does not have', _cldice_arg,
                lambda self, C: range(len(self.cldice))),
               ('region', 'a region term',
                lambda self, C, lab, params, side: (self.spec.get('RegionBCELoss', 0.0) * self.scale, self.spec.get('RegionDiceLoss', 0.0) * self.scale,
                                                    self.regions.batch, self.regions.eps),
                lambda self, C: [self.REGION[name] for name in self.region]))


def stage_names(spec):
    """{stage of ops.level_loss_chain: the names of `spec` that it owns, in spec order}, the stages in chain order"""
    return {key: [name for name in spec if name in owned] for key, owned in LevelCriterion.OWNED.items()}


def cldice_classes(spec):
    """the classes of the clDice names of `spec`, in the order of the label skeletons a LevelCriterion of it builds or takes"""
    return tuple(LevelCriterion.CLDICE[name] for name in stage_names(spec)['cldice'])


def boundary_classes(spec):
    """the classes of the boundary names of `spec`, in the order of the distance maps a LevelCriterion of it builds or takes"""
    return tuple(LevelCriterion.BOUNDARY[name] for name in stage_names(spec)['boundary'])


_DISTRIBUTION_REFUSED = ('no HIP kernel for DistributionLoss: the reference module (loss/criterions.py:119-176) raises a shape '
                         'error on ordinary inputs such as 2x2x8x6x4, so there is no behaviour to port')


class _Single(nn.Module):
    NAME = None

    def __init__(self, **params):
        super().__init__()
        self.impl = LevelCriterion({self.NAME: 1.0}, params=params)

    def forward(self, predict, target):
        return self.impl(predict, target)[0]


class CrossEntroLoss(_Single):
    """loss/criterions.py:696-735"""
    NAME = 'CrossEntroLoss'


def dice_class_name(class_index: int) -> str:
    """the spec name of the Dice of class `class_index`: 'DiceClassLoss0c', 'DiceClassLoss', 'DiceClassLoss2' .. 'DiceClassLoss7'"""
    return _class_name('DiceClassLoss', class_index)


class DiceClassLoss(_Single):
    """loss/criterions.py:35-70 (class 1); loss/multi_criterions.py:58-83 with `class_index`"""
    NAME = 'DiceClassLoss'

    def __init__(self, class_index: int = 1):
        self.NAME = dice_class_name(class_index)
        super().__init__()


class DiceClassLoss2(_Single):
    """loss/multi_criterions.py:85-110 (class 2)"""
    NAME = 'DiceClassLoss2'


class BalanceDiceLoss(_Single):
    """loss/criterions.py:416-442"""
    NAME = 'BalanceDiceLoss'


class DiceClassLoss0(_Single):
    """loss/multi_criterions.py:30-56: Dice of the foreground union (1 - class 0 on both sides)"""
    NAME = 'DiceClassLoss0'


class DiceLoss(_Single):
    """loss/criterions.py:8-32, loss/multi_criterions.py:8-28: 1 - mean_{b,c} (2I + eps) / (P + T + eps)"""
    NAME = 'DiceLoss'

    def __init__(self, eps: float = 1e-5):
        super().__init__(eps=eps)


class IOULoss(_Single):
    """loss/criterions.py:563-585, multi_criterions.py:544-565: 1 - mean_{b,c} (I + eps) / (P + T - I); the eps cancels in the
    denominator as in the reference, which has no guard there"""
    NAME = 'IOULoss'

    def __init__(self, eps: float = 1e-5):
        super().__init__(eps=eps)


class SSLoss(_Single):
    """loss/criterions.py:588-615: mean_{b,c} sigma sum t (p-1)^2 / (T + eps) + (1 - sigma) sum (1-t) p^2 / (S - T + eps)"""
    NAME = 'SSLoss'

    def __init__(self, sigma: float = 0.05, eps: float = 1e-5):
        super().__init__(sigma=sigma, eps=eps)


class FocalLoss(_Single):
    """loss/criterions.py:618-644, multi_criterions.py:568-591: -(1/(B S C)) sum t (1-p)^gamma log p, the log not clamped.
    `eps` is unused, as in the reference.  Deviation: voxels with t = 0 contribute exactly 0; the reference gives NaN there when
    p == 0 exactly (0 * log 0).  At p == 1 exactly the gradient is its limit (0 for gamma > 0), also for gamma < 1 where the
    reference's autograd gives NaN."""
    NAME = 'FocalLoss'

    def __init__(self, gamma: float = 2, eps: float = 1e-9):
        super().__init__(gamma=gamma)


class MSEcLoss(_Single):
    """loss/criterions.py:738-751, multi_criterions.py:666-679 (registered as 'MSELoss'): the mean of (p - onehot)^2 over all
    B S C entries; reduction='sum' gives the sum.  reduction='none' has no scalar to return and is refused."""
    NAME = 'MSELoss'

    def __init__(self, size_average=None, reduce=None, reduction: str = 'mean'):
        if size_average is not None or reduce is not None:
            reduction = nn._reduction.legacy_get_string(size_average, reduce)
        if reduction not in ('mean', 'sum'):
            raise ValueError(f"MSEcLoss: reduction {reduction!r} is not supported (use 'mean' or 'sum')")
        super().__init__()
        self.reduction = reduction

    def forward(self, predict, target):
        v = self.impl(predict, target)[0]
        return v * predict.numel() if self.reduction == 'sum' else v


class ContainLoss(_Single):
    """loss/criterions.py:466-497, class 1: 1 - mean_b (I + eps) / ((1 - alpha)(T + eps) + alpha (P + eps)).  Deviation: the
    target is t = [label == 1] where the reference reads the raw label; the two agree on the binary labels criterions.py is
    written for."""
    NAME, PARAM, ALPHA = 'ContainLoss', 'alpha', 0.4

    def __init__(self, class_index: int = 1, eps: float = 1e-5):
        if class_index != 1:
            raise ValueError(f'{self.NAME}: only class_index=1 has a HIP kernel')
        super().__init__(eps=eps)

    def forward(self, predict, target, alpha: float = None):
        return self.impl(predict, target, {self.PARAM: self.ALPHA if alpha is None else alpha})[0]


class ContainLoss2(ContainLoss):
    """loss/criterions.py:500-530: ContainLoss with alpha = 0.3 by default"""
    NAME, PARAM, ALPHA = 'ContainLoss2', 'alpha2', 0.3


class BalanceDiceLoss2(_Single):
    """loss/multi_criterions.py:517-541: the balanced Dice of BalanceDiceLoss over classes 1 .. C-1 only"""
    NAME = 'BalanceDiceLoss2'

    def __init__(self, eps: float = 1e-5):
        super().__init__(eps=eps)


class CrossEntroLoss0(_Single):
    """loss/multi_criterions.py:640-663: the CrossEntroLoss of the two channels (p_0, 1 - p_0) against (t_0, 1 - t_0)"""
    NAME = 'CrossEntroLoss0'

    def __init__(self, eps: float = 1e-5):
        super().__init__(eps=eps)


class ClassifyLoss(_Single):
    """loss/multi_criterions.py:617-637: with m = 1 - t_0 and y = sum_c c p_c, sum m (y - label)^2 / (sum m + eps), pooled over
    the batch"""
    NAME = 'ClassifyLoss'

    def __init__(self, eps: float = 1e-5):
        super().__init__(eps=eps)


def boundary_name(class_index: int) -> str:
    """the spec name of the boundary term of class `class_index`: 'BoundaryLoss0c', 'BoundaryLoss', 'BoundaryLoss2' .. 'BoundaryLoss7'"""
    return _class_name('BoundaryLoss', class_index)


class BoundaryLoss(nn.Module):
    """Kervadec et al., "Boundary loss for highly unbalanced segmentation" (no reference counterpart): mean over (b, s) of
    p[b, class_index, s] * phi[b, s], phi the signed distance map of {target == class_index} built on the GPU from the label patch
    with `spacing` (ops.signed_distance_maps); forward(predict, target, phi=None) takes maps built elsewhere as [B,1,...]"""

    def __init__(self, class_index: int = 1, spacing=(1.0, 1.0, 1.0)):
        super().__init__()
        self.impl = LevelCriterion({boundary_name(class_index): 1.0}, spacing=spacing)

    def forward(self, predict, target, phi=None):
        return self.impl(predict, target, phi=phi)[0]


class TopKCELoss(nn.Module):
    """nnU-Net's TopKLoss (no reference counterpart): the cross-entropy -log(max(p[label], 1e-6)) averaged over the hardest `k`
    percent of the voxels of the whole batch; voxels tied at the threshold share the remaining weight (ops.level_loss_topk)"""

    def __init__(self, k: float = 10.0):
        super().__init__()
        self.impl = LevelCriterion({'TopKCELoss': 1.0}, topk_fraction=float(k) / 100.0)

    def forward(self, predict, target):
        return self.impl(predict, target)[0]


def tversky_name(class_index: int) -> str:
    """the spec name of the Tversky term of class `class_index`: 'TverskyLoss0c', 'TverskyLoss', 'TverskyLoss2' .. 'TverskyLoss7'"""
    return _class_name('TverskyLoss', class_index)


class TverskyLoss(nn.Module):
    """Salehi et al., "Tversky loss function for image segmentation using 3D fully convolutional deep networks", and with gamma > 1
    the focal Tversky loss of Abraham & Khan (no reference counterpart): (1 - TI)^(1 / gamma) of class `class_index`, TI = (I + eps)
    / (I + alpha FP + beta FN + eps), per sample and averaged, or with `batch` on sums over the whole batch
    (ops.level_loss_imbalance)"""

    def __init__(self, class_index: int = 1, alpha: float = 0.3, beta: float = 0.7, gamma: float = 1.0, batch: bool = False):
        super().__init__()
        self.impl = LevelCriterion({tversky_name(class_index): 1.0},
                                   imbalance=Imbalance(alpha=alpha, beta=beta, tversky_gamma=gamma, batch=batch))

    def forward(self, predict, target):
        return self.impl(predict, target)[0]


class FocalCELoss(nn.Module):
    """Focal cross-entropy on the label's channel at up to 8 classes (Lin et al.; no reference counterpart - the reference's
    FocalLoss is the term of the wider family, which stops at 4 classes): the mean over all voxels of alpha[label] (1 - p[label])^gamma
    (-log max(p[label], 1e-6)); gamma 0 or in [1, 5], 0 without alpha being the plain mean cross-entropy of nnU-Net and monai's
    DiceCELoss (ops.level_loss_imbalance)"""

    def __init__(self, gamma: float = 2.0, alpha=None):
        super().__init__()
        self.impl = LevelCriterion({'FocalCELoss': 1.0}, imbalance=Imbalance(focal_gamma=gamma, focal_alpha=alpha))

    def forward(self, predict, target):
        return self.impl(predict, target)[0]


def cldice_name(class_index: int) -> str:
    """the spec name of the clDice term of class `class_index`: 'ClDiceLoss0c', 'ClDiceLoss', 'ClDiceLoss2' .. 'ClDiceLoss7'"""
    return _class_name('ClDiceLoss', class_index)


class _RegionSingle(nn.Module):
    NAME = None

    def __init__(self, regions):
        super().__init__()
        self.impl = LevelCriterion({self.NAME: 1.0}, regions=regions)

    def forward(self, predict, target):
        return self.impl(predict, target)[0]


class RegionBCELoss(_RegionSingle):
    """The binary cross-entropy of nnU-Net's region-based training (no reference counterpart) on the sigmoid channels `predict`
    [N,R,...] of the record `regions` against the membership masks of the label `target` [N,1,...], averaged over all voxels and
    regions (ops.level_loss_region, which says where it differs from a cross-entropy on logits).  Not in Loss_Dict: it needs the
    record."""
    NAME = 'RegionBCELoss'


class RegionDiceLoss(_RegionSingle):
    """The soft Dice loss of nnU-Net's region-based training (no reference counterpart): the mean over the regions of (FP + FN) /
    (2 I + FP + FN + 2 eps), on batch sums or per sample as the record says (ops.level_loss_region).  Not in Loss_Dict: it needs the
    record."""
    NAME = 'RegionDiceLoss'


class ClDiceLoss(nn.Module):
    """Shit et al., "clDice - a novel topology-preserving loss function for tubular structure segmentation" (CVPR 2021; no reference
    counterpart): the soft-clDice of class `class_index` on soft skeletons of `iters` iterations (ops.level_loss_cldice, which lists
    the differences from the published loss: one class per term, smooth fixed at 1)"""

    def __init__(self, class_index: int = 1, iters: int = 3):
        super().__init__()
        self.impl = LevelCriterion({cldice_name(class_index): 1.0}, cldice_iters=iters)

    def forward(self, predict, target, skeletons=None):
        return self.impl(predict, target, skeletons=skeletons)[0]


class _EvalMetric(nn.Module):
    """the evaluation losses train3D.py:143 requests besides the Dice losses (`eval_list`): computed on the un-thresholded class
    probabilities by the metric kernels of the inference driver (csrc/infer.hip); evaluation only, no gradient"""
    INDEX, COMPLEMENT = 0, False

    def forward(self, predict, target):
        from . import infer
        with torch.no_grad():
            v = infer.evaluate(predict, target, threshold=-1.0)[infer.METRIC_NAMES[self.INDEX]]
        return 1.0 - v if self.COMPLEMENT else v


class RecallLoss(_EvalMetric):
    """loss/criterions.py:314-345: 1 - mean_b (sum p t + 1e-5) / (sum t + 1e-5)"""
    INDEX, COMPLEMENT = 1, True


class PrecisionLoss(_EvalMetric):
    """loss/criterions.py:382-413: 1 - mean_b (sum p t + 1e-5) / (sum p + 1e-5)"""
    INDEX, COMPLEMENT = 2, True


class Recall(_EvalMetric):
    """loss/criterions.py:280-311: mean_b (sum p t + 1e-5) / (sum t + 1e-5)"""
    INDEX = 1


class Precision(_EvalMetric):
    """loss/criterions.py:348-379: mean_b (sum p t + 1e-5) / (sum p + 1e-5)"""
    INDEX = 2


class LocalizationLoss(_EvalMetric):
    """loss/criterions.py:179-241 (as written there: all three "axes" reduce to the H profile)"""
    INDEX = 3


Loss_Dict = {
    'CrossEntroLoss': CrossEntroLoss,
    'DiceClassLoss': DiceClassLoss,
    'DiceClassLoss0': DiceClassLoss0,
    'DiceClassLoss2': DiceClassLoss2,
    'BalanceDiceLoss': BalanceDiceLoss,
    'RecallLoss': RecallLoss,
    'PrecisionLoss': PrecisionLoss,
    'LocalizationLoss': LocalizationLoss,
    'DiceLoss': DiceLoss,
    'IOULoss': IOULoss,
    'SSLoss': SSLoss,
    'FocalLoss': FocalLoss,
    'MSELoss': MSEcLoss,
    'ContainLoss': ContainLoss,
    'ContainLoss2': ContainLoss2,
    'BalanceDiceLoss2': BalanceDiceLoss2,
    'CrossEntroLoss0': CrossEntroLoss0,
    'ClassifyLoss': ClassifyLoss,
    'BoundaryLoss': BoundaryLoss,
    'TopKCELoss': TopKCELoss,
    'TverskyLoss': TverskyLoss,
    'FocalCELoss': FocalCELoss,
    'ClDiceLoss': ClDiceLoss,
    'Recall': Recall,
    'Precision': Precision,
}


def get_criterions(name_list):
    """loss/criterions.py:773-782, and the training losses of loss/multi_criterions.py that a `--criterion_list` can name
    (BalanceDiceLoss2, CrossEntroLoss0, ClassifyLoss, DiceClassLoss0, DiceClassLoss2), and BoundaryLoss (class 1, unit spacing) and
    TopKCELoss (k = 10 percent), and TverskyLoss (class 1, alpha 0.3, beta 0.7) and FocalCELoss (gamma 2), and ClDiceLoss (class 1, 3
    iterations).  DistributionLoss is refused."""
    if 'DistributionLoss' in name_list:
        raise KeyError(_DISTRIBUTION_REFUSED)
    return {name: Loss_Dict[name]() for name in name_list}


class _MultiEvalMetric(nn.Module):
    """the evaluation criteria of loss/multi_criterions.py that the multi-class drivers only read (inference_multi_classes.py:153,
    utils_3D_multi_class.py:146-208): one entry of infer.evaluate_multiclass (csrc/class_metrics.hip) on the values as given;
    evaluation only, no gradient"""
    NAME, COMPLEMENT = None, False

    def forward(self, predict, target):
        from . import infer
        with torch.no_grad():
            v = infer.evaluate_multiclass(predict, target)[self.NAME]
        return 1.0 - v if self.COMPLEMENT else v


class MultiRecall(_MultiEvalMetric):
    """loss/multi_criterions.py:320-346: mean_b (sum p_1 t_1 + 1e-5) / (sum t_1 + 1e-5)"""
    NAME = 'Recall'


class MultiRecall2(_MultiEvalMetric):
    """loss/multi_criterions.py:348-375: Recall of class 2"""
    NAME = 'Recall2'


class MultiRecallLoss(_MultiEvalMetric):
    """loss/multi_criterions.py:377-404: 1 - Recall"""
    NAME, COMPLEMENT = 'Recall', True


class MultiPrecision(_MultiEvalMetric):
    """loss/multi_criterions.py:406-433: mean_b (sum p_1 t_1 + 1e-5) / (sum p_1 + 1e-5)"""
    NAME = 'Precision'


class MultiPrecision2(_MultiEvalMetric):
    """loss/multi_criterions.py:435-462: Precision of class 2"""
    NAME = 'Precision2'


class MultiPrecisionLoss(_MultiEvalMetric):
    """loss/multi_criterions.py:464-491: 1 - Precision"""
    NAME, COMPLEMENT = 'Precision', True


class MultiLocalizationLoss(_MultiEvalMetric):
    """loss/multi_criterions.py:219-281: on the foreground union 1 - channel 0 of both sides, no factor 8"""
    NAME = 'LocalizationLoss'


Multi_Loss_Dict = {
    'CrossEntroLoss': CrossEntroLoss,
    'DiceClassLoss0': DiceClassLoss0,
    'DiceClassLoss': DiceClassLoss,
    'DiceClassLoss2': DiceClassLoss2,
    'BoundaryLoss': BoundaryLoss,
    'TopKCELoss': TopKCELoss,
    'Recall': MultiRecall,
    'Precision': MultiPrecision,
    'Recall2': MultiRecall2,
    'Precision2': MultiPrecision2,
    'RecallLoss': MultiRecallLoss,
    'PrecisionLoss': MultiPrecisionLoss,
    'LocalizationLoss': MultiLocalizationLoss,
}


def get_multi_criterions(name_list):
    """loss/multi_criterions.py:704-714 for the names the multi-class scripts request: CrossEntroLoss and DiceClassLoss0 /
    DiceClassLoss / DiceClassLoss2 are the differentiable modules above (train3D_multi_class.py trains with them), as are
    BoundaryLoss and TopKCELoss; Recall,
    Precision, Recall2, Precision2, RecallLoss, PrecisionLoss and the multi-class LocalizationLoss are evaluation-only modules
    over csrc/class_metrics.hip.  Any other name raises KeyError."""
    unknown = [name for name in name_list if name not in Multi_Loss_Dict]
    if unknown:
        raise KeyError(f'no HIP kernel for multi-class criteria {unknown}')
    return {name: Multi_Loss_Dict[name]() for name in name_list}
