"""Loss surface of loss/criterions.py (binary labels) and loss/multi_criterions.py (class labels) over
the fused HIP loss kernels.

`get_criterions(name_list) -> {name: nn.Module}` keeps the reference contract (loss/criterions.py:773-782);
`get_multi_criterions(name_list)` is its multi-class counterpart (loss/multi_criterions.py:704-714):
every module is `forward(predict[N,C,...], target) -> 0-dim tensor`.  `target` is an integer label
volume [N,1,...] (or a one-hot [N,C,...] tensor, as the multi-class scripts pass).  All losses of one
decoder level share one streaming reduction (`LevelCriterion`).
"""
import torch
import torch.nn as nn

from . import ops


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


class LevelCriterion(nn.Module):
    """Weighted sum of CE / balanced Dice / per-class Dice on one prediction, one kernel pass.

    spec: {'CrossEntroLoss': w, 'BalanceDiceLoss': w, 'DiceClassLoss': w (class 1), 'DiceClassLoss2': w (class 2),
           'DiceClassLoss0c': w (class 0), 'DiceClassLoss0': w (foreground union 1 - class 0, multi_criterions.py:30-56)}.  Returns (total, {name: w * value}) with values detached: what the reference
    scripts log (`criterions_w * l(...)`, utils_3D_multi_class.py:85; all weights are 1 in the single-class script).
    """
    _DICE = {'DiceClassLoss': 1, 'DiceClassLoss2': 2, 'DiceClassLoss0c': 0, 'DiceClassLoss0': 4}      # 4 = foreground union

    def __init__(self, spec: dict, scale: float = 1.0, scale_dev=None):
        super().__init__()
        unknown = set(spec) - {'CrossEntroLoss', 'BalanceDiceLoss', *self._DICE}
        if unknown:
            raise KeyError(f'no HIP kernel for losses {sorted(unknown)}')
        self.spec = dict(spec)
        self.scale = scale
        self.scale_dev = scale_dev          # 1-element fp32 device tensor: run-time factor on top of `scale` (captured graphs)

    def forward(self, predict, target):
        p = _channels_last(predict)
        C = p.shape[-1]
        lab = _labels(target, C)
        sc = self.scale
        wd = [0.0] * 5
        for name, cls in self._DICE.items():
            if name in self.spec:
                wd[cls] += self.spec[name] * sc
        total, values = ops.level_loss(p, lab, self.spec.get('CrossEntroLoss', 0.0) * sc,
                                       self.spec.get('BalanceDiceLoss', 0.0) * sc, wd, self.scale_dev)
        named = {}
        for name, w in self.spec.items():
            if name == 'CrossEntroLoss':
                v = values[1]
            elif name == 'BalanceDiceLoss':
                v = values[2]
            else:
                v = values[3 + self._DICE[name]]
            named[name] = v if w == 1.0 else v * w
        return total, named


class _Single(nn.Module):
    NAME = None

    def __init__(self):
        super().__init__()
        self.impl = LevelCriterion({self.NAME: 1.0})

    def forward(self, predict, target):
        return self.impl(predict, target)[0]


class CrossEntroLoss(_Single):
    """loss/criterions.py:696-735"""
    NAME = 'CrossEntroLoss'


class DiceClassLoss(_Single):
    """loss/criterions.py:35-70 (class 1)"""
    NAME = 'DiceClassLoss'


class DiceClassLoss2(_Single):
    """loss/multi_criterions.py:85-110 (class 2)"""
    NAME = 'DiceClassLoss2'


class BalanceDiceLoss(_Single):
    """loss/criterions.py:416-442"""
    NAME = 'BalanceDiceLoss'


class DiceClassLoss0(_Single):
    """loss/multi_criterions.py:30-56: Dice of the foreground union (1 - class 0 on both sides)"""
    NAME = 'DiceClassLoss0'


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
}


def get_criterions(name_list):
    """loss/criterions.py:773-782"""
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
    DiceClassLoss / DiceClassLoss2 are the differentiable modules above (train3D_multi_class.py trains with them); Recall,
    Precision, Recall2, Precision2, RecallLoss, PrecisionLoss and the multi-class LocalizationLoss are evaluation-only modules
    over csrc/class_metrics.hip.  Any other name raises KeyError."""
    unknown = [name for name in name_list if name not in Multi_Loss_Dict]
    if unknown:
        raise KeyError(f'no HIP kernel for multi-class criteria {unknown}')
    return {name: Multi_Loss_Dict[name]() for name in name_list}
