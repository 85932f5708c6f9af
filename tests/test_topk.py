"""Top-k cross-entropy, host side: the new name of losses.LevelCriterion, ops.topk_count, the C-ABI surface of csrc/loss_topk.hip
and the float64 restatement of tests/topk_common.py that the GPU tests compare against."""
import os
import re

import numpy as np
import pytest

from tests.topk_common import count_ref, make_labels, make_probs, tied_probs, topk_ref, voxel_losses_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ltu_loss_topk_scratch_elems', 'ltu_loss_topk_fwd', 'ltu_loss_topk_bwd')


# ---------------------------------------------------------------------------------------------- names
def test_level_criterion_accepts_the_name():
    from lintransunet_amd import losses as L
    crit = L.LevelCriterion({'CrossEntroLoss': 10, 'DiceClassLoss': 1, 'TopKCELoss': 1})
    assert crit.topk and crit.topk_fraction == 0.1 and crit.topk_fraction_dev is None and not crit.boundary
    assert L.LevelCriterion({'TopKCELoss': 2.0}, topk_fraction=0.25).topk_fraction == 0.25
    assert not L.LevelCriterion({'CrossEntroLoss': 1}).topk
    with pytest.raises(KeyError):
        L.LevelCriterion({'CrossEntroLoss': 1, 'TopKLoss': 1})
    with pytest.raises(ValueError):
        L.LevelCriterion({'TopKCELoss': 1}, topk_fraction=0.0)


def test_get_criterions_returns_the_module():
    from lintransunet_amd import losses as L
    m = L.get_criterions(['TopKCELoss'])['TopKCELoss']
    assert isinstance(m, L.TopKCELoss) and m.impl.topk_fraction == 0.1
    assert isinstance(L.get_multi_criterions(['TopKCELoss'])['TopKCELoss'], L.TopKCELoss)
    assert L.TopKCELoss(k=25.0).impl.topk_fraction == 0.25


def test_train_knows_the_term():
    from lintransunet_amd import train
    specs = train.level_specs(5, ('CrossEntroLoss', 'TopKCELoss'), criterion_weight=[1, 1])
    assert train.has_topk(specs) and not train.has_topk(train.level_specs(5))


# ---------------------------------------------------------------------------------------------- ops.topk_count
@pytest.mark.parametrize('N', [1, 210, 19980, 270336, 2 ** 31 - 1])
def test_topk_count_formula(N):
    from lintransunet_amd import ops
    for frac in (1.0 / N, 0.1, 0.5, 1.0):
        f32 = float(np.float32(frac))
        want = min(max(int(np.floor(np.float64(f32) * np.float64(N))), 1), N)
        assert ops.topk_count(frac, N) == want == count_ref(frac, N), (frac, N)
    assert ops.topk_count(1.0, N) == N and ops.topk_count(0.5, N) == max(N // 2, 1)


def test_topk_count_clamps_and_fp32_fraction():
    from lintransunet_amd import ops
    N = 270336
    assert ops.topk_count(0.0, N) == 1 and ops.topk_count(-3.0, N) == 1 and ops.topk_count(1e-9, N) == 1
    assert ops.topk_count(2.0, N) == N and ops.topk_count(1.0000001, N) == N
    assert ops.topk_count(float('nan'), N) == N and ops.topk_count(float('inf'), N) == N
    # 0.1 as fp32 is 0.100000001490116: 27033.6004 -> 27033 (0.1 in double gives the same here; as fp32 rounded DOWN it would not)
    assert ops.topk_count(0.1, N) == 27033
    assert ops.topk_count(0.3, 10) == 3               # fp32(0.3) = 0.30000001192: floor(3.0000001) = 3; in double 0.3 * 10 = 3.0 too
    assert ops.topk_count(0.7, 10) == 6               # fp32(0.7) = 0.699999988: the fp32 fraction decides, not the double one


# ---------------------------------------------------------------------------------------------- C-ABI surface
def test_cabi_surface():
    from lintransunet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ltu_hip.h')).read()
    protos = dict(re.findall(r'^(?:int|long long)\s+(ltu_\w+)\s*\(([^;]*)\);', header, flags=re.M | re.S))
    lib = _lib.load()
    for name in NEW:
        assert name in protos and name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in NEW[1:]:
        params = [re.sub(r'/\*.*?\*/', '', a, flags=re.S).strip() for a in protos[name].split(',')]
        names = [p.split()[-1].lstrip('*') for p in params]
        i = names.index('scratch')
        assert names[i + 1] == 'scratch_elems' and params[i + 1].startswith('long long') and _lib.SIGNATURES[name][i + 1] is _lib.L
        assert not {'ws', 'part_ws', 'lnws1'} & set(names)
    assert lib.ltu_loss_topk_scratch_elems.restype is _lib.L
    n = lib.ltu_loss_topk_scratch_elems(2, 105)
    assert n >= 210 and lib.ltu_loss_topk_scratch_elems(0, 105) == 0 and lib.ltu_loss_topk_scratch_elems(2, 2 ** 30) == 0
    src = open(os.path.join(ROOT, 'lintransunet_amd', 'csrc', 'loss_topk.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    assert 'hipDeviceSynchronize' not in code and 'hipStreamSynchronize' not in code and 'hipMemcpy' not in code
    # every atomic of the file adds integers
    assert re.findall(r'atomic\w+\s*\(', code) and all(re.match(r'atomicAdd\s*\(', m) for m in re.findall(r'atomic\w+\s*\(', code))
    assert not re.search(r'atomicAdd\s*\([^;]*(float|double|\df\b)', code)


# ---------------------------------------------------------------------------------------------- the restatement
def test_reference_at_full_fraction_is_the_mean():
    p, lab = make_probs(2, (7, 5, 3), 3, 1), make_labels(2, (7, 5, 3), 3, 2)
    l, _, _ = voxel_losses_ref(p, lab)
    r = topk_ref(p, lab, l.size)
    assert np.isclose(r['value'], l.mean(), rtol=1e-14) and r['tau'] == l.min() and r['n_gt'] + r['n_eq'] == l.size


def test_reference_gradient_sum_and_selection():
    p, lab = make_probs(3, (9, 4, 5), 4, 3), make_labels(3, (9, 4, 5), 4, 4)
    l, pl, _ = voxel_losses_ref(p, lab)
    N = l.size
    for k in (1, count_ref(0.1, N), N // 2, N):
        r = topk_ref(p, lab, k)
        order = np.sort(l)[::-1]
        assert r['tau'] == order[k - 1] and np.isclose(r['value'], order[:k].mean(), rtol=1e-13)      # no ties here: torch.topk's mean
        sel = l >= r['tau']
        assert sel.sum() == k and np.isclose(r['grad'].sum(), -(1.0 / pl[sel]).sum() / k, rtol=1e-12)
        assert (r['grad'] != 0).sum() == k


def test_reference_tie_rule_and_ignored_labels():
    p, lab, grp = tied_probs(2, (9, 6, 11), 3, 5)
    l, pl, _ = voxel_losses_ref(p, lab)
    N = l.size
    n3, n2 = int((grp == 3).sum()), int((grp == 2).sum())
    k = n3 + n2 // 2                                    # strictly inside the 1/4 group
    r = topk_ref(p, lab, k)
    assert r['tau'] == -np.log(0.25) and r['n_gt'] == n3 and r['n_eq'] == n2
    w = -r['grad'].sum(-1).reshape(-1) * pl             # the voxel weights
    assert np.allclose(w[grp.reshape(-1) == 3], 1.0 / k, rtol=1e-14, atol=0) and not w[grp.reshape(-1) < 2].any()
    assert np.allclose(w[grp.reshape(-1) == 2], (k - n3) / (n2 * k), rtol=1e-14, atol=0)
    assert np.isclose(w.sum(), 1.0, rtol=1e-12)         # the k selected weights of 1 / k, however the ties fall
    assert np.isclose(r['value'], (n3 * np.log(8.0) + (k - n3) * np.log(4.0)) / k, rtol=1e-14)
    full = topk_ref(p, lab, N)
    assert full['tau'] == 0.0 and not np.signbit(full['tau']) and np.isclose(full['value'], l.mean(), rtol=1e-14)
    # labels the prediction has no channel for: l = 0, no gradient, counted in N
    lab2 = lab.copy()
    lab2.reshape(-1)[:7] = 200
    l2, _, valid = voxel_losses_ref(p, lab2)
    assert not l2[:7].any() and not valid[:7].any() and l2.size == N
    r2 = topk_ref(p, lab2, N)
    assert not r2['grad'].reshape(N, -1)[:7].any() and np.isclose(r2['value'], l2.sum() / N, rtol=1e-14)
