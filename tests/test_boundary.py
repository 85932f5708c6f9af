"""Boundary loss, host side: the float64 restatement (tests/boundary_common.py) on volumes whose maps can be written down by hand,
the new names of losses.LevelCriterion, and the argument contract of the five C-ABI entry points (csrc/distmap.hip,
csrc/loss_boundary.hip), which refuse before anything is launched and therefore need no GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.boundary_common import boundary_grad_ref, boundary_values_ref, make_labels, phi_ref, phi_ref_batch

E_SHAPE, E_ARG = -2, -4
FAKE = 0x1000          # a non-null, 8-byte aligned "device pointer": every call below returns before it would be used


# ---------------------------------------------------------------------------------------------- the restatement
def test_single_corner_voxel_of_512x3x2():
    lab = np.zeros((512, 3, 2), np.uint8)
    lab[0, 0, 0] = 1
    phi = phi_ref(lab, 1)
    assert phi[0, 0, 0] == 0.0                                    # inside: -(1 - 1)
    assert phi[511, 2, 1] == math.sqrt(511 ** 2 + 2 ** 2 + 1 ** 2)
    assert phi[7, 0, 0] == 7.0 and phi[0, 2, 0] == 2.0 and phi[0, 0, 1] == 1.0
    # the complement: class 0 is everything but that voxel
    phi0 = phi_ref(lab, 0)
    assert phi0[0, 0, 0] == 1.0 and phi0[1, 0, 0] == 0.0
    assert phi0[5, 1, 1] == -(math.sqrt(5 ** 2 + 1 + 1) - 1.0)


def test_three_voxel_slab():
    lab = np.zeros((9, 4, 3), np.uint8)
    lab[3:6] = 1
    phi = phi_ref(lab, 1)
    want = np.array([3, 2, 1, 0, -1, 0, 1, 2, 3], np.float64)     # inside -(d - 1): 0 at the faces, -1 in the middle plane
    assert np.array_equal(phi, np.broadcast_to(want[:, None, None], phi.shape))
    lab = np.zeros((9, 4, 3), np.uint8)
    lab[0:3] = 1                                                  # a slab at the border: distances are taken inside the patch only
    want = np.array([-2, -1, 0, 1, 2, 3, 4, 5, 6], np.float64)
    assert np.array_equal(phi_ref(lab, 1), np.broadcast_to(want[:, None, None], phi.shape))


def test_anisotropic_spacing():
    lab = np.zeros((6, 6, 6), np.uint8)
    lab[2, 2, 2] = 1
    phi = phi_ref(lab, 1, (0.5, 0.5, 2.0))
    assert phi[2, 2, 2] == -(0.5 - 1.0)                           # nearest outside voxel 0.5 away; the 1 is not scaled
    assert phi[5, 2, 2] == 1.5 and phi[2, 0, 2] == 1.0 and phi[2, 2, 4] == 4.0
    assert phi[4, 2, 3] == math.sqrt(1.0 ** 2 + 2.0 ** 2)


def test_empty_and_full_class_are_zero():
    lab = np.full((5, 4, 3), 2, np.uint8)
    assert not phi_ref(lab, 1).any() and not phi_ref(lab, 2).any()
    labs = make_labels((12, 6, 5))
    phi = phi_ref_batch(labs, (1, 2, 3))
    assert phi.shape == (2, 3, 12, 6, 5)
    assert not phi[0, 2].any() and not phi[1].any()              # class 3: absent in sample 0, all of sample 1
    assert phi[0, 0].min() < 0 < phi[0, 0].max()


def test_values_and_gradient_restatement():
    rng = np.random.default_rng(3)
    p = rng.random((2, 4, 3, 2, 3))
    phi = rng.standard_normal((2, 2, 4, 3, 2))
    v = boundary_values_ref(p, phi, (2, 0))
    assert np.isclose(v[0], (p[..., 2] * phi[:, 0]).sum() / 48) and np.isclose(v[1], (p[..., 0] * phi[:, 1]).sum() / 48)
    g = boundary_grad_ref(p.shape, phi, (2, 0), (0.5, 2.0), g=3.0)
    assert not g[..., 1].any() and np.allclose(g[..., 2], 1.5 * phi[:, 0] / 48) and np.allclose(g[..., 0], 6.0 * phi[:, 1] / 48)


# ---------------------------------------------------------------------------------------------- LevelCriterion
def test_level_criterion_names():
    from lintransunet_amd import losses as L
    names = ['BoundaryLoss0c', 'BoundaryLoss'] + [f'BoundaryLoss{c}' for c in range(2, 8)]
    crit = L.LevelCriterion({'CrossEntroLoss': 1.0, **{n: 0.01 for n in names}}, spacing=(0.5, 0.5, 2.0))
    assert crit.boundary == names and crit.boundary_classes == tuple(range(8)) and crit.spacing == (0.5, 0.5, 2.0)
    assert [L.boundary_name(c) for c in range(8)] == names
    assert not L.LevelCriterion({'CrossEntroLoss': 1.0, 'DiceClassLoss': 1.0}).boundary
    with pytest.raises(KeyError):
        L.LevelCriterion({'BoundaryLoss8': 1.0})
    with pytest.raises(KeyError):
        L.LevelCriterion({'BoundaryLoss': 1.0, 'HausdorffLoss': 1.0})
    with pytest.raises(ValueError):
        L.boundary_name(8)
    assert isinstance(L.get_criterions(['BoundaryLoss'])['BoundaryLoss'], L.BoundaryLoss)
    assert isinstance(L.get_multi_criterions(['BoundaryLoss'])['BoundaryLoss'], L.BoundaryLoss)
    assert L.BoundaryLoss(class_index=2, spacing=(1, 1, 3)).impl.boundary_classes == (2,)


def test_absent_class_raises_before_any_launch():
    """CPU tensors: anything that reached a kernel would raise LtuError ('must live on the GPU'), not ValueError"""
    from lintransunet_amd import losses as L
    predict = torch.full((1, 3, 4, 4, 4), 1.0 / 3)
    target = torch.zeros((1, 1, 4, 4, 4), dtype=torch.uint8)
    for spec in ({'CrossEntroLoss': 1.0, 'BoundaryLoss3': 0.01}, {'BoundaryLoss7': 1.0}, {'FocalLoss': 1.0, 'BoundaryLoss4': 0.01}):
        with pytest.raises(ValueError, match='boundary term of a class'):
            L.LevelCriterion(spec)(predict, target)
    with pytest.raises(ValueError):
        L.BoundaryLoss(class_index=3)(predict, target)


def test_train_helpers_leave_plain_specs_alone():
    from lintransunet_amd import train
    assert not train.has_boundary(train.level_specs(5))
    specs = train.level_specs(5, ('CrossEntroLoss', 'DiceClassLoss', 'BoundaryLoss', 'BoundaryLoss2'), criterion_weight=[10, 1, 0.01, 0.01])
    assert train.has_boundary(specs) and all('BoundaryLoss2' in s for s in specs)


# ---------------------------------------------------------------------------------------------- the C-ABI's argument contract
@pytest.fixture(scope='module')
def lib():
    from lintransunet_amd import _lib
    return _lib.load()


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def _floats(*v):
    return (ctypes.c_float * len(v))(*v)


def _distmap(lib, classes=(1, 2), B=2, H=8, W=8, D=8, sp=(1.0, 1.0, 1.0), label=FAKE, phi=FAKE, scratch=FAKE, elems=None, K=None):
    K = len(classes) if K is None else K
    elems = lib.ltu_distmap_scratch_elems(B, max(K, 1), H, W, D) if elems is None else elems
    return lib.ltu_distmap_signed(label, _ints(*classes), K, phi, scratch, elems, B, H, W, D, *sp, None)


def test_distmap_argument_errors(lib):
    assert _distmap(lib, H=513) == E_SHAPE and _distmap(lib, W=513) == E_SHAPE and _distmap(lib, D=513) == E_SHAPE
    assert _distmap(lib, H=0) == E_SHAPE and _distmap(lib, B=0) == E_SHAPE
    assert _distmap(lib, classes=(1,) * 9) == E_SHAPE and _distmap(lib, classes=(1,), K=0) == E_SHAPE
    assert _distmap(lib, classes=(1, 2, 1)) == E_ARG                       # a repeated id
    assert _distmap(lib, classes=(1, 256)) == E_ARG and _distmap(lib, classes=(-1,)) == E_ARG
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        for axis in range(3):
            sp = [1.0, 1.0, 1.0]
            sp[axis] = bad
            assert _distmap(lib, sp=tuple(sp)) == E_ARG, (bad, axis)
    need = lib.ltu_distmap_scratch_elems(2, 2, 8, 8, 8)
    assert _distmap(lib, elems=need - 1) == E_ARG                          # short scratch
    # null device pointers: the shape and argument errors still answer with their own code, a clean call with E_ARG
    assert _distmap(lib, H=513, label=None, phi=None, scratch=None) == E_SHAPE
    assert _distmap(lib, classes=(3, 3), label=None, phi=None, scratch=None) == E_ARG
    assert _distmap(lib, label=None) == E_ARG and _distmap(lib, phi=None) == E_ARG and _distmap(lib, scratch=None) == E_ARG


def _bfwd(lib, classes=(1, 2), w=(1.0, 1.0), B=2, S=1000, C=3, p=FAKE, phi=FAKE, sums=FAKE, values=FAKE, floats=None):
    K = len(classes)
    floats = lib.ltu_loss_boundary_sums_floats(B, S, max(K, 1)) if floats is None else floats
    return lib.ltu_loss_boundary_fwd(p, phi, _ints(*classes), _floats(*w), K, sums, floats, values, None, None, None, B, S, C, None)


def _bbwd(lib, classes=(1, 2), w=(1.0, 1.0), B=2, S=1000, C=3, phi=FAKE, g=FAKE, dp=FAKE, acc=0):
    return lib.ltu_loss_boundary_bwd(phi, _ints(*classes), _floats(*w), len(classes), None, None, g, dp, acc, B, S, C, None)


def test_loss_boundary_argument_errors(lib):
    for fn in (_bfwd, _bbwd):
        assert fn(lib, classes=(1, 3)) == E_ARG                            # a class the prediction does not have
        assert fn(lib, classes=(-1, 1)) == E_ARG
        assert fn(lib, w=(1.0, float('nan'))) == E_ARG and fn(lib, w=(float('inf'), 1.0)) == E_ARG
        assert fn(lib, C=1) == E_SHAPE and fn(lib, C=9) == E_SHAPE
        assert fn(lib, classes=(0,) * 9, w=(1.0,) * 9, C=8) == E_SHAPE
        assert fn(lib, B=0) == E_SHAPE and fn(lib, S=0) == E_SHAPE
        assert fn(lib, phi=None) == E_ARG
        assert fn(lib, classes=(1, 5), phi=None) == E_ARG and fn(lib, C=9, phi=None) == E_SHAPE
    assert _bfwd(lib, floats=lib.ltu_loss_boundary_sums_floats(2, 1000, 2) - 1) == E_ARG      # short sums
    assert _bfwd(lib, p=None) == E_ARG and _bfwd(lib, sums=None) == E_ARG and _bfwd(lib, values=None) == E_ARG
    assert _bbwd(lib, g=None) == E_ARG and _bbwd(lib, dp=None, acc=1) == E_ARG


def test_size_queries_positive_and_monotone(lib):
    """positive, and never smaller for a larger argument (a caller may size its scratch once for its largest shape)"""
    base = dict(B=2, K=2, H=16, W=16, D=16)
    q = lambda **kw: lib.ltu_distmap_scratch_elems(*[dict(base, **kw)[k] for k in ('B', 'K', 'H', 'W', 'D')])
    assert q() > 0
    for k, top in (('B', 9), ('K', 9), ('H', 513), ('W', 513), ('D', 513)):
        vals = [q(**{k: v}) for v in range(1, top)]
        assert vals[0] > 0 and all(a <= b for a, b in zip(vals, vals[1:])), k
    assert q(B=4) > q(B=2) and q(K=4) > q(K=2)
    s = lib.ltu_loss_boundary_sums_floats
    assert s(1, 1, 1) > 0
    for vals in ([s(b, 5000, 2) for b in range(1, 9)], [s(2, 5000, k) for k in range(1, 9)],
                 [s(2, n, 2) for n in (1, 255, 256, 257, 6660, 10 ** 5, 2 ** 21, 2 ** 31 + 5, 2 ** 33)]):
        assert vals[0] > 0 and all(a <= b for a, b in zip(vals, vals[1:]))
    assert s(4, 5000, 2) > s(2, 5000, 2) and s(2, 5000, 4) > s(2, 5000, 2) and s(2, 10 ** 5, 2) > s(2, 1000, 2)
