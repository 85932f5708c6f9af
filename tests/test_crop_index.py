"""The crop index's host side (data.class_crop_centers, the draws data.CropIndex shares with it) and its C-ABI surface
(include/ltu_hip.h, csrc/crop_index.hip): everything that needs no device."""
import os
import re
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, data  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('ltu_crop_index_elems', 'ltu_crop_index_build', 'ltu_crop_index_select')


def _same_state(a, b):
    a, b = a.get_state(), b.get_state()
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _label(shape=(9, 7, 5), values=(0, 0, 0, 1, 2, 4), seed=0):
    return np.random.RandomState(seed).choice(np.asarray(values, dtype=np.uint8), size=shape)


def test_class_centres_lie_in_the_drawn_class():
    """a patch of one voxel needs no correction: the centre is the drawn voxel itself, and its class is the drawn class"""
    lab = _label()
    rs, replay = np.random.RandomState(3), np.random.RandomState(3)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                      # class 3 is empty
        got = data.class_crop_centers(lab, (1, 1, 1), 300, rand_state=rs)
    classes = replay.choice(5, size=300, p=np.array([1, 1, 1, 0, 1]) / 4)
    assert [int(lab[tuple(c)]) for c in got] == classes.tolist()
    assert set(classes.tolist()) == {0, 1, 2, 4}
    # the rank-th voxel of the class in raster order, through correct_crop_centers for a real patch
    rs, replay = np.random.RandomState(5), np.random.RandomState(5)
    got = data.class_crop_centers(lab, (4, 3, 2), 40, ratios=[1, 2, 3], num_classes=3, rand_state=rs)
    classes = replay.choice(3, size=40, p=np.array([1, 2, 3]) / 6)
    for c, centre in zip(classes, got):
        idx = np.nonzero((lab == c).ravel())[0]
        want = np.unravel_index(idx[replay.randint(len(idx))], lab.shape)
        assert centre == data.correct_crop_centers(list(want), (4, 3, 2), lab.shape)
    assert _same_state(rs, replay)


def test_zero_ratio_and_empty_class_are_never_drawn():
    lab = _label()
    got = data.class_crop_centers(lab, (1, 1, 1), 200, ratios=[1, 0, 1], num_classes=3, rand_state=np.random.RandomState(1))
    assert {int(lab[tuple(c)]) for c in got} == {0, 2}
    with pytest.warns(UserWarning, match='class 3'):
        got = data.class_crop_centers(lab, (1, 1, 1), 200, ratios=[0, 1, 1, 5, 1], rand_state=np.random.RandomState(2))
    assert {int(lab[tuple(c)]) for c in got} == {1, 2, 4}
    ratios = [1, 1, 1, 1, 1]
    with pytest.warns(UserWarning):
        data.class_crop_centers(lab, (1, 1, 1), 1, ratios=ratios, rand_state=np.random.RandomState(2))
    assert ratios == [1, 1, 1, 1, 1]                          # the caller's list is not edited
    # the default number of classes: the highest class below 8 that is present, + 1; values >= 8 are no class
    lab2 = lab.copy()
    lab2[0, 0, 0] = 200
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        a = data.class_crop_centers(lab2, (1, 1, 1), 50, num_classes=5, rand_state=np.random.RandomState(4))
        b = data.class_crop_centers(lab2, (1, 1, 1), 50, rand_state=np.random.RandomState(4))
    assert a == b


def test_bad_ratios_raise():
    lab = _label()
    with pytest.raises(ValueError):
        data.class_crop_centers(lab, (1, 1, 1), 4, ratios=[1, -1, 1], num_classes=3)
    with pytest.raises(ValueError):
        data.class_crop_centers(lab, (1, 1, 1), 4, ratios=[1, 1], num_classes=3)
    with pytest.raises(ValueError):
        data.class_crop_centers(lab, (1, 1, 1), 0, num_classes=3)
    with pytest.raises(ValueError):                           # a patch larger than the label: correct_crop_centers
        data.class_crop_centers(lab, (10, 1, 1), 1, num_classes=3)


@pytest.mark.parametrize('num_samples', [1, 7])
def test_class_centres_consume_exactly_the_listed_draws(num_samples):
    """one rs.choice(len(ratios), size=num_samples, p=...), then one rs.randint(population) per sample: nothing else"""
    lab = _label(seed=6)
    rs, replay = np.random.RandomState(11), np.random.RandomState(11)
    data.class_crop_centers(lab, (3, 3, 3), num_samples, ratios=[2, 1, 1], num_classes=3, rand_state=rs)
    classes = replay.choice(3, size=num_samples, p=np.array([2, 1, 1]) / 4)
    for c in classes:
        replay.randint(int((lab == c).sum()))
    assert _same_state(rs, replay)
    replay.randint(5)
    assert not _same_state(rs, replay)


def test_posneg_queries_repeat_crop_centers_draws():
    """the draws CropIndex.centers makes from the two populations are crop_centers' draws: same ranks, same generator state"""
    for lab in (_label(seed=7), np.zeros((4, 4, 4), np.uint8), np.full((4, 4, 4), 9, np.uint8)):
        flat = (lab > 0).ravel()
        fg, bg = np.nonzero(flat)[0], np.nonzero(~flat)[0]
        rs, ref = np.random.RandomState(8), np.random.RandomState(8)
        q = data._posneg_queries(len(fg), len(bg), 60, 0.7, 0.3, rs)
        got = [list(np.unravel_index((fg if m == data.FG_MASK else bg)[r], lab.shape)) for m, r in q]
        want = data.crop_centers(lab, (1, 1, 1), 60, rand_state=ref)
        assert got == want
        assert _same_state(rs, ref)
    with pytest.raises(ValueError, match='No sampling location available.'):
        data._posneg_queries(0, 0, 1, 0.7, 0.3, np.random.RandomState(0))


def test_cabi_surface():
    header = open(os.path.join(ROOT, 'include', 'ltu_hip.h')).read()
    declared = {n: t for t, n in re.findall(r'^(int|long long)\s+(ltu_\w+)\s*\(', header, flags=re.M)}
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert declared['ltu_crop_index_elems'] == 'long long'
    assert lib.ltu_crop_index_elems.restype is _lib.L
    assert 'crop_index.hip' in open(os.path.join(ROOT, 'lintransunet_amd', 'csrc', 'Makefile')).read()


def test_cabi_refusals_without_launch():
    """n_voxels outside 1 .. 2^32 - 1, a short index buffer, a NULL pointer and a misaligned label are refused before any HIP call;
    the size query answers 0 for the refused sizes"""
    lib = _lib.load()
    fake = 1 << 20                                            # never dereferenced: every call below is refused
    n = 24679
    elems = lib.ltu_crop_index_elems(n)
    assert elems == 9 * (-(-n // 4096) + 1) == 72
    assert lib.ltu_crop_index_elems(1) == 18 and lib.ltu_crop_index_elems(4096) == 18 and lib.ltu_crop_index_elems(4097) == 27
    assert lib.ltu_crop_index_elems(2 ** 32 - 1) == 9 * (2 ** 20 + 1)
    for bad in (0, -1, 2 ** 32, 2 ** 40):
        assert lib.ltu_crop_index_elems(bad) == 0
        assert lib.ltu_crop_index_build(fake, bad, fake, 1 << 40, fake, None) == -2               # LTU_E_SHAPE
        assert lib.ltu_crop_index_select(fake, bad, fake, 1 << 40, fake, fake, 4, None) == -2
    bd = [fake, n, fake, elems, fake, None]                   # lab, n_voxels, index, index_elems, totals, s
    sl = [fake, n, fake, elems, fake, fake, 4, None]          # lab, n_voxels, index, index_elems, queries, out, n, s
    assert lib.ltu_crop_index_build(*bd[:3], elems - 1, *bd[4:]) == -4                            # short index: LTU_E_ARG
    assert lib.ltu_crop_index_select(*sl[:3], elems - 1, *sl[4:]) == -4
    for i in (0, 2, 4):
        assert lib.ltu_crop_index_build(*bd[:i], None, *bd[i + 1:]) == -4, i                      # NULL pointer: LTU_E_ARG
    for i in (0, 2, 4, 5):
        assert lib.ltu_crop_index_select(*sl[:i], None, *sl[i + 1:]) == -4, i
    assert lib.ltu_crop_index_select(*sl[:6], -1, None) == -4
    assert lib.ltu_crop_index_build(fake + 8, *bd[1:]) == -3                                      # LTU_E_ALIGN
    assert lib.ltu_crop_index_select(fake + 8, *sl[1:]) == -3
    assert lib.ltu_crop_index_select(*sl[:5], fake + 4, *sl[6:]) == -3
    assert lib.ltu_crop_index_select(*sl[:6], 0, None) == 0                                       # nothing to do: no launch


def test_crop_index_of_a_cpu_tensor_raises():
    with pytest.raises(_lib.LtuError):
        data.CropIndex(torch.zeros((4, 4, 4), dtype=torch.uint8))
    with pytest.raises(_lib.LtuError):
        data.CropIndex(np.zeros((4, 4, 4), dtype=np.uint8))
