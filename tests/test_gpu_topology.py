"""The topology family on the device (csrc/thinning.hip, ltu_count_cavities of csrc/components.hip; infer.skeletonize,
infer.betti_numbers, infer.topology_metrics) against the numpy / scipy oracle of tests/topology_common.py.  Predicates, skeletons,
iteration counts and Betti numbers are integers and compared exactly.  The rates of the metric are quotients of exact integers taken
in fp64 and rounded once to f32; the float64 oracle rounded to f32 may differ by the double rounding only: 1 f32 ulp."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, infer  # noqa: E402
from lintransunet_amd.ops import _p, _s  # noqa: E402
import topology_common as tc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ragged():
    """odd extents, W D = 35 not a multiple of 4, object voxels on every face"""
    m = tc.noise((13, 7, 5), 5, sigma=1.2)
    m[0, 3, 2] = m[12, 2, 1] = m[5, 0, 3] = m[6, 6, 0] = m[4, 2, 0] = m[9, 4, 4] = True
    return m


def _single():
    m = np.zeros((5, 6, 7), bool)
    m[2, 3, 4] = True
    return m


VOLUMES = {**{name: row[0] for name, row in tc.TABLE.items()}, 'y_tube': tc.y_tube, 'noise_small': lambda: tc.noise((20, 18, 16), 1),
           'noise_large': lambda: tc.noise((40, 36, 33), 3), 'ragged': _ragged, 'empty': lambda: np.zeros((6, 5, 4), bool),
           'single': _single}
_ORACLE = {}


def _oracle(name):
    """(mask, skeleton, iterations) of a named volume, thinned once per session"""
    if name not in _ORACLE:
        m = VOLUMES[name]()
        _ORACLE[name] = (m,) + tc.thin(m)
    return _ORACLE[name]


def test_simple_codes_match_the_oracle():
    codes = np.concatenate([tc.sample_codes(19000, 21, ('random', 'sparse', 'dense')), tc.few_bit_codes(),
                            tc.few_bit_codes()[:48] | tc.CENTRE])        # the centre bit is ignored
    assert len(codes) == 60000
    want = tc.flags_of(codes)
    assert 0.05 < np.mean(want & 1) < 0.95 and (want & 2).any()
    flags = torch.empty(len(codes), device=DEV, dtype=torch.uint8)
    _lib.call('ltu_thin_simple_codes', _p(_dev(codes.astype(np.uint32))), _p(flags), len(codes), _s())
    got = flags.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(hex(int(codes[i])), int(got[i]), int(want[i])) for i in bad[:5]]


@pytest.mark.parametrize('name', sorted(VOLUMES))
def test_skeletonize_equals_the_sequential_oracle(name):
    m, want, iterations = _oracle(name)
    if name in tc.TABLE:
        assert (int(want.sum()), iterations) == tc.TABLE[name][2:4]
    if name == 'ragged':
        assert m.shape[1] * m.shape[2] % 4 and all(m.take(i, axis=a).any() for a in range(3) for i in (0, -1))
    if name in ('empty', 'single'):
        assert iterations == 0 and np.array_equal(want, m)
    src = _dev(m.astype(np.uint8))[None]
    got, its = infer.skeletonize(src)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1,) + m.shape
    assert np.array_equal(src[0].cpu().numpy(), m.astype(np.uint8))             # the input is left alone
    assert np.array_equal(got[0].cpu().numpy(), want)
    assert its == iterations
    again, its2 = infer.skeletonize(src)
    assert torch.equal(again, got) and its2 == its                               # two calls, the same bytes


def test_skeletonize_batch_dtypes_and_five_dims():
    """three different volumes in one call (padded to one shape); the thinning of each is its own"""
    names = ('torus', 'y_tube', 'noise_small')
    shape = tuple(max(_oracle(n)[0].shape[a] for n in names) for a in range(3))
    batch = np.zeros((3,) + shape, bool)
    for i, n in enumerate(names):
        m = _oracle(n)[0]
        batch[(i,) + tuple(slice(0, s) for s in m.shape)] = m
    thinned = [tc.thin(b) for b in batch]            # of the padded volumes: the subfields follow the coordinates, the border moved
    want = np.stack([sk for sk, _ in thinned])
    its_want = max(its for _, its in thinned)        # an iteration counts when it deleted a voxel in any volume
    assert len({its for _, its in thinned}) > 1
    for t in (_dev(batch), _dev(batch.astype(np.float32) * 2.5), _dev(batch.astype(np.int64) * -3), _dev(batch.astype(np.uint8) * 7)[:, None]):
        got, its = infer.skeletonize(t)
        assert np.array_equal(got.cpu().numpy(), want) and its == its_want


def test_skeleton_of_a_many_workgroup_volume_keeps_the_topology():
    m = tc.noise((96, 80, 64), 9, sigma=2.5)
    src = _dev(m.astype(np.uint8))[None]
    got, its = infer.skeletonize(src)
    sk = got[0].cpu().numpy().astype(bool)
    assert its > 0 and sk.sum() < m.sum() and not (sk & ~m).any()
    again, its2 = infer.skeletonize(got)
    assert its2 == 0 and torch.equal(again, got)
    want = tc.betti(m)
    assert tc.betti(sk) == want
    b = infer.betti_numbers(torch.cat([src, got]))
    for i, key in enumerate(('Betti0', 'Betti1', 'Betti2', 'Euler')):
        assert b[key].dtype == torch.int32 and b[key].tolist() == [want[i], want[i]], key


BETTI_VOLUMES = {**{name: row[0] for name, row in tc.TABLE.items()}, 'linked_tori': tc.linked_tori,
                 'shell_with_ball': tc.shell_with_ball, 'cut_noise': tc.cut_noise, 'ragged': _ragged,
                 'empty': lambda: np.zeros((6, 5, 4), bool), 'single': _single}


@pytest.mark.parametrize('name', sorted(BETTI_VOLUMES))
def test_betti_numbers_match_scipy(name):
    m = BETTI_VOLUMES[name]()
    want = tc.betti(m)
    if name in tc.TABLE:
        assert want[:3] == tc.TABLE[name][4]
    if name == 'shell_with_ball':
        assert want[:3] == (2, 0, 1)
    if name == 'linked_tori':
        assert want[:3] == (2, 2, 0)
    flipped = m[::-1, :, ::-1]                        # a second sample in the call: another raster order, the same numbers
    got = infer.betti_numbers(_dev(np.stack([m, flipped]).astype(np.uint8)))
    again = infer.betti_numbers(_dev(np.stack([m, flipped]).astype(np.float32))[:, None])
    for i, key in enumerate(('Betti0', 'Betti1', 'Betti2', 'Euler')):
        assert got[key].tolist() == [want[i], want[i]], (key, got[key].tolist(), want)
        assert torch.equal(got[key], again[key])


def _ulp_close(got, want64):
    want = np.float32(want64)
    return abs(np.float32(got) - want) <= np.spacing(want)


def test_topology_metrics_match_float64_on_oracle_skeletons():
    """B = 2, two classes, a vote volume with a threshold; column order follows class_indices"""
    shape = (20, 18, 16)
    rs = np.random.RandomState(4)
    g1, g2 = tc.noise(shape, 1), tc.noise(shape, 2) & ~tc.noise(shape, 1)
    labels = np.stack([np.where(g1, 1, np.where(g2, 2, 0)), np.where(np.roll(g1, 2, 0), 1, 0)]).astype(np.int64)
    votes = rs.rand(2, 3, *shape).astype(np.float32) * 0.3
    votes[0, 1][np.roll(g1, 1, 1)] += 0.5             # class 1 of sample 0: the label moved by a voxel
    votes[0, 2][g2] += 0.5                            # class 2 of sample 0: the label itself
    votes[1, 1][tc.noise(shape, 6)] += 0.5            # class 1 of sample 1: unrelated blobs; class 2 of sample 1: nothing on either side
    thr, classes = 0.4, (2, 1)
    got = infer.topology_metrics(_dev(votes), _dev(labels)[:, None], class_indices=classes, threshold=thr)
    assert tuple(got) == infer.TOPOLOGY_METRIC_NAMES
    for b in range(2):
        for j, k in enumerate(classes):
            p, g = votes[b, k] >= np.float32(thr), labels[b] == k
            want = tc.cldice(p, g, tc.thin(p)[0].astype(bool), tc.thin(g)[0].astype(bool))
            for name, w in zip(infer.TOPOLOGY_METRIC_NAMES[:3], want):
                v = got[name][b, j].item()
                assert got[name].dtype == torch.float32 and _ulp_close(v, w), (b, k, name, v, w)
            bp, bg = tc.betti(p), tc.betti(g)
            for i in range(3):
                e = got[f'Betti{i}Error']
                assert e.dtype == torch.int32 and e[b, j].item() == abs(bp[i] - bg[i]), (b, k, i)
    assert got['clDice'][0, 0].item() == 1.0 and got['clDice'][1, 0].item() == 1.0      # identical; both empty
    assert 0.0 < got['clDice'][0, 1].item() < 1.0
    again = infer.topology_metrics(_dev(votes), _dev(labels)[:, None], class_indices=classes, threshold=thr)
    assert all(torch.equal(got[n], again[n]) for n in got)


def test_topology_metrics_empty_cases_and_a_break():
    shape = (12, 20, 9)
    h, w, d = np.mgrid[:shape[0], :shape[1], :shape[2]]
    tube = (h - 6) ** 2 + (d - 4) ** 2 <= 3 ** 2
    gap = tube & ~((w >= 9) & (w < 11))               # the tube with a two-voxel gap
    zero = np.zeros(shape, bool)
    pred = np.stack([gap, zero, zero, tube]).astype(np.float32)[:, None].repeat(2, 1)      # [4, 2, ...], class 1 is judged
    labels = np.stack([tube, zero, tube, zero]).astype(np.uint8)[:, None]
    got = infer.topology_metrics(_dev(pred), _dev(labels))
    assert tuple(got['clDice'].shape) == (4, 1)
    for name in infer.TOPOLOGY_METRIC_NAMES[:3]:
        assert got[name][1:, 0].tolist() == [1.0, 0.0, 0.0], name                        # both empty; P empty; G empty
    assert got['Betti0Error'][:, 0].tolist() == [1, 0, 1, 1] and got['Betti1Error'].abs().sum().item() == 0
    sp, sg = tc.thin(gap)[0].astype(bool), tc.thin(tube)[0].astype(bool)
    want = tc.cldice(gap, tube, sp, sg)
    assert want[1] == 1.0 and want[2] < 1.0           # the break costs sensitivity only
    for name, wv in zip(infer.TOPOLOGY_METRIC_NAMES[:3], want):
        assert _ulp_close(got[name][0, 0].item(), wv), name


def test_refusals_on_the_device():
    m = torch.zeros((2, 5, 4, 3), device=DEV, dtype=torch.uint8)
    with pytest.raises(_lib.LtuError):
        infer.skeletonize(m[0])
    with pytest.raises(_lib.LtuError):
        infer.betti_numbers(m[0, 0])
    with pytest.raises(_lib.LtuError):
        infer.topology_metrics(torch.zeros((1, 2, 5, 4, 3), device=DEV), m[:1, None], class_indices=(2,))
    with pytest.raises(_lib.LtuError):
        infer.topology_metrics(torch.zeros((1, 2, 5, 4, 3), device=DEV), m[:, None])
