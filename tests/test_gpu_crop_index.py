"""The crop index on the device (csrc/crop_index.hip, data.CropIndex) against numpy on the host copy of the label.  Every
comparison is exact: voxel indices, centres, generator states, and bit-equal patches."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import data, nifti  # noqa: E402

DEV = 'cuda'
BLOCK = 4096                                          # voxels per block of the index
VALUES = np.array([0, 1, 2, 5, 7, 9, 255], dtype=np.uint8)
SETS = [1 << b for b in range(9)] + [data.FG_MASK]   # every single bin (bin 0 = the background) and the foreground union


def _edge(shape, members, value=1):
    lab = np.zeros(shape, np.uint8)
    lab.ravel()[list(members)] = value
    return lab


def _labels():
    """name -> host label; 5 blocks of 64 x 16 x 20 for the labels built to sit on block edges"""
    rs = np.random.RandomState(0)
    e, ne = (64, 16, 20), 64 * 16 * 20
    return {
        'random': rs.choice(VALUES, size=(37, 29, 23)),                         # 24 679 voxels: 6 full blocks and a partial one
        'tiny': rs.choice(VALUES, size=(5, 4, 3)),                              # one partial block
        'two_blocks': rs.choice(VALUES, size=(32, 16, 16)),                     # exactly 2 * 4096
        'first_voxel': _edge((37, 29, 23), [0]),
        'last_voxel': _edge((37, 29, 23), [37 * 29 * 23 - 1], 200),
        'gap': _edge(e, [5, 4 * BLOCK + 77], 3),                                # three blocks without a member between two members
        'block_seam': _edge(e, [2 * BLOCK - 1, 2 * BLOCK], 7),                  # the last voxel of a block and the first of the next
        'all_fg': np.full((37, 29, 23), 2, np.uint8),
        'all_bg': np.zeros((37, 29, 23), np.uint8),
        'last_lane': _edge(e, list(range(ne - 70, ne)) + [63, 64, 4095], 9),    # strips' last bytes, the last lane of a block
    }


LABELS = _labels()
_INDEX = {}


def _index(name):
    if name not in _INDEX:
        _INDEX[name] = data.CropIndex(torch.from_numpy(LABELS[name]).to(DEV))
    return _INDEX[name]


def _members(lab, mask):
    return np.nonzero(((mask >> np.minimum(lab.ravel(), 8).astype(np.int64)) & 1) != 0)[0]


def _same_state(a, b):
    a, b = a.get_state(), b.get_state()
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _check_selects(idx, lab):
    flat = lab.ravel()
    assert idx.counts == tuple(int(c) for c in np.bincount(np.minimum(flat, 8), minlength=9))
    assert idx.n_background == int((flat == 0).sum()) and idx.n_foreground == int((flat > 0).sum())
    assert idx.shape == lab.shape
    for mask in SETS:
        want = _members(lab, mask)
        got = idx.select([(mask, r) for r in range(len(want) + 1)])            # every rank, and rank = population
        assert got.dtype == np.int64 and got[-1] == -1, mask
        assert np.array_equal(got[:-1], want), mask
    # a few unions of classes, the empty set, and ranks far beyond the population
    for mask in (0x006, 0x1a1, 0x1ff):
        want = _members(lab, mask)
        ranks = np.unique(np.linspace(0, max(len(want) - 1, 0), 50).astype(np.int64))[:len(want)]
        assert np.array_equal(idx.select([(mask, int(r)) for r in ranks]), want[ranks]), mask
    assert np.array_equal(idx.select([(0, 0), (data.FG_MASK, 2 ** 32 - 1), (1, len(flat))]), [-1, -1, -1])


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(LABELS))
def test_select_every_rank_of_every_set(name):
    _check_selects(_index(name), LABELS[name])


@pytest.mark.gpu
def test_tail_beyond_n_voxels_is_neither_loaded_nor_counted():
    """the label is the prefix of a longer buffer of ones and holds no 1 itself: a lane or a byte read beyond n shows in bin 1"""
    n = 37 * 29 * 23
    assert n % BLOCK and n % 16
    host = np.random.RandomState(1).choice(np.array([0, 2, 3, 8], np.uint8), size=n)
    buf = torch.ones(7 * BLOCK + 64, dtype=torch.uint8, device=DEV)
    buf[:n] = torch.from_numpy(host).to(DEV)
    idx = data.CropIndex(buf[:n].view(37, 29, 23))
    assert idx.lab.data_ptr() == buf.data_ptr()
    assert idx.counts[1] == 0
    _check_selects(idx, host.reshape(37, 29, 23))
    assert torch.equal(buf[n:], torch.ones_like(buf[n:]))


def _sizes(shape):
    """the label's own shape, odd extents, one voxel, and an even patch"""
    return [tuple(shape), tuple(min(n, k) for n, k in zip(shape, (5, 3, 7))), (1, 1, 1), tuple(min(n, 4) for n in shape)]


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(LABELS))
def test_centers_equal_the_host_draw_for_draw(name):
    lab, idx = LABELS[name], _index(name)
    for seed, size in enumerate(_sizes(lab.shape)):
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        want = data.crop_centers(lab, size, 200, rand_state=a)
        got = idx.centers(size, 200, rand_state=b)
        assert got == want, size
        assert all(type(v) is int for c in got for v in c)
        assert _same_state(a, b), size
    a, b = np.random.RandomState(9), np.random.RandomState(9)
    assert idx.centers((3, 3, 3), 50, pos=0.2, neg=1.3, rand_state=b) == data.crop_centers(lab, (3, 3, 3), 50, 0.2, 1.3, rand_state=a)
    assert _same_state(a, b)


@pytest.mark.gpu
def test_empty_label_raises_as_the_host_does():
    lab = np.zeros((0, 4, 4), np.uint8)
    idx = data.CropIndex(torch.from_numpy(lab).to(DEV))
    assert idx.counts == (0,) * 9
    for draw in (lambda: data.crop_centers(lab, (1, 1, 1), 2, rand_state=np.random.RandomState(0)),
                 lambda: idx.centers((1, 1, 1), 2, rand_state=np.random.RandomState(0))):
        with pytest.raises(ValueError, match='No sampling location available.'):
            draw()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['random', 'tiny', 'two_blocks', 'gap', 'all_fg', 'all_bg'])
def test_class_centers_equal_the_host(name):
    lab, idx = LABELS[name], _index(name)
    cases = [dict(), dict(num_classes=3), dict(ratios=[1, 0, 2], num_classes=3), dict(ratios=[1, 0, 2, 1, 1, 3, 1, 1], num_classes=8),
             dict(ratios=[0.5, 0.25, 4.0, 1.0], num_classes=4)]
    for seed, kw in enumerate(cases):
        for size in _sizes(lab.shape)[:2]:
            a, b = np.random.RandomState(seed), np.random.RandomState(seed)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')                # empty classes warn on both sides
                want = data.class_crop_centers(lab, size, 200, rand_state=a, **kw)
                got = idx.class_centers(size, 200, rand_state=b, **kw)
            assert got == want, (kw, size)
            assert _same_state(a, b), (kw, size)
    with pytest.raises(ValueError):
        idx.class_centers((1, 1, 1), 4, ratios=[1, -1], num_classes=2)
    with pytest.raises(ValueError):
        idx.class_centers((1, 1, 1), 4, ratios=[1, 1, 1], num_classes=2)
    with pytest.raises(ValueError):
        idx.class_centers((1, 1, 1), 4, num_classes=9)


def _volume(seed, shape=(40, 40, 28)):
    rs = np.random.RandomState(seed)
    img = rs.randn(*shape).astype(np.float32)
    lab = np.zeros(shape, np.uint8)
    lab[8:20, 12:30, 5:17] = 1
    lab[10:14, 14:20, 7:11] = 2
    return img, lab


@pytest.mark.gpu
def test_sample_patches_with_index_bit_equal():
    img, lab = _volume(2)
    di, dl = torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)
    idx = data.CropIndex(dl)
    for seed in (0, 1, 2):
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        wi, wl = data.sample_patches(di, dl, lab, (16, 16, 8), 6, a)
        gi, gl = data.sample_patches(di, dl, None, (16, 16, 8), 6, b, index=idx)
        assert torch.equal(gi, wi) and torch.equal(gl, wl)
        assert _same_state(a, b)
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    assert data.draw_monai_sample(None, (16, 16, 8), b, index=idx) == data.draw_monai_sample(lab, (16, 16, 8), a)
    assert _same_state(a, b)


@pytest.mark.gpu
def test_sample_of_a_nifti_pair_equals_the_host_centre_path(tmp_path):
    img, lab = _volume(3, (28, 40, 40))                                        # stored [Z][Y][X]
    aff = np.diag([-0.5, -0.5, 2.0, 1.0])
    nifti.save(tmp_path / 'img.nii.gz', img, aff)
    nifti.save(tmp_path / 'lab.nii.gz', lab, aff)
    scan = data.SpacedScan(str(tmp_path / 'img.nii.gz'), str(tmp_path / 'lab.nii.gz'), device=DEV)
    assert scan.shape == (40, 40, 28)
    a, b = np.random.RandomState(7), np.random.RandomState(7)
    gi, gl = data.sample(scan, (16, 16, 8), b, num_samples=7)
    assert scan._label_host is None                                            # sampled through the index: no host copy yet
    wi, wl = data.sample(scan, (16, 16, 8), a, num_samples=7, host_centers=True)
    assert torch.equal(gi, wi) and torch.equal(gl, wl)
    assert _same_state(a, b)
    assert np.array_equal(scan.label_host, scan.lab.cpu().numpy()) and scan.label_host is scan.label_host
    assert scan.crop_index is scan.crop_index and scan.crop_index.counts[:3] == tuple(int((scan.label_host == c).sum()) for c in range(3))
    # ratios: RandCropByLabelClassesd centres, device and host alike
    a, b = np.random.RandomState(8), np.random.RandomState(8)
    gi, gl = data.sample(scan, (16, 16, 8), b, num_samples=5, ratios=[0, 1, 3])
    wi, wl = data.sample(scan, (16, 16, 8), a, num_samples=5, ratios=[0, 1, 3], host_centers=True)
    assert torch.equal(gi, wi) and torch.equal(gl, wl)
    assert _same_state(a, b)


@pytest.mark.gpu
def test_two_builds_are_byte_identical():
    lab = torch.from_numpy(LABELS['random']).to(DEV)
    a, b = data.CropIndex(lab), data.CropIndex(lab.clone())
    assert a.index.numel() == 9 * (7 + 1) and torch.equal(a.index, b.index) and a.counts == b.counts
    # the layout the header documents: per bin the exclusive prefixes of the blocks' counts, then the population
    flat = np.minimum(LABELS['random'].ravel(), 8)
    pad = np.full(7 * BLOCK, 255, np.uint8)
    pad[:flat.size] = flat
    per_block = np.stack([(pad.reshape(7, BLOCK) == k).sum(1) for k in range(9)])
    want = np.concatenate([np.zeros((9, 1), np.int64), np.cumsum(per_block, 1)], 1)
    assert np.array_equal(a.index.cpu().numpy().reshape(9, 8), want)


@pytest.mark.gpu
def test_build_and_select_in_a_captured_graph():
    """nothing is allocated, set or synchronised by the entry points: both are captured with their buffers fixed and replayed on a
    changed label and changed queries"""
    from lintransunet_amd import _lib
    host = LABELS['random'].copy()
    lab = torch.from_numpy(host).to(DEV)
    n, elems = lab.numel(), _lib.load().ltu_crop_index_elems(lab.numel())
    index = torch.zeros(elems, dtype=torch.int32, device=DEV)
    totals = torch.zeros(9, dtype=torch.int64, device=DEV)
    queries = torch.zeros((64, 2), dtype=torch.int32, device=DEV)
    out = torch.zeros(64, dtype=torch.int64, device=DEV)

    def launch():
        s = torch.cuda.current_stream().cuda_stream
        _lib.call('ltu_crop_index_build', lab.data_ptr(), n, index.data_ptr(), elems, totals.data_ptr(), s)
        _lib.call('ltu_crop_index_select', lab.data_ptr(), n, index.data_ptr(), elems, queries.data_ptr(), out.data_ptr(), 64, s)

    launch()                                                                   # code objects loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()                                                               # captured, not executed
    for seed in (0, 1):
        host = np.roll(host.ravel(), 1234 * seed + 1).reshape(host.shape)
        lab.copy_(torch.from_numpy(host).to(DEV))
        fg = _members(host, data.FG_MASK)
        ranks = np.random.RandomState(seed).randint(len(fg), size=64)
        queries.copy_(torch.from_numpy(np.stack([np.full(64, data.FG_MASK), ranks], 1).astype(np.int32)).to(DEV))
        graph.replay()
        assert np.array_equal(out.cpu().numpy(), fg[ranks])
        assert totals.cpu().tolist() == np.bincount(np.minimum(host.ravel(), 8), minlength=9).tolist()


@pytest.mark.gpu
def test_voxel_indices_beyond_2_31():
    """a label of 2 147 988 729 voxels (more than 2^31, a partial last block, an odd count): populations beyond int32 and members on
    both sides of 2^31.  The expected indices follow from the few members' positions, so the host never scans the label."""
    shape = (1301, 1299, 1271)
    n = shape[0] * shape[1] * shape[2]
    assert n > 2 ** 31 + 2 * BLOCK and n % BLOCK and n % 16
    members = {0: 1, 2 ** 31 - 1: 2, 2 ** 31: 3, 2 ** 31 + BLOCK + 7: 200, n - 1: 1}
    lab = torch.zeros(n, dtype=torch.uint8, device=DEV)
    lab[list(members)] = torch.tensor(list(members.values()), dtype=torch.uint8, device=DEV)
    idx = data.CropIndex(lab.view(shape))
    assert idx.counts == (n - 5, 2, 1, 1, 0, 0, 0, 0, 1) and idx.n_foreground == 5 and idx.n_background == n - 5
    where = sorted(members)
    assert idx.select([(data.FG_MASK, r) for r in range(6)]).tolist() == where + [-1]
    assert idx.select([(1 << 1, 0), (1 << 1, 1), (1 << 1, 2), (1 << 8, 0), (1 << 3, 0)]).tolist() == [0, n - 1, -1, where[3], 2 ** 31]

    def background(r):                                                         # the r-th voxel that is no member
        for m in where:
            r += m <= r
        return r

    ranks = [0, 1, 2 ** 31 - 3, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31 + BLOCK + 4, 2 ** 31 + BLOCK + 5, n - 7, n - 6]
    want = [background(r) for r in ranks]
    assert want[0] == 1 and want[3] == 2 ** 31 + 1 and want[-1] == n - 2 and all(w not in members for w in want)
    assert idx.select([(data.BG_MASK, r) for r in ranks] + [(data.BG_MASK, n - 5)]).tolist() == want + [-1]
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    got = idx.centers((3, 3, 3), 40, rand_state=b)
    lin = [where[r] if m == data.FG_MASK else background(r) for m, r in data._posneg_queries(5, n - 5, 40, 0.7, 0.3, a)]
    assert got == [data.correct_crop_centers(list(np.unravel_index(i, shape)), (3, 3, 3), shape) for i in lin]
    assert _same_state(a, b)
