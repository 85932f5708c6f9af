"""The single-channel entry points of the patch gather, ltu_sample_affine and ltu_sample_elastic: public C ABI that no Python
wrapper goes through (data.sample_affine calls ltu_sample_channels with K = 1 for a 3-D image).  Each is called directly here and
must give the bits of data.sample_affine on the same arguments: image as int32 words, label as bytes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lintransunet_amd import _lib, data                                    # noqa: E402
from lintransunet_amd.ops import _s                                        # noqa: E402
from tests.test_gpu_multichannel import _gather_mats, _gather_source       # noqa: E402

FILL = -0.75
SIZES = [(4, 6, 8), (5, 6, 7)]            # d % 4 == 0: the 4-wide store; otherwise the scalar store


def _direct(img, lab, mats, size, sigma=None, seeds=None, lattice=None):
    """ltu_sample_elastic (with a lattice) or ltu_sample_affine on one volume, in data.sample_affine's chunks of
    _lib.SAMPLE_AFFINE_MAX patches: ([n,1,h,w,d] f32, [n,1,h,w,d] u8)"""
    H, W, D = lab.shape
    h, w, d = size
    m = np.ascontiguousarray(np.asarray(mats, dtype=np.float64).reshape(-1, 12))
    n = len(m)
    sg = np.ascontiguousarray(sigma, dtype=np.float32) if sigma is not None else None
    sd = np.ascontiguousarray(seeds, dtype=np.uint64) if seeds is not None else None
    lat = torch.from_numpy(np.ascontiguousarray(lattice, dtype=np.float32)).to(img.device) if lattice is not None else None
    oi = torch.empty((n, 1, h, w, d), device=img.device, dtype=torch.float32)
    ol = torch.empty((n, 1, h, w, d), device=img.device, dtype=torch.uint8)
    for s in range(0, n, _lib.SAMPLE_AFFINE_MAX):
        e = min(n, s + _lib.SAMPLE_AFFINE_MAX)
        head = (img.data_ptr(), lab.data_ptr(), oi[s:e].data_ptr(), ol[s:e].data_ptr(), m[s:e].ctypes.data)
        tail = (sg[s:e].ctypes.data if sg is not None else 0, sd[s:e].ctypes.data if sd is not None else 0, e - s, H, W, D, h, w, d,
                FILL, _s())
        if lat is not None:
            _lib.call('ltu_sample_elastic', *head, lat[s:e].data_ptr(), *lat.shape[2:], *tail)
        else:
            _lib.call('ltu_sample_affine', *head, *tail)
    return oi, ol


def _same_bits(got, want):
    (gi, gl), (wi, wl) = got, want
    assert gi.shape == wi.shape and gl.shape == wl.shape
    return torch.equal(gi.view(torch.int32), wi.view(torch.int32)) and torch.equal(gl, wl)


@pytest.mark.parametrize('elastic', [False, True])
@pytest.mark.parametrize('size', SIZES)
def test_single_channel_entry_points_match_sample_affine(size, elastic):
    """the three matrices of _gather_mats together (the general kernel) and each alone (integer, z-decoupled and oblique variants),
    noise on one patch; with `elastic` a non-zero lattice of (4, 5, 4) control points per patch"""
    img, lab = _gather_source()
    img = img[0].contiguous()
    mats = _gather_mats(size)
    sigma = np.array([0.0, 0.5, 0.0], dtype=np.float32)
    seeds = np.array([1000, 1001, 1002], dtype=np.uint64)
    lattice = np.random.RandomState(3).uniform(-1.5, 1.5, (3, 3, 4, 5, 4)).astype(np.float32) if elastic else None
    for k in (slice(0, 3), slice(0, 1), slice(1, 2), slice(2, 3)):
        lat = lattice[k] if elastic else None
        got = data.sample_affine(img, lab, mats[k], size, FILL, sigma[k], seeds[k], elastic=lat)
        want = _direct(img, lab, mats[k], size, sigma[k], seeds[k], lat)
        assert _same_bits(got, want), (size, elastic, k)
        if k == slice(0, 3):
            assert len(torch.unique(want[1])) > 1 and bool(torch.isfinite(want[0]).all())      # the patches were written
            plain = data.sample_affine(img, lab, mats[k], size, FILL, elastic=lat)
            assert not torch.equal(plain[0][1], got[0][1]) and torch.equal(plain[0][0], got[0][0])      # the noise is on patch 1 alone


def test_single_channel_entry_point_across_the_launch_split():
    """33 patches: one more than a call takes, so data.sample_affine and the direct calls both split at _lib.SAMPLE_AFFINE_MAX"""
    img, lab = _gather_source()
    img = img[0].contiguous()
    n, size = _lib.SAMPLE_AFFINE_MAX + 1, (4, 6, 8)
    mats = np.stack([data.patch_matrix((i % 6, i % 5, i % 4), size, bool(i & 1), 0, (0.0, 0.0, 0.1 * (i % 3))) for i in range(n)])
    got = data.sample_affine(img, lab, mats, size, FILL)
    assert got[0].shape == (n, 1) + size
    assert _same_bits(got, _direct(img, lab, mats, size))
