"""The host half of the intensity fingerprint (data.histogram_stats, data.IntensityFingerprint) against numpy on the expanded
values.  No GPU: the histograms come from np.bincount."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import data  # noqa: E402
import intensity_common as ic  # noqa: E402


def _values():
    rs = np.random.RandomState(3)
    return {
        'uniform': ic.uniform_i16(5000, 1),
        'ct_like': ic.ct_like((4999,), 2),
        'single_bin': np.full(777, -1024, np.int16),
        'extremes': np.array([-32768] * 5 + [32767] * 8, np.int16),
        'one_voxel': np.array([123], np.int16),
        'even_ties': np.sort(rs.randint(-3, 4, 1000)).astype(np.int16),
    }


VALUES = _values()


@pytest.mark.parametrize('name', sorted(VALUES))
def test_histogram_stats_against_numpy(name):
    x = VALUES[name]
    got = data.histogram_stats(ic.bincount(x, -32768), ic.PERCENTILES)
    ref = ic.numpy_stats(x, ic.PERCENTILES)
    assert got['count'] == ref['count'] and isinstance(got['count'], int)
    assert got['min'] == ref['min'] and got['max'] == ref['max']
    assert got['percentiles'] == ref['percentiles']                     # bit-equal to np.percentile of the float64 values
    assert got['mean'] == float(x.astype(np.int64).mean())              # sums < 2^53: numpy's int64 mean is exact too
    assert abs(got['std'] - ref['std']) <= 1e-12 * abs(ref['std'])


def test_histogram_stats_offset_and_scale():
    x = np.random.RandomState(4).randint(0, 256, 3001).astype(np.uint8)
    assert data.histogram_stats(ic.bincount(x, 0), ic.PERCENTILES, offset=0)['percentiles'] == ic.numpy_stats(x, ic.PERCENTILES)['percentiles']
    for slope, inter in ((3.0, -1024.0), (-2.0, 17.0)):
        got = data.histogram_stats(ic.bincount(x, 0), ic.PERCENTILES, offset=0, slope=slope, inter=inter)
        ref = ic.numpy_stats(x.astype(np.float64) * slope + inter, ic.PERCENTILES)
        assert (got['min'], got['max'], got['percentiles']) == (ref['min'], ref['max'], ref['percentiles'])
        assert abs(got['mean'] - ref['mean']) <= 1e-12 * abs(ref['mean']) and abs(got['std'] - ref['std']) <= 1e-12 * ref['std']


def test_histogram_stats_empty():
    got = data.histogram_stats(np.zeros(65536, np.int64), (0.5, 99.5))
    assert got['count'] == 0 and len(got['percentiles']) == 2
    assert all(math.isnan(v) for v in (got['min'], got['max'], got['mean'], got['std'], *got['percentiles']))


def _fingerprint(hists, **kw):
    fp = data.IntensityFingerprint(device='cpu')
    for h in hists:
        fp.add_histogram(torch.from_numpy(h), **kw)
    return fp


def test_window_from_a_hand_made_histogram():
    # the values 0 .. 99 once each: mean 49.5, variance (100^2 - 1) / 12, p0.5 = 0.495, p99.5 = 98.505
    h = np.zeros(65536, np.int64)
    h[32768:32868] = 1
    lo, hi, blo, bhi = _fingerprint([h]).window()
    sd = math.sqrt(9999 / 12)
    assert (lo, hi) == (float(np.percentile(np.arange(100.0), 0.5)), float(np.percentile(np.arange(100.0), 99.5)))
    assert abs(lo - 0.495) < 1e-12 and abs(hi - 98.505) < 1e-12
    assert abs(blo - (0.495 - 49.5) / sd) < 1e-12 and abs(bhi - (98.505 - 49.5) / sd) < 1e-12


def test_window_floors_the_std():
    h = np.zeros(65536, np.int64)
    h[32768 + 40] = 12345                                # every voxel 40: std 0, floored at 1e-8 instead of dividing by it
    assert _fingerprint([h]).window() == (40.0, 40.0, 0.0, 0.0)
    h[32768 + 41] = 1                                    # a real std is used as it is
    lo, hi, blo, bhi = _fingerprint([h]).window()
    st = data.histogram_stats(h, (0.5, 99.5))
    assert st['std'] > 1e-8 and blo == (lo - st['mean']) / st['std'] and bhi == (hi - st['mean']) / st['std']


def test_save_restore_merge_equals_one_fingerprint():
    hists = [ic.bincount(ic.ct_like((3000,), s), -32768) for s in range(4)]
    whole = _fingerprint(hists)
    a, b = _fingerprint(hists[:1]), _fingerprint(hists[1:])
    saved = json.loads(json.dumps(b.to_dict()))
    assert {'max', 'mean', 'median', 'min', 'percentile_00_5', 'percentile_99_5', 'std'} <= set(saved)
    merged = a.merge(data.IntensityFingerprint.from_dict(saved))
    assert torch.equal(merged.hist, whole.hist) and merged.scans == whole.scans == 4
    assert merged.window() == whole.window() and merged.to_dict() == whole.to_dict()
    ref = ic.numpy_stats(np.concatenate([ic.ct_like((3000,), s) for s in range(4)]), (0.5, 50.0, 99.5))
    d = whole.to_dict()
    assert (d['min'], d['max'], d['percentile_00_5'], d['median'], d['percentile_99_5']) == (ref['min'], ref['max'], *ref['percentiles'])


def test_empty_scans_are_counted_and_contribute_nothing():
    fp = _fingerprint([np.zeros(65536, np.int64), ic.bincount([5, 6], -32768)])
    assert (fp.scans, fp.empty_scans) == (2, 1) and fp.stats()['count'] == 2


def test_reindexing_under_slope_and_intercept():
    x = np.random.RandomState(5).randint(0, 2000, 4000).astype(np.int16)          # stored values; scaled 2 x - 1024
    fp = _fingerprint([ic.bincount(x, -32768)], slope=2, inter=-1024)
    assert np.array_equal(fp.hist.numpy(), ic.bincount(x.astype(np.int64) * 2 - 1024, -32768))
    u = np.random.RandomState(6).randint(0, 256, 4000).astype(np.uint8)
    fp = _fingerprint([ic.bincount(u, 0)], offset=0, slope=3.0, inter=-300.0)
    assert np.array_equal(fp.hist.numpy(), ic.bincount(u.astype(np.int64) * 3 - 300, -32768))


def test_refusals():
    h = ic.bincount(np.array([-5, 0, 20000], np.int16), -32768)
    with pytest.raises(ValueError, match='case_7'):
        _fingerprint([h], slope=0.5, name='case_7')
    with pytest.raises(ValueError):
        _fingerprint([h], inter=0.25)
    with pytest.raises(ValueError, match='int16'):
        _fingerprint([h], slope=2)                       # 40000
    with pytest.raises(ValueError, match='int16'):
        _fingerprint([h], inter=-32768)                  # -32773
    fp = data.IntensityFingerprint(device='cpu')
    with pytest.raises(ValueError):
        fp.window()
    fp.add_histogram(torch.zeros(65536, dtype=torch.int64))
    with pytest.raises(ValueError):
        fp.window()
    with pytest.raises(ValueError):
        data.histogram_stats(h, (101.0,))
