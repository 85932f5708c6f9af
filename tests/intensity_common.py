"""Case builders shared by test_intensity.py (host) and test_gpu_intensity.py (device)."""
import numpy as np

PERCENTILES = (0, 0.5, 37.3, 50, 99.5, 100)
LABEL_VALUES = np.array([0, 1, 2, 5, 7, 9, 255], dtype=np.uint8)       # as test_gpu_crop_index.py: bins 0, 1, 2, 5, 7 and twice bin 8


def ct_like(shape, seed, dtype=np.int16):
    """60 % air at -1024, the rest around 40 +- 100 HU"""
    rs = np.random.RandomState(seed)
    n = int(np.prod(shape))
    v = np.rint(rs.normal(40.0, 100.0, n))
    v[rs.rand(n) < 0.6] = -1024
    return v.reshape(shape).astype(dtype)


def uniform_i16(shape, seed):
    return np.random.RandomState(seed).randint(-32768, 32768, size=shape).astype(np.int16)


def labels(shape, seed):
    return np.random.RandomState(seed).choice(LABEL_VALUES, size=shape)


def selected(lab, mask):
    """the flat boolean selection of a label under a bin mask (all voxels when lab is None)"""
    return ((mask >> np.minimum(lab.ravel(), 8).astype(np.int64)) & 1) != 0


def bincount(values, offset):
    """int64 [65536]: bin b counts the value b + offset"""
    return np.bincount(np.asarray(values).ravel().astype(np.int64) - offset, minlength=65536).astype(np.int64)


def numpy_stats(x, percentiles):
    """the record of data.histogram_stats from numpy on the float64 values"""
    x = np.asarray(x, dtype=np.float64).ravel()
    return {'count': x.size, 'min': float(x.min()), 'max': float(x.max()), 'mean': float(x.mean()), 'std': float(x.std()),
            'percentiles': [float(np.percentile(x, q)) for q in percentiles]}
