"""The numpy / scipy oracle of the topology family (csrc/thinning.hip, ltu_count_cavities of csrc/components.hip;
infer.skeletonize, infer.betti_numbers, infer.topology_metrics): the simple-point predicate twice (bit-parallel flood fill, and a
scipy.ndimage.label restatement of the definition), the sequential 8-subfield curve thinning, the Betti recipe and the shapes the
tests share.  numpy + scipy only: shared by tests/test_topology.py (CPU) and tests/test_gpu_topology.py.

Neighbourhood code of a voxel p: bit 9 (dh + 1) + 3 (dw + 1) + (dd + 1) is set when p + (dh, dw, dd) is object; bit 13 (the centre)
is ignored everywhere."""
import functools

import numpy as np
from scipy import ndimage

_OFF = [(a - 1, b - 1, c - 1) for a in range(3) for b in range(3) for c in range(3)]
CENTRE = 1 << 13
ALL27 = (1 << 27) - 1
N26 = ALL27 & ~CENTRE
N18 = sum(1 << i for i, o in enumerate(_OFF) if 1 <= sum(v != 0 for v in o) <= 2)
N6 = sum(1 << i for i, o in enumerate(_OFF) if sum(v != 0 for v in o) == 1)


def _plane(axis, value):
    return sum(1 << i for i, o in enumerate(_OFF) if o[axis] == value)


# (shift, bits that may move up by it, bits that may move down by it) per axis: a bit on the far plane has no neighbour beyond it
_AXES = [(9, ALL27 & ~_plane(0, 1), ALL27 & ~_plane(0, -1)), (3, ALL27 & ~_plane(1, 1), ALL27 & ~_plane(1, -1)),
         (1, ALL27 & ~_plane(2, 1), ALL27 & ~_plane(2, -1))]


def _dilate26(x):
    for sh, up, down in _AXES:                          # a box dilation is separable: one axis after the other
        x |= ((x & up) << sh) | ((x & down) >> sh)
    return x


def _dilate6(x):
    y = x
    for sh, up, down in _AXES:
        y |= ((x & up) << sh) | ((x & down) >> sh)
    return y


def _flood(seed, allowed, dilate):
    r = seed
    while True:
        n = dilate(r) & allowed
        if n == r:
            return r
        r = n


def is_endpoint(code):
    return bin(code & N26).count('1') == 1


def is_simple_bits(code):
    """the bit-parallel predicate, the form the kernel evaluates"""
    obj = code & N26
    if obj == 0 or _flood(obj & -obj, obj, _dilate26) != obj:
        return False                                    # (a) one 26-component of object neighbours
    bg = ~code & N18
    faces = bg & N6
    if faces == 0:
        return False
    return faces & ~_flood(faces & -faces, bg, _dilate6) == 0      # (b) one 6-component of N18 background holds every face bit


_S26 = ndimage.generate_binary_structure(3, 3)
_S6 = ndimage.generate_binary_structure(3, 1)


def _block(bits):
    return np.array([(bits >> i) & 1 for i in range(27)], bool).reshape(3, 3, 3)


def is_simple_label(code):
    """conditions (a) and (b) as the definition states them, with scipy.ndimage.label"""
    _, na = ndimage.label(_block(code & N26), _S26)
    if na != 1:
        return False
    lab, _ = ndimage.label(_block(~code & N18), _S6)
    return len(set(lab[_block(N6)].tolist()) - {0}) == 1


def sample_codes(n, seed, kinds=('random', 'sparse')):
    """n codes per kind: 'random' one 27-bit word, 'sparse' the AND of three, 'dense' the OR of three"""
    rs = np.random.RandomState(seed)
    out = []
    for kind in kinds:
        w = rs.randint(0, 1 << 27, size=(3, n), dtype=np.int64)
        out.append({'random': w[0], 'sparse': w[0] & w[1] & w[2], 'dense': w[0] | w[1] | w[2]}[kind])
    return np.concatenate(out)


def few_bit_codes():
    """every code with at most three set bits in N26 (the centre clear): 1 + 26 + 325 + 2600"""
    bits = [i for i in range(27) if i != 13]
    out = [0]
    for i, a in enumerate(bits):
        out.append(1 << a)
        for j in range(i + 1, 26):
            out.append(1 << a | 1 << bits[j])
            for k in range(j + 1, 26):
                out.append(1 << a | 1 << bits[j] | 1 << bits[k])
    return np.array(out, np.int64)


def flags_of(codes):
    """u8 per code: bit 0 simple, bit 1 endpoint (what ltu_thin_simple_codes writes)"""
    return np.array([int(is_simple_bits(int(c))) | int(is_endpoint(int(c))) << 1 for c in codes], np.uint8)


_WEIGHT = (1 << np.arange(27, dtype=np.int64)).reshape(3, 3, 3)


def thin(vol):
    """sequential restatement of the thinning: (skeleton u8 [H, W, D], iterations).  One iteration marks the object voxels with a
    background face neighbour in the image as it stands, then visits the candidates of subfield s = (h & 1) | (w & 1) << 1 |
    (d & 1) << 2 for s = 0 .. 7, one voxel at a time, and deletes a voxel at once when it is simple and not an endpoint in the image
    of that moment.  Iterations that delete at least one voxel are counted."""
    img = np.pad(np.asarray(vol) != 0, 1)
    deletable = functools.lru_cache(maxsize=None)(lambda code: is_simple_bits(code) and not is_endpoint(code))
    iterations = 0
    while True:
        cand = np.argwhere(img & ~ndimage.binary_erosion(img, _S6))       # padded coordinates, raster order
        sub = ((cand[:, 0] - 1) & 1) | ((cand[:, 1] - 1) & 1) << 1 | ((cand[:, 2] - 1) & 1) << 2
        deleted = 0
        for s in range(8):
            for h, w, d in cand[sub == s]:
                code = int((img[h - 1:h + 2, w - 1:w + 2, d - 1:d + 2] * _WEIGHT).sum())
                if deletable(code & N26):
                    img[h, w, d] = False
                    deleted += 1
        if deleted == 0:
            break
        iterations += 1
    return img[1:-1, 1:-1, 1:-1].astype(np.uint8), iterations


def euler(vol):
    """V - E + F - C of the union of the closed unit cubes of the object voxels"""
    p = np.pad(np.asarray(vol) != 0, 1)
    h, l = slice(1, None), slice(None, -1)

    def touched(*axes):                                 # lattice cells spanned by the unit steps NOT in axes: OR over the voxels
        out = p                                         # on either side along every axis in axes
        for a in axes:
            hi, lo = [slice(None)] * 3, [slice(None)] * 3
            hi[a], lo[a] = h, l
            out = out[tuple(hi)] | out[tuple(lo)]
        return int(np.count_nonzero(out))

    V = touched(0, 1, 2)
    E = touched(0, 1) + touched(0, 2) + touched(1, 2)
    F = touched(0) + touched(1) + touched(2)
    C = int(np.count_nonzero(p))
    return V - E + F - C


def betti(vol):
    """(b0, b1, b2, euler): 26-components of the object, 6-components of the background that reach no face of the volume (the
    padded background minus its outer component), b1 from the Euler characteristic of the cubical complex"""
    m = np.asarray(vol) != 0
    b0 = ndimage.label(m, _S26)[1]
    b2 = ndimage.label(~np.pad(m, 1), _S6)[1] - 1
    chi = euler(m)
    return b0, b0 + b2 - chi, b2, chi


def cldice(p, g, sp, sg):
    """(clDice, Tprec, Tsens) in float64 from bool volumes P, G and their skeletons, with the empty-set conventions"""
    return cldice_from_counts(int(np.count_nonzero(sp)), int(np.count_nonzero(sp & g)), int(np.count_nonzero(sg)),
                              int(np.count_nonzero(sg & p)), bool(p.any()), bool(g.any()))


def cldice_from_counts(n_sp, n_sp_g, n_sg, n_sg_p, p_any, g_any):
    if not p_any and not g_any:
        return 1.0, 1.0, 1.0
    if not p_any or not g_any:
        return 0.0, 0.0, 0.0
    tprec, tsens = n_sp_g / n_sp, n_sg_p / n_sg
    return (0.0 if tprec + tsens == 0 else 2.0 * tprec * tsens / (tprec + tsens)), tprec, tsens


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
def _grid(shape):
    return np.mgrid[:shape[0], :shape[1], :shape[2]]


def bar():
    h, w, d = _grid((18, 16, 14))
    return (abs(h - 9) < 7) & (abs(w - 8) < 3) & (abs(d - 7) < 2.5)


def torus():
    h, w, d = _grid((22, 22, 12))
    return (np.hypot(h - 10.5, w - 10.5) - 7) ** 2 + (d - 5.5) ** 2 < 2.6 ** 2


def shell():
    h, w, d = _grid((17, 17, 17))
    r = np.sqrt((h - 8.0) ** 2 + (w - 8.0) ** 2 + (d - 8.0) ** 2)
    return (4 <= r) & (r < 7)


def block():
    return np.ones((12, 10, 7), bool)


def slab():
    m = np.zeros((15, 13, 1), bool)
    m[2:13, 3:11] = True
    m[6:8, 5:8] = False
    return m


# name -> (builder, object voxels, skeleton voxels, iterations, (b0, b1, b2) of the shape and of its skeleton)
TABLE = {'bar': (bar, 325, 9, 2, (1, 0, 0)), 'torus': (torus, 944, 38, 3, (1, 1, 0)), 'shell': (shell, 1114, 278, 2, (1, 0, 1)),
         'block': (block, 840, 14, 4, (1, 0, 0)), 'slab': (slab, 82, 32, 2, (1, 1, 0))}


def y_tube():
    """three tubes of radius 2.2 that meet in one point"""
    shape = (30, 28, 14)
    pts = np.stack(_grid(shape), -1).astype(np.float64)
    c = np.array([15.0, 14.0, 7.0])
    m = np.zeros(shape, bool)
    for end in ([3.0, 14.0, 7.0], [25.0, 4.0, 5.0], [25.0, 24.0, 9.0]):
        ab = np.array(end) - c
        t = np.clip(((pts - c) @ ab) / (ab @ ab), 0.0, 1.0)
        m |= np.linalg.norm(pts - (c + t[..., None] * ab), axis=-1) < 2.2
    return m


def noise(shape, seed, sigma=2.0, level=0.0):
    """smoothed Gaussian noise above `level`: blobs, handles and cavities at every scale from sigma up"""
    rs = np.random.RandomState(seed)
    return ndimage.gaussian_filter(rs.randn(*shape), sigma) > level


def linked_tori():
    """two tori through each other's holes: (1, 1, 0) each, (2, 2, 0) together, and no voxel of one touches the other"""
    h, w, d = _grid((30, 22, 22))
    a = (np.hypot(h - 10.0, w - 10.5) - 7) ** 2 + (d - 10.5) ** 2 < 1.6 ** 2
    b = (np.hypot(h - 17.0, d - 10.5) - 7) ** 2 + (w - 10.5) ** 2 < 1.6 ** 2
    return a | b


def shell_with_ball():
    m = shell()
    h, w, d = _grid((17, 17, 17))
    return m | ((h - 8) ** 2 + (w - 8) ** 2 + (d - 8) ** 2 < 2.0 ** 2)


def cut_noise():
    """a noise volume whose background is cut in two by an object slab across the whole volume: both halves reach a face"""
    m = noise((24, 20, 18), 11)
    m[12] = True
    return m
