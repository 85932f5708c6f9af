"""Host side of the topology family (csrc/thinning.hip, ltu_count_cavities; infer.skeletonize, infer.betti_numbers,
infer.topology_metrics): the oracle of tests/topology_common.py against its own second statement and against the figures that pin
the thinning rule, the C-ABI surface, the refusals made before any launch, and the empty-set conventions of the metric.  The
kernels are judged in tests/test_gpu_topology.py.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lintransunet_amd import _lib, infer  # noqa: E402
import topology_common as tc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ltu_thin_simple_codes', 'ltu_thin_count', 'ltu_thin_ws_elems', 'ltu_thin_iterate', 'ltu_topology_binarize',
       'ltu_topology_overlap', 'ltu_euler_characteristic', 'ltu_count_cavities')


def test_neighbourhood_masks():
    assert bin(tc.N26).count('1') == 26 and bin(tc.N18).count('1') == 18 and bin(tc.N6).count('1') == 6
    assert tc.N6 & ~tc.N18 == 0 and tc.N18 & ~tc.N26 == 0 and not tc.N26 & tc.CENTRE
    assert tc.N6 == sum(1 << i for i in (4, 10, 12, 14, 16, 22))


def test_predicate_restatements_agree():
    codes = tc.sample_codes(4000, 7)                     # 4000 random + 4000 sparse (the AND of three)
    assert len(codes) >= 8000
    simple = 0
    for c in codes:
        c = int(c)
        got = tc.is_simple_bits(c)
        assert got == tc.is_simple_label(c), hex(c)
        assert got == tc.is_simple_bits(c | tc.CENTRE)   # the centre bit is ignored
        simple += got
    assert 0.1 * len(codes) < simple < 0.9 * len(codes)  # both answers are exercised
    assert not tc.is_simple_bits(0) and not tc.is_simple_label(0)                # an isolated voxel
    assert not tc.is_simple_bits(tc.N6) and not tc.is_simple_label(tc.N6)        # all six face neighbours object
    assert tc.is_simple_bits(1 << 4) and tc.is_endpoint(1 << 4) and not tc.is_endpoint(1 << 4 | 1 << 22)
    assert tc.flags_of([0, 1 << 4, 1 << 4 | 1 << 22, tc.N26]).tolist() == [0, 3, 0, 0]
    assert len(tc.few_bit_codes()) == 1 + 26 + 325 + 2600


@pytest.mark.parametrize('name', sorted(tc.TABLE))
def test_oracle_reproduces_the_pinned_figures(name):
    build, n_obj, n_skel, iterations, b = tc.TABLE[name]
    m = build()
    assert int(np.count_nonzero(m)) == n_obj
    assert tc.betti(m)[:3] == b
    skel, its = tc.thin(m)
    assert skel.dtype == np.uint8 and skel.shape == m.shape and set(np.unique(skel).tolist()) <= {0, 1}
    assert (int(np.count_nonzero(skel)), its) == (n_skel, iterations)
    assert not (skel.astype(bool) & ~m).any()            # skeleton inside the mask
    assert tc.betti(skel)[:3] == b                       # topology kept
    again, its2 = tc.thin(skel)
    assert its2 == 0 and np.array_equal(again, skel)     # idempotent


def test_betti_recipe_on_known_shapes():
    assert tc.betti(tc.linked_tori())[:3] == (2, 2, 0)
    assert tc.betti(tc.shell_with_ball())[:3] == (2, 0, 1)
    assert tc.betti(tc.cut_noise())[2] == 0              # both halves of the background reach a face
    assert tc.betti(np.zeros((3, 4, 5), bool)) == (0, 0, 0, 0) and tc.betti(np.ones((1, 1, 1), bool)) == (1, 0, 0, 1)
    two = np.zeros((2, 2, 2), bool)
    two[0, 0, 0] = two[1, 1, 1] = True                   # joined through one lattice vertex: one component, V = 15
    assert tc.betti(two) == (1, 0, 0, 1)


def test_cldice_conventions_on_the_formula():
    assert tc.cldice_from_counts(0, 0, 0, 0, False, False) == (1.0, 1.0, 1.0)
    assert tc.cldice_from_counts(0, 0, 5, 0, False, True) == (0.0, 0.0, 0.0)
    assert tc.cldice_from_counts(5, 0, 0, 0, True, False) == (0.0, 0.0, 0.0)
    assert tc.cldice_from_counts(5, 0, 7, 0, True, True) == (0.0, 0.0, 0.0)      # Tprec + Tsens = 0
    assert tc.cldice_from_counts(4, 2, 8, 8, True, True) == (2 * 0.5 / 1.5, 0.5, 1.0)
    p, g = tc.bar(), np.roll(tc.bar(), 1, axis=2)
    cl, tp, ts = tc.cldice(p, g, tc.thin(p)[0].astype(bool), tc.thin(g)[0].astype(bool))
    assert 0.0 < cl <= 1.0 and cl == 2 * tp * ts / (tp + ts)
    assert infer.TOPOLOGY_METRIC_NAMES == ('clDice', 'Tprec', 'Tsens', 'Betti0Error', 'Betti1Error', 'Betti2Error')


def test_cabi_surface():
    header = open(os.path.join(ROOT, 'include', 'ltu_hip.h')).read()
    protos = dict(re.findall(r'^(?:int|long long)\s+(ltu_\w+)\s*\(([^;]*)\);', header, flags=re.M | re.S))
    lib = _lib.load()
    for name in NEW:
        assert name in protos and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len([a for a in protos[name].split(',') if a.strip()]) == len(_lib.SIGNATURES[name]), name
    assert lib.ltu_thin_ws_elems.restype is _lib.L
    # 16 header elements + one per object voxel; 0 for what the calls refuse
    assert lib.ltu_thin_ws_elems(2, 5, 4, 3, 0) == 16 and lib.ltu_thin_ws_elems(2, 5, 4, 3, 120) == 136
    assert lib.ltu_thin_ws_elems(2, 5, 4, 3, 121) == 0 and lib.ltu_thin_ws_elems(2, 5, 4, 3, -1) == 0
    assert lib.ltu_thin_ws_elems(0, 5, 4, 3, 0) == 0 and lib.ltu_thin_ws_elems(65536, 5, 4, 3, 0) == 0
    assert lib.ltu_thin_ws_elems(1, 2048, 1024, 1024, 0) == 0                    # S >= 2^31
    assert lib.ltu_thin_ws_elems(4, 1024, 1024, 1024, 0) == 0                    # N S >= 2^32
    assert lib.ltu_thin_ws_elems(3, 1024, 1024, 1024, 5) == 21
    src = open(os.path.join(ROOT, 'lintransunet_amd', 'csrc', 'thinning.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    assert 'hipDeviceSynchronize' not in code and 'hipStreamSynchronize' not in code and 'hipMemcpy' not in code
    assert not re.search(r'atomic\w*\s*\([^;]*(float|double)', code)             # integer atomics only
    assert code.count('th_flags(') == 3                  # defined once; called by the codes kernel and by the subfield pass
    assert 'thinning.hip' in open(os.path.join(ROOT, 'lintransunet_amd', 'csrc', 'Makefile')).read()


def test_refusals_launch_nothing():
    """every contract error is answered before a launch: the pointers are fake, so a launch would fault"""
    fake = 0x1000
    E_SHAPE, E_ARG = 'LTU_E_SHAPE', 'LTU_E_ARG'

    def refused(what, name, *args):
        with pytest.raises(_lib.LtuError, match=what):
            _lib.call(name, *args)

    refused(E_SHAPE, 'ltu_thin_simple_codes', fake, fake, 0, 0)
    refused(E_ARG, 'ltu_thin_simple_codes', 0, fake, 10, 0)
    refused(E_ARG, 'ltu_thin_simple_codes', fake, 0, 10, 0)
    for shape in ((0, 5, 4, 3), (2, 0, 4, 3), (2, 5, 4, -1), (65536, 5, 4, 3), (1, 2048, 1024, 1024), (4, 1024, 1024, 1024)):
        refused(E_SHAPE, 'ltu_thin_count', fake, fake, *shape, 0)
        refused(E_SHAPE, 'ltu_thin_iterate', fake, fake, fake, 4, fake, 1 << 40, 10, *shape, 0)
        refused(E_SHAPE, 'ltu_euler_characteristic', fake, fake, *shape, 0)
    refused(E_SHAPE, 'ltu_count_cavities', fake, fake, fake, 1 << 40, 1, 2048, 1024, 1024, 0)
    refused(E_ARG, 'ltu_thin_count', 0, fake, 2, 5, 4, 3, 0)
    refused(E_ARG, 'ltu_thin_count', fake, 0, 2, 5, 4, 3, 0)
    refused(E_ARG, 'ltu_euler_characteristic', 0, fake, 2, 5, 4, 3, 0)
    refused(E_ARG, 'ltu_euler_characteristic', fake, 0, 2, 5, 4, 3, 0)
    refused(E_ARG, 'ltu_count_cavities', 0, fake, fake, 120, 2, 5, 4, 3, 0)
    refused(E_ARG, 'ltu_count_cavities', fake, 0, fake, 120, 2, 5, 4, 3, 0)
    refused(E_ARG, 'ltu_count_cavities', fake, fake, 0, 120, 2, 5, 4, 3, 0)
    refused(E_ARG, 'ltu_count_cavities', fake, fake, fake, 119, 2, 5, 4, 3, 0)   # short scratch
    it = [fake, fake, fake, 4, fake, 16 + 30, 30, 2, 5, 4, 3, 0]
    for i in (0, 1, 2, 4):
        refused(E_ARG, 'ltu_thin_iterate', *it[:i], 0, *it[i + 1:])              # NULL pointers
    refused(E_ARG, 'ltu_thin_iterate', *it[:5], 16 + 29, *it[6:])                # short scratch
    refused(E_ARG, 'ltu_thin_iterate', *it[:6], 121, *it[7:])                    # more objects than voxels
    refused(E_ARG, 'ltu_thin_iterate', *it[:6], -1, *it[7:])
    refused(E_SHAPE, 'ltu_thin_iterate', *it[:3], 0, *it[4:])                    # iters outside 1 .. 64
    refused(E_SHAPE, 'ltu_thin_iterate', *it[:3], 65, *it[4:])
    b = [fake, fake, fake, 2, 3, 1, 0, 1, 5, 4, 3, 0.5, 0]                       # B C k kk K H W D thr
    o = [fake, fake, fake, fake, fake, 2, 3, 1, 0, 1, 5, 4, 3, 0.5, 0]
    for name, args, first, nptr in (('ltu_topology_binarize', b, 3, 3), ('ltu_topology_overlap', o, 5, 5)):
        for i in range(nptr):
            refused(E_ARG, name, *args[:i], 0, *args[i + 1:])
        refused(E_ARG, name, *args[:-2], float('nan'), 0)
        for at, bad in ((0, 0), (1, 0), (2, 3), (2, -1), (3, 1), (3, -1), (4, 0), (5, 0), (0, 40000), (5, 1 << 30)):
            a = list(args)
            a[first + at] = bad
            refused(E_SHAPE, name, *a)


def test_python_surface_refuses_cpu_tensors_and_bad_shapes():
    with pytest.raises(_lib.LtuError, match='GPU only'):
        infer.skeletonize(torch.zeros(1, 4, 4, 4))
    with pytest.raises(_lib.LtuError, match='GPU only'):
        infer.betti_numbers(torch.zeros(1, 4, 4, 4, dtype=torch.uint8))
    with pytest.raises(_lib.LtuError, match='GPU only'):
        infer.topology_metrics(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4, dtype=torch.int64))
