"""Every bf16 3x3x3 conv kernel by name, against a float64 reference.

In bf16 a conv is not one kernel but a fallback chain (conv_halo.hip launch_conv_halo_bf16, gemm.hip ltu_conv3d_dgrad /
ltu_conv3d_wgrad, upconv.hip): each launcher declines a shape it does not handle and the next one tries, steered by shape rules
and LTU_* knobs.  Each case below names the kernel that must run for its op, shape and knobs; the test witnesses the launch
with torch.profiler (forward and backward in separate windows) and checks every output against F.conv3d in float64 on the
CPU, on the same bf16-rounded operands:

* bf16-stored outputs and data gradients element-wise: |got - ref| <= 2^-8 |ref| + 1e-5 max|ref| (the rounding of an fp32
  accumulation of exact bf16 products to bf16, plus fp32 noise);
* fp32 weight and bias gradients: max|got - ref| / max|ref| <= 1e-4;
* padded head columns exactly 0, every output finite.

Persistent kernels get cases whose workgroups walk long, ragged brick runs (width knobs); each such case states its geometry
and test_steady_state_geometry re-derives it from the launchers' formulas.  The CPU tests (no GPU) check that the table names
every conv-family kernel of the newest profiles/r*_bench_kernel_stats.csv and that every named kernel exists in the sources.
LTU_CONV_PATHS_REPORT=<file> appends one JSON line per GPU case: kernels launched, brick geometry, worst error / bound.
"""
import contextlib
import glob
import json
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'lintransunet_amd', 'csrc')
DEV = 'cuda'

BF16_REL = 2.0 ** -8         # bf16 rounding of the fp32 result (8 significant bits)
BF16_ABS = 1e-5              # fp32 accumulation noise, relative to the tensor's max
WGRAD_TOL = 1e-4             # fp32 weight / bias gradients, relative to the max


# ---------------------------------------------------------------------------------------------- the table

class Case:
    """op 'conv3d' (B, Ci, C1, Co, H, W, D, stride, cop), 'pair' (B, Ci, Ca, Cb, n1, H, W, D) or 'upconv' (B, Ci, Co, H, W, D);
    kernels: direction ('fwd' / 'dgrad' / 'wgrad') -> demangled kernel names that must run; steady: (kernel family, knob) of a
    long-run case (see run_geometry)"""

    def __init__(self, name, op, shape, kernels, knobs=None, steady=None):
        self.name, self.op, self.shape, self.kernels = name, op, shape, kernels
        self.knobs = dict(knobs or {})
        self.steady = steady

    def __repr__(self):
        return self.name


def conv(B, Ci, Co, H, W, D, stride=(1, 1, 1), C1=0, cop=None):
    return dict(B=B, Ci=Ci, C1=C1, Co=Co, H=H, W=W, D=D, stride=stride, cop=cop)


def pair(B, Ci, Ca, Cb, n1, H, W, D):
    return dict(B=B, Ci=Ci, Ca=Ca, Cb=Cb, n1=n1, H=H, W=W, D=D)


def up(B, Ci, Co, H, W, D):
    return dict(B=B, Ci=Ci, Co=Co, H=H, W=W, D=D)


C16_F, C16_T = 'conv3_c16_ring_bf16_kernel<false>', 'conv3_c16_ring_bf16_kernel<true>'
FC_F, FC_T = 'conv3_fc_ring_bf16_kernel<false>', 'conv3_fc_ring_bf16_kernel<true>'
WS16, WS32 = 'conv3_halo_ws_bf16_kernel<16>', 'conv3_halo_ws_bf16_kernel<32>'
WR16, WR32 = 'conv3_halo_wr_bf16_kernel<16>', 'conv3_halo_wr_bf16_kernel<32>'
WH_RING = 'conv3_wgrad_halo_ring_bf16_kernel'
WH_PACK, WH_32 = 'conv3_wgrad_halo_bf16_kernel<true>', 'conv3_wgrad_halo_bf16_kernel<false>'
FOLD = 'conv_halo_fold_kernel'


def ring(tn, flip, hb, nw, split):
    return f'conv3_ring_bf16_kernel<{tn}, {str(flip).lower()}, {hb}, {nw}, {str(split).lower()}>'


def halo(wm, wn, tm, tn, ts, cc=32):
    return f'conv3_halo_bf16_kernel<{wm}, {wn}, {tm}, {tn}, {ts}, {cc}>'


def igemm(wm, wn, tm, tn, bk, nb=2):
    return f'igemm_nt_bf16_kernel<{wm}, {wn}, {tm}, {tn}, {bk}, {nb}>'


def tn(wm, wn, tm, tnn):
    return f'wgrad_tn_bf16_kernel<{wm}, {wn}, {tm}, {tnn}>'


def cls_ring(nc, tnn, spc, full):
    return f'conv_class_ring_bf16_kernel<{nc}, {tnn}, {spc}, {str(full).lower()}>'


def cls_halo(nc, tnn):
    return f'conv_class_halo_bf16_kernel<{nc}, {tnn}>'


# the ragged grid most long-run cases share: 21 x 34 x 37 = 6 x 5 x 5 = 150 bricks of 4x8x8 (h, w, d: 1, 2, 5 voxels in the last
# brick), 6 x 9 x 5 = 270 bricks of 4x4x8 (h, w, d: 1, 2, 5)
G = (21, 34, 37)

CASES = [
    # ---- persistent few-channel rings (conv_c16_ring.hip, conv_fc_ring.hip), steady state ---------------------------------------
    # LTU_C16_RING_BLOCKS = 11 on 150 bricks: 14 bricks per workgroup, the last one 10 (forward and data gradient);
    # weight gradient 16 channels: packed first-generation kernel, LTU_WHALO_BLOCKS = 22 on 270 bricks: 13 per split, the last 10
    Case('c16_ring_long_runs', 'conv3d', conv(1, 16, 16, *G),
         {'fwd': [C16_F], 'dgrad': [C16_T], 'wgrad': [WH_PACK]},
         {'LTU_C16_RING_BLOCKS': 11, 'LTU_WHALO_BLOCKS': 22}, steady=[('ring488', 'LTU_C16_RING_BLOCKS'), ('whalo', 'LTU_WHALO_BLOCKS')]),
    # 16 -> 5 outputs padded to an 8-column head (cop): padding columns must stay exactly zero; data gradient 8 -> 16: 8 channels are
    # below the rings, weight-stationary kernel with weights in registers
    Case('c16_ring_head', 'conv3d', conv(1, 16, 5, *G, cop=8), {'fwd': [C16_F], 'dgrad': [WR16]}, {'LTU_C16_RING_BLOCKS': 11},
         steady=[('ring488', 'LTU_C16_RING_BLOCKS')]),
    # LTU_FC_RING_BLOCKS = 11 on 150 bricks: 14 per workgroup, the last 10 (both directions); the stride-1 weight-gradient ring
    # with LTU_WHALO_RING_BLOCKS = 22 (1 chunk x 1 tile): 13 bricks per split, the last 10
    Case('fc_ring_long_runs', 'conv3d', conv(1, 32, 32, *G),
         {'fwd': [FC_F], 'dgrad': [FC_T], 'wgrad': [WH_RING]},
         {'LTU_FC_RING_BLOCKS': 11, 'LTU_WHALO_RING_BLOCKS': 22}, steady=[('ring488', 'LTU_FC_RING_BLOCKS'), ('whalo', 'LTU_WHALO_RING_BLOCKS')]),
    # 16 + 16 concat (c0 % 32 != 0): the weight-gradient ring declines, first-generation 32-chunk kernel; LTU_WHALO_BLOCKS = 22:
    # 13 bricks per split, the last 10.  Forward 16 + 16 -> 24 on fc_ring (14 bricks per workgroup); the data gradient 24 -> 16 + 16
    # has no halo kernel (24 channels: not a multiple of 16), implicit GEMM
    Case('fc_ring_concat_whalo_32', 'conv3d', conv(1, 16, 24, *G, C1=16),
         {'fwd': [FC_F], 'dgrad': [igemm(4, 1, 1, 1, 64)], 'wgrad': [WH_32]},
         {'LTU_FC_RING_BLOCKS': 11, 'LTU_WHALO_BLOCKS': 22}, steady=[('ring488', 'LTU_FC_RING_BLOCKS'), ('whalo', 'LTU_WHALO_BLOCKS')]),
    # ---- weight-gradient ring (wgrad_halo_ring.hip), steady state -------------------------------------------------------------
    # 32 + 32 concat -> 32: 2 chunks x 1 tile, LTU_WHALO_RING_BLOCKS = 44 -> 22 splits: 13 bricks each, the last 10.  Forward 64 -> 32:
    # first-generation halo kernel (conv_ring declines N <= 32); data gradient 32 -> 32 + 32 on 150 bricks < 200 workgroups and one
    # chunk (nothing to split): first-generation halo kernel, 64-column tile
    Case('whalo_ring_concat', 'conv3d', conv(1, 32, 32, *G, C1=32),
         {'fwd': [halo(4, 1, 1, 1, 3)], 'dgrad': [halo(4, 1, 1, 2, 3)], 'wgrad': [WH_RING]},
         {'LTU_WHALO_RING_BLOCKS': 44}, steady=[('whalo', 'LTU_WHALO_RING_BLOCKS')]),
    # conv pair 64 -> 32 + (3 padded to 32): gradient tile = g0 | g1 (grad1), 2 chunks x 2 tiles, LTU_WHALO_RING_BLOCKS = 88 -> 22
    # splits: 13 bricks each, the last 10.  Forward / data gradient: 150 tiles are too few for conv_ring (< 200) and too many for its
    # channel split (> 64): first-generation halo kernel, 64-column tile
    Case('whalo_ring_pair', 'pair', pair(1, 64, 32, 3, 32, *G),
         {'fwd': [halo(4, 1, 1, 2, 3)], 'dgrad': [halo(4, 1, 1, 2, 3)], 'wgrad': [WH_RING]},
         {'LTU_WHALO_RING_BLOCKS': 88}, steady=[('whalo', 'LTU_WHALO_RING_BLOCKS')]),
    # ---- first-generation weight-stationary kernels (conv_halo.hip), steady state: 16 workgroups (XCD order: contiguous runs) on
    # 270 bricks of 4x4x8 -> 17 each, the last 15 -----------------------------------------------------------------------------------
    Case('halo_ws16_long_runs', 'conv3d', conv(1, 16, 16, *G),
         {'fwd': [WS16], 'dgrad': [WS16], 'wgrad': [WH_32]},
         {'LTU_NO_C16_RING': 1, 'LTU_HALO_WR': 0, 'LTU_HALO_WS_BLOCKS': 16, 'LTU_WHALO_NO_PACK': 1, 'LTU_WHALO_BLOCKS': 22},
         steady=[('halo_ws', 'LTU_HALO_WS_BLOCKS'), ('whalo', 'LTU_WHALO_BLOCKS')]),
    Case('halo_wr16_long_runs', 'conv3d', conv(1, 16, 16, *G),
         {'fwd': [WR16], 'dgrad': [WR16], 'wgrad': [WH_PACK]},
         {'LTU_NO_C16_RING': 1, 'LTU_HALO_WR_BLOCKS': 16}, steady=[('halo_ws', 'LTU_HALO_WR_BLOCKS')]),
    # weight gradient 32 -> 32 with the ring switched off (LTU_WHALO_RING = 0): 32-chunk first generation, 13 bricks per split
    Case('halo_ws32_long_runs', 'conv3d', conv(1, 32, 32, *G),
         {'fwd': [WS32], 'dgrad': [WS32], 'wgrad': [WH_32]},
         {'LTU_NO_FC_RING': 1, 'LTU_HALO_WS_BLOCKS': 16, 'LTU_WHALO_RING': 0, 'LTU_WHALO_BLOCKS': 22},
         steady=[('halo_ws', 'LTU_HALO_WS_BLOCKS'), ('whalo', 'LTU_WHALO_BLOCKS')]),
    Case('halo_wr32_long_runs', 'conv3d', conv(1, 32, 32, *G),
         {'fwd': [WR32], 'dgrad': [WR32]},
         {'LTU_NO_FC_RING': 1, 'LTU_HALO_WR': 1, 'LTU_HALO_WR_BLOCKS': 16}, steady=[('halo_ws', 'LTU_HALO_WR_BLOCKS')]),
    # 120 bricks of 4x8x8 (below the rings' 128-brick cut-off) at the default widths: the weight-stationary kernels take it
    Case('halo_ws_below_ring_cutoff', 'conv3d', conv(1, 16, 16, 17, 30, 41, C1=16),
         {'fwd': [WS32], 'dgrad': [WR16]}),
    # ---- conv_ring.hip: 4-wave, 8-wave (8x8x8 bricks), wide (128 columns), channel split ------------------------------------------
    Case('conv_ring_4wave', 'conv3d', conv(1, 64, 64, 17, 18, 20),
         {'fwd': [ring(2, False, 1, 4, False)], 'dgrad': [ring(2, True, 1, 4, False)], 'wgrad': [WH_RING]},
         {'LTU_CONV_RING_MIN_WG': 1}),
    Case('conv_ring_big', 'conv3d', conv(1, 64, 64, 16, 18, 20),
         {'fwd': [ring(2, False, 1, 8, False)], 'dgrad': [ring(2, True, 1, 8, False)]},
         {'LTU_CONV_RING_MIN_WG': 1, 'LTU_CONV_RING_BIG_MIN': 1}),
    # 10 x 4 x 5 = 200 bricks x 1 tile of 128: the 128-column kernel in both directions
    Case('conv_ring_wide', 'conv3d', conv(1, 96, 96, 37, 25, 33),
         {'fwd': [ring(4, False, 2, 4, False)], 'dgrad': [ring(4, True, 2, 4, False)]}),
    Case('conv_ring_split', 'conv3d', conv(1, 128, 96, 6, 9, 12, C1=128),
         {'fwd': [ring(2, False, 1, 4, True), FOLD], 'dgrad': [ring(2, True, 1, 4, True), FOLD]}),
    # ---- first-generation tiled halo kernel (LTU_NO_CONV_RING = 1) ------------------------------------------------------------
    # 128 -> 64, no split: 4 chunks per workgroup -> deep stages (9 taps); data gradient 64 -> 128: 2 chunks, shallow
    Case('halo_deep', 'conv3d', conv(1, 128, 64, 9, 10, 12),
         {'fwd': [halo(4, 1, 1, 2, 9)], 'dgrad': [halo(4, 1, 1, 2, 3)]},
         {'LTU_NO_CONV_RING': 1, 'LTU_NO_HALO_SPLIT': 1}),
    # 64 -> 64 on 18 bricks: the 2 chunks split over 2 workgroups + fold, shallow
    Case('halo_shallow_split', 'conv3d', conv(1, 64, 64, 9, 10, 12),
         {'fwd': [halo(4, 1, 1, 2, 3), FOLD], 'dgrad': [halo(4, 1, 1, 2, 3), FOLD]},
         {'LTU_NO_CONV_RING': 1, 'LTU_HALO_DEEP': 0}),
    # 256 -> 32: 8 chunks split over 8 workgroups (1 chunk each) with deep stages forced, + fold
    Case('halo_deep_split', 'conv3d', conv(1, 256, 32, 9, 10, 12),
         {'fwd': [halo(4, 1, 1, 1, 9), FOLD]},
         {'LTU_HALO_DEEP': 1}),
    # ---- strided convs: forward implicit GEMM, data gradient class kernels, weight gradient TN GEMM ------------------------------
    Case('sdgrad_ring_222', 'conv3d', conv(1, 32, 128, 17, 18, 21, stride=(2, 2, 2)),
         {'fwd': [igemm(2, 2, 1, 2, 32)], 'dgrad': ['sdgrad_ring_bf16_kernel<2>'], 'wgrad': [tn(2, 2, 2, 2)]},
         {'LTU_NT_VARIANT': 1}),
    Case('sdgrad_ring_221', 'conv3d', conv(1, 32, 64, 17, 18, 20, stride=(2, 2, 1)),
         {'fwd': [igemm(4, 1, 1, 2, 64)], 'dgrad': ['sdgrad_ring_bf16_kernel<1>'], 'wgrad': [tn(1, 4, 2, 1)]}),
    Case('class_ring_222', 'conv3d', conv(1, 16, 32, 17, 18, 21, stride=(2, 2, 2)),
         {'fwd': [igemm(4, 1, 1, 1, 32)], 'dgrad': [cls_ring(8, 1, 1, False)], 'wgrad': [tn(1, 4, 1, 1)]},
         {'LTU_NO_SDGRAD_RING': 1, 'LTU_NT_VARIANT': 1}),
    Case('class_ring_221', 'conv3d', conv(1, 40, 64, 17, 18, 19, stride=(2, 2, 1)),
         {'fwd': [igemm(4, 1, 1, 2, 32)], 'dgrad': [cls_ring(4, 2, 3, False)]},
         {'LTU_NO_SDGRAD_RING': 1, 'LTU_NT_VARIANT': 1}),
    Case('class_halo_222', 'conv3d', conv(1, 16, 64, 9, 7, 10, stride=(2, 2, 2)),
         {'dgrad': [cls_halo(8, 1)]},
         {'LTU_NO_SDGRAD_RING': 1, 'LTU_NO_CLASS_RING': 1}),
    Case('class_halo_221', 'conv3d', conv(1, 40, 32, 9, 5, 17, stride=(2, 2, 1)),
         {'dgrad': [cls_halo(4, 2)]},
         {'LTU_NO_SDGRAD_RING': 1, 'LTU_NO_CLASS_RING': 1}),
    Case('class_gemm_222', 'conv3d', conv(1, 32, 64, 9, 7, 11, stride=(2, 2, 2)),
         {'dgrad': [igemm(4, 1, 1, 1, 64)]},
         {'LTU_NO_SDGRAD_RING': 1, 'LTU_NO_CLASS_HALO': 1}),
    Case('class_gemm_221', 'conv3d', conv(1, 24, 32, 9, 7, 11, stride=(2, 2, 1)),
         {'dgrad': [igemm(4, 1, 1, 1, 64)]},
         {'LTU_NO_SDGRAD_RING': 1, 'LTU_NO_CLASS_HALO': 1}),
    # K = 27 x 128 on a tiny grid: the K-split implicit GEMM (64 x 128 tiles, BK 64) and its fold
    Case('strided_ksplit', 'conv3d', conv(2, 128, 128, 8, 8, 8, stride=(2, 2, 2)),
         {'fwd': [igemm(2, 2, 1, 2, 64), 'igemm_fold_kernel']}),
    # ---- un-embedding (nearest x2 + conv) --------------------------------------------------------------------------------------
    Case('upconv_ring', 'upconv', up(1, 128, 32, 5, 9, 11),
         {'fwd': ['upconv_ring_bf16_kernel'], 'dgrad': ['updgrad_ring_bf16_kernel<2>'], 'wgrad': ['upconv_wgrad_ring_bf16_kernel']}),
    Case('upconv_dgrad_ring_wide', 'upconv', up(1, 128, 32, 5, 9, 11),
         {'dgrad': ['updgrad_ring_bf16_kernel<4>']},
         {'LTU_UPDGRAD_WIDE_MIN': 1}),
    # Forward without the ring: the class kernels (all 8 classes x 8 slots: the full class ring), or one implicit GEMM per class.
    # The data gradient has no class kernel: without its ring it is one 64-tap implicit GEMM (K split + fold on small grids).
    # Weight gradient: the first-generation class kernel (LTU_UPW_RING = 0), or per class a TN GEMM + fold (LTU_NO_CLASS_HALO).
    Case('upconv_class_ring', 'upconv', up(1, 128, 32, 5, 9, 11),
         {'fwd': [cls_ring(8, 1, 1, True)], 'dgrad': [igemm(2, 2, 1, 2, 64), 'igemm_fold_kernel'], 'wgrad': ['upconv_wgrad_class_bf16_kernel']},
         {'LTU_NO_UPRING': 1, 'LTU_NO_UPDGRAD_RING': 1, 'LTU_UPW_RING': 0}),
    Case('upconv_class_halo', 'upconv', up(1, 64, 32, 5, 9, 11),
         {'fwd': [cls_halo(8, 1)], 'dgrad': [igemm(4, 1, 1, 2, 64)]},
         {'LTU_NO_UPRING': 1, 'LTU_NO_UPDGRAD_RING': 1, 'LTU_NO_CLASS_RING': 1}),
    Case('upconv_class_gemm', 'upconv', up(1, 64, 32, 5, 9, 11),
         {'fwd': [igemm(4, 1, 1, 1, 64)], 'dgrad': [igemm(4, 1, 1, 2, 64)], 'wgrad': [tn(1, 4, 1, 1), 'upconv_fold_kernel']},
         {'LTU_NO_UPRING': 1, 'LTU_NO_UPDGRAD_RING': 1, 'LTU_NO_CLASS_HALO': 1}),
]

# Kernels of the conv family in a profile: names matching FAMILY, and the GEMM instantiations matching GEMMS that strided convs
# reach.  wgrad_ring_bf16_kernel is a dense-GEMM kernel only (launch_tn_ring_bf16 declines every multi-tap gather, ntaps != 1):
# no 3x3x3 conv reaches it, test_gpu_token_paths.py names it.
FAMILY = re.compile(r'conv3_|conv_class|sdgrad_|updgrad_|upconv_|conv_halo_fold')
GEMMS = re.compile(r'igemm_nt_bf16|wgrad_tn_bf16')
NOT_CONV = {}


def kernel_base(name):
    """'void f<1, 2>(Args)' -> 'f<1, 2>'"""
    name = name.strip()
    if name.startswith('void '):
        name = name[5:]
    depth = 0
    for i, ch in enumerate(name):
        if ch == '<':
            depth += 1
        elif ch == '>':
            depth -= 1
        elif ch == '(' and depth == 0:
            return name[:i].strip()
    return name


def named_kernels():
    return {k for c in CASES for ks in c.kernels.values() for k in ks}


# ---------------------------------------------------------------------------------------------- brick geometry of the launchers

def _cdiv(a, b):
    return -(-a // b)


def _runs(bricks, per):
    n = _cdiv(bricks, per)
    return per, n, bricks - (n - 1) * per


def run_geometry(case, family, knob):
    """(bricks per workgroup, workgroups with work, bricks of the last one) of a persistent kernel, from its launcher's formula"""
    s = case.shape
    B, H, W, D = s['B'], s['H'], s['W'], s['D']
    v = case.knobs[knob]
    if family == 'ring488':              # conv_c16_ring / conv_fc_ring: min(bricks, width) workgroups, contiguous runs
        bricks = B * _cdiv(H, 4) * _cdiv(W, 8) * _cdiv(D, 8)
        grid = min(bricks, v)
        return _runs(bricks, _cdiv(bricks, grid))
    bricks = B * _cdiv(H, 4) * _cdiv(W, 4) * _cdiv(D, 8)
    if family == 'halo_ws':              # conv3_halo_ws / _wr: grid % 8 == 0 -> contiguous runs of ceil(bricks / grid)
        grid = min(bricks, v)
        assert grid % 8 == 0, 'runs are contiguous only for grids of a multiple of 8 (XCD order)'
        return _runs(bricks, _cdiv(bricks, grid))
    assert family == 'whalo'             # weight gradients: width / (chunks x 32-column tiles) splits of contiguous runs
    C = s['Ci'] + s.get('C1', 0)
    N = s['Ca'] + s['n1'] if case.op == 'pair' else s['Co']
    cc = 32 if C % 32 == 0 else 16
    ns = max(1, v // (_cdiv(C, cc) * _cdiv(N, 32)))
    ns = min(ns, bricks)
    return _runs(bricks, _cdiv(bricks, ns))


# ---------------------------------------------------------------------------------------------- CPU checks

def _newest_profile():
    paths = glob.glob(os.path.join(ROOT, 'profiles', 'r*_bench_kernel_stats.csv'))
    assert paths, 'no profiles/r*_bench_kernel_stats.csv'
    return max(paths, key=lambda p: int(re.match(r'r(\d+)_', os.path.basename(p)).group(1)))


def profile_conv_kernels():
    import csv
    with open(_newest_profile()) as f:
        names = {kernel_base(r['Name']) for r in csv.DictReader(f)}
    return sorted(n for n in names if FAMILY.search(n) or GEMMS.search(n))


def test_table_names_every_profiled_conv_kernel():
    named = named_kernels()
    missing = [k for k in profile_conv_kernels() if k not in named]
    assert not missing, f'conv-family kernels of {os.path.basename(_newest_profile())} without a case: {missing}'
    assert len({c.name for c in CASES}) == len(CASES)


def _names(case, *directions):
    return {k for d in (directions or case.kernels) for k in case.kernels.get(d, ())}


# width knob of each persistent kernel and the brick geometry (run_geometry) it sets
WIDTH = {C16_F: ('ring488', 'LTU_C16_RING_BLOCKS'), C16_T: ('ring488', 'LTU_C16_RING_BLOCKS'),
         FC_F: ('ring488', 'LTU_FC_RING_BLOCKS'), FC_T: ('ring488', 'LTU_FC_RING_BLOCKS'),
         WS16: ('halo_ws', 'LTU_HALO_WS_BLOCKS'), WS32: ('halo_ws', 'LTU_HALO_WS_BLOCKS'),
         WR16: ('halo_ws', 'LTU_HALO_WR_BLOCKS'), WR32: ('halo_ws', 'LTU_HALO_WR_BLOCKS'),
         WH_RING: ('whalo', 'LTU_WHALO_RING_BLOCKS'), WH_PACK: ('whalo', 'LTU_WHALO_BLOCKS'), WH_32: ('whalo', 'LTU_WHALO_BLOCKS')}


def _steady(case, kernel):
    return kernel in _names(case) and WIDTH[kernel] in (case.steady or [])


def _cls(kernel_prefix, stride, knob_set):
    return lambda c: (c.op == 'conv3d' and c.shape['stride'] == stride and set(knob_set) <= set(c.knobs)
                      and any(k.startswith(kernel_prefix) for k in _names(c, 'dgrad'))
                      and any(v % 2 for v in (c.shape['H'], c.shape['W'], c.shape['D'])))


# What the table must cover besides the profiled kernels: the fallbacks that are the default at no production shape, and a long-run
# case for every persistent kernel.  test_every_row_is_needed: each row is the only one meeting one of these (or naming a profiled kernel).
OBLIGATIONS = [
    ('whalo 32-chunk, ring off', lambda c: WH_32 in _names(c) and c.knobs.get('LTU_WHALO_RING') == 0),
    ('whalo 32-chunk, no pack at C = 16', lambda c: WH_32 in _names(c) and c.knobs.get('LTU_WHALO_NO_PACK') == 1 and c.shape['Ci'] + c.shape.get('C1', 0) == 16),
    ('whalo 32-chunk, c0 % 32 concat', lambda c: WH_32 in _names(c) and c.shape.get('C1', 0) > 0 and c.shape['Ci'] % 32 != 0),
    ('halo_ws<16>', lambda c: WS16 in _names(c)),
    ('halo_ws<32>', lambda c: WS32 in _names(c)),
    ('halo_wr<32> by LTU_HALO_WR', lambda c: WR32 in _names(c) and 'LTU_HALO_WR' in c.knobs),
    ('halo deep, no split', lambda c: any(k.startswith('conv3_halo_bf16_kernel') and ', 9, ' in k for k in _names(c)) and FOLD not in _names(c)),
    ('halo deep, split + fold', lambda c: any(k.startswith('conv3_halo_bf16_kernel') and ', 9, ' in k for k in _names(c)) and FOLD in _names(c)),
    ('halo shallow under LTU_NO_CONV_RING, split + fold', lambda c: c.knobs.get('LTU_NO_CONV_RING') == 1 and FOLD in _names(c)),
    ('conv_ring wide, forward', lambda c: ring(4, False, 2, 4, False) in _names(c)),
    ('conv_ring wide, data gradient', lambda c: ring(4, True, 2, 4, False) in _names(c)),
    ('class ring (2,2,2)', _cls('conv_class_ring', (2, 2, 2), ['LTU_NO_SDGRAD_RING'])),
    ('class ring (2,2,1)', _cls('conv_class_ring', (2, 2, 1), ['LTU_NO_SDGRAD_RING'])),
    ('class halo (2,2,2)', _cls('conv_class_halo', (2, 2, 2), ['LTU_NO_SDGRAD_RING', 'LTU_NO_CLASS_RING'])),
    ('class halo (2,2,1)', _cls('conv_class_halo', (2, 2, 1), ['LTU_NO_SDGRAD_RING', 'LTU_NO_CLASS_RING'])),
    ('per-class GEMM (2,2,2)', _cls('igemm_nt_bf16', (2, 2, 2), ['LTU_NO_SDGRAD_RING', 'LTU_NO_CLASS_HALO'])),
    ('per-class GEMM (2,2,1)', _cls('igemm_nt_bf16', (2, 2, 1), ['LTU_NO_SDGRAD_RING', 'LTU_NO_CLASS_HALO'])),
    ('strided forward, K split + fold', lambda c: c.op == 'conv3d' and c.shape['stride'] != (1, 1, 1) and 'igemm_fold_kernel' in _names(c, 'fwd')),
    ('upconv forward, class ring', lambda c: c.op == 'upconv' and any(k.startswith('conv_class_ring') for k in _names(c, 'fwd'))),
    ('upconv forward, class halo', lambda c: c.op == 'upconv' and any(k.startswith('conv_class_halo') for k in _names(c, 'fwd'))),
    ('upconv forward, per-class GEMM', lambda c: c.op == 'upconv' and 'LTU_NO_CLASS_HALO' in c.knobs and any(k.startswith('igemm_nt') for k in _names(c, 'fwd'))),
    ('upconv data gradient, GEMM + K split', lambda c: c.op == 'upconv' and 'igemm_fold_kernel' in _names(c, 'dgrad')),
    ('upconv weight gradient, first-generation class kernel', lambda c: 'upconv_wgrad_class_bf16_kernel' in _names(c, 'wgrad')),
    ('upconv weight gradient, per-class GEMM + fold', lambda c: 'upconv_fold_kernel' in _names(c, 'wgrad')),
    ('padded head on a ring', lambda c: c.op == 'conv3d' and c.shape['cop'] and any('ring' in k for k in _names(c, 'fwd'))),
    ('weight-stationary kernels below the rings\' cut-off at default widths', lambda c: not c.knobs and WS32 in _names(c, 'fwd')),
    ('long runs: whalo ring, plain conv', lambda c: _steady(c, WH_RING) and c.op == 'conv3d' and not c.shape['C1']),
    ('long runs: whalo ring, 32 + 32 concat', lambda c: _steady(c, WH_RING) and c.op == 'conv3d' and c.shape['C1'] and c.shape['Ci'] % 32 == 0),
    ('long runs: whalo ring, pair (grad1)', lambda c: _steady(c, WH_RING) and c.op == 'pair'),
] + [(f'long runs: {k}', (lambda k: lambda c: _steady(c, k))(k))
     for k in (C16_F, C16_T, FC_F, FC_T, WS16, WS32, WR16, WR32, WH_PACK, WH_32)]


def _all_obligations():
    return [(f'profiled: {k}', (lambda k: lambda c: k in _names(c))(k)) for k in profile_conv_kernels()] + OBLIGATIONS


def test_table_meets_every_obligation():
    unmet = [what for what, pred in _all_obligations() if not any(pred(c) for c in CASES)]
    assert not unmet, f'no case for: {unmet}'


def test_every_row_is_needed():
    """deleting any row of the table leaves a profiled kernel or an obligation without a case"""
    obl = _all_obligations()
    for c in CASES:
        only = [what for what, pred in obl if pred(c) and not any(pred(o) for o in CASES if o is not c)]
        assert only, f'{c.name}: every kernel / obligation it covers is covered by another case too'


def csrc_text():
    return ''.join(open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, '*.hip'))))


def is_global(fn, src):
    """a __global__ void fn( is defined in src"""
    return re.search(r'__global__\s+void\s+(?:__launch_bounds__\([^()]*(?:\([^()]*\))?[^()]*\)\s+)?' + re.escape(fn) + r'\s*\(', src)


def test_named_kernels_exist_in_sources():
    src = csrc_text()
    for k in sorted(named_kernels() | set(NOT_CONV)):
        fn = k.split('<')[0]
        assert is_global(fn, src), f'{k}: no __global__ {fn} in lintransunet_amd/csrc'


def test_steady_state_geometry():
    """every long-run case: at least 8 bricks per workgroup, a shorter last run, bricks ragged in h, w and d"""
    steady = [c for c in CASES if c.steady]
    assert steady
    for c in steady:
        s = c.shape
        for family, knob in c.steady:
            per, n, last = run_geometry(c, family, knob)
            assert per >= 8 and 0 < last < per and n >= 2, (c.name, family, per, n, last)
            bw = 8 if family == 'ring488' else 4
            assert s['H'] % 4 and s['W'] % bw and s['D'] % 8, (c.name, 'bricks must be ragged in h, w and d')


# ---------------------------------------------------------------------------------------------- GPU: witness, reference, bounds

@contextlib.contextmanager
def knobs(values):
    from lintransunet_amd import _lib
    for k, v in values.items():
        _lib.config_set(k, v)
    try:
        yield
    finally:
        for k in values:
            _lib.config_set(k, None)


def launched(fn):
    """run fn() under torch.profiler; returns (its result, demangled names of the device kernels it launched)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = {kernel_base(e.name) for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    return out, names


def _bf(t):
    return t.bfloat16().double()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _subpixel_weights(w):
    """[Co, Ci, 3, 3, 3] -> [8 classes, Co, Ci, 2, 2, 2]: per axis class p, slot s sums taps {0} | {1, 2} (p = 0) or {0, 1} | {2}
    (p = 1); fp32 sums in the order of the weight-prep kernel (misc.hip kind 5/6), then rounded to bf16"""
    w32 = w.float()
    taps = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}
    out = torch.zeros(8, w.shape[0], w.shape[1], 2, 2, 2)
    for c in range(8):
        ph, pw, pd = c >> 2, (c >> 1) & 1, c & 1
        for sl in range(8):
            sh, sw, sd = sl >> 2, (sl >> 1) & 1, sl & 1
            acc = torch.zeros(w.shape[0], w.shape[1])
            for th in taps[(ph, sh)]:
                for tw in taps[(pw, sw)]:
                    for td in taps[(pd, sd)]:
                        acc = acc + w32[:, :, th, tw, td]
            out[c, :, :, sh, sw, sd] = acc
    return out.bfloat16().double()


def _upconv_classes(x, weff, b):
    """nearest x2 + conv as 8 parity classes of 2x2x2 convs over the coarse grid with the (rounded) sub-pixel weights"""
    B, _, H, W, D = x.shape
    Co = weff.shape[1]
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    y = x.new_zeros(B, Co, 2 * H, 2 * W, 2 * D)
    for c in range(8):
        ph, pw, pd = c >> 2, (c >> 1) & 1, c & 1
        xs = xp[:, :, ph:ph + H + 1, pw:pw + W + 1, pd:pd + D + 1]
        y[:, :, ph::2, pw::2, pd::2] = F.conv3d(xs, weff[c], b)
    return y


_REF = {}


def reference(case, seed=None):
    """operands (bf16-exact, float64, channels-first) and the float64 CPU reference of one case, cached per case; seed: of the
    operands (default: from the case's name)"""
    if case.name in _REF:
        return _REF[case.name]
    s = case.shape
    g = _gen(sum(map(ord, case.name)) if seed is None else seed)
    B, H, W, D = s['B'], s['H'], s['W'], s['D']
    r = {}
    if case.op == 'conv3d':
        Ci, C1, Co = s['Ci'], s['C1'], s['Co']
        x0 = _bf(torch.randn(B, Ci, H, W, D, generator=g))
        x1 = _bf(torch.randn(B, C1, H, W, D, generator=g)) if C1 else None
        w = _bf(torch.randn(Co, Ci + C1, 3, 3, 3, generator=g) * 0.1)
        b = torch.randn(Co, generator=g).double()
        leaves = [t.clone().requires_grad_(True) for t in (x0, x1, w, b) if t is not None]
        xin = torch.cat(leaves[:2], 1) if C1 else leaves[0]
        y = F.conv3d(xin, leaves[-2], leaves[-1], stride=s['stride'], padding=1)
        go = _bf(torch.randn(y.shape, generator=g))
        y.backward(go)
        r.update(x0=x0, x1=x1, w=w, b=b, go=go, y=[y.detach()], dx=[leaves[0].grad] + ([leaves[1].grad] if C1 else []),
                 dw=[leaves[-2].grad], db=[leaves[-1].grad])
    elif case.op == 'pair':
        Ci, Ca, Cb = s['Ci'], s['Ca'], s['Cb']
        x = _bf(torch.randn(B, Ci, H, W, D, generator=g))
        wa, wb = _bf(torch.randn(Ca, Ci, 3, 3, 3, generator=g) * 0.1), _bf(torch.randn(Cb, Ci, 3, 3, 3, generator=g) * 0.1)
        ba, bb = torch.randn(Ca, generator=g).double(), torch.randn(Cb, generator=g).double()
        xr, war, bar, wbr, bbr = (t.clone().requires_grad_(True) for t in (x, wa, ba, wb, bb))
        ya, yb = F.conv3d(xr, war, bar, padding=1), F.conv3d(xr, wbr, bbr, padding=1)
        ga, gb = _bf(torch.randn(ya.shape, generator=g)), _bf(torch.randn(yb.shape, generator=g))
        torch.autograd.backward([ya, yb], [ga, gb])
        r.update(x=x, wa=wa, ba=ba, wb=wb, bb=bb, ga=ga, gb=gb, y=[ya.detach(), yb.detach()], dx=[xr.grad],
                 dw=[war.grad, wbr.grad], db=[bar.grad, bbr.grad])
    else:
        Ci, Co = s['Ci'], s['Co']
        x = _bf(torch.randn(B, Ci, H, W, D, generator=g))
        w = _bf(torch.randn(Co, Ci, 3, 3, 3, generator=g) * 0.1)
        b = torch.randn(Co, generator=g).double()
        weff = _subpixel_weights(w)
        # output and data gradient: the sub-pixel form with the bf16-rounded class weights the kernels multiply by
        xr = x.clone().requires_grad_(True)
        y = _upconv_classes(xr, weff, b)
        go = _bf(torch.randn(y.shape, generator=g))
        y.backward(go)
        # weight / bias gradient: of the plain formulation (exact sums of products, folded onto the 27 taps)
        wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        F.conv3d(F.interpolate(x, scale_factor=2), wr, br, padding=1).backward(go)
        r.update(x=x, w=w, b=b, go=go, weff=weff, y=[y.detach()], dx=[xr.grad], dw=[wr.grad], db=[br.grad])
    _REF[case.name] = r
    return r


def _cl(t):
    """channels-first cpu -> channels-last bf16 cuda"""
    return t.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.bfloat16)


def _cf(t):
    """channels-last cuda -> channels-first float64 cpu"""
    return t.detach().double().cpu().permute(0, 4, 1, 2, 3)


def check_bf16(what, got, ref):
    """element-wise bound of a bf16-stored tensor (channels-first); returns the worst |err| / bound"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f'{what}: non-finite values'
    bound = BF16_REL * ref.abs() + BF16_ABS * ref.abs().max()
    ratio = (got - ref).abs() / bound
    worst = ratio.max().item()
    if worst > 1.0:
        i = int(ratio.argmax())
        b, c, h, w, d = (int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        nbad = int((ratio > 1.0).sum())
        raise AssertionError(f'{what}: {nbad} elements out of bound; worst at (b, h, w, d, c) = ({b}, {h}, {w}, {d}, {c}) '
                             f'[4x8x8 brick ({h // 4}, {w // 8}, {d // 8}), 4x4x8 brick ({h // 4}, {w // 4}, {d // 8})]: '
                             f'got {got[b, c, h, w, d].item():.6g}, ref {ref[b, c, h, w, d].item():.6g}, {worst:.2f} x the bound')
    return worst


def check_f32(what, got, ref):
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all(), f'{what}: non-finite values'
    err = (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
    assert err <= WGRAD_TOL, f'{what}: max|err| / max|ref| = {err:.3g} > {WGRAD_TOL}'
    return err / WGRAD_TOL


def run_case(case, witness=True, backward=True, seed=None):
    """runs one case on the GPU; returns {'seen': {'fwd', 'bwd'}, 'ratio': {output: worst error / bound}, 'fails': [...]}.
    witness = False skips the profiler windows (seen stays empty); backward = False runs and checks the forward alone"""
    from lintransunet_amd import ops
    r = reference(case, seed)
    s = case.shape
    seen, ratios, fails = {}, {}, []

    window = launched if witness else (lambda fn: (fn(), set()))

    class _Ratio(dict):
        def __setitem__(self, k, thunk):
            try:
                ratios[k] = thunk()
            except AssertionError as e:
                ratios[k] = math.inf
                fails.append(str(e))
    ratio = _Ratio()
    with knobs(case.knobs):
        if case.op == 'conv3d':
            cop = s['cop']
            x0 = _cl(r['x0']).requires_grad_(True)
            x1 = _cl(r['x1']).requires_grad_(True) if r['x1'] is not None else None
            w = r['w'].float().to(DEV).requires_grad_(True)
            b = r['b'].float().to(DEV).requires_grad_(True)
            y, seen['fwd'] = window(lambda: ops.conv3d(x0, w, b, stride=s['stride'], x1=x1, cop=cop))
            go = _cl(r['go'])
            if cop:
                assert y.shape[-1] == cop
                pad = torch.zeros(y.shape, device=DEV, dtype=torch.bfloat16)
                pad[..., :s['Co']] = go
                go = pad
                assert y[..., s['Co']:].float().abs().sum().item() == 0.0, 'padded head columns must be exactly 0'    # none at cop = Co
            ratio['y'] = lambda: check_bf16('y', _cf(y)[:, :s['Co']], r['y'][0])
            if backward:
                _, seen['bwd'] = window(lambda: (y.backward(go), ops.flush_deferred()))
                ratio['dx0'] = lambda: check_bf16('dx0', _cf(x0.grad), r['dx'][0])
                if x1 is not None:
                    ratio['dx1'] = lambda: check_bf16('dx1', _cf(x1.grad), r['dx'][1])
                ratio['dw'] = lambda: check_f32('dw', w.grad, r['dw'][0])
                ratio['db'] = lambda: check_f32('db', b.grad, r['db'][0])
        elif not backward:
            raise ValueError('backward = False: conv3d cases only')
        elif case.op == 'pair':
            n1, Cb = s['n1'], s['Cb']
            x = _cl(r['x']).requires_grad_(True)
            p = [r[k].float().to(DEV).requires_grad_(True) for k in ('wa', 'ba', 'wb', 'bb')]
            prep = ops.conv_pair_prep(*(t.detach() for t in p), n1, torch.bfloat16)
            (y0, y1), seen['fwd'] = window(lambda: ops.conv3d_pair(x, *p, prep))
            assert y1.shape[-1] == n1
            assert y1[..., Cb:].float().abs().sum().item() == 0.0, 'padded head columns must be exactly 0'    # none at n1 = Cb
            g1 = torch.zeros(y1.shape, device=DEV, dtype=torch.bfloat16)
            g1[..., :Cb] = _cl(r['gb'])
            _, seen['bwd'] = window(lambda: (torch.autograd.backward([y0, y1], [_cl(r['ga']), g1]), ops.flush_deferred()))
            ratio['y0'] = lambda: check_bf16('y0', _cf(y0), r['y'][0])
            ratio['y1'] = lambda: check_bf16('y1', _cf(y1)[:, :Cb], r['y'][1])
            ratio['dx'] = lambda: check_bf16('dx', _cf(x.grad), r['dx'][0])
            for k, t, ref in (('dwa', p[0], r['dw'][0]), ('dba', p[1], r['db'][0]), ('dwb', p[2], r['dw'][1]), ('dbb', p[3], r['db'][1])):
                ratio[k] = lambda: check_f32(k, t.grad, ref)
        else:
            x = _cl(r['x']).requires_grad_(True)
            w = r['w'].float().to(DEV).requires_grad_(True)
            b = r['b'].float().to(DEV).requires_grad_(True)
            prep = ops.upconv_prep(w.detach(), torch.bfloat16)
            # the kernels' sub-pixel operands are the reference's rounded class weights, exactly
            wf = prep.wf.double().cpu()                                   # [class][Co][slot][Ci]
            ref_wf = r['weff'].permute(0, 1, 3, 4, 5, 2).reshape(wf.shape)
            assert torch.equal(wf, ref_wf), 'sub-pixel forward weights differ from the fp32-summed, bf16-rounded class weights'
            wd = prep.wd.double().cpu()                                   # [Ci][class * 8 + slot][Co]
            assert torch.equal(wd, ref_wf.permute(3, 0, 2, 1).reshape(wd.shape)), 'sub-pixel data-gradient weights differ'
            y, seen['fwd'] = window(lambda: ops.upconv3d(x, w, b, prep))
            _, seen['bwd'] = window(lambda: (y.backward(_cl(r['go'])), ops.flush_deferred()))
            ratio['y'] = lambda: check_bf16('y', _cf(y), r['y'][0])
            ratio['dx'] = lambda: check_bf16('dx', _cf(x.grad), r['dx'][0])
            ratio['dw'] = lambda: check_f32('dw', w.grad, r['dw'][0])
            ratio['db'] = lambda: check_f32('db', b.grad, r['db'][0])
    return {'seen': {k: sorted(v) for k, v in seen.items()}, 'ratio': ratios, 'fails': fails}


def missing_kernels(case, seen):
    out = []
    for direction, names in case.kernels.items():
        window = seen['fwd'] if direction == 'fwd' else seen['bwd']
        out += [f'{direction}: {k}' for k in names if k not in window]
    return out


def _report(case, res):
    path = os.environ.get('LTU_CONV_PATHS_REPORT')
    if path:
        geo = {f'{f}/{k}': run_geometry(case, f, k) for f, k in (case.steady or [])}
        with open(path, 'a') as f:
            f.write(json.dumps({'case': case.name, 'kernels': case.kernels, 'geometry': geo, **res}) + '\n')


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available()
    from lintransunet_amd import ops  # noqa: F401
    return True


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_conv_path(gpu, case):
    res = run_case(case)
    _report(case, res)
    assert not res['fails'], f'{case.name}: ' + '; '.join(res['fails'])
    miss = missing_kernels(case, res['seen'])
    assert not miss, f'{case.name}: expected kernels did not run: {miss}; launched {res["seen"]}'
