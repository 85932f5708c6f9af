"""Every bf16 norm, gate, stencil and resampling kernel of the benchmarked step by name, against float64 references stage by stage.

The third table beside test_gpu_conv_paths.py (convolutions) and test_gpu_token_paths.py (the transformers' token path): InstanceNorm
(norm.hip: the streaming statistics / apply kernels and the one-launch kernels for small tensors), the attention gate
(pointwise.hip gate_*; pw_small.hip for its 1x1x1 projections), the positional depthwise conv (pointwise.hip dwconv_*) and the
resamplers (roi.hip: trilinear x2 and its adjoints, the ROI plans).  Each case names op, shape, knobs and module flags and, per
direction, the kernels that must run (torch.profiler witnesses them) and the name prefixes that must not.

References are float64 on the CPU from the same bf16 operands, PER STAGE where a launcher publishes an intermediate (the C-ABI is
driven directly then): InstanceNorm sums, then y from the kernel's own sums, then the backward sums, then dx from the kernel's own
backward sums; the gate likewise (a, out | dskip, ds | the fp32 sums from the kernel's ds | du1, du2 from the kernel's ds and sums).
Gates (the siblings' constants):

* bf16 outputs per element: |got - ref| <= 2^-8 |ref| + 1e-5 max|ref|, plus the terms named where they are added;
* fp32 sums and statistics: 1e-5 of the sum of the magnitudes they add;
* fp32 weight-like gradients (dpsi_w, dw, db): max|got - ref| / max|ref| <= 1e-4;
* everything finite; rows and channels past the logical extent keep their NaN fill (where the test owns the buffer).

Derivative switches (LeakyReLU in the norm backward, ReLU in the gate backward): an element whose pre-activation lies within 2^-14
of zero relative to the magnitudes summed into it may take either branch in fp32; its bound is widened by the difference between
the branches, and no tensor may have more than 0.1 % of such elements (test_switch_risk_share checks the operands on the CPU).
Statistics end to end: mean and rstd from the published sums against float64 mean / variance; with k the distance from the shift
(the first voxel) to the mean in standard deviations the sums carry 1e-5 of S sigma^2 (1 + k^2), so rstd gets a relative 1e-5 (1 + k^2) and
y gets 2^-8 |ref| + 1e-5 (1 + k^2) |h_ref| + 1e-5 max|ref|.

The trilinear taps are fp32 (src = scale * o, both rounded): a weight is within 2^-22 L of its exact value on an axis of L input
voxels; that term (TAP) is added where a trilinear output is checked.  The separable adjoint stores bf16 after every 1-D pass: through
ops the reference rounds after each pass (with the siblings' one-ulp slack, carried through the later passes), and the same call
through the C-ABI is checked pass by pass on the stored intermediates, without slack.

Unreachable: instnorm_bwd_apply_kernel (the generic backward apply) has no entry point - ltu_instnorm_bwd accepts only channel
counts whose quarter divides 256, and every one of them divides 1024, which selects the fixed-channel kernel.  The generic forward
apply is reached through ltu_instnorm_apply alone (C = 12), with sums supplied by the caller (case in_generic_apply).

The CPU tests (no GPU) hold the census of the newest profiles/r*_bench_kernel_stats.csv over the three tables, the existence of
every named kernel, the obligations, the geometry every long-run / ragged case claims, and the references against torch autograd.
LTU_STREAM_PATHS_REPORT=<file> appends one JSON line per GPU case: kernels launched, geometry, worst error / bound per output.
"""
import csv
import glob
import json
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import stream_common as R
from tests import test_gpu_conv_paths as conv_paths
from tests import test_gpu_token_paths as token_paths
from tests.test_gpu_conv_paths import _newest_profile, kernel_base, knobs, launched
from tests.test_gpu_layer import _masks
from tests.test_gpu_token_paths import BF16_ABS, BF16_REL, F32_REL, WGRAD_TOL, _call, _dev, _nan, _ptr, _stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'lintransunet_amd', 'csrc')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DEV = 'cuda'
P_DROP = 0.3
WIDEN_CAP = 1e-3             # at most 0.1 % of a tensor's elements may sit on a derivative switch
TAP = 2.0 ** -22             # fp32 trilinear tap weights: within TAP * L of exact on an axis of L input voxels


# ---------------------------------------------------------------------------------------------- the table

class Case:
    """op 'in' (B, S, C, res, act, p, ports, edge, ws, mode), 'gate' (B, S, C, ws, fwd_only), 'pw' (M, K, N, bias, acc),
    'dw' (B, H, W, D, C, p, ports, ws, split), 'tri' (B, H, W, D, C, sd, ports), 'roi' (masks, C) or 'conv_wgrad' (a conv3d shape of
    test_gpu_conv_paths.py); kernels: window -> demangled kernel names that must run; absent: window -> prefixes that must not;
    flags: attributes of lintransunet_amd.ops set for the case; claims: the geometry the case is there for (test_geometry)"""

    def __init__(self, name, op, shape, kernels, knobs=None, flags=None, absent=None, claims=None):
        self.name, self.op, self.shape, self.kernels = name, op, shape, kernels
        self.knobs, self.flags, self.absent, self.claims = dict(knobs or {}), dict(flags or {}), dict(absent or {}), dict(claims or {})

    def __repr__(self):
        return self.name


def inorm(B, S, C, res=False, act=True, p=0.0, ports=1, edge=None, ws=True, mode='both'):
    return dict(B=B, S=S, C=C, res=res, act=act, p=p, ports=ports, edge=edge, ws=ws, mode=mode)


IN_STATS, IN_APPLY = 'instnorm_stats_kernel<bf16_t, 4>', 'instnorm_apply_fixedc_kernel<bf16_t, 4, false>'
IN_BSTATS, IN_BAPPLY = 'instnorm_bwd_stats_kernel<bf16_t, 4>', 'instnorm_bwd_apply_fixedc_kernel<bf16_t, 4, false>'
IN_GENERIC, IN_GENERIC_BWD = 'instnorm_apply_kernel<bf16_t>', 'instnorm_bwd_apply_kernel<bf16_t>'
RP = 'reduce_parts_kernel<{}>'.format


def in_stream(nb=None):
    """the streaming path; nb: the fold instance to name (reduce_parts_kernel<4> is the token table's)"""
    fold = [RP(nb)] if nb else []
    return {'fwd': [IN_STATS, IN_APPLY] + fold, 'bwd': [IN_BSTATS, IN_BAPPLY] + fold}


def small_f(nit, apply=True):
    return f'instnorm_small_fwd_kernel<bf16_t, 8, {nit}, {str(apply).lower()}>'


def small_b(nit):
    return f'instnorm_small_bwd_kernel<bf16_t, 8, {nit}>'


def in_small(nit):
    return {'fwd': [small_f(nit)], 'bwd': [small_b(nit)]}


NO_SMALL = {'fwd': ['instnorm_small'], 'bwd': ['instnorm_small']}
NO_STREAM = {'fwd': ['instnorm_stats', 'instnorm_apply', 'reduce_parts'], 'bwd': ['instnorm_bwd', 'reduce_parts']}


def gate(B, S, C, ws=True, fwd_only=False):
    return dict(B=B, S=S, C=C, ws=ws, fwd_only=fwd_only)


def gate_k(C, ws=True, fwd_only=False):
    G = C // 4
    k = {'fwd': [f'gate_fwd_kernel<bf16_t, {G}>']}
    if not fwd_only:
        k['bwd'] = [f'gate_bwd_reduce_kernel<bf16_t, {G}>', f'gate_bwd_apply_kernel<bf16_t, {G}>'] + (['gate_fold_kernel'] if ws else [])
    return k


def pw(M, K, N, bias, acc):
    return dict(M=M, K=K, N=N, bias=bias, acc=acc)


def pw_k(K, N):
    return f'pw_small_bf16_kernel<{K // 16}, {2 if N > 32 else 1}>'


NO_PW = {'fwd': ['pw_small_bf16_kernel']}
PW_M = 65553                 # 2048 tiles of 32 rows + 17 rows


def dw(B, H, W, D, C, p=0.0, ports=1, ws=True, split=False):
    return dict(B=B, H=H, W=W, D=D, C=C, p=p, ports=ports, ws=ws, split=split)


DW0, DW1, DW2, DWF = ('dwconv_halo_kernel<bf16_t, 0>', 'dwconv_halo_kernel<bf16_t, 1>', 'dwconv_halo_kernel<bf16_t, 2>',
                      'dwconv_fold_kernel')
DW_GRID = (9, 10, 19)        # 3 x 3 x 3 bricks of 4x4x8 per sample, the last one of each axis 1, 2 and 3 voxels


def tri(B, H, W, D, C, sd, ports=1):
    return dict(B=B, H=H, W=W, D=D, C=C, sd=sd, ports=ports)


TRI_F, TRI_T = 'trilinear_fwd_kernel<bf16_t>', 'tri_tables_kernel'
TRI_TAB_K, TRI_WIDE_K = 'trilinear_bwd_tab_kernel<bf16_t>', 'trilinear_bwd_kernel<bf16_t>'


def t_rows(two):
    return f'tri_adj1d_pair_rows_kernel<bf16_t, {str(two).lower()}>'


def t_pair(two):
    return f'tri_adj1d_pair_kernel<bf16_t, {str(two).lower()}>'


def t_one(two):
    return f'tri_adj1d_kernel<bf16_t, {str(two).lower()}>'


TAP64 = {'SEPARABLE_TRILINEAR_ADJOINT': False}
ROI_K = {'plan': ['roi_hist_kernel', 'roi_plan_kernel'], 'fwd': ['plan_gather_kernel<bf16_t>'], 'bwd': ['plan_scatter_kernel<bf16_t>']}

CASES = [
    # ---- InstanceNorm, streaming path (S > 4096 or LTU_NO_IN_SMALL): ltu_instnorm_fwd / _bwd through the C-ABI -------------------
    # 1024 / 2 chunks wanted, 64 rows at least: 65 chunks per sample, the last one 37 rows
    Case('in_stream_ragged', 'in', inorm(2, 4133, 16, res=True, p=P_DROP, ports=2), in_stream(), absent=NO_SMALL,
         claims=dict(chunks=65, rows=64, last_rows=37)),
    # LTU_IN_CHUNKS = 9: chunks of 556 rows on 64 row groups: threads walk 9 or 8 rows (the two-row loop and its tail)
    Case('in_stream_two_row_tail', 'in', inorm(1, 5000, 16, act=False), in_stream(), {'LTU_IN_CHUNKS': 9}, absent=NO_SMALL,
         claims=dict(chunks=9, rows=556, row_groups=64, rows_per_thread=9)),
    # C = 256: four row groups of 64 threads, 16 rows per thread; three gradient ports
    Case('in_stream_c256', 'in', inorm(1, 4200, 256, res=True, ports=3), in_stream(), absent=NO_SMALL,
         claims=dict(chunks=66, row_groups=4, rows_per_thread=16, last_rows=40)),
    # C = 8: 128 row groups for 64-row chunks (half of them idle); 301 chunks per sample fold with reduce_parts_kernel<16>
    Case('in_stream_c8_parts16', 'in', inorm(2, 19237, 8), in_stream(16), absent=NO_SMALL, claims=dict(chunks=301, rows=64, row_groups=128)),
    # 131 chunks per sample: reduce_parts_kernel<8>
    Case('in_stream_parts8', 'in', inorm(2, 8325, 16, p=P_DROP), in_stream(8), absent=NO_SMALL, claims=dict(chunks=131, last_rows=5)),
    # no workspace: the statistics kernels add their partials with atomics, no fold launch
    Case('in_stream_atomics', 'in', inorm(2, 4133, 32, res=True, ws=False), in_stream(),
         absent={'fwd': ['instnorm_small', 'reduce_parts'], 'bwd': ['instnorm_small', 'reduce_parts']}, claims=dict(chunks=65)),
    # 64 samples: 64 workgroups per sample for 17 600 four-vectors: the apply kernels' grid-stride loops take two trips (the forward's
    # two-vector loop once, then nothing or its tail)
    Case('in_stream_grid_stride', 'in', inorm(64, 1100, 64, res=True), in_stream(), {'LTU_NO_IN_SMALL': 1}, absent=NO_SMALL,
         claims=dict(apply_blocks=64, apply_trips=2, chunks=16)),
    # the generic apply kernel: reachable through ltu_instnorm_apply alone, with sums from the caller (C = 12: 1024 % 12 != 0)
    Case('in_generic_apply', 'in', inorm(2, 500, 12, res=True, mode='apply'), {'fwd': [IN_GENERIC]},
         absent={'fwd': ['instnorm_apply_fixedc']}),
    # ---- InstanceNorm, one-launch path: every (threads, NIT) in_small_plan returns, ragged S -----------------------------------------
    Case('in_small_77', 'in', inorm(3, 77, 8, res=True, p=P_DROP, ports=3), in_small(1), absent=NO_STREAM, claims=dict(threads=256, nit=1)),
    Case('in_small_300', 'in', inorm(2, 300, 16, res=True), in_small(2), absent=NO_STREAM, claims=dict(threads=256, nit=2)),
    Case('in_small_1000', 'in', inorm(2, 1000, 8, act=False), in_small(4), absent=NO_STREAM, claims=dict(threads=256, nit=4)),
    Case('in_small_1500', 'in', inorm(1, 1500, 16, ports=2), in_small(2), absent=NO_STREAM, claims=dict(threads=1024, nit=2)),
    Case('in_small_4001', 'in', inorm(2, 4001, 16, res=True, p=P_DROP), in_small(4), absent=NO_STREAM, claims=dict(threads=1024, nit=4)),
    Case('in_small_stats_only', 'in', inorm(2, 300, 16, mode='stats'), {'fwd': [small_f(2, False)]}, absent=NO_STREAM,
         claims=dict(threads=256, nit=2)),
    # 512 KB per sample: small only with LTU_IN_SMALL_KB raised
    Case('in_small_kb_raised', 'in', inorm(2, 4000, 64), in_small(4), {'LTU_IN_SMALL_KB': 1024}, absent=NO_STREAM,
         claims=dict(threads=1024, nit=4)),
    # ---- InstanceNorm, numerical edges on both paths ---------------------------------------------------------------------------------
    # channel 1 constant, channel 2 all zero (the stem's padded channels): s1 = s2 = 0, y == res, dx with rstd = eps^-1/2
    Case('in_stream_const_zero', 'in', inorm(2, 4133, 8, res=True, edge='const'), in_stream(), absent=NO_SMALL),
    Case('in_small_const_zero', 'in', inorm(2, 1000, 8, res=True, edge='const'), in_small(4), absent=NO_STREAM),
    # mean / std = 100 (no activation: every xhat is a difference of magnitudes ~100, the switch band would cover ~1 % of them)
    Case('in_stream_mean100', 'in', inorm(2, 4133, 16, act=False, edge='mean100'), in_stream(), absent=NO_SMALL),
    Case('in_small_mean100', 'in', inorm(2, 1000, 16, act=False, edge='mean100'), in_small(4), absent=NO_STREAM),
    # the first voxel of every (sample, channel), which the kernels shift by, 8 standard deviations from the mean
    Case('in_stream_far_shift', 'in', inorm(2, 4133, 16, edge='far'), in_stream(), absent=NO_SMALL),
    Case('in_small_far_shift', 'in', inorm(2, 1000, 16, edge='far'), in_small(4), absent=NO_STREAM),
    # ---- attention gate: ltu_gate_fwd / _bwd on sums from ltu_instnorm_stats, every dispatched C ------------------------------------
    # row blocks of max(256 / (C / 4), ...) rows: at least 3 per sample, the last one short; gate_fold folds them
    Case('gate_c8', 'gate', gate(2, 300, 8), gate_k(8), claims=dict(rows=128, parts=3, last=44)),
    Case('gate_c16', 'gate', gate(2, 213, 16), gate_k(16), claims=dict(rows=64, parts=4, last=21)),
    Case('gate_c32_atomics', 'gate', gate(2, 213, 32, ws=False), gate_k(32, ws=False), absent={'bwd': ['gate_fold_kernel']},
         claims=dict(rows=32, parts=7, last=21)),
    Case('gate_c64', 'gate', gate(2, 213, 64), gate_k(64), claims=dict(rows=16, parts=14, last=5)),
    Case('gate_c128', 'gate', gate(2, 213, 128), gate_k(128), claims=dict(rows=8, parts=27, last=5)),
    # 54 parts: gate_fold's two-part loop and its tail
    Case('gate_c256', 'gate', gate(2, 213, 256), gate_k(256), claims=dict(rows=4, parts=54, last=1)),
    # 1 048 600 rows of 8 channels: 8 193 blocks of 128 rows wanted, 8 192 launched: the forward's grid-stride loop takes a second trip
    Case('gate_fwd_long', 'gate', gate(2, 524300, 8, fwd_only=True), gate_k(8, fwd_only=True), claims=dict(fwd_blocks=8192, fwd_trips=2)),
    # ---- the gates' 1x1x1 projections (pw_small.hip) through ltu_linear_fwd: all eight instances, N in {8 .. 64}, bias, accumulate ---
    Case('pw_k16_n8', 'pw', pw(PW_M, 16, 8, True, 0), {'fwd': [pw_k(16, 8)]}),
    Case('pw_k16_n40_acc', 'pw', pw(PW_M, 16, 40, False, 1), {'fwd': [pw_k(16, 40)]}),
    Case('pw_k32_n16_acc', 'pw', pw(PW_M, 32, 16, False, 1), {'fwd': [pw_k(32, 16)]}),
    Case('pw_k32_n64', 'pw', pw(PW_M, 32, 64, True, 0), {'fwd': [pw_k(32, 64)]}),
    Case('pw_k64_n24_acc', 'pw', pw(PW_M, 64, 24, True, 1), {'fwd': [pw_k(64, 24)]}),
    Case('pw_k64_n64', 'pw', pw(PW_M, 64, 64, False, 0), {'fwd': [pw_k(64, 64)]}),
    Case('pw_k128_n32', 'pw', pw(PW_M, 128, 32, True, 0), {'fwd': [pw_k(128, 32)]}),
    Case('pw_k128_n40_acc', 'pw', pw(PW_M, 128, 40, False, 1), {'fwd': [pw_k(128, 40)]}),
    # the refusals: below 65 536 rows, N > 64, and the knob
    Case('pw_refuses_m65535', 'pw', pw(65535, 16, 16, True, 0), {}, absent=NO_PW),
    Case('pw_refuses_n72', 'pw', pw(PW_M, 16, 72, True, 0), {}, absent=NO_PW),
    Case('pw_refuses_knob', 'pw', pw(PW_M, 16, 16, True, 0), {}, {'LTU_NO_PW_SMALL': 1}, absent=NO_PW),
    # ---- positional depthwise conv: ltu_dwconv_fwd / _bwd -----------------------------------------------------------------------------
    # 54 ragged bricks, 5 workgroups per chunk: 11 bricks each, the last one 10.  C = 8: one partial 64-channel chunk
    Case('dw_c8_long_drop', 'dw', dw(2, *DW_GRID, 8, p=P_DROP, ports=2), {'fwd': [DW0], 'bwd': [DW1, DW2, DWF]},
         {'LTU_DW_BLOCKS': 5, 'LTU_DW_BLOCKS2': 5}, claims=dict(chunks=1, bricks_per_wg=11, wgs=5, last=10)),
    # C = 72: a full chunk plus 8 channels; the weight gradient through atomics (no workspace)
    Case('dw_c72_atomics_drop', 'dw', dw(2, *DW_GRID, 72, p=P_DROP, ws=False), {'fwd': [DW0], 'bwd': [DW1, DW2]},
         {'LTU_DW_BLOCKS': 10, 'LTU_DW_BLOCKS2': 10}, absent={'bwd': [DWF]}, claims=dict(chunks=2, bricks_per_wg=11, wgs=5, last=10)),
    # C = 128: two full chunks; dx-only and dw-only calls
    Case('dw_c128_split_calls', 'dw', dw(2, *DW_GRID, 128, ports=2, split=True), {'fwd': [DW0], 'bwd': [DW1, DW2, DWF]},
         {'LTU_DW_BLOCKS': 10, 'LTU_DW_BLOCKS2': 10}, claims=dict(chunks=2, bricks_per_wg=11, wgs=5, last=10)),
    # one brick, smaller than the halo in every direction
    Case('dw_degenerate', 'dw', dw(1, 1, 2, 3, 8), {'fwd': [DW0], 'bwd': [DW1, DW2, DWF]}, claims=dict(chunks=1, bricks_per_wg=1, wgs=1)),
    # ---- trilinear x(2, 2, sd) and its adjoints, through ops.trilinear_up -------------------------------------------------------------
    # odd lengths (the last row pair has one row); C = 8: every pass is short rows (several pairs per workgroup)
    Case('tri_sd2_rows', 'tri', tri(2, 3, 5, 7, 8, 2, ports=2), {'fwd': [TRI_F], 'bwd': [TRI_T, t_rows(True), t_rows(False)]}),
    # sd = 1: the width pass takes the second gradient, long rows: one pair per workgroup
    Case('tri_sd1_pairs', 'tri', tri(1, 5, 3, 9, 64, 1, ports=2), {'fwd': [TRI_F], 'bwd': [TRI_T, t_pair(True), t_pair(False)]},
         absent={'bwd': ['tri_adj1d_pair_rows']}),
    # C = 520: 65 vectors per row, the depth pass leaves the short-row kernel
    Case('tri_c520', 'tri', tri(1, 2, 3, 3, 520, 2, ports=2), {'fwd': [TRI_F], 'bwd': [TRI_T, t_pair(True), t_pair(False)]},
         absent={'bwd': ['tri_adj1d_pair_rows']}),
    # an axis of length 1 (scale 0: both output rows read row 0)
    Case('tri_axis1', 'tri', tri(1, 1, 4, 5, 8, 2), {'fwd': [TRI_F], 'bwd': [TRI_T, t_rows(False)]}),
    # one row per workgroup
    Case('tri_no_pair', 'tri', tri(2, 3, 5, 7, 8, 2, ports=2), {'bwd': [TRI_T, t_one(True), t_one(False)]}, {'LTU_TRI_NO_PAIR': 1},
         absent={'bwd': ['tri_adj1d_pair']}),
    # the 64-tap gather on both sides of TRI_TAB = 256
    Case('tri_tap64_tab', 'tri', tri(2, 3, 5, 7, 8, 2, ports=2), {'bwd': [TRI_TAB_K]}, flags=TAP64, absent={'bwd': ['tri_adj1d', 'tri_tables']}),
    Case('tri_tap64_wide', 'tri', tri(1, 2, 3, 257, 8, 2), {'fwd': [TRI_F], 'bwd': [TRI_WIDE_K]}, flags=TAP64,
         absent={'bwd': ['tri_adj1d', 'tri_tables', 'trilinear_bwd_tab']}),
    # ---- ROI plans: ops.RoiPlan on the masks of tests/golden/roi.npz, both warps and their adjoints --------------------------------
    # 'corner' touches the top and right borders, its mirror image the bottom and left ones; 'block' is interior
    Case('roi_c8', 'roi', dict(masks=('corner', 'block'), C=8), ROI_K),
    Case('roi_c32', 'roi', dict(masks=('corner!', 'full'), C=32), ROI_K),
    # ---- the fold of a first-level conv weight gradient: 16 -> 16 channels, 150 bricks = 150 splits of 1 728 quads ------------------
    Case('conv_wgrad_reduce64', 'conv_wgrad', conv_paths.conv(1, 16, 16, 17, 18, 41), {'bwd': ['wgrad_reduce_kernel<64>']},
         claims=dict(splits=150, sg=64)),
]

# kernels of the newest profile whose element-wise bf16 tests live elsewhere
ELSEWHERE = {
    'final_fwd_kernel<Softmax, bf16_t, 2>': 'tests/test_gpu_manyclass.py::test_final_softmax',
    'final_bwd_kernel<Softmax, bf16_t, 2>': 'tests/test_gpu_manyclass.py::test_final_softmax',
    'head_fwd_kernel<Softmax, bf16_t, 2, true>': 'tests/test_gpu_manyclass.py::test_head_softmax_wide',
    'head_bwd_bf16x8_kernel<Softmax, 2>': 'tests/test_gpu_manyclass.py::test_head_softmax_wide',
    'loss_sums_kernel<2, true>': 'tests/test_gpu_manyclass.py::test_level_loss_narrow',
    'loss_bwd_kernel<2, true>': 'tests/test_gpu_manyclass.py::test_level_loss_narrow',
    'loss_finalize_kernel<2>': 'tests/test_gpu_manyclass.py::test_level_loss_narrow',
    'label_maxpool_kernel': 'tests/test_gpu_ops.py::test_label_pyramid',
    'window_embed_kernel<bf16_t>': 'tests/test_gpu_multichannel.py::test_window_embed',
}
# names of the profile that the sources have since merged or re-templated (the two table kernels of the trilinear adjoint became
# one; the vector forms of the softmax head and of the level losses became a template argument; the finalizer got its class count;
# the softmax heads became the Softmax instantiations of the head family)
RENAMED = {'tri_table_kernel': 'tri_tables_kernel', 'tri_pair_table_kernel': 'tri_tables_kernel',
           'head_softmax_fwd_vec_kernel<bf16_t, 2>': 'head_fwd_kernel<Softmax, bf16_t, 2, true>',
           'head_softmax_fwd_kernel<bf16_t, 2, true>': 'head_fwd_kernel<Softmax, bf16_t, 2, true>',
           'head_softmax_bwd_bf16x8_kernel<2>': 'head_bwd_bf16x8_kernel<Softmax, 2>',
           'final_softmax_fwd_kernel<bf16_t, 2>': 'final_fwd_kernel<Softmax, bf16_t, 2>',
           'final_softmax_bwd_kernel<bf16_t, 2>': 'final_bwd_kernel<Softmax, bf16_t, 2>',
           'loss_sums_v4_kernel<2>': 'loss_sums_kernel<2, true>', 'loss_bwd_v4_kernel<2>': 'loss_bwd_kernel<2, true>',
           'loss_finalize_kernel': 'loss_finalize_kernel<2>'}
TORCH_OWN = ('at::native::', '__amd_rocclr_')
# kernels no entry point reaches (see the module docstring)
UNREACHABLE = {IN_GENERIC_BWD: 'ltu_instnorm_bwd accepts only C with 256 % (C / 4) == 0, all of which divide 1024: the fixed-channel kernel'}


def named_kernels():
    return {k for c in CASES for ks in c.kernels.values() for k in ks}


def _names(case, *windows):
    return {k for w in (windows or case.kernels) for k in case.kernels.get(w, ())}


def _seed(case):
    return sum(map(ord, case.name))


# ---------------------------------------------------------------------------------------------- CPU: census, existence

def profile_kernels():
    with open(_newest_profile()) as f:
        names = {kernel_base(r['Name']) for r in csv.DictReader(f)}
    return sorted(RENAMED.get(n, n) for n in names if not n.startswith(TORCH_OWN))


def test_census_of_the_newest_profile():
    """every kernel of the newest profile is named by exactly one of the three tables or by ELSEWHERE"""
    claims = {'conv': conv_paths.named_kernels(), 'token': token_paths.named_kernels(), 'stream': named_kernels(), 'elsewhere': set(ELSEWHERE)}
    prof = profile_kernels()
    unclaimed = [k for k in prof if not any(k in v for v in claims.values())]
    assert not unclaimed, f'kernels of {os.path.basename(_newest_profile())} that no table names: {unclaimed}'
    twice = {k: [t for t, v in claims.items() if k in v] for k in prof}
    twice = {k: v for k, v in twice.items() if len(v) > 1}
    assert not twice, f'kernels claimed by more than one table: {twice}'
    assert len({c.name for c in CASES}) == len(CASES)
    stale = [k for k in ELSEWHERE if k not in prof]
    assert not stale, f'ELSEWHERE lists kernels the profile does not have: {stale}'
    # the exclusions of the sibling tables that this one picks up
    for k in token_paths.NOT_TOKEN:
        assert k in named_kernels(), f'{k}: excluded by the token table and not named here'


def test_elsewhere_tests_exist():
    for k, where in ELSEWHERE.items():
        path, test = where.split('::')
        full = os.path.join(ROOT, path)
        assert os.path.isfile(full), f'{k}: {path} does not exist'
        assert re.search(r'^def ' + re.escape(test) + r'\(', open(full).read(), flags=re.M), f'{k}: no {test} in {path}'


def test_named_kernels_exist_in_sources():
    src = ''.join(open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, '*.hip'))))
    for k in sorted(named_kernels() | set(ELSEWHERE) | set(RENAMED.values()) | set(UNREACHABLE)):
        fn = k.split('<')[0]
        assert re.search(r'__global__\s+void\s+(?:__launch_bounds__\([^()]*(?:\([^()]*\))?[^()]*\)\s+)?' + re.escape(fn) + r'\s*\(', src), \
            f'{k}: no __global__ {fn} in lintransunet_amd/csrc'
    for old, new in RENAMED.items():
        if old.split('<')[0] != new.split('<')[0]:
            assert not re.search(r'\b' + re.escape(old.split('<')[0]) + r'\s*\(', src), f'{old} exists again: drop it from RENAMED'


def test_unreachable_kernels_stay_unreachable():
    """the rule that keeps the generic backward apply out of reach, from the launcher's two shape tests"""
    for C in range(4, 1028, 4):
        if R.in_stats_accepts(C):
            assert R.in_fixedc(C), C
    assert not R.in_stats_accepts(12) and not R.in_fixedc(12)
    assert not any(k in named_kernels() for k in UNREACHABLE)


# ---------------------------------------------------------------------------------------------- CPU: obligations

def _is(op, pred=lambda s, c: True):
    return lambda c: c.op == op and pred(c.shape, c)


def _stream_in(s, c):
    return c.op == 'in' and IN_STATS in _names(c)


def _small_in(s, c):
    return c.op == 'in' and any(k.startswith('instnorm_small') for k in _names(c))


def _plan(c):
    s = c.shape
    return R.in_small_plan(s['S'], s['C'], c.knobs.get('LTU_IN_SMALL_KB', 256), bool(c.knobs.get('LTU_NO_IN_SMALL')))


PW_INSTANCES = [f'pw_small_bf16_kernel<{ks}, {nt}>' for ks in (1, 2, 4, 8) for nt in (1, 2)]
GATE_INSTANCES = [k.format(G) for G in (2, 4, 8, 16, 32, 64)
                  for k in ('gate_fwd_kernel<bf16_t, {}>', 'gate_bwd_reduce_kernel<bf16_t, {}>', 'gate_bwd_apply_kernel<bf16_t, {}>')]

OBLIGATIONS = [(f'instance {k}', (lambda k: lambda c: k in _names(c))(k)) for k in PW_INSTANCES + GATE_INSTANCES + [
    IN_GENERIC, small_f(2, False), t_one(True), t_one(False), t_rows(False), TRI_TAB_K, TRI_WIDE_K, DW0, DW1, DW2, DWF, RP(8), RP(16)]] + [
    # InstanceNorm
    ('in stream: many chunks, short last one, residual + dropout + two ports', _is('in', lambda s, c: _stream_in(s, c) and s['p'] and s['res'] and s['ports'] == 2)),
    ('in stream: LTU_IN_CHUNKS lowered: >= 8 rows per thread, odd', _is('in', lambda s, c: 'LTU_IN_CHUNKS' in c.knobs)),
    ('in stream: C = 256', _is('in', lambda s, c: _stream_in(s, c) and s['C'] == 256)),
    ('in stream: C = 8, more row groups than rows', _is('in', lambda s, c: _stream_in(s, c) and s['C'] == 8 and not s['edge'])),
    ('in stream: atomics (no workspace)', _is('in', lambda s, c: _stream_in(s, c) and not s['ws'])),
    ('in stream: apply grid-stride loops, several trips', _is('in', lambda s, c: 'apply_trips' in c.claims)),
    ('in stream: three gradient ports', _is('in', lambda s, c: _stream_in(s, c) and s['ports'] == 3)),
    ('in stream: no activation', _is('in', lambda s, c: _stream_in(s, c) and not s['act'] and not s['edge'])),
    ('in stream: dropout without residual', _is('in', lambda s, c: _stream_in(s, c) and s['p'] and not s['res'])),
    ('in small: LTU_IN_SMALL_KB raised', _is('in', lambda s, c: 'LTU_IN_SMALL_KB' in c.knobs)),
    ('in small: three gradient ports, dropout', _is('in', lambda s, c: _small_in(s, c) and s['ports'] == 3 and s['p'])),
] + [(f'in small: plan {pl}', (lambda pl: _is('in', lambda s, c: _small_in(s, c) and s['mode'] == 'both' and not s['edge'] and
                                               'LTU_IN_SMALL_KB' not in c.knobs and _plan(c) == pl))(pl))
     for pl in ((256, 1), (256, 2), (256, 4), (1024, 2), (1024, 4))] + [
    (f'in {path}: edge {e}', (lambda path, e: _is('in', lambda s, c: s['edge'] == e and (_stream_in if path == 'stream' else _small_in)(s, c)))(path, e))
    for path in ('stream', 'small') for e in ('const', 'mean100', 'far')] + [
    # gate
    ('gate: atomics (no workspace)', _is('gate', lambda s, c: not s['ws'])),
    ('gate: >= 3 row blocks, short last one, folded (C = 16)', _is('gate', lambda s, c: s['C'] == 16 and s['ws'])),
    ('gate: forward grid-stride loop, second trip', _is('gate', lambda s, c: 'fwd_trips' in c.claims)),
    ('gate: fold of more than 32 parts', _is('gate', lambda s, c: s['ws'] and not s['fwd_only'] and R.gate_rows(s['S'], s['B'], s['C'])[1] > 32)),
    # pw_small
    ('pw: refuses M < 65536', _is('pw', lambda s, c: s['M'] < 65536 and c.absent)),
    ('pw: refuses N > 64', _is('pw', lambda s, c: s['N'] > 64 and c.absent)),
    ('pw: LTU_NO_PW_SMALL', _is('pw', lambda s, c: 'LTU_NO_PW_SMALL' in c.knobs)),
] + [(f'pw: N = {n}', (lambda n: _is('pw', lambda s, c: s['N'] == n and not c.absent))(n)) for n in (8, 16, 24, 32, 40, 64)] + [
    ('pw: accumulate with bias', _is('pw', lambda s, c: s['acc'] and s['bias'])),
    ('pw: accumulate without bias', _is('pw', lambda s, c: s['acc'] and not s['bias'])),
    # positional conv
    ('dw: C = 8 (partial chunk), long runs, dropout, two ports', _is('dw', lambda s, c: s['C'] == 8 and s['p'] and s['ports'] == 2 and 'last' in c.claims)),
    ('dw: C = 72, weight gradient through atomics', _is('dw', lambda s, c: s['C'] == 72 and not s['ws'])),
    ('dw: C = 128, dx-only and dw-only calls', _is('dw', lambda s, c: s['C'] == 128 and s['split'])),
    ('dw: degenerate 1x2x3 grid', _is('dw', lambda s, c: (s['H'], s['W'], s['D']) == (1, 2, 3))),
    # resamplers
    ('tri: sd = 2, short rows, two ports', _is('tri', lambda s, c: s['sd'] == 2 and s['ports'] == 2 and t_rows(True) in _names(c))),
    ('tri: sd = 1, width pass takes the second gradient', _is('tri', lambda s, c: s['sd'] == 1 and s['ports'] == 2)),
    ('tri: C = 520', _is('tri', lambda s, c: s['C'] == 520)),
    ('tri: an axis of length 1', _is('tri', lambda s, c: 1 in (s['H'], s['W'], s['D']))),
    ('roi: C = 8', _is('roi', lambda s, c: s['C'] == 8)),
    ('roi: C = 32, mirrored corner box', _is('roi', lambda s, c: s['C'] == 32 and any(m.endswith('!') for m in s['masks']))),
    ('first-level conv weight gradient fold', _is('conv_wgrad')),
]


def _all_obligations():
    mine = named_kernels()
    return [(f'profiled: {k}', (lambda k: lambda c: k in _names(c))(k)) for k in profile_kernels() if k in mine] + OBLIGATIONS


def test_table_meets_every_obligation():
    unmet = [what for what, pred in _all_obligations() if not any(pred(c) for c in CASES)]
    assert not unmet, f'no case for: {unmet}'


def test_every_row_is_needed():
    """deleting any row of the table leaves a profiled kernel or an obligation without a case"""
    obl = _all_obligations()
    for c in CASES:
        only = [what for what, pred in obl if pred(c) and not any(pred(o) for o in CASES if o is not c)]
        assert only, f'{c.name}: every kernel / obligation it covers is covered by another case too'


# ---------------------------------------------------------------------------------------------- CPU: geometry

def geometry(case):
    """what the launchers' formulas give for the case: numbers (compared with case.claims) and the kernels they select"""
    s, kn = case.shape, case.knobs
    g, expect = {}, set()
    if case.op == 'in':
        B, S, C = s['B'], s['S'], s['C']
        plan = _plan(case)
        if s['mode'] == 'apply':
            assert not R.in_fixedc(C) and not R.in_stats_accepts(C)
            expect.add(IN_GENERIC)
        elif plan:
            g.update(threads=plan[0], nit=plan[1])
            assert S > (plan[1] // 2) * plan[0], 'the last trip of every thread would be empty'
            expect |= {small_f(plan[1], s['mode'] != 'stats')} | ({small_b(plan[1])} if s['mode'] == 'both' else set())
        else:
            rows, chunks = R.stats_rows(S, B, kn.get('LTU_IN_CHUNKS', 1024))
            nrg = 256 // (C // 4)
            g.update(rows=rows, chunks=chunks, last_rows=S - (chunks - 1) * rows, row_groups=nrg, rows_per_thread=R.cdiv(rows, nrg))
            blocks = R.per_sample_grid(S * C // 4, B)
            g.update(apply_blocks=blocks, apply_trips=R.cdiv(S * C // 4, blocks * 256))
            assert R.in_fixedc(C) and chunks * B * C * 2 <= (1 << 20)
            expect |= {IN_STATS, IN_APPLY, IN_BSTATS, IN_BAPPLY}
            nb = R.reduce_parts_nb(chunks)
            if s['ws'] and nb != 4:
                expect.add(RP(nb))
            else:
                assert not any(k.startswith('reduce_parts') for k in _names(case))
    elif case.op == 'gate':
        rows, parts, last = R.gate_rows(s['S'], s['B'], s['C'])
        per = 256 // (s['C'] // 4)
        blocks = R.sgrid(s['B'] * s['S'], per)
        g.update(rows=rows, parts=parts, last=last, fwd_blocks=blocks, fwd_trips=R.cdiv(s['B'] * s['S'], blocks * per))
        expect |= set(gate_k(s['C'], s['ws'], s['fwd_only'])['fwd']) | set(gate_k(s['C'], s['ws'], s['fwd_only']).get('bwd', ()))
    elif case.op == 'pw':
        plan = R.pw_small_plan(s['M'], s['N'], s['K'], bool(kn.get('LTU_NO_PW_SMALL')))
        if plan:
            g.update(tiles=plan[3], blocks=plan[2])
            expect.add(f'pw_small_bf16_kernel<{plan[0]}, {plan[1]}>')
            assert plan[3] % 4 and s['M'] % 32, 'ragged: a partly empty last tile, waves with unequal tile counts'
        else:
            assert case.absent == NO_PW and not case.kernels
    elif case.op == 'dw':
        for knob, ks in (('LTU_DW_BLOCKS', (DW0, DW1)), ('LTU_DW_BLOCKS2', (DW2,))):
            nchunk, bpb, nblk, last = R.dw_geometry(s['B'], s['H'], s['W'], s['D'], s['C'], kn.get(knob, 512))
            assert g.get('bricks_per_wg', bpb) == bpb, 'the case gives both passes the same geometry'
            g.update(chunks=nchunk, bricks_per_wg=bpb, wgs=nblk, last=last)
        expect |= {DW0, DW1, DW2} | ({DWF} if s['ws'] else set())
    elif case.op == 'tri':
        if case.flags.get('SEPARABLE_TRILINEAR_ADJOINT', True):
            expect |= {TRI_T} | {k for _, k in R.tri_passes(s['B'], s['H'], s['W'], s['D'], s['C'], s['sd'], s['ports'], not kn.get('LTU_TRI_NO_PAIR'))}
        else:
            expect.add(TRI_TAB_K if s['W'] <= R.TRI_TAB and s['D'] <= R.TRI_TAB else TRI_WIDE_K)
    elif case.op == 'conv_wgrad':
        ns = R.whalo_splits(s['B'], s['H'], s['W'], s['D'], s['Ci'] + s['C1'], s['Co'])
        g.update(splits=ns, sg=R.wgrad_reduce_sg(s['Co'], 27 * (s['Ci'] + s['C1']), ns))
        expect.add(f'wgrad_reduce_kernel<{g["sg"]}>')
    return g, expect


def test_geometry():
    """every case: its claims are what the launchers' formulas give, and the kernels it names are the ones they select"""
    for c in CASES:
        g, expect = geometry(c)
        for k, v in c.claims.items():
            assert g.get(k) == v, (c.name, k, g.get(k), v)
        named = _names(c) - {TRI_F, 'roi_hist_kernel', 'roi_plan_kernel', 'plan_gather_kernel<bf16_t>', 'plan_scatter_kernel<bf16_t>'}
        assert named <= expect, (c.name, 'names kernels the launcher would not select', named - expect)
    by = {c.name: c for c in CASES}
    g = geometry(by['in_stream_two_row_tail'])[0]
    assert g['rows_per_thread'] >= 8 and g['rows_per_thread'] % 2 == 1 and g['last_rows'] < g['rows']
    g = geometry(by['in_stream_c8_parts16'])[0]
    assert g['row_groups'] > g['rows']
    for n in ('in_stream_ragged', 'in_stream_c256', 'in_stream_parts8'):
        g = geometry(by[n])[0]
        assert g['chunks'] >= 3 and 0 < g['last_rows'] < g['rows'], n
    for c in CASES:
        if c.op == 'gate' and not c.shape['fwd_only']:
            g = geometry(c)[0]
            assert g['parts'] >= 3 and 0 < g['last'] < g['rows'], c.name
        if c.op == 'dw' and 'last' in c.claims:
            g = geometry(c)[0]
            s = c.shape
            assert g['bricks_per_wg'] >= 8 and 0 < g['last'] < g['bricks_per_wg'] and s['H'] % 4 and s['W'] % 4 and s['D'] % 8, c.name


# ---------------------------------------------------------------------------------------------- operands (CPU, deterministic)

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bf(t):
    return t.bfloat16().double()


def _f32(t):
    return t.float().double()


def in_operands(case):
    """x, residual, gradient ports of an InstanceNorm case: bf16-exact float64"""
    s = case.shape
    B, S, C = s['B'], s['S'], s['C']
    g = _gen(_seed(case))
    mean = torch.rand(B, 1, C, generator=g) * 2 - 1
    std = 0.5 + 1.5 * torch.rand(B, 1, C, generator=g)
    if s['edge'] == 'mean100':
        std = torch.ones(B, 1, C)
        mean = 100.0 * torch.where(torch.rand(B, 1, C, generator=g) < 0.5, -1.0, 1.0)
    x = mean + std * torch.randn(B, S, C, generator=g)
    if s['edge'] == 'far':
        x[:, 0, :] = (mean + 8 * std)[:, 0, :]
    if s['edge'] == 'const':
        x[:, :, 1] = 3.5
        x[:, :, 2] = 0.0
    res = _bf(torch.randn(B, S, C, generator=g)) if s['res'] else None
    gs = [_bf(torch.randn(B, S, C, generator=g)) for _ in range(s['ports'])]
    return _bf(x), res, gs


def gate_operands(case):
    s = case.shape
    B, S, C = s['B'], s['S'], s['C']
    g = _gen(_seed(case))
    mk = lambda: _bf((torch.rand(B, 1, C, generator=g) - 0.5) + (0.5 + torch.rand(B, 1, C, generator=g)) * torch.randn(B, S, C, generator=g))  # noqa: E731
    u1, u2 = mk(), mk()
    skip, dout = _bf(torch.randn(B, S, C, generator=g)), _bf(torch.randn(B, S, C, generator=g))
    pw, pb = _f32(torch.randn(C, generator=g) / math.sqrt(C)), _f32(0.1 * torch.randn(1, generator=g))
    return u1, u2, skip, dout, pw, pb


def test_switch_risk_share():
    """from the reference alone: the operands of every case leave at most 0.1 % of a tensor's elements on a derivative switch
    (for near-normal pre-activations the expected share is about 0.8 * 2^-14 times the magnitude ratio)"""
    for c in CASES:
        s = c.shape
        if c.op == 'in' and s['act'] and s['mode'] == 'both':
            x, _, _ = in_operands(c)
            shift, s1, s2, _ = R.in_sums(x)
            mean, rstd = R.in_stat2(shift, s1, s2, s['S'])
            share = R.in_risk(x, mean, rstd, (s1 == 0) & (s2 == 0)).double().mean().item()
            assert share <= WIDEN_CAP, (c.name, share)
        if c.op == 'gate' and not s['fwd_only']:
            u1, u2, *_ = gate_operands(c)
            st = [R.in_stat2(*R.in_sums(u)[:3], s['S']) for u in (u1, u2)]
            share = R.gate_risk(u1, *st[0], u2, *st[1]).double().mean().item()
            assert share <= WIDEN_CAP, (c.name, share)


# ---------------------------------------------------------------------------------------------- CPU: the references check themselves

def test_reference_instnorm():
    """the per-stage restatement, composed, against autograd of F.instance_norm + LeakyReLU + dropout mask + residual"""
    g = _gen(1)
    B, S, C = 2, 37, 8
    x = (0.7 + 2 * torch.randn(B, S, C, generator=g)).double()
    res, gy = torch.randn(B, S, C, generator=g).double(), torch.randn(B, S, C, generator=g).double()
    mask = (torch.rand(B, S, C, generator=g) > 0.3).double() / 0.7
    for act in (True, False):
        xr = x.clone().requires_grad_(True)
        h = F.instance_norm(xr.transpose(1, 2), eps=R.IN_EPS).transpose(1, 2)
        y = (F.leaky_relu(h, R.LRELU_SLOPE) if act else h) * mask + res
        y.backward(gy)
        shift, s1, s2, _ = R.in_sums(x)
        mean, rstd = R.in_stat2(shift, s1, s2, S)
        hh = R.in_hat(x, mean, rstd)
        assert torch.allclose(R.in_apply(hh, act, mask, res), y.detach(), rtol=1e-10, atol=1e-10)
        gg = R.in_bwd_g(gy, hh, act, mask)
        bs, _ = R.in_bwd_sums(gg, hh)
        assert torch.allclose(R.in_bwd_apply(gg, hh, rstd, bs, S), xr.grad, rtol=1e-10, atol=1e-10)


def test_reference_gate():
    """against the oracle's attention gate on pre-projected inputs (identity 1x1x1 convs), float64 autograd"""
    from oracle import net as O_net
    g = _gen(2)
    B, S, C = 2, 45, 8
    u1, u2, skip, gy = (torch.randn(B, S, C, generator=g).double() for _ in range(4))
    pw, pb = torch.randn(C, generator=g).double(), torch.randn(1, generator=g).double()
    cf = lambda t: t.transpose(1, 2).reshape(B, C, S, 1, 1)       # noqa: E731
    leaves = [t.clone().requires_grad_(True) for t in (u1, u2, skip, pw, pb)]
    eye = torch.eye(C, dtype=torch.float64).reshape(C, C, 1, 1, 1)
    P = {'G.W_x.0.weight': eye, 'G.W_x.0.bias': torch.zeros(C, dtype=torch.float64), 'G.W_g.0.weight': eye,
         'G.W_g.0.bias': torch.zeros(C, dtype=torch.float64), 'G.psi.0.weight': leaves[3].reshape(1, C, 1, 1, 1), 'G.psi.0.bias': leaves[4]}
    a = O_net.attention_gate(P, 'G', cf(leaves[0]), cf(leaves[1]))
    out = cf(leaves[2]) * a
    out.backward(cf(gy))
    st = [R.in_stat2(*R.in_sums(u)[:3], S) for u in (u1, u2)]
    h1, h2 = R.in_hat(u1, *st[0]), R.in_hat(u2, *st[1])
    _, _, av = R.gate_fwd(h1, h2, pw, pb, skip)
    ok = lambda x, y: torch.allclose(x, y, rtol=1e-10, atol=1e-10)       # noqa: E731
    assert ok(skip * av[..., None], out.detach().reshape(B, C, S).transpose(1, 2))
    dskip, ds = R.gate_bwd_reduce(gy, skip, av)
    dpw, dpb, bs1, bs2 = R.gate_sums(ds, h1, h2, pw)
    dr = R.gate_dr(ds, h1, h2, pw)
    assert ok(dskip, leaves[2].grad) and ok(dpw, leaves[3].grad) and ok(dpb.reshape(1), leaves[4].grad)
    assert ok(R.gate_bwd_apply(dr, h1, st[0][1], bs1, S), leaves[0].grad) and ok(R.gate_bwd_apply(dr, h2, st[1][1], bs2, S), leaves[1].grad)


def test_reference_dwconv():
    """against depthwise F.conv3d on the reference's [B, C, D, H, W] view plus the identity term, float64 autograd"""
    g = _gen(3)
    B, H, W, D, C = 2, 3, 4, 5, 4
    x, gy = torch.randn(B, H, W, D, C, generator=g).double(), torch.randn(B, H, W, D, C, generator=g).double()
    w, b = torch.randn(C, 1, 3, 3, 3, generator=g).double(), torch.randn(C, generator=g).double()
    mask = (torch.rand(B, C, generator=g) > 0.3).double() / 0.7
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    grid = xr.permute(0, 4, 3, 1, 2)
    y = ((grid + F.conv3d(grid, wr, br, padding=1, groups=C)) * mask[:, :, None, None, None]).permute(0, 3, 4, 2, 1)
    y.backward(gy)
    ok = lambda p, q: torch.allclose(p, q, rtol=1e-10, atol=1e-10)       # noqa: E731
    assert ok(R.dw_fwd(x, w, b, mask), y.detach())
    dx, dwt, db = R.dw_bwd(gy, x, w, mask)
    assert ok(dx, xr.grad) and ok(dwt, wr.grad) and ok(db, br.grad)


def test_reference_trilinear():
    """against F.interpolate(trilinear, align_corners=True) and its autograd transpose, pass by pass"""
    g = _gen(4)
    for (B, H, W, D, C), sd in (((2, 3, 5, 7, 2), 2), ((1, 1, 4, 5, 2), 2), ((1, 5, 3, 9, 2), 1)):
        x = torch.randn(B, H, W, D, C, generator=g).double()
        xr = x.clone().requires_grad_(True)
        y = F.interpolate(xr.permute(0, 4, 1, 2, 3), scale_factor=(2, 2, sd), mode='trilinear', align_corners=True).permute(0, 2, 3, 4, 1)
        gy = torch.randn(y.shape, generator=g).double()
        y.backward(gy)
        Ah, Aw, Ad = R.tri_matrix(H, 2 * H), R.tri_matrix(W, 2 * W), R.tri_matrix(D, sd * D)
        assert torch.allclose(R.tri_fwd(x, Ah, Aw, Ad), y.detach(), rtol=1e-10, atol=1e-10)
        t = R.tri_adj_axis(R.tri_adj_axis(R.tri_adj_axis(gy, Ad, 3), Aw, 2), Ah, 1)
        assert torch.allclose(t, xr.grad, rtol=1e-10, atol=1e-10)
        assert ((R.tri_support(Ah) > 0) | (Ah == 0)).all()


def test_reference_roi_plans():
    """plan_matrices / plan_apply against dense matrix products on a hand-made plan, and the adjoint lists as its transpose"""
    B, H, W, eh, ew = 2, 5, 4, 6, 3
    offs = R.plan_offsets(B, H, W, eh, ew)
    ib, fb = torch.zeros(offs['n_int'], dtype=torch.int32), torch.zeros(offs['n_float'])
    g = _gen(5)
    dense = {}
    for name in ('fh', 'fw', 'bh', 'bw'):
        p = offs[name]
        A = torch.zeros(B, p['ND'], p['NS'], dtype=torch.float64)
        for b in range(B):
            fill = [0] * p['NS']
            for i in range(p['ND']):
                s0 = int(torch.randint(-1, p['NS'], (1,), generator=g))
                w0, w1 = (float(v) for v in torch.rand(2, generator=g).float())
                if s0 < 0:
                    w0 = 0.0
                if s0 + 1 > p['NS'] - 1:
                    w1 = 0.0
                ib[p['src0'] + b * p['ND'] + i] = s0
                fb[p['wt'] + (b * p['ND'] + i) * 2], fb[p['wt'] + (b * p['ND'] + i) * 2 + 1] = w0, w1
                for sx, wv in ((s0, w0), (s0 + 1, w1)):
                    if wv != 0.0:
                        A[b, i, sx] += np.float32(wv)
                        k = fill[sx]
                        ib[p['lidx'] + (b * p['NS'] + sx) * p['L'] + k] = i
                        fb[p['lw'] + (b * p['NS'] + sx) * p['L'] + k] = wv
                        fill[sx] += 1
            for sx in range(p['NS']):
                ib[p['cnt'] + b * p['NS'] + sx] = fill[sx]
        dense[name] = A
        got, T = R.plan_matrices(ib, fb, p, B)
        assert torch.equal(got, A) and torch.equal(T, A.transpose(1, 2)), name
    x = torch.randn(B, H, W, 3, 2, generator=g).double()
    ref = torch.stack([torch.tensordot(dense['fh'][b], torch.tensordot(dense['fw'][b], x[b], dims=([1], [1])), dims=([1], [1])) for b in range(B)])
    assert torch.allclose(R.plan_apply(x, dense['fh'], dense['fw']), ref, rtol=1e-10, atol=1e-10)


# ---------------------------------------------------------------------------------------------- GPU: checker

class Ck:
    """collects worst error / bound per output and the share of widened elements; failures are gathered per case"""

    def __init__(self):
        self.ratio, self.fails, self.widened = {}, [], {}

    def _put(self, what, worst, msg=None):
        self.ratio[what] = max(self.ratio.get(what, 0.0), worst)
        if msg:
            self.fails.append(msg)

    def _cmp(self, what, got, ref, bound, note):
        got = got.detach().double().cpu().reshape(ref.shape)
        if not torch.isfinite(got).all():
            return self._put(what, math.inf, f'{what}: non-finite values')
        err = (got - ref).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.expand_as(err).clamp_min(1e-300))
        worst = ratio.max().item()
        msg = None
        if worst > 1.0:
            i = int(ratio.argmax())
            idx = tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape)))
            msg = (f'{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements out of bound ({note}); worst at {idx}: got '
                   f'{got.reshape(-1)[i].item():.8g}, ref {ref.reshape(-1)[i].item():.8g}, {worst:.3g} x the bound')
        self._put(what, worst, msg)

    def bf16(self, what, got, ref, extra=None):
        """bf16-stored output, element-wise; extra: the named terms (float64, broadcastable to ref)"""
        bound = BF16_REL * ref.abs() + BF16_ABS * ref.abs().max()
        self._cmp(what, got, ref, bound + extra if extra is not None else bound, '2^-8 |ref| + 1e-5 max|ref|' + (' + named terms' if extra is not None else ''))

    def f32(self, what, got, ref, mag, extra=None):
        """fp32 sums / statistics: 1e-5 of the magnitude of the sum (+ the named terms)"""
        bound = F32_REL * mag
        self._cmp(what, got, ref, bound + extra if extra is not None else bound, '1e-5 of the summed magnitudes' + (' + named terms' if extra is not None else ''))

    def grad(self, what, got, ref):
        """fp32 weight-like gradients: max|got - ref| / max|ref| <= 1e-4"""
        got = got.detach().double().cpu().reshape(ref.shape)
        if not torch.isfinite(got).all():
            return self._put(what, math.inf, f'{what}: non-finite values')
        err = (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
        self._put(what, err / WGRAD_TOL, f'{what}: max|err| / max|ref| = {err:.3g} > {WGRAD_TOL}' if err > WGRAD_TOL else None)

    def exact(self, what, got, ref):
        ok = torch.equal(got.detach().double().cpu().reshape(ref.shape), ref)
        self._put(what, 0.0 if ok else math.inf, None if ok else f'{what}: not bit-equal to the reference')

    def untouched(self, what, t, n):
        """elements past the logical extent keep their NaN fill"""
        tail = t.reshape(-1)[n:]
        if tail.numel() and not torch.isnan(tail.float()).all():
            self.fails.append(f'{what}: elements past the logical extent were written')

    def widen(self, what, risk):
        share = risk.double().mean().item()
        self.widened[what] = share
        if share > WIDEN_CAP:
            self.fails.append(f'{what}: {share:.2e} of the elements sit on a derivative switch (cap {WIDEN_CAP})')


def _mask(ops, n, p, seed, shape):
    """dropout keep-mask * scale of a tensor of n elements, from the stand-alone GELU + dropout kernel: groups of four by element
    index, the indexing of norm.hip dropmaskv (element index >> 2, + q for the q-th group of a vector)"""
    if p == 0:
        return torch.ones(shape, dtype=torch.float64)
    assert n % 4 == 0
    with ops.use(ops.Context()):
        m = _masks(ops, n // 4, 4, p, (seed, seed, seed))[0]
    vals = torch.unique(m)
    assert vals.numel() == 2 and vals[0].item() == 0.0 and abs(vals[1].item() - 1 / (1 - p)) < 1e-6, vals
    return m.double().reshape(shape)


def _zeros(shape):
    return torch.zeros(shape, device=DEV, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------- GPU: InstanceNorm

def run_in(case, ck):
    from lintransunet_amd import _lib, ops
    s = case.shape
    B, S, C, p, mode = s['B'], s['S'], s['C'], s['p'], s['mode']
    n = B * S * C
    x, res, gs = in_operands(case)
    act = ops.ACT_LRELU if s['act'] else ops.ACT_NONE
    seed = 1000 + _seed(case)
    xg, resg = _dev(x), (_dev(res) if res is not None else None)
    y, dx = _nan((n + 64 * C,)), _nan((n + 64 * C,))
    sums, bsums = _zeros((B, C, 3)), _zeros((B, C, 2))
    ws = torch.empty(_lib.load().ltu_norm_ws_floats(), device=DEV, dtype=torch.float32) if s['ws'] else None
    nws = ws.numel() if ws is not None else 0
    seen = {}
    shift, s1, s2, m1 = R.in_sums(x)
    if mode == 'apply':
        # sums from the caller: the float64 sums rounded to fp32
        sums.copy_(torch.stack((shift, s1, s2), -1).float())
        _, seen['fwd'] = launched(lambda: _call('ltu_instnorm_apply', _ptr(xg), _ptr(sums), _ptr(resg), _ptr(y), B, S, C, act, R.LRELU_SLOPE,
                                                float(p), seed, 0, ops.BF16, _stream()))
    elif mode == 'stats':
        _, seen['fwd'] = launched(lambda: _call('ltu_instnorm_stats', _ptr(xg), _ptr(sums), _ptr(ws), nws, B, S, C, ops.BF16, _stream()))
    else:
        _, seen['fwd'] = launched(lambda: _call('ltu_instnorm_fwd', _ptr(xg), _ptr(sums), _ptr(ws), nws, _ptr(resg), _ptr(y), B, S, C, act,
                                                R.LRELU_SLOPE, float(p), seed, 0, ops.BF16, _stream()))
    torch.cuda.synchronize()
    G = sums.double().cpu()
    const = (s1 == 0) & (s2 == 0)
    # -- stage 1: the published {shift, s1, s2}
    ck.exact('shift', G[..., 0], shift)
    ck.f32('s1', G[..., 1], s1, m1)
    ck.f32('s2', G[..., 2], s2, s2)
    if s['edge'] == 'const':
        assert const[:, 1:3].all() and not const[:, 3:].any()
        ck.exact('s1, s2 of the constant channels', G[:, 1:3, 1:], torch.zeros(B, 2, 2, dtype=torch.float64))
    # -- statistics end to end: mean / rstd from the published sums against float64 mean / variance; k = |shift - mean| / sigma
    mean_t, var_t = x.mean(1), x.var(1, unbiased=False)
    rstd_t = 1 / torch.sqrt(var_t + R.IN_EPS)
    k2 = torch.where(var_t > 0, (shift - mean_t) ** 2 / var_t.clamp_min(1e-300), torch.zeros_like(var_t))
    mean_g, rstd_g = R.in_stat2(G[..., 0], G[..., 1], G[..., 2], S)
    ck.f32('mean', mean_g, mean_t, m1 / S)
    ck.f32('rstd', rstd_g, rstd_t, rstd_t * (1 + k2))
    if mode == 'stats':
        return seen
    mask = _mask(ops, n, p, seed, (B, S, C))
    ck.untouched('y', y, n)
    Y = y[:n].double().cpu().reshape(B, S, C)
    # -- stage 2: y from the kernel's own sums
    h = R.in_hat(x, mean_g, rstd_g)
    ck.bf16('y', Y, R.in_apply(h, s['act'], mask, res))
    # end to end; named term: the statistics' 1e-5 (1 + k^2) on xhat
    h_t = R.in_hat(x, mean_t, rstd_t)
    ck.bf16('y end to end', Y, R.in_apply(h_t, s['act'], mask, res), extra=F32_REL * (1 + k2)[:, None, :] * h_t.abs() * mask)
    if s['edge'] == 'const':
        ck.exact('y of the constant channels == res', Y[:, :, 1:3], res[:, :, 1:3])
    if mode == 'apply':
        return seen
    gg3 = [_dev(t) for t in gs] + [None] * (3 - len(gs))
    _, seen['bwd'] = launched(lambda: _call('ltu_instnorm_bwd', _ptr(gg3[0]), _ptr(gg3[1]), _ptr(gg3[2]), _ptr(xg), _ptr(sums), _ptr(bsums),
                                            _ptr(ws), nws, _ptr(dx), B, S, C, act, R.LRELU_SLOPE, float(p), seed, 0, ops.BF16, _stream()))
    torch.cuda.synchronize()
    ck.untouched('dx', dx, n)
    # -- stage 3: bsums; at-risk elements (xhat within 2^-14 of the LeakyReLU switch) widen by the difference between the branches
    gsum = sum(gs)
    gm = (gsum * mask).abs()
    risk = R.in_risk(x, mean_g, rstd_g, const) if s['act'] else torch.zeros(B, S, C, dtype=torch.bool)
    ck.widen('dx', risk)
    branch = torch.where(risk, gm * (1 - R.LRELU_SLOPE), torch.zeros_like(gm))
    gg = R.in_bwd_g(gsum, h, s['act'], mask)
    bs_ref, bs_mag = R.in_bwd_sums(gg, h)
    BS = bsums.double().cpu()
    ck.f32('bsums', BS, bs_ref, bs_mag, extra=torch.stack((branch.sum(1), (branch * h.abs()).sum(1)), -1))
    # -- stage 4: dx from the kernel's own bsums
    DX = dx[:n].double().cpu().reshape(B, S, C)
    ck.bf16('dx', DX, R.in_bwd_apply(gg, h, rstd_g, BS, S), extra=rstd_g[:, None, :] * branch)
    if s['edge'] == 'const':
        want = torch.full((B, 2), R.IN_EPS ** -0.5, dtype=torch.float64)
        ck.f32('rstd of the constant channels = eps^-1/2', rstd_g[:, 1:3], want, want * 1e-7)
    return seen


# ---------------------------------------------------------------------------------------------- GPU: attention gate

def run_gate(case, ck):
    from lintransunet_amd import _lib, ops
    s = case.shape
    B, S, C = s['B'], s['S'], s['C']
    M, n = B * S, B * S * C
    u1, u2, skip, dout, pw, pb = gate_operands(case)
    u1g, u2g, skg = _dev(u1), _dev(u2), _dev(skip)
    pwg, pbg = _dev(pw, torch.float32), _dev(pb, torch.float32)
    nws = _lib.load().ltu_norm_ws_floats()
    ws = torch.empty(nws, device=DEV, dtype=torch.float32)
    st1, st2 = _zeros((B, C, 3)), _zeros((B, C, 3))
    _call('ltu_instnorm_stats', _ptr(u1g), _ptr(st1), _ptr(ws), nws, B, S, C, ops.BF16, _stream())
    _call('ltu_instnorm_stats', _ptr(u2g), _ptr(st2), _ptr(ws), nws, B, S, C, ops.BF16, _stream())
    a, out = _nan((M + 64,), torch.float32), _nan((n + 64 * C,))
    seen = {}
    _, seen['fwd'] = launched(lambda: _call('ltu_gate_fwd', _ptr(u1g), _ptr(u2g), _ptr(st1), _ptr(st2), _ptr(pwg), _ptr(pbg), _ptr(skg), _ptr(a),
                                            _ptr(out), B, S, C, ops.BF16, _stream()))
    torch.cuda.synchronize()
    ck.untouched('a', a, M)
    ck.untouched('out', out, n)
    G1, G2 = st1.double().cpu(), st2.double().cpu()
    m1, r1 = R.in_stat2(G1[..., 0], G1[..., 1], G1[..., 2], S)
    m2, r2 = R.in_stat2(G2[..., 0], G2[..., 1], G2[..., 2], S)
    h1, h2 = R.in_hat(u1, m1, r1), R.in_hat(u2, m2, r2)
    _, sdot, a_ref = R.gate_fwd(h1, h2, pw, pb, skip)
    # a = sigmoid(sdot): 1e-5 of the magnitudes summed into sdot (the xhat differences included) through sigmoid' = a (1 - a), + 1e-5 a
    hmag = (u1.abs() + m1.abs()[:, None, :]) * r1[:, None, :] + (u2.abs() + m2.abs()[:, None, :]) * r2[:, None, :]
    smag = (hmag * pw.abs()).sum(-1) + pb.abs()
    A = a[:M].double().cpu().reshape(B, S)
    ck.f32('a', A, a_ref, a_ref + a_ref * (1 - a_ref) * smag)
    ck.bf16('out', out[:n].reshape(B, S, C), skip * A[..., None])
    if s['fwd_only']:
        return seen
    dskip, du1, du2 = (_nan((n + 64 * C,)) for _ in range(3))
    ds = _nan((M + 64,), torch.float32)
    dpw, dpb, bs1, bs2 = _zeros((C,)), _zeros((1,)), _zeros((B, C, 2)), _zeros((B, C, 2))
    gg = _dev(dout)
    wsb = ws if s['ws'] else None
    _, seen['bwd'] = launched(lambda: _call('ltu_gate_bwd', _ptr(gg), _ptr(u1g), _ptr(u2g), _ptr(st1), _ptr(st2), _ptr(pwg), _ptr(skg), _ptr(a),
                                            _ptr(dskip), _ptr(ds), _ptr(dpw), _ptr(dpb), _ptr(bs1), _ptr(bs2), _ptr(wsb), nws if s['ws'] else 0,
                                            _ptr(du1), _ptr(du2), B, S, C, ops.BF16, _stream()))
    torch.cuda.synchronize()
    for what, t, k in (('dskip', dskip, n), ('du1', du1, n), ('du2', du2, n), ('ds', ds, M)):
        ck.untouched(what, t, k)
    # -- stage 1: dskip and ds from the kernel's own a
    dskip_ref, ds_ref = R.gate_bwd_reduce(dout, skip, A)
    ck.bf16('dskip', dskip[:n].reshape(B, S, C), dskip_ref)
    DS = ds[:M].double().cpu().reshape(B, S)
    ck.f32('ds', DS, ds_ref, (dout * skip).abs().sum(-1) * A * (1 - A))
    # -- the fp32 sums from the kernel's own ds; pre-activations within 2^-14 of the ReLU switch widen by |dr|, the branch difference
    risk = R.gate_risk(u1, m1, r1, u2, m2, r2)
    ck.widen('du', risk)
    dr_abs = (DS[..., None] * pw).abs()
    branch = torch.where(risk, dr_abs, torch.zeros_like(dr_abs))
    dpw_ref, dpb_ref, bs1_ref, bs2_ref = R.gate_sums(DS, h1, h2, pw)
    dr = R.gate_dr(DS, h1, h2, pw)
    ck.grad('dpsi_w', dpw, dpw_ref)
    ck.f32('dpsi_b', dpb, dpb_ref.reshape(1), DS.abs().sum().reshape(1))
    BS1, BS2 = bs1.double().cpu(), bs2.double().cpu()
    for what, got, ref, hh in (('bs1', BS1, bs1_ref, h1), ('bs2', BS2, bs2_ref, h2)):
        mag = torch.stack((dr.abs().sum(1), (dr * hh).abs().sum(1)), -1)
        ck.f32(what, got, ref, mag, extra=torch.stack((branch.sum(1), (branch * hh.abs()).sum(1)), -1))
    # -- stage 2: du1, du2 from the kernel's own ds, bs1, bs2
    ck.bf16('du1', du1[:n].reshape(B, S, C), R.gate_bwd_apply(dr, h1, r1, BS1, S), extra=r1[:, None, :] * branch)
    ck.bf16('du2', du2[:n].reshape(B, S, C), R.gate_bwd_apply(dr, h2, r2, BS2, S), extra=r2[:, None, :] * branch)
    return seen


# ---------------------------------------------------------------------------------------------- GPU: small pointwise projections

def run_pw(case, ck):
    from lintransunet_amd import ops
    s = case.shape
    M, K, N, acc = s['M'], s['K'], s['N'], s['acc']
    g = _gen(_seed(case))
    x = _bf(torch.randn(M, K, generator=g))
    W = _bf(torch.randn(N, K, generator=g) / math.sqrt(K))
    b = _f32(0.1 * torch.randn(N, generator=g)) if s['bias'] else None
    y0 = _bf(torch.randn(M, N, generator=g)) if acc else None
    xg, wg = _dev(x), _dev(W)
    bg = _dev(b, torch.float32) if b is not None else None
    y = _nan((M + 32, N))
    if acc:
        y[:M] = _dev(y0)
    _, fwd = launched(lambda: _call('ltu_linear_fwd', _ptr(xg), K, ops._ptr_array([wg]), 1, ops._ptr_array([bg]), _ptr(y), N, M, N, K, acc,
                                    ops.BF16, _stream()))
    torch.cuda.synchronize()
    ck.untouched('y', y, M * N)
    prod = x @ W.T + (b if b is not None else 0)
    if acc:
        # the kernel rounds the product (+ bias) to bf16, adds the old bf16 value and rounds again; an element whose fp32 product lies
        # at a rounding midpoint gets one ulp of slack (the siblings' `rounded`)
        mag = x.abs() @ W.abs().T + (b.abs() if b is not None else 0)
        pb_, sl = R.rounded(prod, mag)
        ck.bf16('y', y[:M], pb_ + y0, extra=sl)
    else:
        ck.bf16('y', y[:M], prod)
    return {'fwd': fwd}


# ---------------------------------------------------------------------------------------------- GPU: positional depthwise conv

def run_dw(case, ck):
    from lintransunet_amd import _lib, ops
    s = case.shape
    B, H, W, D, C, p = s['B'], s['H'], s['W'], s['D'], s['C'], s['p']
    n = B * H * W * D * C
    g = _gen(_seed(case))
    x = _bf(torch.randn(B, H, W, D, C, generator=g))
    w, b = _f32(0.3 * torch.randn(C, 1, 3, 3, 3, generator=g)), _f32(torch.randn(C, generator=g))
    gs = [_bf(torch.randn(B, H, W, D, C, generator=g)) for _ in range(s['ports'])]
    dw0, db0 = _f32(torch.randn(C, 1, 3, 3, 3, generator=g)), _f32(torch.randn(C, generator=g))      # the kernels add to existing gradients
    seed = 3000 + _seed(case)
    xg, wg, bg = _dev(x), _dev(w, torch.float32), _dev(b, torch.float32)
    y, dx = _nan((n + 64 * C,)), _nan((n + 64 * C,))
    seen = {}
    _, seen['fwd'] = launched(lambda: _call('ltu_dwconv_fwd', _ptr(xg), _ptr(wg), _ptr(bg), _ptr(y), B, H, W, D, C, float(p), seed, 0, ops.BF16,
                                            _stream()))
    torch.cuda.synchronize()
    ck.untouched('y', y, n)
    Y = y[:n].double().cpu().reshape(B, H, W, D, C)
    # channel dropout: one draw per (sample, channel); read off the forward: dropped planes are exactly 0
    keep = float(np.float32(1) / (np.float32(1) - np.float32(p)))
    dropped = (Y == 0).all(1).all(1).all(1)
    if p == 0:
        assert not dropped.any()
    elif B * C >= 64:
        share = dropped.double().mean().item()
        assert abs(share - p) < 0.15, f'channel dropout drew {share:.2f} of the planes, p = {p}'
    mask = torch.where(dropped, 0.0, keep).double()
    ck.bf16('y', Y, R.dw_fwd(x, w, b, mask))
    # backward: the same mask; two gradient ports are summed to bf16 while staging (pointwise.hip add16)
    gsum = gs[0] if len(gs) == 1 else (gs[0].float() + gs[1].float()).bfloat16().double()
    gg = [_dev(t) for t in gs] + [None]
    dwt, db = _nan(((C + 8) * 27,), torch.float32), _nan((C + 8,), torch.float32)
    dwt[:C * 27] = _dev(dw0, torch.float32).reshape(-1)
    db[:C] = _dev(db0, torch.float32)
    nws = _lib.load().ltu_dwconv_bwd_ws_floats(B, H, W, D, C, ops.BF16)
    ws = torch.empty(nws, device=DEV, dtype=torch.float32) if s['ws'] else None

    def bwd():
        tail = (B, H, W, D, C, float(p), seed, 0, ops.BF16, _stream())
        if s['split']:
            _call('ltu_dwconv_bwd', _ptr(gg[0]), _ptr(gg[1]), _ptr(xg), _ptr(wg), _ptr(dx), 0, 0, 0, 0, *tail)
            _call('ltu_dwconv_bwd', _ptr(gg[0]), _ptr(gg[1]), _ptr(xg), _ptr(wg), 0, _ptr(dwt), _ptr(db), _ptr(ws), nws if s['ws'] else 0, *tail)
        else:
            _call('ltu_dwconv_bwd', _ptr(gg[0]), _ptr(gg[1]), _ptr(xg), _ptr(wg), _ptr(dx), _ptr(dwt), _ptr(db), _ptr(ws), nws if s['ws'] else 0, *tail)
    _, seen['bwd'] = launched(bwd)
    torch.cuda.synchronize()
    ck.untouched('dx', dx, n)
    ck.untouched('dw', dwt, C * 27)
    ck.untouched('db', db, C)
    dx_ref, dw_ref, db_ref = R.dw_bwd(gsum, x, w, mask)
    ck.bf16('dx', dx[:n].reshape(B, H, W, D, C), dx_ref)
    ck.grad('dw', dwt[:C * 27].double().cpu().reshape(dw0.shape) - dw0, dw_ref)
    ck.grad('db', db[:C].double().cpu() - db0, db_ref)
    return seen


# ---------------------------------------------------------------------------------------------- GPU: trilinear

def run_tri(case, ck):
    from lintransunet_amd import ops
    s = case.shape
    B, H, W, D, C, sd, ports = s['B'], s['H'], s['W'], s['D'], s['C'], s['sd'], s['ports']
    g = _gen(_seed(case))
    x = _bf(torch.randn(B, H, W, D, C, generator=g))
    gs = [_bf(torch.randn(B, 2 * H, 2 * W, sd * D, C, generator=g)) for _ in range(ports)]
    xg = _dev(x).requires_grad_(True)
    seen = {}
    with ops.use(ops.Context()):
        ys, seen['fwd'] = launched(lambda: ops.trilinear_up(xg, sd, fork=ports))
        ys = ys if ports > 1 else (ys,)
        _, seen['bwd'] = launched(lambda: torch.autograd.backward(list(ys), [_dev(t) for t in gs]))
    torch.cuda.synchronize()
    Ah, Aw, Ad = R.tri_matrix(H, 2 * H), R.tri_matrix(W, 2 * W), R.tri_matrix(D, sd * D)
    Sh, Sw, Sd = R.tri_support(Ah), R.tri_support(Aw), R.tri_support(Ad)
    # TAP: the fp32 tap weights of an upsampled axis are within 2^-22 L_in of exact
    th, tw, td = TAP * H, TAP * W, (TAP * D if sd == 2 else 0.0)
    ck.bf16('y', ys[0], R.tri_fwd(x, Ah, Aw, Ad), extra=(th + tw + td) * R.tri_fwd(x.abs(), Sh, Sw, Sd))
    gsum = sum(gs)
    adj = R.tri_adj_axis
    if not case.flags.get('SEPARABLE_TRILINEAR_ADJOINT', True):
        # the 64-tap gather: one fp32 sum, one rounding
        ref = adj(adj(adj(gsum, Ad, 3), Aw, 2), Ah, 1)
        ck.bf16('dx', xg.grad, ref, extra=(th + tw + td) * adj(adj(adj(gsum.abs(), Sd, 3), Sw, 2), Sh, 1))
        return seen
    # separable (roi.hip ltu_trilinear_adjoint): depth (sd == 2), width, height; every pass stores bf16: the reference rounds after each
    # pass.  `carry` is what the kernel's value may be off by where a pass rounds it: the TAP term and the slack of the earlier passes,
    # carried through the later ones; a value that close to a rounding midpoint (or within fp32 noise of one) gets one more ulp
    t, carry = gsum, torch.zeros_like(gsum)
    for axis, A, Sx, tap, on in ((3, Ad, Sd, td, sd == 2), (2, Aw, Sw, tw, True)):
        if not on:
            continue
        v, mag = adj(t, A, axis), adj(t.abs(), A, axis)
        carry = adj(carry, A, axis) + tap * adj(t.abs(), Sx, axis)
        t, sl = R.rounded(v, mag + carry / R.RISK)
        carry = carry + sl
    ck.bf16('dx', xg.grad, adj(t, Ah, 1), extra=adj(carry, Ah, 1) + th * adj(t.abs(), Sh, 1))
    # the same call through the C-ABI with a workspace of the test's own: every pass against float64 on the bf16 tensor the pass before
    # it stored (t1 [B][2H][2W][D][C] behind t2 [B][2H][W][D][C] in the workspace): no slack, the TAP term alone
    from lintransunet_amd import _lib
    nws = _lib.load().ltu_trilinear_adjoint_ws_elems(B, H, W, D, C, sd)
    wsb = torch.zeros(nws, device=DEV, dtype=torch.bfloat16)
    n, t2n = B * H * W * D * C, B * 2 * H * W * D * C
    dx2 = _nan((n + 64 * C,))
    gd = [_dev(v) for v in gs] + [None]
    _call('ltu_trilinear_adjoint', _ptr(gd[0]), _ptr(gd[1]), _ptr(dx2), _ptr(wsb), nws, B, H, W, D, C, sd, ops.BF16, _stream())
    torch.cuda.synchronize()
    ck.untouched('dx (C-ABI)', dx2, n)
    ck.exact('dx (C-ABI) == dx (ops)', dx2[:n].reshape(B, H, W, D, C), xg.grad.double().cpu())
    src = gsum
    if sd == 2:
        T1 = wsb[t2n:3 * t2n].double().cpu().reshape(B, 2 * H, 2 * W, D, C)
        ck.bf16('depth pass', T1, adj(src, Ad, 3), extra=td * adj(src.abs(), Sd, 3))
        src = T1
    T2 = wsb[:t2n].double().cpu().reshape(B, 2 * H, W, D, C)
    ck.bf16('width pass', T2, adj(src, Aw, 2), extra=tw * adj(src.abs(), Sw, 2))
    ck.bf16('height pass', dx2[:n].reshape(B, H, W, D, C), adj(T2, Ah, 1), extra=th * adj(T2.abs(), Sh, 1))
    return seen


# ---------------------------------------------------------------------------------------------- GPU: ROI plans

def run_roi(case, ck):
    from lintransunet_amd import ops
    s = case.shape
    C = s['C']
    Gd = np.load(os.path.join(GOLDEN, 'roi.npz'))
    masks, boxes, sizes = [], [], set()
    for name in s['masks']:
        m = torch.from_numpy(Gd[f'{name.rstrip("!")}_mask'])[0, 0]            # bool [H, W, D]
        sizes.add(int(Gd[f'{name.rstrip("!")}_roi_size']))
        masks.append(m.flip(0, 1) if name.endswith('!') else m)
        boxes.append(None if name.endswith('!') else torch.from_numpy(Gd[f'{name}_box'])[0])
    (roi_size,) = sizes
    fg = torch.stack(masks).float()
    B, H, W, D = fg.shape
    prob = torch.stack((1 - fg, fg), -1).contiguous().to(DEV)
    seen = {}
    g = _gen(_seed(case))
    with ops.use(ops.Context()):
        plan, seen['plan'] = launched(lambda: ops.RoiPlan(prob, roi_size, 0.5))
        box = plan.box.cpu()
        for b, want in enumerate(boxes):
            if want is not None:
                ck.exact(f'box[{b}] (golden, bit-exact)', box[b], want.double())
        assert len({tuple(r.tolist()) for r in box}) == B, 'the samples must have different boxes'
        ib, fb = plan.ibuf.cpu(), plan.fbuf.cpu()
        offs = R.plan_offsets(B, H, W, plan.eval_h, plan.eval_w)
        assert offs['n_int'] == ib.numel() and offs['n_float'] == fb.numel()
        mats = {}
        for name in ('fh', 'fw', 'bh', 'bw'):
            A, T = R.plan_matrices(ib, fb, offs[name], B)
            ck.exact(f'{name}: adjoint lists == transposed forward taps', T, A.transpose(1, 2))
            assert (A.sum(-1) > 0).any(), name
            mats[name] = A
        seen['fwd'], seen['bwd'] = set(), set()
        for which, (ph, pw_), fn in ((0, ('fh', 'fw'), ops.roi_warp), (1, ('bh', 'bw'), ops.roi_unwarp)):
            Ah, Aw = mats[ph], mats[pw_]
            x = _bf(torch.randn(B, Ah.shape[2], Aw.shape[2], D, C, generator=g))
            xg = _dev(x).requires_grad_(True)
            y, k = launched(lambda: fn(xg, plan))
            seen['fwd'] |= k
            go = _bf(torch.randn(B, Ah.shape[1], Aw.shape[1], D, C, generator=g))
            _, k = launched(lambda: y.backward(_dev(go)))
            seen['bwd'] |= k
            torch.cuda.synchronize()
            ck.bf16(f'gather[{which}]', y, R.plan_apply(x, Ah, Aw))
            ck.bf16(f'scatter[{which}]', xg.grad, R.plan_apply(go, Ah.transpose(1, 2), Aw.transpose(1, 2)))
    return seen


# ---------------------------------------------------------------------------------------------- GPU: first-level conv weight-gradient fold

def run_conv_wgrad(case, ck):
    """the conv table's runner on a first-level shape: dw (the fp32 gradient wgrad_reduce_kernel<64> folds) against float64 at WGRAD_TOL"""
    res = conv_paths.run_case(conv_paths.Case(case.name, 'conv3d', case.shape, {}))
    ck.ratio.update(res['ratio'])
    ck.fails.extend(res['fails'])
    assert 'dw' in res['ratio'] and 'db' in res['ratio']
    return {k: set(v) for k, v in res['seen'].items()}


RUNNERS = {'in': run_in, 'gate': run_gate, 'pw': run_pw, 'dw': run_dw, 'tri': run_tri, 'roi': run_roi, 'conv_wgrad': run_conv_wgrad}


def run_case(case):
    """runs one case on the GPU; returns {'seen': {window: kernels}, 'ratio': {output: worst error / bound}, 'widened', 'fails'}"""
    from lintransunet_amd import ops
    ck = Ck()
    old = {k: getattr(ops, k) for k in case.flags}
    for k, v in case.flags.items():
        setattr(ops, k, v)
    try:
        with knobs(case.knobs):
            seen = RUNNERS[case.op](case, ck)
    finally:
        for k, v in old.items():
            setattr(ops, k, v)
    return {'seen': {k: sorted(v) for k, v in seen.items()}, 'ratio': ck.ratio, 'widened': ck.widened, 'fails': ck.fails}


def missing_kernels(case, seen):
    out = [f'{w}: {k}' for w, names in case.kernels.items() for k in names if k not in seen.get(w, ())]
    out += [f'{w}: {k} ran (must not)' for w, prefixes in case.absent.items() for k in seen.get(w, ()) if any(k.startswith(p) for p in prefixes)]
    return out


def _report(case, res):
    path = os.environ.get('LTU_STREAM_PATHS_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps({'case': case.name, 'op': case.op, 'kernels': case.kernels, 'knobs': case.knobs, 'flags': case.flags,
                                'geometry': geometry(case)[0], **res}) + '\n')


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from lintransunet_amd import ops  # noqa: F401
    return True


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_stream_path(gpu, case):
    res = run_case(case)
    _report(case, res)
    worst = max(res['ratio'].items(), key=lambda kv: kv[1]) if res['ratio'] else None
    print(f'[stream path {case.name}] worst error / bound {worst}, widened {res["widened"]}')
    assert not res['fails'], f'{case.name}: ' + '; '.join(res['fails'])
    miss = missing_kernels(case, res['seen'])
    assert not miss, f'{case.name}: {miss}; launched {res["seen"]}'
