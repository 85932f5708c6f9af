"""Every bf16 kernel of the transformers' token path by name, against float64 references stage by stage.

The token path is a set of launchers with fallbacks, steered by shapes, LTU_* knobs and module flags: the row-block chain kernels
(tlayer.hip: ltu_layer_tail_fwd / ltu_layer_tail_bwd), the linear-attention core (linattn.hip), the weight-stationary projection
ring (gemm_ring.hip: linear_ring_bf16_kernel, with the GELU + dropout epilogue), the grouped and deferred weight gradients
(wgrad_group_ring + wgroup_fold, wgrad_ring + wgrad_reduce / ltu_reduce_batch), the fragment-order weight prep (misc.hip) and
the op-by-op fallbacks (LayerNorm, GELU + dropout).  Each case below names the kernels that must run for its op, shape and knobs;
torch.profiler witnesses the launches (one window per direction).

The references are float64 on the CPU and are computed PER STAGE from the bf16 / fp32 tensors the kernels stored (the chain
kernels are driven through their C-ABI so that every intermediate is at hand), not end to end: rounding does not pile up along the
chain and the gates stay tight.  Where a kernel rounds a value to bf16 that it does not store, the reference rounds it the same way
(float64 -> fp32 -> bf16, round to nearest even: `rounded`); where the kernel's fp32 value lies so close to a rounding midpoint that
it may round the other way, that element is allowed one bf16 ulp, propagated through the stage (`slack`).  Gates:

* bf16 outputs per element: |got - ref| <= 2^-8 |ref| + 1e-5 max|ref| (+ the propagated slack of unstored rounded intermediates,
  and, where a stage reads a bf16 value the kernel rounded from an fp32 one it used itself, 2^-8 times that value's contribution;
  each such term is named where it is added);
* fp32 statistics (LayerNorm mean / rstd, attention row and column statistics) and the attention context: relative 1e-5 of the
  magnitude of the sum they are (plus the slack or rounding terms named at the check);
* fp32 weight and bias gradients: max|got - ref| / max|ref| <= 1e-4, as in test_gpu_conv_paths.py; the key-projection bias gradient
  of a layer is mathematically zero (test_gpu_layer.py keeps an absolute floor for it) and is not formed here: the weight-gradient
  cases take random operands;
* rows past M (a partly empty last row block) are never written, every output is finite.

Dropout masks (p = 0.3, the benchmarked value) are rebuilt from the stand-alone gelu_dropout kernel, which shares the counter hash
(see test_gpu_layer._masks), and applied at the sites of model/trans_block.py:203-211: after the out projection (seed 1), after GELU
(seed g), after linear2 (seed 2).

Fragment-order weights (weight prep kinds 8 and 9) are not restated: every chain-kernel stage reads them and is checked against the
logical weights, so a misplaced fragment fails the stage that reads it.

Module flags: ops.USE_LAYER_TAIL / USE_LAYER_TAIL_BWD select the chain kernels or the op-by-op kernels (the `ln` and `linear_gelu`
cases with LTU_NO_GELU_FUSE / LTU_NO_NT_RING cover the latter), ops.FUSE_ATTN_APPLY the attention's phase B inside the chain
kernel (ATTN instances) or linattn_apply_rows (the `linattn` cases), ops.FUSE_NEXT_QKV the QKV instances.  Every instance those
flags can select is named by a case below.

The CPU tests (no GPU) check that the table names every token-family kernel of the newest profiles/r*_bench_kernel_stats.csv, that
every obligation has a case and every case is needed, that the named kernels exist, and the long-run geometry of the ring cases.
LTU_TOKEN_PATHS_REPORT=<file> appends one JSON line per GPU case: kernels launched, geometry, worst error / bound per output.
"""
import ctypes
import glob
import json
import math
import os
import re

import pytest
import torch

from tests.test_gpu_conv_paths import FAMILY as CONV_FAMILY, GEMMS as CONV_GEMMS, _newest_profile, kernel_base, knobs, launched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'lintransunet_amd', 'csrc')
DEV = 'cuda'

BF16_REL = 2.0 ** -8         # bf16 rounding of the fp32 result (8 significant bits)
BF16_ABS = 1e-5              # fp32 accumulation noise, relative to the tensor's max
F32_REL = 1e-5               # fp32 statistics / context, relative to the magnitude of their sums
WGRAD_TOL = 1e-4             # fp32 weight / bias gradients, relative to the max
# an fp32 sum of K <= 768 products of bf16 values is within K 2^-24 <= 2^-14 of the sum of magnitudes of its float64 value: closer
# than that to a bf16 rounding midpoint, the kernel's value may round to the other neighbour
RISK = 2.0 ** -14
LN_EPS = 1e-6
P_DROP = 0.3


# ---------------------------------------------------------------------------------------------- the table

class Case:
    """op 'tail' (B, N, d, p, umode, attn, nq, dy2), 'linattn' (B, N, d), 'linear' (M, K, N, nw), 'linear_gelu' (M, K, N, p),
    'ln' (M, d, p, dy2) or 'wgrad' (M, d, mode); kernels: direction ('prep' / 'fwd' / 'bwd') -> demangled kernel names that must
    run; absent: direction -> name prefixes that must not run; steady: [(geometry family, width knob)] of a long-run case"""

    def __init__(self, name, op, shape, kernels, knobs=None, steady=None, absent=None):
        self.name, self.op, self.shape, self.kernels = name, op, shape, kernels
        self.knobs = dict(knobs or {})
        self.steady = steady
        self.absent = dict(absent or {})

    def __repr__(self):
        return self.name


def tail(B, N, d, p=0.0, umode=1, attn=False, nq=False, dy2=False):
    return dict(B=B, N=N, d=d, p=p, umode=umode, attn=attn, nq=nq, dy2=dy2)


def tf(d, attn, qkv):
    return f'tail_fwd_kernel<{d}, {str(attn).lower()}, {str(qkv).lower()}, 4>'


def tb(d, umode, wps, preu):
    return f'tail_bwd_kernel<{d}, {umode}, {wps}, {str(preu).lower()}>'


def ring(wm, tnw, r, gelu=False):
    return f'linear_ring_bf16_kernel<{wm}, {tnw}, {r}, {str(gelu).lower()}>'


def la(kind, d):
    return f'linattn_{kind}<bf16_t, {d}>'


PREP1, PREP4 = 'weight_prep_chunk_kernel<bf16_t, 1>', 'weight_prep_chunk_kernel<bf16_t, 4>'
WG, FOLD, TN6 = 'wgrad_group_ring_bf16_kernel<6>', 'wgroup_fold_kernel', 'wgrad_ring_bf16_kernel<6>'
RED = 'wgrad_reduce_kernel<{}>'.format
GELU_F, GELU_B = 'gelu_drop_bf16x8_kernel<false>', 'gelu_drop_bf16x8_kernel<true>'      # the bf16 forms (pointwise.hip)

CASES = [
    # ---- row-block chain kernels (tlayer.hip), driven through the C-ABI ----------------------------------------------------------
    # every forward instance (d x fused phase B x fused next q|k|v) and every backward instance (d x u_mode x WPS x PRE_U) of the
    # default build; the forward's u_mode follows the backward's.  Ragged M: the last row block is partly empty.
    Case('tail128_ragged_drop', 'tail', tail(1, 999, 128, P_DROP, dy2=True),
         {'prep': [PREP1], 'fwd': [tf(128, False, False)], 'bwd': [tb(128, 1, 4, True)]}),
    # B > 1, N % 32 == 0: phase B of the attention inside the chain kernel (linattn_ctx in front); d = 128 at three waves per SIMD
    Case('tail128_attn_drop_wps3', 'tail', tail(2, 320, 128, P_DROP, attn=True),
         {'fwd': [la('kv_partial', 128), 'linattn_kv_combine1<4>', tf(128, True, False)], 'bwd': [tb(128, 1, 3, True)]},
         {'LTU_TAIL_BWD_WPS': 3}),
    Case('tail128_attn_qkv_umode0', 'tail', tail(2, 160, 128, umode=0, attn=True, nq=True, dy2=True),
         {'fwd': [tf(128, True, True)], 'bwd': [tb(128, 0, 4, True)]}),
    # the next layer's q|k|v inside the chain kernel on a ragged M; the long weight-prep form (four chunks per trip) by its knob
    Case('tail128_qkv_ragged_nopreu', 'tail', tail(1, 777, 128, P_DROP, nq=True),
         {'prep': [PREP4], 'fwd': [tf(128, False, True)], 'bwd': [tb(128, 1, 4, False)]},
         {'LTU_TAIL_BWD_PREU': 0, 'LTU_WPREP_NC4_MIN': 1}),
    Case('tail128_umode0_wps3', 'tail', tail(1, 515, 128, P_DROP, umode=0),
         {'fwd': [tf(128, False, False)], 'bwd': [tb(128, 0, 3, True)]}, {'LTU_TAIL_BWD_WPS': 3}),
    Case('tail128_umode0_nopreu', 'tail', tail(3, 111, 128, umode=0),
         {'fwd': [tf(128, False, False)], 'bwd': [tb(128, 0, 4, False)]}, {'LTU_TAIL_BWD_PREU': 0}),
    Case('tail256_attn_drop', 'tail', tail(2, 224, 256, P_DROP, attn=True),
         {'fwd': [la('kv_partial', 256), tf(256, True, False)], 'bwd': [tb(256, 1, 4, False)]}),
    Case('tail256_attn_qkv_preu', 'tail', tail(3, 96, 256, P_DROP, attn=True, nq=True, dy2=True),
         {'fwd': [tf(256, True, True)], 'bwd': [tb(256, 1, 4, True)]}, {'LTU_TAIL_BWD_PREU': 1}),
    Case('tail256_ragged_umode0_drop', 'tail', tail(1, 1003, 256, P_DROP, umode=0, dy2=True),
         {'fwd': [tf(256, False, False)], 'bwd': [tb(256, 0, 4, False)]}),
    Case('tail256_qkv_umode0_preu', 'tail', tail(1, 555, 256, umode=0, nq=True),
         {'fwd': [tf(256, False, True)], 'bwd': [tb(256, 0, 4, True)]}, {'LTU_TAIL_BWD_PREU': 1}),
    # ---- linear attention outside the chain kernel (N % 32 != 0 or ops.FUSE_ATTN_APPLY off): ltu_linattn_fwd / _bwd ---------------
    # LTU_LA_SPLITS sets the split count, which selects the merge: <= 32 splits kv_combine1<4> / dctx_combine<4>, <= 64 <8>,
    # <= 128 <16>, else <32> (at most 16 x 16 = 256 splits: the one-level merge takes every count, the two-level one needs its knob)
    Case('la128_ragged', 'linattn', dict(B=1, N=1003, d=128),          # 512 splits wanted, 32 tokens each: 32 splits
         {'fwd': [la('kv_partial', 128), 'linattn_kv_combine1<4>', 'linattn_apply_rows<128>'],
          'bwd': [la('dctx_partial', 128), 'linattn_dctx_combine<4>', la('bwd_apply', 128)]}),
    Case('la256_splits8', 'linattn', dict(B=1, N=1600, d=256),         # 64 wanted: 25 -> 32 tokens each, 50 splits
         {'fwd': [la('kv_partial', 256), 'linattn_kv_combine1<8>', 'linattn_apply_rows<256>'],
          'bwd': [la('dctx_partial', 256), 'linattn_dctx_combine<8>', la('bwd_apply', 256)]}, {'LTU_LA_SPLITS': 64}),
    Case('la128_splits16', 'linattn', dict(B=2, N=2500, d=128),        # 128 per sample wanted: 20 -> 32 tokens each, 79 splits
         {'fwd': ['linattn_kv_combine1<16>'], 'bwd': ['linattn_dctx_combine<16>']}, {'LTU_LA_SPLITS': 256}),
    Case('la256_splits32', 'linattn', dict(B=1, N=6000, d=256),        # 300 -> 256 wanted: 24 -> 32 tokens each, 188 splits
         {'fwd': ['linattn_kv_combine1<32>'], 'bwd': ['linattn_dctx_combine<32>']}, {'LTU_LA_SPLITS': 300}),
    Case('la128_two_level', 'linattn', dict(B=2, N=2500, d=128),       # 79 splits in 5 groups of <= 16, then the groups
         {'fwd': ['linattn_kv_combine']}, {'LTU_LA_SPLITS': 256, 'LTU_LA_TWO_LEVEL': 1}, absent={'fwd': ['linattn_kv_combine1']}),
    # ---- projections (gemm_ring.hip launch_nt_ring_bf16): data gradient = the same kernel on cat(W)^T -----------------------------
    # M < 2048 with K <= 256: one 64-column tile per workgroup; K = 384 (the q|k|v data gradient at d = 128): 128 columns, ring of 3.
    # The weight gradient of a ragged M is not the ring's (M % 32 != 0): the TN GEMM of the conv family
    Case('lin_qkv128_ragged', 'linear', dict(M=999, K=128, N=384, nw=3), {'fwd': [ring(4, 1, 4)], 'bwd': [ring(4, 2, 3)]}),
    # 255 row tiles of 32; LTU_RING_BLOCKS = 256 on one 128 x 128 tile: 32 splits of 8 units, the last one 7; 32 splits fold with <16>
    Case('lin_o128_long_runs', 'linear', dict(M=8160, K=128, N=128, nw=1),
         {'fwd': [ring(4, 2, 4)], 'bwd': [ring(4, 2, 4), TN6, RED(16)]}, {'LTU_RING_BLOCKS': 256},
         steady=[('tn_ring', 'LTU_RING_BLOCKS')]),
    # d = 256: q|k|v forward K = 256, its data gradient K = 768 (64-column tiles, ring of 3); weight gradient 9 splits: fold <4>
    Case('lin_qkv256', 'linear', dict(M=2080, K=256, N=768, nw=3), {'fwd': [ring(4, 2, 4)], 'bwd': [ring(4, 1, 3), TN6, RED(4)]}),
    # ---- projection + GELU + dropout (ltu_linear_gelu_fwd) -------------------------------------------------------------------------
    Case('gelu128_ring6', 'linear_gelu', dict(M=2100, K=128, N=256, p=P_DROP),
         {'fwd': [ring(4, 2, 6, True)], 'bwd': [GELU_B, ring(4, 2, 4)]}),
    Case('gelu256_ring5', 'linear_gelu', dict(M=2080, K=256, N=512, p=P_DROP),
         {'fwd': [ring(4, 2, 5, True)], 'bwd': [GELU_B, ring(4, 1, 4)]}),
    Case('gelu128_small', 'linear_gelu', dict(M=999, K=128, N=256, p=P_DROP), {'fwd': [ring(4, 1, 4, True)]}),
    # the op-by-op fallbacks: projection, then the stand-alone GELU + dropout kernel
    Case('gelu_no_fuse', 'linear_gelu', dict(M=999, K=128, N=256, p=P_DROP), {'fwd': [ring(4, 1, 4), GELU_F]},
         {'LTU_NO_GELU_FUSE': 1}, absent={'fwd': ['linear_ring_bf16_kernel<4, 1, 4, true>']}),
    Case('gelu_no_nt_ring', 'linear_gelu', dict(M=999, K=128, N=256, p=P_DROP), {'fwd': [GELU_F], 'bwd': [GELU_B]},
         {'LTU_NO_NT_RING': 1}, absent={'fwd': ['linear_ring_bf16_kernel'], 'bwd': ['linear_ring_bf16_kernel']}),
    # ---- op-by-op LayerNorm (ops.res_layernorm): ragged M, fp32 gamma / beta gradients folded at once (reduce_parts: 63 partials)
    Case('ln128_drop', 'ln', dict(M=999, d=128, p=P_DROP, dy2=False),
         {'fwd': ['layernorm_fwd_kernel<bf16_t, 16, 2>'], 'bwd': ['layernorm_bwd_kernel<bf16_t, 16, 2>', 'reduce_parts_kernel<4>']}),
    Case('ln256_dy2', 'ln', dict(M=333, d=256, p=0.0, dy2=True),
         {'fwd': ['layernorm_fwd_kernel<bf16_t, 32, 2>'], 'bwd': ['layernorm_bwd_kernel<bf16_t, 32, 2>']}),
    # ---- weight gradients of a layer's four projections (q|k|v, out, linear1, linear2) ------------------------------------------
    # grouped, fold mode: LTU_WGROUP_BLOCKS = 64 on 8 tiles (d = 128): 8 splits of 16 units, the last one 15
    Case('wgroup_fold_long_runs', 'wgrad', dict(M=4064, d=128, mode='group'), {'bwd': [WG, FOLD]}, {'LTU_WGROUP_BLOCKS': 64},
         steady=[('wgroup', 'LTU_WGROUP_BLOCKS')]),
    # one split: every tile adds its sums to the gradient itself (direct mode, no partials, no fold) ...
    Case('wgroup_direct', 'wgrad', dict(M=1056, d=256, mode='group'), {'bwd': [WG]}, {'LTU_WGROUP_BLOCKS': 1},
         absent={'bwd': [FOLD]}),
    # ... or, switched off, one split of partials + fold
    Case('wgroup_no_direct', 'wgrad', dict(M=1056, d=256, mode='group'), {'bwd': [WG, FOLD]},
         {'LTU_WGROUP_BLOCKS': 1, 'LTU_WGROUP_NO_DIRECT': 1}),
    # grouping off: one ltu_linear_wgrad per projection (ring + fold <4>)
    Case('wgroup_off', 'wgrad', dict(M=1024, d=128, mode='group'), {'bwd': [TN6, RED(4)]}, {'LTU_NO_WGROUP': 1},
         absent={'bwd': [WG]}),
    # deferred: the ring's partials folded by ltu_reduce_batch (ops.DEFER_WGRAD, the batched second stages)
    Case('wgrad_deferred_batch', 'wgrad', dict(M=2048, d=256, mode='defer'), {'bwd': [TN6, 'reduce_batch_kernel']},
         absent={'bwd': ['wgrad_reduce_kernel']}),
]

# Kernels of the token family in a profile (demangled base names).  Anchored: upconv_wgrad_ring_bf16_kernel is the conv family's.
FAMILY = re.compile(r'^(?:tail_fwd_kernel|tail_bwd_kernel|linear_ring_bf16_kernel|wgrad_group_ring_bf16_kernel|wgrad_ring_bf16_kernel'
                    r'|wgroup_fold_kernel|wgrad_reduce_kernel|linattn_|layernorm_|gelu_drop|weight_prep|reduce_parts_kernel'
                    r'|reduce_batch_kernel)')
NOT_TOKEN = {
    'wgrad_reduce_kernel<64>': 'fewer than 4 096 weight quads: first-level conv weights only (a projection has N, K >= 128)',
    'reduce_parts_kernel<8>': 'in the profiled step only InstanceNorm statistics fold 129-256 partials (the LayerNorm gradients of '
                              'the chain kernels go to reduce_batch); the token path reaches the template in case ln128_drop',
    'reduce_parts_kernel<16>': 'InstanceNorm statistics only (257-512 partials), see reduce_parts_kernel<8>',
}

# default-build instances of the chain kernels (tlayer.hip launchers; the OCC = 5 forward exists in the experiments build only)
TAIL_FWD = [tf(d, a, q) for d in (128, 256) for a in (False, True) for q in (False, True)]
TAIL_BWD = [tb(d, u, w, pre) for d, w, pre in ((256, 4, True), (256, 4, False), (128, 3, True), (128, 4, False), (128, 4, True))
            for u in (0, 1)]


def named_kernels():
    return {k for c in CASES for ks in c.kernels.values() for k in ks}


def _names(case, *directions):
    return {k for d in (directions or case.kernels) for k in case.kernels.get(d, ())}


# ---------------------------------------------------------------------------------------------- long-run geometry of the launchers

def _cdiv(a, b):
    return -(-a // b)


def _wgrad_jobs(d):
    """(N, K, nw) of a layer's four projection weight gradients: q|k|v, out, linear1, linear2"""
    return [(3 * d, d, 3), (d, d, 1), (2 * d, d, 1), (d, 2 * d, 1)]


def run_geometry(case, family, knob):
    """(32-row units per split, splits, units of the last split) of a weight-gradient ring, from its launcher's formula.
    The rings with a width knob are these two; linear_ring_bf16_kernel is persistent too, but its width (256 workgroups over the
    column tiles) has neither knob nor argument"""
    s, v = case.shape, case.knobs[knob]
    M = s['M']
    if family == 'tn_ring':              # gemm_ring.hip tn_ring_geometry
        nk, nn = s['K'] // 128, s['N'] // 128
        want = max(1, v // (nk * nn))
        rows = max(_cdiv(M, want), 128 if M <= 2048 else 256)
        rows = _cdiv(rows, 32) * 32
        n = _cdiv(M, rows)
    else:                                # gemm_ring.hip wgroup_geometry: one split count for the group
        assert family == 'wgroup'
        tiles = sum((N // 128) * (K // 128) for N, K, _ in _wgrad_jobs(s['d']))
        want = max(1, v // tiles)
        rows0 = _cdiv(max(128, _cdiv(M, want)), 32) * 32
        n = _cdiv(M, rows0)
        rows = _cdiv(_cdiv(M, n), 32) * 32
    return rows // 32, n, (M - (n - 1) * rows) // 32


def la_splits(B, N, d, total=None):
    """linattn.hip pick_splits: split count of the token reductions"""
    total = total or (256 if d >= 256 else 512)
    want = min(max(1, total // B), 256)
    tps = max(32, _cdiv(_cdiv(N, want), 32) * 32)
    return _cdiv(N, tps)


# ---------------------------------------------------------------------------------------------- CPU checks

def profile_token_kernels():
    import csv
    with open(_newest_profile()) as f:
        names = {kernel_base(r['Name']) for r in csv.DictReader(f)}
    return sorted(n for n in names if FAMILY.search(n))


def test_family_does_not_overlap_conv():
    import csv
    with open(_newest_profile()) as f:
        names = {kernel_base(r['Name']) for r in csv.DictReader(f)}
    both = [n for n in names if FAMILY.search(n) and (CONV_FAMILY.search(n) or CONV_GEMMS.search(n))]
    assert not both, both
    assert not [k for k in named_kernels() if CONV_FAMILY.search(k)], 'a token case names a conv-family kernel'


def test_table_names_every_profiled_token_kernel():
    named = named_kernels()
    prof = profile_token_kernels()
    missing = [k for k in prof if k not in named and k not in NOT_TOKEN]
    assert not missing, f'token-family kernels of {os.path.basename(_newest_profile())} without a case: {missing}'
    assert not [k for k in NOT_TOKEN if k in named], 'a kernel is both in NOT_TOKEN and named by a case'
    assert not [k for k in NOT_TOKEN if k not in prof], 'NOT_TOKEN lists a kernel the profile does not have'
    assert len({c.name for c in CASES}) == len(CASES)


def _knob(k, v=None):
    return lambda c: k in c.knobs and (v is None or c.knobs[k] == v)


def _tail(pred):
    return lambda c: c.op == 'tail' and pred(c.shape, c)


OBLIGATIONS = [(f'instance {k}', (lambda k: lambda c: k in _names(c))(k)) for k in TAIL_FWD + TAIL_BWD] + [
    (f'instance {k}', (lambda k: lambda c: k in _names(c))(k)) for k in
    ['linattn_kv_combine1<8>', 'linattn_dctx_combine<8>', 'linattn_kv_combine', 'linattn_apply_rows<128>', 'linattn_apply_rows<256>',
     la('kv_partial', 128), la('kv_partial', 256), la('dctx_partial', 128), la('dctx_partial', 256), la('bwd_apply', 128),
     la('bwd_apply', 256), ring(4, 2, 6, True), ring(4, 2, 5, True), ring(4, 1, 4, True), GELU_F, GELU_B,
     'layernorm_fwd_kernel<bf16_t, 16, 2>', 'layernorm_fwd_kernel<bf16_t, 32, 2>', 'layernorm_bwd_kernel<bf16_t, 16, 2>',
     'layernorm_bwd_kernel<bf16_t, 32, 2>', 'reduce_parts_kernel<4>']] + [
    ('chain: ragged M (last row block partly empty), forward and backward', _tail(lambda s, c: (s['B'] * s['N']) % 32 and 'bwd' in c.kernels)),
    ('chain: B > 1, N % 32 == 0, phase B inside (d = 128)', _tail(lambda s, c: s['B'] > 1 and s['attn'] and s['d'] == 128)),
    ('chain: B > 1, N % 32 == 0, phase B inside (d = 256)', _tail(lambda s, c: s['B'] > 1 and s['attn'] and s['d'] == 256)),
    ('chain: dropout 0.3, u_mode 1', _tail(lambda s, c: s['p'] == P_DROP and s['umode'] == 1)),
    ('chain: dropout 0.3, u_mode 0', _tail(lambda s, c: s['p'] == P_DROP and s['umode'] == 0)),
    ('chain: dropout 0.3 with the fused phase B and next q|k|v', _tail(lambda s, c: s['p'] == P_DROP and s['attn'] and s['nq'])),
    ('chain: second gradient of y (dy2)', _tail(lambda s, c: s['dy2'])),
    ('linattn: ragged N (phase B outside the chain kernel)', lambda c: c.op == 'linattn' and c.shape['N'] % 32),
    ('grouped weight gradient, direct mode', lambda c: c.op == 'wgrad' and FOLD in c.absent.get('bwd', ())),
    ('grouped weight gradient, fold mode', lambda c: c.op == 'wgrad' and WG in _names(c) and FOLD in _names(c) and not c.knobs.get('LTU_WGROUP_NO_DIRECT')),
    ('deferred ring + ltu_reduce_batch', lambda c: c.op == 'wgrad' and c.shape['mode'] == 'defer'),
    ('long runs: weight-gradient ring (LTU_RING_BLOCKS)', lambda c: ('tn_ring', 'LTU_RING_BLOCKS') in (c.steady or [])),
    ('long runs: grouped weight gradient (LTU_WGROUP_BLOCKS)', lambda c: ('wgroup', 'LTU_WGROUP_BLOCKS') in (c.steady or [])),
] + [(f'knob {k}', _knob(k)) for k in ('LTU_TAIL_BWD_PREU', 'LTU_TAIL_BWD_WPS', 'LTU_NO_GELU_FUSE', 'LTU_NO_NT_RING', 'LTU_LA_TWO_LEVEL',
                                       'LTU_NO_WGROUP', 'LTU_WGROUP_NO_DIRECT')]


def _all_obligations():
    return [(f'profiled: {k}', (lambda k: lambda c: k in _names(c))(k)) for k in profile_token_kernels() if k not in NOT_TOKEN] + OBLIGATIONS


def test_table_meets_every_obligation():
    unmet = [what for what, pred in _all_obligations() if not any(pred(c) for c in CASES)]
    assert not unmet, f'no case for: {unmet}'


def test_every_row_is_needed():
    """deleting any row of the table leaves a profiled kernel or an obligation without a case"""
    obl = _all_obligations()
    for c in CASES:
        only = [what for what, pred in obl if pred(c) and not any(pred(o) for o in CASES if o is not c)]
        assert only, f'{c.name}: every kernel / obligation it covers is covered by another case too'


def test_named_kernels_exist_in_sources():
    src = ''.join(open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, '*.hip'))))
    for k in sorted(named_kernels() | set(NOT_TOKEN) | set(TAIL_FWD) | set(TAIL_BWD)):
        fn = k.split('<')[0]
        assert re.search(r'__global__\s+void\s+(?:__launch_bounds__\([^()]*(?:\([^()]*\))?[^()]*\)\s+)?' + re.escape(fn) + r'\s*\(', src), \
            f'{k}: no __global__ {fn} in lintransunet_amd/csrc'
    # the chain launchers select exactly the instances TAIL_FWD / TAIL_BWD list (outside the experiments build)
    tl = open(os.path.join(CSRC, 'tlayer.hip')).read()
    tl = re.sub(r'#ifdef LTU_EXPERIMENTS.*?#endif', '', tl, flags=re.S)
    launched_fwd = {f'tail_fwd_kernel<{m.group(1)}>' for m in re.finditer(r'launch\(&tail_fwd_kernel<([^>]*)>', tl)}
    launched_bwd = {f'tail_bwd_kernel<{m.group(1)}>' for m in re.finditer(r'launch\(&tail_bwd_kernel<([^>]*)>', tl)}
    assert launched_fwd == set(TAIL_FWD) and launched_bwd == set(TAIL_BWD), (launched_fwd ^ set(TAIL_FWD), launched_bwd ^ set(TAIL_BWD))


def test_steady_state_geometry():
    """every long-run case: at least 8 units of 32 rows per split, a shorter last split"""
    steady = [c for c in CASES if c.steady]
    assert steady
    for c in steady:
        for family, knob in c.steady:
            per, n, last = run_geometry(c, family, knob)
            assert per >= 8 and 0 < last < per and n >= 2, (c.name, family, per, n, last)


def test_linattn_split_counts():
    """the split counts the linattn cases' comments promise, from pick_splits"""
    want = {'la128_ragged': 32, 'la256_splits8': 50, 'la128_splits16': 79, 'la256_splits32': 188, 'la128_two_level': 79}
    for c in CASES:
        if c.op == 'linattn':
            s = c.shape
            assert la_splits(s['B'], s['N'], s['d'], c.knobs.get('LTU_LA_SPLITS')) == want[c.name], c.name
    for c in CASES:
        for k in _names(c):
            m = re.match(r'linattn_(?:kv_combine1|dctx_combine)<(\d+)>', k)
            if m:
                s = c.shape
                ns = la_splits(s['B'], s['N'], s['d'], c.knobs.get('LTU_LA_SPLITS'))
                nb = int(m.group(1))
                assert ns <= 32 * nb // 4 and (nb == 4 or ns > 32 * nb // 8), (c.name, k, ns)


# ---------------------------------------------------------------------------------------------- float64 references

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bf(t):
    return t.bfloat16().double()


def _f32(t):
    return t.float().double()


def rounded(x, mag):
    """bf16 rounding of an fp32 value the kernel does not store, emulated on its float64 value x: (the rounded value, slack).
    slack is one bf16 ulp where x lies within RISK * mag of a rounding midpoint (the kernel's fp32 value may round the other way)"""
    xb = x.float().bfloat16().double()
    ulp = torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(1e-30))) - 7)
    near = (ulp / 2 - (x - xb).abs()) <= RISK * mag
    return xb, torch.where(near, ulp, torch.zeros_like(ulp))


def _gelu(u):
    return u * 0.5 * (1 + torch.erf(u / math.sqrt(2)))


def _gelu_grad(u):
    return 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-u * u / 2) / math.sqrt(2 * math.pi)


GELU_SLOPE, GELU_CURV = 1.13, 0.8        # max |gelu'| and |gelu''| (at +-1.4 / 0): what one ulp of u moves gelu(u) / gelu'(u) by


def _ln_stats(z):
    mu = z.mean(1, keepdim=True)
    return mu, 1 / torch.sqrt(((z - mu) ** 2).mean(1, keepdim=True) + LN_EPS)


def _ln_bwd(g, zn, rs, gamma):
    gg = g * gamma
    return rs * (gg - gg.mean(1, keepdim=True) - zn * (gg * zn).mean(1, keepdim=True))


class Checker:
    """collects worst error / bound per output; failures are gathered so that one case reports all of its outputs"""

    def __init__(self):
        self.ratio, self.fails = {}, []

    def _put(self, what, worst, msg=None):
        self.ratio[what] = max(self.ratio.get(what, 0.0), worst)
        if msg:
            self.fails.append(msg)

    def bf16(self, what, got, ref, extra=None, rows=None):
        """element-wise bound of a bf16-stored [M, n] tensor; extra: the named slack / rounding terms (float64, like ref)"""
        got = got.double().cpu()
        if rows is not None:
            got = got[:rows]
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        if not torch.isfinite(got).all():
            return self._put(what, math.inf, f'{what}: non-finite values')
        bound = BF16_REL * ref.abs() + BF16_ABS * ref.abs().max()
        if extra is not None:
            bound = bound + extra
        ratio = (got - ref).abs() / bound.clamp_min(1e-30)
        worst = ratio.max().item()
        msg = None
        if worst > 1.0:
            i = int(ratio.argmax())
            r, c = divmod(i, ratio.shape[1])
            msg = (f'{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements out of bound; worst at row {r} (block {r // 32}), '
                   f'column {c} (head {c // 32}): got {got[r, c].item():.6g}, ref {ref[r, c].item():.6g}, {worst:.2f} x the bound')
        self._put(what, worst, msg)

    def f32(self, what, got, ref, mag, rel=F32_REL, extra=None):
        """element-wise: |got - ref| <= rel * mag (+ extra): fp32 statistics and contexts against the magnitude of their sums"""
        got = got.double().cpu().reshape(ref.shape)
        if not torch.isfinite(got).all():
            return self._put(what, math.inf, f'{what}: non-finite values')
        bound = rel * mag + (extra if extra is not None else 0)
        ratio = (got - ref).abs() / bound.clamp_min(1e-30)
        worst = ratio.max().item()
        msg = None
        if worst > 1.0:
            i = int(ratio.argmax())
            msg = (f'{what}: {int((ratio > 1).sum())} elements out of bound; worst at flat index {i} of {tuple(ref.shape)}: got '
                   f'{got.reshape(-1)[i].item():.8g}, ref {ref.reshape(-1)[i].item():.8g}, {worst:.2f} x the bound')
        self._put(what, worst, msg)

    def grad(self, what, got, ref, extra=None):
        """fp32 gradients: max|got - ref| / max|ref| <= WGRAD_TOL; extra: the named slack of an unstored rounded operand (element-wise)"""
        got = got.double().cpu().reshape(ref.shape)
        if not torch.isfinite(got).all():
            return self._put(what, math.inf, f'{what}: non-finite values')
        mx = max(ref.abs().max().item(), 1e-30)
        if extra is None:
            err = (got - ref).abs().max().item() / mx
            return self._put(what, err / WGRAD_TOL, f'{what}: max|err| / max|ref| = {err:.3g} > {WGRAD_TOL}' if err > WGRAD_TOL else None)
        worst = ((got - ref).abs() / (WGRAD_TOL * mx + extra.reshape(ref.shape))).max().item()
        self._put(what, worst, f'{what}: {worst:.2f} x the bound (1e-4 max|ref| + slack)' if worst > 1 else None)

    def untouched(self, what, t, rows):
        """rows past M of an over-allocated output keep their NaN fill"""
        tail = t[rows:]
        if tail.numel() and not torch.isnan(tail.float()).all():
            self.fails.append(f'{what}: rows past M were written')


def _mask(M, width, p, seed):
    """dropout mask {0, 1/(1-p)} of an [M, width] site, from the stand-alone kernel that shares the chain kernels' counter hash"""
    from lintransunet_amd import ops
    if p == 0:
        return torch.ones(M, width, dtype=torch.float64)
    with ops.use(ops.Context()):
        u = torch.full((M, width), 8.0, device=DEV, dtype=torch.float32)       # gelu(8) == 8 in fp32
        m = (ops.gelu_dropout(u, p, seed) / 8.0).cpu()
    vals = torch.unique(m)
    assert vals.numel() == 2 and vals[0].item() == 0.0 and abs(vals[1].item() - 1 / (1 - p)) < 1e-6, vals
    return (m > 0).double() / (1 - p)


def _dev(t, dtype=torch.bfloat16):
    return t.to(DEV, dtype).contiguous()


def _nan(shape, dtype=torch.bfloat16):
    return torch.full(shape, float('nan'), device=DEV, dtype=dtype)


def _call(name, *args):
    from lintransunet_amd import _lib
    _lib.call(name, *args)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- linear attention, per stage

def _heads(t, B, N, H):
    """[B*N, H*32] -> [B, H, N, 32]"""
    return t.reshape(B, N, H, 32).permute(0, 2, 1, 3)


def _unheads(t):
    B, H, N, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * N, H * 32)


def check_ctx(ck, qkv, B, N, d, cx, colstats, tag=''):
    """phase A (kv_partial + merge): column max (exact), column sum and context against float64 on the same bf16 k, v.
    The exponentials are rounded to bf16 before the context product (linattn.hip:223, pack8(pe)): + 2^-8 P^T|v|"""
    from oracle import net as O_net
    H = d // 32
    k, v = _heads(qkv[:, d:2 * d], B, N, H), _heads(qkv[:, 2 * d:], B, N, H)
    cm = k.max(2).values                                           # [B, H, 32]
    e = torch.exp(k - cm[:, :, None, :])
    cs = e.sum(2)
    P = e / cs[:, :, None, :]
    ctx = torch.einsum('bhni,bhnj->bhij', P, v)
    mag = torch.einsum('bhni,bhnj->bhij', P, v.abs())
    # the stage formula is the oracle's (model/trans_block.py:41-67): its float64 output is the product of this context with qs
    q = _heads(qkv[:, :d], B, N, H)
    qs = torch.softmax(q, -1) / math.sqrt(32)
    assert torch.allclose(O_net.linear_attention(q, k, v), torch.einsum('bhni,bhij->bhnj', qs, ctx), rtol=1e-10, atol=1e-12)
    st = colstats.double().cpu().reshape(B, H, 64)
    if not torch.equal(st[..., :32], cm):
        ck.fails.append(f'{tag}colmax: differs from the max of the bf16 keys (exact)')
    ck.f32(f'{tag}colsum', st[..., 32:], cs, cs)
    ck.f32(f'{tag}ctx', cx, ctx, mag, extra=BF16_REL * mag)
    return cm, cs


def apply_ref(q, ctx_got):
    """phase B on the stored fp32 context: qs = softmax(q) / sqrt(32) rounded to bf16 (linattn.hip:632, tlayer.hip:304), the context
    rounded to bf16 (linattn.hip:580, tlayer.hip:282; exact emulation of the stored fp32 value); returns (ref, slack term, mx, inv)"""
    mx = q.max(-1, keepdim=True).values
    e = torch.exp(q - mx)
    inv = 1 / (e.sum(-1, keepdim=True) * math.sqrt(32))
    qs = e * inv
    qsb, sl = rounded(qs, qs)
    cb = _bf(ctx_got)
    return torch.einsum('bhni,bhij->bhnj', qsb, cb), torch.einsum('bhni,bhij->bhnj', sl, cb.abs()), mx, inv


def check_apply(ck, qkv, B, N, d, cx, out, qstat, tag=''):
    H = d // 32
    q = _heads(qkv[:, :d], B, N, H)
    ref, sl, mx, inv = apply_ref(q, cx.double().cpu().reshape(B, H, 32, 32))
    ck.bf16(f'{tag}attn_out', out, _unheads(ref), extra=_unheads(sl), rows=B * N)
    qs_ = qstat.double().cpu()[:B * N].reshape(B, N, H, 2).permute(0, 2, 1, 3)
    if not torch.equal(qs_[..., :1], mx):
        ck.fails.append(f'{tag}qstat row max: differs from the max of the bf16 q row (exact)')
    ck.f32(f'{tag}qstat inv', qs_[..., 1:], inv, inv)


def check_linattn_bwd(ck, qkv, dout, B, N, d, cx, colstats, qstat, dctx, dqkv):
    """dctx_partial + combine, then linattn_bwd_apply, each on the stored inputs of its stage"""
    H = d // 32
    q, k, v = (_heads(qkv[:, i * d:(i + 1) * d], B, N, H) for i in range(3))
    g = _heads(dout, B, N, H)
    st = qstat.double().cpu().reshape(B, N, H, 2).permute(0, 2, 1, 3)
    qs = torch.exp(q - st[..., :1]) * st[..., 1:]                   # from the stored row statistics, as dctx_partial does
    # dctx = qs^T dout, qs rounded to bf16 (linattn.hip:723 / :763, pack8(qe))
    qsb, sl = rounded(qs, qs)
    ref = torch.einsum('bhni,bhnj->bhij', qsb, g)
    mag = torch.einsum('bhni,bhnj->bhij', qsb, g.abs())
    ck.f32('dctx', dctx, ref, mag, extra=torch.einsum('bhni,bhnj->bhij', sl, g.abs()))
    dc = dctx.double().cpu().reshape(B, H, 32, 32)
    ctx = cx.double().cpu().reshape(B, H, 32, 32)
    tv = (dc * ctx).sum(-1)              # the Jacobian term, formed from the stored fp32 values in LDS (linattn.hip:855-860)
    cs = colstats.double().cpu().reshape(B, H, 64)
    P = torch.exp(k - cs[:, :, None, :32]) / cs[:, :, None, 32:]
    # dv = P dctx: both operands rounded to bf16 (linattn.hip:933-934 kk, :862 dcTB; the stored fp32 dctx emulated exactly)
    Pb, slp = rounded(P, P)
    dcb = _bf(dc)
    dv = torch.einsum('bhni,bhij->bhnj', Pb, dcb)
    dv_sl = torch.einsum('bhni,bhij->bhnj', slp, dcb.abs())
    # dk = P (dP - tvec), dP = v dctx^T from a three-way bf16 split of dctx (linattn.hip:871-875: fp32-exact); the difference cancels
    # to ~1e-3 of its terms: fp32 noise 1e-5 of P (|v| |dctx|^T + |tvec|)
    dP = torch.einsum('bhnj,bhij->bhni', v, dc)
    dk = P * (dP - tv[:, :, None, :])
    dk_noise = F32_REL * P * (torch.einsum('bhnj,bhij->bhni', v.abs(), dc.abs()) + tv.abs()[:, :, None, :])
    # dq = qs (dqs - sum_i p_i dqs_i), dqs = dout ctx^T with ctx rounded to bf16 (linattn.hip:862 ctxB); fp32 noise of the difference
    cb = _bf(ctx)
    dqs = torch.einsum('bhnj,bhij->bhni', g, cb)
    p = qs * math.sqrt(32)
    dq = qs * (dqs - (p * dqs).sum(-1, keepdim=True))
    dq_noise = F32_REL * qs * (torch.einsum('bhnj,bhij->bhni', g.abs(), cb.abs()) * 2)
    got = dqkv.double().cpu()[:B * N]
    ck.bf16('dq', got[:, :d], _unheads(dq), extra=_unheads(dq_noise))
    ck.bf16('dk', got[:, d:2 * d], _unheads(dk), extra=_unheads(dk_noise))
    ck.bf16('dv', got[:, 2 * d:], _unheads(dv), extra=_unheads(dv_sl))


# ---- the chain kernels, per stage

def _tail_params(d, seed, nq):
    g = _gen(seed)
    P = {'wo': _bf(torch.randn(d, d, generator=g) / math.sqrt(d)), 'w1': _bf(torch.randn(2 * d, d, generator=g) / math.sqrt(d)),
         'w2': _bf(torch.randn(d, 2 * d, generator=g) / math.sqrt(2 * d))}
    for k, n in (('bo', d), ('b1', 2 * d), ('b2', d), ('be1', d), ('be2', d)):
        P[k] = _f32(0.1 * torch.randn(n, generator=g))
    P['g1'], P['g2'] = (_f32(1 + 0.2 * torch.randn(d, generator=g)) for _ in range(2))
    if nq:
        P['wq'] = [_bf(torch.randn(d, d, generator=g) / math.sqrt(d)) for _ in range(3)]
        P['bq'] = [_f32(0.1 * torch.randn(d, generator=g)) for _ in range(3)]
    return P


def _proj_ref(A, W, b):
    """A W^T + b and the magnitude |A| |W|^T + |b| of the fp32 sum"""
    return A @ W.T + b, A.abs() @ W.abs().T + b.abs()


def check_ln_fwd(ck, tag, z, sl, got_z, stat, got_y, gamma, beta, M):
    """a LayerNorm stage on the kernel's unrounded fp32 sum z (float64 emulation, `sl` its propagated slack): z stored as bf16, the
    statistics against z (their slack: mean |sl| and mean |z - mu| |sl| / var), y from z and the STORED statistics"""
    ck.bf16(f'{tag}.z', got_z, z, extra=sl, rows=M)
    mu, rs = _ln_stats(z)
    st = stat.double().cpu()[:M]
    var = 1 / rs ** 2
    ck.f32(f'{tag}.mean', st[:, :1], mu, (z - mu).abs().mean(1, keepdim=True) + mu.abs(), extra=sl.mean(1, keepdim=True))
    ck.f32(f'{tag}.rstd', st[:, 1:], rs, rs, extra=rs * ((z - mu).abs() * sl).mean(1, keepdim=True) / var)
    mg, rg = st[:, :1], st[:, 1:]
    y = (z - mg) * rg * gamma + beta
    ck.bf16(f'{tag}.y', got_y, y, extra=sl * rg * gamma.abs(), rows=M)


def run_tail(case, ck):
    from lintransunet_amd import ops
    from lintransunet_amd.model import _WeightStore
    s = case.shape
    B, N, d, p, umode = s['B'], s['N'], s['d'], s['p'], s['umode']
    M, H = B * N, d // 32
    P = _tail_params(d, sum(map(ord, case.name)), s['nq'])
    g = _gen(sum(map(ord, case.name)) + 1)
    x = _bf(torch.randn(M, d, generator=g))
    x = _bf(x + 1.5 * (torch.arange(M) < M // 7).double()[:, None])  # not centred: LayerNorm means matter
    a_in = _bf(torch.randn(M, d, generator=g))
    qkv_in = _bf(torch.randn(M, 3 * d, generator=g) * 1.5)
    dy = _bf(torch.randn(M, d, generator=g))
    dy2 = _bf(torch.randn(M, d, generator=g)) if s['dy2'] else None
    seeds = (11 + sum(map(ord, case.name)), 22, 33)
    seen = {}
    st = _WeightStore(torch.device(DEV, torch.cuda.current_device()), torch.bfloat16)
    masters = {k: _dev(P[k], torch.float32) for k in ('wo', 'w1', 'w2')}
    for k in ('wo', 'w1', 'w2'):
        st.add_linear(k, [masters[k]], frag=True)
    if s['nq']:
        wq = [_dev(w, torch.float32) for w in P['wq']]
        st.add_linear('q', wq, frag=True)
    st.finalize()
    _, seen['prep'] = launched(st.refresh)
    lin = st.lin
    par = {k: _dev(P[k], torch.float32) for k in ('bo', 'b1', 'b2', 'g1', 'be1', 'g2', 'be2')}
    bq = [_dev(b, torch.float32) for b in P['bq']] if s['nq'] else [None] * 3
    # outputs over-allocated by one row block and NaN-filled: rows past M must stay untouched
    Mp = M + 32
    z1, t1, z2, y = (_nan((Mp, d)) for _ in range(4))
    u, h = _nan((Mp, 2 * d)), _nan((Mp, 2 * d))
    stat1, stat2 = _nan((Mp, 2), torch.float32), _nan((Mp, 2), torch.float32)
    qn = _nan((Mp, 3 * d)) if s['nq'] else None
    xg = _dev(x)
    qkv = cx = colstats = qstat = ws = None
    if s['attn']:
        qkv = _dev(qkv_in)
        cx = torch.empty((B * H, 32, 32), device=DEV, dtype=torch.float32)
        colstats = torch.empty((B * H, 64), device=DEV, dtype=torch.float32)
        qstat = _nan((Mp, H, 2), torch.float32)
        ws = torch.empty(ops._lib.load().ltu_linattn_ws_floats(B, N, d), device=DEV, dtype=torch.float32)
        a = _nan((Mp, d))
    else:
        a = _dev(a_in)

    def fwd():
        if s['attn']:
            _call('ltu_linattn_ctx', _ptr(qkv), _ptr(cx), _ptr(colstats), _ptr(ws), ws.numel(), B, N, d, ops.BF16, _stream())
        _call('ltu_layer_tail_fwd', _ptr(a), _ptr(xg), _ptr(lin['wo'].frag), _ptr(lin['w1'].frag), _ptr(lin['w2'].frag),
              _ptr(par['bo']), _ptr(par['b1']), _ptr(par['b2']), _ptr(par['g1']), _ptr(par['be1']), _ptr(par['g2']), _ptr(par['be2']),
              _ptr(z1), _ptr(t1), _ptr(u), _ptr(h), _ptr(z2), _ptr(y), _ptr(stat1), _ptr(stat2), M, d, LN_EPS, float(p),
              seeds[0], seeds[1], seeds[2], 0, umode, _ptr(qkv), _ptr(cx), _ptr(qstat), N if s['attn'] else 0,
              _ptr(lin['q'].frag) if s['nq'] else 0, _ptr(bq[0]), _ptr(bq[1]), _ptr(bq[2]), _ptr(qn), ops.BF16, _stream())
    _, seen['fwd'] = launched(fwd)
    # backward on the stored forward tensors
    dr2, dr1_g, dz1_g, da_g = (_nan((Mp, d)) for _ in range(4))
    du = _nan((Mp, 2 * d))
    nblk = ops._lib.load().ltu_layer_tail_blocks(M)
    lnws = _nan((2, nblk, 2 * d), torch.float32)
    dyg, dy2g = _dev(dy), (_dev(dy2) if dy2 is not None else None)

    def bwd():
        _call('ltu_layer_tail_bwd', _ptr(dyg), _ptr(dy2g), _ptr(z2), _ptr(z1), _ptr(u), _ptr(stat2), _ptr(stat1), _ptr(par['g2']),
              _ptr(par['g1']), _ptr(lin['w2'].fragT), _ptr(lin['w1'].fragT), _ptr(lin['wo'].fragT), _ptr(dr2), _ptr(du), _ptr(dr1_g),
              _ptr(dz1_g), _ptr(da_g), _ptr(lnws[0]), _ptr(lnws[1]), nblk * 2 * d, M, d, float(p), seeds[0], seeds[1], seeds[2], 0,
              umode, ops.BF16, _stream())
    _, seen['bwd'] = launched(bwd)
    torch.cuda.synchronize()
    m1, mg, m2 = _mask(M, d, p, seeds[0]), _mask(M, 2 * d, p, seeds[1]), _mask(M, d, p, seeds[2])
    G = lambda t: t.double().cpu()[:M]                               # noqa: E731
    for what, t in (('z1', z1), ('t1', t1), ('u', u), ('h', h), ('z2', z2), ('y', y), ('stat1', stat1), ('stat2', stat2), ('dr2', dr2),
                    ('du', du), ('dr1', dr1_g), ('dz1', dz1_g), ('da', da_g)) + ((('qkv_next', qn),) if s['nq'] else ()) + \
            ((('a', a), ('qstat', qstat)) if s['attn'] else ()):
        ck.untouched(what, t, M)

    # -- forward, stage by stage
    if s['attn']:
        check_ctx(ck, qkv_in, B, N, d, cx, colstats)
        check_apply(ck, qkv_in, B, N, d, cx, a, qstat)
    A = G(a)
    o, omag = _proj_ref(A, P['wo'], P['bo'])
    ob, osl = rounded(o, omag)                                       # out projection rounded to bf16 in LDS (tlayer.hip:335)
    check_ln_fwd(ck, 'ln1', x + m1 * ob, m1 * osl, z1, stat1, t1, P['g1'], P['be1'], M)
    T1 = G(t1)
    uu, umag = _proj_ref(T1, P['w1'], P['b1'])
    if umode == 0:
        ck.bf16('u', u, uu, rows=M)                                  # stored as rounded (tlayer.hip:353 -> :395)
        U = G(u)
        ck.bf16('h', h, _gelu(U) * mg, rows=M)
    else:
        # u is rounded in LDS (tlayer.hip:353) and not stored: the buffer holds mask * gelu'(u) (tlayer.hip:381, :386-388)
        ub, usl = rounded(uu, umag)
        ck.bf16('u_factor', u, mg * _gelu_grad(ub), extra=mg * GELU_CURV * usl, rows=M)
        ck.bf16('h', h, _gelu(ub) * mg, extra=mg * GELU_SLOPE * usl, rows=M)
    f, fmag = _proj_ref(G(h), P['w2'], P['b2'])
    fb, fsl = rounded(f, fmag)                                       # linear2 rounded to bf16 in LDS (tlayer.hip:408)
    check_ln_fwd(ck, 'ln2', T1 + m2 * fb, m2 * fsl, z2, stat2, y, P['g2'], P['be2'], M)
    if s['nq']:
        Y = G(y)
        ref = torch.cat([Y @ w.T + b for w, b in zip(P['wq'], P['bq'])], 1)
        ck.bf16('qkv_next', qn, ref, rows=M)                         # rounded once (tlayer.hip:431)

    # -- backward, stage by stage
    gy = dy + (dy2 if dy2 is not None else 0)
    Z2, S2, Z1, S1 = G(z2), G(stat2), G(z1), G(stat1)
    zn2 = (Z2 - S2[:, :1]) * S2[:, 1:]
    dz2 = _ln_bwd(gy, zn2, S2[:, 1:], P['g2'])
    ck.bf16('dr2', dr2, m2 * dz2, rows=M)
    lw = lnws.double().cpu()
    rowsum = lambda t: torch.nn.functional.pad(t, (0, 0, 0, nblk * 32 - M)).reshape(nblk, 32, -1).sum(1)      # noqa: E731
    ref2 = torch.stack([rowsum(gy * zn2), rowsum(gy)], -1).reshape(nblk, 2 * d)
    ck.grad('lnws2', lw[0], ref2)
    dh, dhmag = _proj_ref(G(dr2), P['w2'].T, torch.zeros(1, dtype=torch.float64))
    dhb, dhsl = rounded(dh, dhmag)                                   # dh rounded to bf16 in LDS (tlayer.hip:628)
    if umode == 1:
        F_ = G(u)
        ck.bf16('du', du, dhb * F_, extra=dhsl * F_.abs(), rows=M)
    else:
        gp = mg * _gelu_grad(G(u))
        ck.bf16('du', du, dhb * gp, extra=dhsl * gp.abs(), rows=M)
    dt1, dtmag = _proj_ref(G(du), P['w1'].T, torch.zeros(1, dtype=torch.float64))
    dtb, dtsl = rounded(dt1, dtmag)                                  # dt1 rounded to bf16 in LDS (tlayer.hip:666)
    # dz2 reaches LayerNorm 1 rounded to bf16 through LDS (tlayer.hip:551, :555): its fp32 value cancels, magnitude = its terms
    gg2 = gy * P['g2']
    dz2mag = S2[:, 1:] * (gg2.abs() + gg2.mean(1, keepdim=True).abs() + zn2.abs() * (gg2 * zn2).mean(1, keepdim=True).abs())
    dz2b, dz2sl = rounded(dz2, dz2mag)
    zn1 = (Z1 - S1[:, :1]) * S1[:, 1:]
    gsum = dtb + dz2b
    dz1 = _ln_bwd(gsum, zn1, S1[:, 1:], P['g1'])
    A_ = (dtsl + dz2sl) * P['g1'].abs()                             # slack of the LayerNorm-1 input through its backward
    sl1 = S1[:, 1:] * (A_ + A_.mean(1, keepdim=True) + zn1.abs() * (A_ * zn1.abs()).mean(1, keepdim=True))
    ck.bf16('dz1', dz1_g, dz1, extra=sl1, rows=M)
    ck.bf16('dr1', dr1_g, m1 * dz1, extra=m1 * sl1, rows=M)
    # LayerNorm-1 column sums per row block: + 2^-8 of the summed magnitudes of the rounded input (slack where it may round away)
    ref1 = torch.stack([rowsum(gsum * zn1), rowsum(gsum)], -1).reshape(nblk, 2 * d)
    sl = dtsl + dz2sl
    ext1 = torch.stack([rowsum(sl * zn1.abs()), rowsum(sl)], -1).reshape(nblk, 2 * d)
    ck.f32('lnws1', lw[1], ref1, ref1.abs().max().expand_as(ref1), rel=WGRAD_TOL, extra=ext1)
    ck.bf16('da', da_g, G(dr1_g) @ P['wo'], rows=M)                  # rounded once (tlayer.hip:678)
    return seen


def run_linattn(case, ck):
    from lintransunet_amd import ops
    s = case.shape
    B, N, d = s['B'], s['N'], s['d']
    M, H = B * N, d // 32
    g = _gen(sum(map(ord, case.name)))
    qkv_in = _bf(torch.randn(M, 3 * d, generator=g) * 1.5)
    dout = _bf(torch.randn(M, d, generator=g))
    qkv, gout = _dev(qkv_in), _dev(dout)
    out, dqkv = _nan((M, d)), _nan((M, 3 * d))
    cx, dctx = (_nan((B * H, 32, 32), torch.float32) for _ in range(2))
    colstats, qstat = _nan((B * H, 64), torch.float32), _nan((M, H, 2), torch.float32)
    n = ops._lib.load().ltu_linattn_ws_floats(B, N, d)
    ws = torch.empty(n, device=DEV, dtype=torch.float32)
    seen = {}
    _, seen['fwd'] = launched(lambda: _call('ltu_linattn_fwd', _ptr(qkv), _ptr(out), _ptr(cx), _ptr(colstats), _ptr(qstat), _ptr(ws), n,
                                            B, N, d, ops.BF16, _stream()))
    _, seen['bwd'] = launched(lambda: _call('ltu_linattn_bwd', _ptr(qkv), _ptr(gout), _ptr(cx), _ptr(colstats), _ptr(qstat), _ptr(dqkv),
                                            _ptr(dctx), 0, _ptr(ws), n, B, N, d, ops.BF16, _stream()))
    torch.cuda.synchronize()
    check_ctx(ck, qkv_in, B, N, d, cx, colstats)
    check_apply(ck, qkv_in, B, N, d, cx, out, qstat)
    check_linattn_bwd(ck, qkv_in, dout, B, N, d, cx, colstats, qstat, dctx, dqkv)
    return seen


def _linear_operands(case, nw, N, K):
    g = _gen(sum(map(ord, case.name)))
    W = [_bf(torch.randn(N // nw, K, generator=g) / math.sqrt(K)) for _ in range(nw)]
    b = [_f32(0.1 * torch.randn(N // nw, generator=g)) for _ in range(nw)]
    return g, W, b


def _store(key, ws):
    from lintransunet_amd.model import _WeightStore
    st = _WeightStore(torch.device(DEV, torch.cuda.current_device()), torch.bfloat16)
    st.add_linear(key, ws)
    st.finalize()
    st.refresh()
    return st.lin[key]


def run_linear(case, ck):
    """ops.linear with prepared operands; the fp32 weight / bias gradients of the plain (non-fused) autograd path"""
    from lintransunet_amd import ops
    s = case.shape
    M, K, N, nw = s['M'], s['K'], s['N'], s['nw']
    g, W, b = _linear_operands(case, nw, N, K)
    x, go = _bf(torch.randn(M, K, generator=g)), _bf(torch.randn(M, N, generator=g))
    wp = [_dev(w, torch.float32).requires_grad_(True) for w in W]
    bp = [_dev(v, torch.float32).requires_grad_(True) for v in b]
    prep = _store('l', wp)
    xg = _dev(x).requires_grad_(True)
    seen = {}
    with ops.use(ops.Context()):
        y, seen['fwd'] = launched(lambda: ops.linear(xg, wp, bp, prep=prep))
        _, seen['bwd'] = launched(lambda: y.backward(_dev(go)))
    torch.cuda.synchronize()
    Wc, bc = torch.cat(W), torch.cat(b)
    ck.bf16('y', y, x @ Wc.T + bc)
    ck.bf16('dx', xg.grad, go @ Wc)
    Ns = N // nw
    for i in range(nw):
        ck.grad(f'dw{i}', wp[i].grad, go[:, i * Ns:(i + 1) * Ns].T @ x)
        ck.grad(f'db{i}', bp[i].grad, go[:, i * Ns:(i + 1) * Ns].sum(0))
    return seen


def run_linear_gelu(case, ck):
    """h = dropout(gelu(x W^T + b)): u (stored) against float64, h from the stored u; backward: the GELU / dropout gradient g is
    rounded to bf16 and not kept (ops._LinearGelu.backward): emulated, with its slack"""
    from lintransunet_amd import ops
    s = case.shape
    M, K, N, p = s['M'], s['K'], s['N'], s['p']
    g, (W,), (b,) = _linear_operands(case, 1, N, K)
    x, gh = _bf(torch.randn(M, K, generator=g)), _bf(torch.randn(M, N, generator=g))
    wp, bp = _dev(W, torch.float32).requires_grad_(True), _dev(b, torch.float32).requires_grad_(True)
    prep = _store('l', [wp])
    xg = _dev(x).requires_grad_(True)
    seed = 1000 + sum(map(ord, case.name))
    seen = {}
    with ops.use(ops.Context()):
        h, seen['fwd'] = launched(lambda: ops.linear_gelu(xg, wp, bp, p, seed, prep=prep))
        u = h.grad_fn.saved_tensors[1].double().cpu()
        _, seen['bwd'] = launched(lambda: h.backward(_dev(gh)))
    torch.cuda.synchronize()
    m = _mask(M, N, p, seed)
    ck.bf16('u', u, x @ W.T + b)
    ck.bf16('h', h, _gelu(u) * m)
    g64 = gh * m * _gelu_grad(u)
    gb, gsl = rounded(g64, g64.abs())
    ck.bf16('dx', xg.grad, gb @ W, extra=gsl @ W.abs())
    ck.grad('dw', wp.grad, gb.T @ x, extra=gsl.T @ x.abs())
    ck.grad('db', bp.grad, gb.sum(0), extra=gsl.sum(0))
    return seen


def run_ln(case, ck):
    """ops.res_layernorm: z = x + dropout(r) (stored in r's buffer), y = LN(z) from the unrounded fp32 z; backward on the stored z"""
    from lintransunet_amd import ops
    s = case.shape
    M, d, p = s['M'], s['d'], s['p']
    g = _gen(sum(map(ord, case.name)))
    x, r = _bf(torch.randn(M, d, generator=g)), _bf(torch.randn(M, d, generator=g))
    x = _bf(x + 2.0 * (torch.arange(M) < M // 5).double()[:, None])
    gamma, beta = _f32(1 + 0.2 * torch.randn(d, generator=g)), _f32(0.1 * torch.randn(d, generator=g))
    gy = [_bf(torch.randn(M, d, generator=g)) for _ in range(2 if s['dy2'] else 1)]
    xg, rg = _dev(x).requires_grad_(True), _dev(r).requires_grad_(True)
    gp, bp = _dev(gamma, torch.float32).requires_grad_(True), _dev(beta, torch.float32).requires_grad_(True)
    seed = 2000 + sum(map(ord, case.name))
    seen = {}
    with ops.use(ops.Context()):
        y, seen['fwd'] = launched(lambda: ops.res_layernorm(xg, rg, gp, bp, LN_EPS, p, seed, fork=s['dy2']))
        ys = y if s['dy2'] else (y,)
        z, stat = (t.double().cpu() for t in ys[0].grad_fn.saved_tensors)
        _, seen['bwd'] = launched(lambda: torch.autograd.backward(list(ys), [_dev(t) for t in gy]))
    torch.cuda.synchronize()
    m = _mask(M, d, p, seed)
    check_ln_fwd(ck, 'ln', x + m * r, torch.zeros(M, d, dtype=torch.float64), z, stat, ys[0], gamma, beta, M)
    G = sum(gy)
    zn = (z - stat[:, :1]) * stat[:, 1:]
    dz = _ln_bwd(G, zn, stat[:, 1:], gamma)
    ck.bf16('dz', xg.grad, dz)
    ck.bf16('dr', rg.grad, m * dz)
    ck.grad('dgamma', gp.grad, (G * zn).sum(0))
    ck.grad('dbeta', bp.grad, G.sum(0))
    return seen


def run_wgrad(case, ck):
    """a layer's four projection weight gradients on random operands, added to random existing gradients (the kernels accumulate):
    grouped (ops.Context._wgrad_group_launch, as a layer's flush point issues them) or deferred (ltu_linear_wgrad with a job, then
    ltu_reduce_batch, as ops.Context._fold_flush issues them)"""
    from lintransunet_amd import _lib, ops
    s = case.shape
    M, d = s['M'], s['d']
    g = _gen(sum(map(ord, case.name)))
    jobs, refs = [], []
    for N, K, nw in _wgrad_jobs(d):
        go, x = _bf(torch.randn(M, N, generator=g)), _bf(torch.randn(M, K, generator=g))
        Ns = N // nw
        w0 = [_f32(torch.randn(Ns, K, generator=g)) for _ in range(nw)]
        b0 = [_f32(torch.randn(Ns, generator=g)) for _ in range(nw)]
        dws, dbs = [_dev(t, torch.float32) for t in w0], [_dev(t, torch.float32) for t in b0]
        jobs.append((_dev(go), _dev(x), dws, dbs, M, N, K))
        refs.append([(go[:, i * Ns:(i + 1) * Ns].T @ x, go[:, i * Ns:(i + 1) * Ns].sum(0), w0[i], b0[i]) for i in range(nw)])
    keep = []
    if s['mode'] == 'group':
        _, seen = launched(lambda: ops.Context()._wgrad_group_launch(jobs, keep))
    else:
        arr = (_lib.ReduceJob * len(jobs))()

        def run():
            for j, (go, x, dws, dbs, M_, N, K) in zip(arr, jobs):
                ws = torch.empty(_lib.load().ltu_wgrad_ws_floats(M_, N, K), device=DEV, dtype=torch.float32)
                keep.append(ws)
                _call('ltu_linear_wgrad', _ptr(go), N, _ptr(x), K, ops._ptr_array(dws), ops._ptr_array(dbs), len(dws), M_, N, K, _ptr(ws),
                      ws.numel(), ctypes.addressof(j), ops.BF16, _stream())
                assert j.part, 'the ring declined the deferred weight gradient'
            _call('ltu_reduce_batch', ctypes.addressof(arr), len(jobs), _stream())
        _, seen = launched(run)
    torch.cuda.synchronize()
    for (_, _, dws, dbs, *_), rr, (N, K, nw) in zip(jobs, refs, _wgrad_jobs(d)):
        for i, (dw, db, w0, b0) in enumerate(rr):
            ck.grad(f'dw[{N}x{K}].{i}', dws[i].double().cpu() - w0, dw)
            ck.grad(f'db[{N}x{K}].{i}', dbs[i].double().cpu() - b0, db)
    return {'bwd': seen}


RUNNERS = {'tail': run_tail, 'linattn': run_linattn, 'linear': run_linear, 'linear_gelu': run_linear_gelu, 'ln': run_ln,
           'wgrad': run_wgrad}


def run_case(case):
    """runs one case on the GPU; returns {'seen': {window: kernels}, 'ratio': {output: worst error / bound}, 'fails': [...]}"""
    ck = Checker()
    with knobs(case.knobs):
        seen = RUNNERS[case.op](case, ck)
    return {'seen': {k: sorted(v) for k, v in seen.items()}, 'ratio': ck.ratio, 'fails': ck.fails}


def missing_kernels(case, seen):
    out = [f'{direction}: {k}' for direction, names in case.kernels.items() for k in names if k not in seen.get(direction, ())]
    out += [f'{direction}: {k} ran (must not)' for direction, prefixes in case.absent.items() for k in seen.get(direction, ())
            if any(k.startswith(p) for p in prefixes)]
    return out


def _report(case, res):
    path = os.environ.get('LTU_TOKEN_PATHS_REPORT')
    if path:
        geo = {f'{f}/{k}': run_geometry(case, f, k) for f, k in (case.steady or [])}
        with open(path, 'a') as f:
            f.write(json.dumps({'case': case.name, 'op': case.op, 'kernels': case.kernels, 'knobs': case.knobs, 'geometry': geo, **res}) + '\n')


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available()
    from lintransunet_amd import ops  # noqa: F401
    return True


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_token_path(gpu, case):
    res = run_case(case)
    _report(case, res)
    worst = max(res['ratio'].items(), key=lambda kv: kv[1]) if res['ratio'] else None
    print(f'[token path {case.name}] worst error / bound {worst}')
    assert not res['fails'], f'{case.name}: ' + '; '.join(res['fails'])
    miss = missing_kernels(case, res['seen'])
    assert not miss, f'{case.name}: {miss}; launched {res["seen"]}'
