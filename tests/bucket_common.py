"""Parameter-side kernels on views packed inside flat buckets: the packed view, the case table, references, the census.

In training every parameter gradient (train.GradReducer._assign) and, once optim.FusedAdamW has re-homed them, every master weight
is a view `flat[off:off + n]` of one fp32 buffer, the parameters back to back with no padding: a view starts at any multiple of
4 bytes and its neighbours are other parameters.  The three path tables (test_gpu_conv_paths / _token_paths / _stream_paths) hand
every kernel a fresh, 256-byte aligned allocation.  This module holds what test_bucket_views.py (CPU) and test_gpu_bucket_views.py
share:

* `packed` / `Packed`: destinations back to back inside one buffer at a chosen residue (view offset mod 4 floats), between two
  guard bands of 64 position-dependent sentinels;
* CASES: for every weight-gradient entry point the sibling cases (shape and knobs are the sibling's) whose destinations are packed,
  the kernels that must run, and the rule that relates residues 1..3 to residue 0 (`bits`: bit-equal; `sum`: the destination is
  reached through fp32 atomics whose order is free, every residue is held against the float64 reference instead);
* float64 closed forms of the gradients that the siblings state inline (projection, LayerNorm gamma / beta) and their summed
  magnitudes; test_bucket_views.py checks them against autograd;
* `wprep_ref`: a numpy restatement of every weight-prep record kind's index map (layouts: model._WeightStore, ops.pair_records,
  ops.upconv_prep), with bf16 round-to-nearest-even;
* `census`: the residue of every parameter's gradient view of a reducer, and the entry point that consumes it.
"""
import math
import re

import numpy as np
import torch

from tests import test_gpu_conv_paths as CP
from tests import test_gpu_stream_paths as SP
from tests import test_gpu_token_paths as TP

GUARD = 64                   # floats of sentinel on either side of a packed body
RESIDUES = (0, 1, 2, 3)
SUM_REL = 1e-5               # biases, gamma / beta, the gate's psi bias: relative to the summed magnitudes (the siblings' F32_REL)
WGRAD_TOL = TP.WGRAD_TOL     # weight-like gradients: max|err| / max|ref|


# ---------------------------------------------------------------------------------------------- the packed view

def _sentinel(first, n):
    """n floats, each position its own value: 1e30 * (1 + i / 128), i counted from `first`"""
    return (1e30 * (1.0 + torch.arange(first, first + n, dtype=torch.float64) / 128.0)).float()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


class Packed:
    """`sizes` destinations back to back (no gap, as in a gradient bucket) in ONE fp32 buffer of 64 + residue + sum(sizes) + 64
    floats; the first destination starts `residue` floats behind a 16-byte boundary.  Everything in front of the body
    (64 + residue floats) and the 64 floats behind it hold sentinels that differ per position; the body holds `olds`
    (the kernels accumulate, so a destination starts from values of the gradient's magnitude, not zeros).
    `guard_fails()` names every guard float whose bits changed.

    Known limit: a read-modify-write that straddles a band and adds exactly 0 to the sentinel (or a value below half an ulp of
    1e30) leaves its bits intact and is not seen; a store of any other value, and any plain store, is."""

    def __init__(self, sizes, residue, olds, device='cuda'):
        assert residue in RESIDUES and len(sizes) == len(olds)
        self.sizes, self.residue = [int(n) for n in sizes], residue
        n = sum(self.sizes)
        self.lo = GUARD + residue
        self.buf = torch.empty(self.lo + n + GUARD, device=device, dtype=torch.float32)
        assert self.buf.data_ptr() % 16 == 0, 'a fresh allocation starts on a 16-byte boundary'
        self.front, self.back = _sentinel(0, self.lo), -_sentinel(self.lo, GUARD)
        self.buf[:self.lo] = self.front.to(device)
        self.buf[self.lo + n:] = self.back.to(device)
        self.views, off = [], self.lo
        for k, old in zip(self.sizes, olds):
            v = self.buf[off:off + k]
            v.copy_(old.reshape(-1).float().to(device))
            assert (v.data_ptr() - self.buf.data_ptr()) // 4 == off
            self.views.append(v)
            off += k
        self.body = self.buf[self.lo:self.lo + n]

    def starts(self):
        """residue (offset mod 4 floats from a 16-byte boundary) of every destination"""
        out, off = [], self.residue
        for k in self.sizes:
            out.append(off % 4)
            off += k
        return out

    def guard_fails(self):
        out = []
        n = sum(self.sizes)
        for what, got, want, base in (('front', self.buf[:self.lo], self.front, -self.lo), ('back', self.buf[self.lo + n:], self.back, n)):
            diff = (_bits(got).cpu() != _bits(want)).nonzero().flatten().tolist()
            if diff:
                out.append(f'{what} guard band written at body offsets {[base + i for i in diff[:8]]}'
                           f'{" ..." if len(diff) > 8 else ""} ({len(diff)} floats)')
        return out


def packed(n, residue, old, device='cuda'):
    """one destination of n floats at `residue`: returns the view `buf[64 + residue : 64 + residue + n]`; `view.pack` is its Packed
    (guards: `view.pack.guard_fails()`)"""
    p = Packed([n], residue, [old], device)
    v = p.views[0]
    v.pack = p
    return v


def bit_equal(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------- the part-1 table

class Case:
    """entry: the C entry point whose destinations are packed; sib: (table, case name) the shape and knobs come from, or None with
    `shape` / `knobs` given here (the shapes the issue adds); kernels: demangled names that must run in the backward window at
    every residue; by_residue: residue -> names, where a launcher provably picks another kernel for that residue; rule: 'bits'
    (residues 1..3 bit-equal to residue 0) or 'sum' (fp32 atomics: every residue against the float64 reference)"""

    def __init__(self, name, entry, sib, kernels, rule='bits', shape=None, knobs=None, op=None, by_residue=None, absent=()):
        self.name, self.entry, self.sib_ref, self.kernels, self.rule = name, entry, sib, list(kernels), rule
        self.by_residue = dict(by_residue or {})
        self.absent = tuple(absent)
        if sib is not None:
            table, sname = sib
            c = next(c for c in {'conv': CP.CASES, 'token': TP.CASES, 'stream': SP.CASES}[table] if c.name == sname)
            self.sib, self.shape, self.knobs = c, c.shape, dict(c.knobs)
            self.op = 'conv3d' if c.op == 'conv_wgrad' else c.op      # the stream table's first-level fold case is a conv3d shape
        else:
            self.sib, self.shape, self.knobs, self.op = None, shape, dict(knobs or {}), op

    def names(self, residue):
        return self.by_residue.get(residue, self.kernels)

    def __repr__(self):
        return self.name


ENTRY_POINTS = ('ltu_conv3d_wgrad', 'ltu_conv3d_pair_wgrad', 'ltu_upconv_wgrad', 'ltu_linear_wgrad', 'ltu_linear_wgrad_group',
                'ltu_layernorm_bwd', 'ltu_layer_tail_bwd', 'ltu_dwconv_bwd', 'ltu_gate_bwd')

RED = TP.RED
TN = CP.tn
LN_BATCH = 'reduce_batch_kernel'      # gamma / beta living in a bucket: the partials are folded by ltu_reduce_batch, not reduce_parts
FAT = 'wgrad_fat_group_bf16_kernel'

CASES = [
    # ---- ltu_conv3d_wgrad ------------------------------------------------------------------------------------------------------
    Case('conv_wgrad_reduce64', 'ltu_conv3d_wgrad', ('stream', 'conv_wgrad_reduce64'), [CP.WH_PACK, RED(64)]),
    Case('whalo_ring_concat', 'ltu_conv3d_wgrad', ('conv', 'whalo_ring_concat'), [CP.WH_RING, RED(4)]),
    Case('halo_deep_split', 'ltu_conv3d_wgrad', ('conv', 'halo_deep_split'), [CP.WH_RING, RED(4)]),
    Case('conv_ring_split', 'ltu_conv3d_wgrad', ('conv', 'conv_ring_split'), [CP.WH_RING, RED(4)]),
    Case('sdgrad_ring_222', 'ltu_conv3d_wgrad', ('conv', 'sdgrad_ring_222'), [TN(2, 2, 2, 2), RED(4)]),
    Case('class_gemm_221', 'ltu_conv3d_wgrad', ('conv', 'class_gemm_221'), [TN(1, 4, 1, 1), RED(4)]),
    # Co = 5 padded to an 8-column head: a weight of 5 * 16 * 27 floats and a bias of 5
    Case('c16_ring_head', 'ltu_conv3d_wgrad', ('conv', 'c16_ring_head'), [CP.WH_PACK, RED(64)]),
    # the mask_conv_list shape of a 3-class model at the third level: 3 x 64 x 27 and a 3-float bias, on an 8-column head
    Case('class_head_3x64', 'ltu_conv3d_wgrad', None, [CP.WH_RING, RED(4)], shape=CP.conv(1, 64, 3, 9, 10, 12, cop=8), op='conv3d'),
    # ---- ltu_conv3d_pair_wgrad: four destinations (64 -> 32 beside a 3-class head padded to 32) -------------------------------------
    Case('whalo_ring_pair', 'ltu_conv3d_pair_wgrad', ('conv', 'whalo_ring_pair'), [CP.WH_RING, RED(4)]),
    # ---- ltu_upconv_wgrad: the class-ordered partial sums are folded onto the 27 taps of the gradient by wgrad_reduce_kernel ---------
    Case('upconv_class_ring', 'ltu_upconv_wgrad', ('conv', 'upconv_class_ring'), ['upconv_wgrad_class_bf16_kernel', RED(4)]),
    Case('upconv_class_halo', 'ltu_upconv_wgrad', ('conv', 'upconv_class_halo'), ['upconv_wgrad_ring_bf16_kernel', RED(4)]),
    Case('upconv_class_gemm', 'ltu_upconv_wgrad', ('conv', 'upconv_class_gemm'), [TN(1, 4, 1, 1), 'upconv_fold_kernel', RED(4)]),
    # ---- ltu_linear_wgrad ------------------------------------------------------------------------------------------------------------
    Case('lin_qkv128_ragged', 'ltu_linear_wgrad', ('token', 'lin_qkv128_ragged'), [TN(2, 2, 2, 2), RED(4)]),
    Case('lin_qkv256', 'ltu_linear_wgrad', ('token', 'lin_qkv256'), [TP.TN6, RED(4)]),
    # the attention gates' 1x1x1 projections W_x (K = 16) and W_g (K = 32) of the first level, on the gate cases' 2 x 213 voxels
    Case('gate_proj_k16', 'ltu_linear_wgrad', None, [TN(1, 4, 1, 1), RED(4)], shape=dict(M=426, K=16, N=16, nw=1), op='linear'),
    Case('gate_proj_k32', 'ltu_linear_wgrad', None, [TN(1, 4, 1, 1), RED(4)], shape=dict(M=426, K=32, N=16, nw=1), op='linear'),
    # ---- ltu_linear_wgrad_group ------------------------------------------------------------------------------------------------------
    Case('wgroup_fold_long_runs', 'ltu_linear_wgrad_group', ('token', 'wgroup_fold_long_runs'), [TP.WG, TP.FOLD]),
    Case('wgroup_direct', 'ltu_linear_wgrad_group', ('token', 'wgroup_direct'), [TP.WG], absent=[TP.FOLD]),
    Case('wgroup_no_direct', 'ltu_linear_wgrad_group', ('token', 'wgroup_no_direct'), [TP.WG, TP.FOLD]),
    Case('wgroup_off', 'ltu_linear_wgrad_group', ('token', 'wgroup_off'), [TP.TN6, RED(4)], absent=[TP.WG]),
    Case('wgrad_deferred_batch', 'ltu_linear_wgrad_group', ('token', 'wgrad_deferred_batch'), [TP.TN6, 'reduce_batch_kernel'],
         absent=['wgrad_reduce_kernel']),
    # the fat-tile grouped kernel at the shape test_gpu_ops.test_linear_wgrad_group runs with fat = 1.  It is compiled into an
    # experiments build only: there LTU_WGROUP_FAT selects it; in the default build the launcher has no such kernel and the same
    # call takes the grouped ring and its fold, which the case then names (test_gpu_bucket_views.fat_kernels)
    Case('wgroup_fat', 'ltu_linear_wgrad_group', None, [FAT], shape=dict(M=2048, d=128, mode='group'), knobs={'LTU_WGROUP_FAT': 1},
         op='wgrad'),
    # ---- ltu_layernorm_bwd and ltu_layer_tail_bwd: gamma / beta of both norms, the tail's projection gradients ---------------------
    Case('ln128_drop', 'ltu_layernorm_bwd', ('token', 'ln128_drop'), ['layernorm_bwd_kernel<bf16_t, 16, 2>', LN_BATCH]),
    Case('ln256_dy2', 'ltu_layernorm_bwd', ('token', 'ln256_dy2'), ['layernorm_bwd_kernel<bf16_t, 32, 2>', LN_BATCH]),
    # ragged M = 999: the grouped ring declines (M % 32), one ltu_linear_wgrad per projection: the conv family's TN GEMM
    Case('tail128_ragged_drop', 'ltu_layer_tail_bwd', ('token', 'tail128_ragged_drop'), [TP.tb(128, 1, 4, True), TN(2, 2, 2, 2), RED(4), LN_BATCH]),
    # M = 448 rows: below the rings' row count too (one ltu_linear_wgrad per projection, folded by wgrad_reduce_kernel<4>)
    Case('tail256_attn_drop', 'ltu_layer_tail_bwd', ('token', 'tail256_attn_drop'), [TP.tb(256, 1, 4, False), TN(2, 2, 2, 2), RED(4), LN_BATCH]),
    # ---- ltu_dwconv_bwd ----------------------------------------------------------------------------------------------------------------
    Case('dw_c8_long_drop', 'ltu_dwconv_bwd', ('stream', 'dw_c8_long_drop'), [SP.DW1, SP.DW2, SP.DWF]),
    Case('dw_c72_atomics_drop', 'ltu_dwconv_bwd', ('stream', 'dw_c72_atomics_drop'), [SP.DW1, SP.DW2], rule='sum', absent=[SP.DWF]),
    # ---- ltu_gate_bwd: psi weight of C floats, psi bias of ONE float, the next parameter's view directly behind it ------------------
    # rule 'sum' for all three: without a workspace every block adds with atomics; with one, gate_fold_kernel (grid.y = samples)
    # still adds each SAMPLE's folded sums to dpsi_w / dpsi_b with atomicAdd (pointwise.hip), so with B = 2 the destination is
    # (old + s0) + s1 or (old + s1) + s0, whichever workgroup comes first: two roundings of one fp32 sum at any address
    Case('gate_c8', 'ltu_gate_bwd', ('stream', 'gate_c8'), SP.gate_k(8)['bwd'], rule='sum'),
    Case('gate_c32_atomics', 'ltu_gate_bwd', ('stream', 'gate_c32_atomics'), SP.gate_k(32, ws=False)['bwd'], rule='sum',
         absent=['gate_fold_kernel']),
    Case('gate_c256', 'ltu_gate_bwd', ('stream', 'gate_c256'), SP.gate_k(256)['bwd'], rule='sum'),
]

NEIGHBOUR = 16               # floats of the view packed behind the gate's one-float psi bias: no kernel may touch them


def named_kernels():
    return {k for c in CASES for ks in [c.kernels] + list(c.by_residue.values()) for k in ks}


def _wgrad_jobs(d):
    return TP._wgrad_jobs(d)


def dest_sizes(case):
    """(label, floats) of every destination of a case in the order they are packed: a bias, gamma or beta directly behind its weight"""
    s = case.shape
    if case.op == 'conv3d':
        return [('dw', s['Co'] * (s['Ci'] + s['C1']) * 27), ('db', s['Co'])]
    if case.op == 'pair':
        return [('dwa', s['Ca'] * s['Ci'] * 27), ('dba', s['Ca']), ('dwb', s['Cb'] * s['Ci'] * 27), ('dbb', s['Cb'])]
    if case.op == 'upconv':
        return [('dw', s['Co'] * s['Ci'] * 27), ('db', s['Co'])]
    if case.op == 'linear':
        ns = s['N'] // s['nw']
        return [x for i in range(s['nw']) for x in ((f'dw{i}', ns * s['K']), (f'db{i}', ns))]
    if case.op == 'wgrad':
        return [x for N, K, nw in _wgrad_jobs(s['d']) for i in range(nw)
                for x in ((f'dw[{N}x{K}].{i}', N // nw * K), (f'db[{N}x{K}].{i}', N // nw))]
    if case.op == 'ln':
        return [('dgamma', s['d']), ('dbeta', s['d'])]
    if case.op == 'tail':
        d = s['d']
        return [('dwo', d * d), ('dbo', d), ('dw1', 2 * d * d), ('db1', 2 * d), ('dw2', 2 * d * d), ('db2', d),
                ('dg1', d), ('dbe1', d), ('dg2', d), ('dbe2', d)]
    if case.op == 'dw':
        return [('dw', s['C'] * 27), ('db', s['C'])]
    assert case.op == 'gate', case.op
    return [('dpsi_w', s['C']), ('dpsi_b', 1), ('neighbour', NEIGHBOUR)]


def old_scale(case):
    """magnitude of the values a destination holds before the call: that of a sum of `terms` products of unit-variance operands"""
    s = case.shape
    if case.op in ('conv3d', 'pair', 'upconv'):
        up = 8 if case.op == 'upconv' else 1
        st = s.get('stride', (1, 1, 1))
        terms = s['B'] * up * -(-s['H'] // st[0]) * -(-s['W'] // st[1]) * -(-s['D'] // st[2])
    elif case.op in ('linear', 'wgrad', 'ln'):
        terms = s['M']
    elif case.op == 'tail':
        terms = s['B'] * s['N']
    elif case.op == 'dw':
        terms = s['B'] * s['H'] * s['W'] * s['D']
    else:
        terms = s['B'] * s['S']
    return math.sqrt(terms)


def olds(case):
    """the values every destination of the case starts from: seeded, the same at every residue"""
    g = torch.Generator().manual_seed(9000 + sum(map(ord, case.name)))
    sc = old_scale(case)
    return [(sc * torch.randn(n, generator=g)).float() for _, n in dest_sizes(case)]


# ---------------------------------------------------------------------------------------------- float64 closed forms

def linear_wgrad_ref(go, x, nw):
    """y = x cat(W_i)^T + cat(b_i), go = dL/dy [M, N], x [M, K] (float64): per block i (dW_i, db_i, the summed magnitudes of db_i)"""
    ns = go.shape[1] // nw
    return [(go[:, i * ns:(i + 1) * ns].T @ x, go[:, i * ns:(i + 1) * ns].sum(0), go[:, i * ns:(i + 1) * ns].abs().sum(0)) for i in range(nw)]


def ln_param_ref(G, z, mean, rstd):
    """LayerNorm y = zn gamma + beta with zn = (z - mean) rstd, G = dL/dy: (dgamma, dbeta, summed magnitudes of both)"""
    zn = (z - mean) * rstd
    return (G * zn).sum(0), G.sum(0), (G * zn).abs().sum(0), G.abs().sum(0)


def adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step, gscale, ema=None, decay=0.0):
    """float64 AdamW step (decoupled weight decay, bias-corrected moments) of misc.hip adamw_kernel / optim.hip: new (p, m, v, ema)"""
    gg = g * gscale
    m2 = b1 * m + (1 - b1) * gg
    v2 = b2 * v + (1 - b2) * gg * gg
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p2 = p * (1 - lr * wd) - (lr / bc1) * m2 / (v2.sqrt() / math.sqrt(bc2) + eps)
    e2 = None if ema is None else decay * ema + (1 - decay) * p2
    return p2, m2, v2, e2


# ---------------------------------------------------------------------------------------------- weight prep, restated

WPREP_CHUNK = 4096


def bf16_bits(x):
    """float32 array -> bf16 bit patterns (uint16), round to nearest even; the inputs are finite"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


_TAPS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}      # (parity class, slot) of one axis -> taps summed


def _subpixel(w):
    """[Co][Ci][3][3][3] float32 -> [class 8][slot 8][Co][Ci]: fp32 sums over the taps of each (class, slot), taps ascending in
    (h, w, d) order starting from 0 as misc.hip kinds 5 / 6 add them"""
    Co, Ci = w.shape[:2]
    out = np.zeros((8, 8, Co, Ci), dtype=np.float32)
    for cls in range(8):
        for sl in range(8):
            acc = np.zeros((Co, Ci), dtype=np.float32)
            for th in _TAPS[(cls >> 2) & 1, (sl >> 2) & 1]:
                for tw in _TAPS[(cls >> 1) & 1, (sl >> 1) & 1]:
                    for td in _TAPS[cls & 1, sl & 1]:
                        acc = (acc + w[:, :, th, tw, td]).astype(np.float32)
            out[cls, sl] = acc
    return out


def wprep_size(kind, R, C, p0, p1, pad):
    """destination elements a record enumerates (model._WeightStore.finalize)"""
    if kind in (0, 1, 4, 8, 9):
        return R * C
    if kind in (2, 3):
        return p0 * 27 * p1
    if kind == 7:
        return (pad & 0xffff) * 27 * p1
    return 64 * p0 * p1


def wprep_ref(kind, src, R, C, p0, p1, pad, extent):
    """the fp32 values record (kind, R, C, p0, p1, pad) stores from `src` (float32, R * C [* 27] values) into a flat destination of
    `extent` elements: (values, written mask).  Elements outside the mask are not the record's to write."""
    src = np.asarray(src, dtype=np.float32)
    val, wr = np.zeros(extent, dtype=np.float32), np.zeros(extent, dtype=bool)

    def put(idx, v):
        idx = np.asarray(idx).reshape(-1)
        assert idx.size == np.unique(idx).size and idx.max() < extent
        val[idx] = np.asarray(v, dtype=np.float32).reshape(-1)
        wr[idx] = True
    if kind in (0, 4):                                   # cast / fp32 copy: dst[i] = src[i]
        put(np.arange(R * C), src.reshape(-1))
    elif kind == 1:                                      # transpose: dst[c * p0 + p1 + r] = src[r][c]
        r, c = np.meshgrid(np.arange(R), np.arange(C), indexing='ij')
        put(c * p0 + p1 + r, src.reshape(R, C))
    elif kind in (2, 3):                                 # conv [Co][Ci][27] -> [CoP][27][CiP] (2) / [CiP][27][CoP] (3), zero padded
        w = np.zeros((p0, p1, 27), dtype=np.float32)
        w[:R, :C] = src.reshape(R, C, 27)
        put(np.arange(p0 * 27 * p1), w.transpose(0, 2, 1) if kind == 2 else w.transpose(1, 2, 0))
    elif kind in (5, 6):                                 # sub-pixel operands: [8][CoP][8][CiP] (5) / [CiP][64][CoP] (6), zero padded
        w = np.zeros((8, 8, p0, p1), dtype=np.float32)
        w[:, :, :R, :C] = _subpixel(src.reshape(R, C, 3, 3, 3))
        put(np.arange(64 * p0 * p1), w.transpose(0, 2, 1, 3) if kind == 5 else w.transpose(3, 0, 1, 2))
    elif kind == 7:                                      # columns [off, off + cnt) of [CiP][27][p0]; pad = off << 16 | cnt
        off, cnt = pad >> 16, pad & 0xffff
        w = np.zeros((cnt, p1, 27), dtype=np.float32)
        w[:R, :C] = src.reshape(R, C, 27)
        ci, t, co = np.meshgrid(np.arange(p1), np.arange(27), np.arange(cnt), indexing='ij')
        put((ci * 27 + t) * p0 + off + co, w.transpose(1, 2, 0))
    else:                                                # MFMA fragment order: element ((ct * KS + ks) * 64 + l) * 8 + j
        assert kind in (8, 9) and R % 32 == 0 and C % 32 == 0
        W = src.reshape(R, C) if kind == 8 else src.reshape(R, C).T        # [outputs][reduction]
        i = np.arange(R * C)
        j, l, t = i & 7, (i >> 3) & 63, i >> 9
        KS = W.shape[1] // 16
        ks, ct = t % KS, t // KS
        put(i, W[ct * 32 + (l & 31), ks * 16 + 8 * (l >> 5) + j])
    return val, wr


def chunk_list(records):
    """(record, chunk) pairs of WPREP_CHUNK destination elements, as model._WeightStore.finalize lists them"""
    return [(i, c) for i, (kind, R, C, p0, p1, pad) in enumerate(records)
            for c in range((wprep_size(kind, R, C, p0, p1, pad) + WPREP_CHUNK - 1) // WPREP_CHUNK)]


# ---------------------------------------------------------------------------------------------- census of a reducer's views

_FAMILY = [
    (r'\.psi\.0\.', 'ltu_gate_bwd'),
    (r'att_conv_list\.\d+\.W_[xg]\.', 'ltu_linear_wgrad'),
    (r'\.up_embed\.', 'ltu_upconv_wgrad'),
    (r'\.pos_encoders?\.', 'ltu_dwconv_bwd'),
    (r'\.self_attn\.linears\.|\.linear[12]\.', 'ltu_linear_wgrad_group'),
    (r'\.layer_norm[12]\.', 'ltu_layer_tail_bwd'),
    (r'mask_conv_list\.|decode\.block_list\.\d+\.conv1\.', 'ltu_conv3d_pair_wgrad'),
]


def family(name):
    """the weight-gradient entry point that writes a parameter's gradient in the bf16 model (model.py: which op a module runs through)"""
    for pat, fam in _FAMILY:
        if re.search(pat, name):
            return fam
    return 'ltu_conv3d_wgrad'


def census(model, reducer):
    """[(parameter name, bucket, residue of its gradient view, floats)] in bucket order; checks that the views tile every bucket"""
    names = {p: n for n, p in model.named_parameters()}
    out = []
    for bi, (plist, flat) in enumerate(zip(reducer.buckets, reducer.flat)):
        off = 0
        for p in plist:
            g = p.grad
            assert g.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() and g.storage_offset() == off, names[p]
            out.append((names[p], bi, off % 4, p.numel()))
            off += p.numel()
        assert off == flat.numel(), f'bucket {bi}: the views cover {off} of {flat.numel()} floats'
    return out


def census_by_family(rows):
    """{entry point: {residue: views}}"""
    out = {}
    for name, _, res, _ in rows:
        d = out.setdefault(family(name), {})
        d[res] = d.get(res, 0) + 1
    return out
