"""The shape rules of the bf16 3x3x3 conv launchers, restated as a table, and the shapes that sit on both sides of each.

A conv is a chain of launchers; each accepts or declines a shape by clauses `if (...) return 1;`.  RULES restates every clause that
an ops-level shape can reach: where it stands (file, function, literal text), the launcher argument it rules, the clause as a
lambda over the launcher's arguments (launcher_args), and two or three adjacent shapes (`sides`) with the kernels that must run on
each.  UNSWEPT lists the clauses no shape within the size caps reaches, each with its reason.  tests/test_conv_sweep.py holds the
table against the sources (a moved threshold fails there until the table follows); tests/test_gpu_conv_sweep.py runs the sides
and random_cases on the GPU against the float64 reference and the gates of tests/test_gpu_conv_paths.py.

Host only: nothing here touches the GPU.
"""
import zlib

import torch

from tests.test_gpu_conv_paths import Case, conv, pair, up

MAX_VOXELS = 70000               # output voxels of a case
MAX_ROW_MACS = 16 * 2 ** 20      # multiply-adds per output voxel row
RANDOM_MACS = 2 ** 26            # random_cases: multiply-adds of one forward (0.1 s of float64 reference)

REFUSED = 'LtuError'             # a side no launcher of the chain accepts: the op raises

HALO, WS, WR = 'conv3_halo_bf16_kernel', 'conv3_halo_ws_bf16_kernel', 'conv3_halo_wr_bf16_kernel'
FC, C16, RING, FOLD = 'conv3_fc_ring_bf16_kernel', 'conv3_c16_ring_bf16_kernel', 'conv3_ring_bf16_kernel', 'conv_halo_fold_kernel'
WH, WHR = 'conv3_wgrad_halo_bf16_kernel', 'conv3_wgrad_halo_ring_bf16_kernel'
IG, TN = 'igemm_nt_bf16_kernel', 'wgrad_tn_bf16_kernel'
SD, CLS_RING, CLS_HALO = 'sdgrad_ring_bf16_kernel', 'conv_class_ring_bf16_kernel', 'conv_class_halo_bf16_kernel'
UPRING, UPDGRAD = 'upconv_ring_bf16_kernel', 'updgrad_ring_bf16_kernel'
UPW_RING, UPW_CLASS, UPFOLD = 'upconv_wgrad_ring_bf16_kernel', 'upconv_wgrad_class_bf16_kernel', 'upconv_fold_kernel'

F_HALO, F_RING, F_C16, F_FC = 'conv_halo.hip', 'conv_ring.hip', 'conv_c16_ring.hip', 'conv_fc_ring.hip'
F_WHR, F_SD, F_UD, F_UR, F_UWR, F_UP, F_GEMM = ('wgrad_halo_ring.hip', 'sdgrad_ring.hip', 'updgrad_ring.hip', 'upconv_ring.hip',
                                                'upconv_wgrad_ring.hip', 'upconv.hip', 'gemm.hip')
L_HALO, L_WH, L_CLS, L_UPW = ('launch_conv_halo_bf16', 'launch_conv_wgrad_halo_bf16', 'launch_conv_class_halo_bf16',
                              'launch_upconv_wgrad_class_bf16')
L_RING, L_C16, L_FC, L_WHR = 'launch_conv_ring_bf16', 'launch_conv_c16_ring_bf16', 'launch_conv_fc_ring_bf16', 'launch_conv_wgrad_halo_ring_bf16'
L_SD, L_UD, L_UR, L_UWR = 'launch_sdgrad_ring_bf16', 'launch_updgrad_ring_bf16', 'launch_upconv_ring_bf16', 'launch_upconv_wgrad_ring_bf16'

# the launchers whose clauses the census reads: whole files, of gemm.hip the conv entry points only
CENSUS_FILES = [F_HALO, F_RING, F_C16, F_FC, F_WHR, F_SD, F_UD, F_UR, F_UWR, F_UP]
CENSUS_GEMM = ['conv_fwd_desc', 'ltu_conv3d_fwd', 'ltu_conv3d_wgrad', 'ltu_conv3d_dgrad', 'ltu_conv3d_pair_fwd', 'ltu_conv3d_pair_dgrad',
               'ltu_conv3d_pair_wgrad']


def _cdiv(a, b):
    return -(-a // b)


class Args(dict):
    __getattr__ = dict.__getitem__


def launcher_args(op, direction, s):
    """what the launchers of one direction see of an op-level shape: C / c0 (reduction channels, first operand's share), N / n0
    (output columns, first output's share), the grid H, W, D (of a strided data gradient: the class kernels' coarse grid Ho, Wo, Do
    beside the fine Hl, Wl, Dl), and the brick counts.  A stride-1 data gradient is the forward launcher with C and N exchanged."""
    B, H, W, D = s['B'], s['H'], s['W'], s['D']
    a = Args(B=B, H=H, W=W, D=D)
    if op == 'conv3d':
        cin, co = s['Ci'] + s['C1'], s['cop'] or s['Co']
        sh, sw, sd = s['stride']
        if direction == 'dgrad':
            a.update(C=co, c0=co, N=cin, n0=s['Ci'], Co=co, sd=sd, Hl=H, Wl=W, Dl=D,
                     Ho=(H - 1) // sh + 1, Wo=(W - 1) // sw + 1, Do=(D - 1) // sd + 1)
        else:
            a.update(C=cin, c0=s['Ci'], N=co, n0=co, C0=s['Ci'], C1=s['C1'], Co=co)
    elif op == 'pair':
        n = s['Ca'] + s['n1']
        if direction == 'dgrad':
            a.update(C=n, c0=s['Ca'], N=s['Ci'], n0=s['Ci'])
        else:
            a.update(C=s['Ci'], c0=s['Ci'], N=n, n0=s['Ca'])
        a.update(N0=s['Ca'], N1=s['n1'])
    else:
        a.update(Ci=s['Ci'], Co=s['Co'], C=s['Ci'], N=s['Co'])
    a['bricks448'] = B * _cdiv(a.H, 4) * _cdiv(a.W, 4) * _cdiv(a.D, 8)
    a['bricks488'] = B * _cdiv(a.H, 4) * _cdiv(a.W, 8) * _cdiv(a.D, 8)
    a['bricks888'] = B * _cdiv(a.H, 8) * _cdiv(a.W, 8) * _cdiv(a.D, 8)
    return a


def case_name(op, s):
    if op == 'conv3d':
        c = f"{s['Ci']}+{s['C1']}" if s['C1'] else f"{s['Ci']}"
        st = '' if s['stride'] == (1, 1, 1) else '_s' + ''.join(map(str, s['stride']))
        return f"conv_{s['B']}x{c}to{s['Co']}{'p%d' % s['cop'] if s['cop'] else ''}_{s['H']}x{s['W']}x{s['D']}{st}"
    if op == 'pair':
        return f"pair_{s['B']}x{s['Ci']}to{s['Ca']}+{s['Cb']}p{s['n1']}_{s['H']}x{s['W']}x{s['D']}"
    return f"up_{s['B']}x{s['Ci']}to{s['Co']}_{s['H']}x{s['W']}x{s['D']}"


def case_seed(name):
    return zlib.crc32(name.encode())


def out_voxels(op, s):
    if op == 'conv3d':
        sh, sw, sd = s['stride']
        return s['B'] * ((s['H'] - 1) // sh + 1) * ((s['W'] - 1) // sw + 1) * ((s['D'] - 1) // sd + 1)
    return s['B'] * s['H'] * s['W'] * s['D'] * (8 if op == 'upconv' else 1)


def row_macs(op, s):
    """multiply-adds per output voxel row"""
    if op == 'conv3d':
        return 27 * (s['Ci'] + s['C1']) * (s['cop'] or s['Co'])
    if op == 'pair':
        return 27 * s['Ci'] * (s['Ca'] + s['n1'])
    return 27 * s['Ci'] * s['Co']


def refusal(op, s, backward=True):
    """why the bf16 C ABI refuses a shape (None: it accepts).  Activations are read 8 channels (16 bytes) at a time and outputs
    written 4 at a time: every launcher down to the implicit GEMM states C % 8 and N % 4; a backward makes the outputs the
    reduction channels of the data gradient and the weight gradient wants N % 8, so there every count is a multiple of 8."""
    if op == 'conv3d':
        if s['Ci'] <= 0 or s['Ci'] % 8 or s['C1'] % 8:
            return 'input channels: C0 % 8, C1 % 8'
        if any(v not in (1, 2) for v in s['stride']):
            return 'stride'
        n, what = s['cop'] or s['Co'], 'Co'
    elif op == 'pair':
        if s['Ci'] <= 0 or s['Ci'] % 8:
            return 'input channels: C % 8'
        if s['Ca'] <= 0 or s['n1'] <= 0 or s['n1'] % 4:
            return 'N1 % 4'
        if backward and s['n1'] % 8:
            return 'N1 % 8 (backward)'
        n, what = s['Ca'], 'N0'
    else:
        if s['Ci'] <= 0 or s['Ci'] % 8:
            return 'input channels: Ci % 8'
        n, what = s['Co'], 'Co'
    if n <= 0 or n % 4:
        return f'{what} % 4'
    if backward and n % 8:
        return f'{what} % 8 (backward)'
    return None


class Side:
    """one shape of a rule: kernels = {direction: [kernel base names that must run]} or REFUSED; backward = False: the shape
    has no backward in bf16 (N % 8, whalo_N_8) and only its forward runs"""

    def __init__(self, shape, kernels, backward=True):
        self.shape, self.kernels, self.backward = shape, kernels, backward


class Rule:
    """sources: [(file, function, clause text)] the rule restates (a clause of an `if (...) return`, the text of a helper's
    condition, or an `ltu_knob_pos(...)` call); arg: the launcher argument ruled and what it is of the op's shape; varies: the keys
    of the op's shape in which the sides differ; clause: the first source over launcher_args(op, direction, shape)"""

    def __init__(self, name, sources, op, direction, arg, varies, clause, sides, knobs=None):
        self.name, self.sources, self.op, self.direction, self.arg = name, sources, op, direction, arg
        self.varies, self.clause, self.sides, self.knobs = tuple(varies), clause, sides, dict(knobs or {})

    def __repr__(self):
        return self.name

    def case(self, side):
        """the Case of a side; named by shape and knobs alone, so rules that share a shape share its reference"""
        kn = ''.join(f'_{k[4:].lower()}{v}' for k, v in sorted(self.knobs.items()))
        c = Case(case_name(self.op, side.shape) + kn, self.op, side.shape, {} if side.kernels == REFUSED else side.kernels, self.knobs)
        c.backward = side.backward
        return c


T = (3, 5, 9)            # the tiny ragged grid of most rules: 4 bricks of 4x4x8, 2 of 4x8x8
S222, S221 = (2, 2, 2), (2, 2, 1)
NO_SD = {'LTU_NO_SDGRAD_RING': 1}


def _dims(name, axis, lo, hi, sources, op, direction, arg, base, kernels_lo, kernels_hi, clause, knobs=None):
    """a minimum-extent rule: the sides are `base` with one axis at lo | hi"""
    def at(v):
        s = dict(base)
        s[axis] = v
        return s
    return Rule(name, sources, op, direction, arg, (axis,), clause, [Side(at(lo), kernels_lo), Side(at(hi), kernels_hi)], knobs)


def _k(fwd=None, dgrad=None, wgrad=None):
    return {d: list(v) for d, v in (('fwd', fwd), ('dgrad', dgrad), ('wgrad', wgrad)) if v}


_GEN1 = _k([IG], [IG], [TN])                     # no halo kernel at all: implicit GEMMs
_C16T = conv(1, 16, 16, *T)
_UPT = up(1, 128, 32, 2, 5, 3)
_UP_GEMM = _k([IG], [IG], [TN, UPFOLD])
_UP_RINGS = _k([UPRING], [UPDGRAD], [UPW_RING])

RULES = [
    # ---------------------------------------------------------------- conv_halo.hip: launch_conv_halo_bf16 (forward, stride-1 dgrad)
    Rule('halo_C_8', [(F_HALO, L_HALO, 'a.C % 8')], 'conv3d', 'fwd', 'a.C = Ci + C1', ['Ci'], lambda a: a.C % 8 != 0,
         [Side(conv(1, 8, 16, *T), _k([WR])), Side(conv(1, 12, 16, *T), REFUSED)]),
    Rule('halo_c0_8', [(F_HALO, L_HALO, 'a.c0 % 8')], 'conv3d', 'fwd', 'a.c0 = Ci', ['Ci', 'C1'], lambda a: a.c0 % 8 != 0,
         [Side(conv(1, 16, 16, *T, C1=16), _k([WS])), Side(conv(1, 12, 16, *T, C1=20), REFUSED)]),
    Rule('halo_N_4', [(F_HALO, L_HALO, 'a.N % 4'), (F_GEMM, 'ltu_conv3d_wgrad', 'Co % 4 != 0'), (F_GEMM, 'ltu_conv3d_dgrad', 'Co % 4 != 0')],
         'conv3d', 'fwd', 'a.N = Co', ['Co'], lambda a: a.N % 4 != 0,
         [Side(conv(1, 16, 8, *T), _k([WR])), Side(conv(1, 16, 6, *T), REFUSED)]),
    _dims('halo_H_2', 'H', 1, 2, [(F_HALO, L_HALO, 'a.H < 2'), (F_HALO, L_WH, 'a.H < 2')], 'conv3d', ('fwd', 'dgrad', 'wgrad'), 'a.H = H',
          _C16T, _GEN1, _k([WR], [WR], [WH]), lambda a: a.H < 2),
    _dims('halo_W_2', 'W', 1, 2, [(F_HALO, L_HALO, 'a.W < 2'), (F_HALO, L_WH, 'a.W < 2')], 'conv3d', ('fwd', 'dgrad', 'wgrad'), 'a.W = W',
          _C16T, _GEN1, _k([WR], [WR], [WH]), lambda a: a.W < 2),
    _dims('halo_D_4', 'D', 3, 4, [(F_HALO, L_HALO, 'a.D < 4'), (F_HALO, L_WH, 'a.D < 4')], 'conv3d', ('fwd', 'dgrad', 'wgrad'), 'a.D = D',
          _C16T, _GEN1, _k([WR], [WR], [WH]), lambda a: a.D < 4),
    # 24 channels: no halo kernel in either generation; 8: the one chunk of 16 is half padding
    Rule('halo_C_16', [(F_HALO, L_HALO, 'a.C % 16 != 0 && a.C != 8'), (F_HALO, 'whalo_shape_ok', '(C % 16 == 0 || C == 8)')],
         'conv3d', ('fwd', 'wgrad'), 'a.C = Ci', ['Ci'], lambda a: a.C % 16 != 0 and a.C != 8,
         [Side(conv(1, 24, 16, *T), _k([IG], None, [TN])), Side(conv(1, 16, 16, *T), _k([WR], None, [WH])),
          Side(conv(1, 8, 16, *T), _k([WR], None, [WH]))]),
    # concat split inside a 16-channel chunk: 8 + 24 has no halo kernel, 16 + 16 runs 16-channel chunks
    Rule('halo_c0_CC', [(F_HALO, L_HALO, 'a.c0 % a.CC != 0 && a.c0 != a.C')], 'conv3d', 'fwd', 'a.c0 = Ci (a.CC = 16: c0 % 32 != 0)',
         ['Ci', 'C1'], lambda a: a.c0 % (32 if a.C % 32 == 0 and a.c0 % 32 == 0 else 16) != 0 and a.c0 != a.C,
         [Side(conv(1, 16, 32, *T, C1=16), _k([WS])), Side(conv(1, 8, 32, *T, C1=24), _k([IG]))]),
    # ---------------------------------------------------------------- halo_split: the channel split of small grids
    Rule('halo_split_ws', [(F_HALO, 'halo_split', 'N <= 32 && C <= 32')], 'conv3d', 'fwd', 'C = Ci', ['Ci'],
         lambda a: a.N <= 32 and a.C <= 32,
         [Side(conv(1, 32, 32, *T), _k([HALO])), Side(conv(1, 64, 32, *T), _k([HALO, FOLD]))], {'LTU_NO_HALO_WS': 1}),
    # 199 | 200 bricks of 4x4x8 x one 64-column tile
    Rule('halo_split_below', [(F_HALO, 'halo_split', 'blocks >= ltu_knob_pos("LTU_HALO_SPLIT_BELOW", 200)')], 'conv3d', 'fwd',
         'blocks = bricks of 4x4x8 x column tiles', ['D'], lambda a: a.bricks448 >= 200,
         [Side(conv(1, 64, 32, 2, 2, 1585), _k([HALO, FOLD])), Side(conv(1, 64, 32, 2, 2, 1593), _k([HALO]))]),
    Rule('halo_split_nchunk', [(F_HALO, 'halo_split', 'nchunk < 2')], 'conv3d', 'fwd', 'nchunk = cdiv(C, CC), C = Ci', ['Ci'],
         lambda a: _cdiv(a.C, 32) < 2,
         [Side(conv(1, 32, 64, *T), _k([HALO])), Side(conv(1, 64, 64, *T), _k([HALO, FOLD]))], {'LTU_NO_CONV_RING': 1}),
    # 128-column tiles from 256 workgroups on; 8 channels: conv_ring declines (C % 32), one half-empty chunk
    Rule('halo_wide_tile', [(F_HALO, L_HALO, 'a.N > 64 && bricks * cdiv(a.N, 128) >= 256')], 'conv3d', 'fwd',
         'bricks of 4x4x8 (x 1 tile of 128)', ['D'], lambda a: a.N > 64 and a.bricks448 * _cdiv(a.N, 128) >= 256,
         [Side(conv(1, 8, 128, 2, 2, 2033), _k([HALO])), Side(conv(1, 8, 128, 2, 2, 2041), _k([HALO]))]),
    # persistent widths: one brick more than workgroups
    Rule('halo_ws_blocks', [(F_HALO, L_HALO, 'ltu_knob_pos("LTU_HALO_WS_BLOCKS", 512)')], 'conv3d', ('fwd', 'dgrad'), 'bricks of 4x4x8', ['D'],
         lambda a: a.bricks448 > 512,
         [Side(conv(1, 32, 32, 2, 2, 4089), _k([WS], [WS])), Side(conv(1, 32, 32, 2, 2, 4097), _k([WS], [WS]))]),
    Rule('halo_wr_blocks', [(F_HALO, L_HALO, 'ltu_knob_pos("LTU_HALO_WR_BLOCKS", a.C > 16 ? 256 : 512)')], 'conv3d', ('fwd', 'dgrad'),
         'bricks of 4x4x8', ['D'], lambda a: a.bricks448 > 512,
         [Side(conv(1, 16, 16, 2, 2, 4089), _k([WR], [WR])), Side(conv(1, 16, 16, 2, 2, 4097), _k([WR], [WR]))]),
    # ---------------------------------------------------------------- conv_halo.hip: launch_conv_wgrad_halo_bf16
    Rule('whalo_N_256', [(F_HALO, L_WH, '!whalo_shape_ok(a.C, a.N)'), (F_HALO, 'whalo_shape_ok', 'N <= 256')], 'conv3d', 'wgrad', 'a.N = Co',
         ['Co'], lambda a: a.N > 256,
         [Side(conv(1, 32, 256, *T), _k(None, None, [WHR])), Side(conv(1, 32, 264, *T), _k(None, None, [TN]))]),
    Rule('whalo_N_8', [(F_HALO, 'whalo_shape_ok', 'N % 8 == 0')], 'conv3d', 'wgrad', 'a.N = Co', ['Co'], lambda a: a.N % 8 != 0,
         [Side(conv(1, 16, 16, *T), _k(None, None, [WH])), Side(conv(1, 16, 12, *T), REFUSED)]),
    # 768 splits of the packed 16-channel kernel on 768 | 769 bricks
    Rule('whalo_blocks', [(F_HALO, 'whalo_blocks', 'ltu_knob_pos("LTU_WHALO_BLOCKS", CC == 16 && !ltu_knob("LTU_WHALO_NO_PACK", 0) ? 768 : 512)')],
         'conv3d', 'wgrad', 'bricks of 4x4x8', ['D'], lambda a: a.bricks448 > 768,
         [Side(conv(1, 16, 16, 2, 2, 6141), _k(None, None, [WH])), Side(conv(1, 16, 16, 2, 2, 6149), _k(None, None, [WH]))]),
    # ---------------------------------------------------------------- conv_halo.hip: launch_conv_class_halo_bf16 (strided dgrad)
    Rule('class_C_32', [(F_HALO, L_CLS, 'a.C % 32')], 'conv3d', 'dgrad', 'a.C = Co', ['Co'], lambda a: a.C % 32 != 0,
         [Side(conv(1, 16, 32, 5, 9, 9, stride=S222), _k(None, [CLS_RING])), Side(conv(1, 16, 48, 5, 9, 9, stride=S222), _k(None, [IG]))], NO_SD),
    _dims('class_H_2', 'H', 2, 3, [(F_HALO, L_CLS, 'a.H < 2')], 'conv3d', 'dgrad', 'a.H = Ho = (H - 1) / 2 + 1',
          conv(1, 16, 32, 3, 9, 9, stride=S222), _k(None, [IG]), _k(None, [CLS_RING]), lambda a: a.Ho < 2, NO_SD),
    _dims('class_W_2', 'W', 2, 3, [(F_HALO, L_CLS, 'a.W < 2')], 'conv3d', 'dgrad', 'a.W = Wo = (W - 1) / 2 + 1',
          conv(1, 16, 32, 5, 3, 9, stride=S222), _k(None, [IG]), _k(None, [CLS_HALO]), lambda a: a.Wo < 2, NO_SD),
    _dims('class_D_2', 'D', 2, 3, [(F_HALO, L_CLS, 'a.D < 2')], 'conv3d', 'dgrad', 'a.D = Do = (D - 1) / 2 + 1',
          conv(1, 16, 32, 5, 9, 3, stride=S222), _k(None, [IG]), _k(None, [CLS_RING]), lambda a: a.Do < 2, NO_SD),
    # ---------------------------------------------------------------- un-embedding: upconv.hip, upconv_ring.hip, updgrad_ring.hip,
    # the weight gradient of conv_halo.hip (launch_upconv_wgrad_class_bf16)
    Rule('up_Ci_4', [(F_UP, 'ltu_upconv_fwd', 'Ci % 4')], 'upconv', 'fwd', 'Ci', ['Ci'], lambda a: a.Ci % 4 != 0,
         [Side(up(1, 8, 32, 2, 5, 3), _k([IG])), Side(up(1, 6, 32, 2, 5, 3), REFUSED)]),
    Rule('up_Co_4', [(F_UP, 'ltu_upconv_fwd', 'Co % 4')], 'upconv', 'fwd', 'Co', ['Co'], lambda a: a.Co % 4 != 0,
         [Side(up(1, 32, 8, 2, 5, 3), _k([CLS_RING])), Side(up(1, 32, 6, 2, 5, 3), REFUSED)]),
    Rule('up_Ci_32', [(F_UR, L_UR, 'Ci % 32'), (F_HALO, L_UPW, '!upw_shape_ok(a.Ci, a.Co, a.H, a.W, a.D)'), (F_HALO, 'upw_shape_ok', 'Ci % 32 == 0')],
         'upconv', ('fwd', 'wgrad'), 'Ci', ['Ci'], lambda a: a.Ci % 32 != 0,
         [Side(up(1, 32, 32, 2, 5, 3), _k([UPRING], None, [UPW_RING])), Side(up(1, 48, 32, 2, 5, 3), _k([IG], None, [TN, UPFOLD]))]),
    Rule('up_Co_8', [(F_HALO, 'upw_shape_ok', 'Co % 8 == 0')], 'upconv', 'wgrad', 'Co', ['Co'], lambda a: a.Co % 8 != 0,
         [Side(up(1, 32, 8, 2, 5, 3), _k(None, None, [UPW_RING])), Side(up(1, 32, 12, 2, 5, 3), REFUSED)]),
    Rule('up_Co_32', [(F_UR, L_UR, 'Co % 32'), (F_UD, L_UD, 'Co % 32')], 'upconv', ('fwd', 'dgrad'), 'Co', ['Co'], lambda a: a.Co % 32 != 0,
         [Side(_UPT, _k([UPRING], [UPDGRAD])), Side(up(1, 128, 40, 2, 5, 3), _k([CLS_RING], [IG]))]),
    Rule('up_Ci_128', [(F_UD, L_UD, 'Ci % 128')], 'upconv', 'dgrad', 'Ci', ['Ci'], lambda a: a.Ci % 128 != 0,
         [Side(_UPT, _k(None, [UPDGRAD])), Side(up(1, 96, 32, 2, 5, 3), _k(None, [IG]))]),
    Rule('up_Ci_512', [(F_UR, L_UR, 'Ci > 512')], 'upconv', 'fwd', 'Ci', ['Ci'], lambda a: a.Ci > 512,
         [Side(up(1, 512, 32, 2, 4, 2), _k([UPRING])), Side(up(1, 544, 32, 2, 4, 2), _k([CLS_RING]))]),
    Rule('up_Co_512', [(F_UD, L_UD, 'Co > 512')], 'upconv', 'dgrad', 'Co', ['Co'], lambda a: a.Co > 512,
         [Side(up(1, 128, 512, 2, 4, 2), _k(None, [UPDGRAD])), Side(up(1, 128, 544, 2, 4, 2), _k(None, [IG]))]),
    # H = 1, D = 1: every halo kernel of the three directions declines (forward: ring, then the class kernel)
    _dims('up_H_2', 'H', 1, 2, [(F_UR, L_UR, 'H < 2'), (F_UD, L_UD, 'H < 2'), (F_HALO, 'upw_shape_ok', 'H >= 2')], 'upconv',
          ('fwd', 'dgrad', 'wgrad'), 'H', _UPT, _UP_GEMM, _UP_RINGS, lambda a: a.H < 2),
    _dims('up_D_2', 'D', 1, 2, [(F_UR, L_UR, 'D < 2'), (F_UD, L_UD, 'D < 2'), (F_HALO, 'upw_shape_ok', 'D >= 2')], 'upconv',
          ('fwd', 'dgrad', 'wgrad'), 'D', _UPT, _UP_GEMM, _UP_RINGS, lambda a: a.D < 2),
    # W = 3: the rings (8 wide bricks) decline, the forward's class kernel (4 wide) takes it
    _dims('up_W_4', 'W', 3, 4, [(F_UR, L_UR, 'W < 4'), (F_UD, L_UD, 'W < 4')], 'upconv', ('fwd', 'dgrad'), 'W', _UPT,
          _k([CLS_HALO], [IG]), _k([UPRING], [UPDGRAD]), lambda a: a.W < 4),
    _dims('up_W_2', 'W', 1, 2, [(F_HALO, 'upw_shape_ok', 'W >= 2')], 'upconv', 'wgrad', 'W', _UPT,
          _k(None, None, [TN, UPFOLD]), _k(None, None, [UPW_RING]), lambda a: a.W < 2),
    # 256 splits (1 chunk x 1 tile) on 256 | 257 coarse bricks of 4x4x8
    Rule('upw_blocks', [(F_HALO, 'upw_blocks', 'ltu_knob_pos("LTU_UPW_BLOCKS", 256)')], 'upconv', 'wgrad', 'coarse bricks of 4x4x8', ['D'],
         lambda a: a.bricks448 > 256,
         [Side(up(1, 32, 32, 2, 2, 2041), _k(None, None, [UPW_RING])), Side(up(1, 32, 32, 2, 2, 2049), _k(None, None, [UPW_RING]))]),
    # 1022 | 1024 fine rows: the 10-bit coordinate fields of the data-gradient ring.  At 511 the last brick's halo reaches fine row
    # (column) 1024 = 8 cdiv(H, 4) (16 cdiv(W, 8)), which no class reads: the kernel marks it padding before the fields could wrap
    _dims('up_2H_1024', 'H', 511, 512, [(F_UD, L_UD, '2 * H >= 1024')], 'upconv', 'dgrad', 'H', up(1, 128, 32, 2, 4, 2),
          _k(None, [UPDGRAD]), _k(None, [IG]), lambda a: 2 * a.H >= 1024),
    _dims('up_2W_1024', 'W', 511, 512, [(F_UD, L_UD, '2 * W >= 1024')], 'upconv', 'dgrad', 'W', up(1, 128, 32, 2, 4, 2),
          _k(None, [UPDGRAD]), _k(None, [IG]), lambda a: 2 * a.W >= 1024),
    _dims('up_2D_1024', 'D', 511, 512, [(F_UD, L_UD, '2 * D >= 1024')], 'upconv', 'dgrad', 'D', up(1, 128, 32, 2, 4, 2),
          _k(None, [UPDGRAD]), _k(None, [IG]), lambda a: 2 * a.D >= 1024),
    # ---------------------------------------------------------------- conv_ring.hip
    # 64 | 65 bricks of 4x8x8 x one 64-column tile
    Rule('ring_split_tiles', [(F_RING, 'conv_ring_split', 'tiles > ltu_knob_pos("LTU_CONV_RING_SPLIT_TILES", 64)'), (F_RING, L_RING, 'ks < 2')],
         'conv3d', 'fwd', 'tiles = bricks of 4x8x8 x 64-column tiles', ['D'], lambda a: a.bricks488 * _cdiv(a.N, 64) > 64,
         [Side(conv(1, 64, 40, 2, 4, 505), _k([RING, FOLD])), Side(conv(1, 64, 40, 2, 4, 513), _k([HALO, FOLD]))]),
    Rule('ring_split_want', [(F_RING, 'conv_ring_split', 'want < 2'), (F_RING, 'conv_ring_splits', 'C < 64')], 'conv3d', 'fwd',
         'want <= nchunk = C / 32, C = Ci', ['Ci'], lambda a: a.C // 32 < 2,
         [Side(conv(1, 32, 64, *T), _k([HALO])), Side(conv(1, 64, 64, *T), _k([RING, FOLD]))]),
    # want = ceil(256 / tiles): 8 ranges of 1 chunk at 36 tiles, 4 ranges of 2 at 37 (8 chunks)
    Rule('ring_split_slots', [(F_RING, 'conv_ring_split', 'ltu_knob_pos("LTU_CONV_RING_SPLIT_SLOTS", 256)')], 'conv3d', 'fwd',
         'tiles = bricks of 4x8x8 x 64-column tiles', ['D'], lambda a: _cdiv(256, a.bricks488 * _cdiv(a.N, 64)) < 8,
         [Side(conv(1, 256, 40, 2, 4, 281), _k([RING, FOLD])), Side(conv(1, 256, 40, 2, 4, 289), _k([RING, FOLD]))]),
    Rule('ring_C_32', [(F_RING, L_RING, 'a.C % 32'), (F_RING, 'conv_ring_splits', 'C % 32')], 'conv3d', 'fwd', 'a.C = Ci', ['Ci'],
         lambda a: a.C % 32 != 0,
         [Side(conv(1, 64, 64, *T), _k([RING, FOLD])), Side(conv(1, 48, 64, *T), _k([HALO, FOLD]))]),
    Rule('ring_C_512', [(F_RING, L_RING, 'a.C > 512')], 'conv3d', 'fwd', 'a.C = Ci', ['Ci'],
         lambda a: a.C > 512,
         [Side(conv(1, 512, 64, 2, 4, 4), _k([RING, FOLD])), Side(conv(1, 544, 64, 2, 4, 4), _k([HALO, FOLD]))]),
    # the same cap seen by a data gradient (and by its workspace query)
    Rule('ring_C_512_dgrad', [(F_RING, 'conv_ring_splits', 'C > 512')], 'conv3d', 'dgrad', 'C = Co', ['Co'], lambda a: a.C > 512,
         [Side(conv(1, 64, 512, 2, 4, 4), _k(None, [RING, FOLD])), Side(conv(1, 64, 544, 2, 4, 4), _k(None, [HALO, FOLD]))]),
    # N = 36: the first generation's 64-column tile with 28 columns of padding; no backward in bf16 (whalo_N_8)
    Rule('ring_N_8', [(F_RING, L_RING, 'a.N % 8'), (F_RING, 'conv_ring_splits', 'N % 8')], 'conv3d', 'fwd', 'a.N = Co', ['Co'],
         lambda a: a.N % 8 != 0,
         [Side(conv(1, 64, 40, *T), _k([RING, FOLD])), Side(conv(1, 64, 36, *T), _k([HALO, FOLD]), backward=False)]),
    Rule('ring_N_32', [(F_RING, L_RING, 'a.N <= 32')], 'conv3d', 'fwd', 'a.N = Co', ['Co'], lambda a: a.N <= 32,
         [Side(conv(1, 64, 32, *T), _k([HALO, FOLD])), Side(conv(1, 64, 40, *T), _k([RING, FOLD]))]),
    # the same rule seen by a conv pair (and by its workspace query): 24 | 32 columns beside a head of 3 padded to 8
    Rule('ring_N_32_pair', [(F_RING, 'conv_ring_splits', 'N <= 32')], 'pair', 'fwd', 'N = Ca + n1', ['Ca'], lambda a: a.N <= 32,
         [Side(pair(1, 64, 24, 3, 8, *T), _k([HALO, FOLD])), Side(pair(1, 64, 32, 3, 8, *T), _k([RING, FOLD]))]),
    # concat 32 + 32 | 16 + 48: forward ring | first generation on 16-channel chunks, and the same for the weight gradient
    Rule('ring_c0_32', [(F_RING, L_RING, 'a.c0 % 32 != 0 && a.c0 != a.C'), (F_WHR, L_WHR, 'a.c0 % 32')], 'conv3d', ('fwd', 'wgrad'),
         'a.c0 = Ci', ['Ci', 'C1'], lambda a: a.c0 % 32 != 0 and a.c0 != a.C,
         [Side(conv(1, 32, 64, *T, C1=32), _k([RING, FOLD], None, [WHR])), Side(conv(1, 16, 64, *T, C1=48), _k([HALO, FOLD], None, [WH]))]),
    _dims('ring_W_4', 'W', 3, 4, [(F_RING, L_RING, 'a.W < 4'), (F_RING, 'conv_ring_splits', 'W < 4')], 'conv3d', ('fwd', 'dgrad'), 'a.W = W',
          conv(1, 64, 64, *T), _k([HALO, FOLD], [HALO, FOLD]), _k([RING, FOLD], [RING, FOLD]), lambda a: a.W < 4),
    # 199 | 200 workgroups (bricks of 4x8x8 x one 64-column tile); 199 is prime and above the split's 64 tiles: first generation
    Rule('ring_min_wg', [(F_RING, L_RING, 'nwg < ltu_knob_pos("LTU_CONV_RING_MIN_WG", 200)')], 'conv3d', 'fwd', 'nwg = bricks of 4x8x8 x tiles',
         ['D'], lambda a: a.bricks488 * _cdiv(a.N, 64) < 200,
         [Side(conv(1, 32, 40, 2, 4, 1585), _k([HALO])), Side(conv(1, 32, 40, 2, 4, 1593), _k([RING]))]),
    # 255 | 256 bricks of 8x8x8 (H = 8: no half-empty brick): the 4-wave | the 8-wave kernel
    Rule('ring_big_min', [(F_RING, L_RING, 'ltu_knob_pos("LTU_CONV_RING_BIG_MIN", 256)')], 'conv3d', 'fwd', 'bricks of 8x8x8 x 64-column tiles',
         ['D'], lambda a: a.bricks888 * _cdiv(a.N, 64) >= 256,
         [Side(conv(1, 32, 40, 8, 4, 2033), _k([RING])), Side(conv(1, 32, 40, 8, 4, 2041), _k([RING]))]),
    # ---------------------------------------------------------------- conv_c16_ring.hip, conv_fc_ring.hip (forward and stride-1 dgrad)
    # 127 | 128 bricks of 4x8x8, ragged in h, w and d
    Rule('c16_bricks_128', [(F_C16, L_C16, 'bricks < 128')], 'conv3d', ('fwd', 'dgrad'), 'bricks of 4x8x8', ['D'], lambda a: a.bricks488 < 128,
         [Side(conv(1, 16, 16, 3, 7, 1010), _k([WR], [WR])), Side(conv(1, 16, 16, 3, 7, 1017), _k([C16], [C16]))]),
    Rule('fc_bricks_128', [(F_FC, L_FC, 'bricks < 128')], 'conv3d', ('fwd', 'dgrad'), 'bricks of 4x8x8', ['D'], lambda a: a.bricks488 < 128,
         [Side(conv(1, 32, 32, 2, 4, 1009), _k([WS], [WS])), Side(conv(1, 32, 32, 2, 4, 1017), _k([FC], [FC]))]),
    Rule('c16_N_8', [(F_C16, L_C16, 'a.N % 8')], 'conv3d', 'fwd', 'a.N = Co', ['Co'], lambda a: a.N % 8 != 0,
         [Side(conv(1, 16, 16, 2, 4, 1017), _k([C16])), Side(conv(1, 16, 12, 2, 4, 1017), _k([WR]), backward=False)]),
    Rule('fc_N_8', [(F_FC, L_FC, 'a.N % 8')], 'conv3d', 'fwd', 'a.N = Co', ['Co'], lambda a: a.N % 8 != 0,
         [Side(conv(1, 32, 32, 2, 4, 1017), _k([FC])), Side(conv(1, 32, 12, 2, 4, 1017), _k([WS]), backward=False)]),
    _dims('c16_W_4', 'W', 3, 4, [(F_C16, L_C16, 'a.W < 4')], 'conv3d', ('fwd', 'dgrad'), 'a.W = W', conv(1, 16, 16, 2, 4, 1017),
          _k([WR], [WR]), _k([C16], [C16]), lambda a: a.W < 4),
    _dims('fc_W_4', 'W', 3, 4, [(F_FC, L_FC, 'a.W < 4')], 'conv3d', ('fwd', 'dgrad'), 'a.W = W', conv(1, 32, 32, 2, 4, 1017),
          _k([WS], [WS]), _k([FC], [FC]), lambda a: a.W < 4),
    Rule('c16_blocks', [(F_C16, L_C16, 'ltu_knob_pos("LTU_C16_RING_BLOCKS", 512)')], 'conv3d', ('fwd', 'dgrad'), 'bricks of 4x8x8', ['D'],
         lambda a: a.bricks488 > 512,
         [Side(conv(1, 16, 16, 2, 4, 4089), _k([C16], [C16])), Side(conv(1, 16, 16, 2, 4, 4097), _k([C16], [C16]))]),
    # 256 | 257 bricks of 4x8x8 and of 4x4x8: the forward ring's width and the weight-gradient ring's 256 splits (1 chunk x 1 tile)
    Rule('fc_blocks', [(F_FC, L_FC, 'ltu_knob_pos("LTU_FC_RING_BLOCKS", 256)'), (F_WHR, L_WHR, 'ltu_knob_pos("LTU_WHALO_RING_BLOCKS", 256)')],
         'conv3d', ('fwd', 'dgrad', 'wgrad'), 'bricks of 4x8x8 (= of 4x4x8 at W = 4)', ['D'], lambda a: a.bricks488 > 256,
         [Side(conv(1, 32, 32, 2, 4, 2041), _k([FC], [FC], [WHR])), Side(conv(1, 32, 32, 2, 4, 2049), _k([FC], [FC], [WHR]))]),
    # ---------------------------------------------------------------- sdgrad_ring.hip (data gradient of stride (2, 2, *))
    Rule('sd_Co_32', [(F_SD, L_SD, 'Co % 32')], 'conv3d', 'dgrad', 'Co', ['Co'], lambda a: a.Co % 32 != 0,
         [Side(conv(1, 16, 32, 5, 9, 9, stride=S222), _k(None, [SD])), Side(conv(1, 16, 48, 5, 9, 9, stride=S222), _k(None, [IG]))]),
    Rule('sd_Co_512', [(F_SD, L_SD, 'Co > 512')], 'conv3d', 'dgrad', 'Co', ['Co'], lambda a: a.Co > 512,
         [Side(conv(1, 8, 512, 4, 8, 4, stride=S222), _k(None, [SD])), Side(conv(1, 8, 544, 4, 8, 4, stride=S222), _k(None, [CLS_RING]))]),
    # 1023 | 1024 output rows: the 10-bit coordinate fields of the ring; beyond them the class kernel (4 wide bricks at Wo = 2)
    _dims('sd_Ho_1024', 'H', 2045, 2047, [(F_SD, L_SD, 'a.Ho >= 1024')], 'conv3d', 'dgrad', 'a.Ho = (H - 1) / 2 + 1',
          conv(1, 16, 32, 4, 4, 4, stride=S222), _k(None, [SD]), _k(None, [CLS_HALO]), lambda a: a.Ho >= 1024),
    _dims('sd_Wo_1024', 'W', 2045, 2047, [(F_SD, L_SD, 'a.Wo >= 1024')], 'conv3d', 'dgrad', 'a.Wo = (W - 1) / 2 + 1',
          conv(1, 16, 32, 4, 4, 4, stride=S222), _k(None, [SD]), _k(None, [CLS_RING]), lambda a: a.Wo >= 1024),
    _dims('sd_Do_1024', 'D', 2045, 2047, [(F_SD, L_SD, 'a.Do >= 1024')], 'conv3d', 'dgrad', 'a.Do = (D - 1) / 2 + 1',
          conv(1, 16, 32, 4, 4, 4, stride=S222), _k(None, [SD]), _k(None, [CLS_HALO]), lambda a: a.Do >= 1024),
    _dims('sd_Do_1024_s221', 'D', 1023, 1024, [(F_SD, L_SD, 'a.Do = (Dl - 1) / sd + 1')], 'conv3d', 'dgrad', 'a.Do = D (stride 1 in d)',
          conv(1, 16, 32, 4, 4, 4, stride=S221), _k(None, [SD]), _k(None, [CLS_HALO]), lambda a: a.Do >= 1024),
    # ---------------------------------------------------------------- gemm.hip: the C ABI's own refusals
    Rule('abi_C0_4', [(F_GEMM, 'conv_fwd_desc', 'C0 % 4 != 0')], 'conv3d', 'fwd', 'C0 = Ci', ['Ci'], lambda a: a.C0 % 4 != 0,
         [Side(conv(1, 8, 16, *T), _k([WR])), Side(conv(1, 6, 16, *T), REFUSED)]),
    Rule('abi_C1_4', [(F_GEMM, 'conv_fwd_desc', 'C1 % 4 != 0')], 'conv3d', 'fwd', 'C1', ['C1'], lambda a: a.C1 % 4 != 0,
         [Side(conv(1, 16, 16, *T, C1=16), _k([WS])), Side(conv(1, 16, 16, *T, C1=6), REFUSED)]),
    Rule('abi_pair_N0_4', [(F_GEMM, 'ltu_conv3d_pair_fwd', 'N0 % 4')], 'pair', 'fwd', 'N0 = Ca', ['Ca'], lambda a: a.N0 % 4 != 0,
         [Side(pair(1, 16, 8, 3, 8, *T), _k([WR])), Side(pair(1, 16, 6, 3, 8, *T), REFUSED)]),
    Rule('abi_pair_N1_4', [(F_GEMM, 'ltu_conv3d_pair_fwd', 'N1 % 4')], 'pair', 'fwd', 'N1 = n1', ['n1'], lambda a: a.N1 % 4 != 0,
         [Side(pair(1, 16, 8, 3, 8, *T), _k([WR])), Side(pair(1, 16, 8, 3, 6, *T), REFUSED)]),
]


# ---------------------------------------------------------------------------------------------- clauses without a rule
_WIDE = 'no case within the size caps: it would need 2^31 bricks or weights (the caps: 70 000 output voxels, 16 M multiply-adds per voxel row)'
_STRIDE = 'ops cannot violate it: the call site fixes the stride - '
_ALIGN = ('pointer alignment: ops only ever passes allocator-aligned tensors; whether the launchers that do not check tolerate a misaligned '
          'base is not known and is not to be found out by running one')
_SWITCH = 'a switch, not a shape rule: tests/test_gpu_conv_paths.py enters the kernels behind it'
_FWD_FIRST = 'ops cannot reach it: the forward of the same shape raises first - '
_CALLER = 'unreachable: its only caller returned on the same condition before - '

_HALO_LD = _STRIDE + 'ltu_conv3d_fwd / _dgrad / _pair_* set lda0 = c0, lda1 = C - c0 (c0 without a concat), ldo0 = n0, ldo1 = N - n0 (n0 without)'

UNSWEPT = [
    # ---- 2^31
    (F_HALO, L_HALO, 'bricks >= (1LL << 31)', _WIDE), (F_HALO, L_WH, 'bricks >= (1LL << 31)', _WIDE),
    (F_HALO, L_CLS, 'bricks >= (1LL << 31)', _WIDE), (F_HALO, L_UPW, 'bricks >= (1LL << 31)', _WIDE),
    (F_RING, L_RING, 'bricks >= (1LL << 31)', _WIDE), (F_RING, L_RING, '(long long)a.N * 27 * a.C >= (1LL << 31)', _WIDE),
    (F_C16, L_C16, 'bricks >= (1LL << 31)', _WIDE), (F_FC, L_FC, 'bricks >= (1LL << 31)', _WIDE), (F_WHR, L_WHR, 'bricks >= (1LL << 31)', _WIDE),
    (F_SD, 'launch_sdgrad', 'rb >= (1LL << 31)', _WIDE), (F_SD, L_SD, '(long long)N * 27 * Co >= (1LL << 31)', _WIDE),
    (F_UD, L_UD, 'rb >= (1LL << 31)', _WIDE), (F_UD, L_UD, '(long long)Ci * 64 * Co >= (1LL << 31)', _WIDE),
    (F_UR, L_UR, 'rb >= (1LL << 31)', _WIDE), (F_UR, L_UR, '(long long)8 * Co * 8 * Ci >= (1LL << 31)', _WIDE),
    (F_UWR, L_UWR, '(long long)6 * a.W * a.D * a.Ci >= (1LL << 31)', _WIDE), (F_UWR, L_UWR, '(long long)16 * a.W * a.D * a.Co >= (1LL << 31)', _WIDE),
    # ---- strides the call sites fix
    *[(F_HALO, L_HALO, t, _HALO_LD) for t in ('a.lda0 % 8', 'a.lda1 % 8', 'a.ldo0 % 4', 'a.ldo1 % 4')],
    *[(F_RING, L_RING, t, _HALO_LD) for t in ('a.lda0 % 8', 'a.lda1 % 8', 'a.ldo0 % 8', 'a.ldo1 % 8')],
    *[(F_C16, L_C16, t, _HALO_LD) for t in ('a.lda0 % 8', 'a.lda1 % 8', 'a.ldo0 % 8', 'a.ldo1 % 8')],
    *[(F_FC, L_FC, t, _HALO_LD) for t in ('a.lda0 % 8', 'a.lda1 % 8', 'a.ldo0 % 8', 'a.ldo1 % 8')],
    *[(f, l, t, _STRIDE + 'ltu_conv3d_wgrad / _pair_wgrad set lda0 = c0, lda1 = C - c0 (c0 without a concat), ldg = N (the pair: N0)')
      for f, l in ((F_HALO, L_WH), (F_WHR, L_WHR)) for t in ('a.lda0 % 8', 'a.lda1 % 8', 'a.ldg % 8')],
    *[(F_HALO, L_CLS, t, _STRIDE + 'ltu_conv3d_dgrad / ltu_upconv_fwd set lda = C, ldo0 = n0, ldo1 = N - n0, wrow = 27 C | 8 C: multiples of 8 after a.C % 32')
      for t in ('a.lda % 8', 'a.ldo0 % 4', 'a.ldo1 % 4', 'a.wrow % 8')],
    (F_HALO, L_CLS, 'a.ent[e].wbase % 8', _STRIDE + 'the entry tables hold wbase = tap * Co | (class * 8 Co + slot) * Ci: multiples of 8 after a.C % 32'),
    (F_HALO, L_CLS, 'a.nent > 64', 'ops cannot violate it: ltu_conv3d_dgrad builds at most 27 entries, ltu_upconv_fwd 64'),
    (F_HALO, L_CLS, 'a.ncls > 8', 'ops cannot violate it: strides are 1 or 2, so at most 8 parity classes'),
    # ---- pointer alignment
    (F_WHR, L_WHR, '((uintptr_t)a.x0 | (uintptr_t)a.x1 | (uintptr_t)a.grad | (uintptr_t)a.grad1) & 15', _ALIGN),
    (F_UWR, L_UWR, '((uintptr_t)a.x | (uintptr_t)a.grad) & 15', _ALIGN),
    # ---- switches
    (F_RING, 'conv_ring_split', 'ltu_knob("LTU_NO_CONV_RING_SPLIT", 0)', _SWITCH),
    (F_RING, 'conv_ring_splits', 'ltu_knob("LTU_NO_CONV_RING", 0)', _SWITCH),
    # ---- the forward of the same shape raises first, so no backward launcher sees the value
    (F_HALO, L_HALO, 'a.n0 % 4', _FWD_FIRST + 'n0 is N in a forward (halo_N_4), C0 in a data gradient (abi_C0_4), N0 in a pair (abi_pair_N0_4)'),
    (F_HALO, L_CLS, 'a.N % 4', _FWD_FIRST + 'N = C0 + C1 of a data gradient (abi_C0_4, abi_C1_4), Co of an un-embedding (up_Co_4)'),
    (F_HALO, L_CLS, 'a.n0 % 4', _FWD_FIRST + 'n0 = C0 of a data gradient (abi_C0_4), Co of an un-embedding (up_Co_4)'),
    (F_HALO, L_WH, 'a.c0 % 8', _FWD_FIRST + 'c0 = C0 (halo_c0_8)'),
    (F_HALO, L_WH, 'a.grad1 != nullptr && (a.gn0 % 8 || a.ldg1 % 8)',
     'ops cannot reach it: gn0 = Ca of a pair, and Ca % 8 != 0 makes the data gradient of the same backward raise first (c0 % 8 of the '
     'implicit GEMM); ldg1 = n1 % 8 != 0 with Ca % 8 == 0 fails N % 8 of whalo_shape_ok (whalo_N_8) before'),
    (F_WHR, L_WHR, 'a.grad1 != nullptr && (a.gn0 % 8 || a.ldg1 % 8)', _CALLER + 'launch_conv_wgrad_halo_bf16'),
    (F_RING, L_RING, 'a.n0 % 8', _FWD_FIRST + 'n0 = N in a forward (ring_N_8 rules it), C0 in a data gradient (halo_c0_8); a pair has N = n0 + n1 '
     'and with n1 % 8 == 0 a.N % 8 fires first'),
    (F_C16, L_C16, 'a.n0 % 8', _FWD_FIRST + 'n0 = N in a forward (c16_N_8 rules it), C0 in a data gradient (halo_c0_8)'),
    (F_FC, L_FC, 'a.n0 % 8', _FWD_FIRST + 'n0 = N in a forward (fc_N_8 rules it), C0 in a data gradient (halo_c0_8)'),
    (F_SD, L_SD, 'N % 8', _FWD_FIRST + 'N = C0 (halo_C_8: C0 % 8 of the implicit GEMM)'),
    (F_UP, 'ltu_upconv_dgrad', 'Ci % 4', _FWD_FIRST + 'up_Ci_4'), (F_UP, 'ltu_upconv_dgrad', 'Co % 4', _FWD_FIRST + 'up_Co_4'),
    (F_UP, 'ltu_upconv_wgrad', 'Ci % 4', _FWD_FIRST + 'up_Ci_4'), (F_UP, 'ltu_upconv_wgrad', 'Co % 4', _FWD_FIRST + 'up_Co_4'),
    (F_GEMM, 'ltu_conv3d_pair_dgrad', 'N0 % 4', _FWD_FIRST + 'abi_pair_N0_4'), (F_GEMM, 'ltu_conv3d_pair_dgrad', 'N1 % 4', _FWD_FIRST + 'abi_pair_N1_4'),
    *[(F_GEMM, f, t, 'an operand without channels is no conv shape: there is no Case, no launch and no reference to compare')
      for f, t in (('conv_fwd_desc', 'C0 <= 0'), ('ltu_conv3d_pair_fwd', 'N0 <= 0'), ('ltu_conv3d_pair_fwd', 'N1 <= 0'),
                   ('ltu_conv3d_pair_dgrad', 'N0 <= 0'), ('ltu_conv3d_pair_dgrad', 'N1 <= 0'))],
    # ---- restated by a launcher that its only caller enters after the same test
    *[(F_RING, L_RING, t, _CALLER + 'launch_conv_halo_bf16 (halo_H_2, halo_D_4)') for t in ('a.H < 2', 'a.D < 4')],
    *[(F_RING, 'conv_ring_splits', t, 'the workspace query alone: launch_conv_halo_bf16 declines the shape before the ring (halo_H_2, halo_D_4), '
       'so the answer only sizes a buffer nobody reads') for t in ('H < 2', 'D < 4')],
    (F_RING, L_RING, 'a.part == nullptr', 'ops cannot violate it: ops._conv_ws allocates the workspace whenever conv_ring_splits says the launcher will split'),
    *[(F_C16, L_C16, t, _CALLER + 'launch_conv_halo_bf16') for t in ('a.C != 16', 'a.N > 32', 'a.c0 % 8', 'a.H < 2', 'a.D < 4')],
    *[(F_FC, L_FC, t, _CALLER + 'launch_conv_halo_bf16') for t in ('a.C != 32', 'a.N > 32', 'a.c0 % 8', 'a.H < 2', 'a.D < 4')],
    *[(f, l, 'a.part != nullptr', 'ops cannot violate it: ltu_conv3d_ws_floats is 0 at C <= 32 and N <= 32 (halo_split returns 1, the implicit '
       "GEMM's K split wants N > 64), so ops._conv_ws passes no workspace") for f, l in ((F_C16, L_C16), (F_FC, L_FC))],
    *[(F_WHR, L_WHR, t, _CALLER + 'launch_conv_wgrad_halo_bf16 (whalo_shape_ok, a.C % 32 == 0, the extents)')
      for t in ('a.C % 32', 'a.N % 8', 'a.N > 256', 'a.H < 2', 'a.W < 2', 'a.D < 4')],
    *[(F_UWR, L_UWR, t, _CALLER + 'launch_upconv_wgrad_class_bf16 (upw_shape_ok)') for t in ('a.Ci % 32', 'a.Co % 8', 'a.H < 2', 'a.W < 2', 'a.D < 2')],
    (F_SD, L_SD, '(sd != 1 && sd != 2)', _CALLER + 'ltu_conv3d_dgrad (LTU_E_ARG)'),
    *[(F_SD, L_SD, t, 'unreachable: (n - 1) / 2 + 1 >= 1 for every extent n >= 1, and a tensor with an empty axis launches nothing')
      for t in ('a.Ho < 1', 'a.Wo < 1', 'a.Do < 1')],
    (F_HALO, 'halo_split', 'want < 2', 'unreachable at the default LTU_HALO_SPLIT_BELOW = 200: blocks < 200 gives ceil(512 / blocks) >= 3, and nchunk >= 2 '
     'passed the clause before; a knob above 512 would be needed, and then 511 | 512 bricks'),
    # ---- over the caps
    (F_UD, L_UD, 'ltu_knob_pos("LTU_UPDGRAD_WIDE_MIN", 160)', 'over the caps: 159 | 160 bricks at H >= 2, W >= 4 and Ci = 128 are 81 984 output voxels '
     '(Ci = 256 halves the bricks and doubles the row: 8.8 G multiply-adds); upconv_dgrad_ring_wide of test_gpu_conv_paths.py enters the wide kernel'),
]


# ---------------------------------------------------------------------------------------------- the seeded random fill
CHANNELS = [8, 16, 24, 32, 40, 48, 64, 96, 128]
ODD_N = [4, 12, 20, 36]                   # N % 8 != 0: a forward only (refusal)
STRIDES = [(1, 1, 1), (2, 2, 1), (2, 2, 2)]
KINDS = ['conv3d', 'conv3d_concat', 'conv3d_head', 'conv3d_oddN', 'pair', 'upconv']


def random_cases(seed, n):
    """n cases over the shapes the bf16 C ABI accepts (refusal() is None): conv3d at the three strides, plain, with a concat split in
    steps of 8, with a padded head (Co 1..8 -> cop 8 / 16 / 32) or with N % 8 != 0 (forward only); the conv pair (n1 8 / 16 / 32);
    the un-embedding.  B 1..3, H, W 1..13, D 1..19, channels of CHANNELS; extents are redrawn until the case is inside the caps
    and one forward stays under RANDOM_MACS multiply-adds.  Kinds and strides go round robin, the rest is drawn from `seed`."""
    g = torch.Generator().manual_seed(seed)

    def r(lo, hi):
        return int(torch.randint(lo, hi + 1, (1,), generator=g))

    def pick(xs):
        return xs[r(0, len(xs) - 1)]

    out = []
    for i in range(n):
        kind = KINDS[i % len(KINDS)]
        stride = STRIDES[(i // len(KINDS)) % 3] if kind in ('conv3d', 'conv3d_concat') else (1, 1, 1)
        if kind == 'pair':
            s = pair(1, pick(CHANNELS), pick(CHANNELS), r(1, 8), pick([8, 16, 32]), 1, 1, 1)
            s['Cb'] = min(s['Cb'], s['n1'])
        elif kind == 'upconv':
            s = up(1, pick(CHANNELS), pick(CHANNELS), 1, 1, 1)
        else:
            c = pick(CHANNELS[1:] if kind == 'conv3d_concat' else CHANNELS)
            c0 = 8 * r(1, c // 8 - 1) if kind == 'conv3d_concat' else c
            co, cop = pick(CHANNELS), None
            if kind == 'conv3d_head':
                co = r(1, 8)
                cop = pick([8, 16, 32])
            elif kind == 'conv3d_oddN':
                co = pick(ODD_N)
            s = conv(1, c0, co, 1, 1, 1, stride=stride, C1=c - c0, cop=cop)
        op = 'conv3d' if kind.startswith('conv3d') else kind
        while True:
            s.update(B=r(1, 3), H=r(1, 13), W=r(1, 13), D=r(1, 19))
            if out_voxels(op, s) <= MAX_VOXELS and out_voxels(op, s) * row_macs(op, s) <= RANDOM_MACS:
                break
        c = Case(f'r{i:03d}_' + case_name(op, s), op, s, {})
        c.backward = kind != 'conv3d_oddN'
        c.kind = kind
        out.append(c)
    return out
