"""CPU side of the packed-view tests (bucket_common.py): the guard bands see a stray store, the part-1 table meets its obligations,
the float64 closed forms agree with torch autograd, the weight-prep restatement agrees with plain torch permute / pad / cat
expressions, and the registration-order census of the benchmark's channels gives 22 / 24 / 24 / 18 gradient views off 16-byte
alignment for 2 / 3 / 5 / 8 classes."""
import glob
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bucket_common as BC
from tests import test_gpu_conv_paths as CP
from tests import test_gpu_stream_paths as SP
from tests import test_gpu_token_paths as TP

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lintransunet_amd', 'csrc')


# ---------------------------------------------------------------------------------------------- the packed view

@pytest.mark.parametrize('residue', BC.RESIDUES)
def test_packed_view_layout_and_guards(residue):
    g = torch.Generator().manual_seed(residue)
    n = 10
    old = torch.randn(n, generator=g)
    v = BC.packed(n, residue, old, device='cpu')
    pk = v.pack
    assert pk.buf.numel() == 64 + residue + n + 64 and pk.buf.data_ptr() % 16 == 0
    assert v.data_ptr() == pk.buf.data_ptr() + 4 * (64 + residue) and (v.data_ptr() % 16) // 4 == residue
    assert torch.equal(v, old) and pk.starts() == [residue] and not pk.guard_fails()
    assert len(set(pk.buf[:64 + residue].tolist())) == 64 + residue and len(set(pk.buf[-64:].tolist())) == 64      # one value per position
    v += 1.0                                                          # the body is the kernel's to write
    assert not pk.guard_fails()
    for off in (-1, n, -(64 + residue), n + 63):                      # one float in front, behind, and at the far ends of the bands
        keep = pk.buf[64 + residue + off].item()
        pk.buf[64 + residue + off] = 0.5
        assert len(pk.guard_fails()) == 1 and str(off) in pk.guard_fails()[0]
        pk.buf[64 + residue + off] = keep
        assert not pk.guard_fails()
    # a read-modify-write across the edge: seen unless it adds nothing to the sentinel (the documented limit)
    pk.buf[64 + residue + n] += 1e24
    assert pk.guard_fails()
    pk.buf[64 + residue + n] -= 1e24
    pk.buf[64 + residue + n] += 0.0
    pk.buf[64 + residue - 1] += 1.0                                   # below half an ulp of 1e30: not seen either
    assert not pk.guard_fails()


def test_packed_group_is_back_to_back():
    sizes = [5 * 16 * 27, 5, 3, 1, 16]
    olds = [torch.full((n,), float(i)) for i, n in enumerate(sizes)]
    pk = BC.Packed(sizes, 3, olds, device='cpu')
    assert pk.starts() == [3, 3, 0, 3, 0]
    assert torch.equal(pk.body, torch.cat(olds))
    for a, b in zip(pk.views, pk.views[1:]):
        assert a.data_ptr() + 4 * a.numel() == b.data_ptr()


# ---------------------------------------------------------------------------------------------- the table

def test_table_meets_its_obligations():
    assert len({c.name for c in BC.CASES}) == len(BC.CASES)
    # every entry point of the list, every sibling case the issue names (Case() fails on an unknown sibling)
    assert {c.entry for c in BC.CASES} == set(BC.ENTRY_POINTS)
    want = {'ltu_conv3d_wgrad': {'conv_wgrad_reduce64', 'whalo_ring_concat', 'halo_deep_split', 'conv_ring_split', 'sdgrad_ring_222',
                                 'class_gemm_221', 'c16_ring_head', 'class_head_3x64'},
            'ltu_conv3d_pair_wgrad': {'whalo_ring_pair'},
            'ltu_upconv_wgrad': {'upconv_class_ring', 'upconv_class_halo', 'upconv_class_gemm'},
            'ltu_linear_wgrad': {'lin_qkv128_ragged', 'lin_qkv256', 'gate_proj_k16', 'gate_proj_k32'},
            'ltu_linear_wgrad_group': {'wgroup_fold_long_runs', 'wgroup_direct', 'wgroup_no_direct', 'wgroup_off', 'wgrad_deferred_batch',
                                       'wgroup_fat'},
            'ltu_layernorm_bwd': {'ln128_drop', 'ln256_dy2'},
            'ltu_layer_tail_bwd': {'tail128_ragged_drop', 'tail256_attn_drop'},
            'ltu_dwconv_bwd': {'dw_c8_long_drop', 'dw_c72_atomics_drop'},
            'ltu_gate_bwd': {'gate_c8', 'gate_c32_atomics', 'gate_c256'}}
    assert {e: {c.name for c in BC.CASES if c.entry == e} for e in BC.ENTRY_POINTS} == want
    for c in BC.CASES:
        # shape and knobs are the sibling's, untouched
        if c.sib is not None:
            assert c.shape is c.sib.shape and c.knobs == c.sib.knobs, c.name
        # where the sibling names weight-gradient kernels, this table names them too
        if c.sib_ref is not None and c.sib_ref[0] == 'conv':
            assert set(c.sib.kernels.get('wgrad', ())) <= set(c.kernels), c.name
        if c.op in ('wgrad', 'dw', 'gate', 'ln') and c.sib is not None:
            sib_bwd = set(c.sib.kernels.get('bwd', ())) - {'reduce_parts_kernel<4>'}      # bucket views defer that fold: reduce_batch
            assert sib_bwd <= set(c.kernels), (c.name, sib_bwd - set(c.kernels))
        # the cases whose destinations are reached through atomics are the ones compared by the fp32-sum bound: the depthwise conv
        # without a workspace, and every gate case (gate_fold_kernel adds the samples' sums with atomicAdd: B = 2 orders)
        assert (c.rule == 'sum') == (c.op == 'gate' or (c.op == 'dw' and not c.shape['ws'])), c.name
        if c.op == 'gate':
            assert c.shape['B'] > 1
        assert c.kernels and all(sz > 0 for _, sz in BC.dest_sizes(c))
    # every residue meets a destination whose length is no multiple of 4, and one that is
    for odd in (True, False):
        met = set()
        for c in BC.CASES:
            sizes = [n for _, n in BC.dest_sizes(c)]
            for res in BC.RESIDUES:
                off = res
                for n in sizes:
                    if (n % 4 != 0) == odd:
                        met.add(off % 4)
                    off += n
        assert met == set(BC.RESIDUES), (odd, met)
    # the shapes the issue states
    sizes = {c.name: dict(BC.dest_sizes(c)) for c in BC.CASES}
    assert sizes['c16_ring_head'] == {'dw': 5 * 16 * 27, 'db': 5}
    assert sizes['class_head_3x64'] == {'dw': 3 * 64 * 27, 'db': 3}
    assert sizes['dw_c72_atomics_drop']['dw'] == 72 * 27
    assert sizes['whalo_ring_pair']['dwb'] == 3 * 64 * 27 and len(sizes['whalo_ring_pair']) == 4
    assert [sizes[f'gate_c{c}']['dpsi_b'] for c in (8, 256)] == [1, 1] and list(sizes['gate_c8']) == ['dpsi_w', 'dpsi_b', 'neighbour']
    assert len(sizes['lin_qkv128_ragged']) == 6 and len(sizes['tail128_ragged_drop']) == 10
    gates = [c.shape for c in BC.CASES if c.name.startswith('gate_proj')]
    assert [(s['M'], s['N'], s['K']) for s in gates] == [(426, 16, 16), (426, 16, 32)]
    fat = next(c for c in BC.CASES if c.name == 'wgroup_fat')
    assert (fat.shape['M'], fat.shape['d']) == (2048, 128) and fat.knobs == {'LTU_WGROUP_FAT': 1}


def test_named_kernels_exist_in_sources():
    src = ''.join(open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, '*.hip'))))
    for k in sorted(BC.named_kernels() | {TP.WG, TP.FOLD}):
        fn = k.split('<')[0]
        assert re.search(r'__global__\s+void\s+(?:__launch_bounds__\([^()]*(?:\([^()]*\))?[^()]*\)\s+)?' + re.escape(fn) + r'\s*\(', src), \
            f'{k}: no __global__ {fn} in lintransunet_amd/csrc'


def test_old_values_are_seeded_and_of_gradient_size():
    c = next(c for c in BC.CASES if c.name == 'lin_qkv256')
    a, b = BC.olds(c), BC.olds(c)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and [t.numel() for t in a] == [n for _, n in BC.dest_sizes(c)]
    assert 0.5 * math.sqrt(2080) < a[0].std().item() < 2 * math.sqrt(2080) and a[0].abs().min().item() > 0


# ---------------------------------------------------------------------------------------------- closed forms against autograd

def test_linear_reference_agrees_with_autograd():
    g = torch.Generator().manual_seed(1)
    M, K, N, nw = 37, 16, 24, 3
    x, go = torch.randn(M, K, generator=g, dtype=torch.float64), torch.randn(M, N, generator=g, dtype=torch.float64)
    W = [torch.randn(N // nw, K, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(nw)]
    b = [torch.randn(N // nw, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(nw)]
    F.linear(x, torch.cat(W), torch.cat(b)).backward(go)
    for (dw, db, mag), w, v in zip(BC.linear_wgrad_ref(go, x, nw), W, b):
        assert torch.allclose(dw, w.grad, rtol=1e-12, atol=1e-12) and torch.allclose(db, v.grad, rtol=1e-12, atol=1e-12)
        assert (mag >= db.abs() - 1e-12).all() and mag.shape == db.shape


def test_layernorm_reference_agrees_with_autograd():
    g = torch.Generator().manual_seed(2)
    M, d = 29, 32
    z, G = torch.randn(M, d, generator=g, dtype=torch.float64) + 0.7, torch.randn(M, d, generator=g, dtype=torch.float64)
    gamma = (1 + 0.2 * torch.randn(d, generator=g, dtype=torch.float64)).requires_grad_(True)
    beta = torch.randn(d, generator=g, dtype=torch.float64).requires_grad_(True)
    F.layer_norm(z, (d,), gamma, beta, TP.LN_EPS).backward(G)
    mean, rstd = TP._ln_stats(z)
    dg, db, mg, mb = BC.ln_param_ref(G, z, mean, rstd)
    assert torch.allclose(dg, gamma.grad, rtol=1e-12, atol=1e-12) and torch.allclose(db, beta.grad, rtol=1e-12, atol=1e-12)
    assert (mg >= dg.abs() - 1e-12).all() and (mb >= db.abs() - 1e-12).all()


def test_conv_reference_of_the_added_head_shape():
    """the conv references are test_gpu_conv_paths.reference (autograd of F.conv3d in float64): its layout is the parameter's"""
    c = next(c for c in BC.CASES if c.name == 'class_head_3x64')
    r = CP.reference(CP.Case('bucket_cpu_' + c.name, c.op, c.shape, {}))
    assert [t.numel() for t in (r['dw'][0], r['db'][0])] == [n for _, n in BC.dest_sizes(c)]
    assert torch.allclose(r['db'][0], r['go'].sum((0, 2, 3, 4)), rtol=1e-12, atol=1e-12)
    assert (r['go'].abs().sum((0, 2, 3, 4)) >= r['db'][0].abs()).all()


def test_adamw_reference_agrees_with_torch():
    g = torch.Generator().manual_seed(3)
    p0, gr = torch.randn(50, generator=g, dtype=torch.float64), torch.randn(50, generator=g, dtype=torch.float64)
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    m, v, q = torch.zeros(50, dtype=torch.float64), torch.zeros(50, dtype=torch.float64), p0.clone()
    for step in (1, 2, 3):
        p.grad = gr * step
        opt.step()
        q, m, v, _ = BC.adamw_ref(q, gr, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-2, step, float(step))
        assert torch.allclose(q, p.detach(), rtol=1e-12, atol=1e-14), step
    e = BC.adamw_ref(q, gr, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 4, 1.0, ema=p0, decay=0.9)
    assert torch.allclose(e[3], 0.9 * p0 + 0.1 * e[0])


# ---------------------------------------------------------------------------------------------- weight prep against plain torch

def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _ref(kind, src, R_, C_, p0=0, p1=0, pad=0, extent=None):
    n = extent if extent is not None else BC.wprep_size(kind, R_, C_, p0, p1, pad)
    val, wr = BC.wprep_ref(kind, src.numpy(), R_, C_, p0, p1, pad, n)
    return torch.from_numpy(val), torch.from_numpy(wr)


def test_bf16_rounding_is_torchs():
    x = torch.cat([_rand(4096, seed=5) * torch.exp(_rand(4096, seed=6) * 4), torch.tensor([1.00390625, 1.01171875, -1.00390625, 0.0])])
    want = x.bfloat16().view(torch.int16).numpy().view(np.uint16)          # the last four: ties, to even
    assert (BC.bf16_bits(x.numpy()) == want).all()


def test_weight_prep_dense_kinds_agree_with_torch():
    for R_, C_ in ((128, 128), (96, 64), (96, 40)):
        w = _rand(R_, C_, seed=R_ + C_)
        val, wr = _ref(0, w, R_, C_)
        assert wr.all() and torch.equal(val, w.reshape(-1))
        val, wr = _ref(4, w, R_, C_)
        assert wr.all() and torch.equal(val, w.reshape(-1))
        # transpose into columns [p1, p1 + R) of a [C][p0] operand: cat(W)^T of a q | k | v group is three of these side by side
        p0, p1 = 3 * R_, R_
        val, wr = _ref(1, w, R_, C_, p0, p1, extent=C_ * p0)
        want = torch.zeros(C_, p0)
        want[:, p1:p1 + R_] = w.T
        mask = torch.zeros(C_, p0, dtype=torch.bool)
        mask[:, p1:p1 + R_] = True
        assert torch.equal(wr.reshape(C_, p0), mask) and torch.equal(val.reshape(C_, p0), want)
        if C_ % 32 == 0:
            # fragment order: output tile ct (32 outputs), reduction step ks (16 terms), lane l = 32 hi + lo, 8 values j:
            # output ct * 32 + lo, term ks * 16 + 8 hi + j
            for kind, W in ((8, w), (9, w.T.contiguous())):
                O, K = W.shape
                want = W.reshape(O // 32, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).reshape(-1)
                val, wr = _ref(kind, w, R_, C_)
                assert wr.all() and torch.equal(val, want), (kind, R_, C_)


def test_weight_prep_conv_kinds_agree_with_torch():
    Co, Ci, CoP, CiP = 5, 12, 8, 16
    w = _rand(Co, Ci, 3, 3, 3, seed=7)
    w27 = F.pad(w.reshape(Co, Ci, 27), (0, 0, 0, CiP - Ci, 0, CoP - Co))          # zero padded [CoP][CiP][27]
    val, wr = _ref(2, w, Co, Ci, CoP, CiP)
    assert wr.all() and torch.equal(val, w27.permute(0, 2, 1).reshape(-1))          # [CoP][27][CiP]
    val, wr = _ref(3, w, Co, Ci, CoP, CiP)
    assert wr.all() and torch.equal(val, w27.permute(1, 2, 0).reshape(-1))          # [CiP][27][CoP]
    assert (val.reshape(CiP, 27, CoP)[Ci:] == 0).all() and (val.reshape(CiP, 27, CoP)[:, :, Co:] == 0).all()
    # kind 7: the members of a conv pair side by side in the columns of wd [Ci][27][n0 + n1], the second padded to n1
    wa, wb, n0, n1 = _rand(8, 16, 3, 3, 3, seed=8), _rand(3, 16, 3, 3, 3, seed=9), 8, 16
    pack_d = lambda t, cop: F.pad(t.reshape(t.shape[0], 16, 27), (0, 0, 0, 0, 0, cop - t.shape[0])).permute(1, 2, 0)      # noqa: E731
    want = torch.cat([pack_d(wa, n0), pack_d(wb, n1)], -1).reshape(-1)
    va, ma = _ref(7, wa, 8, 16, n0 + n1, 16, (0 << 16) | n0, extent=want.numel())
    vb, mb = _ref(7, wb, 3, 16, n0 + n1, 16, (n0 << 16) | n1, extent=want.numel())
    assert not (ma & mb).any() and (ma | mb).all() and torch.equal(va + vb, want)
    # a padded bias: the first C floats
    val, wr = _ref(4, _rand(3, seed=10), 1, 3, extent=8)
    assert wr.tolist() == [True] * 3 + [False] * 5


def test_weight_prep_subpixel_kinds_agree_with_torch():
    """against test_gpu_conv_paths._subpixel_weights (fp32 tap sums per parity class and slot, written with torch indexing)"""
    Co, Ci = 4, 6
    w = _rand(Co, Ci, 3, 3, 3, seed=11)
    weff = CP._subpixel_weights(w.double())                           # [8 classes][Co][Ci][2][2][2], rounded to bf16
    wf = weff.permute(0, 1, 3, 4, 5, 2).reshape(8, Co, 8, Ci)         # [class][Co][slot][Ci]
    val, wr = _ref(5, w, Co, Ci, Co, Ci)
    assert wr.all() and torch.equal(val.bfloat16().double().reshape(8, Co, 8, Ci), wf)
    val, wr = _ref(6, w, Co, Ci, Co, Ci)
    assert wr.all() and torch.equal(val.bfloat16().double().reshape(Ci, 64, Co), wf.permute(3, 0, 2, 1).reshape(Ci, 64, Co))
    # zero padding
    val, _ = _ref(5, w, Co, Ci, 8, 8)
    v = val.reshape(8, 8, 8, 8)
    assert (v[:, Co:] == 0).all() and (v[..., Ci:] == 0).all() and torch.equal(v[:, :Co, :, :Ci].bfloat16().double(), wf)


def test_chunk_list_is_the_weight_stores():
    recs = [(0, 128, 128, 0, 0, 0), (2, 5, 12, 8, 16, 0), (7, 3, 16, 24, 16, (8 << 16) | 16), (5, 32, 64, 32, 64, 0), (4, 1, 3, 0, 0, 0)]
    ch = BC.chunk_list(recs)
    assert [sum(1 for i, _ in ch if i == k) for k in range(5)] == [4, 1, 2, 32, 1]


# ---------------------------------------------------------------------------------------------- census

def _cpu_reducer(classes):
    from lintransunet_amd import train
    from lintransunet_amd.model import get_model_dict
    from oracle import net as O_net
    cfg = O_net.NetConfig(dim_output=classes)
    assert cfg.num_layers == [16, 32, 64, 128, 256]
    m = get_model_dict('MaskTransUnet')(cfg.num_layers, cfg.roi_size_list, cfg.is_roi_list, 1, classes, dropout=0.0, act_dtype=torch.bfloat16)
    return m, train.GradReducer(m, bucket_mb=32.0, unused=train.UNUSED_PARAMETERS)


@pytest.mark.parametrize('classes,want', [(2, 22), (3, 24), (5, 24), (8, 18)])
def test_registration_order_census(classes, want):
    m, red = _cpu_reducer(classes)
    rows = BC.census(m, red)
    off = [r for r in rows if r[2]]
    assert len(rows) == 600 and len(off) == want, (len(rows), len(off))
    assert {r[2] for r in off} == {1, 2, 3}
    fams = BC.census_by_family(rows)
    assert set(fams) <= set(BC.ENTRY_POINTS) and sum(n for d in fams.values() for n in d.values()) == 600
    if classes == 3:
        by_name = {r[0]: r for r in rows}
        assert by_name['decode.att_conv_list.3.W_g.0.weight'][2:] == (1, 128 * 256)
        assert by_name['decode.mask_conv_list.3.weight'][2:] == (3, 3 * 256 * 27)
        # the one-element psi biases and the C-element head biases are what shifts the views behind them
        assert all(by_name[f'decode.att_conv_list.{i}.psi.0.bias'][3] == 1 for i in range(4))


def test_family_of_every_parameter():
    m, _ = _cpu_reducer(3)
    want = {'decode.att_conv_list.0.psi.0.bias': 'ltu_gate_bwd', 'decode.att_conv_list.2.W_g.0.weight': 'ltu_linear_wgrad',
            'decode.mask_conv_list.1.weight': 'ltu_conv3d_pair_wgrad', 'decode.block_list.0.conv1.bias': 'ltu_conv3d_pair_wgrad',
            'decode.block_list.0.conv2.weight': 'ltu_conv3d_wgrad', 'encode.block_list.0.conv1.weight': 'ltu_conv3d_wgrad',
            'decode.final_block.weight': 'ltu_conv3d_wgrad',
            'decode.bridge_list.1.transformer.up_embed.module_list.0.1.weight': 'ltu_upconv_wgrad',
            'decode.bridge_list.1.transformer.down_embed.module_list.0.0.weight': 'ltu_conv3d_wgrad',
            'decode.bridge_list.1.transformer.pos_encoder.proj.weight': 'ltu_dwconv_bwd',
            'decode.bridge_list.4.transformer.layers.0.self_attn.linears.3.bias': 'ltu_linear_wgrad_group',
            'decode.bridge_list.4.transformer.layers.0.linear2.weight': 'ltu_linear_wgrad_group',
            'decode.bridge_list.1.transformer.layers.0.layer_norm1.weight': 'ltu_layer_tail_bwd'}
    names = {n for n, _ in m.named_parameters()}
    for k, fam in want.items():
        assert k in names and BC.family(k) == fam, k
    assert {BC.family(n) for n in names} <= set(BC.ENTRY_POINTS)
