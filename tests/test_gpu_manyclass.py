"""GPU tests of the class-count-templated kernels and of the 5 .. 8-class training path: the head kernels of every class count
1 .. 8 (csrc/pointwise.hip) and the level loss (csrc/loss.hip, both value layouts) against float64 restatements, the final conv and
the level-0 / level-1 conv pairs at the new output widths (each kernel by name, against float64), the whole model against fixtures generated from the reference with dim_output = 5 and 8
(tests/golden/make_golden_manyclass.py), the captured step, the evaluation chain and the refusal of 9 classes.

Shapes are the smallest that reach every path: M = 1031 rows (5 blocks, a tail), the final head on 2 x 3 x 5 x 7 coarse voxels (a grid
tail), the loss on S = 4096 (several blocks of the sums pass), 2052 (four-voxel path with a short last block) and 1003 (one-voxel
path), convs on 6 x 10 x 12 (ragged 4x4x8 and 4x8x8 bricks)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import losses as O_loss
from oracle import net as O_net
from oracle import seedgen
from oracle import step as O_step
from tests import manyclass_common as MC
from tests import test_gpu_conv_paths as CP
from tests.test_gpu_ops import _with_knob

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF16_REL, BF16_ABS = 2.0 ** -8, 1e-5       # a bf16-stored result: rounding of the fp32 value (8 significant bits) + fp32 noise


@pytest.fixture(scope='module')
def ops():
    from lintransunet_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def rel_err(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(np.asarray(b)).double()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def bf16_close(got, ref):
    """element-wise bound of a bf16-stored tensor against its float64 value"""
    got, ref = got.detach().double().cpu(), ref.double()
    return bool(((got - ref).abs() <= BF16_REL * ref.abs() + BF16_ABS * ref.abs().max()).all())


def G(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- mask head

# CP = C: the scalar variants in both dtypes; CP = 4 (C <= 4): one Vec4 per row, in bf16 the 4-wide store path that is not the 16-byte
# one; 8 / 16 / 32: the padded widths of the conv pairs, in bf16 one 16-byte store per 8 columns
HEAD_CASES = [(C, dt, CP) for C in range(1, 9) for dt, cps in ((torch.float32, (C, 8, 16)), (torch.bfloat16, (C, 16, 32)))
              for CP in sorted(set(cps + ((4,) if C <= 4 else ())))]


@pytest.mark.parametrize('C,dtype,CP', HEAD_CASES, ids=[f'C{c}-{str(d)[6:]}-CP{p}' for c, d, p in HEAD_CASES])
def test_head_softmax_wide(ops, C, dtype, CP):
    """tolerances of test_gpu_ops.py::test_softmax_heads (1e-6 on p, 1e-5 on dz); a bf16-stored dz within its rounding.  Every class
    count 1 .. 8; the name dates from when it covered 5 .. 8 only and stays, so that the ids of those cases stay"""
    M = 1031
    g = G(100 + 10 * C + CP)
    z = (torch.randn(M, CP, generator=g) * 2).to(dtype)          # the padding columns hold values too: they must not be read as classes
    zr = z.double().requires_grad_(True)
    pr = torch.softmax(zr[:, :C], dim=1)
    go = torch.randn(M, C, generator=g)
    pr.backward(go.double())
    zd = z.to(DEV).requires_grad_(True)
    pd = ops.head_softmax(zd, C)
    assert pd.shape == (M, C) and pd.dtype == torch.float32
    pd.backward(go.to(DEV))
    torch.cuda.synchronize()
    assert rel_err(pd, pr.detach()) < 1e-6
    assert zd.grad.shape == (M, CP) and zd.grad.dtype == dtype
    if CP > C:
        assert zd.grad[:, C:].float().abs().max().item() == 0.0, 'padding columns of dz must be exactly zero'
    if dtype == torch.float32:
        assert rel_err(zd.grad, zr.grad) < 1e-5
    else:
        assert bf16_close(zd.grad, zr.grad)


@pytest.mark.parametrize('C', [3, 8])
@pytest.mark.parametrize('dtype,CP', [(torch.float32, 8), (torch.bfloat16, 16)], ids=['float32-CP8', 'bfloat16-CP16'])
def test_head_softmax_misaligned_base(ops, C, dtype, CP):
    """contiguous rows whose base lies one element behind a 16-byte boundary take the scalar variants of both passes; the results
    equal those of the vector variants on the aligned copy bit for bit.  (bf16 backward: the aligned run is the 16-byte-store kernel,
    which sums dp p from rounded products where the row kernels run an fma chain - Softmax::grad in csrc/pointwise.hip; the two differ
    in about one bf16 gradient in 10^5, in none of these seeded rows)"""
    from lintransunet_amd import _lib
    M = 1031
    g = G(150 + 10 * C + CP)
    z = (torch.randn(M, CP, generator=g) * 2).to(dtype).to(DEV)
    go = torch.randn(M, C, generator=g).to(DEV)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, device=DEV, dtype=t.dtype)
        buf[1:] = t.flatten()
        v = buf[1:].view(t.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size() and t.data_ptr() % 16 == 0
        return v

    p = ops.head_softmax(z, C)
    assert torch.equal(ops.head_softmax(shifted(z), C), p)
    dz, dzs = torch.full_like(z, 7.0), shifted(torch.full_like(z, 7.0))
    for out in (dz, dzs):
        _lib.call('ltu_head_softmax_bwd', go.data_ptr(), p.data_ptr(), out.data_ptr(), M, C, CP, ops._dt(out),
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert dz[:, :C].float().abs().max().item() > 0 and (CP == C or dz[:, C:].float().abs().max().item() == 0.0)
    assert torch.equal(dzs, dz)


# ---------------------------------------------------------------------------------------------- final head

def _final_cases():
    out = []
    for C in range(1, 9):
        out.append((C, torch.float32, 4 * C))
        out.append((C, torch.bfloat16, (4 * C + 7) // 8 * 8))
        out += [(C, torch.float32, 4 * C + 8), (C, torch.bfloat16, 4 * C + 8)]               # two padded groups behind
    return out


@pytest.mark.parametrize('C,dtype,CP', _final_cases(), ids=[f'C{c}-{str(d)[6:]}-CP{p}' for c, d, p in _final_cases()])
def test_final_softmax(ops, C, dtype, CP):
    B, h, w, D = 2, 3, 5, 7
    g = G(200 + 10 * C + CP)
    z = (torch.randn(B, CP, h, w, D, generator=g) * 2).to(dtype)           # channels-first, padding channels filled
    zr = z.double().requires_grad_(True)
    pr = torch.softmax(O_net.window_unembed(zr[:, :4 * C]), dim=1)         # [B, C, 2h, 2w, D]
    go = torch.randn(pr.shape, generator=g)
    pr.backward(go.double())
    zd = z.permute(0, 2, 3, 4, 1).contiguous().to(DEV).requires_grad_(True)
    pd = ops.final_softmax(zd, C)
    assert pd.shape == (B, 2 * h, 2 * w, D, C)
    pd.backward(go.permute(0, 2, 3, 4, 1).contiguous().to(DEV))
    torch.cuda.synchronize()
    assert (pd.sum(-1) - 1).abs().max().item() <= 1e-5
    assert rel_err(pd.permute(0, 4, 1, 2, 3), pr.detach()) < 1e-6
    dz = zd.grad.permute(0, 4, 1, 2, 3)
    if CP > 4 * C:
        assert dz[:, 4 * C:].float().abs().max().item() == 0.0, 'padding channels of dz must be exactly zero'
    if dtype == torch.float32:
        assert rel_err(dz, zr.grad) < 1e-5
    else:
        assert bf16_close(dz, zr.grad)
    # the channel map on a one-hot logit pattern: channel k = c*4 + kh*2 + kw of coarse voxel (hh, ww) is class c of fine voxel
    # (2 hh + kh, 2 ww + kw); coarse voxel i lights channel i % 4C, every other fine voxel of it is uniform
    n = B * h * w * D
    k = torch.arange(n) % (4 * C)
    zo = torch.full((n, CP), -30.0)
    zo[torch.arange(n), k] = 30.0
    po = ops.final_softmax(zo.view(B, h, w, D, CP).to(dtype).to(DEV), C).cpu()
    bi, hi, wi, di = np.unravel_index(np.arange(n), (B, h, w, D))
    c, kh, kw = (k // 4).numpy(), ((k % 4) // 2).numpy(), (k % 2).numpy()
    lit = po[bi, 2 * hi + kh, 2 * wi + kw, di]                              # [n, C]
    assert torch.equal(lit.argmax(-1), torch.from_numpy(c)) and lit.max(-1).values.min().item() > 0.999
    hot = torch.zeros(B, 2 * h, 2 * w, D, dtype=torch.bool)
    hot[bi, 2 * hi + kh, 2 * wi + kw, di] = True
    assert (po[~hot] - 1.0 / C).abs().max().item() <= 1e-6


# ---------------------------------------------------------------------------------------------- level loss

def _loss_inputs(C, S, seed, B=2):
    g = G(seed)
    if C == 1:
        p = 0.01 + 0.98 * torch.rand(B, S, 1, generator=g)          # a one-class softmax row is constant 1: uniform in (0.01, 0.99) instead
    else:
        p = torch.softmax(torch.randn(B, S, C, generator=g) * 1.5, -1)
    lab = torch.randint(0, C, (B, S), generator=g).to(torch.uint8)
    lab[0, S // 3] = C + 1                                        # a label value that is no class of the prediction
    w = 0.25 + torch.rand(3 + C, generator=g)                      # w_ce, w_bal, w_dice[0 .. C-1], w_fg: all non-zero
    return p, lab, [float(v) for v in w]


def _narrow_dice(w, C):
    """the 5 Dice weights of ops.level_loss (classes 0 .. 3, union) from the C + 1 of ops.level_loss_wide"""
    return w[2:2 + C] + [0.0] * (4 - C) + [w[2 + C]]


def _narrow_live(C):
    """slots of the 8-entry report of ops.level_loss that C classes fill, in the order of the wide report"""
    return [0, 1, 2] + [3 + c for c in range(C)] + [7]


def _loss_reference(p, lab, w, scale):
    """float64 autograd over oracle.losses; the one-hot row of a label >= C is all zero"""
    B, S, C = p.shape
    pr = p.double().requires_grad_(True)
    pred = pr.permute(0, 2, 1)                                                        # [B, C, S]
    t = (lab.long()[:, None, :] == torch.arange(C)[None, :, None]).double()          # [B, C, S]
    ce = O_loss._multi_ce(pred, t)
    # oracle.losses.balanced_dice on a one-hot target
    wc = 1 / (t.sum(dim=2, keepdim=True) + 1e-5) ** 2
    bal = 1 - torch.mean((2 * torch.sum(pred * t * wc, dim=(1, 2)) + 1e-5) / (torch.sum((pred + t) * wc, dim=(1, 2)) + 1e-5))
    dice = [O_loss.dice_class_onehot(pred, t, c) for c in range(C)]
    fg = O_loss.dice_class0_onehot(pred, t)
    total = scale * (w[0] * ce + w[1] * bal + sum(w[2 + c] * dice[c] for c in range(C)) + w[2 + C] * fg)
    total.backward()
    return total.item(), [ce.item(), bal.item()] + [d.item() for d in dice] + [fg.item()], pr.grad


def _check_level_loss(ops, C, S, wide, B=2):
    """either layout of the level loss against float64, with and without the device-resident scale; two calls bit-identical"""
    p, lab, w = _loss_inputs(C, S, 300 + C + S, B)
    for scale in (None, 0.37):
        total_ref, vals_ref, dp_ref = _loss_reference(p, lab, w, 1.0 if scale is None else scale)
        sc = None if scale is None else torch.tensor([scale], device=DEV)
        runs = []
        for _ in range(2):
            pd = p.to(DEV).requires_grad_(True)
            if wide:
                tot, values = ops.level_loss_wide(pd, lab.to(DEV), w[0], w[1], w[2:], sc)
            else:
                tot, values = ops.level_loss(pd, lab.to(DEV), w[0], w[1], _narrow_dice(w, C), sc)
            tot.backward()
            torch.cuda.synchronize()
            assert values.shape == ((C + 4,) if wide else (8,))
            live = values.detach() if wide else values.detach()[_narrow_live(C)]      # the 8-entry report leaves the slots of absent classes unwritten
            runs.append((tot.detach().clone(), live.clone(), pd.grad.clone()))
        (t0, v0, g0), (t1, v1, g1) = runs
        assert torch.equal(t0, t1) and torch.equal(v0, v1) and torch.equal(g0, g1), 'two calls must be bit-identical'
        assert t0.item() == v0[0].item()
        assert abs(t0.item() - total_ref) <= 1e-4 * max(1.0, abs(total_ref)), (t0.item(), total_ref)
        got = v0[1:].cpu().tolist()
        assert np.allclose(got, vals_ref, rtol=0, atol=1e-4), (got, vals_ref)
        assert rel_err(g0, dp_ref) < 1e-4


@pytest.mark.parametrize('S', [4096, 2052, 1003])
@pytest.mark.parametrize('C', [5, 8])
def test_level_loss_wide(ops, C, S):
    """tolerances of test_gpu_ops.py::test_losses_golden on ltu_loss_fwd / ltu_loss_bwd (values 1e-4, gradient 1e-4 of its max)"""
    _check_level_loss(ops, C, S, wide=True)


@pytest.mark.parametrize('S', [2052, 1003])
@pytest.mark.parametrize('C', [1, 2, 3])
def test_level_loss_narrow(ops, C, S):
    """the 9-value layout (ops.level_loss) at the class counts the wide test leaves out, same tolerances: the four-voxel path
    with a short last block (2052; one voxel per thread at C = 1) and the one-voxel path (1003)"""
    _check_level_loss(ops, C, S, wide=False)


WIDE_NARROW = [(C, S, False) for C in (2, 3, 4) for S in (4096, 2052, 1003)] + [(C, 4096, True) for C in (2, 3, 4)]


@pytest.mark.parametrize('C,S,scalar', WIDE_NARROW, ids=[f'C{c}-S{s}' + ('-scalar' if k else '') for c, s, k in WIDE_NARROW])
def test_level_loss_wide_equals_narrow(ops, C, S, scalar):
    """one implementation behind two layouts: for C = 2 .. 4 ltu_loss_wide_fwd / _bwd and ltu_loss_fwd / _bwd agree to the last bit,
    on the four-voxel path, its short last block, the one-voxel path and the one-voxel path forced by LTU_LOSS_SCALAR"""
    p, lab, w = _loss_inputs(C, S, 400 + S)
    sc = torch.tensor([0.61], device=DEV)

    def run(w):
        pa, pb = p.to(DEV).requires_grad_(True), p.to(DEV).requires_grad_(True)
        ta, va = ops.level_loss(pa, lab.to(DEV), w[0], w[1], _narrow_dice(w, C), sc)
        tb, vb = ops.level_loss_wide(pb, lab.to(DEV), w[0], w[1], w[2:], sc)
        ta.backward(); tb.backward()
        torch.cuda.synchronize()
        return ta.detach().clone(), va.clone(), pa.grad, tb.detach().clone(), vb.clone(), pb.grad
    # all weights, then CE and balanced Dice alone: the total is then its first two terms, whose rounding no further term damps
    for wk in (w, w[:2] + [0.0] * (C + 1)):
        ta, va, ga, tb, vb, gb = _with_knob(b'LTU_LOSS_SCALAR', 1, lambda: run(wk)) if scalar else run(wk)
        assert va.shape == (8,) and vb.shape == (C + 4,)
        print(f'[C = {C}, S = {S}, scalar {scalar}] narrow {va.tolist()} wide {vb.tolist()}')
        assert torch.equal(ta, tb) and torch.equal(va[_narrow_live(C)], vb)
        assert torch.equal(ga, gb)


# ---------------------------------------------------------------------------------------------- convs at the new widths

GRID = (6, 10, 12)         # 2 x 3 x 2 bricks of 4x4x8 and 2 x 2 x 2 of 4x8x8, ragged in h, w and d

# bf16: the final conv 16 -> 4C = 20 (cop 24) and 32 (nothing to pad) and the conv pairs with an 8-class head inside their 16 / 32 padding, on
# GRID (below the rings' 128-brick cut-off) and on the 150 ragged bricks of test_gpu_conv_paths.py (what a 128^3 patch runs).  The
# kernels are those the launchers select for these shapes (conv_halo.hip launch_conv_halo_bf16 / launch_conv_wgrad_halo_bf16,
# gemm_bf16.hip launch_nt_bf16): 16 -> N <= 32 forward on conv_c16_ring from 128 bricks on, weights-in-registers kernel below; data
# gradient 24 -> 16 by the implicit GEMM (24 channels: no halo kernel), 32 -> 16 on conv_fc_ring / the weight-stationary kernel;
# weight gradient at 16 input channels by the packed halo kernel.  The pairs have the shapes of every class count (the head is
# padded whatever C is), here with 8 live columns.
CONV_BF16 = [
    CP.Case('final_c5_cop24', 'conv3d', CP.conv(1, 16, 20, *GRID, cop=24),
            {'fwd': [CP.WR16], 'dgrad': [CP.igemm(4, 1, 1, 1, 64)], 'wgrad': [CP.WH_PACK]}),
    CP.Case('final_c8_n32', 'conv3d', CP.conv(1, 16, 32, *GRID),
            {'fwd': [CP.WR16], 'dgrad': [CP.WS32], 'wgrad': [CP.WH_PACK]}),
    CP.Case('final_c5_cop24_ring', 'conv3d', CP.conv(1, 16, 20, *CP.G, cop=24),
            {'fwd': [CP.C16_F], 'dgrad': [CP.igemm(4, 1, 1, 1, 64)], 'wgrad': [CP.WH_PACK]}),
    CP.Case('final_c8_n32_ring', 'conv3d', CP.conv(1, 16, 32, *CP.G),
            {'fwd': [CP.C16_F], 'dgrad': [CP.FC_T], 'wgrad': [CP.WH_PACK]}),
    CP.Case('pair0_head8', 'pair', CP.pair(1, 32, 16, 8, 16, *GRID),
            {'fwd': [CP.WS32], 'dgrad': [CP.WS32]}),
    CP.Case('pair0_head8_ring', 'pair', CP.pair(1, 32, 16, 8, 16, *CP.G),
            {'fwd': [CP.FC_F], 'dgrad': [CP.FC_T]}),
    CP.Case('pair1_head8', 'pair', CP.pair(1, 64, 32, 8, 32, *CP.G),
            {'fwd': [CP.halo(4, 1, 1, 2, 3)], 'dgrad': [CP.halo(4, 1, 1, 2, 3)], 'wgrad': [CP.WH_RING]}),
]


@pytest.mark.parametrize('case', CONV_BF16, ids=[c.name for c in CONV_BF16])
def test_conv_new_widths_bf16(ops, case):
    """run_case of test_gpu_conv_paths.py: float64 reference on bf16-exact operands, padded head columns exactly zero, the named
    kernels witnessed by the profiler"""
    res = CP.run_case(case)
    print(f'[{case.name}] launched {res["seen"]}')
    assert not res['fails'], f'{case.name}: ' + '; '.join(res['fails'])
    miss = CP.missing_kernels(case, res['seen'])
    assert not miss, f'{case.name}: expected kernels did not run: {miss}; launched {res["seen"]}'


def _cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous().float().to(DEV)


def _cf(t):
    return t.detach().double().cpu().permute(0, 4, 1, 2, 3)


IGEMM_F32, WGRAD_F32 = 'igemm_nt_kernel<float, float, 4, 1, 1, 1>', 'wgrad_tn_kernel<float, 1, 4, 1, 1>'


@pytest.mark.parametrize('N', [20, 32])
def test_final_conv_fp32(ops, N):
    """fp32 storage: 16 -> 4C outputs, unpadded; tolerance of test_gpu_ops.py::test_conv3d (1e-4 of the max)"""
    g = G(500 + N)
    H, W, D = GRID
    x = torch.randn(1, 16, H, W, D, generator=g).double()
    w = (torch.randn(N, 16, 3, 3, 3, generator=g) * 0.1).double()
    b = torch.randn(N, generator=g).double()
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    yr = F.conv3d(xr, wr, br, padding=1)
    go = torch.randn(yr.shape, generator=g).double()
    yr.backward(go)
    xd = _cl(x).requires_grad_(True)
    wd, bd = w.float().to(DEV).requires_grad_(True), b.float().to(DEV).requires_grad_(True)
    yd, fwd = CP.launched(lambda: ops.conv3d(xd, wd, bd, cop=N))
    assert yd.shape[-1] == N
    _, bwd = CP.launched(lambda: (yd.backward(_cl(go)), ops.flush_deferred()))
    print(f'[final conv fp32 N = {N}] forward {sorted(fwd)} backward {sorted(bwd)}')
    assert rel_err(_cf(yd), yr.detach()) < 1e-4
    assert rel_err(_cf(xd.grad), xr.grad) < 1e-4
    assert rel_err(wd.grad, wr.grad) < 1e-4 and rel_err(bd.grad, br.grad) < 1e-4
    # fp32 convs are implicit GEMMs (gemm.hip launch_nt / launch_tn): the 32-column instantiations for 20 and for 32 outputs
    assert IGEMM_F32 in fwd and IGEMM_F32 in bwd and WGRAD_F32 in bwd, (fwd, bwd)


@pytest.mark.parametrize('Ci,Ca,n1', [(32, 16, 16), (64, 32, 32)])
@pytest.mark.parametrize('dtype', [torch.float32])
def test_conv_pair_head8_fp32(ops, Ci, Ca, n1, dtype):
    """fp32 conv pair with an 8-class head inside its 16 / 32 padding: padded columns zero, their weight-gradient rows never reach
    the parameter gradients (which have 8 rows); tolerance of test_gpu_ops.py::test_conv3d_pair"""
    Cb = 8
    g = G(600 + Ci)
    H, W, D = GRID
    x = torch.randn(1, Ci, H, W, D, generator=g).double()
    wa, wb = (torch.randn(Ca, Ci, 3, 3, 3, generator=g) * 0.1).double(), (torch.randn(Cb, Ci, 3, 3, 3, generator=g) * 0.1).double()
    ba, bb = torch.randn(Ca, generator=g).double(), torch.randn(Cb, generator=g).double()
    xr, war, wbr, bar, bbr = (t.clone().requires_grad_(True) for t in (x, wa, wb, ba, bb))
    ya, yb = F.conv3d(xr, war, bar, padding=1), F.conv3d(xr, wbr, bbr, padding=1)
    ga, gb = torch.randn(ya.shape, generator=g).double(), torch.randn(yb.shape, generator=g).double()
    torch.autograd.backward([ya, yb], [ga, gb])
    xd = _cl(x).requires_grad_(True)
    pd = [t.float().to(DEV).requires_grad_(True) for t in (wa, ba, wb, bb)]
    prep = ops.conv_pair_prep(*(t.detach() for t in pd), n1, dtype)
    y0, y1 = ops.conv3d_pair(xd, *pd, prep)
    assert y0.shape[-1] == Ca and y1.shape[-1] == n1
    assert y1[..., Cb:].abs().max().item() == 0.0
    g1 = torch.zeros(y1.shape, device=DEV)
    g1[..., :Cb] = _cl(gb)
    torch.autograd.backward([y0, y1], [_cl(ga), g1])
    ops.flush_deferred()
    torch.cuda.synchronize()
    assert rel_err(_cf(y0), ya.detach()) < 1e-4 and rel_err(_cf(y1)[:, :Cb], yb.detach()) < 1e-4
    assert rel_err(_cf(xd.grad), xr.grad) < 1e-4
    assert pd[2].grad.shape == (Cb, Ci, 3, 3, 3) and pd[3].grad.shape == (Cb,)
    for got, ref in zip(pd, (war, bar, wbr, bbr)):
        assert rel_err(got.grad, ref.grad) < 1e-4


# ---------------------------------------------------------------------------------------------- whole model

def _build(C, dtype, dropout=0.0):
    from lintransunet_amd.model import get_model_dict
    cfg = O_net.NetConfig(dim_output=C, **MC.SMALL)
    model = get_model_dict('MaskTransUnet')(cfg.num_layers, cfg.roi_size_list, cfg.is_roi_list, cfg.dim_input, C,
                                            dropout=dropout, act_dtype=dtype)
    model.load_state_dict(seedgen.seeded_params(O_net.param_shapes(cfg), MC.WSEED[C]), strict=True)
    return model.to(DEV).train()


def _inputs(C):
    x = seedgen.seeded_volume((MC.BATCH, 1) + MC.SIZE, MC.WSEED[C] + 1).to(DEV)
    label = MC.seeded_label((MC.BATCH, 1) + MC.SIZE, MC.WSEED[C] + 2, C).to(DEV)
    return x, label


def _step(C, dtype):
    from lintransunet_amd import train
    model = _build(C, dtype)
    x, label = _inputs(C)
    predict, masks = model(x)
    names = MC.criterion_names(C)
    specs = train.level_specs(5, tuple(names), criterion_weight=MC.criterion_weights(C))
    totals, named = train.deep_supervision_loss(predict, masks, label, O_step.dynamic_weights(0), specs=specs)
    torch.autograd.backward(totals, [torch.ones_like(t) for t in totals])
    torch.cuda.synchronize()
    return model, x, label, predict, masks, totals, named, names


def _dice(predict, label, C):
    from lintransunet_amd import losses as L
    return [L.DiceClassLoss(class_index=c)(predict.detach(), label).item() for c in range(C)]


@pytest.mark.parametrize('C', [5, 8])
def test_model_manyclass_fp32(golden_dir, C):
    """tolerances of test_gpu_model.py::test_model_multiclass_fp32"""
    from tests.test_gpu_model import exact_zero_grad
    Gd = np.load(os.path.join(golden_dir, f'model_c{C}_small.npz'))
    model, x, label, predict, masks, totals, named, names = _step(C, torch.float32)
    assert predict.shape == (MC.BATCH, C) + MC.SIZE
    for i, b in enumerate(model.last_boxes):
        assert torch.equal(b.cpu(), torch.from_numpy(Gd[f'box{i}'])), f'box{i}'
    idx = torch.from_numpy(Gd['out_idx'].astype(np.int64))
    assert rel_err(predict.detach().cpu().flatten()[idx], Gd['out_sample']) <= 1e-3
    for i, m in enumerate(masks):
        assert rel_err(m, Gd[f'mask{i}']) <= 1e-3, f'mask{i}'
    total = sum(t.item() for t in totals)
    assert abs(total - float(Gd['total'])) <= 1e-4 * max(1.0, abs(float(Gd['total'])))
    lv = Gd['level_losses']
    for lvl, vals in enumerate(named):
        got = [vals[n].item() for n in names]
        assert np.allclose(got, lv[lvl], rtol=1e-4, atol=1e-5), (lvl, got, lv[lvl])
    dice = _dice(predict, label, C)
    assert np.abs(np.array(dice) - Gd['dice']).max() <= 1e-4, (dice, Gd['dice'])
    norms = dict(zip(Gd['grad_keys'], Gd['grad_norms']))
    sd = dict(model.named_parameters())
    worst = 0.0
    for k, n in norms.items():
        got = sd[k].grad.double().norm().item()
        if exact_zero_grad(k):
            assert got <= 1e-2, k
            continue
        worst = max(worst, abs(got - n) / max(n, 1e-3))
    assert worst <= 1e-2, worst
    # the parameter gradients of the heads have the reference's shapes: no padded row reaches them
    assert model.decode.final_block.weight.grad.shape == (4 * C, 8, 3, 3, 3)
    assert all(mc.weight.grad.shape[0] == C for mc in model.decode.mask_conv_list)


@pytest.mark.parametrize('C', [5, 8])
def test_model_manyclass_bf16(golden_dir, C):
    """tolerances of test_gpu_model.py::test_model_multiclass_bf16"""
    Gd = np.load(os.path.join(golden_dir, f'model_c{C}_small.npz'))
    model, x, label, predict, masks, totals, named, names = _step(C, torch.bfloat16)
    assert predict.shape == (MC.BATCH, C) + MC.SIZE and (predict.sum(1) - 1).abs().max().item() <= 1e-5
    idx = torch.from_numpy(Gd['out_idx'].astype(np.int64))
    ref = torch.from_numpy(Gd['out_sample']).double()
    rel_l2 = ((predict.detach().double().cpu().flatten()[idx] - ref).norm() / ref.norm()).item()
    total = sum(t.item() for t in totals)
    dice = _dice(predict, label, C)
    print(f'[bf16 C = {C}] rel-L2 {rel_l2:.3e}, total {total:.5f} vs {float(Gd["total"]):.5f}, '
          f'worst Dice difference {np.abs(np.array(dice) - Gd["dice"]).max():.3e}')
    assert rel_l2 <= 3e-2
    assert abs(total - float(Gd['total'])) <= 2e-2 * abs(float(Gd['total']))
    assert np.abs(np.array(dice) - Gd['dice']).max() <= 1e-2, (dice, Gd['dice'])
    for k, p in model.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all(), k


def test_graphed_step_8_classes():
    """train.GraphedStep at C = 8 (small configuration, bf16): every gradient against the eager train_step, under the comparison of
    tests/test_gpu_structure.py"""
    from lintransunet_amd import train
    from tests.test_gpu_structure import _compare, _grads
    C = 8
    model = _build(C, torch.bfloat16)
    red = train.GradReducer(model, bucket_mb=32.0, unused=train.UNUSED_PARAMETERS)
    x, label = _inputs(C)
    w = O_step.dynamic_weights(0)
    specs = train.level_specs(5, tuple(MC.criterion_names(C)), criterion_weight=MC.criterion_weights(C))
    for _ in range(2):
        red.zero_grad()
        tot_e, _ = train.train_step(model, x, label, w, specs=specs, reducer=red)
    torch.cuda.synchronize()
    g_eager, tot_e = _grads(model), [t.item() for t in tot_e]
    assert sum(v.abs().sum().item() for v in g_eager.values()) > 0 and all(np.isfinite(tot_e))
    step = train.GraphedStep(model, x, label, w, red, specs=specs)
    for rep in range(2):
        for f in red.flat:
            f.fill_(float('nan'))
        tot_s, _ = step(x, label)
        torch.cuda.synchronize()
        assert [t.item() for t in tot_s] == tot_e
        _compare(_grads(model), g_eager, f'C = 8 replay {rep}: captured step vs eager')


def test_eval_chain_8_classes():
    """eval forward, sliding-window inference (plain average of one-hot windows; Gaussian-weighted softmax) and class_metrics with
    the label map, at C = 8"""
    from lintransunet_amd import infer
    C = 8
    model = _build(C, torch.bfloat16).eval()
    x, _ = _inputs(C)
    with torch.no_grad():
        onehot = model(x)
        probs = model(x, probs=True)
    assert onehot.shape == probs.shape == (MC.BATCH, C) + MC.SIZE
    assert (probs.sum(1) - 1).abs().max().item() <= 1e-5
    assert torch.equal(onehot, F.one_hot(probs.argmax(1), C).movedim(-1, 1).float())
    vol = seedgen.seeded_volume((1, 1, 48, 48, 24), 811).to(DEV)
    lab = MC.seeded_label((1, 1, 48, 48, 24), 812, C).to(DEV)
    with torch.no_grad():
        votes = infer.sliding_window_inference(vol, (32, 32, 16), 2, model, overlap=0.5)
        blend = infer.sliding_window_inference(vol, (32, 32, 16), 2, lambda t: model(t, probs=True), overlap=0.5, mode='gaussian')
    for out in (votes, blend):
        assert out.shape == (1, C, 48, 48, 24) and torch.isfinite(out).all()
        assert (out.sum(1) - 1).abs().max().item() <= 1e-5
        res = infer.class_metrics(out, lab, return_label_map=True)
        lm = res['label_map'] if isinstance(res, dict) else res[-1]
        assert lm.dtype == torch.uint8 and torch.equal(lm.long(), out.argmax(1))


def test_nine_classes_are_refused():
    """dim_output = 9 constructs; its first forward raises LtuError from the mask head, and the device is left in order"""
    from lintransunet_amd import _lib
    from lintransunet_amd.model import get_model_dict
    cfg = O_net.NetConfig(dim_output=9, **MC.SMALL)
    model = get_model_dict('MaskTransUnet')(cfg.num_layers, cfg.roi_size_list, cfg.is_roi_list, 1, 9, dropout=0.0).to(DEV).train()
    x = seedgen.seeded_volume((1, 1, 32, 32, 32), 5).to(DEV)
    with pytest.raises(_lib.LtuError, match='LTU_E_SHAPE|ltu_head_softmax_fwd'):
        model(x)
    torch.cuda.synchronize()
    _, after = CP.launched(lambda: None)
    assert not after, after
