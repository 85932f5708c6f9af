"""GPU parity tests, kernel by kernel: every C-ABI op (through its autograd wrapper) against the CPU oracle /
plain torch fp32 on the same seeded inputs, forward and backward.  Tolerances are stated per test:
fp32 storage 1e-4..1e-3 relative to the tensor's max (fp32 accumulation order differs), bf16 storage 2e-2.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import losses as O_loss          # noqa: E402
from oracle import net as O_net              # noqa: E402
from oracle import roi as O_roi              # noqa: E402
from oracle import seedgen                   # noqa: E402


@pytest.fixture(scope='module')
def ops():
    from lintransunet_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


DEV = 'cuda'


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def to_cl(t, dtype=torch.float32):
    """reference layout [B,C,H,W,D] (cpu) -> channels-last cuda tensor [B,H,W,D,C]"""
    return t.permute(0, 2, 3, 4, 1).contiguous().to(DEV, dtype)


def from_cl(t):
    return t.detach().float().cpu().permute(0, 4, 1, 2, 3)


def G(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- linear
@pytest.mark.parametrize('M,K,N,nw', [(300, 64, 96, 3), (1000, 128, 128, 1), (77, 32, 32, 1), (513, 256, 768, 3), (130, 64, 32, 1)])
def test_linear(ops, M, K, N, nw):
    g = G(1)
    x = torch.randn(M, K, generator=g)
    ws = [torch.randn(N // nw, K, generator=g) * 0.1 for _ in range(nw)]
    bs = [torch.randn(N // nw, generator=g) for _ in range(nw)]
    go = torch.randn(M, N, generator=g)
    xr = x.clone().requires_grad_(True)
    wr = [w.clone().requires_grad_(True) for w in ws]
    br = [b.clone().requires_grad_(True) for b in bs]
    yr = F.linear(xr, torch.cat(wr), torch.cat(br))
    yr.backward(go)
    xd = x.to(DEV).requires_grad_(True)
    wd = [w.to(DEV).requires_grad_(True) for w in ws]
    bd = [b.to(DEV).requires_grad_(True) for b in bs]
    yd = ops.linear(xd, wd, bd)
    yd.backward(go.to(DEV))
    assert rel_err(yd, yr) < 1e-4
    assert rel_err(xd.grad, xr.grad) < 1e-4
    for a, b in zip(wd, wr):
        assert rel_err(a.grad, b.grad) < 1e-4
    for a, b in zip(bd, br):
        assert rel_err(a.grad, b.grad) < 1e-4


@pytest.mark.parametrize('M,K,N', [(70003, 16, 16), (65536, 32, 16), (66001, 64, 64), (65599, 128, 32)])
def test_linear_small_accumulate(M, K, N):
    """ltu_linear_fwd with the accumulating epilogue on the few-channel streaming kernel (the attention gate's dskip += du1 . Wx):
    y += x W^T against torch on the bf16-rounded operands"""
    from lintransunet_amd import _lib
    from lintransunet_amd.ops import _p, _ptr_array, _s
    g = G(55)
    x = torch.randn(M, K, generator=g).bfloat16().to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.2).bfloat16().to(DEV)
    y0 = torch.randn(M, N, generator=g).bfloat16().to(DEV)
    y = y0.clone()
    _lib.call('ltu_linear_fwd', _p(x), K, _ptr_array([w]), 1, _ptr_array([None]), _p(y), N, M, N, K, 1, 1, _s())
    ref = y0.float() + x.float() @ w.float().t()
    assert rel_err(y.float(), ref) < 6e-3


@pytest.mark.parametrize('M,K,N,nw', [(400, 128, 64, 1), (1000, 64, 96, 3), (257, 256, 768, 3), (4100, 32, 32, 1), (300, 128, 8, 1),
                                      (2048, 128, 384, 3), (8640, 256, 128, 1), (1024, 384, 256, 1), (21504, 128, 128, 1),
                                      (1000, 512, 200, 1), (777, 768, 264, 3), (5000, 64, 136, 1),    # LDS-DMA ring kernels
                                      (70000, 16, 16, 1), (65537, 32, 16, 1), (66000, 16, 32, 1), (65536, 64, 64, 1), (65541, 128, 64, 1),
                                      (70001, 64, 32, 1)])   # few-channel streaming projections (pw_small.hip: the attention gates' 1x1x1 convs)
def test_linear_bf16(ops, M, K, N, nw):
    """bf16 matrix-core path (NT forward / data gradient, transposing-read TN weight gradient); bf16 rounding of
    inputs and outputs bounds the error at ~1e-2 of the tensor's max"""
    g = G(2)
    bf = lambda t: t.bfloat16().float()
    x = bf(torch.randn(M, K, generator=g))
    ws = [bf(torch.randn(N // nw, K, generator=g) * 0.1) for _ in range(nw)]
    bs = [torch.randn(N // nw, generator=g) for _ in range(nw)]
    go = bf(torch.randn(M, N, generator=g))
    xr = x.clone().requires_grad_(True)
    wr = [w.clone().requires_grad_(True) for w in ws]
    br = [b.clone().requires_grad_(True) for b in bs]
    yr = F.linear(xr, torch.cat(wr), torch.cat(br))
    yr.backward(go)
    xd = x.to(DEV, torch.bfloat16).requires_grad_(True)
    wd = [w.to(DEV).requires_grad_(True) for w in ws]
    bd = [b.to(DEV).requires_grad_(True) for b in bs]
    yd = ops.linear(xd, wd, bd)
    assert yd.dtype == torch.bfloat16
    yd.backward(go.to(DEV, torch.bfloat16))
    assert rel_err(yd, yr) < 1e-2
    assert rel_err(xd.grad, xr.grad) < 1e-2
    for a, b in zip(wd, wr):
        assert rel_err(a.grad, b.grad) < 2e-3       # fp32 accumulation of exact bf16 products
    for a, b in zip(bd, br):
        assert rel_err(a.grad, b.grad) < 2e-3


@pytest.mark.parametrize('case', [
    (2, 8, 16, 6, 5, 8, (1, 1, 1), 0, False, None),
    (1, 16, 32, 8, 8, 6, (2, 2, 1), 0, False, None),
    (2, 8, 8, 7, 6, 5, (2, 2, 2), 0, False, None),
    (1, 8, 16, 6, 6, 4, (1, 1, 1), 8, False, None),
    (1, 16, 8, 3, 4, 2, (1, 1, 1), 0, True, None),
    (1, 32, 2, 5, 4, 6, (1, 1, 1), 0, False, 8),
    (1, 64, 128, 4, 4, 4, (1, 1, 1), 0, False, None),
    (2, 32, 32, 9, 7, 12, (1, 1, 1), 32, False, None),   # halo kernels: two channel chunks, ragged bricks
    (1, 16, 64, 8, 8, 16, (1, 1, 1), 16, False, None),   # halo kernels: chunk spanning both concat sources, two column tiles
    (3, 16, 16, 4, 12, 8, (1, 1, 1), 0, False, None),
    (2, 16, 64, 9, 7, 10, (2, 2, 2), 0, False, None),    # class-halo data gradient: 8 parity classes, odd input dims
    (1, 40, 32, 8, 5, 17, (2, 2, 1), 0, False, None),    # 4 classes
    (1, 32, 128, 17, 18, 21, (2, 2, 2), 0, False, None), # compile-time class kernel: four channel chunks, bricks ragged in every axis
    (2, 64, 64, 10, 9, 8, (2, 2, 2), 0, False, None),    # ... two column tiles
    (1, 16, 32, 12, 18, 19, (2, 2, 1), 0, False, None),  # ... stride 1 along d: half a column tile
    (1, 64, 96, 9, 16, 6, (2, 2, 1), 0, False, None),    # ... three chunks
    (2, 128, 128, 8, 8, 8, (2, 2, 2), 0, False, None),   # strided forward on a tiny grid with K = 3456: K-split implicit GEMM + fold
    (1, 256, 128, 4, 4, 8, (1, 1, 1), 0, False, None),   # stride-1 halo conv on one brick row: channel-split + fold
    (1, 128, 96, 6, 9, 12, (1, 1, 1), 128, False, None), # conv_ring.hip with the chunks split over workgroups: 128 + 128 concat -> 96 (ragged tile, ragged bricks); data gradient 96 -> 128 + 128
    (1, 16, 16, 36, 38, 60, (1, 1, 1), 0, False, None),  # persistent few-channel rings (conv_c16_ring / conv_fc_ring.hip): 360 ragged
    (1, 32, 32, 36, 38, 60, (1, 1, 1), 0, False, None),  # 4x8x8 bricks, 16 and 32 channels (long brick runs: tests/test_gpu_conv_paths.py)
    (1, 16, 16, 17, 30, 41, (1, 1, 1), 16, False, None), # weight-stationary kernels: 120 ragged 4x8x8 bricks are below the rings' 128-brick
                                                         # cut-off, so 16 + 16 concat -> 16 runs conv3_halo_ws<32>, its data gradient conv3_halo_wr<16>
    (2, 32, 32, 18, 33, 44, (1, 1, 1), 0, False, None),  # ... 32 -> 32, more bricks than workgroups
    (1, 32, 24, 21, 34, 37, (1, 1, 1), 0, False, None),  # ... 24 outputs
    (1, 8, 24, 21, 34, 37, (1, 1, 1), 24, False, None),  # ... 8 + 24 concat
    (1, 64, 64, 20, 33, 41, (1, 1, 1), 0, False, None),  # conv_ring.hip: two chunks, 64-column tile, 240 ragged bricks
    (1, 32, 32, 21, 34, 37, (1, 1, 1), 32, False, None), # ... 32 + 32 concat -> 32 (half a column tile), data gradient 32 -> 64 into two tensors
    (1, 96, 160, 12, 33, 41, (1, 1, 1), 0, False, None), # ... three chunks, 128-column tiles (the second one ragged)
    (2, 64, 72, 9, 32, 40, (1, 1, 1), 64, False, None),  # ... 64 + 64 concat -> 72
    (1, 64, 64, 32, 60, 68, (1, 1, 1), 0, False, None),  # ... eight-wave variant: 8x8x8 bricks (288 of them, ragged in w and d)
    (1, 32, 40, 16, 62, 70, (1, 1, 1), 32, False, None), # ... the same with a 32 + 32 concat and 40 outputs (run at any grid size by the knob below)
    (1, 8, 16, 20, 33, 41, (1, 1, 1), 8, False, None),   # conv_c16_ring.hip: 8 + 8 concat -> 16 on 150 ragged bricks, data gradient into two tensors
    (2, 16, 24, 18, 33, 44, (1, 1, 1), 0, False, None),  # ... 16 -> 24, more bricks than workgroups per CU pair
    (1, 16, 8, 21, 34, 37, (1, 1, 1), 0, False, None),   # ... 16 -> 8 (a head)
    (1, 16, 16, 21, 34, 37, (1, 1, 1), 16, False, None), # ... data gradient 16 -> 16 + 16 (the forward is conv_fc_ring.hip's)
])
def test_conv3d_bf16(ops, case):
    B, Ci, Co, H, W, D, stride, C1, ups, cop = case
    g = G(3)
    bf = lambda t: t.bfloat16().float()
    x0 = bf(torch.randn(B, Ci, H, W, D, generator=g))
    x1 = bf(torch.randn(B, C1, H, W, D, generator=g)) if C1 else None
    w = bf(torch.randn(Co, Ci + C1, 3, 3, 3, generator=g) * 0.1)
    b = torch.randn(Co, generator=g)
    x0r = x0.clone().requires_grad_(True)
    x1r = x1.clone().requires_grad_(True) if C1 else None
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    xin = x0r if not C1 else torch.cat((x0r, x1r), 1)
    if ups:
        xin = F.interpolate(xin, scale_factor=2)
    yr = F.conv3d(xin, wr, br, stride=stride, padding=1)
    go = bf(torch.randn(yr.shape, generator=g))
    yr.backward(go)
    x0d = to_cl(x0, torch.bfloat16).requires_grad_(True)
    x1d = to_cl(x1, torch.bfloat16).requires_grad_(True) if C1 else None
    wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    yd = ops.conv3d(x0d, wd, bd, stride=stride, x1=x1d, ups=ups, cop=cop)
    god = to_cl(go, torch.bfloat16)
    if cop:
        pad = torch.zeros(yd.shape, device=DEV, dtype=torch.bfloat16)
        pad[..., :Co] = god
        god = pad
    yd.backward(god)
    assert rel_err(from_cl(yd)[:, :Co], yr) < 1e-2
    assert rel_err(from_cl(x0d.grad), x0r.grad) < 1e-2
    if C1:
        assert rel_err(from_cl(x1d.grad), x1r.grad) < 1e-2
    assert rel_err(wd.grad, wr.grad) < 2e-3
    assert rel_err(bd.grad, br.grad) < 2e-3


@pytest.mark.parametrize('dtype,tol,wtol', [(torch.float32, 1e-4, 1e-4), (torch.bfloat16, 1e-2, 2e-3)])
@pytest.mark.parametrize('case', [
    # B, Ci, Ca, Cb, n1, H, W, D
    (2, 32, 16, 2, 16, 9, 7, 12),      # level-0 shape class: weight-stationary kernel, data gradient from a 16+16 concat
    (1, 32, 16, 2, 16, 18, 33, 41),    # the same on a grid of 240 ragged bricks: conv_fc_ring.hip, forward into two outputs
    (1, 64, 32, 2, 32, 18, 33, 41),    # conv_ring.hip: 64 -> 32 + 32 pair on 240 bricks, data gradient from the 32 + 32 gradient concat
    (1, 64, 32, 2, 32, 8, 8, 16),      # generic halo kernel, 64-column tile
    (1, 256, 128, 3, 32, 4, 4, 8),     # deep level: channel-split forward, 160-channel gradient concat
])
def test_conv3d_pair(ops, case, dtype, tol, wtol):
    """conv1 + mask head of a decoder level fused into one conv against the two separate F.conv3d calls"""
    B, Ci, Ca, Cb, n1, H, W, D = case
    g = G(13)
    rd = (lambda t: t.bfloat16().float()) if dtype == torch.bfloat16 else (lambda t: t)
    x = rd(torch.randn(B, Ci, H, W, D, generator=g))
    wa, wb = rd(torch.randn(Ca, Ci, 3, 3, 3, generator=g) * 0.1), rd(torch.randn(Cb, Ci, 3, 3, 3, generator=g) * 0.1)
    ba, bb = torch.randn(Ca, generator=g), torch.randn(Cb, generator=g)
    xr, war, wbr, bar, bbr = (t.clone().requires_grad_(True) for t in (x, wa, wb, ba, bb))
    ya, yb = F.conv3d(xr, war, bar, padding=1), F.conv3d(xr, wbr, bbr, padding=1)
    ga, gb = rd(torch.randn(ya.shape, generator=g)), rd(torch.randn(yb.shape, generator=g))
    torch.autograd.backward([ya, yb], [ga, gb])
    xd = to_cl(x, dtype).requires_grad_(True)
    pd = [t.to(DEV).requires_grad_(True) for t in (wa, ba, wb, bb)]
    prep = ops.conv_pair_prep(pd[0].detach(), pd[1].detach(), pd[2].detach(), pd[3].detach(), n1, dtype)
    y0, y1 = ops.conv3d_pair(xd, pd[0], pd[1], pd[2], pd[3], prep)
    assert y0.shape[-1] == Ca and y1.shape[-1] == n1
    assert (y1[..., Cb:].float().abs().max().item() == 0.0)            # padded head columns: zero weights, zero bias
    g1 = torch.zeros(y1.shape, device=DEV, dtype=dtype)
    g1[..., :Cb] = to_cl(gb, dtype)
    torch.autograd.backward([y0, y1], [to_cl(ga, dtype), g1])
    assert rel_err(from_cl(y0), ya) < tol and rel_err(from_cl(y1)[:, :Cb], yb) < tol
    assert rel_err(from_cl(xd.grad), xr.grad) < tol
    for got, ref in zip(pd, (war, bar, wbr, bbr)):
        assert rel_err(got.grad, ref.grad) < wtol


# ---------------------------------------------------------------------------------------------- conv3d
CONV_CASES = [
    # B, Ci, Co, H, W, D, stride, C1, ups, cop
    (2, 8, 16, 6, 5, 8, (1, 1, 1), 0, False, None),
    (1, 16, 32, 8, 8, 6, (2, 2, 1), 0, False, None),
    (2, 8, 8, 7, 6, 5, (2, 2, 2), 0, False, None),
    (1, 8, 16, 6, 6, 4, (1, 1, 1), 8, False, None),      # virtual concat
    (1, 16, 8, 3, 4, 2, (1, 1, 1), 0, True, None),       # fused nearest x2 upsampling
    (1, 32, 2, 5, 4, 6, (1, 1, 1), 0, False, 4),         # padded mask head
    (1, 64, 128, 4, 4, 4, (1, 1, 1), 0, False, None),    # wide tiles
]


@pytest.mark.parametrize('case', CONV_CASES)
def test_conv3d(ops, case):
    B, Ci, Co, H, W, D, stride, C1, ups, cop = case
    g = G(3)
    x0 = torch.randn(B, Ci, H, W, D, generator=g)
    x1 = torch.randn(B, C1, H, W, D, generator=g) if C1 else None
    w = torch.randn(Co, Ci + C1, 3, 3, 3, generator=g) * 0.1
    b = torch.randn(Co, generator=g)
    x0r = x0.clone().requires_grad_(True)
    x1r = x1.clone().requires_grad_(True) if C1 else None
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    xin = x0r if not C1 else torch.cat((x0r, x1r), 1)
    if ups:
        xin = F.interpolate(xin, scale_factor=2)
    yr = F.conv3d(xin, wr, br, stride=stride, padding=1)
    go = torch.randn(yr.shape, generator=g)
    yr.backward(go)

    x0d = to_cl(x0).requires_grad_(True)
    x1d = to_cl(x1).requires_grad_(True) if C1 else None
    wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    yd = ops.conv3d(x0d, wd, bd, stride=stride, x1=x1d, ups=ups, cop=cop)
    god = to_cl(go)
    if cop:
        assert yd.shape[-1] == cop
        pad = torch.zeros(yd.shape, device=DEV)
        pad[..., :Co] = god
        god = pad
        assert yd[..., Co:].abs().max().item() == 0
    yd.backward(god)
    assert rel_err(from_cl(yd)[:, :Co], yr) < 1e-4
    assert rel_err(from_cl(x0d.grad), x0r.grad) < 1e-4
    if C1:
        assert rel_err(from_cl(x1d.grad), x1r.grad) < 1e-4
    assert rel_err(wd.grad, wr.grad) < 1e-4
    assert rel_err(bd.grad, br.grad) < 1e-4


@pytest.mark.parametrize('dtype,tol', [(torch.float32, 1e-4), (torch.bfloat16, 1.5e-2)])
@pytest.mark.parametrize('B,Ci,Co,H,W,D', [(2, 16, 8, 3, 4, 2), (1, 32, 16, 5, 3, 4), (1, 128, 32, 4, 3, 5), (2, 64, 72, 5, 6, 9),
                                          (1, 128, 64, 4, 4, 4),      # K = 64*Co = 4096 on a tiny grid -> K-split data gradient
                                          (1, 128, 32, 5, 9, 11), (2, 256, 64, 6, 8, 9), (1, 256, 128, 4, 10, 8)])   # ring kernels: ragged bricks,
                                                                                                                      # two column halves, four chunks
def test_upconv_subpixel(ops, dtype, tol, B, Ci, Co, H, W, D):
    """nearest x2 + conv3x3x3 computed as 8 parity-class 2x2x2 convs with pre-summed weights == the plain formulation"""
    g = G(13)
    bf = (lambda t: t.bfloat16().float()) if dtype == torch.bfloat16 else (lambda t: t)
    x = bf(torch.randn(B, Ci, H, W, D, generator=g))
    w = bf(torch.randn(Co, Ci, 3, 3, 3, generator=g) * 0.1)
    b = torch.randn(Co, generator=g)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = F.conv3d(F.interpolate(xr, scale_factor=2), wr, br, padding=1)
    go = bf(torch.randn(yr.shape, generator=g))
    yr.backward(go)
    xd = to_cl(x, dtype).requires_grad_(True)
    wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    yd = ops.upconv3d(xd, wd, bd)
    yd.backward(to_cl(go, dtype))
    assert rel_err(from_cl(yd), yr) < tol
    assert rel_err(from_cl(xd.grad), xr.grad) < tol
    assert rel_err(wd.grad, wr.grad) < max(tol / 5, 1e-4)
    assert rel_err(bd.grad, br.grad) < max(tol / 5, 1e-4)


@pytest.mark.parametrize('gen', [1, 0])
def test_upconv_wgrad_long_brick_runs(ops, gen):
    """the un-embedding's weight gradient with few workgroups (LTU_UPW_BLOCKS = 8: one workgroup walks 16 bricks = 32 half-brick units, the
    steady state of the LDS-DMA ring) against torch; gen 0 = the first-generation kernel (LTU_UPW_RING = 0)"""
    from lintransunet_amd import _lib
    B, Ci, Co, H, W, D = 2, 64, 72, 5, 6, 9
    g = G(17)
    bf = lambda t: t.bfloat16().float()
    x = bf(torch.randn(B, Ci, H, W, D, generator=g))
    w = bf(torch.randn(Co, Ci, 3, 3, 3, generator=g) * 0.1)
    b = torch.randn(Co, generator=g)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    yr = F.conv3d(F.interpolate(xr, scale_factor=2), wr, br, padding=1)
    go = bf(torch.randn(yr.shape, generator=g))
    yr.backward(go)
    _lib.config_set('LTU_UPW_BLOCKS', 8)
    _lib.config_set('LTU_UPW_RING', gen)
    try:
        xd = to_cl(x, torch.bfloat16).requires_grad_(True)
        wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        yd = ops.upconv3d(xd, wd, bd)
        yd.backward(to_cl(go, torch.bfloat16))
        torch.cuda.synchronize()
    finally:
        _lib.config_set('LTU_UPW_BLOCKS', None)
        _lib.config_set('LTU_UPW_RING', None)
    assert rel_err(wd.grad, wr.grad) < 3e-3
    assert rel_err(bd.grad, br.grad) < 3e-3


def test_conv3d_stem_padding(ops):
    """stem: 4 real input channels carried in an 8-channel tensor (window embedding)"""
    g = G(4)
    x = torch.randn(2, 1, 12, 8, 6, generator=g)
    w = torch.randn(16, 4, 3, 3, 3, generator=g) * 0.2
    b = torch.randn(16, generator=g)
    yr = F.conv3d(O_net.window_embed(x), w, b, padding=1)
    e = ops.window_embed(x.to(DEV), torch.float32)
    assert e.shape == (2, 6, 4, 6, 8)
    assert rel_err(from_cl(e)[:, :4], O_net.window_embed(x)) == 0
    yd = ops.conv3d(e, w.to(DEV), b.to(DEV))
    assert rel_err(from_cl(yd), yr) < 1e-4


# ---------------------------------------------------------------------------------------------- norms
@pytest.mark.parametrize('C,with_res', [(8, True), (32, False), (128, True), (256, False)])
def test_instnorm_act(ops, C, with_res):
    g = G(5)
    x = torch.randn(2, C, 5, 6, 7, generator=g) * 3 + 1.5
    r = torch.randn(2, C, 5, 6, 7, generator=g) if with_res else None
    xr = x.clone().requires_grad_(True)
    rr = r.clone().requires_grad_(True) if with_res else None
    yr = F.leaky_relu(F.instance_norm(xr, eps=1e-5), 0.01)
    if with_res:
        yr = yr + rr
    go = torch.randn(yr.shape, generator=g)
    yr.backward(go)
    xd = to_cl(x).requires_grad_(True)
    rd = to_cl(r).requires_grad_(True) if with_res else None
    yd = ops.instnorm_act(xd, rd)
    yd.backward(to_cl(go))
    assert rel_err(from_cl(yd), yr) < 1e-4
    assert rel_err(from_cl(xd.grad), xr.grad) < 2e-4
    if with_res:
        assert rel_err(from_cl(rd.grad), rr.grad) < 1e-6


def _instnorm_variants():
    # the two rejected launch variants exist in an experiments build only (make -C lintransunet_amd/csrc EXPERIMENTS=1)
    try:
        from lintransunet_amd import _lib
        exp = _lib.experiments()
    except Exception:
        exp = False
    return ['two_stage', 'streaming'] + (['fold_in_apply', 'vw8'] if exp else [])


@pytest.fixture(params=_instnorm_variants())
def instnorm_variant(request):
    """the InstanceNorm launch variants behind run-time knobs (ltu_config_set): the default, the apply kernels folding the
    statistics partials themselves (no fold launch), 16-byte bf16 vectors"""
    from lintransunet_amd import _lib
    # 'two_stage': the default dispatch (samples of <= 1 MB take the one-launch kernels, the rest partial sums + fold + apply);
    # 'streaming': the three-launch kernels at every size
    knob = {'two_stage': None, 'streaming': b'LTU_NO_IN_SMALL', 'fold_in_apply': b'LTU_IN_FOLD', 'vw8': b'LTU_IN_VW8'}[request.param]
    if knob in (b'LTU_IN_FOLD', b'LTU_IN_VW8') and not _lib.experiments():
        pytest.skip('rejected variant: compiled into an experiments build only (make EXPERIMENTS=1)')
    if knob:
        _lib.call('ltu_config_set', knob, 1, 0)
    yield request.param
    if knob:
        _lib.call('ltu_config_set', knob, 0, 1)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('B,S,C', [(2, 8 * 8 * 8, 256), (2, 37 * 11 * 3, 16), (1, 64 * 64 * 32, 16), (2, 20 * 13 * 8, 64), (3, 4097, 8),
                                   (2, 1000, 4), (2, 70, 128)])
def test_instnorm_fwd_one_call(ops, instnorm_variant, dtype, B, S, C):
    """ltu_instnorm_fwd (statistics + apply in one call; with LTU_IN_FOLD an apply kernel that folds the partial sums itself)
    against the separate ltu_instnorm_stats / ltu_instnorm_apply calls (own fold launch) and a torch fp32 reference; the published
    statistics feed ltu_instnorm_bwd, whose apply kernel folds its partials the same way: checked against autograd"""
    from lintransunet_amd import _lib
    g = G(41)
    x = (torch.randn(B, S, C, generator=g) * 2 + 0.7).to(DEV).to(dtype)
    res = torch.randn(B, S, C, generator=g).to(DEV).to(dtype)
    dt = 0 if dtype == torch.float32 else 1
    ws = torch.empty(_lib.load().ltu_norm_ws_floats(), device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    s1, s2 = torch.zeros(B, C, 3, device=DEV), torch.zeros(B, C, 3, device=DEV)
    y1, y2 = torch.empty_like(x), torch.empty_like(x)
    _lib.call('ltu_instnorm_stats', x.data_ptr(), s1.data_ptr(), ws.data_ptr(), ws.numel(), B, S, C, dt, st)
    _lib.call('ltu_instnorm_apply', x.data_ptr(), s1.data_ptr(), res.data_ptr(), y1.data_ptr(), B, S, C, 1, 0.01, 0.0, 0, 0, dt, st)
    _lib.call('ltu_instnorm_fwd', x.data_ptr(), s2.data_ptr(), ws.data_ptr(), ws.numel(), res.data_ptr(), y2.data_ptr(), B, S, C, 1, 0.01, 0.0, 0, 0, dt, st)
    assert torch.equal(s1[..., 0], s2[..., 0])
    assert rel_err(s2, s1) < 1e-5
    xr = x.float().requires_grad_(True)
    yr = F.leaky_relu(F.instance_norm(xr.transpose(1, 2), eps=1e-5), 0.01).transpose(1, 2) + res.float()
    tol = 1e-4 if dtype == torch.float32 else 6e-3
    assert rel_err(y2.float(), yr) < tol and rel_err(y2.float(), y1.float()) < (1e-5 if dtype == torch.float32 else 3e-3)
    go = torch.randn(B, S, C, generator=g).to(DEV).to(dtype)
    yr.backward(go.float())
    bs, dx = torch.zeros(B, C, 2, device=DEV), torch.empty_like(x)
    _lib.call('ltu_instnorm_bwd', go.data_ptr(), 0, 0, x.data_ptr(), s2.data_ptr(), bs.data_ptr(), ws.data_ptr(), ws.numel(), dx.data_ptr(), B, S, C, 1,
              0.01, 0.0, 0, 0, dt, st)
    assert rel_err(dx.float(), xr.grad) < (2e-4 if dtype == torch.float32 else 8e-3)
    xh = (x.float() - x.float().mean(1, keepdim=True)) * torch.rsqrt(x.float().var(1, unbiased=False, keepdim=True) + 1e-5)
    gg = go.float() * torch.where(xh > 0, 1.0, 0.01)
    want = torch.stack((gg.sum(1), (gg * xh).sum(1)), -1)
    assert rel_err(bs, want) < (1e-4 if dtype == torch.float32 else 2e-3)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('B,S,C', [(2, 8 * 8 * 64, 128), (2, 4 * 4 * 32, 256), (1, 3000, 16), (3, 77, 8), (2, 1025, 32)])
def test_instnorm_small_against_streaming(ops, dtype, B, S, C):
    """the one-launch InstanceNorm of small samples (a workgroup per (sample, 16-byte channel group), the tensor held in registers)
    against the streaming three-launch kernels (LTU_NO_IN_SMALL): forward with residual and dropout (the same mask: the hash is
    indexed by element), statistics-only call, backward with three gradient ports"""
    from lintransunet_amd import _lib
    g = G(43)
    x = (torch.randn(B, S, C, generator=g) * 2 + 0.7).to(DEV).to(dtype)
    res = torch.randn(B, S, C, generator=g).to(DEV).to(dtype)
    gos = [torch.randn(B, S, C, generator=g).to(DEV).to(dtype) for _ in range(3)]
    dt = 0 if dtype == torch.float32 else 1
    ws = torch.empty(_lib.load().ltu_norm_ws_floats(), device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    step = torch.tensor([5], dtype=torch.int64, device=DEV)

    def run():
        s0, s1 = torch.zeros(B, C, 3, device=DEV), torch.zeros(B, C, 3, device=DEV)
        y = torch.empty_like(x)
        _lib.call('ltu_instnorm_stats', x.data_ptr(), s0.data_ptr(), ws.data_ptr(), ws.numel(), B, S, C, dt, st)
        _lib.call('ltu_instnorm_fwd', x.data_ptr(), s1.data_ptr(), ws.data_ptr(), ws.numel(), res.data_ptr(), y.data_ptr(), B, S, C, 1, 0.01, 0.3, 4242,
                  step.data_ptr(), dt, st)
        bs, dx = torch.zeros(B, C, 2, device=DEV), torch.empty_like(x)
        _lib.call('ltu_instnorm_bwd', gos[0].data_ptr(), gos[1].data_ptr(), gos[2].data_ptr(), x.data_ptr(), s1.data_ptr(), bs.data_ptr(),
                  ws.data_ptr(), ws.numel(), dx.data_ptr(), B, S, C, 1, 0.01, 0.3, 4242, step.data_ptr(), dt, st)
        bs1, dx1 = torch.zeros(B, C, 2, device=DEV), torch.empty_like(x)
        _lib.call('ltu_instnorm_bwd', gos[0].data_ptr(), 0, 0, x.data_ptr(), s1.data_ptr(), bs1.data_ptr(), ws.data_ptr(), ws.numel(), dx1.data_ptr(),
                  B, S, C, 0, 0.0, 0.0, 0, 0, dt, st)
        torch.cuda.synchronize()
        return s0, s1, y.float(), bs, dx.float(), bs1, dx1.float()
    a = _with_knob(b'LTU_IN_SMALL_KB', 1024, run)      # (the default limit is 256 KB per sample: the 1 024-thread variant is tested too)
    b = _with_knob(b'LTU_NO_IN_SMALL', 1, run)
    tol = 1e-5 if dtype == torch.float32 else 4e-3
    assert torch.equal(a[0][..., 0], b[0][..., 0]) and torch.equal(a[0], a[1])
    assert rel_err(a[0], b[0]) < 1e-5 and rel_err(a[1], b[1]) < 1e-5
    assert torch.equal((a[2] - res.float()) == 0, (b[2] - res.float()) == 0)          # the same dropout mask
    assert rel_err(a[2], b[2]) < tol
    assert rel_err(a[3], b[3]) < 2e-4 and rel_err(a[5], b[5]) < 2e-4
    assert rel_err(a[4], b[4]) < 2 * tol and rel_err(a[6], b[6]) < 2 * tol


@pytest.mark.parametrize('d', [32, 64, 128, 256])
def test_res_layernorm(ops, d):
    g = G(6)
    M = 333
    x, r = torch.randn(M, d, generator=g), torch.randn(M, d, generator=g)
    gam, bet = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    go = torch.randn(M, d, generator=g)
    xr, rr = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    gr, br = gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    yr = F.layer_norm(xr + rr, (d,), gr, br, 1e-6)
    yr.backward(go)
    xd, rd = x.to(DEV).requires_grad_(True), r.to(DEV).requires_grad_(True)
    gd, bd = gam.to(DEV).requires_grad_(True), bet.to(DEV).requires_grad_(True)
    yd = ops.res_layernorm(xd, rd, gd, bd)
    yd.backward(go.to(DEV))
    assert rel_err(yd, yr) < 1e-4
    assert rel_err(xd.grad, xr.grad) < 1e-4
    assert rel_err(rd.grad, rr.grad) < 1e-4
    assert rel_err(gd.grad, gr.grad) < 1e-4
    assert rel_err(bd.grad, br.grad) < 1e-4


def test_gelu(ops):
    g = G(7)
    u = torch.randn(100, 64, generator=g) * 2
    go = torch.randn(100, 64, generator=g)
    ur = u.clone().requires_grad_(True)
    F.gelu(ur).backward(go)
    ud = u.to(DEV).requires_grad_(True)
    hd = ops.gelu_dropout(ud)
    hd.backward(go.to(DEV))
    assert rel_err(hd, F.gelu(u)) < 1e-5
    assert rel_err(ud.grad, ur.grad) < 1e-5


@pytest.mark.parametrize('M,K,N', [(4096, 128, 256), (1024, 256, 512), (777, 64, 96), (130, 32, 40)])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_linear_gelu_fused(ops, M, K, N, dtype):
    """projection with GELU + dropout in its epilogue == projection followed by the stand-alone GELU kernel, bit for bit
    (same rounding points, same dropout groups), forward and backward; shapes outside the ring kernel take the two-launch path"""
    g = G(17)
    x = torch.randn(M, K, generator=g).to(DEV, dtype)
    w = (torch.randn(N, K, generator=g) * 0.1).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    go = torch.randn(M, N, generator=g).to(DEV, dtype)
    outs = []
    for fused in (True, False):
        xd, wd, bd = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        if fused:
            h = ops.linear_gelu(xd, wd, bd, 0.3, 4242)
        else:
            h = ops.gelu_dropout(ops.linear(xd, [wd], [bd]), 0.3, 4242)
        h.backward(go)
        outs.append((h.detach(), xd.grad, wd.grad, bd.grad))
    for a, c in zip(*outs):
        if dtype == torch.bfloat16:
            assert torch.equal(a, c)
        else:                              # the fp32 weight gradient accumulates with atomics: order varies from run to run
            assert rel_err(a, c) < 1e-5
    keep = (outs[0][0] != 0).float().mean().item()
    assert abs(keep - 0.7) < 0.02


def test_dropout_masks(ops):
    """counter-hash dropout (csrc/common.h: a murmur3 finalizer + a linear expansion per 4-element group): keep rate, 1/(1-p) scaling, and the
    backward regenerates exactly the forward mask"""
    n = 1 << 18
    u = torch.ones(n // 64, 64, device=DEV).requires_grad_(True)
    h = ops.gelu_dropout(u, 0.3, 12345)
    val = F.gelu(torch.ones(1)).item() / 0.7
    kept = h.detach() != 0
    assert abs(kept.float().mean().item() - 0.7) < 5e-3
    assert torch.allclose(h.detach()[kept], torch.full((1,), val, device=DEV), rtol=1e-5)
    h.sum().backward()
    assert torch.equal(u.grad != 0, kept)
    h2 = ops.gelu_dropout(u.detach(), 0.3, 12346)
    assert (kept != (h2 != 0)).float().mean().item() > 0.3        # another seed, another mask
    x = torch.randn(2, 4, 4, 4, 32, device=DEV).requires_grad_(True)
    y = ops.instnorm_act(x, None, 1, 0.3, 777)
    keep = (y.detach() != 0)
    y.backward(torch.ones_like(y))
    # IN backward mixes voxels, so test the mask through a second call instead
    y2 = ops.instnorm_act(x.detach(), None, 1, 0.3, 777)
    assert torch.equal(y2 != 0, keep)


def test_dropout_mask_statistics(ops):
    """the four keep decisions of a 4-element group come from one 32-bit murmur-finalized word and a linear expansion of it: per-slot
    keep rates, pairwise correlations inside a group, correlations between neighbouring groups / rows, and the conditional keep
    rates given the other slots of the group must look like independent Bernoulli(0.7) draws (4 M elements: sigma ~ 1e-3)"""
    n = 1 << 22
    u = torch.ones(n, device=DEV)
    K = (ops.gelu_dropout(u, 0.3, 98765) != 0).double().reshape(-1, 4)
    assert (K.mean(0) - 0.7).abs().max().item() < 3e-3
    C = torch.corrcoef(K.t())
    assert (C - torch.eye(4, device=DEV, dtype=C.dtype)).abs().max().item() < 5e-3
    for lag in (1, 32, 64, 2048):
        a, b = K[:-lag], K[lag:]
        ca, cb = a - a.mean(0), b - b.mean(0)
        corr = (ca.t() @ cb) / (ca.norm(dim=0)[:, None] * cb.norm(dim=0)[None, :])
        assert corr.abs().max().item() < 5e-3, lag
    xy = (K[:, 0] == 1) & (K[:, 1] == 1)
    assert abs(K[xy, 2].mean().item() - 0.7) < 3e-3
    xyz = xy & (K[:, 2] == 1)
    assert abs(K[xyz, 3].mean().item() - 0.7) < 3e-3
    nxy = (K[:, 0] == 0) & (K[:, 1] == 0)
    assert abs(K[nxy, 2].mean().item() - 0.7) < 5e-3 and abs(K[nxy, 3].mean().item() - 0.7) < 5e-3


@pytest.mark.parametrize('p', [0.3, 0.5])
def test_dropout_group_pattern_histogram(ops, p):
    """the four keep decisions of a group are pairwise independent by construction but the third and fourth are functions of the
    first two (one 32-bit hash per group, csrc/common.h: drop4): the JOINT distribution of the 16 keep patterns of a group is
    held against Bernoulli(1 - p)^4 - every pattern within 4 sigma (+ 2e-4 absolute for the 16-bit threshold rounding) at 8 M
    groups, and the distribution of the per-group keep COUNT (what a row of activations feels) likewise"""
    n = 1 << 25
    u = torch.ones(n, device=DEV)
    K = (ops.gelu_dropout(u, p, 424242) != 0).reshape(-1, 4).long()
    pat = K[:, 0] + 2 * K[:, 1] + 4 * K[:, 2] + 8 * K[:, 3]
    hist = torch.bincount(pat, minlength=16).double().cpu() / K.shape[0]
    q = 1.0 - p
    groups = K.shape[0]
    for code in range(16):
        k = bin(code).count('1')
        want = q ** k * p ** (4 - k)
        sigma = (want * (1 - want) / groups) ** 0.5
        assert abs(hist[code].item() - want) < 4 * sigma + 2e-4, (code, hist[code].item(), want)
    counts = torch.bincount(K.sum(1), minlength=5).double().cpu() / groups
    from math import comb
    for k in range(5):
        want = comb(4, k) * q ** k * p ** (4 - k)
        assert abs(counts[k].item() - want) < 4 * (want * (1 - want) / groups) ** 0.5 + 3e-4, (k, counts[k].item(), want)


@pytest.mark.parametrize('fat', [0, 1])
@pytest.mark.parametrize('M,d,width', [(4320, 256, 0), (2048, 128, 0), (21504, 256, 0), (1024, 256, 0), (114816, 128, 0), (114816, 128, 128),
                                       (21504, 256, 128), (8640, 256, 128), (1056, 128, 7), (2080, 256, 1000)])
def test_linear_wgrad_group(ops, M, d, width, fat):
    """the four projection weight gradients of a transformer layer (qkv with 3 blocks, out, ffn1, ffn2) as ONE grouped launch +
    ONE fold against torch fp32 (G^T X and column sums of G on the bf16-rounded operands), accumulated onto existing values; at the
    library's stand-alone width (0) and at the workgroup budget train.GraphedStep hands the side-stream launches (128), plus
    ragged row counts with odd budgets (row splits of unequal length, more / fewer workgroups than tiles)"""
    g = G(31)
    bf = lambda t: t.bfloat16()
    shapes = [(3 * d, d, 3), (d, d, 1), (2 * d, d, 1), (d, 2 * d, 1)]          # (N, K, nw)
    lc = ops.Context()
    if width:
        lc.wq_install(torch.cuda.current_stream(), width=width)              # a queue on the current stream: in line, at that width
    if fat:
        from lintransunet_amd import _lib
        if not _lib.experiments():
            pytest.skip('the fat-tile grouped kernel is compiled into an experiments build only (make EXPERIMENTS=1)')
        _lib.call('ltu_config_set', b'LTU_WGROUP_FAT', 1, 0)
    want, bufs = [], []
    for N, K, nw in shapes:
        gr, x = bf(torch.randn(M, N, generator=g) * 0.1).to(DEV), bf(torch.randn(M, K, generator=g)).to(DEV)
        dws = [torch.full((N // nw, K), 0.5, device=DEV) for _ in range(nw)]      # += semantics: start from a non-zero value
        dbs = [torch.full((N // nw,), -0.25, device=DEV) for _ in range(nw)]
        lc.wgrad_group_push(gr, x, dws, dbs, M, N, K, False)
        dw = gr.float().t() @ x.float()
        want.append((dw + 0.5, gr.float().sum(0) - 0.25))
        bufs.append((dws, dbs))
    assert len(lc.wg_group) == 4
    try:
        lc.flush_deferred()
        lc.wq_join()
    finally:
        if fat:
            _lib.call('ltu_config_set', b'LTU_WGROUP_FAT', 0, 1)
    assert not lc.wg_group
    for (dw_ref, db_ref), (dws, dbs) in zip(want, bufs):
        dw, db = torch.cat(dws, 0), torch.cat(dbs, 0)
        assert rel_err(dw, dw_ref) < 2e-5 and rel_err(db, db_ref) < 2e-5


def test_wgrad_group_short_workspace_is_refused(ops):
    """SURVEY 8(b) error contract for workspaces (round 4's GPU fault: a launch whose geometry needed more than the workspace it had
    been sized for wrote past its end): the launch is told the capacity and returns LTU_E_ARG (-4) WITHOUT launching when its
    geometry - here: a larger workgroup budget than the size query was asked for - needs more; a sufficient workspace runs"""
    import ctypes
    from lintransunet_amd import _lib
    M, d = 8192, 128
    g = G(5)
    gr = (torch.randn(M, 3 * d, generator=g) * 0.1).bfloat16().to(DEV)
    x = torch.randn(M, d, generator=g).bfloat16().to(DEV)
    dws = [torch.zeros(d, d, device=DEV) for _ in range(3)]
    dbs = [torch.zeros(d, device=DEV) for _ in range(3)]
    arr = (_lib.WgradJob * 1)()
    r = arr[0]
    r.grad, r.a, r.ldg, r.lda, r.nw, r.M, r.N, r.K = gr.data_ptr(), x.data_ptr(), 3 * d, d, 3, M, 3 * d, d
    for i in range(3):
        r.dw[i], r.db[i] = dws[i].data_ptr(), dbs[i].data_ptr()
    lib = _lib.load()
    n8, n32 = (lib.ltu_linear_wgrad_group_ws_floats(ctypes.addressof(arr), 1, b) for b in (8, 32))
    assert 0 < n8 < n32
    guard = 1 << 16
    ws = torch.zeros(n32 + guard, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    rc = lib.ltu_linear_wgrad_group(ctypes.addressof(arr), 1, 32, ws.data_ptr(), n8, 1, s)       # sized at 8, launched at 32
    torch.cuda.synchronize()
    assert rc == -4
    assert not ws.any() and not any(t.any() for t in dws)                                        # nothing was launched
    with pytest.raises(_lib.LtuError, match='LTU_E_ARG'):
        _lib.call('ltu_linear_wgrad_group', ctypes.addressof(arr), 1, 32, ws.data_ptr(), n8, 1, s)
    assert lib.ltu_linear_wgrad_group(ctypes.addressof(arr), 1, 32, ws.data_ptr(), n32, 1, s) == 0
    torch.cuda.synchronize()
    assert not ws[n32:].any()                                                                    # ... and stayed inside its size
    assert rel_err(torch.cat(dws, 0), gr.float().t() @ x.float()) < 2e-5


def test_short_workspaces_are_refused(ops):
    """the same contract on the other workspace-taking entry points, one per kind of geometry: a capacity below what the launch is
    about to use yields LTU_E_ARG (-4) and nothing is launched (the outputs keep their fill value)"""
    from lintransunet_amd import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    g = G(6)
    bf = lambda *sh: (torch.randn(*sh, generator=g) * 0.1).bfloat16().to(DEV)
    # (1) dense weight gradient: row splits through the workspace
    M, N, K = 4096, 128, 128
    gr, x = bf(M, N), bf(M, K)
    dw, db = torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
    need = lib.ltu_wgrad_ws_floats(M, N, K)
    ws = torch.zeros(need, device=DEV)
    import ctypes
    arr1 = (ctypes.c_void_p * 3)(dw.data_ptr(), 0, 0)
    arr2 = (ctypes.c_void_p * 3)(db.data_ptr(), 0, 0)
    assert lib.ltu_linear_wgrad(gr.data_ptr(), N, x.data_ptr(), K, arr1, arr2, 1, M, N, K, ws.data_ptr(), 1024, 0, 1, s) == -4
    torch.cuda.synchronize()
    assert not dw.any() and not ws.any()
    assert lib.ltu_linear_wgrad(gr.data_ptr(), N, x.data_ptr(), K, arr1, arr2, 1, M, N, K, ws.data_ptr(), need, 0, 1, s) == 0
    torch.cuda.synchronize()
    assert rel_err(dw, gr.float().t() @ x.float()) < 2e-5
    # (2) sub-pixel un-embedding weight gradient: sized at a budget of 64 workgroups, launched at 256
    B, H, W, D, Ci, Co = 1, 8, 8, 8, 64, 32
    xg, gg = bf(B, H, W, D, Ci), bf(B, 2 * H, 2 * W, 2 * D, Co)
    n64, n256 = (lib.ltu_upconv_wgrad_ws_floats(B * H * W * D, Co, Ci, b) for b in (2, 256))
    assert 0 < n64 < n256
    dweff = torch.zeros(8, Co, 8, Ci, device=DEV)
    dwt, dbt = torch.zeros(Co, Ci, 27, device=DEV), torch.zeros(Co, device=DEV)
    ws = torch.zeros(n256, device=DEV)
    args = lambda cap, blocks: (gg.data_ptr(), xg.data_ptr(), dweff.data_ptr(), dbt.data_ptr(), dwt.data_ptr(), Co, Ci, ws.data_ptr(), cap, blocks,
                                B, H, W, D, Ci, Co, 1, s)
    assert lib.ltu_upconv_wgrad(*args(n64, 256)) == -4
    torch.cuda.synchronize()
    assert not dwt.any() and not ws.any()
    assert lib.ltu_upconv_wgrad(*args(n256, 256)) == 0 and lib.ltu_upconv_wgrad(*args(n64, 2)) == 0
    torch.cuda.synchronize()
    assert dwt.any()
    # (3) linear attention: split partials
    Bq, Nq, d = 2, 4096, 128
    qkv = bf(Bq * Nq, 3 * d)
    Hh = d // 32
    cx, cs = torch.zeros(Bq * Hh, 32, 32, device=DEV), torch.zeros(Bq * Hh, 64, device=DEV)
    need = lib.ltu_linattn_ws_floats(Bq, Nq, d)
    ws = torch.zeros(need, device=DEV)
    assert lib.ltu_linattn_ctx(qkv.data_ptr(), cx.data_ptr(), cs.data_ptr(), ws.data_ptr(), need // 4, Bq, Nq, d, 1, s) == -4
    torch.cuda.synchronize()
    assert not cx.any() and not ws.any()
    assert lib.ltu_linattn_ctx(qkv.data_ptr(), cx.data_ptr(), cs.data_ptr(), ws.data_ptr(), need, Bq, Nq, d, 1, s) == 0
    # (4) the fixed-size scratch of the two-stage norm reductions, the trilinear adjoint's intermediate, the loss partials
    xs = bf(2, 4096, 16)
    sums = torch.zeros(2, 16, 3, device=DEV)
    nws = torch.zeros(lib.ltu_norm_ws_floats(), device=DEV)
    assert lib.ltu_instnorm_stats(xs.data_ptr(), sums.data_ptr(), nws.data_ptr(), 16, 2, 4096, 16, 1, s) == -4
    assert lib.ltu_instnorm_stats(xs.data_ptr(), sums.data_ptr(), nws.data_ptr(), nws.numel(), 2, 4096, 16, 1, s) == 0
    gy = bf(1, 8, 8, 16, 16)
    dxo = torch.zeros(1, 4, 4, 8, 16, device=DEV, dtype=torch.bfloat16)
    ne = lib.ltu_trilinear_adjoint_ws_elems(1, 4, 4, 8, 16, 2)
    tws = torch.zeros(ne, device=DEV, dtype=torch.bfloat16)
    assert lib.ltu_trilinear_adjoint(gy.data_ptr(), 0, dxo.data_ptr(), tws.data_ptr(), ne - 1, 1, 4, 4, 8, 16, 2, 1, s) == -4
    assert lib.ltu_trilinear_adjoint(gy.data_ptr(), 0, dxo.data_ptr(), tws.data_ptr(), ne, 1, 4, 4, 8, 16, 2, 1, s) == 0
    pr = torch.rand(1, 4096, 2, device=DEV)
    lab = torch.zeros(1, 4096, dtype=torch.uint8, device=DEV)
    nl = lib.ltu_loss_ws_floats(1, 4096, 2)
    lsum, vals, coef = torch.zeros(nl, device=DEV), torch.zeros(9, device=DEV), torch.zeros(1, 2, 3, device=DEV)
    wd = (ctypes.c_float * 5)(1, 1, 0, 0, 0)
    assert lib.ltu_loss_fwd(pr.data_ptr(), lab.data_ptr(), lsum.data_ptr(), nl - 1, vals.data_ptr(), coef.data_ptr(), 1, 4096, 2, 1.0, 0.0, wd, 0, s) == -4
    assert lib.ltu_loss_fwd(pr.data_ptr(), lab.data_ptr(), lsum.data_ptr(), nl, vals.data_ptr(), coef.data_ptr(), 1, 4096, 2, 1.0, 0.0, wd, 0, s) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize('M,d,layers', [(2048, 256, 8), (1024, 256, 8), (2048, 128, 8), (4320, 256, 2), (2048, 256, 3)])
def test_linear_wgrad_group_of_layers(ops, M, d, layers):
    """the groups of several layers of a small level as ONE launch (ops.Context.wgrad_group_push keeps them back): with 32 jobs
    every tile has a single owner, which adds its sums to the gradient itself (no partial tiles, no fold); a bias gradient may be
    absent"""
    g = G(37)
    bf = lambda t: t.bfloat16()
    shapes = [(3 * d, d, 3), (d, d, 1), (2 * d, d, 1), (d, 2 * d, 1)]
    lc = ops.Context()
    want, bufs = [], []
    for lay in range(layers):
        for ji, (N, K, nw) in enumerate(shapes):
            gr, x = bf(torch.randn(M, N, generator=g) * 0.1).to(DEV), bf(torch.randn(M, K, generator=g)).to(DEV)
            dws = [torch.full((N // nw, K), 0.5, device=DEV) for _ in range(nw)]
            dbs = [torch.full((N // nw,), -0.25, device=DEV) for _ in range(nw)]
            lc.wgrad_group_push(gr, x, dws, dbs, M, N, K, ji == 3)
            want.append((gr.float().t() @ x.float() + 0.5, gr.float().sum(0) - 0.25))
            bufs.append((dws, dbs))
        if lay < layers - 1 and 4 * (lay + 1) < 32:
            assert len(lc.wg_group) == 4 * (lay + 1)        # kept back: these levels fit ops.WGRAD_DEFER_MB
    lc.flush_deferred()
    assert not lc.wg_group and lc.wg_bytes == 0
    for (dw_ref, db_ref), (dws, dbs) in zip(want, bufs):
        dw, db = torch.cat(dws, 0), torch.cat(dbs, 0)
        assert rel_err(dw, dw_ref) < 2e-5 and rel_err(db, db_ref) < 2e-5


# ---------------------------------------------------------------------------------------------- linear attention
def _qkv_pack(q, k, v):
    B, h, N, dk = q.shape
    f = lambda t: t.transpose(1, 2).reshape(B * N, h * dk)
    return torch.cat((f(q), f(k), f(v)), dim=1).contiguous()


@pytest.mark.parametrize('tag', list(seedgen.LINATTN_CASES))
def test_linattn_golden(ops, golden_dir, tag):
    Gd = np.load(os.path.join(golden_dir, 'linattn.npz'))
    q, k, v, go = seedgen.linattn_case(tag)
    B, h, N, dk = q.shape
    d = h * dk
    qkv = _qkv_pack(q, k, v).to(DEV).requires_grad_(True)
    out = ops.linear_attention(qkv, B, N, d)
    out.backward(go.transpose(1, 2).reshape(B * N, d).to(DEV))
    ref = torch.from_numpy(Gd[f'{tag}_out']).transpose(1, 2).reshape(B * N, d)
    assert rel_err(out, ref) < 1e-4
    dref = _qkv_pack(*(torch.from_numpy(Gd[f'{tag}_d{n}']) for n in 'qkv'))
    assert rel_err(qkv.grad[:, :d], dref[:, :d]) < 2e-4
    assert rel_err(qkv.grad[:, d:2 * d], dref[:, d:2 * d]) < 2e-4
    assert rel_err(qkv.grad[:, 2 * d:], dref[:, 2 * d:]) < 2e-4


@pytest.mark.parametrize('B,h,N', [(2, 1, 40), (1, 2, 1000), (2, 4, 4097), (1, 8, 2500)])
def test_linattn_sizes(ops, B, h, N):
    g = G(8)
    q, k, v, go = (torch.randn(B, h, N, 32, generator=g) for _ in range(4))
    k[:, :, N // 3] += 8.0             # late dominant token: the running max must rescale the accumulators
    k[:, :, 0] += 4.0
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    ref = O_net.linear_attention(qr, kr, vr)
    ref.backward(go)
    d = h * 32
    qkv = _qkv_pack(q, k, v).to(DEV).requires_grad_(True)
    out = ops.linear_attention(qkv, B, N, d)
    out.backward(go.transpose(1, 2).reshape(B * N, d).to(DEV))
    assert rel_err(out, ref.transpose(1, 2).reshape(B * N, d)) < 1e-4
    dref = _qkv_pack(qr.grad, kr.grad, vr.grad)
    for s in range(3):
        assert rel_err(qkv.grad[:, s * d:(s + 1) * d], dref[:, s * d:(s + 1) * d]) < 3e-4


@pytest.mark.parametrize('B,h,N', [(2, 4, 1000), (1, 8, 2500), (2, 8, 517)])
def test_linattn_bf16(ops, B, h, N):
    """bf16 storage: the 32x32 products run on the bf16 matrix cores (fp32 accumulation); compared with the fp32 oracle on
    bf16-rounded inputs, error relative to each tensor's max (bf16 rounding of the outputs alone is 4e-3)"""
    g = G(9)
    bf = lambda t: t.bfloat16().float()
    q, k, v, go = (bf(torch.randn(B, h, N, 32, generator=g)) for _ in range(4))
    k[:, :, N // 3] += 8.0
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    ref = O_net.linear_attention(qr, kr, vr)
    ref.backward(go)
    d = h * 32
    qkv = _qkv_pack(q, k, v).to(DEV, torch.bfloat16).requires_grad_(True)
    out = ops.linear_attention(qkv, B, N, d)
    assert out.dtype == torch.bfloat16
    out.backward(go.transpose(1, 2).reshape(B * N, d).to(DEV, torch.bfloat16))
    assert rel_err(out.float(), ref.transpose(1, 2).reshape(B * N, d)) < 1.5e-2
    dref = _qkv_pack(qr.grad, kr.grad, vr.grad)
    for s in range(3):
        assert rel_err(qkv.grad[:, s * d:(s + 1) * d].float(), dref[:, s * d:(s + 1) * d]) < 2e-2


def _linattn_vs_oracle(ops, B, h, N, dtype, seed=10, late=None):
    """forward + dq/dk/dv of the HIP core against oracle.net.linear_attention (model/trans_block.py:41-67) on the same inputs.
    `late`: token index that receives a dominant key (placed in a later 32-token tile of a split so that the running maximum is
    finite when it has to rescale the accumulators)"""
    g = G(seed)
    rnd = (lambda t: t.bfloat16().float()) if dtype == torch.bfloat16 else (lambda t: t)
    q, k, v, go = (rnd(torch.randn(B, h, N, 32, generator=g)) for _ in range(4))
    k[:, :, N // 3 if late is None else late] += 8.0
    k[:, :, 0] += 4.0
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    ref = O_net.linear_attention(qr, kr, vr)
    ref.backward(go)
    d = h * 32
    qkv = _qkv_pack(q, k, v).to(DEV, dtype).requires_grad_(True)
    out = ops.linear_attention(qkv, B, N, d)
    out.backward(go.transpose(1, 2).reshape(B * N, d).to(DEV, dtype))
    dref = _qkv_pack(qr.grad, kr.grad, vr.grad)
    errs = [rel_err(out.float(), ref.transpose(1, 2).reshape(B * N, d))]
    errs += [rel_err(qkv.grad[:, s * d:(s + 1) * d].float(), dref[:, s * d:(s + 1) * d]) for s in range(3)]
    l2 = lambda a, b: ((a.detach().double().cpu() - b.double()).norm() / b.double().norm()).item()
    errs += [l2(out, ref.transpose(1, 2).reshape(B * N, d))]
    errs += [l2(qkv.grad[:, s * d:(s + 1) * d], dref[:, s * d:(s + 1) * d]) for s in range(3)]
    return errs            # max-abs error relative to the tensor's max (out, dq, dk, dv), then relative L2 of the same four


def _bf16_ok(errs):
    """bf16 storage: q-softmax, context and output are each rounded to 8 significant bits, so single elements of a 32-term dot
    product move by up to ~2e-2 of the tensor's maximum; the relative L2 error stays at the bf16 rounding level"""
    return max(errs[:4]) < 2.5e-2 and all(e < g for e, g in zip(errs[4:], (8e-3, 2.5e-2, 1.5e-2, 8e-3)))


# the token counts of the four transformers at 128^3: ROI level 1 (B=2, h=4, 57 408 tokens: 256
# tokens = 8 tiles per split, the shape bench.py times), ROI level 2, ROI level 3, bottleneck
HEADLINE = [(2, 4, 57408), (2, 8, 10752), (2, 8, 4320), (2, 8, 512)]


@pytest.mark.parametrize('B,h,N', HEADLINE)
def test_linattn_headline_fp32(ops, B, h, N):
    from lintransunet_amd import _lib
    tps = -(-N // max(1, 512 // B))
    tps = max(32, (tps + 31) // 32 * 32)
    assert _lib.load().ltu_linattn_splits(B, N) == -(-N // tps)
    # dominant key in the LAST tile of the first split (finite running max when it arrives)
    errs = _linattn_vs_oracle(ops, B, h, N, torch.float32, late=min(N, tps) - 1)
    assert errs[0] < 1e-4 and max(errs[1:4]) < 3e-4 and max(errs[4:]) < 1e-4, errs


@pytest.mark.parametrize('B,h,N', HEADLINE)
def test_linattn_headline_bf16(ops, B, h, N):
    tps = max(32, (-(-N // max(1, 512 // B)) + 31) // 32 * 32)
    errs = _linattn_vs_oracle(ops, B, h, N, torch.bfloat16, late=min(N, tps) - 1)
    assert _bf16_ok(errs), errs


@pytest.mark.parametrize('splits,B,h,N,late', [(4, 2, 2, 1000, 200), (2, 1, 4, 517, 258), (1, 1, 8, 333, 300), (6, 2, 4, 4097, 1300)])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_linattn_many_tiles_per_split(ops, splits, B, h, N, late, dtype):
    """few splits at small N (knob LTU_LA_SPLITS): every workgroup of linattn_kv_partial / linattn_dctx_partial walks several
    32-token tiles, so the in-kernel running-max rescale (finite m_run, alpha < 1) and the prefetch-next-tile pipeline run
    several iterations; the dominant key sits in a later tile of its split"""
    from lintransunet_amd import _lib
    _lib.config_set('LTU_LA_SPLITS', splits)
    try:
        nsplit = _lib.load().ltu_linattn_splits(B, N)
        assert N / nsplit > 64          # > 2 tiles per split
        errs = _linattn_vs_oracle(ops, B, h, N, dtype, seed=12, late=late)
    finally:
        _lib.config_set('LTU_LA_SPLITS', None)
    if dtype == torch.float32:
        assert errs[0] < 1e-4 and max(errs[1:4]) < 3e-4 and max(errs[4:]) < 1e-4, errs
    else:
        assert _bf16_ok(errs), errs


def test_attn_layer_golden(ops, golden_dir):
    """one whole post-norm layer (qkv GEMM, attention core, out-proj, LN, FFN, LN) vs the reference's vectors"""
    Gd = np.load(os.path.join(golden_dir, 'attn_layer.npz'))
    from lintransunet_amd.model import MaskTransUnet, _transformer_layer, _SeedStream
    d, B, N = 64, 2, 40
    lay = _transformer_layer(d)
    P = seedgen.seeded_params({k: tuple(v.shape) for k, v in lay.state_dict().items()}, seed=21)
    lay.load_state_dict(P)
    lay = lay.to(DEV)
    x = seedgen.seeded_volume((B, N, d), 22).to(DEV).requires_grad_(True)
    go = seedgen.seeded_volume((B, N, d), 23).to(DEV)
    class _NoStore:                      # per-call operand preparation (no weight store)
        class _S:
            lin = type('D', (dict,), {'__getitem__': lambda self, k: None})()
        _store = _S()
        _chain_ok = lambda self, *a: False
    xt = x.view(B * N, d)
    y, _, _ = MaskTransUnet._layer(_NoStore(), lay, xt, xt, B, N, d, 0.0, _SeedStream(0), last=True)
    y.backward(go.view(B * N, d))
    assert rel_err(y.view(B, N, d), torch.from_numpy(Gd['out'])) < 1e-4
    assert rel_err(x.grad, torch.from_numpy(Gd['dx'])) < 5e-4
    for k, p in lay.named_parameters():
        ref = torch.from_numpy(Gd['g_' + k])
        # the key bias has a mathematically zero gradient (softmax over tokens is shift invariant): absolute floor
        assert (p.grad.cpu() - ref).abs().max().item() < 5e-4 * max(ref.abs().max().item(), 1e-3), k


# ---------------------------------------------------------------------------------------------- stencils / resampling
@pytest.mark.parametrize('C', [32, 128])
def test_pos_conv(ops, C):
    g = G(9)
    B, H, W, D = 2, 5, 4, 6
    x = torch.randn(B, C, H, W, D, generator=g)
    w = torch.randn(C, 1, 3, 3, 3, generator=g) * 0.3
    b = torch.randn(C, generator=g)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    grid = xr.permute(0, 1, 4, 2, 3)                       # the reference's [B,C,D,H,W] view
    yr = (grid + F.conv3d(grid, wr, br, padding=1, groups=C)).permute(0, 1, 3, 4, 2)
    go = torch.randn(yr.shape, generator=g)
    yr.backward(go)
    xd, wd, bd = to_cl(x).requires_grad_(True), w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    yd = ops.pos_conv(xd, wd, bd)
    yd.backward(to_cl(go))
    assert rel_err(from_cl(yd), yr) < 1e-5
    assert rel_err(from_cl(xd.grad), xr.grad) < 1e-5
    assert rel_err(wd.grad, wr.grad) < 1e-4
    assert rel_err(bd.grad, br.grad) < 1e-4


@pytest.mark.parametrize('sd,shape', [(2, (2, 8, 3, 4, 5)), (1, (1, 16, 4, 4, 8)), (2, (1, 8, 1, 1, 8)), (1, (1, 8, 2, 2, 16))])
def test_trilinear(ops, sd, shape):
    g = G(10)
    x = torch.randn(shape, generator=g)
    xr = x.clone().requires_grad_(True)
    yr = F.interpolate(xr, scale_factor=(2, 2, sd), mode='trilinear', align_corners=True)
    go = torch.randn(yr.shape, generator=g)
    yr.backward(go)
    xd = to_cl(x).requires_grad_(True)
    yd = ops.trilinear_up(xd, sd)
    yd.backward(to_cl(go))
    assert rel_err(from_cl(yd), yr) < 1e-5
    assert rel_err(from_cl(xd.grad), xr.grad) < 1e-5
    # the separable adjoint (default) against the 64-tap gather it replaces, fp32 and bf16 storage, with a second gradient port
    for dt, tol in ((torch.float32, 1e-5), (torch.bfloat16, 1.5e-2)):
        go2 = torch.randn(yr.shape, generator=g)
        res = []
        for sep in (True, False):
            ops.SEPARABLE_TRILINEAR_ADJOINT = sep
            try:
                xq = to_cl(x).to(dt).requires_grad_(True)
                y1, y2 = ops.trilinear_up(xq, sd, fork=2)
                torch.autograd.backward([y1, y2], [to_cl(go).to(dt), to_cl(go2).to(dt)])
                res.append(xq.grad.float())
            finally:
                ops.SEPARABLE_TRILINEAR_ADJOINT = True
        assert rel_err(res[0], res[1]) < tol, dt


def _with_knob(name, value, fn):
    """run fn() with a run-time knob of the library set (ltu_config_set), then clear it"""
    from lintransunet_amd import _lib
    _lib.call('ltu_config_set', name, value, 0)
    try:
        return fn()
    finally:
        _lib.call('ltu_config_set', name, 0, 1)


@pytest.mark.parametrize('sd,shape', [(2, (2, 8, 5, 7, 6)), (1, (1, 16, 9, 4, 8)), (2, (1, 8, 3, 3, 3)), (2, (2, 32, 4, 5, 7)),
                                      (2, (1, 128, 2, 3, 5)), (2, (1, 520, 2, 2, 3))])
def test_trilinear_adjoint_row_pairs(ops, sd, shape):
    """the separable adjoint with two adjacent output rows per workgroup (merged candidate table) against one row per workgroup
    (LTU_TRI_NO_PAIR): the same terms in the same order, so bit-identical; odd lengths leave a last pair with one row.  Short rows
    (the depth pass: C elements) take several pairs per workgroup (tri_adj1d_pair_rows_kernel); LTU_TRI_NO_ROWS is the one-pair
    kernel: bit-identical as well (the padded union entries carry weight 0)"""
    g = G(12)
    x = torch.randn(shape, generator=g)
    out = []
    go1 = torch.randn(shape[0], shape[1], 2 * shape[2], 2 * shape[3], sd * shape[4], generator=g)
    go2 = torch.randn(go1.shape, generator=g)
    for dt in (torch.float32, torch.bfloat16):

        def run():
            xq = to_cl(x).to(dt).requires_grad_(True)
            y1, y2 = ops.trilinear_up(xq, sd, fork=2)
            torch.autograd.backward([y1, y2], [to_cl(go1).to(dt), to_cl(go2).to(dt)])
            return xq.grad.float().clone()
        a, b = run(), _with_knob(b'LTU_TRI_NO_PAIR', 1, run)
        assert torch.equal(a, b), dt
        assert torch.equal(a, _with_knob(b'LTU_TRI_NO_ROWS', 1, run)), dt
        out.append(a)
    assert rel_err(out[1], out[0]) < 1.5e-2


def test_conv3d_persistent_brick_orders(ops):
    """the persistent few-channel convs with contiguous brick runs per workgroup (XCD-aware, default) against the strided order
    (LTU_HALO_NO_XCD): the same bricks, bit-identical results; 720 ragged bricks on 512 workgroups"""
    from lintransunet_amd import _lib
    if not _lib.experiments():
        pytest.skip('the strided order is compiled into an experiments build only (make EXPERIMENTS=1)')
    g = G(13)
    for Ci, Co in ((16, 16), (32, 32)):
        x = torch.randn(1, Ci, 36, 38, 60, generator=g).bfloat16()
        w = (torch.randn(Co, Ci, 3, 3, 3, generator=g) * 0.1).bfloat16().float()
        b = torch.randn(Co, generator=g)
        go = torch.randn(1, Co, 36, 38, 60, generator=g).bfloat16()

        def run():
            xd = to_cl(x.float(), torch.bfloat16).requires_grad_(True)
            wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
            yd = ops.conv3d(xd, wd, bd)
            yd.backward(to_cl(go.float(), torch.bfloat16))
            return yd.detach().float().clone(), xd.grad.float().clone()
        (y0, dx0), (y1, dx1) = run(), _with_knob(b'LTU_HALO_NO_XCD', 1, run)
        assert torch.equal(y0, y1) and torch.equal(dx0, dx1), (Ci, Co)


def test_level_loss_vector_path(ops):
    """level losses: four voxels per thread (default when S % 4 == 0) against one voxel per thread (LTU_LOSS_SCALAR); the sums
    differ in association only, the gradients not at all"""
    g = G(14)
    for C in (2, 3):
        B, S = 2, 4 * 1237
        logits = torch.randn(B, S, C, generator=g)
        lab = torch.randint(0, C, (B, S), generator=g).to(torch.uint8).to(DEV)

        def run():
            p = torch.softmax(logits, -1).to(DEV).requires_grad_(True)
            tot, values = ops.level_loss(p, lab, 1.0, 1.0, [1.0] * 4 + [1.0])
            tot.backward()
            keep = [0, 1, 2] + [3 + c for c in range(C)] + [7]        # total, CE, balanced Dice, Dice per class, foreground Dice
            return torch.cat((tot.detach().reshape(1), values.detach().reshape(-1)[keep])).clone(), p.grad.clone()
        (v0, g0), (v1, g1) = run(), _with_knob(b'LTU_LOSS_SCALAR', 1, run)
        assert rel_err(v0, v1) < 1e-5
        assert rel_err(g0, g1) < 1e-5


def test_roi_golden(ops, golden_dir):
    """box finder (bit-exact), both warps and their adjoints against the reference's vectors, all edge cases"""
    Gd = np.load(os.path.join(golden_dir, 'roi.npz'))
    for name in Gd['names']:
        mask = torch.from_numpy(Gd[f'{name}_mask'])            # bool [1,1,H,W,D]
        roi_size = int(Gd[f'{name}_roi_size'])
        fg = mask[:, 0].float()
        prob = torch.stack((1 - fg, fg), dim=-1).contiguous().to(DEV)      # [1,H,W,D,2]: 1 - p0 = fg
        plan = ops.RoiPlan(prob, roi_size, 0.5)
        assert torch.equal(plan.box.cpu(), torch.from_numpy(Gd[f'{name}_box'])), name
        feat = torch.from_numpy(Gd[f'{name}_feat'])
        # feature fixtures have 2 channels; the kernels work on 4-channel vectors
        pad = lambda t: to_cl(torch.cat((t, torch.zeros_like(t)), dim=1))
        fd = pad(feat).requires_grad_(True)
        roi = ops.roi_warp(fd, plan)
        assert rel_err(from_cl(roi)[:, :2], torch.from_numpy(Gd[f'{name}_roi'])) < 1e-4, name
        roi.backward(pad(torch.from_numpy(Gd[f'{name}_groi'])))
        assert rel_err(from_cl(fd.grad)[:, :2], torch.from_numpy(Gd[f'{name}_dfeat'])) < 1e-4, name
        rin = pad(torch.from_numpy(Gd[f'{name}_roi_in'])).requires_grad_(True)
        back = ops.roi_unwarp(rin, plan)
        assert rel_err(from_cl(back)[:, :2], torch.from_numpy(Gd[f'{name}_back'])) < 1e-4, name
        back.backward(pad(torch.from_numpy(Gd[f'{name}_gback'])))
        assert rel_err(from_cl(rin.grad)[:, :2], torch.from_numpy(Gd[f'{name}_droi_in'])) < 1e-4, name


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_output_ports_sum_gradients_in_kernel(ops, dtype):
    """a tensor with several consumers is produced with one autograd port per consumer; the producer's backward kernel receives all
    gradient tensors and sums them on load.  Equivalent to one consumer that receives the summed gradient."""
    g = G(41)
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    B, H, W, D, C = 2, 6, 5, 8, 32
    x = torch.randn(B, H, W, D, C, generator=g).to(DEV, dtype)
    mk = lambda *s: torch.randn(*s, generator=g).to(DEV, dtype)
    # trilinear: two ports
    c1, c2 = mk(B, 2 * H, 2 * W, 2 * D, C), mk(B, 2 * H, 2 * W, 2 * D, C)
    xa = x.clone().requires_grad_(True)
    ya, yb = ops.trilinear_up(xa, 2, fork=2)
    ((ya * c1).float().sum() + (yb * c2).float().sum()).backward()
    xb = x.clone().requires_grad_(True)
    (ops.trilinear_up(xb, 2) * (c1.float() + c2.float()).to(dtype)).float().sum().backward()
    assert rel_err(xa.grad.float(), xb.grad.float()) < tol
    # positional conv: two ports
    w, b = (torch.randn(C, 1, 3, 3, 3, generator=g) * 0.2).to(DEV), torch.zeros(C, device=DEV)
    c1, c2 = mk(B, H, W, D, C), mk(B, H, W, D, C)
    wa, wb = w.clone().requires_grad_(True), w.clone().requires_grad_(True)
    xa = x.clone().requires_grad_(True)
    ya, yb = ops.pos_conv(xa, wa, b.clone().requires_grad_(True), fork=2)
    ((ya * c1).float().sum() + (yb * c2).float().sum()).backward()
    xb = x.clone().requires_grad_(True)
    (ops.pos_conv(xb, wb, b.clone().requires_grad_(True)) * (c1.float() + c2.float()).to(dtype)).float().sum().backward()
    assert rel_err(xa.grad.float(), xb.grad.float()) < tol and rel_err(wa.grad, wb.grad) < tol
    # InstanceNorm + LeakyReLU + residual: three ports of the block input (conv branch, residual, residual duplicate), two ports
    # of the block output -- the encoder's pattern
    c1, c2 = mk(B, H, W, D, C), mk(B, H, W, D, C)
    src = x.clone().requires_grad_(True)
    t, t_r, t_r2 = ops.instnorm_act(src, fork=3)
    s1, s2 = ops.instnorm_act(t * 1.5, res=t_r, res_dup=t_r2, fork=2)
    ((s1 * c1).float().sum() + (s2 * c2).float().sum()).backward()
    ref = x.clone().requires_grad_(True)
    t0 = ops.instnorm_act(ref)
    (ops.instnorm_act(t0 * 1.5, res=t0) * (c1.float() + c2.float()).to(dtype)).float().sum().backward()
    assert rel_err(src.grad.float(), ref.grad.float()) < tol


# ---------------------------------------------------------------------------------------------- heads, gate, losses
def test_softmax_heads(ops):
    g = G(11)
    for C in (2, 3):
        z = torch.randn(2, 4, 3, 5, 6, generator=g) * 2           # [B,CP=4,H,W,D]
        zr = z.clone().requires_grad_(True)
        pr = torch.softmax(zr[:, :C], dim=1)
        go = torch.randn(pr.shape, generator=g)
        pr.backward(go)
        zd = to_cl(z).requires_grad_(True)
        pd = ops.head_softmax(zd, C)
        pd.backward(to_cl(go))
        assert rel_err(from_cl(pd), pr) < 1e-6
        assert rel_err(from_cl(zd.grad), zr.grad) < 1e-5
        zf = torch.randn(2, 4 * C, 3, 4, 5, generator=g)
        zfr = zf.clone().requires_grad_(True)
        pf = torch.softmax(O_net.window_unembed(zfr), dim=1)
        gf = torch.randn(pf.shape, generator=g)
        pf.backward(gf)
        zfd = to_cl(zf).requires_grad_(True)
        pfd = ops.final_softmax(zfd, C)
        pfd.backward(to_cl(gf))
        assert rel_err(from_cl(pfd), pf) < 1e-6
        assert rel_err(from_cl(zfd.grad), zfr.grad) < 1e-5
        oh = ops.onehot_argmax(pfd.detach())
        ref = torch.zeros_like(pf.detach()).scatter_(1, pf.detach().argmax(1, keepdim=True), 1)
        assert torch.equal(from_cl(oh), ref)


@pytest.mark.parametrize('C,Cg', [(8, 8), (16, 32), (128, 256)])
def test_attention_gate(ops, C, Cg):
    g = G(12)
    B, H, W, D = 2, 4, 3, 5
    skip, up = torch.randn(B, C, H, W, D, generator=g), torch.randn(B, Cg, H, W, D, generator=g)
    names = {'G.W_x.0': (C, C), 'G.W_g.0': (C, Cg), 'G.psi.0': (1, C)}
    P = {}
    for n, (o, i) in names.items():
        P[n + '.weight'] = (torch.randn(o, i, 1, 1, 1, generator=g) / i ** 0.5).requires_grad_(True)
        P[n + '.bias'] = (0.1 * torch.randn(o, generator=g)).requires_grad_(True)
    sr, ur = skip.clone().requires_grad_(True), up.clone().requires_grad_(True)
    outr = sr * O_net.attention_gate(P, 'G', sr, ur)
    go = torch.randn(outr.shape, generator=g)
    outr.backward(go)
    Pd = {k: v.detach().to(DEV).requires_grad_(True) for k, v in P.items()}
    sd_, ud = to_cl(skip).requires_grad_(True), to_cl(up).requires_grad_(True)
    outd = ops.attention_gate(sd_, ud, Pd['G.W_x.0.weight'], Pd['G.W_x.0.bias'], Pd['G.W_g.0.weight'], Pd['G.W_g.0.bias'],
                              Pd['G.psi.0.weight'], Pd['G.psi.0.bias'])
    outd.backward(to_cl(go))
    assert rel_err(from_cl(outd), outr) < 1e-4
    assert rel_err(from_cl(sd_.grad), sr.grad) < 5e-4
    assert rel_err(from_cl(ud.grad), ur.grad) < 5e-4
    for k in P:
        if k.endswith('bias') and 'psi' not in k:
            continue          # bias of a conv feeding InstanceNorm: gradient is exactly 0 up to rounding
        assert rel_err(Pd[k].grad, P[k].grad) < 1e-3, k


def test_losses_golden(ops, golden_dir):
    from lintransunet_amd import losses as L
    Gd = np.load(os.path.join(golden_dir, 'losses.npz'))
    p = torch.from_numpy(Gd['c2_p'])
    lab = torch.from_numpy(Gd['c2_lab'])
    for name in ('CrossEntroLoss', 'DiceClassLoss', 'BalanceDiceLoss'):
        pd = to_cl(p).requires_grad_(True)
        v = L.get_criterions([name])[name](pd.permute(0, 4, 1, 2, 3), lab.to(DEV))
        v.backward()
        assert abs(v.item() - float(Gd[f'c2_{name}'])) < 1e-5 * max(1, abs(float(Gd[f'c2_{name}']))), name
        assert rel_err(from_cl(pd.grad), torch.from_numpy(Gd[f'c2_{name}_dp'])) < 1e-4, name
    p3 = torch.from_numpy(Gd['c3_p'])
    lab3 = torch.from_numpy(Gd['c3_lab'])
    for name in ('CrossEntroLoss', 'DiceClassLoss', 'DiceClassLoss2', 'DiceClassLoss0'):
        pd = to_cl(p3).requires_grad_(True)
        v = L.get_criterions([name])[name](pd.permute(0, 4, 1, 2, 3), lab3.to(DEV))
        v.backward()
        assert abs(v.item() - float(Gd[f'c3_{name}'])) < 1e-4, name
        assert rel_err(from_cl(pd.grad), torch.from_numpy(Gd[f'c3_{name}_dp'])) < 1e-4, name
    # fused level criterion = weighted sum of the single losses
    pd = to_cl(p).requires_grad_(True)
    tot, named = L.LevelCriterion({'CrossEntroLoss': 1.0, 'BalanceDiceLoss': 1.0}, scale=0.4)(pd.permute(0, 4, 1, 2, 3), lab.to(DEV))
    want = 0.4 * (float(Gd['c2_CrossEntroLoss']) + float(Gd['c2_BalanceDiceLoss']))
    assert abs(tot.item() - want) < 1e-5
    # a device-resident run-time scale multiplies the same total and gradient (captured graphs follow per-epoch level weights)
    pd2 = to_cl(p).requires_grad_(True)
    sc = torch.tensor([0.4], device=DEV)
    tot2, _ = L.LevelCriterion({'CrossEntroLoss': 1.0, 'BalanceDiceLoss': 1.0}, scale_dev=sc)(pd2.permute(0, 4, 1, 2, 3), lab.to(DEV))
    tot.backward(); tot2.backward()
    assert abs(tot2.item() - want) < 1e-5 and rel_err(pd2.grad, pd.grad) < 1e-6
    # the evaluation losses train3D.py:143 asks get_criterions for (eval_list), on un-thresholded probabilities
    ev = L.get_criterions(['BalanceDiceLoss', 'DiceClassLoss', 'RecallLoss', 'PrecisionLoss', 'LocalizationLoss'])
    for name in ('RecallLoss', 'PrecisionLoss', 'LocalizationLoss'):
        v = ev[name](to_cl(p).permute(0, 4, 1, 2, 3), lab.to(DEV))
        assert abs(v.item() - float(Gd[f'c2_{name}'])) < 1e-5 * max(1.0, abs(float(Gd[f'c2_{name}']))), name


def test_label_pyramid(ops):
    from lintransunet_amd import train
    from oracle import step as O_step
    lab = seedgen.seeded_label((2, 1, 32, 32, 16), 5)
    ref = O_step.label_pyramid(lab, 5)
    got = train.label_pyramid(lab.to(DEV), 5)
    for a, b in zip(got, ref):
        assert torch.equal(a.cpu().float(), b[:, 0].float())


@pytest.mark.gpu
@pytest.mark.parametrize('G', [2, 4, 8, 16, 32, 64])
def test_group_reduce_selftest(G):
    """the DPP / permlane-swap reductions of common.h against torch, all-negative input (a zero injected by a mis-set DPP bound
    control, or a swap that returns one half twice, shows in the max as well as in the sum)"""
    from lintransunet_amd import _lib
    from lintransunet_amd.ops import _p, _s
    g = torch.Generator().manual_seed(G)
    x = (-1.0 - 3.0 * torch.rand(64 * 12, generator=g)).to(DEV)
    s, m = torch.empty_like(x), torch.empty_like(x)
    _lib.call('ltu_selftest_group_reduce', _p(x), _p(s), _p(m), x.numel(), G, _s())
    ref_s = x.view(-1, G).sum(1, keepdim=True).expand(-1, G).reshape(-1)
    ref_m = x.view(-1, G).max(1, keepdim=True).values.expand(-1, G).reshape(-1)
    assert torch.allclose(s, ref_s, rtol=1e-5, atol=1e-5)
    assert torch.equal(m, ref_m)


@pytest.mark.parametrize('nwg,n,skew', [(512, 128, 5), (1024, 32, 3), (256, 256, 7), (777, 64, 4)])
def test_last_arriver_reduce(nwg, n, skew):
    """the in-launch 'last arriver' fold (csrc/misc.hip: write-through partial rows, agent-scope ticket, one acquire by the last
    workgroup - the guide's hand-off recipe R1) against the two-stage fold the step uses: uneven per-workgroup load, an L1-warm
    consumer (every workgroup pre-reads the previous launch's partial rows), 2-4 workgroups per CU, 10^4 launches in ONE process on
    alternating data, every output word compared bit for bit.  (VERDICT round 2, item 6.  The reducer is correct here; it is still
    not used in the step because it does not pay: profiles/r03_last_arriver.txt, profiles/HISTORY.md finding 15.)"""
    from lintransunet_amd import _lib
    from lintransunet_amd.ops import _p, _s
    if not _lib.experiments():
        pytest.skip('ltu_selftest_last_arriver is exported by an experiments build only (make EXPERIMENTS=1)')
    rpc = 4
    rows = sum(1 + (7 * i) % skew for i in range(nwg)) * rpc
    g = G(77)
    xs = [torch.randn(rows, n, generator=g).to(DEV) * (1 + k) for k in range(2)]
    part = torch.zeros(nwg * n, device=DEV)
    sink = torch.zeros(nwg, device=DEV)
    counter = torch.zeros(1, device=DEV, dtype=torch.int32)
    refs = []
    for x in xs:                                         # two-stage reference
        out = torch.empty(n, device=DEV)
        _lib.call('ltu_selftest_last_arriver', _p(x), _p(part), _p(out), _p(counter), _p(sink), nwg, n, rpc, skew, 0, _s())
        refs.append(out)
        # and the plain sum, to make sure the reference itself means something
        assert torch.allclose(out.cpu(), x.double().sum(0).float().cpu(), rtol=1e-3, atol=1e-2)
    assert not torch.equal(refs[0], refs[1])
    out = torch.empty(n, device=DEV)
    bad = torch.zeros((), device=DEV, dtype=torch.int64)
    for k in range(10000):
        _lib.call('ltu_selftest_last_arriver', _p(xs[k & 1]), _p(part), _p(out), _p(counter), _p(sink), nwg, n, rpc, skew, 1, _s())
        bad += (out != refs[k & 1]).sum()
    torch.cuda.synchronize()
    assert int(bad.item()) == 0, f'{int(bad.item())} stale / wrong output words in 10^4 launches'
    assert int(counter.item()) == 0 and float(sink.abs().sum().item()) == 0.0
