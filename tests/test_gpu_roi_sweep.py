"""roi_hist_kernel / roi_plan_kernel (csrc/roi.hip) on the seeded case family of tests/roi_common.py, 8 different cases per
ops.RoiPlan call: boxes and all four plans' taps bit for bit against the reference's fixture tests/golden/roi_sweep.npz (which
tests/test_roi_sweep.py pins the oracle and the float32 replay to), the dense tap matrices and the end-to-end warps inside bounds
derived from the float32 roundings of a tap, the adjoint lists against the forward taps, and the histogram's launch-geometry edges
against the oracle computed live.  LTU_ROI_SWEEP_REPORT=<file> appends every bounded comparison's worst error / bound
(profiles/roi_sweep_margins.txt)."""
import os

import numpy as np
import pytest
import torch

from oracle import roi as O_roi
from tests import roi_common as RC
from tests import stream_common as R
from tests.test_gpu_token_paths import BF16_ABS, BF16_REL

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PLANS = ('fh', 'fw', 'bh', 'bw')
U = 2.0 ** -24                      # unit roundoff of float32


def _report(what, ratio):
    print(f'[roi sweep] {what}: worst error / bound {ratio:.4f}')
    path = os.environ.get('LTU_ROI_SWEEP_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(f'{what}\t{ratio:.4f}\n')


@pytest.fixture(scope='module')
def ops():
    from lintransunet_amd import ops as _ops
    assert torch.cuda.is_available()
    return _ops


def plan_coords(Gd, g, k):
    """{plan: (reference coordinates of case k, source length)}"""
    H, W, _, roi_size = RC.GEOMETRIES[g]
    geo = RC.roi_sizes(roi_size)
    up_h, up_w = 2 * ((geo['eval_h'] + 1) // 2), 2 * ((geo['eval_w'] + 1) // 2)
    return {'fh': (Gd[f'g{g}_fx'][k], H), 'fw': (Gd[f'g{g}_fy'][k], W), 'bh': (Gd[f'g{g}_bx'][k], up_h), 'bw': (Gd[f'g{g}_by'][k], up_w)}


def plan_taps(ib, fb, p, B):
    """(src0 [B][ND], wt [B][ND][2]) as numpy"""
    ND = p['ND']
    return ib[p['src0']:p['src0'] + B * ND].reshape(B, ND).numpy(), fb[p['wt']:p['wt'] + B * ND * 2].reshape(B, ND, 2).numpy()


def tap_mismatches(src0, wt, coords, size):
    """destination indices of one sample whose taps differ from F.grid_sample's float32 taps of `coords` (src0 compared only where
    a weight is non-zero)"""
    s0, w0, w1 = RC.taps_f32(coords, size)
    assert src0.shape == s0.shape, (src0.shape, s0.shape)
    bad = (wt[:, 0].view(np.int32) != w0.view(np.int32)) & ~((wt[:, 0] == 0) & (w0 == 0))
    bad |= (wt[:, 1].view(np.int32) != w1.view(np.int32)) & ~((wt[:, 1] == 0) & (w1 == 0))
    bad |= ((w0 != 0) | (w1 != 0)) & (src0 != s0)
    return np.nonzero(bad)[0]


@pytest.fixture(scope='module')
def sweep(ops):
    """every batch of the family through ops.RoiPlan once: [dict(g, j, ks, C, thr, B, box, ib, fb, offs, mats)] on the CPU"""
    out = []
    with ops.use(ops.Context()):
        for g, j, ks, C, thr in RC.batches():
            H, W, D, roi_size = RC.GEOMETRIES[g]
            prob = RC.make_batch(g, ks, C, thr).to(DEV)
            plan = ops.RoiPlan(prob, roi_size, thr)
            torch.cuda.synchronize()
            offs = R.plan_offsets(len(ks), H, W, plan.eval_h, plan.eval_w)
            out.append(dict(g=g, j=j, ks=ks, C=C, thr=thr, B=len(ks), box=plan.box.cpu(), ib=plan.ibuf.cpu(), fb=plan.fbuf.cpu(), offs=offs, mats={}))
    return out


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(GOLDEN, 'roi_sweep.npz')))


def matrices(rec, name):
    if name not in rec['mats']:
        rec['mats'][name] = R.plan_matrices(rec['ib'], rec['fb'], rec['offs'][name], rec['B'])
    return rec['mats'][name]


def test_sweep_boxes_bit_equal_reference(sweep, golden):
    bad = []
    for rec in sweep:
        want = golden[f'g{rec["g"]}_box'][list(rec['ks'])]
        got = rec['box'].numpy()
        for b, k in enumerate(rec['ks']):
            if not np.array_equal(got[b].view(np.int32), want[b].view(np.int32)):
                bad.append((rec['g'], k, RC.KINDS[k], rec['C'], got[b].tolist(), want[b].tolist()))
    assert not bad, f'{len(bad)} of {sum(r["B"] for r in sweep)} boxes differ from the reference: {bad[:6]}'


@pytest.mark.parametrize('name', PLANS)
def test_sweep_taps_bit_equal_reference(sweep, golden, name):
    """src0 / wt of every case equal the float32 taps F.grid_sample derives from the reference's coordinates.
    Red before this test existed, for two reasons.  With one division per slope in map_back (the reference rounds a reciprocal, then
    a product) bh differed in 1 131 of 8 472 coordinates (74 cases) and bw in 798 of 7 872 (61 cases), fh and fw in none.  The commit
    before had that and products fused into the sums they feed (-ffp-contract=fast reaches through __fmul_rn): fh 653 of 4 632,
    fw 516 of 2 712, bh 1 770 of 8 472, bw 1 559 of 7 872 coordinates differed."""
    n_bad = n_all = 0
    cases = []
    for rec in sweep:
        assert rec['offs']['n_int'] == rec['ib'].numel() and rec['offs']['n_float'] == rec['fb'].numel(), (rec['g'], rec['j'])
        src0, wt = plan_taps(rec['ib'], rec['fb'], rec['offs'][name], rec['B'])
        for b, k in enumerate(rec['ks']):
            coords, size = plan_coords(golden, rec['g'], k)[name]
            assert size == rec['offs'][name]['NS']
            bad = tap_mismatches(src0[b], wt[b], coords, size)
            n_all += len(coords)
            if len(bad):
                n_bad += len(bad)
                cases.append((rec['g'], k, bad[:4].tolist()))
    print(f'[roi sweep] {name}: {n_bad} of {n_all} coordinates differ, {len(cases)} cases')
    assert n_bad == 0, f'{name}: {n_bad} of {n_all} coordinates in {len(cases)} cases differ from the reference taps: {cases[:6]}'


@pytest.mark.parametrize('name', PLANS)
def test_sweep_dense_taps_and_adjoint_lists(sweep, golden, name):
    """the dense gather matrix of every case within 4 * 2^-24 * size per entry of the float64 matrix of the reference's coordinates
    (ix carries three float32 roundings of values up to size, the weight one more; a coordinate that lands on an integer moves weight
    between neighbours continuously, so no case is excluded); the adjoint lists equal the transposed forward taps, with cnt <= L"""
    worst = 0.0
    for rec in sweep:
        p = rec['offs'][name]
        A, T = matrices(rec, name)
        assert torch.equal(T, A.transpose(1, 2)), (name, rec['g'], rec['j'])
        cnt = rec['ib'][p['cnt']:p['cnt'] + rec['B'] * p['NS']]
        assert int(cnt.min()) >= 0 and int(cnt.max()) <= p['L'], (name, rec['g'], rec['j'])
        for b, k in enumerate(rec['ks']):
            coords, size = plan_coords(golden, rec['g'], k)[name]
            err = np.abs(A[b].numpy() - RC.dense_f64(coords, size)).max()
            worst = max(worst, err / RC.tap_bound(size))
    _report(f'dense taps {name}', worst)
    assert worst <= 1.0, (name, worst)


# ---------------------------------------------------------------------------------------------- end to end

def _to_cl(t, dtype):
    return t.permute(0, 2, 3, 4, 1).contiguous().to(DEV, dtype)


def _from_cl(t):
    return t.detach().double().cpu().permute(0, 4, 1, 2, 3)


def _live_case(ops, geometry, kinds, seed_base):
    """(plan, oracle box, geo) of B = len(kinds) fresh cases of `geometry`, boxes checked bit for bit"""
    H, W, D, roi_size = geometry
    prob = torch.from_numpy(np.stack([RC.make_case(seed_base, k, 2, 0.5, geometry=geometry, kind=kind, pkind=RC.PKINDS[k % len(RC.PKINDS)])[1]
                                      for k, kind in enumerate(kinds)]))
    geo = O_roi.roi_geometry(roi_size)
    box = O_roi.find_boxes(RC.reference_mask(prob, 0.5), geo['min_h'], geo['min_w'])
    plan = ops.RoiPlan(prob.to(DEV), roi_size, 0.5)
    assert torch.equal(plan.box.cpu(), box), (plan.box.cpu(), box)
    return plan, box, geo


def _f64_matrices(box, geo, H, W, back):
    """per-sample float64 tap matrices of the oracle's coordinates and their tap-error envelopes: (Ah, Aw, Eh, Ew) [B][ND][NS]"""
    x0, y0, _, x1, y1, _ = torch.split(box, 1, dim=1)
    if back:
        gh, gw = O_roi.index_map_back(x0, x1, H - 1, geo['h_roi'], geo['eval_h']), O_roi.index_map_back(y0, y1, W - 1, geo['w_roi'], geo['eval_w'])
        sh, sw = 2 * ((geo['eval_h'] + 1) // 2), 2 * ((geo['eval_w'] + 1) // 2)
    else:
        gh, gw = O_roi.index_map_fwd(x0, x1, H - 1, geo['h_roi'], geo['eval_h']), O_roi.index_map_fwd(y0, y1, W - 1, geo['w_roi'], geo['eval_w'])
        sh, sw = H, W
    Ah = np.stack([RC.dense_f64(r, sh) for r in gh.numpy()])
    Aw = np.stack([RC.dense_f64(r, sw) for r in gw.numpy()])
    t = torch.from_numpy
    return t(Ah), t(Aw), t(RC.tap_bound(sh) * RC.widen(Ah)), t(RC.tap_bound(sw) * RC.widen(Aw))


def _gamma(n):
    return n * U / (1 - n * U)


def _e2e_bound(xabs, Ah, Aw, Eh, Ew, n_terms):
    """|kernel - float64| per element of (A_h (x) A_w) x: the tap envelopes E (|dA| <= 4 * 2^-24 * size on the support widened by one)
    propagated through |x|, plus the float32 arithmetic of the kernel's sum: every term is rounded as a product of the two weights, as
    a product with x and in at most n_terms additions"""
    first = R.plan_apply(xabs, Eh, Aw.abs()) + R.plan_apply(xabs, Ah.abs(), Ew) + R.plan_apply(xabs, Eh, Ew)
    return first + _gamma(2 + n_terms) * R.plan_apply(xabs, Ah.abs() + Eh, Aw.abs() + Ew)


def _run_e2e(ops, geometry, C, back, dtype, seed):
    H, W, D, roi_size = geometry
    kinds = ('box', 'pin_w1', 'small')
    with ops.use(ops.Context()):
        plan, box, geo = _live_case(ops, geometry, kinds, seed)
        B = len(kinds)
        assert len({tuple(r.tolist()) for r in box}) == B
        g = torch.Generator().manual_seed(seed)
        sh, sw = (plan.up_h, plan.up_w) if back else (H, W)
        x = torch.randn(B, C, sh, sw, D, generator=g).to(dtype).double().requires_grad_(True)
        like = torch.zeros(B, C, H, W, D, dtype=torch.float64)
        ref = O_roi.warp_from_roi(like, x, box, geo) if back else O_roi.warp_to_roi(x, box, geo)
        go = torch.randn(ref.shape, generator=g).to(dtype).double()
        ref.backward(go)
        xd = _to_cl(x.detach(), dtype).requires_grad_(True)
        y = (ops.roi_unwarp if back else ops.roi_warp)(xd, plan)
        y.backward(_to_cl(go, dtype))
        torch.cuda.synchronize()
    return box, geo, x.detach(), go, ref.detach(), x.grad, _from_cl(y), _from_cl(xd.grad)


@pytest.mark.parametrize('back', [False, True], ids=['warp', 'unwarp'])
@pytest.mark.parametrize('geometry,C', [((33, 47, 1, 16), 4), ((33, 47, 5, 16), 12), ((40, 36, 5, 20), 4)],
                         ids=['odd-eval D1 C4', 'odd-eval D5 C12', 'D5 C4'])
def test_roi_warp_fp32_end_to_end(ops, geometry, C, back):
    """ops.roi_warp / ops.roi_unwarp and their backward passes in fp32, B = 3 different boxes, against oracle.roi in float64 with the
    adjoints from autograd; per element, within the propagated tap bound plus the float32 arithmetic of the sum (four taps forward;
    the number of list entries meeting at a source element backward)"""
    H, W, D, _ = geometry
    box, geo, x, go, ref, dref, y, dx = _run_e2e(ops, geometry, C, back, torch.float32, 7 + C + D)
    Ah, Aw, Eh, Ew = _f64_matrices(box, geo, H, W, back)
    cl = lambda t: t.permute(0, 2, 3, 4, 1)
    bound = _e2e_bound(cl(x).abs(), Ah, Aw, Eh, Ew, 4)
    ratio = ((cl(y) - cl(ref)).abs() / bound.clamp_min(1e-300)).max().item()
    # backward: element (x, y) of the source sums one product per pair of list entries; the widened support bounds the list lengths
    nh, nw = (Eh != 0).sum(1), (Ew != 0).sum(1)                                   # [B][NS]
    n_terms = int((nh[:, :, None] * nw[:, None, :]).max())
    tr = lambda m: m.transpose(1, 2)
    bound_b = _e2e_bound(cl(go).abs(), tr(Ah), tr(Aw), tr(Eh), tr(Ew), n_terms)
    ratio_b = ((cl(dx) - cl(dref)).abs() / bound_b.clamp_min(1e-300)).max().item()
    which = 'unwarp' if back else 'warp'
    _report(f'fp32 {which} forward {geometry} C={C}', ratio)
    _report(f'fp32 {which} backward {geometry} C={C}', ratio_b)
    assert ratio <= 1.0 and ratio_b <= 1.0, (ratio, ratio_b)
    assert ref.abs().max() > 0.1 and dref.abs().max() > 0.1


@pytest.mark.parametrize('back', [False, True], ids=['warp', 'unwarp'])
def test_roi_warp_bf16_end_to_end(ops, back):
    """one bf16 case per direction against oracle.roi in float64 on the bf16 inputs, with the bf16 bound of the stream-path table:
    2^-8 |ref| + 1e-5 max|ref| per element"""
    geometry, C = (33, 47, 3, 16), 8
    box, geo, x, go, ref, dref, y, dx = _run_e2e(ops, geometry, C, back, torch.bfloat16, 31)
    which = 'unwarp' if back else 'warp'
    for what, got, want in (('forward', y, ref), ('backward', dx, dref)):
        bound = BF16_REL * want.abs() + BF16_ABS * want.abs().max()
        ratio = ((got - want).abs() / bound).max().item()
        _report(f'bf16 {which} {what} {geometry} C={C}', ratio)
        assert ratio <= 1.0, (what, ratio)


# ---------------------------------------------------------------------------------------------- launch geometry of the histogram

def _edge_masks(name):
    rs = np.random.RandomState(77)
    if name == 'capped at 256 blocks':                      # n / 4096 = 260 -> 256 blocks of 4160 voxels, half a row of 8320
        geometry = (128, 128, 65, 40)
        m = np.zeros((2, 128, 128, 65), bool)
        m[0, 37:90, 20:71, :] = rs.rand(53, 51, 65) < 0.5
        m[0, 3, 120, 64] = m[0, 127, 2, 0] = True
        m[1, 100:128, 0:9, 60:65] = True
    elif name == 'both axes at ROI_MAX_LEN':
        geometry = (512, 512, 1, 40)
        m = np.zeros((2, 512, 512, 1), bool)
        m[0, 300:512, 400:512, :] = rs.rand(212, 112, 1) < 0.7
        m[0, 511, 511, 0] = True
        m[1, 511, :, 0] = True
        m[1, :, 511, 0] = True
    elif name == 'D = 1':
        geometry = (33, 47, 1, 16)
        m = np.stack([RC.make_mask(rs, kind, 33, 47, 1, RC.roi_sizes(16)) for kind in ('box', 'tiny_h1', 'box_out', 'full')])
    else:                                                   # 4050 voxels < 4096: one block
        geometry = (30, 27, 5, 12)
        m = np.stack([RC.make_mask(rs, kind, 30, 27, 5, RC.roi_sizes(12)) for kind in ('box', 'pin_w0', 'out', 'empty')])
    return geometry, m


@pytest.mark.parametrize('name', ['capped at 256 blocks', 'both axes at ROI_MAX_LEN', 'D = 1', 'one block'])
def test_roi_hist_launch_geometry(ops, name):
    """boxes bit-equal to the oracle computed live, and all four plans' taps to the oracle's coordinates, where the histogram launch
    changes shape: the block count capped at 256, both axes at ROI_MAX_LEN with foreground in row and column 511, D = 1, one block"""
    (H, W, D, roi_size), m = _edge_masks(name)
    B = len(m)
    fg = torch.from_numpy(m).float()
    prob = torch.stack((1 - fg, fg), -1).contiguous()
    geo = O_roi.roi_geometry(roi_size)
    mask = RC.reference_mask(prob, 0.5)
    assert torch.equal(mask[:, 0], torch.from_numpy(m))
    box = O_roi.find_boxes(mask, geo['min_h'], geo['min_w'])
    with ops.use(ops.Context()):
        plan = ops.RoiPlan(prob.to(DEV), roi_size, 0.5)
        torch.cuda.synchronize()
        got, ib, fb = plan.box.cpu(), plan.ibuf.cpu(), plan.fbuf.cpu()
    assert torch.equal(got, box), (name, got, box)
    x0, y0, _, x1, y1, _ = torch.split(box, 1, dim=1)
    coords = {'fh': (O_roi.index_map_fwd(x0, x1, H - 1, geo['h_roi'], geo['eval_h']), H),
              'fw': (O_roi.index_map_fwd(y0, y1, W - 1, geo['w_roi'], geo['eval_w']), W),
              'bh': (O_roi.index_map_back(x0, x1, H - 1, geo['h_roi'], geo['eval_h']), plan.up_h),
              'bw': (O_roi.index_map_back(y0, y1, W - 1, geo['w_roi'], geo['eval_w']), plan.up_w)}
    offs = R.plan_offsets(B, H, W, plan.eval_h, plan.eval_w)
    assert offs['n_int'] == ib.numel() and offs['n_float'] == fb.numel()
    for pname, (gc, size) in coords.items():
        assert torch.isfinite(gc).all()
        src0, wt = plan_taps(ib, fb, offs[pname], B)
        for b in range(B):
            bad = tap_mismatches(src0[b], wt[b], gc[b].numpy(), size)
            assert len(bad) == 0, (name, pname, b, bad[:8])
