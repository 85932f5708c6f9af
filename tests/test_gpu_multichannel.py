"""GPU tests of the multi-channel input path (dim_input = 1 .. 4): ltu_window_embed_multi, the K-channel stem against the CPU
oracle, ltu_sample_channels against the single-channel gathers it must reproduce bit for bit, data.MultiScan from NIfTI files to
patches, sliding-window inference over K-channel volumes and the two captured paths."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lintransunet_amd import _lib, data, infer, nifti, ops, train          # noqa: E402
from lintransunet_amd.model import get_model_dict                          # noqa: E402
from oracle import net as O_net                                            # noqa: E402
from oracle import seedgen                                                 # noqa: E402
from oracle import step as O_step                                          # noqa: E402
from tests.test_gpu_model import (BF16_DICE_TOL, BF16_DICE_TOL_MOVED_BOX, SMALL, exact_zero_grad, grads_agree,    # noqa: E402
                                  rel_err)

DEV = 'cuda'


def embed_ref(x, k=2):
    """the K-channel window embedding, channel = c k^2 + kh k + kw: the inverse of oracle.net.window_unembed"""
    B, K, H, W, D = x.shape
    return x.reshape(B, K, H // k, k, W // k, k, D).permute(0, 1, 3, 5, 2, 4, 6).reshape(B, K * k * k, H // k, W // k, D)


# ---- 1. embedding ---------------------------------------------------------------------------------------------------------------

def test_embed_ref_inverts_the_oracle_unembedding():
    y = torch.randn(2, 12, 3, 2, 3)
    assert torch.equal(embed_ref(O_net.window_unembed(y)), y)
    x = torch.randn(2, 1, 6, 4, 3)
    assert torch.equal(embed_ref(x), O_net.window_embed(x))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('K', [1, 2, 3, 4])
def test_window_embed(K, dtype):
    x = torch.randn(2, K, 6, 4, 3, generator=torch.Generator().manual_seed(K))
    xd = x.to(DEV)
    y = ops.window_embed(xd, dtype)
    CP = 8 if K <= 2 else 16
    assert y.shape == (2, 3, 2, 3, CP) and y.dtype == dtype
    got = y.permute(0, 4, 1, 2, 3).cpu()
    assert torch.equal(got[:, :4 * K], embed_ref(x).to(dtype))
    assert (got[:, 4 * K:] == 0).all()
    # the multi-channel entry point itself at K = 1: the bits of ltu_window_embed
    if K == 1:
        y1 = torch.full_like(y, 7.0)
        _lib.call('ltu_window_embed_multi', xd.data_ptr(), y1.data_ptr(), ops._dt(y1), 2, 1, 6, 4, 3, None)
        assert torch.equal(y1.view(torch.uint8), y.view(torch.uint8))


def test_window_embed_refusals():
    x = torch.zeros(1, 5, 6, 4, 3, device=DEV)
    y = torch.full((1, 3, 2, 3, 24), 7.0, device=DEV)
    f = _lib.load().ltu_window_embed_multi
    assert f(x.data_ptr(), y.data_ptr(), ops.F32, 1, 2, 5, 4, 3, None) == -2          # odd H
    assert f(x.data_ptr(), y.data_ptr(), ops.F32, 1, 2, 6, 3, 3, None) == -2          # odd W
    assert f(x.data_ptr(), y.data_ptr(), ops.F32, 1, 5, 6, 4, 3, None) == -2          # K = 5
    assert f(x.data_ptr(), y.data_ptr(), ops.F32, 1, 0, 6, 4, 3, None) == -2
    assert f(0, y.data_ptr(), ops.F32, 1, 2, 6, 4, 3, None) == -4
    torch.cuda.synchronize()
    assert (y == 7.0).all()
    with pytest.raises(ValueError):
        ops.window_embed(x, torch.float32)


# ---- 2. the step against the oracle ---------------------------------------------------------------------------------------------

CFG3 = O_net.NetConfig(dim_input=3, **SMALL)
SIZE = (32, 32, 32)


def build(cfg, wseed=100, dtype=torch.float32, params=None):
    model = get_model_dict('MaskTransUnet')(cfg.num_layers, cfg.roi_size_list, cfg.is_roi_list, cfg.dim_input, cfg.dim_output,
                                            dropout=0.0, act_dtype=dtype)
    model.load_state_dict(params if params is not None else seedgen.seeded_params(O_net.param_shapes(cfg), wseed), strict=True)
    return model.to(DEV).train()


def inputs3():
    return seedgen.seeded_volume((2, 3) + SIZE, 101), seedgen.seeded_label((2, 1) + SIZE, 102)


@pytest.fixture(scope='module')
def oracle3():
    """oracle.step.train_step on the CPU with the K-channel embedding in place of oracle.net.window_embed (computed once, shared)"""
    mp = pytest.MonkeyPatch()
    mp.setattr(O_net, 'window_embed', embed_ref)
    try:
        x, label = inputs3()
        P = {k: v.clone().requires_grad_(True) for k, v in seedgen.seeded_params(O_net.param_shapes(CFG3), 100).items()}
        total, per_level, pred, masks = O_step.train_step(P, CFG3, x, label, O_step.dynamic_weights(0))
        boxes = []
        with torch.no_grad():
            O_net.forward({k: v.detach() for k, v in P.items()}, CFG3, x, training=True, boxes_out=boxes)
    finally:
        mp.undo()
    return dict(total=total.item(), levels=[[v.item() for v in vals] for vals in per_level], pred=pred, masks=masks, boxes=boxes,
                grads={k: v.grad for k, v in P.items()})


def step3(dtype):
    model = build(CFG3, dtype=dtype)
    x, label = (t.to(DEV) for t in inputs3())
    predict, masks = model(x)
    totals, named = train.deep_supervision_loss(predict, masks, label, O_step.dynamic_weights(0))
    torch.autograd.backward(totals, [torch.ones_like(t) for t in totals])
    torch.cuda.synchronize()
    return model, label, predict, masks, totals, named


def test_step_matches_oracle_fp32(oracle3):
    R = oracle3
    model, label, predict, masks, totals, named = step3(torch.float32)
    assert predict.shape == (2, 2) + SIZE
    assert len(model.last_boxes) == len(R['boxes'])
    for i, b in enumerate(model.last_boxes):
        assert torch.equal(b.cpu(), R['boxes'][i]), f'box{i}'
    assert rel_err(predict, R['pred']) <= 1e-3
    for i, m in enumerate(masks):
        assert rel_err(m, R['masks'][i]) <= 1e-3, f'mask{i}'
    total = sum(t.item() for t in totals)
    assert abs(total - R['total']) <= 1e-4 * max(1.0, abs(R['total']))
    for lvl, vals in enumerate(named):
        got = [v.item() for v in vals.values()]
        assert np.allclose(got, R['levels'][lvl], rtol=1e-4, atol=1e-5), (lvl, got, R['levels'][lvl])
    sd = dict(model.named_parameters())
    worst = 0.0
    for k, g in R['grads'].items():
        if g is None:
            assert sd[k].grad is None, k
            continue
        got = sd[k].grad.double().norm().item()
        if exact_zero_grad(k):
            assert got <= 1e-2, k
            continue
        n = g.double().norm().item()
        worst = max(worst, abs(got - n) / max(n, 1e-3))
    print(f'[K = 3 fp32] worst gradient-norm deviation {worst:.2e}')
    assert worst <= 1e-2, worst
    gw = sd['encode.input_block.weight'].grad
    assert gw.shape == (8, 12, 3, 3, 3)
    err = rel_err(gw, R['grads']['encode.input_block.weight'])
    print(f'[K = 3 fp32] stem weight gradient rel err {err:.2e}')
    assert err <= 5e-3
    # every input channel's block of the stem gradient is alive
    assert all(gw[:, 4 * c:4 * c + 4].abs().max().item() > 0 for c in range(3))


def test_step_matches_oracle_bf16_dice(oracle3):
    from lintransunet_amd import losses as L
    R = oracle3
    model, label, predict, masks, totals, named = step3(torch.bfloat16)
    dice = L.DiceClassLoss()(predict.detach(), label).item()
    ref = L.DiceClassLoss()(R['pred'].to(DEV), label).item()
    moved = max((b.cpu() - R['boxes'][i]).abs().max().item() for i, b in enumerate(model.last_boxes))
    print(f'[K = 3 bf16] dice {dice:.6f} vs {ref:.6f} (d {dice - ref:+.2e}), largest box move {moved}')
    assert moved <= 1.0
    assert abs(dice - ref) <= (BF16_DICE_TOL if moved == 0 else BF16_DICE_TOL_MOVED_BOX)
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


# ---- 3. channels beyond the first enter, and only through the weights ----------------------------------------------------------------

def test_zero_weight_channel_is_inert():
    """A K = 2 model whose stem weights of channel 1 are zero computes what the K = 1 model with the remaining weights computes on
    channel 0, whatever channel 1 holds.  Both pack to 8 stem channels, so the kernels see the same operands except for products
    with zero: bit-equal outputs and masks."""
    cfg1, cfg2 = O_net.NetConfig(dim_input=1, **SMALL), O_net.NetConfig(dim_input=2, **SMALL)
    P1 = seedgen.seeded_params(O_net.param_shapes(cfg1), 100)
    P2 = {k: v.clone() for k, v in P1.items()}
    w = torch.zeros(8, 8, 3, 3, 3)
    w[:, :4] = P1['encode.input_block.weight']
    P2['encode.input_block.weight'] = w
    x = seedgen.seeded_volume((2, 2) + SIZE, 103)
    x[:, 1] = x[:, 1] * 50.0 - 7.0                                   # arbitrary, finite
    label = seedgen.seeded_label((2, 1) + SIZE, 104).to(DEV)
    res = []
    for cfg, P, xin in ((cfg1, P1, x[:, :1].contiguous()), (cfg2, P2, x)):
        model = build(cfg, params=P)
        predict, masks = model(xin.to(DEV))
        totals, _ = train.deep_supervision_loss(predict, masks, label, O_step.dynamic_weights(0))
        torch.autograd.backward(totals, [torch.ones_like(t) for t in totals])
        torch.cuda.synchronize()
        res.append((model, predict.detach(), [m.detach() for m in masks]))
    (m1, p1, k1), (m2, p2, k2) = res
    assert torch.equal(p1, p2)
    for a, b in zip(k1, k2):
        assert torch.equal(a, b)
    # The forward pass sums in a fixed order: outputs and masks are compared bit for bit above.  The weight-gradient kernels add
    # their split partial sums with fp32 atomics, whose order changes from launch to launch, so two runs of the SAME model already
    # differ in the last bits of a weight gradient (grads_agree's docstring): the gradients are held at that gate instead.
    g1, g2 = dict(m1.named_parameters()), dict(m2.named_parameters())
    for k, p in g1.items():
        if p.grad is None:
            assert g2[k].grad is None, k
        elif k == 'encode.input_block.weight':
            assert grads_agree(g2[k].grad[:, :4], p.grad, k), k
        else:
            assert grads_agree(g2[k].grad, p.grad, k), k
    # the second channel's weights are zero, their gradient is not: the channel did enter
    assert g2['encode.input_block.weight'].grad[:, 4:].abs().max().item() > 0


# ---- 4. one gather for all channels ---------------------------------------------------------------------------------------------

SCAN = (9, 10, 11)
FILLS = (-1.5, 0.25, 3.0)


def _gather_source():
    g = torch.Generator().manual_seed(5)
    img = torch.randn((3,) + SCAN, generator=g)
    lab = (torch.rand(SCAN, generator=g) * 4).to(torch.uint8)
    return img.to(DEV), lab.to(DEV)


def _gather_mats(size):
    """an integer crop + flip + rot90 (square patches only swap), a rotation about D (the depth-separable kernel on its own; with the
    others in one call the general kernel serves all three), an oblique rotation with zoom that reaches outside the scan"""
    k = 1 if size[0] == size[1] else 2
    return np.stack([data.patch_matrix((2, 1, 1), size, True, k),
                     data.patch_matrix((2, 2, 1), size, False, 0, (0.0, 0.0, 0.6)),
                     data.patch_matrix((3, 3, 2), size, False, 0, (0.4, -0.3, 0.8), 0.6, (1.0, 1.2, 2.0))])


@pytest.mark.parametrize('elastic', [False, True])
@pytest.mark.parametrize('size', [(4, 6, 8), (5, 6, 7)])
def test_sample_channels_matches_single_channel_calls(size, elastic):
    img, lab = _gather_source()
    mats = _gather_mats(size)
    sigma = np.array([[0.0, 0.0, 0.0], [0.5, 0.25, 1.0], [0.0, 0.0, 0.0]], dtype=np.float32)
    seeds = np.array([[data.channel_seed(1000 + k, c) for c in range(3)] for k in range(3)], dtype=np.uint64)
    lattice = None
    if elastic:
        lattice = np.random.RandomState(3).uniform(-1.5, 1.5, (3, 3, 4, 5, 4)).astype(np.float32)
    calls = [(mats, sigma, seeds, lattice)]
    if not elastic:
        calls += [(mats[k:k + 1], sigma[k:k + 1], seeds[k:k + 1], None) for k in range(3)]       # each matrix's own kernel variant
    for m, sg, sd, lat in calls:
        oi, ol = data.sample_affine(img, lab, m, size, FILLS, sg, sd, elastic=lat)
        assert oi.shape == (len(m), 3) + size and ol.shape == (len(m), 1) + size
        for c in range(3):
            ri, rl = data.sample_affine(img[c], lab, m, size, FILLS[c], sg[:, c], sd[:, c], elastic=lat)
            assert torch.equal(oi[:, c:c + 1].contiguous().view(torch.int32), ri.view(torch.int32)), (len(m), c)
            assert torch.equal(ol, rl), (len(m), c)
    # a [n] seed vector expands through channel_seed; the noise of patch 1 is noise_reference's
    oi2, _ = data.sample_affine(img, lab, mats, size, FILLS, sigma, [1000, 1001, 1002], elastic=lattice)
    oi, _ = data.sample_affine(img, lab, mats, size, FILLS, sigma, seeds, elastic=lattice)
    assert torch.equal(oi2, oi)
    clean, _ = data.sample_affine(img, lab, mats, size, FILLS, elastic=lattice)
    cnt = size[0] * size[1] * size[2]
    for c in range(3):
        z = (oi[1, c] - clean[1, c]).cpu().numpy().ravel().astype(np.float64) / float(sigma[1, c])
        assert np.abs(z - data.noise_reference(data.channel_seed(1001, c), cnt)).max() <= 1e-4, c
    assert torch.equal(oi[0], clean[0]) and torch.equal(oi[2], clean[2])


def test_sample_channels_splits_long_calls():
    """more patches than one launch of the channel kernels carries: the split does not show"""
    img, lab = _gather_source()
    size = (4, 6, 8)
    mats = np.concatenate([_gather_mats(size)] * 4)[:11]
    oi, ol = data.sample_affine(img[:2].contiguous(), lab, mats, size, FILLS[:2])
    for c in range(2):
        ri, rl = data.sample_affine(img[c], lab, mats, size, FILLS[c])
        assert torch.equal(oi[:, c:c + 1], ri) and torch.equal(ol, rl)


def test_sample_channels_refusals():
    img, lab = _gather_source()
    size = (4, 6, 8)
    mats = _gather_mats(size)
    with pytest.raises(ValueError, match='lattices for'):
        data.sample_affine(img, lab, mats, size, elastic=np.zeros((2, 3, 4, 5, 4), np.float32))
    with pytest.raises(ValueError):
        data.sample_affine(torch.zeros((5,) + SCAN, device=DEV), lab, mats, size)
    with pytest.raises(ValueError):
        data.sample_affine(img.permute(0, 1, 3, 2)[..., :10, :], lab[:, :10, :10].contiguous(), mats, size)
    f = _lib.load().ltu_sample_channels
    oi = torch.full((3, 3) + size, 7.0, device=DEV)
    ol = torch.full((3, 1) + size, 7, device=DEV, dtype=torch.uint8)
    m = np.ascontiguousarray(mats.reshape(3, 12))
    fl = np.array(FILLS + (0.0, 0.0), dtype=np.float32)

    def call(K=3, n=3, fill=fl.ctypes.data, phi=0, g=(0, 0, 0)):
        return f(img.data_ptr(), lab.data_ptr(), oi.data_ptr(), ol.data_ptr(), m.ctypes.data, phi, *g, 0, 0, fill, n, K, *SCAN, *size, None)

    phi = torch.zeros((3, 3, 4, 5, 4), device=DEV)
    assert call(K=5) == -2 and call(K=0) == -2 and call(fill=0) == -4 and call(n=_lib.SAMPLE_AFFINE_MAX + 1) == -4
    assert call(phi=phi.data_ptr(), g=(4, 5, 9)) == -2 and call(phi=phi.data_ptr() + 2, g=(4, 5, 4)) == -3
    bad = fl.copy()
    bad[1] = np.inf
    assert call(fill=bad.ctypes.data) == -4
    torch.cuda.synchronize()
    assert (oi == 7.0).all() and (ol == 7).all()


# ---- 5. scan to patch -----------------------------------------------------------------------------------------------------------

AFFINE = np.array([[-0.9, 0.0, 0.1, 12.0], [0.0, 1.1, 0.0, -7.0], [0.05, 0.0, 2.2, 3.0], [0.0, 0.0, 0.0, 1.0]])
PIXDIM = (1.0, 1.0, 2.0)
WINDOWS = [(-100.0, 200.0, 0.0, 1.0), 'zscore']


@pytest.fixture(scope='module')
def nifti_paths(tmp_path_factory):
    d = tmp_path_factory.mktemp('multiscan')
    X, Y, Z = 12, 10, 6
    rs = np.random.RandomState(8)
    a = (rs.randn(Z, Y, X) * 120 + 30).astype(np.float32)
    b = (rs.rand(Z, Y, X) * 4 + 1).astype(np.float32)
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing='ij')
    lab = (((xx - 6) / 4.0) ** 2 + ((yy - 5) / 3.5) ** 2 + ((zz - 3) / 2.5) ** 2 <= 1).astype(np.uint8)
    paths = {}
    for name, arr in (('a', a), ('b', b), ('lab', lab)):
        paths[name] = str(d / f'{name}.nii.gz')
        nifti.save(paths[name], arr, AFFINE)
    shifted = AFFINE.copy()
    shifted[0, 3] += 0.5
    paths['shifted'] = str(d / 'shifted.nii.gz')
    nifti.save(paths['shifted'], b, shifted)
    return paths


def test_multiscan_channels_are_spaced_scans(nifti_paths):
    p = nifti_paths
    ms = data.MultiScan([p['a'], p['b']], p['lab'], pixdim=PIXDIM, intensity=WINDOWS, device=DEV)
    assert ms.channels == 2 and ms.img.dim() == 4 and ms.img.is_contiguous() and ms.img.dtype == torch.float32
    singles = [data.SpacedScan(p[n], p['lab'], pixdim=PIXDIM, intensity=w, device=DEV) for n, w in zip('ab', WINDOWS)]
    assert tuple(ms.img.shape) == (2,) + tuple(ms.shape) and tuple(ms.shape) == tuple(singles[0].shape)
    for c, s in enumerate(singles):
        assert torch.equal(ms.img[c].view(torch.int32), s.img.view(torch.int32)), c
        assert ms.intensity[c] == s.intensity
    assert torch.equal(ms.lab, singles[0].lab)
    assert np.array_equal(ms.matrix, singles[0].matrix) and np.array_equal(ms.affine, singles[0].affine)
    assert ms.native_shape == singles[0].native_shape and ms.pixdim == singles[0].pixdim
    assert ms.crop_index.counts == singles[0].crop_index.counts and np.array_equal(ms.label_host, singles[0].label_host)
    # one spec serves all channels
    one = data.MultiScan([p['a'], p['b']], p['lab'], pixdim=PIXDIM, intensity=WINDOWS[0], device=DEV)
    assert one.intensity == [WINDOWS[0]] * 2 and torch.equal(one.img[0], ms.img[0])
    with pytest.raises(ValueError):
        data.MultiScan([p['a'], p['shifted']], p['lab'], pixdim=PIXDIM, device=DEV)
    with pytest.raises(ValueError):
        data.MultiScan([p['a']] * 5, p['lab'], pixdim=PIXDIM, device=DEV)
    with pytest.raises(ValueError):
        data.MultiScan([p['a'], p['b']], p['lab'], pixdim=PIXDIM, intensity=[None] * 3, device=DEV)


def _every(p):
    # blur_sigma: a radius int(4 sigma + 0.5) <= 3 stays below the patch depth of 4
    return data.Augmentation(rot_prob=p, zoom_prob=p, noise_prob=p, blur_prob=p, brightness_prob=p, gamma_prob=p, blur_sigma=(0.5, 0.8))


def test_multiscan_sampling(nifti_paths):
    p = nifti_paths
    size = (6, 6, 4)
    single = data.SpacedScan(p['a'], p['lab'], pixdim=PIXDIM, intensity=WINDOWS[0], device=DEV)
    one = data.MultiScan([p['a']], p['lab'], pixdim=PIXDIM, intensity=WINDOWS[0], device=DEV)
    for aug in (None, _every(1.0), _every(0.5)):
        ra, rb = np.random.RandomState(31), np.random.RandomState(31)
        si, sl = data.sample(single, size, ra, num_samples=5, augment=aug)
        mi, ml = data.sample(one, size, rb, num_samples=5, augment=aug)
        assert mi.shape == (5, 1) + size and torch.equal(mi, si) and torch.equal(ml, sl)
        assert ra.randint(1 << 30) == rb.randint(1 << 30)
    # K = 2: the host draws do not depend on K; channel c is the single-scan call except for its noise
    ms = data.MultiScan([p['a'], p['b']], p['lab'], pixdim=PIXDIM, intensity=WINDOWS, device=DEV)
    singles = [single, data.SpacedScan(p['b'], p['lab'], pixdim=PIXDIM, intensity=WINDOWS[1], device=DEV)]
    ra, rb = np.random.RandomState(32), np.random.RandomState(32)
    mi, ml = data.sample(ms, size, ra, num_samples=4)
    si, sl = data.sample(singles[1], size, rb, num_samples=4)
    assert mi.shape == (4, 2) + size and ml.shape == (4, 1) + size
    assert torch.equal(mi[:, 1:2], si) and torch.equal(ml, sl) and ra.randint(1 << 30) == rb.randint(1 << 30)
    geo = data.Augmentation(rot_prob=1.0, zoom_prob=1.0, noise_prob=0.0, blur_prob=1.0, brightness_prob=1.0, gamma_prob=1.0,
                            blur_sigma=(0.5, 0.8))
    mi, ml = data.sample(ms, size, np.random.RandomState(33), num_samples=3, augment=geo)
    for c, s in enumerate(singles):
        si, sl = data.sample(s, size, np.random.RandomState(33), num_samples=3, augment=geo)
        assert torch.equal(mi[:, c:c + 1], si) and torch.equal(ml, sl), c
    # noise alone on top of the geometry: every channel its own deviates, replayed by noise_reference with channel_seed
    noisy = data.Augmentation(rot_prob=1.0, zoom_prob=1.0, noise_prob=1.0, noise_std=(0.5, 1.0), blur_prob=0.0, brightness_prob=0.0,
                              gamma_prob=0.0)
    quiet = data.Augmentation(rot_prob=1.0, zoom_prob=1.0, noise_prob=0.0, noise_std=(0.5, 1.0), blur_prob=0.0, brightness_prob=0.0,
                              gamma_prob=0.0)
    ni, _ = data.sample(ms, size, np.random.RandomState(34), num_samples=2, augment=noisy)
    qi, _ = data.sample(ms, size, np.random.RandomState(34), num_samples=2, augment=quiet)
    _, params = data.sample_draws(ms, size, np.random.RandomState(34), 2, augment=noisy)
    cnt = size[0] * size[1] * size[2]
    for k, prm in enumerate(params):
        for c in range(2):
            z = (ni[k, c] - qi[k, c]).cpu().numpy().ravel().astype(np.float64) / prm['noise_std']
            assert np.abs(z - data.noise_reference(data.channel_seed(prm['seed'], c), cnt)).max() <= 1e-4, (k, c)
    assert not torch.equal(ni[:, 0] - qi[:, 0], ni[:, 1] - qi[:, 1])


# ---- 6. sliding window ----------------------------------------------------------------------------------------------------------

def test_sliding_window_over_channels():
    x = torch.randn(2, 3, 10, 9, 7, generator=torch.Generator().manual_seed(6)).to(DEV)
    roi = (6, 6, 4)
    seen = []

    def mix(w):
        seen.append(tuple(w.shape))
        return torch.stack((w[:, 0], w[:, 1] + 2 * w[:, 2]), 1)

    for kw in (dict(), dict(mode='gaussian', mirror_axes=(0, 1))):
        seen.clear()
        out = infer.sliding_window_inference(x, roi, 3, mix, overlap=0.5, **kw)
        assert out.shape == (2, 2, 10, 9, 7)
        assert all(s[1:] == (3,) + roi and s[0] <= 3 for s in seen)
        first = infer.sliding_window_inference(x[:, :1].contiguous(), roi, 3, lambda w: w, overlap=0.5, **kw)
        second = infer.sliding_window_inference((x[:, 1:2] + 2 * x[:, 2:3]).contiguous(), roi, 3, lambda w: w, overlap=0.5, **kw)
        assert torch.equal(out[:, :1], first) and torch.equal(out[:, 1:], second), kw
        other = infer.sliding_window_inference(x, roi, 5, mix, overlap=0.5, **kw)
        assert torch.equal(out, other), kw
    with pytest.raises(_lib.LtuError):
        infer.sliding_window_inference(torch.zeros(1, 5, 10, 9, 7, device=DEV), roi, 3, mix)


# ---- 7. captured paths ----------------------------------------------------------------------------------------------------------

def test_graphed_step_matches_eager_k3():
    x, label = (t.to(DEV) for t in inputs3())
    w = O_step.dynamic_weights(0)
    ref = build(CFG3)
    train.train_step(ref, x, label, w)
    m = build(CFG3)
    red = train.GradReducer(m, bucket_mb=0.5, unused=train.UNUSED_PARAMETERS)
    g = train.GraphedStep(m, x, label, w, red)
    assert g.x.shape == x.shape
    for _ in range(2):
        g(x, label)
    torch.cuda.synchronize()
    pr, pm = dict(ref.named_parameters()), dict(m.named_parameters())
    for k, p in pr.items():
        if p.grad is None:
            continue
        assert grads_agree(pm[k].grad, p.grad, k), k


def test_infer_volume_graph_matches_eager_k3():
    model = build(CFG3)
    x = seedgen.seeded_volume((1, 3, 32, 32, 16), 105).to(DEV)
    eager = infer.infer_volume(model, x, depth_size=16, roi_xy=32, graph=False)
    graphed = infer.infer_volume(model, x, depth_size=16, roi_xy=32, graph=True)
    assert eager.shape == (1, 2, 32, 32, 16)
    assert torch.equal(eager, graphed)
