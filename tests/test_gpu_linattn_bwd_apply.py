"""linattn_bwd_apply, bf16 storage, at the shapes where its tile loop can go wrong: a single partial tile, a one-token last tile,
ragged last tiles in several samples, and long runs of tiles per workgroup (the steady state of the prefetch and of the in-place
staging).  Driven through the C-ABI (ltu_linattn_fwd, then ltu_linattn_bwd) and checked stage by stage with the float64 references
and gates of tests/test_gpu_token_paths.py.  dqkv carries 64 guard rows behind B*N: no row past the last token may be written, and
every real row must be.
"""
import pytest
import torch

from tests.test_gpu_conv_paths import knobs
from tests.test_gpu_token_paths import (DEV, Checker, _bf, _call, _dev, _gen, _nan, _ptr, _stream, check_apply, check_ctx,
                                        check_linattn_bwd)

GUARD = 64
SENTINEL = 12352.0           # 193 * 64: exact in bf16, so the filled guard rows read back as this value

# (name, B, N, knobs)
SHAPES = [
    ('one_partial_tile', 1, 31, {}),
    ('one_token_last_tile', 2, 33, {}),
    # by default the two tiles of a sample go to two workgroups; one workgroup per sample runs the full tile and then the one-token tile
    ('one_token_last_tile_one_run', 2, 33, {'LTU_LA_TOKB_BLOCKS': 1}),
    ('ragged_three_samples', 3, 101, {}),
    ('long_runs', 2, 1000, {'LTU_LA_TOKB_BLOCKS': 4}),
]


def _inputs(name, B, N, d):
    g = _gen(sum(map(ord, name)) + d)
    qkv = _bf(torch.randn(B * N, 3 * d, generator=g) * 1.5)
    dout = _bf(torch.randn(B * N, d, generator=g))
    return qkv, dout


def _run(qkv_in, dout, B, N, d):
    """forward then backward into fresh buffers; returns the stored outputs of every stage and dqkv with its guard rows"""
    from lintransunet_amd import ops
    M, H = B * N, d // 32
    qkv, gout = _dev(qkv_in), _dev(dout)
    out = _nan((M, d))
    dqkv = _nan((M + GUARD, 3 * d))
    dqkv[M:] = SENTINEL
    cx, dctx = (_nan((B * H, 32, 32), torch.float32) for _ in range(2))
    colstats, qstat = _nan((B * H, 64), torch.float32), _nan((M, H, 2), torch.float32)
    n = ops._lib.load().ltu_linattn_ws_floats(B, N, d)
    ws = torch.empty(n, device=DEV, dtype=torch.float32)
    _call('ltu_linattn_fwd', _ptr(qkv), _ptr(out), _ptr(cx), _ptr(colstats), _ptr(qstat), _ptr(ws), n, B, N, d, ops.BF16, _stream())
    _call('ltu_linattn_bwd', _ptr(qkv), _ptr(gout), _ptr(cx), _ptr(colstats), _ptr(qstat), _ptr(dqkv), _ptr(dctx), 0, _ptr(ws), n,
          B, N, d, ops.BF16, _stream())
    torch.cuda.synchronize()
    return out, cx, colstats, qstat, dctx, dqkv


@pytest.fixture(scope='module')
def gpu():
    assert torch.cuda.is_available()
    from lintransunet_amd import ops  # noqa: F401
    return True


@pytest.mark.gpu
@pytest.mark.parametrize('d', [128, 256])
@pytest.mark.parametrize('name,B,N,kn', SHAPES, ids=[s[0] for s in SHAPES])
def test_bwd_apply(gpu, name, B, N, kn, d):
    M = B * N
    qkv_in, dout = _inputs(name, B, N, d)
    with knobs(kn):
        out, cx, colstats, qstat, dctx, dqkv = _run(qkv_in, dout, B, N, d)
    real, guard = dqkv[:M].float(), dqkv[M:].float()
    assert torch.isfinite(real).all(), f'{int((~torch.isfinite(real)).any(1).sum())} of {M} rows of dqkv hold non-finite values'
    assert (guard == SENTINEL).all(), 'rows of dqkv behind B*N were written'
    ck = Checker()
    check_ctx(ck, qkv_in, B, N, d, cx, colstats)
    check_apply(ck, qkv_in, B, N, d, cx, out, qstat)
    check_linattn_bwd(ck, qkv_in, dout, B, N, d, cx, colstats, qstat, dctx, dqkv[:M])
    print(f'[linattn_bwd_apply {name} d={d}] worst error / bound {max(ck.ratio.items(), key=lambda kv: kv[1])}')
    assert not ck.fails, f'{name} d={d}: ' + '; '.join(ck.fails)


@pytest.mark.gpu
@pytest.mark.parametrize('d', [128, 256])
def test_bwd_apply_repeatable(gpu, d):
    """the long-runs shape twice into fresh buffers: bit-equal dqkv (nothing may depend on what an earlier launch left in LDS)"""
    name, B, N, kn = SHAPES[-1]
    qkv_in, dout = _inputs(name, B, N, d)
    with knobs(kn):
        first = _run(qkv_in, dout, B, N, d)[-1]
        second = _run(qkv_in, dout, B, N, d)[-1]
    assert torch.equal(first.view(torch.int16), second.view(torch.int16))
