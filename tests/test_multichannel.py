"""CPU tests of the multi-channel input path (dim_input = 1 .. 4): the model's parameter surface, the per-channel noise seeds and
the expansion of window descriptors into one gather item per channel."""
import pytest

from oracle import net as O_net

SMALL = dict(num_layers=[8, 8, 8, 16, 32], roi_size_list=[20, 12, 9, 10, 6])


@pytest.mark.parametrize('K', [1, 2, 3, 4])
def test_state_dict_follows_dim_input(K):
    from lintransunet_amd.model import get_model_dict
    cfg = O_net.NetConfig(dim_input=K, **SMALL)
    model = get_model_dict('MaskTransUnet')(cfg.num_layers, cfg.roi_size_list, cfg.is_roi_list, K, cfg.dim_output, dropout=0.0)
    want = O_net.param_shapes(cfg)
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert got == want
    assert list(got) == list(want)
    assert got['encode.input_block.weight'] == (8, 4 * K, 3, 3, 3)
    assert model.dim_input == K


@pytest.mark.parametrize('K', [0, 5, -1])
def test_dim_input_outside_1_to_4_is_refused(K):
    from lintransunet_amd.model import get_model_dict
    cfg = O_net.NetConfig(**SMALL)
    with pytest.raises(ValueError):
        get_model_dict('MaskTransUnet')(cfg.num_layers, cfg.roi_size_list, cfg.is_roi_list, K, cfg.dim_output)


def test_embed_channels():
    from lintransunet_amd import ops
    assert [ops.embed_channels(K) for K in (1, 2, 3, 4)] == [8, 8, 16, 16]


def test_channel_seed():
    from lintransunet_amd import data
    for seed in (0, 1, 0x1234567890ABCDEF, (1 << 62) - 1):
        assert data.channel_seed(seed, 0) == seed
        seeds = [data.channel_seed(seed, c) for c in range(4)]
        assert len(set(seeds)) == 4
        assert all(0 <= s < 1 << 64 for s in seeds)
        for c in (1, 2, 3):
            assert seeds[c] == seed ^ ((c * 0x9E3779B97F4A7C15) % (1 << 64))


@pytest.mark.parametrize('mirror_axes', [(), (0, 1)])
def test_channel_items(mirror_axes):
    from lintransunet_amd import infer
    B, K = 2, 3
    starts = infer.patch_starts((10, 9, 7), (6, 6, 4), infer.scan_interval((10, 9, 7), (6, 6, 4), 0.5))
    items = infer.window_items(B, starts, mirror_axes)
    assert len(items) == B * len(starts) * (1 << len(mirror_axes))
    out = infer.channel_items(items, K)
    assert len(out) == K * len(items)
    for i, it in enumerate(items):
        for c in range(K):
            assert tuple(out[i * K + c]) == (it[0] * K + c, *it[1:])
    assert max(o[0] for o in out) == B * K - 1
    assert infer.channel_items(items, 1) == list(items)
    # the plain path's four-column descriptors expand the same way
    plain = [(b, *s) for b in range(B) for s in starts]
    assert infer.channel_items(plain, K)[K + 1] == (plain[1][0] * K + 1, *plain[1][1:])
