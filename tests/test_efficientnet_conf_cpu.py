"""models/confs/efficientnet_b0.conf on the CPU executor: the net is table 1 of Tan & Le 2019 with the
site counts the layers were added for, and one training step runs.  CPU only."""
import numpy as np
import pytest
import torch

# expansion, kernel, stride, channels, blocks: table 1 of the paper
STAGES = [(1, 3, 1, 16, 1), (6, 3, 2, 24, 2), (6, 5, 2, 40, 2), (6, 3, 2, 80, 3), (6, 5, 1, 112, 3), (6, 5, 2, 192, 4),
          (6, 3, 1, 320, 1)]


def _blocks():
    """(input width, expansion width, kernel, stride, output width) of the 16 blocks"""
    cin, out = 32, []
    for exp, k, s, c, n in STAGES:
        for j in range(n):
            out.append((cin, cin * exp, k, s if j == 0 else 1, c))
            cin = c
    return out


@pytest.fixture(scope="module")
def effnet():
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in load_conf("efficientnet_b0", [("batch_size", "2"), ("dev", "cpu"), ("eval_train", "0"), ("silent", "1"),
                                              ("seed", "1")]):
        tr.set_param(k, v)
    tr.init_model()
    return tr


def test_efficientnet_b0_conf_builds(effnet):
    net = effnet.net
    assert net.nodes[-1].shape == (2, 1, 1, 1000)
    conns = net.connections
    types = [c.type for c in conns]
    blocks = _blocks()
    assert len(blocks) == 16
    # the site counts: silu = the stem, 15 expansions, 16 depthwise, 16 squeezes, the head
    assert types.count(47) == 1 + 15 + 16 + 16 + 1 == 49
    assert types.count(48) == 9 == types.count(41) and types.count(42) == 16 == types.count(4)
    assert types.count(43) == types.count(44) == types.count(45) == types.count(3) == 0
    dw = [c for c in conns if c.type == 10 and c.layer.lp.num_group > 1]
    assert [(c.layer.lp.kernel_height, c.layer.lp.num_channel, c.layer.lp.stride) for c in dw] == \
        [(k, e, s) for _, e, k, s, _ in blocks]
    assert all(c.layer.lp.num_group == c.layer.lp.num_channel == c.nodes_in[0].shape[1] for c in dw)
    assert all(c.layer.lp.pad_y == c.layer.lp.kernel_height // 2 for c in dw)
    # the stem, 15 expansions (the first block has none), 16 depthwise, 16 projections, the 1280 conv
    assert types.count(10) == 1 + 15 + 16 + 16 + 1 == types.count(40)
    assert all(c.layer.lp.no_bias == 1 for c in conns if c.type == 10)
    # the joins: stride 1 and Cin = Cout, no relu, each behind a drop_path on the branch with drop_prob = 0.2 i / 16
    res = [i for i, (ci, _, _, s, co) in enumerate(blocks) if s == 1 and ci == co]
    assert len(res) == 9
    joins = [c for c in conns if c.type == 41]
    assert not any(c.layer.relu for c in joins)
    drops = [(k, c) for k, c in enumerate(conns) if c.type == 48]
    assert [round(c.layer.drop_prob, 6) for _, c in drops] == [round(0.2 * i / 16, 6) for i in res]
    for (k, c), j in zip(drops, joins):
        assert conns[k + 1] is j and j.nodes_in[0] is c.nodes_in[0] and conns[k - 1].type == 40
    # the squeeze widths: a quarter of the block's INPUT width, rounded up to a multiple of 8
    widths = [c.layer.lp.num_hidden for c in conns if c.type == 1]
    assert widths[:-1:2] == [(-(-ci // 4) + 7) // 8 * 8 for ci, _, _, _, _ in blocks]
    assert widths[:-1:2] == [8, 8, 8, 8, 16, 16, 24, 24, 24, 32, 32, 32, 48, 48, 48, 48]
    assert widths[1:-1:2] == [e for _, e, _, _, _ in blocks] and widths[-1] == 1000
    assert [c.nodes_in[1].shape[1:] for c in conns if c.type == 42] == [(1, 1, e) for _, e, _, _, _ in blocks]
    assert types.count(23) == 9 + 16 and types.count(8) == 1 and types.count(2) == 1
    assert types.count(13) == 17  # the sixteen squeezes and the classifier's pooling
    for c in conns:  # every pooling is global and unpadded
        if c.type == 13:
            assert c.nodes_out[0].shape[2:] == (1, 1) and c.layer.lp.kernel_height == c.nodes_in[0].shape[2]
    (drop,) = [c for c in conns if c.type == 8]
    assert drop.layer.threshold == 0.2
    # the blocks end at the table's widths and resolutions, the head at 1280 x 7 x 7
    outs = [net.nodes[effnet.net_cfg.node_name_map["b%d" % i]].shape[1:] for i in range(1, 17)]
    hw, want = 112, []
    for _, _, _, s, co in blocks:
        hw //= s
        want.append((co, hw, hw))
    assert outs == want
    assert net.nodes[effnet.net_cfg.node_name_map["r17"]].shape[1:] == (1280, 7, 7)
    nparam = sum(s.numel for _, s in net.arena.specs)
    assert 5.2e6 < nparam < 5.4e6  # the paper's 5.3 M (5,288,548 in the usual implementations, whose squeezes are not rounded)


def test_efficientnet_b0_one_training_step(effnet):
    from cxxnet_amd.io.data import DataBatch
    g = torch.Generator().manual_seed(1)
    b = DataBatch(torch.randn(2, 3, 224, 224, generator=g), torch.randint(0, 1000, (2, 1), generator=g).float())
    before = effnet.net.arena.w.clone()
    effnet.update(b)
    after = effnet.net.arena.w
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    out = effnet.forward_to([len(effnet.net.nodes) - 1], b)[0].reshape(2, -1)
    assert out.shape == (2, 1000) and np.isfinite(out).all() and np.allclose(out.sum(1), 1.0, atol=1e-5)
