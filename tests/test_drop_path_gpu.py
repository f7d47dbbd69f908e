"""The drop_path kernel (csrc/kernels/droppath_kernels.hip) bit for bit against the CPU path -- one fp32
product and one rounding leave no freedom -- with sentinel guards around the buffer: the vector path, the
scalar path by n and by alignment, one sample, several blocks per sample, a sample longer than a pass of
the capped grid; the forward's mask again in backward, another one after the counter advanced, a null
counter, NaN in a dropped sample; and the layer behind a `split` in a net."""
import numpy as np
import pytest
import torch

from test_drop_path_cpu import _bits, _np_drop_path, _np_keep
from cxxnet_amd import native
from cxxnet_amd.ops import layer_ops as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 24
FILL = 3.0
PASS = 2048 * 256 * 8  # elements of one sample that a pass covers: asserted in test_the_long_sample_case
SEED, PKEEP = 12345, 0.5
SHAPES = [(8, 8), (8, 7), (3, 9), (1, 4099), (5, 2048), (2, PASS + 8 * 256)]


def _ctr(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV) if v is not None else None


def _input(B, n):
    g = torch.Generator().manual_seed(B * 131 + n % 977)
    return (4.0 * torch.randn(B, n, generator=g)).to(torch.bfloat16)


def _run(x_cpu, off, seed, counter, pkeep):
    """x_cpu [B][n] placed `off` elements past a 16-byte boundary; the result on the CPU, guards checked"""
    B, n = x_cpu.shape
    whole = torch.full((off + B * n + GUARD,), FILL, dtype=torch.bfloat16, device=DEV)
    assert whole.data_ptr() % 16 == 0
    view = whole[off:off + B * n].view(B, n)
    view.copy_(x_cpu)
    L.drop_path_apply(view, seed, pkeep, _ctr(counter))
    torch.cuda.synchronize()
    assert (whole[:off] == FILL).all() and (whole[off + B * n:] == FILL).all(), "wrote outside the tensor"
    return view.cpu()


def test_the_long_sample_case():
    assert L.drop_path_pass_elems() == PASS == native.kernels().cxn_drop_path_pass_elems()
    assert SHAPES[-1][1] > PASS and all(n < PASS for _, n in SHAPES[:-1])


@pytest.mark.parametrize("off", [0, 4])   # 16-byte aligned, and 8 bytes past it (the scalar path whatever n)
@pytest.mark.parametrize("B,n", SHAPES)
def test_bit_equal_to_the_cpu_path(B, n, off):
    x = _input(B, n)
    for counter in (3, 5):
        keep = _np_keep(B, SEED, counter, PKEEP)
        if B > 1:
            assert keep.any() and not keep.all(), "the case needs kept and dropped samples"
        want = x.clone()
        L.drop_path_apply(want, SEED, PKEEP, torch.tensor([counter], dtype=torch.int32))
        got = _run(x, off, SEED, counter, PKEEP)
        assert torch.equal(_bits(got), _bits(want)), (B, n, off, counter)
        for b in range(B):  # whole samples, by the mirror's decision
            assert bool((_bits(got)[b] == 0).all()) == (not keep[b])
    if B == 1:  # both outcomes of the one sample
        assert {bool(_np_keep(1, SEED, c, PKEEP)[0]) for c in (3, 5)} == {True, False}
    if n < 10000:  # and against the independent numpy evaluation
        assert torch.equal(_bits(got), _bits(_np_drop_path(x, SEED, 5, PKEEP)[0]))


def test_other_keep_probabilities_round_as_the_cpu_path_does():
    x = _input(64, 24)
    for pkeep in (0.95, 0.8, 0.9125, 1.0):
        want = x.clone()
        L.drop_path_apply(want, 77, pkeep, torch.tensor([1], dtype=torch.int32))
        assert torch.equal(_bits(_run(x, 0, 77, 1, pkeep)), _bits(want)), pkeep
    assert torch.equal(_bits(_run(x, 0, 77, 1, 1.0)), _bits(x))  # pkeep = 1 keeps every sample's bits


def test_the_mask_returns_in_backward_changes_with_the_counter_and_without_one():
    B, n = 16, 40
    x, g = _input(B, n), _input(B + 1, n)[1:]
    y1, y2 = _run(x, 0, SEED, 3, PKEEP), _run(x, 0, SEED, 3, PKEEP)
    assert torch.equal(_bits(y1), _bits(y2))                     # the same call twice: the same bits
    dg = _run(g, 0, SEED, 3, PKEEP)                               # the gradient, with the same counter value
    dropped = lambda t: (_bits(t) == 0).all(1).numpy()            # noqa: E731
    k3 = _np_keep(B, SEED, 3, PKEEP)
    assert np.array_equal(dropped(y1), ~k3) and np.array_equal(dropped(dg), ~k3)
    k4 = _np_keep(B, SEED, 4, PKEEP)
    assert not np.array_equal(k3, k4)
    assert np.array_equal(dropped(_run(x, 0, SEED, 4, PKEEP)), ~k4)   # the counter advanced: another mask
    k0 = _np_keep(B, SEED, None, PKEEP)                           # a null counter: the seed itself
    y0 = _run(x, 0, SEED, None, PKEEP)
    assert np.array_equal(dropped(y0), ~k0)
    assert torch.equal(_bits(y0), _bits(_np_drop_path(x, SEED, None, PKEEP)[0]))


def test_a_dropped_sample_full_of_nan_comes_back_plus_zero():
    B, n = 8, 20
    keep = _np_keep(B, SEED, 2, PKEEP)
    x = torch.full((B, n), float("nan"), dtype=torch.bfloat16)
    x[:, 1], x[:, 2] = float("-inf"), -0.0
    for off in (0, 4):
        got = _run(x, off, SEED, 2, PKEEP)
        for b in range(B):
            if keep[b]:
                assert torch.isnan(got[b, 0]) and got[b, 1] == float("-inf") and _bits(got)[b, 2] == -32768
            else:
                assert (_bits(got)[b] == 0).all()


def test_the_launcher_rejects_bad_arguments():
    k = native.kernels()
    x = torch.full((4, 16), FILL, dtype=torch.bfloat16, device=DEV)
    p = x.data_ptr()
    assert k.cxn_drop_path(None, 4, 16, 1, None, 0.5, None) != 0
    assert k.cxn_drop_path(p, 0, 16, 1, None, 0.5, None) != 0
    assert k.cxn_drop_path(p, 4, 0, 1, None, 0.5, None) != 0
    assert k.cxn_drop_path(p, -4, 16, 1, None, 0.5, None) != 0
    assert k.cxn_drop_path(p, 4, 16, 1, None, 0.0, None) != 0
    assert k.cxn_drop_path(p, 4, 16, 1, None, 1.5, None) != 0
    assert k.cxn_drop_path(p, 4, 16, 1, None, float("nan"), None) != 0
    with pytest.raises(ValueError, match="bf16"):
        L.drop_path_apply(x.float(), 1, 0.5)
    torch.cuda.synchronize()
    assert (x == FILL).all()
    assert k.cxn_drop_path(p, 4, 16, 1, None, 0.25, None) == 0  # the same call with good arguments does write
    torch.cuda.synchronize()
    assert ((x == 0).all(1) | (x == 4 * FILL).all(1)).all() and (x != FILL).all()


NET = """netconfig=start
layer[0->c] = conv:c
  kernel_size = 3
  pad = 1
  nchannel = 8
  no_bias = 1
layer[c->s1,s2] = split
layer[s1->s1] = drop_path:dp
  drop_prob = 0.5
layer[s1,s2->a] = add:join
  add_relu = 0
layer[a->f] = flatten
layer[f->fc] = fullc:fc
  nhidden = 4
layer[fc->fc] = softmax
netconfig=end
input_shape = 4,5,5
random_type = xavier
eta = 0.05
"""


def test_the_split_sibling_is_untouched():
    """drop_path writes its node: a split output with the self-loop keeps a buffer of its own, so the
    sibling output and the split's input still hold the conv's result after the forward pass"""
    from cxxnet_amd.io.data import DataBatch
    from cxxnet_amd.nnet import NetTrainer
    B = 16
    tr = NetTrainer()
    for kv in list(native.rt().parse_config(NET)) + [("batch_size", str(B)), ("dev", "gpu"), ("eval_train", "0"),
                                                     ("silent", "1"), ("seed", "3"), ("cuda_graph", "0"),
                                                     ("launch_replay", "0")]:
        tr.set_param(*kv)
    tr.init_model()
    net = tr.net
    node = {name: net.nodes[i] for i, name in enumerate(tr.net_cfg.node_names)}
    split = next(c.layer for c in net.connections if c.type == 23)
    dp = next(c.layer for c in net.connections if c.type == 48)
    assert not split.alias
    ptrs = {node[k].data.data_ptr() for k in ("c", "s1", "s2")}
    assert len(ptrs) == 3
    g = torch.Generator().manual_seed(0)
    tr._set_batch(DataBatch(torch.randn(B, 4, 5, 5, generator=g), torch.zeros(B, 1)))
    net.forward(True)
    torch.cuda.synchronize()
    counter = int(net.ctx.step_counter.item())  # (the forward pass advanced it before its first layer)
    keep = _np_keep(B, dp.seed, counter, 0.5)
    assert keep.any() and not keep.all()
    c, s1, s2 = node["c"].data, node["s1"].data, node["s2"].data
    assert torch.equal(_bits(s2.cpu()), _bits(c.cpu())) and bool((c != 0).any(-1).any(-1).any(-1).all())
    want = c.cpu().clone()
    L.drop_path_apply(want, dp.seed, 0.5, torch.tensor([counter], dtype=torch.int32))
    assert torch.equal(_bits(s1.cpu()), _bits(want))
    kept = torch.from_numpy(keep)
    assert (s1.cpu()[~kept] == 0).all() and torch.equal(s1.cpu()[kept].float(), 2.0 * c.cpu()[kept].float())
