"""batch_norm_ma in a net on the GPU: against the CPU executor, row-independent inference (and
batch_norm's dependence, for contrast), checkpoint round trip, HIP-graph replay, launch hygiene."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# The conv and the first fullc feed a batch norm, which removes any per-channel constant: their
# biases would get a mathematically zero gradient (rounding noise only), so they have none.
NET = """
netconfig=start
layer[0->1] = conv:c1
  kernel_size = 3
  nchannel = 16
  pad = 1
  no_bias = 1
layer[1->2] = %(bn)s:bn1
layer[2->3] = relu
layer[3->4] = max_pooling
  kernel_size = 2
  stride = 2
layer[4->5] = flatten
layer[5->6] = fullc:f1
  nhidden = 32
  no_bias = 1
layer[6->6] = %(bn)s:bn2
layer[6->7] = relu
layer[7->8] = fullc:f2
  nhidden = 10
layer[8->8] = softmax
netconfig=end
input_shape = 8,12,12
random_type = xavier
eta = 0.05
momentum = 0.9
wd = 0.0005
bn_momentum = 0.75
"""
BATCH = 8


def relerr(a, b):  # tests/test_layer_kernels_gpu.py
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()


def _trainer(dev="gpu", bn="batch_norm_ma", extra=()):
    from cxxnet_amd import native
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in list(native.rt().parse_config(NET % {"bn": bn})) + [
            ("batch_size", str(BATCH)), ("dev", dev), ("eval_train", "0"), ("silent", "1"), ("seed", "3"),
            ("cuda_graph", "0"), ("launch_replay", "0")] + list(extra):
        tr.set_param(k, v)
    return tr


def _make(*args, **kw):
    tr = _trainer(*args, **kw)
    tr.init_model()
    return tr


def _batch(seed, n=BATCH):
    from cxxnet_amd.io.data import DataBatch
    g = torch.Generator().manual_seed(seed)
    return DataBatch(torch.randn(n, 8, 12, 12, generator=g), torch.randint(0, 10, (n, 1), generator=g).float())


def _params(tr):
    return [tr.net.arena.w[s.offset:s.offset + s.numel].detach().cpu().clone() for _, s in tr.net.arena.specs]


def _raw(tr, batch):
    return tr.forward_to([len(tr.net.nodes) - 1], batch)[0].copy()


def _round(t):
    t.copy_(t.to(torch.bfloat16).float())


def _bf16_at_node_boundaries(tr):
    """Make a dev = cpu trainer keep its activations and gradients the way the GPU executor does:
    every node a layer writes (forward: its outputs, backward: its inputs' gradients, and the input
    batch) is rounded to bf16, and the layers' compute copy of the weights is the bf16 rounding of
    the fp32 masters; inside a layer the CPU executor's fp32 formulas run unchanged."""
    for conn in tr.net.connections:
        lay = conn.layer
        f0, b0 = lay.forward, lay.backprop

        def fwd(is_train, nin, nout, f0=f0):
            f0(is_train, nin, nout)
            for n in nout:
                _round(n.data)

        def bwd(prop_grad, nin, nout, b0=b0):
            b0(prop_grad, nin, nout)
            if prop_grad:
                for n in nin:
                    _round(n.gdst)
        lay.forward, lay.backprop = fwd, bwd
    s0, f0 = tr.net.set_input, tr.net.forward

    def set_input(data, extra=()):
        s0(data, extra)
        _round(tr.net.nodes[0].data)

    def forward(is_train, pre_hook=None):
        # the GEMM operands: the bf16 shadow of the fp32 masters, as the arena keeps on the GPU
        for _, spec in tr.net.arena.specs:
            spec.wb = spec.w.to(torch.bfloat16).float()
        f0(is_train, pre_hook=pre_hook)
    tr.net.set_input, tr.net.forward = set_input, forward


STAT_CUTS = {"bn1 mean": (0, 16), "bn1 var": (16, 32), "bn2 mean": (32, 64), "bn2 var": (64, 96)}


def _three_steps(tr):
    first = None
    for seed in (1, 2, 3):
        tr.update(_batch(seed))
        if first is None:
            first = tr.net.bn_state.cpu().clone()
    return first


def test_gpu_matches_the_cpu_executor():
    """Three training steps from one seed on the GPU (bf16 HIP kernels) and on the CPU executor:
    every parameter tensor and every running statistic agrees within relerr 2e-2, each on its own
    scale.

    The oracle is the dev = cpu executor holding its numbers in the GPU executor's storage
    formats (_bf16_at_node_boundaries: bf16 nodes, bf16 compute copy of the weights); the formulas
    inside each layer are its fp32 torch ones.  Against the executor with fp32 storage this net
    cannot meet 2e-2 per tensor, and the kernels are not the reason: with 8 rows and a relu behind
    each batch norm, a bn output that bf16 storage moves across 0 flips a relu mask, which changes
    a whole row of f1's weight gradient and, through f1's data gradient, every gradient below it.
    The CPU executor shows it alone: in bf16 storage its own three-step result moves by relerr
    0.197 (bn2 bias), 0.175 (f1 weights), 0.162 (bn1 bias), 0.042 (conv1 weights) against its
    fp32-storage run -- to the fourth digit the figures of the GPU against that run, measured on
    an MI355X and printed below; against the bf16-storage executor the GPU's tensors all agree
    within 1e-5.  The fp32-storage executor is still held to what does not pass
    through a relu mask: the running statistics after the first step, per layer and statistic."""
    gpu, ora, cpu = _make("gpu"), _make("cpu"), _make("cpu")
    _bf16_at_node_boundaries(ora)
    for a, b in zip(_params(gpu), _params(cpu)):
        assert relerr(a, b) < 1e-5  # the same seed starts all three alike
    fg, fo, fc = _three_steps(gpu), _three_steps(ora), _three_steps(cpu)
    pg, po, pc = _params(gpu), _params(ora), _params(cpu)
    assert len(pg) == len(po) == 8
    keys = [(li, s.tag) for li, s in cpu.net.arena.specs]
    errs = {k: round(relerr(a, b), 5) for k, a, b in zip(keys, pg, po)}
    plain = {k: round(relerr(a, b), 5) for k, a, b in zip(keys, pg, pc)}
    sg, so = gpu.net.bn_state.cpu(), ora.net.bn_state
    assert sg.numel() == so.numel() == 2 * 16 + 2 * 32
    serrs = {k: round(relerr(sg[lo:hi], so[lo:hi]), 5) for k, (lo, hi) in STAT_CUTS.items()}
    first = {k: round(relerr(fg[lo:hi], fc[lo:hi]), 5) for k, (lo, hi) in STAT_CUTS.items()}
    print("per tensor vs bf16-node executor", errs, "running statistics", serrs)
    print("per tensor vs fp32-node executor", plain, "running statistics after step 1", first)
    assert max(errs.values()) < 2e-2, errs
    assert max(serrs.values()) < 2e-2, serrs
    assert max(first.values()) < 2e-2, first
    assert not torch.equal(so[:16], torch.zeros(16))


def _row0_outputs(tr, batch):
    return tr.forward_to([len(tr.net.nodes) - 1], batch)[0][0].copy(), tr.predict(batch)[0], \
        tr.extract_feature(batch, "top[-1]")[0].copy()


def _train_a_little(tr):
    for seed in (1, 2):
        tr.update(_batch(seed))


def test_inference_is_row_independent_on_the_gpu():
    tr = _make()
    _train_a_little(tr)
    a, b = _batch(5), _batch(6)
    b.data[0] = a.data[0]
    ra, rb = _row0_outputs(tr, a), _row0_outputs(tr, b)
    for u, v in zip(ra, rb):
        assert np.array_equal(u, v)
    assert not np.array_equal(_raw(tr, a)[1], _raw(tr, b)[1])
    # the same image alone, through adjust_batch_size
    from cxxnet_amd.io.data import DataBatch
    one = DataBatch(a.data[:1].clone(), a.label[:1].clone())
    r1 = _row0_outputs(tr, one)
    assert tr.net.cur_batch == 1
    for u, v in zip(ra, r1):
        assert np.array_equal(u, v)


def test_batch_norm_depends_on_the_batch():
    """The reference layer normalises with the batch statistics at test time too: the same image
    gives another output among other neighbours.  Not a defect of that layer; the difference
    batch_norm_ma exists for."""
    tr = _make(bn="batch_norm")
    _train_a_little(tr)
    a, b = _batch(5), _batch(6)
    b.data[0] = a.data[0]
    assert not np.array_equal(_raw(tr, a)[0], _raw(tr, b)[0])


def test_save_load_continue_on_the_gpu():
    tr = _make()
    _train_a_little(tr)
    data = tr.save_model()
    probe = _batch(9)
    want = _raw(tr, probe)
    tr2 = _trainer(extra=[("seed", "99")])
    tr2.load_model(data)
    assert torch.equal(tr2.net.bn_state, tr.net.bn_state)
    assert np.array_equal(_raw(tr2, probe), want)
    # training continues from the loaded statistics
    before = tr2.net.bn_state.clone()
    tr2.update(_batch(3))
    assert not torch.equal(tr2.net.bn_state, before)
    assert tr2.epoch_counter == tr.epoch_counter + 1


def test_graph_replay_applies_the_running_update_every_step():
    res = []
    for graph in (0, 1):
        tr = _make(extra=[("cuda_graph", str(graph)), ("deterministic", "1")])
        states = []
        for seed in (1, 2, 3, 4):  # eager, capture + replay, replay, replay
            tr.update(_batch(seed))
            states.append(tr.net.bn_state.clone())
        torch.cuda.synchronize()
        if graph:
            assert tr._graphs, "the step was not captured"
        res.append((_params(tr), [s.cpu() for s in states]))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a, b)
    assert not torch.equal(res[1][1][2], res[1][1][3])


def test_forward_backward_launch_only_library_kernels():
    from torch.profiler import ProfilerActivity, profile
    tr = _make()
    b = _batch(1)
    for _ in range(2):  # tile tuning and lazy buffers happen in the first steps
        tr.update(b)
    tr._set_batch(b)
    net = tr.net
    net.forward(True)
    net.backprop(False, first=True)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        net.forward(True)
        net.backprop(False, first=True)
        torch.cuda.synchronize()
    names = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    foreign = sorted(n for n in names if "at::native" in n)
    assert not foreign, foreign
    assert any("bn_ma_stats" in n for n in names) and any("bn_ma_bwd_apply" in n for n in names), sorted(names)
