"""Teacher-forced, per-element audit of one forward + backward pass of a NetTrainer, on either
device: what the executor's graph fusion (NeuralNet._fuse) makes of a net against the net's
conf-level meaning, in float64, with the bounds the kernel tests already derived.

Recording.  Every connection's layer.forward / layer.backprop is wrapped on the instance.  Right
before a layer's forward its input nodes are copied out; right before its backprop the gradient
buffers (Node.gdst) of its output nodes are.  Nothing under cxxnet_amd/ is changed.

Teacher forcing.  Every reference starts from values the executor itself stored (bf16 on the GPU),
so no error compounds and a relu mask, a dropout mask or a max-pool winner is decided by the stored
activation, as the kernels decide it.

Observation points are the conf's, not the executor's layout.  relu and dropout are elementwise; a
segment is one other layer (its head) and the elementwise layers behind it (its tail).
  forward   the node at the end of a segment, as each non-elementwise reader finds it right before
            its own forward.  conv -> relu is relu(conv_ref(x)) with the conv's bound (relu is
            1-Lipschitz); fullc -> relu -> dropout is 0 where the observed value is 0 and within
            the bound of relu(ref) / pkeep elsewhere.  concat, split, flatten and the max pooling
            move bits: exact.
  backward  the gradient of a head's output node, right before the head's backprop: in the fused
            and the unfused executor alike it is the gradient with respect to the head's raw
            output, the tail's relu' and dropout scale applied.  The reference is what the node's
            readers send back, each computed from that reader's own observed output gradient,
            input and weights, times the tail's mask read from the observed forward value; the
            bound is masked alike, so a masked element must be exactly 0.
              split     is transparent: its output gradients are not observed (sibling groups and
                        the folded split sum never store them); its input's gradient is the sum of
                        what the outputs' readers send back.
              ch_concat sends each input the channel slice of its own observed output gradient,
                        exactly.  Where every input ends a relu tail (a property of the conf), the
                        concat's own output gradient is compared under relu' of the concatenated
                        value: the unfused executor leaves the dead elements unmasked there and
                        the zero-copy one masks them, and the conf discards them either way -- the
                        exact check of the slices one layer down requires the zeros.
              max-pool -> LRN run as one kernel: the pooled gradient never exists, so it is not
                        observed, and the pool's input gradient is bounds.pool_lrn_backward_ref
                        of the LRN's observed output gradient.
  params    after the pass (the deferred bias sums flushed): dW and db of every conv and fullc from
            that layer's observed input and observed output gradient (weight_grad_ref /
            fc_weight_grad_ref / dbias_ref); a sibling group member through its own arena spec.

Fusion flags choose a bound where the fused arithmetic differs; never an expected value.

Bounds this module adds, from the roundings involved (u = 2^-8 bf16 store, eps = 2^-23 charged per
fp32 operation, gamma(K) = (K + 2) eps, as tests/bounds.py):
  scale_store   a value v within b of ref (bf16-stored or not) times the fp32 number s, stored as
            bf16: the product rounds once, |fl(s v) - s ref| <= s b + eps s (|ref| + b) = fp, and
            the store gives layer_bounds.store(s ref, fp).  Covers relu -> dropout in forward
            (fullc's bound b) and dropout's scale in backward; it is no smaller than the one-store
            bound of the fused forward.  The fused backward (the consumer's data-gradient GEMM
            scales by 1 / pkeep) takes fc_data_grad_ref(alpha = 1 / pkeep), whose extra rounding
            is charged against A.
  sum of n gradients (split; a sibling group's one GEMM; the folded split sum):  each term's value
            is within its own bound b_k of ref_k whether or not it was stored as bf16 in between;
            they are added in fp32 in any grouping -- at worst all K_k products of all readers in
            one accumulation -- and stored once:
                B = sum b_k,  gA = gamma(sum K_k + n) sum A_k,  bound = B + gA + u (|ref| + B + gA).
            A_k is the reader's operation on absolute values, K_k its accumulation length.
  fused bias gradient (GPU, not deterministic: summed by the max-pool's backward, the LRN's
            backward or the next conv's data-gradient epilogue from values before their bf16
            store or before the routing sum):  the fused sum's terms and the stored gradient's
            elements are both within the element's bound b_i of the same reference, so the two
            column sums differ by at most 2 sum_i b_i on top of dbias_ref's bound.  That is about
            R u / 128 of sum |dy|: it catches a bias summed from the wrong buffer or with a wrong
            mask, not one missing term; the unfused variants keep dbias_ref's own bound.
"""
from collections import namedtuple

import numpy as np
import torch

import bounds
import layer_bounds as LB
import pool_bounds as PB

ELEMENTWISE = ("relu", "dropout")
POOLS = ("max_pooling", "sum_pooling", "avg_pooling")
HEADS = ("conv", "fullc", "lrn", "ch_concat", "split", "flatten", "softmax") + POOLS
K_MAX = 1500  # weight_grad_ref: N Ho Wo up to which one missing term still exceeds the bound
FLAGS = ("fuse_relu", "zero_copy", "alias", "bias_of", "bias_below", "fused_lrn", "fused_into_producer", "folded")

Failure = namedtuple("Failure", "conn name direction message")
Grad = namedtuple("Grad", "ref bound A K")


def flag_counts(tr):
    """How many layers carry each fusion flag, and the number of sibling groups."""
    lays = [c.layer for c in tr.net.connections]
    out = {}
    for f in FLAGS:
        out[f] = sum(1 for l in lays if getattr(l, f, None) not in (None, False))
    out["sib_groups"] = len(getattr(tr.net, "sib_groups", ()))
    return out


def scale_store(ref, bound, s):
    fp = s * bound + bounds.EPS_F32 * s * (ref.abs() + bound)
    return s * ref, LB.store(s * ref, fp)


def _sum_grads(parts):
    if len(parts) == 1:
        return parts[0]
    ref = sum(p.ref for p in parts)
    B, A = sum(p.bound for p in parts), sum(p.A for p in parts)
    K = sum(p.K for p in parts) + len(parts)
    gA = bounds.gamma(K) * A
    return Grad(ref, B + gA + bounds.U_BF16 * (ref.abs() + B + gA), A, K)


class Report:
    def __init__(self):
        self.worst = {}     # (connection index, direction) -> worst d / bound
        self.failures = []
        self.names = {}

    def net_worst(self):
        return max(self.worst.values()) if self.worst else 0.0

    def by_direction(self):
        out = {}
        for (_, d), v in self.worst.items():
            out[d] = max(out.get(d, 0.0), v)
        return out

    def assert_clean(self):
        if self.failures:
            raise AssertionError("%d audit failures:\n%s" % (len(self.failures), "\n".join(
                f.message for f in self.failures)))


class Audit:
    def __init__(self, tr):
        self.tr, self.net = tr, tr.net
        net = self.net
        self.conns = net.connections
        self.kind = [c.layer.type_name for c in self.conns]
        names = {li: nm for nm, li in tr.net_cfg.layer_name_map.items()}
        self.name = [names.get(i, k) for i, k in enumerate(self.kind)]
        for i, c in enumerate(self.conns):
            if c.shared or self.kind[i] not in HEADS + ELEMENTWISE:
                raise NotImplementedError("net_audit: connection %d (%s) is not in the layer table" % (i, self.kind[i]))
        self.readers = {}
        for j, c in enumerate(self.conns):
            for k, n in enumerate(c.nodes_in):
                self.readers.setdefault(id(n), []).append((j, k))
        self.fwd_in, self.bwd_out, self.bwd_bound = {}, {}, {}
        self.soft = {}
        self.report = Report()
        self.tails = {}
        for i, c in enumerate(self.conns):
            if self.kind[i] in HEADS and self.kind[i] != "softmax":
                self.tails[i] = [self._tail(o) for o in c.nodes_out]
        self.relu_ends = {id(end) for ts in self.tails.values() for tail, end in ts
                          if any(self.kind[j] == "relu" for j in tail)}

    # ------------------------------------------------------------------ graph
    def _tail(self, o):
        tail, cur, seen = [], o, set()
        while True:
            rd = [j for j, _ in self.readers.get(id(cur), [])]
            loops = [j for j in rd if self.kind[j] in ELEMENTWISE and self.conns[j].nodes_out[0] is cur and j not in seen]
            if loops:
                tail.append(loops[0])
                seen.add(loops[0])
                continue
            ew = [j for j in rd if self.kind[j] in ELEMENTWISE and j not in seen]
            if not ew:
                return tail, cur
            non = [j for j in rd if self.kind[j] not in ELEMENTWISE]
            if non or len(ew) != 1:
                raise NotImplementedError("net_audit: node %s is read by an elementwise layer and another one" % cur.name)
            tail.append(ew[0])
            seen.add(ew[0])
            cur = self.conns[ew[0]].nodes_out[0]

    def _real_readers(self, node):
        return [(j, k) for j, k in self.readers.get(id(node), []) if self.kind[j] not in ELEMENTWISE]

    def _tail_ops(self, tail):
        """(has relu, dropout scale or 1.0) of a tail in training"""
        relu, s = False, 1.0
        for j in tail:
            if self.kind[j] == "relu":
                if self.conns[j].layer.kind != "relu":
                    raise NotImplementedError("net_audit: activation %s" % self.conns[j].layer.kind)
                relu = True
            else:
                thr = self.conns[j].layer.threshold
                if thr > 0:
                    if not relu:
                        raise NotImplementedError("net_audit: dropout not behind a relu (its mask cannot be read back)")
                    s *= float(np.float32(1) / np.float32(1.0 - thr))
        return relu, s

    # ------------------------------------------------------------------ recording
    def _snap(self, t, node=None):
        b = self.net.cur_batch
        t = t.detach()[:b]
        if node is not None and t.dim() == 4 and t.shape[2] > max(node.shape[3], 1) and not node.is_mat():
            t = t[:, :, :node.shape[3]]  # a row-padded input node
        return t.to("cpu").clone()

    def _wrap(self):
        self._saved = []
        for i, conn in enumerate(self.conns):
            lay = conn.layer
            self._saved.append((lay, lay.__dict__.get("forward"), lay.__dict__.get("backprop")))
            f0, b0 = lay.forward, lay.backprop

            def fwd(is_train, nin, nout, i=i, f0=f0):
                self.fwd_in[i] = [self._snap(n.data, n) for n in nin]
                f0(is_train, nin, nout)
                if self.kind[i] == "softmax":
                    self.soft = {"y": self._snap(nout[0].data), "p32": self._snap(self.conns[i].layer.p32)}

            def bwd(prop_grad, nin, nout, i=i, b0=b0):
                self.bwd_out[i] = [self._snap(n.gdst, n) for n in nout]
                b0(prop_grad, nin, nout)
            lay.forward, lay.backprop = fwd, bwd

    def _unwrap(self):
        for lay, f, b in self._saved:
            for name, v in (("forward", f), ("backprop", b)):
                if v is None:
                    del lay.__dict__[name]
                else:
                    setattr(lay, name, v)

    # ------------------------------------------------------------------ layer parameters
    def _wb(self, i):
        lay = self.conns[i].layer
        return lay.w.wb.detach().to("cpu"), (lay.b.w.detach().to("cpu") if lay.b is not None else None)

    def _conv_kw(self, i):
        lp = self.conns[i].layer.lp
        return dict(stride=lp.stride, pad=(lp.pad_y, lp.pad_x), groups=lp.num_group)

    def _pool_args(self, i):
        lay = self.conns[i].layer
        lp = lay.lp
        assert not lay.tie_all and not lay.relu
        return lp.kernel_height, lp.kernel_width, lp.stride, lp.pad_y

    def _lrn_args(self, i):
        lay = self.conns[i].layer
        return lay.nsize, lay.alpha, lay.beta, lay.knorm

    # ------------------------------------------------------------------ forward references
    def _forward_ref(self, i):
        """[(ref, bound)] per output of head i, from its observed inputs (before the tail)"""
        kind, xs = self.kind[i], self.fwd_in[i]
        x = xs[0]
        if kind == "conv":
            w, b = self._wb(i)
            return [bounds.forward_ref(x, w, b, **self._conv_kw(i))]
        if kind == "fullc":
            w, b = self._wb(i)
            ref, bound = bounds.fc_forward_ref(x.reshape(x.shape[0], -1), w, b)
            return [(ref.reshape(ref.shape[0], 1, -1, 1), bound.reshape(ref.shape[0], 1, -1, 1))]
        if kind == "max_pooling":
            y, _ = PB.max_forward_ref(x, *self._pool_args(i))
            return [(y, torch.zeros_like(y))]
        if kind in POOLS:
            return [PB.sum_forward_ref(x, *self._pool_args(i), kind[:3])]
        if kind == "lrn":
            return [bounds.lrn_forward_ref(x, *self._lrn_args(i))]
        if kind == "ch_concat":
            y = torch.cat([t.double() for t in xs], -1)
            return [(y, torch.zeros_like(y))]
        if kind == "split":
            return [(x.double(), torch.zeros(x.shape, dtype=torch.float64)) for _ in self.conns[i].nodes_out]
        if kind == "flatten":
            y = x.double().permute(0, 3, 1, 2).reshape(x.shape[0], 1, -1, 1)
            return [(y, torch.zeros_like(y))]
        raise NotImplementedError(kind)

    # ------------------------------------------------------------------ backward references
    def _reader_grad(self, j, k):
        """Grad of what reader j sends back to its k-th input node"""
        kind = self.kind[j]
        x = self.fwd_in[j][k]
        if kind == "split":
            return _sum_grads([self._node_grad(o) for o in self.conns[j].nodes_out])
        dy = self.bwd_out[j][0] if kind != "softmax" else None
        if kind == "conv":
            w, _ = self._wb(j)
            kw = dict(self._conv_kw(j), in_hw=tuple(x.shape[1:3]))
            ref, bound = bounds.data_grad_ref(dy, w, **kw)
            A, _ = bounds.data_grad_ref(dy.abs(), w.abs(), **kw)
            return Grad(ref, bound, A, w.shape[1] * w.shape[2] * (w.shape[0] // kw["groups"]))
        if kind == "fullc":
            w, _ = self._wb(j)
            d2 = dy.reshape(dy.shape[0], -1)
            ref, bound = bounds.fc_data_grad_ref(d2, w)
            A = d2.double().abs() @ w.double().abs()
            return Grad(ref.reshape(x.shape), bound.reshape(x.shape), A.reshape(x.shape), w.shape[0] + 1)
        if kind == "max_pooling":
            args = self._pool_args(j)
            if self.conns[j].layer.fused_lrn is not None:
                (jl, _), = self._real_readers(self.conns[j].nodes_out[0])
                r = bounds.pool_lrn_backward_ref(x, self.bwd_out[jl][0], *self._lrn_args(jl), 0)
                return Grad(r["dx"], r["dx_bound"], r["dx"].abs() + r["dx_bound"], 4)
            _, st = PB.max_forward_ref(x, *args)
            ref, bound = PB.max_backward_ref(x, st, dy, *args)
            A, _ = PB.max_backward_ref(x, st, dy.abs(), *args)
            return Grad(ref, bound, A, PB.windows_over_a_pixel(*args[:3]))
        if kind in POOLS:
            args = self._pool_args(j)
            ref, bound = PB.sum_backward_ref(x, dy, *args, kind[:3])
            A, _ = PB.sum_backward_ref(x, dy.abs(), *args, kind[:3])
            return Grad(ref, bound, A, PB.windows_over_a_pixel(*args[:3]) + 2)
        if kind == "lrn":
            ref, bound = bounds.lrn_backward_ref(x, dy, *self._lrn_args(j))
            return Grad(ref, bound, ref.abs() + bound, self._lrn_args(j)[0])
        if kind == "flatten":
            n, h, w, c = x.shape
            ref = dy.double().reshape(n, c, h, w).permute(0, 2, 3, 1).contiguous()
            return Grad(ref, torch.zeros_like(ref), ref.abs(), 1)
        if kind == "ch_concat":
            off = sum(t.shape[-1] for t in self.fwd_in[j][:k])
            ref = dy.double()[..., off:off + x.shape[-1]].contiguous()
            return Grad(ref, torch.zeros_like(ref), ref.abs(), 1)
        if kind == "softmax":
            lay = self.conns[j].layer
            label = self.net.ctx.label_fields[lay.target][:x.shape[0]].detach().to("cpu")
            bs = lay.batch_size if lay.batch_size > 0 else self.conns[j].nodes_in[0].batch
            scale = lay.grad_scale / (bs * lay.update_period) * getattr(self.net.ctx, "loss_weight", 1.0)
            ref, bound = bounds.loss_grad_ref(self.soft["p32"], label, scale, lay.kind)
            return Grad(ref.reshape(x.shape), bound.reshape(x.shape), ref.abs().reshape(x.shape), 1)
        raise NotImplementedError(kind)

    def _node_grad(self, node):
        rs = self._real_readers(node)
        if not rs:
            raise NotImplementedError("net_audit: node %s has no reader" % node.name)
        return _sum_grads([self._reader_grad(j, k) for j, k in rs])

    # ------------------------------------------------------------------ checks
    def _check(self, i, direction, fn):
        what = "connection %d (%s) %s" % (i, self.name[i], direction)
        try:
            worst = fn(what)
        except AssertionError as e:
            self.report.failures.append(Failure(i, self.name[i], direction, "%s: %s" % (what, e)))
            worst = float("inf")
        key = (i, direction)
        self.report.worst[key] = max(self.report.worst.get(key, 0.0), worst)

    def _check_forward(self, i):
        if self.kind[i] == "softmax":
            def soft(what):
                x = self.fwd_in[i][0]
                p, b32, b16 = bounds.softmax_ref(x.reshape(x.shape[0], -1))
                w1 = bounds.assert_within(self.soft["y"].reshape(p.shape), p, b16, what + " (node)", axes="nk")
                w2 = bounds.assert_within(self.soft["p32"].reshape(p.shape), p, b32, what + " (fp32 copy)", axes="nk")
                return max(w1, w2)
            self._check(i, "fwd", soft)
            return
        refs = self._forward_ref(i)
        for (ref, bound), (tail, end) in zip(refs, self.tails[i]):
            relu, s = self._tail_ops(tail)
            if relu:
                ref = ref.clamp_min(0)
            if s != 1.0:
                ref, bound = scale_store(ref, bound, s)
            for j, k in self._real_readers(end):
                obs = self.fwd_in[j][k]
                r, b = ref, bound
                if s != 1.0:  # dropped elements are exactly 0: the mask is read from the observed value
                    keep = (obs.double() != 0).to(torch.float64)
                    r, b = ref * keep, bound * keep
                self._check(i, "fwd", lambda what, obs=obs, r=r, b=b, j=j: bounds.assert_within(
                    obs, r, b, "%s as read by connection %d (%s)" % (what, j, self.name[j])))

    def _unmaterialised(self, i):
        return self.kind[i] == "max_pooling" and self.conns[i].layer.fused_lrn is not None

    def _check_backward(self, i):
        if self.kind[i] in ("split", "softmax") or self._unmaterialised(i):
            return
        (tail, end), = self.tails[i]
        rs = self._real_readers(end)
        relu, s = self._tail_ops(tail)
        g = self._node_grad(end)
        ref, bound = g.ref, g.bound
        obs = self.bwd_out[i][0]
        fwd_end = self.fwd_in[rs[0][0]][rs[0][1]].double()
        if s != 1.0:
            j = rs[0][0]
            lay = self.conns[j].layer
            if len(rs) == 1 and self.kind[j] == "fullc" and getattr(lay, "grad_alpha", 1.0) != 1.0:
                # the consumer's data-gradient GEMM scales by 1 / pkeep itself (NeuralNet._fuse_dropout)
                dy = self.bwd_out[j][0]
                w, _ = self._wb(j)
                ref, bound = bounds.fc_data_grad_ref(dy.reshape(dy.shape[0], -1), w, alpha=s)
                ref, bound = ref.reshape(obs.shape), bound.reshape(obs.shape)
            else:
                ref, bound = scale_store(ref, bound, s)
        got = obs
        if relu:
            m = (fwd_end > 0).to(torch.float64).reshape(ref.shape)
            ref, bound = ref * m, bound * m
        elif self.kind[i] == "ch_concat" and all(id(n) in self.relu_ends for n in self.conns[i].nodes_in):
            m = (fwd_end > 0).to(torch.float64)
            ref, bound, got = ref * m, bound * m, obs.double() * m
        self.bwd_bound[i] = bound
        self._check(i, "bwd", lambda what: bounds.assert_within(got, ref.reshape(obs.shape), bound.reshape(obs.shape), what))

    def _fused_bias(self, lay):
        from cxxnet_amd.ops.gemm import deterministic
        if not self.net.ctx.is_gpu or deterministic():
            return False
        return any(getattr(c.layer, "bias_of", None) is lay or getattr(c.layer, "bias_below", None) is lay
                   for c in self.conns)

    def _check_params(self, i):
        if self.kind[i] not in ("conv", "fullc"):
            return
        lay = self.conns[i].layer
        x, dy = self.fwd_in[i][0], self.bwd_out[i][0]
        gw = lay.w.g.detach().to("cpu")
        if self.kind[i] == "conv":
            assert dy.shape[0] * dy.shape[1] * dy.shape[2] <= K_MAX, "net too large for weight_grad_ref: %s" % (dy.shape,)
            ref, bound = bounds.weight_grad_ref(x, dy, torch.zeros_like(gw), **self._conv_kw(i))
            axes = "okhc"
        else:
            ref, bound = bounds.fc_weight_grad_ref(x.reshape(x.shape[0], -1), dy.reshape(dy.shape[0], -1))
            axes = "oi"
        self._check(i, "dW", lambda what: bounds.assert_within(gw, ref, bound, what, axes=axes))
        if lay.b is None:
            return
        d2 = dy.reshape(-1, dy.shape[-1]) if self.kind[i] == "conv" else dy.reshape(dy.shape[0], -1)
        bref, bbound = bounds.dbias_ref(d2, 0.0)
        if self._fused_bias(lay) and i in self.bwd_bound:
            bbound = bbound + 2 * self.bwd_bound[i].reshape(-1, d2.shape[-1]).sum(0)
        gb = lay.b.g.detach().to("cpu")
        self._check(i, "db", lambda what: bounds.assert_within(gb, bref, bbound, what, axes="c"))

    # ------------------------------------------------------------------ the pass
    def run(self, batch):
        tr = self.tr
        assert tr.update_period == 2 and tr.sample_counter == 0, "audit the first pass of an update_period = 2 cycle"
        self._wrap()
        try:
            tr.update(batch)
        finally:
            self._unwrap()
        if self.net.device.type == "cuda":
            torch.cuda.synchronize()
        for i in range(len(self.conns)):
            if self.kind[i] in HEADS:
                self._check_forward(i)
        for i in range(len(self.conns) - 1, -1, -1):
            if self.kind[i] in HEADS:
                self._check_backward(i)
        for i in range(len(self.conns)):
            self._check_params(i)
        return self.report


def audit(tr, batch):
    """Run one recorded training pass of batch and return the Report: worst d / bound per
    (connection, direction) and the failures, each naming connection, direction and the first
    offending elements."""
    return Audit(tr).run(batch)


# ---------------------------------------------------------------------------------------- the nets
ALEX_MINI = """
netconfig=start
layer[0->c1] = conv:conv1
  kernel_size = 3
  nchannel = 16
layer[c1->r1] = relu
layer[r1->p1] = max_pooling
  kernel_size = 3
  stride = 2
layer[p1->n1] = lrn
  local_size = 5
  alpha = 1.0
  beta = 0.75
  knorm = 2
layer[n1->c2] = conv:conv2
  kernel_size = 3
  pad = 1
  nchannel = 24
layer[c2->r2] = relu
layer[r2->c3] = conv:conv3
  kernel_size = 3
  pad = 1
  nchannel = 16
layer[c3->r3] = relu
layer[r3->p2] = max_pooling
  kernel_size = 3
  stride = 2
layer[p2->fl] = flatten
layer[fl->f1] = fullc:fc1
  nhidden = 40
layer[f1->h1] = relu
layer[h1->h1] = dropout
  threshold = 0.5
layer[h1->f2] = fullc:fc2
  nhidden = 24
layer[f2->h2] = relu
layer[h2->h2] = dropout
  threshold = 0.5
layer[h2->f3] = fullc:fc3
  nhidden = 10
layer[f3->f3] = softmax
netconfig=end
input_shape = 3,19,17
random_type = xavier
eta = 0.05
momentum = 0.9
wd = 0.0005
"""


def _module(p, src):
    return """
layer[{src}->{p}i1,{p}i2,{p}i3,{p}i4] = split
layer[{p}i1->{p}1] = conv:{p}_1x1
  kernel_size = 1
  nchannel = 8
layer[{p}1->{p}1r] = relu
layer[{p}i2->{p}2] = conv:{p}_3x3r
  kernel_size = 1
  nchannel = 8
layer[{p}2->{p}2r] = relu
layer[{p}2r->{p}3] = conv:{p}_3x3
  kernel_size = 3
  pad = 1
  nchannel = 16
layer[{p}3->{p}3r] = relu
layer[{p}i3->{p}4] = conv:{p}_5x5r
  kernel_size = 1
  nchannel = 8
layer[{p}4->{p}4r] = relu
layer[{p}4r->{p}5] = conv:{p}_5x5
  kernel_size = 5
  pad = 2
  nchannel = 8
layer[{p}5->{p}5r] = relu
layer[{p}i4->{p}p] = max_pooling
  kernel_size = 3
  stride = 1
  pad = 1
layer[{p}p->{p}6] = conv:{p}_proj
  kernel_size = 1
  nchannel = 8
layer[{p}6->{p}6r] = relu
layer[{p}1r,{p}3r,{p}5r,{p}6r->{p}cat] = ch_concat
""".format(p=p, src=src)


INCEPTION_MINI = """
netconfig=start
layer[0->s0] = conv:stem
  kernel_size = 3
  pad = 1
  nchannel = 16
layer[s0->s0r] = relu
layer[s0r->n0] = lrn
  local_size = 5
  alpha = 1.0
  beta = 0.75
  knorm = 2
""" + _module("a", "n0") + _module("b", "acat") + """
layer[bcat->gp] = avg_pooling
  kernel_size = 3
  stride = 2
layer[gp->fl] = flatten
layer[fl->fc] = fullc:fc
  nhidden = 10
layer[fc->fc] = softmax
netconfig=end
input_shape = 8,11,9
random_type = xavier
eta = 0.05
momentum = 0.9
wd = 0.0005
"""

NETS = {"alex_mini": ALEX_MINI, "inception_mini": INCEPTION_MINI}
BATCH = 3


def make_trainer(net, dev, extra=()):
    """A NetTrainer of one of the tiny nets at batch 3, update_period 2 (the first update() is
    forward + backward only: the gradients survive it), eager and hookable, with random biases
    (the initial ones are 0, which would leave the bias add untested)."""
    from cxxnet_amd import native
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in list(native.rt().parse_config(NETS[net])) + [
            ("batch_size", str(BATCH)), ("dev", dev), ("eval_train", "0"), ("silent", "1"), ("seed", "7"),
            ("update_period", "2"), ("cuda_graph", "0"), ("launch_replay", "0")] + list(extra):
        tr.set_param(k, v)
    tr.init_model()
    g = torch.Generator().manual_seed(11)
    for li, spec in sorted(tr.net.arena.specs, key=lambda t: (t[0], t[1].tag)):
        if spec.tag == "bias":
            spec.w.copy_((torch.rand(spec.shape, generator=g) - 0.5) * 0.2)
    tr.net.arena.sync_shadow()
    return tr


def make_batch(net, seed=1):
    from cxxnet_amd.io.data import DataBatch
    c, h, w = [int(v) for v in NETS[net].split("input_shape =")[1].split("\n")[0].split(",")]
    g = torch.Generator().manual_seed(seed)
    return DataBatch(torch.randn(BATCH, c, h, w, generator=g), torch.randint(0, 10, (BATCH, 1), generator=g).float())


def layer_of(tr, name):
    return tr.net.connections[tr.net_cfg.layer_name_map[name]].layer


def conn_of(tr, name):
    return tr.net_cfg.layer_name_map[name]
