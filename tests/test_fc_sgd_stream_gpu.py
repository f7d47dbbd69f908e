"""The streaming fc weight-gradient + SGD kernel (csrc/kernels/fc_wgrad_sgd.hip) against the tile
kernel it replaces (cxn_gemm_set_sgd_stream(0)) -- bitwise -- and against an fp32 torch reference,
on the smallest shapes that take each of its paths: one strip x one chunk; blocks that own several
chunks (the rolling w / m window, the LDS handed from the staging to the next chunk's DMAs) and
cross into the next strip (dy fragments reloaded), which small layers reach only with the block
count capped (cxn_gemm_set_sgd_stream_blocks); tail strip, tail chunk, K tails; both compiled forms
(K <= 256 and K <= 512); fc8's 1000 rows; arena slices between sentinels; device hyper-parameters,
clip, weight decay, a NaN gradient."""
import pytest
import torch

from cxxnet_amd import native, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
RJ, CI = 64, 128  # the kernel's strip rows and chunk columns
FORCED = 2        # cxn_gemm_set_sgd_stream: the stream on every shape it can serve
HYP = (0.01, 5e-4, 0.9, 0.0)  # lr, wd, mom, clip
# 3 strips (the last 8 rows) x 5 chunks (the last 8 columns) in 2 blocks: items [0, 7) and [7, 15),
# so each block owns several chunks of a strip and crosses into the next one
TAILS = (4 * CI + 8, 2 * RJ + 8)


def _inputs(nin, nout, K, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(K, nin, generator=g, device=DEV).to(torch.bfloat16)
    dy = torch.randn(K, nout, generator=g, device=DEV).to(torch.bfloat16)
    w = torch.randn(nout, nin, generator=g, device=DEV) * 0.02
    m = torch.randn(nout, nin, generator=g, device=DEV) * 0.01
    return x, dy, w, m, w.to(torch.bfloat16)


def _run(mode, x, dy, w, m, wb, hyp=HYP, calls=1, dev_hyp=False, expect_stream=None, blocks=0, inplace=False):
    """`calls` fused steps on copies of (w, m, wb) (inplace: on them) with the stream switch at
    `mode` and its block count at `blocks` (0: what the CUs hold); returns the updated tensors.
    expect_stream: assert that the streaming kernel did / did not serve the calls."""
    k = native.kernels()
    if not inplace:
        w, m, wb = w.clone(), m.clone(), wb.clone()
    h = torch.tensor(hyp, device=DEV) if dev_hyp else None
    args = (0.0, 0.0, 0.0, 0.0) if dev_hyp else hyp  # the device array must win over the scalars
    old = k.cxn_gemm_set_sgd_stream(mode)
    old_blocks = k.cxn_gemm_set_sgd_stream_blocks(blocks)
    n0 = k.cxn_gemm_sgd_stream_calls()
    try:
        for _ in range(calls):
            assert ops.fc_backward_weight_sgd(x, dy, w, m, wb, *args, h)
        torch.cuda.synchronize()
    finally:
        k.cxn_gemm_set_sgd_stream(old)
        k.cxn_gemm_set_sgd_stream_blocks(old_blocks)
    if expect_stream is not None:
        assert k.cxn_gemm_sgd_stream_calls() - n0 == (calls if expect_stream else 0)
    return w, m, wb


def _bits_equal(a, b):
    ia = a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int16)
    ib = b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int16)
    return bool(torch.equal(ia, ib))


def _assert_same(got, ref):
    for name, a, b in zip(("w", "m", "wb"), got, ref):
        assert _bits_equal(a, b), f"{name} differs from the tile kernel's"


# (nin, nout, K, blocks)
SHAPES = [
    (CI, RJ, 32, 0),                 # one strip x one chunk
    (3 * CI, 2 * RJ, 256, 0),        # 2 strips x 3 chunks, one block per chunk
    (3 * CI, 2 * RJ, 256, 1),        # ... all in one block: 3 chunks, then the next strip
    (3 * CI, 2 * RJ, 256, 4),        # ... shares of 1, 2, 1, 2 chunks
    TAILS + (96, 2),                 # tail strip, tail chunk, K no multiple of 64, strip crossing
    TAILS + (256, 2),
    TAILS + (320, 2),                # the K <= 512 form (1 block per CU, 8 k-tiles per trip)
    TAILS + (328, 2),                # ... K no multiple of 64 (nor of 32)
    TAILS + (512, 2),
    (3 * CI, 2 * RJ, 512, 0),
    (4096, 1000, 256, 0),            # fc8: 16 x 32 chunks, one per block
    (4096, 1000, 256, 48),           # ... 10-11 per block, every block but the ends crossing strips
]
_ID = lambda t: "x".join(str(v) for v in t)  # noqa: E731


@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
def test_bitwise_against_tile_kernel(shape):
    nin, nout, K, blocks = shape
    t = _inputs(nin, nout, K)
    for calls in (1, 2):
        ref = _run(0, *t, calls=calls, expect_stream=False)
        got = _run(FORCED, *t, calls=calls, expect_stream=True, blocks=blocks)
        _assert_same(got, ref)
        assert not _bits_equal(got[0], t[2]), "the step changed nothing"


def test_default_mode():
    """The default setting serves a layer with at least two chunks per resident block and leaves a
    small one to the tile kernel; the result is the tile kernel's either way."""
    big = _inputs(4096, 2048, 64)
    _assert_same(_run(1, *big, expect_stream=True), _run(0, *big, expect_stream=False))
    small = _inputs(512, 128, 256)
    _assert_same(_run(1, *small, expect_stream=False), _run(0, *small, expect_stream=False))


def test_declined_shape_takes_the_tile_kernel():
    t = _inputs(CI, 128, 1024)  # K > 512: not served by the stream
    got = _run(FORCED, *t, expect_stream=False)
    _assert_same(got, _run(0, *t, expect_stream=False))


@pytest.mark.parametrize("K", [64, 320])
def test_arena_slices_between_sentinels(K):
    nin, nout = TAILS
    x, dy, w0, m0, wb0 = _inputs(nin, nout, K)
    n = nin * nout
    SENT = 12345.0

    def arena(dtype, off, src):
        buf = torch.full((n + 4096,), SENT, dtype=dtype, device=DEV)
        sl = buf[off:off + n].view(nout, nin)
        sl.copy_(src)
        return buf, sl

    # 16-byte aligned, not 1 KiB aligned
    fw, w = arena(torch.float32, 36, w0)
    fm, m = arena(torch.float32, 1028, m0)
    fb, wb = arena(torch.bfloat16, 40, wb0)
    for p in (w, m, wb):
        assert p.data_ptr() % 16 == 0 and p.data_ptr() % 1024 != 0
    ref = _run(0, x, dy, w0, m0, wb0, calls=2)
    _run(FORCED, x, dy, w, m, wb, calls=2, expect_stream=True, blocks=2, inplace=True)
    _assert_same((w, m, wb), ref)
    for buf, off in ((fw, 36), (fm, 1028), (fb, 40)):
        assert bool((buf[:off] == SENT).all()) and bool((buf[off + n:] == SENT).all())


@pytest.mark.parametrize("K", [96, 328])
@pytest.mark.parametrize("case", ["dev_hyp", "clip", "wd0", "nan_clip", "nan_noclip"])
def test_hyper_parameter_and_gradient_edges(case, K):
    x, dy, w, m, wb = _inputs(*TAILS, K)
    hyp, dev = HYP, False
    if case == "dev_hyp":
        hyp, dev = (0.02, 1e-3, 0.8, 0.5), True
    elif case == "clip":
        hyp = (0.01, 5e-4, 0.9, 0.25)
    elif case == "wd0":
        hyp = (0.01, 0.0, 0.9, 0.0)
    elif case.startswith("nan"):
        dy[5, 7] = float("nan")
        hyp = (0.01, 5e-4, 0.9, 0.25 if case == "nan_clip" else 0.0)
    ref = _run(0, x, dy, w, m, wb, hyp=hyp, dev_hyp=dev, calls=2, expect_stream=False)
    got = _run(FORCED, x, dy, w, m, wb, hyp=hyp, dev_hyp=dev, calls=2, expect_stream=True, blocks=2)
    _assert_same(got, ref)
    if case == "nan_clip":
        assert bool(torch.isfinite(got[0]).all())  # NaN gradient -> 0 under clipping


def _relnorm(a, ref):
    a, ref = a.float(), ref.float()
    return ((a - ref).norm() / ref.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("shape", SHAPES, ids=_ID)
def test_against_torch_fp32(shape):
    """As check_fc_sgd of test_tune_table_gpu.py, with its tolerance."""
    nin, nout, K, blocks = shape
    x, dy, w, m, wb = _inputs(nin, nout, K)
    lr, wd, mom, _ = HYP
    g = dy.float().t() @ x.float()
    m_ref = mom * m - lr * (g + wd * w)
    w_ref = w + m_ref
    w1, m1, wb1 = _run(FORCED, x, dy, w, m, wb, expect_stream=True, blocks=blocks)
    err = max(_relnorm(m1, m_ref), _relnorm(w1, w_ref), _relnorm(wb1.float(), w_ref))
    assert err < 1e-2, (nin, nout, K, err)
