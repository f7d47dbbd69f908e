"""Float64 references and derived per-element error bounds for the batch_norm_ma kernels
(csrc/kernels/bn_ma_kernels.hip), in the style of tests/bounds.py: the operands are the exact
bf16 / fp32 values the kernel reads, the reference is float64 on the CPU, and every bound comes
from the arithmetic -- none is tuned to what a kernel gives.

  u = 2^-23   fp32 unit in the last place (a rounded fp32 operation errs by at most u / 2 |v|;
              u itself leaves room for fused / unfused forms and reciprocal-based division)
  U = 2^-8    bf16 unit roundoff of a stored output (tests/bounds.py)
  g(R) = (R + 2) u   R fp32 additions in any order, against the sum of the absolute terms

Statistics over the R rows of a channel (fp32 results, checked directly, so that a wrong
statistic is caught here and not hidden under an output's bf16 rounding):

  mean   e_mean = g(R) sum|x| / R
  var    e_var  = g(R) var                               (the sum of the squared deviations)
                + 8 u max|x| sum|x - mean| / R           (propagated mean error, first order: every
                                                          deviation x - m is formed against a partial
                                                          mean m that is itself a rounded fp32 value,
                                                          within 4 u max|x| of the exact partial mean
                                                          -- product, add, store, subtract -- and
                                                          each term d_old d_new carries it twice)
                + e_mean^2                               (second order: sum (x - m')^2 / R
                                                          = var + (m' - mean)^2)
           This is what a Welford / pairwise-merge / shifted-sum scheme can meet.  Raw fp32 sums
           E[x^2] - E[x]^2 cannot: their error scales with mean^2, not with var
           (tests/test_bn_bounds_cpu.py shows it on case c, mean / std ~ 50).
  inv = (var + eps)^-1/2:   e_inv = inv^3 e_var / 2 + 3 u inv   (first order + sqrt, divide, add)
  running <- m running + (1 - m) batch:  e' = m e + (1 - m) e_batch + 3 u (|m running| + |(1 - m) batch|)
           (m is taken as an exactly representable value, 0.75, in the kernel tests)

Outputs (bf16), with a = slope inv, b = bias - mean a, y = x a + b = (x - mean) a + bias:

  y      U |ref| + |x - mean| |slope| e_inv + |a| e_mean + 4 u (|x a| + |mean a| + |bias|)
  inference y from given fp32 running statistics (exact inputs):
         U |ref| + |x - rmean| 3 u |a| + 4 u (|x a| + |rmean a| + |bias|)
  backward, sg = sum g, sgx = sum g (x - mean), A = a, B = -A inv^2 sgx / R, Cc = -A sg / R,
  dx = A g + (x - mean) B + Cc:
         e_sg  = g(R) sum|g|          e_sgx = g(R) sum|g (x - mean)| + e_mean sum|g|
         gbias  = gbias0 + sg:        g(R) (sum|g| + |gbias0|)
         gslope = gslope0 + inv sgx:  g(R) (inv sum|g (x - mean)| + |gslope0|) + inv e_mean sum|g|
                                      + e_inv sum|g (x - mean)|
         e_A = |slope| e_inv;  e_B = 3 |B| e_inv / inv + |A| inv^2 e_sgx / R + 4 u |B|
         e_C = |Cc| e_inv / inv + |A| e_sg / R + 4 u |Cc|
         dx:  U |ref| + |g| e_A + |x - mean| e_B + |B| e_mean + e_C
              + 4 u (|A g| + |(x - mean) B| + |Cc|)
"""
import torch

from bounds import U_BF16, assert_within, violations  # noqa: F401  (re-exported for the tests)

U32 = 2.0 ** -23


def _f64(t):
    return t.detach().to("cpu", torch.float64)


def g(R):
    return (R + 2) * U32


def stats_ref(x):
    """x [R][C] (exact bf16 values) -> dict of float64 mean, var (biased), and their bounds."""
    x = _f64(x)
    R = x.shape[0]
    mean = x.sum(0) / R
    d = x - mean
    var = (d * d).sum(0) / R
    e_mean = g(R) * x.abs().sum(0) / R
    e_var = g(R) * var + 8 * U32 * x.abs().amax(0) * d.abs().sum(0) / R + e_mean ** 2
    return {"R": R, "mean": mean, "var": var, "e_mean": e_mean, "e_var": e_var, "d": d}


def inv_ref(var, e_var, eps):
    inv = (var + eps) ** -0.5
    return inv, 0.5 * inv ** 3 * e_var + 3 * U32 * inv


def running_ref(run, e_run, batch, e_batch, m):
    """One step of running <- m running + (1 - m) batch, with its propagated bound."""
    new = m * run + (1 - m) * batch
    e = m * e_run + (1 - m) * e_batch + 3 * U32 * ((m * run).abs() + ((1 - m) * batch).abs())
    return new, e


def forward_ref(x, slope, bias, eps):
    """(y ref, y bound, stats) of the training forward."""
    s = stats_ref(x)
    x, slope, bias = _f64(x), _f64(slope), _f64(bias)
    inv, e_inv = inv_ref(s["var"], s["e_var"], eps)
    a = slope * inv
    ref = s["d"] * a + bias
    bound = (U_BF16 * ref.abs() + s["d"].abs() * slope.abs() * e_inv + a.abs() * s["e_mean"]
             + 4 * U32 * ((x * a).abs() + (s["mean"] * a).abs() + bias.abs()))
    s.update(inv=inv, e_inv=e_inv)
    return ref, bound, s


def infer_ref(x, slope, bias, rmean, rvar, eps):
    """(y ref, y bound) of the inference forward from the given fp32 running statistics."""
    x, slope, bias, rmean, rvar = _f64(x), _f64(slope), _f64(bias), _f64(rmean), _f64(rvar)
    a = slope * (rvar + eps) ** -0.5
    ref = (x - rmean) * a + bias
    bound = (U_BF16 * ref.abs() + (x - rmean).abs() * 3 * U32 * a.abs()
             + 4 * U32 * ((x * a).abs() + (rmean * a).abs() + bias.abs()))
    return ref, bound


def backward_ref(gy, x, slope, gslope0, gbias0, eps):
    """dict of (ref, bound) pairs for dx, gslope, gbias; the statistics are those of x."""
    s = stats_ref(x)
    R = s["R"]
    gy, slope, gslope0, gbias0 = _f64(gy), _f64(slope), _f64(gslope0), _f64(gbias0)
    inv, e_inv = inv_ref(s["var"], s["e_var"], eps)
    d, e_mean = s["d"], s["e_mean"]
    sg, sgx = gy.sum(0), (gy * d).sum(0)
    a_g, a_gx = gy.abs().sum(0), (gy * d).abs().sum(0)
    e_sg = g(R) * a_g
    e_sgx = g(R) * a_gx + e_mean * a_g
    A = slope * inv
    B = -A * inv * inv * sgx / R
    Cc = -A * sg / R
    e_A = slope.abs() * e_inv
    e_B = 3 * B.abs() * e_inv / inv + A.abs() * inv * inv * e_sgx / R + 4 * U32 * B.abs()
    e_C = Cc.abs() * e_inv / inv + A.abs() * e_sg / R + 4 * U32 * Cc.abs()
    dx = A * gy + d * B + Cc
    dx_b = (U_BF16 * dx.abs() + gy.abs() * e_A + d.abs() * e_B + B.abs() * e_mean + e_C
            + 4 * U32 * ((A * gy).abs() + (d * B).abs() + Cc.abs()))
    gslope = gslope0 + inv * sgx
    gslope_b = g(R) * (inv * a_gx + gslope0.abs()) + inv * e_mean * a_g + e_inv * a_gx
    gbias = gbias0 + sg
    gbias_b = g(R) * (a_g + gbias0.abs())
    return {"dx": (dx, dx_b), "gslope": (gslope, gslope_b), "gbias": (gbias, gbias_b)}


def case_c_inputs(R=130, C=64, seed=3):
    """Case c of the kernel tests: 64 + 0.5 k, k uniform in -4..4 (exact in bf16), mean / std ~ 50."""
    gen = torch.Generator().manual_seed(seed)
    k = torch.randint(-4, 5, (R, C), generator=gen)
    return (64.0 + 0.5 * k.float()).to(torch.bfloat16)
