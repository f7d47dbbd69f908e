"""bench.py --dump-outputs on the GPU: what it writes does not depend on how many steps were timed."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dump(out_dir, steps):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--model", "alexnet", "--batch", "32",
                        "--steps", str(steps), "--warmup", "2", "--dump-outputs", str(out_dir)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return {f: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}


def test_dump_independent_of_timed_steps(tmp_path):
    """AlexNet at batch 32, 1 against 12 timed steps: every file agrees to 2^-10 of its range.
    The case: batch 32 is the launch-list replay regime and the smallest AlexNet batch of the shipped
    tile table; at a batch outside it (16) the GEMM tiles are timed on first use, two runs may pick
    different kernels, and no dump of them repeats (profiles/bench_dump_repeatability.md).
    The bound: run-to-run noise enters only through the order of fp32 atomic sums (eps 6e-8;
    measured 2.3e-7 of the range), while everything a step computes passes through bf16 (eps 2^-8),
    so a quarter of a bf16 ulp of the range is far above the noise and far below what state carried
    over from the timed steps does (momentum alone is 0.9 of a step)."""
    a, b = _dump(tmp_path / "a", 1), _dump(tmp_path / "b", 12)
    assert a.keys() == b.keys() and "scores.npy" in a
    assert any(f.startswith("step_") for f in a)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for f in a:
        assert a[f].dtype == np.float32 and np.isfinite(a[f]).all()
        rng = float(np.abs(a[f]).max())
        assert rng > 0, f
        d = float(np.abs(a[f].astype(np.float64) - b[f]).max())
        print(f, "range %.3g max|diff| %.3g" % (rng, d))
        assert d <= rng * 2.0 ** -10, (f, d, rng)
