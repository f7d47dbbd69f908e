"""tests/add_bounds.py on the CPU: an fp32 emulation of the add kernels (fp32 sum in input order,
one rounding to bf16) stays inside the derived bound on every case of the GPU kernel test, and
each planted defect -- an input dropped at one element, the relu skipped at one negative element,
one element of the last partial run left unwritten -- leaves it."""
import pytest
import torch

import add_bounds as A

PREFILL = 1000.0  # what an unwritten output element holds


def _f64(t):
    return t.to(torch.float64)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("N", A.NS)
@pytest.mark.parametrize("name", list(A.CASES))
def test_fp32_emulation_stays_inside_the_bound(name, N, relu):
    xs = A.inputs(name)[0][:N]
    ref, bound = A.case_ref(name, N, relu)
    y = A.emulate(xs, relu)
    A.assert_within(y, ref, bound, "%s N=%d relu=%d" % (name, N, relu), axes="i")
    if N == 2:  # the planted cancellations: exactly 0
        assert (y[::5] == 0).all()
    if relu:
        assert (y >= 0).all()
        assert (bound == 0).any(), "no element is pinned to exactly 0"


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("N", A.NS)
def test_a_dropped_input_leaves_the_bound(N, relu):
    name = "n6272"
    xs = A.inputs(name)[0][:N]
    ref, bound = A.case_ref(name, N, relu)
    k = N - 1
    # the element where the last input weighs most against the bound, among those the relu keeps
    live = ref > bound
    score = torch.where(live, _f64(xs[k]).abs() / bound, torch.zeros_like(bound))
    i = int(score.argmax())
    assert score[i] > 4
    broken = [x.clone() for x in xs]
    broken[k][i] = 0.0
    y = A.emulate(broken, relu)
    n, worst, bad = A.violations(y, ref, bound)
    assert n == 1 and bad.tolist() == [i] and worst > 4, (n, worst, bad)


@pytest.mark.parametrize("N", A.NS)
def test_a_skipped_relu_leaves_the_bound(N):
    name = "n225"
    xs = A.inputs(name)[0][:N]
    ref, bound = A.case_ref(name, N, 1)
    plain = A.emulate(xs, 0)
    i = int(_f64(plain).argmin())
    assert plain[i] < 0 and bound[i] == 0
    y = A.emulate(xs, 1)
    y[i] = plain[i]
    n, worst, bad = A.violations(y, ref, bound)
    assert n == 1 and bad.tolist() == [i] and worst == float("inf")


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("name", ["n225", "n10"])
def test_an_unwritten_tail_element_leaves_the_bound(name, relu):
    xs = A.inputs(name)[0][:2]
    ref, bound = A.case_ref(name, 2, relu)
    n_el = A.numel(name)
    assert n_el % 8  # the last run is partial
    y = A.emulate(xs, relu)
    y[n_el - 1] = PREFILL
    n, worst, bad = A.violations(y, ref, bound)
    assert n == 1 and bad.tolist() == [n_el - 1] and worst > 4


def test_the_bound_is_the_stated_formula():
    xs = [torch.tensor([1.5, -2.0, 256.0]).to(torch.bfloat16), torch.tensor([0.25, 0.5, 2.0 ** -8]).to(torch.bfloat16),
          torch.tensor([-0.75, 1.0, 0.0]).to(torch.bfloat16)]
    ref, bound = A.add_ref(xs, False)
    assert ref.tolist() == [1.0, -0.5, 256.0 + 2.0 ** -8]
    g = 5 * 2.0 ** -23
    for i, a in enumerate([2.5, 3.5, 256.0 + 2.0 ** -8]):
        assert abs(bound[i].item() - (2.0 ** -8 * (abs(ref[i].item()) + g * a) + g * a)) < 1e-18
    ref_r, bound_r = A.add_ref(xs, True)
    assert ref_r.tolist() == [1.0, 0.0, 256.0 + 2.0 ** -8]
    assert bound_r[1] == 0 and torch.equal(bound_r[[0, 2]], bound[[0, 2]])
