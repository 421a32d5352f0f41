"""Eager FusedLAMB / FusedAdam (the CPU path, the oracle the native
kernels are compared with elsewhere) against an independent fp64
reference, over the optimizer flags: grad_averaging, bias_correction,
max_grad_norm on/off with clipping active and inactive, a wd = 0 group,
use_nvlamb, an all-zero parameter, and Adam in AdamW and L2 mode. Tensor
sizes sit on the multi-tensor chunk edge (65536, 65537). Bound: the
suite's 1e-4 of max|p| after three steps."""

import pytest

import optim_ref


@pytest.mark.parametrize(
    "name,kwargs,grad_scale,zero_param", optim_ref.LAMB_CASES,
    ids=[c[0] for c in optim_ref.LAMB_CASES],
)
def test_eager_lamb_flags_vs_fp64(name, kwargs, grad_scale, zero_param):
    got, want = optim_ref.run_lamb_case(kwargs, grad_scale, zero_param, "cpu")
    ratio = optim_ref.worst_ratio(got, want)
    print(f"lamb {name}: error/bound = {ratio:.3g}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize(
    "name,kwargs", optim_ref.ADAM_CASES,
    ids=[c[0] for c in optim_ref.ADAM_CASES],
)
def test_eager_adam_flags_vs_fp64(name, kwargs):
    got, want = optim_ref.run_adam_case(kwargs, "cpu")
    ratio = optim_ref.worst_ratio(got, want)
    print(f"adam {name}: error/bound = {ratio:.3g}")
    assert ratio <= 1.0, ratio


def test_reference_distinguishes_the_flags():
    """The flag matrix is not vacuous: every LAMB case's reference result
    differs from the default case's by far more than the bound (so a
    kernel that ignored the flag would fail its case)."""
    base = optim_ref.run_lamb_case({}, 1.0, False, "cpu")[1]
    for name, kwargs, grad_scale, zero_param in optim_ref.LAMB_CASES[2:]:
        if grad_scale != 1.0 or zero_param:
            continue  # other inputs: differs trivially
        want = optim_ref.run_lamb_case(kwargs, grad_scale, zero_param, "cpu")[1]
        assert optim_ref.worst_ratio(want, base) > 10.0, name
