"""Native (HIP multi-tensor) FusedLAMB / FusedAdam against the independent
fp64 reference of optim_ref.py, over the same flag matrix and chunk-edge
tensor sizes as the eager test in test_optim_flags.py. Bound: the suite's
1e-4 of max|p| after three steps; the kernel's fp32
``1 - powf(beta, step)`` costs about 1e-5 of it at step 1."""

import pytest
import torch

import optim_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize(
    "name,kwargs,grad_scale,zero_param", optim_ref.LAMB_CASES,
    ids=[c[0] for c in optim_ref.LAMB_CASES],
)
def test_native_lamb_flags_vs_fp64(name, kwargs, grad_scale, zero_param):
    got, want = optim_ref.run_lamb_case(kwargs, grad_scale, zero_param, DEV)
    ratio = optim_ref.worst_ratio(got, want)
    print(f"native lamb {name}: error/bound = {ratio:.3g}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize(
    "name,kwargs", optim_ref.ADAM_CASES,
    ids=[c[0] for c in optim_ref.ADAM_CASES],
)
def test_native_adam_flags_vs_fp64(name, kwargs):
    got, want = optim_ref.run_adam_case(kwargs, DEV)
    ratio = optim_ref.worst_ratio(got, want)
    print(f"native adam {name}: error/bound = {ratio:.3g}")
    assert ratio <= 1.0, ratio
