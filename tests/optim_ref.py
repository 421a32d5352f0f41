"""Independent fp64 LAMB and Adam, written from the semantics stated in
the optim/lamb.py and optim/adam.py docstrings (not from their code), and
the flag matrix both the eager (CPU) and the native (GPU) optimizer tests
run against it."""

from __future__ import annotations

import math

import torch

# 65536 is the multi-tensor chunk: 65536 fills one exactly, 65537 spills
# one element into a second, 200000 spans four
SIZES = (1, 7, 65536, 65537, 200000)
STEPS = 3
LR = 1e-2
BETAS = (0.9, 0.999)


def lamb_ref(params, grads_per_step, groups, *, eps=1e-6, bias_correction=True,
             grad_averaging=True, max_grad_norm=1.0, use_nvlamb=False):
    """params: list of fp64 tensors (updated in place); groups: list of
    (indices, weight_decay); grads_per_step: list of lists of fp64 grads."""
    b1, b2 = BETAS
    m = [torch.zeros_like(p) for p in params]
    v = [torch.zeros_like(p) for p in params]
    for step, grads in enumerate(grads_per_step, 1):
        gnorm = math.sqrt(sum(float((g * g).sum()) for g in grads))
        clip = max_grad_norm / gnorm if 0 < max_grad_norm < gnorm else 1.0
        c1 = 1 - b1 ** step if bias_correction else 1.0
        c2 = 1 - b2 ** step if bias_correction else 1.0
        for idx, wd in groups:
            for i in idx:
                g = grads[i] * clip
                m[i] = b1 * m[i] + ((1 - b1) if grad_averaging else 1.0) * g
                v[i] = b2 * v[i] + (1 - b2) * g * g
                u = (m[i] / c1) / ((v[i] / c2).sqrt() + eps) + wd * params[i]
                ratio = 1.0
                if wd != 0 or use_nvlamb:
                    wn, un = float(params[i].norm()), float(u.norm())
                    if wn > 0 and un > 0:
                        ratio = wn / un
                params[i] -= LR * ratio * u
    return params


def adam_ref(params, grads_per_step, *, wd, adam_w, eps=1e-8,
             bias_correction=True):
    b1, b2 = BETAS
    m = [torch.zeros_like(p) for p in params]
    v = [torch.zeros_like(p) for p in params]
    for step, grads in enumerate(grads_per_step, 1):
        c1 = 1 - b1 ** step if bias_correction else 1.0
        c2 = 1 - b2 ** step if bias_correction else 1.0
        for i, p in enumerate(params):
            g = grads[i] if adam_w else grads[i] + wd * p  # L2 decay
            m[i] = b1 * m[i] + (1 - b1) * g
            v[i] = b2 * v[i] + (1 - b2) * g * g
            u = (m[i] / c1) / ((v[i] / c2).sqrt() + eps)
            if adam_w:
                u = u + wd * p  # decoupled decay
            params[i] = p - LR * u
    return params


def make_problem(grad_scale, zero_param=False):
    """fp32 params and per-step grads of SIZES; grad_scale sets the global
    gradient norm (about grad_scale * sqrt(330k) = 575 * grad_scale)."""
    gen = torch.Generator().manual_seed(77)
    params = [torch.randn(n, generator=gen) for n in SIZES]
    if zero_param:
        params[1].zero_()  # ||w|| = 0: trust ratio must fall back to 1
    grads = [
        [torch.randn(n, generator=gen) * grad_scale for n in SIZES]
        for _ in range(STEPS)
    ]
    return params, grads


# LAMB cases: (name, optimizer kwargs, grad_scale, zero_param). Two groups
# always: tensors 0-2 with weight decay 0.01, tensors 3-4 with none (the
# wd = 0 group: trust ratio only under use_nvlamb).
# grad_scale 1.0 -> global norm ~575, clipped at max_grad_norm = 1;
# grad_scale 1e-3 -> ~0.575, below it, clipping inactive.
LAMB_CASES = [
    ("default_clip_active", {}, 1.0, False),
    ("clip_inactive", {}, 1e-3, False),
    ("no_clip", {"max_grad_norm": 0.0}, 1.0, False),
    ("no_grad_averaging", {"grad_averaging": False}, 1.0, False),
    ("no_bias_correction", {"bias_correction": False}, 1.0, False),
    ("neither", {"grad_averaging": False, "bias_correction": False,
                 "max_grad_norm": 0.0}, 1e-3, False),
    ("nvlamb", {"use_nvlamb": True}, 1.0, False),
    ("zero_param", {}, 1.0, True),
    ("zero_param_nvlamb", {"use_nvlamb": True}, 1e-3, True),
]
LAMB_GROUPS = [((0, 1, 2), 0.01), ((3, 4), 0.0)]

ADAM_CASES = [
    ("adamw", {"adam_w_mode": True, "weight_decay": 0.01}),
    ("adam_l2", {"adam_w_mode": False, "weight_decay": 0.01}),
    ("adamw_no_bc", {"adam_w_mode": True, "weight_decay": 0.01,
                     "bias_correction": False}),
    ("adam_l2_no_bc", {"adam_w_mode": False, "weight_decay": 0.01,
                       "bias_correction": False}),
    ("adam_no_decay", {"adam_w_mode": False, "weight_decay": 0.0}),
]


def run_lamb_case(kwargs, grad_scale, zero_param, device):
    """-> (params after STEPS of FusedLAMB on `device`, fp64 reference)."""
    from bert_pytorch_amd.optim import FusedLAMB

    p0, grads = make_problem(grad_scale, zero_param)
    params = [torch.nn.Parameter(p.clone().to(device)) for p in p0]
    opt = FusedLAMB(
        [{"params": [params[i] for i in idx], "weight_decay": wd}
         for idx, wd in LAMB_GROUPS],
        lr=LR, betas=BETAS, **kwargs,
    )
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = g.clone().to(device)
        opt.step()
    ref_kw = {k: v for k, v in kwargs.items()}
    want = lamb_ref([p.double() for p in p0],
                    [[g.double() for g in gs] for gs in grads],
                    LAMB_GROUPS, **ref_kw)
    return [p.detach().cpu() for p in params], want


def run_adam_case(kwargs, device):
    from bert_pytorch_amd.optim import FusedAdam

    p0, grads = make_problem(1.0)
    params = [torch.nn.Parameter(p.clone().to(device)) for p in p0]
    opt = FusedAdam(params, lr=LR, betas=BETAS, **kwargs)
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = g.clone().to(device)
        opt.step()
    want = adam_ref([p.double() for p in p0],
                    [[g.double() for g in gs] for gs in grads],
                    wd=kwargs["weight_decay"], adam_w=kwargs["adam_w_mode"],
                    bias_correction=kwargs.get("bias_correction", True))
    return [p.detach().cpu() for p in params], want


def worst_ratio(got, want, bound=1e-4):
    """max over tensors of max|got - want| / (bound * max|want|); the
    tests assert it is at most 1. An all-zero reference is floored at 1e-3
    like the suite's rel_err."""
    worst = 0.0
    for g, w in zip(got, want):
        denom = bound * max(float(w.abs().max()), 1e-3)
        worst = max(worst, float((g.double() - w).abs().max()) / denom)
    return worst
