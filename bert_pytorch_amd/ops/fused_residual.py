"""Fused bias + dropout + residual-add + LayerNorm (HIP, gfx950).

One kernel for the residual junction the reference spells as four ops
(``BertSelfOutput``/``BertOutput``: dense-bias add, dropout, residual
add, LayerNorm — src/modeling.py:432-443, 468-479). The dropout mask is
stored (uint8) so backward is exact. Kernel source:
csrc/ops/fused_residual.hip.

A junction output has two consumers (the next linear and the next
residual input), whose gradients autograd would sum with a stand-alone
add in front of this op's backward. With ``fork=True`` the op hands out
two handles on one output instead; its backward then receives the two
gradients separately and the kernel sums them in fp32 as it loads them
(the ``dy2`` operand). ``BPA_JUNCTION_FORK=0`` (read per call) returns
the same tensor twice, i.e. the ordinary single-output path.
"""

from __future__ import annotations

import os
from typing import Optional, Tuple, Union

import torch

from . import _reference, extension, use_native
from .grad_accum import accum_target
from .rng import next_philox


class _FusedBiasDropoutResidualLN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, residual, weight, ln_bias, p, training, eps,
                fork):
        ext = extension()
        x2d = x.contiguous().view(-1, x.shape[-1])
        r2d = residual.contiguous().view(-1, x.shape[-1])
        seed, offset = next_philox(x2d.numel()) if (training and p > 0) else (0, 0)
        # z = dropout(x + bias) + residual (saved for LN backward)
        y, z, mask, mean, rstd = ext.bias_dropout_residual_ln_fwd(
            x2d, bias, r2d, weight, ln_bias, p if training else 0.0, eps, seed, offset
        )
        ctx.save_for_backward(z, mask, weight, mean, rstd)
        ctx.params = (bias, weight, ln_bias)  # the caller's tensors
        ctx.p = p if training else 0.0
        ctx.has_bias = bias is not None
        ctx.shape = x.shape
        y = y.view(x.shape)
        if not fork:
            return y
        # two tensor objects on one storage; either gradient may be absent
        ctx.set_materialize_grads(False)
        return y, y.detach()

    @staticmethod
    def backward(ctx, dy, dy_fork=None):
        ext = extension()
        z, mask, weight, mean, rstd = ctx.saved_tensors
        if dy is None:
            dy, dy_fork = dy_fork, None
        if dy is None:
            return (None,) * 9
        dy2d = dy.contiguous().view(-1, dy.shape[-1])
        if dy_fork is not None:
            dy_fork = dy_fork.contiguous().view(-1, dy.shape[-1])
        # bias, gamma and beta gradients are added into .grad by the fold
        # where the gate allows, and come back as None
        gbias, gw, gb = (accum_target(p, torch.float32, weight.shape)
                         for p in ctx.params)
        dx, dbias, dz, dw, db = ext.bias_dropout_residual_ln_bwd(
            dy2d, z, mask, weight, mean, rstd, ctx.p, ctx.has_bias, dy_fork,
            dgamma_acc=gw, dbeta_acc=gb, dbias_acc=gbias,
        )
        return (
            dx.view(ctx.shape),
            dbias if ctx.has_bias else None,
            dz.view(ctx.shape),
            dw,
            db,
            None,
            None,
            None,
            None,
        )


def fused_bias_dropout_residual_ln(
    x: torch.Tensor,
    bias: Optional[torch.Tensor],
    residual: torch.Tensor,
    weight: torch.Tensor,
    ln_bias: torch.Tensor,
    p: float,
    training: bool,
    eps: float = 1e-12,
    fork: bool = False,
) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """``fork=True`` returns the output as a pair of handles, one per
    consumer (module docstring); the eager path and
    ``BPA_JUNCTION_FORK=0`` return pairs without any fusion."""
    if use_native(x):
        if fork and os.environ.get("BPA_JUNCTION_FORK") != "0":
            return _FusedBiasDropoutResidualLN.apply(
                x, bias, residual, weight, ln_bias, p, training, eps, True
            )
        y = _FusedBiasDropoutResidualLN.apply(
            x, bias, residual, weight, ln_bias, p, training, eps, False
        )
        return (y, y) if fork else y
    y = _reference.bias_dropout_residual_ln(
        x, bias, residual, weight, ln_bias, p, training, eps
    )
    return (y, y.view_as(y)) if fork else y
