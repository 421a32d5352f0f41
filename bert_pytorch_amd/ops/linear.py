"""Linear projection with HIP column-sum bias gradient (gfx950).

``fused_linear`` behaves like ``F.linear`` (the forward IS one
hipBLASLt GEMM with fused bias epilogue) but its backward computes the
bias gradient with the streaming two-stage ``col_sum`` HIP kernel
instead of ATen's generic reduce — the packed-QKV projection's bias
grad over [B*S, 3H] bf16 was one of the last eager reduce hotspots.

Autocast handling is explicit: the wrapper casts x/w to the autocast
dtype (tracked, so grads flow back through the casts to the fp32
masters exactly as torch autocast would) and runs the Function with
autocast disabled so backward dtypes match the saved tensors. The bias
goes in as it is and is cast inside the Function, whose backward makes
the same roundings a tracked cast would: the column sum is rounded to
the compute dtype and then widened to the bias's. That lets the fold add
it straight into ``bias.grad`` (ops/grad_accum.py).
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from . import extension, use_native
from .grad_accum import accum_target


class _FusedLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        x2 = x.reshape(-1, x.shape[-1])
        ctx.save_for_backward(x2, weight)
        ctx.weight, ctx.bias = weight, bias  # the caller's tensors
        ctx.x_shape = x.shape
        y = F.linear(x2, weight, bias.to(x2.dtype))
        return y.view(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        from .matmul import _wgrad  # noqa: PLC0415

        x2, weight = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        dx = dy2 @ weight
        dw = _wgrad(dy2, x2.contiguous(), ctx.weight)
        bias = ctx.bias
        acc = accum_target(bias, torch.float32, bias.shape)
        if acc is not None:
            # acc += fp32(round_to_compute_dtype(column sum))
            extension().col_sum(dy2, acc=acc, round_to=dy2.dtype)
            return dx.view(ctx.x_shape), dw, None
        db = extension().col_sum(dy2)
        return dx.view(ctx.x_shape), dw, db.to(dy2.dtype).to(bias.dtype)


def fused_linear(x: torch.Tensor, weight: torch.Tensor,
                 bias: torch.Tensor) -> torch.Tensor:
    if not use_native(x):
        return F.linear(x, weight, bias)
    if torch.is_autocast_enabled() and x.is_cuda:
        dt = torch.get_autocast_dtype("cuda")
        x, weight = x.to(dt), weight.to(dt)
    with torch.autocast("cuda", enabled=False):
        return _FusedLinear.apply(x, weight, bias)
