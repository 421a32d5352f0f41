"""K-FAC Kronecker-factor update: ``factor = beta*factor + alpha*C``.

``C`` is the covariance of ``[x, 1]`` (``has_bias``) or of ``x``:
``C[:K,:K] = x^T x``, ``C[K,:K] = C[:K,K] = column sums``, ``C[K,K] = N``.
On 16-bit GPU activations this runs the symmetric split-K MFMA kernel
(csrc/ops/kfac_factor.hip): upper-triangular tiles only, no fp32 copy of
``x``, no ones column, the running average folded into the combine pass,
and an exactly symmetric result. Shapes the kernel does not take (K not
a multiple of 128, fewer than 256 rows, fp32 activations) and CPU
tensors run the eager composite ``_reference.kfac_factor_update``.

``coef``, when given, is a 2-element fp32 tensor ``{beta, alpha}`` on
``x``'s device and replaces the two floats, so values that live on the
device (a loss scale, an overflow check) need no host sync. A zero
``alpha`` gates the update off: the factor is left bit-identical even
when ``x`` holds Inf or NaN.

Reference op being replaced: the factor accumulation inside the
reference's external kfac_pytorch preconditioner
(run_pretraining.py:321-355).
"""

from __future__ import annotations

from typing import Optional

import torch

from . import _reference, extension, use_native

_coef_cache: dict = {}


def device_coef(beta: float, alpha: float, device: torch.device) -> torch.Tensor:
    """{beta, alpha} as a read-only fp32 tensor on ``device``, uploaded
    once per distinct pair (callers must not write to it)."""
    key = (float(beta), float(alpha), device)
    coef = _coef_cache.get(key)
    if coef is None:
        if len(_coef_cache) >= 256:
            _coef_cache.clear()
        coef = torch.tensor([beta, alpha], dtype=torch.float32, device=device)
        _coef_cache[key] = coef
    return coef


def factor_update(
    x2d: torch.Tensor,
    factor: torch.Tensor,
    beta: Optional[float],
    alpha: Optional[float],
    has_bias: bool,
    coef: Optional[torch.Tensor] = None,
    native: Optional[bool] = None,
) -> bool:
    """Update ``factor`` [D, D] fp32 (D = K + has_bias) in place from
    ``x2d`` [N, K]. ``native``: None = HIP kernel where it applies,
    False = always the eager composite. Returns True when the HIP kernel
    ran."""
    if coef is None and (beta is None or alpha is None):
        raise ValueError("factor_update needs beta and alpha, or coef")
    if (
        native is not False
        and use_native(x2d)
        and x2d.dtype in (torch.bfloat16, torch.float16)
        and extension().kfac_factor_supported(x2d.shape[0], x2d.shape[1])
    ):
        if coef is None:
            coef = device_coef(beta, alpha, x2d.device)
        extension().kfac_factor_update(x2d.contiguous(), factor, coef, has_bias)
        return True
    # forward hooks run inside the model's autocast region, where a bare
    # fp32 matmul would be cast down to 16 bits
    with torch.autocast(x2d.device.type, enabled=False):
        _reference.kfac_factor_update(x2d, factor, beta, alpha, has_bias, coef)
    return False
