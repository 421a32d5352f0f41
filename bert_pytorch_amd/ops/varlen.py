"""Padding-free (unpadded) encoder ops (HIP, gfx950).

A padded batch ``[B, S]`` spends every row-wise kernel and GEMM on its
padding. The unpadded mode packs the valid tokens of a batch into one
``[T_pad, H]`` matrix, runs the encoder on that, and runs attention over
a ``cu_seqlens`` index instead of a ``[B, S]`` grid:

* ``unpad_index`` turns an attention mask into the row map ``dest`` and
  the ``cu_seqlens`` prefix sum;
* ``pack_rows`` / ``unpack_rows`` move rows between the two layouts
  (csrc/ops/varlen.hip; each is the other's backward);
* ``fused_attention_varlen`` is ``fused_attention`` for the packed
  layout (the ``VARLEN`` instantiations in csrc/ops/attention.hip).

Packing follows the mask's actual positions, so a mask that is not a
prefix (left padding, holes) keeps the reference's meaning: the tokens
where the mask is 1 attend to each other, in order. The padded path
reduces the mask to a length and treats it as a prefix mask.
"""

from __future__ import annotations

from typing import Tuple

import torch

from . import _reference, extension, use_native
from .rng import next_philox

# T is rounded up to a multiple of this many rows: it keeps the split-K
# wgrad kernel's K % 4 == 0, keeps row-chunked kernels on whole chunks,
# and limits the number of distinct GEMM shapes a run sees.
ROW_ALIGN = 128


def unpad_index(
    attention_mask: torch.Tensor,
) -> Tuple[torch.Tensor, torch.Tensor, int, int]:
    """attention_mask [B, S] (non-zero = valid) ->
    ``(dest, cu_seqlens, T, T_pad)``.

    ``dest`` [B*S] int32 is the exclusive cumulative sum of the flattened
    mask where the mask is set and -1 elsewhere: the packed row of each
    valid token. ``cu_seqlens`` [B+1] int32 is the exclusive prefix sum
    of the per-sequence counts (``cu_seqlens[B] == T``). ``T`` is the
    number of valid tokens and ``T_pad`` is ``T`` rounded up to a
    multiple of 128 (``ROW_ALIGN``).

    This performs ONE device-to-host read, of ``T`` (the packed matrix
    has to be allocated with a host-known size). It is the only
    synchronisation the unpadded mode adds to a step.
    """
    if attention_mask.dim() != 2:
        raise ValueError("attention_mask must be [B, S]")
    valid = attention_mask != 0
    flat = valid.reshape(-1)
    incl = torch.cumsum(flat, 0, dtype=torch.int32)
    dest = torch.where(flat, incl - 1, torch.full_like(incl, -1))
    cu_seqlens = torch.zeros(
        valid.shape[0] + 1, dtype=torch.int32, device=valid.device
    )
    cu_seqlens[1:] = torch.cumsum(valid.sum(-1, dtype=torch.int32), 0)
    total = int(cu_seqlens[-1])  # the one device-to-host read
    t_pad = -(-total // ROW_ALIGN) * ROW_ALIGN
    return dest, cu_seqlens, total, t_pad


def _rows_native(x: torch.Tensor) -> bool:
    """The row-copy kernels move 16-byte chunks of bf16/fp16/fp32 rows."""
    return (
        use_native(x)
        and x.dtype in (torch.bfloat16, torch.float16, torch.float32)
        and (x.shape[-1] * x.element_size()) % 16 == 0
    )


class _PackRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dest, t_pad):
        ctx.save_for_backward(dest)
        ctx.rows = x.shape[0]
        return extension().pack_rows(x.contiguous(), dest, t_pad)

    @staticmethod
    def backward(ctx, dy):
        (dest,) = ctx.saved_tensors
        return extension().unpack_rows(dy.contiguous(), dest, ctx.rows), None, None


class _UnpackRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, dest, rows):
        ctx.save_for_backward(dest)
        ctx.t_pad = y.shape[0]
        return extension().unpack_rows(y.contiguous(), dest, rows)

    @staticmethod
    def backward(ctx, dx):
        (dest,) = ctx.saved_tensors
        return extension().pack_rows(dx.contiguous(), dest, ctx.t_pad), None, None


def pack_rows(x: torch.Tensor, dest: torch.Tensor, t_pad: int) -> torch.Tensor:
    """x [B*S, H] -> [t_pad, H]: row i to row ``dest[i]``; rows with
    ``dest[i] < 0`` are dropped; rows no ``dest`` names are zero."""
    if _rows_native(x):
        return _PackRows.apply(x, dest, t_pad)
    return _reference.pack_rows(x, dest, t_pad)


def unpack_rows(y: torch.Tensor, dest: torch.Tensor, rows: int) -> torch.Tensor:
    """y [t_pad, H] -> [rows, H]: the inverse of ``pack_rows``;
    positions with ``dest[i] < 0`` are zero."""
    if _rows_native(y):
        return _UnpackRows.apply(y, dest, rows)
    return _reference.unpack_rows(y, dest, rows)


class _FusedAttentionVarlen(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cu_seqlens, max_seqlen, num_heads, p, training):
        ext = extension()
        qkv = qkv.contiguous()
        bsz = cu_seqlens.shape[0] - 1
        p_eff = p if training else 0.0
        # the keep-mask has the padded kernel's [B*NH, S, S] bit layout
        # with S = max_seqlen, so it advances the Philox stream alike
        seed, offset = (
            next_philox(bsz * num_heads * max_seqlen * max_seqlen)
            if p_eff > 0
            else (0, 0)
        )
        out, lse, dmask = ext.attention_varlen_fwd(
            qkv, cu_seqlens, max_seqlen, num_heads, p_eff, seed, offset
        )
        ctx.save_for_backward(qkv, cu_seqlens, out, lse, dmask)
        ctx.meta = (max_seqlen, num_heads, p_eff, seed, offset)
        return out

    @staticmethod
    def backward(ctx, dout):
        ext = extension()
        qkv, cu_seqlens, out, lse, dmask = ctx.saved_tensors
        max_seqlen, num_heads, p_eff, seed, offset = ctx.meta
        dqkv = ext.attention_varlen_bwd(
            dout.contiguous(), qkv, cu_seqlens, max_seqlen, out, lse, dmask,
            num_heads, p_eff, seed, offset,
        )
        return dqkv, None, None, None, None, None


def _varlen_kernel_supported(qkv: torch.Tensor, num_heads: int) -> bool:
    """``attention._kernel_supported`` without the S % 16 clause: the
    packed kernels guard every row by its sequence's own length, so
    lengths need no alignment."""
    head_dim = qkv.shape[-1] // 3 // num_heads
    return qkv.dtype in (torch.bfloat16, torch.float16) and head_dim == 64


def fused_attention_varlen(
    qkv: torch.Tensor,
    cu_seqlens: torch.Tensor,
    max_seqlen: int,
    num_heads: int,
    p: float,
    training: bool,
) -> torch.Tensor:
    """qkv [T_pad, 3H] packed, cu_seqlens [B+1] int32 -> context
    [T_pad, H]; rows past ``cu_seqlens[-1]`` are zero."""
    if use_native(qkv) and _varlen_kernel_supported(qkv, num_heads):
        return _FusedAttentionVarlen.apply(
            qkv, cu_seqlens, max_seqlen, num_heads, p, training
        )
    return _reference.attention_varlen(
        qkv, cu_seqlens, max_seqlen, num_heads, p, training
    )
