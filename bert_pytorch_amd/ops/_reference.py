"""Eager fp32 reference composites for every fused HIP op.

These are the single source of truth for the *math* of each fused kernel:
the CPU path runs them directly (differentiable via autograd), and the GPU
numerics tests compare each HIP kernel against them in fp32
(reference semantics: src/modeling.py:118-139 gelu/bias_gelu,
:282-335 LayerNorm, :376-429 attention, run_pretraining.py:58-72 loss).
"""

from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F


def gelu(x: torch.Tensor) -> torch.Tensor:
    """Exact (erf) GELU — the reference's gelu (src/modeling.py:118-120)."""
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def bias_gelu(x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    return gelu(x + bias)


def layer_norm(
    x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-12
) -> torch.Tensor:
    return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)


def bias_dropout_residual_ln(
    x: torch.Tensor,
    bias: Optional[torch.Tensor],
    residual: torch.Tensor,
    weight: torch.Tensor,
    ln_bias: torch.Tensor,
    p: float,
    training: bool,
    eps: float = 1e-12,
) -> torch.Tensor:
    """y = LN(dropout(x + bias) + residual)."""
    if bias is not None:
        x = x + bias
    x = F.dropout(x, p=p, training=training)
    return layer_norm(x + residual, weight, ln_bias, eps)


def embedding_ln_dropout(
    input_ids: torch.Tensor,
    token_type_ids: Optional[torch.Tensor],
    word_emb: torch.Tensor,
    pos_emb: torch.Tensor,
    tok_emb: Optional[torch.Tensor],
    weight: torch.Tensor,
    ln_bias: torch.Tensor,
    p: float,
    training: bool,
    eps: float = 1e-12,
) -> torch.Tensor:
    """y = dropout(LN(word[ids] + pos[0..S-1] + tok[type_ids]))."""
    seq_len = input_ids.shape[1]
    e = F.embedding(input_ids, word_emb) + pos_emb[:seq_len].unsqueeze(0)
    if tok_emb is not None and token_type_ids is not None:
        e = e + F.embedding(token_type_ids, tok_emb)
    e = layer_norm(e, weight, ln_bias, eps)
    return F.dropout(e, p=p, training=training)


def attention(
    qkv: torch.Tensor,
    seqlens: torch.Tensor,
    num_heads: int,
    p: float,
    training: bool,
) -> torch.Tensor:
    """Scaled-dot-product attention with a padding mask.

    qkv: [B, S, 3*H] packed (query | key | value, each H wide).
    seqlens: [B] int — number of valid (non-pad) tokens per sequence.
    Returns [B, S, H]. Padding keys are masked out; padded query rows
    produce (dropout of) uniform-attention values, matching the additive
    -10000 mask semantics of the reference (src/modeling.py:413-425,
    862-870) up to the softmax over all-masked rows.
    """
    bsz, seq, three_h = qkv.shape
    hidden = three_h // 3
    head_dim = hidden // num_heads
    q, k, v = qkv.split(hidden, dim=-1)

    def shape(t):  # [B, S, H] -> [B, nh, S, dh]
        return t.view(bsz, seq, num_heads, head_dim).transpose(1, 2)

    q, k, v = shape(q), shape(k), shape(v)
    scores = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(head_dim)
    key_pad = torch.arange(seq, device=qkv.device).unsqueeze(0) >= seqlens.unsqueeze(1)
    scores = scores.masked_fill(key_pad[:, None, None, :], -10000.0)
    probs = F.softmax(scores, dim=-1)
    probs = F.dropout(probs, p=p, training=training)
    ctx = torch.matmul(probs, v)  # [B, nh, S, dh]
    return ctx.transpose(1, 2).reshape(bsz, seq, hidden)


def attention_varlen(
    qkv: torch.Tensor,
    cu_seqlens: torch.Tensor,
    max_seqlen: int,
    num_heads: int,
    p: float,
    training: bool,
) -> torch.Tensor:
    """Attention over a packed batch.

    qkv: [T_pad, 3*H]; sequence b owns rows cu_seqlens[b]..cu_seqlens[b+1]-1
    (cu_seqlens: [B+1] int, exclusive prefix sum of the lengths, each at
    most ``max_seqlen``). Returns [T_pad, H]; rows past cu_seqlens[-1]
    belong to no sequence and come back as zeros. Each sequence attends
    to itself only, which is what ``attention`` computes for the valid
    rows of the padded layout. Eager composite: one ``attention`` call
    per sequence (the bounds are read on the host).
    """
    hidden = qkv.shape[-1] // 3
    out = qkv.new_zeros(qkv.shape[0], hidden)
    bounds = [int(v) for v in cu_seqlens.tolist()]
    for start, end in zip(bounds[:-1], bounds[1:]):
        n = end - start
        if n <= 0:
            continue
        assert n <= max_seqlen, f"sequence of {n} rows > max_seqlen {max_seqlen}"
        lens = torch.full((1,), n, dtype=torch.int32, device=qkv.device)
        out[start:end] = attention(
            qkv[start:end].unsqueeze(0), lens, num_heads, p, training
        )[0]
    return out


def pack_rows(x: torch.Tensor, dest: torch.Tensor, t_pad: int) -> torch.Tensor:
    """[N, H] -> [t_pad, H]: row i goes to row dest[i]; rows with
    dest[i] < 0 are dropped and rows no dest names are zero."""
    keep = dest >= 0
    out = x.new_zeros(t_pad, x.shape[-1])
    return out.index_copy(0, dest[keep].long(), x[keep])


def unpack_rows(y: torch.Tensor, dest: torch.Tensor, rows: int) -> torch.Tensor:
    """[t_pad, H] -> [rows, H]: inverse of ``pack_rows``; positions with
    dest[i] < 0 are zero."""
    keep = dest >= 0
    gathered = y.index_select(0, dest.clamp(min=0).long())
    return torch.where(keep.unsqueeze(-1), gathered, torch.zeros_like(gathered))


def kfac_factor_update(
    x2d: torch.Tensor,
    factor: torch.Tensor,
    beta: Optional[float],
    alpha: Optional[float],
    has_bias: bool,
    coef: Optional[torch.Tensor] = None,
) -> None:
    """factor <- beta*factor + alpha*[x,1]^T[x,1], in place, in fp32.

    ``coef`` ({beta, alpha} as a tensor) replaces the two floats; a zero
    ``coef[1]`` leaves ``factor`` untouched whatever ``x2d`` holds.
    """
    a = x2d.float()
    if has_bias:
        ones = torch.ones(a.shape[0], 1, dtype=a.dtype, device=a.device)
        a = torch.cat([a, ones], dim=1)
    cov = a.t() @ a
    if coef is None:
        factor.mul_(beta).add_(cov, alpha=alpha)
        return
    new = factor * coef[0] + cov * coef[1]
    factor.copy_(torch.where(coef[1] != 0, new, factor))


def cross_entropy(
    logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -1
) -> torch.Tensor:
    return F.cross_entropy(
        logits.float(), labels, ignore_index=ignore_index, reduction="mean"
    )


def mlm_eval(
    logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -1
) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(loss_sum, count, correct, pred) of [P, V] logits against labels.

    fp32 throughout; ``pred`` is int32 and, on a tie, the lowest column
    that attains the row maximum.
    """
    x = logits.float()
    valid = labels != ignore_index
    lse = torch.logsumexp(x, dim=1)
    picked = x.gather(1, labels.clamp(min=0).unsqueeze(1)).squeeze(1)
    loss_sum = torch.where(valid, lse - picked, torch.zeros_like(lse)).sum()
    pred = torch.argmax(x, dim=1)
    correct = ((pred == labels) & valid).sum()
    return loss_sum, valid.sum().float(), correct.float(), pred.to(torch.int32)
