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


_LO32 = 0xFFFFFFFF


def _mul_hi_lo(m: int, c: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """High and low 32 bits of ``m * c`` (both below 2^32) without leaving
    the non-negative int64 range: ``c`` is split into 16-bit halves."""
    a = (c & 0xFFFF) * m  # < 2^48
    b = (c >> 16) * m  # < 2^48
    mid = b + (a >> 16)  # product = mid * 2^16 + (a & 0xFFFF)
    return mid >> 16, ((mid & 0xFFFF) << 16) | (a & 0xFFFF)


def philox4x32_10_words(c0, c1, c2, c3, k0: int, k1: int) -> list[torch.Tensor]:
    """Philox4x32-10 on int64 tensors holding 32-bit counter words and an
    integer key; the four output words as int64 tensors in [0, 2^32)."""
    for _ in range(10):
        hi0, lo0 = _mul_hi_lo(0xD2511F53, c0)
        hi1, lo1 = _mul_hi_lo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + 0x9E3779B9) & _LO32
        k1 = (k1 + 0xBB67AE85) & _LO32
    return [c0, c1, c2, c3]


def _mlm_mask_draws(
    input_ids, special, sample_index, count_table, seed, epoch, max_pred
):
    """What the mask functions share up to the selection: ``(ids,
    token_type, attention_mask, cand, n, j, w0, w1, w2, w3)``."""
    bsz, seq = input_ids.shape
    dev = input_ids.device
    ids = input_ids.long()
    sp = special.long()
    j = torch.arange(seq, device=dev).unsqueeze(0)  # [1, S]
    s0, s1, s2 = (sp[:, k : k + 1] for k in range(3))  # [B, 1]
    last = s2.clamp(0, seq - 1)
    attention_mask = (j <= last).long()
    token_type = ((j > s1) & (j <= s2)).long()
    cand = (j < last) & (j != s0) & (j != s1) & (j != s2)
    n_cand = cand.sum(1)
    n = torch.minimum(
        count_table.long()[n_cand].clamp(0, max_pred), n_cand
    ).unsqueeze(1)

    seed &= 0xFFFFFFFFFFFFFFFF
    index = sample_index.long().unsqueeze(1)  # two's complement of the u64
    c2 = (index & _LO32).expand(bsz, seq)
    c3 = (((index >> 32) & 0x7FFFFFFF) | 0x80000000).expand(bsz, seq)
    c0 = j.expand(bsz, seq)
    c1 = torch.full_like(c0, epoch & _LO32)
    w0, w1, w2, w3 = philox4x32_10_words(
        c0, c1, c2, c3, seed & _LO32, seed >> 32
    )
    return ids, token_type, attention_mask, cand, n, j, w0, w1, w2, w3


def _mlm_mask_outputs(
    ids, token_type, attention_mask, selected, w1, w2, max_pred, vocab_size,
    mask_token, t_keep, t_rand,
):
    """Token substitution at the selected positions and the padded gather."""
    bsz, seq = ids.shape
    dev = ids.device
    random_ids = (w2 * (vocab_size - 1)) >> 32
    new_ids = torch.where(
        w1 < t_keep,
        ids,
        torch.where(
            w1 < t_keep + t_rand, random_ids, torch.full_like(ids, mask_token)
        ),
    )
    masked_ids = torch.where(selected, new_ids, ids)
    labels = torch.where(selected, ids, torch.full_like(ids, -1))

    # the padded gather of BertForPreTraining.forward
    cap = bsz * max_pred
    flat = selected.reshape(-1)
    slots = torch.cumsum(flat.long(), 0) - 1
    slots = torch.where(flat, slots.clamp(max=cap), torch.full_like(slots, cap))
    positions = torch.zeros(cap + 1, dtype=torch.long, device=dev)
    positions.scatter_(0, slots, torch.arange(bsz * seq, device=dev))
    gathered = torch.full((cap + 1,), -1, dtype=torch.long, device=dev)
    gathered.scatter_(0, slots, labels.reshape(-1))
    return (
        masked_ids, token_type, attention_mask, positions[:cap],
        gathered[:cap], labels,
    )


def mlm_mask(
    input_ids: torch.Tensor,
    special: torch.Tensor,
    sample_index: torch.Tensor,
    count_table: torch.Tensor,
    seed: int,
    epoch: int,
    max_pred: int,
    vocab_size: int,
    mask_token: int,
    t_keep: int,
    t_rand: int,
) -> tuple[torch.Tensor, ...]:
    """Dynamic MLM masking of raw shard rows (csrc/ops/mlm_mask.hip in
    torch integer arithmetic). input_ids [B,S], special [B,3],
    sample_index [B], count_table [S+1] ->
    (masked_ids, token_type_ids, attention_mask, positions,
    gathered_labels, dense_labels), all int64."""
    ids, token_type, attention_mask, cand, n, j, w0, w1, w2, _ = (
        _mlm_mask_draws(
            input_ids, special, sample_index, count_table, seed, epoch,
            max_pred,
        )
    )
    seq = ids.shape[1]
    # (w0 << 32 | j) orders like w0 * S + j; non-candidates sort last
    key = torch.where(cand, w0 * seq + j, torch.full_like(w0, 1 << 62))
    rank = torch.argsort(torch.argsort(key, dim=1), dim=1)
    selected = cand & (rank < n)
    return _mlm_mask_outputs(
        ids, token_type, attention_mask, selected, w1, w2, max_pred,
        vocab_size, mask_token, t_keep, t_rand,
    )


def mlm_mask_whole_word(
    input_ids: torch.Tensor,
    special: torch.Tensor,
    sample_index: torch.Tensor,
    count_table: torch.Tensor,
    word_continues: torch.Tensor,
    seed: int,
    epoch: int,
    max_pred: int,
    vocab_size: int,
    mask_token: int,
    t_keep: int,
    t_rand: int,
) -> tuple[torch.Tensor, ...]:
    """``mlm_mask`` with whole-word masking (the two whole-word kernels of
    csrc/ops/mlm_mask.hip in torch integer arithmetic). word_continues
    uint8 [vocab_size] is 1 where a vocabulary entry continues a word."""
    ids, token_type, attention_mask, cand, n, j, w0, w1, w2, _ = (
        _mlm_mask_draws(
            input_ids, special, sample_index, count_table, seed, epoch,
            max_pred,
        )
    )
    bsz = ids.shape[0]
    n = n.squeeze(1)
    start, head, length, order = _mlm_mask_words(
        ids, cand, j, w0, word_continues, vocab_size
    )

    # the greedy fill, a rank at a time
    length_by_rank = length.gather(1, order)
    start_by_rank = start.gather(1, order)
    taken = torch.zeros_like(start)
    m = torch.zeros_like(n)
    for r in range(int(start.sum(1).max()) if bsz else 0):
        fits = start_by_rank[:, r] & (m < n) & (m + length_by_rank[:, r] <= n)
        m = m + torch.where(fits, length_by_rank[:, r], torch.zeros_like(m))
        taken[:, r] = fits
        if bool((m >= n).all()):
            break
    word_selected = torch.zeros_like(start).scatter_(1, order, taken)
    selected = cand & word_selected.gather(1, head)
    return _mlm_mask_outputs(
        ids, token_type, attention_mask, selected, w1, w2, max_pred,
        vocab_size, mask_token, t_keep, t_rand,
    )


def _mlm_mask_words(ids, cand, j, w0, word_continues, vocab_size):
    """The words of every row: ``start`` [B,S] (a candidate that starts a
    word), ``head`` [B,S] (of a candidate: the start of its word),
    ``length`` [B,S] (at a start: the word's positions) and ``order`` [B,S]
    (positions by ascending ``(w0 << 32) | first``, the starts first)."""
    seq = ids.shape[1]
    # a candidate starts a word unless its id continues a candidate
    in_vocab = (ids >= 0) & (ids < vocab_size)
    continues = word_continues.long()[ids.clamp(0, vocab_size - 1)] == 1
    prev_cand = torch.cat(
        [torch.zeros_like(cand[:, :1]), cand[:, :-1]], dim=1
    )
    start = cand & ~(in_vocab & continues & prev_cand)
    head = torch.cummax(
        torch.where(start, j, torch.full_like(j, -1)), dim=1
    ).values.clamp(min=0)  # of a candidate: the start of its word
    length = torch.zeros_like(ids).scatter_add_(1, head, cand.long())

    key = torch.where(start, w0 * seq + j, torch.full_like(w0, 1 << 62))
    return start, head, length, torch.argsort(key, dim=1)


def mlm_mask_span(
    input_ids: torch.Tensor,
    special: torch.Tensor,
    sample_index: torch.Tensor,
    count_table: torch.Tensor,
    word_continues: torch.Tensor,
    span_table: torch.Tensor,
    seed: int,
    epoch: int,
    max_pred: int,
    vocab_size: int,
    mask_token: int,
    t_keep: int,
    t_rand: int,
) -> tuple[torch.Tensor, ...]:
    """``mlm_mask`` with span masking (the span instantiation of
    csrc/ops/mlm_mask.hip in torch integer arithmetic). span_table int64
    [Lmax] is ``ops.mlm_span_table``: a word that is taken grows over the
    words that follow it, and the span shares the anchor's decision."""
    ids, token_type, attention_mask, cand, n, j, w0, w1, w2, w3 = (
        _mlm_mask_draws(
            input_ids, special, sample_index, count_table, seed, epoch,
            max_pred,
        )
    )
    bsz, seq = ids.shape
    n = n.squeeze(1)
    start, head, length, order = _mlm_mask_words(
        ids, cand, j, w0, word_continues, vocab_size
    )
    lmax = span_table.numel()
    # words of the span a start anchors, from its own w3
    span_len = 1 + (
        w3.unsqueeze(-1) >= span_table.long()[: lmax - 1]
    ).sum(-1)

    # anchor_of[b, first]: 1 + the anchor's position of the span that holds
    # the word at `first`, 0 while the word is free
    anchor_of = torch.zeros_like(ids)
    zero = torch.zeros_like(n)
    rows = torch.arange(bsz, device=ids.device)
    m = torch.zeros_like(n)
    for r in range(int(start.sum(1).max()) if bsz else 0):
        anchor = order[:, r]
        x_len = length[rows, anchor]
        grow = (
            start[rows, anchor] & (anchor_of[rows, anchor] == 0)
            & (m < n) & (m + x_len <= n)
        )
        mark = anchor + 1
        anchor_of[rows, anchor] = torch.where(
            grow, mark, anchor_of[rows, anchor]
        )
        want = span_len[rows, anchor]
        x, t = anchor, torch.where(grow, x_len, zero)
        for step in range(1, lmax):
            y = x + x_len  # the next break; a start when a word follows
            y_in = y.clamp(max=seq - 1)
            y_len = length[rows, y_in]
            grow = (
                grow & (step < want) & (y < seq) & start[rows, y_in]
                & (anchor_of[rows, y_in] == 0) & (m + t + y_len <= n)
            )
            if not bool(grow.any()):
                break
            anchor_of[rows, y_in] = torch.where(
                grow, mark, anchor_of[rows, y_in]
            )
            t = t + torch.where(grow, y_len, zero)
            x = torch.where(grow, y_in, x)
            x_len = torch.where(grow, y_len, x_len)
        m = m + t
        if bool((m >= n).all()):
            break
    mark = anchor_of.gather(1, head)
    selected = cand & (mark != 0)
    span_w1 = w1.gather(1, (mark - 1).clamp(min=0))
    return _mlm_mask_outputs(
        ids, token_type, attention_mask, selected, span_w1, w2, max_pred,
        vocab_size, mask_token, t_keep, t_rand,
    )


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
