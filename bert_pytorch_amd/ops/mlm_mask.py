"""Dynamic MLM masking as a pure function of (seed, epoch, sample, position).

``mlm_mask`` turns raw shard rows (``input_ids`` and the special-token
positions) into the model's inputs and the padded-gather MLM positions in
one HIP launch (csrc/ops/mlm_mask.hip). For each row:

* ``last = clamp(special[2], 0, S-1)``; ``attention_mask[j] = j <= last``;
  ``token_type[j] = special[1] < j <= special[2]``;
* candidates are the positions below ``last`` that no special names, and
  ``n = count_table[#candidates]`` of them are masked;
* candidate ``j`` draws ``philox4x32_10(counter = (j, epoch, lo32(index),
  hi32(index) & 0x7FFFFFFF | 0x80000000), key = seed)``; the ``n``
  smallest ``(w0 << 32) | j`` are selected;
* a selected token keeps its id when ``w1 < t_keep``, becomes
  ``(w2 * (vocab_size - 1)) >> 32`` when ``w1 < t_keep + t_rand`` and
  ``mask_token`` otherwise; its label is the original id.

With a ``word_continues`` table the selection is by whole words (two
launches): candidate ``j`` starts a word unless ``word_continues[id[j]]``
is 1 and ``j - 1`` is a candidate; the words are visited in ascending
``(w0 << 32) | first`` of their first position and one is selected, all
of it, when it still fits into ``n``, until ``n`` is reached
(docs/KERNELS.md has the full definition).

With a ``span_table`` as well (``mlm_span_table``) the selection is by
spans of whole words: a word that is taken grows over the words that
follow it, up to a length drawn from ``w3`` of its first position, while
they are free, adjacent and fit into ``n``; one keep / random / mask
decision, the anchor's, holds for the whole span.

Nothing depends on the batch a sample sits in, on the worker that read
it or on the world size, and nothing is read back to the host. No
autograd: every tensor is an integer.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _reference, extension, use_native


def mlm_thresholds(
    original_token_prob: float, random_token_prob: float
) -> Tuple[int, int]:
    """``(t_keep, t_rand)``: the two probabilities in units of 2^-32,
    rounded down."""
    if not (
        0 <= original_token_prob
        and 0 <= random_token_prob
        and original_token_prob + random_token_prob <= 1
    ):
        raise ValueError(
            "original_token_prob and random_token_prob must be >= 0 and sum "
            f"to at most 1, got {original_token_prob}, {random_token_prob}"
        )
    return (
        int(original_token_prob * (1 << 32)),
        int(random_token_prob * (1 << 32)),
    )


def mlm_count_table(
    seq_len: int, masked_lm_prob: float, max_pred: int
) -> torch.Tensor:
    """int32 [seq_len + 1]: masked tokens of a row with ``c`` candidates,
    ``min(max_pred, max(1, int(c * masked_lm_prob)))`` (0 for ``c == 0``),
    in Python's own arithmetic."""
    return torch.tensor(
        [
            0 if c == 0 else min(max_pred, max(1, int(c * masked_lm_prob)))
            for c in range(seq_len + 1)
        ],
        dtype=torch.int32,
    )


def mlm_span_table(p: float, max_len: int) -> torch.Tensor:
    """int64 [max_len]: the clipped geometric law of the span length in
    units of 2^-32, ``int(F(k) * 2**32)`` for ``k = 1..max_len`` with
    ``F(k) = (1 - (1-p)**k) / (1 - (1-p)**max_len)`` (SpanBERT's law,
    renormalised after clipping), the last entry forced to ``2**32``, in
    Python's own arithmetic. A word draws ``L = 1 + #{k < max_len : w3 >=
    table[k-1]}``."""
    if not (0 < p <= 1):
        raise ValueError(f"span geometric p must be in (0, 1], got {p}")
    if not (1 <= max_len <= 32):
        raise ValueError(f"span max length must be in [1, 32], got {max_len}")
    norm = 1 - (1 - p) ** max_len
    table = [
        int((1 - (1 - p) ** k) / norm * (1 << 32))
        for k in range(1, max_len + 1)
    ]
    table[-1] = 1 << 32
    return torch.tensor(table, dtype=torch.int64)


def _signed64(value: int) -> int:
    value &= 0xFFFFFFFFFFFFFFFF
    return value - (1 << 64) if value >= 1 << 63 else value


def mlm_mask(
    input_ids: torch.Tensor,
    special: torch.Tensor,
    sample_index: torch.Tensor,
    count_table: torch.Tensor,
    *,
    seed: int,
    epoch: int,
    max_pred: int,
    vocab_size: int,
    mask_token: int,
    t_keep: int,
    t_rand: int,
    dense_labels: bool = False,
    word_continues: Optional[torch.Tensor] = None,
    span_table: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
           torch.Tensor, Optional[torch.Tensor]]:
    """input_ids int32 [B,S], special int32 [B,3] (or [B,2]: the last
    entry is repeated), sample_index int64 [B], count_table int32 [S+1]
    (``mlm_count_table``) -> ``(masked_ids, token_type_ids,
    attention_mask, positions, gathered_labels, labels)``.

    The first three are int64 [B,S]. ``positions`` / ``gathered_labels``
    are int64 [B*max_pred] in the layout of ``BertForPreTraining``'s
    padded gather: the masked tokens in ascending flat index, then
    position 0 with label -1. ``labels`` is the dense int64 [B,S] label
    tensor (-1 where unmasked) when ``dense_labels`` is set, else None.

    ``word_continues`` (uint8 [vocab_size], 1 where a vocabulary entry
    continues a word; ``data.tokenization.word_continuation_table``)
    switches to whole-word masking, see above. ``span_table`` (int64
    [Lmax], ``mlm_span_table``) on top of it switches to span masking.
    """
    if span_table is not None and word_continues is None:
        raise ValueError(
            "span_table needs word_continues: spans are made of whole words "
            "(an all-zero table gives token spans)"
        )
    if input_ids.dim() != 2:
        raise ValueError("input_ids must be [B, S]")
    if special.dim() != 2 or special.shape[1] not in (2, 3):
        raise ValueError("special must be [B, 2] or [B, 3]")
    if special.shape[1] == 2:
        special = torch.cat([special, special[:, 1:]], dim=1)
    if use_native(input_ids):
        # spelled out per entry point: on the hot path a call costs less than building
        # and unpacking argument tuples
        if word_continues is None:
            out = extension().mlm_mask(
                input_ids, special.contiguous(), sample_index, count_table,
                _signed64(seed), epoch & 0xFFFFFFFF, max_pred, vocab_size,
                mask_token, t_keep, t_rand, dense_labels,
            )
        elif span_table is None:
            out = extension().mlm_mask_whole_word(
                input_ids, special.contiguous(), sample_index, count_table,
                word_continues, _signed64(seed), epoch & 0xFFFFFFFF, max_pred,
                vocab_size, mask_token, t_keep, t_rand, dense_labels,
            )
        else:
            out = extension().mlm_mask_span(
                input_ids, special.contiguous(), sample_index, count_table,
                word_continues, span_table, _signed64(seed),
                epoch & 0xFFFFFFFF, max_pred, vocab_size, mask_token, t_keep,
                t_rand, dense_labels,
            )
    else:
        seq = input_ids.shape[1]
        if not (1 <= max_pred <= seq and count_table.numel() == seq + 1):
            raise ValueError(
                f"need 1 <= max_pred ({max_pred}) <= S ({seq}) and a count "
                f"table of S + 1 entries, got {count_table.numel()}"
            )
        head = (input_ids, special, sample_index, count_table)
        tail = (seed, epoch, max_pred, vocab_size, mask_token, t_keep, t_rand)
        if word_continues is None:
            out = _reference.mlm_mask(*head, *tail)
        else:
            if (
                word_continues.device != input_ids.device
                or word_continues.dtype != torch.uint8
                or word_continues.dim() != 1
                or word_continues.numel() != vocab_size
            ):
                raise ValueError(
                    f"word_continues must be uint8 [{vocab_size}] on the "
                    f"device of input_ids, got {word_continues.dtype} "
                    f"{tuple(word_continues.shape)} on {word_continues.device}"
                )
            if span_table is None:
                out = _reference.mlm_mask_whole_word(
                    *head, word_continues, *tail
                )
            else:
                if (
                    span_table.device != input_ids.device
                    or span_table.dtype != torch.int64
                    or span_table.dim() != 1
                    or not 1 <= span_table.numel() <= 32
                ):
                    raise ValueError(
                        "span_table must be int64 [Lmax], 1 <= Lmax <= 32, "
                        "on the device of input_ids, got "
                        f"{span_table.dtype} {tuple(span_table.shape)} on "
                        f"{span_table.device}"
                    )
                out = _reference.mlm_mask_span(
                    *head, word_continues, span_table, *tail
                )
    return (*out[:5], out[5] if dense_labels else None)
