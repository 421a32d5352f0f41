"""Training masks made on the device (``--device_masking``).

``ShardedPretrainingDataset(device_masking=True)`` hands out raw rows;
``DeviceMasker`` holds the run constants and turns such a batch, once it
is on the training device, into the model's inputs with ``ops.mlm_mask``.
A sample's mask depends on ``(seed, epoch, global sample index)`` only:
not on the number of loader workers, the world size, the batch the sample
lands in, or whether the run was resumed.
"""

from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from .. import ops


class DeviceMasker:
    def __init__(
        self,
        seed: int,
        mask_token_index: int,
        max_pred_per_seq: int,
        masked_lm_prob: float,
        vocab_size: int,
        original_token_prob: float = 0.1,
        random_token_prob: float = 0.1,
        word_continues: Optional[torch.Tensor] = None,
        span_max_length: Optional[int] = None,
        span_geometric_p: float = 0.2,
    ):
        """``word_continues`` (uint8 [vocab_size],
        ``tokenization.word_continuation_table``) turns on whole-word
        masking; ``span_max_length`` on top of it turns on span masking
        (spans of whole words, ``ops.mlm_span_table(span_geometric_p,
        span_max_length)``)."""
        self.seed = int(seed)
        self.mask_token_index = int(mask_token_index)
        self.max_pred_per_seq = int(max_pred_per_seq)
        self.masked_lm_prob = masked_lm_prob
        self.vocab_size = int(vocab_size)
        self.t_keep, self.t_rand = ops.mlm_thresholds(
            original_token_prob, random_token_prob
        )
        self._tables: Dict[Tuple[int, torch.device], torch.Tensor] = {}
        if word_continues is not None:
            word_continues = torch.as_tensor(word_continues)
            if (
                word_continues.dtype != torch.uint8
                or word_continues.shape != (self.vocab_size,)
            ):
                raise ValueError(
                    f"word_continues must be uint8 [{self.vocab_size}], got "
                    f"{word_continues.dtype} {tuple(word_continues.shape)}"
                )
        self.word_continues = word_continues
        self._word_tables: Dict[torch.device, torch.Tensor] = {}
        self.span_table = None
        if span_max_length is not None:
            if word_continues is None:
                raise ValueError(
                    "span_max_length needs word_continues: spans are made "
                    "of whole words"
                )
            self.span_table = ops.mlm_span_table(
                span_geometric_p, span_max_length
            )
        self._span_tables: Dict[torch.device, torch.Tensor] = {}

    def word_table(self, device: torch.device) -> Optional[torch.Tensor]:
        """``word_continues`` on ``device``, uploaded once; None when
        masking is token-level."""
        if self.word_continues is None:
            return None
        if device not in self._word_tables:
            self._word_tables[device] = self.word_continues.to(device)
        return self._word_tables[device]

    def span_length_table(
        self, device: torch.device
    ) -> Optional[torch.Tensor]:
        """``ops.mlm_span_table`` on ``device``, uploaded once; None without
        span masking."""
        if self.span_table is None:
            return None
        if device not in self._span_tables:
            self._span_tables[device] = self.span_table.to(device)
        return self._span_tables[device]

    def count_table(self, seq_len: int, device: torch.device) -> torch.Tensor:
        """``ops.mlm_count_table`` for this sequence length, uploaded once."""
        key = (seq_len, device)
        if key not in self._tables:
            self._tables[key] = ops.mlm_count_table(
                seq_len, self.masked_lm_prob, self.max_pred_per_seq
            ).to(device)
        return self._tables[key]

    def __call__(self, batch: Sequence[torch.Tensor], epoch: int):
        """``[input_ids, special, nsp_labels, sample_index]`` (the dataset's
        device_masking batch) -> ``(input_ids, segment_ids, input_mask,
        positions, gathered_labels, nsp_labels)``."""
        input_ids, special, nsp_labels, sample_index = batch
        masked, segment_ids, input_mask, positions, gathered, _ = ops.mlm_mask(
            input_ids, special, sample_index,
            self.count_table(input_ids.shape[1], input_ids.device),
            seed=self.seed, epoch=epoch, max_pred=self.max_pred_per_seq,
            vocab_size=self.vocab_size, mask_token=self.mask_token_index,
            t_keep=self.t_keep, t_rand=self.t_rand,
            word_continues=self.word_table(input_ids.device),
            span_table=self.span_length_table(input_ids.device),
        )
        return masked, segment_ids, input_mask, positions, gathered, nsp_labels
