"""Sharded pretraining dataset + chunked checkpointable DistributedSampler.

Re-designed from the reference's ``ShardedPretrainingDataset``
(src/dataset.py:9-338) and chunked ``DistributedSampler``
(src/dataset.py:341-428) with the same external behavior:

* multi-file HDF5 shards, at most 2 resident in RAM, the next shard
  prefetched by a background thread while the current one is consumed
  sequentially;
* RoBERTa-style dynamic masking (80/10/10) computed on CPU workers from
  the new {input_ids, special_token_positions, next_sentence_labels}
  schema, plus the legacy NVIDIA pre-masked schema; ``static_masking``
  instead draws the mask of sample ``idx`` from a generator seeded by
  ``(seed, idx)``, so a held-out set is the same tensors at every
  evaluation, in every run, at any worker count; ``device_masking``
  masks nothing here and hands out the raw row, its special positions
  and its global index for ``DeviceMasker`` (masking.py);
  ``whole_word_masking`` makes the dynamic masks of whole words (the word
  rule and greedy fill of ``ops.mlm_mask``, drawn from this dataset's
  generator); ``span_masking`` makes them of spans of whole words (the
  span fill of ``ops.mlm_mask(..., span_table=)``, lengths and order from
  this dataset's generator, one keep / random / mask decision per span);
  static masks stay token-level;
* a rank-chunked sequential sampler whose position checkpoints into the
  training state dict.

Deliberate fixes over the reference: in-file index uses
``idx - file_sample_start_idx`` (not the accidental negative-index
trick), masked rows are copied before mutation (the reference mutates
the cached shard in place), and mask positions are sampled WITHOUT
replacement so exactly ``mask_count`` distinct tokens are masked.
"""

from __future__ import annotations

import math
import os
import threading
import warnings
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.utils.data

from .h5lite import H5LiteFile


class ShardedPretrainingDataset(torch.utils.data.Dataset):
    def __init__(
        self,
        files: Sequence[str] | str,
        mask_token_index: int,
        max_pred_per_seq: int,
        masked_lm_prob: float,
        vocab_size: int,
        original_token_prob: float = 0.1,
        random_token_prob: float = 0.1,
        shuffle: bool = False,
        seed: Optional[int] = None,
        static_masking: bool = False,
        device_masking: bool = False,
        whole_word_masking: bool = False,
        word_continues=None,
        span_masking: bool = False,
        span_max_length: int = 10,
        span_geometric_p: float = 0.2,
    ):
        if original_token_prob + random_token_prob > 1:
            raise ValueError("original_token_prob + random_token_prob > 1")
        # static (evaluation) masks stay token-level and device_masking
        # masks nothing here: words and spans are a matter of the dynamic path
        span_masking = span_masking and not (device_masking or static_masking)
        whole_word_masking = (
            whole_word_masking and not (device_masking or static_masking)
        ) or span_masking
        if span_masking:
            if not 0 < span_geometric_p <= 1:
                raise ValueError(
                    f"span_geometric_p must be in (0, 1], got "
                    f"{span_geometric_p}"
                )
            if not 1 <= span_max_length <= 32:
                raise ValueError(
                    f"span_max_length must be in [1, 32], got "
                    f"{span_max_length}"
                )
        if whole_word_masking:
            if word_continues is None:
                raise ValueError(
                    f"{'span' if span_masking else 'whole_word'}_masking "
                    "needs word_continues, the uint8 [vocab_size] table of "
                    "tokenization.word_continuation_table"
                )
            word_continues = np.asarray(word_continues, dtype=np.uint8)
            if word_continues.shape != (vocab_size,):
                raise ValueError(
                    f"word_continues must be uint8 [{vocab_size}], got shape "
                    f"{word_continues.shape}"
                )
        if device_masking and static_masking:
            raise ValueError(
                "device_masking and static_masking are mutually exclusive: "
                "one masks on the device from (seed, epoch, sample index), "
                "the other on the CPU from (seed, sample index)"
            )
        if shuffle:
            raise ValueError(
                "shuffle is not supported; pre-shuffle samples in the shards"
            )
        if isinstance(files, str):
            files = [files]
        files = sorted(files)  # all ranks must agree on order
        self.files, self.file_idxs = self._verify_and_count_samples(files)

        self.mask_token_index = mask_token_index
        self.max_pred_per_seq = max_pred_per_seq
        self.masked_lm_prob = masked_lm_prob
        self.vocab_size = vocab_size
        self.original_token_prob = original_token_prob
        self.random_token_prob = random_token_prob
        self.seed = seed
        self.static_masking = static_masking
        self.device_masking = device_masking
        self.whole_word_masking = whole_word_masking  # span masking included
        self.span_masking = span_masking
        self.span_max_length = span_max_length
        # P(L = k) of the clipped geometric law, k = 1..span_max_length
        law = span_geometric_p * (1 - span_geometric_p) ** np.arange(
            span_max_length if span_masking else 1
        )
        self._span_law = law / law.sum()
        self.word_continues = word_continues if self.whole_word_masking else None
        self.epoch = 0
        self._rng = np.random.default_rng(seed)

        self.file_idx: Optional[int] = None
        self.next_file_idx: Optional[int] = None
        self.file_sample_start_idx = -1
        self.file_sample_end_idx = -1
        self.data: Optional[Dict[str, np.ndarray]] = None
        self._next_data: Optional[Dict[str, np.ndarray]] = None
        self._next_thread: Optional[threading.Thread] = None

    # -- public API ------------------------------------------------------
    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def __len__(self) -> int:
        return self.file_idxs[-1][1]

    def rewind(self) -> None:
        """Forget the resident shard so the next read may start at any
        sample again (a held-out set is re-read from its first sample at
        every evaluation; reads stay sequential from there on)."""
        if self._next_thread is not None:
            self._next_thread.join()
        self.data = self._next_data = self._next_thread = None
        self.file_idx = self.next_file_idx = None
        self.file_sample_start_idx = self.file_sample_end_idx = -1

    def __getitem__(self, idx: int) -> List[np.ndarray]:
        if self.data is None:
            self.next_file_idx = self._file_for_sample(idx)
            self._next_thread = self._async_load(self.next_file_idx)

        if not (self.file_sample_start_idx <= idx < self.file_sample_end_idx):
            # current shard exhausted: join the prefetch, swap, prefetch next
            self.data = None
            self._next_thread.join()
            self.data = self._next_data
            self._next_data = None
            self.file_idx = self.next_file_idx
            self.next_file_idx = (self.next_file_idx + 1) % len(self.files)
            self._next_thread = self._async_load(self.next_file_idx)
            self.file_sample_start_idx = self.file_idxs[self.file_idx][0]
            self.file_sample_end_idx = self.file_idxs[self.file_idx][1]

        if not (self.file_sample_start_idx <= idx < self.file_sample_end_idx):
            raise RuntimeError(
                f"idx {idx} outside current shard "
                f"[{self.file_sample_start_idx}, {self.file_sample_end_idx}): "
                "this dataset requires sequential (chunked-sampler) access"
            )

        local = idx - self.file_sample_start_idx
        input_ids = self.data["input_ids"][local]
        next_sentence_label = self.data["next_sentence_labels"][local]

        if self.device_masking:
            return self._raw_item(idx, local, input_ids, next_sentence_label)

        if "special_token_positions" in self.data:
            special = self.data["special_token_positions"][local]
            segment_ids = self._segment_ids(input_ids, special)
            input_mask = self._input_mask(input_ids, special)
            # static: a generator of this sample's own, whatever was read
            # before it and whichever worker reads it; the stream stays put
            rng = (
                np.random.default_rng([self.seed or 0, idx])
                if self.static_masking
                else self._rng
            )
            masked_input_ids, masked_lm_labels = self._mask_input(
                input_ids, special, rng
            )
        else:  # legacy NVIDIA pre-masked format
            if self.whole_word_masking:
                raise ValueError(
                    f"{self.files[self.file_idx]} is a pre-masked shard (it "
                    "has no special_token_positions): "
                    + (
                        "span_masking / --span_masking"
                        if self.span_masking
                        else "whole_word_masking / --whole_word_masking"
                    )
                    + " needs unmasked shards; drop the flag to train on "
                    "this one"
                )
            segment_ids = self.data["segment_ids"][local]
            input_mask = self.data["input_mask"][local]
            masked_input_ids = input_ids
            masked_lm_labels = self._premasked_labels(
                input_ids,
                self.data["masked_lm_positions"][local],
                self.data["masked_lm_ids"][local],
            )

        return [
            masked_input_ids.astype(np.int64),
            segment_ids.astype(np.int64),
            input_mask.astype(np.int64),
            masked_lm_labels.astype(np.int64),
            np.asarray(next_sentence_label).astype(np.int64),
        ]

    # -- internals -------------------------------------------------------
    def _raw_item(self, idx, local, input_ids, next_sentence_label):
        """device_masking: the unmasked row, its specials as [cls, sep, sep]
        and its global index; ``DeviceMasker`` does the rest on the device.
        Draws nothing from ``_rng``."""
        if "special_token_positions" not in self.data:
            raise ValueError(
                f"{self.files[self.file_idx]} is a pre-masked shard (it has "
                "no special_token_positions): device_masking / "
                "--device_masking needs unmasked shards; drop the flag to "
                "train on this one"
            )
        special = np.asarray(self.data["special_token_positions"][local])
        special3 = np.empty(3, dtype=np.int32)
        special3[: len(special)] = special
        special3[len(special):] = special[-1]
        return [
            np.asarray(input_ids).astype(np.int32),
            special3,
            np.asarray(next_sentence_label).astype(np.int64),
            np.asarray(idx, dtype=np.int64),
        ]

    def _file_for_sample(self, idx: int) -> int:
        for i, (start, end) in enumerate(self.file_idxs):
            if start <= idx < end:
                return i
        raise ValueError(f"idx {idx} exceeds dataset size {len(self)}")

    def _async_load(self, file_idx: int) -> threading.Thread:
        def load(path: str) -> None:
            with H5LiteFile(path) as f:
                self._next_data = {k: np.asarray(f[k]) for k in f.keys()}

        th = threading.Thread(target=load, args=(self.files[file_idx],), daemon=True)
        th.start()
        return th

    @staticmethod
    def _segment_ids(input_ids: np.ndarray, special: np.ndarray) -> np.ndarray:
        """[CLS] a.. [SEP] (b.. [SEP]): second segment (if any) gets 1."""
        segment_ids = np.zeros_like(input_ids)
        if len(special) == 3:
            segment_ids[special[1] + 1 : special[2] + 1] = 1
        return segment_ids

    @staticmethod
    def _input_mask(input_ids: np.ndarray, special: np.ndarray) -> np.ndarray:
        input_mask = np.zeros_like(input_ids)
        input_mask[: special[-1] + 1] = 1
        return input_mask

    def _mask_input(
        self,
        input_ids: np.ndarray,
        special: np.ndarray,
        rng: np.random.Generator,
    ) -> Tuple[np.ndarray, np.ndarray]:
        """80/10/10 masking over non-special, non-pad positions, drawn
        from ``rng``."""
        input_ids = input_ids.copy()  # never mutate the cached shard
        masked_lm_labels = np.full_like(input_ids, -1)
        special_set = set(int(s) for s in special)
        candidates = np.array(
            [i for i in range(int(special[-1])) if i not in special_set],
            dtype=np.int64,
        )
        if candidates.size == 0:
            return input_ids, masked_lm_labels
        mask_count = min(
            self.max_pred_per_seq,
            max(1, int(candidates.size * self.masked_lm_prob)),
        )
        if self.span_masking:
            spans = self._span_indices(input_ids, candidates, mask_count, rng)
            return self._substitute_spans(
                input_ids, masked_lm_labels, spans, rng
            )
        if self.whole_word_masking:
            mask_indices = self._whole_word_indices(
                input_ids, candidates, mask_count, rng
            )
            mask_count = mask_indices.size
        else:
            mask_indices = rng.choice(candidates, mask_count, replace=False)
        masked_lm_labels[mask_indices] = input_ids[mask_indices]
        draws = rng.random(mask_count)
        for idx, draw in zip(mask_indices, draws):
            if draw < self.original_token_prob:
                continue  # keep original token
            if draw < self.original_token_prob + self.random_token_prob:
                input_ids[idx] = rng.integers(0, self.vocab_size - 1)
            else:
                input_ids[idx] = self.mask_token_index
        return input_ids, masked_lm_labels

    def _words(
        self, input_ids: np.ndarray, candidates: np.ndarray
    ) -> List[List[int]]:
        """The words of a row, in position order: a candidate starts a word
        unless its id continues one and the position before it is a
        candidate."""
        words: List[List[int]] = []
        for j in candidates.tolist():
            token = int(input_ids[j])
            continues = (
                0 <= token < self.word_continues.size
                and self.word_continues[token] == 1
            )
            if continues and words and words[-1][-1] == j - 1:
                words[-1].append(j)
            else:
                words.append([j])
        return words

    def _whole_word_indices(
        self,
        input_ids: np.ndarray,
        candidates: np.ndarray,
        mask_count: int,
        rng: np.random.Generator,
    ) -> np.ndarray:
        """Whole-word selection, the rule of ``ops.mlm_mask`` with this
        dataset's generator: a candidate starts a word unless its id
        continues one and the position before it is a candidate; the words
        are visited in a random order and one is taken, all of it, when it
        still fits into ``mask_count``, until ``mask_count`` is reached."""
        words = self._words(input_ids, candidates)
        chosen: List[int] = []
        for w in rng.permutation(len(words)):
            if len(chosen) >= mask_count:
                break
            if len(chosen) + len(words[w]) > mask_count:
                continue
            chosen.extend(words[w])
        return np.array(chosen, dtype=np.int64)

    def _span_indices(
        self,
        input_ids: np.ndarray,
        candidates: np.ndarray,
        mask_count: int,
        rng: np.random.Generator,
    ) -> List[List[int]]:
        """Span selection, the rule of ``ops.mlm_mask(..., span_table=)``
        with this dataset's generator: the words are visited in a random
        order; a free word that still fits into ``mask_count`` anchors a
        span, which grows over the words that follow it directly (a special
        token ends it) up to a length of the clipped geometric law, while
        they are free and fit. The spans, each a list of positions."""
        words = self._words(input_ids, candidates)
        visit = rng.permutation(len(words))  # drawn first, as for whole words
        lengths = 1 + rng.choice(
            self.span_max_length, size=len(words), p=self._span_law
        )
        taken = [False] * len(words)
        spans: List[List[int]] = []
        m = 0
        for w in visit:
            if m >= mask_count:
                break
            if taken[w] or m + len(words[w]) > mask_count:
                continue
            span = list(words[w])
            taken[w] = True
            x = w
            for _ in range(int(lengths[w]) - 1):
                y = x + 1
                if (
                    y == len(words)
                    or words[y][0] != words[x][-1] + 1
                    or taken[y]
                    or m + len(span) + len(words[y]) > mask_count
                ):
                    break
                span.extend(words[y])
                taken[y] = True
                x = y
            m += len(span)
            spans.append(span)
        return spans

    def _substitute_spans(
        self,
        input_ids: np.ndarray,
        masked_lm_labels: np.ndarray,
        spans: List[List[int]],
        rng: np.random.Generator,
    ) -> Tuple[np.ndarray, np.ndarray]:
        """One keep / random / mask decision per span; a random span draws
        a token per position."""
        draws = rng.random(len(spans))
        for span, draw in zip(spans, draws):
            masked_lm_labels[span] = input_ids[span]
            if draw < self.original_token_prob:
                continue  # keep the original tokens
            if draw < self.original_token_prob + self.random_token_prob:
                input_ids[span] = rng.integers(
                    0, self.vocab_size - 1, size=len(span)
                )
            else:
                input_ids[span] = self.mask_token_index
        return input_ids, masked_lm_labels

    @staticmethod
    def _premasked_labels(
        input_ids: np.ndarray,
        masked_lm_positions: np.ndarray,
        masked_lm_ids: np.ndarray,
    ) -> np.ndarray:
        labels = np.full_like(input_ids, -1)
        count = len(masked_lm_positions)
        padded = np.nonzero(masked_lm_positions == 0)[0]
        if padded.size:
            count = padded[0]
        labels[masked_lm_positions[:count]] = masked_lm_ids[:count]
        return labels

    @staticmethod
    def _verify_and_count_samples(
        files: Sequence[str],
    ) -> Tuple[List[str], List[Tuple[int, int]]]:
        current = 0
        ok_files, idxs = [], []
        keys = ["input_ids", "next_sentence_labels"]
        for path in files:
            if not os.path.isfile(path):
                warnings.warn(f"file not found, skipping: {path}")
                continue
            try:
                with H5LiteFile(path) as f:
                    counts = [len(f[k]) for k in keys]
            except Exception as e:  # noqa: BLE001
                warnings.warn(f"unreadable shard {path} ({e}); skipping")
                continue
            if len(set(counts)) != 1:
                warnings.warn(f"per-key sample counts differ in {path}; skipping")
                continue
            ok_files.append(path)
            idxs.append((current, current + counts[0]))
            current += counts[0]
        if not ok_files:
            raise RuntimeError("no valid data shards found")
        return ok_files, idxs


class DistributedSampler(torch.utils.data.distributed.DistributedSampler):
    """Rank-chunked sequential sampler with checkpointable position.

    Each rank draws a CONTIGUOUS chunk of the (padded) index space so a
    rank walks its shard files in order — the double-buffered dataset
    then needs one live shard + one prefetch per rank. The iteration
    position (``index``) round-trips through state_dict for mid-epoch
    resume. (Reference: src/dataset.py:341-428.)
    """

    def __init__(self, dataset, num_replicas=None, rank=None, **kwargs):
        kwargs["shuffle"] = False
        super().__init__(dataset, num_replicas, rank, **kwargs)
        if hasattr(self.dataset, "seed"):
            self.dataset.seed = self.seed

        indices = list(range(len(self.dataset)))
        if not self.drop_last:
            padding = self.total_size - len(indices)
            if padding <= len(indices):
                indices += indices[:padding]
            else:
                indices += (indices * math.ceil(padding / len(indices)))[:padding]
        else:
            indices = indices[: self.total_size]
        assert len(indices) == self.total_size
        self.global_indices = indices
        self.index = 0

    def __len__(self) -> int:
        return self.num_samples

    def __iter__(self):
        return self

    def __next__(self) -> int:
        if self.index == self.num_samples:
            self.index = 0
            raise StopIteration
        value = self.global_indices[self.index + self.rank * self.num_samples]
        self.index += 1
        return value

    def state_dict(self) -> dict:
        return {
            "epoch": self.epoch,
            "seed": self.seed,
            "num_replicas": self.num_replicas,
            "total_size": self.total_size,
            "index": self.index,
        }

    def load_state_dict(self, state: dict) -> None:
        if state["total_size"] != self.total_size:
            warnings.warn(
                "dataset size changed since checkpoint; sampler state reset"
            )
            return
        if state["num_replicas"] != self.num_replicas:
            warnings.warn(
                "world size changed since checkpoint; sampler state reset"
            )
            return
        self.epoch = state["epoch"]
        self.seed = state["seed"]
        self.index = state["index"]

    def set_epoch(self, epoch: int) -> None:
        if hasattr(self.dataset, "set_epoch"):
            self.dataset.set_epoch(epoch)
        self.epoch = epoch
