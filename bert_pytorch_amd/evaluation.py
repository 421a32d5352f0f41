"""Held-out evaluation of a pretraining model: loss and top-1 accuracy of
the masked-LM head, loss and accuracy of the next-sentence head.

The MLM head goes through ``BertForPreTraining.forward(mlm_eval=True)``,
i.e. ``ops.mlm_decoder_eval``: on the GPU the logits-free instantiation
of the fused decoder kernel, which hands back the loss sum, the row
count, the number of correct rows and the predictions without a [P, V]
tensor. The six sums accumulate on the device in fp64, are all-reduced
once, and are read by the host once.

An evaluation leaves training as it found it: the model runs in eval
mode (no dropout, so nothing is drawn from the Philox counter of
``ops.rng``) under ``torch.no_grad`` and returns to its previous mode,
and nothing is drawn from the global torch / numpy generators. The
loader is the caller's; build it with ``make_eval_loader`` (or give it a
``generator=`` of its own), because creating a DataLoader iterator
otherwise draws its base seed from the global torch generator.
"""

from __future__ import annotations

import contextlib
from typing import Dict, Iterable, Optional

import torch
import torch.distributed as dist
import torch.nn.functional as F


def make_eval_loader(
    dataset, sampler, batch_size: int, seed: int = 0, num_workers: int = 0,
    pin_memory: bool = False,
) -> torch.utils.data.DataLoader:
    """A DataLoader for a held-out set that owns its generator, so
    iterating it never touches the global torch generator."""
    generator = torch.Generator()
    generator.manual_seed(seed)
    return torch.utils.data.DataLoader(
        dataset,
        sampler=sampler,
        batch_size=batch_size,
        num_workers=num_workers,
        pin_memory=pin_memory,
        drop_last=True,
        generator=generator,
    )


@torch.no_grad()
def evaluate_pretraining(
    model: torch.nn.Module,
    loader: Iterable,
    device: torch.device,
    autocast_dtype: Optional[torch.dtype] = None,
    max_predictions_per_seq: Optional[int] = None,
    max_batches: Optional[int] = None,
) -> Dict[str, float]:
    """Evaluate ``model`` on up to ``max_batches`` batches of ``loader``
    (each rank on its own batches; the sums are all-reduced).

    Returns ``eval_loss`` (MLM mean + NSP mean), ``eval_mlm_loss``,
    ``eval_mlm_accuracy``, ``eval_masked_tokens`` and
    ``eval_sequences``, plus ``eval_nsp_loss`` and ``eval_nsp_accuracy``
    when the model has the next-sentence head.
    """
    raw = model.module if hasattr(model, "module") else model
    was_training = raw.training
    raw.eval()
    # mlm loss-sum / count / correct, nsp loss-sum / count / correct
    sums = torch.zeros(6, dtype=torch.float64, device=device)
    sequences = 0
    has_nsp = False
    try:
        for i, batch in enumerate(loader):
            if max_batches is not None and i >= max_batches:
                break
            input_ids, segment_ids, input_mask, mlm_labels, nsp_labels = (
                t.to(device, non_blocking=True) for t in batch
            )
            sequences += input_ids.shape[0]
            autocast = (
                torch.autocast(device_type=device.type, dtype=autocast_dtype)
                if autocast_dtype is not None
                else contextlib.nullcontext()
            )
            with autocast:
                mlm, seq_rel, _ = raw(
                    input_ids, segment_ids, input_mask,
                    masked_lm_labels=mlm_labels,
                    max_predictions_per_seq=max_predictions_per_seq,
                    mlm_eval=True,
                )
            terms = [mlm.loss_sum, mlm.count, mlm.correct]
            if seq_rel is not None:
                has_nsp = True
                scores = seq_rel.view(-1, 2).float()
                target = nsp_labels.view(-1)
                valid = target != -1
                terms += [
                    F.cross_entropy(
                        scores, target, ignore_index=-1, reduction="sum"
                    ),
                    valid.sum(),
                    ((scores.argmax(dim=1) == target) & valid).sum(),
                ]
            else:
                terms += [sums.new_zeros(())] * 3
            sums += torch.stack([t.to(torch.float64) for t in terms])
    finally:
        raw.train(was_training)

    totals = torch.cat(
        [sums, sums.new_tensor([float(sequences), float(has_nsp)])]
    )
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(totals, op=dist.ReduceOp.SUM)
    (mlm_loss, mlm_count, mlm_correct, nsp_loss, nsp_count, nsp_correct,
     n_seq, any_nsp) = totals.tolist()  # the one host read

    out = {
        "eval_mlm_loss": mlm_loss / max(mlm_count, 1.0),
        "eval_mlm_accuracy": mlm_correct / max(mlm_count, 1.0),
        "eval_masked_tokens": int(mlm_count),
        "eval_sequences": int(n_seq),
    }
    out["eval_loss"] = out["eval_mlm_loss"]
    if any_nsp > 0:
        out["eval_nsp_loss"] = nsp_loss / max(nsp_count, 1.0)
        out["eval_nsp_accuracy"] = nsp_correct / max(nsp_count, 1.0)
        out["eval_loss"] += out["eval_nsp_loss"]
    return out
