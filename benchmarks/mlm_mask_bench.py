"""Microbench of on-device MLM masking (csrc/ops/mlm_mask.hip).

Contenders, at phase-1 (B=96, S=128, max_pred=20) and phase-2 (B=16,
S=512, max_pred=76) shapes:
  mask    ops.mlm_mask on raw rows: masked ids, segment ids, input mask
          and the padded-gather positions/labels, one launch
  gather  what the model runs per micro-step without --device_masking to
          turn dense [B,S] labels into positions (the padded gather of
          BertForPreTraining.forward, copied below); the masks themselves
          are then made on the CPU and are not part of this figure

Default mode alternates the two in one process: each round times every
contender once (device events around ITERS back-to-back calls) and the
table reports the median over rounds with the min-max spread.

``--whole_word`` times whole-word masking instead of the gather:
  wwm     ops.mlm_mask(..., word_continues=table): the whole-word row kernel
          and the scatter kernel, two launches, on the same rows, with a
          table that marks a fifth of the vocabulary as continuation pieces

``--span`` times all three selection rules, alternating:
  mask, wwm as above, and
  span    ops.mlm_mask(..., word_continues=table, span_table=): the span
          instantiation of the row kernel and the scatter kernel, two
          launches, same rows and word table, spans of up to SPAN_MAX words
          with geometric parameter SPAN_P (SpanBERT's 10 and 0.2)

``--trace mask|gather|wwm|span`` instead issues ``--calls`` calls of one contender
per shape after a warm-up and nothing else, for a kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -- \
        python benchmarks/mlm_mask_bench.py --trace mask
Kernel time per call is the stats total over the calls; launches per call
is the number of dispatches over the calls.

Run on a GPU box: python benchmarks/mlm_mask_bench.py [--out FILE.md]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(
    0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
)

import numpy as np
import torch

from bert_pytorch_amd import ops

DEV = "cuda:0"
ROUNDS, ITERS, WARMUP = 15, 50, 10
VOCAB, MASK_TOKEN, PROB = 30522, 103, 0.15
SHAPES = [(96, 128, 20), (16, 512, 76)]
CONTINUES = 0.2  # --whole_word: share of the vocabulary that continues a word
SPAN_P, SPAN_MAX = 0.2, 10


def make_rows(bsz, seq, seed):
    """Shard-like rows: [CLS] a [SEP] b [SEP] pad, 70-100 % full."""
    rng = np.random.default_rng(seed)
    ids = np.zeros((bsz, seq), dtype=np.int32)
    special = np.zeros((bsz, 3), dtype=np.int32)
    for b in range(bsz):
        total = int(rng.integers(int(seq * 0.7), seq + 1))
        ids[b, :total] = rng.integers(1000, VOCAB, size=total)
        special[b] = (0, int(rng.integers(1, total - 2)), total - 1)
    return (
        torch.from_numpy(ids).to(DEV),
        torch.from_numpy(special).to(DEV),
        torch.arange(bsz, dtype=torch.int64, device=DEV),
    )


def padded_gather(masked_lm_labels, max_predictions_per_seq):
    """The padded gather of BertForPreTraining.forward, verbatim."""
    flat_labels = masked_lm_labels.reshape(-1)
    num = flat_labels.numel()
    cap = masked_lm_labels.shape[0] * max_predictions_per_seq
    mask = flat_labels != -1
    slots = torch.cumsum(mask.to(torch.long), 0) - 1
    slots = torch.where(
        mask, slots.clamp_(max=cap), torch.full_like(slots, cap)
    )
    positions = torch.zeros(cap + 1, dtype=torch.long, device=flat_labels.device)
    positions.scatter_(0, slots, torch.arange(num, device=flat_labels.device))
    gathered_labels = torch.full(
        (cap + 1,), -1, dtype=flat_labels.dtype, device=flat_labels.device
    )
    gathered_labels.scatter_(0, slots, flat_labels)
    return positions[:cap], gathered_labels[:cap]


def contenders(bsz, seq, max_pred, whole_word=False, span=False):
    ids, special, index = make_rows(bsz, seq, seed=bsz + seq)
    table = ops.mlm_count_table(seq, PROB, max_pred).to(DEV)
    t_keep, t_rand = ops.mlm_thresholds(0.1, 0.1)

    def run_mask(dense=False, word_continues=None, span_table=None):
        return ops.mlm_mask(
            ids, special, index, table, seed=42, epoch=0, max_pred=max_pred,
            vocab_size=VOCAB, mask_token=MASK_TOKEN, t_keep=t_keep,
            t_rand=t_rand, dense_labels=dense, word_continues=word_continues,
            span_table=span_table,
        )

    if whole_word or span:
        # a fifth of the (uniformly drawn) ids continue a word: words of
        # 1.25 pieces on average, as WordPiece gives on English text
        rng = np.random.default_rng(bsz * seq)
        words = torch.from_numpy(
            (rng.random(VOCAB) < CONTINUES).astype(np.uint8)
        ).to(DEV)
        zeros = torch.zeros_like(words)

        def run_wwm():
            return run_mask(word_continues=words)

        # with no continuation pieces the two paths are one function
        plain = run_mask(dense=True)
        for a, b in zip(plain, run_mask(dense=True, word_continues=zeros)):
            assert torch.equal(a, b)
        got = run_mask(dense=True, word_continues=words)
        positions, gathered = padded_gather(got[5], max_pred)
        assert torch.equal(positions, got[3]) and torch.equal(gathered, got[4])
        if not span:
            return {"mask": run_mask, "wwm": run_wwm}

        lengths = ops.mlm_span_table(SPAN_P, SPAN_MAX).to(DEV)
        one = ops.mlm_span_table(SPAN_P, 1).to(DEV)

        def run_span():
            return run_mask(word_continues=words, span_table=lengths)

        # spans of one word select what whole-word masking selects
        alone = run_mask(dense=True, word_continues=words, span_table=one)
        for k in (1, 2, 3, 4, 5):
            assert torch.equal(alone[k], got[k])
        got = run_mask(dense=True, word_continues=words, span_table=lengths)
        positions, gathered = padded_gather(got[5], max_pred)
        assert torch.equal(positions, got[3]) and torch.equal(gathered, got[4])
        return {"mask": run_mask, "wwm": run_wwm, "span": run_span}

    out = run_mask(dense=True)
    labels = out[5]

    def run_gather():
        return padded_gather(labels, max_pred)

    # the kernel's slots are the gather of its own dense labels
    positions, gathered = run_gather()
    assert torch.equal(positions, out[3]) and torch.equal(gathered, out[4])
    return {"mask": run_mask, "gather": run_gather}


def time_once(fn):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(ITERS):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / ITERS * 1e3  # us per call


def trace(which, calls):
    for bsz, seq, max_pred in SHAPES:
        fn = contenders(bsz, seq, max_pred, whole_word=which == "wwm",
                        span=which == "span")[which]
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    print(f"trace: {which}, {WARMUP} warm-up + {calls} calls at each of "
          f"{SHAPES}; the set-up runs mask and gather once per shape")


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=None, help="also write the table here")
    parser.add_argument("--trace", choices=["mask", "gather", "wwm", "span"],
                        default=None)
    parser.add_argument("--calls", type=int, default=200)
    parser.add_argument("--whole_word", action="store_true",
                        help="time whole-word masking (word_continues=, two "
                             "launches) against token-level ops.mlm_mask")
    parser.add_argument("--span", action="store_true",
                        help="time token-level, whole-word and span masking "
                             "(span_table=), alternating")
    args = parser.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    if args.trace:
        trace(args.trace, args.calls)
        return

    if args.span:
        others = ["ops.mlm_mask, whole words", "ops.mlm_mask, spans"]
    elif args.whole_word:
        others = ["ops.mlm_mask, whole words"]
    else:
        others = ["padded gather (torch)"]
    lines = [
        f"device: {torch.cuda.get_device_name(0)}; {ROUNDS} alternating rounds "
        f"x {ITERS} back-to-back calls, median us per call (min-max over "
        "rounds), host launch cost included",
        "",
        "| B | S | max_pred | ops.mlm_mask | " + " | ".join(others) + " |",
        "|---|---|---|---|" + "---|" * len(others),
    ]
    for bsz, seq, max_pred in SHAPES:
        fns = list(contenders(bsz, seq, max_pred, args.whole_word,
                              args.span).values())
        for fn in fns:
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in fns]
        for _ in range(ROUNDS):
            for slot, fn in enumerate(fns):
                times[slot].append(time_once(fn))

        def cell(t):
            return f"{statistics.median(t):.1f} ({min(t):.1f}-{max(t):.1f})"

        lines.append(
            f"| {bsz} | {seq} | {max_pred} | "
            + " | ".join(cell(t) for t in times) + " |"
        )
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
