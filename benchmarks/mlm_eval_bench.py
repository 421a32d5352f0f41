"""A/B/C microbench of the MLM head in evaluation: the logits-free
instantiation against the training instantiation and the library route.

Contenders, at P in {1280, 2560}, V=30528, K=1024, bf16:
  eval     ext.mlm_head_eval (GEMM + stats + arg-max, no [P,V] store)
  train    ext.mlm_head_fwd  (same GEMM + stats, stores the logits)
  library  F.linear + ext.ce_fwd + torch.argmax + the correct count,
           which is what ops.mlm_decoder_eval runs with BPA_FUSED_MLM=0

The three alternate in one process: each round times every contender
once (device events around ITERS back-to-back calls), and the table
reports the median over rounds with the min-max spread, so drift of the
machine hits all of them alike. Before timing, the outputs of `eval` are
compared with `train` (bitwise) and with the library route (pred).

Run on a GPU box: python benchmarks/mlm_eval_bench.py [--out FILE.md]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(
    0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
)

import torch
import torch.nn.functional as F

from bert_pytorch_amd import ops

DEV = "cuda:0"
ROUNDS, ITERS, WARMUP = 15, 40, 10


def time_once(fn):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(ITERS):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / ITERS * 1e3  # us per call


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=None, help="also write the table here")
    args = parser.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    ext = ops.extension()

    lines = [
        f"device: {torch.cuda.get_device_name(0)}; bf16, V=30528, K=1024; "
        f"{ROUNDS} alternating rounds x {ITERS} calls, median us "
        "(min-max over rounds)",
        "",
        "| P | mlm_head_eval | mlm_head_fwd | GEMM + ce_fwd + argmax | "
        "eval vs fwd | eval vs library |",
        "|---|---|---|---|---|---|",
    ]
    for P, V, K in [(1280, 30528, 1024), (2560, 30528, 1024)]:
        torch.manual_seed(0)
        h = (torch.randn(P, K, device=DEV) * 0.5).bfloat16()
        w = (torch.randn(V, K, device=DEV) * 0.05).bfloat16()
        b = torch.randn(V, device=DEV).float()
        bb = b.bfloat16()
        labels = torch.randint(0, V, (P,), device=DEV)
        labels[::5] = -1

        def run_eval():
            return ext.mlm_head_eval(h, w, b, labels, -1)

        def run_train():
            return ext.mlm_head_fwd(h, w, b, labels, -1)

        def run_library():
            logits = F.linear(h, w, bb)
            loss_sum, count, _ = ext.ce_fwd(logits, labels, -1)
            pred = torch.argmax(logits, dim=1)
            correct = ((pred == labels) & (labels != -1)).sum()
            return loss_sum, count, correct, pred

        # same results first (bias is rounded to bf16 on the library
        # route, so only the kernel pair is compared bitwise)
        e_loss, e_count, e_correct, e_lse, e_pred = run_eval()
        logits, t_loss, t_count, t_lse = run_train()
        assert torch.equal(e_lse, t_lse) and torch.equal(e_loss, t_loss)
        assert torch.equal(e_count, t_count)
        assert torch.equal(e_pred.long(), logits.float().argmax(dim=1))
        del logits

        contenders = [run_eval, run_train, run_library]
        for fn in contenders:
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in contenders]
        for _ in range(ROUNDS):
            for slot, fn in enumerate(contenders):
                times[slot].append(time_once(fn))
        med = [statistics.median(t) for t in times]

        def cell(t):
            return f"{statistics.median(t):.1f} ({min(t):.1f}-{max(t):.1f})"

        lines.append(
            f"| {P} | {cell(times[0])} | {cell(times[1])} | {cell(times[2])} "
            f"| {100 * (med[0] / med[1] - 1):+.1f}% "
            f"| {100 * (med[0] / med[2] - 1):+.1f}% |"
        )
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
