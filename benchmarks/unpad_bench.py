#!/usr/bin/env python3
"""Padded vs unpadded BERT-Large encoder, forward + backward, one GPU.

For each shape (B=16,S=512 and B=32,S=128) and each length distribution
(all full; uniform in [3S/4, S]; uniform in [S/2, S]; short, uniform in
[S/8, 3S/8], mean about S/4) the 24-layer encoder runs a training step's
forward and backward on the embedding output, once through the padded
path (``BertEncoder`` on [B,S,H]) and once through the unpadded path
(``unpad_index`` + ``pack_rows`` + encoder on [T_pad,H] with
variable-length attention + ``unpack_rows``; the mode's device-to-host
read of T is inside the timed region). bf16 autocast, dropout on, the
shipped TunableOp GEMM cache enabled read-only as in the runners - so
the padded GEMM shapes are tuned and the packed ones are not.

The two paths alternate inside each repeat, so the difference is
measured against the run-to-run spread of the same process. Prints one
JSON line per (shape, distribution, path, repeat), a summary line per
(shape, distribution) and a markdown table.

Run (GPU box): python benchmarks/unpad_bench.py [--steps 10 --repeats 3]
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((16, 512), (32, 128))
DISTRIBUTIONS = ("full", "uniform_3S/4..S", "uniform_S/2..S", "short_S/8..3S/8")


def make_lengths(dist: str, bsz: int, seq: int, seed: int = 0) -> torch.Tensor:
    """Per-sequence valid lengths (CPU int64) for one distribution."""
    gen = torch.Generator().manual_seed(seed)
    lo, hi = {
        "full": (seq, seq),
        "uniform_3S/4..S": (3 * seq // 4, seq),
        "uniform_S/2..S": (seq // 2, seq),
        "short_S/8..3S/8": (seq // 8, 3 * seq // 8),
    }[dist]
    return torch.randint(lo, hi + 1, (bsz,), generator=gen)


def prefix_mask(lengths: torch.Tensor, seq: int) -> torch.Tensor:
    return (torch.arange(seq)[None, :] < lengths[:, None]).long()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=10, help="timed steps per sample")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=3,
                   help="alternating padded/unpadded samples per case")
    p.add_argument("--layers", type=int, default=24)
    args = p.parse_args()
    assert torch.cuda.is_available(), "unpad_bench needs a GPU"

    from bert_pytorch_amd.config import BertConfig
    from bert_pytorch_amd.models import BertModel
    from bert_pytorch_amd.utils import tunable

    tunable.enable()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    config = BertConfig(
        vocab_size_or_config_json_file=1024, hidden_size=1024,
        num_hidden_layers=args.layers, num_attention_heads=16,
        intermediate_size=4096, max_position_embeddings=512,
    )
    model = BertModel(config).to(dev).train()
    hidden = config.hidden_size

    def step(path, emb, mask, seqlens, dout):
        model.zero_grad(set_to_none=True)
        emb.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            if path == "unpadded":
                out = model._unpadded_encoder(emb, mask)[-1]
            else:
                out = model.encoder(emb, seqlens)[-1]
        out.backward(dout)

    def sample(path, *inputs):
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.steps):
            step(path, *inputs)
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / args.steps

    rows = []
    for bsz, seq in SHAPES:
        for dist in DISTRIBUTIONS:
            lengths = make_lengths(dist, bsz, seq)
            mask = prefix_mask(lengths, seq).to(dev)
            seqlens = lengths.to(dev, torch.int32)
            tokens = int(lengths.sum())
            pad_frac = 1.0 - tokens / (bsz * seq)
            emb = (torch.randn(bsz, seq, hidden, device=dev) * 0.5).to(
                torch.bfloat16).requires_grad_(True)
            dout = (torch.randn(bsz, seq, hidden, device=dev) * 0.1).to(
                torch.bfloat16) * mask.unsqueeze(-1).to(torch.bfloat16)
            inputs = (emb, mask, seqlens, dout)
            for path in ("padded", "unpadded"):
                for _ in range(args.warmup):
                    step(path, *inputs)
            torch.cuda.synchronize()
            ms = {"padded": [], "unpadded": []}
            for rep in range(args.repeats):
                for path in ("padded", "unpadded"):
                    t = sample(path, *inputs)
                    ms[path].append(t)
                    print(json.dumps({
                        "B": bsz, "S": seq, "lengths": dist, "path": path,
                        "repeat": rep, "ms_per_step": round(t, 3),
                    }), flush=True)
            med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
            rec = {
                "summary": True, "B": bsz, "S": seq, "lengths": dist,
                "tokens": tokens, "padding_fraction": round(pad_frac, 3),
                "padded_ms": round(med["padded"], 3),
                "padded_min_max": [round(min(ms["padded"]), 3),
                                   round(max(ms["padded"]), 3)],
                "unpadded_ms": round(med["unpadded"], 3),
                "unpadded_min_max": [round(min(ms["unpadded"]), 3),
                                     round(max(ms["unpadded"]), 3)],
                "speedup": round(med["padded"] / med["unpadded"], 3),
            }
            print(json.dumps(rec), flush=True)
            rows.append(rec)

    print("\n| B | S | lengths | tokens | padding | padded ms (min-max) | "
          "unpadded ms (min-max) | padded/unpadded |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['B']} | {r['S']} | {r['lengths']} | {r['tokens']} | "
              f"{100 * r['padding_fraction']:.1f}% | {r['padded_ms']:.2f} "
              f"({r['padded_min_max'][0]:.2f}-{r['padded_min_max'][1]:.2f}) | "
              f"{r['unpadded_ms']:.2f} ({r['unpadded_min_max'][0]:.2f}-"
              f"{r['unpadded_min_max'][1]:.2f}) | {r['speedup']:.2f}x |")


if __name__ == "__main__":
    main()
