"""K-FAC factor update: the HIP kernel against the eager expression.

For each phase-1 / phase-2 row count and each factor width of the
encoder (A of QKV and attention-out: K=1024 + bias; G of QKV: K=3072;
A of FFN2: K=4096 + bias) times

    native: ext.kfac_factor_update (bf16 in, EMA folded in)
    eager:  x.float(), cat ones, fp32 a^T a, mul_/add_   (what
            optim/kfac.py evaluated inline before the kernel existed)

with device events, warmed up, the two alternating in one process,
REPEATS windows of ITERS calls each; prints one JSON line per shape with
the median, min and max per-call time of each and the achieved TF/s of
the native path from the FLOPs the algorithm needs, N*K*(K+1) for the
triangle. Also checks the two results against each other.

    python benchmarks/kfac_factor_bench.py [--repeats 7] [--iters 10]
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert_pytorch_amd.ops import _reference, extension  # noqa: E402

SHAPES = [  # (name, N, K, has_bias)
    ("p1 A qkv/attn-out", 12288, 1024, True),
    ("p1 G qkv", 12288, 3072, False),
    ("p1 A ffn2", 12288, 4096, True),
    ("p1 G attn-out/ffn2", 12288, 1024, False),
    ("p2 A qkv/attn-out", 8192, 1024, True),
    ("p2 G qkv", 8192, 3072, False),
    ("p2 A ffn2", 8192, 4096, True),
]


def window(fn, iters):
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    ext = extension()
    print(json.dumps({"device": torch.cuda.get_device_name(0),
                      "repeats": args.repeats, "iters": args.iters,
                      "dtype": args.dtype}), flush=True)
    for name, N, K, has_bias in SHAPES:
        D = K + int(has_bias)
        x = (torch.randn(N, K, device=dev) * 0.5).to(dtype)
        beta, alpha = 0.95, 0.05 / N
        coef = torch.tensor([beta, alpha], device=dev)
        f_nat = torch.zeros(D, D, device=dev)
        f_eag = torch.zeros(D, D, device=dev)

        def native():
            ext.kfac_factor_update(x, f_nat, coef, has_bias, 0)

        def eager():
            _reference.kfac_factor_update(x, f_eag, beta, alpha, has_bias)

        native(), eager()
        torch.cuda.synchronize()
        rel = float((f_nat - f_eag).abs().max() / f_eag.abs().max())
        for _ in range(3):
            native(), eager()
        t_nat, t_eag = [], []
        for _ in range(args.repeats):
            t_nat.append(window(native, args.iters))
            t_eag.append(window(eager, args.iters))
        flops = N * K * (K + 1)
        med_n, med_e = statistics.median(t_nat), statistics.median(t_eag)
        print(json.dumps({
            "shape": name, "N": N, "K": K, "has_bias": has_bias,
            "native_us": {"median": round(med_n, 1), "min": round(min(t_nat), 1),
                          "max": round(max(t_nat), 1)},
            "eager_us": {"median": round(med_e, 1), "min": round(min(t_eag), 1),
                         "max": round(max(t_eag), 1)},
            "speedup_median": round(med_e / med_n, 2),
            "native_wins_beyond_spread": max(t_nat) < min(t_eag),
            "native_tflops_triangle": round(flops / med_n / 1e6, 1),
            "max_rel_diff": rel,
        }), flush=True)
        del x, f_nat, f_eag


if __name__ == "__main__":
    main()
