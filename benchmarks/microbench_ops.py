#!/usr/bin/env python3
"""Per-op microbenchmarks on MI355X: time each HIP kernel at the
phase-1/phase-2 training shapes, report effective HBM bandwidth
against the measured copy ceiling (~6.3 TB/s) and against the eager
PyTorch composition.

Run (GPU box): python benchmarks/microbench_ops.py [--phase 1]
                  [--dtype bf16|fp16]
Prints one JSON line per op.

``--section mfma`` times only the three MFMA kernels that exist in a
bf16 and an fp16 instantiation (attention, split-K wgrad at the four
encoder shapes next to the library's ``dy.t() @ x``, MLM head). With
several ``--dtype`` values and ``--repeats N`` the dtypes alternate
inside each repeat, so fp16 is compared with the bf16 run-to-run spread
of the same process; a final summary line per op gives min/median/max.

``--section varlen`` times variable-length (packed) attention against
padded attention at B=16,S=512 and B=32,S=128 for the length
distributions of benchmarks/unpad_bench.py, forward and backward, with
and without dropout; the two kernels alternate inside each repeat.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bert_pytorch_amd import ops  # noqa: E402
from bert_pytorch_amd.ops import (  # noqa: E402
    fused_attention,
    fused_bias_dropout_residual_ln,
    fused_bias_gelu,
    fused_cross_entropy,
    fused_layer_norm,
)


def timeit(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters * 1e3  # us


def report(name, us, bytes_moved, extra=None):
    rec = {
        "op": name,
        "us": round(us, 2),
        "GB": round(bytes_moved / 1e9, 4),
        "TB_s": round(bytes_moved / (us * 1e-6) / 1e12, 2),
    }
    if extra:
        rec.update(extra)
    print(json.dumps(rec), flush=True)
    return rec


DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def bench_mfma(phase, dtypes, repeats):
    """attention / wgrad / MLM-head kernels, called through the
    extension so nothing but the kernels under test is timed."""
    dev = torch.device("cuda:0")
    ext = ops.extension()
    b, s = (96, 128) if phase == 1 else (16, 512)
    rows = b * s
    H, FFN, NH, V, P = 1024, 4096, 16, 30528, 1280
    samples = {}

    def timeit_long(fn):  # ~10-60 ms timed window per sample
        return timeit(fn, iters=200, warmup=20)

    def rec(name, dname, us, extra=None):
        report(f"{name}[{dname}]", us, 0, extra)
        samples.setdefault((name, dname), []).append(us)

    inputs = {}
    for dname in dtypes:
        dt = DTYPES[dname]
        torch.manual_seed(0)
        inp = {
            "qkv": (torch.randn(b, s, 3 * H, device=dev) * 0.5).to(dt),
            "do": (torch.randn(b, s, H, device=dev) * 0.5).to(dt),
            "h": (torch.randn(P, H, device=dev) * 0.5).to(dt),
            "wv": (torch.randn(V, H, device=dev) * 0.05).to(dt),
        }
        # the four encoder wgrad shapes (M = out features, N = in)
        for tag, (m, n) in {
            "qkv": (3 * H, H), "attn_out": (H, H),
            "ffn1": (FFN, H), "ffn2": (H, FFN),
        }.items():
            inp["dy_" + tag] = torch.randn(rows, m, device=dev, dtype=dt)
            inp["x_" + tag] = torch.randn(rows, n, device=dev, dtype=dt)
        inputs[dname] = inp
    seqlens = torch.full((b,), s, device=dev, dtype=torch.int32)
    bias_v = torch.randn(V, device=dev) * 0.1
    labels = torch.randint(0, V, (P,), device=dev)
    aflops = 4 * b * NH * s * s * 64

    for _ in range(repeats):
        for dname in dtypes:
            inp = inputs[dname]
            qkv, do = inp["qkv"], inp["do"]
            for p_drop, sfx in ((0.0, ""), (0.1, "_drop")):
                us = timeit_long(
                    lambda: ext.attention_fwd(qkv, seqlens, NH, p_drop, 7, 0)
                )
                rec("attn_fwd" + sfx, dname, us,
                    {"TFLOP_s": round(aflops / (us * 1e-6) / 1e12, 1)})
                out, lse, dmask = ext.attention_fwd(
                    qkv, seqlens, NH, p_drop, 7, 0
                )
                # delta + dK/dV kernel + dQ kernel (split per kernel:
                # rocprofv3 --kernel-trace --stats on this same command)
                us = timeit_long(
                    lambda: ext.attention_bwd(
                        do, qkv, seqlens, out, lse, dmask, NH, p_drop, 7, 0
                    )
                )
                rec("attn_bwd" + sfx, dname, us,
                    {"TFLOP_s": round(2.5 * aflops / (us * 1e-6) / 1e12, 1)})
            for tag in ("qkv", "attn_out", "ffn1", "ffn2"):
                dy, x = inp["dy_" + tag], inp["x_" + tag]
                wflops = 2 * rows * dy.shape[1] * x.shape[1]
                shape = f"K{rows}_M{dy.shape[1]}_N{x.shape[1]}"
                us = timeit_long(lambda: ext.wgrad_tn(dy, x))
                rec(f"wgrad_tn_{tag}_{shape}", dname, us,
                    {"TFLOP_s": round(wflops / (us * 1e-6) / 1e12, 1),
                     "routed_in_repo": bool(ext.wgrad_tn_profitable(
                         rows, dy.shape[1], x.shape[1]))})
                us = timeit_long(lambda: dy.t() @ x)
                rec(f"wgrad_lib_{tag}_{shape}", dname, us,
                    {"TFLOP_s": round(wflops / (us * 1e-6) / 1e12, 1)})
            us = timeit_long(
                lambda: ext.mlm_head_fwd(
                    inp["h"], inp["wv"], bias_v, labels, -1
                )
            )
            rec(f"mlm_head_fwd_P{P}", dname, us,
                {"TFLOP_s": round(2 * P * H * V / (us * 1e-6) / 1e12, 1)})

    for (name, dname), v in samples.items():
        v = sorted(v)
        print(json.dumps({
            "summary": name, "dtype": dname, "n": len(v),
            "min_us": round(v[0], 2), "median_us": round(v[len(v) // 2], 2),
            "max_us": round(v[-1], 2),
        }), flush=True)


def bench_varlen(dtypes, repeats):
    """attention_varlen_fwd/bwd next to attention_fwd/bwd on the same
    sequences: the padded call sees [B,S,3H] and per-sequence lengths,
    the packed call the valid rows only and cu_seqlens."""
    from unpad_bench import DISTRIBUTIONS, SHAPES, make_lengths

    dev = torch.device("cuda:0")
    ext = ops.extension()
    H, NH = 1024, 16
    samples = {}

    def timeit_long(fn):
        return timeit(fn, iters=200, warmup=20)

    def rec(name, us, extra):
        report(name, us, 0, extra)
        samples.setdefault(name, []).append(us)

    for dname in dtypes:
        dt = DTYPES[dname]
        for b, s in SHAPES:
            for dist in DISTRIBUTIONS:
                torch.manual_seed(0)
                lengths = make_lengths(dist, b, s)
                total = int(lengths.sum())
                t_pad = -(-total // 128) * 128
                cu = torch.zeros(b + 1, dtype=torch.int32)
                cu[1:] = torch.cumsum(lengths, 0)
                cu = cu.to(dev)
                seqlens = lengths.to(dev, torch.int32)
                qkv_p = (torch.randn(b, s, 3 * H, device=dev) * 0.5).to(dt)
                do_p = (torch.randn(b, s, H, device=dev) * 0.5).to(dt)
                qkv_v = (torch.randn(t_pad, 3 * H, device=dev) * 0.5).to(dt)
                do_v = (torch.randn(t_pad, H, device=dev) * 0.5).to(dt)
                # useful work: the valid [len, len] score blocks only
                aflops = 4 * NH * 64 * int((lengths * lengths).sum())
                info = {"pad_frac": round(1 - total / (b * s), 3)}
                for _ in range(repeats):
                    for p_drop, sfx in ((0.0, ""), (0.1, "_drop")):
                        tag = f"B{b}_S{s}_{dist}{sfx}[{dname}]"
                        calls = {
                            "padded": (
                                lambda: ext.attention_fwd(
                                    qkv_p, seqlens, NH, p_drop, 7, 0),
                                lambda o, l, m: ext.attention_bwd(
                                    do_p, qkv_p, seqlens, o, l, m, NH,
                                    p_drop, 7, 0),
                            ),
                            "varlen": (
                                lambda: ext.attention_varlen_fwd(
                                    qkv_v, cu, s, NH, p_drop, 7, 0),
                                lambda o, l, m: ext.attention_varlen_bwd(
                                    do_v, qkv_v, cu, s, o, l, m, NH,
                                    p_drop, 7, 0),
                            ),
                        }
                        for kind, (fwd, bwd) in calls.items():
                            us = timeit_long(fwd)
                            rec(f"attn_{kind}_fwd_{tag}", us, dict(
                                info, useful_TFLOP_s=round(
                                    aflops / (us * 1e-6) / 1e12, 1)))
                            o, l, m = fwd()
                            us = timeit_long(lambda: bwd(o, l, m))
                            rec(f"attn_{kind}_bwd_{tag}", us, dict(
                                info, useful_TFLOP_s=round(
                                    2.5 * aflops / (us * 1e-6) / 1e12, 1)))

    for name, v in samples.items():
        v = sorted(v)
        print(json.dumps({
            "summary": name, "n": len(v), "min_us": round(v[0], 2),
            "median_us": round(v[len(v) // 2], 2),
            "max_us": round(v[-1], 2),
        }), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--phase", type=int, default=1, choices=[1, 2])
    p.add_argument("--dtype", nargs="+", default=["bf16"],
                   choices=sorted(DTYPES),
                   help="16-bit element type(s); --section all uses the first")
    p.add_argument("--section", default="all", choices=["all", "mfma", "varlen"])
    p.add_argument("--repeats", type=int, default=1,
                   help="--section mfma/varlen: timed repeats per op and dtype")
    args = p.parse_args()
    assert torch.cuda.is_available()
    if args.section == "mfma":
        bench_mfma(args.phase, args.dtype, args.repeats)
        return
    if args.section == "varlen":
        bench_varlen(args.dtype, args.repeats)
        return
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    b, s = (96, 128) if args.phase == 1 else (16, 512)
    rows = b * s
    H, FFN, NH, V = 1024, 4096, 16, 30528
    dt = DTYPES[args.dtype[0]]
    e = 2  # bytes/elem

    # ---- ceiling: pure copy
    x_big = torch.randn(rows, FFN, device=dev, dtype=dt)
    y_big = torch.empty_like(x_big)
    us = timeit(lambda: y_big.copy_(x_big))
    report("copy_ceiling[rows,4096]", us, 2 * rows * FFN * e)

    # ---- bias-GELU fwd/bwd at FFN shape
    bias = torch.randn(FFN, device=dev, dtype=torch.float32)
    us = timeit(lambda: fused_bias_gelu(x_big, bias))
    report("bias_gelu_fwd[rows,4096]", us, 2 * rows * FFN * e)
    eag = lambda: torch.nn.functional.gelu(x_big.float() + bias).to(dt)  # noqa: E731
    us_e = timeit(eag, iters=20)
    report("bias_gelu_fwd_eager", us_e, 2 * rows * FFN * e)

    xg = x_big.clone().requires_grad_(True)
    yv = fused_bias_gelu(xg, bias)
    dy = torch.randn_like(yv)

    def bwd():
        ext = ops.extension()
        ext.bias_gelu_bwd(dy, x_big, bias)

    us = timeit(bwd)
    report("bias_gelu_bwd[rows,4096]", us, 3 * rows * FFN * e)

    # ---- bdrl fwd/bwd at H shape
    x = torch.randn(rows, H, device=dev, dtype=dt)
    res = torch.randn_like(x)
    g = torch.ones(H, device=dev, dtype=torch.float32)
    bt = torch.zeros(H, device=dev, dtype=torch.float32)
    hb = torch.randn(H, device=dev, dtype=torch.float32)
    ext = ops.extension()
    us = timeit(
        lambda: ext.bias_dropout_residual_ln_fwd(x, hb, res, g, bt, 0.1,
                                                 1e-12, 123, 0)
    )
    # x + res reads, z + y + mask writes
    report("bdrl_fwd[rows,1024]", us, rows * H * (4 * e + 1))
    yy, z, mask, mean, rstd = ext.bias_dropout_residual_ln_fwd(
        x, hb, res, g, bt, 0.1, 1e-12, 123, 0
    )
    dyt = torch.randn_like(yy)
    us = timeit(
        lambda: ext.bias_dropout_residual_ln_bwd(dyt, z, mask, g, mean, rstd,
                                                 0.1, True)
    )
    report("bdrl_bwd[rows,1024]", us, rows * H * (4 * e + 1))

    # ---- LayerNorm fwd/bwd
    w = torch.ones(H, device=dev, dtype=torch.float32)
    us = timeit(lambda: ext.ln_fwd(x, w, bt, 1e-12))
    report("ln_fwd[rows,1024]", us, 2 * rows * H * e)
    yv2, mean2, rstd2 = ext.ln_fwd(x, w, bt, 1e-12)
    us = timeit(lambda: ext.ln_bwd(dyt, x, w, mean2, rstd2))
    report("ln_bwd[rows,1024]", us, 3 * rows * H * e)

    # ---- embedding gather + add + LayerNorm + dropout forward (fp32
    # tables and a 16-bit output, as under autocast)
    ids = torch.randint(0, V, (b, s), device=dev)
    tt = torch.randint(0, 2, (b, s), device=dev)
    word = torch.randn(V, H, device=dev)
    pos = torch.randn(512, H, device=dev)
    tok = torch.randn(2, H, device=dev)
    us = timeit(
        lambda: ext.embedding_ln_dropout_fwd(ids, tt, word, pos, tok, w, bt,
                                             0.1, 1e-12, 123, 0, dt)
    )
    # three fp32 table rows read per output row (nominal: repeated ids and
    # the 128 position rows come from cache, so the rate can exceed the
    # copy ceiling); fp32 z, y and the byte mask written
    report("embed_fwd[rows,1024]", us, rows * H * (3 * 4 + 4 + e + 1))

    # ---- attention fwd/bwd
    qkv = torch.randn(b, s, 3 * H, device=dev, dtype=dt)
    seqlens = torch.full((b,), s, device=dev, dtype=torch.int32)
    us = timeit(lambda: fused_attention(qkv, seqlens, NH, 0.0, True))
    flops = 4 * b * NH * s * s * 64  # 2 GEMMs of [s,64]x[64,s]
    report("attn_fwd", us, 0, {"TFLOP_s": round(flops / (us * 1e-6) / 1e12, 1)})
    out = fused_attention(qkv.requires_grad_(True), seqlens, NH, 0.0, True)
    do = torch.randn_like(out)
    us = timeit(lambda: torch.autograd.grad(out, qkv, do, retain_graph=True))
    report("attn_bwd", us, 0,
           {"TFLOP_s": round(2.5 * flops / (us * 1e-6) / 1e12, 1)})
    # production path: dropout p=0.1 (bit-packed stored mask: gen kernel
    # in fwd, mask reads in fwd + both bwd kernels)
    us = timeit(lambda: fused_attention(qkv.detach(), seqlens, NH, 0.1, True))
    report("attn_fwd_drop", us, 0,
           {"TFLOP_s": round(flops / (us * 1e-6) / 1e12, 1)})
    out = fused_attention(qkv, seqlens, NH, 0.1, True)
    us = timeit(lambda: torch.autograd.grad(out, qkv, do, retain_graph=True))
    report("attn_bwd_drop", us, 0,
           {"TFLOP_s": round(2.5 * flops / (us * 1e-6) / 1e12, 1)})

    # ---- cross entropy at vocab shape
    logits = torch.randn(rows, V, device=dev, dtype=dt)
    labels = torch.randint(-1, V, (rows,), device=dev)
    lf = logits.requires_grad_(True)
    us = timeit(lambda: fused_cross_entropy(lf, labels, -1), iters=20)
    report("ce_fwd[rows,30528]", us, rows * V * e)

    # ---- GEMM reference points (hipBLASLt through torch.matmul)
    a = torch.randn(rows, H, device=dev, dtype=dt)
    w1 = torch.randn(FFN, H, device=dev, dtype=dt)
    us = timeit(lambda: torch.nn.functional.linear(a, w1))
    report("gemm_ffn1", us, 0,
           {"TFLOP_s": round(2 * rows * H * FFN / (us * 1e-6) / 1e12, 1)})
    wv = torch.randn(V, H, device=dev, dtype=dt)
    us = timeit(lambda: torch.nn.functional.linear(a, wv))
    report("gemm_vocab", us, 0,
           {"TFLOP_s": round(2 * rows * H * V / (us * 1e-6) / 1e12, 1)})


if __name__ == "__main__":
    main()
