"""dtype/shape gates that route fp16 to the native kernels. The gates
are pure functions of dtype and shape, so they are checked on CPU
tensors (no GPU, no extension needed)."""

import torch

from bert_pytorch_amd.ops import attention as attn_ops
from bert_pytorch_amd.ops import ffn as ffn_ops
from bert_pytorch_amd.ops import mlm as mlm_ops


def test_attention_gate_accepts_fp16():
    qkv = torch.zeros(2, 128, 768, dtype=torch.float16)
    assert attn_ops._kernel_supported(qkv, 4)
    assert attn_ops._kernel_supported(qkv.bfloat16(), 4)


def test_attention_gate_rejects_fp32_and_small_heads():
    qkv = torch.zeros(2, 128, 768, dtype=torch.float16)
    assert not attn_ops._kernel_supported(qkv.float(), 4)
    assert not attn_ops._kernel_supported(qkv, 8)  # head_dim 32
    assert not attn_ops._kernel_supported(qkv[:, :72], 4)  # S % 16 != 0


def test_ffn_gate_rejects_fp16(monkeypatch):
    """The GEMM-epilogue FFN is bf16-only; fp16 must take the standalone
    bias-GELU kernels even where the library offers the epilogue."""
    monkeypatch.setattr(ffn_ops, "use_native", lambda t: True)
    monkeypatch.setattr(ffn_ops, "_aux_supported", True)
    x = torch.zeros(4, 256)
    assert not ffn_ops.ffn_supported(x.half())
    assert not ffn_ops.ffn_supported(x)
    assert ffn_ops.ffn_supported(x.bfloat16())


def test_mlm_kernel_dtype_choice():
    x = torch.zeros(4, 256)
    assert mlm_ops._kernel_dtype(x.half()) == torch.float16
    assert mlm_ops._kernel_dtype(x.bfloat16()) == torch.bfloat16
    assert mlm_ops._kernel_dtype(x) is None
