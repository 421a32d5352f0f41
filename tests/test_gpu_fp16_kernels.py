"""fp16 instantiations of the MFMA kernels (attention, split-K wgrad,
MLM head) vs the eager fp32 composites. The bounds are the project's
bf16 bounds from tests/test_gpu_kernels.py: fp16 carries three more
mantissa bits, so it has to meet them; a wrong fragment layout shows as
O(1) error. All tests @pytest.mark.gpu."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bert_pytorch_amd import ops
    from bert_pytorch_amd.ops import _reference as ref

DEV = "cuda:0"
F16 = torch.float16


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    a = a.float()
    b = b.float()
    denom = b.abs().max().clamp(min=1e-3)
    return float((a - b).abs().max() / denom)


def ext():
    return ops.extension()


def _count_calls(monkeypatch, *names):
    """Wrap extension entry points so calls through ops.* are counted."""
    mod = ext()
    counts = {n: 0 for n in names}

    def wrap(name, fn):
        def inner(*a, **kw):
            counts[name] += 1
            return fn(*a, **kw)

        return inner

    for n in names:
        monkeypatch.setattr(mod, n, wrap(n, getattr(mod, n)))
    return counts


# ---------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------
@pytest.mark.parametrize(
    "B,S,NH",
    [
        (3, 80, 4),    # S not a multiple of 64: partial key tile
        (2, 128, 4),
        (1, 16, 2),    # minimum S
        (1, 512, 2),   # several key tiles
    ],
)
def test_attention_forward_fp16(B, S, NH):
    torch.manual_seed(7)
    H = NH * 64
    qkv = (torch.randn(B, S, 3 * H, device=DEV) * 0.5).half()
    seqlens = torch.randint(S // 2, S + 1, (B,), device=DEV, dtype=torch.int32)
    out, lse, _mask = ext().attention_fwd(qkv, seqlens, NH, 0.0, 0, 0)
    assert out.dtype == F16 and lse.dtype == torch.float32
    out_ref = ref.attention(qkv.float(), seqlens, NH, 0.0, False)
    assert rel_err(out, out_ref) < 3e-2


def test_attention_forward_spike_fp16():
    """Online-softmax max tracking: one huge key must not break numerics."""
    torch.manual_seed(8)
    B, S, NH = 2, 128, 4
    H = NH * 64
    qkv = torch.randn(B, S, 3 * H, device=DEV) * 0.3
    # spike a late key so the running max jumps at the last tile
    qkv[:, S - 3, H : 2 * H] += 40.0
    qkv = qkv.half()
    seqlens = torch.full((B,), S, device=DEV, dtype=torch.int32)
    out, _, _m = ext().attention_fwd(qkv, seqlens, NH, 0.0, 0, 0)
    out_ref = ref.attention(qkv.float(), seqlens, NH, 0.0, False)
    assert torch.isfinite(out.float()).all()
    assert rel_err(out, out_ref) < 5e-2


@pytest.mark.parametrize("B,S,NH", [(3, 80, 4), (2, 128, 4), (1, 512, 2)])
def test_attention_backward_fp16(B, S, NH):
    torch.manual_seed(9)
    H = NH * 64
    qkv = (torch.randn(B, S, 3 * H, device=DEV) * 0.5).half()
    seqlens = torch.randint(S // 2, S + 1, (B,), device=DEV, dtype=torch.int32)
    qr = qkv.float().detach().requires_grad_(True)
    out_ref = ref.attention(qr, seqlens, NH, 0.0, False)
    dout = torch.randn_like(out_ref) * 0.5
    out_ref.backward(dout)

    out, lse, _mask = ext().attention_fwd(qkv, seqlens, NH, 0.0, 0, 0)
    dqkv = ext().attention_bwd(
        dout.half(), qkv, seqlens, out, lse, _mask, NH, 0.0, 0, 0
    )
    assert dqkv.dtype == F16
    assert rel_err(dqkv, qr.grad) < 6e-2


@pytest.mark.parametrize("B,S,NH", [(2, 128, 4), (1, 512, 2)])
def test_attention_dropout_numerics_fp16(B, S, NH):
    """Forward and backward with dropout vs an eager fp32 reference
    conditioned on the kernel's own stored keep-mask; the mask itself is
    dtype-independent, so it must equal a bf16 call's bit for bit."""
    torch.manual_seed(21)
    H = NH * 64
    p = 0.1
    p_q = round(p * 256) / 256  # the kernel's 8-bit-quantized drop prob
    qkv = (torch.randn(B, S, 3 * H, device=DEV) * 0.5).half()
    seqlens = torch.randint(S // 2, S + 1, (B,), device=DEV, dtype=torch.int32)

    out, lse, dmask = ext().attention_fwd(qkv, seqlens, NH, p, 77, 5)
    _o, _l, dmask_bf16 = ext().attention_fwd(
        qkv.bfloat16(), seqlens, NH, p, 77, 5
    )
    assert torch.equal(dmask, dmask_bf16)

    # dmask is bit-packed: [B*NH, S, ceil(S/32)] int32, LSB-first
    bits = dmask.view(torch.uint8).reshape(B, NH, S, -1).int()
    shifts = torch.arange(8, device=DEV, dtype=torch.int32)
    keep = ((bits.unsqueeze(-1) >> shifts) & 1).reshape(B, NH, S, -1)
    keep = keep[..., :S].float()

    qr = qkv.float().detach().requires_grad_(True)
    q, k, v = qr.split(H, dim=-1)

    def shape(t):
        return t.view(B, S, NH, 64).transpose(1, 2)

    scores = torch.matmul(shape(q), shape(k).transpose(-1, -2)) / 8.0
    key_pad = torch.arange(S, device=DEV).unsqueeze(0) >= seqlens.unsqueeze(1)
    scores = scores.masked_fill(key_pad[:, None, None, :], -10000.0)
    probs = torch.softmax(scores, dim=-1) * keep / (1 - p_q)
    out_ref = (
        torch.matmul(probs, shape(v)).transpose(1, 2).reshape(B, S, H)
    )
    assert rel_err(out, out_ref) < 3e-2

    dout = torch.randn_like(out_ref) * 0.5
    out_ref.backward(dout)
    dqkv = ext().attention_bwd(
        dout.half(), qkv, seqlens, out, lse, dmask, NH, p, 77, 5
    )
    assert rel_err(dqkv, qr.grad) < 6e-2


def test_attention_bwd_loss_scale_linearity_fp16():
    """A loss-scaled dout must scale dqkv linearly and stay finite: this
    catches a narrowing to fp16 in the wrong place on the dS path."""
    torch.manual_seed(22)
    B, S, NH = 2, 128, 4
    H = NH * 64
    qkv = (torch.randn(B, S, 3 * H, device=DEV) * 0.5).half()
    seqlens = torch.randint(S // 2, S + 1, (B,), device=DEV, dtype=torch.int32)
    dout = (torch.randn(B, S, H, device=DEV) * 0.5).half()
    out, lse, m = ext().attention_fwd(qkv, seqlens, NH, 0.0, 0, 0)
    d1 = ext().attention_bwd(dout, qkv, seqlens, out, lse, m, NH, 0.0, 0, 0)
    d2 = ext().attention_bwd(
        dout * 1024, qkv, seqlens, out, lse, m, NH, 0.0, 0, 0
    )
    assert torch.isfinite(d2.float()).all()
    assert rel_err(d2, d1.float() * 1024) < 1e-2


def test_mixed_dtype_operands_raise():
    torch.manual_seed(23)
    B, S, NH = 1, 16, 2
    H = NH * 64
    qkv = (torch.randn(B, S, 3 * H, device=DEV) * 0.5).half()
    seqlens = torch.full((B,), S, device=DEV, dtype=torch.int32)
    out, lse, m = ext().attention_fwd(qkv, seqlens, NH, 0.0, 0, 0)
    dout = torch.randn(B, S, H, device=DEV).bfloat16()
    with pytest.raises(RuntimeError, match="BFloat16.*Half"):
        ext().attention_bwd(dout, qkv, seqlens, out, lse, m, NH, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="BFloat16.*Half"):
        ext().attention_bwd(
            dout.half(), qkv, seqlens, out.bfloat16(), lse, m, NH, 0.0, 0, 0
        )
    dy = torch.randn(256, 128, device=DEV, dtype=F16)
    x = torch.randn(256, 128, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="BFloat16.*Half"):
        ext().wgrad_tn(dy, x)


def test_attention_bwd_operand_checks_raise():
    """Malformed operands of the padded backward are rejected on the host,
    naming the operand; nothing is launched (dqkv is never allocated)."""
    torch.manual_seed(23)
    B, S, NH = 1, 16, 2
    H = NH * 64
    p = 0.1
    qkv = (torch.randn(B, S, 3 * H, device=DEV) * 0.5).half()
    seqlens = torch.full((B,), S, device=DEV, dtype=torch.int32)
    out, lse, m = ext().attention_fwd(qkv, seqlens, NH, 0.0, 0, 0)
    _o, _l, dmask = ext().attention_fwd(qkv, seqlens, NH, p, 77, 5)
    dout = torch.randn(B, S, H, device=DEV).half()

    def bwd(out=out, lse=lse, mask=m, seqlens=seqlens, p=0.0):
        return ext().attention_bwd(
            dout, qkv, seqlens, out, lse, mask, NH, p, 77, 5
        )

    bwd()  # the well-formed call goes through
    bwd(mask=dmask, p=p)
    with pytest.raises(RuntimeError, match="attn_bwd: lse dtype BFloat16"):
        bwd(lse=lse.bfloat16())
    with pytest.raises(RuntimeError, match="attn_bwd: lse must be"):
        bwd(lse=lse[:, :-1])
    with pytest.raises(RuntimeError, match="attn_bwd: keep-mask must be"):
        bwd(mask=dmask.flatten()[:-1], p=p)
    wide = torch.zeros(B, S, 2 * H, device=DEV, dtype=F16)
    out_view = wide[:, :, :H]
    assert out_view.shape == out.shape and not out_view.is_contiguous()
    with pytest.raises(RuntimeError, match="attn_bwd: out must be contig"):
        bwd(out=out_view)
    longer = torch.full((B + 1,), S, device=DEV, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="attn_bwd: seqlens must have"):
        bwd(seqlens=longer)


def test_attention_fwd_seqlens_length_raises():
    B, S, NH = 1, 16, 2
    qkv = torch.zeros(B, S, 3 * NH * 64, device=DEV, dtype=F16)
    longer = torch.full((B + 1,), S, device=DEV, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="attn_fwd: seqlens must have"):
        ext().attention_fwd(qkv, longer, NH, 0.0, 0, 0)


# ---------------------------------------------------------------------------
# split-K MFMA wgrad GEMM
# ---------------------------------------------------------------------------
@pytest.mark.parametrize(
    "K,M,N",
    [
        (384, 128, 128),    # minimal tile
        (4100, 256, 128),   # K not a multiple of the k-step: zero-pad tail
    ],
)
@pytest.mark.parametrize("bk", [32, 64])
def test_wgrad_tn_parity_fp16(K, M, N, bk, monkeypatch):
    monkeypatch.setenv("BPA_WGRAD_BK", str(bk))
    torch.manual_seed(K + M + N)
    dy = torch.randn(K, M, device=DEV, dtype=F16)
    x = torch.randn(K, N, device=DEV, dtype=F16)
    assert ext().wgrad_tn_supported(K, M, N)
    out = ext().wgrad_tn(dy, x)
    assert out.dtype == F16
    ref_fp32 = dy.float().t() @ x.float()
    assert rel_err(out, ref_fp32) < 1e-2, rel_err(out, ref_fp32)


def test_wgrad_tn_overflow_rounds_to_inf_fp16():
    """The final fp32 -> fp16 cast must give +inf beyond the fp16 range
    (a GradScaler detects overflow by looking for inf; a saturated
    finite value would corrupt training silently), and must be exact
    just below it."""
    K, M, N = 256, 128, 128
    dy = torch.full((K, M), 16.0, device=DEV, dtype=F16)
    x = torch.full((K, N), 16.0, device=DEV, dtype=F16)
    out = ext().wgrad_tn(dy, x)  # true result 65536 everywhere
    assert torch.equal(out, torch.full_like(out, float("inf")))
    out = ext().wgrad_tn(dy, x * 0.5)  # true result 32768 everywhere
    assert torch.equal(out, torch.full_like(out, 32768.0))


@pytest.mark.parametrize("with_bias", [False, True])
def test_wgrad_routes_in_linear_fp16(with_bias, monkeypatch):
    """linear_nobias / fused_linear backward on fp16 inputs go through
    wgrad_tn ([4096,1024] x [1024,1024] is the smallest shape
    wgrad_tn_profitable admits) and match eager F.linear."""
    counts = _count_calls(monkeypatch, "wgrad_tn")
    torch.manual_seed(0)
    x = torch.randn(4096, 1024, device=DEV, dtype=F16, requires_grad=True)
    w = torch.randn(1024, 1024, device=DEV, dtype=F16, requires_grad=True)
    b = (
        torch.randn(1024, device=DEV, dtype=F16, requires_grad=True)
        if with_bias
        else None
    )
    y = ops.fused_linear(x, w, b) if with_bias else ops.linear_nobias(x, w)
    gy = torch.randn_like(y)
    y.backward(gy)
    assert counts["wgrad_tn"] == 1
    x2 = x.detach().clone().requires_grad_(True)
    w2 = w.detach().clone().requires_grad_(True)
    b2 = b.detach().clone() if with_bias else None
    torch.nn.functional.linear(x2, w2, b2).backward(gy)
    assert w.grad.dtype == F16
    assert rel_err(w.grad, w2.grad.float()) < 1e-2
    assert rel_err(x.grad, x2.grad.float()) < 1e-2


# ---------------------------------------------------------------------------
# fused MLM decoder GEMM + bias + cross-entropy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize(
    "P,V,K",
    [
        (128, 4096, 256),   # small, V % 128 == 0
        (200, 1000, 128),   # row padding + vocab tail tile
    ],
)
def test_mlm_head_fwd_kernel_fp16(P, V, K):
    torch.manual_seed(11)
    p_pad = ((P + 255) // 256) * 256
    h = (torch.randn(p_pad, K, device=DEV) * 0.5).half()
    w = (torch.randn(V, K, device=DEV) * 0.05).half()
    b = torch.randn(V, device=DEV) * 0.1
    labels = torch.randint(0, V, (p_pad,), device=DEV)
    labels[::5] = -1
    labels[P:] = -1
    logits, loss_sum, count, lse = ext().mlm_head_fwd(h, w, b, labels, -1)
    assert logits.dtype == F16
    # GEMM + bias parity vs the library path at the same (fp16) precision
    ref_logits = (h.float() @ w.float().t() + b).half()
    assert rel_err(logits, ref_logits) < 2e-2
    # CE statistics computed from the fp16-rounded logits
    ref_lse = torch.logsumexp(ref_logits.float(), dim=-1)
    assert rel_err(lse, ref_lse) < 1e-3
    valid = labels != -1
    ref_loss = (
        ref_lse[valid]
        - ref_logits.float()[valid].gather(1, labels[valid, None]).squeeze(1)
    ).sum()
    assert float(count) == int(valid.sum())
    assert abs(float(loss_sum) - float(ref_loss)) / max(
        abs(float(ref_loss)), 1.0
    ) < 1e-3


def test_mlm_decoder_loss_autograd_fp16(monkeypatch):
    counts = _count_calls(monkeypatch, "mlm_head_fwd")
    torch.manual_seed(12)
    P, V, K = 200, 1000, 128
    h = (torch.randn(P, K, device=DEV) * 0.5).half().requires_grad_(True)
    w = (torch.randn(V, K, device=DEV) * 0.05).half().requires_grad_(True)
    b = (torch.randn(V, device=DEV) * 0.1).requires_grad_(True)
    labels = torch.randint(0, V, (P,), device=DEV)
    labels[::3] = -1

    hr = h.detach().float().requires_grad_(True)
    wr = w.detach().float().requires_grad_(True)
    br = b.detach().float().requires_grad_(True)
    loss_ref = ref.cross_entropy(
        torch.nn.functional.linear(hr, wr, br), labels, -1
    )
    loss_ref.backward()

    loss = ops.mlm_decoder_loss(h, w, b, labels)
    assert counts["mlm_head_fwd"] == 1, "fp16 must take the fused kernel"
    assert loss.dim() == 0
    assert abs(float(loss) - float(loss_ref)) < 3e-2
    loss.backward()
    assert h.grad.dtype == F16 and w.grad.dtype == F16
    assert rel_err(h.grad, hr.grad) < 3e-2
    assert rel_err(w.grad, wr.grad) < 3e-2
    assert rel_err(b.grad, br.grad) < 3e-2


def test_mlm_decoder_loss_all_ignored_fp16():
    h = torch.randn(128, 256, device=DEV).half()
    w = torch.randn(512, 256, device=DEV).half()
    b = torch.zeros(512, device=DEV)
    labels = torch.full((128,), -1, device=DEV, dtype=torch.long)
    assert float(ops.mlm_decoder_loss(h, w, b, labels)) == 0.0


# ---------------------------------------------------------------------------
# end to end: fp16 autocast + GradScaler reaches the native kernels
# ---------------------------------------------------------------------------
def test_model_step_fp16(monkeypatch):
    """The tiny model of test_model_step_bf16 under fp16 autocast with a
    GradScaler trains, and does so THROUGH the MFMA kernels (no silent
    eager fallback).

    The scaler starts at 2**10 instead of its default 2**16: with only
    8 steps there is no room for the default's halve-on-overflow warm-up
    (each overflowed step is skipped), and 2**10 keeps every scaled
    gradient of this model far inside the fp16 range (|dlogits| <=
    2**10 / 64 valid rows) while still lifting the smallest ones out of
    the subnormals. Overflow-to-inf itself is covered by
    test_wgrad_tn_overflow_rounds_to_inf_fp16."""
    from bert_pytorch_amd.config import BertConfig
    from bert_pytorch_amd.models import (
        BertForPreTraining,
        BertPretrainingCriterion,
    )
    from bert_pytorch_amd.optim import FusedLAMB

    counts = _count_calls(
        monkeypatch, "attention_fwd", "attention_bwd", "mlm_head_fwd"
    )
    torch.manual_seed(14)
    config = BertConfig(
        vocab_size_or_config_json_file=2048, hidden_size=256,
        num_hidden_layers=2, num_attention_heads=4,
        intermediate_size=512, max_position_embeddings=128,
    )
    model = BertForPreTraining(config).to(DEV)
    criterion = BertPretrainingCriterion(config.vocab_size)
    opt = FusedLAMB(model.parameters(), lr=1e-3)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0**10)
    losses = []
    ids = torch.randint(0, 2048, (8, 128), device=DEV)
    tt = torch.zeros_like(ids)
    mask = torch.ones_like(ids)
    labels = torch.full_like(ids, -1)
    labels[:, 4:12] = ids[:, 4:12]
    nsp = torch.randint(0, 2, (8,), device=DEV)
    for _ in range(8):
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.float16):
            # compute_mlm_loss=True is the runner's path: the decoder
            # GEMM + CE go through ops.mlm_decoder_loss
            scores, rel, gl = model(
                ids, tt, mask, masked_lm_labels=labels, compute_mlm_loss=True
            )
            loss = criterion(scores, rel, gl, nsp)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        losses.append(float(loss))
    assert all(l == l for l in losses), f"NaN loss: {losses}"
    assert losses[-1] < losses[0], f"loss did not drop: {losses}"
    for name, n in counts.items():
        assert n >= 1, f"{name} was never called under fp16 autocast"
