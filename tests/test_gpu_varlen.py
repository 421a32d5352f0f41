"""Variable-length (packed) attention kernels, row pack/unpack kernels
and the unpadded model path vs the eager fp32 composites and the padded
kernels. Bounds are the padded attention tests' rel_err bounds
(tests/test_gpu_kernels.py, tests/test_gpu_fp16_kernels.py: 3e-2
forward, 6e-2 backward, for bf16 and fp16 alike). All tests
@pytest.mark.gpu."""

import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bert_pytorch_amd import ops
    from bert_pytorch_amd.ops import _reference as ref

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
FWD_TOL, BWD_TOL = 3e-2, 6e-2


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


def _cu(lengths):
    cu = [0]
    for n in lengths:
        cu.append(cu[-1] + n)
    return cu


def _t_pad(total):
    return -(-total // 128) * 128


# (lengths, max_seqlen): odd lengths, row bases off any 16-row boundary,
# a key-tile edge (64/65) and a query-tile edge (129); and an empty
# sequence between two short ones
CASES = {
    "edges": ((1, 17, 64, 65, 129, 200), 200),
    "empty": ((5, 0, 33), 48),
}
NH = 2
H = NH * 64


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    """Inputs (rounded to ``dtype``) and the per-sequence fp32 eager
    reference, computed once and shared; nothing here is modified."""
    lengths, max_seqlen = CASES[name]
    cu = _cu(lengths)
    total, t_pad = cu[-1], _t_pad(cu[-1])
    gen = torch.Generator(device=DEV).manual_seed(100 + len(lengths))
    qkv = (torch.randn(t_pad, 3 * H, device=DEV, generator=gen) * 0.5).to(dtype)
    dout = (torch.randn(t_pad, H, device=DEV, generator=gen) * 0.5).to(dtype)
    out_ref = torch.zeros(t_pad, H, device=DEV)
    dqkv_ref = torch.zeros(t_pad, 3 * H, device=DEV)
    for s, e in zip(cu[:-1], cu[1:]):
        if e == s:
            continue
        x = qkv[s:e].float().unsqueeze(0).requires_grad_(True)
        lens = torch.tensor([e - s], device=DEV, dtype=torch.int32)
        o = ref.attention(x, lens, NH, 0.0, False)
        o.backward(dout[s:e].float().unsqueeze(0))
        out_ref[s:e] = o[0].detach()
        dqkv_ref[s:e] = x.grad[0]
    cu_t = torch.tensor(cu, device=DEV, dtype=torch.int32)
    return dict(lengths=lengths, max_seqlen=max_seqlen, cu=cu, cu_t=cu_t,
                total=total, t_pad=t_pad, qkv=qkv, dout=dout,
                out_ref=out_ref, dqkv_ref=dqkv_ref)


def _run(c, qkv=None, dout=None, p=0.0, seed=0, offset=0):
    qkv = c["qkv"] if qkv is None else qkv
    dout = c["dout"] if dout is None else dout
    out, lse, dmask = ext().attention_varlen_fwd(
        qkv, c["cu_t"], c["max_seqlen"], NH, p, seed, offset
    )
    dqkv = ext().attention_varlen_bwd(
        dout, qkv, c["cu_t"], c["max_seqlen"], out, lse, dmask, NH, p,
        seed, offset,
    )
    return out, lse, dmask, dqkv


# ---------------------------------------------------------------------------
# forward and backward vs the fp32 eager reference, per sequence
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_varlen_forward_backward_per_sequence(name, dtype):
    c = _case(name, dtype)
    if name == "edges":
        assert c["total"] == 476 and c["t_pad"] == 512
    out, lse, _m, dqkv = _run(c)
    assert out.dtype == dtype and dqkv.dtype == dtype
    assert out.shape == (c["t_pad"], H) and dqkv.shape == (c["t_pad"], 3 * H)
    assert lse.shape == (len(c["lengths"]) * NH, c["max_seqlen"])
    for b, (s, e) in enumerate(zip(c["cu"][:-1], c["cu"][1:])):
        if e == s:
            continue
        ef = rel_err(out[s:e], c["out_ref"][s:e])
        eb = rel_err(dqkv[s:e], c["dqkv_ref"][s:e])
        print(f"{name} {dtype} seq {b} len {e - s}: fwd {ef:.3e} bwd {eb:.3e}")
        assert ef < FWD_TOL, (b, e - s, ef)
        assert eb < BWD_TOL, (b, e - s, eb)
        # lse against the eager log-sum-exp of the scaled scores
        x = c["qkv"][s:e].float()
        q = x[:, :H].view(-1, NH, 64).transpose(0, 1)
        k = x[:, H:2 * H].view(-1, NH, 64).transpose(0, 1)
        lse_ref = torch.logsumexp(q @ k.transpose(-1, -2) / 8.0, dim=-1)
        got = lse.view(-1, NH, c["max_seqlen"])[b, :, : e - s]
        assert rel_err(got, lse_ref) < 1e-2


# ---------------------------------------------------------------------------
# tail rows and isolation between sequences
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_varlen_tail_is_zero_and_never_read(dtype):
    c = _case("edges", dtype)
    total = c["total"]
    qkv = c["qkv"].clone()
    dout = c["dout"].clone()
    qkv[total:] = float("nan")
    dout[total:] = float("nan")
    out, lse, _m, dqkv = _run(c, qkv, dout)
    assert torch.isfinite(out[:total].float()).all()
    assert torch.isfinite(dqkv[:total].float()).all()
    lse3 = lse.view(-1, NH, c["max_seqlen"])
    for b, n in enumerate(c["lengths"]):
        assert torch.isfinite(lse3[b, :, :n]).all()
    assert (out[total:] == 0).all()
    assert (dqkv[total:] == 0).all()
    # same valid rows as the run with a finite tail, bit for bit
    out0, _l, _m0, dqkv0 = _run(c)
    assert torch.equal(out[:total], out0[:total])
    assert torch.equal(dqkv[:total], dqkv0[:total])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_varlen_sequences_are_isolated(dtype):
    c = _case("edges", dtype)
    out0, _l, _m, dqkv0 = _run(c)
    victim = 3  # the 65-row sequence: rows 82..146, both neighbours odd
    s, e = c["cu"][victim], c["cu"][victim + 1]
    qkv = c["qkv"].clone()
    gen = torch.Generator(device=DEV).manual_seed(5)
    qkv[s:e] = (torch.randn(e - s, 3 * H, device=DEV, generator=gen) * 3).to(dtype)
    out1, _l1, _m1, dqkv1 = _run(c, qkv)
    assert not torch.equal(out1[s:e], out0[s:e])
    for lo, hi in ((0, s), (e, c["t_pad"])):
        assert torch.equal(out1[lo:hi], out0[lo:hi])
        assert torch.equal(dqkv1[lo:hi], dqkv0[lo:hi])


# ---------------------------------------------------------------------------
# dropout
# ---------------------------------------------------------------------------
def _padded_from_packed(x, cu, seq):
    """[T_pad, W] packed -> [B, seq, W] padded with zero rows."""
    out = x.new_zeros(len(cu) - 1, seq, x.shape[-1])
    for b, (s, e) in enumerate(zip(cu[:-1], cu[1:])):
        out[b, : e - s] = x[s:e]
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_varlen_dropout_mask_and_numerics(dtype):
    torch.manual_seed(21)
    lengths, S = (128, 77), 128
    B = len(lengths)
    cu = _cu(lengths)
    total, t_pad = cu[-1], _t_pad(cu[-1])
    p = 0.1
    p_q = round(p * 256) / 256  # the kernel's 8-bit-quantized drop prob
    qkv = (torch.randn(t_pad, 3 * H, device=DEV) * 0.5).to(dtype)
    cu_t = torch.tensor(cu, device=DEV, dtype=torch.int32)
    seqlens = torch.tensor(lengths, device=DEV, dtype=torch.int32)

    out, lse, dmask = ext().attention_varlen_fwd(qkv, cu_t, S, NH, p, 77, 5)
    qkv_pad = _padded_from_packed(qkv, cu, S)
    _o, _l, dmask_pad = ext().attention_fwd(qkv_pad, seqlens, NH, p, 77, 5)
    assert dmask.shape == dmask_pad.shape
    assert torch.equal(dmask, dmask_pad)

    # eager reference conditioned on the stored keep-mask (bit-packed
    # [B*NH, S, ceil(S/32)] int32, LSB-first)
    bits = dmask.view(torch.uint8).reshape(B, NH, S, -1).int()
    shifts = torch.arange(8, device=DEV, dtype=torch.int32)
    keep = ((bits.unsqueeze(-1) >> shifts) & 1).reshape(B, NH, S, -1)
    keep = keep[..., :S].float()

    qr = qkv_pad.float().detach().requires_grad_(True)
    q, k, v = qr.split(H, dim=-1)

    def shape(t):
        return t.view(B, S, NH, 64).transpose(1, 2)

    scores = torch.matmul(shape(q), shape(k).transpose(-1, -2)) / 8.0
    key_pad = torch.arange(S, device=DEV).unsqueeze(0) >= seqlens.unsqueeze(1)
    scores = scores.masked_fill(key_pad[:, None, None, :], -10000.0)
    probs = torch.softmax(scores, dim=-1) * keep / (1 - p_q)
    out_ref = torch.matmul(probs, shape(v)).transpose(1, 2).reshape(B, S, H)

    dout = (torch.randn(t_pad, H, device=DEV) * 0.5).to(dtype)
    dout[total:] = 0
    out_ref.backward(_padded_from_packed(dout, cu, S).float())
    dqkv = ext().attention_varlen_bwd(
        dout, qkv, cu_t, S, out, lse, dmask, NH, p, 77, 5
    )
    for b, (s, e) in enumerate(zip(cu[:-1], cu[1:])):
        ef = rel_err(out[s:e], out_ref.detach()[b, : e - s])
        eb = rel_err(dqkv[s:e], qr.grad[b, : e - s])
        print(f"dropout {dtype} seq {b}: fwd {ef:.3e} bwd {eb:.3e}")
        assert ef < FWD_TOL
        assert eb < BWD_TOL


# ---------------------------------------------------------------------------
# agreement with the padded kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_varlen_agrees_with_padded_kernel(dtype):
    torch.manual_seed(22)
    lengths, S = (48, 16, 128, 96), 128
    cu = _cu(lengths)
    total, t_pad = cu[-1], _t_pad(cu[-1])
    qkv = (torch.randn(t_pad, 3 * H, device=DEV) * 0.5).to(dtype)
    dout = (torch.randn(t_pad, H, device=DEV) * 0.5).to(dtype)
    dout[total:] = 0
    cu_t = torch.tensor(cu, device=DEV, dtype=torch.int32)
    seqlens = torch.tensor(lengths, device=DEV, dtype=torch.int32)

    out, lse, m = ext().attention_varlen_fwd(qkv, cu_t, S, NH, 0.0, 0, 0)
    dqkv = ext().attention_varlen_bwd(
        dout, qkv, cu_t, S, out, lse, m, NH, 0.0, 0, 0
    )
    qkv_pad = _padded_from_packed(qkv, cu, S)
    out_p, lse_p, m_p = ext().attention_fwd(qkv_pad, seqlens, NH, 0.0, 0, 0)
    dqkv_p = ext().attention_bwd(
        _padded_from_packed(dout, cu, S), qkv_pad, seqlens, out_p, lse_p,
        m_p, NH, 0.0, 0, 0,
    )
    bitwise = True
    for b, (s, e) in enumerate(zip(cu[:-1], cu[1:])):
        n = e - s
        assert rel_err(out[s:e], out_p[b, :n]) < FWD_TOL
        assert rel_err(dqkv[s:e], dqkv_p[b, :n]) < BWD_TOL
        bitwise &= torch.equal(out[s:e], out_p[b, :n])
        bitwise &= torch.equal(dqkv[s:e], dqkv_p[b, :n])
    print(f"varlen vs padded kernel, {dtype}: bitwise equal = {bitwise}")


# ---------------------------------------------------------------------------
# pack_rows / unpack_rows on device
# ---------------------------------------------------------------------------
def _holed_mask():
    gen = torch.Generator().manual_seed(9)
    mask = (torch.rand(3, 48, generator=gen) < 0.6).long()
    mask[1, :5] = 0      # left padding
    mask[2, 40:] = 0     # right padding
    return mask.to(DEV)


@pytest.mark.parametrize(
    "dtype", [torch.bfloat16, torch.float16, torch.float32],
    ids=["bf16", "fp16", "fp32"],
)
@pytest.mark.parametrize("hidden", [64, 1024])
def test_pack_unpack_rows_kernels(hidden, dtype):
    torch.manual_seed(hidden)
    mask = _holed_mask()
    rows = mask.numel()
    dest, _cu_t, total, t_pad = ops.unpad_index(mask)
    assert 0 < total < rows and t_pad == 128
    keep = mask.reshape(-1).bool()
    idx = dest[keep].long()
    x = torch.randn(rows, hidden, device=DEV).to(dtype)

    packed = ext().pack_rows(x, dest, t_pad)
    want = torch.zeros(t_pad, hidden, device=DEV, dtype=dtype)
    want.index_copy_(0, idx, x[keep])
    assert packed.dtype == dtype and torch.equal(packed, want)
    assert (packed[total:] == 0).all()
    assert torch.equal(packed, ext().pack_rows(x, dest, t_pad))

    y = torch.randn(t_pad, hidden, device=DEV).to(dtype)
    unpacked = ext().unpack_rows(y, dest, rows)
    want = torch.zeros(rows, hidden, device=DEV, dtype=dtype)
    want[keep] = y.index_select(0, idx)
    assert unpacked.dtype == dtype and torch.equal(unpacked, want)
    assert (unpacked[~keep] == 0).all()
    assert torch.equal(unpacked, ext().unpack_rows(y, dest, rows))

    # autograd: each op's backward is the other op
    xg = x.float().requires_grad_(True) if dtype == torch.float32 else None
    if xg is not None:
        g = torch.randn(t_pad, hidden, device=DEV)
        (gx,) = torch.autograd.grad(ops.pack_rows(xg, dest, t_pad), xg, g)
        assert torch.equal(gx, ext().unpack_rows(g, dest, rows))


# ---------------------------------------------------------------------------
# model: routing and a training step
# ---------------------------------------------------------------------------
def _small_model(p_drop):
    from bert_pytorch_amd.config import BertConfig
    from bert_pytorch_amd.models import BertForPreTraining

    config = BertConfig(
        vocab_size_or_config_json_file=512, hidden_size=128,
        num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
        max_position_embeddings=64, hidden_dropout_prob=p_drop,
        attention_probs_dropout_prob=p_drop,
    )
    return BertForPreTraining(config), config


def _batch(device):
    gen = torch.Generator().manual_seed(17)
    lengths, S = [48, 19, 1], 48
    ids = torch.randint(0, 512, (3, S), generator=gen)
    tt = torch.zeros_like(ids)
    tt[0, 24:] = 1
    mask = (torch.arange(S)[None, :] < torch.tensor(lengths)[:, None]).long()
    labels = torch.full_like(ids, -1)
    labels[:, 0] = ids[:, 0]
    labels[0, 5:40:5] = ids[0, 5:40:5]
    labels[1, 3:19:4] = ids[1, 3:19:4]
    nsp = torch.tensor([0, 1, 1])
    return [t.to(device) for t in (ids, tt, mask, labels, nsp)]


def _step(model, criterion, batch, autocast):
    ids, tt, mask, labels, nsp = batch
    model.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        scores, rel, gl = model(ids, tt, mask, masked_lm_labels=labels)
        loss = criterion(scores, rel, gl, nsp)
    loss.backward()
    return loss.detach().float(), {
        n: p.grad.detach().float().clone()
        for n, p in model.named_parameters() if p.grad is not None
    }


def test_unpadded_model_routes_to_varlen_kernels(monkeypatch):
    from bert_pytorch_amd.models import BertPretrainingCriterion

    counts = _count_calls(
        monkeypatch, "attention_varlen_fwd", "attention_varlen_bwd",
        "attention_fwd", "attention_bwd", "pack_rows", "unpack_rows",
    )
    torch.manual_seed(30)
    model, config = _small_model(0.1)
    model = model.to(DEV).train()
    model.unpad_inputs(True)
    criterion = BertPretrainingCriterion(config.vocab_size)
    loss, _g = _step(model, criterion, _batch(DEV), autocast=True)
    assert bool(torch.isfinite(loss))
    assert counts["attention_varlen_fwd"] == 2   # one per layer
    assert counts["attention_varlen_bwd"] == 2
    assert counts["attention_fwd"] == 0 and counts["attention_bwd"] == 0
    # pack + unpack forward, and each one's backward is the other
    assert counts["pack_rows"] == 2 and counts["unpack_rows"] == 2


def test_unpadded_model_step_matches_padded(monkeypatch):
    """bf16-autocast step, dropout off: loss and every parameter
    gradient of the unpadded and of the padded model are each compared
    with the fp32 eager model (a CPU copy). The unpadded error may be at
    most 1.5x the padded path's error plus 1e-3 absolute slack."""
    from bert_pytorch_amd.models import BertPretrainingCriterion

    counts = _count_calls(monkeypatch, "attention_fwd", "attention_varlen_fwd")
    torch.manual_seed(31)
    eager, config = _small_model(0.0)
    eager = eager.train()
    criterion = BertPretrainingCriterion(config.vocab_size)
    padded = copy.deepcopy(eager).to(DEV)
    unpadded = copy.deepcopy(eager).to(DEV)
    unpadded.unpad_inputs(True)

    ids, tt, mask, labels, nsp = _batch("cpu")
    scores, rel, gl = eager(ids, tt, mask, masked_lm_labels=labels)
    loss_ref = criterion(scores, rel, gl, nsp)
    loss_ref.backward()
    loss_ref = loss_ref.detach()
    grads_ref = {n: p.grad for n, p in eager.named_parameters()
                 if p.grad is not None}

    batch = _batch(DEV)
    loss_p, grads_p = _step(padded, criterion, batch, autocast=True)
    loss_u, grads_u = _step(unpadded, criterion, batch, autocast=True)
    assert set(grads_u) == set(grads_p) == set(grads_ref)
    # each model took its own path: one forward launch per layer
    assert counts == {"attention_fwd": 2, "attention_varlen_fwd": 2}

    err_p = abs(float(loss_p) - float(loss_ref))
    err_u = abs(float(loss_u) - float(loss_ref))
    print(f"loss: eager {float(loss_ref):.6f} padded err {err_p:.3e} "
          f"unpadded err {err_u:.3e}")
    failures = []
    if err_u > 1.5 * err_p + 1e-3:
        failures.append(("loss", err_u, err_p))
    for name, g_ref in grads_ref.items():
        g_ref = g_ref.to(DEV)
        e_p = float((grads_p[name] - g_ref).abs().max())
        e_u = float((grads_u[name] - g_ref).abs().max())
        print(f"{name}: |g|max {float(g_ref.abs().max()):.3e} "
              f"padded err {e_p:.3e} unpadded err {e_u:.3e}")
        if e_u > 1.5 * e_p + 1e-3:
            failures.append((name, e_u, e_p))
    assert not failures, failures


def test_unpadded_steps_bitwise_repeatable_with_dropout():
    from bert_pytorch_amd.models import BertPretrainingCriterion
    from bert_pytorch_amd.ops import rng

    def run():
        torch.manual_seed(32)
        rng.reset(32)
        model, config = _small_model(0.1)
        model = model.to(DEV).train()
        model.unpad_inputs(True)
        criterion = BertPretrainingCriterion(config.vocab_size)
        return _step(model, criterion, _batch(DEV), autocast=True)

    loss1, grads1 = run()
    loss2, grads2 = run()
    assert bool(torch.isfinite(loss1))
    assert torch.equal(loss1, loss2)
    for name in grads1:
        assert torch.equal(grads1[name], grads2[name]), name
