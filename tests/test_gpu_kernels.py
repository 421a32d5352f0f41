"""HIP kernel numerics: every gfx950 kernel vs the eager fp32 reference
(the same composites the CPU path runs). All tests @pytest.mark.gpu."""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bert_pytorch_amd import ops
    from bert_pytorch_amd.ops import _reference as ref

DEV = "cuda:0"


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    a = a.float()
    b = b.float()
    denom = b.abs().max().clamp(min=1e-3)
    return float((a - b).abs().max() / denom)


def ext():
    return ops.extension()


# ---------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(128, 1024), (777, 1024), (64, 4096)])
def test_ln_forward(dtype, shape):
    torch.manual_seed(0)
    x = torch.randn(shape, device=DEV, dtype=dtype)
    w = torch.randn(shape[1], device=DEV) * 0.1 + 1.0
    b = torch.randn(shape[1], device=DEV) * 0.1
    y, mean, rstd = ext().ln_fwd(x, w, b, 1e-12)
    y_ref = ref.layer_norm(x.float(), w, b, 1e-12)
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert rel_err(y, y_ref) < tol


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ln_backward(dtype):
    torch.manual_seed(1)
    rows, H = 512, 1024
    x = torch.randn(rows, H, device=DEV, dtype=dtype)
    w = (torch.randn(H, device=DEV) * 0.1 + 1.0).requires_grad_(True)
    b = (torch.randn(H, device=DEV) * 0.1).requires_grad_(True)
    xr = x.float().detach().requires_grad_(True)
    y_ref = ref.layer_norm(xr, w, b, 1e-12)
    dy = torch.randn_like(y_ref)
    y_ref.backward(dy)

    _, mean, rstd = ext().ln_fwd(x, w.detach(), b.detach(), 1e-12)
    dx, dw, db = ext().ln_bwd(dy.to(dtype), x, w.detach(), mean, rstd)
    tol = 1e-4 if dtype == torch.float32 else 3e-2
    assert rel_err(dx, xr.grad) < tol
    assert rel_err(dw, w.grad) < tol
    assert rel_err(db, b.grad) < tol


# ---------------------------------------------------------------------------
# bias + GELU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bias_gelu(dtype):
    torch.manual_seed(2)
    rows, H = 512, 4096
    x = torch.randn(rows, H, device=DEV, dtype=dtype)
    bias = torch.randn(H, device=DEV, requires_grad=True)
    xr = x.float().detach().requires_grad_(True)
    y_ref = ref.bias_gelu(xr, bias)
    dy = torch.randn_like(y_ref)
    y_ref.backward(dy)

    y = ext().bias_gelu_fwd(x, bias.detach())
    dx, db = ext().bias_gelu_bwd(dy.to(dtype), x, bias.detach())
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert rel_err(y, y_ref) < tol
    assert rel_err(dx, xr.grad) < (1e-4 if dtype == torch.float32 else 3e-2)
    assert rel_err(db, bias.grad) < (1e-4 if dtype == torch.float32 else 3e-2)


# ---------------------------------------------------------------------------
# fused bias+dropout+residual+LN
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bdrl_no_dropout(dtype):
    torch.manual_seed(3)
    rows, H = 512, 1024
    x = torch.randn(rows, H, device=DEV, dtype=dtype)
    res = torch.randn(rows, H, device=DEV, dtype=dtype)
    bias = torch.randn(H, device=DEV, requires_grad=True)
    w = (torch.randn(H, device=DEV) * 0.1 + 1.0).requires_grad_(True)
    lb = (torch.randn(H, device=DEV) * 0.1).requires_grad_(True)
    xr = x.float().detach().requires_grad_(True)
    rr = res.float().detach().requires_grad_(True)
    y_ref = ref.bias_dropout_residual_ln(xr, bias, rr, w, lb, 0.0, False)
    dy = torch.randn_like(y_ref)
    y_ref.backward(dy)

    y, z, mask, mean, rstd = ext().bias_dropout_residual_ln_fwd(
        x, bias.detach(), res, w.detach(), lb.detach(), 0.0, 1e-12, 0, 0
    )
    assert rel_err(y, y_ref) < (1e-5 if dtype == torch.float32 else 2e-2)
    dx, db, dres, dw, dlb = ext().bias_dropout_residual_ln_bwd(
        dy.to(dtype), z, mask, w.detach(), mean, rstd, 0.0, True
    )
    tol = 1e-4 if dtype == torch.float32 else 3e-2
    assert rel_err(dx, xr.grad) < tol
    assert rel_err(dres, rr.grad) < tol
    assert rel_err(db, bias.grad) < tol
    assert rel_err(dw, w.grad) < tol
    assert rel_err(dlb, lb.grad) < tol


def test_bdrl_dropout_self_consistent():
    """With p>0: y must equal LN(mask*(x+b)/(1-p)+res) for the returned
    mask, drop fraction ~= p, and backward consistent with the mask."""
    torch.manual_seed(4)
    rows, H, p = 1024, 1024, 0.3
    x = torch.randn(rows, H, device=DEV, dtype=torch.bfloat16)
    res = torch.randn(rows, H, device=DEV, dtype=torch.bfloat16)
    bias = torch.randn(H, device=DEV)
    w = torch.randn(H, device=DEV) * 0.1 + 1.0
    lb = torch.randn(H, device=DEV) * 0.1
    y, z, mask, mean, rstd = ext().bias_dropout_residual_ln_fwd(
        x, bias, res, w, lb, p, 1e-12, 12345, 7
    )
    frac = float(mask.float().mean())
    assert abs(frac - (1 - p)) < 0.01
    # recompute with the mask through the fp32 composite
    keep = mask.float()
    z_ref = keep * (x.float() + bias) / (1 - p) + res.float()
    assert rel_err(z, z_ref) < 2e-2
    y_ref = ref.layer_norm(z_ref, w, lb, 1e-12)
    assert rel_err(y, y_ref) < 3e-2


# ---------------------------------------------------------------------------
# embedding + LN + dropout
# ---------------------------------------------------------------------------
def test_embedding_fwd_bwd():
    torch.manual_seed(5)
    B, S, H, V, P, T = 8, 128, 1024, 1000, 512, 2
    ids = torch.randint(0, V, (B, S), device=DEV)
    tt = torch.randint(0, T, (B, S), device=DEV)
    word = torch.randn(V, H, device=DEV, requires_grad=True)
    pos = torch.randn(P, H, device=DEV, requires_grad=True)
    tok = torch.randn(T, H, device=DEV, requires_grad=True)
    w = (torch.randn(H, device=DEV) * 0.1 + 1.0).requires_grad_(True)
    lb = (torch.randn(H, device=DEV) * 0.1).requires_grad_(True)

    y_ref = ref.embedding_ln_dropout(ids, tt, word, pos, tok, w, lb, 0.0, False)
    dy = torch.randn_like(y_ref)
    y_ref.backward(dy)

    y, z, mask, mean, rstd = ext().embedding_ln_dropout_fwd(
        ids, tt, word.detach(), pos.detach(), tok.detach(), w.detach(),
        lb.detach(), 0.0, 1e-12, 0, 0, torch.float32,
    )
    assert rel_err(y, y_ref) < 1e-4
    d_word, d_pos, d_tok, dw, dlb = ext().embedding_ln_dropout_bwd(
        dy, ids, tt, z, mask, w.detach(), mean, rstd, 0.0, V, P, T
    )
    assert rel_err(d_word, word.grad) < 1e-3
    assert rel_err(d_pos, pos.grad) < 1e-3
    assert rel_err(d_tok, tok.grad) < 1e-3
    assert rel_err(dw, w.grad) < 1e-3
    assert rel_err(dlb, lb.grad) < 1e-3


def _ids_from_counts(counts, rows, gen):
    """Ids with the given multiplicities, shuffled over `rows` positions."""
    flat = torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in counts])
    assert flat.numel() == rows
    return flat[torch.randperm(rows, generator=gen)]


def _embedding_id_cases():
    # rows = 5 * 61 = 305 = 19 blocks of kWordRows (16) sorted positions + 1.
    # After the kernel's stable sort the runs of "edges" lie as follows:
    #   id 3   x16  positions   0-15   exactly block 0 (head, ends at edge)
    #   id 7   x5   positions  16-20   from a block's start, ends inside
    #   id 9   x1   position   21      interior single (direct store)
    #   id 11  x75  positions  22-96   from mid block 1 over blocks 2-5
    #                                  (whole-block pieces) into block 6
    #   id 20  x15  positions  97-111  from inside block 6 to its edge
    #   id 21  x32  positions 112-143  exactly blocks 7 and 8
    #   ids 30-141  singles   144-255  block starts/ends as single runs
    #   id 900 x49  positions 256-304  blocks 16-18 and the one-row last
    #                                  block: reaches the last position
    rows = 305
    edges = [(3, 16), (7, 5), (9, 1), (11, 75), (20, 15), (21, 32)]
    edges += [(30 + i, 1) for i in range(112)] + [(900, 49)]
    # benchmark-like: 15 % one id ([MASK]), 1 per sequence another ([CLS])
    masky = [(103, 46), (101, 5)] + [(200 + i, 1) for i in range(254)]
    return {"edges": edges, "one_id": [(999, rows)], "mask_heavy": masky}


@pytest.mark.parametrize("case", ["edges", "one_id", "mask_heavy"])
def test_embedding_bwd_repeated_ids(case):
    """Word-embedding gradient with runs of one id that cross the sorted
    16-row blocks of the ordered scatter (whole-block runs, runs ending on
    a block edge, a run reaching the last position), against the fp32
    autograd composite, and bitwise equal between two launches.

    Bound 1e-3 as in test_embedding_fwd_bwd: same reference, and the
    longest sum here (305 fp32 terms, error <= 305 * 2^-24 of the sum of
    magnitudes) stays far inside it."""
    B, S, H, V, P, T = 5, 61, 1024, 1000, 64, 2
    gen = torch.Generator().manual_seed(55)
    ids = _ids_from_counts(_embedding_id_cases()[case], B * S, gen)
    ids = ids.view(B, S).to(DEV)
    torch.manual_seed(6)
    tt = torch.randint(0, T, (B, S), device=DEV)
    word = torch.randn(V, H, device=DEV, requires_grad=True)
    pos = torch.randn(P, H, device=DEV, requires_grad=True)
    tok = torch.randn(T, H, device=DEV, requires_grad=True)
    w = (torch.randn(H, device=DEV) * 0.1 + 1.0).requires_grad_(True)
    lb = (torch.randn(H, device=DEV) * 0.1).requires_grad_(True)
    y_ref = ref.embedding_ln_dropout(ids, tt, word, pos, tok, w, lb, 0.0, False)
    dy = torch.randn_like(y_ref)
    y_ref.backward(dy)

    y, z, mask, mean, rstd = ext().embedding_ln_dropout_fwd(
        ids, tt, word.detach(), pos.detach(), tok.detach(), w.detach(),
        lb.detach(), 0.0, 1e-12, 0, 0, torch.float32,
    )
    outs = [
        ext().embedding_ln_dropout_bwd(
            dy, ids, tt, z, mask, w.detach(), mean, rstd, 0.0, V, P, T
        )
        for _ in range(2)
    ]
    d_word, d_pos, d_tok, dw, dlb = outs[0]
    assert rel_err(d_word, word.grad) < 1e-3
    # rows of ids that do not occur stay exactly zero
    absent = torch.ones(V, dtype=torch.bool, device=DEV)
    absent[ids.view(-1)] = False
    assert float(d_word[absent].abs().max()) == 0.0
    assert rel_err(d_tok, tok.grad) < 1e-3
    assert rel_err(d_pos, pos.grad) < 1e-3
    assert rel_err(dw, w.grad) < 1e-3
    assert rel_err(dlb, lb.grad) < 1e-3
    for a, b in zip(*outs):
        assert torch.equal(a, b), "two launches differ bitwise"


# ---------------------------------------------------------------------------
# ordered column reduce (many partial rows) and ordered norm reductions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize(
    "rows,H",
    [
        (1573, 1028),  # 50 partials: 2 chunks of 32, last short; 2nd strip 4 cols
        (4160, 2048),  # 130 partials: 5 chunks, two full strips
        (16500, 1028),  # 516 partials: 17 chunks, more than one fold batch (16)
    ],
)
def test_col_sum_ordered_reduce(rows, H):
    """col_sum through the one-launch ordered column reduce (more than 48
    partial rows): every column within the fp32 summation bound
    rows * 2^-24 * sum|x| of the fp64 sum, and bitwise equal between two
    launches."""
    torch.manual_seed(20)
    x = torch.randn(rows, H, device=DEV)
    a = ext().col_sum(x)
    b = ext().col_sum(x)
    ref64 = x.double().sum(0)
    bound = rows * 2.0 ** -24 * x.double().abs().sum(0)
    assert a.shape == (H,)
    assert bool(((a.double() - ref64).abs() <= bound).all())
    assert torch.equal(a, b), "two launches differ bitwise"


def test_ln_backward_many_rows_repeatable():
    """LayerNorm backward at a row count whose dgamma/dbeta partials take
    the ordered column reduce (2000 rows -> 125 partial rows)."""
    torch.manual_seed(21)
    rows, H = 2000, 1024
    x = torch.randn(rows, H, device=DEV)
    w = (torch.randn(H, device=DEV) * 0.1 + 1.0).requires_grad_(True)
    b = (torch.randn(H, device=DEV) * 0.1).requires_grad_(True)
    xr = x.detach().clone().requires_grad_(True)
    y_ref = ref.layer_norm(xr, w, b, 1e-12)
    dy = torch.randn_like(y_ref)
    y_ref.backward(dy)
    _, mean, rstd = ext().ln_fwd(x, w.detach(), b.detach(), 1e-12)
    o1 = ext().ln_bwd(dy, x, w.detach(), mean, rstd)
    o2 = ext().ln_bwd(dy, x, w.detach(), mean, rstd)
    # kernel and reference both sum `rows` fp32 terms per column, each
    # within rows * 2^-24 * sum|term| of the exact sum; the normalised x
    # in dgamma's terms carries a few more ulps, hence 2^-22 in all
    xhat = (x - x.mean(1, keepdim=True)) * torch.rsqrt(
        x.var(1, unbiased=False, keepdim=True) + 1e-12)
    bound_b = rows * 2.0 ** -22 * dy.abs().sum(0)
    bound_g = rows * 2.0 ** -22 * (dy * xhat).abs().sum(0)
    assert bool(((o1[2] - b.grad).abs() <= bound_b).all())
    assert bool(((o1[1] - w.grad).abs() <= bound_g).all())
    for t1, t2 in zip(o1, o2):
        assert torch.equal(t1, t2), "two launches differ bitwise"


def test_l2norm_sq_ordered():
    """Global grad-norm^2 over tensors of 4, 2, 1 and 1 chunks (64Ki
    elements each): within n * 2^-24 of the fp64 value, bitwise equal
    between two launches."""
    torch.manual_seed(22)
    ts = [torch.randn(n, device=DEV) for n in (200_000, 70_000, 5, 65_536)]
    a = ext().multi_tensor_l2norm_sq(ts)
    b = ext().multi_tensor_l2norm_sq(ts)
    want = sum(float((t.double() ** 2).sum()) for t in ts)
    n = sum(t.numel() for t in ts)
    assert abs(float(a) - want) <= n * 2.0 ** -24 * want
    assert torch.equal(a, b), "two launches differ bitwise"


def test_fused_lamb_repeatable():
    """Two FusedLAMB runs from equal states end bitwise equal; the
    (30528, 8) tensor spans 4 chunks, so its trust-ratio norms are folded
    from several per-chunk partials."""
    from bert_pytorch_amd.optim import FusedLAMB

    shapes = [(128, 128), (1024,), (30528, 8), (7,)]
    torch.manual_seed(23)
    init = [torch.randn(s, device=DEV) for s in shapes]
    grads = [torch.randn(s, device=DEV) for s in shapes]
    results = []
    for _ in range(2):
        params = [p.clone().requires_grad_(True) for p in init]
        opt = FusedLAMB(params, lr=1e-2, weight_decay=0.01)
        for step in range(3):
            for p, g in zip(params, grads):
                p.grad = (g * (step + 1)).clone()
            opt.step()
        results.append([p.detach().clone() for p in params])
    for p1, p2, p0 in zip(results[0], results[1], init):
        assert not torch.equal(p1, p0)
        assert torch.equal(p1, p2), "two runs differ bitwise"


# ---------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cross_entropy(dtype):
    torch.manual_seed(6)
    N, V = 512, 30528
    logits = (torch.randn(N, V, device=DEV) * 3).to(dtype)
    labels = torch.randint(0, V, (N,), device=DEV)
    labels[::3] = -1  # ignored rows
    lr = logits.float().detach().requires_grad_(True)
    loss_ref = ref.cross_entropy(lr, labels, -1)
    loss_ref.backward()

    loss = ops.fused_cross_entropy(logits.requires_grad_(True), labels, -1)
    assert abs(float(loss) - float(loss_ref)) < (
        1e-4 if dtype == torch.float32 else 3e-2
    )
    loss.backward()
    assert rel_err(logits.grad, lr.grad) < (
        1e-4 if dtype == torch.float32 else 3e-2
    )


def test_cross_entropy_all_ignored():
    logits = torch.randn(16, 128, device=DEV)
    labels = torch.full((16,), -1, device=DEV, dtype=torch.long)
    loss = ops.fused_cross_entropy(logits, labels, -1)
    assert float(loss) == 0.0


# ---------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,S,NH", [(4, 128, 16), (2, 512, 16), (3, 128, 4), (3, 80, 4)])
def test_attention_forward(B, S, NH):
    torch.manual_seed(7)
    H = NH * 64
    qkv = (torch.randn(B, S, 3 * H, device=DEV) * 0.5).bfloat16()
    seqlens = torch.randint(S // 2, S + 1, (B,), device=DEV, dtype=torch.int32)
    out, lse, _mask = ext().attention_fwd(qkv, seqlens, NH, 0.0, 0, 0)
    out_ref = ref.attention(qkv.float(), seqlens, NH, 0.0, False)
    assert rel_err(out, out_ref) < 3e-2


def test_attention_forward_spike():
    """Online-softmax max tracking: one huge key must not break numerics
    (guide rule 26: force the rescale path)."""
    torch.manual_seed(8)
    B, S, NH = 2, 128, 4
    H = NH * 64
    qkv = (torch.randn(B, S, 3 * H, device=DEV) * 0.3)
    # spike a late key so the running max jumps at the last tile
    qkv[:, S - 3, H : 2 * H] += 40.0
    qkv = qkv.bfloat16()
    seqlens = torch.full((B,), S, device=DEV, dtype=torch.int32)
    out, _, _m = ext().attention_fwd(qkv, seqlens, NH, 0.0, 0, 0)
    out_ref = ref.attention(qkv.float(), seqlens, NH, 0.0, False)
    assert torch.isfinite(out.float()).all()
    assert rel_err(out, out_ref) < 5e-2


@pytest.mark.parametrize("B,S,NH", [(4, 128, 8), (2, 512, 4), (3, 80, 4)])
def test_attention_backward(B, S, NH):
    torch.manual_seed(9)
    H = NH * 64
    qkv = (torch.randn(B, S, 3 * H, device=DEV) * 0.5).bfloat16()
    seqlens = torch.randint(S // 2, S + 1, (B,), device=DEV, dtype=torch.int32)
    qr = qkv.float().detach().requires_grad_(True)
    out_ref = ref.attention(qr, seqlens, NH, 0.0, False)
    dout = (torch.randn_like(out_ref) * 0.5)
    out_ref.backward(dout)

    out, lse, _mask = ext().attention_fwd(qkv, seqlens, NH, 0.0, 0, 0)
    dqkv = ext().attention_bwd(
        dout.bfloat16(), qkv, seqlens, out, lse, _mask, NH, 0.0, 0, 0
    )
    assert rel_err(dqkv, qr.grad) < 6e-2


def test_attention_dropout_stats_and_determinism():
    torch.manual_seed(10)
    B, S, NH, p = 2, 128, 4, 0.5
    H = NH * 64
    qkv = (torch.randn(B, S, 3 * H, device=DEV) * 0.5).bfloat16()
    seqlens = torch.full((B,), S, device=DEV, dtype=torch.int32)
    o1, l1, _m1 = ext().attention_fwd(qkv, seqlens, NH, p, 99, 1)
    o2, l2, _m2 = ext().attention_fwd(qkv, seqlens, NH, p, 99, 1)
    assert torch.equal(o1, o2), "same philox state must reproduce"
    o3, _, _m3 = ext().attention_fwd(qkv, seqlens, NH, p, 99, 2)
    assert not torch.equal(o1, o3), "different offset must differ"
    # dropped-mean check: E[out_p] == out_0 within tolerance
    o0, _, _m0 = ext().attention_fwd(qkv, seqlens, NH, 0.0, 0, 0)
    acc = torch.zeros_like(o0, dtype=torch.float32)
    n = 32
    for i in range(n):
        oi, _, _mi = ext().attention_fwd(qkv, seqlens, NH, p, 1234, 100 + i * 10**7)
        acc += oi.float()
    mean = acc / n
    err = (mean - o0.float()).abs().mean() / o0.float().abs().mean()
    assert err < 0.2, f"dropout mean deviates: {err}"
    # backward runs and is finite
    dq = ext().attention_bwd(
        qkv[..., : H].contiguous(), qkv, seqlens, o1, l1, _m1, NH, p, 99, 1
    )
    assert torch.isfinite(dq.float()).all()


# ---------------------------------------------------------------------------
# multi-tensor optimizers
# ---------------------------------------------------------------------------
def _rand_tensors(seed, shapes):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.randn(s, generator=g, device=DEV) for s in shapes]


def test_l2norm_and_clip():
    shapes = [(1000,), (37, 55), (256, 256), (3,)]
    grads = _rand_tensors(11, shapes)
    expected = torch.sqrt(sum(g.pow(2).sum() for g in grads))
    gsq = ext().multi_tensor_l2norm_sq(grads)
    assert abs(float(gsq.sqrt()) - float(expected)) / float(expected) < 1e-5
    ext().multi_tensor_clip_scale(grads, gsq, 1.0)
    after = torch.sqrt(sum(g.pow(2).sum() for g in grads))
    assert abs(float(after) - 1.0) < 1e-4


def test_fused_lamb_matches_eager():
    from bert_pytorch_amd.optim import FusedLAMB

    shapes = [(128, 128), (1024,), (30528, 8), (7,)]
    torch.manual_seed(12)
    params_g = [torch.randn(s, device=DEV) for s in shapes]
    params_c = [p.clone() for p in params_g]
    grads = [torch.randn(s, device=DEV) for s in shapes]

    def build(params):
        opt = FusedLAMB(
            [
                {"params": params[:2], "weight_decay": 0.01},
                {"params": params[2:], "weight_decay": 0.0},
            ],
            lr=1e-2,
        )
        return opt

    opt_native = build([p.requires_grad_(True) for p in params_g])
    opt_eager = build([p.requires_grad_(True) for p in params_c])
    for step in range(5):
        for p, pc, g in zip(params_g, params_c, grads):
            p.grad = (g * (step + 1)).clone()
            pc.grad = (g * (step + 1)).clone()
        opt_native.step()
        os.environ["BPA_FORCE_EAGER"] = "1"
        try:
            opt_eager.step()
        finally:
            del os.environ["BPA_FORCE_EAGER"]
    for p, pc in zip(params_g, params_c):
        assert rel_err(p, pc) < 1e-4, "HIP LAMB diverges from eager LAMB"


def test_fused_adam_matches_eager():
    from bert_pytorch_amd.optim import FusedAdam

    torch.manual_seed(13)
    shapes = [(333,), (64, 64)]
    params_g = [torch.randn(s, device=DEV).requires_grad_(True) for s in shapes]
    params_c = [p.detach().clone().requires_grad_(True) for p in params_g]
    opt_n = FusedAdam(params_g, lr=1e-2, weight_decay=0.01)
    opt_e = FusedAdam(params_c, lr=1e-2, weight_decay=0.01)
    for step in range(5):
        g = [torch.randn(s, device=DEV) for s in shapes]
        for p, pc, gi in zip(params_g, params_c, g):
            p.grad = gi.clone()
            pc.grad = gi.clone()
        opt_n.step()
        os.environ["BPA_FORCE_EAGER"] = "1"
        try:
            opt_e.step()
        finally:
            del os.environ["BPA_FORCE_EAGER"]
    for p, pc in zip(params_g, params_c):
        assert rel_err(p, pc) < 1e-4


# ---------------------------------------------------------------------------
# end-to-end on GPU
# ---------------------------------------------------------------------------
def test_model_step_bf16():
    from bert_pytorch_amd.config import BertConfig
    from bert_pytorch_amd.models import (
        BertForPreTraining,
        BertPretrainingCriterion,
    )
    from bert_pytorch_amd.optim import FusedLAMB

    torch.manual_seed(14)
    config = BertConfig(
        vocab_size_or_config_json_file=2048, hidden_size=256,
        num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
        max_position_embeddings=128,
    )
    model = BertForPreTraining(config).to(DEV)
    criterion = BertPretrainingCriterion(config.vocab_size)
    opt = FusedLAMB(model.parameters(), lr=1e-3)
    losses = []
    ids = torch.randint(0, 2048, (8, 128), device=DEV)
    tt = torch.zeros_like(ids)
    mask = torch.ones_like(ids)
    labels = torch.full_like(ids, -1)
    labels[:, 4:12] = ids[:, 4:12]
    nsp = torch.randint(0, 2, (8,), device=DEV)
    for _ in range(8):
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            scores, rel, gl = model(ids, tt, mask, masked_lm_labels=labels)
            loss = criterion(scores, rel, gl, nsp)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(l == l for l in losses), f"NaN loss: {losses}"
    assert losses[-1] < losses[0], f"loss did not drop: {losses}"


def test_train_steps_bitwise_repeatable():
    """Two trainings from one seed (dropout on, 1024 rows so that the
    bias/LayerNorm gradients take the ordered column reduce, repeated
    ids, three LAMB updates) end with bitwise equal losses and
    parameters."""
    from bert_pytorch_amd.config import BertConfig
    from bert_pytorch_amd.models import (
        BertForPreTraining,
        BertPretrainingCriterion,
    )
    from bert_pytorch_amd.ops import rng
    from bert_pytorch_amd.optim import FusedLAMB

    def run():
        torch.manual_seed(31)
        rng.reset(31)
        config = BertConfig(
            vocab_size_or_config_json_file=2048, hidden_size=256,
            num_hidden_layers=2, num_attention_heads=4,
            intermediate_size=512, max_position_embeddings=128,
        )
        model = BertForPreTraining(config).to(DEV)
        criterion = BertPretrainingCriterion(config.vocab_size)
        opt = FusedLAMB(model.parameters(), lr=1e-3)
        ids = torch.randint(0, 2048, (8, 128), device=DEV)
        ids[:, 20:40] = 103  # a long run of one id for the sorted scatter
        tt = torch.zeros_like(ids)
        tt[:, 64:] = 1
        mask = torch.ones_like(ids)
        labels = torch.full_like(ids, -1)
        labels[:, 20:40] = torch.randint(0, 2048, (8, 20), device=DEV)
        nsp = torch.randint(0, 2, (8,), device=DEV)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                scores, rel, gl = model(ids, tt, mask, masked_lm_labels=labels)
                loss = criterion(scores, rel, gl, nsp)
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
        return losses, [p.detach().clone() for p in model.parameters()]

    l1, p1 = run()
    l2, p2 = run()
    assert all(bool(torch.isfinite(l)) for l in l1)
    for a, b in zip(l1, l2):
        assert torch.equal(a, b), "losses differ between two runs"
    for a, b in zip(p1, p2):
        assert torch.equal(a, b), "parameters differ between two runs"


def test_gpu_matches_cpu_forward():
    """Same weights/input: GPU HIP path vs CPU eager path agree."""
    from bert_pytorch_amd.config import BertConfig
    from bert_pytorch_amd.models import BertForPreTraining

    torch.manual_seed(15)
    config = BertConfig(
        vocab_size_or_config_json_file=1024, hidden_size=128,
        num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
        max_position_embeddings=64,
    )
    model = BertForPreTraining(config).eval()
    ids = torch.randint(0, 1024, (2, 64))
    mask = torch.ones_like(ids)
    mask[:, 50:] = 0
    tt = torch.zeros_like(ids)
    with torch.no_grad():
        s_cpu, r_cpu = model(ids, tt, mask)
    model_gpu = model.to(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        s_gpu, r_gpu = model_gpu(ids.to(DEV), tt.to(DEV), mask.to(DEV))
    assert rel_err(s_gpu[:, :50], s_cpu[:, :50].to(DEV)) < 0.08


# ---------------------------------------------------------------------------
# column sum + fused linear (packed-QKV bias-grad path)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(128, 1024), (1000, 3072)])
def test_col_sum(dtype, shape):
    torch.manual_seed(0)
    x = torch.randn(shape, device=DEV, dtype=dtype)
    out = ext().col_sum(x)
    ref_out = x.float().sum(dim=0)
    assert rel_err(out, ref_out) < (1e-5 if dtype == torch.float32 else 2e-2)


def test_fused_linear_matches_flinear():
    from bert_pytorch_amd.ops import fused_linear

    torch.manual_seed(0)
    x = torch.randn(64, 8, 256, device=DEV, requires_grad=True)
    w = torch.randn(768, 256, device=DEV, requires_grad=True)
    b = torch.randn(768, device=DEV, requires_grad=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = fused_linear(x, w, b)
        y.float().pow(2).mean().backward()
    gx, gw, gb = x.grad.clone(), w.grad.clone(), b.grad.clone()
    x.grad = w.grad = b.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y2 = torch.nn.functional.linear(x, w, b)
        y2.float().pow(2).mean().backward()
    assert rel_err(y, y2) < 1e-6
    assert rel_err(gx, x.grad) < 2e-2
    assert rel_err(gw, w.grad) < 2e-2
    assert rel_err(gb, b.grad) < 2e-2


def test_fused_linear_pure_bf16():
    from bert_pytorch_amd.ops import fused_linear

    torch.manual_seed(0)
    x = torch.randn(32, 128, device=DEV, dtype=torch.bfloat16,
                    requires_grad=True)
    w = torch.randn(64, 128, device=DEV, dtype=torch.bfloat16,
                    requires_grad=True)
    b = torch.randn(64, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    y = fused_linear(x, w, b)
    y.float().sum().backward()
    assert b.grad.dtype == torch.bfloat16
    assert rel_err(b.grad, torch.full_like(b, 32.0)) < 2e-2


# ---------------------------------------------------------------------------
# optimizer master-weight path + K-FAC on device
# ---------------------------------------------------------------------------
def test_fused_lamb_master_weights_native():
    """Native (HIP) LAMB with bf16 params + fp32 masters matches the
    fp32-params run step-for-step (same update in fp32 master space)."""
    from bert_pytorch_amd.optim import FusedLAMB

    torch.manual_seed(0)
    w0 = torch.randn(64, 64, device=DEV)
    # run A: fp32 params
    pa = torch.nn.Parameter(w0.clone())
    oa = FusedLAMB([pa], lr=1e-2)
    # run B: bf16 params + masters
    pb = torch.nn.Parameter(w0.clone().to(torch.bfloat16))
    ob = FusedLAMB([pb], lr=1e-2, master_weights=True)
    for i in range(4):
        g = torch.randn(64, 64, device=DEV)
        pa.grad = g.clone()
        pb.grad = g.to(torch.bfloat16)
        oa.step()
        ob.step()
    master = ob.state[pb]["master"]
    # master tracks the fp32 trajectory up to bf16-grad rounding
    assert rel_err(master, pa.detach()) < 5e-2
    assert torch.equal(pb.data, master.to(torch.bfloat16))


def test_fused_adam_master_weights_native():
    from bert_pytorch_amd.optim import FusedAdam

    torch.manual_seed(1)
    p = torch.nn.Parameter(torch.randn(128, device=DEV, dtype=torch.bfloat16))
    opt = FusedAdam([p], lr=1e-2, master_weights=True)
    for _ in range(3):
        p.grad = torch.randn(128, device=DEV, dtype=torch.bfloat16)
        opt.step()
    st = opt.state[p]
    assert st["master"].dtype == torch.float32
    assert st["exp_avg"].dtype == torch.float32
    assert torch.equal(p.data, st["master"].to(torch.bfloat16))


def test_kfac_gpu_step():
    """K-FAC factor accumulation + damped eigh inverse + precondition on
    the GPU (tiny BERT)."""
    from bert_pytorch_amd.config import BertConfig
    from bert_pytorch_amd.models import (
        BertForPreTraining,
        BertPretrainingCriterion,
    )
    from bert_pytorch_amd.optim.kfac import KFAC

    torch.manual_seed(0)
    config = BertConfig(
        vocab_size_or_config_json_file=256, hidden_size=64,
        num_hidden_layers=2, num_attention_heads=4,
        intermediate_size=128, max_position_embeddings=64,
    )
    model = BertForPreTraining(config).to(DEV)
    criterion = BertPretrainingCriterion(config.vocab_size)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    kfac = KFAC(model, optimizer=opt, inv_update_interval=2)
    ids = torch.randint(0, 256, (4, 32), device=DEV)
    mask = torch.ones_like(ids)
    labels = torch.full((4, 32), -1, dtype=torch.long, device=DEV)
    labels[:, 3:6] = 7
    nsp = torch.zeros(4, dtype=torch.long, device=DEV)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            s, r, gl = model(ids, None, mask, masked_lm_labels=labels)
            loss = criterion(s, r, gl, nsp)
        loss.backward()
        kfac.step()
        opt.step()
        losses.append(float(loss))
    assert all(v == v for v in losses), "NaN loss"
    assert losses[-1] < losses[0]
    assert any(st.A_inv is not None for st in kfac.layers)


# ---------------------------------------------------------------------------
# fused FFN (hipBLASLt GELU epilogues)
# ---------------------------------------------------------------------------
def test_fused_ffn_matches_eager():
    from bert_pytorch_amd.ops import fused_ffn
    from bert_pytorch_amd.ops.ffn import ffn_supported

    if not ffn_supported(torch.zeros(1, device=DEV)):
        pytest.skip("hipBLASLt build lacks GELU_AUX_BIAS/DGELU_BGRAD")

    torch.manual_seed(11)
    M, H, F = 512, 1024, 4096
    x = torch.randn(M, H, device=DEV, requires_grad=True)
    w1 = (torch.randn(F, H, device=DEV) * 0.02).requires_grad_(True)
    b1 = torch.randn(F, device=DEV, requires_grad=True)
    w2 = (torch.randn(H, F, device=DEV) * 0.02).requires_grad_(True)

    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = fused_ffn(x, w1, b1, w2)
    dy = torch.randn_like(y.float())
    y.backward(dy.to(y.dtype))
    gx, gw1, gb1, gw2 = (t.grad.clone() for t in (x, w1, b1, w2))
    for t in (x, w1, b1, w2):
        t.grad = None

    # eager fp32 composite (exact-erf GELU; hipBLASLt uses the tanh
    # approximation - tolerances absorb the ~1e-3 difference)
    act = torch.nn.functional.gelu(x.float() @ w1.float().t() + b1.float())
    y_ref = act @ w2.float().t()
    y_ref.backward(dy)
    assert rel_err(y, y_ref) < 3e-2
    assert rel_err(gx, x.grad) < 4e-2
    assert rel_err(gw1, w1.grad) < 4e-2
    assert rel_err(gb1, b1.grad) < 4e-2
    assert rel_err(gw2, w2.grad) < 4e-2


def test_model_uses_fused_ffn_path():
    """BertLayer forward on device matches the CPU forward (takes the
    fused-FFN branch when the hipBLASLt build supports it)."""
    from bert_pytorch_amd.config import BertConfig
    from bert_pytorch_amd.models import BertForPreTraining

    torch.manual_seed(12)
    config = BertConfig(
        vocab_size_or_config_json_file=512, hidden_size=256,
        num_hidden_layers=2, num_attention_heads=4,
        intermediate_size=1024, max_position_embeddings=64,
    )
    model = BertForPreTraining(config).to(DEV).eval()
    ids = torch.randint(0, 512, (2, 32), device=DEV)
    mask = torch.ones_like(ids)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        scores, _ = model(ids, None, mask)
    cpu_model = BertForPreTraining(config).eval()
    cpu_model.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    with torch.no_grad():
        scores_cpu, _ = cpu_model(ids.cpu(), None, mask.cpu())
    assert rel_err(scores.cpu(), scores_cpu) < 5e-2


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,NH", [(2, 128, 4), (1, 512, 2)])
def test_attention_dropout_numerics(B, S, NH):
    """Forward AND backward with dropout must match an eager fp32
    reference conditioned on the kernel's own stored keep-mask (this is
    the regression test for the bwd mask-staging bug, where attn_bwd
    read an unwritten LDS tile when p > 0)."""
    torch.manual_seed(21)
    H = NH * 64
    p = 0.1
    p_q = round(p * 256) / 256  # the kernel's 8-bit-quantized drop prob
    qkv = (torch.randn(B, S, 3 * H, device=DEV) * 0.5).bfloat16()
    seqlens = torch.randint(S // 2, S + 1, (B,), device=DEV, dtype=torch.int32)

    out, lse, dmask = ext().attention_fwd(qkv, seqlens, NH, p, 77, 5)
    # dmask is bit-packed: [B*NH, S, ceil(S/32)] int32, LSB-first
    bits = dmask.view(torch.uint8).reshape(B, NH, S, -1).int()
    shifts = torch.arange(8, device=DEV, dtype=torch.int32)
    keep = ((bits.unsqueeze(-1) >> shifts) & 1).reshape(B, NH, S, -1)
    keep = keep[..., :S].float()
    # keep-rate sanity: mean within 3 sigma of 1 - p_q
    n = keep.numel()
    assert abs(keep.mean().item() - (1 - p_q)) < 4 * (p_q * (1 - p_q) / n) ** 0.5 + 1e-3

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
        dout.bfloat16(), qkv, seqlens, out, lse, dmask, NH, p, 77, 5
    )
    assert rel_err(dqkv, qr.grad) < 6e-2


# ---------------------------------------------------------------------------
# split-K MFMA wgrad GEMM (csrc/ops/wgrad.hip)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K,M,N", [
    (12288, 3072, 1024),   # QKV wgrad, phase 1
    (12288, 1024, 4096),   # FFN2 wgrad
    (8192, 4096, 1024),    # FFN1 wgrad, phase 2
    (8192, 1024, 1024),    # attn-out wgrad (splitk 8)
    (4100, 1024, 1024),    # K not a multiple of 64: zero-pad tail path
    (384, 128, 128),       # minimal tile
])
@pytest.mark.parametrize("bk", [32, 64])
def test_wgrad_tn_parity(K, M, N, bk, monkeypatch):
    monkeypatch.setenv("BPA_WGRAD_BK", str(bk))
    torch.manual_seed(K + M + N)
    dy = torch.randn(K, M, device=DEV, dtype=torch.bfloat16)
    x = torch.randn(K, N, device=DEV, dtype=torch.bfloat16)
    assert ext().wgrad_tn_supported(K, M, N)
    out = ext().wgrad_tn(dy, x)
    ref_fp32 = dy.float().t() @ x.float()
    # fp32 accumulation inside the kernel; only the final bf16 cast and
    # the split-K summation order differ from the fp32 reference
    assert rel_err(out, ref_fp32) < 1e-2, rel_err(out, ref_fp32)


def test_wgrad_routes_in_linear_nobias():
    """linear_nobias backward produces the same dW as eager F.linear."""
    torch.manual_seed(0)
    x = torch.randn(4096, 1024, device=DEV, dtype=torch.bfloat16,
                    requires_grad=True)
    w = torch.randn(1024, 1024, device=DEV, dtype=torch.bfloat16,
                    requires_grad=True)
    y = ops.linear_nobias(x, w)
    gy = torch.randn_like(y)
    y.backward(gy)
    x2 = x.detach().clone().requires_grad_(True)
    w2 = w.detach().clone().requires_grad_(True)
    torch.nn.functional.linear(x2, w2).backward(gy)
    assert rel_err(w.grad, w2.grad.float()) < 1e-2
    assert rel_err(x.grad, x2.grad.float()) < 1e-2


# ---------------------------------------------------------------------------
# fused MLM decoder GEMM + bias + cross-entropy (csrc/ops/mlm_head.hip)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize(
    "P,V,K",
    [
        (1280, 30528, 1024),  # phase-1/2 production shape (B*max_pred)
        (128, 4096, 256),     # small, V % 128 == 0
        (200, 1000, 128),     # row padding + vocab tail tile
    ],
)
def test_mlm_head_fwd_kernel(P, V, K):
    torch.manual_seed(11)
    p_pad = ((P + 255) // 256) * 256
    h = (torch.randn(p_pad, K, device=DEV) * 0.5).bfloat16()
    w = (torch.randn(V, K, device=DEV) * 0.05).bfloat16()
    b = torch.randn(V, device=DEV) * 0.1
    labels = torch.randint(0, V, (p_pad,), device=DEV)
    labels[::5] = -1
    labels[P:] = -1
    logits, loss_sum, count, lse = ext().mlm_head_fwd(h, w, b, labels, -1)
    # GEMM + bias parity vs the library path at the same (bf16) precision
    ref_logits = (h.float() @ w.float().t() + b).bfloat16()
    assert rel_err(logits, ref_logits) < 2e-2
    # CE statistics computed from the bf16-rounded logits
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


@pytest.mark.parametrize("P", [1280, 200])
def test_mlm_decoder_loss_autograd(P, monkeypatch):
    monkeypatch.setenv("BPA_FUSED_MLM", "1")  # the kernel path is opt-in
    torch.manual_seed(12)
    V, K = 30528, 1024
    h = (torch.randn(P, K, device=DEV) * 0.5).bfloat16().requires_grad_(True)
    w = (torch.randn(V, K, device=DEV) * 0.05).bfloat16().requires_grad_(True)
    b = (torch.randn(V, device=DEV) * 0.1).requires_grad_(True)
    labels = torch.randint(0, V, (P,), device=DEV)
    labels[::4] = -1

    hr = h.detach().float().requires_grad_(True)
    wr = w.detach().float().requires_grad_(True)
    br = b.detach().float().requires_grad_(True)
    loss_ref = ref.cross_entropy(
        torch.nn.functional.linear(hr, wr, br), labels, -1
    )
    loss_ref.backward()

    loss = ops.mlm_decoder_loss(h, w, b, labels)
    assert loss.dim() == 0
    assert abs(float(loss) - float(loss_ref)) < 3e-2
    loss.backward()
    assert rel_err(h.grad, hr.grad) < 3e-2
    assert rel_err(w.grad, wr.grad) < 3e-2
    assert rel_err(b.grad, br.grad) < 3e-2


def test_mlm_decoder_loss_all_ignored(monkeypatch):
    monkeypatch.setenv("BPA_FUSED_MLM", "1")
    h = torch.randn(128, 256, device=DEV).bfloat16()
    w = torch.randn(512, 256, device=DEV).bfloat16()
    b = torch.zeros(512, device=DEV)
    labels = torch.full((128,), -1, device=DEV, dtype=torch.long)
    assert float(ops.mlm_decoder_loss(h, w, b, labels)) == 0.0


# ---------------------------------------------------------------------------
# RCCL on-device smoke (the "nccl" backend on ROCm IS RCCL)
# ---------------------------------------------------------------------------
def test_rccl_collectives_on_device(monkeypatch):
    """RCCL init + all_reduce/broadcast/all_gather + a DDP-wrapped
    forward/backward on the MI355X. The pool leases single-GPU boxes
    (RCCL does not allow two ranks on one device), so this is world=1:
    it verifies the RCCL library loads, a communicator forms, and the
    exact collective calls the multi-GPU path issues execute on-device;
    multi-rank semantics are covered by the gloo world-2/4/8 suites
    (tests/test_distributed_cpu.py, test_distributed_runner.py) and the
    driver's round-end SCALE run."""
    import torch.distributed as dist

    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29531")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "1")
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        x = torch.arange(1024, device=DEV, dtype=torch.float32)
        dist.all_reduce(x)
        assert torch.equal(x, torch.arange(1024, device=DEV).float())
        dist.broadcast(x, src=0)
        out = [torch.empty_like(x)]
        dist.all_gather(out, x)
        assert torch.equal(out[0], x)

        m = torch.nn.Linear(64, 64).to(DEV)
        ddp = torch.nn.parallel.DistributedDataParallel(
            m, device_ids=[0], gradient_as_bucket_view=True
        )
        y = ddp(torch.randn(8, 64, device=DEV)).sum()
        y.backward()
        assert m.weight.grad is not None
        assert torch.isfinite(m.weight.grad).all()
    finally:
        dist.destroy_process_group()


def test_mlm_decoder_loss_fallback_matches_fused(monkeypatch):
    """BPA_FUSED_MLM=0 (library GEMM + fused-CE route) and the default
    in-repo fused kernel agree on loss and gradients."""
    torch.manual_seed(13)
    P, V, K = 512, 30528, 1024
    h = (torch.randn(P, K, device=DEV) * 0.5).bfloat16()
    w = (torch.randn(V, K, device=DEV) * 0.05).bfloat16()
    b = torch.randn(V, device=DEV) * 0.1
    labels = torch.randint(0, V, (P,), device=DEV)
    labels[::3] = -1

    results = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("BPA_FUSED_MLM", mode)
        hg = h.clone().requires_grad_(True)
        wg = w.clone().requires_grad_(True)
        bg = b.clone().requires_grad_(True)
        loss = ops.mlm_decoder_loss(hg, wg, bg, labels)
        loss.backward()
        results[mode] = (float(loss), hg.grad, wg.grad, bg.grad)

    assert abs(results["1"][0] - results["0"][0]) < 2e-2
    for i in (1, 2, 3):
        assert rel_err(results["1"][i], results["0"][i]) < 3e-2
