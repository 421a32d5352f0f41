"""One-pass LayerNorm-family backward (ln_bwd_rows_kernel, rowwise.h):
ln_bwd and bias_dropout_residual_ln_bwd ("bdrl_bwd") at the edges of the
row groups, at every width the multi-row core instantiates, and with the
second upstream gradient dy2. All tests @pytest.mark.gpu.

The reference is the fp64 LayerNorm backward formula at the operands the
kernel is handed; the bounds are those of test_gpu_rowwise_kernels.py:
  dx, dz_res   ulp_T * |ref| + 1e-4 * max|ref|
  dbeta, dbias rows * 2^-24 * sum|terms|
  dgamma       rows * 2^-22 * sum|terms|

Geometry (ln_bwd_rows in rowwise.h): a block has lanes = 512 / threads
row lanes (threads from launch_by_items; 1 lane from 512 threads up); a
lane takes max(2, ceil(ceil(rows / lanes) / 512)) rows, one per pass, and
the block writes one partial row; col_reduce_full folds nparts =
ceil(rows / rows_per_block) partial rows with one block up to 48 of them
and in 32-row chunks with a last-block fold above that. At H = 1024 the
16-bit types run 4 lanes of 128 threads (8 rows per block up to 4096
rows), fp32 2 lanes of 256 (4 rows per block up to 2048 rows).
"""

import pytest
import torch

import test_gpu_rowwise_kernels as rk
from test_gpu_rowwise_kernels import A_BWD, DEV, DT_IDS, DTYPES, F32, Acc, ext

pytestmark = pytest.mark.gpu

# rows at H = 1024       16-bit (4 lanes x 2 rows)        fp32 (2 lanes x 2 rows)
#    1  one block, one lane, one pass                same
#    3  one block, one pass, last lane idle          one block, second pass 1 row
#   37  5 parts, tail block 5 rows                   10 parts, tail 1 row
#  130  17 parts, tail 2 rows                        33 parts, tail 2 rows
#  192  24 parts                                     48 parts: last one-block fold
#  193  25 parts                                     49 parts: first chunked fold
#  384  48 parts: last one-block fold                96 parts: 3 full chunks
#  385  49 parts: chunks of 32 + 17                  97 parts
# 1031  129 parts, tail 7 rows (1031 is prime)       258 parts, tail 3 rows
# 4099  3 rows per lane: 342 blocks of 12, tail 7    5 rows per lane: 410 blocks
#       (4099 is prime)                              of 10, tail 9
ROWS = [1, 3, 37, 130, 192, 193, 384, 385, 1031, 4099]
H_EDGE = 1024

# one H per launch_by_items branch; rows 37 (two passes per lane, idle
# lanes in the tail block) and 1031 (prime; 3 rows per lane where the
# block is one lane, i.e. from 512 threads up)
WIDTHS_16 = [64, 768, 1024, 2056, 8200]
WIDTHS_32 = [64, 768, 1032, 4104]
WIDTH_ROWS = [37, 1031]


def _operands(rows, H, dtype, p, seed):
    """What the junction's forward hands its backward: z, the byte
    keep-mask, gamma and the fp32 mean/rstd of z; plus dy and dy2."""
    gamma, beta, _ = rk._params(H, seed)
    z = rk._randn(rows, H, dtype, seed + 1, shift=0.5)
    dy = rk._randn(rows, H, dtype, seed + 2)
    dy2 = rk._randn(rows, H, dtype, seed + 3)
    mu, rs = rk._stats64(z.double())
    g = torch.Generator(device=DEV).manual_seed(seed + 4)
    if p > 0:
        mask = (torch.rand(rows, H, device=DEV, generator=g) >= p).to(torch.uint8)
    else:
        mask = torch.empty(0, device=DEV, dtype=torch.uint8)
    return z, mask, gamma, mu.float(), rs.float(), dy, dy2


def _check_columns(acc, tag, rows, out_g, out_b, dg_r, db_r, abs_g, abs_b):
    acc.col(f"{tag} dgamma", out_g, dg_r, rows * 2.0 ** -22 * abs_g)
    acc.col(f"{tag} dbeta", out_b, db_r, rows * 2.0 ** -24 * abs_b)


def _check_ln(acc, dtype, rows, H, seed):
    z, _, gamma, mean, rstd, dy, _ = _operands(rows, H, dtype, 0.0, seed)
    o1 = ext().ln_bwd(dy, z, gamma, mean, rstd)
    o2 = ext().ln_bwd(dy, z, gamma, mean, rstd)
    dz_r, dg_r, db_r, abs_g, abs_b = rk._ln_backward_formula(
        z, dy, gamma, mean, rstd)
    acc.elem("ln dx", o1[0], dz_r, dtype, A_BWD)
    _check_columns(acc, "ln", rows, o1[1], o1[2], dg_r, db_r, abs_g, abs_b)
    rk._same(o1, o2)


def _check_bdrl(acc, dtype, rows, H, p, seed, with_dy2=False):
    """bdrl_bwd with and without the bias output, against fp64 at
    dy (+ dy2); returns the with-bias outputs."""
    tag = f"bdrl p{p}" + (" dy2" if with_dy2 else "")
    z, mask, gamma, mean, rstd, dy, dy2 = _operands(rows, H, dtype, p, seed)
    f = ext().bias_dropout_residual_ln_bwd
    extra = (dy2,) if with_dy2 else ()
    ob = f(dy, z, mask, gamma, mean, rstd, p, True, *extra)
    ob2 = f(dy, z, mask, gamma, mean, rstd, p, True, *extra)
    on = f(dy, z, mask, gamma, mean, rstd, p, False, *extra)
    on2 = f(dy, z, mask, gamma, mean, rstd, p, False, *extra)
    rk._same(ob, ob2)
    rk._same(on, on2)
    d64 = dy.double() + dy2.double() if with_dy2 else dy.double()
    dz_r, dg_r, db_r, abs_g, abs_b = rk._ln_backward_formula(
        z, d64, gamma, mean, rstd)
    dx_r = dz_r * mask.double() / (1.0 - p) if p > 0 else dz_r
    for name, o in (("bias", ob), ("nobias", on)):
        dx, dbias, dres, dgamma, dbeta = o
        acc.elem(f"{tag} {name} dres", dres, dz_r, dtype, A_BWD)
        acc.elem(f"{tag} {name} dx", dx, dx_r, dtype, A_BWD)
        _check_columns(acc, f"{tag} {name}", rows, dgamma, dbeta, dg_r, db_r,
                       abs_g, abs_b)
        if p > 0:
            assert float(dx[mask == 0].abs().max()) == 0.0
    # dx and dz_res do not depend on whether dbias is asked for
    assert torch.equal(ob[0], on[0]) and torch.equal(ob[2], on[2])
    assert on[1].numel() == 0
    # dbias is the column sum of the dx that is handed back
    dx64 = ob[0].double()
    acc.col(f"{tag} dbias", ob[1], dx64.sum(0),
            rows * 2.0 ** -24 * dx64.abs().sum(0))
    return ob


def _row_cases(rows_list):
    return [pytest.param(dt, r, id=f"{n}-rows{r}")
            for dt, n in zip(DTYPES, DT_IDS) for r in rows_list]


@pytest.mark.parametrize("dtype,rows", _row_cases(ROWS))
def test_row_group_edges(dtype, rows):
    acc = Acc("rowgroup", dtype)
    _check_ln(acc, dtype, rows, H_EDGE, rows)
    for p in (0.0, 0.1):
        _check_bdrl(acc, dtype, rows, H_EDGE, p, rows + 10)
    acc.done()


def _width_cases():
    out = []
    for dt, n in zip(DTYPES, DT_IDS):
        for H in (WIDTHS_32 if dt == F32 else WIDTHS_16):
            for r in WIDTH_ROWS:
                out.append(pytest.param(dt, H, r, id=f"{n}-H{H}-rows{r}"))
    return out


@pytest.mark.parametrize("dtype,H,rows", _width_cases())
def test_widths(dtype, H, rows):
    acc = Acc("width", dtype)
    _check_ln(acc, dtype, rows, H, H)
    for p in (0.0, 0.1):
        _check_bdrl(acc, dtype, rows, H, p, H + 10)
    acc.done()


@pytest.mark.parametrize("dtype,rows", _row_cases([3, 385, 4099]))
def test_dy2_sums_second_gradient(dtype, rows):
    """The kernel adds dy2 to dy in fp32 before anything else; reference:
    fp64 at dy.double() + dy2.double()."""
    acc = Acc("dy2", dtype)
    for p in (0.0, 0.1):
        _check_bdrl(acc, dtype, rows, H_EDGE, p, rows + 20, with_dy2=True)
    acc.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_dy2_none_omitted_and_zeros_agree(dtype):
    rows, p = 130, 0.1
    z, mask, gamma, mean, rstd, dy, _ = _operands(rows, H_EDGE, dtype, p, 7)
    f = ext().bias_dropout_residual_ln_bwd
    omitted = f(dy, z, mask, gamma, mean, rstd, p, True)
    none = f(dy, z, mask, gamma, mean, rstd, p, True, None)
    keyword = f(dy, z, mask, gamma, mean, rstd, p, True, dy2=None)
    zeros = f(dy, z, mask, gamma, mean, rstd, p, True, torch.zeros_like(dy))
    rk._same(omitted, none)
    rk._same(omitted, keyword)
    rk._same(omitted, zeros)


def test_dy2_rejects_mismatched_operand():
    xf, xb, v, st, _ = rk._rej_tensors()
    none = torch.empty(0, device=DEV, dtype=torch.uint8)
    f = ext().bias_dropout_residual_ln_bwd
    with pytest.raises(RuntimeError, match="dy2 dtype.*BFloat16.*Float"):
        f(xf, xf, none, v, st, st, 0.0, True, xb)
    with pytest.raises(RuntimeError, match="dy2 shape"):
        f(xf, xf, none, v, st, st, 0.0, True, xf[:-1])
    with pytest.raises(RuntimeError, match="dy2 must be contiguous"):
        f(xf, xf, none, v, st, st, 0.0, True, xf.t().contiguous().t())
    with pytest.raises(RuntimeError, match="dy2 device"):
        f(xf, xf, none, v, st, st, 0.0, True, xf.cpu())
    f(xf, xf, none, v, st, st, 0.0, True, xf)  # the well-formed call passes
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# model level: the forked junction outputs (BPA_JUNCTION_FORK)
# ---------------------------------------------------------------------------
def _tiny_step(dtype_autocast, dropout, checkpoint, seed=15):
    """One forward + backward of the 2-layer H=128 model of
    test_gpu_matches_cpu_forward; returns the loss and every gradient."""
    from bert_pytorch_amd.config import BertConfig
    from bert_pytorch_amd.models import (BertForPreTraining,
                                         BertPretrainingCriterion)
    from bert_pytorch_amd.ops import rng

    torch.manual_seed(seed)
    rng.reset(seed)
    config = BertConfig(
        vocab_size_or_config_json_file=1024, hidden_size=128,
        num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
        max_position_embeddings=64, hidden_dropout_prob=dropout,
        attention_probs_dropout_prob=dropout,
    )
    model = BertForPreTraining(config).to(DEV).train()
    model.checkpoint_activations(checkpoint)
    criterion = BertPretrainingCriterion(config.vocab_size)
    ids = torch.randint(0, 1024, (2, 64), device=DEV)
    mask = torch.ones_like(ids)
    mask[:, 50:] = 0
    tt = torch.zeros_like(ids)
    labels = torch.full((2, 64), -1, dtype=torch.long, device=DEV)
    labels[:, 5:10] = torch.randint(0, 1024, (2, 5), device=DEV)
    nsp = torch.randint(0, 2, (2,), device=DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16,
                        enabled=dtype_autocast is not None):
        scores, rel, glabels = model(ids, tt, mask, masked_lm_labels=labels,
                                     compute_mlm_loss=True)
        loss = criterion(scores, rel, glabels, nsp)
    loss.backward()
    grads = {n: p.grad.clone() for n, p in model.named_parameters()
             if p.grad is not None}
    return loss.detach().clone(), grads


@pytest.mark.parametrize("checkpoint", [False, True], ids=["plain", "ckpt"])
def test_fork_on_off_bitwise_fp32(monkeypatch, checkpoint):
    """In fp32 the sum inside the kernel is the add autograd would have
    made, so the switch changes no bit of the loss or of any gradient."""
    monkeypatch.setenv("BPA_JUNCTION_FORK", "1")
    loss1, g1 = _tiny_step(None, 0.0, checkpoint)
    monkeypatch.setenv("BPA_JUNCTION_FORK", "0")
    loss0, g0 = _tiny_step(None, 0.0, checkpoint)
    assert torch.equal(loss1, loss0)
    assert g1.keys() == g0.keys() and len(g1) > 20
    for n in g1:
        assert torch.equal(g1[n], g0[n]), n


def test_fork_bf16_dropout_repeatable(monkeypatch):
    monkeypatch.setenv("BPA_JUNCTION_FORK", "1")
    loss_a, ga = _tiny_step(torch.bfloat16, 0.1, False)
    loss_b, gb = _tiny_step(torch.bfloat16, 0.1, False)
    assert torch.isfinite(loss_a)
    assert torch.equal(loss_a, loss_b)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
