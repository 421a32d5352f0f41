"""Accumulating outputs of the native backward entry points: with a
destination (``acc`` / ``*_acc``) a kernel adds its result into an
existing gradient instead of storing it. Every comparison is
``torch.equal`` against "run unfused, then add with torch": the fused add
makes the same roundings (fp32 adds for the folds; for wgrad the 16-bit
rounding of the stored dW, then torch's round(float(a) + float(b))).
Also that ordered folds with destinations repeat bit for bit, on two
streams at once. All tests need a GPU.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
H16 = [torch.bfloat16, torch.float16]
H16_IDS = ["bf16", "fp16"]


def ext():
    from bert_pytorch_amd.ops import extension

    return extension()


def _randn(shape, dtype, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * scale).to(dtype)


# ---------------------------------------------------------------- wgrad

# (K, M, N, splitk); 0 = the kernel's own split. 260 / 3 leaves a ragged
# last slice; [4096, 1024, 128] is what wgrad_tn_profitable admits
WGRAD_CASES = [(256, 128, 128, 1), (256, 128, 128, 2), (260, 128, 256, 3),
               (4096, 1024, 128, 0)]


@pytest.mark.parametrize("dtype", H16, ids=H16_IDS)
@pytest.mark.parametrize("K,M,N,sk", WGRAD_CASES)
def test_wgrad_acc_equals_store_then_add(dtype, K, M, N, sk):
    dy = _randn((K, M), dtype, 1)
    x = _randn((K, N), dtype, 2)
    g = _randn((M, N), dtype, 3, scale=8.0)
    want = g + ext().wgrad_tn(dy, x, sk)
    acc = g.clone()
    assert ext().wgrad_tn(dy, x, sk, acc=acc) is None
    assert torch.equal(acc, want)
    # and once more on top of the result
    want2 = want + ext().wgrad_tn(dy, x, sk)
    ext().wgrad_tn(dy, x, sk, acc=acc)
    assert torch.equal(acc, want2)


def test_wgrad_acc_fp16_overflow_is_inf():
    K, M, N = 256, 128, 128
    dy = torch.zeros(K, M, device=DEV, dtype=torch.float16)
    x = torch.zeros(K, N, device=DEV, dtype=torch.float16)
    # 256 * 16 * 16 = 65536 > 65504 at [0, 0], its negative at [1, 0]
    dy[:, 0] = 16.0
    dy[:, 1] = -16.0
    x[:, 0] = 16.0
    g = _randn((M, N), torch.float16, 4, scale=100.0)
    assert bool(torch.isfinite(g).all())
    want = g + ext().wgrad_tn(dy, x, 1)
    acc = g.clone()
    ext().wgrad_tn(dy, x, 1, acc=acc)
    assert torch.equal(acc, want)
    assert float(acc[0, 0]) == float("inf")
    assert float(acc[1, 0]) == float("-inf")
    assert int(torch.isinf(acc).sum()) == 2


def test_wgrad_acc_rejects_bad_destination():
    dy = _randn((256, 128), torch.bfloat16, 1)
    x = _randn((256, 128), torch.bfloat16, 2)
    good = torch.zeros(128, 128, device=DEV, dtype=torch.bfloat16)
    bad = [
        good.to(torch.float16),
        good.float(),
        torch.zeros(128, 256, device=DEV, dtype=torch.bfloat16),
        torch.zeros(128 * 128, device=DEV, dtype=torch.bfloat16),
        torch.zeros(128, 256, device=DEV, dtype=torch.bfloat16)[:, ::2],
        good.cpu(),
    ]
    for acc in bad:
        with pytest.raises(RuntimeError, match="wgrad_tn: acc"):
            ext().wgrad_tn(dy, x, 1, acc=acc)
    ext().wgrad_tn(dy, x, 1, acc=good)
    assert torch.equal(good, ext().wgrad_tn(dy, x, 1))


# -------------------------------------------------------------- col_sum

# [1536, 8]: 48 partial rows, the one-block fold. [1568, 8]: 49, the
# ordered fold with one strip. [3200, 1032]: 100 partial rows and two
# strips, the second only 8 columns wide.
COLSUM_SHAPES = [(1536, 8), (1568, 8), (3200, 1032)]


@pytest.mark.parametrize("dtype", [F32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", COLSUM_SHAPES)
def test_col_sum_acc_equals_sum_then_add(dtype, shape):
    x = _randn(shape, dtype, 5)
    g = _randn((shape[1],), F32, 6, scale=30.0)
    s = ext().col_sum(x)
    acc = g.clone()
    assert ext().col_sum(x, acc=acc) is None
    assert torch.equal(acc, g + s)
    # a gradient that reaches its fp32 parameter through a 16-bit cast
    for rt in H16:
        acc = g.clone()
        ext().col_sum(x, acc=acc, round_to=rt)
        assert torch.equal(acc, g + s.to(rt).to(F32))
    assert torch.equal(ext().col_sum(x), s)


def test_col_sum_acc_rejects_bad_destination():
    x = _randn((64, 128), torch.bfloat16, 1)
    for acc in (torch.zeros(128, device=DEV, dtype=torch.bfloat16),
                torch.zeros(64, device=DEV), torch.zeros(256, device=DEV)[::2],
                torch.zeros(1, 128, device=DEV), torch.zeros(128)):
        with pytest.raises(RuntimeError, match="col_sum: acc"):
            ext().col_sum(x, acc=acc)
    with pytest.raises(RuntimeError, match="round_to goes with acc"):
        ext().col_sum(x, round_to=torch.bfloat16)


# ------------------------------------------------- LN family, bias_gelu

# rows at H = 128: 2048 rows give more than 48 partial rows (ordered
# fold), 64 rows at most 48 (one-block fold)
ROWS = [2048, 64]
H = 128


def _ln_operands(rows, dtype, seed):
    z = _randn((rows, H), dtype, seed) + 0.5
    dy = _randn((rows, H), dtype, seed + 1)
    dy2 = _randn((rows, H), dtype, seed + 2)
    gamma = 1.0 + 0.1 * _randn((H,), F32, seed + 3)
    zf = z.float()
    mean = zf.mean(1)
    rstd = (zf.var(1, unbiased=False) + 1e-12).rsqrt()
    return z, dy, dy2, gamma, mean.contiguous(), rstd.contiguous()


def _grads(n, seed):
    return [_randn((H,), F32, seed + i, scale=20.0) for i in range(n)]


def _check_fused(ref, out, dsts, g0, col_idx):
    """``ref``/``out``: unfused and fused outputs. ``col_idx`` are the
    positions of the column gradients, ``dsts`` the destination (or None)
    of each and ``g0`` what each held before."""
    for i in range(len(ref)):
        if i in col_idx:
            continue
        assert torch.equal(out[i], ref[i]), i  # dx, dz untouched
    for i, d, g in zip(col_idx, dsts, g0):
        if d is None:
            assert torch.equal(out[i], ref[i]), i
        else:
            assert out[i] is None, i
            assert torch.equal(d, g + ref[i]), i


@pytest.mark.parametrize("dtype", [F32] + H16, ids=["fp32"] + H16_IDS)
@pytest.mark.parametrize("rows", ROWS)
def test_ln_bwd_acc(dtype, rows):
    z, dy, _, gamma, mean, rstd = _ln_operands(rows, dtype, 10)
    ref = ext().ln_bwd(dy, z, gamma, mean, rstd)
    for use in ((True, True), (True, False), (False, True), (False, False)):
        g0 = _grads(2, 20)
        dsts = [g.clone() if u else None for g, u in zip(g0, use)]
        out = ext().ln_bwd(dy, z, gamma, mean, rstd, dgamma_acc=dsts[0],
                           dbeta_acc=dsts[1])
        _check_fused(ref, out, dsts, g0, (1, 2))


@pytest.mark.parametrize("dtype", [F32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("with_dy2", [False, True], ids=["dy", "dy2"])
def test_bdrl_bwd_acc(dtype, rows, p, with_dy2):
    z, dy, dy2, gamma, mean, rstd = _ln_operands(rows, dtype, 30)
    if p > 0:
        gen = torch.Generator(device=DEV).manual_seed(31)
        mask = (torch.rand(rows, H, device=DEV, generator=gen) >= p).to(
            torch.uint8)
    else:
        mask = torch.empty(0, device=DEV, dtype=torch.uint8)
    f = ext().bias_dropout_residual_ln_bwd
    second = dy2 if with_dy2 else None
    # outputs: dx, dbias, dz_res, dgamma, dbeta
    for has_bias in (True, False):
        ref = f(dy, z, mask, gamma, mean, rstd, p, has_bias, second)
        masks = [(True, True, True), (False, False, True),
                 (True, True, False), (False, False, False)]
        for use in masks:
            if not has_bias and use[2]:
                continue
            g0 = _grads(3, 40)
            dsts = [g.clone() if u else None for g, u in zip(g0, use)]
            out = f(dy, z, mask, gamma, mean, rstd, p, has_bias, second,
                    dgamma_acc=dsts[0], dbeta_acc=dsts[1], dbias_acc=dsts[2])
            if has_bias:
                _check_fused(ref, out, dsts, g0, (3, 4, 1))
            else:
                assert out[1].numel() == 0
                _check_fused(ref[:1] + ref[2:], out[:1] + out[2:], dsts[:2],
                             g0[:2], (2, 3))
    with pytest.raises(RuntimeError, match="dbias_acc without a bias"):
        f(dy, z, mask, gamma, mean, rstd, p, False, second,
          dbias_acc=torch.zeros(H, device=DEV))


@pytest.mark.parametrize("dtype", [F32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows", ROWS)
def test_bias_gelu_bwd_acc(dtype, rows):
    x = _randn((rows, H), dtype, 50)
    dy = _randn((rows, H), dtype, 51)
    bias = 0.1 * _randn((H,), F32, 52)
    ref = ext().bias_gelu_bwd(dy, x, bias)
    (g0,) = _grads(1, 53)
    acc = g0.clone()
    out = ext().bias_gelu_bwd(dy, x, bias, dbias_acc=acc)
    _check_fused(ref, out, [acc], [g0], (1,))
    out = ext().bias_gelu_bwd(dy, x, bias, dbias_acc=None)
    _check_fused(ref, out, [None], [g0], (1,))


def test_fold_acc_rejects_bad_destination():
    z, dy, _, gamma, mean, rstd = _ln_operands(64, torch.bfloat16, 60)
    bad = [torch.zeros(H, device=DEV, dtype=torch.bfloat16),
           torch.zeros(H + 8, device=DEV), torch.zeros(2 * H, device=DEV)[::2],
           torch.zeros(H)]
    mask = torch.empty(0, device=DEV, dtype=torch.uint8)
    for b in bad:
        with pytest.raises(RuntimeError, match="dbeta_acc"):
            ext().ln_bwd(dy, z, gamma, mean, rstd, dbeta_acc=b)
        with pytest.raises(RuntimeError, match="dgamma_acc"):
            ext().bias_dropout_residual_ln_bwd(
                dy, z, mask, gamma, mean, rstd, 0.0, True, dgamma_acc=b)
        with pytest.raises(RuntimeError, match="dbias_acc"):
            ext().bias_gelu_bwd(dy, z, gamma, dbias_acc=b)


# ---------------------------------------------------------- determinism

def _interleaved(xa, xb, ga, gb, n):
    outs = []
    for _ in range(n):
        a, b = ga.clone(), gb.clone()
        ext().col_sum(xa, acc=a)
        ext().col_sum(xb, acc=b, round_to=torch.bfloat16)
        outs.append((a, b))
    return outs


def test_accumulating_folds_repeat_across_calls_and_streams():
    """16 accumulating ordered folds of two shapes (one strip, two strips)
    interleaved on one stream, and the same on a second stream alongside:
    the fixed summation order and the add into the destination give every
    call the first call's bits."""
    xa = _randn((1568, 8), F32, 70)
    xb = _randn((3200, 1032), F32, 71)
    ga = _randn((8,), F32, 72, scale=30.0)
    gb = _randn((1032,), F32, 73, scale=30.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        outs_side = _interleaved(xa, xb, ga, gb, 16)
    outs_main = _interleaved(xa, xb, ga, gb, 16)
    torch.cuda.current_stream().synchronize()
    side.synchronize()
    first_a, first_b = outs_main[0]
    assert torch.equal(first_a, ga + ext().col_sum(xa))
    assert torch.equal(
        first_b, gb + ext().col_sum(xb).to(torch.bfloat16).to(F32))
    for outs in (outs_main, outs_side):
        for a, b in outs:
            assert torch.equal(a, first_a)
            assert torch.equal(b, first_b)
