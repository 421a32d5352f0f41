"""Row-wise and element-wise HIP kernels against fp64: ln_fwd/ln_bwd,
bias_dropout_residual_ln ("bdrl"), bias_gelu, col_sum, the embedding
kernel and ce_fwd/ce_bwd, in fp32, bf16 and fp16, at every launch shape
of the block-per-row kernels, on ill-conditioned rows, with dropout
(masks bit for bit against tests/philox_ref.py) and at the
cross-entropy edges. All tests @pytest.mark.gpu.

Bounds (per element, not max-normalised):
  element-wise outputs  |out - ref| <= ulp_T * |ref| + a * max|ref|
      ulp_T = 2^-7 (bf16), 2^-10 (fp16), 0 (fp32): one ulp, twice the
      rounding error of the final cast; a = 1e-5 forward, 1e-4 backward
      (the suite's fp32 bounds).
  column reductions     rows * 2^-24 * sum|terms|  (dbeta, col_sum)
                        rows * 2^-22 * sum|terms|  (dgamma: the normalised
                        x in its terms carries a few ulps of its own)
The reference is the fp64 composite of the same rounded inputs, with
gradients by fp64 autograd. A backward kernel's inputs are what it is
handed: bdrl_bwd reads the z that the forward stored rounded to T
together with the mean/rstd of the unrounded z, so no autograd graph has
its inputs; its reference is the LayerNorm backward formula in fp64 at
exactly those operands (checked against autograd where z is exact, in
fp32). mean and rstd themselves are held to 1e-6 of fp64 in the forward.

Every check prints ``RATIO <family> <what> <error/bound>`` before it
asserts error/bound <= 1.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

import philox_ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bert_pytorch_amd import ops

DEV = "cuda:0"
EPS = 1e-12
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
DT_IDS = ["fp32", "bf16", "fp16"]
ULP = {F32: 0.0, BF16: 2.0 ** -7, F16: 2.0 ** -10}
A_FWD, A_BWD = 1e-5, 1e-4


def ext():
    return ops.extension()


class Acc:
    """Collects error/bound ratios of one test; prints each, asserts all."""

    def __init__(self, family, dtype=None):
        if dtype is not None:
            family += "/" + str(dtype).replace("torch.", "")
        self.family, self.bad = family, []

    def add(self, what, ratio):
        print(f"RATIO {self.family} {what} {ratio:.3g}")
        if not ratio <= 1.0:
            self.bad.append(f"{what}: error/bound = {ratio:.3g}")

    def elem(self, what, out, ref, dtype, a, extra=0.0):
        ref = ref.double()
        bound = ULP[dtype] * ref.abs() + a * ref.abs().max() + extra
        self.add(what, float(((out.double() - ref).abs() / bound).max()))

    def col(self, what, out, ref, bound):
        """Column reduction against a per-column bound tensor; columns
        whose bound is 0 must match exactly."""
        err = (out.double() - ref.double()).abs()
        exact = bound == 0
        r = float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0
        if exact.any() and float(err[exact].max()) != 0.0:
            r = float("inf")
        self.add(what, r)

    def rel(self, what, out, ref, tol):
        ref = ref.double()
        self.add(what, float(((out.double() - ref).abs() / ref.abs()).max()) / tol)

    def done(self):
        assert not self.bad, "; ".join(self.bad)


def _same(o1, o2):
    for a, b in zip(o1, o2):
        assert torch.equal(a, b), "two launches differ bitwise"


# ---------------------------------------------------------------------------
# 2. shape and dtype sweep
# ---------------------------------------------------------------------------
# (H, rows). Slices = H / VEC (VEC 8 for 16-bit, 4 for fp32); the branch
# of launch_by_items (rowwise.h, shared by layernorm.hip and
# fused_residual.hip):
H_16BIT = [
    (64, 37),     # 8 slices: one wave, block_reduce's nwaves == 1 return
    (768, 37),    # 96 slices on 128 threads: last wave half filled
    (2056, 37),   # 257 slices: ITEMS 2 x 256 threads, 2nd item one slice
    (8200, 37),   # 1025 slices: ITEMS 4 x 512 threads
    (16392, 5),   # 2049 slices: ITEMS 4 x 1024 threads
]
H_FP32 = [
    (64, 37),     # 16 slices: one wave
    (768, 37),    # 192 slices on 192 threads
    (1032, 37),   # 258 slices: ITEMS 2 x 256 threads
    (4104, 37),   # 1026 slices: ITEMS 4 x 512 threads
    (8200, 5),    # 2050 slices: ITEMS 4 x 1024 threads
]
# bias_gelu and col_sum have no ITEMS dispatch: one wave, a part-filled
# block, more than one column block. rows = 37 gives bias_gelu_bwd's four
# waves 4/4/4/4, 4/4/4/4 and 2/1/1/1 rows of the three 16-row stripes.
H_FLAT_16BIT = [(64, 37), (768, 37), (2056, 37)]
H_FLAT_FP32 = [(64, 37), (768, 37), (1032, 37)]


def _sweep(cases16, cases32):
    out = []
    for dt, name in zip(DTYPES, DT_IDS):
        for H, rows in (cases32 if dt == F32 else cases16):
            out.append(pytest.param(dt, H, rows, id=f"{name}-H{H}"))
    return out


def _params(H, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    gamma = torch.randn(H, device=DEV, generator=g) * 0.1 + 1.0
    beta = torch.randn(H, device=DEV, generator=g) * 0.1
    bias = torch.randn(H, device=DEV, generator=g) * 0.5
    return gamma, beta, bias


def _randn(rows, H, dtype, seed, shift=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(rows, H, device=DEV, generator=g) + shift).to(dtype)


def _ln64(x64, gamma, beta):
    return F.layer_norm(x64, (x64.shape[-1],), gamma.double(), beta.double(), EPS)


def _stats64(x64):
    mu = x64.mean(1)
    return mu, torch.rsqrt(x64.var(1, unbiased=False) + EPS)


def _ln_backward_ref(x, dy, gamma, beta):
    """fp64 autograd through LayerNorm at x: dx, dgamma, dbeta, and the
    column-reduction bounds' sum|terms|."""
    x64 = x.double().requires_grad_(True)
    g64 = gamma.double().requires_grad_(True)
    b64 = beta.double().requires_grad_(True)
    y = F.layer_norm(x64, (x.shape[1],), g64, b64, EPS)
    y.backward(dy.double())
    mu, rs = _stats64(x64.detach())
    xhat = (x64.detach() - mu[:, None]) * rs[:, None]
    abs_b = dy.double().abs().sum(0)
    abs_g = (dy.double() * xhat).abs().sum(0)
    return x64.grad, g64.grad, b64.grad, abs_g, abs_b


@pytest.mark.parametrize("dtype,H,rows", _sweep(H_16BIT, H_FP32))
def test_ln_sweep(dtype, H, rows):
    """ln_fwd + ln_bwd at every launch shape. Inputs are randn + 0.5, so
    the row mean is well conditioned for the 1e-6 relative check."""
    acc = Acc("sweep", dtype)
    gamma, beta, _ = _params(H, H)
    x = _randn(rows, H, dtype, H + 1, shift=0.5)
    dy = _randn(rows, H, dtype, H + 2)
    y, mean, rstd = ext().ln_fwd(x, gamma, beta, EPS)
    assert y.dtype == dtype and mean.dtype == F32 and mean.shape == (rows,)
    x64 = x.double()
    mu64, rs64 = _stats64(x64)
    acc.elem("ln y", y, _ln64(x64, gamma, beta), dtype, A_FWD)
    acc.rel("ln mean", mean, mu64, 1e-6)
    acc.rel("ln rstd", rstd, rs64, 1e-6)
    o1 = ext().ln_bwd(dy, x, gamma, mean, rstd)
    o2 = ext().ln_bwd(dy, x, gamma, mean, rstd)
    dx_r, dg_r, db_r, abs_g, abs_b = _ln_backward_ref(x, dy, gamma, beta)
    acc.elem("ln dx", o1[0], dx_r, dtype, A_BWD)
    acc.col("ln dgamma", o1[1], dg_r, rows * 2.0 ** -22 * abs_g)
    acc.col("ln dbeta", o1[2], db_r, rows * 2.0 ** -24 * abs_b)
    _same(o1, o2)
    acc.done()


def _ln_backward_formula(z, dy, gamma, mean, rstd):
    """LayerNorm backward in fp64 from the saved operands (z, mean, rstd):
    dz, dgamma, dbeta and the column bounds' sum|terms|."""
    dy64 = dy.double()
    rs = rstd.double()[:, None]
    xhat = (z.double() - mean.double()[:, None]) * rs
    dw = dy64 * gamma.double()
    s1 = (dw * xhat).mean(1, keepdim=True)
    s2 = dw.mean(1, keepdim=True)
    dz = rs * (dw - s2 - xhat * s1)
    return (dz, (dy64 * xhat).sum(0), dy64.sum(0),
            (dy64 * xhat).abs().sum(0), dy64.abs().sum(0))


def _bdrl_backward_check(acc, tag, dtype, z, mask, p, dy, gamma, beta, mean,
                         rstd, has_bias):
    """bdrl_bwd against the fp64 LayerNorm backward at its operands, with
    dx = mask * dz / (1 - p); two launches bitwise equal."""
    rows = z.shape[0]
    o1 = ext().bias_dropout_residual_ln_bwd(dy, z, mask, gamma, mean, rstd,
                                            p, has_bias)
    o2 = ext().bias_dropout_residual_ln_bwd(dy, z, mask, gamma, mean, rstd,
                                            p, has_bias)
    dx, dbias, dres, dgamma, dbeta = o1
    dz_r, dg_r, db_r, abs_g, abs_b = _ln_backward_formula(
        z, dy, gamma, mean, rstd)
    if dtype == F32:
        # z is exact here: the formula must agree with fp64 autograd to
        # the 1e-6 that the kernel's fp32 mean/rstd carry
        auto = _ln_backward_ref(z, dy, gamma, beta)
        for a, b in zip(auto[:3], (dz_r, dg_r, db_r)):
            assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max())
    dx_r = dz_r * mask.double() / (1.0 - p) if p > 0 else dz_r
    acc.elem(f"{tag} dres", dres, dz_r, dtype, A_BWD)
    acc.elem(f"{tag} dx", dx, dx_r, dtype, A_BWD)
    acc.col(f"{tag} dgamma", dgamma, dg_r, rows * 2.0 ** -22 * abs_g)
    acc.col(f"{tag} dbeta", dbeta, db_r, rows * 2.0 ** -24 * abs_b)
    if has_bias:
        # dbias sums the dx the kernel stored, i.e. rounded to T: one
        # ulp_T per term plus the fp32 summation
        abs_x = dx_r.abs().sum(0)
        bound = (ULP[dtype] + rows * 2.0 ** -24) * abs_x
        acc.col(f"{tag} dbias", dbias, dx_r.sum(0), bound)
    else:
        assert dbias.numel() == 0
    if p > 0:
        assert float(dx[mask == 0].abs().max()) == 0.0
    _same(o1, o2)


@pytest.mark.parametrize("has_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype,H,rows", _sweep(H_16BIT, H_FP32))
def test_bdrl_sweep(dtype, H, rows, has_bias):
    """bdrl forward + backward (p = 0) at every launch shape. x and the
    residual are randn + 0.5 each: the row mean (about 1, the bias's own
    mean is below 0.2) is well conditioned for the 1e-6 relative check."""
    acc = Acc("sweep", dtype)
    gamma, beta, bias = _params(H, H + 10)
    x = _randn(rows, H, dtype, H + 11, shift=0.5)
    res = _randn(rows, H, dtype, H + 12, shift=0.5)
    dy = _randn(rows, H, dtype, H + 13)
    y, z, mask, mean, rstd = ext().bias_dropout_residual_ln_fwd(
        x, bias if has_bias else None, res, gamma, beta, 0.0, EPS, 0, 0
    )
    assert mask.numel() == 0
    z64 = x.double() + res.double()
    if has_bias:
        z64 = z64 + bias.double()
    mu64, rs64 = _stats64(z64)
    acc.elem("bdrl z", z, z64, dtype, A_FWD)
    acc.elem("bdrl y", y, _ln64(z64, gamma, beta), dtype, A_FWD)
    acc.rel("bdrl mean", mean, mu64, 1e-6)
    acc.rel("bdrl rstd", rstd, rs64, 1e-6)
    _bdrl_backward_check(acc, "bdrl", dtype, z, mask, 0.0, dy, gamma, beta,
                         mean, rstd, has_bias)
    acc.done()


@pytest.mark.parametrize("dtype,H,rows", _sweep(H_FLAT_16BIT, H_FLAT_FP32))
def test_bias_gelu_and_col_sum_sweep(dtype, H, rows):
    acc = Acc("sweep", dtype)
    _, _, bias = _params(H, H + 20)
    x = _randn(rows, H, dtype, H + 21)
    dy = _randn(rows, H, dtype, H + 22)
    y = ext().bias_gelu_fwd(x, bias)
    x64 = x.double().requires_grad_(True)
    b64 = bias.double().requires_grad_(True)
    y64 = F.gelu(x64 + b64)
    y64.backward(dy.double())
    acc.elem("gelu y", y, y64.detach(), dtype, A_FWD)
    o1 = ext().bias_gelu_bwd(dy, x, bias)
    o2 = ext().bias_gelu_bwd(dy, x, bias)
    acc.elem("gelu dx", o1[0], x64.grad, dtype, A_BWD)
    # dbias sums the unrounded fp32 dx: the plain column-sum bound
    acc.col("gelu dbias", o1[1], b64.grad,
            rows * 2.0 ** -24 * x64.grad.abs().sum(0))
    _same(o1, o2)
    s1, s2 = ext().col_sum(x), ext().col_sum(x)
    assert s1.dtype == F32 and s1.shape == (H,)
    acc.col("col_sum", s1, x.double().sum(0),
            rows * 2.0 ** -24 * x.double().abs().sum(0))
    assert torch.equal(s1, s2)
    acc.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_bad_widths_rejected(dtype):
    """H that is no multiple of the 16 B slice, and one slice more than
    the block-per-row limit of 4096: refused on the host before a launch."""
    vec = 4 if dtype == F32 else 8
    rows = 2

    def call_all(H, block_per_row_only, message):
        x = torch.zeros(rows, H, device=DEV, dtype=dtype)
        v = torch.zeros(H, device=DEV)
        st = torch.zeros(rows, device=DEV)
        no_mask = torch.empty(0, device=DEV, dtype=torch.uint8)
        calls = [
            lambda: ext().ln_fwd(x, v, v, EPS),
            lambda: ext().ln_bwd(x, x, v, st, st),
            lambda: ext().bias_dropout_residual_ln_fwd(
                x, v, x, v, v, 0.0, EPS, 0, 0),
            lambda: ext().bias_dropout_residual_ln_bwd(
                x, x, no_mask, v, st, st, 0.0, True),
        ]
        if not block_per_row_only:
            calls += [
                lambda: ext().bias_gelu_fwd(x, v),
                lambda: ext().bias_gelu_bwd(x, x, v),
                lambda: ext().col_sum(x),
            ]
        for c in calls:
            with pytest.raises(RuntimeError, match=message):
                c()

    call_all(1030 if dtype == F32 else 1028, False,
             rf"H must be a multiple of {vec}|H % {vec} != 0")
    call_all(4097 * vec, True, "H too large")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 3. ill-conditioned rows: variance as the mean of (v - mu)^2
# ---------------------------------------------------------------------------
RATIOS = (0.0, 10.0, 100.0, 1000.0)  # |mean| / std of a row group
ILL_H = 1024
ILL_ROWS_PER = 8


def _ill_offsets():
    """[rows] offsets: ordinary rows mixed with mean/std 10, 100, 1000."""
    return torch.tensor(RATIOS, device=DEV).repeat(ILL_ROWS_PER)


def _ill_check(acc, tag, dtype, y, mean, rstd, z64, gamma, beta, groups):
    """Per group of equally conditioned rows: error against fp64 at most
    8x the error torch's fp32 layer_norm makes on the same rows (floored
    at 1e-6 of max|y|); 16-bit outputs add the element-wise bound above.
    rstd likewise, relative, floored at 1e-6; the mean likewise, absolute,
    floored at 1e-6 of the group's max|z|.

    Measured error/bound on an MI355X, worst group. Single-pass variance
    (sumsq/H - mu^2, the kernels before the two-pass change), fp32:
    ln y 643, bdrl y 507, embedding y 168, rstd 2770 to 6150; bf16/fp16:
    y 7.8 to 71, rstd 1230 to 5560. Two-pass: fp32 y 0.15 to 0.20, rstd
    below 0.08; bf16/fp16 y below 0.5 (the final cast)."""
    H = z64.shape[1]
    y64 = _ln64(z64, gamma, beta)
    mu64, rs64 = _stats64(z64)
    ty, tmean, trstd = torch.native_layer_norm(
        z64.float(), (H,), gamma, beta, EPS)
    for r in RATIOS:
        sel = groups == r
        ymax = float(y64[sel].abs().max())
        t_err = float((ty[sel].double() - y64[sel]).abs().max())
        extra = 8.0 * max(t_err, 1e-6 * ymax)
        ref = y64[sel]
        bound = extra + (ULP[dtype] * ref.abs() + A_FWD * ymax
                         if dtype != F32 else 0.0)
        acc.add(f"{tag} y ratio={r:g}",
                float(((y[sel].double() - ref).abs() / bound).max()))
        t_rs = float(((trstd.reshape(-1)[sel].double() - rs64[sel]).abs()
                      / rs64[sel]).max())
        acc.add(f"{tag} rstd ratio={r:g}",
                float(((rstd[sel].double() - rs64[sel]).abs()
                       / rs64[sel]).max()) / (8.0 * max(t_rs, 1e-6)))
        t_mu = float((tmean.reshape(-1)[sel].double() - mu64[sel]).abs().max())
        zmax = float(z64[sel].abs().max())
        acc.add(f"{tag} mean ratio={r:g}",
                float((mean[sel].double() - mu64[sel]).abs().max())
                / (8.0 * max(t_mu, 1e-6 * zmax)))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_ill_conditioned_ln(dtype):
    acc = Acc("illcond", dtype)
    gamma, beta, _ = _params(ILL_H, 31)
    off = _ill_offsets()
    x = (_randn(off.numel(), ILL_H, F32, 32) + off[:, None]).to(dtype)
    y, mean, rstd = ext().ln_fwd(x, gamma, beta, EPS)
    _ill_check(acc, "ln", dtype, y, mean, rstd, x.double(), gamma, beta, off)
    acc.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_ill_conditioned_bdrl(dtype):
    """The offset arrives through the residual (as in a deep encoder)."""
    acc = Acc("illcond", dtype)
    gamma, beta, bias = _params(ILL_H, 33)
    off = _ill_offsets()
    x = _randn(off.numel(), ILL_H, dtype, 34)
    res = (_randn(off.numel(), ILL_H, F32, 35) * 0.5 + off[:, None]).to(dtype)
    y, z, _, mean, rstd = ext().bias_dropout_residual_ln_fwd(
        x, bias, res, gamma, beta, 0.0, EPS, 0, 0)
    z64 = x.double() + bias.double() + res.double()
    _ill_check(acc, "bdrl", dtype, y, mean, rstd, z64, gamma, beta, off)
    acc.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_ill_conditioned_embedding(dtype):
    """The offset arrives through the position table: position s carries
    RATIOS[s % 4]. fp32 tables, output in ``dtype``."""
    acc = Acc("illcond", dtype)
    H, B, S, V = ILL_H, 4, 8, 30
    gamma, beta, _ = _params(H, 36)
    g = torch.Generator(device=DEV).manual_seed(37)
    ids = torch.randint(0, V, (B, S), device=DEV, generator=g)
    tt = torch.randint(0, 2, (B, S), device=DEV, generator=g)
    word = torch.randn(V, H, device=DEV, generator=g) * 0.7
    tok = torch.randn(2, H, device=DEV, generator=g) * 0.7
    pos_off = torch.tensor(RATIOS, device=DEV).repeat(S // 4)
    pos = torch.randn(S, H, device=DEV, generator=g) * 0.2 + pos_off[:, None]
    y, z, _, mean, rstd = ext().embedding_ln_dropout_fwd(
        ids, tt, word, pos, tok, gamma, beta, 0.0, EPS, 0, 0, dtype)
    z64 = (word.double()[ids] + pos.double()[None] + tok.double()[tt])
    z64 = z64.view(B * S, H)
    acc.add("embed z", float((z.double() - z64).abs().max()
                             / (A_FWD * z64.abs().max())))
    _ill_check(acc, "embed", dtype, y.view(B * S, H), mean, rstd, z64, gamma,
               beta, pos_off.repeat(B))
    acc.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_ill_conditioned_backward(dtype):
    """ln_bwd and bdrl_bwd (fp32) need no change for rows with
    mean/std = 100: the section-2 bounds, see below."""
    acc = Acc("illcond", dtype)
    rows, H = 37, ILL_H
    gamma, beta, _ = _params(H, 38)
    x = (_randn(rows, H, F32, 39) + 100.0).to(dtype)
    dy = _randn(rows, H, dtype, 40)
    _, mean, rstd = ext().ln_fwd(x, gamma, beta, EPS)
    dx, dgamma, dbeta = ext().ln_bwd(dy, x, gamma, mean, rstd)
    dx_r, dg_r, db_r, abs_g, abs_b = _ln_backward_ref(x, dy, gamma, beta)
    # as in the forward: an fp32 mean of values near 100 is itself off by
    # a few 2^-24 * 100 whatever the algorithm, so each bound gains 8x the
    # error torch's fp32 LayerNorm backward makes on the same input
    x32 = x.float().requires_grad_(True)
    g32 = gamma.clone().requires_grad_(True)
    b32 = beta.clone().requires_grad_(True)
    F.layer_norm(x32, (H,), g32, b32, EPS).backward(dy.float())
    e_dx = 8.0 * float((x32.grad.double() - dx_r).abs().max())
    e_dg = 8.0 * float((g32.grad.double() - dg_r).abs().max())
    e_db = 8.0 * float((b32.grad.double() - db_r).abs().max())
    acc.elem("ln dx ratio=100", dx, dx_r, dtype, A_BWD, extra=e_dx)
    acc.col("ln dgamma ratio=100", dgamma, dg_r,
            rows * 2.0 ** -22 * abs_g + e_dg)
    acc.col("ln dbeta ratio=100", dbeta, db_r,
            rows * 2.0 ** -24 * abs_b + e_db)
    if dtype == F32:
        zero = torch.zeros_like(x)
        _, z, mask, mean, rstd = ext().bias_dropout_residual_ln_fwd(
            zero, None, x, gamma, beta, 0.0, EPS, 0, 0)
        assert torch.equal(z, x)
        _bdrl_backward_check(acc, "bdrl ratio=100", dtype, z, mask, 0.0, dy,
                             gamma, beta, mean, rstd, False)
    acc.done()


# ---------------------------------------------------------------------------
# 4. dropout: conditioned on the stored mask, and the exact streams
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_bdrl_dropout_fwd_bwd(dtype, H, p):
    """x and the residual are randn + 0.5 each, so the row mean (about 1)
    is well conditioned for the 1e-6 relative check, as in the sweep."""
    acc = Acc("dropout", dtype)
    rows = 37
    gamma, beta, bias = _params(H, H + 40)
    x = _randn(rows, H, dtype, H + 41, shift=0.5)
    res = _randn(rows, H, dtype, H + 42, shift=0.5)
    dy = _randn(rows, H, dtype, H + 43)
    y, z, mask, mean, rstd = ext().bias_dropout_residual_ln_fwd(
        x, bias, res, gamma, beta, p, EPS, 4242, 11)
    assert mask.dtype == torch.uint8 and mask.shape == (rows, H)
    assert 0 < int(mask.sum()) < mask.numel() and int(mask.max()) == 1
    keep = mask.double()
    z64 = keep * (x.double() + bias.double()) / (1.0 - p) + res.double()
    acc.elem("bdrl z", z, z64, dtype, A_FWD)
    acc.elem("bdrl y", y, _ln64(z64, gamma, beta), dtype, A_FWD)
    mu64, rs64 = _stats64(z64)
    acc.rel("bdrl mean", mean, mu64, 1e-6)
    acc.rel("bdrl rstd", rstd, rs64, 1e-6)
    _bdrl_backward_check(acc, "bdrl", dtype, z, mask, p, dy, gamma, beta,
                         mean, rstd, True)
    acc.done()


# (output dtype, table dtype)
EMBED_MODES = [(F32, F32), (BF16, F32), (F16, F32), (BF16, BF16)]
EMBED_IDS = ["fp32", "bf16", "fp16", "pure-bf16"]


def _embed_inputs(H, tdtype, has_tok, seed):
    B, S, V, P, T = 3, 29, 50, 40, 2
    g = torch.Generator(device=DEV).manual_seed(seed)
    ids = torch.randint(0, V, (B, S), device=DEV, generator=g)
    ids[0, :6] = 7  # a repeated id ([MASK]-like)
    tt = torch.randint(0, T, (B, S), device=DEV, generator=g) if has_tok else None
    word = (torch.randn(V, H, device=DEV, generator=g)).to(tdtype)
    pos = (torch.randn(P, H, device=DEV, generator=g) * 0.5).to(tdtype)
    tok = (torch.randn(T, H, device=DEV, generator=g) * 0.5).to(tdtype) \
        if has_tok else None
    return B, S, V, P, T, ids, tt, word, pos, tok


@pytest.mark.parametrize("has_tok", [True, False], ids=["tok", "notok"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("H", [64, 768])
@pytest.mark.parametrize("odtype,tdtype", EMBED_MODES, ids=EMBED_IDS)
def test_embedding_dropout_fwd_bwd(odtype, tdtype, H, p, has_tok):
    """Embedding forward/backward with p > 0, conditioned on the stored
    mask (applied after the LayerNorm), dy in the output dtype.

    The table gradients are fp32 column sums of n rows of the fp32 dz:
    n * 2^-24 * sum|dz| for the summation, as for every column sum here,
    plus n * 2^-20 * max|dz| for dz itself, which no 16-bit cast follows:
    dz = rs * (dw - mean(dw) - xhat * mean(dw * xhat)) is a dozen fp32
    roundings, each relative to the largest operand, not to the (possibly
    cancelled) result; 16 half-ulps allows for them. That is 100x below the
    a * max|ref| of the element-wise outputs, so a 16-bit accumulation
    (2^-9) cannot pass. Rows that nothing maps to have n = 0: exactly 0."""
    acc = Acc("dropout", odtype)
    B, S, V, P, T, ids, tt, word, pos, tok = _embed_inputs(
        H, tdtype, has_tok, H + 50)
    rows = B * S
    gamma, beta, _ = _params(H, H + 51)
    dy = _randn(rows, H, odtype, H + 52).view(B, S, H)
    y, z, mask, mean, rstd = ext().embedding_ln_dropout_fwd(
        ids, tt, word, pos, tok, gamma, beta, p, EPS, 99, 3, odtype)
    assert y.dtype == odtype and z.dtype == F32
    assert mask.shape == (rows, H) and 0 < int(mask.sum()) < mask.numel()

    w64 = word.double().requires_grad_(True)
    p64 = pos.double().requires_grad_(True)
    t64 = tok.double().requires_grad_(True) if has_tok else None
    g64 = gamma.double().requires_grad_(True)
    b64 = beta.double().requires_grad_(True)
    z64 = w64[ids] + p64[:S][None]
    if has_tok:
        z64 = z64 + t64[tt]
    z64.retain_grad()
    keep = mask.double().view(B, S, H)
    y64 = F.layer_norm(z64, (H,), g64, b64, EPS) * keep / (1.0 - p)
    y64.backward(dy.double())
    acc.elem("embed z", z, z64.detach().view(rows, H), F32, A_FWD)
    acc.elem("embed y", y, y64.detach(), odtype, A_FWD)
    mu64, rs64 = _stats64(z64.detach().view(rows, H))
    acc.rel("embed rstd", rstd, rs64, 1e-6)

    args = (dy, ids, tt, z, mask, gamma, mean, rstd, p, V, P,
            T if has_tok else 0)
    o1 = ext().embedding_ln_dropout_bwd(*args)
    o2 = ext().embedding_ln_dropout_bwd(*args)
    d_word, d_pos, d_tok, dgamma, dbeta = o1
    dz_abs = z64.grad.abs().view(rows, H)
    a_dz = 2.0 ** -20 * float(dz_abs.max())
    ones = torch.ones(rows, device=DEV, dtype=torch.double)

    def table_bound(n_rows, index):
        """n * (2^-20 * max|dz| + 2^-24 * sum|dz|) per table row, column."""
        n = torch.zeros(n_rows, device=DEV, dtype=torch.double).index_add_(
            0, index, ones)
        sum_abs = torch.zeros(n_rows, H, device=DEV, dtype=torch.double)
        sum_abs.index_add_(0, index, dz_abs)
        return n[:, None] * (a_dz + 2.0 ** -24 * sum_abs)

    pos_idx = torch.arange(S, device=DEV).repeat(B)
    acc.col("embed d_word", d_word, w64.grad, table_bound(V, ids.view(-1)))
    acc.col("embed d_pos", d_pos, p64.grad, table_bound(P, pos_idx))
    assert float(d_pos[S:].abs().max()) == 0.0  # rows 29..39
    if has_tok:
        acc.col("embed d_tok", d_tok, t64.grad, table_bound(T, tt.view(-1)))
    else:
        assert d_tok.numel() == 0
    d_eff = (dy.double() * keep / (1.0 - p)).view(rows, H)
    xhat = (z64.detach().view(rows, H) - mu64[:, None]) * rs64[:, None]
    acc.col("embed dgamma", dgamma, g64.grad,
            rows * 2.0 ** -22 * (d_eff * xhat).abs().sum(0))
    acc.col("embed dbeta", dbeta, b64.grad,
            rows * 2.0 ** -24 * d_eff.abs().sum(0))
    _same(o1, o2)
    acc.done()


SEEDS = [5, 2 ** 40 + 12345]          # the second uses the key's high word
OFFSETS = [7, 2 ** 32 - 3, 2 ** 33 + 1]  # the middle one carries into c1
#                                          inside the tensor


@functools.lru_cache(maxsize=None)
def _want_mask(rows, H, p, seed, offset):
    return torch.from_numpy(philox_ref.bdrl_keep_mask(rows, H, p, seed, offset))


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("seed", SEEDS)
def test_bdrl_and_embedding_mask_stream_exact(seed, offset):
    """The byte masks equal the numpy Philox stream bit for bit, for every
    input dtype (VEC 4 or 8: same counter mapping), p in {0.1, 0.5}."""
    rows, H = 37, 768
    B, S = 3, 29
    for p in (0.1, 0.5):
        want = _want_mask(rows, H, p, seed, offset)
        assert 0 < int(want.sum()) < want.numel()
        for dtype in DTYPES:
            x = _randn(rows, H, dtype, 60)
            v = torch.ones(H, device=DEV)
            mask = ext().bias_dropout_residual_ln_fwd(
                x, None, x, v, v, p, EPS, seed, offset)[2]
            assert torch.equal(mask.cpu(), want), (p, dtype)
        want_e = _want_mask(B * S, 64, p, seed, offset)
        _, _, V, P, T, ids, tt, word, pos, tok = _embed_inputs(64, F32, True, 61)
        v = torch.ones(64, device=DEV)
        for odtype in DTYPES:
            mask = ext().embedding_ln_dropout_fwd(
                ids, tt, word, pos, tok, v, v, p, EPS, seed, offset, odtype)[2]
            assert torch.equal(mask.cpu(), want_e), (p, odtype)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("S", [48, 128])
def test_attention_mask_stream_exact(S, seed, offset):
    """attention_fwd's bit-packed dmask equals the numpy stream as int32
    words, padding bits of a row's last word included (S = 48: 16 of
    them); attention_varlen_fwd gives the same words."""
    B, NH = 1, 2
    Hh = NH * 64
    g = torch.Generator(device=DEV).manual_seed(62)
    qkv = (torch.randn(B, S, 3 * Hh, device=DEV, generator=g) * 0.5).bfloat16()
    seqlens = torch.full((B,), S, device=DEV, dtype=torch.int32)
    t_pad = -(-S // 128) * 128
    packed = qkv.new_zeros(t_pad, 3 * Hh)
    packed[:S] = qkv[0]
    cu = torch.tensor([0, S], device=DEV, dtype=torch.int32)
    for p in (0.1, 0.5):
        want = torch.from_numpy(
            philox_ref.attention_keep_bits(B * NH, S, p, seed, offset))
        dmask = ext().attention_fwd(qkv, seqlens, NH, p, seed, offset)[2]
        assert dmask.dtype == torch.int32 and dmask.shape == want.shape
        assert torch.equal(dmask.cpu(), want), p
        assert not bool((dmask == -1).all()) and not bool((dmask == 0).all())
        dmask_v = ext().attention_varlen_fwd(
            packed, cu, S, NH, p, seed, offset)[2]
        assert torch.equal(dmask_v.cpu(), want), p


# ---------------------------------------------------------------------------
# 5. cross-entropy edges
# ---------------------------------------------------------------------------
def _ce_inputs(V, N, dtype, case):
    """randn * 3 logits; ``case``: plain | ignored (every third row) |
    spike_first | spike_last | spike_lastthread (+30 at one column)."""
    g = torch.Generator(device=DEV).manual_seed(V * 7 + N)
    logits = torch.randn(N, V, device=DEV, generator=g) * 3.0
    labels = torch.randint(0, V, (N,), device=DEV, generator=g)
    # labels include 0 and V - 1. A one-row batch has room for one; it
    # must not sit on the spike, or every true gradient (1 - p at the
    # label, about e^-30) lies below fp32's resolution of p near 1
    labels[0] = V - 1 if not (N == 1 and case == "spike_last") else 0
    if N > 1:
        labels[1] = 0
    if case == "ignored":
        labels[2::3] = -1
    if case.startswith("spike"):
        vec = 4 if dtype == F32 else 8
        slices = V // vec
        col = {"spike_first": 0, "spike_last": V - 1,
               # first column of the last thread that owns any slice
               "spike_lastthread": (min(slices, 256) - 1) * vec}[case]
        logits[:, col] += 30.0
        if N > 2:
            labels[2] = col
    return logits.to(dtype), labels


CE_CASES = ["plain", "ignored", "spike_first", "spike_last", "spike_lastthread"]


@pytest.mark.parametrize("case", CE_CASES)
@pytest.mark.parametrize("N", [1, 37])
@pytest.mark.parametrize("V", [8, 1000, 4104])  # V = 8: 255 of 256 threads
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)  # idle (s == 0 merge)
def test_cross_entropy_edges(dtype, V, N, case):
    acc = Acc("ce", dtype)
    logits, labels = _ce_inputs(V, N, dtype, case)
    l64 = logits.double().requires_grad_(True)
    loss64 = F.cross_entropy(l64, labels, ignore_index=-1)
    loss64.backward()
    lse64 = torch.logsumexp(l64.detach(), 1)

    loss_sum, count, lse = ext().ce_fwd(logits, labels, -1)
    n_valid = int((labels != -1).sum())
    assert float(count) == n_valid
    acc.add("ce loss", abs(float(loss_sum) / n_valid - float(loss64)) / 1e-5)
    acc.rel("ce lse", lse, lse64, 1e-5)
    one = torch.ones((), device=DEV)
    d1 = ext().ce_bwd(one, logits, labels, lse, count, -1)
    d2 = ext().ce_bwd(one, logits, labels, lse, count, -1)
    assert d1.dtype == dtype
    acc.elem("ce dlogits", d1, l64.grad, dtype, A_BWD)
    assert torch.equal(d1, d2)
    if case == "ignored" and N > 2:
        assert float(d1[2::3].abs().max()) == 0.0
    if dtype == F16:
        # loss scaling: dloss = 1024 gives 1024 x the unscaled gradient
        ds = ext().ce_bwd(one * 1024.0, logits, labels, lse, count, -1)
        acc.elem("ce dlogits x1024", ds, l64.grad * 1024.0, dtype, A_BWD)

    # the autograd wrapper
    lw = logits.clone().requires_grad_(True)
    loss = ops.fused_cross_entropy(lw, labels, -1)
    loss.backward()
    acc.add("ce wrapper loss", abs(float(loss) - float(loss64)) / 1e-5)
    acc.elem("ce wrapper dlogits", lw.grad, l64.grad, dtype, A_BWD)
    acc.done()


def _rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-3))


@pytest.mark.parametrize("V,P", [(1002, 37), (30522, 64)])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_cross_entropy_unaligned_vocab(dtype, V, P):
    """V that is no multiple of the 16 B slice (the unpadded BERT
    vocabulary): rows are not 16 B aligned, the kernels run their scalar
    instantiation. Same bounds as the aligned cases; every element of
    dlogits is compared, so a slice spilling into the next row shows."""
    acc = Acc("ce_unaligned", dtype)
    logits, labels = _ce_inputs(V, P, dtype, "ignored")
    l64 = logits.double().requires_grad_(True)
    loss64 = F.cross_entropy(l64, labels, ignore_index=-1)
    loss64.backward()
    lw = logits.clone().requires_grad_(True)
    loss = ops.fused_cross_entropy(lw, labels, -1)
    loss.backward()
    acc.add("ce loss", abs(float(loss) - float(loss64)) / 1e-5)
    acc.elem("ce dlogits", lw.grad, l64.grad, dtype, A_BWD)
    assert float(lw.grad[2::3].abs().max()) == 0.0
    acc.done()


@pytest.mark.parametrize("V,P,K", [(1002, 37, 128), (30522, 64, 64)])
def test_mlm_decoder_loss_unaligned_vocab(V, P, K, monkeypatch):
    """ops.mlm_decoder_loss forward and backward on an unpadded
    vocabulary, bounds of test_mlm_decoder_loss_autograd (3e-2)."""
    monkeypatch.setenv("BPA_FUSED_MLM", "1")
    acc = Acc("ce_unaligned")
    g = torch.Generator(device=DEV).manual_seed(V)
    h = (torch.randn(P, K, device=DEV, generator=g) * 0.5).bfloat16()
    w = (torch.randn(V, K, device=DEV, generator=g) * 0.2).bfloat16()
    b = torch.randn(V, device=DEV, generator=g) * 0.1
    labels = torch.randint(0, V, (P,), device=DEV, generator=g)
    labels[0], labels[1] = V - 1, 0
    labels[2::4] = -1
    h.requires_grad_(True), w.requires_grad_(True), b.requires_grad_(True)
    hr = h.detach().double().requires_grad_(True)
    wr = w.detach().double().requires_grad_(True)
    br = b.detach().double().requires_grad_(True)
    loss_ref = F.cross_entropy(F.linear(hr, wr, br), labels, ignore_index=-1)
    loss_ref.backward()
    assert ext().mlm_head_supported(256, V, K)
    loss = ops.mlm_decoder_loss(h, w, b, labels)
    loss.backward()
    acc.add("mlm loss", abs(float(loss) - float(loss_ref)) / 3e-2)
    acc.add("mlm dh", _rel_err(h.grad, hr.grad) / 3e-2)
    acc.add("mlm dw", _rel_err(w.grad, wr.grad) / 3e-2)
    acc.add("mlm dbias", _rel_err(b.grad, br.grad) / 3e-2)
    acc.done()


# ---------------------------------------------------------------------------
# 6. mixed-dtype and shape rejections (host side, before any launch)
# ---------------------------------------------------------------------------
ROWS_R, H_R = 4, 64
BF_THEN_F = r"BFloat16.*Float"
F_THEN_BF = r"dtype Float .*BFloat16"


def _rej_tensors():
    xf = torch.zeros(ROWS_R, H_R, device=DEV)
    xb = xf.bfloat16()
    v = torch.ones(H_R, device=DEV)
    st = torch.ones(ROWS_R, device=DEV)
    short = torch.ones(ROWS_R - 1, device=DEV)
    return xf, xb, v, st, short


def test_ln_bwd_rejects_mismatched_operands():
    xf, xb, v, st, short = _rej_tensors()
    with pytest.raises(RuntimeError, match=BF_THEN_F):
        ext().ln_bwd(xb, xf, v, st, st)
    with pytest.raises(RuntimeError, match=F_THEN_BF):
        ext().ln_bwd(xf, xb, v, st, st)
    with pytest.raises(RuntimeError, match="mean"):
        ext().ln_bwd(xf, xf, v, short, st)
    with pytest.raises(RuntimeError, match="rstd"):
        ext().ln_bwd(xf, xf, v, st, short)
    with pytest.raises(RuntimeError, match="rstd.*BFloat16.*Float"):
        ext().ln_bwd(xf, xf, v, st, st.bfloat16())
    with pytest.raises(RuntimeError, match="shape"):
        ext().ln_bwd(xf[:-1], xf, v, st, st)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext().ln_bwd(xf.t().contiguous().t(), xf, v, st, st)
    ext().ln_bwd(xf, xf, v, st, st)  # the well-formed call passes
    torch.cuda.synchronize()


def test_bdrl_bwd_rejects_mismatched_operands():
    xf, xb, v, st, short = _rej_tensors()
    none = torch.empty(0, device=DEV, dtype=torch.uint8)
    mask = torch.ones(ROWS_R, H_R, device=DEV, dtype=torch.uint8)
    f = ext().bias_dropout_residual_ln_bwd
    with pytest.raises(RuntimeError, match=BF_THEN_F):
        f(xb, xf, none, v, st, st, 0.0, True)
    with pytest.raises(RuntimeError, match=F_THEN_BF):
        f(xf, xb, none, v, st, st, 0.0, True)
    with pytest.raises(RuntimeError, match="mean"):
        f(xf, xf, none, v, short, st, 0.0, True)
    with pytest.raises(RuntimeError, match="rstd"):
        f(xf, xf, none, v, st, short, 0.0, True)
    with pytest.raises(RuntimeError, match="mask"):
        f(xf, xf, none, v, st, st, 0.1, True)  # p > 0 needs the mask
    with pytest.raises(RuntimeError, match="mask"):
        f(xf, xf, mask[:-1], v, st, st, 0.1, True)
    with pytest.raises(RuntimeError, match="mask.*Float.*Byte"):
        f(xf, xf, mask.float(), v, st, st, 0.1, True)
    f(xf, xf, mask, v, st, st, 0.1, True)
    torch.cuda.synchronize()


def test_bias_gelu_bwd_rejects_mismatched_operands():
    xf, xb, v, st, short = _rej_tensors()
    with pytest.raises(RuntimeError, match=BF_THEN_F):
        ext().bias_gelu_bwd(xb, xf, v)
    with pytest.raises(RuntimeError, match=F_THEN_BF):
        ext().bias_gelu_bwd(xf, xb, v)
    with pytest.raises(RuntimeError, match="shape"):
        ext().bias_gelu_bwd(xf[:-1], xf, v)
    with pytest.raises(RuntimeError, match="bias"):
        ext().bias_gelu_bwd(xf, xf, v[:-8])
    ext().bias_gelu_bwd(xf, xf, v)
    torch.cuda.synchronize()


def test_ce_bwd_rejects_mismatched_operands():
    """ce_bwd has no dy; its per-row operand is lse, fp32 of length rows
    whatever the logits' dtype."""
    xf, xb, v, st, short = _rej_tensors()
    labels = torch.zeros(ROWS_R, device=DEV, dtype=torch.long)
    one = torch.ones((), device=DEV)
    cnt = torch.full((), float(ROWS_R), device=DEV)
    for logits in (xf, xb):
        with pytest.raises(RuntimeError, match="lse.*" + BF_THEN_F):
            ext().ce_bwd(one, logits, labels, st.bfloat16(), cnt, -1)
        with pytest.raises(RuntimeError, match="lse"):
            ext().ce_bwd(one, logits, labels, short, cnt, -1)
        with pytest.raises(RuntimeError, match="labels"):
            ext().ce_bwd(one, logits, labels[:-1], st, cnt, -1)
        ext().ce_bwd(one, logits, labels, st, cnt, -1)
    torch.cuda.synchronize()


def test_embedding_bwd_rejects_mismatched_operands():
    """dy carries the output dtype and is dispatched on; the saved z is
    always fp32, so a 16-bit z is the mixed-dtype case here."""
    B, S = 2, 2
    xf, xb, v, st, short = _rej_tensors()
    ids = torch.zeros(B, S, device=DEV, dtype=torch.long)
    none = torch.empty(0, device=DEV, dtype=torch.uint8)
    mask = torch.ones(ROWS_R, H_R, device=DEV, dtype=torch.uint8)
    dy = xf.view(B, S, H_R)

    def f(dy_, z, mask_, mean, rstd, p):
        return ext().embedding_ln_dropout_bwd(
            dy_, ids, None, z, mask_, v, mean, rstd, p, 5, 4, 0)

    with pytest.raises(RuntimeError, match="z.*" + BF_THEN_F):
        f(dy.bfloat16(), xb, none, st, st, 0.0)
    with pytest.raises(RuntimeError, match="z.*" + BF_THEN_F):
        f(dy, xb, none, st, st, 0.0)
    with pytest.raises(RuntimeError, match="dy"):
        f(dy[:, :1], xf, none, st, st, 0.0)
    with pytest.raises(RuntimeError, match="mean"):
        f(dy, xf, none, short, st, 0.0)
    with pytest.raises(RuntimeError, match="rstd"):
        f(dy, xf, none, st, short, 0.0)
    with pytest.raises(RuntimeError, match="mask"):
        f(dy, xf, none, st, st, 0.1)
    with pytest.raises(RuntimeError, match="exceeds max_pos"):
        ext().embedding_ln_dropout_bwd(  # S = 2 positions, a 1-row table
            dy, ids, None, xf, none, v, st, st, 0.0, 5, 1, 0)
    with pytest.raises(RuntimeError, match=r"H % 8 != 0"):
        z68 = torch.zeros(ROWS_R, 68, device=DEV)  # 68 % 4 == 0, % 8 != 0
        ext().embedding_ln_dropout_bwd(
            z68.view(B, S, 68).bfloat16(), ids, None, z68, none,
            torch.ones(68, device=DEV), st, st, 0.0, 5, 4, 0)
    f(dy, xf, mask, st, st, 0.1)
    f(dy.bfloat16(), xf, none, st, st, 0.0)  # 16-bit dy with fp32 z: valid
    torch.cuda.synchronize()
