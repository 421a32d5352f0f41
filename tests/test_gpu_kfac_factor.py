"""K-FAC factor kernel (csrc/ops/kfac_factor.hip) against fp64.

factor <- beta*factor + alpha*C with C the covariance of [x, 1] (or x),
computed from the same 16-bit inputs in fp64. Per-element bound

    (N + 3) * 2^-23 * (beta*|F_ij| + alpha*(|x|^T |x|)_ij)

The rigorous fp32 bound for a length-N sum in ANY order is
gamma_N ~ N * 2^-24 times the sum of magnitudes; it is doubled because
the MFMA's internal adds need not round per IEEE step, and the +3
covers the alpha product, the beta product and the final add. Nothing
here is a measured tolerance. Inputs carry a different scale per column,
so no tile is symmetric within itself and a transposed tile write cannot
hide. All tests @pytest.mark.gpu.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bert_pytorch_amd import ops
    from bert_pytorch_amd.ops import _reference as ref

DEV = "cuda:0"
EPS = 2.0 ** -23


def ext():
    return ops.extension()


def _inputs(N, K, dtype, seed=0):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    col_scale = torch.linspace(0.25, 2.0, K, device=DEV)
    x = torch.randn(N, K, device=DEV, generator=gen) * col_scale + 0.125
    return x.to(dtype)


def _aug64(x, has_bias):
    a = x.double()
    if has_bias:
        a = torch.cat([a, torch.ones(a.shape[0], 1, dtype=a.dtype, device=DEV)], 1)
    return a


def _sym_factor(D, seed=1):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    f = torch.randn(D, D, device=DEV, generator=gen)
    return (f + f.t()).contiguous()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("has_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("N", [256, 260, 1000])
@pytest.mark.parametrize("K", [128, 256, 384])
def test_factor_update_vs_fp64(K, N, has_bias, dtype):
    """K: one diagonal tile / first off-diagonal tile and its mirror /
    packed triangular index beyond two. N: the minimum / a tail shorter
    than the k-step / uneven split-K slices."""
    x = _inputs(N, K, dtype)
    a = _aug64(x, has_bias)
    cov = a.t() @ a
    cov_abs = a.abs().t() @ a.abs()
    D = K + int(has_bias)
    alpha0 = 1.0 / N
    for splitk in (0, 3):
        for beta, alpha, start in (
            (0.0, alpha0, torch.zeros(D, D, device=DEV)),
            (0.95, 0.05 * alpha0, _sym_factor(D)),
        ):
            coef = torch.tensor([beta, alpha], device=DEV)
            f1, f2 = start.clone(), start.clone()
            ext().kfac_factor_update(x, f1, coef, has_bias, splitk)
            ext().kfac_factor_update(x, f2, coef, has_bias, splitk)
            tag = f"splitk={splitk} beta={beta}"
            # the coefficients as the kernel holds them (fp32)
            b32, a32 = (float(v) for v in coef.double().cpu())
            want = b32 * start.double() + a32 * cov
            bound = (N + 3) * EPS * (b32 * start.double().abs() + a32 * cov_abs)
            err = (f1.double() - want).abs()
            worst = float((err / bound.clamp_min(1e-300)).max())
            print(f"K={K} N={N} bias={has_bias} {dtype} {tag}: "
                  f"max err/bound {worst:.3f}")
            assert torch.isfinite(f1).all(), tag
            assert bool((err <= bound).all()), f"{tag}: err/bound {worst}"
            assert torch.equal(f1, f1.t()), f"{tag}: not exactly symmetric"
            assert torch.equal(f1, f2), f"{tag}: not reproducible"


@pytest.mark.parametrize("has_bias", [False, True], ids=["nobias", "bias"])
def test_zero_alpha_leaves_factor_bit_identical(has_bias):
    K, N = 256, 260
    x = _inputs(N, K, torch.float16)
    x[::3] = float("inf")
    x[1::3] = float("nan")
    x[2::3, ::2] = float("-inf")
    D = K + int(has_bias)
    start = _sym_factor(D)
    f = start.clone()
    coef = torch.tensor([1.0, 0.0], device=DEV)
    ext().kfac_factor_update(x, f, coef, has_bias, 0)
    ext().kfac_factor_update(x, f, coef, has_bias, 3)
    assert torch.equal(f, start)
    # through the op wrapper too, and a finite update still lands after it
    assert ops.factor_update(x, f, None, None, has_bias, coef=coef) is True
    assert torch.equal(f, start)
    good = _inputs(N, K, torch.float16, seed=2)
    assert ops.factor_update(good, f, 0.5, 0.5 / N, has_bias) is True
    assert torch.isfinite(f).all() and not torch.equal(f, start)


@pytest.mark.parametrize("N,K", [(256, 96), (100, 128)], ids=["K96", "N100"])
def test_unsupported_shape_raises_and_routes_to_eager(N, K):
    assert not ext().kfac_factor_supported(N, K)
    x = _inputs(N, K, torch.bfloat16)
    D = K + 1
    f = torch.zeros(D, D, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext().kfac_factor_update(x, f, torch.tensor([0.0, 1.0], device=DEV), True, 0)
    assert not f.any()
    assert ops.factor_update(x, f, 0.0, 1.0 / N, True) is False
    a = _aug64(x, True)
    want = a.t() @ a / N
    bound = (N + 3) * EPS * (a.abs().t() @ a.abs()) / N
    assert bool(((f.double() - want).abs() <= bound).all())


def test_fp32_activations_route_to_eager():
    x = _inputs(256, 128, torch.float32)
    f = torch.zeros(128, 128, device=DEV)
    assert ops.factor_update(x, f, 0.0, 1.0 / 256, False) is False
    assert ops.factor_update(x.bfloat16(), f, 0.0, 1.0 / 256, False) is True
    assert ops.factor_update(x.bfloat16(), f, 0.0, 1.0 / 256, False, native=False) is False


def _train_step_factors(native_factors):
    """One bf16-autocast forward/backward of a 2-layer model with K-FAC
    attached. Returns {layer: (A, G)}, the per-factor magnitude sums
    alpha*|x|^T|x| (same keys) and the native update count."""
    from bert_pytorch_amd.config import BertConfig
    from bert_pytorch_amd.models import BertForPreTraining, BertPretrainingCriterion
    from bert_pytorch_amd.optim.kfac import KFAC

    torch.manual_seed(0)
    cfg = BertConfig(
        vocab_size_or_config_json_file=512, hidden_size=128,
        num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
        max_position_embeddings=64,
    )
    cfg.hidden_dropout_prob = 0.0
    cfg.attention_probs_dropout_prob = 0.0
    model = BertForPreTraining(cfg).to(DEV)
    criterion = BertPretrainingCriterion(cfg.vocab_size)
    kfac = KFAC(model, native_factors=native_factors)

    mags = {}
    inner = kfac._factor_update

    def recording(x2d, factor, beta, alpha, has_bias, coef=None):
        mag = torch.zeros_like(factor)
        with torch.autocast("cuda", enabled=False):  # A hooks run under it
            ref.kfac_factor_update(x2d.abs(), mag, beta, alpha, has_bias, coef)
        mags[factor.data_ptr()] = mag
        return inner(x2d, factor, beta, alpha, has_bias, coef)

    kfac._factor_update = recording

    gen = torch.Generator(device=DEV).manual_seed(11)
    B, S = 4, 64
    ids = torch.randint(0, 512, (B, S), device=DEV, generator=gen)
    mask = torch.ones_like(ids)
    labels = torch.full((B, S), -1, dtype=torch.long, device=DEV)
    labels[:, 3:9] = torch.randint(0, 512, (B, 6), device=DEV, generator=gen)
    nsp = torch.randint(0, 2, (B,), device=DEV, generator=gen)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        scores, rel, glabels = model(ids, torch.zeros_like(ids), mask,
                                     masked_lm_labels=labels)
        loss = criterion(scores, rel, glabels, nsp)
    loss.backward()
    torch.cuda.synchronize()
    factors, bounds = {}, {}
    for st in kfac.layers:
        factors[st.name] = (st.A, st.G)
        bounds[st.name] = tuple(
            None if f is None else mags[f.data_ptr()] for f in (st.A, st.G)
        )
    return factors, bounds, kfac.native_updates


def test_end_to_end_native_matches_eager_factors():
    nat, mag, n_native = _train_step_factors(None)
    eag, _, n_eager = _train_step_factors(False)
    assert n_native > 0 and n_eager == 0
    rows = 4 * 64
    kinds = ("attention.self", "attention.output.dense", "output.dense")
    seen = set()
    assert nat.keys() == eag.keys()
    for name, pair in nat.items():
        for which, f_nat, f_eag, m in zip("AG", pair, eag[name], mag[name]):
            if name.startswith("bert.encoder"):
                assert f_nat is not None and f_eag is not None, (name, which)
                seen.update(k for k in kinds if name.endswith(k))
            if f_nat is None:
                assert f_eag is None
                continue
            assert torch.isfinite(f_nat).all() and f_nat.abs().sum() > 0
            # each side is within (N+3)*2^-23*mag of the exact value
            bound = 2 * (rows + 3) * EPS * m.double()
            err = (f_nat.double() - f_eag.double()).abs()
            assert bool((err <= bound).all()), (
                name, which, float((err / bound.clamp_min(1e-300)).max()))
    assert seen == set(kinds)
