"""K-FAC layer coverage, loss scaling and the non-finite gate (CPU).

The preconditioner must collect factors for every linear it registers
under the encoder (packed QKV, attention output, FFN output - the last
two are modules whose forward is the bias-free GEMM), must not change
what the model computes, must accumulate G from unscaled gradients when
given the loop's GradScaler, and must skip a G update whose gradient
holds a non-finite value.
"""

import torch
from torch import nn

from bert_pytorch_amd.config import BertConfig
from bert_pytorch_amd.models import BertForPreTraining, BertPretrainingCriterion
from bert_pytorch_amd.ops import _reference
from bert_pytorch_amd.optim.kfac import KFAC


def _tiny_config(dropout=None):
    cfg = BertConfig(
        vocab_size_or_config_json_file=128, hidden_size=32,
        num_hidden_layers=2, num_attention_heads=2,
        intermediate_size=64, max_position_embeddings=32,
    )
    if dropout is not None:
        cfg.hidden_dropout_prob = dropout
        cfg.attention_probs_dropout_prob = dropout
    return cfg


def _tiny_batch():
    gen = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 128, (4, 16), generator=gen)
    mask = torch.ones(4, 16, dtype=torch.long)
    labels = torch.full((4, 16), -1, dtype=torch.long)
    labels[:, 2:5] = torch.randint(0, 128, (4, 3), generator=gen)
    nsp = torch.zeros(4, dtype=torch.long)
    return ids, mask, labels, nsp


def _forward_backward(model, criterion):
    ids, mask, labels, nsp = _tiny_batch()
    scores, rel, glabels = model(ids, None, mask, masked_lm_labels=labels)
    criterion(scores, rel, glabels, nsp).backward()
    return scores, rel


def test_every_encoder_linear_gets_factors():
    torch.manual_seed(0)
    model = BertForPreTraining(_tiny_config())
    kfac = KFAC(model)
    _forward_backward(model, BertPretrainingCriterion(128))
    kfac.step()

    enc = [st for st in kfac.layers if st.name.startswith("bert.encoder")]
    kinds = {st.name.split("layer.")[1].split(".", 1)[1] for st in enc}
    assert kinds == {"attention.self", "attention.output.dense", "output.dense"}
    assert len(enc) == 3 * 2
    for st in enc:
        out_f, in_f = st.weight().shape
        assert st.has_bias
        assert st.A is not None and st.G is not None, st.name
        assert st.A.shape == (in_f + 1, in_f + 1), st.name
        assert st.G.shape == (out_f, out_f), st.name
        assert st.A_inv is not None and st.A_inv.shape == st.A.shape, st.name
        assert st.G_inv is not None and st.G_inv.shape == st.G.shape, st.name
        assert torch.isfinite(st.A).all() and torch.isfinite(st.G).all()


def test_hooks_change_no_output_gradient_or_key():
    def run(with_kfac):
        torch.manual_seed(0)
        model = BertForPreTraining(_tiny_config(dropout=0.0))
        kfac = KFAC(model) if with_kfac else None
        scores, rel = _forward_backward(model, BertPretrainingCriterion(128))
        grads = {n: p.grad.clone() for n, p in model.named_parameters()
                 if p.grad is not None}
        return model, kfac, scores.detach(), rel.detach(), grads

    model, _, s0, r0, g0 = run(False)
    _, kfac, s1, r1, g1 = run(True)
    assert any(st.G is not None for st in kfac.layers)
    assert torch.equal(s0, s1) and torch.equal(r0, r1)
    assert g0.keys() == g1.keys() and g0
    for name in g0:
        assert torch.equal(g0[name], g1[name]), name
    keys = model.state_dict().keys()
    for layer in range(2):
        for mod in ("attention.output.dense", "output.dense"):
            for leaf in ("weight", "bias"):
                assert f"bert.encoder.layer.{layer}.{mod}.{leaf}" in keys


def _one_linear_G(scale_loss, **kfac_kwargs):
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(8, 6))
    kfac = KFAC(model, **kfac_kwargs)
    x = torch.randn(32, 8, generator=torch.Generator().manual_seed(1))
    for _ in range(2):  # first update and a running-average update
        loss = (model(x) ** 2).mean()
        scale_loss(loss).backward()
    return kfac.layers[0].G


def test_grad_scaler_unscales_G():
    scaler = torch.amp.GradScaler("cpu", init_scale=1024.0)
    assert scaler.is_enabled()
    plain = _one_linear_G(lambda loss: loss)
    scaled = _one_linear_G(scaler.scale, grad_scaler=scaler)
    # a power-of-two scale is exact in fp32 on both g and 1/scale^2
    torch.testing.assert_close(scaled, plain, rtol=1e-6, atol=0.0)
    unaware = _one_linear_G(scaler.scale)
    assert not torch.allclose(unaware, plain, rtol=1e-3)


def test_nonfinite_gradient_leaves_G_untouched():
    torch.manual_seed(0)
    scaler = torch.amp.GradScaler("cpu", init_scale=1024.0)
    model = nn.Sequential(nn.Linear(8, 6))
    kfac = KFAC(model, grad_scaler=scaler)
    st = kfac.layers[0]
    x = torch.randn(32, 8)
    scaler.scale((model(x) ** 2).mean()).backward()
    G0, A0 = st.G.clone(), st.A.clone()
    assert torch.isfinite(G0).all() and G0.abs().sum() > 0

    y = model(2 * x)
    y.backward(torch.full_like(y, float("inf")))
    assert torch.equal(st.G, G0)
    assert torch.isfinite(st.G).all()
    assert not torch.equal(st.A, A0)  # A is not gated
    assert torch.isfinite(st.A).all()

    # and the next finite micro-batch updates G again
    scaler.scale((model(x) ** 2).mean()).backward()
    assert not torch.equal(st.G, G0) and torch.isfinite(st.G).all()


def test_first_kept_update_after_dropped_ones_is_a_first_update():
    """A scaler that starts too high drops the first micro-batches; the
    first one that is kept must initialise G (beta = 0), not average it
    into the zeros the dropped ones left."""
    scaler = torch.amp.GradScaler("cpu", init_scale=1024.0)
    x = torch.randn(32, 8, generator=torch.Generator().manual_seed(1))

    def run(drop_first):
        torch.manual_seed(0)
        model = nn.Sequential(nn.Linear(8, 6))
        kfac = KFAC(model, grad_scaler=scaler)
        for _ in range(2 if drop_first else 0):
            y = model(x)
            y.backward(torch.full_like(y, float("nan")))
            assert not kfac.layers[0].G.any()
        for _ in range(2):
            scaler.scale((model(x) ** 2).mean()).backward()
        return kfac.layers[0].G

    assert torch.equal(run(True), run(False))


def test_reference_composite_is_the_old_formula():
    """ops._reference.kfac_factor_update against the expressions
    optim/kfac.py used to evaluate inline. N is a power of two, so
    folding 1/N (A) or N (G) into alpha rescales exactly and the results
    must be bit-equal."""
    gen = torch.Generator().manual_seed(5)
    decay = 0.95
    a1, a2 = (torch.randn(64, 12, generator=gen) for _ in range(2))

    def old_cov_A(a):
        a = a.reshape(-1, a.shape[-1]).float()
        ones = torch.ones(a.shape[0], 1, dtype=a.dtype, device=a.device)
        a = torch.cat([a, ones], dim=1)
        return a.t() @ a / a.shape[0]

    old = old_cov_A(a1)
    old.mul_(decay).add_(old_cov_A(a2), alpha=1 - decay)
    new = torch.zeros(13, 13)
    _reference.kfac_factor_update(a1, new, 0.0, 1.0 / 64, True)
    _reference.kfac_factor_update(a2, new, decay, (1 - decay) / 64, True)
    assert torch.equal(new, old)

    g1, g2 = (torch.randn(64, 6, generator=gen) * 1e-2 for _ in range(2))

    def old_cov_G(g):
        g = g.reshape(-1, g.shape[-1]).float()
        return g.t() @ g * g.shape[0]

    old = old_cov_G(g1)
    old.mul_(decay).add_(old_cov_G(g2), alpha=1 - decay)
    new = torch.zeros(6, 6)
    _reference.kfac_factor_update(g1, new, 0.0, 64.0, False)
    _reference.kfac_factor_update(g2, new, decay, (1 - decay) * 64, False)
    assert torch.equal(new, old)

    # the tensor form of {beta, alpha} agrees, and a zero alpha gates
    coef = torch.tensor([decay, (1 - decay) * 64])
    via_coef = torch.zeros(6, 6)
    _reference.kfac_factor_update(g1, via_coef, 0.0, 64.0, False)
    _reference.kfac_factor_update(g2, via_coef, None, None, False, coef)
    torch.testing.assert_close(via_coef, old, rtol=1e-6, atol=0.0)
    before = via_coef.clone()
    bad = torch.full((64, 6), float("nan"))
    _reference.kfac_factor_update(
        bad, via_coef, None, None, False, torch.tensor([1.0, 0.0])
    )
    assert torch.equal(via_coef, before)
