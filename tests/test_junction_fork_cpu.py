"""The forked junction output on the eager (CPU) path: a pair of handles
on one output, with the forward value and every gradient exactly those of
the single-output path."""

import torch

from bert_pytorch_amd import ops
from bert_pytorch_amd.models.bert import BertEncoder


def _junction_inputs():
    g = torch.Generator().manual_seed(3)
    mk = lambda *s: torch.randn(*s, generator=g).requires_grad_(True)  # noqa: E731
    return [mk(2, 8, 64), mk(64), mk(2, 8, 64), mk(64), mk(64)]


def _consume(a, b):
    # two consumers with different weights, as the next linear and the
    # next residual input are
    return (a * 3.0).sum() + (b * b).sum()


def test_fork_pair_matches_single_output():
    x, bias, res, w, b = _junction_inputs()
    y = ops.fused_bias_dropout_residual_ln(x, bias, res, w, b, 0.0, True)
    _consume(y, y).backward()
    ref = [t.grad.clone() for t in (x, bias, res, w, b)]
    for t in (x, bias, res, w, b):
        t.grad = None
    pair = ops.fused_bias_dropout_residual_ln(x, bias, res, w, b, 0.0, True,
                                              fork=True)
    assert isinstance(pair, tuple) and len(pair) == 2
    ya, yb = pair
    assert ya is not yb and ya.data_ptr() == yb.data_ptr()
    assert torch.equal(ya, y) and torch.equal(yb, y)
    _consume(ya, yb).backward()
    for t, r in zip((x, bias, res, w, b), ref):
        assert torch.equal(t.grad, r)


def test_fork_pair_one_handle_unused():
    x, bias, res, w, b = _junction_inputs()
    ya, _ = ops.fused_bias_dropout_residual_ln(x, bias, res, w, b, 0.0, True,
                                               fork=True)
    ya.sum().backward()
    got = x.grad.clone()
    x.grad = None
    ops.fused_bias_dropout_residual_ln(x, bias, res, w, b, 0.0, True).sum().backward()
    assert torch.equal(got, x.grad)


def test_encoder_forks_between_layers(tiny_config):
    """BertEncoder (plain and checkpointed) against the same layers
    chained by hand through their single-tensor interface."""
    tiny_config.hidden_dropout_prob = 0.0
    tiny_config.attention_probs_dropout_prob = 0.0
    torch.manual_seed(0)
    enc = BertEncoder(tiny_config).train()
    with torch.no_grad():  # the packed QKV weights are left to the model's init
        for p in enc.parameters():
            p.normal_(0.0, 0.1)
    x = torch.randn(2, 16, tiny_config.hidden_size, requires_grad=True)
    seqlens = torch.tensor([16, 11], dtype=torch.int32)

    h = x
    for layer in enc.layer:
        h = layer(h, seqlens)
        assert isinstance(h, torch.Tensor)
    h.pow(2).sum().backward()
    ref_out = h.detach().clone()
    ref = {n: p.grad.clone() for n, p in enc.named_parameters()}
    ref_x = x.grad.clone()

    for ckpt in (False, True):
        enc.zero_grad(set_to_none=True)
        x.grad = None
        enc._checkpoint_activations = ckpt
        out = enc(x, seqlens)[-1]
        assert isinstance(out, torch.Tensor) and torch.equal(out, ref_out)
        out.pow(2).sum().backward()
        assert torch.equal(x.grad, ref_x)
        for n, p in enc.named_parameters():
            assert torch.equal(p.grad, ref[n]), n
