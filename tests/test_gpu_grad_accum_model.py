"""Fused gradient accumulation at model level (ops/grad_accum.py): with
``.grad`` populated, the native backward kernels add into it and the
Functions return ``None`` for those parameters. The switch must change no
bit of any gradient, must really engage, and must keep out of
``torch.autograd.grad`` and of backward passes that do not reach the
parameter. All tests need a GPU.

Model: 2 layers, hidden 128, 2 heads, intermediate 1024, B = 32, S = 128,
matmul weights in bf16 as bench.py sets them; FFN1's weight gradient
(K = 4096, M = 1024, N = 128) then takes the in-repo split-K kernel.
"""

import pytest
import torch
from torch.profiler import ProfilerActivity, profile

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, S, VOCAB = 32, 128, 1024


def _model(bf16_weights, seed=7):
    from bert_pytorch_amd.config import BertConfig
    from bert_pytorch_amd.models import (BertForPreTraining,
                                         BertPretrainingCriterion)

    torch.manual_seed(seed)
    config = BertConfig(
        vocab_size_or_config_json_file=VOCAB, hidden_size=128,
        num_hidden_layers=2, num_attention_heads=2, intermediate_size=1024,
        max_position_embeddings=S,
    )
    model = BertForPreTraining(config).to(DEV).train()
    if bf16_weights:
        for n, prm in model.named_parameters():
            if prm.dim() >= 2 and "LayerNorm" not in n:
                prm.data = prm.data.to(torch.bfloat16)
    return model, BertPretrainingCriterion(config.vocab_size)


def _batch(step):
    g = torch.Generator(device=DEV).manual_seed(100 + step)
    ids = torch.randint(0, VOCAB, (B, S), device=DEV, generator=g)
    mask = torch.ones_like(ids)
    mask[:, 100 + step:] = 0
    tt = torch.zeros_like(ids)
    labels = torch.full((B, S), -1, dtype=torch.long, device=DEV)
    labels[:, 5:15] = torch.randint(0, VOCAB, (B, 10), device=DEV, generator=g)
    nsp = torch.randint(0, 2, (B,), device=DEV, generator=g)
    return ids, tt, mask, labels, nsp


def _loss(model, criterion, step):
    """Forward of micro-step ``step``; dropout masks depend on the step
    alone, so a repeated forward is the same function."""
    from bert_pytorch_amd.ops import rng

    torch.manual_seed(1000 + step)
    rng.reset(1000 + step)
    ids, tt, mask, labels, nsp = _batch(step)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        scores, rel, glabels = model(ids, tt, mask, masked_lm_labels=labels,
                                     compute_mlm_loss=True)
        return criterion(scores, rel, glabels, nsp) / 3


def _grads(model):
    return {n: p.grad.clone() for n, p in model.named_parameters()
            if p.grad is not None}


def _accumulating_nodes(prof):
    """AccumulateGrad executions that accumulate. The engine also runs
    (and the profiler records) the node of a parameter whose Function
    returned None; such a run adds nothing and has no aten::add_ under it."""
    n = 0
    for e in prof.events():
        if e.name == "torch::autograd::AccumulateGrad" and any(
                c.name.startswith("aten::add") for c in e.cpu_children):
            n += 1
    return n


def _run(monkeypatch, switch, bf16_weights, steps=3):
    """``steps`` accumulated micro-steps; the gradients after each and the
    number of accumulating AccumulateGrad nodes of the second backward."""
    monkeypatch.setenv("BPA_FUSED_GRAD_ACCUM", switch)
    model, criterion = _model(bf16_weights)
    after, n_acc = [], None
    for step in range(steps):
        loss = _loss(model, criterion, step)
        if step == 1:
            with profile(activities=[ProfilerActivity.CPU]) as prof:
                loss.backward()
            n_acc = _accumulating_nodes(prof)
        else:
            loss.backward()
        after.append(_grads(model))
    return model, after, n_acc


def _admitted(model, bf16_weights):
    """Parameters whose gradient the gate lets the kernels add in place,
    from the model: per encoder layer the two junctions' bias, gamma and
    beta, the QKV bias, FFN1's bias, and each bf16 weight whose wgrad takes
    the in-repo kernel; in the MLM head's transform the bias-GELU bias and
    the LayerNorm pair (and its weight under the same rule). The embedding,
    the decoder, the pooler and the NSP head are not fused."""
    from bert_pytorch_amd.models.bert import (BertLayer,
                                              BertPredictionHeadTransform)
    from bert_pytorch_amd.ops import extension

    def weight(w, K):
        return int(bf16_weights and w.dtype == torch.bfloat16
                   and extension().wgrad_tn_profitable(K, w.shape[0],
                                                       w.shape[1]))

    n = 0
    for m in model.modules():
        if isinstance(m, BertLayer):
            n += 3 + 3 + 1 + 1
            n += weight(m.attention.self.qkv_weight, B * S)
            n += weight(m.attention.output.dense.weight, B * S)
            n += weight(m.intermediate.dense_act.weight, B * S)
            n += weight(m.output.dense.weight, B * S)
        elif isinstance(m, BertPredictionHeadTransform):
            n += 1 + 2
            n += weight(m.dense_act.weight, B * 10)  # labelled rows
    return n


def _assert_same(ga, gb):
    assert ga.keys() == gb.keys() and len(ga) > 30
    for n in ga:
        assert ga[n].dtype == gb[n].dtype, n
        assert torch.equal(ga[n], gb[n]), n


def test_switch_changes_no_gradient_bit_and_engages(monkeypatch):
    model, on, n_on = _run(monkeypatch, "1", True)
    _, off, n_off = _run(monkeypatch, "0", True)
    for a, b in zip(on, off):
        _assert_same(a, b)
    admitted = _admitted(model, True)
    # 2 x (8 + FFN1's weight) + 3
    assert admitted == 21
    assert n_off - n_on == admitted
    # accumulation really happened: step 2 changed the gradients
    name = "bert.encoder.layer.0.intermediate.dense_act.weight"
    assert on[0][name].dtype == torch.bfloat16
    assert not torch.equal(on[0][name], on[1][name])


def test_fp32_weights_under_autocast_are_not_fused(monkeypatch):
    model, on, n_on = _run(monkeypatch, "1", False, steps=2)
    _, off, n_off = _run(monkeypatch, "0", False, steps=2)
    for a, b in zip(on, off):
        _assert_same(a, b)
    admitted = _admitted(model, False)
    assert admitted == 19  # no weight: the Functions see cast copies
    assert n_off - n_on == admitted


def test_autograd_grad_and_partial_backward_leave_grad_alone(monkeypatch):
    monkeypatch.setenv("BPA_FUSED_GRAD_ACCUM", "1")
    model, criterion = _model(True)
    _loss(model, criterion, 0).backward()
    first = _grads(model)
    layer = model.bert.encoder.layer[0]
    params = [layer.intermediate.dense_act.weight,  # split-K wgrad
              layer.intermediate.dense_act.bias,
              layer.attention.self.qkv_bias,
              layer.output.LayerNorm.weight,
              model.cls.predictions.transform.LayerNorm.bias]
    names = {id(p): n for n, p in model.named_parameters()}

    # the same forward again: autograd.grad hands the gradients back ...
    got = torch.autograd.grad(_loss(model, criterion, 0), params)
    for p, g in zip(params, got):
        assert torch.equal(g, first[names[id(p)]]), names[id(p)]
    # ... and no .grad has moved
    _assert_same(_grads(model), first)

    # a backward pass that only reaches an activation
    seen = []
    hook = model.bert.embeddings.register_forward_hook(
        lambda mod, args, out: seen.append(out))
    loss = _loss(model, criterion, 0)
    hook.remove()
    act = seen[0][0] if isinstance(seen[0], (tuple, list)) else seen[0]
    assert act.requires_grad
    loss.backward(inputs=[act])
    assert act.grad is not None and bool(act.grad.abs().sum() > 0)
    _assert_same(_grads(model), first)

    # and an ordinary backward still doubles them, fused
    _loss(model, criterion, 0).backward()
    after = _grads(model)
    for p in params:
        n = names[id(p)]
        assert torch.equal(after[n], first[n] + first[n]), n
