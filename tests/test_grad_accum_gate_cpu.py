"""The gate of fused gradient accumulation (ops/grad_accum.py), as far as
it can be checked without a GPU: what it refuses, what the autograd engine
tells it, that CPU training is untouched and that a single-process
``wrap_ddp`` leaves the switch on.
"""

import json
import os

import torch

from bert_pytorch_amd.ops import grad_accum

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "grad_accum_cpu_two_steps.json")


def _param(shape=(4, 3), dtype=torch.float32, grad=True):
    p = torch.nn.Parameter(torch.randn(*shape, dtype=dtype))
    if grad:
        p.grad = torch.zeros_like(p)
    return p


class _Probe(torch.autograd.Function):
    """y = x * w; its backward records what the gate's engine query says
    about w, and adds w's gradient in place (returning None) if told to."""

    seen = []

    @staticmethod
    def forward(ctx, x, w, fuse):
        ctx.save_for_backward(x, w)
        ctx.w, ctx.fuse = w, fuse
        return x * w

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        will = grad_accum.will_accumulate(ctx.w)
        _Probe.seen.append(will)
        if ctx.fuse and will and ctx.w.grad is not None:
            ctx.w.grad.add_(dy * x)
            return dy * w, None, None
        return dy * w, dy * x, None


def _probe(call, fuse=False):
    w = torch.nn.Parameter(torch.tensor([1.0, 2.0, 3.0]))
    x = torch.tensor([0.5, 0.25, 2.0], requires_grad=True)
    _Probe.seen = []
    out = call(_Probe.apply(x, w, fuse).sum(), x, w)
    assert len(_Probe.seen) == 1
    return _Probe.seen[0], out, x, w


def test_engine_query_follows_what_the_pass_will_write():
    assert _probe(lambda l, x, w: l.backward())[0] is True
    assert _probe(lambda l, x, w: l.backward(inputs=[w]))[0] is True
    assert _probe(lambda l, x, w: l.backward(inputs=[x]))[0] is False
    will, (gx,), x, w = _probe(lambda l, x, w: torch.autograd.grad(l, [x]))
    assert will is False and w.grad is None
    # autograd.grad over w itself: the engine query raises, the gate says no
    will, (gw,), x, w = _probe(lambda l, x, w: torch.autograd.grad(l, [w]))
    assert will is False and w.grad is None
    assert torch.equal(gw, x.detach())
    # outside any backward pass
    assert grad_accum.will_accumulate(_param()) is False


def test_none_plus_in_place_add_accumulates_once():
    w = torch.nn.Parameter(torch.tensor([1.0, 2.0, 3.0]))
    x = torch.tensor([0.5, 0.25, 2.0], requires_grad=True)
    for _ in range(2):
        _Probe.apply(x, w, True).sum().backward()
    assert torch.equal(w.grad, 2 * x.detach())
    # autograd.grad never writes .grad, fused or not
    before = w.grad.clone()
    (gw,) = torch.autograd.grad(_Probe.apply(x, w, True).sum(), [w])
    assert torch.equal(gw, x.detach()) and torch.equal(w.grad, before)


def test_clear_releases_the_kept_nodes():
    import gc
    import weakref

    w = torch.nn.Parameter(torch.tensor([1.0, 2.0]))
    x = torch.tensor([0.5, 0.25], requires_grad=True)
    _Probe.apply(x, w, True).sum().backward()  # looks w's node up
    assert id(w) in grad_accum._nodes
    ref = weakref.ref(w)
    grad_accum.clear()
    assert not grad_accum._nodes
    del w
    gc.collect()
    assert ref() is None


def test_gate_refuses(monkeypatch):
    monkeypatch.delenv("BPA_FUSED_GRAD_ACCUM", raising=False)
    assert grad_accum.enabled()
    p = _param()
    # a CPU parameter, even with everything else in order
    assert grad_accum.accum_target(p, p.dtype, p.shape) is None
    assert grad_accum.accum_target(None, torch.float32, (3,)) is None
    assert grad_accum.accum_target(p.detach(), p.dtype, p.shape) is None
    assert grad_accum.accum_target(p * 2, p.dtype, p.shape) is None  # non-leaf
    assert grad_accum.accum_target(_param(grad=False), p.dtype, p.shape) is None


def test_gate_refuses_before_asking_the_engine(monkeypatch):
    """Pretend the parameter is on the GPU and the engine says yes: the
    remaining conditions are what is left to refuse."""
    monkeypatch.delenv("BPA_FUSED_GRAD_ACCUM", raising=False)
    monkeypatch.delenv("BPA_FORCE_EAGER", raising=False)
    monkeypatch.setattr(grad_accum, "has_extension", lambda: True)
    monkeypatch.setattr(grad_accum, "will_accumulate", lambda p: True)

    class GpuParam(torch.nn.Parameter):
        is_cuda = True

    def make(grad=True):
        p = GpuParam(torch.randn(4, 3))
        if grad:
            p.grad = torch.zeros(4, 3)
        return p

    with torch.no_grad():  # as inside a backward pass
        p = make()
        assert grad_accum.accum_target(p, torch.float32, (4, 3)) is p.grad
        assert grad_accum.accum_target(make(False), torch.float32, (4, 3)) is None
        assert grad_accum.accum_target(p, torch.bfloat16, (4, 3)) is None
        assert grad_accum.accum_target(p, torch.float32, (3, 4)) is None
        assert grad_accum.accum_target(p, torch.float32, (12,)) is None
        q = make(False)
        q.grad = torch.zeros(3, 4).t()  # right shape, not contiguous
        assert grad_accum.accum_target(q, torch.float32, (4, 3)) is None
        assert grad_accum.accum_target(p * 1, torch.float32, (4, 3)) is None
        frozen = make()
        frozen.requires_grad_(False)
        assert grad_accum.accum_target(frozen, torch.float32, (4, 3)) is None
        hooked = make()
        hooked.register_hook(lambda g: g)
        assert grad_accum.accum_target(hooked, torch.float32, (4, 3)) is None
        # the switch, both ways of turning it off
        monkeypatch.setenv("BPA_FUSED_GRAD_ACCUM", "0")
        assert grad_accum.accum_target(p, torch.float32, (4, 3)) is None
        monkeypatch.setenv("BPA_FUSED_GRAD_ACCUM", "1")
        assert grad_accum.accum_target(p, torch.float32, (4, 3)) is p.grad
        grad_accum.set_enabled(False)
        try:
            assert grad_accum.accum_target(p, torch.float32, (4, 3)) is None
        finally:
            grad_accum.set_enabled(True)
        assert grad_accum.accum_target(p, torch.float32, (4, 3)) is p.grad
        monkeypatch.setenv("BPA_FORCE_EAGER", "1")
        assert grad_accum.accum_target(p, torch.float32, (4, 3)) is None
    # grad mode on (create_graph): accumulation is out of place
    monkeypatch.delenv("BPA_FORCE_EAGER")
    with torch.enable_grad():
        assert grad_accum.accum_target(p, torch.float32, (4, 3)) is None


def test_wrap_ddp_single_process_leaves_switch_on(tiny_config):
    from bert_pytorch_amd.models import BertForPreTraining
    from bert_pytorch_amd.parallel import comm

    model = BertForPreTraining(tiny_config)
    assert comm.wrap_ddp(model, 0) is model
    assert grad_accum.enabled()


def cpu_two_step_summary(tiny_config):
    """Two accumulated CPU micro-steps of the tiny model; per parameter the
    fp64 sum and L2 norm of the accumulated gradient, and its size."""
    from bert_pytorch_amd.models import (BertForPreTraining,
                                         BertPretrainingCriterion)

    torch.manual_seed(3)
    model = BertForPreTraining(tiny_config).train()
    criterion = BertPretrainingCriterion(tiny_config.vocab_size)
    g = torch.Generator().manual_seed(4)
    for _ in range(2):
        ids = torch.randint(0, 512, (2, 32), generator=g)
        mask = torch.ones_like(ids)
        mask[:, 24:] = 0
        labels = torch.full((2, 32), -1, dtype=torch.long)
        labels[:, 3:8] = torch.randint(0, 512, (2, 5), generator=g)
        nsp = torch.randint(0, 2, (2,), generator=g)
        scores, rel, glabels = model(ids, torch.zeros_like(ids), mask,
                                     masked_lm_labels=labels)
        (criterion(scores, rel, glabels, nsp) / 2).backward()
    return {n: [float(p.grad.double().sum()),
                float(p.grad.double().norm()), p.grad.numel()]
            for n, p in model.named_parameters() if p.grad is not None}


def test_cpu_training_gradients_unchanged(tiny_config):
    """Against the values the parent commit gave (tests/golden). fp32
    sums may be re-associated by the CPU GEMM library from one machine to
    the next: 1e-4 of the gradient's norm is some hundred times the fp32
    rounding of these few-thousand-term sums and far below any real change."""
    with open(GOLDEN) as f:
        want = json.load(f)
    got = cpu_two_step_summary(tiny_config)
    assert got.keys() == want.keys() and len(got) > 30
    for n in want:
        tol = 1e-4 * want[n][1] + 1e-12
        assert abs(got[n][1] - want[n][1]) <= tol, n
        # |sum of a difference| <= sqrt(numel) * its norm
        assert got[n][2] == want[n][2], n
        assert abs(got[n][0] - want[n][0]) <= tol * want[n][2] ** 0.5, n
