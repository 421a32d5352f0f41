"""The gate of fused gradient accumulation.

The native backward entry points can add a parameter's gradient into an
existing ``p.grad`` inside the kernel that produces it (``acc`` /
``*_acc`` operands) instead of writing it out for autograd's
``AccumulateGrad`` to read back and add. A Function's backward that does
so returns ``None`` for that parameter. ``accum_target`` answers whether
it may: it returns ``p.grad`` to add into, or ``None`` for the ordinary
path. It says yes only if all of this holds:

* the extension is in use and ``p`` is a CUDA leaf ``nn.Parameter`` (the
  very tensor the Function was given, not a cast copy of it);
* ``p.grad`` exists, strided and contiguous, on ``p``'s device, with the
  dtype and shape the native entry point expects, and no tensor or
  post-accumulate hook sits on ``p`` (they would see no gradient);
* the engine is going to run ``p``'s ``AccumulateGrad`` node in this very
  backward pass. ``torch.autograd.grad`` and ``backward(inputs=[...])``
  over other tensors must never write into ``.grad``; for them
  ``torch._C._will_engine_execute_node`` is false or raises;
* the process-wide switch is on. ``BPA_FUSED_GRAD_ACCUM=0`` (read per
  call) turns it off, and so does ``set_enabled(False)``, which
  ``parallel/comm.py::wrap_ddp`` calls when it really wraps: DDP's reducer
  hooks live on the ``AccumulateGrad`` nodes.

The ``AccumulateGrad`` node of a parameter is looked up once and kept: the
parameter itself holds it only weakly, and a node rebuilt later would be
another object than the one in the running graph. The node in turn owns
the parameter, so a parameter that has been fused once lives until
``clear()`` drops the kept nodes; a process that builds one model after
another (sweeps, tests) calls it between them.

The fused result is bit for bit the unfused one where a parameter gets
its gradient from one fused Function per backward pass, as every
parameter of the BERT models here does. A parameter shared by two fused
call sites would get ``(grad + g1) + g2`` where the engine adds
``grad + (g1 + g2)``: right, but not to the last bit.
"""

from __future__ import annotations

import os
from typing import Dict, Optional

import torch

from . import has_extension

_enabled = True
_nodes: Dict[int, "torch.autograd.graph.Node"] = {}


def set_enabled(on: bool) -> None:
    """Process-wide switch (on by default)."""
    global _enabled
    _enabled = bool(on)


def clear() -> None:
    """Forget the kept ``AccumulateGrad`` nodes, and with them the hold on
    their parameters. Not during a backward pass."""
    _nodes.clear()


def enabled() -> bool:
    return _enabled and os.environ.get("BPA_FUSED_GRAD_ACCUM") != "0"


def _accumulate_node(p: torch.Tensor):
    node = _nodes.get(id(p))
    if node is None:
        with torch.enable_grad():
            node = p.view_as(p).grad_fn.next_functions[0][0]
        # the node keeps p alive, so id(p) is never handed out again
        _nodes[id(p)] = node
    return node


def will_accumulate(p: torch.Tensor) -> bool:
    """True if the running backward pass executes ``p``'s
    ``AccumulateGrad`` node, i.e. is going to write ``p.grad``."""
    try:
        return bool(torch._C._will_engine_execute_node(_accumulate_node(p)))
    except RuntimeError:
        # outside a backward pass, or torch.autograd.grad over p itself
        return False


def accum_target(p, dtype: torch.dtype, shape) -> Optional[torch.Tensor]:
    """``p.grad`` if this backward may add ``p``'s gradient (of ``dtype``
    and ``shape``) into it in place and return ``None`` for ``p``."""
    if not enabled():
        return None
    if not (
        isinstance(p, torch.nn.Parameter)
        and p.is_cuda
        and p.is_leaf
        and p.requires_grad
    ):
        return None
    if not has_extension() or os.environ.get("BPA_FORCE_EAGER") == "1":
        return None
    g = p.grad
    if (
        g is None
        or g.dtype != dtype
        or g.shape != torch.Size(shape)
        or g.layout != torch.strided
        or g.device != p.device
        or not g.is_contiguous()
        or p._backward_hooks
        or getattr(p, "_post_accumulate_grad_hooks", None)
    ):
        return None
    # create_graph=True keeps grad mode on and accumulates out of place
    if torch.is_grad_enabled() or g.requires_grad:
        return None
    return g if will_accumulate(p) else None
