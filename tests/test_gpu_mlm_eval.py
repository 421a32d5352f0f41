"""Logits-free evaluation instantiation of the MLM head
(csrc/ops/mlm_head.hip, ``mlm_head_eval``) against the training
instantiation ``mlm_head_fwd``. The two run the same arithmetic, so every
comparison here is exact: bitwise for floats, equality for integers.
All tests @pytest.mark.gpu."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bert_pytorch_amd import ops

DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def ext():
    return ops.extension()


def _count_calls(monkeypatch, *names):
    """Wrap extension entry points so calls through ops.* are counted."""
    mod = ext()
    counts = {n: 0 for n in names}

    def wrap(name, fn):
        def inner(*a, **kw):
            counts[name] += 1
            return fn(*a, **kw)

        return inner

    for n in names:
        monkeypatch.setattr(mod, n, wrap(n, getattr(mod, n)))
    return counts


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32).cpu()


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(_bits(a), _bits(b))


def _inputs(P, V, K, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    h = (torch.randn(P, K, generator=g) * 0.5).to(DEV, dtype)
    w = (torch.randn(V, K, generator=g) * 0.5).to(DEV, dtype)
    b = torch.randn(V, generator=g).to(DEV)
    labels = torch.randint(0, V, (P,), generator=g)
    labels[::5] = -1
    return h, w, b, labels.to(DEV)


def _check_against_training(h, w, b, labels):
    """Every output of mlm_head_eval against mlm_head_fwd on the same
    inputs; returns (eval outputs, training logits widened on the CPU)."""
    V = w.shape[0]
    logits, loss_sum, count, lse = ext().mlm_head_fwd(h, w, b, labels, -1)
    e_loss, e_count, e_correct, e_lse, e_pred = ext().mlm_head_eval(
        h, w, b, labels, -1
    )
    assert e_pred.dtype == torch.int32 and e_pred.shape == labels.shape
    assert _same_bits(e_lse, lse), "lse differs from the training kernel"
    assert _same_bits(e_loss, loss_sum), (float(e_loss), float(loss_sum))
    assert _same_bits(e_count, count), (float(e_count), float(count))
    wide = logits.float().cpu()
    pred = e_pred.cpu().long()
    assert int(pred.min()) >= 0 and int(pred.max()) < V
    want = wide.argmax(dim=1)
    bad = (pred != want).nonzero().flatten().tolist()
    assert not bad, f"pred != argmax of the stored logits at rows {bad[:8]}"
    lab = labels.cpu()
    n_ok = int(((pred == lab) & (lab != -1)).sum())
    assert float(e_correct) == n_ok, (float(e_correct), n_ok)
    again = ext().mlm_head_eval(h, w, b, labels, -1)
    for first, second in zip(
        (e_loss, e_count, e_correct, e_lse, e_pred), again
    ):
        assert torch.equal(first.cpu(), second.cpu()), "two calls differ"
    return (e_loss, e_count, e_correct, e_lse, e_pred), wide


# V=200: the fourth stripe (columns 192..255) has 8 valid columns and the
# waves past it none; 1000 and 4096 span several blocks along V; 30528 x
# 1024 is the pretraining shape, where bf16 logits tie at the top.
@pytest.mark.parametrize(
    "P,V,K,dt",
    [
        (256, 200, 64, "bf16"), (256, 200, 64, "fp16"),
        (256, 1000, 128, "bf16"), (256, 1000, 128, "fp16"),
        (512, 4096, 256, "bf16"), (512, 4096, 256, "fp16"),
        (1280, 30528, 1024, "bf16"),
    ],
)
def test_eval_matches_training_kernel(P, V, K, dt):
    h, w, b, labels = _inputs(P, V, K, DTYPES[dt], seed=P + V + K)
    _check_against_training(h, w, b, labels)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_ties_take_the_lowest_column(dt):
    """W row 3 (and its bias) copied to 4 (adjacent lane), 19 (same lane,
    next 16-column tile), 70 (another stripe of the block) and 700
    (another block): five columns hold the identical row maximum."""
    P, V, K = 256, 1000, 128
    h, w, b, labels = _inputs(P, V, K, DTYPES[dt], seed=7)
    copies = [4, 19, 70, 700]
    for c in copies:
        w[c] = w[3]
        b[c] = b[3]
    labels[:] = -1
    for row, lab in enumerate([3] + copies):
        h[row] = 4 * w[3]  # |4 w3|.|w3| = 4*|w3|^2 ~ 128 >> 4 w3.wj ~ 11
        labels[row] = lab
    (_, count, correct, _, pred), wide = _check_against_training(
        h, w, b, labels
    )
    top = wide[:5].max(dim=1).values
    for c in [3] + copies:
        assert torch.equal(wide[:5, c], top), "the tie was not constructed"
    assert pred[:5].tolist() == [3] * 5
    assert float(count) == 5 and float(correct) == 1


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_constant_row_predicts_column_zero(dt):
    P, V, K = 256, 1000, 128
    h, w, b, labels = _inputs(P, V, K, DTYPES[dt], seed=8)
    b[:] = 0.25
    h[0] = 0
    (_, _, _, _, pred), _ = _check_against_training(h, w, b, labels)
    assert int(pred[0]) == 0


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_vocab_tail_never_wins(dt):
    """V=1000 leaves 24 masked columns in the last block. With h == 0 and
    bias == -5 every real logit is -5; a masked column that entered the
    statistics would carry logit 0 and win."""
    P, V, K = 256, 1000, 128
    h, w, b, labels = _inputs(P, V, K, DTYPES[dt], seed=9)
    b[:] = -5.0
    h[0] = 0
    (_, _, _, _, pred), _ = _check_against_training(h, w, b, labels)
    assert int(pred[0]) == 0
    # the last valid column far below every other: the clamped W rows the
    # staging loop re-reads for columns >= V repeat exactly that column
    b[999] = -1.0e4
    labels[1] = 999
    (_, _, _, _, pred), _ = _check_against_training(h, w, b, labels)
    assert int(pred.max()) < V and int(pred.min()) >= 0
    assert int((pred == 999).sum()) == 0


def test_model_eval_matches_training_loss(monkeypatch):
    from bert_pytorch_amd.config import BertConfig
    from bert_pytorch_amd.models import BertForPreTraining
    from bert_pytorch_amd.ops import rng

    torch.manual_seed(21)
    config = BertConfig(
        vocab_size_or_config_json_file=1000, hidden_size=128,
        num_hidden_layers=2, num_attention_heads=2,
        intermediate_size=256, max_position_embeddings=32,
    )
    model = BertForPreTraining(config).to(DEV).eval()
    B, S, MAXP = 8, 32, 5
    ids = torch.randint(0, 1000, (B, S), device=DEV)
    tt = torch.zeros_like(ids)
    mask = torch.ones_like(ids)
    mask[:, 28:] = 0
    labels = torch.full_like(ids, -1)
    labels[:, 3:7] = ids[:, 3:7]
    kw = dict(masked_lm_labels=labels, max_predictions_per_seq=MAXP)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        loss, _, _ = model(ids, tt, mask, compute_mlm_loss=True, **kw)
        counts = _count_calls(monkeypatch, "mlm_head_eval", "mlm_head_fwd")
        offset = rng._offset
        ev, rel, gathered = model(ids, tt, mask, mlm_eval=True, **kw)
        assert rng._offset == offset, "evaluation drew from the Philox counter"
    assert counts == {"mlm_head_eval": 1, "mlm_head_fwd": 0}
    assert isinstance(ev, ops.MlmEval)
    assert ev.pred.shape == gathered.shape == (B * MAXP,)
    assert rel.shape == (B, 2)
    assert float(ev.count) == B * 4
    assert _same_bits(ev.loss_sum / ev.count.clamp(min=1), loss)
    assert float(ev.correct) == int((ev.pred == gathered).sum())
    assert not ev.loss_sum.requires_grad
