"""Span masking on the device (the span instantiation of the row kernel and
the scatter kernel of csrc/ops/mlm_mask.hip, ``ops.mlm_mask(...,
span_table=)``).

The expected values come from ``spec_mlm_mask_span``, the sequential
plain-Python specification in tests/mlm_span_spec.py; the cases are that
file's too, each computed once per session. The kernel runs with sync
debugging set to raise. Integer arithmetic end to end: every comparison is
``torch.equal``. All tests @pytest.mark.gpu.
"""

import numpy as np
import pytest
import torch

from mlm_mask_spec import MASK, NAMES, VOCAB, assert_equal_spec, random_rows, run_op
from mlm_span_spec import (SPAN_CASES, check_span_case_facts, run_span_op,
                           span_spec_of)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bert_pytorch_amd import ops
    from bert_pytorch_amd.config import BertConfig
    from bert_pytorch_amd.data import DeviceMasker
    from bert_pytorch_amd.ops import _reference
    from bert_pytorch_amd.models import (BertForPreTraining,
                                         BertPretrainingCriterion)

DEV = "cuda:0"


def run_without_sync(case, dense_labels=True):
    """The op on the device, with every input uploaded beforehand and sync
    debugging set to raise: it reads nothing back."""
    S = case["input_ids"].shape[1]
    ids = torch.from_numpy(np.asarray(case["input_ids"], np.int32)).to(DEV)
    special = torch.from_numpy(np.asarray(case["special"], np.int32)).to(DEV)
    index = torch.from_numpy(
        np.asarray(case["sample_index"], np.int64)).to(DEV)
    words = torch.from_numpy(np.asarray(case["word_continues"])).to(DEV)
    count = ops.mlm_count_table(
        S, case["masked_lm_prob"],
        case.get("table_max_pred") or case["max_pred"]).to(DEV)
    spans = ops.mlm_span_table(case["span_p"], case["span_max"]).to(DEV)
    t_keep, t_rand = ops.mlm_thresholds(0.1, 0.1)
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:  # noqa: BLE001
        pytest.fail(f"sync debug mode is not available on this build: {e}")
    try:
        return ops.mlm_mask(
            ids, special, index, count, seed=case["seed"],
            epoch=case["epoch"], max_pred=case["max_pred"], vocab_size=VOCAB,
            mask_token=MASK, t_keep=t_keep, t_rand=t_rand,
            dense_labels=dense_labels, word_continues=words, span_table=spans,
        )
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.mark.parametrize("name", list(SPAN_CASES))
def test_kernel_equals_spec(name):
    case, want, trace = span_spec_of(name)
    check_span_case_facts(name, case, want, trace)
    got = run_without_sync(case)
    assert all(t.is_cuda for t in got)
    assert_equal_spec(got, want)


def test_dense_labels_on_request_only():
    case, want, _ = span_spec_of("two_specials")
    assert_equal_spec(run_without_sync(case, dense_labels=False), want,
                      dense_labels=False)


@pytest.mark.parametrize("name", ["S128_two_rounds", "B300_S16_prefix",
                                  "vocab_edge_ids", "Lmax32_small_p"])
def test_torch_twin_on_the_device_equals_the_kernel(name):
    case, _, _ = span_spec_of(name)
    got = run_span_op(**case, device=DEV)
    S = case["input_ids"].shape[1]
    twin = _reference.mlm_mask_span(
        torch.from_numpy(np.asarray(case["input_ids"], np.int32)).to(DEV),
        torch.from_numpy(np.asarray(case["special"], np.int32)).to(DEV),
        torch.from_numpy(np.asarray(case["sample_index"], np.int64)).to(DEV),
        ops.mlm_count_table(S, case["masked_lm_prob"],
                            case.get("table_max_pred")
                            or case["max_pred"]).to(DEV),
        torch.from_numpy(np.asarray(case["word_continues"])).to(DEV),
        ops.mlm_span_table(case["span_p"], case["span_max"]).to(DEV),
        case["seed"], case["epoch"], case["max_pred"], VOCAB, MASK,
        *ops.mlm_thresholds(0.1, 0.1))
    assert all(t.is_cuda for t in twin)
    for n, g, f in zip(NAMES, got, twin):
        assert torch.equal(g, f), n
    fallback = run_span_op(**case, device="cpu")
    for n, g, f in zip(NAMES, got, fallback):
        assert torch.equal(g.cpu(), f), n


@pytest.mark.parametrize("name", ["S128_two_rounds", "crafted_S16",
                                  "B300_S16_prefix", "S1024_B2",
                                  "max_pred_below_table"])
def test_max_length_one_equals_the_whole_word_kernel(name):
    case = dict(span_spec_of(name)[0], span_max=1)
    span = run_span_op(**case, device=DEV)
    case.pop("span_p"), case.pop("span_max")
    whole = run_op(case.pop("input_ids"), case.pop("special"),
                   case.pop("sample_index"), case.pop("word_continues"),
                   **case, device=DEV)
    for k in (1, 2, 3, 4, 5):  # all but masked_ids
        assert torch.equal(span[k], whole[k]), NAMES[k]
    free = whole[5] == -1
    assert torch.equal(span[0][free], whole[0][free])
    assert bool((whole[5] != -1).any())


def test_two_calls_are_bitwise_equal():
    case, _, _ = span_spec_of("S1024_B2")
    first = run_span_op(**case, device=DEV)
    second = run_span_op(**case, device=DEV)
    for n, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), n


def test_a_sample_has_one_mask_in_any_batch():
    case, want, _ = span_spec_of("S128_two_rounds")
    index = np.asarray(case["sample_index"])
    for pick in ([3, 1], [0, 2, 2, 3, 1]):
        sub = dict(case, input_ids=case["input_ids"][pick],
                   special=case["special"][pick], sample_index=index[pick])
        got = run_span_op(**sub, device=DEV)
        for row, src in enumerate(pick):
            for k in (0, 1, 2, 5):
                assert torch.equal(got[k][row].cpu(),
                                   torch.from_numpy(want[k][src]))


def test_entry_point_checks():
    """Every bad span table is stopped on the host, before any launch."""
    ext = ops.extension()
    ids = torch.zeros(2, 16, dtype=torch.int32, device=DEV)
    special = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    index = torch.zeros(2, dtype=torch.int64, device=DEV)
    table = torch.zeros(17, dtype=torch.int32, device=DEV)
    words = torch.zeros(VOCAB, dtype=torch.uint8, device=DEV)
    spans = ops.mlm_span_table(0.2, 10).to(DEV)
    tail = (1, 0, 4, VOCAB, MASK, 1, 1, False)
    out = ext.mlm_mask_span(ids, special, index, table, words, spans, *tail)
    assert len(out) == 5
    for bad in (
        spans.int(),                                        # dtype
        spans.cpu(),                                        # device
        spans[:0],                                          # Lmax = 0
        torch.zeros(33, dtype=torch.int64, device=DEV),     # Lmax > 32
        torch.zeros(20, dtype=torch.int64, device=DEV)[::2],
        spans.reshape(1, 10),                               # rank
    ):
        with pytest.raises(RuntimeError, match="span_table"):
            ext.mlm_mask_span(ids, special, index, table, words, bad, *tail)
    with pytest.raises(RuntimeError, match="word_continues"):
        ext.mlm_mask_span(ids, special, index, table, words[:-1], spans, *tail)
    with pytest.raises(ValueError, match="word_continues"):
        ops.mlm_mask(ids, special, index, table, seed=1, epoch=0, max_pred=4,
                     vocab_size=VOCAB, mask_token=MASK, t_keep=1, t_rand=1,
                     span_table=spans)


@pytest.mark.parametrize("unpad", [False, True], ids=["padded", "unpad"])
def test_device_masker_with_spans_feeds_the_model(unpad):
    torch.manual_seed(0)
    config = BertConfig(
        vocab_size_or_config_json_file=1024, hidden_size=128,
        num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
        max_position_embeddings=64,
    )
    model = BertForPreTraining(config).to(DEV)
    model.unpad_inputs(unpad)
    criterion = BertPretrainingCriterion(config.vocab_size)
    B, S, max_pred = 6, 64, 12
    ids, special = random_rows(B, S, seed=12)
    ids = (ids % 900) + 110
    words = torch.from_numpy(
        (np.random.default_rng(5).random(1024) < 0.4).astype(np.uint8))
    masker = DeviceMasker(seed=42, mask_token_index=MASK,
                          max_pred_per_seq=max_pred, masked_lm_prob=0.2,
                          vocab_size=1024, word_continues=words,
                          span_max_length=10, span_geometric_p=0.2)
    batch = [torch.from_numpy(ids).to(DEV), torch.from_numpy(special).to(DEV),
             torch.randint(0, 2, (B,), device=DEV),
             torch.arange(B, device=DEV)]
    masked, tt, am, positions, gathered, nsp = masker(batch, epoch=0)
    assert int((gathered != -1).sum()) > B
    assert int(masked.max()) < 1024
    with torch.autocast("cuda", dtype=torch.bfloat16):
        scores, rel, labels = model(
            masked, tt, am, masked_lm_labels=gathered,
            max_predictions_per_seq=max_pred, compute_mlm_loss=True,
            masked_lm_positions=positions)
        loss = criterion(scores, rel, labels, nsp)
    loss.backward()
    value = float(loss.detach())
    assert value == value and value > 0
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
