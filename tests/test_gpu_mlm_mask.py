"""On-device MLM masking, token level (csrc/ops/mlm_mask.hip,
``ops.mlm_mask``).

The expected values come from ``spec_mlm_mask``, the numpy specification in
tests/mlm_mask_spec.py, which shares no code with the package; the cases are
that file's too, each computed once per session. The kernel is integer
arithmetic end to end, so every comparison is ``torch.equal``. All tests
@pytest.mark.gpu.
"""

import numpy as np
import pytest
import torch

from mlm_mask_spec import (
    MASK,
    NAMES,
    TOKEN_CASES as CASES,
    VECTORS,
    VOCAB,
    assert_equal_spec,
    random_rows,
    run_op,
    spec_count_table,
    spec_mlm_mask,
    spec_of,
    spec_row_words,
    vector_inputs,
)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bert_pytorch_amd import ops
    from bert_pytorch_amd.config import BertConfig
    from bert_pytorch_amd.models import BertForPreTraining

DEV = "cuda:0"


@pytest.mark.parametrize("vec", VECTORS, ids=["vector1", "vector2"])
def test_spec_vectors(vec):
    ids, special = vector_inputs()
    words = spec_row_words(16, vec["seed"], vec["epoch"], vec["sample_index"])
    assert " ".join(f"{int(w):08x}" for w in words[1]) == vec["words"]
    kw = dict(seed=vec["seed"], epoch=vec["epoch"], masked_lm_prob=0.5,
              max_pred=8)
    want = spec_mlm_mask(ids, special, [vec["sample_index"]], **kw)
    assert want[0][0].tolist() == vec["ids"]
    assert np.nonzero(want[5][0] != -1)[0].tolist() == vec["label_pos"]
    assert_equal_spec(
        run_op(ids, special, [vec["sample_index"]], device=DEV, **kw), want)


def test_spec_row_counts():
    table = spec_count_table(16, 0.15, 20)
    for special, n in (((0, 9, 9), 1), ((0, 1, 2), 0), ((0, 1, 3), 1)):
        ids = np.full((1, 16), 2000, dtype=np.int32)
        want = spec_mlm_mask(ids, [special], [0], seed=1, epoch=0,
                             masked_lm_prob=0.15, max_pred=20)
        assert int((want[5] != -1).sum()) == n
    assert table[0] == 0 and table[1] == 1


# ---------------------------------------------------------------------------
# kernel == spec == fallback
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_spec(name):
    case, want = spec_of(name, False)
    assert_equal_spec(run_op(**case, device=DEV), want)
    if name == "S512_cap":
        counts = (want[5] != -1).sum(axis=1).tolist()
        assert counts[0] == 76 and counts[1] == 44, counts
    if name == "keep_plus_random_is_one":
        changed = want[0] != case["input_ids"]
        assert changed.any() and not (want[0][changed] == MASK).any()
    if name == "zero_prob_floor":
        assert (want[5] != -1).sum(axis=1).tolist() == [1, 1, 0, 1, 1, 1]


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_fallback(name):
    case, _ = spec_of(name, False)
    got = run_op(**case, device=DEV)
    fallback = run_op(**case, device="cpu")
    for n, g, f in zip(NAMES, got, fallback):
        assert not f.is_cuda
        assert torch.equal(g.cpu(), f), n


def test_dense_labels_on_request_only():
    case, want = spec_of("S48", False)
    S = case["input_ids"].shape[1]
    table = ops.mlm_count_table(S, case["masked_lm_prob"], case["max_pred"])
    t_keep, t_rand = ops.mlm_thresholds(0.1, 0.1)
    out = ops.mlm_mask(
        torch.from_numpy(case["input_ids"]).to(DEV),
        torch.from_numpy(case["special"]).to(DEV),
        torch.tensor(case["sample_index"], device=DEV),
        table.to(DEV), seed=case["seed"], epoch=case["epoch"],
        max_pred=case["max_pred"], vocab_size=VOCAB, mask_token=MASK,
        t_keep=t_keep, t_rand=t_rand,
    )
    assert out[5] is None
    for g, w in zip(out[:5], want[:5]):
        assert torch.equal(g.cpu(), torch.from_numpy(w))


def test_entry_point_checks():
    ext = ops.extension()
    ids = torch.zeros(2, 16, dtype=torch.int32, device=DEV)
    special = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    index = torch.zeros(2, dtype=torch.int64, device=DEV)
    table = torch.zeros(17, dtype=torch.int32, device=DEV)
    tail = (1, 0, 4, VOCAB, MASK, 1, 1, False)
    ext.mlm_mask(ids, special, index, table, *tail)
    with pytest.raises(RuntimeError, match="input_ids"):
        ext.mlm_mask(ids.long(), special, index, table, *tail)
    with pytest.raises(RuntimeError, match="special"):
        ext.mlm_mask(ids, special[:, :2].contiguous(), index, table, *tail)
    with pytest.raises(RuntimeError, match="sample_index"):
        ext.mlm_mask(ids, special, index.int(), table, *tail)
    with pytest.raises(RuntimeError, match="count_table"):
        ext.mlm_mask(ids, special, index, table[:16], *tail)
    with pytest.raises(RuntimeError, match="contiguous"):
        wide = torch.zeros(2, 32, dtype=torch.int32, device=DEV)
        ext.mlm_mask(wide[:, ::2], special, index, table, *tail)
    with pytest.raises(RuntimeError, match="max_pred"):
        ext.mlm_mask(ids, special, index, table, 1, 0, 17, VOCAB, MASK, 1, 1,
                     False)
    with pytest.raises(RuntimeError, match="1024"):
        ext.mlm_mask(
            torch.zeros(1, 1025, dtype=torch.int32, device=DEV), special[:1],
            index[:1], torch.zeros(1026, dtype=torch.int32, device=DEV),
            *tail)


def test_no_host_sync():
    """The op reads nothing back: it runs with sync debugging set to raise."""
    case, want = spec_of("B96_prefix", False)
    S = case["input_ids"].shape[1]
    ids = torch.from_numpy(case["input_ids"]).to(DEV)
    special = torch.from_numpy(case["special"]).to(DEV)
    index = torch.from_numpy(np.asarray(case["sample_index"])).to(DEV)
    table = ops.mlm_count_table(S, 0.15, 20).to(DEV)
    t_keep, t_rand = ops.mlm_thresholds(0.1, 0.1)
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:  # noqa: BLE001
        pytest.fail(f"sync debug mode is not available on this build: {e}")
    try:
        out = ops.mlm_mask(
            ids, special, index, table, seed=case["seed"],
            epoch=case["epoch"], max_pred=20, vocab_size=VOCAB,
            mask_token=MASK, t_keep=t_keep, t_rand=t_rand, dense_labels=True,
        )
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert_equal_spec(out, want)


# ---------------------------------------------------------------------------
# model level: positions from the kernel == the padded gather of its labels
# ---------------------------------------------------------------------------
def test_model_positions_path_equals_dense_labels_path():
    torch.manual_seed(0)
    config = BertConfig(
        vocab_size_or_config_json_file=1024, hidden_size=128,
        num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
        max_position_embeddings=64,
    )
    model = BertForPreTraining(config).to(DEV).eval()
    B, S, max_pred = 6, 64, 10
    ids, special = random_rows(B, S, seed=12)
    ids = (ids % 900) + 110
    masked, tt, am, positions, gathered, dense = run_op(
        ids, special, np.arange(B), seed=42, epoch=0, masked_lm_prob=0.15,
        max_pred=max_pred, vocab_size=1024, device=DEV,
    )
    assert int((gathered != -1).sum()) > B

    def run(**kw):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss, _rel, labels = model(masked, tt, am, compute_mlm_loss=True,
                                       **kw)
        loss.backward()
        grads = {n: p.grad.clone() for n, p in model.named_parameters()
                 if p.grad is not None}
        return loss.detach().clone(), labels, grads

    loss_a, labels_a, grads_a = run(masked_lm_labels=gathered,
                                    masked_lm_positions=positions)
    loss_b, labels_b, grads_b = run(masked_lm_labels=dense,
                                    max_predictions_per_seq=max_pred)
    assert torch.equal(labels_a, labels_b)
    assert torch.equal(loss_a, loss_b), (float(loss_a), float(loss_b))
    assert grads_a.keys() == grads_b.keys() and grads_a
    for n in grads_a:
        assert torch.equal(grads_a[n], grads_b[n]), n
