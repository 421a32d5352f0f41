"""Whole-word masking on the device (the whole-word instantiation of the row
kernel and the scatter kernel of csrc/ops/mlm_mask.hip,
``ops.mlm_mask(..., word_continues=)``).

The expected values come from ``spec_mlm_mask_wwm``, the sequential
plain-Python specification in tests/mlm_mask_spec.py; the cases are that
file's too, each computed once per session. Integer
arithmetic end to end: every comparison is ``torch.equal``. All tests
@pytest.mark.gpu.
"""

import numpy as np
import pytest
import torch

from mlm_mask_spec import (
    MASK,
    NAMES,
    VOCAB,
    WWM_CASES as CASES,
    assert_equal_spec,
    check_case_facts,
    run_op,
    spec_mlm_mask_wwm,
    spec_of,
)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bert_pytorch_amd import ops

DEV = "cuda:0"


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "no_dense"])
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_spec(name, dense):
    case, want = spec_of(name, True)
    check_case_facts(name, case, want)
    got = run_op(**case, dense_labels=dense, device=DEV)
    assert all(t.is_cuda for t in got[:5])
    assert_equal_spec(got, want, dense_labels=dense)


@pytest.mark.parametrize("name", ["B8_S512", "B300_S16_prefix",
                                  "vocab_edge_ids"])
def test_kernel_equals_fallback(name):
    case, _ = spec_of(name, True)
    got = run_op(**case, device=DEV)
    fallback = run_op(**case, device="cpu")
    for n, g, f in zip(NAMES, got, fallback):
        assert torch.equal(g.cpu(), f), n


def test_two_epochs_give_different_masks():
    case, want = spec_of("B8_S128", True)
    other = dict(case, epoch=case["epoch"] + 1)
    got = run_op(**other, device=DEV)
    assert not torch.equal(got[5].cpu(), torch.from_numpy(want[5]))
    assert torch.equal(got[1].cpu(), torch.from_numpy(want[1]))
    assert_equal_spec(got, spec_mlm_mask_wwm(**other))


def test_a_sample_has_one_mask_in_any_batch():
    case, want = spec_of("B8_S128", True)
    index = np.asarray(case["sample_index"])
    for pick in ([5, 2], [0, 7, 7, 3, 5]):
        sub = dict(case, input_ids=case["input_ids"][pick],
                   special=case["special"][pick], sample_index=index[pick])
        got = run_op(**sub, device=DEV)
        for row, src in enumerate(pick):
            for k in (0, 1, 2, 5):
                assert torch.equal(got[k][row].cpu(),
                                   torch.from_numpy(want[k][src]))


@pytest.mark.parametrize("name", ["B8_S128", "B300_S16_prefix", "B3_S1024",
                                  "max_pred_below_table"])
def test_all_zero_table_equals_the_token_level_kernel(name):
    case, _ = spec_of(name, True)
    zeros = dict(case, word_continues=np.zeros(VOCAB, dtype=np.uint8))
    got = run_op(**zeros, device=DEV)
    plain = run_op(**dict(case, word_continues=None), device=DEV)
    for n, g, p in zip(NAMES, got, plain):
        assert torch.equal(g, p), n


def test_no_host_sync():
    """The op reads nothing back: it runs with sync debugging set to raise."""
    case, want = spec_of("B8_S128", True)
    S = case["input_ids"].shape[1]
    ids = torch.from_numpy(case["input_ids"]).to(DEV)
    special = torch.from_numpy(case["special"]).to(DEV)
    index = torch.from_numpy(np.asarray(case["sample_index"])).to(DEV)
    words = torch.from_numpy(case["word_continues"]).to(DEV)
    table = ops.mlm_count_table(S, case["masked_lm_prob"],
                                case["max_pred"]).to(DEV)
    t_keep, t_rand = ops.mlm_thresholds(0.1, 0.1)
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:  # noqa: BLE001
        pytest.fail(f"sync debug mode is not available on this build: {e}")
    try:
        out = ops.mlm_mask(
            ids, special, index, table, seed=case["seed"],
            epoch=case["epoch"], max_pred=case["max_pred"], vocab_size=VOCAB,
            mask_token=MASK, t_keep=t_keep, t_rand=t_rand, dense_labels=True,
            word_continues=words,
        )
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert_equal_spec(out, want)


def test_entry_point_checks():
    """Every bad argument is stopped on the host, before any launch."""
    ext = ops.extension()
    ids = torch.zeros(2, 16, dtype=torch.int32, device=DEV)
    special = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    index = torch.zeros(2, dtype=torch.int64, device=DEV)
    table = torch.zeros(17, dtype=torch.int32, device=DEV)
    words = torch.zeros(VOCAB, dtype=torch.uint8, device=DEV)
    tail = (1, 0, 4, VOCAB, MASK, 1, 1, False)
    out = ext.mlm_mask_whole_word(ids, special, index, table, words, *tail)
    assert len(out) == 5
    for bad in (
        words.int(),                                     # dtype
        words.cpu(),                                     # device
        words[:-1],                                      # length
        torch.zeros(VOCAB + 1, dtype=torch.uint8, device=DEV),
        torch.zeros(2 * VOCAB, dtype=torch.uint8, device=DEV)[::2],
        words.reshape(1, VOCAB),                         # rank
    ):
        with pytest.raises(RuntimeError, match="word_continues"):
            ext.mlm_mask_whole_word(ids, special, index, table, bad, *tail)
    # and the checks it shares with the token-level entry point
    with pytest.raises(RuntimeError, match="input_ids"):
        ext.mlm_mask_whole_word(ids.long(), special, index, table, words,
                                *tail)
    with pytest.raises(RuntimeError, match="special"):
        ext.mlm_mask_whole_word(ids, special[:, :2].contiguous(), index,
                                table, words, *tail)
    with pytest.raises(RuntimeError, match="sample_index"):
        ext.mlm_mask_whole_word(ids, special, index.int(), table, words,
                                *tail)
    with pytest.raises(RuntimeError, match="count_table"):
        ext.mlm_mask_whole_word(ids, special, index, table[:16], words, *tail)
    with pytest.raises(RuntimeError, match="max_pred"):
        ext.mlm_mask_whole_word(ids, special, index, table, words, 1, 0, 17,
                                VOCAB, MASK, 1, 1, False)
    with pytest.raises(RuntimeError, match="1024"):
        ext.mlm_mask_whole_word(
            torch.zeros(1, 1025, dtype=torch.int32, device=DEV), special[:1],
            index[:1], torch.zeros(1026, dtype=torch.int32, device=DEV),
            words, *tail)
