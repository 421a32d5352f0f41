"""Whole-word masking without a GPU: ``ops.mlm_mask(..., word_continues=)``
on the CPU (the torch twin of the whole-word kernels), the continuation
table, the CPU loader and the runner.

The expected values come from ``spec_mlm_mask_wwm``, the sequential
plain-Python specification in tests/mlm_mask_spec.py, which shares no code
with the package. Everything is integer arithmetic, so every comparison is
exact. tests/test_gpu_whole_word_masking.py runs the kernels against the
same cases.
"""

import json
import math

import numpy as np
import pytest
import torch

import run_pretraining
from bert_pytorch_amd.data import (
    DeviceMasker,
    ShardedPretrainingDataset,
    synth,
)
from bert_pytorch_amd.data.tokenization import word_continuation_table
from mlm_mask_spec import (
    MASK,
    NAMES,
    VOCAB,
    WWM_CASES as CASES,
    _argv,
    _losses,
    _raw,
    assert_equal_spec,
    check_case_facts,
    make_workspace,
    random_rows,
    random_table,
    run_op,
    spec_count_table,
    spec_mlm_mask,
    spec_mlm_mask_wwm,
    spec_of,
    spec_row_word_lists,
)


# ---------------------------------------------------------------------------
# CPU op == spec
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_cpu_op_equals_sequential_spec(name):
    case, want = spec_of(name, True)
    check_case_facts(name, case, want)
    assert_equal_spec(run_op(**case), want)


def test_dense_labels_on_request_only():
    case, want = spec_of("B3_S128", True)
    assert_equal_spec(run_op(**case, dense_labels=False), want,
                      dense_labels=False)


def test_word_boundaries_of_the_crafted_rows():
    case, _ = spec_of("sep_and_cls_break_words", True)
    table = case["word_continues"]
    words = spec_row_word_lists(case["input_ids"][0], [1, 2, 3, 5, 6, 7, 8, 9,
                                                       10, 11], table, VOCAB)
    assert words == [[1, 2, 3], [5, 6], [7], [8], [9], [10], [11]]
    words = spec_row_word_lists(case["input_ids"][1], [1, 2, 3, 4, 5, 7, 8, 9,
                                                       10, 11], table, VOCAB)
    assert words[:2] == [[1, 2], [3]]


def test_epochs_differ_and_batch_layout_does_not_matter():
    case, want = spec_of("B8_S128", True)
    other = dict(case, epoch=case["epoch"] + 1)
    e1 = run_op(**other)
    assert not torch.equal(e1[5], torch.from_numpy(want[5]))
    assert_equal_spec(e1, spec_mlm_mask_wwm(**other))
    # rows 5 and 2 in a batch of two
    pick = [5, 2]
    sub = dict(case, input_ids=case["input_ids"][pick],
               special=case["special"][pick],
               sample_index=np.asarray(case["sample_index"])[pick])
    got = run_op(**sub)
    for row, src in enumerate(pick):
        for k in (0, 1, 2, 5):
            assert torch.equal(got[k][row], torch.from_numpy(want[k][src]))


def test_bad_table_raises_on_cpu():
    case, _ = spec_of("B1_S16", True)
    for bad in (case["word_continues"][:-1],
                case["word_continues"].astype(np.int32)):
        with pytest.raises(ValueError, match="word_continues"):
            run_op(**dict(case, word_continues=bad))


# ---------------------------------------------------------------------------
# invariants on random batches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_invariants_on_random_batches(seed):
    B, S, max_pred, prob = 12, 64, 9, 0.15
    ids, special = random_rows(B, S, seed=50 + seed)
    special[0] = (0, 1, 2)  # no candidates
    table = random_table(60 + seed, frac=0.6)
    ids[1, 1:] = np.nonzero(table)[0][0]  # one long word per segment
    masked, _tt, _am, positions, gathered, labels = run_op(
        ids, special, np.arange(B) + 100 * seed, table, seed=seed, epoch=0,
        masked_lm_prob=prob, max_pred=max_pred,
    )
    count_table = spec_count_table(S, prob, max_pred)
    labels_np, masked_np = labels.numpy(), masked.numpy()
    partial_rows = 0
    for b in range(B):
        sp = [int(v) for v in special[b]]
        cand = [j for j in range(sp[2]) if j not in sp]
        n = int(count_table[len(cand)])
        words = spec_row_word_lists(ids[b], cand, table, VOCAB)
        selected = set(np.nonzero(labels_np[b] != -1)[0].tolist())
        assert selected <= set(cand)
        for word in words:  # all of a word or none of it
            assert len(selected & set(word)) in (0, len(word)), (b, word)
        m = len(selected)
        assert m <= n
        if m == 0:
            assert not cand or all(len(w) > n for w in words)
        if m < n:  # then no untouched word fits into what is left
            partial_rows += 1
            assert all(len(w) > n - m for w in words
                       if not selected & set(w))
        orig = ids[b].astype(np.int64)
        picked = sorted(selected)
        assert np.array_equal(labels_np[b, picked], orig[picked])
        rest = [j for j in range(S) if j not in selected]
        assert (labels_np[b, rest] == -1).all()
        assert np.array_equal(masked_np[b, rest], orig[rest])
    flat = labels.reshape(-1)
    real = torch.nonzero(flat != -1).squeeze(-1)
    assert torch.equal(positions[: real.numel()], real)  # ascending
    assert torch.equal(gathered[: real.numel()], flat[real])
    assert not positions[real.numel():].any()
    assert (gathered[real.numel():] == -1).all()
    assert positions.numel() == B * max_pred
    assert partial_rows >= 1  # row 1 at least: its words are too long


@pytest.mark.parametrize("name", ["B8_S128", "B300_S16_prefix", "B3_S1024",
                                  "max_pred_below_table"])
def test_all_zero_table_is_token_level_masking(name):
    case, _ = spec_of(name, True)
    zeros = dict(case, word_continues=np.zeros(VOCAB, dtype=np.uint8))
    got = run_op(**zeros)
    plain = run_op(**dict(case, word_continues=None))
    for n, g, p in zip(NAMES, got, plain):
        assert torch.equal(g, p), n
    if "table_max_pred" not in case:  # and both are the numpy token spec
        kw = {k: v for k, v in case.items() if k != "word_continues"}
        for g, w in zip(got, spec_mlm_mask(**kw)):
            assert torch.equal(g, torch.from_numpy(w))


# ---------------------------------------------------------------------------
# the continuation table
# ---------------------------------------------------------------------------
def test_wordpiece_continuation_table(tmp_path):
    tokens = ["[PAD]", "[unused0]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "the",
              "##s", "play", "##ing", "##", "#", "[", "a##b", "##[x]"]
    path = tmp_path / "vocab.txt"
    path.write_text("\n".join(tokens) + "\n", encoding="utf-8")
    table = word_continuation_table(str(path), 64)
    assert table.dtype == torch.uint8 and table.shape == (64,)
    want = [int(t.startswith("##")) for t in tokens]
    assert want == [0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 1]
    assert table[: len(tokens)].tolist() == want
    assert not table[len(tokens):].any()  # the padding entries
    assert word_continuation_table(str(path), len(tokens)).tolist() == want
    with pytest.raises(ValueError, match="vocab_size"):
        word_continuation_table(str(path), len(tokens) - 1)


@pytest.mark.parametrize("as_json", [True, False], ids=["json", "lines"])
def test_byte_bpe_continuation_table(tmp_path, as_json):
    tokens = ["<s>", "<pad>", "</s>", "<unk>", "<mask>", "Ġthe", "Ġ", "s",
              "ing", "Ġplay", ".", "<", "Ċ"]
    if as_json:
        path = tmp_path / "vocab.json"
        path.write_text(json.dumps({t: i for i, t in enumerate(tokens)}),
                        encoding="utf-8")
    else:
        path = tmp_path / "vocab.txt"
        path.write_text("\n".join(tokens) + "\n", encoding="utf-8")
    table = word_continuation_table(str(path), 16)
    assert table.tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 1, 1, 1, 0, 0, 0]


# ---------------------------------------------------------------------------
# DeviceMasker
# ---------------------------------------------------------------------------
def test_device_masker_passes_the_table_on():
    case, want = spec_of("B3_S128", True)
    kw = dict(seed=case["seed"], mask_token_index=MASK,
              max_pred_per_seq=case["max_pred"],
              masked_lm_prob=case["masked_lm_prob"], vocab_size=VOCAB)
    masker = DeviceMasker(word_continues=torch.from_numpy(case["word_continues"]),
                          **kw)
    batch = [torch.from_numpy(case["input_ids"]),
             torch.from_numpy(case["special"]), torch.zeros(3, dtype=torch.long),
             torch.from_numpy(np.asarray(case["sample_index"]))]
    out = masker(batch, case["epoch"])
    for g, w in zip(out[:5], want[:5]):
        assert torch.equal(g, torch.from_numpy(w))
    assert masker.word_table(torch.device("cpu")) is masker.word_table(
        torch.device("cpu"))
    assert DeviceMasker(**kw).word_table(torch.device("cpu")) is None
    with pytest.raises(ValueError, match="word_continues"):
        DeviceMasker(word_continues=torch.zeros(5, dtype=torch.uint8), **kw)


# ---------------------------------------------------------------------------
# CPU loader
# ---------------------------------------------------------------------------
SEQ, MAX_PRED, PROB = 48, 8, 0.15


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    directory = tmp_path_factory.mktemp("wwm_shards")
    return synth.make_dataset(
        str(directory), num_shards=2, samples_per_shard=16, seq_len=SEQ,
        vocab_size=VOCAB, seed=3,
    )


def _dataset(files, **kw):
    return ShardedPretrainingDataset(
        files, mask_token_index=MASK, max_pred_per_seq=MAX_PRED,
        masked_lm_prob=PROB, vocab_size=VOCAB, seed=42, **kw,
    )


def test_loader_masks_whole_words(shards):
    raw_ids, raw_special = _raw(shards)
    table = random_table(77, frac=0.6)
    dataset = _dataset(shards, whole_word_masking=True, word_continues=table)
    multi = 0
    for idx in range(len(dataset)):
        masked, _seg, _am, labels, _nsp = dataset[idx]
        sp = [int(v) for v in raw_special[idx]]
        cand = [j for j in range(sp[-1]) if j not in sp]
        n = min(MAX_PRED, max(1, int(len(cand) * PROB)))
        words = spec_row_word_lists(raw_ids[idx], cand, table, VOCAB)
        selected = set(np.nonzero(labels != -1)[0].tolist())
        assert selected <= set(cand)
        for word in words:
            hit = len(selected & set(word))
            assert hit in (0, len(word)), (idx, word)
            multi += hit > 1
        assert len(selected) <= n
        if len(selected) < n:
            assert all(len(w) > n - len(selected) for w in words
                       if not selected & set(w))
        picked = sorted(selected)
        assert np.array_equal(labels[picked], raw_ids[idx][picked])
        rest = [j for j in range(SEQ) if j not in selected]
        assert np.array_equal(masked[rest], raw_ids[idx][rest])
    assert multi > 0  # some word of several pieces was masked


def test_loader_is_unchanged_without_the_flag(shards):
    """Seed for seed today's masks: a copy of the token-level selection of
    the parent commit, run on the same generator."""
    raw_ids, raw_special = _raw(shards)
    dataset = _dataset(shards)
    assert dataset.whole_word_masking is False
    rng = np.random.default_rng(42)
    for idx in range(len(dataset)):
        masked, _seg, _am, labels, _nsp = dataset[idx]
        sp = set(int(v) for v in raw_special[idx])
        cand = np.array([j for j in range(int(raw_special[idx][-1]))
                         if j not in sp], dtype=np.int64)
        count = min(MAX_PRED, max(1, int(cand.size * PROB)))
        picks = rng.choice(cand, count, replace=False)
        want_ids = raw_ids[idx].astype(np.int64).copy()
        for j, draw in zip(picks, rng.random(count)):
            if draw < 0.1:
                continue
            if draw < 0.2:
                want_ids[j] = rng.integers(0, VOCAB - 1)
            else:
                want_ids[j] = MASK
        assert sorted(np.nonzero(labels != -1)[0].tolist()) == sorted(picks)
        assert np.array_equal(masked, want_ids)


def test_loader_flag_needs_the_table_and_leaves_static_masks_alone(shards):
    with pytest.raises(ValueError, match="word_continues"):
        _dataset(shards, whole_word_masking=True)
    with pytest.raises(ValueError, match="word_continues"):
        _dataset(shards, whole_word_masking=True,
                 word_continues=np.zeros(7, dtype=np.uint8))
    table = np.ones(VOCAB, dtype=np.uint8)  # every segment one long word
    static = _dataset(shards, static_masking=True)
    static_wwm = _dataset(shards, static_masking=True, whole_word_masking=True,
                          word_continues=table)
    for idx in (0, 1, 2):
        for a, b in zip(static[idx], static_wwm[idx]):
            assert np.array_equal(a, b)


# ---------------------------------------------------------------------------
# runner
# ---------------------------------------------------------------------------
@pytest.fixture
def workspace(tmp_path):
    return make_workspace(tmp_path, with_vocab=True)


def test_flag_parses_from_cli_and_json_and_needs_a_vocab_file(workspace):
    tmp_path, data_dir, cfg_path, vocab_path = workspace
    argv = _argv(tmp_path, data_dir, cfg_path)
    assert run_pretraining.parse_arguments(argv).whole_word_masking is False
    args = run_pretraining.parse_arguments(
        argv + ["--whole_word_masking", "--vocab_file", vocab_path])
    assert args.whole_word_masking is True
    train_cfg = tmp_path / "train.json"
    train_cfg.write_text(json.dumps(
        {"whole_word_masking": True, "vocab_file": vocab_path}))
    args = run_pretraining.parse_arguments(
        argv + ["--config_file", str(train_cfg)])
    assert args.whole_word_masking is True and args.vocab_file == vocab_path
    with pytest.raises(ValueError, match="--vocab_file"):
        run_pretraining.parse_arguments(argv + ["--whole_word_masking"])
    args = run_pretraining.parse_arguments(
        argv + ["--whole_word_masking", "--vocab_file",
                str(tmp_path / "missing.txt")])
    with pytest.raises(ValueError, match="does not exist"):
        run_pretraining.prepare_masker(args)


@pytest.mark.parametrize(
    "extra", [("--device_masking",), ("--device_masking", "--unpad"), ()],
    ids=["device_masking", "device_masking_unpad", "cpu_loader"])
def test_runner_with_whole_word_masking(workspace, extra):
    tmp_path, data_dir, cfg_path, vocab_path = workspace
    args = run_pretraining.parse_arguments(
        _argv(tmp_path, data_dir, cfg_path, "--whole_word_masking",
              "--vocab_file", vocab_path, *extra))
    if extra:
        masker = run_pretraining.prepare_masker(args)
        assert masker.word_continues.shape == (512,)
        assert masker.word_continues.sum() == len(range(6, 512, 3))
    assert run_pretraining.main(args) == 2
    losses = _losses(tmp_path)
    assert len(losses) == 2
    assert all(math.isfinite(v) and v > 0 for v in losses), losses
