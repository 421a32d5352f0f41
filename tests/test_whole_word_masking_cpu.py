"""Whole-word masking without a GPU: ``ops.mlm_mask(..., word_continues=)``
on the CPU (the torch twin of the whole-word kernels), the continuation
table, the CPU loader and the runner.

``spec_mlm_mask_wwm`` is a sequential plain-Python implementation written
from the definition in docs/KERNELS.md and tests/philox_ref.py alone; it
shares no code with the package. Everything is integer arithmetic, so
every comparison is exact. tests/test_gpu_whole_word_masking.py runs the
kernels against the same cases.
"""

import csv
import json
import math

import numpy as np
import pytest
import torch

import run_pretraining
from bert_pytorch_amd import ops
from bert_pytorch_amd.data import (
    DeviceMasker,
    ShardedPretrainingDataset,
    h5lite,
    synth,
)
from bert_pytorch_amd.data.tokenization import word_continuation_table
from test_gpu_mlm_mask import (
    spec_count_table,
    spec_mlm_mask,
    spec_row_words,
    spec_thresholds,
)

VOCAB = 30522
MASK = 103
NAMES = ("masked_ids", "token_type_ids", "attention_mask", "positions",
         "gathered_labels", "dense_labels")


# ---------------------------------------------------------------------------
# sequential specification
# ---------------------------------------------------------------------------
def spec_row_word_lists(ids_row, cand, word_continues, vocab_size):
    """The words of one row: lists of positions, in position order."""
    cand_set = set(cand)
    words = []
    for j in cand:
        token = int(ids_row[j])
        continues = False
        if 0 <= token < vocab_size:  # never index the table outside it
            continues = int(word_continues[token]) == 1
        if continues and (j - 1) in cand_set:
            words[-1].append(j)
        else:
            words.append([j])
    return words


def spec_mlm_mask_wwm(input_ids, special, sample_index, word_continues, *,
                      seed, epoch, masked_lm_prob, max_pred, vocab_size=VOCAB,
                      mask_token=MASK, original_token_prob=0.1,
                      random_token_prob=0.1, table_max_pred=None):
    """(masked_ids, token_type, attention_mask, positions, gathered_labels,
    dense_labels) as int64 numpy arrays. ``table_max_pred`` builds the count
    table for another cap than ``max_pred``, which then binds on its own."""
    input_ids = np.asarray(input_ids)
    special = np.asarray(special)
    B, S = input_ids.shape
    if special.shape[1] == 2:
        special = np.concatenate([special, special[:, -1:]], axis=1)
    table = spec_count_table(S, masked_lm_prob, table_max_pred or max_pred)
    t_keep, t_rand = spec_thresholds(original_token_prob, random_token_prob)
    ids = input_ids.astype(np.int64).copy()
    tt = np.zeros((B, S), dtype=np.int64)
    am = np.zeros((B, S), dtype=np.int64)
    labels = np.full((B, S), -1, dtype=np.int64)
    for b in range(B):
        sp = [int(v) for v in special[b]]
        last = min(max(sp[2], 0), S - 1)
        for j in range(S):
            am[b, j] = int(j <= last)
            tt[b, j] = int(sp[1] < j <= sp[2])
        inside = {v for v in sp if 0 <= v < S}
        cand = [j for j in range(last) if j not in inside]
        n = min(int(table[len(cand)]), max_pred)
        draws = spec_row_words(S, seed, epoch, sample_index[b])
        words = spec_row_word_lists(input_ids[b], cand, word_continues,
                                    vocab_size)
        words.sort(key=lambda w: (int(draws[w[0], 0]) << 32) | w[0])
        m = 0
        for word in words:
            if m >= n:
                break
            if m + len(word) > n:
                continue
            m += len(word)
            for j in word:
                w1, w2 = int(draws[j, 1]), int(draws[j, 2])
                labels[b, j] = ids[b, j]
                if w1 < t_keep:
                    pass
                elif w1 < t_keep + t_rand:
                    ids[b, j] = (w2 * (vocab_size - 1)) >> 32
                else:
                    ids[b, j] = mask_token
    cap = B * max_pred
    positions = np.zeros(cap, dtype=np.int64)
    gathered = np.full(cap, -1, dtype=np.int64)
    flat = labels.reshape(-1)
    where = np.nonzero(flat != -1)[0]
    positions[: where.size] = where
    gathered[: where.size] = flat[where]
    return ids, tt, am, positions, gathered, labels


# ---------------------------------------------------------------------------
# cases (shared with the GPU test)
# ---------------------------------------------------------------------------
def random_table(seed, vocab_size=VOCAB, frac=0.45):
    rng = np.random.default_rng(seed)
    return (rng.random(vocab_size) < frac).astype(np.uint8)


def random_rows(B, S, seed, vocab_size=VOCAB):
    """Shard-like rows: [CLS] a [SEP] b [SEP] pad, lengths in [S/2, S]."""
    rng = np.random.default_rng(seed)
    ids = np.zeros((B, S), dtype=np.int32)
    special = np.zeros((B, 3), dtype=np.int32)
    for b in range(B):
        total = int(rng.integers(max(5, S // 2), S + 1))
        ids[b, :total] = rng.integers(min(1000, vocab_size // 2), vocab_size,
                                      size=total)
        split = int(rng.integers(1, total - 2))
        special[b] = (0, split, total - 1)
    return ids, special


def _grid_case(B, S):
    def make():
        ids, special = random_rows(B, S, seed=100 * S + B)
        return dict(input_ids=ids, special=special,
                    sample_index=np.arange(B) + 7 * S,
                    word_continues=random_table(S + B), seed=42, epoch=1,
                    masked_lm_prob=0.15, max_pred=max(1, int(S * 0.15)))
    return make


def _case_many_rows():
    ids, special = random_rows(300, 16, seed=11)
    return dict(input_ids=ids, special=special,
                sample_index=np.arange(300) + 5000,
                word_continues=random_table(11), seed=9, epoch=0,
                masked_lm_prob=0.3, max_pred=4)


CONT, HEAD = 2000, 2001  # a continuation id and a word-start id below


def _crafted_table():
    table = np.zeros(VOCAB, dtype=np.uint8)
    table[CONT] = 1
    table[VOCAB - 1] = 1
    return table


def _case_all_continuations():
    """Rows 0 and 1 hold continuation pieces only: every segment is one
    word. Row 0's two words (14 and 15 long) exceed n = 4: nothing is
    selected. Row 1's first segment is 2 long and fits."""
    ids = np.full((3, 32), CONT, dtype=np.int32)
    special = np.array([(0, 15, 31), (0, 3, 31), (0, 15, 31)], dtype=np.int32)
    ids[2] = HEAD  # all starts: token-level behaviour
    return dict(input_ids=ids, special=special, sample_index=[1, 2, 3],
                word_continues=_crafted_table(), seed=5, epoch=0,
                masked_lm_prob=0.15, max_pred=8)


def _case_no_candidates():
    ids, special = random_rows(4, 16, seed=12)
    special[0] = (0, 1, 2)
    special[2] = (0, 0, 0)
    special[3] = (-3, -1, -7)
    return dict(input_ids=ids, special=special, sample_index=[0, 1, 2, 3],
                word_continues=random_table(12), seed=5, epoch=0,
                masked_lm_prob=0.15, max_pred=3)


def _case_sep_and_cls_break_words():
    """Row 0: H C C [SEP] C C H ... - the continuation after [SEP] starts a
    word. Row 1: a continuation at position 1, right after [CLS]."""
    ids = np.full((2, 16), HEAD, dtype=np.int32)
    special = np.array([(0, 4, 12), (0, 6, 12)], dtype=np.int32)
    ids[0, [2, 3, 5, 6]] = CONT
    ids[1, [1, 2]] = CONT
    return dict(input_ids=ids, special=special, sample_index=[21, 22],
                word_continues=_crafted_table(), seed=3, epoch=0,
                masked_lm_prob=0.5, max_pred=8)


def _case_cap_binds():
    """max_pred below the table's counts: the table is built for a cap of
    20, the call passes 5."""
    ids, special = random_rows(6, 128, seed=13)
    return dict(input_ids=ids, special=special, sample_index=np.arange(6),
                word_continues=random_table(13), seed=42, epoch=0,
                masked_lm_prob=0.15, max_pred=5, table_max_pred=20)


def _case_max_pred_one():
    ids, special = random_rows(8, 48, seed=14)
    return dict(input_ids=ids, special=special, sample_index=np.arange(8),
                word_continues=random_table(14, frac=0.3), seed=42, epoch=0,
                masked_lm_prob=0.15, max_pred=1)


def _case_vocab_edge_ids():
    """Ids at vocab_size - 1 (a continuation in the crafted table) and ids
    outside the vocabulary, which start words and never index the table."""
    ids = np.full((3, 24), VOCAB - 1, dtype=np.int32)
    special = np.array([(0, 10, 23), (0, 12, 20), (0, 5, 23)], dtype=np.int32)
    ids[0, ::3] = HEAD
    ids[1, ::2] = VOCAB
    ids[1, 5] = -1
    ids[1, 7] = 2 ** 31 - 1
    ids[2, ::4] = HEAD
    return dict(input_ids=ids, special=special, sample_index=[4, 5, 6],
                word_continues=_crafted_table(), seed=8, epoch=2,
                masked_lm_prob=0.3, max_pred=6)


def _case_wide_integers():
    ids, special = random_rows(5, 64, seed=15)
    return dict(input_ids=ids, special=special,
                sample_index=(2 ** 33 + 17) + np.arange(5) * (2 ** 32 + 1),
                word_continues=random_table(15),
                seed=2 ** 63 + 2 ** 40 + 9, epoch=5, masked_lm_prob=0.15,
                max_pred=9)


CASES = {f"B{B}_S{S}": _grid_case(B, S)
         for S in (16, 128, 512, 1024) for B in (1, 3, 8)}
CASES.update({
    "B300_S16_prefix": _case_many_rows,
    "all_continuations": _case_all_continuations,
    "no_candidates": _case_no_candidates,
    "sep_and_cls_break_words": _case_sep_and_cls_break_words,
    "max_pred_below_table": _case_cap_binds,
    "max_pred_one": _case_max_pred_one,
    "vocab_edge_ids": _case_vocab_edge_ids,
    "sample_index_above_2_32": _case_wide_integers,
})

_SPEC_CACHE = {}


def spec_of(name):
    """The case and its expected outputs, computed once per session."""
    if name not in _SPEC_CACHE:
        case = CASES[name]()
        _SPEC_CACHE[name] = (case, spec_mlm_mask_wwm(**case))
    return _SPEC_CACHE[name]


def run_op(input_ids, special, sample_index, word_continues, *, seed, epoch,
           masked_lm_prob, max_pred, vocab_size=VOCAB, mask_token=MASK,
           table_max_pred=None, dense_labels=True, device="cpu"):
    S = np.asarray(input_ids).shape[1]
    table = ops.mlm_count_table(S, masked_lm_prob, table_max_pred or max_pred)
    t_keep, t_rand = ops.mlm_thresholds(0.1, 0.1)
    words = None
    if word_continues is not None:
        words = torch.as_tensor(np.asarray(word_continues)).to(device)
    return ops.mlm_mask(
        torch.as_tensor(np.asarray(input_ids, dtype=np.int32)).to(device),
        torch.as_tensor(np.asarray(special, dtype=np.int32)).to(device),
        torch.as_tensor(np.asarray(sample_index, dtype=np.int64)).to(device),
        table.to(device), seed=seed, epoch=epoch, max_pred=max_pred,
        vocab_size=vocab_size, mask_token=mask_token, t_keep=t_keep,
        t_rand=t_rand, dense_labels=dense_labels, word_continues=words,
    )


def assert_equal_spec(got, want, dense_labels=True):
    assert len(got) == len(want) == 6
    for name, g, w in zip(NAMES, got, want):
        if name == "dense_labels" and not dense_labels:
            assert g is None
            continue
        w = torch.from_numpy(w)
        assert g.dtype == torch.int64, (name, g.dtype)
        assert g.shape == w.shape, (name, g.shape, w.shape)
        assert torch.equal(g.cpu(), w), name


def check_case_facts(name, case, want):
    """What a crafted case is there to show, read off the expected values."""
    counts = (want[5] != -1).sum(axis=1).tolist()
    if name == "all_continuations":
        assert counts == [0, 2, 4], counts
        assert np.nonzero(want[5][1] != -1)[0].tolist() == [1, 2]
    if name == "no_candidates":
        assert counts[0] == counts[2] == counts[3] == 0 and counts[1] > 0
    if name == "sep_and_cls_break_words":
        lab0, lab1 = want[5][0] != -1, want[5][1] != -1
        # words of row 0: [1,2,3] [5,6] [7] .. [11]; of row 1: [1,2] [3] ..
        assert lab0[1] == lab0[2] == lab0[3] and lab0[5] == lab0[6]
        assert lab1[1] == lab1[2]
    if name == "max_pred_below_table":
        assert max(counts) == 5 and min(counts) >= 3, counts
    if name == "max_pred_one":
        assert set(counts) <= {0, 1} and sum(counts) >= 4, counts
    if name == "B300_S16_prefix":
        assert sum(counts) > 300


# ---------------------------------------------------------------------------
# CPU op == spec
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_cpu_op_equals_sequential_spec(name):
    case, want = spec_of(name)
    check_case_facts(name, case, want)
    assert_equal_spec(run_op(**case), want)


def test_dense_labels_on_request_only():
    case, want = spec_of("B3_S128")
    assert_equal_spec(run_op(**case, dense_labels=False), want,
                      dense_labels=False)


def test_word_boundaries_of_the_crafted_rows():
    case, _ = spec_of("sep_and_cls_break_words")
    table = case["word_continues"]
    words = spec_row_word_lists(case["input_ids"][0], [1, 2, 3, 5, 6, 7, 8, 9,
                                                       10, 11], table, VOCAB)
    assert words == [[1, 2, 3], [5, 6], [7], [8], [9], [10], [11]]
    words = spec_row_word_lists(case["input_ids"][1], [1, 2, 3, 4, 5, 7, 8, 9,
                                                       10, 11], table, VOCAB)
    assert words[:2] == [[1, 2], [3]]


def test_epochs_differ_and_batch_layout_does_not_matter():
    case, want = spec_of("B8_S128")
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
    case, _ = spec_of("B1_S16")
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
    case, _ = spec_of(name)
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
    case, want = spec_of("B3_S128")
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


def _raw(files):
    ids, special = [], []
    for path in files:
        with h5lite.H5LiteFile(path) as f:
            ids.append(np.asarray(f["input_ids"]))
            special.append(np.asarray(f["special_token_positions"]))
    return np.concatenate(ids), np.concatenate(special)


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
    data_dir = tmp_path / "data"
    synth.make_dataset(
        str(data_dir), num_shards=2, samples_per_shard=16, seq_len=32,
        vocab_size=512, seed=0,
    )
    model_cfg = {
        "vocab_size": 512, "hidden_size": 64, "num_hidden_layers": 2,
        "num_attention_heads": 4, "intermediate_size": 128,
        "max_position_embeddings": 64, "type_vocab_size": 2,
        "hidden_act": "gelu", "hidden_dropout_prob": 0.1,
        "attention_probs_dropout_prob": 0.1, "initializer_range": 0.02,
        "next_sentence": True,
    }
    cfg_path = tmp_path / "model.json"
    cfg_path.write_text(json.dumps(model_cfg))
    tokens = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    tokens += [f"w{i}" if i % 3 else f"##p{i}" for i in range(5, 512)]
    vocab_path = tmp_path / "vocab.txt"
    vocab_path.write_text("\n".join(tokens) + "\n", encoding="utf-8")
    return tmp_path, str(data_dir), str(cfg_path), str(vocab_path)


def _argv(tmp_path, data_dir, cfg_path, *extra):
    return [
        "--model_config_file", cfg_path, "--input_dir", data_dir,
        "--output_dir", str(tmp_path / "out"), "--local_batch_size", "4",
        "--global_batch_size", "8", "--max_steps", "2",
        "--learning_rate", "1e-3", "--warmup_proportion", "0.2",
        "--num_steps_per_checkpoint", "2", "--seed", "7",
        "--num_workers", "0", "--max_predictions_per_seq", "5", *extra,
    ]


def _losses(tmp_path):
    (path,) = (tmp_path / "out").glob("*_metrics.csv")
    with open(path, newline="", encoding="utf-8") as f:
        return [float(r["step_loss"]) for r in csv.DictReader(f)
                if r["tag"] == "train"]


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
