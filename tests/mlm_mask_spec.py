"""Independent specifications of the MLM mask function, the shared cases and
the helpers of the four masking test modules (a plain helper module like
philox_ref.py; no fixtures, no tests).

``spec_mlm_mask`` (numpy) and ``spec_mlm_mask_wwm`` (sequential plain
Python) are written from the definition in docs/KERNELS.md and
tests/philox_ref.py alone; they share no code with the package. Everything
is integer arithmetic, so every comparison is exact.
"""

import csv
import json

import numpy as np
import torch

import philox_ref
from bert_pytorch_amd import ops
from bert_pytorch_amd.data import h5lite, synth

VOCAB = 30522
MASK = 103
NAMES = ("masked_ids", "token_type_ids", "attention_mask", "positions",
         "gathered_labels", "dense_labels")


# ---------------------------------------------------------------------------
# numpy specification, token level
# ---------------------------------------------------------------------------
def spec_count_table(S, masked_lm_prob, max_pred):
    return np.array(
        [0 if c == 0 else min(max_pred, max(1, int(c * masked_lm_prob)))
         for c in range(S + 1)],
        dtype=np.int32,
    )


def spec_thresholds(original_token_prob, random_token_prob):
    return (int(original_token_prob * (1 << 32)),
            int(random_token_prob * (1 << 32)))


def spec_row_words(S, seed, epoch, sample_index):
    """Philox words [S, 4] of every position of one row."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    idx = int(sample_index)
    c3 = ((idx >> 32) & 0x7FFFFFFF) | 0x80000000
    return philox_ref.philox4x32_10_words(
        np.arange(S), int(epoch) & 0xFFFFFFFF, idx & 0xFFFFFFFF, c3,
        seed & 0xFFFFFFFF, seed >> 32,
    )


def spec_mlm_mask(input_ids, special, sample_index, *, seed, epoch,
                  masked_lm_prob, max_pred, vocab_size=VOCAB, mask_token=MASK,
                  original_token_prob=0.1, random_token_prob=0.1):
    """(masked_ids, token_type, attention_mask, positions, gathered_labels,
    dense_labels) as int64 numpy arrays."""
    input_ids = np.asarray(input_ids)
    special = np.asarray(special)
    B, S = input_ids.shape
    if special.shape[1] == 2:
        special = np.concatenate([special, special[:, -1:]], axis=1)
    table = spec_count_table(S, masked_lm_prob, max_pred)
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
        n = int(table[len(cand)])
        words = spec_row_words(S, seed, epoch, sample_index[b])
        order = sorted(cand, key=lambda j: (int(words[j, 0]) << 32) | j)
        for j in order[:n]:
            w1, w2 = int(words[j, 1]), int(words[j, 2])
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
# the specification's own cross-check vectors (no package code involved in
# the expected values)
# ---------------------------------------------------------------------------
def vector_inputs():
    ids = np.zeros((1, 16), dtype=np.int32)
    ids[0, :14] = 1000 + np.arange(14)
    return ids, np.array([[0, 7, 13]], dtype=np.int32)


VECTORS = [
    dict(seed=42, epoch=0, sample_index=5,
         words="059e6417 3435e4c7 5c702e16 7c9842ba",
         ids=[1000, 103, 103, 1003, 20422, 1005, 1006, 1007, 103, 1009, 1010,
              1011, 1012, 1013, 0, 0],
         label_pos=[1, 2, 4, 8, 11]),
    dict(seed=2 ** 40 + 7, epoch=3, sample_index=2 ** 33 + 5,
         words="5a3de554 1d7d1a78 01615034 268cf770",
         ids=[1000, 1001, 103, 103, 1004, 1005, 1006, 1007, 27743, 103, 1010,
              1011, 103, 1013, 0, 0],
         label_pos=[2, 3, 8, 9, 12]),
]


# ---------------------------------------------------------------------------
# sequential specification, whole words
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
# running the op and comparing it
# ---------------------------------------------------------------------------
def run_op(input_ids, special, sample_index, word_continues=None, *, seed,
           epoch, masked_lm_prob, max_pred, vocab_size=VOCAB, mask_token=MASK,
           original_token_prob=0.1, random_token_prob=0.1,
           table_max_pred=None, dense_labels=True, device="cpu"):
    S = np.asarray(input_ids).shape[1]
    table = ops.mlm_count_table(S, masked_lm_prob, table_max_pred or max_pred)
    t_keep, t_rand = ops.mlm_thresholds(original_token_prob, random_token_prob)
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


def random_rows(B, S, seed, n_special=3, vocab_size=VOCAB):
    """Shard-like rows: [CLS] a [SEP] b [SEP] pad, lengths in [S/2, S]."""
    rng = np.random.default_rng(seed)
    ids = np.zeros((B, S), dtype=np.int32)
    special = np.zeros((B, n_special), dtype=np.int32)
    for b in range(B):
        total = int(rng.integers(max(5, S // 2), S + 1))
        ids[b, :total] = rng.integers(min(1000, vocab_size // 2), vocab_size,
                                      size=total)
        split = int(rng.integers(1, total - 2))
        special[b] = (0, split, total - 1) if n_special == 3 else (0, total - 1)
    return ids, special


# ---------------------------------------------------------------------------
# token-level cases
# ---------------------------------------------------------------------------
def _token_edge_rows():
    ids, special = random_rows(5, 16, seed=1)
    special[:4] = [(0, 1, 2), (0, 1, 3), (0, 9, 9), (0, 7, 15)]
    ids[3] = 1000 + np.arange(16)
    return dict(input_ids=ids, special=special,
                sample_index=[3, 1, 4, 1, 5], seed=7, epoch=0,
                masked_lm_prob=0.15, max_pred=4)


def _token_s48():
    ids, special = random_rows(3, 48, seed=2)
    return dict(input_ids=ids, special=special, sample_index=[10, 11, 12],
                seed=42, epoch=1, masked_lm_prob=0.15, max_pred=8)


def _token_s512():
    ids, special = random_rows(4, 512, seed=3)
    special[0] = (0, 200, 511)   # 509 candidates -> int(76.35) = 76, the cap
    special[1] = (0, 100, 300)   # 298 candidates -> 44, below it
    ids[0] = np.random.default_rng(30).integers(1000, VOCAB, size=512)
    return dict(input_ids=ids, special=special,
                sample_index=[0, 1, 2, 3], seed=42, epoch=0,
                masked_lm_prob=0.15, max_pred=76)


def _token_many_rows():
    ids, special = random_rows(96, 128, seed=4)
    return dict(input_ids=ids, special=special,
                sample_index=np.arange(96) + 1000, seed=42, epoch=2,
                masked_lm_prob=0.15, max_pred=20)


def _token_wide_integers():
    ids, special = random_rows(6, 64, seed=5)
    return dict(input_ids=ids, special=special,
                sample_index=(2 ** 33 + 17) + np.arange(6) * (2 ** 32 + 1),
                seed=2 ** 63 + 2 ** 40 + 9, epoch=5, masked_lm_prob=0.15,
                max_pred=10)


def _token_no_mask_token():
    ids, special = random_rows(8, 64, seed=6)
    return dict(input_ids=ids, special=special, sample_index=np.arange(8),
                seed=3, epoch=0, masked_lm_prob=0.3, max_pred=20,
                original_token_prob=0.5, random_token_prob=0.5)


def _token_zero_prob():
    ids, special = random_rows(6, 32, seed=7)
    special[2] = (0, 1, 2)
    return dict(input_ids=ids, special=special, sample_index=np.arange(6),
                seed=11, epoch=0, masked_lm_prob=0.0, max_pred=5)


def _token_two_specials():
    ids, special = random_rows(7, 80, seed=8, n_special=2)
    return dict(input_ids=ids, special=special, sample_index=np.arange(7),
                seed=5, epoch=1, masked_lm_prob=0.15, max_pred=12)


def _token_wild_specials():
    """Nothing in ``special`` may take an access out of bounds."""
    ids, special = random_rows(6, 32, seed=9)
    special[:] = [(-5, 40, 100), (0, -1, -7), (31, 31, 31),
                  (2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1), (5, 3, 0), (0, 20, 10)]
    return dict(input_ids=ids, special=special, sample_index=np.arange(6),
                seed=13, epoch=0, masked_lm_prob=0.15, max_pred=6)


def _token_thread_map_case(B, S, max_pred, row0_special, prob=0.15):
    """The smallest shapes at which the position-to-thread map (position
    k * 256 + tid, one ballot word per 64 positions) takes another path."""
    def make():
        if S == 1:  # no candidates: nothing selected, every slot is tail
            ids = 1000 + np.arange(B, dtype=np.int32).reshape(B, 1)
            special = np.zeros((B, 3), dtype=np.int32)
        else:
            ids, special = random_rows(B, S, seed=100 * S + B)
        if row0_special is not None:
            special[0] = row0_special
            ids[0] = np.random.default_rng(S).integers(1000, VOCAB, size=S)
        return dict(input_ids=ids, special=special,
                    sample_index=np.arange(B) + 77, seed=42, epoch=1,
                    masked_lm_prob=prob, max_pred=max_pred)
    return make


TOKEN_CASES = {
    "edge_rows_S16": _token_edge_rows,
    "S48": _token_s48,
    "S512_cap": _token_s512,
    "B96_prefix": _token_many_rows,
    "wide_integers": _token_wide_integers,
    "keep_plus_random_is_one": _token_no_mask_token,
    "zero_prob_floor": _token_zero_prob,
    "two_specials": _token_two_specials,
    "wild_specials": _token_wild_specials,
    # no candidates; one position in the second ballot word; one in the
    # second per-thread slot; the maximum length; more rows than threads in
    # the rows-before loop. Masked tokens per row: 0 0 0; 9 6 7; 38 34 20;
    # 153 118; 678 over the 300 rows.
    "S1": _token_thread_map_case(3, 1, 1, (0, 0, 0)),
    "S65": _token_thread_map_case(3, 65, 9, (0, 30, 64)),
    "S257": _token_thread_map_case(3, 257, 38, (0, 100, 256)),
    "S1024": _token_thread_map_case(2, 1024, 153, (0, 500, 1023)),
    "B300_S16_prefix": _token_thread_map_case(300, 16, 4, None, prob=0.3),
}


# ---------------------------------------------------------------------------
# whole-word cases
# ---------------------------------------------------------------------------
def random_table(seed, vocab_size=VOCAB, frac=0.45):
    rng = np.random.default_rng(seed)
    return (rng.random(vocab_size) < frac).astype(np.uint8)


def _wwm_grid_case(B, S):
    def make():
        ids, special = random_rows(B, S, seed=100 * S + B)
        return dict(input_ids=ids, special=special,
                    sample_index=np.arange(B) + 7 * S,
                    word_continues=random_table(S + B), seed=42, epoch=1,
                    masked_lm_prob=0.15, max_pred=max(1, int(S * 0.15)))
    return make


def _wwm_many_rows():
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


def _wwm_all_continuations():
    """Rows 0 and 1 hold continuation pieces only: every segment is one
    word. Row 0's two words (14 and 15 long) exceed n = 4: nothing is
    selected. Row 1's first segment is 2 long and fits."""
    ids = np.full((3, 32), CONT, dtype=np.int32)
    special = np.array([(0, 15, 31), (0, 3, 31), (0, 15, 31)], dtype=np.int32)
    ids[2] = HEAD  # all starts: token-level behaviour
    return dict(input_ids=ids, special=special, sample_index=[1, 2, 3],
                word_continues=_crafted_table(), seed=5, epoch=0,
                masked_lm_prob=0.15, max_pred=8)


def _wwm_no_candidates():
    ids, special = random_rows(4, 16, seed=12)
    special[0] = (0, 1, 2)
    special[2] = (0, 0, 0)
    special[3] = (-3, -1, -7)
    return dict(input_ids=ids, special=special, sample_index=[0, 1, 2, 3],
                word_continues=random_table(12), seed=5, epoch=0,
                masked_lm_prob=0.15, max_pred=3)


def _wwm_sep_and_cls_break_words():
    """Row 0: H C C [SEP] C C H ... - the continuation after [SEP] starts a
    word. Row 1: a continuation at position 1, right after [CLS]."""
    ids = np.full((2, 16), HEAD, dtype=np.int32)
    special = np.array([(0, 4, 12), (0, 6, 12)], dtype=np.int32)
    ids[0, [2, 3, 5, 6]] = CONT
    ids[1, [1, 2]] = CONT
    return dict(input_ids=ids, special=special, sample_index=[21, 22],
                word_continues=_crafted_table(), seed=3, epoch=0,
                masked_lm_prob=0.5, max_pred=8)


def _wwm_cap_binds():
    """max_pred below the table's counts: the table is built for a cap of
    20, the call passes 5."""
    ids, special = random_rows(6, 128, seed=13)
    return dict(input_ids=ids, special=special, sample_index=np.arange(6),
                word_continues=random_table(13), seed=42, epoch=0,
                masked_lm_prob=0.15, max_pred=5, table_max_pred=20)


def _wwm_max_pred_one():
    ids, special = random_rows(8, 48, seed=14)
    return dict(input_ids=ids, special=special, sample_index=np.arange(8),
                word_continues=random_table(14, frac=0.3), seed=42, epoch=0,
                masked_lm_prob=0.15, max_pred=1)


def _wwm_vocab_edge_ids():
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


def _wwm_wide_integers():
    ids, special = random_rows(5, 64, seed=15)
    return dict(input_ids=ids, special=special,
                sample_index=(2 ** 33 + 17) + np.arange(5) * (2 ** 32 + 1),
                word_continues=random_table(15),
                seed=2 ** 63 + 2 ** 40 + 9, epoch=5, masked_lm_prob=0.15,
                max_pred=9)


WWM_CASES = {f"B{B}_S{S}": _wwm_grid_case(B, S)
             for S in (16, 128, 512, 1024) for B in (1, 3, 8)}
WWM_CASES.update({
    "B300_S16_prefix": _wwm_many_rows,
    "all_continuations": _wwm_all_continuations,
    "no_candidates": _wwm_no_candidates,
    "sep_and_cls_break_words": _wwm_sep_and_cls_break_words,
    "max_pred_below_table": _wwm_cap_binds,
    "max_pred_one": _wwm_max_pred_one,
    "vocab_edge_ids": _wwm_vocab_edge_ids,
    "sample_index_above_2_32": _wwm_wide_integers,
})

_SPEC_CACHE = {}


def spec_of(name, whole_word):
    """The case of that table and its expected outputs, computed once per
    session."""
    if (name, whole_word) not in _SPEC_CACHE:
        if whole_word:
            case = WWM_CASES[name]()
            want = spec_mlm_mask_wwm(**case)
        else:
            case = TOKEN_CASES[name]()
            want = spec_mlm_mask(**case)
        _SPEC_CACHE[name, whole_word] = (case, want)
    return _SPEC_CACHE[name, whole_word]


def check_case_facts(name, case, want):
    """What a crafted whole-word case is there to show, read off the expected
    values."""
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
# runner helpers of the two CPU modules
# ---------------------------------------------------------------------------
def _raw(files):
    ids, special = [], []
    for path in files:
        with h5lite.H5LiteFile(path) as f:
            ids.append(np.asarray(f["input_ids"]))
            special.append(np.asarray(f["special_token_positions"]))
    return np.concatenate(ids), np.concatenate(special)


def make_workspace(tmp_path, with_vocab):
    """(tmp_path, data dir, model config[, vocab file]) of a tiny run."""
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
    if not with_vocab:
        return tmp_path, str(data_dir), str(cfg_path)
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
