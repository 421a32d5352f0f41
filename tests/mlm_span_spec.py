"""Independent specification of span masking, its cases and the helpers of
the two span-masking test modules (a plain helper module like
mlm_mask_spec.py; no fixtures, no tests).

``spec_mlm_mask_span`` is sequential plain Python written from the
definition in docs/KERNELS.md ("Span masking") and tests/philox_ref.py alone;
it shares no code with the package. Besides the six outputs it returns a
trace: per row, the spans taken with their anchor, why each stopped growing,
and the anchors that were skipped because a span had already taken them.
Everything is integer arithmetic, so every comparison is exact.
"""

import numpy as np
import torch

from bert_pytorch_amd import ops
from mlm_mask_spec import (CONT, HEAD, MASK, VOCAB, _crafted_table,
                           random_rows, random_table, spec_count_table,
                           spec_row_word_lists, spec_row_words,
                           spec_thresholds)

# why a span stopped growing
LENGTH, NO_NEIGHBOUR, SELECTED, BUDGET = ("length", "no_neighbour",
                                          "selected", "budget")
REASONS = (LENGTH, NO_NEIGHBOUR, SELECTED, BUDGET)


def spec_span_table(p, max_len):
    norm = 1 - (1 - p) ** max_len
    table = [int((1 - (1 - p) ** k) / norm * 2 ** 32)
             for k in range(1, max_len + 1)]
    table[-1] = 2 ** 32
    return table


def spec_span_length(w3, table):
    """L = 1 + #{k in 1..Lmax-1 : w3 >= table[k-1]}."""
    return 1 + sum(1 for k in range(1, len(table)) if w3 >= table[k - 1])


def spec_mlm_mask_span(input_ids, special, sample_index, word_continues, *,
                       seed, epoch, masked_lm_prob, max_pred, span_p,
                       span_max, vocab_size=VOCAB, mask_token=MASK,
                       original_token_prob=0.1, random_token_prob=0.1,
                       table_max_pred=None):
    """((masked_ids, token_type, attention_mask, positions, gathered_labels,
    dense_labels) as int64 numpy arrays, trace). ``trace[b]`` is a dict:
    ``n``, ``m``, ``ranks`` (first position of a word -> its place in the
    visiting order), ``spans`` (dicts with ``anchor``, ``words`` (the first
    positions), ``positions``, ``stop``, ``decision``) and
    ``skipped_selected`` (anchors met when already selected)."""
    input_ids = np.asarray(input_ids)
    special = np.asarray(special)
    B, S = input_ids.shape
    if special.shape[1] == 2:
        special = np.concatenate([special, special[:, -1:]], axis=1)
    count = spec_count_table(S, masked_lm_prob, table_max_pred or max_pred)
    span_table = spec_span_table(span_p, span_max)
    t_keep, t_rand = spec_thresholds(original_token_prob, random_token_prob)
    ids = input_ids.astype(np.int64).copy()
    tt = np.zeros((B, S), dtype=np.int64)
    am = np.zeros((B, S), dtype=np.int64)
    labels = np.full((B, S), -1, dtype=np.int64)
    chosen = np.zeros((B, S), dtype=bool)
    trace = []
    for b in range(B):
        sp = [int(v) for v in special[b]]
        last = min(max(sp[2], 0), S - 1)
        for j in range(S):
            am[b, j] = int(j <= last)
            tt[b, j] = int(sp[1] < j <= sp[2])
        inside = {v for v in sp if 0 <= v < S}
        cand = [j for j in range(last) if j not in inside]
        n = min(int(count[len(cand)]), max_pred)
        draws = spec_row_words(S, seed, epoch, sample_index[b])
        words = spec_row_word_lists(input_ids[b], cand, word_continues,
                                    vocab_size)
        by_first = {w[0]: w for w in words}
        words.sort(key=lambda w: (int(draws[w[0], 0]) << 32) | w[0])
        row = dict(n=n, m=0, spans=[], skipped_selected=[],
                   ranks={w[0]: r for r, w in enumerate(words)})
        selected = set()  # first positions of the selected words
        m = 0
        for word in words:
            if m >= n:
                break
            if word[0] in selected:
                row["skipped_selected"].append(word[0])
                continue
            if m + len(word) > n:
                continue
            length = spec_span_length(int(draws[word[0], 3]), span_table)
            span, t, x = [word], len(word), word
            stop = LENGTH
            while len(span) < length:
                y = by_first.get(x[0] + len(x))
                if y is None:
                    stop = NO_NEIGHBOUR
                    break
                if y[0] in selected:
                    stop = SELECTED
                    break
                if m + t + len(y) > n:
                    stop = BUDGET
                    break
                span.append(y)
                t += len(y)
                x = y
            w1 = int(draws[word[0], 1])
            decision = ("keep" if w1 < t_keep else
                        "random" if w1 < t_keep + t_rand else "mask")
            for w in span:
                selected.add(w[0])
                for j in w:
                    labels[b, j] = ids[b, j]
                    chosen[b, j] = True
                    if decision == "random":
                        ids[b, j] = (int(draws[j, 2]) * (vocab_size - 1)) >> 32
                    elif decision == "mask":
                        ids[b, j] = mask_token
            m += t
            row["spans"].append(dict(
                anchor=word[0], words=[w[0] for w in span],
                positions=[j for w in span for j in w], stop=stop,
                decision=decision))
        row["m"] = m
        trace.append(row)
    cap = B * max_pred
    positions = np.zeros(cap, dtype=np.int64)
    gathered = np.full(cap, -1, dtype=np.int64)
    where = np.nonzero(chosen.reshape(-1))[0]  # ascending flat index
    positions[: where.size] = where
    gathered[: where.size] = labels.reshape(-1)[where]
    return (ids, tt, am, positions, gathered, labels), trace


# ---------------------------------------------------------------------------
# running the op
# ---------------------------------------------------------------------------
def run_span_op(input_ids, special, sample_index, word_continues, *, seed,
                epoch, masked_lm_prob, max_pred, span_p, span_max,
                vocab_size=VOCAB, mask_token=MASK, original_token_prob=0.1,
                random_token_prob=0.1, table_max_pred=None, dense_labels=True,
                device="cpu"):
    S = np.asarray(input_ids).shape[1]
    table = ops.mlm_count_table(S, masked_lm_prob, table_max_pred or max_pred)
    t_keep, t_rand = ops.mlm_thresholds(original_token_prob, random_token_prob)
    return ops.mlm_mask(
        torch.as_tensor(np.asarray(input_ids, dtype=np.int32)).to(device),
        torch.as_tensor(np.asarray(special, dtype=np.int32)).to(device),
        torch.as_tensor(np.asarray(sample_index, dtype=np.int64)).to(device),
        table.to(device), seed=seed, epoch=epoch, max_pred=max_pred,
        vocab_size=vocab_size, mask_token=mask_token, t_keep=t_keep,
        t_rand=t_rand, dense_labels=dense_labels,
        word_continues=torch.as_tensor(np.asarray(word_continues)).to(device),
        span_table=ops.mlm_span_table(span_p, span_max).to(device),
    )


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
def _span_crafted_s16():
    """Rows 0-1: continuation pieces only, every segment one word. Row 0's
    words (6 and 7 long) exceed n = 3: nothing is selected; row 1's first
    segment is 2 long and fits. Row 2: H C C [SEP] C C H ...: the
    continuation after [SEP] starts a word. Row 3: a continuation right
    after [CLS]. Row 4: every id a start, n = 1 (two candidates)."""
    ids = np.full((5, 16), HEAD, dtype=np.int32)
    special = np.array([(0, 7, 15), (0, 3, 15), (0, 4, 12), (0, 6, 12),
                        (0, 2, 4)], dtype=np.int32)
    ids[0] = ids[1] = CONT
    ids[2, [2, 3, 5, 6]] = CONT
    ids[3, [1, 2]] = CONT
    return dict(input_ids=ids, special=special,
                sample_index=[1, 2, 21, 22, 23],
                word_continues=_crafted_table(), seed=5, epoch=0,
                masked_lm_prob=0.25, max_pred=8, span_p=0.2, span_max=4)


def _span_full_rows(B, S, split, table_seed, frac, prob, span_p, span_max,
                    seed=42):
    """Rows that use all S positions, so that words and spans reach the last
    ballot word and per-thread slot."""
    def make():
        ids, special = random_rows(B, S, seed=100 * S + B)
        rng = np.random.default_rng(S)
        for b in range(B):
            ids[b] = rng.integers(1000, VOCAB, size=S)
            special[b] = (0, split, S - 1)
        return dict(input_ids=ids, special=special,
                    sample_index=np.arange(B) + 7 * S,
                    word_continues=random_table(table_seed, frac=frac),
                    seed=seed, epoch=1, masked_lm_prob=prob,
                    max_pred=max(1, int(S * prob)), span_p=span_p,
                    span_max=span_max)
    return make


def _span_many_rows():
    ids, special = random_rows(300, 16, seed=11)
    return dict(input_ids=ids, special=special,
                sample_index=np.arange(300) + 5000,
                word_continues=random_table(11), seed=9, epoch=0,
                masked_lm_prob=0.3, max_pred=4, span_p=0.3, span_max=3)


def _span_long_into_last():
    """Lmax = 32 with a small p: spans want about 15 words and run into a
    [SEP], `last` or the budget."""
    ids, special = random_rows(6, 64, seed=16)
    special[0] = (0, 20, 63)
    special[1] = (0, 5, 40)
    return dict(input_ids=ids, special=special, sample_index=np.arange(6) + 3,
                word_continues=random_table(16, frac=0.2), seed=42, epoch=0,
                masked_lm_prob=0.5, max_pred=32, span_p=0.02, span_max=32)


def _span_cap_binds():
    """max_pred below the table's counts: the table is built for a cap of
    20, the call passes 5."""
    ids, special = random_rows(6, 128, seed=13)
    return dict(input_ids=ids, special=special, sample_index=np.arange(6),
                word_continues=random_table(13), seed=42, epoch=0,
                masked_lm_prob=0.15, max_pred=5, table_max_pred=20,
                span_p=0.2, span_max=10)


def _span_vocab_edge_ids():
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
                masked_lm_prob=0.4, max_pred=8, span_p=0.3, span_max=5)


def _span_wide_integers():
    ids, special = random_rows(5, 64, seed=15)
    return dict(input_ids=ids, special=special,
                sample_index=(2 ** 33 + 17) + np.arange(5) * (2 ** 32 + 1),
                word_continues=random_table(15),
                seed=2 ** 63 + 2 ** 40 + 9, epoch=5, masked_lm_prob=0.15,
                max_pred=9, span_p=0.2, span_max=10)


def _span_two_specials():
    ids, special = random_rows(7, 80, seed=8, n_special=2)
    return dict(input_ids=ids, special=special, sample_index=np.arange(7),
                word_continues=random_table(8), seed=5, epoch=1,
                masked_lm_prob=0.15, max_pred=12, span_p=0.2, span_max=10)


def _span_token_spans():
    """An all-zero word table: every word is one token."""
    ids, special = random_rows(4, 48, seed=17)
    return dict(input_ids=ids, special=special, sample_index=np.arange(4),
                word_continues=np.zeros(VOCAB, dtype=np.uint8), seed=42,
                epoch=0, masked_lm_prob=0.2, max_pred=9, span_p=0.2,
                span_max=10)


SPAN_CASES = {
    "crafted_S16": _span_crafted_s16,
    # `last` is position 64, the first of the second ballot word, and
    # position 256, the first of the second per-thread slot: a span grows up
    # to the last candidate and looks for its neighbour across that boundary
    "S65": _span_full_rows(3, 65, 30, 65, 0.3, 0.3, 0.1, 16, seed=40),
    "S257": _span_full_rows(3, 257, 100, 257, 0.3, 0.3, 0.1, 16, seed=40),
    # about 100 words a row and a budget of 100 tokens: the wave fill needs
    # a second round of 64 words
    "S128_two_rounds": _span_full_rows(4, 128, 60, 128, 0.2, 0.8, 0.3, 8,
                                       seed=41),
    "S1024_B2": _span_full_rows(2, 1024, 500, 1024, 0.45, 0.15, 0.2, 10),
    "B300_S16_prefix": _span_many_rows,
    "Lmax32_small_p": _span_long_into_last,
    "max_pred_below_table": _span_cap_binds,
    "vocab_edge_ids": _span_vocab_edge_ids,
    "sample_index_above_2_32": _span_wide_integers,
    "two_specials": _span_two_specials,
    "token_spans": _span_token_spans,
}

_SPEC_CACHE = {}


def span_spec_of(name):
    """(case, expected outputs, trace) of that case, computed once per
    session."""
    if name not in _SPEC_CACHE:
        case = SPAN_CASES[name]()
        want, trace = spec_mlm_mask_span(**case)
        _SPEC_CACHE[name] = (case, want, trace)
    return _SPEC_CACHE[name]


def _runs_into(trace, position):
    """A span of several words that ends right below ``position`` because
    no word starts there."""
    return any(s["positions"][-1] == position - 1 and len(s["words"]) > 1
               and s["stop"] == NO_NEIGHBOUR
               for row in trace for s in row["spans"])


def _crosses(trace, position):
    """A span with positions on both sides of ``position``."""
    return any(s["positions"][0] < position <= s["positions"][-1]
               for row in trace for s in row["spans"])


def check_span_case_facts(name, case, want, trace):
    """What a case is there to show, read off the twin's values."""
    counts = (want[5] != -1).sum(axis=1).tolist()
    if name == "crafted_S16":
        assert [row["n"] for row in trace] == [3, 3, 2, 2, 1]
        assert counts[0] == 0 and counts[4] == 1, counts
        assert np.nonzero(want[5][1] != -1)[0].tolist() == [1, 2]
        lab2, lab3 = want[5][2] != -1, want[5][3] != -1
        # words of row 2: [1,2,3] [5,6] [7] .. [11]; of row 3: [1,2] [3] ..
        assert lab2[1] == lab2[2] == lab2[3] and lab2[5] == lab2[6]
        assert lab3[1] == lab3[2]
    if name == "S65":
        assert _runs_into(trace, 64)
    if name == "S257":
        assert _runs_into(trace, 256)
        assert any(_crosses(trace, p) for p in (64, 128, 192))
    if name == "S128_two_rounds":
        # a span anchored in the first 64 words of the visiting order takes
        # a word of the second 64: round two must see what round one did
        assert all(len(row["ranks"]) > 64 for row in trace)
        assert any(row["ranks"][s["anchor"]] < 64
                   and any(row["ranks"][w] >= 64 for w in s["words"])
                   for row in trace for s in row["spans"])
        # round two skips an anchor that a span has taken, and anchors spans
        # of its own
        assert any(row["ranks"][first] >= 64
                   for row in trace for first in row["skipped_selected"])
        assert any(row["ranks"][s["anchor"]] >= 64
                   for row in trace for s in row["spans"])
    if name == "S1024_B2":
        assert max(s["positions"][-1] for s in trace[0]["spans"]) > 768
        assert any(_crosses(trace, p) for p in (256, 512, 768))
    if name == "B300_S16_prefix":
        assert sum(counts) > 300
    if name == "Lmax32_small_p":
        assert any(s["stop"] == NO_NEIGHBOUR and len(s["words"]) > 4
                   for row in trace for s in row["spans"])
    if name == "max_pred_below_table":
        assert max(counts) == 5 and min(counts) >= 3, counts
    if name == "token_spans":
        assert all(len(s["positions"]) == len(s["words"])
                   for row in trace for s in row["spans"])
        assert any(len(s["words"]) > 1 for row in trace for s in row["spans"])


def check_span_invariants(case, want, trace):
    """m <= n, no word split, no special inside a span, one decision class
    per span: read off the outputs, with the words of the twin."""
    input_ids = np.asarray(case["input_ids"])
    special = np.asarray(case["special"])
    ids, labels = want[0], want[5]
    B, S = input_ids.shape
    for b in range(B):
        sp = [int(v) for v in special[b]]
        last = min(max(sp[-1], 0), S - 1)
        inside = {v for v in sp if 0 <= v < S}
        cand = [j for j in range(last) if j not in inside]
        # (an id of -1, outside every vocabulary, is its own label: the
        # selected positions are read off the trace, not off `labels != -1`)
        chosen = {j for s in trace[b]["spans"] for j in s["positions"]}
        assert all(labels[b, j] == (input_ids[b, j] if j in chosen else -1)
                   for j in range(S))
        assert len(chosen) == trace[b]["m"] <= trace[b]["n"]
        assert chosen <= set(cand)
        for word in spec_row_word_lists(input_ids[b], cand,
                                        case["word_continues"],
                                        case.get("vocab_size", VOCAB)):
            assert len(chosen & set(word)) in (0, len(word)), word
        covered = set()
        for span in trace[b]["spans"]:
            pos = span["positions"]
            assert pos == list(range(pos[0], pos[-1] + 1))
            assert not inside & set(pos)  # no special inside
            assert not covered & set(pos)
            covered |= set(pos)
            mask_token = case.get("mask_token", MASK)
            if span["decision"] == "keep":
                assert all(ids[b, j] == input_ids[b, j] for j in pos)
            elif span["decision"] == "mask":
                assert all(ids[b, j] == mask_token for j in pos)
            else:
                assert all(0 <= ids[b, j] < case.get("vocab_size", VOCAB) - 1
                           for j in pos)
        assert covered == chosen
