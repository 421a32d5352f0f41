"""Span masking without a GPU: the op's CPU path against the sequential twin
of mlm_span_spec.py, the span-length table, the DataLoader path and the
runner's flags."""

import json
import math

import numpy as np
import pytest
import torch

import run_pretraining
from bert_pytorch_amd import ops
from bert_pytorch_amd.data import DeviceMasker, ShardedPretrainingDataset, synth
from mlm_mask_spec import (MASK, VOCAB, _argv, _losses, _raw, assert_equal_spec,
                           make_workspace, random_rows, random_table, run_op,
                           spec_row_word_lists, spec_row_words)
from mlm_span_spec import (REASONS, SPAN_CASES, check_span_case_facts,
                           check_span_invariants, run_span_op, span_spec_of,
                           spec_mlm_mask_span, spec_span_length,
                           spec_span_table)


# ---------------------------------------------------------------------------
# the op against the twin
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SPAN_CASES))
def test_cpu_op_equals_sequential_spec(name):
    case, want, trace = span_spec_of(name)
    check_span_case_facts(name, case, want, trace)
    check_span_invariants(case, want, trace)
    assert_equal_spec(run_span_op(**case), want)


def test_cases_reach_every_stop_reason_and_the_selected_anchor_skip():
    """A condition on the case table, checked with the twin alone."""
    seen = {reason: [] for reason in REASONS}
    skipped = []
    for name in SPAN_CASES:
        _case, _want, trace = span_spec_of(name)
        for row in trace:
            for span in row["spans"]:
                seen[span["stop"]].append(name)
            if row["skipped_selected"]:
                skipped.append(name)
    for reason in REASONS:
        assert seen[reason], reason
    assert skipped
    # a row may end below its budget
    assert any(row["m"] < row["n"] for name in SPAN_CASES
               for row in span_spec_of(name)[2])


def test_span_table_needs_word_continues_and_dense_labels_on_request_only():
    case, want, _ = span_spec_of("two_specials")
    got = run_span_op(**case, dense_labels=False)
    assert_equal_spec(got, want, dense_labels=False)
    S = case["input_ids"].shape[1]
    kw = dict(seed=1, epoch=0, max_pred=case["max_pred"], vocab_size=VOCAB,
              mask_token=MASK, t_keep=0, t_rand=0)
    args = (torch.from_numpy(case["input_ids"]),
            torch.from_numpy(case["special"]),
            torch.arange(len(case["input_ids"])),
            ops.mlm_count_table(S, 0.15, case["max_pred"]))
    with pytest.raises(ValueError, match="word_continues"):
        ops.mlm_mask(*args, span_table=ops.mlm_span_table(0.2, 10), **kw)
    words = torch.zeros(VOCAB, dtype=torch.uint8)
    for bad in (torch.zeros(33, dtype=torch.int64),
                torch.zeros(0, dtype=torch.int64),
                torch.zeros(4, dtype=torch.int32)):
        with pytest.raises(ValueError, match="span_table"):
            ops.mlm_mask(*args, word_continues=words, span_table=bad, **kw)


# ---------------------------------------------------------------------------
# Lmax = 1 and the all-zero word table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S128_two_rounds", "crafted_S16",
                                  "max_pred_below_table", "vocab_edge_ids"])
def test_max_length_one_is_whole_word_masking(name):
    case = dict(span_spec_of(name)[0])
    case.pop("span_p"), case.pop("span_max")
    whole = run_op(case.pop("input_ids"), case.pop("special"),
                   case.pop("sample_index"), case.pop("word_continues"),
                   **case)
    case = dict(span_spec_of(name)[0], span_max=1)
    span = run_span_op(**case)
    for k in (1, 2, 3, 4, 5):  # all but masked_ids
        assert torch.equal(span[k], whole[k]), k
    free = whole[5] == -1
    assert torch.equal(span[0][free], whole[0][free])
    assert (whole[5] != -1).any()


def test_all_zero_word_table_masks_token_spans():
    case, want, trace = span_spec_of("token_spans")
    # with Lmax = 1 on top: the token-level selection
    one = run_span_op(**dict(case, span_max=1))
    case = dict(case)
    case.pop("span_p"), case.pop("span_max"), case.pop("word_continues")
    token = run_op(case.pop("input_ids"), case.pop("special"),
                   case.pop("sample_index"), **case)
    for k in (1, 2, 3, 4, 5):
        assert torch.equal(one[k], token[k]), k


# ---------------------------------------------------------------------------
# mlm_span_table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("p,max_len", [(0.2, 10), (0.02, 32), (0.5, 2),
                                       (1.0, 8), (0.3, 1)])
def test_span_table(p, max_len):
    table = ops.mlm_span_table(p, max_len)
    assert table.dtype == torch.int64 and table.shape == (max_len,)
    values = table.tolist()
    assert values == spec_span_table(p, max_len)
    assert values[-1] == 2 ** 32
    assert all(a <= b for a, b in zip(values, values[1:]))
    assert all(0 < v <= 2 ** 32 for v in values)
    if p == 1.0 or max_len == 1:  # every entry 2^32: no w3 reaches it
        assert all(spec_span_length(w3, values) == 1
                   for w3 in (0, 1, 2 ** 31, 2 ** 32 - 1))


def test_span_table_rejects_bad_arguments():
    for p, max_len in [(0.0, 10), (-0.1, 10), (1.5, 10), (0.2, 0), (0.2, 33)]:
        with pytest.raises(ValueError):
            ops.mlm_span_table(p, max_len)


def test_span_length_law():
    """Mean L over the twin's own w3 draws against the mean the table
    implies, sum k * (T_k - T_{k-1}) / 2^32. The draws are independent, so
    the sample mean has standard error sigma / sqrt(N) with the table's own
    sigma; 4 standard errors are missed by chance once in 16000 runs (and
    the seed is fixed)."""
    table = spec_span_table(0.2, 10)
    prob = [(t - s) / 2 ** 32 for s, t in zip([0] + table[:-1], table)]
    mean = sum(k * q for k, q in zip(range(1, 11), prob))
    var = sum(k * k * q for k, q in zip(range(1, 11), prob)) - mean ** 2
    lengths = []
    for index in range(16):
        draws = spec_row_words(1024, 42, 0, index)
        lengths += [spec_span_length(int(w3), table) for w3 in draws[:, 3]]
    N = len(lengths)
    assert N == 16384
    assert abs(sum(lengths) / N - mean) <= 4 * math.sqrt(var / N)
    assert set(lengths) == set(range(1, 11))
    # SpanBERT's figure for p = 0.2, clipped at 10: a mean length of 3.8
    assert abs(mean - 3.8) < 0.05


# ---------------------------------------------------------------------------
# invariants and order independence on random rows
# ---------------------------------------------------------------------------
def _random_case(seed):
    rng = np.random.default_rng(seed)
    S = int(rng.choice([24, 70, 130]))
    ids, special = random_rows(6, S, seed=seed)
    prob = float(rng.choice([0.15, 0.4]))
    return dict(input_ids=ids, special=special,
                sample_index=rng.integers(0, 2 ** 40, size=6),
                word_continues=random_table(seed, frac=float(rng.random())),
                seed=int(rng.integers(0, 2 ** 63)), epoch=int(rng.integers(9)),
                masked_lm_prob=prob, max_pred=max(1, int(S * prob)),
                span_p=float(rng.choice([0.05, 0.2, 0.6])),
                span_max=int(rng.choice([2, 10, 32])))


@pytest.mark.parametrize("seed", range(6))
def test_invariants_on_random_batches(seed):
    case = _random_case(seed)
    want, trace = spec_mlm_mask_span(**case)
    check_span_invariants(case, want, trace)
    got = run_span_op(**case)
    assert_equal_spec(got, want)


def test_a_row_does_not_depend_on_its_batch():
    case, want, _ = span_spec_of("S128_two_rounds")
    perm = np.random.default_rng(0).permutation(len(case["input_ids"]))
    shuffled = dict(case, input_ids=case["input_ids"][perm],
                    special=case["special"][perm],
                    sample_index=np.asarray(case["sample_index"])[perm])
    got = run_span_op(**shuffled)
    for k in (0, 1, 2, 5):
        assert torch.equal(got[k], torch.from_numpy(want[k][perm])), k
    alone = run_span_op(**dict(case, input_ids=case["input_ids"][3:4],
                               special=case["special"][3:4],
                               sample_index=case["sample_index"][3:4]))
    assert torch.equal(alone[0][0], torch.from_numpy(want[0][3]))
    assert torch.equal(alone[5][0], torch.from_numpy(want[5][3]))
    other_epoch = run_span_op(**dict(case, epoch=case["epoch"] + 1))
    assert not torch.equal(other_epoch[5], torch.from_numpy(want[5]))


# ---------------------------------------------------------------------------
# DeviceMasker
# ---------------------------------------------------------------------------
def test_device_masker_builds_and_passes_the_span_table():
    case, want, _ = span_spec_of("two_specials")
    kw = dict(seed=case["seed"], mask_token_index=MASK,
              max_pred_per_seq=case["max_pred"],
              masked_lm_prob=case["masked_lm_prob"], vocab_size=VOCAB)
    words = torch.from_numpy(case["word_continues"])
    masker = DeviceMasker(word_continues=words, span_max_length=10,
                          span_geometric_p=0.2, **kw)
    B = len(case["input_ids"])
    batch = [torch.from_numpy(case["input_ids"]),
             torch.from_numpy(case["special"]), torch.zeros(B, dtype=torch.long),
             torch.from_numpy(np.asarray(case["sample_index"]))]
    out = masker(batch, case["epoch"])
    for g, w in zip(out[:5], want[:5]):
        assert torch.equal(g, torch.from_numpy(w))
    cpu = torch.device("cpu")
    assert masker.span_length_table(cpu) is masker.span_length_table(cpu)
    assert torch.equal(masker.span_length_table(cpu),
                       ops.mlm_span_table(0.2, 10))
    assert DeviceMasker(word_continues=words, **kw).span_length_table(cpu) is None
    with pytest.raises(ValueError, match="word_continues"):
        DeviceMasker(span_max_length=10, **kw)
    with pytest.raises(ValueError):
        DeviceMasker(word_continues=words, span_max_length=40, **kw)


# ---------------------------------------------------------------------------
# CPU loader
# ---------------------------------------------------------------------------
SEQ, MAX_PRED, PROB = 48, 12, 0.3


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    directory = tmp_path_factory.mktemp("span_shards")
    return synth.make_dataset(
        str(directory), num_shards=2, samples_per_shard=16, seq_len=SEQ,
        vocab_size=VOCAB, seed=3,
    )


def _dataset(files, seed=42, **kw):
    return ShardedPretrainingDataset(
        files, mask_token_index=MASK, max_pred_per_seq=MAX_PRED,
        masked_lm_prob=PROB, vocab_size=VOCAB, seed=seed, **kw,
    )


def _runs(positions):
    """Maximal runs of consecutive positions."""
    runs = []
    for j in sorted(positions):
        if runs and runs[-1][-1] == j - 1:
            runs[-1].append(j)
        else:
            runs.append([j])
    return runs


def test_loader_masks_spans_of_whole_words(shards):
    raw_ids, raw_special = _raw(shards)
    table = random_table(77, frac=0.4)
    dataset = _dataset(shards, span_masking=True, word_continues=table,
                       span_max_length=6, span_geometric_p=0.3,
                       original_token_prob=0.3, random_token_prob=0.3)
    assert dataset.span_masking and dataset.whole_word_masking
    several, classes = 0, set()
    for idx in range(len(dataset)):
        masked, _seg, _am, labels, _nsp = dataset[idx]
        sp = [int(v) for v in raw_special[idx]]
        cand = [j for j in range(sp[-1]) if j not in sp]
        n = min(MAX_PRED, max(1, int(len(cand) * PROB)))
        words = spec_row_word_lists(raw_ids[idx], cand, table, VOCAB)
        selected = set(np.nonzero(labels != -1)[0].tolist())
        assert selected <= set(cand)  # no special
        assert len(selected) <= n
        for word in words:
            assert len(selected & set(word)) in (0, len(word)), (idx, word)
        picked = sorted(selected)
        assert np.array_equal(labels[picked], raw_ids[idx][picked])
        rest = [j for j in range(SEQ) if j not in selected]
        assert np.array_equal(masked[rest], raw_ids[idx][rest])
        # a maximal run of selected positions is one or more whole spans; a
        # [MASK] inside it marks a "mask" span, which is [MASK] throughout:
        # so every word of the run is all [MASK] or has none
        for run in _runs(selected):
            several += sum(1 for w in words if w[0] in run) > 1
            for word in (w for w in words if w[0] in run):
                hits = sum(int(masked[j] == MASK) for j in word)
                assert hits in (0, len(word))
                kept = sum(int(masked[j] == raw_ids[idx][j]) for j in word)
                classes.add("mask" if hits else
                            "keep" if kept == len(word) else "random")
    assert several > 0  # some span of several words was masked
    assert classes == {"mask", "keep", "random"}


def test_loader_is_deterministic_per_seed(shards):
    table = random_table(77, frac=0.4)
    kw = dict(span_masking=True, word_continues=table)
    a, b, c = (_dataset(shards, seed=s, **kw) for s in (42, 42, 43))
    same = True
    for idx in range(8):
        xa, xb, xc = a[idx], b[idx], c[idx]
        for u, v in zip(xa, xb):
            assert np.array_equal(u, v)
        same = same and np.array_equal(xa[3], xc[3])
    assert not same


def test_loader_max_length_one_follows_the_whole_word_rule(shards):
    """With span_max_length = 1 a span is one word and the words are visited
    in the order whole-word masking draws from the same generator state: the
    first sample of two fresh datasets has the same selected positions."""
    table = random_table(77, frac=0.6)
    span = _dataset(shards, span_masking=True, span_max_length=1,
                    word_continues=table)
    whole = _dataset(shards, whole_word_masking=True, word_continues=table)
    a, b = span[0][3], whole[0][3]
    assert np.array_equal(a != -1, b != -1) and (a != -1).any()
    assert np.array_equal(a, b)


def test_loader_flag_errors_and_static_masks(shards):
    with pytest.raises(ValueError, match="span_masking needs word_continues"):
        _dataset(shards, span_masking=True)
    with pytest.raises(ValueError, match="word_continues"):
        _dataset(shards, span_masking=True,
                 word_continues=np.zeros(7, dtype=np.uint8))
    table = np.ones(VOCAB, dtype=np.uint8)
    with pytest.raises(ValueError, match="span_max_length"):
        _dataset(shards, span_masking=True, word_continues=table,
                 span_max_length=33)
    with pytest.raises(ValueError, match="span_geometric_p"):
        _dataset(shards, span_masking=True, word_continues=table,
                 span_geometric_p=0.0)
    static = _dataset(shards, static_masking=True)
    static_span = _dataset(shards, static_masking=True, span_masking=True,
                           word_continues=table)
    assert static_span.span_masking is False
    raw = _dataset(shards, device_masking=True)
    raw_span = _dataset(shards, device_masking=True, span_masking=True)
    for idx in (0, 1, 2):
        for a, b in zip(static[idx], static_span[idx]):
            assert np.array_equal(a, b)
        for a, b in zip(raw[idx], raw_span[idx]):
            assert np.array_equal(a, b)


def test_loader_is_unchanged_without_the_flag(shards):
    """Seed for seed the masks of the parent commit: a copy of its
    token-level selection, run on the same generator, with the new keywords
    at their defaults and at other values (inert without span_masking)."""
    raw_ids, raw_special = _raw(shards)
    for kw in ({}, dict(span_max_length=3, span_geometric_p=0.7)):
        dataset = _dataset(shards, **kw)
        assert dataset.span_masking is False
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
            assert np.array_equal(masked, want_ids)


# ---------------------------------------------------------------------------
# runner
# ---------------------------------------------------------------------------
@pytest.fixture
def workspace(tmp_path):
    return make_workspace(tmp_path, with_vocab=True)


def test_flags_parse_from_cli_and_json_and_need_a_vocab_file(workspace):
    tmp_path, data_dir, cfg_path, vocab_path = workspace
    argv = _argv(tmp_path, data_dir, cfg_path)
    args = run_pretraining.parse_arguments(argv)
    assert args.span_masking is False
    assert (args.span_max_length, args.span_geometric_p) == (10, 0.2)
    args = run_pretraining.parse_arguments(
        argv + ["--span_masking", "--span_max_length", "6",
                "--span_geometric_p", "0.3", "--vocab_file", vocab_path])
    assert args.span_masking is True and args.whole_word_masking is True
    assert (args.span_max_length, args.span_geometric_p) == (6, 0.3)
    train_cfg = tmp_path / "train.json"
    train_cfg.write_text(json.dumps(
        {"span_masking": True, "span_max_length": 5, "span_geometric_p": 0.4,
         "vocab_file": vocab_path}))
    args = run_pretraining.parse_arguments(
        argv + ["--config_file", str(train_cfg)])
    assert args.span_masking is True and args.vocab_file == vocab_path
    assert (args.span_max_length, args.span_geometric_p) == (5, 0.4)
    masker = run_pretraining.prepare_masker(args)
    assert torch.equal(masker.span_table, ops.mlm_span_table(0.4, 5))
    with pytest.raises(ValueError, match="--span_masking needs --vocab_file"):
        run_pretraining.parse_arguments(argv + ["--span_masking"])
    with pytest.raises(ValueError, match="--span_max_length"):
        run_pretraining.parse_arguments(
            argv + ["--span_masking", "--span_max_length", "33",
                    "--vocab_file", vocab_path])
    with pytest.raises(ValueError, match="--span_geometric_p"):
        run_pretraining.parse_arguments(
            argv + ["--span_masking", "--span_geometric_p", "0",
                    "--vocab_file", vocab_path])
    args = run_pretraining.parse_arguments(
        argv + ["--span_masking", "--vocab_file",
                str(tmp_path / "missing.txt")])
    with pytest.raises(ValueError, match="--span_masking.*does not exist"):
        run_pretraining.prepare_masker(args)
    # whole-word masking alone builds no span table
    args = run_pretraining.parse_arguments(
        argv + ["--whole_word_masking", "--vocab_file", vocab_path])
    assert run_pretraining.prepare_masker(args).span_table is None


def _workspace(tmp_path, name):
    (tmp_path / name).mkdir()
    return make_workspace(tmp_path / name, with_vocab=True)


def _run(workspace, *extra):
    tmp_path, data_dir, cfg_path, vocab_path = workspace
    args = run_pretraining.parse_arguments(
        _argv(tmp_path, data_dir, cfg_path, "--vocab_file", vocab_path,
              *extra))
    assert run_pretraining.main(args) == 2
    losses = _losses(tmp_path)
    assert len(losses) == 2
    assert all(math.isfinite(v) and v > 0 for v in losses), losses
    return losses


@pytest.mark.parametrize(
    "extra", [("--device_masking",), ("--device_masking", "--unpad"), (),
              ("--whole_word_masking",)],
    ids=["device_masking", "device_masking_unpad", "cpu_loader",
         "with_whole_word_flag"])
def test_runner_with_span_masking(tmp_path, extra):
    """Two steps train; the same seed gives the same losses; giving
    --whole_word_masking as well changes nothing."""
    first = _run(_workspace(tmp_path, "a"),
                 "--span_masking", *extra)
    rest = tuple(e for e in extra if e != "--whole_word_masking")
    again = _run(_workspace(tmp_path, "b"),
                 "--span_masking", *rest)
    assert first == again


def test_runner_without_the_flag_is_unchanged(tmp_path):
    """The span options are inert without --span_masking: bit for bit the
    losses of the plain run, whose masks are the parent commit's
    (test_loader_is_unchanged_without_the_flag), and not those of a span
    run."""
    plain = _run(_workspace(tmp_path, "a"))
    inert = _run(_workspace(tmp_path, "b"),
                 "--span_max_length", "3", "--span_geometric_p", "0.7")
    span = _run(_workspace(tmp_path, "c"),
                "--span_masking")
    assert plain == inert
    assert plain != span
