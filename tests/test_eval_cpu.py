"""Held-out evaluation on the CPU: the fp32 reference of
ops.mlm_decoder_eval, static masking, evaluate_pretraining, the runner's
--eval_* flags end to end, and a two-rank gloo evaluation."""

import csv
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

import run_pretraining
from bert_pytorch_amd import ops
from bert_pytorch_amd.config import BertConfig
from bert_pytorch_amd.data import (
    DistributedSampler,
    ShardedPretrainingDataset,
    synth,
)
from bert_pytorch_amd.evaluation import evaluate_pretraining, make_eval_loader
from bert_pytorch_amd.models import BertForPreTraining
from bert_pytorch_amd.utils import checkpoint as ckpt_io

CPU = torch.device("cpu")
VOCAB, SEQ, MAX_PRED = 512, 32, 4


# ---------------------------------------------------------------------------
# reference path of ops.mlm_decoder_eval
# ---------------------------------------------------------------------------
def test_reference_matches_cross_entropy_and_argmax():
    g = torch.Generator().manual_seed(0)
    h = torch.randn(37, 24, generator=g)
    w = torch.randn(101, 24, generator=g)
    b = torch.randn(101, generator=g)
    labels = torch.randint(0, 101, (37,), generator=g)
    labels[::5] = -1
    out = ops.mlm_decoder_eval(h, w, b, labels)
    assert isinstance(out, ops.MlmEval)
    scores = F.linear(h, w, b)
    want = F.cross_entropy(scores, labels, ignore_index=-1, reduction="sum")
    torch.testing.assert_close(out.loss_sum, want, rtol=1e-6, atol=1e-5)
    valid = labels != -1
    assert float(out.count) == int(valid.sum())
    pred = scores.argmax(dim=1)
    assert torch.equal(out.pred.long(), pred)
    assert float(out.correct) == int(((pred == labels) & valid).sum())
    assert not out.loss_sum.requires_grad


def test_reference_ties_take_the_lowest_column():
    g = torch.Generator().manual_seed(1)
    w = torch.randn(64, 16, generator=g)
    b = torch.randn(64, generator=g)
    for c in (9, 40, 63):
        w[c] = w[3]
        b[c] = b[3]
    h = torch.randn(6, 16, generator=g)
    h[:4] = 4 * w[3]  # columns 3, 9, 40, 63 share the row maximum
    h[4] = 0
    b_const = torch.full_like(b, 0.5)
    labels = torch.tensor([3, 9, 40, 63, 0, -1])
    out = ops.mlm_decoder_eval(h, w, b, labels)
    assert out.pred[:4].tolist() == [3, 3, 3, 3]
    out = ops.mlm_decoder_eval(h[4:5], w, b_const, labels[4:5])
    assert out.pred.tolist() == [0] and float(out.correct) == 1
    want = F.cross_entropy(
        F.linear(h, w, b), labels, ignore_index=-1, reduction="sum"
    )
    torch.testing.assert_close(
        ops.mlm_decoder_eval(h, w, b, labels).loss_sum, want,
        rtol=1e-6, atol=1e-5,
    )


# ---------------------------------------------------------------------------
# static masking
# ---------------------------------------------------------------------------
def _dataset(data_dir, static=True, seed=5):
    files = sorted(
        os.path.join(data_dir, f) for f in os.listdir(data_dir)
        if f.endswith(".hdf5")
    )
    return ShardedPretrainingDataset(
        files, mask_token_index=103, max_pred_per_seq=MAX_PRED,
        masked_lm_prob=0.15, vocab_size=VOCAB, seed=seed,
        static_masking=static,
    )


def _same_sample(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def eval_dir(tmp_path_factory):
    path = tmp_path_factory.mktemp("heldout")
    synth.make_dataset(
        str(path), num_shards=1, samples_per_shard=32, seq_len=SEQ,
        vocab_size=VOCAB, seed=11,
    )
    return str(path)


def test_static_masking_is_a_function_of_seed_and_index(eval_dir):
    ds = _dataset(eval_dir)
    first = ds[7]
    assert _same_sample(first, ds[7]), "repeated access differs"
    other = _dataset(eval_dir)
    for i in (0, 3, 5):  # another instance, other samples read before
        other[i]
    assert _same_sample(first, other[7])
    assert not _same_sample(first, ds[8])
    assert not np.array_equal(first[3], ds[8][3]), "two idx share a mask"
    assert not _same_sample(first, _dataset(eval_dir, seed=6)[7])
    # the default stays the stateful stream: a second read re-masks
    dyn = _dataset(eval_dir, static=False)
    reads = [dyn[7] for _ in range(4)]
    assert not all(_same_sample(reads[0], r) for r in reads[1:])


def test_static_masking_leaves_the_dynamic_stream_alone(eval_dir):
    """The default path draws what it drew before static_masking existed:
    one choice, one random, one integers per replaced token, from the
    dataset's own generator."""
    ds = _dataset(eval_dir, static=False, seed=3)
    got = ds[0]
    rng = np.random.default_rng(3)
    ids = ds.data["input_ids"][0].copy()
    special = ds.data["special_token_positions"][0]
    want_ids, want_labels = _dataset(eval_dir, static=False)._mask_input(
        ids, special, rng
    )
    assert np.array_equal(got[0], want_ids)
    assert np.array_equal(got[3], want_labels)


# ---------------------------------------------------------------------------
# evaluate_pretraining
# ---------------------------------------------------------------------------
def _model(next_sentence=True, seed=0):
    torch.manual_seed(seed)
    config = BertConfig(
        vocab_size_or_config_json_file=VOCAB, hidden_size=64,
        num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
        max_position_embeddings=64, next_sentence=next_sentence,
    )
    return BertForPreTraining(config)


def _loader(data_dir, world=1, rank=0, batch=4):
    ds = _dataset(data_dir)
    sampler = DistributedSampler(ds, num_replicas=world, rank=rank, seed=5)
    return make_eval_loader(ds, sampler, batch, seed=5)


def _evaluate(model, loader, max_batches):
    loader.sampler.index = 0
    loader.dataset.rewind()
    return evaluate_pretraining(
        model, loader, CPU, autocast_dtype=None,
        max_predictions_per_seq=MAX_PRED, max_batches=max_batches,
    )


def test_evaluate_pretraining_is_repeatable_and_side_effect_free(eval_dir):
    model = _model()
    model.train()
    loader = _loader(eval_dir)
    torch_state = torch.get_rng_state()
    numpy_state = np.random.get_state()[1].copy()
    first = _evaluate(model, loader, max_batches=3)
    second = _evaluate(model, loader, max_batches=3)
    assert first == second
    assert torch.equal(torch.get_rng_state(), torch_state)
    assert np.array_equal(np.random.get_state()[1], numpy_state)
    assert model.training, "previous mode not restored"
    assert all(p.grad is None for p in model.parameters())
    model.eval()
    _evaluate(model, loader, max_batches=1)
    assert not model.training

    assert set(first) == {
        "eval_loss", "eval_mlm_loss", "eval_nsp_loss", "eval_mlm_accuracy",
        "eval_nsp_accuracy", "eval_masked_tokens", "eval_sequences",
    }
    assert 0.0 <= first["eval_mlm_accuracy"] <= 1.0
    assert 0.0 <= first["eval_nsp_accuracy"] <= 1.0
    assert first["eval_loss"] == pytest.approx(
        first["eval_mlm_loss"] + first["eval_nsp_loss"], rel=1e-12
    )
    assert np.isfinite(first["eval_loss"])
    ds = _dataset(eval_dir)
    tokens = sum(int((ds[i][3] != -1).sum()) for i in range(12))
    assert first["eval_masked_tokens"] == tokens
    assert first["eval_sequences"] == 12


def test_evaluate_pretraining_without_nsp_head(tmp_path):
    synth.make_dataset(
        str(tmp_path), num_shards=1, samples_per_shard=16, seq_len=SEQ,
        vocab_size=VOCAB, seed=2, nsp=False,
    )
    out = _evaluate(_model(next_sentence=False), _loader(str(tmp_path)), 2)
    assert "eval_nsp_loss" not in out and "eval_nsp_accuracy" not in out
    assert out["eval_loss"] == out["eval_mlm_loss"]
    assert out["eval_sequences"] == 8 and out["eval_masked_tokens"] > 0
    assert 0.0 <= out["eval_mlm_accuracy"] <= 1.0


@pytest.mark.parametrize("mode", ["unpad", "pure_bf16"])
def test_evaluate_pretraining_on_unpadded_and_bf16_models(eval_dir, mode):
    model = _model()
    plain = _evaluate(model, _loader(eval_dir), max_batches=2)
    if mode == "unpad":
        model.unpad_inputs(True)
    else:
        model.to(torch.bfloat16)
    out = _evaluate(model, _loader(eval_dir), max_batches=2)
    assert out.keys() == plain.keys()
    assert out["eval_masked_tokens"] == plain["eval_masked_tokens"]
    assert out["eval_sequences"] == plain["eval_sequences"] == 8
    assert np.isfinite(out["eval_loss"])
    # same model, same batches: the unpadded encoder computes the same
    # rows (fp32 reassociation only), bf16 weights keep ~3 digits
    rel = 1e-4 if mode == "unpad" else 5e-2
    assert out["eval_loss"] == pytest.approx(plain["eval_loss"], rel=rel)


def test_evaluate_pretraining_scores_a_model_that_knows_the_answer(eval_dir):
    """Accuracy is measured, not merely in range: a decoder bias that
    towers over one token makes every prediction that token."""
    ds = _dataset(eval_dir)
    labels = np.concatenate([ds[i][3] for i in range(8)])
    token = int(np.bincount(labels[labels != -1]).argmax())
    hits = int((labels == token).sum())
    assert hits > 0
    model = _model()
    with torch.no_grad():
        model.cls.predictions.bias[token] = 1.0e4
    out = _evaluate(model, _loader(eval_dir), max_batches=2)
    assert out["eval_mlm_accuracy"] == hits / int((labels != -1).sum())


# ---------------------------------------------------------------------------
# runner end to end (forced onto the CPU wherever it runs)
# ---------------------------------------------------------------------------
@pytest.fixture
def workspace(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    train_dir, held_dir = tmp_path / "data", tmp_path / "heldout"
    synth.make_dataset(
        str(train_dir), num_shards=2, samples_per_shard=32, seq_len=SEQ,
        vocab_size=VOCAB, seed=0,
    )
    synth.make_dataset(
        str(held_dir), num_shards=2, samples_per_shard=8, seq_len=SEQ,
        vocab_size=VOCAB, seed=1,
    )
    model_cfg = {
        "vocab_size": VOCAB, "hidden_size": 64, "num_hidden_layers": 2,
        "num_attention_heads": 4, "intermediate_size": 128,
        "max_position_embeddings": 64, "type_vocab_size": 2,
        "hidden_act": "gelu", "hidden_dropout_prob": 0.1,
        "attention_probs_dropout_prob": 0.1, "initializer_range": 0.02,
        "next_sentence": True,
    }
    cfg_path = tmp_path / "model.json"
    cfg_path.write_text(json.dumps(model_cfg))
    return tmp_path, str(train_dir), str(held_dir), str(cfg_path)


def _args(tmp_path, data_dir, cfg_path, out="out", **overrides):
    argv = [
        "--model_config_file", cfg_path,
        "--input_dir", data_dir,
        "--output_dir", str(tmp_path / out),
        "--local_batch_size", "4",
        "--global_batch_size", "8",
        "--max_steps", "4",
        "--max_predictions_per_seq", str(MAX_PRED),
        "--learning_rate", "1e-3",
        "--warmup_proportion", "0.2",
        "--num_steps_per_checkpoint", "100",
        "--seed", "7",
        "--num_workers", "0",
    ]
    for key, value in overrides.items():
        argv += [f"--{key}", str(value)]
    return run_pretraining.parse_arguments(argv)


def _rows(out_dir):
    (path,) = out_dir.glob("*_metrics.csv")
    with open(path, newline="", encoding="utf-8") as f:
        return list(csv.DictReader(f))


EVAL_KEYS = (
    "eval_loss", "eval_mlm_loss", "eval_nsp_loss", "eval_mlm_accuracy",
    "eval_nsp_accuracy", "eval_masked_tokens", "eval_sequences",
)


def test_runner_logs_eval_rows_and_leaves_training_untouched(workspace):
    tmp_path, train_dir, held_dir, cfg_path = workspace
    run_pretraining.main(_args(tmp_path, train_dir, cfg_path, out="plain"))
    run_pretraining.main(_args(
        tmp_path, train_dir, cfg_path, out="with_eval",
        eval_input_dir=held_dir, eval_interval=2, eval_batches=3,
    ))
    rows = [r for r in _rows(tmp_path / "with_eval") if r["tag"] == "eval"]
    assert [int(r["step"]) for r in rows] == [2, 4]
    for row in rows:
        for key in EVAL_KEYS:
            assert np.isfinite(float(row[key])), (key, row[key])
        assert int(row["eval_sequences"]) == 12
        assert 0.0 <= float(row["eval_mlm_accuracy"]) <= 1.0
    assert rows[0]["eval_masked_tokens"] == rows[1]["eval_masked_tokens"]
    assert rows[0]["eval_loss"] != rows[1]["eval_loss"], "model did not move"
    assert not [r for r in _rows(tmp_path / "plain") if r["tag"] == "eval"]

    states = []
    for out in ("plain", "with_eval"):
        path, step = ckpt_io.find_latest(str(tmp_path / out))
        assert step == 4
        states.append(ckpt_io.load(path)["model"])
    assert states[0].keys() == states[1].keys()
    for name, tensor in states[0].items():
        assert torch.equal(tensor, states[1][name]), f"{name} differs"


def test_runner_eval_once_after_the_last_step(workspace):
    tmp_path, train_dir, held_dir, cfg_path = workspace
    run_pretraining.main(_args(
        tmp_path, train_dir, cfg_path, max_steps=3,
        eval_input_dir=held_dir, eval_batches=2,
    ))
    rows = [r for r in _rows(tmp_path / "out") if r["tag"] == "eval"]
    assert [int(r["step"]) for r in rows] == [3]


def test_runner_eval_flags_come_from_the_json_config(workspace):
    tmp_path, train_dir, held_dir, cfg_path = workspace
    cfg = tmp_path / "train.json"
    cfg.write_text(json.dumps({
        "eval_input_dir": held_dir, "eval_interval": 5, "eval_batches": 2,
    }))
    args = run_pretraining.parse_arguments(
        ["--config_file", str(cfg), "--eval_batches", "1"]
    )
    assert args.eval_input_dir == held_dir
    assert args.eval_interval == 5 and args.eval_batches == 1


def test_runner_rejects_a_too_small_eval_set(workspace):
    tmp_path, train_dir, held_dir, cfg_path = workspace
    args = _args(
        tmp_path, train_dir, cfg_path,
        eval_input_dir=held_dir, eval_batches=5,  # 16 samples = 4 batches
    )
    with pytest.raises(ValueError, match="eval_batches.*16"):
        run_pretraining.main(args)
    assert ckpt_io.find_latest(str(tmp_path / "out")) is None, "trained first"


# ---------------------------------------------------------------------------
# gloo, world 2
# ---------------------------------------------------------------------------
WORLD = 2


def _run_eval_rank(rank, world, port, data_dir, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        out = _evaluate(
            _model(), _loader(data_dir, world=world, rank=rank), max_batches=2
        )
        q.put((rank, out))
        dist.destroy_process_group()
    except Exception as e:  # noqa: BLE001
        q.put((rank, f"ERROR: {e!r}"))


@pytest.mark.timeout(120)
def test_two_ranks_agree_with_one_process_over_their_union(tmp_path):
    """16 samples, batches of 4: rank 0 reads samples 0..7 and rank 1
    samples 8..15, which are the four batches one process reads. Counts
    are equal; the loss sums are the same four fp64 addends in another
    order, so the means may differ in the last bits of an fp64."""
    synth.make_dataset(
        str(tmp_path), num_shards=1, samples_per_shard=16, seq_len=SEQ,
        vocab_size=VOCAB, seed=4,
    )
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [
        ctx.Process(
            target=_run_eval_rank, args=(r, WORLD, 29571, str(tmp_path), q)
        )
        for r in range(WORLD)
    ]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=110) for _ in range(WORLD))
    for p in procs:
        p.join(timeout=30)
    for rank in range(WORLD):
        assert isinstance(results[rank], dict), f"rank {rank}: {results[rank]}"
    assert results[0] == results[1]

    union = _evaluate(_model(), _loader(str(tmp_path)), max_batches=4)
    assert union.keys() == results[0].keys()
    for key, value in union.items():
        if key in ("eval_masked_tokens", "eval_sequences"):
            assert results[0][key] == value, key
        else:
            assert results[0][key] == pytest.approx(value, rel=1e-12), key
    assert union["eval_sequences"] == 16
