"""Padding-free encoder on the eager (CPU) path: index construction,
row pack/unpack, the per-sequence attention composite, model equivalence
with the padded path, and the runners' --unpad flag. No GPU needed."""

import copy
import json

import pytest
import torch

from bert_pytorch_amd import ops
from bert_pytorch_amd.models import (
    BertForPreTraining,
    BertModel,
    BertPretrainingCriterion,
)
from bert_pytorch_amd.ops import _reference as ref


def prefix_mask(lengths, seq):
    return (torch.arange(seq)[None, :] < torch.tensor(lengths)[:, None]).long()


# ---------------------------------------------------------------------------
# unpad_index
# ---------------------------------------------------------------------------
def test_unpad_index_prefix_mask():
    mask = prefix_mask([5, 2, 7], 8)
    dest, cu, total, t_pad = ops.unpad_index(mask)
    assert dest.dtype == torch.int32 and cu.dtype == torch.int32
    assert total == 14 and t_pad == 128 and t_pad % 128 == 0
    assert cu.tolist() == [0, 5, 7, 14]
    expect = [0, 1, 2, 3, 4, -1, -1, -1,
              5, 6, -1, -1, -1, -1, -1, -1,
              7, 8, 9, 10, 11, 12, 13, -1]
    assert dest.tolist() == expect


def test_unpad_index_holes_and_left_padding():
    mask = torch.tensor([
        [0, 0, 1, 1, 1, 1],   # left padding
        [1, 0, 1, 0, 0, 1],   # holes
    ])
    dest, cu, total, t_pad = ops.unpad_index(mask)
    assert total == 7 and t_pad == 128
    assert cu.tolist() == [0, 4, 7]
    assert dest.tolist() == [-1, -1, 0, 1, 2, 3, 4, -1, 5, -1, -1, 6]


def test_unpad_index_all_zero_row_and_rounding():
    mask = torch.zeros(3, 130, dtype=torch.long)
    mask[0, :] = 1
    mask[2, :3] = 1          # row 1 stays empty
    dest, cu, total, t_pad = ops.unpad_index(mask)
    assert total == 133 and t_pad == 256 and t_pad % 128 == 0
    assert cu.tolist() == [0, 130, 130, 133]
    assert (dest.view(3, 130)[1] == -1).all()
    assert dest.view(3, 130)[2, :4].tolist() == [130, 131, 132, -1]
    # exactly 128 valid tokens is not rounded any further
    assert ops.unpad_index(torch.ones(2, 64))[3] == 128
    # no valid token at all
    d0, cu0, t0, tp0 = ops.unpad_index(torch.zeros(2, 4))
    assert t0 == 0 and tp0 == 0 and (d0 == -1).all() and cu0.tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------
# pack_rows / unpack_rows (eager fallback)
# ---------------------------------------------------------------------------
def test_pack_unpack_round_trip():
    torch.manual_seed(0)
    mask = torch.tensor([[1, 1, 0, 1], [0, 0, 0, 0], [0, 1, 1, 0]])
    dest, _cu, total, t_pad = ops.unpad_index(mask)
    x = torch.randn(12, 6)
    packed = ops.pack_rows(x, dest, t_pad)
    assert packed.shape == (t_pad, 6)
    keep = mask.reshape(-1).bool()
    assert torch.equal(packed[:total], x[keep])
    assert (packed[total:] == 0).all()
    back = ops.unpack_rows(packed, dest, 12)
    assert torch.equal(back[keep], x[keep])
    assert (back[~keep] == 0).all()
    # a dropped position never reads the packed matrix
    packed[0] = float("nan")
    back = ops.unpack_rows(packed, dest, 12)
    assert torch.isfinite(back[~keep]).all()


def test_pack_unpack_gradcheck_float64():
    torch.manual_seed(1)
    mask = torch.tensor([[0, 1, 1], [1, 0, 1]])
    dest, _cu, _total, _t_pad = ops.unpad_index(mask)
    t_pad = 6  # gradcheck perturbs every element; keep the matrix small
    x = torch.randn(6, 3, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: ops.pack_rows(t, dest, t_pad), (x,))
    y = torch.randn(t_pad, 3, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: ops.unpack_rows(t, dest, 6), (y,))
    # each op's backward is the other op
    g = torch.randn(t_pad, 3, dtype=torch.float64)
    (gx,) = torch.autograd.grad(ops.pack_rows(x, dest, t_pad), x, g)
    assert torch.equal(gx, ops.unpack_rows(g, dest, 6))


# ---------------------------------------------------------------------------
# eager variable-length attention
# ---------------------------------------------------------------------------
def test_reference_attention_varlen_matches_padded():
    torch.manual_seed(2)
    lengths, seq, nh, hidden = [1, 17, 48], 48, 2, 32
    mask = prefix_mask(lengths, seq)
    dest, cu, total, t_pad = ops.unpad_index(mask)
    qkv = torch.randn(3, seq, 3 * hidden)
    out_pad = ref.attention(
        qkv, torch.tensor(lengths, dtype=torch.int32), nh, 0.0, False
    )
    packed = ops.pack_rows(qkv.view(-1, 3 * hidden), dest, t_pad)
    out = ops.fused_attention_varlen(packed, cu, seq, nh, 0.0, False)
    assert out.shape == (t_pad, hidden)
    assert (out[total:] == 0).all()
    back = ops.unpack_rows(out, dest, 3 * seq).view(3, seq, hidden)
    valid = mask.bool()
    assert torch.allclose(back[valid], out_pad[valid], atol=1e-6)
    assert (back[~valid] == 0).all()


# ---------------------------------------------------------------------------
# model equivalence
# ---------------------------------------------------------------------------
LENGTHS, SEQ = [24, 9, 1], 24


def _inputs(vocab):
    torch.manual_seed(3)
    ids = torch.randint(0, vocab, (len(LENGTHS), SEQ))
    tt = torch.randint(0, 2, (len(LENGTHS), SEQ))
    return ids, tt, prefix_mask(LENGTHS, SEQ)


def test_unpad_inputs_toggle(tiny_config):
    model = BertForPreTraining(tiny_config)
    assert model.bert._unpad_inputs is False  # off by default
    model.unpad_inputs(True)
    assert model.bert._unpad_inputs is True
    model.unpad_inputs(False)
    assert model.bert._unpad_inputs is False


@pytest.mark.parametrize("all_layers", [False, True])
def test_bert_model_unpad_matches_padded_eval(tiny_config, all_layers):
    tiny_config.output_all_encoded_layers = all_layers
    torch.manual_seed(4)
    model = BertModel(tiny_config).eval()
    ids, tt, mask = _inputs(tiny_config.vocab_size)
    with torch.no_grad():
        enc_pad, pooled_pad = model(ids, tt, mask)
        model.unpad_inputs(True)
        enc, pooled = model(ids, tt, mask)
    if not all_layers:
        enc_pad, enc = [enc_pad], [enc]
    assert len(enc) == len(enc_pad) == (2 if all_layers else 1)
    valid = mask.bool()
    for a, b in zip(enc, enc_pad):
        assert a.shape == b.shape
        assert torch.allclose(a[valid], b[valid], atol=1e-5)
        assert (a[~valid] == 0).all()
    assert torch.allclose(pooled, pooled_pad, atol=1e-5)


@pytest.mark.parametrize("checkpoint", [False, True])
def test_pretraining_loss_and_grads_match(tiny_config, checkpoint):
    tiny_config.hidden_dropout_prob = 0.0
    tiny_config.attention_probs_dropout_prob = 0.0
    torch.manual_seed(5)
    padded = BertForPreTraining(tiny_config).train()
    unpadded = copy.deepcopy(padded)
    unpadded.unpad_inputs(True)
    if checkpoint:
        padded.checkpoint_activations(True)
        unpadded.checkpoint_activations(True)
    criterion = BertPretrainingCriterion(tiny_config.vocab_size)
    ids, tt, mask = _inputs(tiny_config.vocab_size)
    labels = torch.full_like(ids, -1)
    labels[:, 0] = ids[:, 0]           # valid in every sequence
    labels[0, 20] = ids[0, 20]
    labels[1, 8] = ids[1, 8]
    nsp = torch.tensor([0, 1, 1])

    losses = []
    for model in (padded, unpadded):
        scores, rel, gathered = model(ids, tt, mask, masked_lm_labels=labels)
        loss = criterion(scores, rel, gathered, nsp)
        loss.backward()
        losses.append(loss.detach())
    assert torch.allclose(losses[0], losses[1], atol=1e-5)
    grads_p = dict(padded.named_parameters())
    for name, prm in unpadded.named_parameters():
        gp = grads_p[name].grad
        assert (gp is None) == (prm.grad is None), name
        if gp is not None:
            assert torch.allclose(prm.grad, gp, atol=1e-5), name


def test_left_padded_mask_matches_right_padded_encoder(tiny_config):
    """A mask that is not a prefix keeps its positions: the encoder over
    left-padded sequences equals the padded encoder over the same
    sequences shifted to the left edge (compared after the embedding
    layer, so position embeddings are out of the picture)."""
    torch.manual_seed(6)
    model = BertModel(tiny_config).eval()
    model.unpad_inputs(True)
    seq, hidden = 16, tiny_config.hidden_size
    lengths = [16, 5, 11]
    left = torch.stack([torch.arange(seq) >= seq - n for n in lengths]).long()
    emb_left = torch.randn(3, seq, hidden)
    emb_right = torch.zeros_like(emb_left)
    for b, n in enumerate(lengths):
        emb_right[b, :n] = emb_left[b, seq - n:]
    with torch.no_grad():
        out_left = model._unpadded_encoder(emb_left, left)[-1]
        out_right = model.encoder(
            emb_right, torch.tensor(lengths, dtype=torch.int32)
        )[-1]
    for b, n in enumerate(lengths):
        assert torch.allclose(out_left[b, seq - n:], out_right[b, :n], atol=1e-5)
        assert (out_left[b, : seq - n] == 0).all()


# ---------------------------------------------------------------------------
# runners
# ---------------------------------------------------------------------------
@pytest.fixture
def model_cfg(tmp_path):
    cfg = {
        "vocab_size": 128, "hidden_size": 64, "num_hidden_layers": 1,
        "num_attention_heads": 4, "intermediate_size": 128,
        "max_position_embeddings": 64, "type_vocab_size": 2,
        "hidden_act": "gelu", "next_sentence": True,
    }
    path = tmp_path / "model.json"
    path.write_text(json.dumps(cfg))
    return str(path)


def _flag(model):
    return [m._unpad_inputs for m in model.modules() if isinstance(m, BertModel)]


def test_run_pretraining_unpad_reaches_model(model_cfg, tmp_path):
    import run_pretraining

    base = ["--model_config_file", model_cfg]
    args = run_pretraining.parse_arguments(base)
    assert args.unpad is False
    model, *_ = run_pretraining.prepare_model(args, torch.device("cpu"))
    assert _flag(model) == [False]

    args = run_pretraining.parse_arguments(base + ["--unpad"])
    assert args.unpad is True
    model, *_ = run_pretraining.prepare_model(args, torch.device("cpu"))
    assert _flag(model) == [True]

    # settable from the JSON training config like the other flags
    train_cfg = tmp_path / "train.json"
    train_cfg.write_text(json.dumps({"unpad": True}))
    args = run_pretraining.parse_arguments(
        base + ["--config_file", str(train_cfg)]
    )
    assert args.unpad is True


def test_run_pretraining_unpad_with_kfac_raises(model_cfg, tmp_path):
    import run_pretraining

    with pytest.raises(ValueError, match="--unpad.*--kfac"):
        run_pretraining.parse_arguments(
            ["--model_config_file", model_cfg, "--unpad", "--kfac"]
        )
    train_cfg = tmp_path / "train.json"
    train_cfg.write_text(json.dumps({"kfac": True}))
    with pytest.raises(ValueError, match="--unpad.*--kfac"):
        run_pretraining.parse_arguments(
            ["--config_file", str(train_cfg), "--unpad"]
        )


def test_run_squad_unpad_reaches_model(model_cfg):
    import run_squad
    from bert_pytorch_amd.config import BertConfig

    config = BertConfig.from_json_file(model_cfg)
    for argv, want in ([], False), (["--unpad"], True):
        args = run_squad.parse_args(argv)
        assert args.unpad is want
        model = run_squad.prepare_model(args, config, torch.device("cpu"))
        assert _flag(model) == [want]


def test_run_ner_unpad_reaches_model(model_cfg):
    import run_ner
    from bert_pytorch_amd.config import BertConfig

    config = BertConfig.from_json_file(model_cfg)
    for argv, want in ([], False), (["--unpad"], True):
        args = run_ner.parse_args(argv)
        assert args.unpad is want
        model = run_ner.prepare_model(args, config, 5, torch.device("cpu"))
        assert _flag(model) == [want]
