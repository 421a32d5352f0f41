"""On-device MLM masking (csrc/ops/mlm_mask.hip, ``ops.mlm_mask``).

``spec_mlm_mask`` below is a numpy implementation of the mask function
written from its specification and tests/philox_ref.py alone; it shares no
code with the package. The kernel is integer arithmetic end to end, so
every comparison is ``torch.equal``. All tests @pytest.mark.gpu.
"""

import numpy as np
import pytest
import torch

import philox_ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from bert_pytorch_amd import ops
    from bert_pytorch_amd.config import BertConfig
    from bert_pytorch_amd.models import BertForPreTraining

DEV = "cuda:0"
VOCAB = 30522
MASK = 103


# ---------------------------------------------------------------------------
# numpy specification
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
# the specification's own cross-check vectors (no GPU involved in the
# expected values; the kernel is run on the same inputs)
# ---------------------------------------------------------------------------
def _vector_inputs():
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


def _run_op(input_ids, special, sample_index, *, seed, epoch, masked_lm_prob,
            max_pred, vocab_size=VOCAB, mask_token=MASK,
            original_token_prob=0.1, random_token_prob=0.1, device=DEV):
    S = input_ids.shape[1]
    table = ops.mlm_count_table(S, masked_lm_prob, max_pred).to(device)
    t_keep, t_rand = ops.mlm_thresholds(original_token_prob, random_token_prob)
    return ops.mlm_mask(
        torch.as_tensor(np.asarray(input_ids, dtype=np.int32)).to(device),
        torch.as_tensor(np.asarray(special, dtype=np.int32)).to(device),
        torch.as_tensor(np.asarray(sample_index, dtype=np.int64)).to(device),
        table, seed=seed, epoch=epoch, max_pred=max_pred,
        vocab_size=vocab_size, mask_token=mask_token, t_keep=t_keep,
        t_rand=t_rand, dense_labels=True,
    )


NAMES = ("masked_ids", "token_type_ids", "attention_mask", "positions",
         "gathered_labels", "dense_labels")


def _assert_equal_spec(got, want):
    assert len(got) == len(want) == 6
    for name, g, w in zip(NAMES, got, want):
        w = torch.from_numpy(w)
        assert g.dtype == torch.int64, (name, g.dtype)
        assert g.shape == w.shape, (name, g.shape, w.shape)
        assert torch.equal(g.cpu(), w), name


@pytest.mark.parametrize("vec", VECTORS, ids=["vector1", "vector2"])
def test_spec_vectors(vec):
    ids, special = _vector_inputs()
    words = spec_row_words(16, vec["seed"], vec["epoch"], vec["sample_index"])
    assert " ".join(f"{int(w):08x}" for w in words[1]) == vec["words"]
    kw = dict(seed=vec["seed"], epoch=vec["epoch"], masked_lm_prob=0.5,
              max_pred=8)
    want = spec_mlm_mask(ids, special, [vec["sample_index"]], **kw)
    assert want[0][0].tolist() == vec["ids"]
    assert np.nonzero(want[5][0] != -1)[0].tolist() == vec["label_pos"]
    _assert_equal_spec(_run_op(ids, special, [vec["sample_index"]], **kw), want)


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
def _random_rows(B, S, seed, n_special=3):
    """Shard-like rows: [CLS] a [SEP] b [SEP] pad, lengths in [S/2, S]."""
    rng = np.random.default_rng(seed)
    ids = np.zeros((B, S), dtype=np.int32)
    special = np.zeros((B, n_special), dtype=np.int32)
    for b in range(B):
        total = int(rng.integers(max(5, S // 2), S + 1))
        ids[b, :total] = rng.integers(1000, VOCAB, size=total)
        split = int(rng.integers(1, total - 2))
        special[b] = (0, split, total - 1) if n_special == 3 else (0, total - 1)
    return ids, special


def _case_edge_rows():
    ids, special = _random_rows(5, 16, seed=1)
    special[:4] = [(0, 1, 2), (0, 1, 3), (0, 9, 9), (0, 7, 15)]
    ids[3] = 1000 + np.arange(16)
    return dict(input_ids=ids, special=special,
                sample_index=[3, 1, 4, 1, 5], seed=7, epoch=0,
                masked_lm_prob=0.15, max_pred=4)


def _case_s48():
    ids, special = _random_rows(3, 48, seed=2)
    return dict(input_ids=ids, special=special, sample_index=[10, 11, 12],
                seed=42, epoch=1, masked_lm_prob=0.15, max_pred=8)


def _case_s512():
    ids, special = _random_rows(4, 512, seed=3)
    special[0] = (0, 200, 511)   # 509 candidates -> int(76.35) = 76, the cap
    special[1] = (0, 100, 300)   # 298 candidates -> 44, below it
    ids[0] = np.random.default_rng(30).integers(1000, VOCAB, size=512)
    return dict(input_ids=ids, special=special,
                sample_index=[0, 1, 2, 3], seed=42, epoch=0,
                masked_lm_prob=0.15, max_pred=76)


def _case_many_rows():
    ids, special = _random_rows(96, 128, seed=4)
    return dict(input_ids=ids, special=special,
                sample_index=np.arange(96) + 1000, seed=42, epoch=2,
                masked_lm_prob=0.15, max_pred=20)


def _case_wide_integers():
    ids, special = _random_rows(6, 64, seed=5)
    return dict(input_ids=ids, special=special,
                sample_index=(2 ** 33 + 17) + np.arange(6) * (2 ** 32 + 1),
                seed=2 ** 63 + 2 ** 40 + 9, epoch=5, masked_lm_prob=0.15,
                max_pred=10)


def _case_no_mask_token():
    ids, special = _random_rows(8, 64, seed=6)
    return dict(input_ids=ids, special=special, sample_index=np.arange(8),
                seed=3, epoch=0, masked_lm_prob=0.3, max_pred=20,
                original_token_prob=0.5, random_token_prob=0.5)


def _case_zero_prob():
    ids, special = _random_rows(6, 32, seed=7)
    special[2] = (0, 1, 2)
    return dict(input_ids=ids, special=special, sample_index=np.arange(6),
                seed=11, epoch=0, masked_lm_prob=0.0, max_pred=5)


def _case_two_specials():
    ids, special = _random_rows(7, 80, seed=8, n_special=2)
    return dict(input_ids=ids, special=special, sample_index=np.arange(7),
                seed=5, epoch=1, masked_lm_prob=0.15, max_pred=12)


def _case_wild_specials():
    """Nothing in ``special`` may take an access out of bounds."""
    ids, special = _random_rows(6, 32, seed=9)
    special[:] = [(-5, 40, 100), (0, -1, -7), (31, 31, 31),
                  (2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1), (5, 3, 0), (0, 20, 10)]
    return dict(input_ids=ids, special=special, sample_index=np.arange(6),
                seed=13, epoch=0, masked_lm_prob=0.15, max_pred=6)


CASES = {
    "edge_rows_S16": _case_edge_rows,
    "S48": _case_s48,
    "S512_cap": _case_s512,
    "B96_prefix": _case_many_rows,
    "wide_integers": _case_wide_integers,
    "keep_plus_random_is_one": _case_no_mask_token,
    "zero_prob_floor": _case_zero_prob,
    "two_specials": _case_two_specials,
    "wild_specials": _case_wild_specials,
}

_SPEC_CACHE = {}


def _spec_of(name):
    if name not in _SPEC_CACHE:
        case = CASES[name]()
        _SPEC_CACHE[name] = (case, spec_mlm_mask(**case))
    return _SPEC_CACHE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_spec(name):
    case, want = _spec_of(name)
    _assert_equal_spec(_run_op(**case), want)
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
    case, _ = _spec_of(name)
    got = _run_op(**case)
    fallback = _run_op(**case, device="cpu")
    for n, g, f in zip(NAMES, got, fallback):
        assert not f.is_cuda
        assert torch.equal(g.cpu(), f), n


def test_dense_labels_on_request_only():
    case, want = _spec_of("S48")
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
    case, want = _spec_of("B96_prefix")
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
    _assert_equal_spec(out, want)


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
    ids, special = _random_rows(B, S, seed=12)
    ids = (ids % 900) + 110
    masked, tt, am, positions, gathered, dense = _run_op(
        ids, special, np.arange(B), seed=42, epoch=0, masked_lm_prob=0.15,
        max_pred=max_pred, vocab_size=1024,
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
