"""Device masking on the CPU (the torch fallback of ``ops.mlm_mask``):
mask invariants on synthetic shards, independence from how the run is
launched, the distribution of the draws on fixed inputs, and the runner."""

import json
import math

import numpy as np
import pytest
import torch

import run_pretraining
from bert_pytorch_amd import ops
from bert_pytorch_amd.data import (
    DeviceMasker,
    DistributedSampler,
    ShardedPretrainingDataset,
    h5lite,
    synth,
)
from bert_pytorch_amd.parallel import comm
from mlm_mask_spec import (
    MASK,
    TOKEN_CASES,
    VECTORS,
    VOCAB,
    _argv,
    _losses,
    _raw,
    assert_equal_spec,
    make_workspace,
    run_op,
    spec_mlm_mask,
    spec_of,
    vector_inputs,
)

SEQ = 48
MAX_PRED = 8
PROB = 0.15
BATCH = 4


def _dataset(files, **kw):
    return ShardedPretrainingDataset(
        files, mask_token_index=MASK, max_pred_per_seq=MAX_PRED,
        masked_lm_prob=PROB, vocab_size=VOCAB, seed=42, device_masking=True,
        **kw,
    )


def _masker(seed=42):
    return DeviceMasker(
        seed=seed, mask_token_index=MASK, max_pred_per_seq=MAX_PRED,
        masked_lm_prob=PROB, vocab_size=VOCAB,
    )


def _loader(files, num_workers=0, sampler_state=None):
    dataset = _dataset(files)
    sampler = DistributedSampler(dataset, 1, rank=0, seed=42)
    if sampler_state is not None:
        sampler.load_state_dict(sampler_state)
    loader = torch.utils.data.DataLoader(
        dataset, sampler=sampler, batch_size=BATCH, num_workers=num_workers,
        worker_init_fn=comm.WorkerInitObj(42), drop_last=True,
    )
    return loader, sampler


@pytest.fixture(scope="module", params=[True, False], ids=["nsp", "no_nsp"])
def shards(request, tmp_path_factory):
    directory = tmp_path_factory.mktemp("shards")
    files = synth.make_dataset(
        str(directory), num_shards=2, samples_per_shard=16, seq_len=SEQ,
        vocab_size=VOCAB, nsp=request.param, seed=3,
    )
    return files


@pytest.fixture(scope="module")
def nsp_shards(tmp_path_factory):
    directory = tmp_path_factory.mktemp("nsp_shards")
    return synth.make_dataset(
        str(directory), num_shards=2, samples_per_shard=16, seq_len=SEQ,
        vocab_size=VOCAB, seed=5,
    )


def _mask_all(batch, epoch, masker=None, dense=True):
    masker = masker or _masker()
    input_ids, special, _nsp, index = batch
    return ops.mlm_mask(
        input_ids, special, index,
        masker.count_table(input_ids.shape[1], input_ids.device),
        seed=masker.seed, epoch=epoch, max_pred=masker.max_pred_per_seq,
        vocab_size=masker.vocab_size, mask_token=masker.mask_token_index,
        t_keep=masker.t_keep, t_rand=masker.t_rand, dense_labels=dense,
    )


# ---------------------------------------------------------------------------
# dataset mode
# ---------------------------------------------------------------------------
def test_dataset_returns_raw_rows_and_draws_nothing(shards):
    raw_ids, raw_special = _raw(shards)
    dataset = _dataset(shards)
    before = dataset._rng.bit_generator.state
    for idx in (0, 1, 17):
        ids, special, nsp, index = dataset[idx]
        assert ids.dtype == np.int32 and ids.shape == (SEQ,)
        assert special.dtype == np.int32 and special.shape == (3,)
        assert nsp.dtype == np.int64 and index.dtype == np.int64
        assert int(index) == idx
        assert np.array_equal(ids, raw_ids[idx])
        want = list(raw_special[idx])
        assert special.tolist() == want + [want[-1]] * (3 - len(want))
    assert dataset._rng.bit_generator.state == before


def test_exclusive_with_static_masking(shards):
    with pytest.raises(ValueError, match="mutually exclusive"):
        _dataset(shards, static_masking=True)


def test_premasked_shard_raises_naming_the_flag(tmp_path):
    n, s, p = 4, 16, 3
    path = str(tmp_path / "legacy.hdf5")
    h5lite.write(path, {
        "input_ids": np.full((n, s), 1000, dtype=np.int32),
        "segment_ids": np.zeros((n, s), dtype=np.int32),
        "input_mask": np.ones((n, s), dtype=np.int32),
        "masked_lm_positions": np.tile(np.arange(1, p + 1, dtype=np.int32), (n, 1)),
        "masked_lm_ids": np.full((n, p), 1000, dtype=np.int32),
        "next_sentence_labels": np.zeros(n, dtype=np.int8),
    })
    dataset = ShardedPretrainingDataset(
        [path], mask_token_index=MASK, max_pred_per_seq=p, masked_lm_prob=PROB,
        vocab_size=VOCAB, seed=0, device_masking=True,
    )
    with pytest.raises(ValueError, match="device_masking"):
        dataset[0]
    # without the flag the same shard still reads
    plain = ShardedPretrainingDataset(
        [path], mask_token_index=MASK, max_pred_per_seq=p, masked_lm_prob=PROB,
        vocab_size=VOCAB, seed=0,
    )
    assert len(plain[0]) == 5


# ---------------------------------------------------------------------------
# invariants
# ---------------------------------------------------------------------------
def test_mask_invariants_on_synthetic_shards(shards):
    raw_ids, raw_special = _raw(shards)
    loader, _ = _loader(shards)
    seen = 0
    for batch in loader:
        masked, tt, am, positions, gathered, labels = _mask_all(batch, epoch=0)
        index = batch[3].tolist()
        for row, idx in enumerate(index):
            orig = raw_ids[idx].astype(np.int64)
            special = [int(v) for v in raw_special[idx]]
            last = special[-1]
            lab = labels[row].numpy()
            where = np.nonzero(lab != -1)[0]
            assert all(j < last and j not in special for j in where)
            assert np.array_equal(lab[where], orig[where])
            cands = last - len(set(special) - {last})
            assert len(where) == min(MAX_PRED, max(1, int(cands * PROB)))
            changed = np.nonzero(masked[row].numpy() != orig)[0]
            assert set(changed) <= set(where)
            assert am[row].tolist() == [int(j <= last) for j in range(SEQ)]
            want_tt = [0] * SEQ
            if len(special) == 3:
                want_tt = [int(special[1] < j <= special[2]) for j in range(SEQ)]
            assert tt[row].tolist() == want_tt
        # the gathered layout is the padded gather of the dense labels
        flat = labels.reshape(-1)
        real = torch.nonzero(flat != -1).squeeze(-1)
        assert torch.equal(positions[: real.numel()], real)
        assert torch.equal(gathered[: real.numel()], flat[real])
        assert not positions[real.numel():].any()
        assert (gathered[real.numel():] == -1).all()
        assert positions.numel() == BATCH * MAX_PRED
        seen += len(index)
    assert seen == 32


def test_fallback_equals_numpy_spec(shards):
    raw_ids, raw_special = _raw(shards)
    index = np.arange(len(raw_ids)) + 2 ** 33
    kw = dict(seed=2 ** 40 + 7, epoch=3, masked_lm_prob=PROB, max_pred=MAX_PRED)
    want = spec_mlm_mask(raw_ids, raw_special, index, **kw)
    t_keep, t_rand = ops.mlm_thresholds(0.1, 0.1)
    got = ops.mlm_mask(
        torch.from_numpy(raw_ids), torch.from_numpy(raw_special),
        torch.from_numpy(index), ops.mlm_count_table(SEQ, PROB, MAX_PRED),
        seed=kw["seed"], epoch=3, max_pred=MAX_PRED, vocab_size=VOCAB,
        mask_token=MASK, t_keep=t_keep, t_rand=t_rand, dense_labels=True,
    )
    for g, w in zip(got, want):
        assert g.dtype == torch.int64
        assert torch.equal(g, torch.from_numpy(w))


@pytest.mark.parametrize("name", list(TOKEN_CASES))
def test_cpu_op_equals_numpy_spec(name):
    case, want = spec_of(name, False)
    assert_equal_spec(run_op(**case), want)


@pytest.mark.parametrize("vec", VECTORS, ids=["vector1", "vector2"])
def test_fallback_on_the_cross_check_vectors(vec):
    ids, special = vector_inputs()
    t_keep, t_rand = ops.mlm_thresholds(0.1, 0.1)
    masked, _tt, am, positions, gathered, labels = ops.mlm_mask(
        torch.from_numpy(ids), torch.from_numpy(special),
        torch.tensor([vec["sample_index"]]), ops.mlm_count_table(16, 0.5, 8),
        seed=vec["seed"], epoch=vec["epoch"], max_pred=8, vocab_size=VOCAB,
        mask_token=MASK, t_keep=t_keep, t_rand=t_rand, dense_labels=True,
    )
    assert masked[0].tolist() == vec["ids"]
    assert torch.nonzero(labels[0] != -1).flatten().tolist() == vec["label_pos"]
    assert positions.tolist() == vec["label_pos"] + [0, 0, 0]
    assert gathered.tolist() == [1000 + j for j in vec["label_pos"]] + [-1] * 3
    assert am[0].tolist() == [1] * 14 + [0, 0]


def test_thresholds_and_count_table():
    assert ops.mlm_thresholds(0.1, 0.1) == (429496729, 429496729)
    assert sum(ops.mlm_thresholds(0.5, 0.5)) == 1 << 32
    with pytest.raises(ValueError):
        ops.mlm_thresholds(0.6, 0.5)
    table = ops.mlm_count_table(128, 0.15, 20)
    assert table.dtype == torch.int32 and table.shape == (129,)
    assert table.tolist() == [
        0 if c == 0 else min(20, max(1, int(c * 0.15))) for c in range(129)
    ]
    assert ops.mlm_count_table(16, 0.0, 5).tolist() == [0] + [1] * 16


# ---------------------------------------------------------------------------
# launch independence
# ---------------------------------------------------------------------------
def _masked_batches(loader, epoch=0):
    masker = _masker()
    return [masker(batch, epoch) for batch in loader]


def _assert_same_batches(a, b):
    assert len(a) == len(b) and a
    for x, y in zip(a, b):
        assert len(x) == len(y) == 6
        for t, u in zip(x, y):
            assert torch.equal(t, u)


def test_worker_count_does_not_change_masks(nsp_shards):
    single, _ = _loader(nsp_shards, num_workers=0)
    multi, _ = _loader(nsp_shards, num_workers=2)
    _assert_same_batches(_masked_batches(single), _masked_batches(multi))


def test_resumed_loader_reproduces_the_uninterrupted_run(nsp_shards):
    full = _masked_batches(_loader(nsp_shards)[0])
    k = 3
    loader, sampler = _loader(nsp_shards)
    masker = _masker()
    head = []
    it = iter(loader)
    for _ in range(k):
        head.append(masker(next(it), 0))
    state = sampler.state_dict()
    assert state["index"] == k * BATCH
    del it, loader, sampler
    resumed, _ = _loader(nsp_shards, sampler_state=state)
    tail = _masked_batches(resumed)
    assert len(tail) == len(full) - k
    _assert_same_batches(head + tail, full)


def test_epochs_differ_and_batch_layout_does_not_matter(nsp_shards):
    loader, _ = _loader(nsp_shards)
    batches = list(loader)
    first = batches[0]
    e0 = _mask_all(first, epoch=0)
    e1 = _mask_all(first, epoch=1)
    assert not torch.equal(e0[5], e1[5])
    assert torch.equal(e0[1], e1[1]) and torch.equal(e0[2], e1[2])
    # the same samples in another order, in a batch of another size
    both = [torch.cat([a, b]) for a, b in zip(batches[2], first)]
    perm = torch.tensor([6, 1, 4, 7, 0])
    mixed = [t[perm] for t in both]
    got = _mask_all(mixed, epoch=0)
    for row, src in enumerate(perm.tolist()):
        if src < BATCH:
            continue  # a row of batches[2]
        for k in (0, 1, 2, 5):
            assert torch.equal(got[k][row], e0[k][src - BATCH])
    # another seed is another mask
    other = _mask_all(first, epoch=0, masker=_masker(seed=43))
    assert not torch.equal(other[5], e0[5])


# ---------------------------------------------------------------------------
# distribution on fixed inputs
# ---------------------------------------------------------------------------
def test_distribution_on_fixed_inputs():
    rows, seq = 4096, 128
    rng = np.random.default_rng(0)
    ids = rng.integers(1000, VOCAB, size=(rows, seq)).astype(np.int32)
    special = np.tile(np.array([[0, 50, 101]], dtype=np.int32), (rows, 1))
    index = np.arange(rows, dtype=np.int64)
    t_keep, t_rand = ops.mlm_thresholds(0.1, 0.1)
    masked, _tt, _am, _pos, _gl, labels = ops.mlm_mask(
        torch.from_numpy(ids), torch.from_numpy(special),
        torch.from_numpy(index), ops.mlm_count_table(seq, 0.15, 20), seed=42,
        epoch=0, max_pred=20, vocab_size=VOCAB, mask_token=MASK,
        t_keep=t_keep, t_rand=t_rand, dense_labels=True,
    )
    # the first rows against the numpy specification
    want = spec_mlm_mask(ids[:32], special[:32], index[:32], seed=42, epoch=0,
                         masked_lm_prob=0.15, max_pred=20)
    assert torch.equal(masked[:32], torch.from_numpy(want[0]))
    assert torch.equal(labels[:32], torch.from_numpy(want[5]))

    masked, labels = masked.numpy(), labels.numpy()
    selected = labels != -1
    assert (selected.sum(axis=1) == 14).all()
    assert selected.sum() == 57344
    freq = selected.mean(axis=0)
    never = [0, 50, 101] + list(range(102, seq))
    candidates = [j for j in range(seq) if j not in never]
    assert len(candidates) == 99
    assert not selected[:, never].any()
    lo, hi = freq[candidates].min(), freq[candidates].max()
    print(f"selection frequency range {lo:.4f}-{hi:.4f}")
    assert 0.125 <= lo and hi <= 0.158, (lo, hi)

    orig = ids.astype(np.int64)
    assert np.array_equal(labels[selected], orig[selected])
    assert np.array_equal(masked[~selected], orig[~selected])
    new, old = masked[selected], orig[selected]
    total = float(new.size)
    unchanged = (new == old).sum() / total
    to_mask = ((new == MASK) & (new != old)).sum() / total
    other = ((new != MASK) & (new != old)).sum() / total
    print(f"unchanged {unchanged:.4f} mask {to_mask:.4f} other {other:.4f}")
    assert abs(unchanged - 0.100) <= 0.005, unchanged
    assert abs(to_mask - 0.800) <= 0.005, to_mask
    assert abs(other - 0.100) <= 0.005, other
    random_ids = new[(new != MASK) & (new != old)]
    print(f"random replacements {random_ids.min()}-{random_ids.max()}")
    assert random_ids.min() >= 0 and random_ids.max() <= VOCAB - 2


# ---------------------------------------------------------------------------
# runner
# ---------------------------------------------------------------------------
@pytest.fixture
def workspace(tmp_path):
    return make_workspace(tmp_path, with_vocab=False)


@pytest.mark.parametrize("extra", [(), ("--unpad",)], ids=["padded", "unpad"])
def test_runner_with_device_masking(workspace, extra):
    tmp_path, data_dir, cfg_path = workspace
    args = run_pretraining.parse_arguments(
        _argv(tmp_path, data_dir, cfg_path, "--device_masking", *extra)
    )
    assert args.device_masking is True
    assert run_pretraining.main(args) == 2
    losses = _losses(tmp_path)
    assert len(losses) == 2
    assert all(math.isfinite(v) and v > 0 for v in losses), losses


def test_flag_defaults_off_and_reads_from_json(workspace):
    tmp_path, data_dir, cfg_path = workspace
    argv = _argv(tmp_path, data_dir, cfg_path)
    assert run_pretraining.parse_arguments(argv).device_masking is False
    train_cfg = tmp_path / "train.json"
    train_cfg.write_text(json.dumps({"device_masking": True}))
    args = run_pretraining.parse_arguments(
        argv + ["--config_file", str(train_cfg)]
    )
    assert args.device_masking is True


def test_runner_masker_uses_the_run_seed(workspace):
    tmp_path, data_dir, cfg_path = workspace
    args = run_pretraining.parse_arguments(
        _argv(tmp_path, data_dir, cfg_path, "--device_masking")
    )
    args.local_rank = 3
    masker = run_pretraining.prepare_masker(args)
    assert masker.seed == 7  # --seed, not --seed + rank
    assert masker.vocab_size == 512 and masker.max_pred_per_seq == 5
