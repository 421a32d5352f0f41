"""bench.py driver-contract test.

The round driver runs ``python bench.py --gpus N --steps K --warmup W``
and parses the single JSON line rank 0 prints (see bench.py docstring).
This test runs the real script on CPU with a tiny model config and
asserts the schema the driver depends on, plus cwd-independence of the
default config path.
"""

from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TINY = {
    "vocab_size": 512,
    "hidden_size": 64,
    "num_hidden_layers": 2,
    "num_attention_heads": 4,
    "intermediate_size": 128,
    "hidden_act": "gelu",
    "hidden_dropout_prob": 0.1,
    "attention_probs_dropout_prob": 0.1,
    "max_position_embeddings": 512,
    "type_vocab_size": 2,
    "initializer_range": 0.02,
}

REQUIRED_KEYS = {
    "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
}


@pytest.mark.timeout(300)
def test_bench_json_contract(tmp_path):
    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(TINY))
    # run from a DIFFERENT cwd to cover default-path resolution too
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"),
         "--gpus", "1", "--steps", "2", "--warmup", "1",
         "--local_batch", "2", "--accumulation", "2",
         "--model_config", str(cfg)],
        cwd=str(tmp_path), capture_output=True, text=True, timeout=280,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.strip().splitlines()[-1]
    rec = json.loads(line)
    assert REQUIRED_KEYS.issubset(rec.keys()), sorted(REQUIRED_KEYS - set(rec))
    assert rec["n_gpus"] == 1 and rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["metric"] == "sequences/sec"
    assert rec["higher_is_better"] is True
    assert rec["scaling"] == "weak"
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    # whole-job value consistency: value = local_batch * 1e3 / ms_per_step
    assert rec["value"] == pytest.approx(2 * 1e3 / rec["ms_per_step"], rel=0.05)
    assert rec["data"] == "synthetic"
    assert rec["config"]["seq_len"] == 128
    # global_batch = world * local_batch * accumulation
    assert rec["config"]["global_batch"] == 4


@pytest.mark.timeout(300)
def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes float32 .npy arrays of the last timed step,
    within 64 MB in all, identical from run to run for the same arguments;
    --full is accepted and keeps the result-line contract."""
    import numpy as np

    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(TINY))
    dumps = []
    for tag, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / f"dump_{tag}"
        out = subprocess.run(
            [sys.executable, os.path.join(REPO, "bench.py"),
             "--gpus", "1", "--steps", "3", "--warmup", "1",
             "--local_batch", "2", "--accumulation", "2",
             "--model_config", str(cfg), "--dump-outputs", str(d)] + extra,
            cwd=str(tmp_path), capture_output=True, text=True, timeout=280,
        )
        assert out.returncode == 0, out.stderr[-2000:]
        rec = json.loads(out.stdout.strip().splitlines()[-1])
        assert REQUIRED_KEYS.issubset(rec.keys())
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0
        files = sorted(p.name for p in d.iterdir())
        assert {"loss.npy", "mlm_loss.npy", "mlm_labels.npy",
                "nsp_scores.npy", "grads.npy", "params.npy"} == set(files)
        assert sum(p.stat().st_size for p in d.iterdir()) <= 64 * 2**20
        dumps.append({f[:-len(".npy")]: np.load(d / f) for f in files})
    a, b = dumps
    for name, arr in a.items():
        assert arr.dtype == np.float32, name
        assert np.isfinite(arr).all(), name
        # CPU eager path is deterministic: same arguments, same outputs
        np.testing.assert_array_equal(arr, b[name], err_msg=name)
    assert a["loss"].shape == (1,) and a["loss"][0] > 0
    assert a["nsp_scores"].shape == (2, 2)
    # step 3 of an accumulation-2 window leaves its gradients in place
    assert a["grads"].size == a["params"].size > 0
    assert np.abs(a["grads"]).max() > 0


def test_dump_outputs_sampling(tmp_path, monkeypatch):
    """dump_outputs with tensors larger than its budget: the seeded-sample
    branch keeps each group within the budget (plus one element per
    tensor), draws only values of the source tensors, and draws the same
    ones on every call."""
    import importlib.util

    import numpy as np
    import torch

    spec = importlib.util.spec_from_file_location(
        "bench_under_test", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(bench, "DUMP_GROUP_ELEMS", 100)

    torch.manual_seed(0)
    named = []
    for i, n in enumerate((1000, 300, 7)):
        p = torch.nn.Parameter(torch.randn(n))
        p.grad = torch.randn(n)
        named.append((f"p{i}", p))
    last = (torch.tensor(1.5), torch.tensor(9.0), torch.randn(4, 2),
            torch.arange(6))
    arrays = []
    for tag in ("a", "b"):
        d = tmp_path / tag
        bench.dump_outputs(str(d), last, named)
        arrays.append({f.name: np.load(f) for f in sorted(d.iterdir())})
    a, b = arrays
    for name in a:
        assert a[name].dtype == np.float32
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    # shares of the 100-element budget: 76 + 22 + max(1, 0) = 99
    assert a["params.npy"].size == a["grads.npy"].size == 99
    all_p = torch.cat([p.detach() for _, p in named]).numpy()
    all_g = torch.cat([p.grad for _, p in named]).numpy()
    assert np.isin(a["params.npy"], all_p).all()
    assert np.isin(a["grads.npy"], all_g).all()
    assert a["loss.npy"].tolist() == [1.5] and a["mlm_loss.npy"].tolist() == [9.0]
    assert a["nsp_scores.npy"].shape == (4, 2)
    assert a["mlm_labels.npy"].tolist() == [0, 1, 2, 3, 4, 5]

    # the BERT-Large benchmark's dump stays within 64 MB: two sampled
    # groups of at most DUMP_GROUP_ELEMS + one element per tensor, plus
    # the labels and NSP scores of the largest phase (local batch 96)
    monkeypatch.undo()
    n_tensors = 400
    total = 4 * (2 * (bench.DUMP_GROUP_ELEMS + n_tensors) + 96 * 80 + 96 * 2 + 2)
    assert total + 6 * 128 <= 64 * 2**20


@pytest.mark.timeout(300)
def test_bench_two_rank_gloo(tmp_path):
    """bench.py under the driver's exact torchrun launch pattern
    (--nnodes=1 --nproc-per-node N --master-addr 127.0.0.1) with
    world_size 2 on CPU/gloo: rank 0 prints one whole-job JSON line."""
    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(TINY))
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29518",
         os.path.join(REPO, "bench.py"),
         "--gpus", "2", "--steps", "2", "--warmup", "1",
         "--local_batch", "2", "--accumulation", "2",
         "--model_config", str(cfg)],
        cwd=str(tmp_path), capture_output=True, text=True, timeout=280,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line (rank 0 only)"
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2
    assert rec["config"]["parallelism"] == "dp2"
    # whole-job value: world * local_batch * 1e3 / ms_per_step
    assert rec["value"] == pytest.approx(2 * 2 * 1e3 / rec["ms_per_step"], rel=0.05)
