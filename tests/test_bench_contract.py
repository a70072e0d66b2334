"""bench.py's output contract (one JSON line per run; the driver parses it) and its N > 1 code path.

CPU: `--cpu-only` (BASELINE config 1: the CPU restatement timed on the host cores) prints the contract's keys.
GPU: a plain run carries only the headline figures and can dump the last step's outputs; a short single-GPU run with
`--full` carries `roofline` and `roofline_detail`; two ranks launched the way the driver launches
them (`python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 ... bench.py --gpus 2`)
run the data-parallel path end to end -- on this one-GPU box over gloo with both ranks on card 0
(SFCVIT_DIST_BACKEND / SFCVIT_FORCE_DEVICE, rehearsal knobs the driver's RCCL runs do not set)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
        "dtype", "data", "config"}


def _run(cmd, env=None, timeout=600):
    e = dict(os.environ, **(env or {}))
    r = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                      # exactly ONE JSON line, from rank 0
    return json.loads(lines[0])


def test_cpu_only_line():
    d = _run([sys.executable, "bench.py", "--cpu-only", "--cpu-steps", "1"])
    assert KEYS <= set(d) and d["n_gpus"] == 0 and d["unit"] == "images/s" and d["value"] > 0
    assert d["vs_baseline"] is None and d["higher_is_better"] is True
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and "sample" in cb and cb["value"] == pytest.approx(d["value"], rel=1e-3)
    assert "workload" in d["config"] and "model" not in d["config"]


@pytest.mark.gpu
def test_single_gpu_line_has_roofline():
    d = _run([sys.executable, "bench.py", "--full", "--workload", "vit_tiny16_32_hilbert", "--steps", "4", "--warmup", "2",
              "--no-cpu-baseline"])
    assert KEYS <= set(d) and d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["scaling"] == "weak"
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["dtype"] == "bf16" and d["data"].startswith("synthetic")
    r = d["roofline"]
    assert r["bound"] in ("mfma", "hbm") and r["unit"] in ("TFLOP/s", "GB/s") and 0 < r["frac"] < 1
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-2, abs=1e-4)      # both are rounded in the line
    assert "attention_fwd" in d["roofline_detail"] and "workload" in d["config"]


def test_dump_outputs_sample_is_fixed_float32_and_within_budget(tmp_path, monkeypatch):
    """--dump-outputs: the loss, every parameter and every gradient as float32 .npy; a tensor above the per-tensor cap
    contributes the same seeded positions on every run, and the files stay within the byte budget."""
    import numpy as np
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    model = torch.nn.Sequential(torch.nn.Linear(512, 1024), torch.nn.LayerNorm(1024))
    loss = model(torch.randn(4, 512)).square().mean()
    loss.backward()
    loss = loss.detach()
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), loss, model)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert names == sorted(["loss.npy"] + [f"{k}.{n}.npy" for n, _ in model.named_parameters() for k in ("param", "grad")])
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 1 << 20
    w = np.load(tmp_path / "a" / "param.0.weight.npy")
    assert w.dtype == np.float32 and 0 < w.size < 512 * 1024
    assert set(w.tolist()) <= set(model[0].weight.detach().reshape(-1).tolist())
    assert np.array_equal(np.load(tmp_path / "a" / "param.1.bias.npy"), model[1].bias.detach().numpy())
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [pytest.approx(float(loss))]
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))


@pytest.mark.gpu
def test_plain_line_is_lean_and_dumps_repeat(tmp_path):
    """A plain run times exactly --steps steps and carries none of --full's figures; --dump-outputs of two runs with the
    same arguments are identical (same seeded inputs, deterministic kernels)."""
    import numpy as np
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d_out in dirs:
        d = _run([sys.executable, "bench.py", "--workload", "vit_tiny16_32_hilbert", "--steps", "3", "--warmup", "1",
                  "--dump-outputs", str(d_out)])
        assert KEYS <= set(d) and d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["dtype"] == "bf16"
        assert not {"roofline", "roofline_detail", "cpu_baseline", "rccl", "kernel_timing"} & set(d)
    names = sorted(os.listdir(dirs[0]))
    assert "loss.npy" in names and any(n.startswith("grad.") for n in names) and names == sorted(os.listdir(dirs[1]))
    assert sum(os.path.getsize(dirs[0] / n) for n in names) <= 64 << 20
    for n in names:
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype == np.float32 and np.isfinite(a).all() and np.array_equal(a, b), n


@pytest.mark.gpu
def test_two_rank_launch_runs_the_data_parallel_path():
    import torch
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    env = {"HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    if backend == "gloo":
        env.update(SFCVIT_DIST_BACKEND="gloo", SFCVIT_FORCE_DEVICE="0")
    d = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
              "--master-port", "29533", "bench.py", "--gpus", "2", "--full", "--workload", "vit_tiny16_32_hilbert", "--steps", "3",
              "--warmup", "2", "--no-cpu-baseline"], env=env)
    assert KEYS <= set(d) and d["n_gpus"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    assert d["config"]["global_batch"] == 2 * 256 and d["config"]["parallelism"] == "dp2"
    rc = d["rccl"]
    assert rc["world_size"] == 2 and rc["backend"] == backend and rc["bytes_per_step"] > 0 and rc["buckets"] >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
def test_entry_script_trains_checkpoints_and_resumes(tmp_path, graph):
    """The repository's main.py (structure, defaults and printed line of the reference's main.py:255-354) as a
    subprocess on synthetic CIFAR-shaped batches: one epoch of the default model (hierarchical Morton tokenizer, 768
    wide, 8 layers, 4 heads = head dim 192), eagerly and with --graph; the checkpoint carries the reference's keys and
    --resume continues from it."""
    import re
    import torch
    pkg = os.path.join(ROOT, "space-filling-curves-for-vision-transformers_amd")
    base = [sys.executable, os.path.join(pkg, "main.py"), "--synthetic", "--train-size", "1024", "--test-size", "512",
            "--batch-size", "256", "--checkpoint-dir", str(tmp_path)] + (["--graph"] if graph else [])
    r = subprocess.run(base + ["--epochs", "1"], cwd=pkg, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("Epoch 1/1")]
    assert len(line) == 1 and re.search(r"Train Loss: \d+\.\d{4}, Train Acc: \d\.\d{4} \| Test Loss: \d+\.\d{4}, Test Acc: \d\.\d{4}", line[0])
    ck = torch.load(os.path.join(str(tmp_path), "checkpoint_hier_morton.pt"), map_location="cpu", weights_only=True)
    assert {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "train_loss", "train_acc", "test_loss",
            "test_acc"} <= set(ck)                                           # main.py:345-354
    assert ck["epoch"] == 0 and "patch_embed.fusion.weight" in ck["model_state_dict"]
    r2 = subprocess.run(base + ["--epochs", "2", "--resume", os.path.join(str(tmp_path), "checkpoint_hier_morton.pt")],
                        cwd=pkg, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stderr[-2000:]
    out = [ln for ln in r2.stdout.splitlines() if ln.startswith("Epoch")]
    assert len(out) == 1 and out[0].startswith("Epoch 2/2")                  # epoch 1 came from the checkpoint
