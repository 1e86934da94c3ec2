"""bench.py's command line: a plain run does only what the headline needs, `--full` adds the legs that run steps of their
own, `--dump-outputs DIR` writes the last timed step's results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("other_fp32_math", "prepared", "cpu_baseline", "gpu_over_cpu")


def test_dump_outputs_samples_what_does_not_fit(tmp_path, monkeypatch):
    """dump_outputs on CPU tensors with a 4 000-byte budget: the small state arrays are stored whole, the outputs as a
    sample that fills their share and is the same elements on every call; float32 throughout, total within the budget."""
    import torch
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    g = torch.Generator().manual_seed(5)
    out = torch.rand(3, 50, 16, generator=g, dtype=torch.float64)        # 2 400 elements: does not fit
    h, c = torch.rand(1, 3, 16, generator=g), torch.rand(1, 3, 16, generator=g)
    bench.dump_outputs(str(tmp_path / "a"), (out, (h, c)), "ttlstm")
    bench.dump_outputs(str(tmp_path / "b"), (out * 2.0, (h, c)), "ttlstm")
    a = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in ("outputs", "h_n", "c_n")}
    b_out = np.load(str(tmp_path / "b" / "outputs.npy"))
    assert all(v.dtype == np.float32 for v in a.values())
    assert np.array_equal(a["h_n"], h.numpy()) and np.array_equal(a["c_n"], c.numpy())
    assert a["outputs"].shape == ((4000 - 2 * 48 * 4) // 4,)
    assert sum(v.nbytes for v in a.values()) <= 4000
    assert set(np.unique(a["outputs"])) <= set(np.unique(out.float().numpy()))
    assert np.array_equal(b_out, a["outputs"] * np.float32(2.0))           # the same elements of the second array
    bench.dump_outputs(str(tmp_path / "g"), (out[:, :4], h[0]), "ttgru")     # fits: stored whole, in its own shape
    assert np.array_equal(np.load(str(tmp_path / "g" / "outputs.npy")), out[:, :4].float().numpy())
    assert sorted(os.listdir(str(tmp_path / "g"))) == ["h_n.npy", "outputs.npy"]
    bench.dump_outputs(str(tmp_path / "t"), torch.tensor(0.25), "train")
    assert np.load(str(tmp_path / "t" / "loss.npy")) == np.float32(0.25)


def _bench(extra, out_dir):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "cfg1", "--steps", "4", "--warmup", "1",
           "--dump-outputs", str(out_dir)] + extra
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert lines[-1].startswith('{"metric"'), lines[-3:]
    return json.loads(lines[-1]), {n[:-4]: np.load(os.path.join(str(out_dir), n)) for n in sorted(os.listdir(str(out_dir)))}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench_dump")
    return _bench([], d / "plain"), _bench(["--full", "--no-cpu-baseline"], d / "full")


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(runs):
    (rec, _), (full, _) = runs
    assert rec["steps"] == 4 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert rec["unit"] == "timesteps/s" and rec["higher_is_better"] is True
    assert abs(rec["value"] - 784 / (rec["ms_per_step"] * 1e-3)) <= 1e-6 * rec["value"]
    assert rec["checked"]["finite"] is True and rec["roofline"]["frac"] > 0
    assert not [k for k in FULL_ONLY if k in rec] and rec["ms_per_step_blocks"] is None
    assert (full["metric"], full["unit"], full["dtype"]) == (rec["metric"], rec["unit"], rec["dtype"])
    assert full["prepared"]["ms_per_step"] > 0 and full["other_fp32_math"]["ms_per_step"] > 0
    assert full["ms_per_step_blocks"]["steps_per_block"] == 4 and "cpu_baseline" not in full


@pytest.mark.gpu
def test_dump_outputs_writes_the_last_steps_results(runs):
    """cfg1 (B = 32, T = 784, H = 128): outputs, h_n, c_n whole in float32; a second process with the same arguments (here with
    `--full` on top) starts from the same seeded weights and input, so it writes the same arrays — to 1e-5, smoke()'s fp32 bound."""
    (_, a), (_, b) = runs
    assert sorted(a) == ["c_n", "h_n", "outputs"] and sorted(b) == sorted(a)
    assert a["outputs"].shape == (32, 784, 128) and a["h_n"].shape == (32, 128) and a["c_n"].shape == (32, 128)
    for n in a:
        assert a[n].dtype == np.float32 and np.isfinite(a[n]).all()
        assert np.abs(a[n] - b[n]).max() <= 1e-5
    assert np.abs(a["outputs"][:, -1] - a["h_n"]).max() <= 1e-6 and a["outputs"].std() > 1e-3      # |h| < 1: a few fp32 ulp
    assert sum(v.nbytes for v in a.values()) <= 64 * 2 ** 20
