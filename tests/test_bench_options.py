"""bench.py's run modes: a plain run measures the headline only (everything else needs --full, or
SLK_BENCH_FULL=1, where each --no-* switch still works), --steps sets the number of timed steps whatever the
loss ring's default size, and --dump-outputs writes the timed trainer's parameters and per-step losses,
identical from run to run."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import PARAMS

import bench

EXTRAS = ["no_cpu_baseline", "no_kernel_pass", "no_conv_compare", "no_dropin", "no_hub_loopback", "no_k5",
          "no_exchange_phase"]
# what only a --full run puts into the result line at N = 1
FULL_ONLY = {"cpu_baseline", "speedup_vs_cpu_baseline", "kernels", "roofline", "conv_presets", "k4_server_loopback",
             "dropin_modules", "widened"}


def _parse(monkeypatch, *argv, env=None):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    monkeypatch.delenv("SLK_BENCH_FULL", raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return bench.parse()


def test_plain_run_switches_every_extra_off(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert not a.full and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    assert all(getattr(a, k) for k in EXTRAS)


def test_full_keeps_every_extra_and_its_switch(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not any(getattr(a, k) for k in EXTRAS)
    a = _parse(monkeypatch, "--full", "--no-k5", "--no-cpu-baseline")
    assert [k for k in EXTRAS if getattr(a, k)] == ["no_cpu_baseline", "no_k5"]


def test_environment_switch_equals_full(monkeypatch):
    a = _parse(monkeypatch, "--no-dropin", env={"SLK_BENCH_FULL": "1"})
    assert a.full and [k for k in EXTRAS if getattr(a, k)] == ["no_dropin"]
    assert not _parse(monkeypatch, env={"SLK_BENCH_FULL": "0"}).full


def test_dump_outputs_writes_float_arrays(tmp_path):
    import torch
    d = str(tmp_path / "sub" / "dump")   # created on demand
    bench.dump_outputs(d, {"w": torch.arange(6, dtype=torch.float32).view(2, 3), "loss": [0.5, 0.25],
                           "i": torch.ones(3, dtype=torch.int32)})
    assert sorted(os.listdir(d)) == ["i.npy", "loss.npy", "w.npy"]
    w, loss = np.load(os.path.join(d, "w.npy")), np.load(os.path.join(d, "loss.npy"))
    assert w.dtype == np.float32 and w.shape == (2, 3) and np.array_equal(w.ravel(), np.arange(6))
    assert loss.dtype == np.float64 and loss.tolist() == [0.5, 0.25]
    assert np.load(os.path.join(d, "i.npy")).dtype == np.float32


def _main(monkeypatch, capsys, *argv):
    """bench.main() in this process with a plain command line; returns its one JSON result line."""
    _parse(monkeypatch, "--gpus", "1", *argv)   # sets sys.argv and a clean environment
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    capsys.readouterr()
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_single_gpu_run_prints_the_headline_and_dumps_reproducible_outputs(gpu, monkeypatch, capsys, tmp_path):
    outs = [_main(monkeypatch, capsys, "--steps", "3", "--warmup", "2", "--batch", "68", "--dump-outputs",
                  str(tmp_path / t)) for t in "ab"]
    for out in outs:
        assert out["metric"] == "training samples/sec (node) for split CNN" and out["unit"] == "samples/s"
        assert out["higher_is_better"] is True and out["dtype"] == "fp32" and (out["steps"], out["warmup"]) == (3, 2)
        assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(68 / (out["ms_per_step"] * 1e-3))
        assert not FULL_ONLY & set(out)     # the headline only
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in PARAMS + ["loss"]}
    b = {k: np.load(tmp_path / "b" / f"{k}.npy") for k in PARAMS + ["loss"]}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{k}.npy" for k in a)
    assert a["loss"].dtype == np.float64 and a["loss"].shape == (5,)      # warm-up + timed steps
    assert np.isfinite(a["loss"]).all() and outs[0]["loss_first_last"] == [round(a["loss"][0], 5), round(a["loss"][-1], 5)]
    from splitcnn.data import init_models
    c, s = init_models(seed=0)
    init = dict(zip(PARAMS, [c.conv1.weight, c.conv1.bias, s.conv2.weight, s.conv2.bias, s.fc1.weight, s.fc1.bias]))
    for k in PARAMS:
        assert a[k].dtype == np.float32 and a[k].shape == tuple(init[k].shape)
        assert not np.array_equal(a[k], init[k].detach().numpy()), k      # the trained values, not the initial ones
        assert np.array_equal(a[k], b[k]), k                              # same arguments, same outputs
    assert np.array_equal(a["loss"], b["loss"])


@pytest.mark.gpu
def test_steps_beyond_the_default_loss_ring(gpu, monkeypatch, capsys, tmp_path):
    from splitcnn.engine import LossLog
    n = LossLog(gpu).capacity + 4
    out = _main(monkeypatch, capsys, "--steps", str(n), "--warmup", "1", "--batch", "4", "--dump-outputs", str(tmp_path))
    loss = np.load(tmp_path / "loss.npy")
    assert loss.shape == (n + 1,) and np.isfinite(loss).all() and out["ms_per_step"] > 0 and out["steps"] == n


@pytest.mark.gpu
def test_widened_config_run_dumps_reproducible_outputs(gpu, monkeypatch, capsys, tmp_path):
    from splitcnn.wide import CLIENT_NPARAM, SERVER_NPARAM
    outs = [_main(monkeypatch, capsys, "--config", "k5", "--k5-batch", "12", "--steps", "3", "--warmup", "1",
                  "--dump-outputs", str(tmp_path / t)) for t in "ab"]
    for out in outs:
        assert out["dtype"] == "bf16" and out["unit"] == "samples/s" and out["higher_is_better"] is True
        assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(12 / (out["ms_per_step"] * 1e-3))
        assert not FULL_ONLY & set(out)
    names = ["client_params", "server_params", "loss"]
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in names}
    b = {k: np.load(tmp_path / "b" / f"{k}.npy") for k in names}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{k}.npy" for k in names)
    assert a["client_params"].shape == (CLIENT_NPARAM,) and a["server_params"].shape == (SERVER_NPARAM,)
    assert a["client_params"].dtype == a["server_params"].dtype == np.float32
    assert a["loss"].dtype == np.float64 and a["loss"].shape == (4,) and np.isfinite(a["loss"]).all()
    for k in names:
        assert np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k
