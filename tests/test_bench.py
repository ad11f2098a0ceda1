"""bench.py's command line: a plain run measures the headline step only (--full adds the rest), --dump-outputs writes the last
timed step's outputs as .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import bench

EXTRAS = ("no_device_time", "no_roofline", "no_pmc", "no_children", "no_cpu_baseline")


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_plain_run_drops_every_side_measurement(monkeypatch):
    args = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert args.steps == 7 and args.warmup == 2 and not args.full and args.dump_outputs is None
    assert all(getattr(args, k) for k in EXTRAS)


def test_full_keeps_the_side_measurements_and_their_switches(monkeypatch):
    args = _parse(monkeypatch, "--full")
    assert not any(getattr(args, k) for k in EXTRAS)
    args = _parse(monkeypatch, "--full", "--no_roofline", "--dump-outputs", "d")
    assert args.no_roofline and not args.no_device_time and args.dump_outputs == "d"


def test_dump_outputs_types_and_limit(tmp_path, monkeypatch):
    bench.dump_outputs(str(tmp_path / "a"), {"x": torch.arange(6, dtype=torch.float16).view(2, 3), "i": torch.tensor([3, 1]),
                                             "d": torch.ones(2, dtype=torch.float64), "s": 0})
    x = np.load(str(tmp_path / "a" / "x.npy"))
    assert x.dtype == np.float32 and x.shape == (2, 3) and x[1, 2] == 5
    assert np.load(str(tmp_path / "a" / "i.npy")).dtype == np.float64
    assert np.load(str(tmp_path / "a" / "d.npy")).dtype == np.float64
    assert np.load(str(tmp_path / "a" / "s.npy")).shape == ()
    # past the limit: a seeded sample of the array, the same in every call
    monkeypatch.setattr(bench, "DUMP_LIMIT", 400)
    big = torch.randn(1000)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"big": big})
    b, c = np.load(str(tmp_path / "b" / "big.npy")), np.load(str(tmp_path / "c" / "big.npy"))
    assert b.nbytes <= 400 and b.size == 100 and np.array_equal(b, c) and np.isin(b, big.numpy()).all()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_bench_run_dumps_the_last_step(hip_device, tmp_path):
    out_dir = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--bsz", "3", "--frames", "12",
           "--regions", "8", "--sub_words", "10", "--qa_words", "9", "--hsz", "64", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=500)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["higher_is_better"] is True
    assert not any(k in rec for k in ("roofline", "cpu_baseline", "device_ms_per_step", "exact_f32"))
    got = {f[:-4]: np.load(str(out_dir / f)) for f in os.listdir(str(out_dir))}
    assert set(got) == {"logits", "targets", "att_loss", "temporal_loss", "temporal_scores", "loss", "grad", "params"}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    assert got["logits"].shape[1] == 5 and got["logits"].shape[0] == got["targets"].shape[0]
    assert abs(float(got["loss"]) - rec["config"]["final_loss"]) < 1e-3 * (1 + abs(rec["config"]["final_loss"]))
    assert got["grad"].shape == got["params"].shape and np.abs(got["grad"]).max() > 0
