"""bench.py as a command: what a plain run prints and what --full adds to it."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA = ("roofline", "cpu_baseline", "accuracy", "f16", "f32", "train", "train_f16", "train_f32")


def _bench(*flags):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "CTDET_BENCH_BACKEND")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", *flags],
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = [ln for ln in out.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_alone(tmp_path):
    """`bench.py --gpus 1 --steps N --warmup W`: the result line with the headline's fields and none of the legs that --full
    adds; --dump-outputs still writes the detections of the last timed step"""
    rec = _bench("--dump-outputs", str(tmp_path / "out"))
    assert rec["metric"] == "images/sec at 512x512 (infer bs=64)" and rec["unit"] == "images/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "f16x3" and rec["n_gpus"] == 1
    assert (rec["steps"], rec["warmup"]) == (3, 1)
    assert rec["value"] > 0 and abs(rec["value"] * rec["ms_per_step"] - 64 * 1000.0) < 1e-6 * 64 * 1000.0
    assert not [k for k in EXTRA if k in rec]
    assert sorted(os.listdir(tmp_path / "out")) == ["boxes.npy", "classes.npy", "detections_per_image.npy", "scores.npy"]


def test_full_run_adds_its_legs_to_the_same_line():
    """--full measures the rest after the headline (here every leg but the roofline is dropped again with its --no-* option)"""
    rec = _bench("--full", "--no-cpu-baseline", "--no-f32", "--no-f16", "--no-train")
    assert rec["dtype"] == "f16x3" and rec["value"] > 0 and (rec["steps"], rec["warmup"]) == (3, 1)
    assert rec["roofline"]["kernel"] and rec["roofline"]["decode"]["trained_like"]["ms_per_step"] > 0
    assert not [k for k in EXTRA if k in rec and k != "roofline"]
