"""bench.py on one GPU: the persistent engine's run, and the fallback when a persistent run reports a hand-off
error (HOPSX_BENCH_FAKE_PERSIST_ERR sets the error word after the timed run): the bench then times the
multi-kernel engine and says so, instead of dying without a JSON line."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(env_extra, args=("--no-taxi",)):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "bench.py", "--steps", "20", "--warmup", "3", *args], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bench_persistent_and_fallback():
    ok = _bench({})
    assert ok["config"]["engine"] == "PersistentMnistStep" and ok["value"] > 0
    fb = _bench({"HOPSX_BENCH_FAKE_PERSIST_ERR": str((3 << 24) | 5)})
    assert fb["config"]["engine"] == "TrainStep", fb["config"]
    assert "timed on TrainStep instead" in (fb["config"]["persistent_note"] or "")
    assert fb["value"] > 0 and fb["final_loss"] == fb["final_loss"]


def test_bench_full_adds_the_taxi_trainer_and_plain_dumps_outputs(tmp_path):
    """--full is where the Chicago-taxi trainer runs; a plain run leaves it out and, with --dump-outputs,
    writes the persistent step's last loss / correct and the fp32 weights after the timed steps."""
    import numpy as np

    full = _bench({}, ("--full",))
    assert full["chicago_taxi"]["steps_per_sec"] > 0, full["chicago_taxi"]
    plain = _bench({}, ("--dump-outputs", str(tmp_path)))
    assert plain["chicago_taxi"] is None and plain["steps"] == 20 and plain["ms_per_step"] > 0
    assert plain["config"]["engine"] == "PersistentMnistStep"
    a = {p.stem: np.load(p) for p in sorted(tmp_path.glob("*.npy"))}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(v.size for k, v in a.items() if k.startswith("param.")) == 1_394_282
    assert abs(float(a["loss"].reshape(-1)[0]) - plain["final_loss"]) < 1e-3 and float(a["count"]) == 32
